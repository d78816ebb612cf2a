// qd_scan.h -- kernels of the stateless 2-D scans over any two controls (qd_scan2d).  A scan query occupies one slot of a
// second set of parameter, state and signal buffers with ONE channel image; the search kernels run with the scan front
// end (qd_scan_voltages, qd_pixel.h: qd_k_scan_tile, qd_k_scan_candidates), everything behind them reads a pixel from its
// QdPixelRec and runs as in a step.  The gather kernel here fills the slot from the env's blocks and the query arrays, the
// write kernel hands the result to the caller.
#pragma once
#include "qd_kernels.h"

#define QD_SCAN_BLOCK 128
struct QdScanQuery {
    const int* env_of_query;                                   // [nq]
    const int* axes;                                           // [nq][2]
    const double *range, *gate_v, *barrier_v, *sensor_v;       // [nq][4], [nq][N], [nq][N-1], [nq] or null
    const double *vgm, *gamma;                                 // [nq][G][G] or null, [nq] or null
    int frame;
};

// a query renders when its env id is in [0, B) and its axes are two different controls in [0, 2N)
__device__ __forceinline__ bool qd_scan_live(const QdScanQuery& Q, int q, int B, int N) {
    const int e = Q.env_of_query[q], ax = Q.axes[2 * (size_t)q], ay = Q.axes[2 * (size_t)q + 1];
    return e >= 0 && e < B && ax >= 0 && ax < 2 * N && ay >= 0 && ay < 2 * N && ax != ay;
}

// ---------------------------------------------------------------------------
// gather: slot k (query base + k) <- parameter and state block of env env_of_query[base + k], with the gate, barrier and
// sensor voltages of the query, its virtual gate matrix if given, and its axes descriptor in the place of the Kalman means
// (QdFrontScan, qd_pixel.h).  The peak width the sensor
// stage will use becomes a CONSTANT of the slot's parameter copy (scal[1], with scal[3] = -1: "constant width"): the
// query's gamma if given; else, with two virtual plungers as axes, the rule of qd_peak_width on their base voltages; else
// the env's constant.  A query that is not live renders a clamped env over controls (0, 1) (the write kernel skips it).
// grid = cnt, block = QD_SCAN_BLOCK.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(QD_SCAN_BLOCK)
qd_k_scan_gather(QdScanQuery Q, int base, int B, int N, const double* __restrict__ params, const double* __restrict__ state,
                 double* __restrict__ sparams, double* __restrict__ sstate) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.x, q = base + k, nb = N - 1, G = N + 1;
    const bool live = qd_scan_live(Q, q, B, N);
    int e = Q.env_of_query[q];
    e = e < 0 ? 0 : (e >= B ? B - 1 : e);
    const int ax = live ? Q.axes[2 * (size_t)q] : 0, ay = live ? Q.axes[2 * (size_t)q + 1] : 1;
    const double* par = params + (size_t)e * L.size;
    const double* st = state + (size_t)e * L.s_size;
    double* dp = sparams + (size_t)k * L.size;
    double* ds = sstate + (size_t)k * L.s_size;
    for (int i = threadIdx.x; i < L.s_size; i += QD_SCAN_BLOCK) {
        double v = st[i];
        if (i >= L.s_vgm && i < L.s_vgm + G * G) { if (Q.vgm) v = Q.vgm[(size_t)q * G * G + (i - L.s_vgm)]; }
        else if (i >= L.s_gate_v && i < L.s_gate_v + N) v = Q.gate_v[(size_t)q * N + (i - L.s_gate_v)];
        else if (i >= L.s_barrier_v && i < L.s_barrier_v + nb) v = Q.barrier_v[(size_t)q * nb + (i - L.s_barrier_v)];
        else if (i == L.s_sensor_gt) v = Q.sensor_v ? Q.sensor_v[q] : 0.0;      // sensor_voltage=None -> 0.0
        else if (i >= L.s_kmean && i < L.s_kmean + 6) continue;                // the axes descriptor's place (thread 0 below)
        ds[i] = v;
    }
    for (int i = threadIdx.x; i < L.size; i += QD_SCAN_BLOCK) if (i != L.scal + 1 && i != L.scal + 3) dp[i] = par[i];
    __syncthreads();                                           // (thread 0 reads the slot's gate voltages back)
    if (threadIdx.x == 0) {
        double gamma = par[L.scal + 1];
        if (Q.gamma) gamma = Q.gamma[q];
        else if (Q.frame == QD_SCAN_VIRTUAL && ax < N && ay < N) gamma = qd_peak_width_pair(par, ds, L, ax, ay);
        dp[L.scal + 1] = gamma;
        dp[L.scal + 3] = -1.0;
        QdScanAxes A;
        A.x_lo = Q.range[4 * (size_t)q]; A.x_hi = Q.range[4 * (size_t)q + 1];
        A.y_lo = Q.range[4 * (size_t)q + 2]; A.y_hi = Q.range[4 * (size_t)q + 3];
        A.ax = ax; A.ay = ay; A.frame = Q.frame; A.pad = 0;
        *reinterpret_cast<QdScanAxes*>(ds + L.s_kmean) = A;
    }
}

// ---------------------------------------------------------------------------
// write: slot k -> the caller's slot base + k.  raw [nq][P] float64, image [nq][R][R] float32 normalised with the slot's
// own percentiles (qd_norm, as qd_k_write_obs), plohi [nq][2], occupations [nq][P][N] float64; each may be null.  Queries
// that are not live leave their slots untouched.  grid = (ceil(P/256), cnt).
// ---------------------------------------------------------------------------
__global__ void qd_k_scan_write(QdScanQuery Q, int base, int B, int N, int P, const double* __restrict__ sz,
                                const double* __restrict__ splohi, const double* __restrict__ socc, double* __restrict__ raw_dst,
                                float* __restrict__ image_dst, double* __restrict__ plohi_dst, double* __restrict__ occ_dst) {
    const int k = blockIdx.y, q = base + k;
    if (!qd_scan_live(Q, q, B, N)) return;
    const double lo = splohi[2 * k], hi = splohi[2 * k + 1];
    if (plohi_dst && blockIdx.x == 0 && threadIdx.x < 2) plohi_dst[2 * (size_t)q + threadIdx.x] = threadIdx.x ? hi : lo;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const double z = sz[(size_t)k * P + p];
    if (raw_dst) raw_dst[(size_t)q * P + p] = z;
    if (image_dst) image_dst[(size_t)q * P + p] = qd_norm(z, lo, hi);
    if (occ_dst)
        for (int i = 0; i < N; ++i) occ_dst[((size_t)q * P + p) * N + i] = socc[((size_t)k * P + p) * N + i];
}
