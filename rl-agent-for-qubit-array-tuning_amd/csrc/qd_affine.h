// qd_affine.h -- kernels of the stateless 2-D scans along two DIRECTION VECTORS over the 2N controls (qd_scan_affine).  A
// query occupies one slot of the scan buffers (those of qd_scan2d) with ONE channel image and one QdAffineAxes descriptor in
// a buffer of its own; the search kernels run with the affine front end (qd_affine_voltages, qd_pixel.h), everything behind
// them reads a pixel from its QdPixelRec and runs as in a step.  The gather kernel here fills the slot and its descriptor
// from the env's blocks and the query arrays, the write kernel hands the result to the caller.
#pragma once
#include "qd_kernels.h"

#define QD_AFFINE_BLOCK 128
struct QdAffineQuery {
    const int* env_of_query;                                   // [nq]
    const double* dir;                                         // [nq][2][2N]: dx, dy
    const double *range, *gate_v, *barrier_v, *sensor_v;       // [nq][4], [nq][N], [nq][N-1], [nq] or null
    const double *vgm, *gamma;                                 // [nq][G][G] or null, [nq] or null
    int frame;
};

// a query renders when its env id is in [0, B): any two directions are legal, the zero vector too (a repeated 1-D sweep)
__device__ __forceinline__ bool qd_affine_live(const QdAffineQuery& Q, int q, int B) {
    const int e = Q.env_of_query[q];
    return e >= 0 && e < B;
}

// ---------------------------------------------------------------------------
// gather: slot k (query base + k) <- parameter and state block of env env_of_query[base + k], with the gate, barrier and
// sensor voltages of the query (the base point W0 of the scan), its virtual gate matrix if given, and the ADDRESS of the
// slot's descriptor axes[k] in the place of the Kalman means (QdFrontAffine, qd_pixel.h); axes[k] <- the query's ranges,
// directions and frame.  The peak width the sensor stage will use becomes a CONSTANT of the slot's parameter copy (scal[1],
// with scal[3] = -1: "constant width"): the query's gamma if given, else the env's constant.  The vary_peak_width rule of a
// step is NOT applied: it is a function of the swept plunger pair, and an affine axis has no pair.  A query that is not
// live renders a clamped env (the write kernel skips it).  Non-finite coefficients are not looked for.
// grid = cnt, block = QD_AFFINE_BLOCK.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(QD_AFFINE_BLOCK)
qd_k_affine_gather(QdAffineQuery Q, int base, int B, int N, const double* __restrict__ params, const double* __restrict__ state,
                   double* __restrict__ sparams, double* __restrict__ sstate, QdAffineAxes* __restrict__ axes) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.x, q = base + k, nb = N - 1, G = N + 1, V = 2 * N;
    int e = Q.env_of_query[q];
    e = e < 0 ? 0 : (e >= B ? B - 1 : e);
    const double* par = params + (size_t)e * L.size;
    const double* st = state + (size_t)e * L.s_size;
    double* dp = sparams + (size_t)k * L.size;
    double* ds = sstate + (size_t)k * L.s_size;
    QdAffineAxes* A = axes + k;
    for (int i = threadIdx.x; i < L.s_size; i += QD_AFFINE_BLOCK) {
        double v = st[i];
        if (i >= L.s_vgm && i < L.s_vgm + G * G) { if (Q.vgm) v = Q.vgm[(size_t)q * G * G + (i - L.s_vgm)]; }
        else if (i >= L.s_gate_v && i < L.s_gate_v + N) v = Q.gate_v[(size_t)q * N + (i - L.s_gate_v)];
        else if (i >= L.s_barrier_v && i < L.s_barrier_v + nb) v = Q.barrier_v[(size_t)q * nb + (i - L.s_barrier_v)];
        else if (i == L.s_sensor_gt) v = Q.sensor_v ? Q.sensor_v[q] : 0.0;      // sensor_voltage=None -> 0.0
        else if (i == L.s_kmean) continue;                                      // the descriptor's address (thread 0 below)
        ds[i] = v;
    }
    for (int i = threadIdx.x; i < L.size; i += QD_AFFINE_BLOCK) if (i != L.scal + 1 && i != L.scal + 3) dp[i] = par[i];
    for (int i = threadIdx.x; i < 2 * QD_MAXN; i += QD_AFFINE_BLOCK) {
        A->dx[i] = i < V ? Q.dir[((size_t)q * 2 + 0) * V + i] : 0.0;
        A->dy[i] = i < V ? Q.dir[((size_t)q * 2 + 1) * V + i] : 0.0;
    }
    if (threadIdx.x == 0) {
        dp[L.scal + 1] = Q.gamma ? Q.gamma[q] : par[L.scal + 1];
        dp[L.scal + 3] = -1.0;
        A->x_lo = Q.range[4 * (size_t)q]; A->x_hi = Q.range[4 * (size_t)q + 1];
        A->y_lo = Q.range[4 * (size_t)q + 2]; A->y_hi = Q.range[4 * (size_t)q + 3];
        A->frame = Q.frame; A->pad = 0;
        *reinterpret_cast<const QdAffineAxes**>(ds + L.s_kmean) = A;
    }
}

// ---------------------------------------------------------------------------
// write: slot k -> the caller's slot base + k.  raw [nq][P] float64, image [nq][R][R] float32 normalised with the slot's
// own percentiles (qd_norm, as qd_k_write_obs), plohi [nq][2], occupations [nq][P][N] float64; each may be null.  Queries
// that are not live leave their slots untouched.  grid = (ceil(P/256), cnt).
// ---------------------------------------------------------------------------
__global__ void qd_k_affine_write(QdAffineQuery Q, int base, int B, int N, int P, const double* __restrict__ sz,
                                  const double* __restrict__ splohi, const double* __restrict__ socc, double* __restrict__ raw_dst,
                                  float* __restrict__ image_dst, double* __restrict__ plohi_dst, double* __restrict__ occ_dst) {
    const int k = blockIdx.y, q = base + k;
    if (!qd_affine_live(Q, q, B)) return;
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
