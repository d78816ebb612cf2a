// qd_line.h -- dense 1-D sweeps along a DIRECTION VECTOR over the 2N controls (qd_scan1d): the reference model layer's
// do1d_open(gate, min, max, points) over GateVoltageComposer.do1d (GateVoltageComposer.py:35-84, 213-222).  A line of n points
// occupies a slot of its OWN size: Rl x Rl records with Rl = ceil(sqrt(n)), record p = point p, the Rl*Rl - n tail records
// the inert all-zero record of qd_k_points_front.  The front kernel here fills the records in the hand-over form of the tile
// search, and the redo instantiation of the per-pixel search, the ground-state kernels, the telegraph chain, the sensor stage
// and the percentile kernel then run on the slot with the geometry (Rl, Rl*Rl) as DATA: none of them is changed.  What a line
// needs of its own is small: gather, front, the latching walk over ONE row of n points, a pack of the n leading values of a
// slot into a dense row for the percentile kernel, and the write.  qd_line_voltages and the slot arithmetic are
// __host__ __device__, so the CPU tier checks them (tests/hosttest_line).
#pragma once
#include "qd_points.h"

// the descriptor of one line in flight, in a buffer of its own (one per slot)
struct QdLineAxes {
    double lo, hi;                                               // range of the scalar s
    double d[2 * QD_MAXN];                                       // direction over the controls, the first 2N
    int32_t frame, pad;
};

// ---------------------------------------------------------------------------
// Slot arithmetic.  side = ceil(sqrt(n)) exactly (the double square root is only the first guess), so side*side >= n >
// (side-1)*(side-1): the tail is shorter than 2 side - 1 records, and with n <= P of the handle side <= R.
// ---------------------------------------------------------------------------
QD_HD int qd_line_side(int n) {
    int r = (int)sqrt((double)n);
    while ((long long)r * r < n) ++r;
    while (r > 1 && (long long)(r - 1) * (r - 1) >= n) --r;
    return r;
}
QD_HD int qd_line_tail(int n) { const int r = qd_line_side(n); return r * r - n; }
// ground-state batches (slabs) of one slot, ppb pixels each
QD_HD int qd_line_batches(int n, int ppb) { const int r = qd_line_side(n); return (r * r + ppb - 1) / ppb; }

// ---------------------------------------------------------------------------
// Front end of point t of a line of n: s = linspace(lo, hi, n)[t] and, with W0[2N] = [gate_v, sensor_v, barrier_v] of the state
// block,  W[i] = fma(s, d[i], W0[i]);  then the frame, vpp and tc exactly as the tail of qd_affine_voltages: same operations,
// same order, same fences.  With dx = d, dy = 0 and R = n, row 0 of an affine scan computes fma(sy, 0, fma(sx, d[i], W0[i])),
// which is the inner fma for finite sy (a sum with +0 changes no bits but those of -0): the bits of this function.
// ---------------------------------------------------------------------------
template <int N>
QD_HD void qd_line_voltages(const double* par, const double* st, const QdLineAxes* axes, int n, int t,
                            double* v_ext, double* vpp, double* tc) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
    const double* vgm = st + L.s_vgm;
    const double s = qd_linspace(axes->lo, axes->hi, n, t);
    double W[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const double w0 = i < N ? st[L.s_gate_v + i] : (i == N ? st[L.s_sensor_gt] : st[L.s_barrier_v + (i - G)]);
        W[i] = fma(s, axes->d[i], w0);
    }
    if (axes->frame == QD_SCAN_PHYSICAL) {
#pragma unroll
        for (int i = 0; i < V; ++i) v_ext[i] = W[i];
    } else {
#pragma unroll
        for (int i = 0; i < G; ++i) { v_ext[i] = qd_dotN<G>(vgm + i * G, W) + par[L.origin + i]; QD_ROW_FENCE(); }
#pragma unroll
        for (int b = 0; b < NB; ++b) v_ext[G + b] = W[G + b];
    }
#pragma unroll
    for (int i = 0; i < G; ++i) { vpp[i] = qd_dotN<V>(par + L.cgd + i * V, v_ext); QD_ROW_FENCE(); }
    const double tc_base = par[L.scal + 0];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double vb_eff = v_ext[G + b] + qd_dotN<G>(par + L.cbg + b * G, v_ext);
        tc[b] = tc_base * exp(-par[L.alpha + b] * vb_eff);
        QD_ROW_FENCE();
    }
}

// ---------------------------------------------------------------------------
// Record j of a slot: point j of the line (true: vpp and tc are in the record, vd, ncont and isa come back for the hand-over),
// or, from n on, the inert record (false: all zero -- nvalid = 0, K copies of |0..0> without a coupling; the redo pass skips
// it, the structure kernel finds every state isolated and emits no task).
// ---------------------------------------------------------------------------
template <int N>
QD_HD bool qd_line_record(const double* par, const double* st, const QdLineAxes* axes, int n, int j, QdPixelRec* rec,
                          double* v_ext, double* vd, double* ncont, double* isa) {
    constexpr int G = N + 1, NB = N - 1;
    if (j >= n) {
        static_assert(sizeof(QdPixelRec) % 8 == 0, "the inert record is written in 64-bit words");
        unsigned long long* w = reinterpret_cast<unsigned long long*>(rec);
#pragma unroll
        for (int i = 0; i < (int)(sizeof(QdPixelRec) / 8); ++i) w[i] = 0ull;
        return false;
    }
    double vpp[G], tc[NB];
    qd_line_voltages<N>(par, st, axes, n, j, v_ext, vpp, tc);
    qd_point_front<N>(par, v_ext, vpp, tc, vd, ncont, isa);
#pragma unroll
    for (int i = 0; i < G; ++i) rec->vpp[i] = vpp[i];
#pragma unroll
    for (int b = 0; b < NB; ++b) rec->tc[b] = tc[b];
    return true;
}

#if defined(__HIPCC__)
#include "qd_kernels.h"
#include "qd_latch.h"

#define QD_LINE_BLOCK 128
// slots in flight per launch at the most (qdsim.h: QD_LINE_SLOTS); the grids of the search and sensor kernels carry the slot
// in their z dimension (< 65536)
#define QD_LINE_MAX_SLOTS 4096

struct QdLineQuery {
    const int* env_of_query;                                   // [nq]
    const double* dir;                                         // [nq][2N]
    const double *range, *gate_v, *barrier_v, *sensor_v;       // [nq][2], [nq][N], [nq][N-1], [nq] or null
    const double *vgm, *gamma;                                 // [nq][G][G] or null, [nq] or null
    int frame;
};

// a query renders when its env id is in [0, B): any direction is legal, the zero vector too (a repeated point)
__device__ __forceinline__ bool qd_line_live(const QdLineQuery& Q, int q, int B) {
    const int e = Q.env_of_query[q];
    return e >= 0 && e < B;
}

// ---------------------------------------------------------------------------
// gather: slot k (query base + k) <- parameter and state block of env env_of_query[base + k], with the base point, the
// virtual gate matrix and the peak width of the query applied as qd_k_affine_gather applies them (constant width: scal[1] =
// the query's gamma or the env's constant, scal[3] = -1); axes[k] <- range, direction and frame.  The Kalman block is copied
// as it is: no kernel behind a line reads it.  A query that is not live renders a clamped env (the write kernel skips it).
// grid = cnt, block = QD_LINE_BLOCK.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(QD_LINE_BLOCK)
qd_k_line_gather(QdLineQuery Q, int base, int B, int N, const double* __restrict__ params, const double* __restrict__ state,
                 double* __restrict__ sparams, double* __restrict__ sstate, QdLineAxes* __restrict__ axes) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.x, q = base + k, nb = N - 1, G = N + 1, V = 2 * N;
    int e = Q.env_of_query[q];
    e = e < 0 ? 0 : (e >= B ? B - 1 : e);
    const double* par = params + (size_t)e * L.size;
    const double* st = state + (size_t)e * L.s_size;
    double* dp = sparams + (size_t)k * L.size;
    double* ds = sstate + (size_t)k * L.s_size;
    QdLineAxes* A = axes + k;
    for (int i = threadIdx.x; i < L.s_size; i += QD_LINE_BLOCK) {
        double v = st[i];
        if (i >= L.s_vgm && i < L.s_vgm + G * G) { if (Q.vgm) v = Q.vgm[(size_t)q * G * G + (i - L.s_vgm)]; }
        else if (i >= L.s_gate_v && i < L.s_gate_v + N) v = Q.gate_v[(size_t)q * N + (i - L.s_gate_v)];
        else if (i >= L.s_barrier_v && i < L.s_barrier_v + nb) v = Q.barrier_v[(size_t)q * nb + (i - L.s_barrier_v)];
        else if (i == L.s_sensor_gt) v = Q.sensor_v ? Q.sensor_v[q] : 0.0;      // sensor_voltage=None -> 0.0
        ds[i] = v;
    }
    for (int i = threadIdx.x; i < L.size; i += QD_LINE_BLOCK) if (i != L.scal + 1 && i != L.scal + 3) dp[i] = par[i];
    for (int i = threadIdx.x; i < 2 * QD_MAXN; i += QD_LINE_BLOCK) A->d[i] = i < V ? Q.dir[(size_t)q * V + i] : 0.0;
    if (threadIdx.x == 0) {
        dp[L.scal + 1] = Q.gamma ? Q.gamma[q] : par[L.scal + 1];
        dp[L.scal + 3] = -1.0;
        A->lo = Q.range[2 * (size_t)q]; A->hi = Q.range[2 * (size_t)q + 1];
        A->frame = Q.frame; A->pad = 0;
    }
}

// ---------------------------------------------------------------------------
// front end, one record per lane: record j of slot k (SP = Rl*Rl records) <- point j of the slot's line in hand-over form,
// nvalid = QD_T_REDO: the redo pass searches it; from n on the inert record.  grid = (ceil(SP / block), slots).
// ---------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(QD_LINE_BLOCK)
qd_k_line_front(int n, int SP, const double* __restrict__ sparams, const double* __restrict__ sstate,
                const QdLineAxes* __restrict__ axes, QdPixelRec* __restrict__ recs) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.y;
    const int j = blockIdx.x * QD_LINE_BLOCK + threadIdx.x;
    if (j >= SP) return;
    QdPixelRec* rec = recs + (size_t)k * SP + j;
    double v_ext[2 * N], vd[N], ncont[N], isa;
    if (qd_line_record<N>(sparams + (size_t)k * L.size, sstate + (size_t)k * L.s_size, axes + k, n, j, rec, v_ext, vd, ncont, &isa))
        qd_tile_hand_over<N>(rec, vd, ncont, isa);
}

// ---------------------------------------------------------------------------
// latching, one lane per line: qd_latch_row as it is on ONE row of n points (row 0, R = n, channel 0), so the held state
// starts at point 0 and is never reset and the Philox counter is the point index.  occ [slots][SP][N], zraw [slots][SP].
// grid = ceil(slots / 64), block = 64.
// ---------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(64)
qd_k_latch_lines(int n_slots, int n, int SP, const double* __restrict__ sparams, double* __restrict__ occ, double* __restrict__ zraw,
                 QdNoiseCfg nz) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n_slots) return;
    qd_latch_row<N>(sparams + (size_t)k * L.size, L, occ + (size_t)k * SP * N, zraw + (size_t)k * SP, 0, n, 0, nz.seed, nz.ser_lo,
                    nz.ser_hi, nz.env_off + (uint32_t)k);
}

// pack: the n leading values of each slot's SP into a dense [slots][n] buffer (the percentile kernel reads rows whose
// stride equals their count).  grid = (ceil(n / 256), slots).
__global__ void qd_k_line_pack(int n, int SP, const double* __restrict__ sz, double* __restrict__ dense) {
    const int k = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) dense[(size_t)k * n + p] = sz[(size_t)k * SP + p];
}

// ---------------------------------------------------------------------------
// write: slot k -> the caller's slot base + k.  raw [nq][n] float64, image [nq][n] float32 normalised with the line's own
// percentiles (qd_norm), plohi [nq][2], occupations [nq][n][N] float64; each may be null.  Queries that are not live leave
// their slots untouched.  grid = (ceil(n / 256), cnt).
// ---------------------------------------------------------------------------
__global__ void qd_k_line_write(QdLineQuery Q, int base, int B, int N, int n, int SP, const double* __restrict__ dense,
                                const double* __restrict__ splohi, const double* __restrict__ socc, double* __restrict__ raw_dst,
                                float* __restrict__ image_dst, double* __restrict__ plohi_dst, double* __restrict__ occ_dst) {
    const int k = blockIdx.y, q = base + k;
    if (!qd_line_live(Q, q, B)) return;
    const double lo = splohi[2 * k], hi = splohi[2 * k + 1];
    if (plohi_dst && blockIdx.x == 0 && threadIdx.x < 2) plohi_dst[2 * (size_t)q + threadIdx.x] = threadIdx.x ? hi : lo;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double z = dense[(size_t)k * n + p];
    if (raw_dst) raw_dst[(size_t)q * n + p] = z;
    if (image_dst) image_dst[(size_t)q * n + p] = qd_norm(z, lo, hi);
    if (occ_dst)
        for (int i = 0; i < N; ++i) occ_dst[((size_t)q * n + p) * N + i] = socc[((size_t)k * SP + p) * N + i];
}

#endif  // __HIPCC__
