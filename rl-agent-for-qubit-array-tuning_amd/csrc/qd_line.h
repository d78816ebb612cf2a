// qd_line.h -- dense 1-D sweeps along a DIRECTION VECTOR over the 2N controls (qd_scan1d): the reference model layer's
// do1d_open(gate, min, max, points) over GateVoltageComposer.do1d (GateVoltageComposer.py:35-84, 213-222).  A line of n points
// occupies a slot of its OWN size: Rl x Rl records with Rl = ceil(sqrt(n)), record p = point p, the Rl*Rl - n tail records
// the inert all-zero record (qd_inert_record, qd_query.h).  The front kernel here fills the records in the hand-over form of the tile
// search, and the redo instantiation of the per-pixel search, the ground-state kernels, the telegraph chain, the sensor stage
// and the percentile kernel then run on the slot with the geometry (Rl, Rl*Rl) as DATA: none of them is changed.  What a line
// needs of its own is small: gather (around qd_slot_copy, qd_query.h), front, the latching walk over ONE row of n points and
// a pack of the n leading values of a slot into a dense row for the percentile kernel and for qd_k_query_write (qd_query.h).
// qd_line_voltages and the slot arithmetic are __host__ __device__, so the CPU tier checks them (tests/hosttest_line).
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
// block,  W[i] = fma(s, d[i], W0[i]);  then the frame, vpp and tc by qd_control_voltages (qd_query.h), the tail of
// qd_affine_voltages.  With dx = d, dy = 0 and R = n, row 0 of an affine scan computes fma(sy, 0, fma(sx, d[i], W0[i])),
// which is the inner fma for finite sy (a sum with +0 changes no bits but those of -0): the bits of this function.
// ---------------------------------------------------------------------------
template <int N>
QD_HD void qd_line_voltages(const double* par, const double* st, const QdLineAxes* axes, int n, int t,
                            double* v_ext, double* vpp, double* tc) {
    constexpr int G = N + 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
    const double s = qd_linspace(axes->lo, axes->hi, n, t);
    double W[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const double w0 = i < N ? st[L.s_gate_v + i] : (i == N ? st[L.s_sensor_gt] : st[L.s_barrier_v + (i - G)]);
        W[i] = fma(s, axes->d[i], w0);
    }
    qd_control_voltages<N>(par, st, axes->frame, W, v_ext, vpp, tc);
}

// ---------------------------------------------------------------------------
// Record of a slot that a front kernel fills before the search.  live: the point whose control voltages `voltages(v_ext, vpp,
// tc)` computes (true: vpp and tc are in the record, vd, ncont and isa come back for the hand-over); else the inert record
// (false; qd_inert_record).
// ---------------------------------------------------------------------------
template <int N, class Voltages>
QD_HD bool qd_slot_record(const double* par, bool live, QdPixelRec* rec, double* v_ext, double* vd, double* ncont, double* isa,
                          Voltages voltages) {
    constexpr int G = N + 1, NB = N - 1;
    if (!live) { qd_inert_record(rec); return false; }
    double vpp[G], tc[NB];
    voltages(v_ext, vpp, tc);
    qd_point_front<N>(par, v_ext, vpp, tc, vd, ncont, isa);
#pragma unroll
    for (int i = 0; i < G; ++i) rec->vpp[i] = vpp[i];
#pragma unroll
    for (int b = 0; b < NB; ++b) rec->tc[b] = tc[b];
    return true;
}

// record j of a line's slot: point j of the line, or, from n on, the inert record
template <int N>
QD_HD bool qd_line_record(const double* par, const double* st, const QdLineAxes* axes, int n, int j, QdPixelRec* rec,
                          double* v_ext, double* vd, double* ncont, double* isa) {
    return qd_slot_record<N>(par, j < n, rec, v_ext, vd, ncont, isa,
                             [&](double* ve, double* vpp, double* tc) { qd_line_voltages<N>(par, st, axes, n, j, ve, vpp, tc); });
}

#if defined(__HIPCC__)
#include "qd_kernels.h"
#include "qd_latch.h"

#define QD_LINE_BLOCK 128
// slots in flight per launch at the most (qdsim.h: QD_LINE_SLOTS); the grids of the search and sensor kernels carry the slot
// in their z dimension (< 65536)
#define QD_LINE_MAX_SLOTS 4096

// ---------------------------------------------------------------------------
// gather: slot k (query base + k) <- parameter and state block of env env_of_query[base + k] with the query applied
// (qd_slot_copy, qd_query.h: the base point, the virtual gate matrix, the constant peak width); axes[k] <- range, direction
// and frame.  The Kalman block is copied as it is: no kernel behind a line reads it.  A query that is not live renders a
// clamped env (the write kernel skips it).  grid = cnt, block = QD_LINE_BLOCK.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(QD_LINE_BLOCK)
qd_k_line_gather(QdAffineQuery Q, int base, int B, int N, const double* __restrict__ params, const double* __restrict__ state,
                 double* __restrict__ sparams, double* __restrict__ sstate, QdLineAxes* __restrict__ axes) {
    const int k = blockIdx.x, q = base + k, V = 2 * N;
    qd_slot_copy<QD_LINE_BLOCK>(Q, q, k, B, qd_layout(N), params, state, sparams, sstate, 0);
    QdLineAxes* A = axes + k;
    for (int i = threadIdx.x; i < 2 * QD_MAXN; i += QD_LINE_BLOCK) A->d[i] = i < V ? Q.dir[(size_t)q * V + i] : 0.0;
    if (threadIdx.x == 0) {
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
// stride equals their count; qd_k_query_write then reads the same rows).  grid = (ceil(n / 256), slots).
__global__ void qd_k_line_pack(int n, int SP, const double* __restrict__ sz, double* __restrict__ dense) {
    const int k = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) dense[(size_t)k * n + p] = sz[(size_t)k * SP + p];
}

#endif  // __HIPCC__
