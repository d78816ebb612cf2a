// qd_scan.h -- the gather kernel of the stateless 2-D scans over any two controls (qd_scan2d).  A scan query occupies one slot
// of a second set of parameter, state and signal buffers with ONE channel image; the search kernels run with the scan front
// end (qd_scan_voltages, qd_pixel.h: qd_k_scan_tile, qd_k_scan_candidates), everything behind them reads a pixel from its
// QdPixelRec and runs as in a step.  The gather kernel here fills the slot from the env's blocks and the query arrays
// (qd_slot_copy, qd_query.h); qd_k_query_write (there) hands the result to the caller.
#pragma once
#include "qd_query.h"

#define QD_SCAN_BLOCK 128
struct QdScanQuery {
    const int* env_of_query;                                   // [nq]
    const int* axes;                                           // [nq][2]
    const double *range, *gate_v, *barrier_v, *sensor_v;       // [nq][4], [nq][N], [nq][N-1], [nq] or null
    const double *vgm, *gamma;                                 // [nq][G][G] or null, [nq] or null
    int frame;
};

// ---------------------------------------------------------------------------
// gather: slot k (query base + k) <- parameter and state block of env env_of_query[base + k] with the query applied
// (qd_slot_copy), and its axes descriptor in the place of the Kalman means (QdFrontScan, qd_pixel.h).  The constant peak
// width of the slot: the query's gamma if given; else, with two virtual plungers as axes, the rule of qd_peak_width on their
// base voltages; else the env's constant.  A query that is not live (qd_query_live: env id in [0, B), two different axes in
// [0, 2N)) renders a clamped env over controls (0, 1) (the write kernel skips it).  grid = cnt, block = QD_SCAN_BLOCK.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(QD_SCAN_BLOCK)
qd_k_scan_gather(QdScanQuery Q, int base, int B, int N, const double* __restrict__ params, const double* __restrict__ state,
                 double* __restrict__ sparams, double* __restrict__ sstate) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.x, q = base + k;
    const bool live = qd_query_live(Q.env_of_query, Q.axes, q, B, N);
    const int ax = live ? Q.axes[2 * (size_t)q] : 0, ay = live ? Q.axes[2 * (size_t)q + 1] : 1;
    const QdSlot S = qd_slot_copy<QD_SCAN_BLOCK>(Q, q, k, B, L, params, state, sparams, sstate, 6);   // (6 words: the axes descriptor)
    __syncthreads();                                           // (thread 0 reads the slot's gate voltages back)
    if (threadIdx.x == 0) {
        if (!Q.gamma && Q.frame == QD_SCAN_VIRTUAL && ax < N && ay < N) S.dp[L.scal + 1] = qd_peak_width_pair(S.par, S.ds, L, ax, ay);
        QdScanAxes A;
        A.x_lo = Q.range[4 * (size_t)q]; A.x_hi = Q.range[4 * (size_t)q + 1];
        A.y_lo = Q.range[4 * (size_t)q + 2]; A.y_hi = Q.range[4 * (size_t)q + 3];
        A.ax = ax; A.ay = ay; A.frame = Q.frame; A.pad = 0;
        *reinterpret_cast<QdScanAxes*>(S.ds + L.s_kmean) = A;
    }
}
