// qd_affine.h -- the gather kernel of the stateless 2-D scans along two DIRECTION VECTORS over the 2N controls
// (qd_scan_affine).  A query occupies one slot of the scan buffers (those of qd_scan2d) with ONE channel image and one
// QdAffineAxes descriptor in a buffer of its own; the search kernels run with the affine front end (qd_affine_voltages,
// qd_pixel.h), everything behind them reads a pixel from its QdPixelRec and runs as in a step.  The gather kernel here fills
// the slot (qd_slot_copy, qd_query.h) and its descriptor from the env's blocks and the query arrays (QdAffineQuery, there);
// qd_k_query_write (there) hands the result to the caller.
#pragma once
#include "qd_query.h"

#define QD_AFFINE_BLOCK 128

// ---------------------------------------------------------------------------
// gather: slot k (query base + k) <- parameter and state block of env env_of_query[base + k] with the query applied
// (qd_slot_copy: the base point W0 of the scan, the virtual gate matrix, the constant peak width), and the ADDRESS of the
// slot's descriptor axes[k] in the place of the Kalman means (QdFrontAffine, qd_pixel.h); axes[k] <- the query's ranges,
// directions and frame.  The vary_peak_width rule of a step is NOT applied: it is a function of the swept plunger pair, and
// an affine axis has no pair.  A query that is not live renders a clamped env (the write kernel skips it).  Non-finite
// coefficients are not looked for.  grid = cnt, block = QD_AFFINE_BLOCK.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(QD_AFFINE_BLOCK)
qd_k_affine_gather(QdAffineQuery Q, int base, int B, int N, const double* __restrict__ params, const double* __restrict__ state,
                   double* __restrict__ sparams, double* __restrict__ sstate, QdAffineAxes* __restrict__ axes) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.x, q = base + k, V = 2 * N;
    const QdSlot S = qd_slot_copy<QD_AFFINE_BLOCK>(Q, q, k, B, L, params, state, sparams, sstate, 1);   // (1 word: the descriptor's address)
    QdAffineAxes* A = axes + k;
    for (int i = threadIdx.x; i < 2 * QD_MAXN; i += QD_AFFINE_BLOCK) {
        A->dx[i] = i < V ? Q.dir[((size_t)q * 2 + 0) * V + i] : 0.0;
        A->dy[i] = i < V ? Q.dir[((size_t)q * 2 + 1) * V + i] : 0.0;
    }
    if (threadIdx.x == 0) {
        A->x_lo = Q.range[4 * (size_t)q]; A->x_hi = Q.range[4 * (size_t)q + 1];
        A->y_lo = Q.range[4 * (size_t)q + 2]; A->y_hi = Q.range[4 * (size_t)q + 3];
        A->frame = Q.frame; A->pad = 0;
        *reinterpret_cast<const QdAffineAxes**>(S.ds + L.s_kmean) = A;
    }
}
