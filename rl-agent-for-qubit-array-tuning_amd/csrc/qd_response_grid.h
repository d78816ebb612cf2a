// qd_response_grid.h -- what qd_api.hip sees of the charge-response grids: the caller's rows and the launcher of
// qd_k_thermal_grid_response (qd_response_blocks.h).  The kernel's instances live in a translation unit of their own,
// qd_response_grid.hip: qd_response_solve<N> is shared with qd_k_thermal_response<N>, and with that second caller in ONE
// translation unit the compiler emitted the existing kernel differently (1 or 2 VGPRs, some tens of bytes, and 2.5 % of the
// 8-dot point route's time: DESIGN 7).  Apart, the device code of qd_api.hip is that of its own sources.
#pragma once
#include <hip/hip_runtime.h>

// the caller's rows of qd_scan_grid_response, [nq][ny][nx] x the shapes below; any subset may be null
struct QdGridResponseDst {
    double *chi, *jac, *dsignal;            // [N][2N-1], [N][2N], [2N]
    double *docc_axes, *dsignal_axes;       // [N][2], [2]
};

// Launches qd_k_thermal_grid_response<N, WS> on `grid` blocks of one wave; whole: WS = QdResponseWs (qd_thermal_solve and
// qd_response_solve on the whole block), else QdResponseBlocksWs.  query: the call's QdAffineQuery, query_bytes its sizeof; axes:
// its QdGridAxes, recs: its QdPixelRec (the other unit includes the headers into a namespace of its own, so these travel
// untyped).  false: N outside 2..8 or a query of another size, nothing launched.
__attribute__((visibility("hidden")))
bool qd_launch_thermal_grid_response(int N, bool whole, dim3 grid, hipStream_t s, const void* query, size_t query_bytes, int base,
                                     int B, int n, int SP, int kept, const double* kT_dev, const double* sparams,
                                     const double* sstate, const void* axes, const void* recs, double* zraw, double* socc,
                                     double* var_dst, double* ztail_dst, const QdGridResponseDst& R);
