// qd_response_grid.hip -- the instances of qd_k_thermal_grid_response (qd_response_blocks.h) and their launcher, in a translation
// unit of their own inside libqdsim.so (qd_response_grid.h says why).  The kernel headers also define kernels that are no
// templates; qd_api.hip defines them for the library.  Here the headers are included into an unnamed namespace, so nothing is
// defined twice.  The compiler still emits those seven kernels here (qd_k_grid_gather, qd_k_line_gather, qd_k_points_gather,
// qd_k_query_write, qd_k_line_pack, qd_k_telegraph, qd_k_snapshot): copies under this unit's own names that nothing launches.
// Taking them out of the shared headers, or marking them there, would touch the sources of every existing kernel and is left.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include "qdsim.h"
#include "qd_response_grid.h"

namespace {
#include "qd_response_blocks.h"

template <class WS>
bool qd_rsg_launch(int N, dim3 grid, hipStream_t s, const QdAffineQuery& Q, int base, int B, int n, int SP, int kept,
                   const double* kT, const double* sparams, const double* sstate, const QdGridAxes* axes, const QdPixelRec* recs,
                   double* zraw, double* socc, double* var_dst, double* ztail_dst, const QdGridResponseDst& R) {
    switch (N) {
#define QD_RSG_CASE(NN)                                                                                                              \
    case NN:                                                                                                                         \
        qd_k_thermal_grid_response<NN, WS><<<grid, dim3(64), 0, s>>>(Q, base, B, n, SP, kept, kT, sparams, sstate, axes, recs, zraw,     \
                                                                     socc, var_dst, ztail_dst, R);                                   \
        return true;
        QD_RSG_CASE(2) QD_RSG_CASE(3) QD_RSG_CASE(4) QD_RSG_CASE(5) QD_RSG_CASE(6) QD_RSG_CASE(7) QD_RSG_CASE(8)
#undef QD_RSG_CASE
    }
    return false;
}
}  // namespace

bool qd_launch_thermal_grid_response(int N, bool whole, dim3 grid, hipStream_t s, const void* query, size_t query_bytes, int base,
                                     int B, int n, int SP, int kept, const double* kT_dev, const double* sparams,
                                     const double* sstate, const void* axes, const void* recs, double* zraw, double* socc,
                                     double* var_dst, double* ztail_dst, const QdGridResponseDst& R) {
    QdAffineQuery Q;
    if (query_bytes != sizeof(Q)) return false;
    memcpy(&Q, query, sizeof(Q));
    const QdGridAxes* ax = static_cast<const QdGridAxes*>(axes);
    const QdPixelRec* rc = static_cast<const QdPixelRec*>(recs);
    return whole ? qd_rsg_launch<QdResponseWs>(N, grid, s, Q, base, B, n, SP, kept, kT_dev, sparams, sstate, ax, rc, zraw, socc, var_dst,
                                               ztail_dst, R)
                 : qd_rsg_launch<QdResponseBlocksWs>(N, grid, s, Q, base, B, n, SP, kept, kT_dev, sparams, sstate, ax, rc, zraw, socc,
                                                     var_dst, ztail_dst, R);
}
