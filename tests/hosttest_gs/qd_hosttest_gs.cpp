// CPU driver of the hop predicate of csrc/qd_groundstate.h (qd_gs_hop), the pair test of the structure kernel.
#include <stdint.h>
#include "qd_groundstate.h"

// out[k] = qd_gs_hop(ci[k], cj[k], tcq[k]): codes with one digit per nibble, tcq with bit 4q set iff pair N-2-q couples
extern "C" void qdhg_hop(long n, const uint32_t* ci, const uint32_t* cj, const uint32_t* tcq, uint32_t* out) {
    for (long k = 0; k < n; ++k) out[k] = qd_gs_hop(ci[k], cj[k], tcq[k]);
}
