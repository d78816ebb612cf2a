// CPU driver of qd_latch_row (csrc/qd_latch.h): one raster row of the latching walk, in place.
#include <stdint.h>
#include "qd_latch.h"

// occ [R*R][N] and z [R*R] of channel ch of one scan; latches row `row` only.  par: a parameter block; the Philox key is
// (seed, k1), the serial (ser_lo, ser_hi).
extern "C" int qdhl_latch_row(int N, const double* par, double* occ, double* z, int row, int R, int ch, uint32_t seed,
                              uint32_t ser_lo, uint32_t ser_hi, uint32_t k1) {
    if (row < 0 || row >= R) return 1;
    switch (N) {
#define C(n) case n: qd_latch_row<n>(par, qd_layout(n), occ + (size_t)row * R * n, z + (size_t)row * R, row, R, ch, seed, ser_lo, ser_hi, k1); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}
