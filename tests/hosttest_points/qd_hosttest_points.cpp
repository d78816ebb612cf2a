// CPU driver of the point front end of csrc/qd_points.h (qd_point_front) and of the scan front end's voltage synthesis
// (csrc/qd_pixel.h: qd_pixel_voltages), whose v_ext the points of the tests are.
#include <stdint.h>
#include "qd_points.h"

// v_ext [P][2N], vpp [P][N+1], tc [P][N-1] of every pixel of channel ch of an R x R scan
template <int N>
static void scan_voltages(const double* par, const double* st, int ch, int R, double* v_ext, double* vpp, double* tc) {
    for (int p = 0; p < R * R; ++p)
        qd_pixel_voltages<N>(par, st, ch, R, p % R, p / R, v_ext + (size_t)p * 2 * N, vpp + (size_t)p * (N + 1), tc + (size_t)p * (N - 1));
}

// the point front end at n rows of v_ext [n][2N]: vpp [n][N+1], tc [n][N-1], vd [n][N], ncont [n][N], isa [n]
template <int N>
static void point_front(const double* par, long n, const double* v_ext, double* vpp, double* tc, double* vd, double* ncont, double* isa) {
    for (long q = 0; q < n; ++q)
        qd_point_front<N>(par, v_ext + q * 2 * N, vpp + q * (N + 1), tc + q * (N - 1), vd + q * N, ncont + q * N, isa + q);
}

extern "C" int qdhp_scan_voltages(int N, const double* par, const double* st, int ch, int R, double* v_ext, double* vpp, double* tc) {
    switch (N) {
#define C(n) case n: scan_voltages<n>(par, st, ch, R, v_ext, vpp, tc); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}

extern "C" int qdhp_point_front(int N, const double* par, long npts, const double* v_ext, double* vpp, double* tc, double* vd,
                                double* ncont, double* isa) {
    switch (N) {
#define C(n) case n: point_front<n>(par, npts, v_ext, vpp, tc, vd, ncont, isa); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}
