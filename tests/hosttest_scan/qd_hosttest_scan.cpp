// CPU driver of the scan front end of csrc/qd_pixel.h (qd_scan_voltages), of the env's front end it must reproduce on
// adjacent virtual plungers (qd_pixel_voltages) and of the point front end (csrc/qd_points.h) it must agree with at its
// own v_ext.
#include <stdint.h>
#include "qd_points.h"

// v_ext [P][2N], vpp [P][N+1], tc [P][N-1] of every pixel (row-major: p = y R + x) of an R x R scan over (ax, ay)
template <int N>
static void scan(const double* par, const double* st, const QdScanAxes& A, int R, double* v_ext, double* vpp, double* tc) {
    for (int p = 0; p < R * R; ++p)
        qd_scan_voltages<N>(par, st, A, R, p % R, p / R, v_ext + (size_t)p * 2 * N, vpp + (size_t)p * (N + 1), tc + (size_t)p * (N - 1));
}
template <int N>
static void pixel(const double* par, const double* st, int ch, int R, double* v_ext, double* vpp, double* tc) {
    for (int p = 0; p < R * R; ++p)
        qd_pixel_voltages<N>(par, st, ch, R, p % R, p / R, v_ext + (size_t)p * 2 * N, vpp + (size_t)p * (N + 1), tc + (size_t)p * (N - 1));
}
// vpp [n][N+1], tc [n][N-1] of qd_point_front at n rows of v_ext
template <int N>
static void point(const double* par, long n, const double* v_ext, double* vpp, double* tc) {
    double vd[N], ncont[N], isa;
    for (long q = 0; q < n; ++q) qd_point_front<N>(par, v_ext + q * 2 * N, vpp + q * (N + 1), tc + q * (N - 1), vd, ncont, &isa);
}

extern "C" int qdhs_scan_voltages(int N, const double* par, const double* st, int ax, int ay, int frame, const double* range4,
                                  int R, double* v_ext, double* vpp, double* tc) {
    if (ax < 0 || ax >= 2 * N || ay < 0 || ay >= 2 * N || ax == ay) return 2;
    QdScanAxes A;
    A.x_lo = range4[0]; A.x_hi = range4[1]; A.y_lo = range4[2]; A.y_hi = range4[3];
    A.ax = ax; A.ay = ay; A.frame = frame; A.pad = 0;
    switch (N) {
#define C(n) case n: scan<n>(par, st, A, R, v_ext, vpp, tc); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}

extern "C" int qdhs_pixel_voltages(int N, const double* par, const double* st, int ch, int R, double* v_ext, double* vpp, double* tc) {
    switch (N) {
#define C(n) case n: pixel<n>(par, st, ch, R, v_ext, vpp, tc); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}

extern "C" int qdhs_point_front(int N, const double* par, long npts, const double* v_ext, double* vpp, double* tc) {
    switch (N) {
#define C(n) case n: point<n>(par, npts, v_ext, vpp, tc); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}

extern "C" double qdhs_peak_width_pair(int N, const double* par, const double* st, int i, int j) {
    return qd_peak_width_pair(par, st, qd_layout(N), i, j);
}
extern "C" double qdhs_peak_width(int N, const double* par, const double* st, int ch) {
    return qd_peak_width(par, st, qd_layout(N), ch);
}
