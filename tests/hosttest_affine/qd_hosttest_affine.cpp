// CPU driver of the affine front end of csrc/qd_pixel.h (qd_affine_voltages, through QdFrontAffine: the descriptor's address
// travels in the state block copy, as on the device).
#include <stdint.h>
#include <string.h>
#include "qd_pixel.h"

// v_ext [P][2N], vpp [P][N+1], tc [P][N-1] of every pixel (row-major: p = y R + x) of an R x R scan along (dx, dy)
template <int N>
static void affine(const double* par, const double* st_in, const QdAffineAxes& A, int R, double* v_ext, double* vpp, double* tc) {
    const QdLayout L = qd_layout(N);
    double st[QD_MAXN * (4 * QD_MAXN + 8)];                       // >= s_size = (N+1)^2 + 4N - 1 + 2 N^2 (+ 1)
    memcpy(st, st_in, sizeof(double) * L.s_size);
    const QdAffineAxes* addr = &A;
    memcpy(st + L.s_kmean, &addr, sizeof(addr));
    for (int p = 0; p < R * R; ++p)
        QdFrontAffine::voltages<N>(par, st, 0, R, p % R, p / R, v_ext + (size_t)p * 2 * N, vpp + (size_t)p * (N + 1), tc + (size_t)p * (N - 1));
}

// dir2 [2][2N]: dx then dy
extern "C" int qdha_affine_voltages(int N, const double* par, const double* st, const double* dir2, int frame, const double* range4,
                                    int R, double* v_ext, double* vpp, double* tc) {
    if (N < 2 || N > QD_MAXN) return 1;
    QdAffineAxes A;
    memset(&A, 0, sizeof(A));
    A.x_lo = range4[0]; A.x_hi = range4[1]; A.y_lo = range4[2]; A.y_hi = range4[3];
    for (int i = 0; i < 2 * N; ++i) { A.dx[i] = dir2[i]; A.dy[i] = dir2[2 * N + i]; }
    A.frame = frame;
    switch (N) {
#define C(n) case n: affine<n>(par, st, A, R, v_ext, vpp, tc); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}
