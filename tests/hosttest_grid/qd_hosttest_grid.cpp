// CPU driver of the grid front end of csrc/qd_grid.h (qd_grid_voltages, qd_grid_record) and of the row walk of its latching
// stage (qd_grid_latch_row).
#include <stdint.h>
#include <string.h>
#include "qd_grid.h"

static QdGridAxes axes_of(int N, const double* dir2, int frame, const double* range4, int nx, int ny) {
    QdGridAxes A;
    memset(&A, 0, sizeof(A));
    A.x_lo = range4[0]; A.x_hi = range4[1]; A.y_lo = range4[2]; A.y_hi = range4[3];
    for (int i = 0; i < 2 * N; ++i) { A.dx[i] = dir2[i]; A.dy[i] = dir2[2 * N + i]; }
    A.nx = nx; A.ny = ny; A.frame = frame;
    return A;
}

// v_ext [ny*nx][2N], vpp [ny*nx][N+1], tc [ny*nx][N-1] of every point (row-major: p = y nx + x) of an nx x ny grid
template <int N>
static void grid(const double* par, const double* st, const QdGridAxes& A, double* v_ext, double* vpp, double* tc) {
    for (int p = 0; p < A.nx * A.ny; ++p)
        qd_grid_voltages<N>(par, st, &A, A.nx, A.ny, p % A.nx, p / A.nx, v_ext + (size_t)p * 2 * N, vpp + (size_t)p * (N + 1),
                            tc + (size_t)p * (N - 1));
}

// the side*side records of the grid's slot as the front kernel fills them (before the hand-over): live [SP] says which are points
template <int N>
static void records(const double* par, const double* st, const QdGridAxes& A, QdPixelRec* recs, int* live) {
    const int side = qd_line_side(A.nx * A.ny), SP = side * side;
    for (int j = 0; j < SP; ++j) {
        double v_ext[2 * N], vd[N], ncont[N], isa;
        live[j] = qd_grid_record<N>(par, st, &A, A.nx, A.ny, j, recs + j, v_ext, vd, ncont, &isa) ? 1 : 0;
    }
}

// dir2 [2][2N]: dx then dy
extern "C" int qdhg_grid_voltages(int N, const double* par, const double* st, const double* dir2, int frame, const double* range4,
                                  int nx, int ny, double* v_ext, double* vpp, double* tc) {
    if (N < 2 || N > QD_MAXN || nx < 1 || ny < 1) return 1;
    const QdGridAxes A = axes_of(N, dir2, frame, range4, nx, ny);
    switch (N) {
#define C(k) case k: grid<k>(par, st, A, v_ext, vpp, tc); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}

extern "C" int qdhg_record_bytes(void) { return (int)sizeof(QdPixelRec); }
extern "C" int qdhg_axes_bytes(void) { return (int)sizeof(QdGridAxes); }

extern "C" int qdhg_grid_records(int N, const double* par, const double* st, const double* dir2, int frame, const double* range4,
                                 int nx, int ny, unsigned char* recs, int* live) {
    if (N < 2 || N > QD_MAXN || nx < 1 || ny < 1) return 1;
    const QdGridAxes A = axes_of(N, dir2, frame, range4, nx, ny);
    switch (N) {
#define C(k) case k: records<k>(par, st, A, reinterpret_cast<QdPixelRec*>(recs), live); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}

// the latching walk of one slot as qd_k_latch_grid runs it, rows from the last to the first (they are independent): occ
// [SP][N] and z [SP] with SP >= nx*ny, the tail is not touched.  The Philox key is (seed, k1), the serial (ser_lo, ser_hi).
extern "C" int qdhg_latch_grid(int N, const double* par, double* occ, double* z, int nx, int ny, uint32_t seed, uint32_t ser_lo,
                               uint32_t ser_hi, uint32_t k1) {
    if (N < 2 || N > QD_MAXN || nx < 1 || ny < 1) return 1;
    switch (N) {
#define C(k) case k: for (int y = ny - 1; y >= 0; --y) qd_grid_latch_row<k>(par, qd_layout(k), occ, z, nx, y, seed, ser_lo, ser_hi, k1); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}
