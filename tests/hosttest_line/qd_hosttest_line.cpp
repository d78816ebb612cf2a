// CPU driver of the line front end of csrc/qd_line.h (qd_line_voltages, qd_line_record) and of its slot arithmetic
// (qd_line_side, qd_line_tail, qd_line_batches).
#include <stdint.h>
#include <string.h>
#include "qd_line.h"

static QdLineAxes axes_of(int N, const double* dir, int frame, const double* range2) {
    QdLineAxes A;
    memset(&A, 0, sizeof(A));
    A.lo = range2[0]; A.hi = range2[1];
    for (int i = 0; i < 2 * N; ++i) A.d[i] = dir[i];
    A.frame = frame;
    return A;
}

// v_ext [n][2N], vpp [n][N+1], tc [n][N-1] of every point of a line of n along dir
template <int N>
static void line(const double* par, const double* st, const QdLineAxes& A, int n, double* v_ext, double* vpp, double* tc) {
    for (int t = 0; t < n; ++t)
        qd_line_voltages<N>(par, st, &A, n, t, v_ext + (size_t)t * 2 * N, vpp + (size_t)t * (N + 1), tc + (size_t)t * (N - 1));
}

// the side*side records of the line's slot as the front kernel fills them (before the hand-over): live [SP] says which are points
template <int N>
static void records(const double* par, const double* st, const QdLineAxes& A, int n, QdPixelRec* recs, int* live) {
    const int side = qd_line_side(n), SP = side * side;
    for (int j = 0; j < SP; ++j) {
        double v_ext[2 * N], vd[N], ncont[N], isa;
        live[j] = qd_line_record<N>(par, st, &A, n, j, recs + j, v_ext, vd, ncont, &isa) ? 1 : 0;
    }
}

extern "C" int qdhl_line_voltages(int N, const double* par, const double* st, const double* dir, int frame, const double* range2,
                                  int n, double* v_ext, double* vpp, double* tc) {
    if (N < 2 || N > QD_MAXN || n < 1) return 1;
    const QdLineAxes A = axes_of(N, dir, frame, range2);
    switch (N) {
#define C(k) case k: line<k>(par, st, A, n, v_ext, vpp, tc); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}

extern "C" int qdhl_record_bytes(void) { return (int)sizeof(QdPixelRec); }

extern "C" int qdhl_line_records(int N, const double* par, const double* st, const double* dir, int frame, const double* range2,
                                 int n, unsigned char* recs, int* live) {
    if (N < 2 || N > QD_MAXN || n < 1) return 1;
    const QdLineAxes A = axes_of(N, dir, frame, range2);
    switch (N) {
#define C(k) case k: records<k>(par, st, A, n, reinterpret_cast<QdPixelRec*>(recs), live); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}

// out3: side, tail records, ground-state batches of one slot
extern "C" int qdhl_slot(int n, int ppb, int* out3) {
    if (n < 1 || ppb < 1) return 1;
    out3[0] = qd_line_side(n); out3[1] = qd_line_tail(n); out3[2] = qd_line_batches(n, ppb);
    return 0;
}
