// qd_hosttest.cpp -- CPU-only TEST HARNESS around the __host__ __device__ code
// in qd_pixel.h and qd_eig.h.  It exists so the per-pixel device code (sweep,
// continuous state, exact k-best search, sensor stage) and the per-task dense
// eigen-solver of the ground-state kernel can be checked against the oracle /
// numpy in the no-GPU test tier.  It is NOT part of the product: nothing in
// qadapt_hip loads it (the hop structure / task emission / selection phases of the
// ground-state kernel only exist as HIP code).  It also drives the buffer owner of qd_scratch.h on a fake memory policy
// (tests/test_scratch_cpu.py).  Built by tests/hosttest/Makefile.
#include <string.h>
#include "qd_pixel.h"
#include "qd_rng.h"
#include "qd_eig.h"
#include "qd_scratch.h"
#include <stdlib.h>

template <int N>
static int run_front(const double* par, const double* st, int ch, int R, int p0, int p1,
                     int32_t* states, int32_t* floors, double* vpp_out, double* tc_out,
                     int32_t* nvalid, unsigned long long* stats, double* vd_out, double* e_out) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N;
    for (int p = p0; p < p1; ++p) {
        int y = p / R, x = p % R;
        double v_ext[V], vpp[G], vd[N], ncont[N], tc[NB > 0 ? NB : 1], isa;
        qd_pixel_front<N>(par, st, ch, R, x, y, v_ext, vpp, vd, ncont, tc, &isa);
        double e[QD_K]; uint16_t id[QD_K]; int32_t fl[N];
        int nv = qd_candidates<N>(par, vd, ncont, e, 1, id, 1, fl, true, stats);
        if (vd_out) memcpy(vd_out + (size_t)p * N, vd, sizeof(double) * N);
        if (e_out) for (int m = 0; m < QD_K; ++m) e_out[(size_t)p * QD_K + m] = m < nv ? e[m] * isa : 0.0;
        static const int DELTA[4] = {-1, 0, 1, 2};
        for (int m = 0; m < QD_K; ++m)
            for (int i = 0; i < N; ++i) {
                int dig = (id[m] >> (2 * (N - 1 - i))) & 3;
                states[((size_t)p * QD_K + m) * N + i] = m < nv ? fl[i] + DELTA[dig] : 0;
            }
        memcpy(floors + (size_t)p * N, fl, sizeof(int32_t) * N);
        memcpy(vpp_out + (size_t)p * G, vpp, sizeof(double) * G);
        memcpy(tc_out + (size_t)p * NB, tc, sizeof(double) * NB);
        nvalid[p] = nv;
    }
    return 0;
}

extern "C" int qdh_front(int N, const double* par, const double* st, int ch, int R, int p0, int p1,
                         int32_t* states, int32_t* floors, double* vpp_out, double* tc_out,
                         int32_t* nvalid, unsigned long long* stats, double* vd_out, double* e_out) {
    switch (N) {
#define C(n) case n: return run_front<n>(par, st, ch, R, p0, p1, states, floors, vpp_out, tc_out, nvalid, stats, vd_out, e_out);
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return 1;
}

extern "C" double qdh_peak_width(int N, const double* par, const double* st, int ch) {
    return qd_peak_width(par, st, qd_layout(N), ch);
}

extern "C" double qdh_sensor(int N, const double* par, const double* vpp, const double* occ, double gamma) {
    switch (N) {
#define C(n) case n: return qd_sensor<n>(par, vpp, occ, gamma);
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return -1.0;
}

extern "C" void qdh_layout(int N, int* out) {
    QdLayout L = qd_layout(N);
    memcpy(out, &L, sizeof(L));
}
extern "C" int qdh_layout_ints() { return (int)(sizeof(QdLayout) / sizeof(int)); }

extern "C" void qdh_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out4) {
    QdPhilox r = qd_philox4x32_10(c0, c1, c2, c3, k0, k1);
    for (int i = 0; i < 4; ++i) out4[i] = r.v[i];
}
extern "C" void qdh_normals(uint32_t k0, uint32_t k1, int n, double* out) {
    for (int i = 0; i < n; i += 2) {
        QdPhilox r = qd_philox4x32_10((uint32_t)(i / 2), 7u, 0u, 0u, k0, k1);
        double a, b; qd_normal2(r, a, b);
        out[i] = a; if (i + 1 < n) out[i + 1] = b;
    }
}

// lowest eigenpair of one packed symmetric block with the kernel's own solver (csrc/qd_eig.h): register version for
// s <= QD_EIG_REG, in-memory version above
extern "C" int qdh_eig_lowest(int s, const double* packed, double* lam, double* x, double* resid, int* iters) {
    switch (s) {
#define C(n) case n: qd_eig_lowest<n, true>(packed, *lam, x, *resid, iters); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8) C(10) C(12)
#undef C
        // odd sizes above 8 run padded, exactly as the kernel's size classes do
        case 9: { double xx[10]; qd_eig_lowest<10, true>(packed, *lam, xx, *resid, iters, 9); memcpy(x, xx, sizeof(double) * 9); return 0; }
        case 11: { double xx[12]; qd_eig_lowest<12, true>(packed, *lam, xx, *resid, iters, 11); memcpy(x, xx, sizeof(double) * 11); return 0; }
    }
    if (s < 2 || s > 32) return 1;
    const int ne = s * (s + 1) / 2;
    double* M = (double*)malloc(sizeof(double) * (ne + 4 * s));
    if (!M) return 2;
    memcpy(M, packed, sizeof(double) * ne);
    qd_eig_lowest_mem(s, M, M + ne, packed, *lam, *resid, iters);
    memcpy(x, M + ne + 3 * s, sizeof(double) * s);
    free(M);
    return 0;
}

// ---- qd_scratch.h: QdBuf and qd_reserve_group on a memory policy that counts live blocks, records the sizes asked for,
// fails the k-th next allocation on request, and checks IN alloc() that no more blocks are alive than buffers exist
// (a growing buffer has given its old block back by then)
struct QdhFake {
    static long long live, limit, over, allocs, releases, last_bytes, fail_in;
    static int alloc(void** p, size_t bytes) {
        ++allocs; last_bytes = (long long)bytes;
        if (live + 1 > limit) over = 1;
        if (fail_in > 0 && --fail_in == 0) return 2;
        *p = malloc(bytes);
        if (!*p) return 2;
        ++live;
        return 0;
    }
    static int release(void* p) { ++releases; --live; free(p); return 0; }
};
long long QdhFake::live, QdhFake::limit, QdhFake::over, QdhFake::allocs, QdhFake::releases, QdhFake::last_bytes, QdhFake::fail_in;

struct QdhScratch { QdBuf<double, QdhFake> b[4]; };

// nbuf: how many of the four buffers the caller is going to use (the fake's bound on live blocks)
extern "C" void* qdh_scr_new(int nbuf) {
    QdhFake::live = QdhFake::over = QdhFake::allocs = QdhFake::releases = QdhFake::last_bytes = QdhFake::fail_in = 0;
    QdhFake::limit = nbuf;
    return new QdhScratch();
}
extern "C" void qdh_scr_delete(void* o) { delete (QdhScratch*)o; }
extern "C" int qdh_scr_reserve(void* o, int k, long long n) { return ((QdhScratch*)o)->b[k].reserve((size_t)n); }
extern "C" int qdh_scr_reserve_group(void* o, const long long* n4) {
    QdhScratch* t = (QdhScratch*)o;
    QdBuf<double, QdhFake>* const g[] = {&t->b[0], &t->b[1], &t->b[2], &t->b[3]};
    const size_t n[] = {(size_t)n4[0], (size_t)n4[1], (size_t)n4[2], (size_t)n4[3]};
    return qd_reserve_group(g, n);
}
extern "C" void qdh_scr_fail_in(int k) { QdhFake::fail_in = k; }
// out[0..3]: the buffers' pointers (as integers), out[4..7]: their capacities
extern "C" void qdh_scr_bufs(void* o, long long* out) {
    for (int k = 0; k < 4; ++k) { out[k] = (long long)(size_t)((QdhScratch*)o)->b[k].p; out[4 + k] = (long long)((QdhScratch*)o)->b[k].cap; }
}
// out[0..4]: live blocks, bound exceeded (0 / 1), alloc calls, release calls, bytes of the last request
extern "C" void qdh_scr_fake(long long* out) {
    out[0] = QdhFake::live; out[1] = QdhFake::over; out[2] = QdhFake::allocs; out[3] = QdhFake::releases; out[4] = QdhFake::last_bytes;
}
