// CPU build of the array-level pieces of the tile search (csrc/qd_tile.h: packed floor ranges, selection) and of
// the two forms of the projected gradient (csrc/qd_pixel.h: qd_pixel_continuous<N, INTERLEAVED>), each beside a literal
// restatement of the code it replaced.  TEST INFRASTRUCTURE: loaded only by tests/test_tile_front_cpu.py (and linked into
// qd_tile_asan); never used by the product.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "qd_tile.h"

namespace {

template <int N>
void pg_batch(int interleaved, long n, const double* par, long par_stride, const double* v_ext, const double* vd_in,
              double* vd_out, double* ncont, double* isa) {
    for (long b = 0; b < n; ++b) {
        double vd[N];
        for (int i = 0; i < N; ++i) vd[i] = vd_in[b * N + i];
        if (interleaved) qd_pixel_continuous<N, true>(par + b * par_stride, v_ext + b * 2 * N, vd, ncont + b * N, isa + b);
        else qd_pixel_continuous<N, false>(par + b * par_stride, v_ext + b * 2 * N, vd, ncont + b * N, isa + b);
        for (int i = 0; i < N; ++i) vd_out[b * N + i] = vd[i];
    }
}

template <int KC>
void select(int fill, int nS, int nSfront, int scap, const uint32_t* scode, const double* sD, const double* sa, const double* sb,
            double xs, double ys, uint32_t blo, uint32_t bhi, double amb, double* e_out, uint16_t* id_out, double* maxE, int* ms,
            double* eout, int* redo) {
    static double ke[QD_K * 64];
    static uint16_t kid[QD_K * 64];
    for (int k = 0; k < QD_K * 64; ++k) { ke[k] = -1.0; kid[k] = 0xFFFF; }
    const int lane = 37;
    int count;
    if (fill) qd_tile_select<KC, true>(nS, nSfront, scap, scode, sD, sa, sb, xs, ys, blo, bhi, ke + lane, kid + lane, *maxE, ms[0], ms[1], count, *eout);
    else qd_tile_select<KC, false>(nS, nSfront, scap, scode, sD, sa, sb, xs, ys, blo, bhi, ke + lane, kid + lane, *maxE, ms[0], ms[1], count, *eout);
    ms[2] = count;
    *redo = (count < KC) || !(*eout - *maxE > amb);                        // the decision of qd_k_tile
    for (int k = 0; k < KC; ++k) { e_out[k] = ke[k * 64 + lane]; id_out[k] = kid[k * 64 + lane]; }
}

}  // namespace

#define QDHT_N(CALL)                                                                                                   \
    switch (N) {                                                                                                       \
        case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; case 5: CALL(5); break;                \
        case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break; default: return 1;                     \
    }

extern "C" {

int qdht_pg(int N, int interleaved, long n, const double* par, long par_stride, const double* v_ext, const double* vd_in,
            double* vd_out, double* ncont, double* isa) {
#define C(NN) pg_batch<NN>(interleaved, n, par, par_stride, v_ext, vd_in, vd_out, ncont, isa)
    QDHT_N(C)
#undef C
    return 0;
}

int qdht_fl_packable(int fl) { return qd_fl_packable(fl) ? 1 : 0; }

// minimum and maximum of 64 packable floors as qd_wminmax_fl reduces them: the four row steps (lane ^ 1, lane ^ 2, the
// mirror of 8, the mirror of 16) with the per-field minimum, then the fold of the four row words
void qdht_fl_minmax(const int* fl, int* mn, int* mx) {
    uint32_t v[64], t[64];
    for (int l = 0; l < 64; ++l) v[l] = qd_fl_pack(fl[l]);
    for (int step = 0; step < 4; ++step) {
        for (int l = 0; l < 64; ++l) {
            const int src = step == 0 ? (l ^ 1) : step == 1 ? (l ^ 2) : step == 2 ? ((l & ~7) | (7 - (l & 7))) : ((l & ~15) | (15 - (l & 15)));
            t[l] = qd_fl_pkmin(v[l], v[src]);
        }
        memcpy(v, t, sizeof v);
    }
    uint32_t w = v[0];
    for (int r = 16; r < 64; r += 16) w = qd_fl_pkmin(w, v[r]);
    qd_fl_unpack(w, *mn, *mx);
}

int qdht_select(int KC, int fill, int nS, int nSfront, int scap, const uint32_t* scode, const double* sD, const double* sa,
                const double* sb, double xs, double ys, uint32_t blo, uint32_t bhi, double amb, double* e_out, uint16_t* id_out,
                double* maxE, int* ms, double* eout, int* redo) {
#define C(KK) select<KK>(fill, nS, nSfront, scap, scode, sD, sa, sb, xs, ys, blo, bhi, amb, e_out, id_out, maxE, ms, eout, redo)
    switch (KC) { case 8: C(8); break; case 16: C(16); break; case 32: C(32); break; default: return 1; }
#undef C
    return 0;
}

}  // extern "C"
