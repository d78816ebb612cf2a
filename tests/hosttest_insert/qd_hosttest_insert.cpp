// CPU build of both forms of the kept-set insert of the exact per-pixel search (csrc/qd_pixel.h: qd_search_insert and what it
// calls, QdSearch<N, KC, PACKED>) and of the whole search qd_candidates<N, KC, PACKED> in both forms.
// TEST INFRASTRUCTURE: loaded only by tests/test_search_insert_cpu.py (and linked into qd_insert_asan); never used by the product.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "qd_pixel.h"

// One row of QDHI_ROW 64-bit words per insert: count, the KC energies (bits), the KC ids, then for 4 groups (zero past NG)
// the maximum's energy (bits), id and slot, then maxE (bits), maxI, maxS, maxG and lim (bits).
#define QDHI_ROW (1 + 32 + 32 + 12 + 5)
// the buffer is strided as on the device: slot k of lane l at k * 64 + l
#define QDHI_STRIDE 64
#define QDHI_LANE 37

namespace {

uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, sizeof u); return u; }

template <int KC, bool PACKED>
void stream(long n, const double* E, const uint32_t* idx, uint64_t* rows) {
    static double ke[32 * QDHI_STRIDE];
    static uint16_t kid[32 * QDHI_STRIDE];
    for (int k = 0; k < 32 * QDHI_STRIDE; ++k) { ke[k] = -1.0; kid[k] = 0xFFFF; }
    QdSearch<8, KC, PACKED> S;
    constexpr int NG = QdSearch<8, KC, PACKED>::NG;
    // every member the insert reads or leaves alone, set alike in both forms
    S.Em = 0.25; S.e = ke + QDHI_LANE; S.es = QDHI_STRIDE; S.id = kid + QDHI_LANE; S.is = QDHI_STRIDE;
    S.count = 0; S.lim = INFINITY; S.idx = 0; S.maxE = 0.0; S.maxI = 0; S.maxS = 0; S.maxG = 0; S.gSp = 0;
    for (int g = 0; g < NG; ++g) { S.gE[g] = 0.0; S.gI[g] = 0; S.gS[g] = 0; }
    S.nodes = S.leaves = S.inserts = S.shifts = 0;
    for (long t = 0; t < n; ++t) {
        qd_search_insert(S, E[t], idx[t]);
        uint64_t* r = rows + (size_t)t * QDHI_ROW;
        memset(r, 0, sizeof(uint64_t) * QDHI_ROW);
        r[0] = (uint64_t)S.count;
        for (int k = 0; k < KC; ++k) { r[1 + k] = bits(ke[k * QDHI_STRIDE + QDHI_LANE]); r[33 + k] = kid[k * QDHI_STRIDE + QDHI_LANE]; }
        for (int g = 0; g < NG; ++g) { r[65 + g] = bits(S.gE[g]); r[69 + g] = S.gI[g]; r[73 + g] = (uint64_t)(int64_t)S.group_slot(g); }
        r[77] = bits(S.maxE); r[78] = S.maxI; r[79] = (uint64_t)(int64_t)S.maxS; r[80] = (uint64_t)(int64_t)S.maxG; r[81] = bits(S.lim);
    }
    // nothing outside the lane's KC slots was written
    for (int k = 0; k < 32 * QDHI_STRIDE; ++k) {
        const bool own = (k % QDHI_STRIDE) == QDHI_LANE && k / QDHI_STRIDE < KC;
        if (!own && (ke[k] != -1.0 || kid[k] != 0xFFFF)) rows[0] = ~0ull;
    }
}

template <int N, int KC, bool PACKED>
void front(const double* par, const double* st, int ch, int R, int sort, double* e_out, uint16_t* id_out, int32_t* nvalid,
           int32_t* fl_out, unsigned long long* stats) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N;
    for (int p = 0; p < R * R; ++p) {
        double v_ext[V], vpp[G], vd[N], ncont[N], tc[NB > 0 ? NB : 1], isa;
        qd_pixel_front<N>(par, st, ch, R, p % R, p / R, v_ext, vpp, vd, ncont, tc, &isa);
        double e[KC]; uint16_t id[KC];
        for (int k = 0; k < KC; ++k) { e[k] = -1.0; id[k] = 0xFFFF; }
        nvalid[p] = qd_candidates<N, KC, PACKED>(par, vd, ncont, e, 1, id, 1, fl_out + (size_t)p * N, sort != 0, stats);
        memcpy(e_out + (size_t)p * KC, e, sizeof e);
        memcpy(id_out + (size_t)p * KC, id, sizeof id);
    }
}

}  // namespace

extern "C" {

int qdhi_row_words() { return QDHI_ROW; }

// n inserts of (E[t], idx[t]) into an empty kept set of KC slots in the form `packed`; rows: [n][QDHI_ROW]
int qdhi_stream(int KC, int packed, long n, const double* E, const uint32_t* idx, uint64_t* rows) {
#define C(KK) if (packed) stream<KK, true>(n, E, idx, rows); else stream<KK, false>(n, E, idx, rows)
    switch (KC) { case 8: C(8); break; case 16: C(16); break; case 32: C(32); break; default: return 1; }
#undef C
    return 0;
}

// the whole search over the R x R pixels of channel ch in the form `packed`: e_out, id_out [R*R][KC] (slots from nvalid on
// keep -1.0 / 0xFFFF), nvalid [R*R], fl_out [R*R][N], stats [4] (nodes, leaves, inserts, shifts; added to)
int qdhi_front(int N, int KC, int packed, const double* par, const double* st, int ch, int R, int sort, double* e_out,
               uint16_t* id_out, int32_t* nvalid, int32_t* fl_out, unsigned long long* stats) {
#define F(NN, KK) if (packed) front<NN, KK, true>(par, st, ch, R, sort, e_out, id_out, nvalid, fl_out, stats); \
                  else front<NN, KK, false>(par, st, ch, R, sort, e_out, id_out, nvalid, fl_out, stats)
#define C(NN) switch (KC) { case 8: F(NN, 8); break; case 16: F(NN, 16); break; case 32: F(NN, 32); break; default: return 1; }
    switch (N) {
        case 2: C(2); break; case 3: C(3); break; case 4: C(4); break; case 5: C(5); break;
        case 6: C(6); break; case 7: C(7); break; case 8: C(8); break; default: return 1;
    }
#undef C
#undef F
    return 0;
}

}  // extern "C"
