// CPU driver of csrc/qd_levels_blocks.h: the core a wavefront runs on the block of one point, with the lanes as a loop.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "qd_levels_blocks.h"

// A workspace that outlives a call, so that a test can solve one task after another in it, as a block of the kernel does.
// fill: 0 zeros, 1 all-ones bits (a NaN as a double, 255 as a byte), 2 a pattern of finite garbage.
extern "C" void* qdlb_ws_new() { return calloc(1, sizeof(QdLevelsBlocksWs)); }
extern "C" void qdlb_ws_free(void* w) { free(w); }
extern "C" void qdlb_ws_fill(void* w, int fill) {
    if (fill == 2) {
        unsigned char* p = (unsigned char*)w;
        for (size_t i = 0; i < sizeof(QdLevelsBlocksWs); ++i) p[i] = (unsigned char)(37u + 11u * (unsigned)i);
        double* d = (double*)w;
        for (size_t i = 0; i < sizeof(QdLevelsWs) / sizeof(double); ++i) d[i] = 0.001 * (double)((i * 7919u) % 1000u) - 0.5;
    } else {
        memset(w, fill == 1 ? 0xFF : 0, sizeof(QdLevelsBlocksWs));
    }
}

// packed: lower triangle, row-major, s (s + 1) / 2 doubles.  Outputs: lev[L] (+inf from min(L, s) on), label[s] (the lowest
// state of the component of state i), al[s], be[s] (the concatenated tridiagonal on the solver's scale; s >= 2), mem[s] (the
// states ordered by component; s >= 2); any of the last three may be null.  Returns 0, or 1 for a size or level count outside
// the contract.
extern "C" int qdlb_levels_in(void* w, int s, int L, const double* packed, double* lev, int32_t* label, double* al, double* be,
                              int32_t* mem) {
    if (s < 1 || s > QD_LV_MAX || L < 1 || L > QD_LEVELS_MAX) return 1;
    QdLevelsBlocksWs* W = (QdLevelsBlocksWs*)w;
    qd_levels_load_packed(W->L, packed, s);
    qd_levels_blocks_solve(*W, s, L);
    for (int k = 0; k < L; ++k) lev[k] = k < s ? W->L.lev[k] : INFINITY;
    for (int i = 0; i < s; ++i) {
        label[i] = __builtin_ctz(W->ma[i]);
        if (s >= 2) {
            if (al) al[i] = W->L.al[i];
            if (be) be[i] = W->L.be[i];
            if (mem) mem[i] = W->mem[i];
        }
    }
    return 0;
}

extern "C" int qdlb_levels(int s, int L, const double* packed, double* lev, int32_t* label, double* al, double* be, int32_t* mem) {
    void* w = malloc(sizeof(QdLevelsBlocksWs));
    if (!w) return 2;
    const int rc = qdlb_levels_in(w, s, L, packed, lev, label, al, be, mem);
    free(w);
    return rc;
}

extern "C" int qdlb_ws_bytes() { return (int)sizeof(QdLevelsBlocksWs); }
extern "C" int qdlb_whole_ws_bytes() { return (int)sizeof(QdLevelsWs); }

// The record path of qd_k_levels_grid for one point: the record is put together from its fields (idx[32], fl[N], tc[N-1], E[32],
// nvalid), nv = min(nvalid, kept).  Outputs: lev[L] (+inf from nv on), hnorm.  Returns nv, or -1 for a bad argument.
template <int N>
static int record(const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept, int L, double* lev,
                  double* hnorm) {
    QdPixelRec* rec = (QdPixelRec*)calloc(1, sizeof(QdPixelRec));
    QdLevelsBlocksWs* W = (QdLevelsBlocksWs*)malloc(sizeof(QdLevelsBlocksWs));
    if (!rec || !W) { free(rec); free(W); return -1; }
    for (int m = 0; m < QD_K; ++m) { rec->idx[m] = idx[m]; rec->E[m] = E[m]; }
    for (int i = 0; i < N; ++i) rec->fl[i] = fl[i];
    for (int b = 0; b < N - 1; ++b) rec->tc[b] = tc[b];
    rec->nvalid = nvalid;
    int nv = nvalid < kept ? nvalid : kept;
    nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
    *hnorm = 0.0;
    if (nv > 0) {
        *hnorm = qd_levels_record<N>(W->L, rec, nv);
        qd_levels_blocks_solve(*W, nv, L);
    }
    for (int k = 0; k < L; ++k) lev[k] = k < nv ? W->L.lev[k] : INFINITY;
    free(W); free(rec);
    return nv;
}

extern "C" int qdlb_record(int N, const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept,
                           int L, double* lev, double* hnorm) {
    if (kept < 1 || kept > QD_K || L < 1 || L > QD_LEVELS_MAX) return -1;
    switch (N) {
        case 2: return record<2>(idx, fl, tc, E, nvalid, kept, L, lev, hnorm);
        case 3: return record<3>(idx, fl, tc, E, nvalid, kept, L, lev, hnorm);
        case 4: return record<4>(idx, fl, tc, E, nvalid, kept, L, lev, hnorm);
        case 5: return record<5>(idx, fl, tc, E, nvalid, kept, L, lev, hnorm);
        case 6: return record<6>(idx, fl, tc, E, nvalid, kept, L, lev, hnorm);
        case 7: return record<7>(idx, fl, tc, E, nvalid, kept, L, lev, hnorm);
        case 8: return record<8>(idx, fl, tc, E, nvalid, kept, L, lev, hnorm);
    }
    return -1;
}
