// CPU driver of csrc/qd_levels.h: the core a wavefront runs on the block of one point, with the lanes as a loop.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "qd_levels.h"

// packed: lower triangle, row-major, s (s + 1) / 2 doubles; lev[L].  Levels from s on are +inf.
// 0 on success, 1 for a size outside 1..32 or L outside 1..QD_LEVELS_MAX.
extern "C" int qdhl_levels(int s, int L, const double* packed, double* lev) {
    if (s < 1 || s > QD_LV_MAX || L < 1 || L > QD_LEVELS_MAX) return 1;
    QdLevelsWs* W = (QdLevelsWs*)malloc(sizeof(QdLevelsWs));
    if (!W) return 2;
    qd_levels_load_packed(*W, packed, s);
    qd_levels_solve(*W, s, L);
    for (int k = 0; k < L; ++k) lev[k] = k < s ? W->lev[k] : INFINITY;
    free(W);
    return 0;
}

extern "C" int qdhl_rounds(int L) { return qd_levels_rounds(64 / L); }
extern "C" int qdhl_ws_bytes() { return (int)sizeof(QdLevelsWs); }

// The record path of qd_k_levels for one point: the record is put together from its fields (idx[32], fl[N], tc[N-1], E[32],
// nvalid), nv = min(nvalid, kept).  Outputs: H[32][32] row-major, the lower triangle as the core built it mirrored to the full
// matrix (rows and columns from nv on: zero), hnorm, lev[L] (+inf from nv on).  Returns nv, or -1 for a bad argument.
template <int N>
static int record(const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept, int L,
                  double* H, double* hnorm, double* lev) {
    QdPixelRec* rec = (QdPixelRec*)calloc(1, sizeof(QdPixelRec));
    QdLevelsWs* W = (QdLevelsWs*)malloc(sizeof(QdLevelsWs));
    if (!rec || !W) { free(rec); free(W); return -1; }
    for (int m = 0; m < QD_K; ++m) { rec->idx[m] = idx[m]; rec->E[m] = E[m]; }
    for (int i = 0; i < N; ++i) rec->fl[i] = fl[i];
    for (int b = 0; b < N - 1; ++b) rec->tc[b] = tc[b];
    rec->nvalid = nvalid;
    int nv = nvalid < kept ? nvalid : kept;
    nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
    memset(H, 0, sizeof(double) * QD_LV_MAX * QD_LV_MAX);
    *hnorm = 0.0;
    if (nv > 0) {
        *hnorm = qd_levels_record<N>(*W, rec, nv);
        for (int i = 0; i < nv; ++i)
            for (int j = 0; j <= i; ++j) H[i * QD_LV_MAX + j] = H[j * QD_LV_MAX + i] = W->A[i * QD_LV_LD + j];
        qd_levels_solve(*W, nv, L);
    }
    for (int k = 0; k < L; ++k) lev[k] = k < nv ? W->lev[k] : INFINITY;
    free(W); free(rec);
    return nv;
}

extern "C" int qdhl_record(int N, const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept,
                           int L, double* H, double* hnorm, double* lev) {
    if (L < 1 || L > QD_LEVELS_MAX || kept < 1 || kept > QD_K) return -1;
    switch (N) {
        case 2: return record<2>(idx, fl, tc, E, nvalid, kept, L, H, hnorm, lev);
        case 3: return record<3>(idx, fl, tc, E, nvalid, kept, L, H, hnorm, lev);
        case 4: return record<4>(idx, fl, tc, E, nvalid, kept, L, H, hnorm, lev);
        case 5: return record<5>(idx, fl, tc, E, nvalid, kept, L, H, hnorm, lev);
        case 6: return record<6>(idx, fl, tc, E, nvalid, kept, L, H, hnorm, lev);
        case 7: return record<7>(idx, fl, tc, E, nvalid, kept, L, H, hnorm, lev);
        case 8: return record<8>(idx, fl, tc, E, nvalid, kept, L, H, hnorm, lev);
    }
    return -1;
}
