// CPU driver of csrc/qd_thermal.h: the core a wavefront runs on the block of one point, with the lanes as a loop.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "qd_thermal.h"

// packed: lower triangle, row-major, s (s + 1) / 2 doubles.  Outputs: pop[s], lam[s] (units of the input, the order of the
// columns of V), V[s][s] row-major (column k: eigenvector k), ztail.  Returns the number of sweeps, or -1 for a size outside
// 1..32 or a kT that is not finite and positive, -2 without memory.
extern "C" int qdht_thermal(int s, const double* packed, double kT, double* pop, double* lam, double* V, double* ztail) {
    if (s < 1 || s > QD_LV_MAX || !(kT > 0.0) || !(kT < INFINITY)) return -1;
    QdThermalWs* W = (QdThermalWs*)malloc(sizeof(QdThermalWs));
    if (!W) return -2;
    qd_levels_load_packed(W->B, packed, s);
    const int sweeps = qd_thermal_solve(*W, s, kT);
    for (int i = 0; i < s; ++i) {
        pop[i] = W->pop[i]; lam[i] = W->lam[i];
        for (int j = 0; j < s; ++j) V[i * s + j] = W->V[i * QD_LV_LD + j];
    }
    *ztail = W->ztail;
    free(W);
    return sweeps;
}

extern "C" int qdht_sweep_cap() { return QD_TH_SWEEPS; }
extern "C" int qdht_ws_bytes() { return (int)sizeof(QdThermalWs); }

// The record path of qd_k_thermal for one point: the record is put together from its fields (idx[32], fl[N], tc[N-1], E[32],
// nvalid), nv = min(nvalid, kept).  Outputs: pop[32] (zero from nv on), occ[N], var[N], ztail.  Returns nv, or -1 for a bad
// argument.
template <int N>
static int record(const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept, double kT,
                  double* pop, double* occ, double* var, double* ztail) {
    QdPixelRec* rec = (QdPixelRec*)calloc(1, sizeof(QdPixelRec));
    QdThermalWs* W = (QdThermalWs*)malloc(sizeof(QdThermalWs));
    if (!rec || !W) { free(rec); free(W); return -1; }
    for (int m = 0; m < QD_K; ++m) { rec->idx[m] = idx[m]; rec->E[m] = E[m]; }
    for (int i = 0; i < N; ++i) rec->fl[i] = fl[i];
    for (int b = 0; b < N - 1; ++b) rec->tc[b] = tc[b];
    rec->nvalid = nvalid;
    int nv = nvalid < kept ? nvalid : kept;
    nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
    memset(pop, 0, sizeof(double) * QD_LV_MAX);
    for (int i = 0; i < N; ++i) occ[i] = var[i] = 0.0;
    *ztail = 1.0;
    if (nv > 0) {
        qd_levels_record<N>(W->B, rec, nv);
        qd_thermal_solve(*W, nv, kT);
        qd_thermal_moments<N>(*W, rec, nv);
        for (int m = 0; m < nv; ++m) pop[m] = W->pop[m];
        for (int i = 0; i < N; ++i) { occ[i] = W->occ[i]; var[i] = W->var[i]; }
        *ztail = W->ztail;
    }
    free(W); free(rec);
    return nv;
}

extern "C" int qdht_record(int N, const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept,
                           double kT, double* pop, double* occ, double* var, double* ztail) {
    if (kept < 1 || kept > QD_K || !(kT > 0.0) || !(kT < INFINITY)) return -1;
    switch (N) {
        case 2: return record<2>(idx, fl, tc, E, nvalid, kept, kT, pop, occ, var, ztail);
        case 3: return record<3>(idx, fl, tc, E, nvalid, kept, kT, pop, occ, var, ztail);
        case 4: return record<4>(idx, fl, tc, E, nvalid, kept, kT, pop, occ, var, ztail);
        case 5: return record<5>(idx, fl, tc, E, nvalid, kept, kT, pop, occ, var, ztail);
        case 6: return record<6>(idx, fl, tc, E, nvalid, kept, kT, pop, occ, var, ztail);
        case 7: return record<7>(idx, fl, tc, E, nvalid, kept, kT, pop, occ, var, ztail);
        case 8: return record<8>(idx, fl, tc, E, nvalid, kept, kT, pop, occ, var, ztail);
    }
    return -1;
}
