// CPU driver of csrc/qd_thermal_blocks.h: the core a wavefront runs on the block of one point, with the lanes as a loop.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "qd_thermal_blocks.h"

// packed: lower triangle, row-major, s (s + 1) / 2 doubles.  Outputs: pop[s], lam[s] (units of the input, the order of the
// columns of V), V[s][s] row-major (column k: eigenvector k), ztail, label[s] (the lowest state of the component of state i),
// Aout[s][s] (the block after the solve, on the solver's scale; may be null).  Returns the number of sweeps, or -1 for a size
// outside 1..32 or a kT that is not finite and positive, -2 without memory.
extern "C" int qdtb_thermal(int s, const double* packed, double kT, double* pop, double* lam, double* V, double* ztail,
                            int32_t* label, double* Aout) {
    if (s < 1 || s > QD_LV_MAX || !(kT > 0.0) || !(kT < INFINITY)) return -1;
    QdThermalBlocksWs* W = (QdThermalBlocksWs*)malloc(sizeof(QdThermalBlocksWs));
    if (!W) return -2;
    qd_levels_load_packed(W->T.B, packed, s);
    const int sweeps = qd_thermal_blocks_solve(*W, s, kT);
    for (int i = 0; i < s; ++i) {
        pop[i] = W->T.pop[i]; lam[i] = W->T.lam[i];
        label[i] = __builtin_ctz(W->ma[i]);
        for (int j = 0; j < s; ++j) {
            V[i * s + j] = W->T.V[i * QD_LV_LD + j];
            if (Aout) Aout[i * s + j] = W->T.B.A[i * QD_LV_LD + j];
        }
    }
    *ztail = W->T.ztail;
    free(W);
    return sweeps;
}

extern "C" int qdtb_sweep_cap() { return QD_TH_SWEEPS; }
extern "C" int qdtb_ws_bytes() { return (int)sizeof(QdThermalBlocksWs); }

// The record path of qd_k_thermal_grid for one point: the record is put together from its fields (idx[32], fl[N], tc[N-1],
// E[32], nvalid), nv = min(nvalid, kept).  Outputs: pop[32] (zero from nv on), occ[N], var[N], ztail.  Returns nv, or -1 for a
// bad argument.
template <int N>
static int record(const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept, double kT,
                  double* pop, double* occ, double* var, double* ztail) {
    QdPixelRec* rec = (QdPixelRec*)calloc(1, sizeof(QdPixelRec));
    QdThermalBlocksWs* W = (QdThermalBlocksWs*)malloc(sizeof(QdThermalBlocksWs));
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
        qd_levels_record<N>(W->T.B, rec, nv);
        qd_thermal_blocks_solve(*W, nv, kT);
        qd_thermal_moments<N>(W->T, rec, nv);
        for (int m = 0; m < nv; ++m) pop[m] = W->T.pop[m];
        for (int i = 0; i < N; ++i) { occ[i] = W->T.occ[i]; var[i] = W->T.var[i]; }
        *ztail = W->T.ztail;
    }
    free(W); free(rec);
    return nv;
}

extern "C" int qdtb_record(int N, const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept,
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
