// CPU driver of csrc/qd_response.h: the epilogue a wavefront runs behind the thermal core, with the lanes as a loop.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "qd_response.h"

// One block, npert perturbations.  packed: lower triangle, row-major.  kind[p]: 0 a diagonal X, x[p][m] its entries; 1 a sparse
// symmetric X with at most two partners per state, nb[p][m][0..1] the partners (255: none) and x[p][m], x[p][32 + m] their
// coefficients.  poison: the workspace starts as all-ones bits (NaN doubles).  Outputs: dP[npert][32] (zero from s on),
// pop[32].  Returns the sweeps of the thermal core, -1 for a bad argument, -2 without memory.
extern "C" int qdhr_response(int s, const double* packed, double kT, int npert, const int32_t* kind, const double* x,
                             const uint8_t* nb, int poison, double* dP, double* pop) {
    if (s < 1 || s > QD_LV_MAX || !(kT > 0.0) || !(kT < INFINITY) || npert < 0) return -1;
    for (int p = 0; p < npert; ++p)
        if (kind[p] == 1)
            for (int m = 0; m < 2 * s; ++m)
                if (nb[(size_t)p * 64 + m] != QD_RS_NONE && nb[(size_t)p * 64 + m] >= s) return -1;
    QdResponseWs* W = (QdResponseWs*)malloc(sizeof(QdResponseWs));
    if (!W) return -2;
    if (poison) memset(W, 0xFF, sizeof(*W));
    qd_levels_load_packed(W->T.B, packed, s);
    qd_response_scale(*W, s);
    const int sweeps = qd_thermal_solve(W->T, s, kT);
    for (int m = 0; m < QD_LV_MAX; ++m) pop[m] = m < s ? W->T.pop[m] : 0.0;
    qd_response_begin(*W, s, kT);
    for (int p = 0; p < npert; ++p) {
        const double* xp = x + (size_t)p * 64;
        for (int m = 0; m < s; ++m) {
            W->T.B.x[m] = xp[m];
            if (kind[p] == 1) {
                W->T.B.x[32 + m] = xp[32 + m];
                W->nb[m][0] = nb[(size_t)p * 64 + 2 * m]; W->nb[m][1] = nb[(size_t)p * 64 + 2 * m + 1];
            }
        }
        if (kind[p] == 1) qd_response_apply<true>(*W, s, kT); else qd_response_apply<false>(*W, s, kT);
        for (int m = 0; m < QD_LV_MAX; ++m) dP[(size_t)p * QD_LV_MAX + m] = m < s ? W->dP[m] : 0.0;
    }
    free(W);
    return sweeps;
}

extern "C" int qdhr_ws_bytes() { return (int)sizeof(QdResponseWs); }
extern "C" int qdhr_thermal_ws_bytes() { return (int)sizeof(QdThermalWs); }

// The record path of qd_k_thermal_response for one point: the record from its fields as in hosttest_thermal, par the parameter
// block.  Outputs: chi[N][2N-1], jac[N][2N], dc0[2N], occ[N], var[N].  Returns nv, or -1 for a bad argument.
template <int N>
static int record(const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept, double kT,
                  const double* par, int poison, double* chi, double* jac, double* dc0, double* occ, double* var) {
    constexpr int NB = N - 1, V = 2 * N, X = 2 * N - 1;
    QdPixelRec* rec = (QdPixelRec*)calloc(1, sizeof(QdPixelRec));
    QdResponseWs* W = (QdResponseWs*)malloc(sizeof(QdResponseWs));
    if (!rec || !W) { free(rec); free(W); return -1; }
    if (poison) memset(W, 0xFF, sizeof(*W));
    for (int m = 0; m < QD_K; ++m) { rec->idx[m] = idx[m]; rec->E[m] = E[m]; }
    for (int i = 0; i < N; ++i) rec->fl[i] = fl[i];
    for (int b = 0; b < N - 1; ++b) rec->tc[b] = tc[b];
    rec->nvalid = nvalid;
    int nv = nvalid < kept ? nvalid : kept;
    nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
    for (int i = 0; i < N; ++i) occ[i] = var[i] = 0.0;
    if (nv > 0) {
        qd_levels_record<N>(W->T.B, rec, nv);
        qd_response_scale(*W, nv);
        qd_thermal_solve(W->T, nv, kT);
        qd_thermal_moments<N>(W->T, rec, nv);
        for (int i = 0; i < N; ++i) { occ[i] = W->T.occ[i]; var[i] = W->T.var[i]; }
    }
    qd_response_solve<N>(*W, rec, nv, kT, par);
    for (int i = 0; i < N; ++i) {
        for (int c = 0; c < X; ++c) chi[i * X + c] = c < N ? W->T.B.lo[i * N + c] : W->T.B.hi[i * NB + c - N];
        for (int c = 0; c < V; ++c) jac[i * V + c] = c < N ? W->T.B.v[i * N + c] : W->T.B.w[i * N + c - N];
    }
    for (int c = 0; c < V; ++c) dc0[c] = W->T.c[c];
    free(W); free(rec);
    return nv;
}

extern "C" int qdhr_record(int N, const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept,
                           double kT, const double* par, int poison, double* chi, double* jac, double* dc0, double* occ, double* var) {
    if (kept < 1 || kept > QD_K || !(kT > 0.0) || !(kT < INFINITY)) return -1;
    switch (N) {
        case 2: return record<2>(idx, fl, tc, E, nvalid, kept, kT, par, poison, chi, jac, dc0, occ, var);
        case 3: return record<3>(idx, fl, tc, E, nvalid, kept, kT, par, poison, chi, jac, dc0, occ, var);
        case 4: return record<4>(idx, fl, tc, E, nvalid, kept, kT, par, poison, chi, jac, dc0, occ, var);
        case 5: return record<5>(idx, fl, tc, E, nvalid, kept, kT, par, poison, chi, jac, dc0, occ, var);
        case 6: return record<6>(idx, fl, tc, E, nvalid, kept, kT, par, poison, chi, jac, dc0, occ, var);
        case 7: return record<7>(idx, fl, tc, E, nvalid, kept, kT, par, poison, chi, jac, dc0, occ, var);
        case 8: return record<8>(idx, fl, tc, E, nvalid, kept, kT, par, poison, chi, jac, dc0, occ, var);
    }
    return -1;
}
