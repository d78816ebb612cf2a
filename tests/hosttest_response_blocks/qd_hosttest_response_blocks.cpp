// CPU driver of csrc/qd_response_blocks.h: the epilogue a wavefront runs behind the per-component thermal core, with the lanes as a loop.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "qd_response_blocks.h"

// One block, npert perturbations: the arguments and results of qdhr_response (tests/hosttest_response), the sparse tables
// respecting the components of the block.  Returns the sweeps of the thermal core, -1 for a bad argument, -2 without memory.
extern "C" int qdhrb_response(int s, const double* packed, double kT, int npert, const int32_t* kind, const double* x,
                              const uint8_t* nb, int poison, double* dP, double* pop) {
    if (s < 1 || s > QD_LV_MAX || !(kT > 0.0) || !(kT < INFINITY) || npert < 0) return -1;
    for (int p = 0; p < npert; ++p)
        if (kind[p] == 1)
            for (int m = 0; m < 2 * s; ++m)
                if (nb[(size_t)p * 64 + m] != QD_RS_NONE && nb[(size_t)p * 64 + m] >= s) return -1;
    QdResponseBlocksWs* W = (QdResponseBlocksWs*)malloc(sizeof(QdResponseBlocksWs));
    if (!W) return -2;
    if (poison) memset(W, 0xFF, sizeof(*W));
    QdThermalWs& T = W->TB.T;
    qd_levels_load_packed(T.B, packed, s);
    qd_response_blocks_scale(*W, s);
    const int sweeps = qd_thermal_blocks_solve(W->TB, s, kT);
    for (int m = 0; m < QD_LV_MAX; ++m) pop[m] = m < s ? T.pop[m] : 0.0;
    qd_response_blocks_begin(*W, s, kT);
    for (int p = 0; p < npert; ++p) {
        const double* xp = x + (size_t)p * 64;
        for (int m = 0; m < s; ++m) {
            T.B.x[m] = xp[m];
            if (kind[p] == 1) {
                T.B.x[32 + m] = xp[32 + m];
                W->nb[m][0] = nb[(size_t)p * 64 + 2 * m]; W->nb[m][1] = nb[(size_t)p * 64 + 2 * m + 1];
            }
        }
        if (kind[p] == 1) qd_response_blocks_apply<true>(*W, s, kT); else qd_response_blocks_apply<false>(*W, s, kT);
        for (int m = 0; m < QD_LV_MAX; ++m) dP[(size_t)p * QD_LV_MAX + m] = m < s ? W->dP[m] : 0.0;
    }
    free(W);
    return sweeps;
}

extern "C" int qdhrb_ws_bytes() { return (int)sizeof(QdResponseBlocksWs); }
extern "C" int qdhrb_thermal_blocks_ws_bytes() { return (int)sizeof(QdThermalBlocksWs); }
extern "C" double qdhrb_sensor_slope(double c0, double a, double gamma) { return qd_sensor_slope(c0, a, gamma); }

// u[2N] = the physical direction of an axis scalar (qd_grid_axis_direction) from the state block st and the direction dir[2N]
extern "C" int qdhrb_axis_direction(int N, const double* st, int frame, const double* dir, double* u) {
    switch (N) {
#define C(k) case k: for (int i = 0; i < 2 * k; ++i) u[i] = qd_grid_axis_direction<k>(st, frame, dir, i); return 0;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return -1;
}

// The record path of qd_k_thermal_grid_response<N, QdResponseBlocksWs> for one point: the arguments and results of qdhr_record.
template <int N>
static int record(const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept, double kT,
                  const double* par, int poison, double* chi, double* jac, double* dc0, double* occ, double* var) {
    constexpr int NB = N - 1, V = 2 * N, X = 2 * N - 1;
    QdPixelRec* rec = (QdPixelRec*)calloc(1, sizeof(QdPixelRec));
    QdResponseBlocksWs* W = (QdResponseBlocksWs*)malloc(sizeof(QdResponseBlocksWs));
    if (!rec || !W) { free(rec); free(W); return -1; }
    if (poison) memset(W, 0xFF, sizeof(*W));
    QdThermalWs& T = W->TB.T;
    for (int m = 0; m < QD_K; ++m) { rec->idx[m] = idx[m]; rec->E[m] = E[m]; }
    for (int i = 0; i < N; ++i) rec->fl[i] = fl[i];
    for (int b = 0; b < N - 1; ++b) rec->tc[b] = tc[b];
    rec->nvalid = nvalid;
    int nv = nvalid < kept ? nvalid : kept;
    nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
    for (int i = 0; i < N; ++i) occ[i] = var[i] = 0.0;
    if (nv > 0) {
        qd_levels_record<N>(T.B, rec, nv);
        qd_response_blocks_scale(*W, nv);
        qd_thermal_blocks_solve(W->TB, nv, kT);
        qd_thermal_moments<N>(T, rec, nv);
        for (int i = 0; i < N; ++i) { occ[i] = T.occ[i]; var[i] = T.var[i]; }
    }
    qd_response_blocks_solve<N>(*W, rec, nv, kT, par);
    for (int i = 0; i < N; ++i) {
        for (int c = 0; c < X; ++c) chi[i * X + c] = c < N ? T.B.lo[i * N + c] : T.B.hi[i * NB + c - N];
        for (int c = 0; c < V; ++c) jac[i * V + c] = c < N ? T.B.v[i * N + c] : T.B.w[i * N + c - N];
    }
    for (int c = 0; c < V; ++c) dc0[c] = T.c[c];
    free(W); free(rec);
    return nv;
}

extern "C" int qdhrb_record(int N, const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, int nvalid, int kept,
                            double kT, const double* par, int poison, double* chi, double* jac, double* dc0, double* occ, double* var) {
    if (kept < 1 || kept > QD_K || !(kT > 0.0) || !(kT < INFINITY)) return -1;
    switch (N) {
#define C(k) case k: return record<k>(idx, fl, tc, E, nvalid, kept, kT, par, poison, chi, jac, dc0, occ, var);
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    return -1;
}
