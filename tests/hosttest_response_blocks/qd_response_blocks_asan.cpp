// Stand-alone sanitizer run of the per-component charge-response epilogue (csrc/qd_response_blocks.h): random symmetric blocks of
// the sizes 1, 2, 3, 7, 16, 31, 32 at three temperatures, each as it is and cut into interleaved components (state i in component
// i mod g, so that members are never contiguous), with on-site perturbations and a sparse one that respects the partition, and
// the record path with the chain rule on random records of 2..8 dots -- every run from a workspace filled with NaN bits, with the
// workspace, the packed block, the record and the parameter block each alone in a heap block of exactly its size, so a read or
// write past any of them is an AddressSanitizer report, and a signed overflow or a bad shift a UBSan one.  Checks what needs no
// reference: everything is finite, dP of every perturbation sums to zero (the populations sum to one whatever the Hamiltonian),
// one state gives zeros exactly, and a pair with tc == 0 an exact zero column.  Built with -fsanitize=address,undefined; exit
// status 0 and the line "response blocks asan ok" mean a clean run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "qd_response_blocks.h"

static double unit(uint64_t& s) {                      // splitmix64 -> (-1, 1)
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 31;
    return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

static int blocks(uint64_t seed) {
    static const int sizes[] = {1, 2, 3, 7, 16, 31, 32};
    int bad = 0;
    for (int s : sizes)
        for (int t = 0; t < 3; ++t)
            for (int g = 1; g <= 11; g += (g == 1 ? 1 : 3)) {          // g = 1, 2, 5, 8, 11 interleaved components
                const int ne = s * (s + 1) / 2;
                const double kT = t == 0 ? 1e-3 : (t == 1 ? 0.1 : 50.0);
                double* A = (double*)malloc(sizeof(double) * ne);
                QdResponseBlocksWs* W = (QdResponseBlocksWs*)malloc(sizeof(QdResponseBlocksWs));
                memset(W, 0xFF, sizeof(*W));
                QdThermalWs& T = W->TB.T;
                for (int i = 0; i < s; ++i)
                    for (int j = 0; j <= i; ++j) {
                        double a = (i == j) ? unit(seed) : ((i + j + t) % 3 ? 0.3 * unit(seed) : 0.0);
                        if (i != j && (i % g) != (j % g)) a = 0.0;
                        A[i * (i + 1) / 2 + j] = a;
                    }
                qd_levels_load_packed(T.B, A, s);
                qd_response_blocks_scale(*W, s);
                if (!(qd_thermal_blocks_solve(W->TB, s, kT) < QD_TH_SWEEPS)) ++bad;
                qd_response_blocks_begin(*W, s, kT);
                for (int pert = 0; pert < 3; ++pert) {
                    for (int m = 0; m < s; ++m) {
                        T.B.x[m] = pert < 2 ? (double)((m * 7 + pert) % 4) : 0.0;
                        T.B.x[32 + m] = 0.0;
                        W->nb[m][0] = W->nb[m][1] = QD_RS_NONE;
                    }
                    if (pert == 2)                                      // partners m <-> m + g: inside the components, a linked pair only
                        for (int m = 0; m + g < s; m += 2 * g)
                            if (A[(m + g) * (m + g + 1) / 2 + m] != 0.0) {
                                W->nb[m][1] = (unsigned char)(m + g); W->nb[m + g][0] = (unsigned char)m;
                                T.B.x[32 + m] = -0.4; T.B.x[m + g] = -0.4;
                            }
                    if (pert == 2) qd_response_blocks_apply<true>(*W, s, kT); else qd_response_blocks_apply<false>(*W, s, kT);
                    double sum = 0.0, mag = 0.0;
                    for (int m = 0; m < s; ++m) {
                        if (!isfinite(W->dP[m])) ++bad;
                        sum += W->dP[m]; mag += fabs(W->dP[m]);
                    }
                    if (s == 1 && W->dP[0] != 0.0) ++bad;
                    if (!(fabs(sum) <= 1e-9 * (mag + 1.0 / kT))) { ++bad; fprintf(stderr, "response blocks asan: s=%d g=%d sum %g\n", s, g, sum); }
                }
                free(W); free(A);
            }
    return bad;
}

template <int N>
static int records(int points, uint64_t seed) {
    constexpr int NB = N - 1;
    const QdLayout L = qd_layout(N);
    int bad = 0;
    for (int p = 0; p < points; ++p) {
        QdPixelRec* rec = (QdPixelRec*)malloc(sizeof(QdPixelRec));
        QdResponseBlocksWs* W = (QdResponseBlocksWs*)malloc(sizeof(QdResponseBlocksWs));
        double* par = (double*)malloc(sizeof(double) * L.size);
        memset(rec, 0, sizeof(*rec));
        memset(W, 0xFF, sizeof(*W));
        QdThermalWs& T = W->TB.T;
        for (int i = 0; i < L.size; ++i) par[i] = 0.1 * unit(seed);
        const int nv = (p % 9 == 0) ? 0 : 1 + (int)((unit(seed) + 1.0) * 15.99);
        const unsigned span = 1u << (2 * N);
        unsigned c = (unsigned)((unit(seed) + 1.0) * 0.5 * span) % span;
        const unsigned stride = (p % 2) ? 1u : 3u;
        for (int m = 0; m < nv; ++m) { rec->idx[m] = (uint16_t)c; c = (c + stride) % span; rec->E[m] = 50.0 + unit(seed); }
        for (int m = nv > 0 ? nv : 1; m < QD_K; ++m) rec->E[m] = rec->E[m - 1];
        for (int i = 0; i < N; ++i) rec->fl[i] = (p % 4 == 0) ? 1 : 1 + (int)((unit(seed) + 1.0) * 2.0);
        for (int b = 0; b < NB; ++b) rec->tc[b] = (p % 7 == 0 && b == 0) ? 0.0 : 0.05 * (unit(seed) + 1.0);
        rec->nvalid = nv;
        const double kT = p % 3 == 0 ? 1e-3 : 0.2;
        if (nv > 0) {
            qd_levels_record<N>(T.B, rec, nv);
            qd_response_blocks_scale(*W, nv);
            qd_thermal_blocks_solve(W->TB, nv, kT);
            qd_thermal_moments<N>(T, rec, nv);
        }
        qd_response_blocks_solve<N>(*W, rec, nv, kT, par);
        for (int i = 0; i < N; ++i) {
            for (int k = 0; k < N; ++k) {
                if (!isfinite(T.B.lo[i * N + k])) ++bad;
                if (nv <= 1 && T.B.lo[i * N + k] != 0.0) ++bad;
            }
            for (int d = 0; d < NB; ++d) {
                if (!isfinite(T.B.hi[i * NB + d])) ++bad;
                if ((nv <= 1 || rec->tc[d] == 0.0) && T.B.hi[i * NB + d] != 0.0) ++bad;
            }
            for (int j = 0; j < N; ++j)
                if (!isfinite(T.B.v[i * N + j]) || !isfinite(T.B.w[i * N + j])) ++bad;
        }
        for (int j = 0; j < 2 * N; ++j)
            if (!isfinite(T.c[j])) ++bad;
        if (!isfinite(qd_sensor_slope(T.c[0], par[L.cdd_inv], 0.3))) ++bad;
        double u[2 * N], dir[2 * N];
        for (int j = 0; j < 2 * N; ++j) dir[j] = unit(seed);
        double* st = (double*)malloc(sizeof(double) * L.s_size);
        for (int i = 0; i < L.s_size; ++i) st[i] = unit(seed);
        for (int j = 0; j < 2 * N; ++j) { u[j] = qd_grid_axis_direction<N>(st, p % 2 ? QD_SCAN_PHYSICAL : QD_SCAN_VIRTUAL, dir, j); if (!isfinite(u[j])) ++bad; }
        free(st); free(par); free(W); free(rec);
    }
    if (bad) fprintf(stderr, "response blocks asan: records N=%d: %d violations\n", N, bad);
    return bad;
}

int main() {
    int bad = 0;
    uint64_t seed = 2031;
    bad += blocks(seed++);
    bad += records<2>(60, seed++); bad += records<3>(60, seed++); bad += records<4>(60, seed++); bad += records<5>(40, seed++);
    bad += records<6>(40, seed++); bad += records<7>(40, seed++); bad += records<8>(60, seed++);
    if (bad) return 1;
    printf("response blocks asan ok\n");
    return 0;
}
