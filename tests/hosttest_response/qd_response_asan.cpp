// Stand-alone sanitizer run of the charge-response epilogue (csrc/qd_response.h) behind the thermal core: random symmetric blocks
// of the sizes 1, 2, 3, 7, 16, 31, 32 with a diagonal and a sparse perturbation each, and the record path with the chain rule on
// random records of 2..8 dots, with the workspace, the packed block, the record and the parameter block each alone in a heap
// block of exactly its size and the workspace filled with NaN bits first, so a read or write past any of them is an
// AddressSanitizer report, a signed overflow or a bad shift a UBSan one, and a read of something the code did not write shows as
// a NaN.  Checks what needs no reference: every result is finite, dP sums to zero (the populations sum to one whatever the
// Hamiltonian), one state gives zeros exactly, the on-site block of chi is symmetric and has no positive diagonal entry, a pair
// without coupling gives an exact zero column.  Built with -fsanitize=address,undefined; exit status 0 and the line
// "response asan ok" mean a clean run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "qd_response.h"

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
        for (int t = 0; t < 3; ++t) {
            const int ne = s * (s + 1) / 2;
            double* A = (double*)malloc(sizeof(double) * ne);
            QdResponseWs* W = (QdResponseWs*)malloc(sizeof(QdResponseWs));
            memset(W, 0xFF, sizeof(*W));
            for (int i = 0; i < s; ++i)
                for (int j = 0; j <= i; ++j) A[i * (i + 1) / 2 + j] = (i == j) ? 50.0 + unit(seed) : ((i + j + t) % 3 ? 0.3 * unit(seed) : 0.0);
            const double kT = t == 0 ? 1e-3 : (t == 1 ? 0.1 : 50.0);
            qd_levels_load_packed(W->T.B, A, s);
            qd_response_scale(*W, s);
            qd_thermal_solve(W->T, s, kT);
            qd_response_begin(*W, s, kT);
            for (int hop = 0; hop < 2; ++hop) {
                for (int m = 0; m < s; ++m) {
                    if (!hop) { W->T.B.x[m] = (double)(m % 4); continue; }
                    W->nb[m][0] = (unsigned char)(m + 1 < s ? m + 1 : QD_RS_NONE);
                    W->nb[m][1] = (unsigned char)(m > 0 ? m - 1 : QD_RS_NONE);
                    W->T.B.x[m] = -0.5 - 0.01 * m;
                    W->T.B.x[32 + m] = m > 0 ? -0.5 - 0.01 * (m - 1) : 0.0;
                }
                if (hop) qd_response_apply<true>(*W, s, kT); else qd_response_apply<false>(*W, s, kT);
                double sum = 0.0, big = 0.0;
                for (int m = 0; m < s; ++m) {
                    if (!isfinite(W->dP[m])) ++bad;
                    sum += W->dP[m]; big = fmax(big, fabs(W->dP[m]));
                }
                if (!(fabs(sum) <= 1e-9 * (big + 1.0 / kT))) { ++bad; fprintf(stderr, "response asan: s=%d t=%d hop=%d: sum dP = %g\n", s, t, hop, sum); }
                if (s == 1 && W->dP[0] != 0.0) ++bad;
            }
            free(W); free(A);
        }
    return bad;
}

template <int N>
static int records(int points, uint64_t seed) {
    constexpr int NB = N - 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
    int bad = 0;
    for (int p = 0; p < points; ++p) {
        QdPixelRec* rec = (QdPixelRec*)malloc(sizeof(QdPixelRec));
        QdResponseWs* W = (QdResponseWs*)malloc(sizeof(QdResponseWs));
        double* par = (double*)malloc(sizeof(double) * L.size);
        memset(rec, 0, sizeof(*rec));
        memset(W, 0xFF, sizeof(*W));
        for (int i = 0; i < L.size; ++i) par[i] = 0.2 * unit(seed);
        const int nv = p == 0 ? 1 : 1 + (int)((unit(seed) + 1.0) * 15.99);
        const unsigned span = 1u << (2 * N);
        unsigned c = (unsigned)((unit(seed) + 1.0) * 0.5 * span) % span;
        const unsigned stride = (p % 2) ? 1u : 3u;
        for (int m = 0; m < nv; ++m) { rec->idx[m] = (uint16_t)c; c = (c + stride) % span; rec->E[m] = 50.0 + unit(seed); }
        for (int m = nv; m < QD_K; ++m) rec->E[m] = rec->E[nv - 1];
        for (int i = 0; i < N; ++i) rec->fl[i] = (p % 4 == 0) ? 1 : 1 + (int)((unit(seed) + 1.0) * 2.0);
        for (int b = 0; b < NB; ++b) rec->tc[b] = (p % 3 == 0 && b == 0) ? 0.0 : 0.05 * (unit(seed) + 1.0);
        rec->nvalid = nv;
        const double kT = p % 3 == 0 ? 1e-3 : 0.2;
        qd_levels_record<N>(W->T.B, rec, nv);
        qd_response_scale(*W, nv);
        qd_thermal_solve(W->T, nv, kT);
        qd_thermal_moments<N>(W->T, rec, nv);
        qd_response_solve<N>(*W, rec, nv, kT, par);
        for (int i = 0; i < N; ++i) {
            for (int k = 0; k < N; ++k) {
                const double a = W->T.B.lo[i * N + k], b = W->T.B.lo[k * N + i];
                if (!isfinite(a) || !(fabs(a - b) <= 1e-9 * (fabs(a) + 1.0 / kT))) ++bad;
                if (nv == 1 && a != 0.0) ++bad;
            }
            if (!(W->T.B.lo[i * N + i] <= 1e-9 / kT)) ++bad;
            for (int d = 0; d < NB; ++d) {
                const double a = W->T.B.hi[i * NB + d];
                if (!isfinite(a) || (rec->tc[d] == 0.0 && a != 0.0)) ++bad;
            }
            for (int j = 0; j < N; ++j)
                if (!isfinite(W->T.B.v[i * N + j]) || !isfinite(W->T.B.w[i * N + j])) ++bad;
        }
        for (int j = 0; j < V; ++j) if (!isfinite(W->T.c[j])) ++bad;
        if (bad) { fprintf(stderr, "response asan: record N=%d p=%d nv=%d: %d violations\n", N, p, nv, bad); free(par); free(W); free(rec); return bad; }
        free(par); free(W); free(rec);
    }
    return bad;
}

int main() {
    int bad = 0;
    uint64_t seed = 2031;
    bad += blocks(seed++);
    bad += records<2>(40, seed++); bad += records<3>(40, seed++); bad += records<4>(40, seed++); bad += records<5>(30, seed++);
    bad += records<6>(30, seed++); bad += records<7>(30, seed++); bad += records<8>(40, seed++);
    if (bad) return 1;
    printf("response asan ok\n");
    return 0;
}
