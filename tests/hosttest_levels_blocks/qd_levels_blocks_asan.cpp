// Stand-alone sanitizer run of the per-component energy-level core (csrc/qd_levels_blocks.h): block-diagonal matrices of every
// size 1..32 at every L in 1..8, their states dealt over 1..6 components by a stride so that members are scattered, and the
// record path on random records of 2..8 dots, with the workspace, the packed block and the record each alone in a heap block of
// exactly its size, so a read or write past any of them is an AddressSanitizer report, and a signed overflow or a bad shift a
// UBSan one.  The workspace is filled with all-ones bits before every solve.  Checks what needs no reference: the levels are
// finite, increasing, inside the Gershgorin interval of the block, and for s <= L they sum to the trace.  Built with
// -fsanitize=address,undefined; exit status 0 and the line "levels blocks asan ok" mean a clean run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "qd_levels_blocks.h"

static double unit(uint64_t& s) {                      // splitmix64 -> (-1, 1)
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 31;
    return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

static int check(const QdLevelsWs* W, int s, int L, double glo, double ghi, double trace, const char* what) {
    int bad = 0;
    const int Le = L < s ? L : s;
    const double tol = 1e-12 * fmax(fabs(glo), fabs(ghi));
    double sum = 0.0;
    for (int k = 0; k < Le; ++k) {
        const double x = W->lev[k];
        if (!(x >= glo - tol && x <= ghi + tol)) ++bad;
        if (k > 0 && !(W->lev[k - 1] <= x)) ++bad;
        sum += x;
    }
    if (s <= L && !(fabs(sum - trace) <= 64.0 * tol)) ++bad;
    if (bad) fprintf(stderr, "levels blocks asan: %s s=%d L=%d: %d violations\n", what, s, L, bad);
    return bad;
}

static void gershgorin(const QdLevelsWs* W, int s, double& glo, double& ghi, double& trace) {
    glo = INFINITY; ghi = -INFINITY; trace = 0.0;
    for (int i = 0; i < s; ++i) {
        double rad = 0.0;
        for (int j = 0; j < s; ++j) if (j != i) rad += fabs(j < i ? W->A[i * QD_LV_LD + j] : W->A[j * QD_LV_LD + i]);
        const double d = W->A[i * QD_LV_LD + i];
        glo = fmin(glo, d - rad); ghi = fmax(ghi, d + rad); trace += d;
    }
}

static int blocks(uint64_t seed) {
    int bad = 0;
    for (int s = 1; s <= QD_LV_MAX; ++s)
        for (int L = 1; L <= QD_LEVELS_MAX; ++L) {
            const int ne = s * (s + 1) / 2;
            double* A = (double*)malloc(sizeof(double) * ne);
            QdLevelsBlocksWs* W = (QdLevelsBlocksWs*)malloc(sizeof(QdLevelsBlocksWs));
            memset(W, 0xFF, sizeof(*W));
            const int ncomp = 1 + (s + L) % 6;                 // state i belongs to component i % ncomp
            const double off = (s % 3 == 0) ? 1e4 : 0.0, cpl = (s % 5 == 0) ? 1e6 : 0.3;
            for (int i = 0; i < s; ++i)
                for (int j = 0; j <= i; ++j)
                    A[i * (i + 1) / 2 + j] = (i == j) ? off + unit(seed) : ((i - j) % ncomp == 0 ? cpl * unit(seed) : 0.0);
            qd_levels_load_packed(W->L, A, s);
            double glo, ghi, trace;
            gershgorin(&W->L, s, glo, ghi, trace);
            qd_levels_blocks_solve(*W, s, L);
            bad += check(&W->L, s, L, glo, ghi, trace, "block");
            free(W); free(A);
        }
    return bad;
}

template <int N>
static int records(int points, uint64_t seed) {
    int bad = 0;
    for (int p = 0; p < points; ++p) {
        QdPixelRec* rec = (QdPixelRec*)malloc(sizeof(QdPixelRec));
        QdLevelsBlocksWs* W = (QdLevelsBlocksWs*)malloc(sizeof(QdLevelsBlocksWs));
        memset(rec, 0, sizeof(*rec));
        memset(W, 0xFF, sizeof(*W));
        const int nv = 1 + (int)((unit(seed) + 1.0) * 15.99);
        const unsigned span = 1u << (2 * N);
        unsigned c = (unsigned)((unit(seed) + 1.0) * 0.5 * span) % span;
        const unsigned stride = (p % 2) ? 1u : 3u;
        for (int m = 0; m < nv; ++m) { rec->idx[m] = (uint16_t)c; c = (c + stride) % span; rec->E[m] = 50.0 + unit(seed); }
        for (int m = nv; m < QD_K; ++m) rec->E[m] = rec->E[nv - 1];
        for (int i = 0; i < N; ++i) rec->fl[i] = (p % 4 == 0) ? 0 : 1 + (int)((unit(seed) + 1.0) * 2.0);
        for (int b = 0; b < N - 1; ++b) rec->tc[b] = (p % 7 == 0 && b == 0) ? 0.0 : 0.05 * (unit(seed) + 1.0);
        rec->nvalid = nv;
        const double hn = qd_levels_record<N>(W->L, rec, nv);
        double glo, ghi, trace;
        gershgorin(&W->L, nv, glo, ghi, trace);
        if (!(hn >= fmax(fabs(glo), fabs(ghi)) * (1.0 - 1e-14))) { ++bad; fprintf(stderr, "levels blocks asan: hnorm\n"); }
        const int L = 1 + p % QD_LEVELS_MAX;
        qd_levels_blocks_solve(*W, nv, L);
        bad += check(&W->L, nv, L, glo, ghi, trace, "record");
        free(W); free(rec);
    }
    return bad;
}

int main() {
    int bad = 0;
    uint64_t seed = 2029;
    bad += blocks(seed++);
    bad += records<2>(60, seed++); bad += records<3>(60, seed++); bad += records<4>(60, seed++); bad += records<5>(40, seed++);
    bad += records<6>(40, seed++); bad += records<7>(40, seed++); bad += records<8>(60, seed++);
    if (bad) return 1;
    printf("levels blocks asan ok\n");
    return 0;
}
