// Stand-alone sanitizer run of the per-component thermal core (csrc/qd_thermal_blocks.h): random symmetric blocks of every size
// 1..32 at three temperatures, each once as it is and once cut into interleaved components (state i in component i mod g, so
// that members are never contiguous and odd components meet), and the record path on random records of 2..8 dots, with the
// workspace, the packed block and the record each alone in a heap block of exactly its size, so a read or write past any of them
// is an AddressSanitizer report, and a signed overflow or a bad shift a UBSan one.  Checks what needs no reference: the
// populations are finite, non-negative and sum to 1, the eigenvalues sum to the trace, the columns of V are orthonormal, the
// sweep cap is not reached, ztail is in [0, 1], and the occupations of a record lie between the smallest and the largest
// occupation of its states.  Built with -fsanitize=address,undefined; exit status 0 and the line "thermal blocks asan ok" mean a
// clean run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "qd_thermal_blocks.h"

static double unit(uint64_t& s) {                      // splitmix64 -> (-1, 1)
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 31;
    return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

static int check(const QdThermalBlocksWs* W, int s, int sweeps, double trace, double scale, const char* what) {
    int bad = 0;
    double sum = 0.0, tr = 0.0;
    for (int i = 0; i < s; ++i) {
        const double p = W->T.pop[i];
        if (!(p >= 0.0 && p <= 1.0 + 1e-12)) ++bad;
        sum += p; tr += W->T.lam[i];
    }
    if (!(fabs(sum - 1.0) <= 1e-12)) ++bad;
    if (!(fabs(tr - trace) <= 1e-11 * scale)) ++bad;
    if (!(W->T.ztail >= 0.0 && W->T.ztail <= 1.0)) ++bad;
    if (s > 1 && !(sweeps < QD_TH_SWEEPS)) ++bad;
    if (s > 1)
        for (int a = 0; a < s; ++a)
            for (int b = 0; b <= a; ++b) {
                double d = 0.0;
                for (int i = 0; i < s; ++i) d += W->T.V[i * QD_LV_LD + a] * W->T.V[i * QD_LV_LD + b];
                if (!(fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-13)) ++bad;
            }
    if (bad) fprintf(stderr, "thermal blocks asan: %s s=%d: %d violations\n", what, s, bad);
    return bad;
}

static int blocks(uint64_t seed) {
    int bad = 0;
    for (int s = 1; s <= QD_LV_MAX; ++s)
        for (int t = 0; t < 3; ++t)
            for (int g = 1; g <= 11; g += (g == 1 ? 1 : 3)) {          // g = 1, 2, 5, 8, 11 interleaved components
                const int ne = s * (s + 1) / 2;
                double* A = (double*)malloc(sizeof(double) * ne);
                QdThermalBlocksWs* W = (QdThermalBlocksWs*)malloc(sizeof(QdThermalBlocksWs));
                const double off = (s % 3 == 0) ? 1e4 : 0.0, cpl = (s % 5 == 0) ? 1e6 : 0.3;
                double trace = 0.0, scale = 0.0;
                for (int i = 0; i < s; ++i)
                    for (int j = 0; j <= i; ++j) {
                        double a = (i == j) ? off + unit(seed) : ((i + j + t) % 3 ? cpl * unit(seed) : 0.0);
                        if (i != j && (i % g) != (j % g)) a = 0.0;
                        A[i * (i + 1) / 2 + j] = a;
                        if (i == j) trace += a;
                        scale += fabs(a);
                    }
                qd_levels_load_packed(W->T.B, A, s);
                const int sweeps = qd_thermal_blocks_solve(*W, s, t == 0 ? 1e-3 : (t == 1 ? 0.1 : 50.0));
                bad += check(W, s, sweeps, trace, scale, "block");
                free(W); free(A);
            }
    return bad;
}

template <int N>
static int records(int points, uint64_t seed) {
    int bad = 0;
    for (int p = 0; p < points; ++p) {
        QdPixelRec* rec = (QdPixelRec*)malloc(sizeof(QdPixelRec));
        QdThermalBlocksWs* W = (QdThermalBlocksWs*)malloc(sizeof(QdThermalBlocksWs));
        memset(rec, 0, sizeof(*rec));
        const int nv = 1 + (int)((unit(seed) + 1.0) * 15.99);
        // distinct random states: a random start and an odd stride through the 4^N codes
        const unsigned span = 1u << (2 * N);
        unsigned c = (unsigned)((unit(seed) + 1.0) * 0.5 * span) % span;
        const unsigned stride = (p % 2) ? 1u : 3u;
        for (int m = 0; m < nv; ++m) { rec->idx[m] = (uint16_t)c; c = (c + stride) % span; rec->E[m] = 50.0 + unit(seed); }
        for (int m = nv; m < QD_K; ++m) rec->E[m] = rec->E[nv - 1];
        for (int i = 0; i < N; ++i) rec->fl[i] = (p % 4 == 0) ? 1 : 1 + (int)((unit(seed) + 1.0) * 2.0);
        for (int b = 0; b < N - 1; ++b) rec->tc[b] = (p % 7 == 0 && b == 0) ? 0.0 : 0.05 * (unit(seed) + 1.0);
        rec->nvalid = nv;
        qd_levels_record<N>(W->T.B, rec, nv);
        double trace = 0.0, scale = 0.0;
        for (int i = 0; i < nv; ++i) {
            trace += W->T.B.A[i * QD_LV_LD + i];
            for (int j = 0; j <= i; ++j) scale += fabs(W->T.B.A[i * QD_LV_LD + j]);
        }
        const int sweeps = qd_thermal_blocks_solve(*W, nv, p % 3 == 0 ? 1e-3 : 0.2);
        bad += check(W, nv, sweeps, trace, scale, "record");
        qd_thermal_moments<N>(W->T, rec, nv);
        for (int d = 0; d < N; ++d) {
            double lo = INFINITY, hi = -INFINITY;
            for (int m = 0; m < nv; ++m) {
                const double n = (double)(rec->fl[d] + (int)((rec->idx[m] >> (2 * (N - 1 - d))) & 3u) - 1);
                lo = fmin(lo, n); hi = fmax(hi, n);
            }
            if (!(W->T.occ[d] >= lo - 1e-12 && W->T.occ[d] <= hi + 1e-12 && W->T.var[d] >= 0.0 &&
                  W->T.var[d] <= (hi - lo) * (hi - lo) + 1e-12)) {
                ++bad; fprintf(stderr, "thermal blocks asan: moments of dot %d\n", d);
            }
        }
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
    printf("thermal blocks asan ok\n");
    return 0;
}
