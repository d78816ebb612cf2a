// Stand-alone sanitizer run of the closed regime's front (csrc/qd_closed.h): centre, sector search and record at random
// voltages and total charges, with the kept buffers on the heap at exactly KC entries and the record alone in a heap block, so
// a read or write past either is an AddressSanitizer report, and a signed overflow or a bad shift in the search a UBSan one.
// Checks what needs no reference: the states are non-negative, sum to Q, come in increasing (E, idx) order, and the padding
// follows the rule.  Built with -fsanitize=address,undefined; exit status 0 and the line "closed asan ok" mean a clean run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>
#include "qd_closed.h"

static double unit(uint64_t& s) {                      // splitmix64 -> (-1, 1)
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

template <int N, int KC>
static int walk(int points, uint64_t seed) {
    constexpr int G = N + 1;
    const QdLayout L = qd_layout(N);
    std::vector<double> par((size_t)L.size, 0.0);
    // a diagonally dominant symmetric cdd_inv and its upper factor A = U U^T (reversed Cholesky)
    double A[N][N], U[N][N];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j <= i; ++j) A[i][j] = A[j][i] = (i == j) ? 0.25 + 0.05 * unit(seed) : 0.02 * unit(seed);
    memset(U, 0, sizeof(U));
    for (int j = N - 1; j >= 0; --j) {
        double d = A[j][j];
        for (int k = j + 1; k < N; ++k) d -= U[j][k] * U[j][k];
        U[j][j] = sqrt(d);
        for (int i = 0; i < j; ++i) {
            double s = A[i][j];
            for (int k = j + 1; k < N; ++k) s -= U[i][k] * U[j][k];
            U[i][j] = s / U[j][j];
        }
    }
    for (int i = 0; i < N; ++i) {
        for (int j = 0; j < N; ++j) { par[L.cdd_inv + i * G + j] = A[i][j]; par[L.ufac + i * N + j] = U[i][j]; }
        par[L.uinv + i] = 1.0 / U[i][i];
    }
    int bad = 0;
    for (int p = 0; p < points; ++p) {
        double vd[N];
        for (int i = 0; i < N; ++i) vd[i] = (p % 3 ? 2.0 : -0.5) + 2.5 * unit(seed);
        const int Qs[] = {0, 1, N, 2 * N + 1, 3 + (p % 5), p % 7 == 0 ? QD_CLOSED_QMAX : 2};
        for (int Q : Qs) {
            double* e = (double*)malloc(sizeof(double) * KC);
            uint16_t* id = (uint16_t*)malloc(sizeof(uint16_t) * KC);
            QdPixelRec* rec = (QdPixelRec*)malloc(sizeof(QdPixelRec));
            memset(rec, 0xA5, sizeof(*rec));
            const int nv = qd_closed_record<N, KC>(par.data(), vd, 1.0, Q, e, 1, id, 1, rec);
            if (nv < 1 || nv > KC || rec->nvalid != nv) ++bad;
            for (int k = 0; k < KC; ++k) {
                if (k >= nv) { if (rec->idx[k] != 0 || (nv > 0 && rec->E[k] != rec->E[nv - 1])) ++bad; continue; }
                long sum = 0;
                for (int i = 0; i < N; ++i) {
                    const int c = rec->fl[i] + (int)((rec->idx[k] >> (2 * (N - 1 - i))) & 3) - 1;
                    if (c < 0) ++bad;
                    sum += c;
                }
                if (sum != Q) ++bad;
                if (k > 0 && !(rec->E[k - 1] < rec->E[k] || (rec->E[k - 1] == rec->E[k] && rec->idx[k - 1] < rec->idx[k]))) ++bad;
            }
            free(rec); free(id); free(e);
        }
    }
    if (bad) fprintf(stderr, "closed asan: N=%d KC=%d: %d violations\n", N, KC, bad);
    return bad;
}

int main() {
    int bad = 0;
    uint64_t seed = 2026;
    bad += walk<2, 32>(200, seed++); bad += walk<3, 32>(200, seed++); bad += walk<4, 8>(200, seed++);
    bad += walk<5, 16>(200, seed++); bad += walk<6, 32>(100, seed++); bad += walk<8, 32>(60, seed++); bad += walk<8, 8>(60, seed++);
    if (bad) return 1;
    printf("closed asan ok\n");
    return 0;
}
