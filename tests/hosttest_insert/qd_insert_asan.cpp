// Stand-alone sanitizer run of tests/hosttest_insert (make qd_insert_asan; -fsanitize=address,undefined): drives both entry
// points of qd_hosttest_insert.cpp, both forms of the insert, over pseudo-random streams and devices, and compares them.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "qd_common.h"

extern "C" {
int qdhi_row_words();
int qdhi_stream(int KC, int packed, long n, const double* E, const uint32_t* idx, uint64_t* rows);
int qdhi_front(int N, int KC, int packed, const double* par, const double* st, int ch, int R, int sort, double* e_out,
               uint16_t* id_out, int32_t* nvalid, int32_t* fl_out, unsigned long long* stats);
}

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static double urand() { rs = rs * 6364136223846793005ull + 1442695040888963407ull; return (double)(rs >> 11) / 9007199254740992.0; }

int main() {
    int bad = 0;
    const int W = qdhi_row_words();
    // streams.  kind 0: random; 1: few distinct energies (exact ties, at the maximum and inside a group); 2: strictly
    // descending (every insert replaces); 3: strictly ascending (none does); 4: inf / NaN / -inf mixed in; 5: fewer than KC
    for (int KC = 8; KC <= 32; KC *= 2)
        for (int kind = 0; kind < 6; ++kind)
            for (int rep = 0; rep < 20; ++rep) {
                const long n = kind == 5 ? (long)(urand() * KC) : 40 + (long)(urand() * 400);
                std::vector<double> E(n + 1); std::vector<uint32_t> id(n + 1);
                std::vector<uint32_t> perm(65536);
                for (uint32_t i = 0; i < 65536; ++i) perm[i] = i;
                for (long t = 0; t < n; ++t) {                                // distinct ids, as the leaves of one tree have
                    const uint32_t j = (uint32_t)t + (uint32_t)(urand() * (65536 - t));
                    const uint32_t x = perm[t]; perm[t] = perm[j]; perm[j] = x;
                    id[t] = perm[t];
                    E[t] = kind == 1 ? floor(4.0 * urand()) : kind == 2 ? (double)(n - t) : kind == 3 ? (double)t : 10.0 * urand() - 5.0;
                    if (kind == 4 && urand() < 0.2) { const double u = urand(); E[t] = u < 0.4 ? INFINITY : u < 0.8 ? NAN : -INFINITY; }
                }
                std::vector<uint64_t> r0((size_t)(n + 1) * W, 1), r1((size_t)(n + 1) * W, 2);
                bad |= qdhi_stream(KC, 0, n, E.data(), id.data(), r0.data());
                bad |= qdhi_stream(KC, 1, n, E.data(), id.data(), r1.data());
                bad |= n > 0 && memcmp(r0.data(), r1.data(), (size_t)n * W * sizeof(uint64_t)) != 0;
                bad |= n > 0 && r0[0] == ~0ull;                              // (a write outside the lane's slots)
            }
    // whole searches on synthetic devices: A = cdd_inv symmetric and diagonally dominant, U its upper factor (A = U U^T),
    // identity gate matrix, voltages spread over a few electrons, some dots depleted
    for (int N = 2; N <= 8; ++N) {
        const QdLayout L = qd_layout(N);
        const int G = N + 1, V = 2 * N, R = N >= 7 ? 3 : 5;
        for (int rep = 0; rep < 3; ++rep) {
            std::vector<double> par(L.size, 0.0), st(L.s_size, 0.0);
            double* A = &par[L.cdd_inv];
            for (int i = 0; i < G; ++i) for (int j = 0; j <= i; ++j) A[i * G + j] = A[j * G + i] = (i == j ? 1.0 : 0.15 * urand());
            double* U = &par[L.ufac];
            for (int k = N - 1; k >= 0; --k) {
                double d = A[k * G + k];
                for (int m = k + 1; m < N; ++m) d -= U[k * N + m] * U[k * N + m];
                U[k * N + k] = sqrt(d); par[L.uinv + k] = 1.0 / U[k * N + k];
                for (int i = 0; i < k; ++i) {
                    double s = A[i * G + k];
                    for (int m = k + 1; m < N; ++m) s -= U[i * N + m] * U[k * N + m];
                    U[i * N + k] = s / U[k * N + k];
                }
            }
            for (int i = 0; i < G; ++i) par[L.cgd + i * V + i] = 1.0;
            par[L.scal + 0] = 1e-3; par[L.scal + 1] = 0.1; par[L.scal + 2] = 1.5; par[L.scal + 3] = -1.0;
            for (int i = 0; i < G; ++i) st[L.s_vgm + i * G + i] = 1.0;
            for (int i = 0; i < N; ++i) st[L.s_gate_v + i] = 5.0 * urand() - 1.5;
            for (int KC = 8; KC <= 32; KC *= 2)
                for (int sort = 0; sort < 2; ++sort) {
                    const int P = R * R;
                    std::vector<double> e[2]; std::vector<uint16_t> id[2]; std::vector<int32_t> nv[2], fl[2];
                    unsigned long long stats[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
                    for (int f = 0; f < 2; ++f) {
                        e[f].assign((size_t)P * KC, 0.0); id[f].assign((size_t)P * KC, 0); nv[f].assign(P, 0); fl[f].assign((size_t)P * N, 0);
                        bad |= qdhi_front(N, KC, f, par.data(), st.data(), 0, R, sort, e[f].data(), id[f].data(), nv[f].data(), fl[f].data(), stats[f]);
                    }
                    bad |= memcmp(e[0].data(), e[1].data(), e[0].size() * sizeof(double)) != 0;
                    bad |= id[0] != id[1] || nv[0] != nv[1] || fl[0] != fl[1] || memcmp(stats[0], stats[1], sizeof stats[0]) != 0;
                    bad |= stats[0][2] == 0;                                 // (the searches inserted)
                }
        }
    }
    printf(bad ? "qd_insert_asan: MISMATCH\n" : "qd_insert_asan: ok\n");
    return bad ? 1 : 0;
}
