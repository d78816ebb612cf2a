// Stand-alone sanitizer run of tests/hosttest_tile (make qd_tile_asan; -fsanitize=address,undefined): drives every entry
// point of qd_hosttest_tile.cpp over pseudo-random inputs, both forms of each piece, and compares them.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "qd_common.h"

extern "C" {
int qdht_pg(int N, int interleaved, long n, const double* par, long par_stride, const double* v_ext, const double* vd_in,
            double* vd_out, double* ncont, double* isa);
int qdht_fl_packable(int fl);
void qdht_fl_minmax(const int* fl, int* mn, int* mx);
int qdht_select(int KC, int fill, int nS, int nSfront, int scap, const uint32_t* scode, const double* sD, const double* sa,
                const double* sb, double xs, double ys, uint32_t blo, uint32_t bhi, double amb, double* e_out, uint16_t* id_out,
                double* maxE, int* ms, double* eout, int* redo);
}

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static double urand() { rs = rs * 6364136223846793005ull + 1442695040888963407ull; return (double)(rs >> 11) / 9007199254740992.0; }

int main() {
    int bad = 0;
    for (int N = 2; N <= 8; ++N) {
        const QdLayout L = qd_layout(N);
        const int G = N + 1, nblk = 50;
        std::vector<double> par((size_t)nblk * L.size, 0.0), vx(nblk * 2 * N), vd(nblk * N);
        for (int b = 0; b < nblk; ++b) {
            double* A = &par[(size_t)b * L.size + L.cdd_inv];
            for (int i = 0; i < G; ++i) for (int j = 0; j <= i; ++j) A[i * G + j] = A[j * G + i] = (i == j ? 1.0 : 0.2 * urand());
            par[(size_t)b * L.size + L.scal + 4] = b & 1; par[(size_t)b * L.size + L.scal + 5] = 0.01; par[(size_t)b * L.size + L.scal + 6] = 0.02;
            for (int i = 0; i < 2 * N; ++i) vx[b * 2 * N + i] = 4.0 * urand() - 2.0;
            for (int i = 0; i < N; ++i) vd[b * N + i] = 6.0 * urand() - 2.0;
        }
        std::vector<double> o[2][3];
        for (int il = 0; il < 2; ++il) {
            o[il][0].resize(nblk * N); o[il][1].resize(nblk * N); o[il][2].resize(nblk);
            bad |= qdht_pg(N, il, nblk, par.data(), L.size, vx.data(), vd.data(), o[il][0].data(), o[il][1].data(), o[il][2].data());
        }
        for (int k = 0; k < 3; ++k) bad |= memcmp(o[0][k].data(), o[1][k].data(), o[0][k].size() * sizeof(double)) != 0;
    }
    // floors of a tile on both sides of 0x7FFF, the limit of the packed reduction.  kind 0: anywhere below 32768; 1: a tile's
    // spread around the limit (some lanes packable, others not); 2: all above; 3: a spread around 0 with negative floors; 4: a
    // spread that ends exactly at the limit.  Per lane qd_fl_packable is the range test, and the kernel's test of the OR of a
    // lane's floors is the AND of the single tests; a tile whose lanes are all packable reduces to the plain min / max (any
    // other tile takes the plain reductions in the kernel and is not packed here).
    int packed_tiles = 0, plain_tiles = 0;
    for (int rep = 0; rep < 1000; ++rep) {
        const int kind = rep % 5;
        const int base = kind == 1 ? 0x7FFF - 7 + (int)(urand() * 8.0) : kind == 2 ? 0x8000 + (int)(urand() * 40000.0)
                       : kind == 3 ? -3 : kind == 4 ? 0x7FFF - 7 : 0;
        int fl[64], mn, mx, rmn = 0x7FFFFFFF, rmx = -0x7FFFFFFF, orfl = 0;
        bool all = true;
        for (int l = 0; l < 64; ++l) {
            fl[l] = kind == 0 ? (int)(urand() * 32768.0) : base + (int)(urand() * 8.0);
            rmn = fl[l] < rmn ? fl[l] : rmn; rmx = fl[l] > rmx ? fl[l] : rmx;
            const bool want = fl[l] >= 0 && fl[l] <= 0x7FFF;
            bad |= (qdht_fl_packable(fl[l]) != 0) != want;
            all = all && want;
            orfl |= fl[l];
        }
        bad |= (qdht_fl_packable(orfl) != 0) != all;
        if (kind == 0 || kind == 4) bad |= !all;
        if (kind == 2) bad |= all;
        if (all) {
            qdht_fl_minmax(fl, &mn, &mx);
            bad |= mn != rmn || mx != rmx;
            packed_tiles++;
        } else plain_tiles++;
    }
    bad |= packed_tiles < 400 || plain_tiles < 300;                          // both sides were drawn
    const int scap = 383;
    std::vector<uint32_t> sc(scap); std::vector<double> sD(scap), sa(scap), sb(scap);
    for (int KC = 8; KC <= 32; KC *= 2)
        for (int rep = 0; rep < 200; ++rep) {
            const int nf = KC + (int)(urand() * 40), nb = (int)(urand() * 60);
            for (int s = 0; s < scap; ++s) { sc[s] = (s < nf || urand() < 0.5) ? 0x11111111u : 0x77777777u; sD[s] = floor(6.0 * urand()); sa[s] = floor(3.0 * urand()); sb[s] = 0.0; }
            double e[2][32], mE[2], eo[2]; uint16_t id[2][32]; int ms[2][3], redo[2];
            for (int f = 0; f < 2; ++f)
                bad |= qdht_select(KC, f, nf + nb, nf, scap, sc.data(), sD.data(), sa.data(), sb.data(), 1.0, -2.0, 0x00000000u, 0x33333333u, 0.5,
                                   e[f], id[f], &mE[f], ms[f], &eo[f], &redo[f]);
            bad |= memcmp(e[0], e[1], KC * sizeof(double)) != 0 || memcmp(id[0], id[1], KC * sizeof(uint16_t)) != 0 || mE[0] != mE[1] ||
                   memcmp(ms[0], ms[1], sizeof ms[0]) != 0 || eo[0] != eo[1] || redo[0] != redo[1];
        }
    printf(bad ? "qd_tile_asan: MISMATCH\n" : "qd_tile_asan: ok\n");
    return bad ? 1 : 0;
}
