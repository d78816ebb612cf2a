// Stand-alone sanitizer run of the grid front end (csrc/qd_grid.h): walks qd_grid_record over slots with a tail, each slot in
// a heap buffer of exactly side*side records, and the latching walk over occupation and signal buffers of exactly nx*ny
// entries, so a record, a row or a descriptor read past its end is an AddressSanitizer report.  Built with
// -fsanitize=address,undefined; exit status 0 and the line "grid asan ok" mean a clean run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "qd_grid.h"

static double unit(uint64_t& s) {                      // splitmix64 -> (-1, 1)
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

template <int N>
static int walk(int nx, int ny, int frame, uint64_t seed) {
    const QdLayout L = qd_layout(N);
    const int n = nx * ny, side = qd_line_side(n), SP = side * side;
    std::vector<double> par((size_t)L.size), st((size_t)L.s_size);
    for (double& v : par) v = 0.3 * unit(seed);
    for (double& v : st) v = 0.3 * unit(seed);
    for (int i = 0; i < N; ++i) par[L.pleads + i] = 0.5;
    for (int i = 0; i < N * N; ++i) par[L.pinter + i] = 0.5;
    QdGridAxes* A = (QdGridAxes*)malloc(sizeof(QdGridAxes));      // on the heap: a read past the descriptor is a report
    memset(A, 0, sizeof(*A));
    A->x_lo = -2.0; A->x_hi = 3.0; A->y_lo = 1.5; A->y_hi = -0.5;
    for (int i = 0; i < 2 * N; ++i) { A->dx[i] = unit(seed); A->dy[i] = unit(seed); }
    A->nx = nx; A->ny = ny; A->frame = frame;
    QdPixelRec* recs = (QdPixelRec*)malloc(sizeof(QdPixelRec) * (size_t)SP);
    memset(recs, 0xA5, sizeof(QdPixelRec) * (size_t)SP);
    int live = 0, bad = 0;
    for (int j = 0; j < SP; ++j) {
        double v_ext[2 * N], vd[N], ncont[N], isa;
        if (qd_grid_record<N>(par.data(), st.data(), A, nx, ny, j, recs + j, v_ext, vd, ncont, &isa)) {
            ++live;
            if (j >= n) ++bad;
        } else {
            const unsigned char* b = reinterpret_cast<const unsigned char*>(recs + j);
            for (size_t i = 0; i < sizeof(QdPixelRec); ++i) bad += b[i] != 0;
            if (j < n) ++bad;
        }
    }
    if (live != n) ++bad;
    // the latching walk on buffers of exactly n points
    double* occ = (double*)malloc(sizeof(double) * (size_t)n * N);
    double* z = (double*)malloc(sizeof(double) * (size_t)n);
    for (int p = 0; p < n; ++p) {
        z[p] = unit(seed);
        for (int i = 0; i < N; ++i) occ[(size_t)p * N + i] = (double)(int)(2.0 * unit(seed));
    }
    for (int y = 0; y < ny; ++y) qd_grid_latch_row<N>(par.data(), L, occ, z, nx, y, 0x1234u, 7u, 0u, 99u);
    free(z); free(occ); free(recs); free(A);
    if (bad) fprintf(stderr, "grid asan: N=%d %dx%d frame %d: %d wrong records\n", N, nx, ny, frame, bad);
    return bad;
}

int main() {
    int bad = 0;
    const int shapes[][2] = {{1, 1}, {5, 3}, {3, 5}, {8, 1}, {1, 8}, {18, 5}, {10, 6}, {16, 4}, {37, 3}};
    uint64_t seed = 2026;
    for (const auto& s : shapes)
        for (int frame = 0; frame < 2; ++frame) {
            bad += walk<2>(s[0], s[1], frame, seed++);
            bad += walk<4>(s[0], s[1], frame, seed++);
            bad += walk<8>(s[0], s[1], frame, seed++);
        }
    if (bad) return 1;
    printf("grid asan ok\n");
    return 0;
}
