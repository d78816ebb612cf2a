// qd_latch.h -- charge latching (a14) one raster row at a time, for the probe scans (qd_probe_ex).
// qd_k_latch (qd_kernels.h) walks the P pixels of an (env, channel) on one thread; its held state is reset at every row
// start, so the rows are independent.  qd_latch_row is the body of that walk for ONE row -- the same isclose test, the same
// Philox counter (absolute pixel index, channel | QD_RNG_LATCH << 16, serial), the same fma chain for the correction of
// the sensor constant -- and qd_k_latch_rows runs one lane per (slot, channel, row): R times as many lanes, chains of R
// pixels instead of R*R.  Same bits as qd_k_latch.  __host__ __device__ so the no-GPU tests walk rows on the CPU.
#pragma once
#include <math.h>
#include "qd_rng.h"

// One row of the latching walk, in place: occ_row [R][N] occupations and z_row [R] sensor constants c0 of pixels
// row*R .. row*R + R - 1 of channel ch.  par: the env's parameter block; (seed, k1): Philox key; (ser_lo, ser_hi): serial.
template <int N>
QD_HD void qd_latch_row(const double* par, const QdLayout& L, double* occ_row, double* z_row, int row, int R, int ch,
                        uint32_t seed, uint32_t ser_lo, uint32_t ser_hi, uint32_t k1) {
    constexpr int G = N + 1;
    double hold[N];
    for (int x = 0; x < R; ++x) {
        double nn[N];
#pragma unroll
        for (int i = 0; i < N; ++i) nn[i] = occ_row[(size_t)x * N + i];
        bool accept = true;
        if (x != 0) {
            int cnt = 0, a = 0, b = 0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const bool differ = !(fabs(hold[i] - nn[i]) <= 1e-8 + 1e-5 * fabs(nn[i]));
                if (differ) { if (cnt == 0) a = i; else if (cnt == 1) b = i; cnt++; }
            }
            if (cnt == 1 || cnt == 2) {
                const uint32_t p = (uint32_t)(row * R + x);
                const QdPhilox r = qd_philox4x32_10(p, (uint32_t)ch | (QD_RNG_LATCH << 16), ser_lo, ser_hi, seed, k1);
                const double u = qd_u01(r.v[0], r.v[1]);
                const double pa = (cnt == 1) ? par[L.pleads + a] : par[L.pinter + a * N + b];
                accept = u < pa;
            }
        }
        if (accept) {
#pragma unroll
            for (int i = 0; i < N; ++i) hold[i] = nn[i];
        } else {
            double corr = 0.0;
#pragma unroll
            for (int i = 0; i < N; ++i) { corr = fma(par[L.cdd_inv + N * G + i], hold[i] - nn[i], corr); occ_row[(size_t)x * N + i] = hold[i]; }
            z_row[x] += 2.0 * corr;
        }
    }
}

#if defined(__HIPCC__)
#include "qd_kernels.h"

// One lane per (slot, channel, row) of n_slots probe slots (slot = block index of the buffers; no env list): lane t works on
// row t % R of channel (t / R) % C of slot t / (R C), so a wave holds 64 consecutive rows -- at R = 64 one channel image.
// Neighbouring lanes are R*N doubles apart (4 KB at 8 dots, 64x64): nothing coalesces, each lane streams its own row of
// N*8-byte records front to back, as the one thread of qd_k_latch does, and the R-fold parallelism is the gain.
// Replaced channels (qd_radial_replaced: qd_k_sensor writes pure noise) return at once.  grid = ceil(n_slots C R / 64).
#define QD_LATCH_ROWS_BLOCK 64
// C: channel images per slot (N - 1 on probe buffers; 1 on those of qd_scan2d)
template <int N, int C = N - 1>
__global__ void __launch_bounds__(QD_LATCH_ROWS_BLOCK)
qd_k_latch_rows(int n_slots, int R, const double* __restrict__ params, const double* __restrict__ state,
                double* __restrict__ occ, double* __restrict__ zraw, QdNoiseCfg nz) {
    const QdLayout L = qd_layout(N);
    const long t = (long)blockIdx.x * QD_LATCH_ROWS_BLOCK + threadIdx.x;
    if (t >= (long)n_slots * C * R) return;
    const int row = (int)(t % R);
    const int sc = (int)(t / R), slot = sc / C, ch = sc - slot * C;
    const double* par = params + (size_t)slot * L.size;
    const double* st = state + (size_t)slot * L.s_size;
    if (qd_radial_replaced(par, st, L, ch, nz.flags)) return;
    const size_t p0 = ((size_t)slot * C + ch) * R * R + (size_t)row * R;
    qd_latch_row<N>(par, L, occ + p0 * N, zraw + p0, row, R, ch, nz.seed, nz.ser_lo, nz.ser_hi, nz.env_off + (uint32_t)slot);
}
#endif
