// qd_probe.h -- kernels of the stateless probe scans (qd_probe) and of the device-range composite (qd_probe_compose).
// A probe renders queries through the SAME candidate / ground-state / sensor / percentile kernels as qd_observe, on a
// second set of parameter, state and signal buffers: the gather kernel fills those from the env blocks and the query
// arrays, the write kernel hands the result to the caller.  The composite needs percentiles of nx*ny*P values (millions
// for a real map), far beyond the one block per env of qd_k_percentile: the select here is the same MSB-first radix
// select on the same keys (qd_key), with the histogram of each pass spread over the grid.
#pragma once
#include "qd_kernels.h"

// ---------------------------------------------------------------------------
// gather: probe slot k (query base + k) <- parameter and state block of env env_of_query[base + k], with the window
// (scal[2]), the gate / barrier voltages and the sensor slot taken from the query.  An id outside [0, B) renders a
// clamped env (the write kernel skips its slot).  grid = cnt, block = QD_PROBE_BLOCK.
// ---------------------------------------------------------------------------
#define QD_PROBE_BLOCK 128
struct QdProbeQuery {
    const int* env_of_query;
    const double *gate_v, *barrier_v, *sensor_v, *window;      // [nq][N], [nq][N-1], [nq] or null, [nq] or null
};

__global__ void __launch_bounds__(QD_PROBE_BLOCK)
qd_k_probe_gather(QdProbeQuery Q, int base, int B, int N, const double* __restrict__ params, const double* __restrict__ state,
                  double* __restrict__ pparams, double* __restrict__ pstate) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.x, q = base + k, nb = N - 1;
    int e = Q.env_of_query[q];
    e = e < 0 ? 0 : (e >= B ? B - 1 : e);
    const double* par = params + (size_t)e * L.size;
    const double* st = state + (size_t)e * L.s_size;
    double* dp = pparams + (size_t)k * L.size;
    double* ds = pstate + (size_t)k * L.s_size;
    for (int i = threadIdx.x; i < L.size; i += QD_PROBE_BLOCK)
        dp[i] = (i == L.scal + 2 && Q.window) ? Q.window[q] : par[i];
    for (int i = threadIdx.x; i < L.s_size; i += QD_PROBE_BLOCK) {
        double v = st[i];
        if (i >= L.s_gate_v && i < L.s_gate_v + N) v = Q.gate_v[(size_t)q * N + (i - L.s_gate_v)];
        else if (i >= L.s_barrier_v && i < L.s_barrier_v + nb) v = Q.barrier_v[(size_t)q * nb + (i - L.s_barrier_v)];
        else if (i == L.s_sensor_gt) v = Q.sensor_v ? Q.sensor_v[q] : 0.0;      // sensor_voltage=None -> 0.0
        ds[i] = v;
    }
}

// ---------------------------------------------------------------------------
// write: probe slot k -> the caller's slot base + k.  raw [nq][C][P] float64, image [nq][R][R][C] float32 normalised with
// the slot's own percentiles (qd_norm, as qd_k_write_obs), plohi [nq][2].  grid = (ceil(P/256), cnt).
// ---------------------------------------------------------------------------
__global__ void qd_k_probe_write(const int* __restrict__ env_of_query, int base, int B, int C, int P, const double* __restrict__ pz,
                                 const double* __restrict__ pplohi, double* __restrict__ raw_dst, float* __restrict__ image_dst,
                                 double* __restrict__ plohi_dst) {
    const int k = blockIdx.y, q = base + k;
    const int e = env_of_query[q];
    if (e < 0 || e >= B) return;
    const double lo = pplohi[2 * k], hi = pplohi[2 * k + 1];
    if (plohi_dst && blockIdx.x == 0 && threadIdx.x < 2) plohi_dst[2 * (size_t)q + threadIdx.x] = threadIdx.x ? hi : lo;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    for (int c = 0; c < C; ++c) {
        const double z = pz[((size_t)k * C + c) * P + p];
        if (raw_dst) raw_dst[((size_t)q * C + c) * P + p] = z;
        if (image_dst) image_dst[((size_t)q * P + p) * C + c] = qd_norm(z, lo, hi);
    }
}

// ---------------------------------------------------------------------------
// write, occupations (qd_probe_ex with occ_dst): probe slot k -> the caller's slot base + k, [nq][C][P][N] float64 as
// qd_get_occupations lays them out.  A channel the radial stage replaced by white noise (qd_radial_replaced on the probe's
// own parameter and state copies) was never solved: its occupations are NaN.  Ids outside [0, B) are skipped.
// grid = (ceil(P N / 256), C, cnt).
// ---------------------------------------------------------------------------
__global__ void qd_k_probe_write_occ(const int* __restrict__ env_of_query, int base, int B, int N, int P, const double* __restrict__ pparams,
                                     const double* __restrict__ pstate, int noise_flags, const double* __restrict__ pocc,
                                     double* __restrict__ occ_dst) {
    const int k = blockIdx.z, ch = blockIdx.y, q = base + k, C = N - 1;
    const int e = env_of_query[q];
    if (e < 0 || e >= B) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * N) return;
    const QdLayout L = qd_layout(N);
    const bool replaced = qd_radial_replaced(pparams + (size_t)k * L.size, pstate + (size_t)k * L.s_size, L, ch, noise_flags);
    occ_dst[((size_t)q * C + ch) * P * N + i] = replaced ? NAN : pocc[((size_t)k * C + ch) * P * N + i];
}

// ---------------------------------------------------------------------------
// composite, step 1: one channel of the probe signals, compact: cz[q][p] = raw[q][channel][p].  grid-stride.
// ---------------------------------------------------------------------------
__global__ void qd_k_map_extract(const double* __restrict__ raw, long nq, int C, int P, int channel, double* __restrict__ cz) {
    const long n = nq * P;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long q = i / P, p = i - q * P;
        cz[i] = raw[((size_t)q * C + channel) * P + p];
    }
}

// ---------------------------------------------------------------------------
// composite, step 2 (QD_MAP_GLOBAL): the 0.5 / 99.5 percentiles (numpy 'linear') of n values, exact, by the radix select
// of qd_radix_select2 with every pass's histogram built by the whole grid: each block counts its share in LDS and adds its
// non-empty bins to the global histogram (integer atomics: exact whatever the order); a one-block kernel then picks the
// bin of each rank and clears the histogram for the next pass.  8 x (histogram + pick), one rank pass, one finish.
// ---------------------------------------------------------------------------
#define QD_SEL_BLOCK 256
struct QdSelState {
    unsigned long long prefix[2];
    long t[2];
    unsigned long long cnt_le[2], mn[2];
    unsigned hist[2][256];
    int nan;
};

__global__ void qd_k_sel_init(QdSelState* S, long t0, long t1) {
    const int i = threadIdx.x;
    if (i < 512) S->hist[i >> 8][i & 255] = 0;
    if (i < 2) { S->prefix[i] = 0; S->t[i] = i ? t1 : t0; S->cnt_le[i] = 0; S->mn[i] = ~0ull; }
    if (i == 0) S->nan = 0;
}

__global__ void __launch_bounds__(QD_SEL_BLOCK)
qd_k_sel_hist(const double* __restrict__ z, long n, int pass, QdSelState* S) {
    __shared__ unsigned hist[2][256];
    for (int i = threadIdx.x; i < 512; i += QD_SEL_BLOCK) hist[i >> 8][i & 255] = 0;
    __syncthreads();
    const int shift = pass * 8;
    const unsigned long long mask = pass == 7 ? 0ull : (~0ull << (shift + 8));
    const unsigned long long prefix[2] = {S->prefix[0], S->prefix[1]};
    int has_nan = 0;
    // (whole blocks step together, `valid` false past the end: the wave votes below need every lane in the loop)
    for (long i0 = (long)blockIdx.x * QD_SEL_BLOCK; i0 < n; i0 += (long)gridDim.x * QD_SEL_BLOCK) {
        const long i = i0 + threadIdx.x;
        const bool valid = i < n;
        const double v = valid ? z[i] : 0.0;
        has_nan |= (v != v);
        const unsigned long long k = qd_key(v);
        const unsigned d = (unsigned)(k >> shift) & 255u;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const bool in = valid && (k & mask) == prefix[w];
            // the leading bytes of a map's values are mostly equal: one LDS add per wave instead of 64 colliding ones
            const unsigned long long act = __ballot(in);
            if (act) {
                const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, __builtin_ctzll(act));
                if (__ballot(in && d == d0) == act) {
                    if ((int)(threadIdx.x & 63) == __builtin_ctzll(act)) atomicAdd(&hist[w][d0], (unsigned)__builtin_popcountll(act));
                } else if (in) atomicAdd(&hist[w][d], 1u);
            }
        }
    }
    if (pass == 7 && has_nan) S->nan = 1;
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += QD_SEL_BLOCK) {
        const unsigned c = hist[i >> 8][i & 255];
        if (c) atomicAdd(&S->hist[i >> 8][i & 255], c);
    }
}

// block = 128: wave w picks the bin of rank w (first bin b with count(bins <= b) > t), 4 bins per lane, as qd_radix_select2
__global__ void __launch_bounds__(128)
qd_k_sel_pick(int pass, QdSelState* S) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int shift = pass * 8;
    const long tw = S->t[w];
    const unsigned long long pw = S->prefix[w];
    unsigned h4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { h4[j] = S->hist[w][4 * l + j]; S->hist[w][4 * l + j] = 0; }
    const long own = (long)h4[0] + (long)h4[1] + (long)h4[2] + (long)h4[3];
    long inc = own;
    for (int o = 1; o < 64; o <<= 1) { const long v = (long)__shfl_up((long long)inc, o, 64); if (l >= o) inc += v; }
    const long exc = inc - own;
    const unsigned long long hit = __ballot(inc > tw);
    const int wl = hit ? __builtin_ctzll(hit) : 63;
    if (l == wl) {
        long acc = exc; int b = 4 * l;
        for (int j = 0; j < 4; ++j, ++b) { if (acc + (long)h4[j] > tw) break; acc += h4[j]; }
        if (b > 255) b = 255;
        S->prefix[w] = pw | ((unsigned long long)b << shift);
        S->t[w] = tw - acc;
    }
}

// rank ip + 1 of each selection: equal to the selected key if enough values are <= it, else the smallest key above it
__global__ void __launch_bounds__(QD_SEL_BLOCK)
qd_k_sel_rank(const double* __restrict__ z, long n, QdSelState* S) {
    const unsigned long long ka[2] = {S->prefix[0], S->prefix[1]};
    unsigned long long cnt[2] = {0, 0}, mn[2] = {~0ull, ~0ull};
    for (long i = (long)blockIdx.x * QD_SEL_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * QD_SEL_BLOCK) {
        const unsigned long long k = qd_key(z[i]);
#pragma unroll
        for (int w = 0; w < 2; ++w) { cnt[w] += k <= ka[w]; if (k > ka[w] && k < mn[w]) mn[w] = k; }
    }
    __shared__ unsigned long long red[4][QD_SEL_BLOCK / 64];
#pragma unroll
    for (int w = 0; w < 2; ++w)
        for (int o = 32; o > 0; o >>= 1) {
            cnt[w] += (unsigned long long)__shfl_xor((long long)cnt[w], o, 64);
            const unsigned long long other = (unsigned long long)__shfl_xor((long long)mn[w], o, 64);
            mn[w] = other < mn[w] ? other : mn[w];
        }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = cnt[0]; red[1][threadIdx.x >> 6] = cnt[1];
        red[2][threadIdx.x >> 6] = mn[0]; red[3][threadIdx.x >> 6] = mn[1];
    }
    __syncthreads();
    if (threadIdx.x < 2) {                                  // one add and one min per block and rank
        const int w = threadIdx.x;
        unsigned long long tot = 0, gm = ~0ull;
        for (int v = 0; v < QD_SEL_BLOCK / 64; ++v) { tot += red[w][v]; gm = red[2 + w][v] < gm ? red[2 + w][v] : gm; }
        if (tot) atomicAdd(&S->cnt_le[w], tot);
        if (gm != ~0ull) atomicMin(&S->mn[w], gm);
    }
}

__global__ void qd_k_sel_finish(const QdSelState* S, long ip0, long ip1, long in0, long in1, double g0, double g1,
                                double* __restrict__ plohi, double* __restrict__ plohi_dst) {
    if (threadIdx.x >= 2) return;
    const int w = threadIdx.x;
    const long ip = w ? ip1 : ip0, in = w ? in1 : in0;
    const double g = w ? g1 : g0;
    double r = NAN;
    if (!S->nan) {
        const unsigned long long ka = S->prefix[w];
        unsigned long long kb = ka;
        if (in != ip) kb = ((long)S->cnt_le[w] > in) ? ka : S->mn[w];
        r = qd_lerp(qd_unkey(ka), qd_unkey(kb), g);
    }
    plohi[w] = r;
    if (plohi_dst) plohi_dst[w] = r;
}

// ---------------------------------------------------------------------------
// composite, step 3: scan (i, j) = query i*ny + j goes to columns i*R.. and row block j (flip: ny-1-j), normalised with
// the composite's percentiles (per_scan 0: plohi[0..1]) or its own (per_scan 1: plohi[2q..]).  grid = (ceil(P/256), nx*ny).
// ---------------------------------------------------------------------------
__global__ void qd_k_map_place(const double* __restrict__ cz, int nx, int ny, int R, int per_scan, int flip,
                               const double* __restrict__ plohi, float* __restrict__ composite, double* __restrict__ plohi_dst) {
    const int q = blockIdx.y, i = q / ny, j = q - i * ny, P = R * R;
    const double lo = plohi[per_scan ? 2 * q : 0], hi = plohi[per_scan ? 2 * q + 1 : 1];
    if (per_scan && plohi_dst && blockIdx.x == 0 && threadIdx.x < 2) plohi_dst[2 * (size_t)q + threadIdx.x] = threadIdx.x ? hi : lo;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int y = p / R, x = p - y * R;
    const int jb = flip ? ny - 1 - j : j;
    composite[((size_t)jb * R + y) * ((size_t)nx * R) + (size_t)i * R + x] = qd_norm(cz[(size_t)q * P + p], lo, hi);
}
