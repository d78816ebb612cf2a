// qd_fullspace.h -- the untruncated charge-state space (qd_config.num_charge_states = QD_ALL_CHARGE_STATES(m); reference:
// TunnelCoupledChargeSensed.num_charge_states = None, ground_state.py:29, 79-83, 149-162): every state with 0..m carriers
// per dot, M = (m + 1)^N of them, the same list for every pixel (charge_states.py:5-34, enumerated in base m + 1 with dot 0
// the most significant digit), H = diag(F) + H_t over all of them and the ground vector of its dense eigh.
//
// Hopping conserves the total charge Q, so H is block diagonal by Q and the blocks (sectors) are the same for every
// pixel: the handle builds their tables once (QdFullTab, positions ordered by (Q, reference index)).  No continuous
// ground state and no candidate search run in this mode.  Per launch chunk:
//
//   qd_k_full_structure  one pixel per wave, 2 / 4 / 8 states per lane (M <= 128 / 256 / 512): the front end (voltages, tunnel couplings, the linear
//                        capacitance scale factors), the M free energies in the canonical form of the candidate search,
//                        Gershgorin pruning per component, and one task per surviving component of >= 2 states in the
//                        slab and the tile lists of qd_k_gs_structure (so the solve launches and qd_eig.h are shared).
//                        A component is a sector; where a pair's coupling is exactly zero the sector splits further
//                        (the charge left of that pair is conserved too), so tc == 0 still gives integer occupations.
//   qd_k_gs_solve<class> unchanged (components of 2..32 states)
//   qd_k_full_solve_wide components of 33..64 states, one per wavefront (qd_eig_wave.h): the WIDE class.  It has a task list
//                        and an eigenvalue array of its own, in a buffer that only handles with a sector above 32 states
//                        allocate (QdWide); its task count sits in the free slot cnt[QD_GS_WBIN] of the slab; its links are
//                        QD_LINK_WIDE0 + position in that list.  Handles without such a sector run the kernels without the
//                        class (template parameter WIDE = false) and launch exactly what they launched before it existed.
//   qd_k_full_select     one pixel per lane: the lowest component (ties: lowest reference index), <n> from the winner's
//                        vector and the state table, the sensor constant c0 (qd_gs_emit).
//
// The slabs keep the size of the K-state mode; a batch holds ppb <= QD_GS_PPB pixels, chosen by qd_full_ppb so that the
// worst case (every component surviving) fits the pool, the task lists and the per-state link / rank arrays.
#pragma once
#include <math.h>
#include <algorithm>
#include "qd_kernels.h"
#include "qd_eig_wave.h"

#define QD_FULL_MAXM 512          // states of the full space, at most
#define QD_FULL_MAXSEC 32         // total-charge sectors, N m + 1, at most
#define QD_FULL_MAXCAR 15         // carriers per dot, at most (the state tables keep 4 bits per dot)
#define QD_FULL_MAXSECTOR QD_EW_MAX   // states of a sector, at most: one per lane of the wide solver
#define QD_GS_WBIN QD_GS_NBIN     // the wide class: slot of its task count in the slab's cnt[]
#define QD_LINK_WIDE0 0x80000000u // links of wide tasks: QD_LINK_WIDE0 + position in the batch's wide list
#define QD_FULL_MAXNB (2 * (QD_MAXN - 1))   // hop neighbours of a state

struct QdFullTab {
    int M, nsec, maxsec, pad;
    int sec_start[QD_FULL_MAXSEC + 1];              // positions of sector q: sec_start[q] .. sec_start[q + 1] - 1
    int sec[QD_FULL_MAXM];                          // sector of position p
    unsigned idx[QD_FULL_MAXM];                     // reference index of position p
    unsigned dig[QD_FULL_MAXM];                     // its occupations, 4 bits per dot (dot i at bit 4 i)
    int nnb[QD_FULL_MAXM];                          // hop neighbours of position p
    unsigned short nbr[QD_FULL_MAXM][QD_FULL_MAXNB];//   their positions
    unsigned char nbd[QD_FULL_MAXM][QD_FULL_MAXNB]; //   the adjacent pair (d, d + 1) of the hop
    double nbf[QD_FULL_MAXM][QD_FULL_MAXNB];        //   sqrt(n_from (n_to + 1)) with the occupations of the row state
};

// M and the largest sector of (N dots, at most m carriers each); false when M exceeds QD_FULL_MAXM
static inline bool qd_full_sizes(int N, int m, int& M, int& maxsec) {
    if (N < 2 || N > QD_MAXN || m < 1 || m > QD_FULL_MAXCAR) return false;
    // (also what the component keys need: the charge left of a pair, <= N m <= 31, is packed in 7 bits per pair)
    if (N * m + 1 > QD_FULL_MAXSEC) return false;
    M = 1;
    for (int i = 0; i < N; ++i) { M *= m + 1; if (M > QD_FULL_MAXM) return false; }
    int cnt[QD_FULL_MAXSEC] = {0};
    maxsec = 0;
    for (int s = 0; s < M; ++s) {
        int q = 0, r = s;
        for (int i = 0; i < N; ++i) { q += r % (m + 1); r /= m + 1; }
        if (++cnt[q] > maxsec) maxsec = cnt[q];
    }
    return true;
}

static inline bool qd_full_supported(int N, int m) {
    int M, maxsec;
    return qd_full_sizes(N, m, M, maxsec) && maxsec <= QD_FULL_MAXSECTOR;
}
// states per lane of the structure kernel, and whether the handle needs the wide class
static inline int qd_full_spl(int M) { return M <= 128 ? 2 : (M <= 256 ? 4 : 8); }
static inline bool qd_full_wide(int maxsec) { return maxsec > QD_K; }
// record of a task: blocks of 33..64 states carry no workspace (the wave solver keeps the block in LDS and computes the
// residual from the record itself before it overwrites it)
__host__ __device__ inline int qd_full_task_doubles(int s, bool validate) {
    return s > QD_K ? ((2 + s * (s + 1) / 2 + 1) & ~1) : qd_gs_task_doubles(s, validate);
}

// host: the tables of a supported (N, m)
static inline void qd_full_build(int N, int m, QdFullTab& t) {
    int M, maxsec;
    qd_full_sizes(N, m, M, maxsec);
    t = QdFullTab{};
    t.M = M; t.maxsec = maxsec; t.nsec = N * m + 1;
    int digits[QD_FULL_MAXM][QD_MAXN], charge[QD_FULL_MAXM];
    for (int s = 0; s < M; ++s) {                   // reference index s: dot 0 is the most significant digit
        int r = s; charge[s] = 0;
        for (int i = N - 1; i >= 0; --i) { digits[s][i] = r % (m + 1); r /= m + 1; charge[s] += digits[s][i]; }
    }
    int pos_of[QD_FULL_MAXM], p = 0;
    for (int q = 0; q < t.nsec; ++q) {
        t.sec_start[q] = p;
        for (int s = 0; s < M; ++s)
            if (charge[s] == q) {
                pos_of[s] = p; t.sec[p] = q; t.idx[p] = (unsigned)s;
                unsigned d = 0;
                for (int i = 0; i < N; ++i) d |= (unsigned)digits[s][i] << (4 * i);
                t.dig[p] = d;
                ++p;
            }
    }
    t.sec_start[t.nsec] = p;
    // hops of hamiltonian_build.py:75-137 inside the list: s_j = s_i -+ e_d +- e_{d+1}, H_ij = -t_d sqrt(n_from (n_to + 1))
    // with n the occupations of the row state i
    for (int s = 0; s < M; ++s) {
        const int pi = pos_of[s];
        int k = 0;
        for (int d = 0; d + 1 < N; ++d) {
            const int a = digits[s][d], b = digits[s][d + 1];
            int stride = 1;                                  // reference-index weight of dot d + 1
            for (int i = d + 2; i < N; ++i) stride *= m + 1;
            if (a >= 1 && b <= m - 1) {                      // forward: one carrier d -> d + 1
                t.nbr[pi][k] = (unsigned short)pos_of[s - stride * (m + 1) + stride];
                t.nbd[pi][k] = (unsigned char)d; t.nbf[pi][k] = sqrt((double)a * ((double)b + 1.0)); ++k;
            }
            if (b >= 1 && a <= m - 1) {                      // backward: d + 1 -> d
                t.nbr[pi][k] = (unsigned short)pos_of[s + stride * (m + 1) - stride];
                t.nbd[pi][k] = (unsigned char)d; t.nbf[pi][k] = sqrt((double)b * ((double)a + 1.0)); ++k;
            }
        }
        t.nnb[pi] = k;
    }
}

// host: pixels per slab in this mode.  Worst case per pixel: every sector one surviving task (a split sector needs no more
// pool, its parts being smaller); tasks of a size class: at most floor(size / smallest size of the class) per sector.
// 0 when not even one pixel fits (qd_create refuses).  The wide class has no fixed list: the handle sizes it as
// ppb * qd_full_wide_tasks.
static inline int qd_full_wide_tasks(const QdFullTab& t) {
    int n = 0;
    for (int q = 0; q < t.nsec; ++q) n += (t.sec_start[q + 1] - t.sec_start[q]) / (QD_K + 1);
    return n;
}
static inline int qd_full_ppb(const QdFullTab& t, bool validate) {
    size_t pool = 0;
    int tasks[QD_GS_NBIN] = {0};
    for (int q = 0; q < t.nsec; ++q) {
        const int s = t.sec_start[q + 1] - t.sec_start[q];
        if (s >= 2) pool += (size_t)qd_full_task_doubles(s, validate);
        for (int b = 0; b < QD_GS_NBIN; ++b) tasks[b] += s / qd_gs_bin_min(b);
    }
    size_t ppb = QD_GS_PPB;
    ppb = std::min(ppb, (size_t)(QD_GS_PPB * 32 / t.M));                 // link / rank: one entry per (state, pixel)
    if (pool) ppb = std::min(ppb, qd_gs_pool_doubles(validate) / pool);
    for (int b = 0; b < QD_GS_NBIN; ++b)
        if (tasks[b]) ppb = std::min(ppb, (size_t)(qd_gs_list_cap(b) / tasks[b]));
    return (int)ppb;
}

// the wide class's buffer, per batch: capw eigenvalues, then capw record offsets (capw = ppb * qd_full_wide_tasks, even)
struct QdWide { unsigned char* buf; unsigned capw; };
__host__ __device__ inline size_t qd_wide_bytes(unsigned capw) { return (size_t)capw * 12; }
__host__ __device__ inline double* qd_wide_lam(const QdWide& w, size_t batch) { return (double*)(w.buf + batch * qd_wide_bytes(w.capw)); }
__host__ __device__ inline unsigned* qd_wide_list(const QdWide& w, size_t batch) { return (unsigned*)(qd_wide_lam(w, batch) + w.capw); }

#if defined(__HIPCC__)

template <int MM>                            // MM = 64 x states per lane
struct QdFullWaveLds {
    double F[MM];                            // free energies relative to the pixel's lowest
    double lo[MM];                           // F - sum_j |H_ij|  (Gershgorin)
    unsigned long long key[MM];              // charges left of the pairs whose coupling is exactly zero
    unsigned base[MM];                       // component leader -> members: the task's record offset
    unsigned gi[MM];                         //   and its position in the task lists
    unsigned char rk[MM];                    // index inside the component
};
// waves per block of the structure kernel: 4.2 KB of LDS per wave at 2 states per lane, 8.4 KB at 4, 16.9 KB at 8
template <int SPL> struct QdFullWpb { static constexpr int v = SPL == 8 ? 2 : 4; };

__device__ __forceinline__ double qd_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}

template <int N>
__device__ __forceinline__ double qd_full_pick(const double* tc, int d) {   // tc[d] with static indices only
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < N - 1; ++q) t = (q == d) ? tc[q] : t;
    return t;
}

// one pixel (p, slot ps of the batch) on one wave; SPL states per lane; WIDE: components of 33..64 states go to the wide list
// (wcnt: its length so far, in LDS)
template <int N, bool VALIDATE, int SPL, bool WIDE>
__device__ __forceinline__ void qd_full_pixel(const double* __restrict__ par, const double* __restrict__ st, int ch, int R, int p,
                                              int ps, int ppb, const QdFullTab* __restrict__ tab, QdPixelRec* __restrict__ rec,
                                              QdFullWaveLds<64 * SPL>& W, QdBlockLds& S, const QdSlab& sl, unsigned* wcnt,
                                              unsigned* __restrict__ wlist) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
    const int lane = threadIdx.x & 63;
    const int M = tab->M;
    double v_ext[V], vpp[G], tc[NB];
    qd_pixel_voltages<N>(par, st, ch, R, p % R, p / R, v_ext, vpp, tc);
    double sa, sb;
    qd_vc_scales<N>(par, L, v_ext, sa, sb);
    const double isa = 1.0 / sa;
    double vd[N];
#pragma unroll
    for (int i = 0; i < N; ++i) vd[i] = vpp[i] * sb;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < G; ++i) rec->vpp[i] = vpp[i];          // the select kernel's sensor constant
    }
    unsigned zmask = 0;                                            // pairs whose coupling is exactly zero
#pragma unroll
    for (int d = 0; d < NB; ++d) zmask |= (tc[d] == 0.0 ? 1u : 0u) << d;

    // ---- free energies (canonical form: rows t_i = fma chain of A[i][j] (s_j - v'_j), E = fma chain of (s_i - v'_i) t_i,
    // times 1 / sa), Gershgorin radii, component keys
    double F[SPL], rad[SPL];
    unsigned long long key[SPL];
#pragma unroll
    for (int h = 0; h < SPL; ++h) {
        const int pos = lane + 64 * h;
        F[h] = INFINITY; rad[h] = 0.0; key[h] = 0;
        if (pos < M) {
            const unsigned dg = tab->dig[pos];
            double dd[N];
#pragma unroll
            for (int i = 0; i < N; ++i) dd[i] = (double)((dg >> (4 * i)) & 15u) - vd[i];
            double E = 0.0;
#pragma unroll 1
            for (int i = 0; i < N; ++i) {
                const double t = qd_dotN<N>(par + L.cdd_inv + i * G, dd);
                double di = dd[0];
#pragma unroll
                for (int j = 1; j < N; ++j) di = (j == i) ? dd[j] : di;
                E = fma(di, t, E);
            }
            F[h] = E * isa;
            const int nn = tab->nnb[pos];
            for (int k = 0; k < nn; ++k) rad[h] += fabs(-qd_full_pick<N>(tc, tab->nbd[pos][k]) * tab->nbf[pos][k]);
            if (zmask) {
                unsigned acc = 0;
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    acc += (dg >> (4 * i)) & 15u;
                    if ((zmask >> i) & 1u) key[h] |= (unsigned long long)acc << (7 * i);
                }
            }
        }
    }
    // the diagonal enters relative to the pixel's lowest free energy (as in qd_ground_structure)
    double fm = fmin(F[0], F[1]);
#pragma unroll
    for (int h = 2; h < SPL; ++h) fm = fmin(fm, F[h]);
    const double fshift = qd_wave_min(fm);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int h = 0; h < SPL; ++h) {
        const int pos = lane + 64 * h;
        if (pos < M) { W.F[pos] = F[h] - fshift; W.lo[pos] = (F[h] - fshift) - rad[h]; W.key[pos] = key[h]; }
    }
    __builtin_amdgcn_wave_barrier();

    // ---- components inside the sector, pruning, tasks
    int r[SPL], sz[SPL], lead[SPL];
    bool solve[SPL], active[SPL];
#pragma unroll
    for (int h = 0; h < SPL; ++h) {
        const int pos = lane + 64 * h;
        r[h] = 0; sz[h] = 0; lead[h] = pos; solve[h] = false; active[h] = false;
        if (pos < M) {
            const int q = tab->sec[pos];
            const int s0 = tab->sec_start[q], s1 = tab->sec_start[q + 1];
            double lower = INFINITY;
            for (int j = s0; j < s1; ++j) {
                if (W.key[j] != key[h]) continue;
                if (sz[h] == 0) lead[h] = j;
                r[h] += j < pos ? 1 : 0;
                ++sz[h];
                lower = fmin(lower, W.lo[j]);
            }
            active[h] = lower <= 0.0;
            solve[h] = active[h] && sz[h] > 1;
            W.rk[pos] = (unsigned char)r[h];
            if (solve[h] && r[h] == 0) {
                if (WIDE && sz[h] > QD_K) {
                    const unsigned base = atomicAdd(&S.pool_top, (unsigned)qd_full_task_doubles(sz[h], VALIDATE));
                    const unsigned wi = atomicAdd(wcnt, 1u);
                    wlist[wi] = base;
                    sl.pool[base + 1] = (double)sz[h];
                    W.base[pos] = base; W.gi[pos] = QD_LINK_WIDE0 + wi;
                } else {
                const unsigned base = atomicAdd(&S.pool_top, (unsigned)qd_gs_task_doubles(sz[h], VALIDATE));
                const int bin = qd_gs_bin(sz[h]);
                const unsigned gi = (unsigned)qd_gs_list_off(bin) + atomicAdd(&S.cnt[bin], 1u);
                sl.lists[gi] = base;
                if (sz[h] > 8) sl.pool[base + 1] = (double)sz[h];
                W.base[pos] = base; W.gi[pos] = gi;
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    double hn = 0.0;
#pragma unroll
    for (int h = 0; h < SPL; ++h) {
        const int pos = lane + 64 * h;
        if (pos >= M) continue;
        if (VALIDATE) hn = fmax(hn, fabs(F[h]) + rad[h]);
        if (!solve[h]) { sl.link[pos * ppb + ps] = active[h] ? QD_LINK_SINGLE : QD_LINK_NONE; sl.rank[pos * ppb + ps] = 0; continue; }
        sl.link[pos * ppb + ps] = W.gi[lead[h]];
        sl.rank[pos * ppb + ps] = (unsigned char)r[h];
        // my row of the lower triangle: zeros, the couplings to members of lower rank, F on the diagonal
        double* row = sl.pool + W.base[lead[h]] + 2 + (r[h] * (r[h] + 1)) / 2;
        for (int c = 0; c < r[h]; ++c) row[c] = 0.0;
        const int nn = tab->nnb[pos];
        for (int k = 0; k < nn; ++k) {
            const double c = -qd_full_pick<N>(tc, tab->nbd[pos][k]) * tab->nbf[pos][k];
            if (c == 0.0) continue;                        // zero couplings link nothing (the neighbour is in another component)
            const int rj = W.rk[tab->nbr[pos][k]];
            if (rj < r[h]) row[rj] = c;
        }
        row[r[h]] = W.F[pos];
    }
    if (VALIDATE) {
        // ||H||_inf over all M states (unshifted) and the offset of the eigenvalues
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) hn = fmax(hn, __shfl_xor(hn, o, 64));
        if (lane == 0) { sl.aux[ps] = hn; sl.aux[QD_GS_PPB + ps] = fshift; }
    }
    __builtin_amdgcn_wave_barrier();
}

// grid = batches (of ppb pixels of one (env, channel)), 4 waves per block (2 at 8 states per lane), one pixel per wave at a time
template <int N, bool VALIDATE, int SPL, bool WIDE>
__global__ void __launch_bounds__(64 * QdFullWpb<SPL>::v)
qd_k_full_structure(const int* __restrict__ env_ids, int env_base, int rec_slot0, QdGsGeom g, int ppb, int R,
                    const double* __restrict__ params, const double* __restrict__ state, int noise_flags,
                    const QdFullTab* __restrict__ tab, QdPixelRec* __restrict__ recs, unsigned char* __restrict__ slabs,
                    unsigned* __restrict__ gtiles, unsigned* __restrict__ tilelist, size_t batches_cap, QdWide wide) {
    const QdLayout L = qd_layout(N);
    constexpr int WPB = QdFullWpb<SPL>::v;
    __shared__ QdFullWaveLds<64 * SPL> sW[WPB];
    __shared__ QdBlockLds sB;
    __shared__ unsigned sWcnt;
    const int batch = blockIdx.x;
    const QdSlab sl = qd_gs_slab(slabs + (size_t)batch * qd_gs_slab_bytes(VALIDATE), VALIDATE);
    const int wave = threadIdx.x >> 6;
    const int slot = batch / (g.C * g.nb);
    const int rem = batch - slot * g.C * g.nb;
    const int ch = rem / g.nb, p0 = (rem - ch * g.nb) * ppb;
    const int e = env_ids ? env_ids[env_base + slot] : env_base + slot;
    const double* par = params + (size_t)e * L.size;
    const double* st = state + (size_t)e * L.s_size;
    if (qd_radial_replaced(par, st, L, ch, noise_flags)) {               // qd_k_sensor writes pure noise: no tasks
        if (threadIdx.x < QD_GS_NBIN + (WIDE ? 1 : 0)) sl.cnt[threadIdx.x] = 0;
        return;
    }
    QdPixelRec* rbase = recs + ((size_t)(rec_slot0 + slot) * g.C + ch) * g.P;
    if (threadIdx.x <= QD_GS_NBIN) { if (threadIdx.x == 0) sB.pool_top = 0; else sB.cnt[threadIdx.x - 1] = 0; }
    if (WIDE && threadIdx.x == 0) sWcnt = 0;
    __syncthreads();
    unsigned* wlist = WIDE ? qd_wide_list(wide, (size_t)batch) : nullptr;
    for (int ps = wave; ps < ppb; ps += WPB) {
        const int p = p0 + ps;
        if (p >= g.P) break;                                             // uniform for the wave
        qd_full_pixel<N, VALIDATE, SPL, WIDE>(par, st, ch, R, p, ps, ppb, tab, rbase + p, sW[wave], sB, sl, &sWcnt, wlist);
    }
    __syncthreads();
    qd_gs_publish_tiles(sB, sl, batch, gtiles, tilelist, batches_cap);
    if (WIDE && threadIdx.x == 0) sl.cnt[QD_GS_WBIN] = sWcnt;
}

// The wide class: persistent single-wave blocks striding over (batch, slot of the batch's wide list); a slot beyond the
// batch's count costs one load.  stats (validate mode): tasks and Laguerre iterations with the other classes', the class's
// own count at stats[20 + QD_GS_WBIN].
template <bool VALIDATE>
__global__ void __launch_bounds__(64)
qd_k_full_solve_wide(unsigned char* __restrict__ slabs, QdWide wide, unsigned batches, unsigned long long* __restrict__ stats) {
    __shared__ QdEigWaveWs W;
    const size_t slab_bytes = qd_gs_slab_bytes(VALIDATE);
    const size_t total = (size_t)batches * wide.capw;
    for (size_t t = blockIdx.x; t < total; t += gridDim.x) {
        const size_t batch = t / wide.capw;
        const unsigned j = (unsigned)(t - batch * wide.capw);
        const QdSlab sl = qd_gs_slab(slabs + batch * slab_bytes, VALIDATE);
        if (j >= sl.cnt[QD_GS_WBIN]) continue;                           // uniform for the wave
        double* rec = sl.pool + qd_wide_list(wide, batch)[j];
        const int s = (int)rec[1];
        double lam, resid;
        int its = 0;
        qd_eig_wave_lowest<VALIDATE>(W, rec + 2, s, lam, resid, rec + 2, VALIDATE ? &its : nullptr);
        if (threadIdx.x == 0) {
            qd_wide_lam(wide, batch)[j] = lam;
            if (VALIDATE) {
                rec[1] = resid;
                if (stats) {
                    atomicAdd(&stats[16], 1ull); atomicAdd(&stats[17], (unsigned long long)its);
                    atomicAdd(&stats[20 + QD_GS_WBIN], 1ull);
                }
            }
        }
    }
}

// end of qd_k_full_select for pixel gp = (env, channel, pixel), the same operations as the end of qd_k_gs_select (kept inline
// there: the K-state kernels stay instruction for instruction as they were): the sensor constant c0, the occupations and
// (validate mode) the eigenpair's energy and residual
template <int N, bool VALIDATE>
__device__ __forceinline__ void qd_gs_emit(const double* __restrict__ par, const QdLayout& L, const QdPixelRec* __restrict__ rec,
                                           size_t gp, const double* occ, double lam, double resid, double* __restrict__ zraw,
                                           double* __restrict__ occ_out, double* __restrict__ eig_out) {
    constexpr int G = N + 1;
    double b = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) b = fma(par[L.cdd_inv + N * G + i], occ[i] - rec->vpp[i], b);
    const double vs = rec->vpp[N];
    const double Ns = rint(vs);                                 // np.round: half to even
    zraw[gp] = 2.0 * b + par[L.cdd_inv + N * G + N] * (2.0 * (Ns - vs) + 1.0);
    if (occ_out) {
#pragma unroll
        for (int i = 0; i < N; ++i) occ_out[gp * N + i] = occ[i];
    }
    if (VALIDATE && eig_out) { eig_out[gp * 2] = lam; eig_out[gp * 2 + 1] = resid; }
}

// grid = batches, one pixel per lane
template <int N, bool VALIDATE, bool WIDE>
__global__ void __launch_bounds__(QD_GS_BLOCK)
qd_k_full_select(const int* __restrict__ env_ids, int env_base, int rec_slot0, QdGsGeom g, int ppb, const double* __restrict__ params,
                 const QdPixelRec* __restrict__ recs, double* __restrict__ zraw, double* __restrict__ occ_out,
                 const double* __restrict__ state, int noise_flags, double* __restrict__ eig_out, const QdFullTab* __restrict__ tab,
                 unsigned char* __restrict__ slabs, QdWide wide) {
    const QdLayout L = qd_layout(N);
    const int batch = blockIdx.x;
    const QdSlab sl = qd_gs_slab(slabs + (size_t)batch * qd_gs_slab_bytes(VALIDATE), VALIDATE);
    const int slot = batch / (g.C * g.nb);
    const int rem = batch - slot * g.C * g.nb;
    const int ch = rem / g.nb, p0 = (rem - ch * g.nb) * ppb;
    const int e = env_ids ? env_ids[env_base + slot] : env_base + slot;
    const double* par = params + (size_t)e * L.size;
    const double* st = state + (size_t)e * L.s_size;
    if (qd_radial_replaced(par, st, L, ch, noise_flags)) return;
    const double* wlam = WIDE ? qd_wide_lam(wide, (size_t)batch) : nullptr;
    const unsigned* wlist = WIDE ? qd_wide_list(wide, (size_t)batch) : nullptr;
    const int ps = threadIdx.x, p = p0 + ps;
    if (ps >= ppb || p >= g.P) return;
    const QdPixelRec* rec = recs + ((size_t)(rec_slot0 + slot) * g.C + ch) * g.P + p;
    const int M = tab->M;
    // the lowest component: its leader (rank 0) carries the task's list position, or marks an isolated state
    double best = INFINITY; unsigned bestkey = 0xFFFFFFFFu, wl = QD_LINK_NONE; int wpos = 0;
    for (int pos = 0; pos < M; ++pos) {
        const unsigned lk = sl.link[pos * ppb + ps];
        if (lk == QD_LINK_NONE || sl.rank[pos * ppb + ps] != 0) continue;
        double lam;
        if (WIDE && lk >= QD_LINK_WIDE0 && lk < QD_LINK_SINGLE) lam = wlam[lk - QD_LINK_WIDE0];
        else lam = lk == QD_LINK_SINGLE ? 0.0 : sl.lam[lk];
        const unsigned key = tab->idx[pos];
        if ((lam < best) | ((lam == best) & (key < bestkey))) { best = lam; bestkey = key; wl = lk; wpos = pos; }
    }
    const bool wtask = wl < QD_LINK_SINGLE;
    unsigned woff = 0u;
    if (WIDE && wtask && wl >= QD_LINK_WIDE0) woff = wlist[wl - QD_LINK_WIDE0];
    else woff = wtask ? sl.lists[wl] : 0u;
    double occ[N];
#pragma unroll
    for (int i = 0; i < N; ++i) occ[i] = 0.0;
    const int q = tab->sec[wpos];
    for (int pos = tab->sec_start[q]; pos < tab->sec_start[q + 1]; ++pos) {
        const bool member = wtask ? sl.link[pos * ppb + ps] == wl : pos == wpos;
        if (!member) continue;
        const double x = wtask ? sl.pool[woff + 2 + sl.rank[pos * ppb + ps]] : 1.0;
        const double pr = x * x;
        const unsigned dg = tab->dig[pos];
#pragma unroll
        for (int i = 0; i < N; ++i) occ[i] = fma(pr, (double)((dg >> (4 * i)) & 15u), occ[i]);
    }
    double lam = best, resid = 0.0;
    if (VALIDATE) {
        const double hn = sl.aux[ps];
        lam = best + sl.aux[QD_GS_PPB + ps];
        if (wtask) resid = sl.pool[woff + 1] / (hn > 0.0 ? hn : 1.0);
    }
    qd_gs_emit<N, VALIDATE>(par, L, rec, ((size_t)e * g.C + ch) * g.P + p, occ, lam, resid, zraw, occ_out, eig_out);
}

#endif  // __HIPCC__
