// qd_levels_blocks.h -- the energy levels of a point, PER HOP COMPONENT (qd_scan_grid_levels): the contract of qd_levels_solve
// (qd_levels.h) -- the lower triangle of the block in the workspace, 1 <= s <= 32, 1 <= L <= QD_LEVELS_MAX -> lev[0 .. min(L, s) - 1],
// increasing and counted with multiplicity -- by a Householder tridiagonalisation that never leaves the connected components of
// the coupling pattern.  States of different components do not couple, so H is block diagonal up to a permutation, and the
// tridiagonals of the components, laid side by side with a zero off-diagonal between them, are a tridiagonal matrix with the
// spectrum of H.  qd_levels_solve reflects s - 2 columns of the whole block, each a chain of barriers; here the components
// reflect CONCURRENTLY, max_c s_c - 2 steps, and the loops inside a step run over the members of one component.
//
//   1. step 1 of qd_levels_solve as it is: shift by the lowest diagonal entry, ONE power-of-two scale of the whole block to
//      ||A||_inf in [1, 2): the fixed rounds, pivmin and the 1e-12 ||H||_inf bar are on that global scale.  In the pass that sums
//      the rows lane i also collects the neighbour mask of state i from the UNSCALED entries: bit j set iff A_ij != 0.  Exact
//      zeros do not link; a denormal coupling links, whether or not the scaling flushes it.
//   2. components: the closure of the reach masks (qd_thermal_blocks.h, step 2).  The label of a component is its lowest state,
//      the members are ordered by (label, index); per state its component's offset in that list, its size and the state's
//      local index.  Local order is index order, so the entry (local a, local b), a > b, is in the stored lower triangle.
//   3. step r reflects local column r of EVERY component with at least r + 3 states.  Whether a component reflects is a
//      per-lane matter: the work is predicated, the barriers are not.  All sums of a component (the norm of the column tail,
//      B v, p.v) are taken by each of its lanes for itself over the component's members in index order, read from the
//      workspace: the lanes of a component agree bitwise, and two components with the same entries in the same local places
//      get the same tridiagonal bit for bit.  The members are walked through the component's mask (ctz and clear: no list
//      read in the inner loops); mc[i] is the mask of the members of local index >= r, advanced by every lane for its own
//      state.  Guards of qd_levels_solve: tails below 1e-200 in the square or below 1e-34 x0^2 are dropped, not reflected.
//      Component c writes al, be at off_c .. off_c + s_c - 1; be at its LAST position is exactly 0, for components of one
//      and two states too.  Entries of A between different components are never written after step 1.
//   4. the multisection of qd_levels_solve, step 3, on the concatenated al, be, b2 with the same fixed rounds: with b2 = 0 the
//      recurrence restarts at a component boundary and the counts add.  Equal levels, across components too, see the same
//      counts at the same shifts and come back bitwise equal.  (The step is a copy: the kernels of qd_levels.h stay as built.)
//      A block WITHOUT A COUPLING (every component one state; all tc = 0) skips it: its levels are its diagonal entries as
//      given, sorted by rank, exactly.
// Everything a second point could inherit (masks, member list, per-state bytes, t, al, be, b2) is written for the current
// point before it is read.
//
// The same source compiles for the host through the lane macros of qd_eig_wave.h; tests/hosttest_levels_blocks checks it
// against numpy.linalg.eigvalsh without a GPU.
//
// LDS: the embedded QdLevelsWs (12 864 B; its x doubles as the per-state t of a step), the masks ma, mb, mc (384 B) and 128 B
// of byte arrays: sizeof(QdLevelsBlocksWs) = 13 376 B, twelve single-wave blocks per CU as qd_k_levels (163 840 / 12 = 13 653).
// No permuted copy of the block.  qd_k_levels_grid<8, QdLevelsBlocksWs> for gfx950: 72 VGPRs, 106 SGPRs, no spill, no scratch (the
// compiler's resource report, -Rpass-analysis=kernel-resource-usage; the two short loops over the masks are kept rolled: unrolled
// by 16 they cost two SGPR spills); the LDS, not the registers, bounds the waves per SIMD.
#pragma once
#include "qd_levels.h"

struct QdLevelsBlocksWs {
    QdLevelsWs L;                           // L.A: the block; L.al, L.be, L.b2: the concatenated tridiagonal; L.lev: the result
    unsigned ma[32], mb[32];                // reach masks of the states, double buffered; the closure in both afterwards
    unsigned mc[32];                        // per state: the members of its component from the step's column on
    unsigned char mem[32];                  // the states ordered by (label, index)
    unsigned char st_off[32], st_sz[32], st_li[32];     // per state: offset and size of its component, its local index
};

static_assert(sizeof(QdLevelsBlocksWs) == 13376, "the header comment states the size");
static_assert(sizeof(QdLevelsBlocksWs) <= 13648, "twelve single-wave blocks per CU");

#define QD_LB_A(i, j) T.A[(i) * QD_LV_LD + (j)]

// The lower triangle of W.L.A (rows 0 .. s-1, 1 <= s <= 32; destroyed) -> W.L.lev[0 .. min(L, s) - 1], the lowest eigenvalues in
// increasing order and in the units of the input, valid in every lane after the call; W.ma[i]: the states of the component
// of state i, as a mask.  1 <= L <= QD_LEVELS_MAX.
QD_HD void qd_levels_blocks_solve(QdLevelsBlocksWs& W, int s, int L) {
    QdLevelsWs& T = W.L;
    if (s == 1) {                                             // (uniform) one state: its energy, exactly
        const double a = QD_LB_A(0, 0);
        if (QD_EW_LANE0) { T.lev[0] = a; W.ma[0] = 1u; }
        QD_EW_SYNC();
        return;
    }
    // ---- 1. shift by the lowest diagonal entry, scale; the neighbour masks ----
    QD_EW_EACH(i) {
        const double d = i < s ? QD_LB_A(i, i) : INFINITY;
        T.w[i] = d;                                           // (the diagonal as given, for the block without a coupling below)
        T.red[i] = -d;
    }
    const double dmin = -qd_ew_max(T.red);
    QD_EW_EACH(i) { if (i < s) QD_LB_A(i, i) -= dmin; }
    QD_EW_SYNC();
    QD_EW_EACH(i) {
        double rs = 0.0;
        if (i < s) {
            unsigned nb = 1u << i;
            for (int j = 0; j < s; ++j) {
                const double a = j <= i ? QD_LB_A(i, j) : QD_LB_A(j, i);
                rs += fabs(a);
                if (a != 0.0) nb |= 1u << j;
            }
            W.ma[i] = nb;
        }
        T.red[i] = rs;
    }
    const double anorm = qd_ew_max(T.red);
    double tsc, tusc;
    qd_pow2_scale(anorm, tsc, tusc);
    QD_EW_EACH(i) {
        if (i < s)
            for (int j = 0; j <= i; ++j) QD_LB_A(i, j) *= tsc;
    }
    // ---- 2. components: the closure of the reach masks (the masks of pass n in ma for even n, mb for odd n) ----
    bool in_a = true;
    for (;;) {
        QD_EW_EACH(i) {
            double ch = 0.0;
            if (i < s) {
                const unsigned* src = in_a ? W.ma : W.mb;
                const unsigned m0 = src[i];
                unsigned m = m0;
                for (unsigned rest = m0; rest; rest &= rest - 1) m |= src[__builtin_ctz(rest)];
                (in_a ? W.mb : W.ma)[i] = m;
                if (m != m0) ch = 1.0;
            }
            T.red[i] = ch;
        }
        const bool more = qd_ew_max(T.red) != 0.0;            // (its barriers order the two buffers)
        in_a = !in_a;
        if (!more) break;                                     // (no mask changed: ma and mb hold the same closure)
    }
    int maxsz = 1;                                            // (uniform: every lane reads the same masks) max_c s_c
#pragma unroll 1
    for (int j = 0; j < s; ++j) {
        const int sz = __builtin_popcount(W.ma[j]);
        if (sz > maxsz) maxsz = sz;
    }
    const int steps = maxsz > 2 ? maxsz - 2 : 0;
    QD_EW_EACH(i) {
        if (i < s) {
            const unsigned mi = W.ma[i];
            const int lab = __builtin_ctz(mi), sz = __builtin_popcount(mi), li = __builtin_popcount(mi & ((1u << i) - 1u));
            int off = 0;
#pragma unroll 1
            for (int j = 0; j < lab; ++j) {                   // the components with a lower label
                const unsigned mj = W.ma[j];
                if (__builtin_ctz(mj) == j) off += __builtin_popcount(mj);
            }
            W.mem[off + li] = (unsigned char)i;
            W.st_off[i] = (unsigned char)off; W.st_sz[i] = (unsigned char)sz; W.st_li[i] = (unsigned char)li;
            W.mc[i] = mi;
        }
    }
    QD_EW_SYNC();
    // ---- 3. Householder, all components at once: step r reflects local column r of the components of >= r + 3 states ----
    for (int r = 0; r < steps; ++r) {
        // a. the squares of the column tails (local index >= r + 2)
        QD_EW_EACH(i) {
            double sq = 0.0;
            const unsigned cm = i < s ? W.mc[i] : 0u, t1 = cm & (cm - 1), t2 = t1 & (t1 - 1);
            if ((t2 >> (i & 31)) & 1u) {                      // (i is a member behind the sub-diagonal: its component reflects)
                const double xi = QD_LB_A(i, __builtin_ctz(cm));
                sq = xi * xi;
            }
            T.red[i] = sq;
        }
        QD_EW_SYNC();
        // b. the reflector, by every lane of the trailing block (local index >= r + 1) for itself; v and t per state
        QD_EW_EACH(i) {
            {
                const unsigned cm = i < s ? W.mc[i] : 0u, t1 = cm & (cm - 1), t2 = t1 & (t1 - 1);
                if (t2 != 0u && ((t1 >> (i & 31)) & 1u)) {    // (>= 3 members left, and i is behind the column)
                    const int col = __builtin_ctz(cm), k1 = __builtin_ctz(t1);
                    double sigma = 0.0;
                    for (unsigned rest = t2; rest; rest &= rest - 1) sigma += T.red[__builtin_ctz(rest)];
                    const double x0 = QD_LB_A(k1, col);
                    const bool refl = (sigma > 1e-200) & (sigma > 1e-34 * x0 * x0);   // (see qd_eig_lowest)
                    const double mu = qd_sqrt1(fma(x0, x0, sigma) + 1e-300);
                    const double v0 = (x0 <= 0.0) ? x0 - mu : -sigma * qd_rcp(x0 + mu);
                    const double v0sq = v0 * v0;
                    const double t = refl ? 2.0 * v0sq * qd_rcp(sigma + v0sq) : 0.0;
                    const double iv0 = refl ? qd_rcp(v0) : 0.0;
                    T.v[i] = i == k1 ? 1.0 : QD_LB_A(i, col) * iv0;
                    T.x[i] = t;
                    if (i == k1) {
                        const int pos = W.st_off[i] + r;
                        T.be[pos] = refl ? mu : x0; T.al[pos] = QD_LB_A(col, col);
                    }
                }
            }
        }
        QD_EW_SYNC();
        // c. trailing block B of the component:  p = t B v
        QD_EW_EACH(i) {
            {
                const unsigned cm = i < s ? W.mc[i] : 0u, t1 = cm & (cm - 1), t2 = t1 & (t1 - 1);
                if (t2 != 0u && ((t1 >> (i & 31)) & 1u) && T.x[i] != 0.0) {            // (t = 0: the update changes nothing)
                    double acc = 0.0;
                    for (unsigned rest = t1; rest; rest &= rest - 1) {
                        const int j = __builtin_ctz(rest);
                        acc = fma(j <= i ? QD_LB_A(i, j) : QD_LB_A(j, i), T.v[j], acc);
                    }
                    const double p = T.x[i] * acc;
                    T.w[i] = p;
                    T.red[i] = p * T.v[i];
                }
            }
        }
        QD_EW_SYNC();
        // d. K = t/2 p.v,  w = p - K v
        QD_EW_EACH(i) {
            {
                const unsigned cm = i < s ? W.mc[i] : 0u, t1 = cm & (cm - 1), t2 = t1 & (t1 - 1);
                if (t2 != 0u && ((t1 >> (i & 31)) & 1u) && T.x[i] != 0.0) {
                    double pv = 0.0;
                    for (unsigned rest = t1; rest; rest &= rest - 1) pv += T.red[__builtin_ctz(rest)];
                    T.w[i] = fma(-(0.5 * T.x[i] * pv), T.v[i], T.w[i]);
                }
            }
        }
        QD_EW_SYNC();
        // e. B -= v w^T + w v^T, row i up to the diagonal; the column leaves the component's mask
        QD_EW_EACH(i) {
            {
                const unsigned cm = i < s ? W.mc[i] : 0u, t1 = cm & (cm - 1), t2 = t1 & (t1 - 1);
                if (t2 != 0u && ((t1 >> (i & 31)) & 1u) && T.x[i] != 0.0) {
                    const double vi = T.v[i], wi = T.w[i];
                    for (unsigned rest = t1 & ((2u << i) - 1u); rest; rest &= rest - 1) {
                        const int j = __builtin_ctz(rest);
                        QD_LB_A(i, j) = fma(-vi, T.w[j], fma(-wi, T.v[j], QD_LB_A(i, j)));
                    }
                }
                if (t2 != 0u) W.mc[i] = t1;                         // (a component of two members left stays: its tail is read below)
            }
        }
        QD_EW_SYNC();
    }
    // the last two positions of every component; be at the last one is exactly zero
    QD_EW_EACH(i) {
        if (i < s) {
            const unsigned mi = W.ma[i];
            const int sz = W.st_sz[i], li = W.st_li[i], pos = W.st_off[i] + li;
            if (li >= sz - 2) {
                T.al[pos] = QD_LB_A(i, i);
                T.be[pos] = li == sz - 1 ? 0.0 : QD_LB_A(31 - __builtin_clz(mi), i);
            }
        }
    }
    QD_EW_SYNC();
    if (maxsz == 1) {
        // (uniform) every component is one state: the block is diagonal and its levels are its diagonal entries AS GIVEN, sorted,
        // exactly -- neither the shift nor a bracket's midpoint rounds them.  Lane i ranks its entry (ties by index) and writes it.
        QD_EW_EACH(i) {
            if (i < s) {
                const double d = T.w[i];
                int rank = 0;
                for (int j = 0; j < s; ++j) {
                    const double e = T.w[j];
                    rank += (e < d) | ((e == d) & (j < i)) ? 1 : 0;
                }
                if (rank < L) T.lev[rank] = d;
            }
        }
        QD_EW_SYNC();
        return;
    }
    // ---- 4. multisection of the concatenated T (qd_levels_solve, step 3) ----
    double gl = INFINITY, gu = -INFINITY, tscale = 0.0;
    for (int i = 0; i < s; ++i) {
        const double b = T.be[i];
        const double rad = (i > 0 ? fabs(T.be[i - 1]) : 0.0) + fabs(b);
        gl = fmin(gl, T.al[i] - rad);
        gu = fmax(gu, T.al[i] + rad);
        tscale = fmax(tscale, fabs(T.al[i]) + rad);
        if (QD_EW_LANE0) T.b2[i] = b * b;
    }
    QD_EW_SYNC();
    const double pivmin = 0x1p-1020;                          // (dstebz: safemin max(1, max b^2); ||T|| < 2, so b^2 / pivmin stays finite)
    const double fudge = 1e-14 * tscale + 2.0 * pivmin;
    gl -= fudge; gu += fudge;
    const int Le = L < s ? L : s;
    const int P = 64 / Le;
    const int rounds = qd_levels_rounds(P);
    const double step = 1.0 / (double)(P + 1);
    QD_EW_EACH(l) { T.lo[l] = gl; T.hi[l] = gu; }
    for (int r = 0; r < rounds; ++r) {
        QD_EW_EACH(l) {
            const int k = l / P, j = l - k * P;
            const double lo = T.lo[l], hi = T.hi[l];
            const double x = fma(hi - lo, (double)(j + 1) * step, lo);
            double q = T.al[0] - x;
            if (fabs(q) < pivmin) q = -pivmin;
            int c = q < 0.0 ? 1 : 0;
            for (int i = 1; i < s; ++i) {
                q = (T.al[i] - x) - T.b2[i - 1] / q;
                if (fabs(q) < pivmin) q = -pivmin;
                c += q < 0.0 ? 1 : 0;
            }
            T.x[l] = x; T.cnt[l] = c;
        }
        QD_EW_SYNC();
        // the cell of level k: behind the last shift with N <= k (every lane of the level finds it for itself: broadcast reads)
        QD_EW_EACH(l) {
            const int k = l / P, b = k * P;
            if (k < Le) {
                int jl = -1;
                for (int j = 0; j < P; ++j) if (T.cnt[b + j] <= k) jl = j;
                if (jl >= 0) T.lo[l] = T.x[b + jl];
                if (jl + 1 < P) T.hi[l] = T.x[b + jl + 1];
            }
        }
        QD_EW_SYNC();
    }
    // midpoints, unscaled and shifted back; a running maximum keeps levels whose brackets overlap in order
    {
        double prev = -INFINITY;
        for (int k = 0; k < Le; ++k) {
            const double lo = T.lo[k * P], hi = T.hi[k * P];
            const double lam = fmax(prev, dmin + fma(0.5, hi - lo, lo) * tusc);
            if (QD_EW_LANE0) T.lev[k] = lam;
            prev = lam;
        }
    }
    QD_EW_SYNC();
}

#if defined(__HIPCC__)
#include "qd_grid.h"            // qd_query_live (qd_query.h)

#define QD_LVG_BLOCKS 4096      // blocks per slot at the most; the blocks of a slot stride over its points

// the two cores behind one kernel body: the per-component one on its workspace, qd_levels_solve on a bare QdLevelsWs
__device__ __forceinline__ QdLevelsWs& qd_lvg_state(QdLevelsBlocksWs& W) { return W.L; }
__device__ __forceinline__ QdLevelsWs& qd_lvg_state(QdLevelsWs& W) { return W; }
__device__ __forceinline__ void qd_lvg_solve(QdLevelsBlocksWs& W, int s, int L) { qd_levels_blocks_solve(W, s, L); }
__device__ __forceinline__ void qd_lvg_solve(QdLevelsWs& W, int s, int L) { qd_levels_solve(W, s, L); }

// ---------------------------------------------------------------------------------------------------------------
// The levels of the live records of a grid launch, one point per wavefront, behind the search and before the ground-state stage:
// blocks of ONE wave, grid = (min(n, QD_LVG_BLOCKS), slots).  WS = QdLevelsBlocksWs: the per-component core, the open regime's.
// WS = QdLevelsWs: qd_levels_solve on the whole block, the closed regime's -- a closed list is ONE total-charge sector, whose
// states hops connect: one component, nothing to skip.  Point p < n = nx*ny of slot k (query q = base + k, SP records per
// slot): reads the record, runs qd_levels_record -> the core, and lane 0 writes levels_dst[(q n + p) L + i] (+inf from nv on)
// and hnorm_dst[q n + p] (may be null) of the caller's rows.  Nothing else is written: the records and the slots stay as the
// search left them.  A query that is not live writes nothing at all (its block returns at once); the inert records n .. SP-1
// are never read.
// ---------------------------------------------------------------------------------------------------------------
template <int N, class WS>
__global__ void __launch_bounds__(64)
qd_k_levels_grid(const int* __restrict__ env_of_query, int base, int B, int n, int SP, int kept, int L,
                 const QdPixelRec* __restrict__ recs, double* __restrict__ levels_dst, double* __restrict__ hnorm_dst) {
    __shared__ WS W;
    QdLevelsWs& T = qd_lvg_state(W);
    const int k = blockIdx.y, q = base + k;
    if (!qd_query_live(env_of_query, nullptr, q, B, N)) return;           // (uniform over the block)
    for (int p = blockIdx.x; p < n; p += gridDim.x) {
        const QdPixelRec* rec = recs + (size_t)k * SP + p;
        const size_t dst = (size_t)q * n + p;
        int nv = rec->nvalid < kept ? rec->nvalid : kept;
        nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
        nv = __builtin_amdgcn_readfirstlane(nv);
        double hn = 0.0;
        if (nv > 0) {
            hn = qd_levels_record<N>(T, rec, nv);
            qd_lvg_solve(W, nv, L);
        }
        if (threadIdx.x == 0) {
            for (int i = 0; i < L; ++i) levels_dst[dst * (size_t)L + i] = i < nv ? T.lev[i] : INFINITY;
            if (hnorm_dst) hnorm_dst[dst] = hn;
        }
        __syncthreads();                                   // (lane 0 has read W.lev before the next point overwrites it)
    }
}
#endif  // __HIPCC__

#undef QD_LB_A
