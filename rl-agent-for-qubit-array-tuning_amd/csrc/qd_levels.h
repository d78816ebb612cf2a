// qd_levels.h -- energy levels of a point (qd_eval_points_ex): the L lowest eigenvalues, L <= QD_LEVELS_MAX, and the infinity
// norm of the Hamiltonian H = diag(E_0 .. E_{nv-1}) + H_t over the nv = min(nvalid, K) valid kept states of a QdPixelRec.
// That is the reference's matrix of hamiltonian_build.py:75-137 with the |0..0> padding copies left out (they are always
// isolated and would only add copies of one diagonal entry); E is the search's canonical energy, absolute.  The ground-state
// stage (qd_groundstate.h) solves the lowest eigenpair of the components that can hold the ground state and prunes the rest,
// so the excited levels are nowhere in it: this file works on the whole block, ONE POINT PER WAVEFRONT.
//
//   1. the diagonal is shifted by its minimum (the common offset, |E| ~ 1e3 .. 1e5 against spreads of O(1), would cost
//      eps |E| in every subtraction) and the block scaled by a power of two to ||A||_inf in [1, 2) (qd_pow2_scale)
//   2. Householder tridiagonalisation, the reflector step of qd_eig_wave.h with its guards (column tails below 1e-100 or
//      below 1e-17 |x0| are dropped instead of reflected); no reflector is kept, there is no eigenvector to carry back
//   3. Sturm-count multisection of T.  N(x) = #{eigenvalues < x} is the number of negative q_i of the dstebz recurrence
//      q_0 = a_0 - x, q_i = (a_i - x) - b_{i-1}^2 / q_{i-1}, with |q| < pivmin replaced by -pivmin: s <= 32 serial steps per
//      lane and no cross-lane traffic inside them.  Level k keeps a bracket [lo_k, hi_k] with N(lo_k) <= k < N(hi_k); all
//      brackets start as the Gershgorin interval of T and shrink together: the 64 lanes are split between the Le = min(L, s)
//      wanted levels, P = 64 / Le lanes each, lane j of level k counts at lo_k + (hi_k - lo_k) (j + 1) / (P + 1), and the
//      bracket becomes the cell between the last shift with N <= k and the next one: a (P + 1)-section per round.
//      ROUNDS ARE FIXED (qd_levels_rounds): the Gershgorin interval of a matrix with ||A||_inf < 2 is at most 2^2 wide, the
//      midpoint of the final bracket is to be within 2^-54 (half an ulp of a value in [1, 2), 53 bits) with 2 guard bits, so
//      the width has to fall by 2^58: the smallest r with (P + 1)^r >= 2^58 -- 10 rounds of 65-section for one level, 12 for
//      two (33-section), 19 for eight (9-section).  No loop in here depends on the data.
//      Counts make clusters and exact degeneracies harmless: levels k and k + 1 of a double eigenvalue see the same counts
//      at the same shifts in every round, keep the same bracket and come back bitwise equal.  (Laguerre with deflation, the
//      choice of the lowest-eigenpair solvers, is neither robust at clusters nor lane-parallel.)
//
// The same source compiles for the host in the manner of qd_eig_wave.h, whose lane macros it uses: code outside QD_EW_EACH is
// wave-uniform, code inside runs per lane, whatever crosses lanes goes through the workspace with QD_EW_SYNC in between.
// tests/hosttest_levels checks it against numpy.linalg.eigvalsh without a GPU.
//
// LDS: the block is stored at an odd row stride of 33 doubles (row-wise and column-wise ds_read_b64 of the lanes fall on
// different banks), 8 448 B; beside it three 64-double vectors (v, w, red: the host loop of qd_eig_wave.h's reductions reads 64
// entries), al, be, b2 of 32, the per-lane brackets, shifts and counts, and the state codes: sizeof(QdLevelsWs) = 12 864 B,
// twelve single-wave blocks per CU (160 KB of LDS).
#pragma once
#include "qd_eig_wave.h"        // the lane macros, qd_ew_sum, qd_ew_max; qd_eig.h: qd_pow2_scale, qd_sqrt1, qd_rcp
#include "qd_groundstate.h"     // qd_gs_hop

#ifndef QD_LEVELS_MAX
#define QD_LEVELS_MAX 8         // (qdsim.h)
#endif
#define QD_LV_MAX 32            // states of a block, at most: QD_K
#define QD_LV_LD 33             // row stride of the block in the workspace

struct QdLevelsWs {
    double A[QD_LV_MAX * QD_LV_LD];
    double v[64], w[64], red[64];
    double al[QD_LV_MAX], be[QD_LV_MAX], b2[QD_LV_MAX];
    double lo[64], hi[64], x[64];       // per lane: the bracket of its level and its shift of the round
    int cnt[64];                        // per lane: N(x)
    unsigned code[64];                  // per state: its delta code, one digit per nibble (qd_gs_hop)
    double lev[QD_LEVELS_MAX];          // the result
};

// rounds of (P + 1)-section that shrink a bracket by 2^58 (see above); P = 64 / Le
QD_HD constexpr int qd_levels_rounds(int P) {
    int r = 0;
    for (double f = 1.0; f < 0x1p58; f *= (double)(P + 1)) ++r;
    return r;
}
static_assert(qd_levels_rounds(64) == 10 && qd_levels_rounds(32) == 12 && qd_levels_rounds(8) == 19, "65-, 33- and 9-section to 2^-58");

#define QD_LV_A(i, j) W.A[(i) * QD_LV_LD + (j)]

// the packed lower triangle Ain (s (s + 1) / 2 doubles, row-major) into the workspace
QD_HD void qd_levels_load_packed(QdLevelsWs& W, const double* Ain, int s) {
    QD_EW_EACH(l) {
        for (int r = 0; r < s; ++r)
            if (l <= r) QD_LV_A(r, l) = Ain[r * (r + 1) / 2 + l];
    }
    QD_EW_SYNC();
}

// The lower triangle of W.A (rows 0 .. s-1, 1 <= s <= 32; destroyed) -> W.lev[0 .. min(L, s) - 1], the lowest eigenvalues in
// increasing order and in the units of the input, valid in every lane after the call.  1 <= L <= QD_LEVELS_MAX.
QD_HD void qd_levels_solve(QdLevelsWs& W, int s, int L) {
    if (s == 1) {                                             // (uniform) one state: its energy, exactly
        const double a = QD_LV_A(0, 0);
        if (QD_EW_LANE0) W.lev[0] = a;
        QD_EW_SYNC();
        return;
    }
    // ---- 1. shift by the lowest diagonal entry, scale ----
    QD_EW_EACH(i) { W.red[i] = i < s ? -QD_LV_A(i, i) : -INFINITY; }
    const double dmin = -qd_ew_max(W.red);
    QD_EW_EACH(i) { if (i < s) QD_LV_A(i, i) -= dmin; }
    QD_EW_SYNC();
    QD_EW_EACH(i) {
        double rs = 0.0;
        if (i < s)
            for (int j = 0; j < s; ++j) rs += fabs(j <= i ? QD_LV_A(i, j) : QD_LV_A(j, i));
        W.red[i] = rs;
    }
    const double anorm = qd_ew_max(W.red);
    double tsc, tusc;
    qd_pow2_scale(anorm, tsc, tusc);
    QD_EW_EACH(i) {
        if (i < s)
            for (int j = 0; j <= i; ++j) QD_LV_A(i, j) *= tsc;
    }
    QD_EW_SYNC();
    // ---- 2. Householder: reflector k zeroes column k below the sub-diagonal (qd_eig_wave_lowest, step 2) ----
    for (int k = 0; k + 2 < s; ++k) {
        QD_EW_EACH(i) {
            const double xi = (i >= k + 2 && i < s) ? QD_LV_A(i, k) : 0.0;
            W.red[i] = xi * xi;
        }
        const double sigma = qd_ew_sum(W.red);
        const double x0 = QD_LV_A(k + 1, k);
        const bool refl = (sigma > 1e-200) & (sigma > 1e-34 * x0 * x0);   // (see qd_eig_lowest)
        const double mu = qd_sqrt1(fma(x0, x0, sigma) + 1e-300);
        const double v0 = (x0 <= 0.0) ? x0 - mu : -sigma * qd_rcp(x0 + mu);
        const double v0sq = v0 * v0;
        const double t = refl ? 2.0 * v0sq * qd_rcp(sigma + v0sq) : 0.0;
        const double iv0 = refl ? qd_rcp(v0) : 0.0;
        const double akk = QD_LV_A(k, k);
        QD_EW_EACH(i) {
            double vi = 0.0;
            if (i == k + 1) vi = 1.0;
            else if (i >= k + 2 && i < s) vi = QD_LV_A(i, k) * iv0;
            W.v[i] = vi;
        }
        if (QD_EW_LANE0) { W.be[k] = refl ? mu : x0; W.al[k] = akk; }
        QD_EW_SYNC();
        if (!refl) continue;                                              // (t = 0: the update changes nothing)
        // trailing block B = A[k+1.., k+1..]:  p = t B v,  K = t/2 p.v,  w = p - K v,  B -= v w^T + w v^T
        QD_EW_EACH(i) {
            double p = 0.0;
            if (i >= k + 1 && i < s) {
                double acc = 0.0;
                for (int j = k + 1; j < s; ++j) acc = fma(j <= i ? QD_LV_A(i, j) : QD_LV_A(j, i), W.v[j], acc);
                p = t * acc;
            }
            W.w[i] = p;
            W.red[i] = p * W.v[i];
        }
        const double K = 0.5 * t * qd_ew_sum(W.red);
        QD_EW_EACH(i) { W.w[i] = fma(-K, W.v[i], W.w[i]); }
        QD_EW_SYNC();
        QD_EW_EACH(i) {
            if (i >= k + 1 && i < s) {
                const double vi = W.v[i], wi = W.w[i];
                for (int j = k + 1; j <= i; ++j) QD_LV_A(i, j) = fma(-vi, W.w[j], fma(-wi, W.v[j], QD_LV_A(i, j)));
            }
        }
        QD_EW_SYNC();
    }
    if (s >= 2) {
        const double a0 = QD_LV_A(s - 2, s - 2), b0 = QD_LV_A(s - 1, s - 2);
        if (QD_EW_LANE0) { W.al[s - 2] = a0; W.be[s - 2] = b0; }
    }
    {
        const double a1 = QD_LV_A(s - 1, s - 1);
        if (QD_EW_LANE0) { W.al[s - 1] = a1; W.be[s - 1] = 0.0; }
    }
    QD_EW_SYNC();
    // ---- 3. multisection of T ----
    // Gershgorin interval (wave-uniform; every lane runs the loop on the same T), widened so that N(gl) = 0 and N(gu) = s
    // also in floating point
    double gl = INFINITY, gu = -INFINITY, tscale = 0.0;
    for (int i = 0; i < s; ++i) {
        const double b = W.be[i];
        const double rad = (i > 0 ? fabs(W.be[i - 1]) : 0.0) + fabs(b);
        gl = fmin(gl, W.al[i] - rad);
        gu = fmax(gu, W.al[i] + rad);
        tscale = fmax(tscale, fabs(W.al[i]) + rad);
        if (QD_EW_LANE0) W.b2[i] = b * b;
    }
    QD_EW_SYNC();
    const double pivmin = 0x1p-1020;                          // (dstebz: safemin max(1, max b^2); ||T|| < 2, so b^2 / pivmin stays finite)
    const double fudge = 1e-14 * tscale + 2.0 * pivmin;
    gl -= fudge; gu += fudge;
    const int Le = L < s ? L : s;
    const int P = 64 / Le;
    const int rounds = qd_levels_rounds(P);
    const double step = 1.0 / (double)(P + 1);
    QD_EW_EACH(l) { W.lo[l] = gl; W.hi[l] = gu; }
    for (int r = 0; r < rounds; ++r) {
        QD_EW_EACH(l) {
            const int k = l / P, j = l - k * P;
            const double lo = W.lo[l], hi = W.hi[l];
            const double x = fma(hi - lo, (double)(j + 1) * step, lo);
            double q = W.al[0] - x;
            if (fabs(q) < pivmin) q = -pivmin;
            int c = q < 0.0 ? 1 : 0;
            for (int i = 1; i < s; ++i) {
                q = (W.al[i] - x) - W.b2[i - 1] / q;
                if (fabs(q) < pivmin) q = -pivmin;
                c += q < 0.0 ? 1 : 0;
            }
            W.x[l] = x; W.cnt[l] = c;
        }
        QD_EW_SYNC();
        // the cell of level k: behind the last shift with N <= k (every lane of the level finds it for itself: broadcast reads)
        QD_EW_EACH(l) {
            const int k = l / P, b = k * P;
            if (k < Le) {
                int jl = -1;
                for (int j = 0; j < P; ++j) if (W.cnt[b + j] <= k) jl = j;
                if (jl >= 0) W.lo[l] = W.x[b + jl];
                if (jl + 1 < P) W.hi[l] = W.x[b + jl + 1];
            }
        }
        QD_EW_SYNC();
    }
    // midpoints, unscaled and shifted back; a running maximum keeps levels whose brackets overlap in order
    {
        double prev = -INFINITY;
        for (int k = 0; k < Le; ++k) {
            const double lo = W.lo[k * P], hi = W.hi[k * P];
            const double lam = fmax(prev, dmin + fma(0.5, hi - lo, lo) * tusc);
            if (QD_EW_LANE0) W.lev[k] = lam;
            prev = lam;
        }
    }
    QD_EW_SYNC();
}

// ---------------------------------------------------------------------------------------------------------------
// The block of a record into the workspace: lane m < nv owns state m and row m of the lower triangle.  Hop test qd_gs_hop on the
// delta codes, coefficients H_ij = -tc_d sqrt(n_from (n_to + 1)) with the occupations fl + delta - 1 of the ROW state
// (qd_ground_structure, phase 2; pairs whose coupling is exactly zero do not link states), diagonal rec->E.  Returns
// ||H||_inf = max_i (|E_i| + sum_j |H_ij|), unshifted.  1 <= nv <= 32.
// ---------------------------------------------------------------------------------------------------------------
template <int N>
QD_HD double qd_levels_record(QdLevelsWs& W, const QdPixelRec* rec, int nv) {
    unsigned tcq = 0;                                     // bit 4q set iff pair N-2-q couples
#pragma unroll
    for (int q = 0; q < N - 1; ++q) {
        const double t = rec->tc[N - 2 - q];
        if (t != 0.0) tcq |= 1u << (4 * q);
    }
    QD_EW_EACH(m) {
        unsigned e = m < nv ? (unsigned)rec->idx[m] : 0u;
        e = (e | (e << 8)) & 0x00FF00FFu;
        e = (e | (e << 4)) & 0x0F0F0F0Fu;
        e = (e | (e << 2)) & 0x33333333u;
        W.code[m] = e;
    }
    QD_EW_SYNC();
    QD_EW_EACH(i) {
        if (i < nv) {
            const unsigned ci = W.code[i];
            for (int j = 0; j < i; ++j) {
                const unsigned cj = W.code[j];
                double c = 0.0;
                if (qd_gs_hop(ci, cj, tcq)) {
                    const int Y = (int)cj - (int)ci;
                    const unsigned ay = (unsigned)(Y < 0 ? -Y : Y);
                    const int q = __builtin_ctz(ay) >> 2;
                    const int d = N - 2 - q;               // adjacent pair (d, d+1)
                    const int nd = rec->fl[d] + (int)((ci >> (4 * (q + 1))) & 3u) - 1;
                    const int nd1 = rec->fl[d + 1] + (int)((ci >> (4 * q)) & 3u) - 1;
                    // Y < 0: s_j = s_i - e_d + e_{d+1}; else the other way.  (exact products in float64)
                    const double prod = (Y < 0) ? (double)nd * (double)(nd1 + 1) : (double)nd1 * (double)(nd + 1);
                    double sq_ = 0.0;
                    if (prod > 0.0) sq_ = qd_sqrt1(prod);
                    c = -rec->tc[d] * sq_;
                }
                QD_LV_A(i, j) = c;
            }
            QD_LV_A(i, i) = rec->E[i];
        }
    }
    QD_EW_SYNC();
    QD_EW_EACH(i) {
        double rs = -INFINITY;
        if (i < nv) {
            rs = 0.0;
            for (int j = 0; j < nv; ++j) rs += fabs(j <= i ? QD_LV_A(i, j) : QD_LV_A(j, i));
        }
        W.red[i] = rs;
    }
    return qd_ew_max(W.red);
}

#if defined(__HIPCC__)
#include "qd_points.h"          // QdPointSlots

// ---------------------------------------------------------------------------------------------------------------
// Levels of the live records of a point launch, one point per wavefront.  Blocks of ONE wave (the barriers of the core are
// then wave barriers plus the LDS fence, as in qd_k_full_solve_wide), grid = (blocks, slots): the blocks of slot k stride over
// its T.cnt[k] points; the inert records behind them (qd_k_points_front) are never read.  Reads the record only.  Lane 0
// writes levels_dst[q * L + k] (+inf from nv on) and hnorm_dst[q] for point q = T.start[k] + j.
// ---------------------------------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(64)
qd_k_levels(QdPointSlots T, int CP, int kept, int L, const QdPixelRec* __restrict__ recs, double* __restrict__ levels_dst,
            double* __restrict__ hnorm_dst) {
    __shared__ QdLevelsWs W;
    const int k = blockIdx.y;
    const int cnt = T.cnt[k] < CP ? T.cnt[k] : CP;
    for (int j = blockIdx.x; j < cnt; j += gridDim.x) {
        const QdPixelRec* rec = recs + (size_t)k * CP + j;
        const size_t q = (size_t)(T.start[k] + j);
        int nv = rec->nvalid < kept ? rec->nvalid : kept;
        nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
        nv = __builtin_amdgcn_readfirstlane(nv);
        double hn = 0.0;
        if (nv > 0) {
            hn = qd_levels_record<N>(W, rec, nv);
            qd_levels_solve(W, nv, L);
        }
        if (threadIdx.x == 0) {
            for (int i = 0; i < L; ++i) levels_dst[q * (size_t)L + i] = i < nv ? W.lev[i] : INFINITY;
            if (hnorm_dst) hnorm_dst[q] = hn;
        }
        __syncthreads();                                   // (lane 0 has read W.lev before the next point overwrites it)
    }
}
#endif  // __HIPCC__

#undef QD_LV_A
