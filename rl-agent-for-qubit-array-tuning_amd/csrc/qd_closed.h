// qd_closed.h -- the CLOSED regime: a dot array that is isolated from its reservoirs and holds exactly Q carriers
// (ground_state_closed / charge_sensor_closed / do1d_closed / do2d_closed of the reference's model class,
// TunnelCoupledChargeSensed.py:256-268, 291-309, 382-426).  The reference calls a _ground_state_closed that it never
// defines; what is built here is the open algorithm of charge_states.py / ground_state.py restricted to ONE total-charge
// sector (DESIGN "closed regime" is the contract):
//   centre   m = argmin (n - v')^T A (n - v')  over  n >= 0, sum(n) = Q           (qd_closed_centre)
//   kept     the K lowest by (E, idx) of c = floor(m) + delta, delta in {-1,0,1,2}^N, c >= 0, sum(c) = Q
//                                                                                    (qd_candidates_closed)
// The tunnelling Hamiltonian conserves the total charge, so a kept list from one sector needs nothing new behind the
// search: the record, the ground-state kernels and the sensor expression run as they are.  The front of the pipeline is
// what is new: one kernel, qd_k_closed, one record per lane, behind the front kernels of qd_eval_points / qd_scan_grid (which
// leave v' and 1 / s_a in the record's hand-over form) and in the place of the redo pass of the open search.
// qd_closed_centre and qd_candidates_closed are __host__ __device__ and use + - * / sqrt fma alone in one fixed order, so the
// CPU tier checks the bits the device produces (tests/hosttest_closed).
#pragma once
#include "qd_points.h"

#define QD_CLOSED_QMAX 32767     // n_charge of a query: 0..QD_CLOSED_QMAX (qdsim.h)

// ---------------------------------------------------------------------------
// Centre.  With b = A v' the equality-constrained problem on a free set F (n = 0 elsewhere) is
//   A_FF n_F = b_F - mu 1,   sum(n_F) = Q      =>  n_F = y - mu z,  A_FF y = b_F,  A_FF z = 1,  mu = (sum y - Q) / sum z
// and lambda = 2 mu is the multiplier of the sum constraint: g~ = 2 A (n - v') + lambda is 0 on F and must be >= 0 on the
// clamped dots.  The solves run on the FULL N x N matrix with the rows and columns of the clamped dots replaced by those of
// the identity and their right-hand sides by 0 (still positive definite; the clamped components come out as exact zeros),
// so every index is static.  Cholesky A = L L^T, row by row.
// Primal active set, at most 2N + 2 rounds from "all free": a negative free component -> clamp the most negative (lowest
// index on ties); else a clamped dot with a negative multiplier -> re-free the most negative; else stop.  When the bound is
// hit the last iterate is kept, clipped at 0.  The free dot of highest index is formed as Q minus the sum of the others, so
// a lone free dot holds exactly Q.  Q = 0: m = 0, lambda = 0.
//   vd[N]: the (scaled) v';  out  m[N], *lambda.  Returns the rounds used (host statistics).
// ---------------------------------------------------------------------------
template <int N>
QD_HD int qd_closed_centre(const double* par, const double* vd, int Q, double* m, double* lambda) {
    constexpr int G = N + 1;
    const QdLayout L = qd_layout(N);
    const double* A = par + L.cdd_inv;
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] = 0.0;
    *lambda = 0.0;
    if (Q <= 0) return 0;
    const double q = (double)Q;
    double b[N], n[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { b[i] = qd_dotN<N>(A + i * G, vd); n[i] = 0.0; QD_ROW_FENCE(); }
    unsigned fr = (1u << N) - 1u;                          // bit i: dot i is free
    double mu = 0.0;
    bool done = false;
    int round = 0;
#pragma unroll 1
    for (; round < 2 * N + 2 && !done; ++round) {
        // Cholesky of the masked matrix (lower, row by row) with the two forward substitutions folded into the row
        double C[N][N], wy[N], wz[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const bool fi = (fr >> i) & 1u;
            double sy = fi ? b[i] : 0.0, sz = fi ? 1.0 : 0.0;
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const bool fj = (fr >> j) & 1u;
                double s = (fi && fj) ? A[i * G + j] : (i == j ? 1.0 : 0.0);
#pragma unroll
                for (int k = 0; k < j; ++k) s = fma(-C[i][k], C[j][k], s);
                if (j < i) {
                    C[i][j] = s / C[j][j];
                    sy = fma(-C[i][j], wy[j], sy);
                    sz = fma(-C[i][j], wz[j], sz);
                } else {
                    C[i][i] = sqrt(s);
                }
            }
            wy[i] = sy / C[i][i]; wz[i] = sz / C[i][i];
        }
        // back substitution  L^T y = wy,  L^T z = wz
        double y[N], z[N];
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {
            double sy = wy[i], sz = wz[i];
#pragma unroll
            for (int k = i + 1; k < N; ++k) { sy = fma(-C[k][i], y[k], sy); sz = fma(-C[k][i], z[k], sz); }
            y[i] = sy / C[i][i]; z[i] = sz / C[i][i];
        }
        double ysum = 0.0, zsum = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) { ysum += y[i]; zsum += z[i]; }
        mu = (ysum - q) / zsum;
        // the free dot of highest index takes what the others leave of Q
        int top = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) if ((fr >> i) & 1u) top = i;
        double others = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            n[i] = ((fr >> i) & 1u) ? fma(-mu, z[i], y[i]) : 0.0;
            if (i != top) others += n[i];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) if (i == top) n[i] = q - others;
        // most negative free component
        int pick = -1; double worst = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) if (((fr >> i) & 1u) && n[i] < worst) { worst = n[i]; pick = i; }
        if (pick >= 0) { fr &= ~(1u << pick); continue; }
        // most negative multiplier of a clamped dot
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double gt = fma(2.0, qd_dotN<N>(A + i * G, n) - b[i], 2.0 * mu);
            if (!((fr >> i) & 1u) && gt < worst) { worst = gt; pick = i; }
            QD_ROW_FENCE();
        }
        if (pick >= 0) fr |= 1u << pick; else done = true;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] = n[i] > 0.0 ? n[i] : 0.0;
    *lambda = 2.0 * mu;
    return round;
}

// ---------------------------------------------------------------------------
// Exact k-best search over the sector sum(c) = Q of the box of the open search, in the style of QdLevel (qd_pixel.h), whose
// kept buffer, insertion, sort and leaf it uses as they are.  Two changes:
//   * the charge still to place, rem, travels down the tree as two slacks against what the dots from L on can hold,
//       shi = sum_{j>=L} cmax_j - rem >= 0,   slo = rem - sum_{j>=L} cmin_j >= 0      (cmax = fl + 2, cmin = max(fl - 1, 0)),
//     and the digit k of dot L (c = fl + k - 1; cmax - c = 3 - k, c - cmin = k - kmin) takes 3 - k from shi and k - kmin from
//     slo: it is confined to the window [3 - shi, kmin + slo] that keeps both >= 0.  Behind the last dot both are 0: it is
//     forced.  A dot takes at most 3 from either slack, so a slack of 3N or more never binds and is held as 3N (<= 24): the
//     two travel in one register, 32 shi + slo.
//   * the linear part of the bound uses g~ = 2 A (m - v') + lambda: on the sector sum(c - m) = Q - sum(m), so
//       E(c) = [E(m) - lambda (Q - sum m)] + g~ . (c - m) + (c - m)^T A (c - m)      exactly, for any m and lambda
//     (the bracket is the search's Em; Q - sum(m) is 0 up to rounding unless the centre's bound was hit).  g~ is ~0 on free
//     dots and >= 0 on clamped ones, so the bound is as tight as the open one's.
// Bounds only prune, with the open search's margin (qd_search_set_bound); every leaf gets the canonical energy from
// QdLevel<N, N, KC>::run, i.e. by the fma chain of the open search, shared row sums included.
// ---------------------------------------------------------------------------
template <int N, int L, int KC>
struct QdClosedLevel {
    static QD_HD void run(QdSearch<N, KC>& S, double partial, int slack) {
#ifndef __HIP_DEVICE_COMPILE__
        S.nodes++;
#endif
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < L; ++j) s = fma(S.U[j * N + L], S.dm[j], s);
        const double uLL = S.U[L * N + L];
        const double flL = S.fl[L];
        const double base = flL - S.m[L];                  // c - m for delta = 0
        const double gL = S.g[L];
        const double ui = S.uinv[L];
        const double kstar = (fma(-s, ui, -(0.5 * gL) * (ui * ui)) - base) + 1.0;
        // digits that keep c >= 0 and leave the dots behind a charge they can hold
        const int k0 = (flL > 0.0) ? 0 : 1;                // delta = -1 would give c < 0
        const int ka = 3 - (slack >> 5), kb = k0 + (slack & 31);
        const int kmin = ka > k0 ? ka : k0, kmax = kb < 3 ? kb : 3;
        if (kmin > kmax) return;
        double kc = rint(kstar);
        kc = fmin(fmax(kc, (double)kmin), (double)kmax);
        if (!(kc == kc)) kc = (double)kmin;                // NaN guard
        int k = (int)kc, lo = k - 1, hi = k + 1;
        const unsigned sh = 2u * (unsigned)(N - 1 - L);
        const double tl = S.tail[L];
        // convex in k: visited in order of distance from k*, the first digit that fails the bound ends the node
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
            const double x = base + (double)(k - 1);
            const double t = fma(uLL, x, s);
            const double pn = partial + fma(t, t, gL * x);
            if (pn + tl > S.lim) return;
            S.dm[L] = x;
            S.dv[L] = (flL + (double)(k - 1)) - S.vdash[L];
            S.idx = (S.idx & ~(3u << sh)) | ((unsigned)k << sh);
            // the shared canonical row sums of QdLevel, for its leaf
            if constexpr (L == QdSplit<N>::A) {
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j <= QdSplit<N>::A; ++j) acc = fma(S.A[i * S.lda + j], S.dv[j], acc);
                    S.pre1[i] = acc;
                }
            }
            if constexpr (L == QdSplit<N>::B) {
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    double acc = (QdSplit<N>::A >= 0) ? S.pre1[i] : 0.0;
#pragma unroll
                    for (int j = QdSplit<N>::A + 1; j <= QdSplit<N>::B; ++j) acc = fma(S.A[i * S.lda + j], S.dv[j], acc);
                    S.pre2[i] = acc;
                }
            }
            QdClosedLevel<N, L + 1, KC>::run(S, pn, slack - (32 * (3 - k) + (k - k0)));
            const bool can_lo = lo >= kmin, can_hi = hi <= kmax;
            if (!((int)can_lo | (int)can_hi)) return;
            const bool take_lo = (bool)((int)can_lo & ((int)!can_hi | (int)((kstar - (double)lo) <= ((double)hi - kstar))));
            k = take_lo ? lo : hi;
            lo -= take_lo ? 1 : 0;
            hi += take_lo ? 0 : 1;
        }
    }
};

template <int N, int KC>
struct QdClosedLevel<N, N, KC> {
    static QD_HD void run(QdSearch<N, KC>& S, double, int) {           // (both slacks are 0: the window of the last dot saw to it)
        QdLevel<N, N, KC>::run(S, 0.0);
    }
};

// Returns the number of candidates found (<= KC); the list is left in the reference order, increasing (E, idx).
//   vd: the (scaled) v';  m, lambda: qd_closed_centre's;  e/es, id/is: the strided kept buffer;  fl_out[N] = floor(m).
template <int N, int KC = QD_K>
QD_HD int qd_candidates_closed(const double* par, const double* vd, const double* m, double lambda, int Q,
                               double* e, int es, uint16_t* id, int is, int32_t* fl_out, unsigned long long* stats = nullptr) {
    const QdLayout L = qd_layout(N);
    QdSearch<N, KC> S;
    S.A = par + L.cdd_inv; S.lda = N + 1; S.U = par + L.ufac; S.uinv = par + L.uinv;
    double mv[N], msum = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        S.fl[i] = floor(m[i]); S.vdash[i] = vd[i]; S.m[i] = m[i];
        S.dm[i] = 0.0; S.dv[i] = 0.0;
        fl_out[i] = (int32_t)S.fl[i];
        mv[i] = m[i] - vd[i];
        msum += m[i];
    }
    double Em = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double t = qd_dotN<N>(S.A + i * S.lda, mv);
        S.g[i] = fma(2.0, t, lambda);
        Em = fma(mv[i], t, Em);
        QD_ROW_FENCE();
    }
    S.Em = fma(-lambda, (double)Q - msum, Em);
    double acc = 0.0;
    int shi = -Q, slo = Q;
#pragma unroll
    for (int j = N - 1; j >= 0; --j) {
        S.tail[j] = acc;                                   // sum over levels > j
        const double cmin = S.fl[j] > 0.0 ? S.fl[j] - 1.0 : 0.0, cmax = S.fl[j] + 2.0;
        const double lo = S.g[j] * (cmin - S.m[j]), hi = S.g[j] * (cmax - S.m[j]);
        acc += lo < hi ? lo : hi;
        shi += (int)cmax; slo -= (int)cmin;
    }
    S.e = e; S.es = es; S.id = id; S.is = is;
    S.count = 0; S.lim = INFINITY; S.idx = 0;
    S.nodes = S.leaves = S.inserts = S.shifts = 0;
    if (shi >= 0 && slo >= 0) {                            // (else the box does not reach the sector: no candidate)
        shi = shi < 3 * N ? shi : 3 * N; slo = slo < 3 * N ? slo : 3 * N;
        QdClosedLevel<N, 0, KC>::run(S, 0.0, 32 * shi + slo);
    }
    qd_search_sort(S);
#ifndef __HIP_DEVICE_COMPILE__
    if (stats) { stats[0] += S.nodes; stats[1] += S.leaves; stats[2] += S.inserts; stats[3] += S.shifts; }
#endif
    return S.count;
}

// ---------------------------------------------------------------------------
// The record of one point at total charge Q from its hand-over form (vd = v', isa = 1 / s_a): centre, search, and the list in
// the record as the ground-state kernels read it -- idx and E * isa of the nv candidates found, in the reference order;
// every slot from nv on gets idx = 0 and the largest kept energy (the ground-state kernels neither hop to such a slot nor
// let it win a tie, and with this energy it is never below the sector's ground state); fl = floor(m); nvalid = nv.
// e/es, id/is: the strided kept buffer of KC entries (LDS on the device).
// ---------------------------------------------------------------------------
template <int N, int KC>
QD_HD int qd_closed_record(const double* par, const double* vd, double isa, int Q, double* e, int es, uint16_t* id, int is,
                           QdPixelRec* rec, double* m_out = nullptr, unsigned long long* stats = nullptr) {
    double m[N], lambda;
    qd_closed_centre<N>(par, vd, Q, m, &lambda);
    int32_t fl[N];
    const int nv = qd_candidates_closed<N, KC>(par, vd, m, lambda, Q, e, es, id, is, fl, stats);
    const double epad = nv > 0 ? e[(nv - 1) * es] : 0.0;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        rec->idx[k] = k < nv ? id[k * is] : (uint16_t)0;
        rec->E[k] = (k < nv ? e[k * es] : epad) * isa;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) rec->fl[i] = fl[i];
    rec->nvalid = nv;
    if (m_out) {
#pragma unroll
        for (int i = 0; i < N; ++i) m_out[i] = m[i];
    }
    return nv;
}

#if defined(__HIPCC__)
#include "qd_kernels.h"     // QdPixelRec's hand-over form: qd_tile_hand_over, QD_T_REDO

#define QD_CLOSED_BLOCK 64

// ---------------------------------------------------------------------------
// One record per lane: record j of slot k (SP records per slot) in hand-over form (nvalid == QD_T_REDO; v' at E[8..],
// 1 / s_a at E[16]) -> the closed list at total charge qslot[k].  Inert records (nvalid = 0) are skipped, as the redo pass
// skips them.  The slot's parameter copy is block-uniform (scalar loads); the kept buffers live in LDS, [KC][64] energies
// then [KC][64] indices, as in qd_k_candidates.  grid = (ceil(SP / 64), slots), dynamic LDS = KC * 64 * 10 bytes.
// ---------------------------------------------------------------------------
template <int N, int KC>
__global__ void __launch_bounds__(QD_CLOSED_BLOCK, 2)
qd_k_closed(int SP, const double* __restrict__ sparams, const int32_t* __restrict__ qslot, QdPixelRec* __restrict__ recs) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.y;
    const int j = blockIdx.x * QD_CLOSED_BLOCK + threadIdx.x;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* se = (double*)smem_raw;                           // [KC][BLOCK]
    uint16_t* sid = (uint16_t*)(se + KC * QD_CLOSED_BLOCK);   // [KC][BLOCK]
    if (j >= SP) return;
    QdPixelRec* rec = recs + (size_t)k * SP + j;
    if (rec->nvalid != QD_T_REDO) return;
    const double* spar = sparams + (size_t)k * L.size;
    double vd[N];
#pragma unroll
    for (int i = 0; i < N; ++i) vd[i] = rec->E[8 + i];
    const double isa = rec->E[16];
    qd_closed_record<N, KC>(spar, vd, isa, qslot[k], se + threadIdx.x, QD_CLOSED_BLOCK, sid + threadIdx.x, QD_CLOSED_BLOCK, rec);
}

// the total charges of the slots of one qd_eval_points_closed launch, from the kernel's argument to the device table
struct QdClosedQ { int32_t q[QD_POINTS_MAX_SLOTS]; };
__global__ void qd_k_closed_setq(QdClosedQ T, int n, int32_t* __restrict__ qslot) {
    const int i = threadIdx.x;
    if (i < n) qslot[i] = T.q[i];
}

// the kept states of the points of a launch in list order: states_dst [np][K][N] int32, c_i = fl_i + digit_i - 1 for the
// nvalid first slots, zeros behind them.  One point per lane.  grid = (ceil(SP / 256), slots).
template <int N>
__global__ void qd_k_closed_states(QdPointSlots T, int SP, int K, const QdPixelRec* __restrict__ recs, int32_t* __restrict__ states_dst) {
    const int k = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= SP || j >= T.cnt[k]) return;
    const QdPixelRec* rec = recs + (size_t)k * SP + j;
    int32_t* out = states_dst + (size_t)(T.start[k] + j) * K * N;
    const int nv = rec->nvalid < K ? rec->nvalid : K;
    for (int s = 0; s < K; ++s) {
        const unsigned code = rec->idx[s];
#pragma unroll
        for (int i = 0; i < N; ++i)
            out[s * N + i] = s < nv ? rec->fl[i] + (int)((code >> (2 * (N - 1 - i))) & 3u) - 1 : 0;
    }
}

#endif  // __HIPCC__
