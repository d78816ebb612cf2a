// qd_thermal.h -- the thermal state of a point (qd_eval_points_thermal): rho = exp(-H / kT) / Z of the Hamiltonian
// H = diag(E_0 .. E_{nv-1}) + H_t over the nv = min(nvalid, K) valid kept states of a QdPixelRec, the block of qd_levels.h
// (qd_levels_record builds it here too; the |0..0> padding copies are left out: an isolated copy of one diagonal entry would
// carry Boltzmann weight of its own).  The ground-state stage and the levels kernel stop short of the excited eigenvectors;
// this file computes the whole decomposition, ONE POINT PER WAVEFRONT, and the quantities that consume all of it:
//   P_m = sum_k w_k V[m,k]^2,  w_k = exp(-(lam_k - lam_min) / kT) / Z      populations of the kept charge states
//   occ[d] = sum_m P_m s_m[d],  var[d] = sum_m P_m (s_m[d] - occ[d])^2      (= sum_m P_m s_m[d]^2 - occ[d]^2, never negative)
//   ztail = w of the HIGHEST kept level: the caller's check on the truncation to K states at this kT
// and the sensor constant c0 = 2 b + a (2 (Ns - v''_s) + 1) of qd_k_gs_select from the thermal occupations.
//
//   1. the diagonal is shifted by its minimum and the block scaled by a power of two to ||A||_inf in [1, 2), as step 1 of
//      qd_levels_solve; the lower triangle is mirrored, the block is kept full
//   2. cyclic Jacobi, round-robin ordering: ne = s rounded up to even, ne - 1 rounds per sweep, round r pairs (ne-1, r) and
//      ((r + k) mod (ne-1), (r - k) mod (ne-1)), k = 1 .. ne/2 - 1: up to 16 disjoint rotations; with s odd the pair of the idle
//      index ne - 1 = s is never rotated (row and column s of A are zero; its partner of the round still takes the other pairs'
//      rotations through their common blocks).  A round is two phases with one barrier behind each:
//        a. lane k < ne/2 computes (c, s) of its pair (p, q) from a_pp, a_qq, a_pq (the smaller root t of
//           t^2 + 2 theta t - 1 = 0).  A pair with |a_pq| <= 2^-56 (of ||A|| in [1, 2)) is not rotated; in particular an entry
//           that is EXACTLY ZERO never is, so states of different hop components never mix, V stays block diagonal and
//           tc == 0 gives the classical Boltzmann distribution over the integer states exactly
//        b. A <- J^T A J by 2 x 2 blocks: item (a, b) owns the four entries of rows (p_a, q_a) and columns (p_b, q_b), reads
//           and writes nothing else, and needs no barrier between the row and the column half.  Item (b, a) runs the same
//           operations on the transposed block in the same order, so A stays exactly symmetric; the diagonal item sets
//           a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0.  In the same phase V <- V J, lane = row, pairs split over the two
//           half-waves
//      A sweep in which no pair rotated ends the iteration (a wave-uniform count, one reduction per sweep); QD_TH_SWEEPS
//      caps it.  What is left off the diagonal is at most 2^-56 per entry, a backward error of 32 * 2^-56 = 4.4e-16 ||A||.
//      Clusters need no care: the thermal state does not depend on the basis inside a cluster.
//   3. weights, populations, moments.  A weight that underflows to zero is expected and harmless.
//
// The same source compiles for the host through the lane macros of qd_eig_wave.h (code outside QD_EW_EACH is wave-uniform, code
// inside runs per lane, whatever crosses lanes goes through the workspace with QD_EW_SYNC in between); tests/hosttest_thermal
// checks it against numpy.linalg.eigh without a GPU.
//
// LDS: A is the block of the embedded QdLevelsWs (12 864 B: 32 rows at the odd stride of 33 doubles, so that the 32 lanes of a
// half-wave fall on different banks whether they walk a row or a column, and the vectors of qd_levels_record), V a second
// 32 x 33 block (8 448 B), then lam, w, pop (768 B), the round's c, s, t (384 B) and p, q, rot (192 B), occ and var (128 B) and
// ztail: sizeof(QdThermalWs) = 22 792 B, seven single-wave blocks per CU (160 KB = 163 840 B of LDS; 7 x 22 792 =
// 159 544).
#pragma once
#include "qd_levels.h"

#define QD_TH_SWEEPS 24         // sweep cap (s = 32 converges in 7 to 10)
#define QD_TH_THRESH 0x1p-56    // off-diagonal entries at or below it (||A||_inf in [1, 2)) are not rotated

struct QdThermalWs {
    QdLevelsWs B;                           // B.A: the block; B.red, B.code: qd_levels_record's
    double V[QD_LV_MAX * QD_LV_LD];
    double lam[QD_LV_MAX], w[QD_LV_MAX], pop[QD_LV_MAX];
    double c[16], s[16], t[16];
    int p[16], q[16], rot[16];              // the round's pairs, p < q, and whether they rotate
    double occ[8], var[8];
    double ztail;
};

static_assert(sizeof(QdThermalWs) == 22792, "the header comment states the size");

#define QD_TH_A(i, j) W.B.A[(i) * QD_LV_LD + (j)]
#define QD_TH_V(i, j) W.V[(i) * QD_LV_LD + (j)]

// The lower triangle of W.B.A (rows 0 .. s-1, 1 <= s <= 32; destroyed) and kT > 0 (units of the input) ->
//   W.lam[k]   the eigenvalues in the units of the input (in no particular order), W.V column k the unit eigenvector
//   W.pop[m]   the thermal population of state m;  W.ztail the normalised weight of the highest level.
// Returns the number of sweeps run (wave-uniform); QD_TH_SWEEPS means the cap ended the iteration.
QD_HD int qd_thermal_solve(QdThermalWs& W, int s, double kT) {
    if (s == 1) {                                             // (uniform) one state: P = 1 exactly
        const double a = QD_TH_A(0, 0);
        if (QD_EW_LANE0) { W.lam[0] = a; W.pop[0] = 1.0; W.w[0] = 1.0; W.V[0] = 1.0; W.ztail = 1.0; }
        QD_EW_SYNC();
        return 0;
    }
    // ---- 1. shift by the lowest diagonal entry, scale, mirror; V = I ----
    QD_EW_EACH(i) { W.B.red[i] = i < s ? -QD_TH_A(i, i) : -INFINITY; }
    const double dmin = -qd_ew_max(W.B.red);
    QD_EW_EACH(i) { if (i < s) QD_TH_A(i, i) -= dmin; }
    QD_EW_SYNC();
    QD_EW_EACH(i) {
        double rs = 0.0;
        if (i < s)
            for (int j = 0; j < s; ++j) rs += fabs(j <= i ? QD_TH_A(i, j) : QD_TH_A(j, i));
        W.B.red[i] = rs;
    }
    const double anorm = qd_ew_max(W.B.red);
    double tsc, tusc;
    qd_pow2_scale(anorm, tsc, tusc);
    QD_EW_EACH(i) {
        if (i < s)
            for (int j = 0; j <= i; ++j) {
                const double a = QD_TH_A(i, j) * tsc;
                QD_TH_A(i, j) = a;
                QD_TH_A(j, i) = a;
            }
    }
    QD_EW_EACH(l) {
        const int i = l & 31;
        if (i < s)
            for (int j = l >> 5; j < s; j += 2) QD_TH_V(i, j) = (i == j) ? 1.0 : 0.0;
        if ((s & 1) && l <= s) { QD_TH_A(s, l) = 0.0; QD_TH_A(l, s) = 0.0; }   // the idle index of an odd s (<= 31): a zero row and column
    }
    QD_EW_SYNC();
    // ---- 2. Jacobi ----
    const int ne = s + (s & 1), h = ne >> 1, m = ne - 1;
    int hb = 0;
    while ((1 << hb) < h) ++hb;
    const int items = h << hb;
    int sweeps = 0;
    for (; sweeps < QD_TH_SWEEPS; ++sweeps) {
        QD_EW_EACH(l) { W.B.red[l] = 0.0; }
        for (int r = 0; r < m; ++r) {
            // a. the pair lanes
            QD_EW_EACH(k) {
                if (k < h) {
                    int p = k == 0 ? m : (r + k) % m;
                    int q = k == 0 ? r : (r - k + m) % m;
                    if (p > q) { const int x = p; p = q; q = x; }
                    double c = 1.0, sn = 0.0, t = 0.0;
                    bool rot = false;
                    if (q < s) {
                        const double apq = QD_TH_A(p, q);
                        if (fabs(apq) > QD_TH_THRESH) {
                            const double theta = (QD_TH_A(q, q) - QD_TH_A(p, p)) * qd_rcp(2.0 * apq);
                            const double root = qd_sqrt1(fma(theta, theta, 1.0));
                            t = copysign(1.0, theta) * qd_rcp(fabs(theta) + root);
                            double sq, rsq;
                            qd_sqrt_rsqrt(fma(t, t, 1.0), sq, rsq);
                            c = rsq; sn = t * rsq;
                            rot = true;
                        }
                    }
                    W.c[k] = c; W.s[k] = sn; W.t[k] = t;
                    W.p[k] = p; W.q[k] = q; W.rot[k] = rot ? 1 : 0;
                    if (rot) W.B.red[k] = 1.0;
                }
            }
            QD_EW_SYNC();
            // b. A <- J^T A J by 2 x 2 blocks, V <- V J
            QD_EW_EACH(l) {
                for (int it = l; it < items; it += 64) {
                    const int a = it >> hb, b = it & ((1 << hb) - 1);
                    if (b >= h) continue;
                    if (!(W.rot[a] | W.rot[b])) continue;                 // neither pair rotates: the block stays
                    const int ra = W.p[a], qa = W.q[a], rb = W.p[b], qb = W.q[b];
                    if (a == b) {
                        const double d = W.t[a] * QD_TH_A(ra, qa);
                        QD_TH_A(ra, ra) -= d;
                        QD_TH_A(qa, qa) += d;
                        QD_TH_A(ra, qa) = 0.0;
                        QD_TH_A(qa, ra) = 0.0;
                        continue;
                    }
                    // (an unrotated pair, that of the idle index included, takes part with c = 1, s = 0: the identity, exactly)
                    // canonical order: the pair with the lower number rotates the rows of ITS block first
                    const bool up = a < b;
                    const int i0 = up ? ra : rb, i1 = up ? qa : qb, j0 = up ? rb : ra, j1 = up ? qb : qa;
                    const double ci = up ? W.c[a] : W.c[b], si = up ? W.s[a] : W.s[b];
                    const double cj = up ? W.c[b] : W.c[a], sj = up ? W.s[b] : W.s[a];
                    // the block of rows (i0, i1) and columns (j0, j1), read from this item's own entries
                    const double x00 = up ? QD_TH_A(i0, j0) : QD_TH_A(j0, i0), x01 = up ? QD_TH_A(i0, j1) : QD_TH_A(j1, i0);
                    const double x10 = up ? QD_TH_A(i1, j0) : QD_TH_A(j0, i1), x11 = up ? QD_TH_A(i1, j1) : QD_TH_A(j1, i1);
                    const double r00 = ci * x00 - si * x10, r01 = ci * x01 - si * x11;
                    const double r10 = si * x00 + ci * x10, r11 = si * x01 + ci * x11;
                    const double y00 = cj * r00 - sj * r01, y01 = sj * r00 + cj * r01;
                    const double y10 = cj * r10 - sj * r11, y11 = sj * r10 + cj * r11;
                    if (up) { QD_TH_A(i0, j0) = y00; QD_TH_A(i0, j1) = y01; QD_TH_A(i1, j0) = y10; QD_TH_A(i1, j1) = y11; }
                    else    { QD_TH_A(j0, i0) = y00; QD_TH_A(j1, i0) = y01; QD_TH_A(j0, i1) = y10; QD_TH_A(j1, i1) = y11; }
                }
                const int i = l & 31;
                if (i < s)
                    for (int k = l >> 5; k < h; k += 2) {
                        if (!W.rot[k]) continue;
                        const int p = W.p[k], q = W.q[k];
                        const double c = W.c[k], sn = W.s[k];
                        const double vp = QD_TH_V(i, p), vq = QD_TH_V(i, q);
                        QD_TH_V(i, p) = c * vp - sn * vq;
                        QD_TH_V(i, q) = sn * vp + c * vq;
                    }
            }
            QD_EW_SYNC();
        }
        if (qd_ew_max(W.B.red) == 0.0) break;                             // (uniform) no pair rotated in this sweep
    }
    // ---- 3. weights and populations ----
    QD_EW_EACH(k) { W.B.red[k] = k < s ? -QD_TH_A(k, k) : -INFINITY; }
    const double lmin = -qd_ew_max(W.B.red);
    QD_EW_EACH(k) {
        double w = 0.0;
        if (k < s) {
            const double a = QD_TH_A(k, k);
            w = exp(-(((a - lmin) * tusc) / kT));           // (0 / kT = 0: the lowest level has weight 1 at any kT)
            W.lam[k] = dmin + a * tusc;
            W.w[k] = w;
        }
        W.B.red[k] = w;
    }
    const double Z = qd_ew_sum(W.B.red);
    QD_EW_EACH(k) { W.B.red[k] = k < s ? -W.w[k] : -INFINITY; }
    const double wtail = -qd_ew_max(W.B.red);
    const double iZ = 1.0 / Z;
    QD_EW_EACH(i) {
        if (i < s) {
            double acc = 0.0;
            for (int k = 0; k < s; ++k) { const double v = QD_TH_V(i, k); acc = fma(W.w[k], v * v, acc); }
            W.pop[i] = acc * iZ;
        }
    }
    if (QD_EW_LANE0) W.ztail = wtail * iZ;
    QD_EW_SYNC();
    return sweeps;
}

// Occupations and variances of the N dots from the populations W.pop[0 .. nv-1] and the states of the record (digit of dot d
// in bits 2 (N-1-d) of idx, occupation fl[d] + digit - 1, as qd_ground_select reads them): lane d < N sums its dot over the
// states in list order.  -> W.occ, W.var, valid in every lane after the call.
template <int N>
QD_HD void qd_thermal_moments(QdThermalWs& W, const QdPixelRec* rec, int nv) {
    QD_EW_EACH(d) {
        if (d < N) {
            const int fl = rec->fl[d], sh = 2 * (N - 1 - d);
            double o = 0.0;
            for (int m = 0; m < nv; ++m) o = fma(W.pop[m], (double)(fl + (int)(((unsigned)rec->idx[m] >> sh) & 3u) - 1), o);
            double v = 0.0;
            for (int m = 0; m < nv; ++m) {
                const double dn = (double)(fl + (int)(((unsigned)rec->idx[m] >> sh) & 3u) - 1) - o;
                v = fma(W.pop[m], dn * dn, v);
            }
            W.occ[d] = o; W.var[d] = v;
        }
    }
    QD_EW_SYNC();
}

#if defined(__HIPCC__)
#include "qd_points.h"          // QdPointSlots

// kT of the slots of one launch; travels as a kernel argument beside QdPointSlots
struct QdThermalKT { double kT[QD_POINTS_MAX_SLOTS]; };

// ---------------------------------------------------------------------------------------------------------------
// The thermal state of the live records of a point launch, one point per wavefront, in place of the ground-state stage: blocks
// of ONE wave, grid = (blocks, slots), the blocks of slot k stride over its T.cnt[k] points (qd_k_levels).  Reads the record
// and the slot's parameter copy.  Writes the sensor constant to the slot's zraw and the occupations to the slot's occ, where
// qd_k_points_write finds them, and var_dst[q * N + d], ztail_dst[q] (either may be null) for point q = T.start[k] + j.
// A record without a valid state (never produced by the searches) counts as |0..0>.
// ---------------------------------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(64)
qd_k_thermal(QdPointSlots T, QdThermalKT TK, int CP, int kept, const double* __restrict__ qparams,
             const QdPixelRec* __restrict__ recs, double* __restrict__ qz, double* __restrict__ qocc,
             double* __restrict__ var_dst, double* __restrict__ ztail_dst) {
    constexpr int G = N + 1;
    __shared__ QdThermalWs W;
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.y;
    const int cnt = T.cnt[k] < CP ? T.cnt[k] : CP;
    const double kT = TK.kT[k];
    const double* par = qparams + (size_t)k * L.size;
    for (int j = blockIdx.x; j < cnt; j += gridDim.x) {
        const size_t sp = (size_t)k * CP + j;
        const QdPixelRec* rec = recs + sp;
        const size_t q = (size_t)(T.start[k] + j);
        int nv = rec->nvalid < kept ? rec->nvalid : kept;
        nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
        nv = __builtin_amdgcn_readfirstlane(nv);
        if (nv > 0) {
            qd_levels_record<N>(W.B, rec, nv);
            qd_thermal_solve(W, nv, kT);
            qd_thermal_moments<N>(W, rec, nv);
        }
        if (threadIdx.x == 0) {
            // c0 = 2 b + a (2 (Ns - v''_s) + 1), b = sum_i A[N][i] (<n_i> - v''_i): the operations of qd_k_gs_select
            double b = 0.0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const double o = nv > 0 ? W.occ[i] : 0.0;
                b = fma(par[L.cdd_inv + N * G + i], o - rec->vpp[i], b);
                qocc[sp * N + i] = o;
                if (var_dst) var_dst[q * N + i] = nv > 0 ? W.var[i] : 0.0;
            }
            const double vs = rec->vpp[N];
            const double Ns = rint(vs);
            qz[sp] = 2.0 * b + par[L.cdd_inv + N * G + N] * (2.0 * (Ns - vs) + 1.0);
            if (ztail_dst) ztail_dst[q] = nv > 0 ? W.ztail : 1.0;
        }
        __syncthreads();                                   // (lane 0 has read W before the next point overwrites it)
    }
}
#endif  // __HIPCC__

#undef QD_TH_A
#undef QD_TH_V
