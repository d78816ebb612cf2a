// qd_thermal_blocks.h -- the thermal state of a point, PER HOP COMPONENT (qd_scan_grid_thermal): the contract of
// qd_thermal_solve (qd_thermal.h) -- the lower triangle of the block in the workspace, 1 <= s <= 32, kT > 0 -> pop, lam, V, ztail
// and the number of sweeps -- by a Jacobi iteration that never leaves the connected components of the coupling pattern.  States
// of different components do not couple, qd_thermal_solve already refuses to rotate exact zeros, so its 31 rounds per sweep
// (s = 32) mostly turn over pairs that have nothing to do.  Here a sweep has max_c (2 ceil(s_c / 2) - 1) rounds and touches the
// entries inside components only.  (The LARGEST component of a pixel sets the rounds: 8 to 16 of 32 states in a 4-dot scan
// window, 5 to 23 at 8 dots -- DESIGN 7 has the census and the rates: 2.6 and 1.5 times qd_k_thermal on open grids at K = 32.)
//
//   1. step 1 of qd_thermal_solve as it is: shift by the lowest diagonal entry, ONE power-of-two scale of the whole block to
//      ||A||_inf in [1, 2), mirror, V = I; the rotation threshold 2^-56 is on that global scale, so the error argument of
//      tests/thermal_helpers.py (hs, hn of the whole block) carries over.  In the pass that sums the rows lane i also collects
//      the neighbour mask of state i from the UNSCALED entries: bit j set iff A_ij != 0.  Exact zeros do not link (the rule of
//      the ground-state stage); a denormal coupling links, whether or not the scaling flushes it.
//   2. components: lane i holds the 32-bit mask R_i of the states it reaches, R_i = {i} + neighbours at first, and
//      R_i <- OR of R_j over j in R_i until no mask changed (a wave-uniform reduction): the reach doubles per pass, at most 5
//      passes for a chain of 32.  The label of a state is the lowest index of its component, ctz(R_i).  From the masks, per
//      lane and by counting alone: the size s_c, the local index, the offset of the component in the member list (ordered by
//      label, then index), its first pair slot and its first item.  A component of s_c >= 2 states has h_c = ceil(s_c / 2)
//      pair slots, a single state none.  Pair slots of all components lie side by side, sum h_c <= 21 (ten of 3 and one of 2).
//   3. cyclic Jacobi per component: component c runs the round-robin of qd_thermal_solve on its LOCAL indices with
//      m_c = 2 h_c - 1 and takes part in round r of a sweep iff r < m_c.  An odd component has an idle local index s_c whose
//      pair is never rotated and HAS NO ROW OR COLUMN: its partner of the round takes the other pairs' rotations as 1 x 2 and
//      2 x 1 blocks (an absent entry is read as zero and not written).  Items (a, b) exist for two pair slots of the same
//      component only, sum h_c^2 <= 256, in a list built once per point; item (b, a) repeats item (a, b) on the transposed
//      block in the same order, so A stays exactly symmetric.  V <- V J per row over the pair slots of the row's own component.
//      A sweep in which no pair rotated ends the iteration; QD_TH_SWEEPS caps it.  All components single: no sweep, V = I.
//   4. weights w_k = exp(-(lam_k - lam_min) / kT) over ALL levels, one Z; P_i = sum over k in comp(i) of w_k V_ik^2 / Z; ztail.
// Entries of A and V between different components are never written after step 1: they stay exactly zero.
//
// The same source compiles for the host through the lane macros of qd_eig_wave.h; tests/hosttest_thermal_blocks checks it
// against numpy.linalg.eigh without a GPU.  Everything a second point could inherit (masks, member list, slot and item lists,
// the round arrays) is written for the current point before it is read.
//
// LDS: the embedded QdThermalWs (22 792 B: the block, V, lam, w, pop and the moments, where qd_thermal_moments finds them; its
// 16-entry round arrays stay unused), the round's c, s, t of 32 pair slots (768 B), the masks (256 B), the item list (512 B) and
// 352 B of byte arrays: sizeof(QdThermalBlocksWs) = 24 680 B, six single-wave blocks per CU (160 KB = 163 840 B of LDS;
// 6 x 24 680 = 148 080).  qd_k_thermal_grid<8, QdThermalBlocksWs> for gfx950: 160 VGPRs, 106 SGPRs, no spill, no scratch (the compiler's
// resource report, -Rpass-analysis=kernel-resource-usage); the LDS, not the registers, bounds the waves per SIMD.
#pragma once
#include "qd_thermal.h"

#define QD_THB_IDLE 255         // the partner of the idle index of an odd component: no row, no column

struct QdThermalBlocksWs {
    QdThermalWs T;                          // T.B.A: the block; T.V, T.lam, T.w, T.pop, T.occ, T.var, T.ztail: the results
    double c[32], s[32], t[32];             // the round's rotations, one per pair slot
    unsigned ma[32], mb[32];                // reach masks of the states, double buffered
    unsigned short item[256];               // (pair slot a) << 8 | pair slot b, both of one component
    unsigned char p[32], q[32], rot[32];    // the round's pairs in state indices, p < q (q may be QD_THB_IDLE), and whether they rotate
    unsigned char mem[32];                  // the states ordered by (label, index)
    unsigned char sk[32], soff[32], ssz[32];            // per pair slot: its number inside the component, the component's offset in mem and size
    unsigned char st_off[32], st_sz[32], st_slot[32], st_h[32];   // per state: offset and size of its component, first pair slot, pair slots
};

static_assert(sizeof(QdThermalBlocksWs) == 24680, "the header comment states the size");

#define QD_TB_A(i, j) W.T.B.A[(i) * QD_LV_LD + (j)]
#define QD_TB_V(i, j) W.T.V[(i) * QD_LV_LD + (j)]

// The lower triangle of W.T.B.A (rows 0 .. s-1, 1 <= s <= 32; destroyed) and kT > 0 (units of the input) ->
//   W.T.lam[k]  the eigenvalues in the units of the input (in no particular order), W.T.V column k the unit eigenvector
//   W.T.pop[m]  the thermal population of state m;  W.T.ztail the normalised weight of the highest level
//   W.ma[i]     the states of the component of state i, as a mask.
// Returns the number of sweeps run (wave-uniform); QD_TH_SWEEPS means the cap ended the iteration.
QD_HD int qd_thermal_blocks_solve(QdThermalBlocksWs& W, int s, double kT) {
    if (s == 1) {                                             // (uniform) one state: P = 1 exactly
        const double a = QD_TB_A(0, 0);
        if (QD_EW_LANE0) { W.T.lam[0] = a; W.T.pop[0] = 1.0; W.T.w[0] = 1.0; W.T.V[0] = 1.0; W.T.ztail = 1.0; W.ma[0] = 1u; }
        QD_EW_SYNC();
        return 0;
    }
    // ---- 1. shift by the lowest diagonal entry, scale, mirror; V = I; the neighbour masks ----
    QD_EW_EACH(i) { W.T.B.red[i] = i < s ? -QD_TB_A(i, i) : -INFINITY; }
    const double dmin = -qd_ew_max(W.T.B.red);
    QD_EW_EACH(i) { if (i < s) QD_TB_A(i, i) -= dmin; }
    QD_EW_SYNC();
    QD_EW_EACH(i) {
        double rs = 0.0;
        if (i < s) {
            unsigned nb = 1u << i;
            for (int j = 0; j < s; ++j) {
                const double a = j <= i ? QD_TB_A(i, j) : QD_TB_A(j, i);
                rs += fabs(a);
                if (a != 0.0) nb |= 1u << j;
            }
            W.ma[i] = nb;
        }
        W.T.B.red[i] = rs;
    }
    const double anorm = qd_ew_max(W.T.B.red);
    double tsc, tusc;
    qd_pow2_scale(anorm, tsc, tusc);
    QD_EW_EACH(i) {
        if (i < s)
            for (int j = 0; j <= i; ++j) {
                const double a = QD_TB_A(i, j) * tsc;
                QD_TB_A(i, j) = a;
                QD_TB_A(j, i) = a;
            }
    }
    QD_EW_EACH(l) {
        const int i = l & 31;
        if (i < s)
            for (int j = l >> 5; j < s; j += 2) QD_TB_V(i, j) = (i == j) ? 1.0 : 0.0;
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
            W.T.B.red[i] = ch;
        }
        const bool more = qd_ew_max(W.T.B.red) != 0.0;        // (its barriers order the two buffers)
        in_a = !in_a;
        if (!more) break;                                     // (no mask changed: ma and mb hold the same closure)
    }
    // slots and items in all, rounds per sweep (uniform: every lane reads the same masks)
    int nslots = 0, nitems = 0, rounds = 0;
    for (int j = 0; j < s; ++j) {
        const unsigned mj = W.ma[j];
        if (__builtin_ctz(mj) != j) continue;                 // (a component counts at its label)
        const int sz = __builtin_popcount(mj), h = sz > 1 ? (sz + 1) >> 1 : 0;
        nslots += h; nitems += h * h;
        if (2 * h - 1 > rounds) rounds = 2 * h - 1;
    }
    QD_EW_EACH(i) {
        if (i < s) {
            const unsigned mi = W.ma[i];
            const int lab = __builtin_ctz(mi), sz = __builtin_popcount(mi), pos = __builtin_popcount(mi & ((1u << i) - 1u));
            const int h = sz > 1 ? (sz + 1) >> 1 : 0;
            int off = 0, slot0 = 0, it0 = 0;
            for (int j = 0; j < lab; ++j) {                   // the components with a lower label
                const unsigned mj = W.ma[j];
                if (__builtin_ctz(mj) != j) continue;
                const int szj = __builtin_popcount(mj), hj = szj > 1 ? (szj + 1) >> 1 : 0;
                off += szj; slot0 += hj; it0 += hj * hj;
            }
            W.mem[off + pos] = (unsigned char)i;
            W.st_off[i] = (unsigned char)off; W.st_sz[i] = (unsigned char)sz;
            W.st_slot[i] = (unsigned char)slot0; W.st_h[i] = (unsigned char)h;
            if (pos < h) {                                    // the first h states of a component fill its pair slots and item rows
                const int sl = slot0 + pos;
                W.sk[sl] = (unsigned char)pos; W.soff[sl] = (unsigned char)off; W.ssz[sl] = (unsigned char)sz;
                for (int b = 0; b < h; ++b) W.item[it0 + pos * h + b] = (unsigned short)((sl << 8) | (slot0 + b));
            }
        }
    }
    QD_EW_SYNC();
    // ---- 3. Jacobi inside the components ----
    int sweeps = 0;
    for (; rounds > 0 && sweeps < QD_TH_SWEEPS; ++sweeps) {
        QD_EW_EACH(l) { W.T.B.red[l] = 0.0; }
        for (int r = 0; r < rounds; ++r) {
            // a. the pair lanes
            QD_EW_EACH(sl) {
                if (sl < nslots) {
                    const int k = W.sk[sl], off = W.soff[sl], sz = W.ssz[sl];
                    const int m = ((sz + 1) & ~1) - 1;
                    double c = 1.0, sn = 0.0, t = 0.0;
                    int gp = 0, gq = QD_THB_IDLE;
                    bool rot = false;
                    if (r < m) {                              // (else: the component has finished its rounds of this sweep)
                        int p = r + k, q = r - k;
                        if (p >= m) p -= m;
                        if (q < 0) q += m;
                        if (k == 0) { p = m; q = r; }
                        if (p > q) { const int x = p; p = q; q = x; }
                        gp = W.mem[off + p];
                        if (q < sz) {
                            gq = W.mem[off + q];
                            const double apq = QD_TB_A(gp, gq);
                            if (fabs(apq) > QD_TH_THRESH) {
                                const double theta = (QD_TB_A(gq, gq) - QD_TB_A(gp, gp)) * qd_rcp(2.0 * apq);
                                const double root = qd_sqrt1(fma(theta, theta, 1.0));
                                t = copysign(1.0, theta) * qd_rcp(fabs(theta) + root);
                                double sq, rsq;
                                qd_sqrt_rsqrt(fma(t, t, 1.0), sq, rsq);
                                c = rsq; sn = t * rsq;
                                rot = true;
                            }
                        }
                    }
                    W.c[sl] = c; W.s[sl] = sn; W.t[sl] = t;
                    W.p[sl] = (unsigned char)gp; W.q[sl] = (unsigned char)gq; W.rot[sl] = rot ? 1 : 0;
                    if (rot) W.T.B.red[sl] = 1.0;
                }
            }
            QD_EW_SYNC();
            // b. A <- J^T A J by blocks of two pair slots of one component, V <- V J
            QD_EW_EACH(l) {
                for (int it = l; it < nitems; it += 64) {
                    const int a = W.item[it] >> 8, b = W.item[it] & 255;
                    if (!(W.rot[a] | W.rot[b])) continue;                 // neither pair rotates: the block stays
                    const int ra = W.p[a], qa = W.q[a], rb = W.p[b], qb = W.q[b];
                    if (a == b) {
                        const double d = W.t[a] * QD_TB_A(ra, qa);
                        QD_TB_A(ra, ra) -= d;
                        QD_TB_A(qa, qa) += d;
                        QD_TB_A(ra, qa) = 0.0;
                        QD_TB_A(qa, ra) = 0.0;
                        continue;
                    }
                    // (an unrotated pair, that of the idle index included, takes part with c = 1, s = 0: the identity, exactly)
                    // canonical order: the pair slot with the lower number rotates the rows of ITS block first
                    const bool up = a < b;
                    const int i0 = up ? ra : rb, i1 = up ? qa : qb, j0 = up ? rb : ra, j1 = up ? qb : qa;
                    const bool hi = i1 != QD_THB_IDLE, hj = j1 != QD_THB_IDLE;      // (at most one of them is absent)
                    const double ci = up ? W.c[a] : W.c[b], si = up ? W.s[a] : W.s[b];
                    const double cj = up ? W.c[b] : W.c[a], sj = up ? W.s[b] : W.s[a];
                    // the block of rows (i0, i1) and columns (j0, j1), read from this item's own entries
                    const double x00 = up ? QD_TB_A(i0, j0) : QD_TB_A(j0, i0);
                    const double x01 = !hj ? 0.0 : (up ? QD_TB_A(i0, j1) : QD_TB_A(j1, i0));
                    const double x10 = !hi ? 0.0 : (up ? QD_TB_A(i1, j0) : QD_TB_A(j0, i1));
                    const double x11 = !(hi && hj) ? 0.0 : (up ? QD_TB_A(i1, j1) : QD_TB_A(j1, i1));
                    const double r00 = ci * x00 - si * x10, r01 = ci * x01 - si * x11;
                    const double r10 = si * x00 + ci * x10, r11 = si * x01 + ci * x11;
                    const double y00 = cj * r00 - sj * r01, y01 = sj * r00 + cj * r01;
                    const double y10 = cj * r10 - sj * r11, y11 = sj * r10 + cj * r11;
                    if (up) {
                        QD_TB_A(i0, j0) = y00;
                        if (hj) QD_TB_A(i0, j1) = y01;
                        if (hi) QD_TB_A(i1, j0) = y10;
                        if (hi && hj) QD_TB_A(i1, j1) = y11;
                    } else {
                        QD_TB_A(j0, i0) = y00;
                        if (hj) QD_TB_A(j1, i0) = y01;
                        if (hi) QD_TB_A(j0, i1) = y10;
                        if (hi && hj) QD_TB_A(j1, i1) = y11;
                    }
                }
                const int i = l & 31;
                if (i < s) {
                    const int k0 = W.st_slot[i], k1 = k0 + W.st_h[i];
                    for (int k = k0 + (l >> 5); k < k1; k += 2) {
                        if (!W.rot[k]) continue;
                        const int p = W.p[k], q = W.q[k];
                        const double c = W.c[k], sn = W.s[k];
                        const double vp = QD_TB_V(i, p), vq = QD_TB_V(i, q);
                        QD_TB_V(i, p) = c * vp - sn * vq;
                        QD_TB_V(i, q) = sn * vp + c * vq;
                    }
                }
            }
            QD_EW_SYNC();
        }
        if (qd_ew_max(W.T.B.red) == 0.0) break;                           // (uniform) no pair rotated in this sweep
    }
    // ---- 4. weights and populations ----
    QD_EW_EACH(k) { W.T.B.red[k] = k < s ? -QD_TB_A(k, k) : -INFINITY; }
    const double lmin = -qd_ew_max(W.T.B.red);
    QD_EW_EACH(k) {
        double w = 0.0;
        if (k < s) {
            const double a = QD_TB_A(k, k);
            w = exp(-(((a - lmin) * tusc) / kT));           // (0 / kT = 0: the lowest level has weight 1 at any kT)
            W.T.lam[k] = dmin + a * tusc;
            W.T.w[k] = w;
        }
        W.T.B.red[k] = w;
    }
    const double Z = qd_ew_sum(W.T.B.red);
    QD_EW_EACH(k) { W.T.B.red[k] = k < s ? -W.T.w[k] : -INFINITY; }
    const double wtail = -qd_ew_max(W.T.B.red);
    const double iZ = 1.0 / Z;
    QD_EW_EACH(i) {
        if (i < s) {
            const int off = W.st_off[i], sz = W.st_sz[i];
            double acc = 0.0;
            for (int j = 0; j < sz; ++j) {
                const int k = W.mem[off + j];
                const double v = QD_TB_V(i, k);
                acc = fma(W.T.w[k], v * v, acc);
            }
            W.T.pop[i] = acc * iZ;
        }
    }
    if (QD_EW_LANE0) W.T.ztail = wtail * iZ;
    QD_EW_SYNC();
    return sweeps;
}

#if defined(__HIPCC__)
#include "qd_grid.h"            // QdAffineQuery, qd_query_live (qd_query.h)

#define QD_THG_BLOCKS 4096      // blocks per slot at the most; the blocks of a slot stride over its points

// the two cores behind one kernel body: the per-component one on its workspace, qd_thermal_solve on a bare QdThermalWs
__device__ __forceinline__ QdThermalWs& qd_thg_state(QdThermalBlocksWs& W) { return W.T; }
__device__ __forceinline__ QdThermalWs& qd_thg_state(QdThermalWs& W) { return W; }
__device__ __forceinline__ int qd_thg_solve(QdThermalBlocksWs& W, int s, double kT) { return qd_thermal_blocks_solve(W, s, kT); }
__device__ __forceinline__ int qd_thg_solve(QdThermalWs& W, int s, double kT) { return qd_thermal_solve(W, s, kT); }

// ---------------------------------------------------------------------------------------------------------------
// The thermal state of the live records of a grid launch, one point per wavefront, in place of the ground-state stage: blocks
// of ONE wave, grid = (min(n, QD_THG_BLOCKS), slots).  WS = QdThermalBlocksWs: the per-component core, the open regime's.
// WS = QdThermalWs: qd_thermal_solve on the whole block, the closed regime's -- a closed list is ONE total-charge sector, whose
// states hops connect: one component, nothing for the schedule to skip, and the component bookkeeping and the smaller number
// of blocks per CU cost 20 to 40 % there (measured).  Point p < n = nx*ny of slot k (query base + k, SP records per slot):
// reads the record and the slot's parameter copy, runs qd_levels_record -> the core -> qd_thermal_moments and
// writes the sensor constant to the slot's zraw and the occupations to the slot's occ, where the sensor stage and
// qd_k_query_write find them (c0 by the operations of qd_k_thermal), and var_dst[(q n + p) N + d], ztail_dst[q n + p] (either
// may be null) of the caller's rows; a query that is not live is rendered like any other and writes no caller's row
// (qd_k_query_write).  The inert records n .. SP-1 are not touched.  A record without a valid state counts as |0..0>.
// ---------------------------------------------------------------------------------------------------------------
template <int N, class WS>
__global__ void __launch_bounds__(64)
qd_k_thermal_grid(QdAffineQuery Q, int base, int B, int n, int SP, int kept, const double* __restrict__ kT_dev,
                  const double* __restrict__ sparams, const QdPixelRec* __restrict__ recs, double* __restrict__ zraw,
                  double* __restrict__ socc, double* __restrict__ var_dst, double* __restrict__ ztail_dst) {
    constexpr int G = N + 1;
    __shared__ WS W;
    QdThermalWs& T = qd_thg_state(W);
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.y, q = base + k;
    const bool live = qd_query_live(Q.env_of_query, nullptr, q, B, N);
    const double kT = kT_dev[q];
    const double* par = sparams + (size_t)k * L.size;
    for (int p = blockIdx.x; p < n; p += gridDim.x) {
        const size_t sp = (size_t)k * SP + p;
        const QdPixelRec* rec = recs + sp;
        const size_t dst = (size_t)q * n + p;
        int nv = rec->nvalid < kept ? rec->nvalid : kept;
        nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
        nv = __builtin_amdgcn_readfirstlane(nv);
        if (nv > 0) {
            qd_levels_record<N>(T.B, rec, nv);
            qd_thg_solve(W, nv, kT);
            qd_thermal_moments<N>(T, rec, nv);
        }
        if (threadIdx.x == 0) {
            // c0 = 2 b + a (2 (Ns - v''_s) + 1), b = sum_i A[N][i] (<n_i> - v''_i): the operations of qd_k_gs_select
            double b = 0.0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const double o = nv > 0 ? T.occ[i] : 0.0;
                b = fma(par[L.cdd_inv + N * G + i], o - rec->vpp[i], b);
                socc[sp * N + i] = o;
                if (var_dst && live) var_dst[dst * N + i] = nv > 0 ? T.var[i] : 0.0;
            }
            const double vs = rec->vpp[N];
            const double Ns = rint(vs);
            zraw[sp] = 2.0 * b + par[L.cdd_inv + N * G + N] * (2.0 * (Ns - vs) + 1.0);
            if (ztail_dst && live) ztail_dst[dst] = nv > 0 ? T.ztail : 1.0;
        }
        __syncthreads();                                   // (lane 0 has read W before the next point overwrites it)
    }
}
#endif  // __HIPCC__

#undef QD_TB_A
#undef QD_TB_V
