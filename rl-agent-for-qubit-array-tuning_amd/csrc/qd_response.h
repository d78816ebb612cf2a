// qd_response.h -- the charge response of a point in the thermal state (qd_eval_points_response): how the thermal occupations
// <n_i> of qd_thermal.h move with the terms of the Hamiltonian and, through them, with the voltages.  It is an epilogue of
// qd_thermal_solve: after it the wave holds the whole decomposition H = V diag(lam) V^T and the weights w in LDS, and the block A
// is free again.  ONE POINT PER WAVEFRONT, as the siblings.  The kept list is held FIXED: this is the derivative of the truncated
// K-state model at this point, not of the infinite system.
//
// For a perturbation H + eps X and an observable O, in the eigenbasis, with p_a = w_a / Z:
//     d<O>/d eps = sum_ab D_ab O_ab X_ba + (1 / kT) <O> <X>
//     D_aa = -p_a / kT,   D_ab = -p_lo phi(x) / kT  (a != b),  lo the lower level of the pair, x = |lam_a - lam_b| / kT,
//     phi(x) = -expm1(-x) / x,  phi(0) = 1:  the divided difference (p_a - p_b) / (lam_a - lam_b), continuous across an exact
//     degeneracy, so the result does not depend on the basis the Jacobi leaves inside a cluster.  Level differences come from the
//     shifted, scaled diagonal (a_k * tusc), not from lam = dmin + a_k tusc, which has lost them to the offset.
// The observables are the occupations, diagonal in the charge basis, so only the diagonal of d rho is needed:
//     G = V^T X V;   dP_m = sum_ab V_ma (D_ab G_ab) V_mb + pop_m <X> / kT,  <X> = sum_a p_a G_aa;   chi[i][X] = sum_m n_m[i] dP_m
// Perturbations:  X = n_k (columns 0 .. N-1), diagonal in the charge basis;  X = T_d (columns N .. 2N-2), the pair-d part of H_t at
// the point's own tc_d, i.e. d/d(ln tc_d): sparse, at most two partners per state (one electron moved d -> d+1 or d+1 -> d).  H_t
// is gone after the Jacobi; pattern and coefficients of pair d are rebuilt from the delta codes with qd_gs_hop, as
// qd_levels_record builds them.  A pair with tc_d == 0 is skipped: an exact zero column.
// The chain rule to the voltages v = (vg[0..N], vb[0..N-2]) runs on the slot's parameter copy:
//     jac[i][j] = sum_k chi[i][k] Lam[k][j] + sum_d chi[i][N+d] Gam[d][j],   Lam = -2 cdd_inv[:N,:N] cgd[:N],
//     Gam[d][j] = -alpha_d d(vb_eff_d)/dv_j  (cbg[d][j] for a gate, 1 for the pair's own barrier)
//     dc0[j]   = 2 sum_i A_full[N][i] (jac[i][j] - cgd[i][j]) - 2 A_full[N][N] cgd[N][j]      (Ns = rint(v''_s) is piecewise constant)
//
// G and D are symmetric: D lives in the lower triangle of A, D o G in the upper one, G_aa beside them; pairs (a, b) are dealt to
// the lanes cyclically, lane (a, h) takes b = (a + k) mod s for k = h, h + 2, ..., so that the 32 lanes of a half-wave read
// consecutive entries of a row of V (stride 33: conflict-free) and every lane has the same trip count.  All loop bounds and the
// partner tests are wave-uniform.  About 2 s^3 / 2 fused multiply-adds per perturbation, 2 N - 1 perturbations.
//
// LDS: the embedded QdThermalWs is unchanged.  After the solve its vectors are free and are used under the names below (ek, pa,
// gd, x, the results); this struct adds dP (256 B), tusc (8 B) and the neighbour table (64 B): sizeof(QdResponseWs) = 23 120 B,
// seven single-wave blocks per CU still (7 x 23 120 = 161 840 of 163 840).
#pragma once
#include "qd_thermal.h"

struct QdResponseWs {
    QdThermalWs T;
    double dP[QD_LV_MAX];                   // d P_m / d eps of the current perturbation
    double tusc;                            // the power of two that unscales the diagonal (qd_response_scale)
    unsigned char nb[QD_LV_MAX][2];         // partners of state m over the current pair: [0] d -> d+1, [1] d+1 -> d; 255: none
};

static_assert(sizeof(QdResponseWs) == 23120, "the header comment states the size");
static_assert(7 * sizeof(QdResponseWs) <= 160 * 1024, "seven single-wave blocks per CU");

#define QD_RS_NONE 255
#define QD_RS_A(i, j) W.T.B.A[(i) * QD_LV_LD + (j)]
#define QD_RS_V(i, j) W.T.V[(i) * QD_LV_LD + (j)]
// the free vectors of the embedded workspaces under the names of this file
#define QD_RS_EK W.T.B.al                   // [32] level a relative to the shift, units of the input
#define QD_RS_PA W.T.B.be                   // [32] p_a
#define QD_RS_GD W.T.w                      // [32] G_aa (the weights are folded into p_a by then)
#define QD_RS_X W.T.B.x                     // [64] on-site: x_m;  hop: the coefficients of nb[m][0] in [m], of nb[m][1] in [32 + m]
#define QD_RS_CHIN W.T.B.lo                 // [i * N + k]        chi, on-site columns
#define QD_RS_CHIT W.T.B.hi                 // [i * (N-1) + d]    chi, ln tc columns
#define QD_RS_JACG W.T.B.v                  // [i * N + j]        jacobian, columns 0 .. N-1 (the plunger gates)
#define QD_RS_JACB W.T.B.w                  // [i * N + j - N]    jacobian, columns N .. 2N-1 (sensor gate, barriers)
#define QD_RS_DC0 W.T.c                     // [2N] dc0/dv

// BEFORE qd_thermal_solve, on the block as qd_levels_record or qd_levels_load_packed left it (read only): the unscaling factor of
// its step 1, by the same operations in the same order.
QD_HD void qd_response_scale(QdResponseWs& W, int s) {
    double tusc = 1.0;
    if (s > 1) {
        QD_EW_EACH(i) { W.T.B.red[i] = i < s ? -QD_RS_A(i, i) : -INFINITY; }
        const double dmin = -qd_ew_max(W.T.B.red);
        QD_EW_EACH(i) {
            double rs = 0.0;
            if (i < s)
                for (int j = 0; j < s; ++j) {
                    const double dii = QD_RS_A(i, i) - dmin;
                    rs += fabs(j < i ? QD_RS_A(i, j) : (j == i ? dii : QD_RS_A(j, i)));
                }
            W.T.B.red[i] = rs;
        }
        const double anorm = qd_ew_max(W.T.B.red);
        double tsc;
        qd_pow2_scale(anorm, tsc, tusc);
    }
    if (QD_EW_LANE0) W.tusc = tusc;
    QD_EW_SYNC();
}

// The pairs of lane l: a = l & 31 and b = (a + k) mod s for the offsets k = l >> 5, + 2, ... <= s / 2.  With s even the offset s / 2
// meets every pair twice and is taken from the lower half only: qd_response_pair says whether (a, k) is a pair and gives b.
QD_HD bool qd_response_pair(int s, int a, int k, int& b) {
    b = a + k - (a + k >= s ? s : 0);
    return !(2 * k == s && a >= k);
}

// AFTER qd_thermal_solve (s > 1): ek, p_a, and D into the lower triangle of A.
QD_HD void qd_response_begin(QdResponseWs& W, int s, double kT) {
    if (s == 1) return;
    const double tusc = W.tusc, ikT = 1.0 / kT;
    QD_EW_EACH(k) { W.T.B.red[k] = k < s ? W.T.w[k] : 0.0; }
    const double iZ = 1.0 / qd_ew_sum(W.T.B.red);
    QD_EW_EACH(k) {
        if (k < s) { QD_RS_EK[k] = QD_RS_A(k, k) * tusc; QD_RS_PA[k] = W.T.w[k] * iZ; }
    }
    QD_EW_SYNC();
    QD_EW_EACH(l) {
        const int a = l & 31;
        if (a < s) {
            for (int k = l >> 5; k <= (s >> 1); k += 2) {
                int b;
                if (k == 0 || !qd_response_pair(s, a, k, b)) continue;
                const double ea = QD_RS_EK[a], eb = QD_RS_EK[b];
                const double plo = ea <= eb ? QD_RS_PA[a] : QD_RS_PA[b];
                const double x = fabs(ea - eb) * ikT;
                double phi = 1.0;
                if (x > 0.0) phi = -expm1(-x) / x;
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                QD_RS_A(hi, lo) = -(plo * phi) * ikT;
            }
        }
    }
    QD_EW_SYNC();
}

// One perturbation -> W.dP[0 .. s-1].  HOP false: X = diag(QD_RS_X[m]).  HOP true: X_mj = QD_RS_X[m] for j = nb[m][0],
// QD_RS_X[32 + m] for j = nb[m][1] (the caller's table is symmetric).  Needs qd_response_begin.
template <bool HOP>
QD_HD void qd_response_apply(QdResponseWs& W, int s, double kT) {
    if (s == 1) {                                             // (uniform) one state: P = 1 whatever the Hamiltonian
        if (QD_EW_LANE0) W.dP[0] = 0.0;
        QD_EW_SYNC();
        return;
    }
    const double ikT = 1.0 / kT;
    // G = V^T X V over the pairs a <= b; off the diagonal times D, into the upper triangle
    QD_EW_EACH(l) {
        const int a = l & 31;
        if (a < s) {
            for (int k = l >> 5; k <= (s >> 1); k += 2) {
                int b;
                if (!qd_response_pair(s, a, k, b)) continue;
                double acc = 0.0;
                for (int m = 0; m < s; ++m) {
                    if (HOP) {
                        const int j0 = W.nb[m][0], j1 = W.nb[m][1];           // (uniform)
                        if (j0 == QD_RS_NONE && j1 == QD_RS_NONE) continue;
                        double y = 0.0;
                        if (j0 != QD_RS_NONE) y = QD_RS_X[m] * QD_RS_V(j0, b);
                        if (j1 != QD_RS_NONE) y = fma(QD_RS_X[32 + m], QD_RS_V(j1, b), y);
                        acc = fma(QD_RS_V(m, a), y, acc);
                    } else {
                        acc = fma(QD_RS_V(m, a) * QD_RS_X[m], QD_RS_V(m, b), acc);
                    }
                }
                if (k == 0) QD_RS_GD[a] = acc;
                else if (a < b) QD_RS_A(a, b) = acc * QD_RS_A(b, a);
                else QD_RS_A(b, a) = acc * QD_RS_A(a, b);
            }
        }
    }
    QD_EW_SYNC();
    QD_EW_EACH(a) { W.T.B.red[a] = a < s ? QD_RS_PA[a] * QD_RS_GD[a] : 0.0; }
    const double xbar = qd_ew_sum(W.T.B.red);
    // dP_m = sum_a V_ma (D_aa G_aa V_ma + 2 sum_{b > a} (D o G)_ab V_mb): lane (m, h) takes the rows a of parity h
    QD_EW_EACH(l) {
        const int m = l & 31;
        double acc = 0.0;
        if (m < s)
            for (int a = l >> 5; a < s; a += 2) {
                const double vma = QD_RS_V(m, a);
                double in = -0.5 * (QD_RS_PA[a] * ikT) * QD_RS_GD[a] * vma;
                for (int b = a + 1; b < s; ++b) in = fma(QD_RS_A(a, b), QD_RS_V(m, b), in);
                acc = fma(2.0 * vma, in, acc);
            }
        W.T.B.red[l] = acc;
    }
    QD_EW_SYNC();
    QD_EW_EACH(m) {
        if (m < s) W.dP[m] = (W.T.B.red[m] + W.T.B.red[32 + m]) + W.T.pop[m] * xbar * ikT;
    }
    QD_EW_SYNC();
}

// occupation of dot i in state m of the record (qd_thermal_moments)
template <int N>
QD_HD double qd_response_occ(const QdPixelRec* rec, int m, int i) {
    return (double)(rec->fl[i] + (int)(((unsigned)rec->idx[m] >> (2 * (N - 1 - i))) & 3u) - 1);
}

// neighbour table and coefficients of pair d (tc_d != 0) from the delta codes W.T.B.code of qd_levels_record: lane m owns state m
template <int N>
QD_HD void qd_response_hop_table(QdResponseWs& W, const QdPixelRec* rec, int nv, int d) {
    const int q = N - 2 - d;
    const unsigned tcq = 1u << (4 * q);
    const double tc = rec->tc[d];
    QD_EW_EACH(m) {
        if (m < nv) {
            const unsigned ci = W.T.B.code[m];
            const int nd = rec->fl[d] + (int)((ci >> (4 * (q + 1))) & 3u) - 1;
            const int nd1 = rec->fl[d + 1] + (int)((ci >> (4 * q)) & 3u) - 1;
            int j0 = QD_RS_NONE, j1 = QD_RS_NONE;
            for (int j = 0; j < nv; ++j) {
                const unsigned cj = W.T.B.code[j];
                if (qd_gs_hop(ci, cj, tcq)) {
                    if ((int)cj - (int)ci < 0) j0 = j; else j1 = j;
                }
            }
            // (qd_levels_record: exact products in float64; Y < 0: s_j = s_m - e_d + e_{d+1})
            const double p0 = (double)nd * (double)(nd1 + 1), p1 = (double)nd1 * (double)(nd + 1);
            QD_RS_X[m] = j0 != QD_RS_NONE && p0 > 0.0 ? -tc * qd_sqrt1(p0) : 0.0;
            QD_RS_X[32 + m] = j1 != QD_RS_NONE && p1 > 0.0 ? -tc * qd_sqrt1(p1) : 0.0;
            W.nb[m][0] = (unsigned char)j0; W.nb[m][1] = (unsigned char)j1;
        }
    }
    QD_EW_SYNC();
}

// The response of a record, behind qd_response_scale, qd_levels_record, qd_thermal_solve and qd_thermal_moments (nv >= 1), or of
// a record without a valid state (nv == 0: counts as |0..0>, as in qd_k_thermal).  par: the slot's parameter block.
// -> QD_RS_CHIN, QD_RS_CHIT, QD_RS_JACG, QD_RS_JACB, QD_RS_DC0, valid in every lane after the call.  nv <= 1: chi and the
// jacobian are zero exactly.
template <int N>
QD_HD void qd_response_solve(QdResponseWs& W, const QdPixelRec* rec, int nv, double kT, const double* par) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
    if (nv <= 1) {
        QD_EW_EACH(l) { QD_RS_CHIN[l] = 0.0; QD_RS_CHIT[l] = 0.0; }
        QD_EW_SYNC();
    } else {
        qd_response_begin(W, nv, kT);
        for (int k = 0; k < N; ++k) {
            QD_EW_EACH(m) { if (m < nv) QD_RS_X[m] = qd_response_occ<N>(rec, m, k); }
            QD_EW_SYNC();
            qd_response_apply<false>(W, nv, kT);
            QD_EW_EACH(i) {
                if (i < N) {
                    double c = 0.0;
                    for (int m = 0; m < nv; ++m) c = fma(qd_response_occ<N>(rec, m, i), W.dP[m], c);
                    QD_RS_CHIN[i * N + k] = c;
                }
            }
            QD_EW_SYNC();
        }
        for (int d = 0; d < NB; ++d) {
            if (rec->tc[d] == 0.0) {                          // (uniform) the pair does not couple: an exact zero column
                QD_EW_EACH(i) { if (i < N) QD_RS_CHIT[i * NB + d] = 0.0; }
                QD_EW_SYNC();
                continue;
            }
            qd_response_hop_table<N>(W, rec, nv, d);
            qd_response_apply<true>(W, nv, kT);
            QD_EW_EACH(i) {
                if (i < N) {
                    double c = 0.0;
                    for (int m = 0; m < nv; ++m) c = fma(qd_response_occ<N>(rec, m, i), W.dP[m], c);
                    QD_RS_CHIT[i * NB + d] = c;
                }
            }
            QD_EW_SYNC();
        }
    }
    // the chain rule: jac = chi_n Lam + chi_t Gam, Lam = -2 A cgd[:N]: entry (i, j) first folds chi_n[i][:] with A, then with cgd
    const double* A = par + L.cdd_inv;
    const double* cgd = par + L.cgd;
    QD_EW_EACH(l) {
        for (int e = l; e < N * V; e += 64) {
            const int i = e / V, j = e - i * V;
            double acc = 0.0;
            for (int r = 0; r < N; ++r) {
                double u = 0.0;
                for (int k = 0; k < N; ++k) u = fma(QD_RS_CHIN[i * N + k], A[k * G + r], u);
                acc = fma(u, cgd[r * V + j], acc);
            }
            acc *= -2.0;
            for (int d = 0; d < NB; ++d) {
                const double dvb = j < G ? par[L.cbg + d * G + j] : (j - G == d ? 1.0 : 0.0);
                acc = fma(QD_RS_CHIT[i * NB + d], -par[L.alpha + d] * dvb, acc);
            }
            if (j < N) QD_RS_JACG[i * N + j] = acc; else QD_RS_JACB[i * N + j - N] = acc;
        }
    }
    QD_EW_SYNC();
    QD_EW_EACH(j) {
        if (j < V) {
            double b = 0.0;
            for (int i = 0; i < N; ++i) {
                const double jij = j < N ? QD_RS_JACG[i * N + j] : QD_RS_JACB[i * N + j - N];
                b = fma(A[N * G + i], jij - cgd[i * V + j], b);
            }
            QD_RS_DC0[j] = 2.0 * b - 2.0 * A[N * G + N] * cgd[N * V + j];
        }
    }
    QD_EW_SYNC();
}

#if defined(__HIPCC__)
#include "qd_points.h"          // QdPointSlots

// ---------------------------------------------------------------------------------------------------------------
// qd_k_thermal with the response behind it: the same grid, the same calls in the same order on the embedded workspace, so what
// qd_k_thermal writes is written here with the same bits, plus per point q = T.start[k] + j (any of the three may be null)
// chi_dst[q][N][2N-1], jac_dst[q][N][2N] and dc0_dst[q][2N] = dc0/dv, which qd_k_points_dsignal scales to dS/dv in place.
// ---------------------------------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(64)
qd_k_thermal_response(QdPointSlots T, QdThermalKT TK, int CP, int kept, const double* __restrict__ qparams,
                      const QdPixelRec* __restrict__ recs, double* __restrict__ qz, double* __restrict__ qocc,
                      double* __restrict__ var_dst, double* __restrict__ ztail_dst, double* __restrict__ chi_dst,
                      double* __restrict__ jac_dst, double* __restrict__ dc0_dst) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N, X = 2 * N - 1;
    __shared__ QdResponseWs W;
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
            qd_levels_record<N>(W.T.B, rec, nv);
            qd_response_scale(W, nv);
            qd_thermal_solve(W.T, nv, kT);
            qd_thermal_moments<N>(W.T, rec, nv);
        }
        if (threadIdx.x == 0) {
            // (qd_k_thermal, operation for operation)
            double b = 0.0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const double o = nv > 0 ? W.T.occ[i] : 0.0;
                b = fma(par[L.cdd_inv + N * G + i], o - rec->vpp[i], b);
                qocc[sp * N + i] = o;
                if (var_dst) var_dst[q * N + i] = nv > 0 ? W.T.var[i] : 0.0;
            }
            const double vs = rec->vpp[N];
            const double Ns = rint(vs);
            qz[sp] = 2.0 * b + par[L.cdd_inv + N * G + N] * (2.0 * (Ns - vs) + 1.0);
            if (ztail_dst) ztail_dst[q] = nv > 0 ? W.T.ztail : 1.0;
        }
        __syncthreads();                                   // (lane 0 has read occ, var and ztail before the epilogue reuses the vectors)
        qd_response_solve<N>(W, rec, nv, kT, par);
        const int l = (int)threadIdx.x;
        if (chi_dst)
            for (int e = l; e < N * X; e += 64) {
                const int i = e / X, c = e - i * X;
                chi_dst[q * (N * X) + e] = c < N ? QD_RS_CHIN[i * N + c] : QD_RS_CHIT[i * NB + c - N];
            }
        if (jac_dst)
            for (int e = l; e < N * V; e += 64) {
                const int i = e / V, c = e - i * V;
                jac_dst[q * (N * V) + e] = c < N ? QD_RS_JACG[i * N + c] : QD_RS_JACB[i * N + c - N];
            }
        if (dc0_dst && l < V) dc0_dst[q * V + l] = QD_RS_DC0[l];
        __syncthreads();                                   // (the lanes have read W before the next point overwrites it)
    }
}

// ---------------------------------------------------------------------------------------------------------------
// dS/dv behind the unchanged qd_k_points_write, one point per lane: dsignal[q][j] holds dc0/dv_j and is scaled by
//   S'(c0) = sum_{k=-5..4} -2 rr_k / (gamma (rr_k^2 + 1)^2),  rr_k = (c0 + 2 a k) / gamma
// the derivative of the write kernel's expression, with its peak count and its choice of gamma (taken as constant).
// grid = (ceil(C P / block), slots).
// ---------------------------------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(QD_POINTS_BLOCK)
qd_k_points_dsignal(QdPointSlots T, int CP, const double* __restrict__ qparams, const double* __restrict__ qz,
                    double* __restrict__ dsignal) {
    constexpr int G = N + 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.y;
    const int j = blockIdx.x * QD_POINTS_BLOCK + threadIdx.x;
    if (j >= CP || j >= T.cnt[k]) return;
    const double* par = qparams + (size_t)k * L.size;
    const size_t q = (size_t)(T.start[k] + j), sp = (size_t)k * CP + j;
    const double c0 = qz[sp];
    const double a = par[L.cdd_inv + N * G + N];
    const double gamma = T.own_gamma ? par[L.scal + 1] : T.gamma[k];
    double ds = 0.0;
#pragma unroll
    for (int kk = -QD_NPEAK; kk < QD_NPEAK; ++kk) {
        const double dF = c0 + 2.0 * a * (double)kk;
        const double rr = dF / gamma;
        const double den = rr * rr + 1.0;
        ds -= 2.0 * rr / (gamma * den * den);
    }
#pragma unroll
    for (int c = 0; c < V; ++c) dsignal[q * V + c] *= ds;
}
#endif  // __HIPCC__

#undef QD_RS_A
#undef QD_RS_V
