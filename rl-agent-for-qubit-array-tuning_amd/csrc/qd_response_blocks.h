// qd_response_blocks.h -- the charge response of a point in the thermal state, PER HOP COMPONENT (qd_scan_grid_response): the
// contract of qd_response_solve (qd_response.h) -- chi_n, chi_t, the jacobian and dc0/dv of a record from the slot's parameter
// copy -- as an epilogue of qd_thermal_blocks_solve (qd_thermal_blocks.h), which leaves the decomposition block diagonal over the
// connected components of the coupling pattern.  The ingredients of the response do not couple states of different components:
//     V is block diagonal;  X = n_k is diagonal in the charge basis;  X = T_d has an entry only where H_t has one, so a
//     non-zero X_ij links i and j;  hence G = V^T X V and D o G are block diagonal.
// Only Z, p_a = w_a / Z and <X> = sum_a p_a G_aa are global.  With the formulas of qd_response.h:
//     D_ab                       for the pairs a < b of ONE component (expm1 on differences of the shifted, scaled diagonal times tusc)
//     G_ab = sum_{m in comp} V_ma X_mj V_jb    for the pairs a <= b of one component, m over that component's members
//     xbar = sum_a p_a G_aa      over all levels
//     dP_m = sum_{a, b in comp(m)} V_ma (D o G)_ab V_mb + pop_m xbar / kT;     chi[i][X] = sum_m n_m[i] dP_m
// A single state has G_aa = X_aa and the diagonal and xbar terms only.  Level a is column a of V: it belongs to the component of
// state a, whose members W.TB.mem lists from W.TB.st_off[a] on, W.TB.st_sz[a] of them in increasing order.
//
// Schedule: that of qd_response.h in LOCAL indices.  Lane (a, h) -- state a = lane & 31, half h = lane >> 5 -- takes the pairs of
// level a with the levels b = mem[off + (la + k) mod s_c], la the local index of a, for the offsets k = h, h + 2, ... <= s_c / 2
// (qd_response_pair with the component's size), and the dP pass gives lane (m, h) the rows of comp(m) of parity h.  A lane's trip
// counts are those of ITS component, read from the tables that qd_thermal_blocks_solve wrote for the current point; the largest
// component sets the time of a pass, about s_max^3 / 4 fused multiply-adds where the whole block needs s^3 / 4.  Entries of A
// between different components are neither read nor written.  Everything a second point of a persistent block could inherit
// (ek, p_a, D, G_aa, x, the neighbour table, dP, tusc) is written for the current point before it is read.
//
// The chain rule and the neighbour table are those of qd_response_solve, operation for operation, on this workspace (they are
// repeated here and not shared: qd_response.h and the kernels built from it stay as they are).
//
// LDS: the embedded QdThermalBlocksWs is unchanged (24 680 B).  After the solve the vectors of its QdThermalWs are free and are
// used under the names of qd_response.h; the component tables (ma, mem, st_off, st_sz) are read as the solver left them.  This
// struct adds dP (256 B), tusc (8 B) and the neighbour table (64 B): sizeof(QdResponseBlocksWs) = 25 008 B, six single-wave
// blocks per CU still (6 x 25 008 = 150 048 of 163 840; the grid kernel adds 256 B for the two axis directions).
// qd_k_thermal_grid_response<8, QdResponseBlocksWs> for gfx950: 237 VGPRs, 106 SGPRs (214 more held in VGPR lanes), no VGPR spill, no
// scratch (the compiler's resource report, -Rpass-analysis=kernel-resource-usage); 25 264 B of LDS per block with the axis
// directions, so the LDS, six blocks per CU, bounds the waves per SIMD, not the registers (two waves per SIMD at 237).
#pragma once
#include "qd_thermal_blocks.h"
#include "qd_response.h"

struct QdResponseBlocksWs {
    QdThermalBlocksWs TB;
    double dP[QD_LV_MAX];                   // d P_m / d eps of the current perturbation
    double tusc;                            // the power of two that unscales the diagonal (qd_response_blocks_scale)
    unsigned char nb[QD_LV_MAX][2];         // partners of state m over the current pair: [0] d -> d+1, [1] d+1 -> d; 255: none
};

static_assert(sizeof(QdResponseBlocksWs) == 25008, "the header comment states the size");
static_assert(6 * sizeof(QdResponseBlocksWs) <= 160 * 1024, "six single-wave blocks per CU");

#define QD_RB_A(i, j) T.B.A[(i) * QD_LV_LD + (j)]
#define QD_RB_V(i, j) T.V[(i) * QD_LV_LD + (j)]
// the free vectors of the embedded QdThermalWs `T`, the places of qd_response.h
#define QD_RB_EK T.B.al
#define QD_RB_PA T.B.be
#define QD_RB_GD T.w
#define QD_RB_X T.B.x
#define QD_RB_CHIN T.B.lo
#define QD_RB_CHIT T.B.hi
#define QD_RB_JACG T.B.v
#define QD_RB_JACB T.B.w
#define QD_RB_DC0 T.c

// The slope of the sensor expression at c0: S'(c0) = sum_{k=-5..4} -2 rr_k / (gamma (rr_k^2 + 1)^2), rr_k = (c0 + 2 a k) / gamma,
// the expression of qd_k_points_dsignal (qd_response.h) operation for operation.
QD_HD double qd_sensor_slope(double c0, double a, double gamma) {
    double ds = 0.0;
#pragma unroll
    for (int kk = -QD_NPEAK; kk < QD_NPEAK; ++kk) {
        const double dF = c0 + 2.0 * a * (double)kk;
        const double rr = dF / gamma;
        const double den = rr * rr + 1.0;
        ds -= 2.0 * rr / (gamma * den * den);
    }
    return ds;
}

// BEFORE qd_thermal_blocks_solve, on the block as qd_levels_record or qd_levels_load_packed left it (read only): the unscaling
// factor of its step 1, by the same operations in the same order (qd_response_scale on this workspace).
QD_HD void qd_response_blocks_scale(QdResponseBlocksWs& W, int s) {
    QdThermalWs& T = W.TB.T;
    double tusc = 1.0;
    if (s > 1) {
        QD_EW_EACH(i) { T.B.red[i] = i < s ? -QD_RB_A(i, i) : -INFINITY; }
        const double dmin = -qd_ew_max(T.B.red);
        QD_EW_EACH(i) {
            double rs = 0.0;
            if (i < s)
                for (int j = 0; j < s; ++j) {
                    const double dii = QD_RB_A(i, i) - dmin;
                    rs += fabs(j < i ? QD_RB_A(i, j) : (j == i ? dii : QD_RB_A(j, i)));
                }
            T.B.red[i] = rs;
        }
        const double anorm = qd_ew_max(T.B.red);
        double tsc;
        qd_pow2_scale(anorm, tsc, tusc);
    }
    if (QD_EW_LANE0) W.tusc = tusc;
    QD_EW_SYNC();
}

// component of state a (s > 1): offset and size in the member list, local index of a
QD_HD void qd_response_blocks_comp(const QdResponseBlocksWs& W, int a, int& off, int& sz, int& la) {
    off = W.TB.st_off[a]; sz = W.TB.st_sz[a];
    la = __builtin_popcount(W.TB.ma[a] & ((1u << a) - 1u));
}

// AFTER qd_thermal_blocks_solve (s > 1): ek, p_a, and D into the lower triangle of A, inside the components.
QD_HD void qd_response_blocks_begin(QdResponseBlocksWs& W, int s, double kT) {
    if (s == 1) return;
    QdThermalWs& T = W.TB.T;
    const double tusc = W.tusc, ikT = 1.0 / kT;
    QD_EW_EACH(k) { T.B.red[k] = k < s ? T.w[k] : 0.0; }
    const double iZ = 1.0 / qd_ew_sum(T.B.red);
    QD_EW_EACH(k) {
        if (k < s) { QD_RB_EK[k] = QD_RB_A(k, k) * tusc; QD_RB_PA[k] = T.w[k] * iZ; }
    }
    QD_EW_SYNC();
    QD_EW_EACH(l) {
        const int a = l & 31;
        if (a < s) {
            int off, sz, la;
            qd_response_blocks_comp(W, a, off, sz, la);
            for (int k = l >> 5; k <= (sz >> 1); k += 2) {
                int lb;
                if (k == 0 || !qd_response_pair(sz, la, k, lb)) continue;
                const int b = W.TB.mem[off + lb];
                const double ea = QD_RB_EK[a], eb = QD_RB_EK[b];
                const double plo = ea <= eb ? QD_RB_PA[a] : QD_RB_PA[b];
                const double x = fabs(ea - eb) * ikT;
                double phi = 1.0;
                if (x > 0.0) phi = -expm1(-x) / x;
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                QD_RB_A(hi, lo) = -(plo * phi) * ikT;
            }
        }
    }
    QD_EW_SYNC();
}

// One perturbation -> W.dP[0 .. s-1], the contract of qd_response_apply.  The table of a sparse X respects the components (a
// partner in another component would meet exact zeros of V and add nothing).  Needs qd_response_blocks_begin.
template <bool HOP>
QD_HD void qd_response_blocks_apply(QdResponseBlocksWs& W, int s, double kT) {
    if (s == 1) {                                             // (uniform) one state: P = 1 whatever the Hamiltonian
        if (QD_EW_LANE0) W.dP[0] = 0.0;
        QD_EW_SYNC();
        return;
    }
    QdThermalWs& T = W.TB.T;
    const double ikT = 1.0 / kT;
    // G = V^T X V over the pairs a <= b of one component; off the diagonal times D, into the upper triangle
    QD_EW_EACH(l) {
        const int a = l & 31;
        if (a < s) {
            int off, sz, la;
            qd_response_blocks_comp(W, a, off, sz, la);
            for (int k = l >> 5; k <= (sz >> 1); k += 2) {
                int lb;
                if (!qd_response_pair(sz, la, k, lb)) continue;
                const int b = W.TB.mem[off + lb];
                double acc = 0.0;
                for (int im = 0; im < sz; ++im) {
                    const int m = W.TB.mem[off + im];
                    if (HOP) {
                        const int j0 = W.nb[m][0], j1 = W.nb[m][1];
                        if (j0 == QD_RS_NONE && j1 == QD_RS_NONE) continue;
                        double y = 0.0;
                        if (j0 != QD_RS_NONE) y = QD_RB_X[m] * QD_RB_V(j0, b);
                        if (j1 != QD_RS_NONE) y = fma(QD_RB_X[32 + m], QD_RB_V(j1, b), y);
                        acc = fma(QD_RB_V(m, a), y, acc);
                    } else {
                        acc = fma(QD_RB_V(m, a) * QD_RB_X[m], QD_RB_V(m, b), acc);
                    }
                }
                if (k == 0) QD_RB_GD[a] = acc;
                else if (a < b) QD_RB_A(a, b) = acc * QD_RB_A(b, a);
                else QD_RB_A(b, a) = acc * QD_RB_A(a, b);
            }
        }
    }
    QD_EW_SYNC();
    QD_EW_EACH(a) { T.B.red[a] = a < s ? QD_RB_PA[a] * QD_RB_GD[a] : 0.0; }
    const double xbar = qd_ew_sum(T.B.red);
    // dP_m = sum_{a in comp(m)} V_ma (D_aa G_aa V_ma + 2 sum_{b > a in comp(m)} (D o G)_ab V_mb): lane (m, h) takes the rows of parity h
    QD_EW_EACH(l) {
        const int m = l & 31;
        double acc = 0.0;
        if (m < s) {
            const int off = W.TB.st_off[m], sz = W.TB.st_sz[m];
            for (int ia = l >> 5; ia < sz; ia += 2) {
                const int a = W.TB.mem[off + ia];
                const double vma = QD_RB_V(m, a);
                double in = -0.5 * (QD_RB_PA[a] * ikT) * QD_RB_GD[a] * vma;
                for (int ib = ia + 1; ib < sz; ++ib) {
                    const int b = W.TB.mem[off + ib];              // (the members of a component are listed in increasing order: a < b)
                    in = fma(QD_RB_A(a, b), QD_RB_V(m, b), in);
                }
                acc = fma(2.0 * vma, in, acc);
            }
        }
        T.B.red[l] = acc;
    }
    QD_EW_SYNC();
    QD_EW_EACH(m) {
        if (m < s) W.dP[m] = (T.B.red[m] + T.B.red[32 + m]) + T.pop[m] * xbar * ikT;
    }
    QD_EW_SYNC();
}

// neighbour table and coefficients of pair d (tc_d != 0): qd_response_hop_table on this workspace
template <int N>
QD_HD void qd_response_blocks_hop_table(QdResponseBlocksWs& W, const QdPixelRec* rec, int nv, int d) {
    QdThermalWs& T = W.TB.T;
    const int q = N - 2 - d;
    const unsigned tcq = 1u << (4 * q);
    const double tc = rec->tc[d];
    QD_EW_EACH(m) {
        if (m < nv) {
            const unsigned ci = T.B.code[m];
            const int nd = rec->fl[d] + (int)((ci >> (4 * (q + 1))) & 3u) - 1;
            const int nd1 = rec->fl[d + 1] + (int)((ci >> (4 * q)) & 3u) - 1;
            int j0 = QD_RS_NONE, j1 = QD_RS_NONE;
            for (int j = 0; j < nv; ++j) {
                const unsigned cj = T.B.code[j];
                if (qd_gs_hop(ci, cj, tcq)) {
                    if ((int)cj - (int)ci < 0) j0 = j; else j1 = j;
                }
            }
            const double p0 = (double)nd * (double)(nd1 + 1), p1 = (double)nd1 * (double)(nd + 1);
            QD_RB_X[m] = j0 != QD_RS_NONE && p0 > 0.0 ? -tc * qd_sqrt1(p0) : 0.0;
            QD_RB_X[32 + m] = j1 != QD_RS_NONE && p1 > 0.0 ? -tc * qd_sqrt1(p1) : 0.0;
            W.nb[m][0] = (unsigned char)j0; W.nb[m][1] = (unsigned char)j1;
        }
    }
    QD_EW_SYNC();
}

// The response of a record, behind qd_response_blocks_scale, qd_levels_record, qd_thermal_blocks_solve and qd_thermal_moments
// (nv >= 1), or of a record without a valid state (nv == 0: counts as |0..0>): the contract of qd_response_solve.
// -> QD_RB_CHIN, QD_RB_CHIT, QD_RB_JACG, QD_RB_JACB, QD_RB_DC0 of W.TB.T, valid in every lane after the call.  nv <= 1: chi and
// the jacobian are zero exactly.
template <int N>
QD_HD void qd_response_blocks_solve(QdResponseBlocksWs& W, const QdPixelRec* rec, int nv, double kT, const double* par) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N;
    QdThermalWs& T = W.TB.T;
    const QdLayout L = qd_layout(N);
    if (nv <= 1) {
        QD_EW_EACH(l) { QD_RB_CHIN[l] = 0.0; QD_RB_CHIT[l] = 0.0; }
        QD_EW_SYNC();
    } else {
        qd_response_blocks_begin(W, nv, kT);
        for (int k = 0; k < N; ++k) {
            QD_EW_EACH(m) { if (m < nv) QD_RB_X[m] = qd_response_occ<N>(rec, m, k); }
            QD_EW_SYNC();
            qd_response_blocks_apply<false>(W, nv, kT);
            QD_EW_EACH(i) {
                if (i < N) {
                    double c = 0.0;
                    for (int m = 0; m < nv; ++m) c = fma(qd_response_occ<N>(rec, m, i), W.dP[m], c);
                    QD_RB_CHIN[i * N + k] = c;
                }
            }
            QD_EW_SYNC();
        }
        for (int d = 0; d < NB; ++d) {
            if (rec->tc[d] == 0.0) {                          // (uniform) the pair does not couple: an exact zero column
                QD_EW_EACH(i) { if (i < N) QD_RB_CHIT[i * NB + d] = 0.0; }
                QD_EW_SYNC();
                continue;
            }
            qd_response_blocks_hop_table<N>(W, rec, nv, d);
            qd_response_blocks_apply<true>(W, nv, kT);
            QD_EW_EACH(i) {
                if (i < N) {
                    double c = 0.0;
                    for (int m = 0; m < nv; ++m) c = fma(qd_response_occ<N>(rec, m, i), W.dP[m], c);
                    QD_RB_CHIT[i * NB + d] = c;
                }
            }
            QD_EW_SYNC();
        }
    }
    // the chain rule of qd_response_solve
    const double* A = par + L.cdd_inv;
    const double* cgd = par + L.cgd;
    QD_EW_EACH(l) {
        for (int e = l; e < N * V; e += 64) {
            const int i = e / V, j = e - i * V;
            double acc = 0.0;
            for (int r = 0; r < N; ++r) {
                double u = 0.0;
                for (int k = 0; k < N; ++k) u = fma(QD_RB_CHIN[i * N + k], A[k * G + r], u);
                acc = fma(u, cgd[r * V + j], acc);
            }
            acc *= -2.0;
            for (int d = 0; d < NB; ++d) {
                const double dvb = j < G ? par[L.cbg + d * G + j] : (j - G == d ? 1.0 : 0.0);
                acc = fma(QD_RB_CHIT[i * NB + d], -par[L.alpha + d] * dvb, acc);
            }
            if (j < N) QD_RB_JACG[i * N + j] = acc; else QD_RB_JACB[i * N + j - N] = acc;
        }
    }
    QD_EW_SYNC();
    QD_EW_EACH(j) {
        if (j < V) {
            double b = 0.0;
            for (int i = 0; i < N; ++i) {
                const double jij = j < N ? QD_RB_JACG[i * N + j] : QD_RB_JACB[i * N + j - N];
                b = fma(A[N * G + i], jij - cgd[i * V + j], b);
            }
            QD_RB_DC0[j] = 2.0 * b - 2.0 * A[N * G + N] * cgd[N * V + j];
        }
    }
    QD_EW_SYNC();
}

// The physical direction u = dv/ds of one step of an axis scalar of a grid, entry i of 2N: dir itself in the physical frame;
// in the virtual frame u[i] = sum_j vgm[i][j] dir[j] over the G gates (index order, fma from 0.0) with the slot's matrix, and
// the barriers pass through.
template <int N>
QD_HD double qd_grid_axis_direction(const double* st, int frame, const double* dir, int i) {
    constexpr int G = N + 1;
    if (frame == QD_SCAN_PHYSICAL || i >= G) return dir[i];
    const double* vgm = st + qd_layout(N).s_vgm + i * G;
    double u = 0.0;
    for (int j = 0; j < G; ++j) u = fma(vgm[j], dir[j], u);
    return u;
}

#if defined(__HIPCC__)
#include "qd_response_grid.h"    // QdGridResponseDst

// the two epilogues behind one kernel body: the per-component one on its workspace, qd_response_solve on a QdResponseWs
__device__ __forceinline__ QdThermalWs& qd_rsg_state(QdResponseBlocksWs& W) { return W.TB.T; }
__device__ __forceinline__ QdThermalWs& qd_rsg_state(QdResponseWs& W) { return W.T; }
__device__ __forceinline__ void qd_rsg_scale(QdResponseBlocksWs& W, int s) { qd_response_blocks_scale(W, s); }
__device__ __forceinline__ void qd_rsg_scale(QdResponseWs& W, int s) { qd_response_scale(W, s); }
__device__ __forceinline__ void qd_rsg_thermal(QdResponseBlocksWs& W, int s, double kT) { qd_thermal_blocks_solve(W.TB, s, kT); }
__device__ __forceinline__ void qd_rsg_thermal(QdResponseWs& W, int s, double kT) { qd_thermal_solve(W.T, s, kT); }
template <int N>
__device__ __forceinline__ void qd_rsg_solve(QdResponseBlocksWs& W, const QdPixelRec* rec, int nv, double kT, const double* par) {
    qd_response_blocks_solve<N>(W, rec, nv, kT, par);
}
template <int N>
__device__ __forceinline__ void qd_rsg_solve(QdResponseWs& W, const QdPixelRec* rec, int nv, double kT, const double* par) {
    qd_response_solve<N>(W, rec, nv, kT, par);
}

// ---------------------------------------------------------------------------------------------------------------
// qd_k_thermal_grid with the response behind it: the same grid, the same calls in the same order on the embedded workspace, so
// zraw, socc, var_dst and ztail_dst get the bits of qd_k_thermal_grid.  After lane 0 has read occ, var and ztail the epilogue
// runs and the point writes its rows at dst = q n + p:  chi, the jacobian, dsignal = S'(c0) dc0/dv with the slope at the c0 that
// went to zraw and the slot's constant peak width par[scal + 1], and the two a grid is plotted with,
//     docc_axes[i][a] = sum_j jac[i][j] u_a[j],   dsignal_axes[a] = sum_j dsignal[j] u_a[j]     (j = 0 .. 2N-1 in order, fma from 0.0)
// u_x, u_y the physical directions of the two axis scalars (qd_grid_axis_direction): derivatives per unit of sx / sy.
// WS = QdResponseBlocksWs: the per-component epilogue, the open regime's.  WS = QdResponseWs: qd_response_solve behind
// qd_thermal_solve, the closed regime's (one component per list).  A query that is not live is rendered like any other and
// writes no caller's row; the inert records n .. SP-1 are not touched; a record without a valid state counts as |0..0>.
// ---------------------------------------------------------------------------------------------------------------
template <int N, class WS>
__global__ void __launch_bounds__(64)
qd_k_thermal_grid_response(QdAffineQuery Q, int base, int B, int n, int SP, int kept, const double* __restrict__ kT_dev,
                           const double* __restrict__ sparams, const double* __restrict__ sstate,
                           const QdGridAxes* __restrict__ axes, const QdPixelRec* __restrict__ recs, double* __restrict__ zraw,
                           double* __restrict__ socc, double* __restrict__ var_dst, double* __restrict__ ztail_dst,
                           QdGridResponseDst R) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N, X = 2 * N - 1;
    __shared__ WS W;
    __shared__ double U[2][V];
    QdThermalWs& T = qd_rsg_state(W);
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.y, q = base + k;
    const int l = (int)threadIdx.x;
    const bool live = qd_query_live(Q.env_of_query, nullptr, q, B, N);
    const double kT = kT_dev[q];
    const double* par = sparams + (size_t)k * L.size;
    if (l < 2 * V) {
        const int a = l / V, i = l - a * V;
        const QdGridAxes* ax = axes + k;
        U[a][i] = qd_grid_axis_direction<N>(sstate + (size_t)k * L.s_size, ax->frame, a ? ax->dy : ax->dx, i);
    }
    __syncthreads();
    for (int p = blockIdx.x; p < n; p += gridDim.x) {
        const size_t sp = (size_t)k * SP + p;
        const QdPixelRec* rec = recs + sp;
        const size_t dst = (size_t)q * n + p;
        int nv = rec->nvalid < kept ? rec->nvalid : kept;
        nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
        nv = __builtin_amdgcn_readfirstlane(nv);
        if (nv > 0) {
            qd_levels_record<N>(T.B, rec, nv);
            qd_rsg_scale(W, nv);
            qd_rsg_thermal(W, nv, kT);
            qd_thermal_moments<N>(T, rec, nv);
        }
        // (qd_k_thermal_grid, operation for operation; every lane holds c0, lane 0 writes)
        double b = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double o = nv > 0 ? T.occ[i] : 0.0;
            b = fma(par[L.cdd_inv + N * G + i], o - rec->vpp[i], b);
            if (l == 0) {
                socc[sp * N + i] = o;
                if (var_dst && live) var_dst[dst * N + i] = nv > 0 ? T.var[i] : 0.0;
            }
        }
        const double vs = rec->vpp[N];
        const double Ns = rint(vs);
        const double c0 = 2.0 * b + par[L.cdd_inv + N * G + N] * (2.0 * (Ns - vs) + 1.0);
        if (l == 0) {
            zraw[sp] = c0;
            if (ztail_dst && live) ztail_dst[dst] = nv > 0 ? T.ztail : 1.0;
        }
        __syncthreads();                                   // (lane 0 has read occ, var and ztail before the epilogue reuses the vectors)
        if (!live) continue;                               // (uniform over the block: no caller's row, nothing to compute)
        qd_rsg_solve<N>(W, rec, nv, kT, par);
        const double ds = qd_sensor_slope(c0, par[L.cdd_inv + N * G + N], par[L.scal + 1]);
        if (R.chi)
            for (int e = l; e < N * X; e += 64) {
                const int i = e / X, c = e - i * X;
                R.chi[dst * (N * X) + e] = c < N ? QD_RB_CHIN[i * N + c] : QD_RB_CHIT[i * NB + c - N];
            }
        if (R.jac)
            for (int e = l; e < N * V; e += 64) {
                const int i = e / V, c = e - i * V;
                R.jac[dst * (N * V) + e] = c < N ? QD_RB_JACG[i * N + c] : QD_RB_JACB[i * N + c - N];
            }
        if (R.dsignal && l < V) R.dsignal[dst * V + l] = QD_RB_DC0[l] * ds;
        if (R.docc_axes && l < 2 * N) {
            const int i = l >> 1, a = l & 1;
            double acc = 0.0;
            for (int j = 0; j < V; ++j) acc = fma(j < N ? QD_RB_JACG[i * N + j] : QD_RB_JACB[i * N + j - N], U[a][j], acc);
            R.docc_axes[dst * (2 * N) + l] = acc;
        }
        if (R.dsignal_axes && l < 2) {
            double acc = 0.0;
            for (int j = 0; j < V; ++j) acc = fma(QD_RB_DC0[j] * ds, U[l][j], acc);
            R.dsignal_axes[dst * 2 + l] = acc;
        }
        __syncthreads();                                   // (the lanes have read W before the next point overwrites it)
    }
}
#endif  // __HIPCC__

#undef QD_RB_A
#undef QD_RB_V
#undef QD_RB_EK
#undef QD_RB_PA
#undef QD_RB_GD
#undef QD_RB_X
#undef QD_RB_CHIN
#undef QD_RB_CHIT
#undef QD_RB_JACG
#undef QD_RB_JACB
#undef QD_RB_DC0
