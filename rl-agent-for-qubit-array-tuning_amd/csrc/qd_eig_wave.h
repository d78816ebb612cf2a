// qd_eig_wave.h -- lowest eigenpair of ONE dense real symmetric block of up to 64 states PER WAVEFRONT: the solver of the
// total-charge sectors of 33..64 states that the untruncated charge-state space produces (qd_fullspace.h).  One basis state
// per lane, lane i owning row i of the trailing matrix; the block lives in the wave's LDS.
//
// The numerical recipe is that of qd_eig_lowest (qd_eig.h), step for step, so that its accuracy argument carries over:
//   1. power-of-two scaling to ||A||_inf in [1, 2)
//   2. Householder tridiagonalisation: the column norm, p = A v and v^T p are wave reductions, the rank-2 update is per
//      lane (row i, columns <= i: only the lower triangle is kept, the matrix-vector product reads it through both
//      indices, so the trailing matrix stays exactly symmetric).  Column tails below 1e-100, or below 1e-17 |x0|, are
//      dropped instead of reflected (the guards of qd_eig.h)
//   3. lowest eigenvalue of T: Laguerre from the left of the spectrum, stopped by qd_laguerre_step.  The three-term
//      recurrences are serial in the tridiagonal index; every lane runs them redundantly on the same T (as cheap as one
//      lane running them, and the result needs no broadcast).  With up to 64 rows the minors are renormalised by exact
//      powers of two whenever they leave 1e-100 .. 1e100
//   4. eigenvector of T - lambda by the twisted factorisation (dlar1v), serial and redundant like step 3
//   5. x = Q y by the stored reflectors in reverse (one wave reduction per reflector), normalised.
//
// The same source compiles for the host, where the 64 lanes are a loop: code outside QD_EW_EACH is wave-uniform (every
// lane computes the same value; the host computes it once), code inside runs per lane, and whatever crosses lanes goes
// through the workspace (LDS on the device) with QD_EW_SYNC between writer and reader.  tests/hosttest_wave checks it
// against numpy.linalg.eigh without a GPU.
//
// LDS: the block is stored full, 64 rows of 65 doubles (the odd stride keeps row-wise and column-wise access of the 64
// lanes on different banks), 33 280 B, plus ten 64-double vectors: 38 400 B per wave, four waves per CU.
#pragma once
#include "qd_eig.h"

#define QD_EW_MAX 64              // states of a block, at most: one per lane
#define QD_EW_LD 65               // row stride of the block in the workspace

struct QdEigWaveWs {
    double A[QD_EW_MAX * QD_EW_LD];
    double v[QD_EW_MAX], w[QD_EW_MAX], y[QD_EW_MAX], red[QD_EW_MAX];
    double al[QD_EW_MAX], be[QD_EW_MAX], tau[QD_EW_MAX];
    double um[QD_EW_MAX], lp[QD_EW_MAX], dmk[QD_EW_MAX];
};

#if defined(__HIP_DEVICE_COMPILE__)
// the kernel runs ONE wave per block: __syncthreads is then a wave barrier plus the LDS / memory fence
#define QD_EW_EACH(l) for (int l = (int)(threadIdx.x & 63u), once_ = 1; once_; once_ = 0)
#define QD_EW_SYNC() __syncthreads()
#define QD_EW_LANE0 ((threadIdx.x & 63u) == 0u)
// every lane has written red[lane]
QD_HD double qd_ew_sum(const double* red) {
    QD_EW_SYNC();
    double x = red[threadIdx.x & 63u];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    QD_EW_SYNC();
    return x;
}
QD_HD double qd_ew_max(const double* red) {
    QD_EW_SYNC();
    double x = red[threadIdx.x & 63u];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    QD_EW_SYNC();
    return x;
}
#else
#define QD_EW_EACH(l) for (int l = 0; l < QD_EW_MAX; ++l)
#define QD_EW_SYNC() ((void)0)
#define QD_EW_LANE0 true
// the butterfly of the device version, so that the sums are rounded alike
QD_HD double qd_ew_sum(const double* red) {
    double t[QD_EW_MAX], u[QD_EW_MAX];
    for (int l = 0; l < QD_EW_MAX; ++l) t[l] = red[l];
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < QD_EW_MAX; ++l) u[l] = t[l] + t[l ^ o];
        for (int l = 0; l < QD_EW_MAX; ++l) t[l] = u[l];
    }
    return t[0];
}
QD_HD double qd_ew_max(const double* red) {
    double x = red[0];
    for (int l = 1; l < QD_EW_MAX; ++l) x = fmax(x, red[l]);
    return x;
}
#endif

// Ain: packed lower triangle, s (s + 1) / 2 doubles, 2 <= s <= 64.  Outputs as qd_eig_lowest: lam (units of Ain), the
// unit eigenvector in xout[0 .. s-1] (xout may be Ain: it is written after the last read of Ain), with RESID the absolute
// residual ||A x - lam x||_2, and the Laguerre iterations.  All of them wave-uniform except xout (lane i writes x_i).
template <bool RESID>
QD_HD void qd_eig_wave_lowest(QdEigWaveWs& W, const double* Ain, int s, double& lam_out, double& resid_out, double* xout,
                              int* iters = nullptr) {
#define QD_EW_A(i, j) W.A[(i) * QD_EW_LD + (j)]
#define QD_EW_IX(i, j) ((i) * ((i) + 1) / 2 + (j))
    // ---- 0. the lower triangle into the workspace (row r: lanes 0..r read consecutive doubles) ----
    QD_EW_EACH(l) {
        for (int r = 0; r < s; ++r)
            if (l <= r) QD_EW_A(r, l) = Ain[QD_EW_IX(r, l)];
        W.y[l] = 0.0;
    }
    QD_EW_SYNC();
    // ---- 1. scale ----
    QD_EW_EACH(i) {
        double rs = 0.0;
        if (i < s)
            for (int j = 0; j < s; ++j) rs += fabs(j <= i ? QD_EW_A(i, j) : QD_EW_A(j, i));
        W.red[i] = rs;
    }
    const double anorm = qd_ew_max(W.red);
    double tsc, tusc;
    qd_pow2_scale(anorm, tsc, tusc);
    QD_EW_EACH(i) {
        if (i < s)
            for (int j = 0; j <= i; ++j) QD_EW_A(i, j) *= tsc;
    }
    QD_EW_SYNC();
    // ---- 2. Householder: reflector k zeroes column k below the sub-diagonal; v_k (v_k[k+1] = 1) stays in the zeroed
    // entries, tau_k in W.tau ----
    for (int k = 0; k + 2 < s; ++k) {
        QD_EW_EACH(i) {
            const double xi = (i >= k + 2 && i < s) ? QD_EW_A(i, k) : 0.0;
            W.red[i] = xi * xi;
        }
        const double sigma = qd_ew_sum(W.red);
        const double x0 = QD_EW_A(k + 1, k);
        const bool refl = (sigma > 1e-200) & (sigma > 1e-34 * x0 * x0);   // (see qd_eig_lowest)
        const double mu = qd_sqrt1(fma(x0, x0, sigma) + 1e-300);
        const double v0 = (x0 <= 0.0) ? x0 - mu : -sigma * qd_rcp(x0 + mu);
        const double v0sq = v0 * v0;
        const double t = refl ? 2.0 * v0sq * qd_rcp(sigma + v0sq) : 0.0;
        const double iv0 = refl ? qd_rcp(v0) : 0.0;
        const double akk = QD_EW_A(k, k);
        QD_EW_EACH(i) {
            double vi = 0.0;
            if (i == k + 1) vi = 1.0;
            else if (i >= k + 2 && i < s) { vi = QD_EW_A(i, k) * iv0; QD_EW_A(i, k) = vi; }
            W.v[i] = vi;
        }
        if (QD_EW_LANE0) { W.tau[k] = t; W.be[k] = refl ? mu : x0; W.al[k] = akk; }
        QD_EW_SYNC();
        if (!refl) continue;                                              // (t = 0: the update changes nothing)
        // trailing block B = A[k+1.., k+1..]:  p = t B v,  K = t/2 p.v,  w = p - K v,  B -= v w^T + w v^T
        QD_EW_EACH(i) {
            double p = 0.0;
            if (i >= k + 1 && i < s) {
                double acc = 0.0;
                for (int j = k + 1; j < s; ++j) acc = fma(j <= i ? QD_EW_A(i, j) : QD_EW_A(j, i), W.v[j], acc);
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
                for (int j = k + 1; j <= i; ++j) QD_EW_A(i, j) = fma(-vi, W.w[j], fma(-wi, W.v[j], QD_EW_A(i, j)));
            }
        }
        QD_EW_SYNC();
    }
    {
        const double a0 = QD_EW_A(s - 2, s - 2), b0 = QD_EW_A(s - 1, s - 2), a1 = QD_EW_A(s - 1, s - 1);
        if (QD_EW_LANE0) { W.al[s - 2] = a0; W.be[s - 2] = b0; W.al[s - 1] = a1; W.be[s - 1] = 0.0; }
    }
    QD_EW_SYNC();
    // ---- 3. lowest eigenvalue of T (wave-uniform) ----
    double lo = INFINITY, tscale = 0.0;
    for (int i = 0; i < s; ++i) {
        const double rad = (i > 0 ? fabs(W.be[i - 1]) : 0.0) + fabs(W.be[i]);
        lo = fmin(lo, W.al[i] - rad);
        tscale = fmax(tscale, fabs(W.al[i]) + rad);
    }
    double xl = lo - (1e-3 * tscale + 1e-300);
    {
        bool more = true;
        int myit = 0;
        const double dk = (double)s;
        for (int it = 0; it < QD_EIG_MAXIT && more; ++it) {
            // p, p', p'' at xl; only their ratios matter, so all six are rescaled together by an exact power of two
            // whenever p leaves 1e-100 .. 1e100 (64 rows: the minors can shrink or grow by a factor per row)
            double p0 = 1.0, p1 = W.al[0] - xl, d0 = 0.0, d1 = -1.0, e0 = 0.0, e1 = 0.0;
            for (int i = 1; i < s; ++i) {
                const double a_ = W.al[i] - xl, b2 = W.be[i - 1] * W.be[i - 1];
                const double p2 = fma(a_, p1, -(b2 * p0));
                const double d2 = fma(a_, d1, -(b2 * d0)) - p1;
                const double e2 = fma(a_, e1, -(b2 * e0)) - 2.0 * d1;
                p0 = p1; p1 = p2; d0 = d1; d1 = d2; e0 = e1; e1 = e2;
                const double ap = fabs(p1);
                if ((ap > 1e100) | ((ap < 1e-100) & (ap > 0.0))) {
                    double dn, up;
                    qd_pow2_scale(p1, dn, up);
                    p0 *= dn; p1 *= dn; d0 *= dn; d1 *= dn; e0 *= dn; e1 *= dn;
                }
            }
            more = qd_laguerre_step(dk, p1, d1, e1, tscale, xl);
            ++myit;
        }
        if (iters) *iters = myit;
    }
    const double lam = xl;
    // ---- 4. eigenvector of T by the twisted factorisation of T - lam (see qd_eig_lowest; wave-uniform) ----
    {
        const double pivmin = 2.3e-16 * tscale + 1e-300;
        double dm = W.al[s - 1] - lam;
        if (QD_EW_LANE0) W.dmk[s - 1] = dm;
        for (int i = s - 2; i >= 0; --i) {
            if (fabs(dm) < pivmin) dm = -pivmin;
            const double u = W.be[i] * qd_rcp(dm);
            dm = (W.al[i] - lam) - u * W.be[i];
            if (QD_EW_LANE0) { W.um[i] = u; W.dmk[i] = dm; }
        }
        QD_EW_SYNC();
        double dp = W.al[0] - lam;
        double gbest = fabs(W.dmk[0]);
        int kbest = 0;
        for (int i = 0; i + 1 < s; ++i) {
            if (fabs(dp) < pivmin) dp = -pivmin;
            const double l = W.be[i] * qd_rcp(dp);
            if (QD_EW_LANE0) W.lp[i] = l;
            dp = (W.al[i + 1] - lam) - l * W.be[i];
            const double g = fabs(dp + W.dmk[i + 1] - (W.al[i + 1] - lam));
            if (g < gbest) { gbest = g; kbest = i + 1; }
        }
        QD_EW_SYNC();
        double yy = 1.0;
        if (QD_EW_LANE0) W.y[kbest] = 1.0;
        for (int i = kbest + 1; i < s; ++i) { yy = -W.um[i - 1] * yy; if (QD_EW_LANE0) W.y[i] = yy; }
        yy = 1.0;
        for (int i = kbest - 1; i >= 0; --i) { yy = -W.lp[i] * yy; if (QD_EW_LANE0) W.y[i] = yy; }
    }
    QD_EW_SYNC();
    // ---- 5. x = Q y = H_0 (H_1 (.. y)); lane i keeps y_i ----
    for (int k = s - 3; k >= 0; --k) {
        const double tk = W.tau[k];
        if (tk == 0.0) continue;                                          // (no reflector: f = 0)
        QD_EW_EACH(i) {
            double c = 0.0;
            if (i == k + 1) c = W.y[i];
            else if (i >= k + 2 && i < s) c = QD_EW_A(i, k) * W.y[i];
            W.red[i] = c;
        }
        const double f = tk * qd_ew_sum(W.red);
        QD_EW_EACH(i) {
            if (i == k + 1) W.y[i] -= f;
            else if (i >= k + 2 && i < s) W.y[i] = fma(-f, QD_EW_A(i, k), W.y[i]);
        }
    }
    {
        QD_EW_EACH(i) { W.red[i] = W.y[i] * W.y[i]; }
        const double nrm = qd_ew_sum(W.red);
        double sn = 0.0, inv = 1.0;
        if (nrm > 0.0 && nrm < INFINITY) qd_sqrt_rsqrt(nrm, sn, inv);
        QD_EW_EACH(i) { W.y[i] *= inv; }
    }
    QD_EW_SYNC();
    lam_out = lam * tusc;
    resid_out = 0.0;
    if constexpr (RESID) {
        const double lamu = lam * tusc;
        QD_EW_EACH(i) {
            double acc = 0.0;
            if (i < s) {
                acc = -lamu * W.y[i];
                for (int j = 0; j < s; ++j) acc = fma(Ain[j <= i ? QD_EW_IX(i, j) : QD_EW_IX(j, i)], W.y[j], acc);
            }
            W.red[i] = acc * acc;
        }
        resid_out = sqrt(qd_ew_sum(W.red));
    }
    QD_EW_EACH(i) { if (i < s) xout[i] = W.y[i]; }
    QD_EW_SYNC();
#undef QD_EW_A
#undef QD_EW_IX
}
