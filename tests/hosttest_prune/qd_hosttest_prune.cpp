// CPU driver of the pruning bound of csrc/qd_groundstate.h (qd_gs_pair_bound, qd_gs_prune_margin, qd_gs_is_task): what a half-wave
// of the structure kernel computes for one pixel, one state per "lane", in the kernel's order of operations.
#include <math.h>
#include <stdint.h>
#include "qd_groundstate.h"

// One pixel of K states.  Fabs[K]: free energies; H[K*K]: the couplings, row-major (the diagonal is not read; states i, j are
// neighbours iff H[i][j] != 0).  Out: lower[i] = F_i - radius_i in the frame of the lowest free energy, *ub, *margin, *fshift.
extern "C" void qdhp_pixel(int K, const double* Fabs, const double* H, double* lower, double* ub, double* margin, double* fshift) {
    double fs = INFINITY;
    for (int i = 0; i < K; ++i) fs = fmin(fs, Fabs[i]);
    double u = 0.0, hnorm = 0.0;
    for (int i = 0; i < K; ++i) {
        const double F = Fabs[i] - fs;
        double radius = 0.0, ubl = 0.0;
        for (int j = 0; j < K; ++j) {                      // (the kernel walks the neighbour mask from its lowest bit)
            if (j == i || H[i * K + j] == 0.0) continue;
            const double c = H[i * K + j];
            ubl = fmin(ubl, qd_gs_pair_bound(F, Fabs[j] - fs, c));
            radius += fabs(c);
        }
        lower[i] = F - radius;
        u = fmin(u, ubl);
        hnorm = fmax(hnorm, F + radius);
    }
    *ub = u; *margin = qd_gs_prune_margin(hnorm); *fshift = fs;
}

// out[k] = 1 iff a component of >= 2 states with the Gershgorin lower bound comp_lower[k] becomes a task
extern "C" void qdhp_is_task(long n, const double* comp_lower, double ub, double margin, uint8_t* out) {
    for (long k = 0; k < n; ++k) out[k] = qd_gs_is_task(comp_lower[k], ub, margin) ? 1 : 0;
}
