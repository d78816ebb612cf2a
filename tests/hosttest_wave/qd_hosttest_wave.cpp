// CPU driver of csrc/qd_eig_wave.h: the solver a wavefront runs on a 33..64-state block, with the lanes as a loop.
#include <stdlib.h>
#include "qd_eig_wave.h"

// packed: lower triangle, row-major, s (s + 1) / 2 doubles.  0 on success, 1 for a size outside 2..64.
extern "C" int qdhw_eig_lowest(int s, const double* packed, double* lam, double* x, double* resid, int* iters) {
    if (s < 2 || s > QD_EW_MAX) return 1;
    QdEigWaveWs* W = (QdEigWaveWs*)malloc(sizeof(QdEigWaveWs));
    if (!W) return 2;
    qd_eig_wave_lowest<true>(*W, packed, s, *lam, *resid, x, iters);
    free(W);
    return 0;
}
