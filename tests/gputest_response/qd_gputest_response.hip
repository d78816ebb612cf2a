// qd_gputest_response.hip -- DEVICE TEST HARNESS around the charge-response epilogue (csrc/qd_response.h): matrices and
// perturbations given by the test go through qd_levels_load_packed, qd_response_scale, qd_thermal_solve, qd_response_begin and
// one qd_response_apply per perturbation in persistent single-wave blocks, the shape of qd_k_thermal_response.  It is NOT part of
// the product: nothing in qadapt_hip loads it.  Built by tests/gputest_response/Makefile, loaded by
// tests/test_gpu_response_device.py.
//
// qdgr_response:
//   n, sizes[n]          tasks and their block sizes, 1 .. 32
//   packed, ld           task t's lower triangle, row-major, at packed + t * ld
//   kT[n]                finite and > 0
//   npert, kind[npert]   perturbations per task; 0: diagonal, 1: sparse with at most two partners per state
//   x[n][npert][64]      diagonal: x_m in [m];  sparse: the coefficients of nb[m][0] in [m], of nb[m][1] in [32 + m]
//   nb[n][npert][32][2]  sparse: the partners, each below the task's size, or 255 for none
//   blocks               persistent single-wave blocks striding over the tasks; 0: one per task, at most 256
//   poison               0: LDS as found.  1: before a block's first task every lane overwrites the whole __shared__ workspace
//                        with all-ones bits (a NaN as a double, 255 as a byte), then a barrier.  2: the same before every task
//   dP[n][npert][32], pop[n][32]   zero from s on
// Return: 0, 1 for a bad argument, 2 for a HIP failure (nothing is launched or read after one).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "qd_response.h"

__device__ void qdgr_poison(QdResponseWs& W) {
    static_assert(sizeof(QdResponseWs) % 8 == 0, "whole 64-bit words");
    unsigned long long* p = reinterpret_cast<unsigned long long*>(&W);
    for (unsigned i = threadIdx.x; i < (unsigned)(sizeof(QdResponseWs) / 8); i += 64u) p[i] = ~0ull;
    __syncthreads();
}

__global__ void __launch_bounds__(64)
qdgr_k_response(const double* __restrict__ packed, int ld, const int* __restrict__ sizes, const double* __restrict__ kT, unsigned n,
                int npert, const int* __restrict__ kind, const double* __restrict__ x, const uint8_t* __restrict__ nb, int poison,
                double* __restrict__ dP, double* __restrict__ pop) {
    __shared__ QdResponseWs W;
    const int l = (int)threadIdx.x;
    if (poison == 1) qdgr_poison(W);
    for (unsigned t = blockIdx.x; t < n; t += gridDim.x) {
        if (poison == 2) qdgr_poison(W);
        const int s = __builtin_amdgcn_readfirstlane(sizes[t]);
        const double kt = kT[t];
        qd_levels_load_packed(W.T.B, packed + (size_t)t * (size_t)ld, s);
        qd_response_scale(W, s);
        qd_thermal_solve(W.T, s, kt);
        if (l < QD_LV_MAX) pop[(size_t)t * QD_LV_MAX + l] = l < s ? W.T.pop[l] : 0.0;
        __syncthreads();
        qd_response_begin(W, s, kt);
        for (int p = 0; p < npert; ++p) {
            const size_t tp = (size_t)t * (size_t)npert + (size_t)p;
            const int hop = __builtin_amdgcn_readfirstlane(kind[p]);
            if (l < s) {
                W.T.B.x[l] = x[tp * 64 + l];
                if (hop) {
                    W.T.B.x[32 + l] = x[tp * 64 + 32 + l];
                    W.nb[l][0] = nb[tp * 64 + 2 * l]; W.nb[l][1] = nb[tp * 64 + 2 * l + 1];
                }
            }
            __syncthreads();
            if (hop) qd_response_apply<true>(W, s, kt); else qd_response_apply<false>(W, s, kt);
            if (l < QD_LV_MAX) dP[tp * QD_LV_MAX + l] = l < s ? W.dP[l] : 0.0;
            __syncthreads();                               // (the lanes have read W.dP before the next perturbation overwrites it)
        }
    }
}

namespace {

int bad_arg(char* err, int errlen, const char* msg) {
    if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", msg);
    return 1;
}

#define QDG_HIP(call)                                                                                      \
    do {                                                                                                   \
        const hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                            \
            if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s: %s", #call, hipGetErrorString(e_));  \
            return 2;                                                                                      \
        }                                                                                                  \
    } while (0)

// device buffers of one call, freed on every way out
struct DevList {
    std::vector<void*> p;
    ~DevList() { for (void* q : p) (void)hipFree(q); }
};

#define QDG_ALLOC(ptr, bytes)                                  \
    do {                                                       \
        void* q_ = nullptr;                                    \
        QDG_HIP(hipMalloc(&q_, (bytes)));                      \
        d.p.push_back(q_);                                     \
        (ptr) = reinterpret_cast<decltype(ptr)>(q_);           \
    } while (0)

}  // namespace

extern "C" int qdgr_ws_bytes() { return (int)sizeof(QdResponseWs); }

extern "C" int qdgr_response(int n, const int* sizes, const double* packed, int ld, const double* kT, int npert, const int* kind,
                             const double* x, const uint8_t* nb, int blocks, int poison, double* dP, double* pop, char* err,
                             int errlen) {
    if (err && errlen > 0) err[0] = 0;
    if (n < 1 || !sizes || !packed || !kT || !kind || !x || !nb || !dP || !pop) return bad_arg(err, errlen, "null argument or n < 1");
    if (npert < 1 || npert > 64) return bad_arg(err, errlen, "npert outside 1..64");
    int smax = 0;
    for (int t = 0; t < n; ++t) {
        if (sizes[t] < 1 || sizes[t] > QD_LV_MAX) return bad_arg(err, errlen, "block size outside 1..32");
        if (sizes[t] > smax) smax = sizes[t];
        if (!(kT[t] > 0.0) || !isfinite(kT[t])) return bad_arg(err, errlen, "kT must be finite and > 0");
    }
    if (ld < smax * (smax + 1) / 2) return bad_arg(err, errlen, "ld too small");
    if (blocks < 0 || blocks > 65535) return bad_arg(err, errlen, "blocks outside 0..65535");
    if (poison < 0 || poison > 2) return bad_arg(err, errlen, "poison outside 0..2");
    for (int p = 0; p < npert; ++p) {
        if (kind[p] != 0 && kind[p] != 1) return bad_arg(err, errlen, "kind outside 0..1");
        if (kind[p] == 1)
            for (int t = 0; t < n; ++t)
                for (int m = 0; m < 2 * sizes[t]; ++m) {
                    const uint8_t j = nb[((size_t)t * npert + p) * 64 + m];
                    if (j != QD_RS_NONE && j >= sizes[t]) return bad_arg(err, errlen, "a partner outside the block");
                }
    }
    const size_t un = (size_t)n, np_ = un * (size_t)npert;
    const size_t pb = un * (size_t)ld * sizeof(double), sb = un * sizeof(double), xb = np_ * 64 * sizeof(double), nbb = np_ * 64,
                 db = np_ * QD_LV_MAX * sizeof(double), vb = un * QD_LV_MAX * sizeof(double);
    DevList d;
    double *dpk, *dkt, *dx, *ddp, *dpop;
    int *dsz, *dkind;
    uint8_t* dnb;
    QDG_ALLOC(dpk, pb);
    QDG_ALLOC(dsz, un * sizeof(int));
    QDG_ALLOC(dkt, sb);
    QDG_ALLOC(dkind, (size_t)npert * sizeof(int));
    QDG_ALLOC(dx, xb);
    QDG_ALLOC(dnb, nbb);
    QDG_ALLOC(ddp, db);
    QDG_ALLOC(dpop, vb);
    QDG_HIP(hipMemcpy(dpk, packed, pb, hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dsz, sizes, un * sizeof(int), hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dkt, kT, sb, hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dkind, kind, (size_t)npert * sizeof(int), hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dx, x, xb, hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dnb, nb, nbb, hipMemcpyHostToDevice));
    QDG_HIP(hipMemset(ddp, 0xFF, db));
    QDG_HIP(hipMemset(dpop, 0xFF, vb));
    const dim3 grid(blocks > 0 ? (unsigned)blocks : (n < 256 ? (unsigned)n : 256u)), block(64);
    qdgr_k_response<<<grid, block>>>(dpk, ld, dsz, dkt, (unsigned)n, npert, dkind, dx, dnb, poison, ddp, dpop);
    QDG_HIP(hipGetLastError());
    QDG_HIP(hipDeviceSynchronize());
    QDG_HIP(hipMemcpy(dP, ddp, db, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(pop, dpop, vb, hipMemcpyDeviceToHost));
    return 0;
}
