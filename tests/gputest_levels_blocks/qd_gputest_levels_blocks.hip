// qd_gputest_levels_blocks.hip -- DEVICE TEST HARNESS around the per-component energy-level core (csrc/qd_levels_blocks.h):
// matrices given by the test go through qd_levels_load_packed + qd_levels_blocks_solve in persistent single-wave blocks, the
// shape of qd_k_levels_grid.  It is NOT part of the product: nothing in qadapt_hip loads it.  Built by
// tests/gputest_levels_blocks/Makefile, loaded by tests/test_gpu_levels_blocks_device.py.
//
// qdgl_levels_blocks:
//   n, sizes[n]      tasks and their block sizes, 1 .. 32
//   packed, ld       task t's lower triangle, row-major, at packed + t * ld
//   nlev[n]          levels wanted of task t, 1 .. QD_LEVELS_MAX
//   blocks           persistent single-wave blocks striding over the tasks; 0: one per task, at most 256
//   poison           0: LDS as found.  1: before a block's first task every lane overwrites the whole __shared__ workspace
//                    with all-ones bits (a NaN as a double, -1 as an int, 255 as a byte), then a barrier.  2: the same before
//                    every task
//   lev[n][QD_LEVELS_MAX] (+inf from min(nlev, s) on), label[n][32] (the lowest state of the component of state i; -1 from s on)
// Return: 0, 1 for a bad argument, 2 for a HIP failure (nothing is launched or read after one).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "qd_levels_blocks.h"

__device__ void qdgl_poison(QdLevelsBlocksWs& W) {
    static_assert(sizeof(QdLevelsBlocksWs) % 8 == 0, "whole 64-bit words");
    unsigned long long* p = reinterpret_cast<unsigned long long*>(&W);
    for (unsigned i = threadIdx.x; i < (unsigned)(sizeof(QdLevelsBlocksWs) / 8); i += 64u) p[i] = ~0ull;
    __syncthreads();
}

__global__ void __launch_bounds__(64)
qdgl_k_levels_blocks(const double* __restrict__ packed, int ld, const int* __restrict__ sizes, const int* __restrict__ nlev, unsigned n,
                     int poison, double* __restrict__ lev, int* __restrict__ label) {
    __shared__ QdLevelsBlocksWs W;
    const int l = (int)threadIdx.x;
    if (poison == 1) qdgl_poison(W);
    for (unsigned t = blockIdx.x; t < n; t += gridDim.x) {
        if (poison == 2) qdgl_poison(W);
        const int s = __builtin_amdgcn_readfirstlane(sizes[t]);
        const int L = __builtin_amdgcn_readfirstlane(nlev[t]);
        qd_levels_load_packed(W.L, packed + (size_t)t * (size_t)ld, s);
        qd_levels_blocks_solve(W, s, L);
        if (l < QD_LEVELS_MAX) lev[(size_t)t * QD_LEVELS_MAX + l] = (l < L && l < s) ? W.L.lev[l] : INFINITY;
        if (l < QD_LV_MAX) label[(size_t)t * QD_LV_MAX + l] = l < s ? (int)__builtin_ctz(W.ma[l]) : -1;
        __syncthreads();                                   // (the lanes have read W before the next task overwrites it)
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

extern "C" int qdgl_ws_bytes() { return (int)sizeof(QdLevelsBlocksWs); }

extern "C" int qdgl_levels_blocks(int n, const int* sizes, const double* packed, int ld, const int* nlev, int blocks, int poison,
                                  double* lev, int* label, char* err, int errlen) {
    if (err && errlen > 0) err[0] = 0;
    if (n < 1 || !sizes || !packed || !nlev || !lev || !label) return bad_arg(err, errlen, "null argument or n < 1");
    int smax = 0;
    for (int t = 0; t < n; ++t) {
        if (sizes[t] < 1 || sizes[t] > QD_LV_MAX) return bad_arg(err, errlen, "block size outside 1..32");
        if (nlev[t] < 1 || nlev[t] > QD_LEVELS_MAX) return bad_arg(err, errlen, "levels outside 1..8");
        if (sizes[t] > smax) smax = sizes[t];
    }
    if (ld < smax * (smax + 1) / 2) return bad_arg(err, errlen, "ld too small");
    if (blocks < 0 || blocks > 65535) return bad_arg(err, errlen, "blocks outside 0..65535");
    if (poison < 0 || poison > 2) return bad_arg(err, errlen, "poison outside 0..2");
    const size_t un = (size_t)n, pb = un * (size_t)ld * sizeof(double), lb = un * QD_LEVELS_MAX * sizeof(double),
                 ib = un * QD_LV_MAX * sizeof(int);
    DevList d;
    double *dpk, *dlev;
    int *dsz, *dnl, *dlab;
    QDG_ALLOC(dpk, pb);
    QDG_ALLOC(dsz, un * sizeof(int));
    QDG_ALLOC(dnl, un * sizeof(int));
    QDG_ALLOC(dlev, lb);
    QDG_ALLOC(dlab, ib);
    QDG_HIP(hipMemcpy(dpk, packed, pb, hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dsz, sizes, un * sizeof(int), hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dnl, nlev, un * sizeof(int), hipMemcpyHostToDevice));
    QDG_HIP(hipMemset(dlev, 0xFF, lb));
    QDG_HIP(hipMemset(dlab, 0xFF, ib));
    const dim3 grid(blocks > 0 ? (unsigned)blocks : (n < 256 ? (unsigned)n : 256u)), block(64);
    qdgl_k_levels_blocks<<<grid, block>>>(dpk, ld, dsz, dnl, (unsigned)n, poison, dlev, dlab);
    QDG_HIP(hipGetLastError());
    QDG_HIP(hipDeviceSynchronize());
    QDG_HIP(hipMemcpy(lev, dlev, lb, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(label, dlab, ib, hipMemcpyDeviceToHost));
    return 0;
}
