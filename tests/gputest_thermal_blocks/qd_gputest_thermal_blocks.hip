// qd_gputest_thermal_blocks.hip -- DEVICE TEST HARNESS around the per-component thermal core (csrc/qd_thermal_blocks.h):
// matrices given by the test go through qd_levels_load_packed + qd_thermal_blocks_solve in persistent single-wave blocks, the
// shape of qd_k_thermal_grid.  It is NOT part of the product: nothing in qadapt_hip loads it.  Built by
// tests/gputest_thermal_blocks/Makefile, loaded by tests/test_gpu_thermal_blocks_device.py.
//
// qdgb_thermal:
//   n, sizes[n]      tasks and their block sizes, 1 .. 32
//   packed, ld       task t's lower triangle, row-major, at packed + t * ld
//   kT[n]            finite and > 0
//   blocks           persistent single-wave blocks striding over the tasks; 0: one per task, at most 256
//   poison           0: LDS as found.  1: before a block's first task every lane overwrites the whole __shared__ workspace
//                    with all-ones bits (a NaN as a double, -1 as an int, 255 as a byte), then a barrier.  2: the same before
//                    every task
//   pop[n][32], lam[n][32] (zero from s on), ztail[n], sweeps[n], label[n][32] (the lowest state of the component of state
//   i; -1 from s on), V[n][32][32] (row-major, zero outside the block; a null pointer skips it), and from the workspace after
//   the solve, in the scaled units of the block:  asym[n] = max |A_ij - A_ji|,  cross[n] = the largest |A_ij| or |V_ij|
//   between two states of different components (NaN if any entry read is; both 0 for s == 1)
// Return: 0, 1 for a bad argument, 2 for a HIP failure (nothing is launched or read after one).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "qd_thermal_blocks.h"

__device__ void qdgb_poison(QdThermalBlocksWs& W) {
    static_assert(sizeof(QdThermalBlocksWs) % 8 == 0, "whole 64-bit words");
    unsigned long long* p = reinterpret_cast<unsigned long long*>(&W);
    for (unsigned i = threadIdx.x; i < (unsigned)(sizeof(QdThermalBlocksWs) / 8); i += 64u) p[i] = ~0ull;
    __syncthreads();
}

__global__ void __launch_bounds__(64)
qdgb_k_thermal(const double* __restrict__ packed, int ld, const int* __restrict__ sizes, const double* __restrict__ kT, unsigned n,
               int poison, double* __restrict__ pop, double* __restrict__ lam, double* __restrict__ ztail, int* __restrict__ sweeps,
               int* __restrict__ label, double* __restrict__ V, double* __restrict__ asym, double* __restrict__ cross) {
    __shared__ QdThermalBlocksWs W;
    const int l = (int)threadIdx.x;
    if (poison == 1) qdgb_poison(W);
    for (unsigned t = blockIdx.x; t < n; t += gridDim.x) {
        if (poison == 2) qdgb_poison(W);
        const int s = __builtin_amdgcn_readfirstlane(sizes[t]);
        qd_levels_load_packed(W.T.B, packed + (size_t)t * (size_t)ld, s);
        const int sw = qd_thermal_blocks_solve(W, s, kT[t]);
        // what is left of A and V: lane i takes row i; a NaN anywhere makes the figure NaN (fmax would drop it)
        double da = 0.0, dc = 0.0;
        bool bad = false;
        if (s > 1 && l < s) {
            const unsigned mine = W.ma[l];
            for (int j = 0; j < s; ++j) {
                const double a = W.T.B.A[l * QD_LV_LD + j], b = W.T.B.A[j * QD_LV_LD + l], v = W.T.V[l * QD_LV_LD + j];
                bad |= (a != a) | (b != b) | (v != v);
                da = fmax(da, fabs(a - b));
                if (!((mine >> j) & 1u)) dc = fmax(dc, fmax(fabs(a), fabs(v)));
            }
        }
        W.T.B.v[l] = bad ? NAN : da;
        W.T.B.w[l] = bad ? NAN : dc;
        __syncthreads();
        if (l < QD_LV_MAX) {
            pop[(size_t)t * QD_LV_MAX + l] = l < s ? W.T.pop[l] : 0.0;
            lam[(size_t)t * QD_LV_MAX + l] = l < s ? W.T.lam[l] : 0.0;
            label[(size_t)t * QD_LV_MAX + l] = l < s ? (int)__builtin_ctz(W.ma[l]) : -1;
        }
        if (V)
            for (int e = l; e < QD_LV_MAX * QD_LV_MAX; e += 64) {
                const int i = e / QD_LV_MAX, j = e % QD_LV_MAX;
                V[(size_t)t * (QD_LV_MAX * QD_LV_MAX) + e] = (i < s && j < s) ? W.T.V[i * QD_LV_LD + j] : 0.0;
            }
        if (l == 0) {
            double ma = 0.0, mc = 0.0;
            bool nan = false;
            for (int i = 0; i < s; ++i) {
                const double a = W.T.B.v[i], c = W.T.B.w[i];
                nan |= (a != a) | (c != c);
                ma = fmax(ma, a); mc = fmax(mc, c);
            }
            asym[t] = nan ? NAN : ma;
            cross[t] = nan ? NAN : mc;
            ztail[t] = W.T.ztail;
            sweeps[t] = sw;
        }
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

extern "C" int qdgb_ws_bytes() { return (int)sizeof(QdThermalBlocksWs); }

extern "C" int qdgb_thermal(int n, const int* sizes, const double* packed, int ld, const double* kT, int blocks, int poison,
                            double* pop, double* lam, double* ztail, int* sweeps, int* label, double* V, double* asym, double* cross,
                            char* err, int errlen) {
    if (err && errlen > 0) err[0] = 0;
    if (n < 1 || !sizes || !packed) return bad_arg(err, errlen, "null argument or n < 1");
    int smax = 0;
    for (int t = 0; t < n; ++t) {
        if (sizes[t] < 1 || sizes[t] > QD_LV_MAX) return bad_arg(err, errlen, "block size outside 1..32");
        if (sizes[t] > smax) smax = sizes[t];
    }
    if (ld < smax * (smax + 1) / 2) return bad_arg(err, errlen, "ld too small");
    if (blocks < 0 || blocks > 65535) return bad_arg(err, errlen, "blocks outside 0..65535");
    if (poison < 0 || poison > 2) return bad_arg(err, errlen, "poison outside 0..2");
    if (!kT || !pop || !lam || !ztail || !sweeps || !label || !asym || !cross) return bad_arg(err, errlen, "null argument");
    for (int t = 0; t < n; ++t)
        if (!(kT[t] > 0.0) || !isfinite(kT[t])) return bad_arg(err, errlen, "kT must be finite and > 0");
    const size_t un = (size_t)n, pb = un * (size_t)ld * sizeof(double), vb = un * QD_LV_MAX * sizeof(double),
                 ib = un * QD_LV_MAX * sizeof(int), sb = un * sizeof(double), Vb = un * QD_LV_MAX * QD_LV_MAX * sizeof(double);
    DevList d;
    double *dpk, *dkt, *dpop, *dlam, *dzt, *dV = nullptr, *dasym, *dcross;
    int *dsz, *dsw, *dlab;
    QDG_ALLOC(dpk, pb);
    QDG_ALLOC(dsz, un * sizeof(int));
    QDG_ALLOC(dkt, sb);
    QDG_ALLOC(dpop, vb);
    QDG_ALLOC(dlam, vb);
    QDG_ALLOC(dzt, sb);
    QDG_ALLOC(dsw, un * sizeof(int));
    QDG_ALLOC(dlab, ib);
    QDG_ALLOC(dasym, sb);
    QDG_ALLOC(dcross, sb);
    if (V) QDG_ALLOC(dV, Vb);
    QDG_HIP(hipMemcpy(dpk, packed, pb, hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dsz, sizes, un * sizeof(int), hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dkt, kT, sb, hipMemcpyHostToDevice));
    QDG_HIP(hipMemset(dpop, 0xFF, vb));
    QDG_HIP(hipMemset(dlam, 0xFF, vb));
    QDG_HIP(hipMemset(dzt, 0xFF, sb));
    QDG_HIP(hipMemset(dsw, 0xFF, un * sizeof(int)));
    QDG_HIP(hipMemset(dlab, 0xFF, ib));
    QDG_HIP(hipMemset(dasym, 0xFF, sb));
    QDG_HIP(hipMemset(dcross, 0xFF, sb));
    if (V) QDG_HIP(hipMemset(dV, 0xFF, Vb));
    const dim3 grid(blocks > 0 ? (unsigned)blocks : (n < 256 ? (unsigned)n : 256u)), block(64);
    qdgb_k_thermal<<<grid, block>>>(dpk, ld, dsz, dkt, (unsigned)n, poison, dpop, dlam, dzt, dsw, dlab, dV, dasym, dcross);
    QDG_HIP(hipGetLastError());
    QDG_HIP(hipDeviceSynchronize());
    QDG_HIP(hipMemcpy(pop, dpop, vb, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(lam, dlam, vb, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(ztail, dzt, sb, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(sweeps, dsw, un * sizeof(int), hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(label, dlab, ib, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(asym, dasym, sb, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(cross, dcross, sb, hipMemcpyDeviceToHost));
    if (V) QDG_HIP(hipMemcpy(V, dV, Vb, hipMemcpyDeviceToHost));
    return 0;
}
