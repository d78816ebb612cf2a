// qd_gputest_response_blocks.hip -- DEVICE TEST HARNESS around the per-component charge-response epilogue
// (csrc/qd_response_blocks.h): matrices and perturbations given by the test go through qd_levels_load_packed,
// qd_response_blocks_scale, qd_thermal_blocks_solve, qd_response_blocks_begin and one qd_response_blocks_apply per perturbation in
// persistent single-wave blocks, the shape of qd_k_thermal_grid_response.  The sparse perturbations respect the components of
// their block.  It is NOT part of the product: nothing in qadapt_hip loads it.  Built by tests/gputest_response_blocks/Makefile,
// loaded by tests/test_gpu_response_blocks_device.py.
//
// qdgrb_response:
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
#include "qd_response_blocks.h"

__device__ void qdgrb_poison(QdResponseBlocksWs& W) {
    static_assert(sizeof(QdResponseBlocksWs) % 8 == 0, "whole 64-bit words");
    unsigned long long* p = reinterpret_cast<unsigned long long*>(&W);
    for (unsigned i = threadIdx.x; i < (unsigned)(sizeof(QdResponseBlocksWs) / 8); i += 64u) p[i] = ~0ull;
    __syncthreads();
}

__global__ void __launch_bounds__(64)
qdgrb_k_response(const double* __restrict__ packed, int ld, const int* __restrict__ sizes, const double* __restrict__ kT, unsigned n,
                int npert, const int* __restrict__ kind, const double* __restrict__ x, const uint8_t* __restrict__ nb, int poison,
                double* __restrict__ dP, double* __restrict__ pop) {
    __shared__ QdResponseBlocksWs W;
    QdThermalWs& T = W.TB.T;
    const int l = (int)threadIdx.x;
    if (poison == 1) qdgrb_poison(W);
    for (unsigned t = blockIdx.x; t < n; t += gridDim.x) {
        if (poison == 2) qdgrb_poison(W);
        const int s = __builtin_amdgcn_readfirstlane(sizes[t]);
        const double kt = kT[t];
        qd_levels_load_packed(T.B, packed + (size_t)t * (size_t)ld, s);
        qd_response_blocks_scale(W, s);
        qd_thermal_blocks_solve(W.TB, s, kt);
        if (l < QD_LV_MAX) pop[(size_t)t * QD_LV_MAX + l] = l < s ? T.pop[l] : 0.0;
        __syncthreads();
        qd_response_blocks_begin(W, s, kt);
        for (int p = 0; p < npert; ++p) {
            const size_t tp = (size_t)t * (size_t)npert + (size_t)p;
            const int hop = __builtin_amdgcn_readfirstlane(kind[p]);
            if (l < s) {
                T.B.x[l] = x[tp * 64 + l];
                if (hop) {
                    T.B.x[32 + l] = x[tp * 64 + 32 + l];
                    W.nb[l][0] = nb[tp * 64 + 2 * l]; W.nb[l][1] = nb[tp * 64 + 2 * l + 1];
                }
            }
            __syncthreads();
            if (hop) qd_response_blocks_apply<true>(W, s, kt); else qd_response_blocks_apply<false>(W, s, kt);
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

extern "C" int qdgrb_ws_bytes() { return (int)sizeof(QdResponseBlocksWs); }

extern "C" int qdgrb_response(int n, const int* sizes, const double* packed, int ld, const double* kT, int npert, const int* kind,
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
    qdgrb_k_response<<<grid, block>>>(dpk, ld, dsz, dkt, (unsigned)n, npert, dkind, dx, dnb, poison, ddp, dpop);
    QDG_HIP(hipGetLastError());
    QDG_HIP(hipDeviceSynchronize());
    QDG_HIP(hipMemcpy(dP, ddp, db, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(pop, dpop, vb, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// qdgrb_record: the body of one point of qd_k_thermal_grid_response<N, QdResponseBlocksWs> on a hand-made record -- the record
// from its fields as tests/hosttest_response_blocks builds it, par the parameter block; nvalid = 0 is the record without a valid
// state, which the searches never produce: the thermal calls are skipped, the epilogue starts from whatever LDS holds (poison as
// above), c0 is formed at <n> = 0.  Outputs: chi[N][2N-1], jac[N][2N], dsignal[2N] = S'(c0) dc0/dv, c0.  Return as qdgrb_response.
// ---------------------------------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(64)
qdgrb_k_record(const QdPixelRec* __restrict__ rec, int kept, double kT, const double* __restrict__ par, int poison,
               double* __restrict__ chi, double* __restrict__ jac, double* __restrict__ dsignal, double* __restrict__ c0_dst) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N, X = 2 * N - 1;
    __shared__ QdResponseBlocksWs W;
    QdThermalWs& T = W.TB.T;
    const QdLayout L = qd_layout(N);
    const int l = (int)threadIdx.x;
    if (poison) qdgrb_poison(W);
    int nv = rec->nvalid < kept ? rec->nvalid : kept;
    nv = nv < 0 ? 0 : (nv > QD_LV_MAX ? QD_LV_MAX : nv);
    nv = __builtin_amdgcn_readfirstlane(nv);
    if (nv > 0) {
        qd_levels_record<N>(T.B, rec, nv);
        qd_response_blocks_scale(W, nv);
        qd_thermal_blocks_solve(W.TB, nv, kT);
        qd_thermal_moments<N>(T, rec, nv);
    }
    double b = 0.0;
    for (int i = 0; i < N; ++i) {
        const double o = nv > 0 ? T.occ[i] : 0.0;
        b = fma(par[L.cdd_inv + N * G + i], o - rec->vpp[i], b);
    }
    const double vs = rec->vpp[N];
    const double Ns = rint(vs);
    const double c0 = 2.0 * b + par[L.cdd_inv + N * G + N] * (2.0 * (Ns - vs) + 1.0);
    __syncthreads();
    qd_response_blocks_solve<N>(W, rec, nv, kT, par);
    const double ds = qd_sensor_slope(c0, par[L.cdd_inv + N * G + N], par[L.scal + 1]);
    for (int e = l; e < N * X; e += 64) {
        const int i = e / X, c = e - i * X;
        chi[e] = c < N ? T.B.lo[i * N + c] : T.B.hi[i * NB + c - N];
    }
    for (int e = l; e < N * V; e += 64) {
        const int i = e / V, c = e - i * V;
        jac[e] = c < N ? T.B.v[i * N + c] : T.B.w[i * N + c - N];
    }
    if (l < V) dsignal[l] = T.c[l] * ds;
    if (l == 0) c0_dst[0] = c0;
}

extern "C" int qdgrb_record(int N, const uint16_t* idx, const int32_t* fl, const double* tc, const double* E, const double* vpp,
                            int nvalid, int kept, double kT, const double* par, int poison, double* chi, double* jac,
                            double* dsignal, double* c0, char* err, int errlen) {
    if (err && errlen > 0) err[0] = 0;
    if (N < 2 || N > QD_MAXN || !idx || !fl || !tc || !E || !vpp || !par || !chi || !jac || !dsignal || !c0)
        return bad_arg(err, errlen, "null argument or N outside 2..8");
    if (kept < 1 || kept > QD_K || nvalid < 0 || nvalid > QD_K) return bad_arg(err, errlen, "kept outside 1..K or nvalid outside 0..K");
    if (!(kT > 0.0) || !isfinite(kT)) return bad_arg(err, errlen, "kT must be finite and > 0");
    if (poison < 0 || poison > 1) return bad_arg(err, errlen, "poison outside 0..1");
    QdPixelRec rec;
    memset(&rec, 0, sizeof(rec));
    for (int m = 0; m < QD_K; ++m) { rec.idx[m] = idx[m]; rec.E[m] = E[m]; }
    for (int i = 0; i < N; ++i) rec.fl[i] = fl[i];
    for (int b = 0; b < N - 1; ++b) rec.tc[b] = tc[b];
    for (int i = 0; i <= N; ++i) rec.vpp[i] = vpp[i];
    rec.nvalid = nvalid;
    const QdLayout L = qd_layout(N);
    const size_t nx = (size_t)N * (2 * N - 1), nj = (size_t)N * 2 * N, nd = (size_t)2 * N;
    DevList d;
    QdPixelRec* drec;
    double *dpar, *dchi, *djac, *dds, *dc0;
    QDG_ALLOC(drec, sizeof(rec));
    QDG_ALLOC(dpar, sizeof(double) * (size_t)L.size);
    QDG_ALLOC(dchi, sizeof(double) * nx);
    QDG_ALLOC(djac, sizeof(double) * nj);
    QDG_ALLOC(dds, sizeof(double) * nd);
    QDG_ALLOC(dc0, sizeof(double));
    QDG_HIP(hipMemcpy(drec, &rec, sizeof(rec), hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dpar, par, sizeof(double) * (size_t)L.size, hipMemcpyHostToDevice));
    QDG_HIP(hipMemset(dchi, 0xFF, sizeof(double) * nx));
    QDG_HIP(hipMemset(djac, 0xFF, sizeof(double) * nj));
    QDG_HIP(hipMemset(dds, 0xFF, sizeof(double) * nd));
    switch (N) {
#define C(k) case k: qdgrb_k_record<k><<<dim3(1), dim3(64)>>>(drec, kept, kT, dpar, poison, dchi, djac, dds, dc0); break;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
    }
    QDG_HIP(hipGetLastError());
    QDG_HIP(hipDeviceSynchronize());
    QDG_HIP(hipMemcpy(chi, dchi, sizeof(double) * nx, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(jac, djac, sizeof(double) * nj, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(dsignal, dds, sizeof(double) * nd, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(c0, dc0, sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
