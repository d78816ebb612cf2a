// qd_gputest_eig.hip -- DEVICE TEST HARNESS around the three dense eigen-solvers of the ground-state stage
// (csrc/qd_eig.h, csrc/qd_eig_wave.h): matrices given by the test go through the product's own task wrappers
// (qd_eig_task, qd_eig_task_mem, qd_eig_wave_lowest with the record as its output) in records laid out as the structure
// kernels lay them out, one launch shape per class as the product launches them.  It is NOT part of the product:
// nothing in qadapt_hip loads it.  Built by tests/gputest_eig/Makefile, loaded by tests/test_gpu_eig_device.py.
//
// One C entry point per class (register, memory, wide), and qdg_prims for the primitives.  Common arguments:
//   n, sizes[n]      tasks and their block sizes
//   packed, ld       task t's lower triangle, row-major, at packed + t * ld
//   solo             (per-lane classes) 1: every task in a launch of its own, one active lane
//   validate         1: the VALIDATE = true instantiation (residual and Laguerre iterations), 0: the product-mode one
//   lam[n]           eigenvalue, from the dense array the solve kernels write
//   x, ldx           task t's vector at x + t * ldx, read back from the record (where the select kernel reads it)
//   resid[n]         rec[1] after the solve (validate only, else 0)
//   iters[n]         Laguerre iterations (validate only, else 0)
//   err, errlen      text of a failure
// Return: 0, 1 for a bad argument, 2 for a HIP failure (nothing is launched or read after one).
//
// Below them, the two one-point-per-wavefront cores of the point queries, csrc/qd_levels.h (qd_levels_solve) and
// csrc/qd_thermal.h (qd_thermal_solve), behind qd_levels_load_packed in persistent single-wave blocks, the shape of
// qd_k_levels / qd_k_thermal: qdg_levels and qdg_thermal, loaded by tests/test_gpu_spectrum_device.py.  Their arguments
// are described where they are defined.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "qd_fullspace.h"          // qd_kernels.h (size class -> solver, launch bounds), qd_eig_wave.h, the wide record
#include "qd_thermal.h"            // qd_levels.h: the two cores and their workspaces

// ---- per-lane classes: one task per lane in 256-thread blocks, as qd_k_gs_solve<BIN> runs a tile ----
template <int BIN, bool VALIDATE>
__global__ void __launch_bounds__(256, QdGsSolveWaves<BIN>::v)
qdg_k_lane(double* __restrict__ pool, const unsigned* __restrict__ off, unsigned n, double* __restrict__ lam_out,
           int* __restrict__ its_out) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t < n) {
        double lam;
        const int its = qd_gs_solve_task<BIN, VALIDATE>(pool + off[t], lam);
        lam_out[t] = lam;
        its_out[t] = its;
    }
}

// ---- wide class: persistent single-wave blocks striding over the tasks, the shape of qd_k_full_solve_wide.  ALIASED:
// the vector overwrites the record (what the product does); otherwise it goes to xsep + t * QD_EW_MAX ----
template <bool VALIDATE, bool ALIASED>
__global__ void __launch_bounds__(64)
qdg_k_wide(double* __restrict__ pool, const unsigned* __restrict__ off, unsigned n, double* xsep, double* __restrict__ lam_out,
           int* __restrict__ its_out) {
    __shared__ QdEigWaveWs W;
    for (unsigned t = blockIdx.x; t < n; t += gridDim.x) {
        double* rec = pool + off[t];
        const int s = (int)rec[1];
        double lam, resid;
        int its = 0;
        qd_eig_wave_lowest<VALIDATE>(W, rec + 2, s, lam, resid, ALIASED ? rec + 2 : xsep + (size_t)t * QD_EW_MAX,
                                     VALIDATE ? &its : nullptr);
        if (threadIdx.x == 0) {
            lam_out[t] = lam;
            its_out[t] = its;
            if (VALIDATE) rec[1] = resid;
        }
    }
}

// ---- the device forms of the solvers' primitives (rcp / rsq builtins + Newton steps), one argument per lane ----
__global__ void __launch_bounds__(256)
qdg_k_prims(const double* __restrict__ x, unsigned n, double* __restrict__ out) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t < n) {
        double s, r;
        qd_sqrt_rsqrt(x[t], s, r);
        out[t] = qd_rcp(x[t]);
        out[(size_t)n + t] = qd_rcp1(x[t]);
        out[2 * (size_t)n + t] = qd_sqrt1(x[t]);
        out[3 * (size_t)n + t] = s;
        out[4 * (size_t)n + t] = r;
    }
}

namespace {

struct DevBufs {
    double* pool = nullptr; unsigned* off = nullptr; double* lam = nullptr; int* its = nullptr; double* xsep = nullptr;
    ~DevBufs() { (void)hipFree(pool); (void)hipFree(off); (void)hipFree(lam); (void)hipFree(its); (void)hipFree(xsep); }
};

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

enum Class { REG, MEM, WIDE };

// solo: every task in a launch of its own, one active lane
template <int BIN>
void launch_lane(bool validate, bool solo, unsigned n, const DevBufs& d) {
    const unsigned launches = solo ? n : 1u, per = solo ? 1u : n;
    const dim3 grid((per + 255u) / 256u), block(256);
    for (unsigned t = 0; t < launches; ++t) {
        if (validate) qdg_k_lane<BIN, true><<<grid, block>>>(d.pool, d.off + t, per, d.lam + t, d.its + t);
        else          qdg_k_lane<BIN, false><<<grid, block>>>(d.pool, d.off + t, per, d.lam + t, d.its + t);
    }
}

// cls REG: S is the class's solver size (2..8, 10, 12), sizes[t] == S, or S - 1 for the padded classes
// cls REG, MEM: solo = one launch per task instead of one task per lane
// cls WIDE: blocks = persistent blocks launched (0: one per task, at most 256), aliased = the product's call
int run(Class cls, int S, int n, const int* sizes, const double* packed, int ld, int validate, int solo, int blocks, int aliased,
        double* lam, double* x, int ldx, double* resid, int* iters, char* err, int errlen) {
    if (err && errlen > 0) err[0] = 0;
    if (n < 1 || !sizes || !packed || !lam || !x || !resid || !iters) return bad_arg(err, errlen, "null argument or n < 1");
    const bool val = validate != 0;
    int smax = 0;
    std::vector<unsigned> off((size_t)n);
    size_t top = 0;
    for (int t = 0; t < n; ++t) {
        const int s = sizes[t];
        bool ok;
        if (cls == REG) ok = (S <= 8) ? (s == S) : (s == S || s == S - 1);
        else if (cls == MEM) ok = s > QD_EIG_REG && s <= QD_K;
        else ok = s >= 2 && s <= QD_EW_MAX;
        if (!ok) return bad_arg(err, errlen, "block size outside the class");
        if (s > smax) smax = s;
        off[(size_t)t] = (unsigned)top;
        // the wide class solves any size from the record of a wide task (no workspace: the block lives in LDS)
        top += (size_t)(cls == WIDE ? ((2 + s * (s + 1) / 2 + 1) & ~1) : qd_gs_task_doubles(s, val));
    }
    if (cls == REG && !(S >= 2 && S <= QD_EIG_REG && (S <= 8 || S == 10 || S == 12))) return bad_arg(err, errlen, "no such register class");
    if (ld < smax * (smax + 1) / 2 || ldx < smax) return bad_arg(err, errlen, "ld / ldx too small");
    if (top >= 0xFFFFFFFFull) return bad_arg(err, errlen, "pool too large");
    if (cls == WIDE && qd_full_task_doubles(QD_EW_MAX, val) != ((2 + QD_EW_MAX * (QD_EW_MAX + 1) / 2 + 1) & ~1))
        return bad_arg(err, errlen, "wide record layout changed");
    // records back to back as the bump allocator of the structure kernels leaves them; whatever the product does not
    // write (rec[0], the size of per-lane blocks of <= 8 states, the workspace of the memory solver) is NaN
    std::vector<double> pool(top);
    memset(pool.data(), 0xFF, top * sizeof(double));
    for (int t = 0; t < n; ++t) {
        const int s = sizes[t];
        double* rec = pool.data() + off[(size_t)t];
        if (s > 8 || cls == WIDE) rec[1] = (double)s;          // (a wide task always carries its size)
        memcpy(rec + 2, packed + (size_t)t * (size_t)ld, sizeof(double) * (size_t)(s * (s + 1) / 2));
    }
    DevBufs d;
    const bool sep = cls == WIDE && !aliased;
    QDG_HIP(hipMalloc(&d.pool, top * sizeof(double)));
    QDG_HIP(hipMalloc(&d.off, (size_t)n * sizeof(unsigned)));
    QDG_HIP(hipMalloc(&d.lam, (size_t)n * sizeof(double)));
    QDG_HIP(hipMalloc(&d.its, (size_t)n * sizeof(int)));
    if (sep) QDG_HIP(hipMalloc(&d.xsep, (size_t)n * QD_EW_MAX * sizeof(double)));
    QDG_HIP(hipMemcpy(d.pool, pool.data(), top * sizeof(double), hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(d.off, off.data(), (size_t)n * sizeof(unsigned), hipMemcpyHostToDevice));
    QDG_HIP(hipMemset(d.lam, 0xFF, (size_t)n * sizeof(double)));
    QDG_HIP(hipMemset(d.its, 0xFF, (size_t)n * sizeof(int)));
    if (sep) QDG_HIP(hipMemset(d.xsep, 0xFF, (size_t)n * QD_EW_MAX * sizeof(double)));
    const unsigned un = (unsigned)n;
    if (cls == MEM) launch_lane<9>(val, solo != 0, un, d);
    else if (cls == REG) {
        switch (S) {
#define C(s_, bin_) case s_: launch_lane<bin_>(val, solo != 0, un, d); break;
            C(2, 0) C(3, 1) C(4, 2) C(5, 3) C(6, 4) C(7, 5) C(8, 6) C(10, 7) C(12, 8)
#undef C
        }
    } else {
        const dim3 grid(blocks > 0 ? (unsigned)blocks : (un < 256u ? un : 256u)), block(64);
        if (val) {
            if (sep) qdg_k_wide<true, false><<<grid, block>>>(d.pool, d.off, un, d.xsep, d.lam, d.its);
            else     qdg_k_wide<true, true><<<grid, block>>>(d.pool, d.off, un, nullptr, d.lam, d.its);
        } else {
            if (sep) qdg_k_wide<false, false><<<grid, block>>>(d.pool, d.off, un, d.xsep, d.lam, d.its);
            else     qdg_k_wide<false, true><<<grid, block>>>(d.pool, d.off, un, nullptr, d.lam, d.its);
        }
    }
    QDG_HIP(hipGetLastError());
    QDG_HIP(hipDeviceSynchronize());
    QDG_HIP(hipMemcpy(pool.data(), d.pool, top * sizeof(double), hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(lam, d.lam, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(iters, d.its, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<double> xs;
    if (sep) {
        xs.resize((size_t)n * QD_EW_MAX);
        QDG_HIP(hipMemcpy(xs.data(), d.xsep, xs.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (int t = 0; t < n; ++t) {
        const int s = sizes[t];
        const double* rec = pool.data() + off[(size_t)t];
        resid[t] = val ? rec[1] : 0.0;
        memcpy(x + (size_t)t * (size_t)ldx, sep ? xs.data() + (size_t)t * QD_EW_MAX : rec + 2, sizeof(double) * (size_t)s);
    }
    return 0;
}

}  // namespace

extern "C" int qdg_eig_reg(int S, int n, const int* sizes, const double* packed, int ld, int validate, int solo, double* lam,
                           double* x, int ldx, double* resid, int* iters, char* err, int errlen) {
    return run(REG, S, n, sizes, packed, ld, validate, solo, 0, 1, lam, x, ldx, resid, iters, err, errlen);
}

extern "C" int qdg_eig_mem(int n, const int* sizes, const double* packed, int ld, int validate, int solo, double* lam,
                           double* x, int ldx, double* resid, int* iters, char* err, int errlen) {
    return run(MEM, 0, n, sizes, packed, ld, validate, solo, 0, 1, lam, x, ldx, resid, iters, err, errlen);
}

extern "C" int qdg_eig_wide(int n, const int* sizes, const double* packed, int ld, int validate, int blocks, int aliased,
                            double* lam, double* x, int ldx, double* resid, int* iters, char* err, int errlen) {
    return run(WIDE, 0, n, sizes, packed, ld, validate, 0, blocks, aliased, lam, x, ldx, resid, iters, err, errlen);
}

// out[5][n]: qd_rcp, qd_rcp1, qd_sqrt1 and the two results of qd_sqrt_rsqrt at x[0 .. n-1]
extern "C" int qdg_prims(int n, const double* x, double* out, char* err, int errlen) {
    if (err && errlen > 0) err[0] = 0;
    if (n < 1 || !x || !out) return bad_arg(err, errlen, "null argument or n < 1");
    DevBufs d;                                             // (pool: the arguments, lam: the results)
    QDG_HIP(hipMalloc(&d.pool, (size_t)n * sizeof(double)));
    QDG_HIP(hipMalloc(&d.lam, 5 * (size_t)n * sizeof(double)));
    QDG_HIP(hipMemcpy(d.pool, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    QDG_HIP(hipMemset(d.lam, 0xFF, 5 * (size_t)n * sizeof(double)));
    qdg_k_prims<<<dim3(((unsigned)n + 255u) / 256u), dim3(256)>>>(d.pool, (unsigned)n, d.lam);
    QDG_HIP(hipGetLastError());
    QDG_HIP(hipDeviceSynchronize());
    QDG_HIP(hipMemcpy(out, d.lam, 5 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The levels and the thermal core (csrc/qd_levels.h, csrc/qd_thermal.h).  Common arguments:
//   n, sizes[n]      tasks and their block sizes, 1 .. 32
//   packed, ld       task t's lower triangle, row-major, at packed + t * ld
//   blocks           persistent single-wave blocks striding over the tasks; 0: one per task, at most 256
//   poison           0: LDS as found.  1: before a block's first task every lane overwrites the whole __shared__ workspace
//                    with all-ones bits (a NaN as a double, -1 as an int), then a barrier.  2: the same before every task
// qdg_levels:  L in 1 .. QD_LEVELS_MAX;  lev[n][8]: the levels, +inf from min(L, s) on, as qd_k_levels writes them
// qdg_thermal: kT[n] finite and > 0;  pop[n][32], lam[n][32] (zero from s on), ztail[n], sweeps[n], V[n][32][32] (row-major,
//              zero outside the block; a null pointer skips it), and from the workspace after the solve, in the scaled units
//              of the block (||A||_inf in [1, 2)):  asym[n] = max |A_ij - A_ji|,  off[n] = max over i != j of |A_ij|
//              (NaN if any entry is; both 0 for s == 1, whose block the core never mirrors)
// ---------------------------------------------------------------------------------------------------------------
template <class WS>
__device__ void qdg_poison(WS& W) {
    static_assert(sizeof(WS) % 8 == 0, "whole 64-bit words");
    unsigned long long* p = reinterpret_cast<unsigned long long*>(&W);
    for (unsigned i = threadIdx.x; i < (unsigned)(sizeof(WS) / 8); i += 64u) p[i] = ~0ull;
    __syncthreads();
}

__global__ void __launch_bounds__(64)
qdg_k_levels(const double* __restrict__ packed, int ld, const int* __restrict__ sizes, unsigned n, int L, int poison,
             double* __restrict__ lev_out) {
    __shared__ QdLevelsWs W;
    if (poison == 1) qdg_poison(W);
    for (unsigned t = blockIdx.x; t < n; t += gridDim.x) {
        if (poison == 2) qdg_poison(W);
        const int s = __builtin_amdgcn_readfirstlane(sizes[t]);
        qd_levels_load_packed(W, packed + (size_t)t * (size_t)ld, s);
        qd_levels_solve(W, s, L);
        if (threadIdx.x == 0)
            for (int i = 0; i < QD_LEVELS_MAX; ++i) lev_out[(size_t)t * QD_LEVELS_MAX + i] = (i < L && i < s) ? W.lev[i] : INFINITY;
        __syncthreads();                                   // (lane 0 has read W.lev before the next task overwrites it)
    }
}

__global__ void __launch_bounds__(64)
qdg_k_thermal(const double* __restrict__ packed, int ld, const int* __restrict__ sizes, const double* __restrict__ kT, unsigned n,
              int poison, double* __restrict__ pop, double* __restrict__ lam, double* __restrict__ ztail, int* __restrict__ sweeps,
              double* __restrict__ V, double* __restrict__ asym, double* __restrict__ off) {
    __shared__ QdThermalWs W;
    const int l = (int)threadIdx.x;
    if (poison == 1) qdg_poison(W);
    for (unsigned t = blockIdx.x; t < n; t += gridDim.x) {
        if (poison == 2) qdg_poison(W);
        const int s = __builtin_amdgcn_readfirstlane(sizes[t]);
        qd_levels_load_packed(W.B, packed + (size_t)t * (size_t)ld, s);
        const int sw = qd_thermal_solve(W, s, kT[t]);
        // what is left of A: lane i takes row i; a NaN anywhere makes the figure NaN (fmax would drop it)
        double da = 0.0, df = 0.0;
        bool bad = false;
        if (s > 1 && l < s)
            for (int j = 0; j < s; ++j) {
                const double a = W.B.A[l * QD_LV_LD + j], b = W.B.A[j * QD_LV_LD + l];
                bad |= (a != a) | (b != b);
                da = fmax(da, fabs(a - b));
                if (j != l) df = fmax(df, fabs(a));
            }
        W.B.v[l] = bad ? NAN : da;
        W.B.w[l] = bad ? NAN : df;
        __syncthreads();
        if (l < QD_LV_MAX) {
            pop[(size_t)t * QD_LV_MAX + l] = l < s ? W.pop[l] : 0.0;
            lam[(size_t)t * QD_LV_MAX + l] = l < s ? W.lam[l] : 0.0;
        }
        if (V)
            for (int e = l; e < QD_LV_MAX * QD_LV_MAX; e += 64) {
                const int i = e / QD_LV_MAX, j = e % QD_LV_MAX;
                V[(size_t)t * (QD_LV_MAX * QD_LV_MAX) + e] = (i < s && j < s) ? W.V[i * QD_LV_LD + j] : 0.0;
            }
        if (l == 0) {
            double ma = 0.0, mf = 0.0;
            bool nan = false;
            for (int i = 0; i < s; ++i) {
                const double a = W.B.v[i], f = W.B.w[i];
                nan |= (a != a) | (f != f);
                ma = fmax(ma, a); mf = fmax(mf, f);
            }
            asym[t] = nan ? NAN : ma;
            off[t] = nan ? NAN : mf;
            ztail[t] = W.ztail;
            sweeps[t] = sw;
        }
        __syncthreads();                                   // (the lanes have read W before the next task overwrites it)
    }
}

namespace {

// device buffers of one call, freed on every way out
struct DevList {
    std::vector<void*> p;
    ~DevList() { for (void* q : p) (void)hipFree(q); }
};

// the checks both entry points share; smax out
int spectrum_args(int n, const int* sizes, const double* packed, int ld, int blocks, int poison, char* err, int errlen) {
    if (n < 1 || !sizes || !packed) return bad_arg(err, errlen, "null argument or n < 1");
    int smax = 0;
    for (int t = 0; t < n; ++t) {
        if (sizes[t] < 1 || sizes[t] > QD_LV_MAX) return bad_arg(err, errlen, "block size outside 1..32");
        if (sizes[t] > smax) smax = sizes[t];
    }
    if (ld < smax * (smax + 1) / 2) return bad_arg(err, errlen, "ld too small");
    if (blocks < 0 || blocks > 65535) return bad_arg(err, errlen, "blocks outside 0..65535");
    if (poison < 0 || poison > 2) return bad_arg(err, errlen, "poison outside 0..2");
    return 0;
}

#define QDG_ALLOC(ptr, bytes)                                  \
    do {                                                       \
        void* q_ = nullptr;                                    \
        QDG_HIP(hipMalloc(&q_, (bytes)));                      \
        d.p.push_back(q_);                                     \
        (ptr) = reinterpret_cast<decltype(ptr)>(q_);           \
    } while (0)

}  // namespace

extern "C" int qdg_levels(int n, const int* sizes, const double* packed, int ld, int L, int blocks, int poison, double* lev,
                          char* err, int errlen) {
    if (err && errlen > 0) err[0] = 0;
    if (int rc = spectrum_args(n, sizes, packed, ld, blocks, poison, err, errlen)) return rc;
    if (!lev) return bad_arg(err, errlen, "null output");
    if (L < 1 || L > QD_LEVELS_MAX) return bad_arg(err, errlen, "L outside 1..8");
    const size_t un = (size_t)n, pb = un * (size_t)ld * sizeof(double), lb = un * QD_LEVELS_MAX * sizeof(double);
    DevList d;
    double *dpk, *dlev;
    int* dsz;
    QDG_ALLOC(dpk, pb);
    QDG_ALLOC(dsz, un * sizeof(int));
    QDG_ALLOC(dlev, lb);
    QDG_HIP(hipMemcpy(dpk, packed, pb, hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dsz, sizes, un * sizeof(int), hipMemcpyHostToDevice));
    QDG_HIP(hipMemset(dlev, 0xFF, lb));
    const dim3 grid(blocks > 0 ? (unsigned)blocks : (n < 256 ? (unsigned)n : 256u)), block(64);
    qdg_k_levels<<<grid, block>>>(dpk, ld, dsz, (unsigned)n, L, poison, dlev);
    QDG_HIP(hipGetLastError());
    QDG_HIP(hipDeviceSynchronize());
    QDG_HIP(hipMemcpy(lev, dlev, lb, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int qdg_thermal(int n, const int* sizes, const double* packed, int ld, const double* kT, int blocks, int poison,
                           double* pop, double* lam, double* ztail, int* sweeps, double* V, double* asym, double* off, char* err,
                           int errlen) {
    if (err && errlen > 0) err[0] = 0;
    if (int rc = spectrum_args(n, sizes, packed, ld, blocks, poison, err, errlen)) return rc;
    if (!kT || !pop || !lam || !ztail || !sweeps || !asym || !off) return bad_arg(err, errlen, "null argument");
    for (int t = 0; t < n; ++t)
        if (!(kT[t] > 0.0) || !isfinite(kT[t])) return bad_arg(err, errlen, "kT must be finite and > 0");
    const size_t un = (size_t)n, pb = un * (size_t)ld * sizeof(double), vb = un * QD_LV_MAX * sizeof(double),
                 sb = un * sizeof(double), Vb = un * QD_LV_MAX * QD_LV_MAX * sizeof(double);
    DevList d;
    double *dpk, *dkt, *dpop, *dlam, *dzt, *dV = nullptr, *dasym, *doff;
    int *dsz, *dsw;
    QDG_ALLOC(dpk, pb);
    QDG_ALLOC(dsz, un * sizeof(int));
    QDG_ALLOC(dkt, sb);
    QDG_ALLOC(dpop, vb);
    QDG_ALLOC(dlam, vb);
    QDG_ALLOC(dzt, sb);
    QDG_ALLOC(dsw, un * sizeof(int));
    QDG_ALLOC(dasym, sb);
    QDG_ALLOC(doff, sb);
    if (V) QDG_ALLOC(dV, Vb);
    QDG_HIP(hipMemcpy(dpk, packed, pb, hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dsz, sizes, un * sizeof(int), hipMemcpyHostToDevice));
    QDG_HIP(hipMemcpy(dkt, kT, sb, hipMemcpyHostToDevice));
    QDG_HIP(hipMemset(dpop, 0xFF, vb));
    QDG_HIP(hipMemset(dlam, 0xFF, vb));
    QDG_HIP(hipMemset(dzt, 0xFF, sb));
    QDG_HIP(hipMemset(dsw, 0xFF, un * sizeof(int)));
    QDG_HIP(hipMemset(dasym, 0xFF, sb));
    QDG_HIP(hipMemset(doff, 0xFF, sb));
    if (V) QDG_HIP(hipMemset(dV, 0xFF, Vb));
    const dim3 grid(blocks > 0 ? (unsigned)blocks : (n < 256 ? (unsigned)n : 256u)), block(64);
    qdg_k_thermal<<<grid, block>>>(dpk, ld, dsz, dkt, (unsigned)n, poison, dpop, dlam, dzt, dsw, dV, dasym, doff);
    QDG_HIP(hipGetLastError());
    QDG_HIP(hipDeviceSynchronize());
    QDG_HIP(hipMemcpy(pop, dpop, vb, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(lam, dlam, vb, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(ztail, dzt, sb, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(sweeps, dsw, un * sizeof(int), hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(asym, dasym, sb, hipMemcpyDeviceToHost));
    QDG_HIP(hipMemcpy(off, doff, sb, hipMemcpyDeviceToHost));
    if (V) QDG_HIP(hipMemcpy(V, dV, Vb, hipMemcpyDeviceToHost));
    return 0;
}
