// qd_query.h -- what every stateless query family shares around a slot (qd_scan2d, qd_scan_affine, qd_scan1d, qd_scan_grid*; the
// inert record also serves qd_eval_points).  A query occupies one slot of a second set of parameter, state and signal
// buffers: its gather kernel copies the env's blocks into the slot with the query's base point applied (qd_slot_copy) and
// fills the family's own descriptor, the stages of an observation run on the slot, and qd_k_query_write hands the result to
// the caller.  The host part -- the inert record and the tail of the front ends that fill their records before the search
// (qd_line.h, qd_grid.h) -- is __host__ __device__, so the CPU tier checks it through those headers.  The front ends INSIDE
// the search kernels (qd_pixel.h) keep their own copies of that tail: sharing it moves their register allocation.
#pragma once
#include "qd_pixel.h"

// The inert record: all zero -- nvalid = 0, i.e. K copies of |0..0> without a coupling.  The redo pass skips it, the
// structure kernel finds every state isolated and emits no task.
QD_HD void qd_inert_record(QdPixelRec* rec) {
    static_assert(sizeof(QdPixelRec) % 8 == 0, "the inert record is written in 64-bit words");
    unsigned long long* w = reinterpret_cast<unsigned long long*>(rec);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(QdPixelRec) / 8); ++i) w[i] = 0ull;
}

// ---------------------------------------------------------------------------
// Tail of a front end: the 2N control values W of a point -> v_ext through the frame, then vpp and tc, exactly as the tail of
// qd_affine_voltages: same operations, same order, same fences.
// ---------------------------------------------------------------------------
template <int N>
QD_HD void qd_control_voltages(const double* par, const double* st, int frame, const double* W, double* v_ext, double* vpp,
                               double* tc) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
    const double* vgm = st + L.s_vgm;
    if (frame == QD_SCAN_PHYSICAL) {
#pragma unroll
        for (int i = 0; i < V; ++i) v_ext[i] = W[i];
    } else {
#pragma unroll
        for (int i = 0; i < G; ++i) { v_ext[i] = qd_dotN<G>(vgm + i * G, W) + par[L.origin + i]; QD_ROW_FENCE(); }
#pragma unroll
        for (int b = 0; b < NB; ++b) v_ext[G + b] = W[G + b];
    }
#pragma unroll
    for (int i = 0; i < G; ++i) { vpp[i] = qd_dotN<V>(par + L.cgd + i * V, v_ext); QD_ROW_FENCE(); }
    const double tc_base = par[L.scal + 0];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double vb_eff = v_ext[G + b] + qd_dotN<G>(par + L.cbg + b * G, v_ext);
        tc[b] = tc_base * exp(-par[L.alpha + b] * vb_eff);
        QD_ROW_FENCE();
    }
}

#if defined(__HIPCC__)
#include "qd_kernels.h"

// The query arrays of the families that sweep along direction vectors: qd_scan_affine and qd_scan_grid* (two directions and
// two ranges per query), qd_scan1d (one of each).
struct QdAffineQuery {
    const int* env_of_query;                                   // [nq]
    const double* dir;                                         // [nq][2][2N]: dx, dy; a line: [nq][2N]
    const double *range, *gate_v, *barrier_v, *sensor_v;       // [nq][4] (a line: [nq][2]), [nq][N], [nq][N-1], [nq] or null
    const double *vgm, *gamma;                                 // [nq][G][G] or null, [nq] or null
    int frame;
};

// a query renders when its env id is in [0, B) -- any direction is legal, the zero vector too -- and, where it names its
// axes (qd_scan2d; else `axes` is null), those are two different controls in [0, 2N)
__device__ __forceinline__ bool qd_query_live(const int* env_of_query, const int* axes, int q, int B, int N) {
    const int e = env_of_query[q];
    if (e < 0 || e >= B) return false;
    if (!axes) return true;
    const int ax = axes[2 * (size_t)q], ay = axes[2 * (size_t)q + 1];
    return ax >= 0 && ax < 2 * N && ay >= 0 && ay < 2 * N && ax != ay;
}

// ---------------------------------------------------------------------------
// Slot copy, by all BLOCK threads of a gather kernel's block: slot k (query q) <- parameter and state block of env env_of_query[q]
// (clamped into [0, B): a query that is not live renders a clamped env, the write kernel skips it), with the gate, barrier
// and sensor voltages of the query and its virtual gate matrix if given.  The `skip` state words from s_kmean on are left
// to the caller: the place of a descriptor that the front end inside the search reads (QdFrontScan, QdFrontAffine); with
// skip = 0 the Kalman block is copied as it is, no kernel behind a front kernel reads it.  The peak width the sensor stage
// will use becomes a CONSTANT of the slot's parameter copy (scal[1], with scal[3] = -1: "constant width"): the query's
// gamma if given, else the env's constant.  Returns the env's parameter block and the slot's two blocks.
// ---------------------------------------------------------------------------
struct QdSlot { const double* par; double *dp, *ds; };
template <int BLOCK, class Query>
__device__ __forceinline__ QdSlot qd_slot_copy(const Query& Q, int q, int k, int B, const QdLayout& L, const double* __restrict__ params,
                                               const double* __restrict__ state, double* __restrict__ sparams,
                                               double* __restrict__ sstate, int skip) {
    const int N = L.N, nb = L.nb, G = L.G;
    int e = Q.env_of_query[q];
    e = e < 0 ? 0 : (e >= B ? B - 1 : e);
    const double* par = params + (size_t)e * L.size;
    const double* st = state + (size_t)e * L.s_size;
    double* dp = sparams + (size_t)k * L.size;
    double* ds = sstate + (size_t)k * L.s_size;
    for (int i = threadIdx.x; i < L.s_size; i += BLOCK) {
        double v = st[i];
        if (i >= L.s_vgm && i < L.s_vgm + G * G) { if (Q.vgm) v = Q.vgm[(size_t)q * G * G + (i - L.s_vgm)]; }
        else if (i >= L.s_gate_v && i < L.s_gate_v + N) v = Q.gate_v[(size_t)q * N + (i - L.s_gate_v)];
        else if (i >= L.s_barrier_v && i < L.s_barrier_v + nb) v = Q.barrier_v[(size_t)q * nb + (i - L.s_barrier_v)];
        else if (i == L.s_sensor_gt) v = Q.sensor_v ? Q.sensor_v[q] : 0.0;      // sensor_voltage=None -> 0.0
        else if (i >= L.s_kmean && i < L.s_kmean + skip) continue;
        ds[i] = v;
    }
    for (int i = threadIdx.x; i < L.size; i += BLOCK) if (i != L.scal + 1 && i != L.scal + 3) dp[i] = par[i];
    if (threadIdx.x == 0) {
        dp[L.scal + 1] = Q.gamma ? Q.gamma[q] : par[L.scal + 1];
        dp[L.scal + 3] = -1.0;
    }
    return QdSlot{par, dp, ds};
}

// ---------------------------------------------------------------------------
// write: slot k -> the caller's slot base + k, n values each.  raw [nq][n] float64, image [nq][n] float32 normalised with the
// slot's own percentiles (qd_norm, as qd_k_write_obs), plohi [nq][2], occupations [nq][n][N] float64; each may be null.
// Value p of slot k is sz[k * zs + p], its occupations socc[(k * os + p) * N ..]: an image has n = zs = os = P, a line or a
// grid of n points in a slot of SP records the packed row (zs = n) and os = SP.  Queries that are not live (qd_query_live)
// leave their slots untouched.  grid = (ceil(n / 256), cnt).
// ---------------------------------------------------------------------------
__global__ void qd_k_query_write(const int* __restrict__ env_of_query, const int* __restrict__ axes, int base, int B, int N, int n,
                                 int zs, int os, const double* __restrict__ sz, const double* __restrict__ splohi,
                                 const double* __restrict__ socc, double* __restrict__ raw_dst, float* __restrict__ image_dst,
                                 double* __restrict__ plohi_dst, double* __restrict__ occ_dst) {
    const int k = blockIdx.y, q = base + k;
    if (!qd_query_live(env_of_query, axes, q, B, N)) return;
    const double lo = splohi[2 * k], hi = splohi[2 * k + 1];
    if (plohi_dst && blockIdx.x == 0 && threadIdx.x < 2) plohi_dst[2 * (size_t)q + threadIdx.x] = threadIdx.x ? hi : lo;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double z = sz[(size_t)k * zs + p];
    if (raw_dst) raw_dst[(size_t)q * n + p] = z;
    if (image_dst) image_dst[(size_t)q * n + p] = qd_norm(z, lo, hi);
    if (occ_dst)
        for (int i = 0; i < N; ++i) occ_dst[((size_t)q * n + p) * N + i] = socc[((size_t)k * os + p) * N + i];
}

#endif  // __HIPCC__
