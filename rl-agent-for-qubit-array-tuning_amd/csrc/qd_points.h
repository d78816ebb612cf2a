// qd_points.h -- point evaluation (qd_eval_points): charge_sensor_open(vg, vb) / ground_state_open(vg, vb) of the reference's
// physics package (TunnelCoupledChargeSensed.py:312-380, ground_state.py:24-166) at arbitrary physical voltages, not at the
// pixels of a scan.  A point takes the place of a pixel: the front kernel fills its QdPixelRec from the caller's voltages in
// the hand-over form of the tile search (qd_tile_hand_over), the redo instantiation of the per-pixel search and the
// ground-state kernels then run on those records as they do behind a scan, and the write kernel forms the noise-free sensor
// signal.  qd_point_front is __host__ __device__ like the rest of the pixel front end, so the CPU tier checks it against
// qd_pixel_voltages (tests/hosttest_points).
#pragma once
#include "qd_query.h"

// ---------------------------------------------------------------------------
// a10 + a8 front end of one point.  par: env parameter block; v_ext[2N] = [physical gate voltages (G), barrier voltages (nb)].
// Outputs as qd_pixel_voltages + qd_pixel_continuous give them for a pixel with the same v_ext, operation for operation
// (qd_pixel_voltages lines "vpp" and "a10", then the non-redo branch of qd_k_candidates): vpp[G] = cgd_full @ v_ext, tc[nb],
// vd[N] the (possibly scaled) v', ncont[N], isa = 1 / s_a.
// ---------------------------------------------------------------------------
template <int N>
QD_HD void qd_point_front(const double* par, const double* v_ext, double* vpp, double* tc, double* vd, double* ncont, double* isa) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
#pragma unroll
    for (int i = 0; i < G; ++i) { vpp[i] = qd_dotN<V>(par + L.cgd + i * V, v_ext); QD_ROW_FENCE(); }
    const double tc_base = par[L.scal + 0];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double vb_eff = v_ext[G + b] + qd_dotN<G>(par + L.cbg + b * G, v_ext);
        tc[b] = tc_base * exp(-par[L.alpha + b] * vb_eff);
        QD_ROW_FENCE();
    }
#pragma unroll
    for (int i = 0; i < N; ++i) vd[i] = vpp[i];
    qd_pixel_continuous<N>(par, v_ext, vd, ncont, isa);
}

#if defined(__HIPCC__)
#include "qd_kernels.h"     // QdPixelRec's users: qd_tile_hand_over, QD_T_REDO

// Slots of one launch: slot k is one env's parameter copy and C*P records; it evaluates `cnt` (1..C*P) consecutive points
// starting at row `start` of the caller's arrays, on env `env`.  The table travels as a kernel argument.
#define QD_POINTS_MAX_SLOTS 64      // (qdsim.h: QD_POINTS_SLOTS)
#define QD_POINTS_BLOCK 256
struct QdPointSlots {
    long long start[QD_POINTS_MAX_SLOTS];
    double gamma[QD_POINTS_MAX_SLOTS];      // peak width of the slot's group (own_gamma: the env's scal[1] instead)
    int env[QD_POINTS_MAX_SLOTS];
    int cnt[QD_POINTS_MAX_SLOTS];
    int own_gamma;
};

// slot k <- parameter and state block of env T.env[k].  grid = slots, block = QD_POINTS_BLOCK.
__global__ void __launch_bounds__(QD_POINTS_BLOCK)
qd_k_points_gather(QdPointSlots T, int N, const double* __restrict__ params, const double* __restrict__ state,
                   double* __restrict__ qparams, double* __restrict__ qstate) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.x, e = T.env[k];
    const double* par = params + (size_t)e * L.size;
    const double* st = state + (size_t)e * L.s_size;
    for (int i = threadIdx.x; i < L.size; i += QD_POINTS_BLOCK) qparams[(size_t)k * L.size + i] = par[i];
    for (int i = threadIdx.x; i < L.s_size; i += QD_POINTS_BLOCK) qstate[(size_t)k * L.s_size + i] = st[i];
}

// ---------------------------------------------------------------------------
// front end, one point per lane: record j of slot k (channel j / P, pixel j % P of the slot's C*P records) <- point
// T.start[k] + j in hand-over form, nvalid = QD_T_REDO: the redo pass searches it.  Past the slot's points the inert record
// (qd_inert_record, qd_query.h).  grid = (ceil(C P / block), slots).
// ---------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(QD_POINTS_BLOCK)
qd_k_points_front(QdPointSlots T, int CP, const double* __restrict__ vg, const double* __restrict__ vb,
                  const double* __restrict__ qparams, QdPixelRec* __restrict__ recs) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.y;
    const int j = blockIdx.x * QD_POINTS_BLOCK + threadIdx.x;
    if (j >= CP) return;
    QdPixelRec* rec = recs + (size_t)k * CP + j;
    if (j >= T.cnt[k]) { qd_inert_record(rec); return; }
    const double* par = qparams + (size_t)k * L.size;
    const size_t q = (size_t)(T.start[k] + j);
    double v_ext[V], vpp[G], tc[NB], vd[N], ncont[N], isa;
#pragma unroll
    for (int i = 0; i < G; ++i) v_ext[i] = vg[q * G + i];
#pragma unroll
    for (int b = 0; b < NB; ++b) v_ext[G + b] = vb[q * NB + b];
    qd_point_front<N>(par, v_ext, vpp, tc, vd, ncont, &isa);
#pragma unroll
    for (int i = 0; i < G; ++i) rec->vpp[i] = vpp[i];
#pragma unroll
    for (int b = 0; b < NB; ++b) rec->tc[b] = tc[b];
    qd_tile_hand_over<N>(rec, vd, ncont, isa);
}

// ---------------------------------------------------------------------------
// The kept lists of n records from search order into the reference order, increasing (E, idx), in place: the order a
// QD_FLAG_VALIDATE handle's search hands to the ground-state stage (qd_search_sort, same comparison), whose occupations the
// points' occupations then equal bit for bit.  Only the first nvalid slots move (the |0..0> padding behind them carries one
// energy); inert records (nvalid = 0) are left alone.  One record per lane, lists in LDS.  grid = ceil(n / 64), block = 64.
// ---------------------------------------------------------------------------
template <int KC>
__global__ void __launch_bounds__(64)
qd_k_points_sort(QdPixelRec* __restrict__ recs, long n) {
    __shared__ double se[KC * 64];
    __shared__ uint16_t sid[KC * 64];
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    QdPixelRec* rec = recs + i;
    const int nv = rec->nvalid < KC ? rec->nvalid : KC;
    if (nv < 2) return;
    for (int m = 0; m < nv; ++m) { se[m * 64 + threadIdx.x] = rec->E[m]; sid[m * 64 + threadIdx.x] = rec->idx[m]; }
    QdSearch<2, KC> S;                                     // (the sort reads its buffer, strides and count only)
    S.e = se + threadIdx.x; S.es = 64; S.id = sid + threadIdx.x; S.is = 64; S.count = nv;
    qd_search_sort(S);
    for (int m = 0; m < nv; ++m) { rec->E[m] = se[m * 64 + threadIdx.x]; rec->idx[m] = sid[m * 64 + threadIdx.x]; }
}

// ---------------------------------------------------------------------------
// a15 without noise, one point per lane: c0 from qd_k_gs_select ->
//   signal = sum_{k=-5..4} 1 / (((c0 + 2 a k) / gamma)^2 + 1)
// (the expression of qd_k_sensor with eta = 0, in its order), and the occupations, to the caller's rows.  Padding lanes
// write nothing.  grid = (ceil(C P / block), slots).
// ---------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(QD_POINTS_BLOCK)
qd_k_points_write(QdPointSlots T, int CP, const double* __restrict__ qparams, const double* __restrict__ qz,
                  const double* __restrict__ qocc, double* __restrict__ signal_dst, double* __restrict__ occ_dst) {
    constexpr int G = N + 1;
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.y;
    const int j = blockIdx.x * QD_POINTS_BLOCK + threadIdx.x;
    if (j >= CP || j >= T.cnt[k]) return;
    const double* par = qparams + (size_t)k * L.size;
    const size_t q = (size_t)(T.start[k] + j), sp = (size_t)k * CP + j;
    if (signal_dst) {
        const double c0 = qz[sp];
        const double a = par[L.cdd_inv + N * G + N];
        const double gamma = T.own_gamma ? par[L.scal + 1] : T.gamma[k];
        const double eta = 0.0;
        double s = 0.0;
#pragma unroll
        for (int kk = -QD_NPEAK; kk < QD_NPEAK; ++kk) {
            const double dF = c0 + 2.0 * a * ((double)kk + eta);
            const double rr = dF / gamma;
            s += 1.0 / (rr * rr + 1.0);
        }
        signal_dst[q] = s;
    }
    if (occ_dst) {
#pragma unroll
        for (int i = 0; i < N; ++i) occ_dst[q * N + i] = qocc[sp * N + i];
    }
}

#endif  // __HIPCC__
