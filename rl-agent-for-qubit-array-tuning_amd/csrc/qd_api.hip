// qd_api.hip -- C-ABI of libqdsim.so (include/qdsim.h): handle, device buffers,
// kernel launches.  gfx950 only; no torch, no exceptions across the boundary.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <type_traits>

#include "qdsim.h"
#include "qd_kernels.h"
#include "qd_fullspace.h"
#include "qd_probe.h"
#include "qd_latch.h"
#include "qd_points.h"
#include "qd_scan.h"
#include "qd_affine.h"
#include "qd_line.h"
#include "qd_grid.h"
#include "qd_closed.h"
#include "qd_levels.h"
#include "qd_thermal.h"
#include "qd_thermal_blocks.h"
#include "qd_response_grid.h"
#include "qd_response.h"
#include "qd_levels_blocks.h"
#include "qd_scratch.h"

// The owners of a stream and of an event.  With the two memory policies of qd_scratch.h these are the only places that
// allocate, create, free or destroy.
struct QdStream : QdNoCopy {
    hipStream_t s = nullptr;
    ~QdStream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};
struct QdEvent : QdNoCopy {
    hipEvent_t e = nullptr;
    ~QdEvent() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e, flags); }
};

// Scratch + streams of one launch chunk in flight.  Product mode keeps TWO: consecutive chunks alternate between them on
// two internal streams, so the candidate search of one chunk (float64 VALU bound) runs beside the ground-state stage of
// the other (its solve / select launches wait on memory most of the time).
#define QD_MAX_LANES 4
struct QdLane {
    QdDev<QdPixelRec> recs;                            // [chunk][C][P] candidate records (validate mode: all B envs)
    QdDev<unsigned char> slabs;                        // scratch of the ground-state kernels: one slab per batch of ppb pixels in flight
    QdDev<unsigned> gtiles;                            // [QD_GS_NBIN] tiles per size class of the launch in flight, then the tile lists
    QdDev<unsigned char> wide;                         // the wide class's lists (full space with a sector above 32 states)
    QdStream run, side, side2;                         // the solve launches of the size classes run on three streams: the memory solver
    QdEvent ev_fork, ev_join, ev_join2, ev_done;       // of the rare 13..32-state blocks is one long latency chain, and the short
};                                                     // register-solver launches fill each other's tails

// Pinned two-slot staging ring of qd_load_episodes (doubles per slot) with one event per slot that says when the stream
// has consumed it: the call returns without waiting for the stream.
struct QdStageRing {
    QdBuf<double, QdPinned> slot[2];
    QdEvent ev[2];
    bool busy[2] = {false, false}; int turn = 0;
    ~QdStageRing() { for (int k = 0; k < 2; ++k) (void)wait(k); }      // (runs before the slots are freed)
    hipError_t wait(int k) {
        const hipError_t e = busy[k] ? hipEventSynchronize(ev[k].e) : hipSuccess;
        if (e == hipSuccess) busy[k] = false;
        return e;
    }
    // room for `need` doubles in both slots; growing waits for the slots in use
    hipError_t room(size_t need) {
        if (need <= slot[0].cap) return hipSuccess;
        for (int k = 0; k < 2; ++k) {
            if (hipError_t e = wait(k)) return e;
            if (!ev[k].e) if (hipError_t e = ev[k].create(hipEventDisableTiming)) return e;
        }
        QdBuf<double, QdPinned>* const both[] = {&slot[0], &slot[1]};
        const size_t n[] = {need, need};
        return qd_reserve_group(both, n);
    }
    // the next slot, free to be written
    hipError_t take(int& k) { k = turn; turn ^= 1; return wait(k); }
};

// The per-env device buffers the hot launchers work on, handed to them as an argument: qd_env_bufs() is the view of the
// handle's own envs, a QdScratchSet gives one of its blocks starting from a zeroed object, so whatever a probe does not
// set reaches the kernels as nullptr / 0 and never as the envs' pointer.  The view also says what shape its blocks have,
// and every launcher reads grid, front end and channel template argument from there.
// who fills the records: QdFrontEnv / QdFrontScan / QdFrontAffine (qd_pixel.h) inside the search kernels, or, QD_FRONT_LINE, a
// front kernel of its own before them (qd_k_line_front), behind which only the redo instantiation of the search runs
enum QdFront { QD_FRONT_ENV, QD_FRONT_SCAN, QD_FRONT_AFFINE, QD_FRONT_LINE };
struct QdEnvBufs {
    double *params, *state, *zraw, *plohi, *occ, *eig;
    int channels;                           // channel images per block: h->C, or 1 on the buffers of qd_scan2d
    int R, P;                               // side and pixel count of one channel image: h->R and h->P, or those of a line's slot (qd_scan1d)
    QdFront front;
    int noise_flags;
    unsigned long long* tel; int tel_words;
    unsigned long long serial;              // number of the observation being rendered (Philox counter word)
    uint32_t env_off;                       // global env id of block 0 (Philox key word = env_off + block index)
};

// A second set of per-env buffers for the slots in flight of qd_probe or qd_eval_points: parameter copies, state blocks
// and signals, with percentiles (probes), occupations (points; probes that latch or hand them out) or telegraph words
// (probes with sensor noise).  One group: all of them are there, or none.  A member asked for with 0 per slot keeps what
// an earlier call gave it, so a set only grows.
struct QdScratchSet {
    QdDev<double> params, state, z, plohi, occ;
    QdDev<unsigned long long> tel;
    hipError_t reserve(const QdLayout& L, size_t CP, size_t slots, size_t plohi_per_slot, size_t occ_per_slot, size_t tel_per_slot) {
        QdDev<double>* const all[] = {&params, &state, &z, &plohi, &occ};
        const size_t n[] = {slots * L.size, slots * L.s_size, slots * CP, slots * plohi_per_slot, slots * occ_per_slot};
        hipError_t e = qd_reserve_group(all, n);
        if (e == hipSuccess && (e = tel.reserve(slots * tel_per_slot)) != hipSuccess)
            for (QdDev<double>* b : all) b->release();
        if (e != hipSuccess) tel.release();
        return e;
    }
    // without noise, eigenvalues or telegraph words
    QdEnvBufs view(int channels, int R, QdFront front) const {
        QdEnvBufs b{};
        b.params = params.p; b.state = state.p; b.zraw = z.p; b.plohi = plohi.p; b.occ = occ.p;
        b.channels = channels; b.R = R; b.P = R * R; b.front = front;
        return b;
    }
};

struct qd_handle {
    qd_config cfg;
    QdLane lanes[QD_MAX_LANES]; int nlanes;
    QdEvent ev_start;
    int device;
    QdLayout L;
    int N, R, B, C, P;
    int chunk;
    QdDev<double> params, state, zraw, plohi, occ, eig;
    QdDev<int> steps;
    float *gimg, *pimg, *bimg, *volt;
    QdDev<unsigned long long> tel; int tel_words;
    QdDev<unsigned long long> tstats;       // tile-search [0..15] and eigen-solver [16..31] counters (validate mode)
    int tile_search;                        // 0: per-pixel search only; 1: tile-shared candidate search + exact redo pass
    int kept, kc;                           // K = num_charge_states (1..32) and the kept-set size the candidate stage runs (8, 16, 32)
    int full_m;                             // > 0: the untruncated space with at most full_m carriers per dot (qd_fullspace.h)
    QdDev<QdFullTab> ftab;                  //   its sector tables (device)
    int full_spl;                           //   states per lane of its structure kernel (2, 4, 8)
    QdWide wide;                            //   the wide class (sectors of 33..64 states): capw > 0 when the handle has one; buf is the lane's
    int ppb;                                // pixels per ground-state batch (slab): QD_GS_PPB, or qd_full_ppb in the full space
    int gs_chunk;                           // envs per ground-state launch (<= chunk)
    size_t gs_batches;                      // slabs a lane holds = gs_chunk * C * batches per image
    int cus;                                // compute units of the device
    int solve_grid[QD_GS_NBIN];             // persistent blocks of qd_k_gs_solve per size class: as many as are resident at once
    QdStageRing stage;
    unsigned long long obs_serial;
    // probe scans (qd_probe): one launch chunk of parameter copies, state blocks, signals and percentiles, allocated by the
    // first probe; the composite's compact channel, per-scan percentiles and select state (qd_probe_compose) likewise
    QdScratchSet probe;
    QdDev<double> cz, cplohi;
    QdDev<QdSelState> sel;
    // point evaluation (qd_eval_points): parameter and state copies, sensor constants and occupations of the slots in flight,
    // allocated by the first call
    QdScratchSet points;
    // axis scans (qd_scan2d): one launch chunk of parameter copies, state blocks (with the axes descriptors), P doubles of signal and
    // percentiles per query in flight (occupations and telegraph words when asked for), allocated by the first call
    QdScratchSet scan;
    // affine scans (qd_scan_affine) render on the slots of `scan`; one descriptor (ranges, two direction vectors, frame) per
    // query in flight, whose address the slot's state block copy carries, allocated by the first call
    QdDev<QdAffineAxes> affine_axes;
    // lines (qd_scan1d): slots of ceil(sqrt(n))^2 records each -- parameter copies, state blocks, signals, percentiles
    // (occupations and telegraph words when asked for), one descriptor and a dense row of n signals per line in flight,
    // allocated by the first call and grown by a call that needs more
    QdScratchSet line;
    QdDev<QdLineAxes> line_axes;
    QdDev<double> line_dense;
    // grids (qd_scan_grid): the line buffers above and one descriptor per grid in flight
    QdDev<QdGridAxes> grid_axes;
    // the closed regime (qd_eval_points_closed): the total charge of every slot in flight, allocated by the first call
    QdDev<int32_t> closed_q;
    // per env (B bytes, calloc in qd_create, freed in qd_destroy): the parameter block of its last qd_load_episodes switches the
    // voltage-dependent capacitance model on (scal[4]); qd_eval_points_response refuses such envs on the host.  qd_load_episodes
    // is the only path that uploads parameter blocks, so the note cannot go stale.
    unsigned char* vc_on;
    mutable char err[512];                  // (the launchers take the handle const and still report through it)
};

static bool qd_validate(const qd_handle* h) { return (h->cfg.flags & QD_FLAG_VALIDATE) != 0; }

static QdEnvBufs qd_env_bufs(const qd_handle* h) {
    QdEnvBufs b{};
    b.params = h->params.p; b.state = h->state.p; b.zraw = h->zraw.p; b.plohi = h->plohi.p; b.occ = h->occ.p; b.eig = h->eig.p;
    b.channels = h->C; b.R = h->R; b.P = h->P; b.front = QD_FRONT_ENV;
    b.noise_flags = h->cfg.noise_flags;
    b.tel = h->tel.p; b.tel_words = h->tel_words;
    b.serial = h->obs_serial;
    b.env_off = (uint32_t)h->cfg.env_id_offset;
    return b;
}

static int qd_fail(const qd_handle* h, int code, const char* what) { if (h) snprintf(h->err, sizeof(h->err), "%s", what); return code; }
static int qd_fail(const qd_handle* h, int code, const char* what, hipError_t e) {      // e: the failure of a HIP call
    if (h) snprintf(h->err, sizeof(h->err), "%s: %s", what, hipGetErrorString(e));
    return code;
}
// a message that names the entry point: `fmt` has one %s for `who`, and may have a second one for `what`
static int qd_failf(const qd_handle* h, int code, const char* fmt, const char* who, const char* what) {
    if (h) snprintf(h->err, sizeof(h->err), fmt, who, what);
    return code;
}
static int qd_failf(const qd_handle* h, int code, const char* fmt, const char* who) { return qd_failf(h, code, fmt, who, ""); }
// the struct_size (first field) of any option struct; `opts` null is a call without options; `what` is the whole message
static int qd_check_struct_size(const qd_handle* h, const void* opts, size_t size, const char* what) {
    int32_t got = (int32_t)size;
    if (opts) memcpy(&got, opts, sizeof(got));
    return got == (int32_t)size ? (int)QD_OK : qd_fail(h, QD_ERR_ARG, what);
}
// the temperatures of a points call, one per group on the host
static int qd_check_kT_host(const qd_handle* h, const char* who, const double* kT, int ng) {
    if (!kT) return qd_failf(h, QD_ERR_ARG, "%s: kT_host is NULL", who);
    for (int g = 0; g < ng; ++g)
        if (!(kT[g] > 0.0) || !(kT[g] < INFINITY)) return qd_failf(h, QD_ERR_ARG, "%s: kT must be finite and > 0", who);
    return QD_OK;
}
// the refusal of the response calls, points and grids, for an env with the voltage-dependent capacitance model (h->vc_on)
static int qd_fail_vc(const qd_handle* h, const char* who) {
    return qd_failf(h, QD_ERR_STATE, "%s: the env carries the voltage-dependent capacitance model, whose per-point scale "
                                    "factors make d F / d v depend on v; that chain rule is not built", who);
}
#define QD_HIP(call)                                                              \
    do { hipError_t e_ = (call); if (e_ != hipSuccess) return qd_fail(h, QD_ERR_HIP, #call, e_); } while (0)

// Every entry point works on the handle's GPU and leaves the calling thread's current device
// (which is also PyTorch's) as it found it.
struct QdDeviceGuard {
    int prev; bool switched; hipError_t err;
    explicit QdDeviceGuard(int dev) : prev(-1), switched(false), err(hipSuccess) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = (err == hipSuccess); }
    }
    ~QdDeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define QD_ON_DEVICE(h)                                                           \
    QdDeviceGuard guard_((h)->device);                                            \
    if (guard_.err != hipSuccess) return qd_fail((h), QD_ERR_HIP, "hipSetDevice", guard_.err)

// two events that are destroyed on every exit path
struct QdEventPair {
    QdEvent a, b; bool ok;
    QdEventPair() : ok(a.create(hipEventDefault) == hipSuccess && b.create(hipEventDefault) == hipSuccess) {}
};

#define QD_DISPATCH_N(N_, ...)                                                    \
    switch (N_) {                                                                 \
        case 2: { constexpr int NN = 2; __VA_ARGS__; } break;                            \
        case 3: { constexpr int NN = 3; __VA_ARGS__; } break;                            \
        case 4: { constexpr int NN = 4; __VA_ARGS__; } break;                            \
        case 5: { constexpr int NN = 5; __VA_ARGS__; } break;                            \
        case 6: { constexpr int NN = 6; __VA_ARGS__; } break;                            \
        case 7: { constexpr int NN = 7; __VA_ARGS__; } break;                            \
        case 8: { constexpr int NN = 8; __VA_ARGS__; } break;                            \
        default: return qd_fail(h, QD_ERR_ARG, "n_dot must be in 2..8");          \
    }

// kept-set size of the candidate stage (KK = h->kc)
#define QD_DISPATCH_KC(KC_, ...)                                                  \
    switch (KC_) {                                                                \
        case 8: { constexpr int KK = 8; __VA_ARGS__; } break;                            \
        case 16: { constexpr int KK = 16; __VA_ARGS__; } break;                          \
        case 32: { constexpr int KK = 32; __VA_ARGS__; } break;                          \
        default: return qd_fail(h, QD_ERR_ARG, "kept-set size must be 8, 16 or 32");     \
    }

// a boolean template argument: NAME_ is a constexpr bool inside the statement
#define QD_DISPATCH_BOOL(COND_, NAME_, ...)                                       \
    { if (COND_) { constexpr bool NAME_ = true; __VA_ARGS__; } else { constexpr bool NAME_ = false; __VA_ARGS__; } }

// the front end of a buffer view's records: FE is the search kernels' policy type inside the statement.  (A line's records
// are filled before the search: its redo pass never asks FE for voltages, only for the ONE channel image per slot, and so
// runs the instantiation of the affine scans.)
#define QD_DISPATCH_FRONT(FRONT_, ...)                                            \
    { if ((FRONT_) == QD_FRONT_SCAN) { using FE = QdFrontScan; __VA_ARGS__; }                                    \
      else if ((FRONT_) == QD_FRONT_AFFINE || (FRONT_) == QD_FRONT_LINE) { using FE = QdFrontAffine; __VA_ARGS__; } \
      else { using FE = QdFrontEnv; __VA_ARGS__; } }

extern "C" int qd_param_block_doubles(int n) { return (n < 2 || n > QD_MAXN) ? -1 : qd_layout(n).size; }
extern "C" int qd_state_block_doubles(int n) { return (n < 2 || n > QD_MAXN) ? -1 : qd_layout(n).s_size; }
extern "C" int qd_layout_query(int n, int32_t* out) {
    if (n < 2 || n > QD_MAXN || !out) return QD_ERR_ARG;
    QdLayout L = qd_layout(n);
    memcpy(out, &L, sizeof(L));
    return QD_OK;
}

// Kalman priors (KalmanUpdater.py:64-81): NN couplings prior_mean, NNN couplings prior_mean_nnn when they are
// tracked (include_nnn = not nearest_neighbour, env.py:784), variance prior_variance; everything else 0.
static void qd_kalman_priors(const qd_config& cfg, int N, double* km, double* kv) {
    for (int i = 0; i < N * N; ++i) { km[i] = 0.0; kv[i] = 0.0; }
    for (int i = 0; i < N - 1; ++i) {
        km[i * N + i + 1] = km[(i + 1) * N + i] = cfg.kalman_prior_mean;
        kv[i * N + i + 1] = kv[(i + 1) * N + i] = cfg.kalman_prior_variance;
    }
    if (cfg.cnn_outputs != 2)
        for (int i = 0; i < N - 2; ++i) {
            km[i * N + i + 2] = km[(i + 2) * N + i] = cfg.kalman_prior_mean_nnn;
            kv[i * N + i + 2] = kv[(i + 2) * N + i] = cfg.kalman_prior_variance;
        }
}

// persistent waves: per size class as many blocks of qd_k_gs_solve as are resident at once for its register budget
template <bool VAL, int BIN = 0>
static hipError_t qd_solve_grids(int cus, int* grid) {
    if constexpr (BIN < QD_GS_NBIN) {
        int n = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, qd_k_gs_solve<BIN, VAL>, 256, 0);
        if (e != hipSuccess) return e;
        grid[BIN] = cus * (n < 1 ? 1 : n);
        return qd_solve_grids<VAL, BIN + 1>(cus, grid);
    } else {
        return hipSuccess;
    }
}

extern "C" const char* qd_last_error(const qd_handle* h) { return h ? h->err : "null handle"; }

extern "C" int qd_create(const qd_config* cfg, int device, qd_handle** out) {
    if (!cfg || !out || cfg->struct_size != (int32_t)sizeof(qd_config)) return QD_ERR_ARG;
    if (cfg->n_dot < 2 || cfg->n_dot > QD_MAXN || cfg->resolution < 2 || cfg->batch < 1) return QD_ERR_ARG;
    if (cfg->cnn_outputs != 2 && cfg->cnn_outputs != 3) return QD_ERR_ARG;
    if (cfg->gate_curve_type < 0 || cfg->gate_curve_type > 3 || cfg->update_method < 0 || cfg->update_method > 1) return QD_ERR_ARG;
    if (cfg->flags & QD_FLAG_RETIRED_TILE_FUSED) return QD_ERR_ARG;      // the fused tile kernel of round 2 is gone
    if (cfg->num_charge_states > QD_K) return QD_ERR_ARG;
    if (cfg->num_charge_states < 0 && !qd_full_supported(cfg->n_dot, -cfg->num_charge_states)) return QD_ERR_ARG;
    qd_handle* h = new (std::nothrow) qd_handle();
    if (!h) return QD_ERR_NOMEM;
    h->cfg = *cfg; h->device = device;
    h->N = cfg->n_dot; h->R = cfg->resolution; h->B = cfg->batch;
    h->vc_on = (unsigned char*)calloc((size_t)cfg->batch, 1);
    if (!h->vc_on) { delete h; return QD_ERR_NOMEM; }
    h->C = h->N - 1; h->P = h->R * h->R; h->L = qd_layout(h->N);
    // K kept states; the candidate stage runs the smallest kept-set size >= K and hands over its first K
    h->kept = cfg->num_charge_states > 0 ? cfg->num_charge_states : QD_K;
    h->kc = h->kept <= 8 ? 8 : (h->kept <= 16 ? 16 : 32);
    h->full_m = cfg->num_charge_states < 0 ? -cfg->num_charge_states : 0;
    *out = h;
    QD_ON_DEVICE(h);
    const bool val = (cfg->flags & QD_FLAG_VALIDATE) != 0;
    QdFullTab ftab;
    h->ppb = QD_GS_PPB;
    if (h->full_m) {
        qd_full_build(h->N, h->full_m, ftab);
        h->ppb = qd_full_ppb(ftab, val);
        if (h->ppb < 1) return qd_fail(h, QD_ERR_ARG, "the full charge-state space of this shape does not fit a slab");
        h->full_spl = qd_full_spl(ftab.M);
        if (qd_full_wide(ftab.maxsec)) h->wide.capw = (unsigned)((h->ppb * qd_full_wide_tasks(ftab) + 1) & ~1);
        QD_HIP(h->ftab.reserve(1));
        QD_HIP(hipMemcpy(h->ftab.p, &ftab, sizeof(QdFullTab), hipMemcpyHostToDevice));
    }
    const size_t per_env_rec = (size_t)h->C * h->P * sizeof(QdPixelRec);
    const size_t batches_per_env = (size_t)h->C * ((h->P + h->ppb - 1) / h->ppb);
    const size_t per_env_slab = batches_per_env * (qd_gs_slab_bytes(val) + 4 * (qd_gs_tile_off(QD_GS_NBIN, 1)) + qd_wide_bytes(h->wide.capw));
    // scratch in flight per launch, sized for 288 GB of HBM: candidate records (488 B / pixel) + the ground-state slabs
    // (worst case 5.7 KB / pixel: a pixel whose 32 states form ONE hop component needs a 528-double block) -- 64 GiB, i.e.
    // 388 envs of the 8-dot 64x64 headline per launch (measured, whole bench: 20 GiB 9 070, 40 GiB 9 670, 64 GiB 9 950 env-steps/s),
    // but never more than a third of what is free on the device right now
    size_t budget = (size_t)64 << 30, free_b = 0, total_b = 0;
    if (const char* gib = getenv("QDSIM_SCRATCH_GIB")) { const long g = atol(gib); if (g > 0) budget = (size_t)g << 30; }   // (sizing experiments)
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b / 3 < budget) budget = free_b / 3;
    int chunk = cfg->env_chunk, gs_chunk;
    h->nlanes = 1;
    if (val) {
        // validate mode keeps every env's records (qd_get_candidates); only the slabs are chunked
        chunk = h->B;
        size_t g = budget / per_env_slab;
        gs_chunk = (int)(g < 1 ? 1 : (g > (size_t)h->B ? (size_t)h->B : g));
        if (cfg->env_chunk > 0 && cfg->env_chunk < gs_chunk) gs_chunk = cfg->env_chunk;
    } else {
        h->nlanes = 2;
        if (const char* ls = getenv("QDSIM_LANES")) { const int l = atoi(ls); if (l >= 1 && l <= QD_MAX_LANES) h->nlanes = l; }   // (experiments)
        if (chunk <= 0) {
            size_t g = budget / h->nlanes / (per_env_rec + per_env_slab);   // the lanes share the budget
            chunk = (int)(g < 1 ? 1 : g);
        }
        if (const char* cs = getenv("QDSIM_CHUNK")) { const int c = atoi(cs); if (c >= 1) chunk = c; }              // (experiments)
        if (chunk >= h->B) {
            // one launch would cover the batch: two halves on the two lanes still overlap the search of one with the ground-state
            // stage of the other as long as a half fills the GPU (4-dot 256 envs 32 020 -> 33 160 env-steps/s, 8-dot 256 envs
            // 10 390 -> 10 560, 4-dot 1024 envs 38 140 -> 38 830; thirds: no further gain)
            const int half = (h->B + 1) / 2;
            if (h->nlanes >= 2 && cfg->env_chunk <= 0 && (size_t)half * batches_per_env >= 2048) chunk = half;
            else { chunk = h->B; h->nlanes = 1; }
        }
        gs_chunk = chunk;
    }
    // (tile descriptors carry the batch number in 20 bits)
    if ((size_t)gs_chunk * batches_per_env > ((size_t)1 << 20) - 1) {
        gs_chunk = (int)((((size_t)1 << 20) - 1) / batches_per_env);
        if (gs_chunk < 1) return qd_fail(h, QD_ERR_ARG, "resolution too large for the tile descriptors");
        if (!val && chunk > gs_chunk) chunk = gs_chunk;
    }
    h->chunk = chunk;
    h->gs_chunk = gs_chunk; h->gs_batches = (size_t)gs_chunk * batches_per_env;
    {
        hipDeviceProp_t prop;
        QD_HIP(hipGetDeviceProperties(&prop, device));
        h->cus = prop.multiProcessorCount;
    }
    QD_HIP(val ? qd_solve_grids<true>(h->cus, h->solve_grid) : qd_solve_grids<false>(h->cus, h->solve_grid));
    QD_HIP(h->params.reserve((size_t)h->B * h->L.size));
    QD_HIP(h->state.reserve((size_t)h->B * h->L.s_size));
    QD_HIP(h->steps.reserve((size_t)h->B));
    QD_HIP(h->zraw.reserve((size_t)h->B * h->C * h->P));
    QD_HIP(h->plohi.reserve(2 * (size_t)h->B));
    QD_HIP(h->ev_start.create(hipEventDisableTiming));
    for (int k = 0; k < h->nlanes; ++k) {
        QdLane& ln = h->lanes[k];
        QD_HIP(ln.recs.reserve(per_env_rec / sizeof(QdPixelRec) * (size_t)h->chunk));
        for (QdStream* q : {&ln.run, &ln.side, &ln.side2}) QD_HIP(q->create());
        for (QdEvent* ev : {&ln.ev_fork, &ln.ev_join, &ln.ev_join2, &ln.ev_done}) QD_HIP(ev->create(hipEventDisableTiming));
    }
    h->tel_words = (h->P + 63) / 64;
    if (cfg->noise_flags & QD_NOISE_SENSOR) {
        QD_HIP(h->tel.reserve((size_t)h->B * h->C * h->tel_words));
        QD_HIP(hipMemset(h->tel.p, 0, sizeof(unsigned long long) * (size_t)h->B * h->C * h->tel_words));
    }
    if ((cfg->flags & QD_FLAG_VALIDATE) || (cfg->noise_flags & QD_NOISE_LATCH))
        QD_HIP(h->occ.reserve((size_t)h->B * h->C * h->P * h->N));
    // the tile-shared search pays off where neighbouring pixels are close in voltage (fine grids) and needs >= 32
    // candidates valid across a tile (N >= 4); otherwise every pixel is searched on its own
    h->tile_search = (h->N >= 4 && h->R >= 32 && !(cfg->flags & QD_FLAG_PIXEL_SEARCH) && !h->full_m) ? 1 : 0;
    for (int k = 0; k < h->nlanes; ++k) {
        QD_HIP(h->lanes[k].slabs.reserve(h->gs_batches * qd_gs_slab_bytes(val)));
        QD_HIP(h->lanes[k].gtiles.reserve(16 + qd_gs_tile_off(QD_GS_NBIN, h->gs_batches)));
        if (h->wide.capw) QD_HIP(h->lanes[k].wide.reserve(h->gs_batches * qd_wide_bytes(h->wide.capw)));
    }
    if (cfg->flags & QD_FLAG_VALIDATE) {
        QD_HIP(h->tstats.reserve(32));
        QD_HIP(hipMemset(h->tstats.p, 0, sizeof(unsigned long long) * 32));
        QD_HIP(h->eig.reserve(2 * (size_t)h->B * h->C * h->P));
        QD_HIP(hipMemset(h->eig.p, 0, sizeof(double) * 2 * (size_t)h->B * h->C * h->P));
    }
    QD_HIP(hipMemset(h->params.p, 0, sizeof(double) * (size_t)h->B * h->L.size));
    QD_HIP(hipMemset(h->steps.p, 0, sizeof(int) * (size_t)h->B));
    QD_HIP(hipMemset(h->zraw.p, 0, sizeof(double) * (size_t)h->B * h->C * h->P));
    QD_HIP(hipMemset(h->plohi.p, 0, sizeof(double) * 2 * (size_t)h->B));
    // Kalman priors into every env's state block
    {
        const int N = h->N;
        double* host = (double*)calloc((size_t)h->B * h->L.s_size, sizeof(double));
        if (!host) return qd_fail(h, QD_ERR_NOMEM, "calloc");
        for (int e = 0; e < h->B; ++e) {
            double* st = host + (size_t)e * h->L.s_size;
            for (int i = 0; i < N + 1; ++i) st[h->L.s_vgm + i * (N + 1) + i] = -1.0;
            qd_kalman_priors(*cfg, N, st + h->L.s_kmean, st + h->L.s_kvar);
        }
        hipError_t e_ = hipMemcpy(h->state.p, host, sizeof(double) * (size_t)h->B * h->L.s_size, hipMemcpyHostToDevice);
        free(host);
        if (e_ != hipSuccess) return qd_fail(h, QD_ERR_HIP, "hipMemcpy(state)", e_);
    }
    snprintf(h->err, sizeof(h->err), "ok");
    return QD_OK;
}

extern "C" int qd_destroy(qd_handle* h) {
    if (!h) return QD_ERR_ARG;
    QdDeviceGuard guard_(h->device);
    free(h->vc_on);
    delete h;
    return QD_OK;
}

extern "C" int qd_bind_outputs(qd_handle* h, float* g, float* p, float* b, float* v) {
    if (!h) return QD_ERR_ARG;
    h->gimg = g; h->pimg = p; h->bimg = b; h->volt = v;
    return QD_OK;
}

extern "C" int qd_load_episodes(qd_handle* h, const int32_t* env_ids, int n, const double* params,
                                const double* state, int reset_kalman, void* stream) {
    if (!h || !env_ids || n < 0 || !params || !state) return qd_fail(h, QD_ERR_ARG, "qd_load_episodes: bad argument");
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    const QdLayout& L = h->L;
    const int N = h->N;
    const size_t pre = (size_t)L.s_kmean;                        // everything before the Kalman block
    if (n == 0) return QD_OK;
    for (int k = 0; k < n; ++k)
        if (env_ids[k] < 0 || env_ids[k] >= h->B) return qd_fail(h, QD_ERR_ARG, "qd_load_episodes: env id out of range");
    bool contiguous = true;
    for (int k = 1; k < n && contiguous; ++k) contiguous = env_ids[k] == env_ids[0] + k;
    // The caller's (pageable) buffers are copied into a pinned staging slot and uploaded from there; an event per slot
    // says when the stream has consumed it, so the call returns at once instead of draining the stream -- the host goes on
    // to queue the resets' observation and the next step while the GPU is still busy with the previous one.
    const size_t prow = (size_t)L.size, srow = (size_t)L.s_size;
    const size_t need = (size_t)n * (prow + srow);
    QD_HIP(h->stage.room(need < (size_t)64 * (prow + srow) ? (size_t)64 * (prow + srow) : need));   // (64 rows at the least)
    int slot;
    QD_HIP(h->stage.take(slot));
    double* sp = h->stage.slot[slot].p;
    double* ss = sp + (size_t)n * prow;
    memcpy(sp, params, sizeof(double) * (size_t)n * prow);
    for (int k = 0; k < n; ++k) h->vc_on[(size_t)env_ids[k]] = params[(size_t)k * prow + L.scal + 4] != 0.0 ? 1 : 0;
    memcpy(ss, state, sizeof(double) * (size_t)n * srow);
    // the state rows uploaded are the first `pre` doubles, or the whole row with fresh Kalman priors
    size_t width = pre;
    if (reset_kalman) {
        double km[QD_MAXN * QD_MAXN], kv[QD_MAXN * QD_MAXN];
        qd_kalman_priors(h->cfg, N, km, kv);
        for (int k = 0; k < n; ++k) {
            double* row = ss + (size_t)k * srow;
            memcpy(row + L.s_kmean, km, sizeof(double) * N * N);
            memcpy(row + L.s_kvar, kv, sizeof(double) * N * N);
        }
        width = (size_t)L.s_kvar + (size_t)N * N;
    }
    hipError_t er = hipSuccess;
    if (contiguous) {
        const int e0 = env_ids[0];
        er = hipMemcpyAsync(h->params.p + (size_t)e0 * prow, sp, sizeof(double) * prow * n, hipMemcpyHostToDevice, s);
        if (er == hipSuccess)
            er = hipMemcpy2DAsync(h->state.p + (size_t)e0 * srow, sizeof(double) * srow, ss,
                                  sizeof(double) * srow, sizeof(double) * width, n, hipMemcpyHostToDevice, s);
        if (er == hipSuccess) er = hipMemsetAsync(h->steps.p + e0, 0, sizeof(int) * n, s);
    } else {
        for (int k = 0; k < n && er == hipSuccess; ++k) {
            const int e = env_ids[k];
            er = hipMemcpyAsync(h->params.p + (size_t)e * prow, sp + (size_t)k * prow, sizeof(double) * prow, hipMemcpyHostToDevice, s);
            if (er == hipSuccess)
                er = hipMemcpyAsync(h->state.p + (size_t)e * srow, ss + (size_t)k * srow, sizeof(double) * width, hipMemcpyHostToDevice, s);
            if (er == hipSuccess) er = hipMemsetAsync(h->steps.p + e, 0, sizeof(int), s);
        }
    }
    if (er == hipSuccess) er = hipEventRecord(h->stage.ev[slot].e, s);
    if (er != hipSuccess) return qd_fail(h, QD_ERR_HIP, "qd_load_episodes: copy", er);
    h->stage.busy[slot] = true;
    return QD_OK;
}

extern "C" int qd_apply_actions(qd_handle* h, const float* actions, double* rewards, uint8_t* truncated, void* stream) {
    if (!h || !actions) return qd_fail(h, QD_ERR_ARG, "qd_apply_actions: bad argument");
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    const qd_config& c = h->cfg;
    QdRewardCfg rc{c.gate_ramp_start, c.gate_quadratic_start, c.barrier_ramp_start, c.max_steps,
                   c.use_deltas, c.sparse_reward, c.gate_curve_type, c.delta_max, c.gate_curve_exponent,
                   c.plunger_radius, c.outer_plunger_radius, c.outer_plunger_reward_max, c.barrier_radius};
    const int blk = 64, grd = (h->B + blk - 1) / blk;
    QD_DISPATCH_N(h->N, qd_k_actions<NN><<<dim3(grd), dim3(blk), 0, s>>>(h->B, h->params.p,
                                            h->state.p, h->steps.p, actions, rewards, truncated, rc));
    QD_HIP(hipGetLastError());
    return QD_OK;
}

static int qd_cand_blocks(int R) {
    const int tiles = ((R + 7) / 8) * ((R + 7) / 8), per_block = QD_CAND_BLOCK / 64;
    return (tiles + per_block - 1) / per_block;
}

static QdNoiseCfg qd_noise_cfg(const qd_handle* h, const QdEnvBufs& b) {
    QdNoiseCfg nz;
    nz.flags = b.noise_flags;
    nz.seed = (uint32_t)(h->cfg.rng_seed ^ (h->cfg.rng_seed >> 32));
    nz.env_off = b.env_off;
    nz.ser_lo = (uint32_t)b.serial; nz.ser_hi = (uint32_t)(b.serial >> 32);
    nz.tel = b.tel; nz.tel_words = b.tel_words;
    return nz;
}

// The stages of one launch chunk, in pipeline order; the timing hooks launch them one by one.
enum {
    QD_ST_TILE = 1, QD_ST_REDO = 2, QD_ST_STRUCTURE = 4, QD_ST_SOLVE = 8, QD_ST_SELECT = 16,
    QD_ST_SEARCH = QD_ST_TILE | QD_ST_REDO,
    QD_ST_GROUND = QD_ST_STRUCTURE | QD_ST_SOLVE | QD_ST_SELECT,
    QD_ST_ALL = QD_ST_SEARCH | QD_ST_GROUND
};

// the stages this handle has: the full space has no candidate search, and without the tile search the redo pass is the
// whole (per-pixel) search
static int qd_stages(const qd_handle* h) {
    return h->full_m ? QD_ST_GROUND : (h->tile_search ? QD_ST_ALL : QD_ST_ALL & ~QD_ST_TILE);
}

template <int BIN>
static hipError_t qd_launch_solve(const qd_handle* h, const QdLane& ln, hipStream_t s) {   // s: the stream this size class runs on
    const dim3 grid((unsigned)h->solve_grid[BIN]);
    QD_DISPATCH_BOOL(qd_validate(h), VAL,
                     qd_k_gs_solve<BIN, VAL><<<grid, dim3(256), 0, s>>>(ln.slabs.p, ln.gtiles.p, ln.gtiles.p + 16, h->gs_batches, h->tstats.p));
    return hipGetLastError();
}

// a11-a13 + a15 for the envs at list positions [base, base + cnt): structure -> solve per size class -> select (those of
// them in `st`), in launches of at most gs_chunk envs (the slabs in flight)
static int qd_launch_ground(const qd_handle* h, const QdEnvBufs& b, const QdLane& ln, const int32_t* env_ids, int base, int cnt,
                            hipStream_t s, int st) {
    const int nb = (b.P + h->ppb - 1) / h->ppb, C = b.channels;
    // blocks per launch: what the slabs hold (the handle's own geometry: gs_chunk)
    const int per = (int)(h->gs_batches / ((size_t)C * nb));
    unsigned* tilelist = ln.gtiles.p + 16;
    const bool val = qd_validate(h);
    QdWide wide = h->wide; wide.buf = ln.wide.p;
    // records: product mode keeps one launch chunk (slot = position in the chunk), validate mode all envs (position in the list)
    const int rec0 = val ? base : 0;
    for (int off = 0; off < cnt; off += per) {
        const int n = cnt - off < per ? cnt - off : per;
        const QdGsGeom g{n, C, b.P, nb};
        const unsigned batches = (unsigned)((size_t)n * C * nb);
        if (st & QD_ST_STRUCTURE) {
            QD_HIP(hipMemsetAsync(ln.gtiles.p, 0, sizeof(unsigned) * 16, s));
            if (h->full_m) {
                // (shapes without a sector above 32 states have M <= 128: the kernel without the wide class, 2 states per lane)
#define QD_DISPATCH_FULL(...)                                                                                  \
                if (!wide.capw && h->full_spl == 2) { constexpr int SPL = 2; constexpr bool WIDE = false; __VA_ARGS__; }  \
                else if (h->full_spl == 2) { constexpr int SPL = 2; constexpr bool WIDE = true; __VA_ARGS__; }            \
                else if (h->full_spl == 4) { constexpr int SPL = 4; constexpr bool WIDE = true; __VA_ARGS__; }            \
                else { constexpr int SPL = 8; constexpr bool WIDE = true; __VA_ARGS__; }
                QD_DISPATCH_BOOL(val, VAL, QD_DISPATCH_FULL(QD_DISPATCH_N(h->N,
                    qd_k_full_structure<NN, VAL, SPL, WIDE><<<dim3(batches), dim3(64 * QdFullWpb<SPL>::v), 0, s>>>(env_ids, base + off,
                        rec0 + off, g, h->ppb, b.R, b.params, b.state, b.noise_flags, h->ftab.p, ln.recs.p, ln.slabs.p, ln.gtiles.p, tilelist,
                        h->gs_batches, wide))));
#undef QD_DISPATCH_FULL
            } else {
                // (small launches: 16 waves per batch instead of 4, see the kernel)
                QD_DISPATCH_BOOL(val, VAL, QD_DISPATCH_BOOL(batches < (unsigned)h->cus, SMALL, QD_DISPATCH_N(h->N,
                    qd_k_gs_structure<NN, VAL, (SMALL ? 16 : 4)><<<dim3(batches), dim3(64 * (SMALL ? 16 : 4)), 0, s>>>(env_ids, base + off,
                        rec0 + off, g, b.R, b.params, ln.recs.p, b.state, b.noise_flags, ln.slabs.p, ln.gtiles.p, tilelist, h->gs_batches,
                        h->kept, (h->cfg.flags & QD_FLAG_GS_GERSHGORIN_ZERO) ? 1 : 0))));
            }
            QD_HIP(hipGetLastError());
        }
        if (st & QD_ST_SOLVE) {
            // A hop component lies in one total-charge sector of the kept states: at most 4 states for 2 dots (16 candidates), 12 for
            // 3 dots; the launches of size classes that cannot occur are skipped.  From 4 dots on the memory solver of the rare
            // 13..32-state blocks (one long latency chain: 0.4 ms for 8 envs, 0.9 ms for 180) and the wide register solvers go on
            // two side streams, whatever the batch.  Nor can a component hold more than the K kept states (K = 1: no task at all).
            // In the full space a component is at most a sector.
            int max_bin = h->N == 2 ? qd_gs_bin(4) : (h->N == 3 ? qd_gs_bin(12) : QD_GS_NBIN - 1);
            if (h->full_m) {
                int M = 0, maxsec = 0;
                qd_full_sizes(h->N, h->full_m, M, maxsec);
                max_bin = qd_gs_bin(maxsec < QD_K ? maxsec : QD_K);
            } else if (h->kept < 2) max_bin = -1;
            else if (qd_gs_bin(h->kept) < max_bin) max_bin = qd_gs_bin(h->kept);
            const bool forked = max_bin >= 9;            // (8-dot, 4 envs: 1 760 -> 2 520 env-steps/s, 8 envs 3 390 -> 3 590; 2 and 3 dots have no memory-solver launch to hide)
            hipStream_t s9 = forked ? ln.side.s : s, s48 = forked ? ln.side2.s : s;
            if (forked) {
                QD_HIP(hipEventRecord(ln.ev_fork.e, s));
                QD_HIP(hipStreamWaitEvent(ln.side.s, ln.ev_fork.e, 0));
                QD_HIP(hipStreamWaitEvent(ln.side2.s, ln.ev_fork.e, 0));
            }
            if (wide.capw) {                               // the wide class first: its tasks are the longest
                const size_t slots = (size_t)batches * wide.capw, full = (size_t)h->cus * 4;
                const dim3 wgrid((unsigned)(slots < full ? slots : full));
                QD_DISPATCH_BOOL(val, VAL, qd_k_full_solve_wide<VAL><<<wgrid, dim3(64), 0, s>>>(ln.slabs.p, wide, batches, h->tstats.p));
                QD_HIP(hipGetLastError());
            }
            if (max_bin >= 9) QD_HIP(qd_launch_solve<9>(h, ln, s9));
            if (forked) QD_HIP(hipEventRecord(ln.ev_join.e, ln.side.s));
            if (max_bin >= 8) QD_HIP(qd_launch_solve<8>(h, ln, s48));
            if (max_bin >= 7) QD_HIP(qd_launch_solve<7>(h, ln, s48));
            if (max_bin >= 6) QD_HIP(qd_launch_solve<6>(h, ln, s48));
            if (max_bin >= 5) QD_HIP(qd_launch_solve<5>(h, ln, s48));
            if (max_bin >= 4) QD_HIP(qd_launch_solve<4>(h, ln, s48));
            if (forked) QD_HIP(hipEventRecord(ln.ev_join2.e, ln.side2.s));
            if (max_bin >= 0) QD_HIP(qd_launch_solve<0>(h, ln, s));
            if (max_bin >= 1) QD_HIP(qd_launch_solve<1>(h, ln, s));
            if (max_bin >= 2) QD_HIP(qd_launch_solve<2>(h, ln, s));
            if (max_bin >= 3) QD_HIP(qd_launch_solve<3>(h, ln, s));
            if (forked) {
                QD_HIP(hipStreamWaitEvent(s, ln.ev_join.e, 0));
                QD_HIP(hipStreamWaitEvent(s, ln.ev_join2.e, 0));
            }
        }
        if (st & QD_ST_SELECT) {
            if (h->full_m) {
                const unsigned blk = (unsigned)((h->ppb + 63) / 64 * 64);
                QD_DISPATCH_BOOL(val, VAL, QD_DISPATCH_BOOL(wide.capw != 0, WIDE, QD_DISPATCH_N(h->N,
                    qd_k_full_select<NN, VAL, WIDE><<<dim3(batches), dim3(blk), 0, s>>>(env_ids, base + off, rec0 + off, g, h->ppb,
                        b.params, ln.recs.p, b.zraw, b.occ, b.state, b.noise_flags, b.eig, h->ftab.p, ln.slabs.p, wide))));
            } else {
                QD_DISPATCH_BOOL(val, VAL, QD_DISPATCH_N(h->N, QD_DISPATCH_KC(h->kc,
                    qd_k_gs_select<NN, VAL, KK><<<dim3(batches), dim3(QD_GS_BLOCK), 0, s>>>(env_ids, base + off, rec0 + off, g, b.R,
                        b.params, ln.recs.p, b.zraw, b.occ, b.state, b.noise_flags, b.eig, ln.slabs.p))));
            }
            QD_HIP(hipGetLastError());
        }
    }
    return QD_OK;
}

// (not QD_DISPATCH_N: qd_k_tile exists from 4 dots on)
#define QD_DISPATCH_TILE(N_, ...)                                                 \
    switch (N_) {                                                                 \
        case 4: { constexpr int NN = 4; __VA_ARGS__; } break;                            \
        case 5: { constexpr int NN = 5; __VA_ARGS__; } break;                            \
        case 6: { constexpr int NN = 6; __VA_ARGS__; } break;                            \
        case 7: { constexpr int NN = 7; __VA_ARGS__; } break;                            \
        case 8: { constexpr int NN = 8; __VA_ARGS__; } break;                            \
        default: return qd_fail(h, QD_ERR_ARG, "tile kernels need n_dot in 4..8");      \
    }

// validate mode keeps the records' kept states in the reference order; K < KC needs it too, the ground-state stage takes the first K
static int qd_sorted_records(const qd_handle* h) { return (qd_validate(h) || h->kept != h->kc) ? 1 : 0; }

// a5/a8-a10 by the per-pixel search on `cnt` blocks of `b`.  tiled: the exact redo pass, only on the pixels whose record
// asks for it (behind the tile search, or behind a front end that filled the records itself); else every pixel.
// (in both search kernels noise_flags reaches qd_radial_replaced alone, false without the radial bit, which qd_scan2d and
// qd_scan_affine refuse)
static int qd_launch_candidates(const qd_handle* h, const QdEnvBufs& b, const QdLane& ln, const int32_t* env_ids, int base, int cnt,
                                hipStream_t s, bool tiled) {
    const size_t shm = (size_t)h->kc * QD_CAND_BLOCK * (sizeof(double) + sizeof(uint16_t));
    if (b.front == QD_FRONT_LINE && !tiled) return qd_fail(h, QD_ERR_STATE, "a line's records have no front end inside the search");
    const dim3 grid(qd_cand_blocks(b.R), b.channels, cnt);
    QD_DISPATCH_FRONT(b.front, QD_DISPATCH_BOOL(tiled, TILED, QD_DISPATCH_N(h->N, QD_DISPATCH_KC(h->kc,
        qd_k_candidates<NN, TILED, KK, FE><<<grid, dim3(QD_CAND_BLOCK), shm, s>>>(env_ids, base, b.R, b.params, b.state, ln.recs.p,
                                                                                  qd_sorted_records(h), b.noise_flags)))));
    QD_HIP(hipGetLastError());
    return QD_OK;
}

// The closed regime's place in a stateless query: behind a front kernel that left `cnt` slots of SP records in hand-over form,
// and instead of the redo pass -- centre and sector search of every live record at the total charge qslot[slot] (device).
static int qd_launch_closed(const qd_handle* h, const QdEnvBufs& b, const QdLane& ln, int SP, const int32_t* qslot, int cnt, hipStream_t s) {
    const size_t shm = (size_t)h->kc * QD_CLOSED_BLOCK * (sizeof(double) + sizeof(uint16_t));
    const dim3 grid((unsigned)((SP + QD_CLOSED_BLOCK - 1) / QD_CLOSED_BLOCK), cnt);
    QD_DISPATCH_N(h->N, QD_DISPATCH_KC(h->kc,
        qd_k_closed<NN, KK><<<grid, dim3(QD_CLOSED_BLOCK), shm, s>>>(SP, b.params, qslot, ln.recs.p)));
    QD_HIP(hipGetLastError());
    return QD_OK;
}

// a5-a13 for `cnt` envs starting at list position `base`: those of the stages in `st` that the handle has (qd_stages) --
// tile search + exact redo pass or the per-pixel search alone, then the ground-state kernels.  On the blocks of a scan
// (b.front) slot k renders ONE image over the axes in its state block copy instead of the env's C channel images.
static int qd_launch_csd(const qd_handle* h, const QdEnvBufs& b, const QdLane& ln, const int32_t* env_ids, int base, int cnt,
                         hipStream_t s, int st) {
    st &= qd_stages(h);
    if (st & QD_ST_TILE) {
        const int tiles = ((b.R + 7) / 8) * ((b.R + 7) / 8);
        QD_DISPATCH_FRONT(b.front, QD_DISPATCH_TILE(h->N, QD_DISPATCH_KC(h->kc,
            qd_k_tile<NN, KK, FE><<<dim3(tiles, b.channels, cnt), dim3(64), 0, s>>>(env_ids, base, b.R, b.params, b.state, ln.recs.p,
                                                                                    qd_sorted_records(h), b.noise_flags, h->tstats.p))));
        QD_HIP(hipGetLastError());
    }
    if (st & QD_ST_REDO)
        if (int rc = qd_launch_candidates(h, b, ln, env_ids, base, cnt, s, h->tile_search != 0)) return rc;
    if (st & QD_ST_GROUND) return qd_launch_ground(h, b, ln, env_ids, base, cnt, s, st);
    return QD_OK;
}

// a16 on the signal of `n` envs (their list `ids`, or 0..n-1), in place
static int qd_launch_sensor(const qd_handle* h, const QdEnvBufs& b, const int32_t* ids, int n, hipStream_t s) {
    const dim3 g3((b.P + 255) / 256, b.channels, n);
    QD_DISPATCH_BOOL(b.channels == 1, ONE, QD_DISPATCH_N(h->N,
        qd_k_sensor<NN, (ONE ? 1 : NN - 1)><<<g3, dim3(256), 0, s>>>(ids, b.R, b.params, b.state, b.zraw, qd_noise_cfg(h, b))));
    QD_HIP(hipGetLastError());
    return QD_OK;
}

// a17: one block per row of `count` values; the keys stay in registers where a block can hold them
// (the caller checks hipGetLastError)
static void qd_launch_percentile(const int32_t* ids, unsigned blocks, long count, const double* z, double* plohi, hipStream_t s) {
    QD_DISPATCH_BOOL(count <= (long)QD_PCT_KPT * QD_PCT_BLOCK, CACHED,
                     qd_k_percentile<CACHED><<<dim3(blocks), dim3(QD_PCT_BLOCK), 0, s>>>(ids, count, z, plohi));
}

extern "C" int qd_observe(qd_handle* h, const int32_t* env_ids, int n, void* stream) {
    if (!h || n < 0) return qd_fail(h, QD_ERR_ARG, "qd_observe: bad argument");
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    if (!env_ids) n = h->B;
    if (n == 0) return QD_OK;
    if (n > h->B) return qd_fail(h, QD_ERR_ARG, "qd_observe: n > batch");
    const QdLayout& L = h->L;
    h->obs_serial++;
    const QdEnvBufs b = qd_env_bufs(h);
    if (b.noise_flags & QD_NOISE_SENSOR) {
        const int nt = n * h->C;
        qd_k_telegraph<<<dim3((nt + 63) / 64), dim3(64), 0, s>>>(env_ids, n, h->C, h->P, L.size, L.noise, b.params, b.tel, qd_noise_cfg(h, b));
        QD_HIP(hipGetLastError());
    }
    if (h->nlanes == 1 || n <= h->chunk) {
        for (int base = 0; base < n; base += h->chunk) {
            const int cnt = (n - base < h->chunk) ? n - base : h->chunk;
            int rc = qd_launch_csd(h, b, h->lanes[0], env_ids, base, cnt, s, QD_ST_ALL);
            if (rc) return rc;
        }
    } else {
        // consecutive chunks go round the lanes (own scratch, own stream): search and ground state of different chunks overlap
        QD_HIP(hipEventRecord(h->ev_start.e, s));
        for (int k = 0; k < h->nlanes; ++k) QD_HIP(hipStreamWaitEvent(h->lanes[k].run.s, h->ev_start.e, 0));
        // (measured: 2 lanes 11 520 env-steps/s, 3 lanes 10 920, 4 lanes 11 350; starting the second lane half a chunk out of
        // phase: 11 310 against 11 620 in the same run)
        int i = 0;
        for (int base = 0; base < n; base += h->chunk, ++i) {
            const int cnt = (n - base < h->chunk) ? n - base : h->chunk;
            const QdLane& ln = h->lanes[i % h->nlanes];
            int rc = qd_launch_csd(h, b, ln, env_ids, base, cnt, ln.run.s, QD_ST_ALL);
            if (rc) return rc;
        }
        for (int k = 0; k < h->nlanes; ++k) {
            QD_HIP(hipEventRecord(h->lanes[k].ev_done.e, h->lanes[k].run.s));
            QD_HIP(hipStreamWaitEvent(s, h->lanes[k].ev_done.e, 0));
        }
    }
    if (b.noise_flags & QD_NOISE_LATCH) {
        const int nt = n * h->C;
        QD_DISPATCH_N(h->N, qd_k_latch<NN><<<dim3((nt + 63) / 64), dim3(64), 0, s>>>(env_ids, n, h->R, b.params, b.state, b.occ, b.zraw, qd_noise_cfg(h, b)));
        QD_HIP(hipGetLastError());
    }
    if (int rc = qd_launch_sensor(h, b, env_ids, n, s)) return rc;
    qd_launch_percentile(env_ids, (unsigned)n, (long)h->C * h->P, b.zraw, b.plohi, s);
    QD_HIP(hipGetLastError());
    if (h->gimg || h->pimg || h->bimg || h->volt) {
        dim3 g4((h->P + 255) / 256, n);
        QD_DISPATCH_N(h->N, qd_k_write_obs<NN><<<g4, dim3(256), 0, s>>>(env_ids, h->R, h->params.p,
                                                h->state.p, h->zraw.p, h->plohi.p, h->gimg, h->pimg, h->bimg, h->volt));
        QD_HIP(hipGetLastError());
    }
    return QD_OK;
}

extern "C" int qd_update_capacitance(qd_handle* h, const int32_t* env_ids, int n, const float* values,
                                     const float* log_vars, int recompute_gt, void* stream) {
    if (!h || n < 0) return qd_fail(h, QD_ERR_ARG, "qd_update_capacitance: bad argument");
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    if (!env_ids) n = h->B;
    if (n == 0) return QD_OK;
    QdKalmanCfg kc{h->cfg.kalman_variance_threshold, h->cfg.kalman_process_noise, h->cfg.update_method == QD_UPDATE_DIRECT ? 1 : 0,
                   h->cfg.cnn_outputs};
    const int blk = QD_UPD_BLOCK, grd = n;                           // one wave per env
    QD_DISPATCH_N(h->N, qd_k_update<NN><<<dim3(grd), dim3(blk), 0, s>>>(env_ids, n, h->params.p,
                                            h->state.p, values, log_vars, recompute_gt, kc));
    QD_HIP(hipGetLastError());
    return QD_OK;
}

extern "C" int qd_step(qd_handle* h, const float* actions, const float* values, const float* log_vars,
                       double* rewards, uint8_t* truncated, void* stream) {
    int rc = qd_apply_actions(h, actions, rewards, truncated, stream);
    if (rc) return rc;
    rc = qd_observe(h, nullptr, 0, stream);
    if (rc) return rc;
    return qd_update_capacitance(h, nullptr, 0, values, log_vars, 1, stream);
}

extern "C" int qd_snapshot(qd_handle* h, const int32_t* env_ids, int n, float* global_dst, float* plunger_dst,
                           float* barrier_dst, float* voltages_dst, double* state_dst, double* params_dst,
                           int32_t* steps_dst, void* stream) {
    if (!h || n < 0) return qd_fail(h, QD_ERR_ARG, "qd_snapshot: bad argument");
    if (n == 0) return QD_OK;
    if (n > h->B) return qd_fail(h, QD_ERR_ARG, "qd_snapshot: n > batch");
    if (!env_ids) return qd_fail(h, QD_ERR_ARG, "qd_snapshot: env_ids_dev is NULL");
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    const long long P = h->P, N = h->N, C = h->C;
    const struct { const void* src; void* dst; long long bytes; } want[QD_SNAP_SEGS] = {
        {h->gimg, global_dst, (long long)sizeof(float) * P * C},
        {h->pimg, plunger_dst, (long long)sizeof(float) * N * P * 2},
        {h->bimg, barrier_dst, (long long)sizeof(float) * C * P},
        {h->volt, voltages_dst, (long long)sizeof(float) * (2 * N - 1)},
        {h->state.p, state_dst, (long long)sizeof(double) * h->L.s_size},
        {h->params.p, params_dst, (long long)sizeof(double) * h->L.size},
        {h->steps.p, steps_dst, (long long)sizeof(int32_t)}};
    QdSnapArgs a{};
    int k = 0;
    for (const auto& w : want)                            // unbound outputs and NULL destinations are skipped
        if (w.src && w.dst) a.seg[k++] = QdSnapSeg{(const unsigned char*)w.src, (unsigned char*)w.dst, w.bytes};
    if (k == 0) return QD_OK;
    qd_k_snapshot<<<dim3(n, k), dim3(QD_SNAP_BLOCK), 0, s>>>(env_ids, h->B, a);
    QD_HIP(hipGetLastError());
    return QD_OK;
}

// The option values of a stateless query: qd_probe_opts gives the first four, the scans' option structs all of them.
struct QdQueryOpts {
    int noise_flags; unsigned long long serial; long long stream_base;
    bool occ;                               // the slots carry occupations: the caller takes them, or a thermal kernel writes them
    double* occ_dst; const double *vgm, *gamma; int frame;
};

// The slots of a stateless query: `channels` images of side x side records each, of which the percentile kernel reads
// `count` values per slot; `slots` of them in flight; `front` fills the records.
struct QdSlotGeom { int channels, side; long count; int slots; QdFront front; };

// The stateless queries: `nq` of them in launches of g.slots slots on the blocks of `set`.  Per launch: gather(base, cnt, bufs)
// copies the envs' blocks into the slots and applies the queries; then the stages of an observation in qd_observe's order --
// telegraph words, solve(base, cnt, bufs): search and ground (or thermal) state, latch(cnt, bufs), sensor, pack(cnt, bufs): the rows
// of g.count values that the percentile kernel reads, percentiles -- on the slots alone, without eigenvalues; occupations,
// telegraph words and noise only as asked for, keyed by the caller's serial and stream base; write(base, cnt, bufs, rows)
// hands the results out.  gather, pack and write only launch, the runner checks; solve and latch return a status.  Nothing
// of the envs is written.
template <class Gather, class Solve, class Latch, class Pack, class Write>
static int qd_run_queries(qd_handle* h, QdScratchSet& set, const QdSlotGeom& g, const QdQueryOpts& o, int nq, hipStream_t s,
                          Gather gather, Solve solve, Latch latch, Pack pack, Write write) {
    const bool want_occ = (o.noise_flags & QD_NOISE_LATCH) || o.occ, want_tel = (o.noise_flags & QD_NOISE_SENSOR) != 0;
    const int pc = g.slots, tel_words = (g.side * g.side + 63) / 64;     // (a chain of side^2 states per channel image)
    const size_t CP = (size_t)g.channels * g.side * g.side;
    QD_HIP(set.reserve(h->L, CP, (size_t)pc, 2, want_occ ? CP * h->N : 0, want_tel ? (size_t)g.channels * tel_words : 0));
    QdEnvBufs b = set.view(g.channels, g.side, g.front);
    b.occ = want_occ ? set.occ.p : nullptr;
    b.noise_flags = o.noise_flags;
    if (want_tel) { b.tel = set.tel.p; b.tel_words = tel_words; }
    b.serial = o.serial;
    for (int base = 0; base < nq; base += pc) {
        const int cnt = nq - base < pc ? nq - base : pc;
        b.env_off = (uint32_t)(o.stream_base + base);        // slot k of the launch draws as global env stream_base + base + k
        gather(base, cnt, b);
        QD_HIP(hipGetLastError());
        if (want_tel) {
            const int nt = cnt * g.channels;
            qd_k_telegraph<<<dim3((nt + 63) / 64), dim3(64), 0, s>>>(nullptr, cnt, g.channels, b.P, h->L.size, h->L.noise, b.params, b.tel,
                                                                     qd_noise_cfg(h, b));
            QD_HIP(hipGetLastError());
        }
        if (int rc = solve(base, cnt, b)) return rc;
        if (o.noise_flags & QD_NOISE_LATCH) {
            if (int rc = latch(cnt, b)) return rc;
            QD_HIP(hipGetLastError());
        }
        if (int rc = qd_launch_sensor(h, b, nullptr, cnt, s)) return rc;
        const double* rows = pack(cnt, b);
        qd_launch_percentile(nullptr, (unsigned)cnt, g.count, rows, b.plohi, s);
        QD_HIP(hipGetLastError());
        write(base, cnt, b, rows);
        QD_HIP(hipGetLastError());
    }
    return QD_OK;
}

// The queries that render images of the handle's own size (qd_probe_ex, qd_scan2d, qd_scan_affine): h->chunk slots in flight
// (lane 0's scratch), each `channels` images filled by `front` inside the search; the latching walk by rows; no pack.
template <class Gather, class Write>
static int qd_run_queries(qd_handle* h, QdScratchSet& set, int channels, QdFront front, const QdQueryOpts& o, int nq, hipStream_t s,
                          Gather gather, Write write) {
    return qd_run_queries(h, set, QdSlotGeom{channels, h->R, (long)channels * h->P, h->chunk, front}, o, nq, s, gather,
        [&](int, int cnt, const QdEnvBufs& b) { return qd_launch_csd(h, b, h->lanes[0], nullptr, 0, cnt, s, QD_ST_ALL); },
        [&](int cnt, const QdEnvBufs& b) {
#ifdef QD_PROBE_SERIAL_LATCH        // (measurement only, DESIGN.md 7: probes take the one-thread walk of qd_observe on their buffers)
            if (front == QD_FRONT_ENV) {
                QD_DISPATCH_N(h->N, qd_k_latch<NN><<<dim3((cnt * channels + 63) / 64), dim3(64), 0, s>>>(nullptr, cnt, h->R, b.params, b.state,
                                                                                                       b.occ, b.zraw, qd_noise_cfg(h, b)));
                return (int)QD_OK;
            }
#endif
            const long rows = (long)cnt * channels * b.R;
            const dim3 grid((unsigned)((rows + QD_LATCH_ROWS_BLOCK - 1) / QD_LATCH_ROWS_BLOCK));
            QD_DISPATCH_BOOL(channels == 1, ONE, QD_DISPATCH_N(h->N,
                qd_k_latch_rows<NN, (ONE ? 1 : NN - 1)><<<grid, dim3(QD_LATCH_ROWS_BLOCK), 0, s>>>(cnt, b.R, b.params, b.state, b.occ,
                                                                                                   b.zraw, qd_noise_cfg(h, b))));
            return (int)QD_OK;
        },
        [](int, const QdEnvBufs& b) { return (const double*)b.zraw; },
        [&](int base, int cnt, const QdEnvBufs& b, const double*) { write(base, cnt, b); });
}

extern "C" int qd_probe_ex(qd_handle* h, const int32_t* env_of_query, int nq, const double* gate_v, const double* barrier_v,
                           const double* sensor_v, const double* window, double* raw_dst, float* image_dst, double* plohi_dst,
                           const qd_probe_opts* opts, void* stream) {
    if (!h) return QD_ERR_ARG;
    if (nq < 0) return qd_fail(h, QD_ERR_ARG, "qd_probe: nq < 0");
    if (!env_of_query) return qd_fail(h, QD_ERR_ARG, "qd_probe: env_of_query_dev is NULL");
    if (!gate_v || !barrier_v) return qd_fail(h, QD_ERR_ARG, "qd_probe: gate_v_dev or barrier_v_dev is NULL");
    if (int rc = qd_check_struct_size(h, opts, sizeof(qd_probe_opts), "qd_probe_ex: opts->struct_size is not sizeof(qd_probe_opts)")) return rc;
    if (opts && (opts->noise_flags & ~(QD_NOISE_SENSOR | QD_NOISE_RADIAL | QD_NOISE_LATCH)))
        return qd_fail(h, QD_ERR_ARG, "qd_probe_ex: opts->noise_flags has a bit that is no QD_NOISE_* stage");
    if (h->cfg.flags & QD_FLAG_VALIDATE)
        return qd_fail(h, QD_ERR_STATE, "qd_probe: a QD_FLAG_VALIDATE handle keeps records, occupations and eigenvalues of its "
                                        "B envs' last observe and renders no probes; use a handle without the flag");
    if (nq == 0) return QD_OK;
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    const QdQueryOpts o = opts ? QdQueryOpts{opts->noise_flags, opts->serial, opts->stream_base, opts->occ_dst != nullptr} : QdQueryOpts{};
    double* const occ_dst = opts ? opts->occ_dst : nullptr;
    const QdProbeQuery Q{env_of_query, gate_v, barrier_v, sensor_v, window};
    return qd_run_queries(h, h->probe, h->C, QD_FRONT_ENV, o, nq, s,
        [&](int base, int cnt, const QdEnvBufs& pb) {
            qd_k_probe_gather<<<dim3(cnt), dim3(QD_PROBE_BLOCK), 0, s>>>(Q, base, h->B, h->N, h->params.p, h->state.p, pb.params, pb.state);
        },
        [&](int base, int cnt, const QdEnvBufs& pb) {
            if (raw_dst || image_dst || plohi_dst)
                qd_k_probe_write<<<dim3((h->P + 255) / 256, cnt), dim3(256), 0, s>>>(env_of_query, base, h->B, h->C, h->P, pb.zraw, pb.plohi,
                                                                                     raw_dst, image_dst, plohi_dst);
            if (occ_dst)
                qd_k_probe_write_occ<<<dim3((h->P * h->N + 255) / 256, h->C, cnt), dim3(256), 0, s>>>(env_of_query, base, h->B, h->N, h->P,
                                                                                                      pb.params, pb.state, o.noise_flags, pb.occ, occ_dst);
        });
}

extern "C" int qd_probe(qd_handle* h, const int32_t* env_of_query, int nq, const double* gate_v, const double* barrier_v,
                        const double* sensor_v, const double* window, double* raw_dst, float* image_dst, double* plohi_dst,
                        void* stream) {
    return qd_probe_ex(h, env_of_query, nq, gate_v, barrier_v, sensor_v, window, raw_dst, image_dst, plohi_dst, nullptr, stream);
}

// qdsim.h keeps one option struct per scan family; they are one layout, and the library reads them all as a qd_scan_opts
template <class T>
constexpr bool qd_is_scan_opts() {
    return sizeof(T) == sizeof(qd_scan_opts) && offsetof(T, struct_size) == offsetof(qd_scan_opts, struct_size) &&
           offsetof(T, frame) == offsetof(qd_scan_opts, frame) && offsetof(T, noise_flags) == offsetof(qd_scan_opts, noise_flags) &&
           offsetof(T, reserved) == offsetof(qd_scan_opts, reserved) && offsetof(T, serial) == offsetof(qd_scan_opts, serial) &&
           offsetof(T, stream_base) == offsetof(qd_scan_opts, stream_base) && offsetof(T, vgm_dev) == offsetof(qd_scan_opts, vgm_dev) &&
           offsetof(T, gamma_dev) == offsetof(qd_scan_opts, gamma_dev) && offsetof(T, occ_dst) == offsetof(qd_scan_opts, occ_dst);
}
static_assert(qd_is_scan_opts<qd_scan_affine_opts>() && qd_is_scan_opts<qd_scan1d_opts>() && qd_is_scan_opts<qd_scan_grid_opts>(),
              "the scans' option structs are one layout");
static_assert(QD_SCAN_VIRTUAL == 0, "a call without options is one with all-zero options");

// The first checks of every scan: the count and the arrays that none can do without (`second`: axes_dev or dir_dev).
static int qd_check_scan_arrays(const qd_handle* h, const char* who, int nq, const void* env_of_query, const void* second,
                                const char* second_name, const void* range, const void* gate_v, const void* barrier_v) {
    if (nq < 0) return qd_failf(h, QD_ERR_ARG, "%s: nq < 0", who);
    if (!env_of_query || !second || !range) return qd_failf(h, QD_ERR_ARG, "%s: env_of_query_dev, %s or range_dev is NULL", who, second_name);
    if (!gate_v || !barrier_v) return qd_failf(h, QD_ERR_ARG, "%s: gate_v_dev or barrier_v_dev is NULL", who);
    return QD_OK;
}

// The checks of a scan's options (`opts`: null, or one of the scans' option structs, `opts_type` by name) and of the handle,
// for the entry point `who` that renders `what` (scan, line, grid; thermal: at a temperature); o <- the options.
static int qd_check_scan(const qd_handle* h, const char* who, const char* opts_type, const char* what, const void* opts, bool thermal,
                         QdQueryOpts& o) {
    qd_scan_opts so{};
    char size_msg[128];
    snprintf(size_msg, sizeof(size_msg), "%s: opts->struct_size is not sizeof(%s)", who, opts_type);
    if (int rc = qd_check_struct_size(h, opts, sizeof(qd_scan_opts), size_msg)) return rc;
    if (opts) memcpy(&so, opts, sizeof(so));
    if (so.frame != QD_SCAN_VIRTUAL && so.frame != QD_SCAN_PHYSICAL)
        return qd_failf(h, QD_ERR_ARG, "%s: opts->frame is neither QD_SCAN_VIRTUAL nor QD_SCAN_PHYSICAL", who);
    if (so.frame == QD_SCAN_PHYSICAL && so.vgm_dev) return qd_failf(h, QD_ERR_ARG, "%s: vgm_dev has no meaning in the physical frame", who);
    if (so.noise_flags & ~(QD_NOISE_SENSOR | QD_NOISE_LATCH))
        return qd_failf(h, QD_ERR_ARG, "%s: noise_flags takes QD_NOISE_SENSOR and QD_NOISE_LATCH only (the radial stage is "
                                      "centred on the env's own adjacent-pair observation)", who);
    if (thermal && (so.noise_flags & QD_NOISE_LATCH))
        return qd_failf(h, QD_ERR_ARG, "%s: QD_NOISE_LATCH has no thermal form: the latching model holds an integer "
                                      "configuration, a thermal mean has none", who);
    if (h->cfg.flags & QD_FLAG_VALIDATE)
        return qd_failf(h, QD_ERR_STATE, "%s: a QD_FLAG_VALIDATE handle keeps records, occupations and eigenvalues of its "
                                        "B envs' last observe and renders no %ss; use a handle without the flag", who, what);
    if (h->full_m)
        return qd_failf(h, QD_ERR_STATE, "%s: the full charge-state space synthesises its own voltages "
                                        "(qd_k_full_structure); a %s front end for it is not built", who, what);
    o = QdQueryOpts{so.noise_flags, so.serial, so.stream_base, so.occ_dst || thermal, so.occ_dst, so.vgm_dev, so.gamma_dev, so.frame};
    return QD_OK;
}

// the one write kernel of the scans: `n` values per slot from rows of stride zs, occupations from slots of `os` points
static void qd_launch_query_write(const qd_handle* h, const int32_t* env_of_query, const int32_t* axes, int base, int cnt, int n, int zs,
                                  int os, const double* rows, const QdEnvBufs& b, double* raw_dst, float* image_dst, double* plohi_dst,
                                  double* occ_dst, hipStream_t s) {
    if (raw_dst || image_dst || plohi_dst || occ_dst)
        qd_k_query_write<<<dim3((n + 255) / 256, cnt), dim3(256), 0, s>>>(env_of_query, axes, base, h->B, h->N, n, zs, os, rows, b.plohi,
                                                                          b.occ, raw_dst, image_dst, plohi_dst, occ_dst);
}

extern "C" int qd_scan2d(qd_handle* h, const int32_t* env_of_query, int nq, const int32_t* axes, const double* range,
                         const double* gate_v, const double* barrier_v, const double* sensor_v, double* raw_dst, float* image_dst,
                         double* plohi_dst, const qd_scan_opts* opts, void* stream) {
    if (!h) return QD_ERR_ARG;
    QdQueryOpts o;
    if (int rc = qd_check_scan_arrays(h, "qd_scan2d", nq, env_of_query, axes, "axes_dev", range, gate_v, barrier_v)) return rc;
    if (int rc = qd_check_scan(h, "qd_scan2d", "qd_scan_opts", "scan", opts, false, o)) return rc;
    if (nq == 0) return QD_OK;
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    const QdScanQuery Q{env_of_query, axes, range, gate_v, barrier_v, sensor_v, o.vgm, o.gamma, o.frame};
    // ONE channel image per slot, over the axes that the gather kernel leaves in the slot's state block copy
    return qd_run_queries(h, h->scan, 1, QD_FRONT_SCAN, o, nq, s,
        [&](int base, int cnt, const QdEnvBufs& sb) {
            qd_k_scan_gather<<<dim3(cnt), dim3(QD_SCAN_BLOCK), 0, s>>>(Q, base, h->B, h->N, h->params.p, h->state.p, sb.params, sb.state);
        },
        [&](int base, int cnt, const QdEnvBufs& sb) {
            qd_launch_query_write(h, env_of_query, axes, base, cnt, h->P, h->P, h->P, sb.zraw, sb, raw_dst, image_dst, plohi_dst, o.occ_dst, s);
        });
}

extern "C" int qd_scan_affine(qd_handle* h, const int32_t* env_of_query, int nq, const double* dir, const double* range,
                              const double* gate_v, const double* barrier_v, const double* sensor_v, double* raw_dst,
                              float* image_dst, double* plohi_dst, const qd_scan_affine_opts* opts, void* stream) {
    if (!h) return QD_ERR_ARG;
    QdQueryOpts o;
    if (int rc = qd_check_scan_arrays(h, "qd_scan_affine", nq, env_of_query, dir, "dir_dev", range, gate_v, barrier_v)) return rc;
    if (int rc = qd_check_scan(h, "qd_scan_affine", "qd_scan_affine_opts", "scan", opts, false, o)) return rc;
    if (nq == 0) return QD_OK;
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    const QdAffineQuery Q{env_of_query, dir, range, gate_v, barrier_v, sensor_v, o.vgm, o.gamma, o.frame};
    // one descriptor per query in flight (qd_run_queries: h->chunk slots), beside the slots of the scan buffers
    QD_HIP(h->affine_axes.reserve((size_t)h->chunk));
    QdAffineAxes* const axes = h->affine_axes.p;
    return qd_run_queries(h, h->scan, 1, QD_FRONT_AFFINE, o, nq, s,
        [&](int base, int cnt, const QdEnvBufs& sb) {
            qd_k_affine_gather<<<dim3(cnt), dim3(QD_AFFINE_BLOCK), 0, s>>>(Q, base, h->B, h->N, h->params.p, h->state.p, sb.params, sb.state,
                                                                           axes);
        },
        [&](int base, int cnt, const QdEnvBufs& sb) {
            qd_launch_query_write(h, env_of_query, nullptr, base, cnt, h->P, h->P, h->P, sb.zraw, sb, raw_dst, image_dst, plohi_dst, o.occ_dst, s);
        });
}

// slots in flight of qd_scan1d and qd_scan_grid* for nq queries of n points: what lane 0's record buffer (chunk * C * P records)
// and its slabs (gs_batches) hold in slots of the line's own size, at most QD_LINE_SLOTS.  With n <= P both hold one slot at
// the least.
static int qd_line_slots(const qd_handle* h, int n, int nq) {
    const int side = qd_line_side(n);
    const size_t sp = (size_t)side * side;
    size_t slots = (size_t)h->chunk * h->C * h->P / sp;
    const size_t by_slabs = h->gs_batches / (size_t)qd_line_batches(n, h->ppb);
    if (by_slabs < slots) slots = by_slabs;
    if (slots > QD_LINE_MAX_SLOTS) slots = QD_LINE_MAX_SLOTS;
    return (size_t)nq < slots ? nq : (int)slots;
}

// qd_scan1d and qd_scan_grid* on the runner, `pc` slots in flight: the slot of n points is side x side records, record p =
// point p, the tail inert, filled by a front kernel of the caller's (in solve) before the redo pass; the n leading values of a
// slot are packed into a dense row for the percentile and the write kernel.
template <class Gather, class Solve, class Latch>
static int qd_run_lines(qd_handle* h, int n, int pc, const QdQueryOpts& o, const int32_t* env_of_query, int nq, double* raw_dst,
                        float* image_dst, double* plohi_dst, hipStream_t s, Gather gather, Solve solve, Latch latch) {
    QD_HIP(h->line_dense.reserve((size_t)pc * n));
    double* const dense = h->line_dense.p;
    return qd_run_queries(h, h->line, QdSlotGeom{1, qd_line_side(n), n, pc, QD_FRONT_LINE}, o, nq, s, gather, solve, latch,
        [&](int cnt, const QdEnvBufs& b) {
            qd_k_line_pack<<<dim3((n + 255) / 256, cnt), dim3(256), 0, s>>>(n, b.P, b.zraw, dense);
            return (const double*)dense;
        },
        [&](int base, int cnt, const QdEnvBufs& b, const double* rows) {
            qd_launch_query_write(h, env_of_query, nullptr, base, cnt, n, n, b.P, rows, b, raw_dst, image_dst, plohi_dst, o.occ_dst, s);
        });
}

extern "C" int qd_scan1d(qd_handle* h, const int32_t* env_of_query, int nq, int n_points, const double* dir, const double* range,
                         const double* gate_v, const double* barrier_v, const double* sensor_v, double* raw_dst, float* image_dst,
                         double* plohi_dst, const qd_scan1d_opts* opts, void* stream) {
    static_assert(QD_LINE_MAX_SLOTS == QD_LINE_SLOTS, "qdsim.h states the bound");
    if (!h) return QD_ERR_ARG;
    QdQueryOpts o;
    if (int rc = qd_check_scan_arrays(h, "qd_scan1d", nq, env_of_query, dir, "dir_dev", range, gate_v, barrier_v)) return rc;
    if (n_points < 1 || n_points > h->P) return qd_fail(h, QD_ERR_ARG, "qd_scan1d: n_points must be in 1..P (P = resolution^2 of the handle)");
    if (int rc = qd_check_scan(h, "qd_scan1d", "qd_scan1d_opts", "line", opts, false, o)) return rc;
    if (nq == 0) return QD_OK;
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    const QdAffineQuery Q{env_of_query, dir, range, gate_v, barrier_v, sensor_v, o.vgm, o.gamma, o.frame};
    const int n = n_points, pc = qd_line_slots(h, n, nq);
    QD_HIP(h->line_axes.reserve((size_t)pc));
    const QdLane& ln = h->lanes[0];
    QdLineAxes* const axes = h->line_axes.p;
    return qd_run_lines(h, n, pc, o, env_of_query, nq, raw_dst, image_dst, plohi_dst, s,
        [&](int base, int cnt, const QdEnvBufs& b) {
            qd_k_line_gather<<<dim3(cnt), dim3(QD_LINE_BLOCK), 0, s>>>(Q, base, h->B, h->N, h->params.p, h->state.p, b.params, b.state, axes);
        },
        [&](int, int cnt, const QdEnvBufs& b) {
            QD_DISPATCH_N(h->N, qd_k_line_front<NN><<<dim3((b.P + QD_LINE_BLOCK - 1) / QD_LINE_BLOCK, cnt), dim3(QD_LINE_BLOCK), 0, s>>>(
                                    n, b.P, b.params, b.state, axes, ln.recs.p));
            QD_HIP(hipGetLastError());
            if (int rc = qd_launch_candidates(h, b, ln, nullptr, 0, cnt, s, true)) return rc;
            return qd_launch_ground(h, b, ln, nullptr, 0, cnt, s, QD_ST_GROUND);
        },
        [&](int cnt, const QdEnvBufs& b) {
            QD_DISPATCH_N(h->N, qd_k_latch_lines<NN><<<dim3((cnt + 63) / 64), dim3(64), 0, s>>>(cnt, n, b.P, b.params, b.occ, b.zraw,
                                                                                              qd_noise_cfg(h, b)));
            return (int)QD_OK;
        });
}

// A range check that reads the device: one copy of the nq values of `dev` and a wait for the stream, then ok() of each.
// copy_what and range_fmt: the texts of the two failures.
template <class T, class Ok>
static int qd_check_device_range(const qd_handle* h, const char* who, const T* dev, int nq, hipStream_t s, const char* copy_what,
                                 const char* range_fmt, Ok ok) {
    T* host = (T*)malloc(sizeof(T) * (size_t)nq);
    if (!host) return qd_fail(h, QD_ERR_NOMEM, "malloc");
    hipError_t e_ = hipMemcpyAsync(host, dev, sizeof(T) * (size_t)nq, hipMemcpyDeviceToHost, s);
    if (e_ == hipSuccess) e_ = hipStreamSynchronize(s);
    bool bad = false;
    for (int q = 0; q < nq && e_ == hipSuccess; ++q) bad = bad || !ok(host[q]);
    free(host);
    if (e_ != hipSuccess) return qd_fail(h, QD_ERR_HIP, copy_what, e_);
    return bad ? qd_failf(h, QD_ERR_ARG, range_fmt, who) : (int)QD_OK;
}

// Which core the levels kernel of a grid runs on: the whole-block one in the closed regime (one component per list), the
// per-component one in the open regime.  MEASURED ahead of the whole-block core there by more than the run-to-run spread are 4
// and 8 dots at K = 8 and K = 32 (19 to 58 % at K = 32, 10 to 13 % at 4 dots and K = 8, 1.3 to 1.7 % at 8 dots and K = 8, the
// narrowest cell: DESIGN 7); every other N and K is unmeasured.  Under the measurement-only build macro QD_LVG_FORCE_WHOLE
// (scripts/levels_grid_rate.py, route c) every grid runs the whole-block core.
#ifdef QD_LVG_FORCE_WHOLE
#define QD_LVG_WHOLE(n_charge) true
#else
#define QD_LVG_WHOLE(n_charge) ((n_charge) != nullptr)
#endif

// Which core and epilogue the response kernel of a grid runs: qd_thermal_solve and qd_response_solve on the whole block in the
// closed regime (one component per list), the per-component pair of qd_thermal_blocks.h and qd_response_blocks.h in the open
// regime.  MEASURED ahead of the whole-block pair there by more than the run-to-run spread are 4 and 8 dots at K = 32 (2.93 and
// 1.65 times the rate of the whole call, spread 0.5 %; both the core and the epilogue are exchanged, so the figure includes what
// the per-component thermal core gains: DESIGN 7); every other N and K is unmeasured.  Under the measurement-only build macro
// QD_RSG_FORCE_WHOLE (scripts/response_grid_rate.py, route e) every grid runs the whole-block core and epilogue.
#ifdef QD_RSG_FORCE_WHOLE
#define QD_RSG_WHOLE(n_charge) true
#else
#define QD_RSG_WHOLE(n_charge) ((n_charge) != nullptr)
#endif

// What runs behind the search of a grid (qd_grid_run) or of points (qd_points_run).  All off, as a value starts, is qd_scan_grid /
// qd_eval_points; every other entry point sets by name what it adds.  Per query on the device (grids), per group on the host (points).
struct QdBehindSearch {
    // qd_*_closed: qd_k_closed at these total charges replaces the redo pass of the open search; states_dst (points): the kept states
    const int32_t* n_charge = nullptr; int32_t* states_dst = nullptr;
    // qd_*_thermal (a host kT is checked by the caller): the thermal kernel (qd_thermal_blocks.h, qd_thermal.h) in place of the
    // ground-state stage, once, on the lists as the search left them; a grid's slots always carry occupations then
    const double* kT = nullptr; double *var_dst = nullptr, *ztail_dst = nullptr;
    // n_levels > 0 (qd_scan_grid_levels, qd_eval_points_ex): the levels kernel (qd_levels_blocks.h, qd_levels.h) behind the search and
    // before the ground-state stage; it reads the records and writes the caller's rows
    int n_levels = 0; double *levels_dst = nullptr, *hnorm_dst = nullptr;
    // any row, with kT (qd_*_response; points: chi, jac, dsignal): the thermal kernel with the response epilogue in its place
    QdGridResponseDst rd{};
    bool response() const { return rd.chi || rd.jac || rd.dsignal || rd.docc_axes || rd.dsignal_axes; }
    const double* gamma = nullptr;                      // points: the peak width of every group; null: each env's own
};

// qd_scan_grid and its four siblings on the runner of the lines; x: what runs behind the search
static int qd_grid_run(qd_handle* h, const char* who, const int32_t* env_of_query, int nq, int nx, int ny, const double* dir,
                       const double* range, const double* gate_v, const double* barrier_v, const double* sensor_v, double* raw_dst,
                       float* image_dst, double* plohi_dst, const qd_scan_grid_opts* opts, const QdBehindSearch& x, void* stream) {
    static_assert(QD_GRID_MAX_SLOTS == QD_GRID_SLOTS, "qdsim.h states the bound");
    static_assert(QD_THG_BLOCKS <= QD_GRID_MAX_SLOTS && QD_LVG_BLOCKS <= QD_GRID_MAX_SLOTS, "a launch dimension");
    QdQueryOpts o;
    if (int rc = qd_check_scan_arrays(h, who, nq, env_of_query, dir, "dir_dev", range, gate_v, barrier_v)) return rc;
    if (nx < 1 || ny < 1 || (long long)nx * ny > h->P)
        return qd_failf(h, QD_ERR_ARG, "%s: nx and ny must be >= 1 with nx*ny <= P (P = resolution^2 of the handle)", who);
    if (int rc = qd_check_scan(h, who, "qd_scan_grid_opts", "grid", opts, x.kT != nullptr, o)) return rc;
    if (x.n_charge && o.noise_flags)
        return qd_failf(h, QD_ERR_ARG, "%s: the closed regime has no noise stages: noise_flags must be 0", who);
    if (nq == 0) return QD_OK;
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    if (x.n_charge)
        if (int rc = qd_check_device_range(h, who, x.n_charge, nq, s, "hipMemcpyAsync(n_charge)", "%s: n_charge must be in 0..32767",
                                           [](int32_t v) { return v >= 0 && v <= QD_CLOSED_QMAX; })) return rc;
    if (x.kT)
        if (int rc = qd_check_device_range(h, who, x.kT, nq, s, "hipMemcpyAsync(kT)", "%s: kT must be finite and > 0",
                                           [](double v) { return v > 0.0 && v < INFINITY; })) return rc;
    if (x.response()) {
        // (with no response destination the call is qd_scan_grid_thermal, which takes such envs)
        bool vc = false;
        if (int rc = qd_check_device_range(h, who, env_of_query, nq, s, "hipMemcpyAsync(env_of_query)", "%s: env_of_query",
                                           [&](int32_t e) { vc = vc || (e >= 0 && e < h->B && h->vc_on[(size_t)e]); return true; })) return rc;
        if (vc) return qd_fail_vc(h, who);
    }
    const QdAffineQuery Q{env_of_query, dir, range, gate_v, barrier_v, sensor_v, o.vgm, o.gamma, o.frame};
    // the slot of a grid is that of a line of nx*ny points, record p = y*nx + x
    const int n = nx * ny, pc = qd_line_slots(h, n, nq);
    QD_HIP(h->grid_axes.reserve((size_t)pc));
    const QdLane& ln = h->lanes[0];
    QdGridAxes* const axes = h->grid_axes.p;
    return qd_run_lines(h, n, pc, o, env_of_query, nq, raw_dst, image_dst, plohi_dst, s,
        [&](int base, int cnt, const QdEnvBufs& b) {
            qd_k_grid_gather<<<dim3(cnt), dim3(QD_GRID_BLOCK), 0, s>>>(Q, base, h->B, h->N, nx, ny, h->params.p, h->state.p, b.params, b.state,
                                                                       axes);
        },
        [&](int base, int cnt, const QdEnvBufs& b) {
            const int SP = b.P;
            QD_DISPATCH_N(h->N, qd_k_grid_front<NN><<<dim3((SP + QD_GRID_BLOCK - 1) / QD_GRID_BLOCK, cnt), dim3(QD_GRID_BLOCK), 0, s>>>(
                                    SP, b.params, b.state, axes, ln.recs.p));
            QD_HIP(hipGetLastError());
            if (x.n_charge) { if (int rc = qd_launch_closed(h, b, ln, SP, x.n_charge + base, cnt, s)) return rc; }
            else if (int rc = qd_launch_candidates(h, b, ln, nullptr, 0, cnt, s, true)) return rc;
            if (x.n_levels > 0) {
                // the levels of the list as the search left it (a closed list is one hop component: the whole-block core)
                const dim3 lgrid((unsigned)(n < QD_LVG_BLOCKS ? n : QD_LVG_BLOCKS), cnt);
                QD_DISPATCH_BOOL(QD_LVG_WHOLE(x.n_charge), WHOLE, QD_DISPATCH_N(h->N,
                    qd_k_levels_grid<NN, std::conditional_t<WHOLE, QdLevelsWs, QdLevelsBlocksWs>><<<lgrid, dim3(64), 0, s>>>(
                        env_of_query, base, h->B, n, SP, h->kept, x.n_levels, ln.recs.p, x.levels_dst, x.hnorm_dst)));
                QD_HIP(hipGetLastError());
            }
            if (!x.kT) return qd_launch_ground(h, b, ln, nullptr, 0, cnt, s, QD_ST_GROUND);
            // the thermal state instead of the ground state: c0 and <n> into the slots' zraw and occ, then the unchanged stages
            const dim3 tgrid((unsigned)(n < QD_THG_BLOCKS ? n : QD_THG_BLOCKS), cnt);
            if (x.response()) {
                // qd_scan_grid_response: the thermal kernel with the response epilogue (qd_response_blocks.h), whose instances are
                // compiled in qd_response_grid.hip
                if (!qd_launch_thermal_grid_response(h->N, QD_RSG_WHOLE(x.n_charge), tgrid, s, &Q, sizeof(Q), base, h->B, n, SP, h->kept, x.kT,
                                                     b.params, b.state, axes, ln.recs.p, b.zraw, b.occ, x.var_dst, x.ztail_dst, x.rd))
                    return qd_fail(h, QD_ERR_ARG, "n_dot must be in 2..8");
                QD_HIP(hipGetLastError());
                return (int)QD_OK;
            }
            // (a closed list is one hop component: the whole-block core, see qd_k_thermal_grid)
            QD_DISPATCH_BOOL(x.n_charge != nullptr, WHOLE, QD_DISPATCH_N(h->N,
                qd_k_thermal_grid<NN, std::conditional_t<WHOLE, QdThermalWs, QdThermalBlocksWs>><<<tgrid, dim3(64), 0, s>>>(
                    Q, base, h->B, n, SP, h->kept, x.kT, b.params, ln.recs.p, b.zraw, b.occ, x.var_dst, x.ztail_dst)));
            QD_HIP(hipGetLastError());
            return (int)QD_OK;
        },
        [&](int cnt, const QdEnvBufs& b) {
            const long rows = (long)cnt * ny;
            QD_DISPATCH_N(h->N, qd_k_latch_grid<NN><<<dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, s>>>(cnt, nx, ny, b.P, b.params, b.occ,
                                                                                                          b.zraw, qd_noise_cfg(h, b)));
            return (int)QD_OK;
        });
}

extern "C" int qd_scan_grid(qd_handle* h, const int32_t* env_of_query, int nq, int nx, int ny, const double* dir, const double* range,
                            const double* gate_v, const double* barrier_v, const double* sensor_v, double* raw_dst, float* image_dst,
                            double* plohi_dst, const qd_scan_grid_opts* opts, void* stream) {
    if (!h) return QD_ERR_ARG;
    return qd_grid_run(h, "qd_scan_grid", env_of_query, nq, nx, ny, dir, range, gate_v, barrier_v, sensor_v, raw_dst, image_dst,
                       plohi_dst, opts, QdBehindSearch{}, stream);
}

extern "C" int qd_scan_grid_closed(qd_handle* h, const int32_t* env_of_query, int nq, int nx, int ny, const double* dir,
                                   const double* range, const double* gate_v, const double* barrier_v, const double* sensor_v,
                                   const int32_t* n_charge, double* raw_dst, float* image_dst, double* plohi_dst,
                                   const qd_scan_grid_opts* opts, void* stream) {
    if (!h) return QD_ERR_ARG;
    if (!n_charge) return qd_fail(h, QD_ERR_ARG, "qd_scan_grid_closed: n_charge_dev is NULL");
    QdBehindSearch x; x.n_charge = n_charge;
    return qd_grid_run(h, "qd_scan_grid_closed", env_of_query, nq, nx, ny, dir, range, gate_v, barrier_v, sensor_v, raw_dst, image_dst,
                       plohi_dst, opts, x, stream);
}

extern "C" int qd_scan_grid_thermal(qd_handle* h, const int32_t* env_of_query, int nq, int nx, int ny, const double* dir,
                                    const double* range, const double* gate_v, const double* barrier_v, const double* sensor_v,
                                    const double* kT, double* raw_dst, float* image_dst, double* plohi_dst,
                                    const qd_scan_grid_opts* opts, const qd_grid_thermal_opts* topts, void* stream) {
    if (!h) return QD_ERR_ARG;
    if (!kT) return qd_fail(h, QD_ERR_ARG, "qd_scan_grid_thermal: kT_dev is NULL");
    if (int rc = qd_check_struct_size(h, topts, sizeof(qd_grid_thermal_opts),
                                      "qd_scan_grid_thermal: topts->struct_size is not sizeof(qd_grid_thermal_opts)")) return rc;
    QdBehindSearch x; x.kT = kT;
    if (topts) { x.n_charge = topts->n_charge_dev; x.var_dst = topts->var_dst; x.ztail_dst = topts->ztail_dst; }
    return qd_grid_run(h, "qd_scan_grid_thermal", env_of_query, nq, nx, ny, dir, range, gate_v, barrier_v, sensor_v, raw_dst, image_dst,
                       plohi_dst, opts, x, stream);
}

extern "C" int qd_scan_grid_response(qd_handle* h, const int32_t* env_of_query, int nq, int nx, int ny, const double* dir,
                                     const double* range, const double* gate_v, const double* barrier_v, const double* sensor_v,
                                     const double* kT, double* raw_dst, float* image_dst, double* plohi_dst,
                                     const qd_scan_grid_opts* opts, const qd_grid_response_opts* ropts, void* stream) {
    if (!h) return QD_ERR_ARG;
    if (!kT) return qd_fail(h, QD_ERR_ARG, "qd_scan_grid_response: kT_dev is NULL");
    if (int rc = qd_check_struct_size(h, ropts, sizeof(qd_grid_response_opts),
                                      "qd_scan_grid_response: ropts->struct_size is not sizeof(qd_grid_response_opts)")) return rc;
    QdBehindSearch x; x.kT = kT;
    if (ropts) { x.n_charge = ropts->n_charge_dev; x.var_dst = ropts->var_dst; x.ztail_dst = ropts->ztail_dst; }
    // (with all five null the call launches qd_k_thermal_grid itself)
    if (ropts) x.rd = QdGridResponseDst{ropts->chi_dst, ropts->jac_dst, ropts->dsignal_dst, ropts->docc_axes_dst, ropts->dsignal_axes_dst};
    return qd_grid_run(h, "qd_scan_grid_response", env_of_query, nq, nx, ny, dir, range, gate_v, barrier_v, sensor_v, raw_dst, image_dst,
                       plohi_dst, opts, x, stream);
}

extern "C" int qd_scan_grid_levels(qd_handle* h, const int32_t* env_of_query, int nq, int nx, int ny, const double* dir,
                                   const double* range, const double* gate_v, const double* barrier_v, const double* sensor_v,
                                   double* raw_dst, float* image_dst, double* plohi_dst, const qd_scan_grid_opts* opts,
                                   const qd_grid_levels_opts* lopts, void* stream) {
    if (!h) return QD_ERR_ARG;
    if (!lopts) return qd_fail(h, QD_ERR_ARG, "qd_scan_grid_levels: lopts is NULL");
    if (int rc = qd_check_struct_size(h, lopts, sizeof(qd_grid_levels_opts),
                                      "qd_scan_grid_levels: lopts->struct_size is not sizeof(qd_grid_levels_opts)")) return rc;
    if (lopts->n_levels < 1 || lopts->n_levels > QD_LEVELS_MAX)
        return qd_fail(h, QD_ERR_ARG, "qd_scan_grid_levels: n_levels must be in 1..QD_LEVELS_MAX (8)");
    if (!lopts->levels_dst) return qd_fail(h, QD_ERR_ARG, "qd_scan_grid_levels: levels_dst is NULL");
    QdBehindSearch x; x.n_charge = lopts->n_charge_dev;
    x.n_levels = lopts->n_levels; x.levels_dst = lopts->levels_dst; x.hnorm_dst = lopts->hnorm_dst;
    return qd_grid_run(h, "qd_scan_grid_levels", env_of_query, nq, nx, ny, dir, range, gate_v, barrier_v, sensor_v, raw_dst, image_dst,
                       plohi_dst, opts, x, stream);
}

// slots in flight of qd_eval_points: one launch chunk of lane 0's records, at most QD_POINTS_SLOTS
static int qd_points_slots(const qd_handle* h) { return h->chunk < QD_POINTS_MAX_SLOTS ? h->chunk : QD_POINTS_MAX_SLOTS; }

// qd_eval_points and its four siblings on one slot loop, as qd_grid_run; x: what runs behind the search of every flush.
static int qd_points_run(qd_handle* h, const char* who, const int32_t* group_env, const int64_t* group_start, int ng, const double* vg,
                         const double* vb, double* signal_dst, double* occ_dst, const QdBehindSearch& x, void* stream) {
    static_assert(QD_POINTS_MAX_SLOTS == QD_POINTS_SLOTS, "qdsim.h states the bound");
    if (ng < 0) return qd_failf(h, QD_ERR_ARG, "%s: ng < 0", who);
    if (!group_env || !group_start) return qd_failf(h, QD_ERR_ARG, "%s: group_env_host or group_start_host is NULL", who);
    if (!vg || !vb) return qd_failf(h, QD_ERR_ARG, "%s: vg_dev or vb_dev is NULL", who);
    if (group_start[0] < 0) return qd_failf(h, QD_ERR_ARG, "%s: group_start is negative", who);
    for (int g = 0; g < ng; ++g) {
        if (group_start[g + 1] < group_start[g]) return qd_failf(h, QD_ERR_ARG, "%s: group_start is not non-decreasing", who);
        if (group_env[g] < 0 || group_env[g] >= h->B) return qd_failf(h, QD_ERR_ARG, "%s: env id out of range", who);
        if (x.n_charge && (x.n_charge[g] < 0 || x.n_charge[g] > QD_CLOSED_QMAX)) return qd_failf(h, QD_ERR_ARG, "%s: n_charge must be in 0..32767", who);
    }
    if (h->cfg.flags & QD_FLAG_VALIDATE)
        return qd_failf(h, QD_ERR_STATE, "%s: a QD_FLAG_VALIDATE handle keeps records, occupations and eigenvalues of its "
                                        "B envs' last observe and evaluates no points; use a handle without the flag", who);
    if (h->full_m)
        return qd_failf(h, QD_ERR_STATE, "%s: the full charge-state space synthesises its own voltages "
                                        "(qd_k_full_structure); a point front end for it is not built yet", who);
    if (ng == 0 || group_start[ng] == group_start[0]) return QD_OK;
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    const int ps = qd_points_slots(h);
    const long long CP = (long long)h->C * h->P;
    QD_HIP(h->points.reserve(h->L, (size_t)CP, (size_t)ps, 0, (size_t)CP * h->N, 0));      // (neither percentiles nor telegraph words)
    // the ground-state launcher runs on the point buffers, without noise or eigenvalues; nothing of the envs is written
    const QdEnvBufs qb = h->points.view(h->C, h->R, QD_FRONT_ENV);
    const QdLane& ln = h->lanes[0];
    if (x.n_charge) QD_HIP(h->closed_q.reserve((size_t)QD_POINTS_MAX_SLOTS));
    QdPointSlots T;
    memset(&T, 0, sizeof(T));
    QdClosedQ TQ;
    memset(&TQ, 0, sizeof(TQ));
    QdThermalKT TK;
    memset(&TK, 0, sizeof(TK));
    T.own_gamma = x.gamma ? 0 : 1;
    int n = 0;
    // one launch per `ps` slots: gather -> front end -> per-pixel search of the handed-over records -> ground state -> write
    auto flush = [&]() -> int {
        if (n == 0) return QD_OK;
        const dim3 grid((unsigned)((CP + QD_POINTS_BLOCK - 1) / QD_POINTS_BLOCK), n);
        qd_k_points_gather<<<dim3(n), dim3(QD_POINTS_BLOCK), 0, s>>>(T, h->N, h->params.p, h->state.p, qb.params, qb.state);
        QD_HIP(hipGetLastError());
        QD_DISPATCH_N(h->N, qd_k_points_front<NN><<<grid, dim3(QD_POINTS_BLOCK), 0, s>>>(T, (int)CP, vg, vb, qb.params, ln.recs.p));
        QD_HIP(hipGetLastError());
        // (the redo instantiation, and not through qd_launch_csd: on handles without a tile search that would pick the
        // whole per-pixel search and overwrite the front end)
        if (x.n_charge) {
            // the closed regime: the slots' total charges to the device, then centre and sector search instead of the redo pass
            qd_k_closed_setq<<<dim3(1), dim3(QD_POINTS_MAX_SLOTS), 0, s>>>(TQ, n, h->closed_q.p);
            QD_HIP(hipGetLastError());
            if (int rc = qd_launch_closed(h, qb, ln, (int)CP, h->closed_q.p, n, s)) return rc;
            if (x.states_dst) {
                QD_DISPATCH_N(h->N, qd_k_closed_states<NN><<<grid, dim3(QD_POINTS_BLOCK), 0, s>>>(T, (int)CP, h->kept, ln.recs.p, x.states_dst));
                QD_HIP(hipGetLastError());
            }
        } else if (int rc = qd_launch_candidates(h, qb, ln, nullptr, 0, n, s, true)) return rc;
        if (x.n_levels > 0) {
            // the levels of the list as the search left it, before any qd_k_points_sort: one point per single-wave block
            const dim3 lgrid((unsigned)(CP < 4096 ? CP : 4096), n);
            QD_DISPATCH_N(h->N, qd_k_levels<NN><<<lgrid, dim3(64), 0, s>>>(T, (int)CP, h->kept, x.n_levels, ln.recs.p, x.levels_dst, x.hnorm_dst));
            QD_HIP(hipGetLastError());
            if (!signal_dst && !occ_dst) { n = 0; return QD_OK; }          // levels only: no ground-state stage
        }
        if (x.kT) {
            // the thermal state instead of the ground state: c0 and <n> into the slots' zraw and occ, then the unchanged write
            const dim3 tgrid((unsigned)(CP < 4096 ? CP : 4096), n);
            if (x.response()) {
                // qd_eval_points_response: the thermal kernel with the response epilogue (qd_response.h); dc0/dv into x.rd.dsignal
                QD_DISPATCH_N(h->N, qd_k_thermal_response<NN><<<tgrid, dim3(64), 0, s>>>(
                    T, TK, (int)CP, h->kept, qb.params, ln.recs.p, qb.zraw, qb.occ, x.var_dst, x.ztail_dst, x.rd.chi, x.rd.jac, x.rd.dsignal));
            } else {
                QD_DISPATCH_N(h->N, qd_k_thermal<NN><<<tgrid, dim3(64), 0, s>>>(T, TK, (int)CP, h->kept, qb.params, ln.recs.p, qb.zraw,
                                                                               qb.occ, x.var_dst, x.ztail_dst));
            }
            QD_HIP(hipGetLastError());
            if (signal_dst || occ_dst) {
                QD_DISPATCH_N(h->N, qd_k_points_write<NN><<<grid, dim3(QD_POINTS_BLOCK), 0, s>>>(T, (int)CP, qb.params, qb.zraw, qb.occ,
                                                                                               signal_dst, occ_dst));
                QD_HIP(hipGetLastError());
            }
            if (x.rd.dsignal) {
                QD_DISPATCH_N(h->N, qd_k_points_dsignal<NN><<<grid, dim3(QD_POINTS_BLOCK), 0, s>>>(T, (int)CP, qb.params, qb.zraw, x.rd.dsignal));
                QD_HIP(hipGetLastError());
            }
            n = 0;
            return QD_OK;
        }
        // The signal comes from the list as the search left it, which is what qd_observe and qd_probe solve: the probe's bits.
        // The occupations come from the list in the reference order, which is what a validate handle solves and
        // qd_get_occupations returns: with K == KC (search order) the records are sorted and the ground-state stage runs again.
        // (the closed lists are in the reference order as they come)
        const bool resort = !x.n_charge && !qd_sorted_records(h) && occ_dst;
        if (signal_dst || !resort) {
            if (int rc = qd_launch_ground(h, qb, ln, nullptr, 0, n, s, QD_ST_GROUND)) return rc;
            if (signal_dst || occ_dst) {
                QD_DISPATCH_N(h->N, qd_k_points_write<NN><<<grid, dim3(QD_POINTS_BLOCK), 0, s>>>(T, (int)CP, qb.params, qb.zraw, qb.occ,
                                                                                               signal_dst, resort ? nullptr : occ_dst));
                QD_HIP(hipGetLastError());
            }
        }
        if (resort) {
            const long nrec = (long)n * CP;
            QD_DISPATCH_KC(h->kc, qd_k_points_sort<KK><<<dim3((unsigned)((nrec + 63) / 64)), dim3(64), 0, s>>>(ln.recs.p, nrec));
            QD_HIP(hipGetLastError());
            if (int rc = qd_launch_ground(h, qb, ln, nullptr, 0, n, s, QD_ST_GROUND)) return rc;
            QD_DISPATCH_N(h->N, qd_k_points_write<NN><<<grid, dim3(QD_POINTS_BLOCK), 0, s>>>(T, (int)CP, qb.params, qb.zraw, qb.occ,
                                                                                           nullptr, occ_dst));
            QD_HIP(hipGetLastError());
        }
        n = 0;
        return QD_OK;
    };
    for (int g = 0; g < ng; ++g) {
        for (long long p0 = group_start[g]; p0 < group_start[g + 1]; p0 += CP) {
            const long long left = group_start[g + 1] - p0;
            T.start[n] = p0; T.env[n] = group_env[g]; T.cnt[n] = (int)(left < CP ? left : CP);
            T.gamma[n] = x.gamma ? x.gamma[g] : 0.0;
            TQ.q[n] = x.n_charge ? x.n_charge[g] : 0;
            TK.kT[n] = x.kT ? x.kT[g] : 0.0;
            if (++n == ps) if (int rc = flush()) return rc;
        }
    }
    return flush();
}

extern "C" int qd_eval_points(qd_handle* h, const int32_t* group_env, const int64_t* group_start, int ng, const double* vg,
                              const double* vb, const double* gamma, double* signal_dst, double* occ_dst, void* stream) {
    if (!h) return QD_ERR_ARG;
    QdBehindSearch x; x.gamma = gamma;
    return qd_points_run(h, "qd_eval_points", group_env, group_start, ng, vg, vb, signal_dst, occ_dst, x, stream);
}

extern "C" int qd_eval_points_closed(qd_handle* h, const int32_t* group_env, const int64_t* group_start, int ng, const double* vg,
                                     const double* vb, const double* gamma, const int32_t* n_charge, double* signal_dst,
                                     double* occ_dst, int32_t* states_dst, void* stream) {
    if (!h) return QD_ERR_ARG;
    if (!n_charge) return qd_fail(h, QD_ERR_ARG, "qd_eval_points_closed: n_charge_host is NULL");
    QdBehindSearch x; x.gamma = gamma; x.n_charge = n_charge; x.states_dst = states_dst;
    return qd_points_run(h, "qd_eval_points_closed", group_env, group_start, ng, vg, vb, signal_dst, occ_dst, x, stream);
}

extern "C" int qd_eval_points_ex(qd_handle* h, const int32_t* group_env, const int64_t* group_start, int ng, const double* vg,
                                 const double* vb, double* signal_dst, double* occ_dst, const qd_points_opts* opts, void* stream) {
    static_assert(QD_LEVELS_MAX <= QD_LV_MAX, "a level per state at most");
    if (!h) return QD_ERR_ARG;
    QdBehindSearch x;
    if (!opts) return qd_points_run(h, "qd_eval_points_ex", group_env, group_start, ng, vg, vb, signal_dst, occ_dst, x, stream);
    if (int rc = qd_check_struct_size(h, opts, sizeof(qd_points_opts), "qd_eval_points_ex: opts->struct_size is not sizeof(qd_points_opts)")) return rc;
    if (opts->n_levels < 0 || opts->n_levels > QD_LEVELS_MAX)
        return qd_fail(h, QD_ERR_ARG, "qd_eval_points_ex: opts->n_levels must be in 0..QD_LEVELS_MAX (8)");
    if (opts->n_levels > 0 && !opts->levels_dst)
        return qd_fail(h, QD_ERR_ARG, "qd_eval_points_ex: opts->n_levels > 0 needs opts->levels_dst");
    if (opts->states_dst && !opts->n_charge_host)
        return qd_fail(h, QD_ERR_ARG, "qd_eval_points_ex: opts->states_dst is an output of the closed regime and needs opts->n_charge_host");
    x.gamma = opts->gamma_host; x.n_charge = opts->n_charge_host; x.states_dst = opts->states_dst;
    x.n_levels = opts->n_levels; x.levels_dst = opts->levels_dst; x.hnorm_dst = opts->hnorm_dst;
    return qd_points_run(h, "qd_eval_points_ex", group_env, group_start, ng, vg, vb, signal_dst, occ_dst, x, stream);
}

extern "C" int qd_eval_points_thermal(qd_handle* h, const int32_t* group_env, const int64_t* group_start, int ng, const double* vg,
                                      const double* vb, const double* kT, double* signal_dst, double* occ_dst,
                                      const qd_thermal_opts* opts, void* stream) {
    if (!h) return QD_ERR_ARG;
    if (int rc = qd_check_kT_host(h, "qd_eval_points_thermal", kT, ng)) return rc;
    if (int rc = qd_check_struct_size(h, opts, sizeof(qd_thermal_opts), "qd_eval_points_thermal: opts->struct_size is not sizeof(qd_thermal_opts)")) return rc;
    QdBehindSearch x; x.kT = kT;
    if (opts) { x.gamma = opts->gamma_host; x.n_charge = opts->n_charge_host; x.var_dst = opts->var_dst; x.ztail_dst = opts->ztail_dst; }
    return qd_points_run(h, "qd_eval_points_thermal", group_env, group_start, ng, vg, vb, signal_dst, occ_dst, x, stream);
}

extern "C" int qd_eval_points_response(qd_handle* h, const int32_t* group_env, const int64_t* group_start, int ng, const double* vg,
                                       const double* vb, const double* kT, double* signal_dst, double* occ_dst,
                                       const qd_response_opts* opts, void* stream) {
    if (!h) return QD_ERR_ARG;
    if (int rc = qd_check_kT_host(h, "qd_eval_points_response", kT, ng)) return rc;
    if (int rc = qd_check_struct_size(h, opts, sizeof(qd_response_opts), "qd_eval_points_response: opts->struct_size is not sizeof(qd_response_opts)")) return rc;
    QdBehindSearch x; x.kT = kT;
    if (opts) { x.gamma = opts->gamma_host; x.n_charge = opts->n_charge_host; x.var_dst = opts->var_dst; x.ztail_dst = opts->ztail_dst; }
    if (opts) { x.rd.chi = opts->chi_dst; x.rd.jac = opts->jac_dst; x.rd.dsignal = opts->dsignal_dst; }
    // (with no response destination the call is qd_eval_points_thermal, which takes such envs)
    for (int g = 0; group_env && x.response() && g < ng; ++g)
        if (group_env[g] >= 0 && group_env[g] < h->B && h->vc_on[(size_t)group_env[g]]) return qd_fail_vc(h, "qd_eval_points_response");
    return qd_points_run(h, "qd_eval_points_response", group_env, group_start, ng, vg, vb, signal_dst, occ_dst, x, stream);
}

// numpy 'linear' percentile ranks of n values, as qd_k_percentile takes them
static void qd_pct_ranks(long n, double q, long& ip, long& in, double& g) {
    const double virt = (double)(n - 1) * q, prev = floor(virt);
    ip = (long)prev; if (ip < 0) ip = 0; if (ip > n - 1) ip = n - 1;
    in = ip + 1; if (in > n - 1) in = n - 1;
    g = virt - prev;
}

// exact 0.5 / 99.5 percentiles of z[0..n) into plohi[0..1] (and plohi_dst when given), grid-wide radix select
static int qd_launch_select(qd_handle* h, const double* z, long n, double* plohi, double* plohi_dst, hipStream_t s) {
    long ip[2], in[2]; double g[2];
    qd_pct_ranks(n, 0.5 / 100.0, ip[0], in[0], g[0]);
    qd_pct_ranks(n, 99.5 / 100.0, ip[1], in[1], g[1]);
    // 8 values per thread and pass keep the per-block histogram flush (<= 512 atomics) a small part of the pass
    long blocks = (n + (long)QD_SEL_BLOCK * 8 - 1) / ((long)QD_SEL_BLOCK * 8);
    const long full = (long)h->cus * 8;
    if (blocks > full) blocks = full;
    if (blocks < 1) blocks = 1;
    qd_k_sel_init<<<dim3(1), dim3(512), 0, s>>>(h->sel.p, ip[0], ip[1]);
    for (int pass = 7; pass >= 0; --pass) {
        qd_k_sel_hist<<<dim3((unsigned)blocks), dim3(QD_SEL_BLOCK), 0, s>>>(z, n, pass, h->sel.p);
        qd_k_sel_pick<<<dim3(1), dim3(128), 0, s>>>(pass, h->sel.p);
    }
    qd_k_sel_rank<<<dim3((unsigned)blocks), dim3(QD_SEL_BLOCK), 0, s>>>(z, n, h->sel.p);
    qd_k_sel_finish<<<dim3(1), dim3(64), 0, s>>>(h->sel.p, ip[0], ip[1], in[0], in[1], g[0], g[1], plohi, plohi_dst);
    QD_HIP(hipGetLastError());
    return QD_OK;
}

// the composite's compact channel, per-scan percentiles and select state
static int qd_compose_scratch(qd_handle* h, size_t nq) {
    QD_HIP(h->cz.reserve(nq * (size_t)h->P));
    QD_HIP(h->cplohi.reserve(2 * nq));
    QD_HIP(h->sel.reserve(1));
    return QD_OK;
}

extern "C" int qd_probe_compose(qd_handle* h, const double* raw, int nx, int ny, int channel, int mode, float* composite_dst,
                                double* plohi_dst, void* stream) {
    if (!h) return QD_ERR_ARG;
    if (!raw || !composite_dst || nx < 1 || ny < 1) return qd_fail(h, QD_ERR_ARG, "qd_probe_compose: bad argument");
    if (channel < 0 || channel >= h->C) return qd_fail(h, QD_ERR_ARG, "qd_probe_compose: channel out of range");
    if (mode != QD_MAP_GLOBAL && mode != QD_MAP_PER_SCAN) return qd_fail(h, QD_ERR_ARG, "qd_probe_compose: unknown mode");
    if ((long long)nx * ny > 65535) return qd_fail(h, QD_ERR_ARG, "qd_probe_compose: more than 65535 scans");
    // (the select's histogram bins are 32-bit counters)
    if ((long long)nx * ny * h->P >= (1ll << 32)) return qd_fail(h, QD_ERR_ARG, "qd_probe_compose: nx*ny*P must stay below 2^32");
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    const long nq = (long)nx * ny, n = nq * h->P;
    // (a grown scratch is freed only after the stream work that used the old one: hipFree waits for the device)
    int rc = qd_compose_scratch(h, (size_t)nq);
    if (rc) return rc;
    {
        long blocks = (n + 1023) / 1024;
        if (blocks > (long)h->cus * 8) blocks = (long)h->cus * 8;
        qd_k_map_extract<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(raw, nq, h->C, h->P, channel, h->cz.p);
        QD_HIP(hipGetLastError());
    }
    const int per_scan = mode == QD_MAP_PER_SCAN ? 1 : 0;
    if (per_scan) {
        qd_launch_percentile(nullptr, (unsigned)nq, (long)h->P, h->cz.p, h->cplohi.p, s);
        QD_HIP(hipGetLastError());
    } else {
        rc = qd_launch_select(h, h->cz.p, n, h->cplohi.p, plohi_dst, s);
        if (rc) return rc;
    }
    qd_k_map_place<<<dim3((h->P + 255) / 256, (unsigned)nq), dim3(256), 0, s>>>(h->cz.p, nx, ny, h->R, per_scan, per_scan, h->cplohi.p,
                                                                               composite_dst, plohi_dst);
    QD_HIP(hipGetLastError());
    return QD_OK;
}

// Mean duration in milliseconds of a launch sequence on `s`: `rounds` times prep() untimed, then `reps` times timed() back to
// back between two events.  prep and timed return a QD_ code.
template <class Prep, class Timed>
static int qd_time_mean(const qd_handle* h, hipStream_t s, int rounds, int reps, Prep prep, Timed timed, float* mean_ms) {
    QdEventPair ev;
    if (!ev.ok) return qd_fail(h, QD_ERR_HIP, "hipEventCreate");
    float total = 0.f;
    for (int r = 0; r < rounds; ++r) {
        if (int rc = prep()) return rc;
        QD_HIP(hipEventRecord(ev.a.e, s));
        for (int i = 0; i < reps; ++i) if (int rc = timed()) return rc;
        QD_HIP(hipEventRecord(ev.b.e, s));
        QD_HIP(hipEventSynchronize(ev.b.e));
        float ms = 0.f;
        QD_HIP(hipEventElapsedTime(&ms, ev.a.e, ev.b.e));
        total += ms;
    }
    *mean_ms = total / ((float)rounds * (float)reps);
    return QD_OK;
}

// timing hook of scripts/probe_rate.py: the 0.5 / 99.5 percentiles of n caller-owned device doubles by the grid-wide select
// (single_block 0) or by one qd_k_percentile block (single_block 1); out_dev [2]
extern "C" int qd_time_select(qd_handle* h, const double* z_dev, long long n, int single_block, int iters, double* out_dev,
                              float* mean_ms, void* stream) {
    if (!h || !z_dev || n < 1 || n >= (1ll << 32) || iters < 1 || !out_dev || !mean_ms)
        return qd_fail(h, QD_ERR_ARG, "qd_time_select: bad argument");
    hipStream_t s = (hipStream_t)stream;
    QD_ON_DEVICE(h);
    QD_HIP(h->sel.reserve(1));
    return qd_time_mean(h, s, 1, iters, [] { return QD_OK; }, [&]() -> int {
        if (!single_block) return qd_launch_select(h, z_dev, (long)n, out_dev, nullptr, s);
        qd_launch_percentile(nullptr, 1, (long)n, z_dev, out_dev, s);
        QD_HIP(hipGetLastError());
        return QD_OK;
    }, mean_ms);
}

extern "C" int qd_get_state(qd_handle* h, double* state, int32_t* steps) {
    if (!h) return QD_ERR_ARG;
    QD_ON_DEVICE(h);
    QD_HIP(hipDeviceSynchronize());
    if (state) QD_HIP(hipMemcpy(state, h->state.p, sizeof(double) * (size_t)h->B * h->L.s_size, hipMemcpyDeviceToHost));
    if (steps) QD_HIP(hipMemcpy(steps, h->steps.p, sizeof(int) * (size_t)h->B, hipMemcpyDeviceToHost));
    return QD_OK;
}
extern "C" int qd_set_state(qd_handle* h, const double* state, const int32_t* steps) {
    if (!h) return QD_ERR_ARG;
    QD_ON_DEVICE(h);
    QD_HIP(hipDeviceSynchronize());
    if (state) QD_HIP(hipMemcpy(h->state.p, state, sizeof(double) * (size_t)h->B * h->L.s_size, hipMemcpyHostToDevice));
    if (steps) QD_HIP(hipMemcpy(h->steps.p, steps, sizeof(int) * (size_t)h->B, hipMemcpyHostToDevice));
    return QD_OK;
}
extern "C" int qd_get_raw(qd_handle* h, double* raw, double* plohi) {
    if (!h) return QD_ERR_ARG;
    QD_ON_DEVICE(h);
    QD_HIP(hipDeviceSynchronize());
    if (raw) QD_HIP(hipMemcpy(raw, h->zraw.p, sizeof(double) * (size_t)h->B * h->C * h->P, hipMemcpyDeviceToHost));
    if (plohi) QD_HIP(hipMemcpy(plohi, h->plohi.p, sizeof(double) * 2 * (size_t)h->B, hipMemcpyDeviceToHost));
    return QD_OK;
}
extern "C" int qd_get_occupations(qd_handle* h, double* occ) {
    if (!h || !occ) return QD_ERR_ARG;
    if (!h->occ.p) return qd_fail(h, QD_ERR_STATE, "qd_get_occupations needs QD_FLAG_VALIDATE");
    QD_ON_DEVICE(h);
    QD_HIP(hipDeviceSynchronize());
    QD_HIP(hipMemcpy(occ, h->occ.p, sizeof(double) * (size_t)h->B * h->C * h->P * h->N, hipMemcpyDeviceToHost));
    return QD_OK;
}
extern "C" int qd_get_candidates(qd_handle* h, int32_t* states) {
    if (!h || !states) return QD_ERR_ARG;
    if (!(h->cfg.flags & QD_FLAG_VALIDATE)) return qd_fail(h, QD_ERR_STATE, "qd_get_candidates needs QD_FLAG_VALIDATE");
    if (h->full_m) return qd_fail(h, QD_ERR_ARG, "qd_get_candidates: the full charge-state space keeps no candidate list");
    QD_ON_DEVICE(h);
    QD_HIP(hipDeviceSynchronize());
    // records come over in bounded slices (64 MiB of host staging at most)
    const size_t nrec = (size_t)h->B * h->C * h->P;
    const size_t slice = ((size_t)64 << 20) / sizeof(QdPixelRec);
    QdPixelRec* host = (QdPixelRec*)malloc((nrec < slice ? nrec : slice) * sizeof(QdPixelRec));
    if (!host) return qd_fail(h, QD_ERR_NOMEM, "malloc");
    static const int DELTA[4] = {-1, 0, 1, 2};
    const int N = h->N;
    for (size_t r0 = 0; r0 < nrec; r0 += slice) {
        const size_t cnt = nrec - r0 < slice ? nrec - r0 : slice;
        hipError_t e_ = hipMemcpy(host, h->lanes[0].recs.p + r0, cnt * sizeof(QdPixelRec), hipMemcpyDeviceToHost);
        if (e_ != hipSuccess) { free(host); return qd_fail(h, QD_ERR_HIP, "hipMemcpy(recs)", e_); }
        // slots 0..K-1: the kept states (|0..0> padding from nvalid on); slots K..31: -1
        for (size_t r = 0; r < cnt; ++r) {
            const int nv = host[r].nvalid < h->kept ? host[r].nvalid : h->kept;
            for (int m = 0; m < QD_K; ++m)
                for (int i = 0; i < N; ++i) {
                    int v = -1;
                    if (m < h->kept) v = m < nv ? host[r].fl[i] + DELTA[(host[r].idx[m] >> (2 * (N - 1 - i))) & 3] : 0;
                    states[((r0 + r) * QD_K + m) * N + i] = v;
                }
        }
    }
    free(host);
    return QD_OK;
}

extern "C" int qd_get_eigen(qd_handle* h, double* eig) {
    if (!h || !eig) return QD_ERR_ARG;
    if (!h->eig.p) return qd_fail(h, QD_ERR_STATE, "qd_get_eigen needs QD_FLAG_VALIDATE");
    QD_ON_DEVICE(h);
    QD_HIP(hipDeviceSynchronize());
    QD_HIP(hipMemcpy(eig, h->eig.p, sizeof(double) * 2 * (size_t)h->B * h->C * h->P, hipMemcpyDeviceToHost));
    return QD_OK;
}

extern "C" int qd_get_search_stats(qd_handle* h, uint64_t* out16) {
    if (!h || !out16) return QD_ERR_ARG;
    if (!h->tstats.p) return qd_fail(h, QD_ERR_STATE, "qd_get_search_stats needs QD_FLAG_VALIDATE");
    QD_ON_DEVICE(h);
    QD_HIP(hipDeviceSynchronize());
    QD_HIP(hipMemcpy(out16, h->tstats.p, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost));
    return QD_OK;
}

extern "C" int qd_get_solver_stats(qd_handle* h, uint64_t* out16) {
    if (!h || !out16) return QD_ERR_ARG;
    if (!h->tstats.p) return qd_fail(h, QD_ERR_STATE, "qd_get_solver_stats needs QD_FLAG_VALIDATE");
    QD_ON_DEVICE(h);
    QD_HIP(hipDeviceSynchronize());
    QD_HIP(hipMemcpy(out16, h->tstats.p + 16, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost));
    return QD_OK;
}

extern "C" int qd_get_rng_state(const qd_handle* h, uint64_t* obs_serial) {
    if (!h || !obs_serial) return QD_ERR_ARG;
    *obs_serial = h->obs_serial;
    return QD_OK;
}
extern "C" int qd_set_rng_state(qd_handle* h, uint64_t obs_serial) {
    if (!h) return QD_ERR_ARG;
    h->obs_serial = obs_serial;
    return QD_OK;
}

// `rounds` x (`prep` stages untimed, then `reps` x the `timed` stages) of lane 0 on the first launch chunk of the envs
static int qd_time_stages(qd_handle* h, hipStream_t s, int rounds, int reps, int prep, int timed, float* mean_ms) {
    const QdEnvBufs b = qd_env_bufs(h);
    const int cnt = h->chunk < h->B ? h->chunk : h->B;
    return qd_time_mean(h, s, rounds, reps, [&] { return qd_launch_csd(h, b, h->lanes[0], nullptr, 0, cnt, s, prep); },
                        [&] { return qd_launch_csd(h, b, h->lanes[0], nullptr, 0, cnt, s, timed); }, mean_ms);
}

extern "C" int qd_time_ground_kernel(qd_handle* h, int iters, float* mean_ms, void* stream) {
    if (!h || iters < 1 || !mean_ms) return QD_ERR_ARG;
    QD_ON_DEVICE(h);
    return qd_time_stages(h, (hipStream_t)stream, 1, iters, 0, QD_ST_GROUND, mean_ms);
}

extern "C" int qd_time_candidates_kernel(qd_handle* h, int iters, float* mean_ms, void* stream) {
    if (!h || iters < 1 || !mean_ms) return QD_ERR_ARG;
    QD_ON_DEVICE(h);
    return qd_time_stages(h, (hipStream_t)stream, 1, iters, 0, QD_ST_SEARCH, mean_ms);
}

extern "C" const char* qd_timed_kernel_name(int k) {
    static const char* names[QD_TIMED_KERNELS] = {"qd_k_tile", "qd_k_candidates", "qd_k_gs_structure", "qd_k_gs_solve", "qd_k_gs_select"};
    return (k >= 0 && k < QD_TIMED_KERNELS) ? names[k] : "";
}

extern "C" int qd_time_kernels(qd_handle* h, int iters, float* mean_ms_out, void* stream) {
    if (!h || iters < 1 || !mean_ms_out) return QD_ERR_ARG;
    QD_ON_DEVICE(h);
    // (the redo pass consumes the tile search's flags and the solvers overwrite their input blocks: the producing kernel is
    // re-run, untimed, in front of each of their launches)
    static const int stage[QD_TIMED_KERNELS] = {QD_ST_TILE, QD_ST_REDO, QD_ST_STRUCTURE, QD_ST_SOLVE, QD_ST_SELECT};
    static const int producer[QD_TIMED_KERNELS] = {0, QD_ST_TILE, 0, QD_ST_STRUCTURE, 0};
    for (int k = 0; k < QD_TIMED_KERNELS; ++k) {
        mean_ms_out[k] = 0.f;                                            // a stage the handle does not have
        if (!(qd_stages(h) & stage[k])) continue;
        if (int rc = qd_time_stages(h, (hipStream_t)stream, iters, 1, producer[k], stage[k], &mean_ms_out[k])) return rc;
    }
    return QD_OK;
}

extern "C" int qd_chunk_envs(const qd_handle* h) { return h ? h->chunk : -1; }
