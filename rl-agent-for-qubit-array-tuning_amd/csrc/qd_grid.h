// qd_grid.h -- stateless 2-D scans on any nx x ny GRID of points along two direction vectors over the 2N controls
// (qd_scan_grid): the reference model layer's do2d_open(x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points) over
// GateVoltageComposer.do2d (GateVoltageComposer.py:224-255), which takes the two point counts from the caller.  A grid is a
// line's slot (qd_line.h) with two scalars: nx*ny points in a slot of its OWN size, Rl x Rl records with Rl =
// qd_line_side(nx*ny), record p = y*nx + x, the tail inert.  The front kernel here fills the records in the hand-over form
// of the tile search; the redo instantiation of the per-pixel search, the ground-state kernels, the telegraph chain, the
// sensor stage, the pack of qd_line.h and the percentile kernel then run on the slot with the geometry (Rl, Rl*Rl) as DATA:
// none of them is changed.  What a grid needs of its own: gather, front, a latching walk that is reset at every row start
// (one lane per slot and row, rows of nx points) and the write.  qd_grid_voltages and qd_grid_record are __host__ __device__,
// so the CPU tier checks them (tests/hosttest_grid).
#pragma once
#include "qd_line.h"
#include "qd_latch.h"

// the descriptor of one grid in flight, in a buffer of its own (one per slot)
struct QdGridAxes {
    double x_lo, x_hi, y_lo, y_hi;                               // ranges of the two scalars sx, sy
    double dx[2 * QD_MAXN], dy[2 * QD_MAXN];                     // directions over the controls, the first 2N of each
    int32_t nx, ny, frame, pad;
};

// The descriptor is uniform over a block and constant while the front kernel runs (the gather kernel before it wrote it), so
// on the device its address is taken as one into the constant address space, as QdAffineAxesPtr (qd_pixel.h): ranges,
// directions and counts arrive through scalar loads.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) QdGridAxes* QdGridAxesPtr;
#else
typedef const QdGridAxes* QdGridAxesPtr;
#endif

// ---------------------------------------------------------------------------
// Front end of point (row y, column x) of an nx x ny grid: sx = linspace(x_lo, x_hi, nx)[x], sy = linspace(y_lo, y_hi, ny)[y]
// and, with W0[2N] = [gate_v, sensor_v, barrier_v] of the state block,  W[i] = fma(sy, dy[i], fma(sx, dx[i], W0[i]));  then
// the frame, vpp and tc exactly as the tail of qd_affine_voltages: same operations, same order, same fences.  With nx = ny =
// R these are the bits of qd_affine_voltages; with ny = 1 and dy = 0 those of qd_line_voltages (sy = y_lo is finite, and a
// sum with +-0 changes no bits but those of -0, as qd_line.h says of row 0 of an affine scan).
// ---------------------------------------------------------------------------
template <int N>
QD_HD void qd_grid_voltages(const double* par, const double* st, QdGridAxesPtr axes, int nx, int ny, int x, int y,
                            double* v_ext, double* vpp, double* tc) {
    constexpr int G = N + 1, NB = N - 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
    const double* vgm = st + L.s_vgm;
    const double sx = qd_linspace(axes->x_lo, axes->x_hi, nx, x);
    const double sy = qd_linspace(axes->y_lo, axes->y_hi, ny, y);
    double W[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const double w0 = i < N ? st[L.s_gate_v + i] : (i == N ? st[L.s_sensor_gt] : st[L.s_barrier_v + (i - G)]);
        W[i] = fma(sy, axes->dy[i], fma(sx, axes->dx[i], w0));
    }
    if (axes->frame == QD_SCAN_PHYSICAL) {
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

// ---------------------------------------------------------------------------
// Record j of a slot: point (j / nx, j % nx) of the grid (true: vpp and tc are in the record, vd, ncont and isa come back for
// the hand-over), or, from nx*ny on, the inert all-zero record of a line's slot (false; qd_line_record).
// ---------------------------------------------------------------------------
template <int N>
QD_HD bool qd_grid_record(const double* par, const double* st, QdGridAxesPtr axes, int nx, int ny, int j, QdPixelRec* rec,
                          double* v_ext, double* vd, double* ncont, double* isa) {
    constexpr int G = N + 1, NB = N - 1;
    if (j >= nx * ny) {
        static_assert(sizeof(QdPixelRec) % 8 == 0, "the inert record is written in 64-bit words");
        unsigned long long* w = reinterpret_cast<unsigned long long*>(rec);
#pragma unroll
        for (int i = 0; i < (int)(sizeof(QdPixelRec) / 8); ++i) w[i] = 0ull;
        return false;
    }
    double vpp[G], tc[NB];
    const int y = j / nx;
    qd_grid_voltages<N>(par, st, axes, nx, ny, j - y * nx, y, v_ext, vpp, tc);
    qd_point_front<N>(par, v_ext, vpp, tc, vd, ncont, isa);
#pragma unroll
    for (int i = 0; i < G; ++i) rec->vpp[i] = vpp[i];
#pragma unroll
    for (int b = 0; b < NB; ++b) rec->tc[b] = tc[b];
    return true;
}

// ---------------------------------------------------------------------------
// Row y of the latching walk of a grid, in place: qd_latch_row as it is on the nx records from y*nx of the slot (row = y, R =
// nx, channel 0), so the held state is reset at every row start and the Philox counter of a point is y*nx + x.  occ [SP][N]
// and z [SP] of ONE slot; (y + 1) * nx <= nx*ny <= SP.
// ---------------------------------------------------------------------------
template <int N>
QD_HD void qd_grid_latch_row(const double* par, const QdLayout& L, double* occ, double* z, int nx, int y, uint32_t seed,
                             uint32_t ser_lo, uint32_t ser_hi, uint32_t k1) {
    const size_t p0 = (size_t)y * nx;
    qd_latch_row<N>(par, L, occ + p0 * N, z + p0, y, nx, 0, seed, ser_lo, ser_hi, k1);
}

#if defined(__HIPCC__)
#include "qd_affine.h"

#define QD_GRID_BLOCK 128
// slots in flight per launch at the most (qdsim.h: QD_GRID_SLOTS), as a line's
#define QD_GRID_MAX_SLOTS QD_LINE_MAX_SLOTS

// ---------------------------------------------------------------------------
// gather: slot k (query base + k) <- parameter and state block of env env_of_query[base + k] with the base point, the
// virtual gate matrix and the peak width of the query applied as qd_k_affine_gather applies them (constant width: scal[1] =
// the query's gamma or the env's constant, scal[3] = -1); axes[k] <- ranges, directions, counts and frame.  The Kalman block
// is copied as it is: the descriptor reaches the front kernel as an argument, and no kernel behind it reads the block.  A
// query that is not live renders a clamped env (the write kernel skips it).  grid = cnt, block = QD_GRID_BLOCK.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(QD_GRID_BLOCK)
qd_k_grid_gather(QdAffineQuery Q, int base, int B, int N, int nx, int ny, const double* __restrict__ params,
                 const double* __restrict__ state, double* __restrict__ sparams, double* __restrict__ sstate,
                 QdGridAxes* __restrict__ axes) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.x, q = base + k, nb = N - 1, G = N + 1, V = 2 * N;
    int e = Q.env_of_query[q];
    e = e < 0 ? 0 : (e >= B ? B - 1 : e);
    const double* par = params + (size_t)e * L.size;
    const double* st = state + (size_t)e * L.s_size;
    double* dp = sparams + (size_t)k * L.size;
    double* ds = sstate + (size_t)k * L.s_size;
    QdGridAxes* A = axes + k;
    for (int i = threadIdx.x; i < L.s_size; i += QD_GRID_BLOCK) {
        double v = st[i];
        if (i >= L.s_vgm && i < L.s_vgm + G * G) { if (Q.vgm) v = Q.vgm[(size_t)q * G * G + (i - L.s_vgm)]; }
        else if (i >= L.s_gate_v && i < L.s_gate_v + N) v = Q.gate_v[(size_t)q * N + (i - L.s_gate_v)];
        else if (i >= L.s_barrier_v && i < L.s_barrier_v + nb) v = Q.barrier_v[(size_t)q * nb + (i - L.s_barrier_v)];
        else if (i == L.s_sensor_gt) v = Q.sensor_v ? Q.sensor_v[q] : 0.0;      // sensor_voltage=None -> 0.0
        ds[i] = v;
    }
    for (int i = threadIdx.x; i < L.size; i += QD_GRID_BLOCK) if (i != L.scal + 1 && i != L.scal + 3) dp[i] = par[i];
    for (int i = threadIdx.x; i < 2 * QD_MAXN; i += QD_GRID_BLOCK) {
        A->dx[i] = i < V ? Q.dir[((size_t)q * 2 + 0) * V + i] : 0.0;
        A->dy[i] = i < V ? Q.dir[((size_t)q * 2 + 1) * V + i] : 0.0;
    }
    if (threadIdx.x == 0) {
        dp[L.scal + 1] = Q.gamma ? Q.gamma[q] : par[L.scal + 1];
        dp[L.scal + 3] = -1.0;
        A->x_lo = Q.range[4 * (size_t)q]; A->x_hi = Q.range[4 * (size_t)q + 1];
        A->y_lo = Q.range[4 * (size_t)q + 2]; A->y_hi = Q.range[4 * (size_t)q + 3];
        A->nx = nx; A->ny = ny; A->frame = Q.frame; A->pad = 0;
    }
}

// ---------------------------------------------------------------------------
// front end, one record per lane: record j of slot k (SP = Rl*Rl records) <- point j of the slot's grid in hand-over form,
// nvalid = QD_T_REDO: the redo pass searches it; from nx*ny on the inert record.  The counts are read from the slot's
// descriptor with its ranges, on the scalar path.  grid = (ceil(SP / block), slots).
// ---------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(QD_GRID_BLOCK)
qd_k_grid_front(int SP, const double* __restrict__ sparams, const double* __restrict__ sstate,
                const QdGridAxes* __restrict__ axes, QdPixelRec* __restrict__ recs) {
    const QdLayout L = qd_layout(N);
    const int k = blockIdx.y;
    const int j = blockIdx.x * QD_GRID_BLOCK + threadIdx.x;
    if (j >= SP) return;
    const QdGridAxesPtr A = (QdGridAxesPtr)(uintptr_t)(axes + k);
    QdPixelRec* rec = recs + (size_t)k * SP + j;
    double v_ext[2 * N], vd[N], ncont[N], isa;
    if (qd_grid_record<N>(sparams + (size_t)k * L.size, sstate + (size_t)k * L.s_size, A, A->nx, A->ny, j, rec, v_ext, vd, ncont, &isa))
        qd_tile_hand_over<N>(rec, vd, ncont, isa);
}

// ---------------------------------------------------------------------------
// latching, one lane per (slot, row): qd_grid_latch_row on row y of slot k.  occ [slots][SP][N], zraw [slots][SP].
// grid = ceil(slots * ny / 64), block = 64.
// ---------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(64)
qd_k_latch_grid(int n_slots, int nx, int ny, int SP, const double* __restrict__ sparams, double* __restrict__ occ,
                double* __restrict__ zraw, QdNoiseCfg nz) {
    const QdLayout L = qd_layout(N);
    const long t = (long)blockIdx.x * 64 + threadIdx.x;
    if (t >= (long)n_slots * ny) return;
    const int k = (int)(t / ny), y = (int)(t - (long)k * ny);
    qd_grid_latch_row<N>(sparams + (size_t)k * L.size, L, occ + (size_t)k * SP * N, zraw + (size_t)k * SP, nx, y, nz.seed, nz.ser_lo,
                         nz.ser_hi, nz.env_off + (uint32_t)k);
}

// ---------------------------------------------------------------------------
// write: slot k -> the caller's slot base + k.  n = nx*ny; raw [nq][ny][nx] float64, image [nq][ny][nx] float32 normalised
// with the grid's own percentiles (qd_norm), plohi [nq][2], occupations [nq][ny][nx][N] float64; each may be null.  Queries
// that are not live leave their slots untouched.  grid = (ceil(n / 256), cnt).
// ---------------------------------------------------------------------------
__global__ void qd_k_grid_write(QdAffineQuery Q, int base, int B, int N, int n, int SP, const double* __restrict__ dense,
                                const double* __restrict__ splohi, const double* __restrict__ socc, double* __restrict__ raw_dst,
                                float* __restrict__ image_dst, double* __restrict__ plohi_dst, double* __restrict__ occ_dst) {
    const int k = blockIdx.y, q = base + k;
    if (!qd_affine_live(Q, q, B)) return;
    const double lo = splohi[2 * k], hi = splohi[2 * k + 1];
    if (plohi_dst && blockIdx.x == 0 && threadIdx.x < 2) plohi_dst[2 * (size_t)q + threadIdx.x] = threadIdx.x ? hi : lo;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double z = dense[(size_t)k * n + p];
    if (raw_dst) raw_dst[(size_t)q * n + p] = z;
    if (image_dst) image_dst[(size_t)q * n + p] = qd_norm(z, lo, hi);
    if (occ_dst)
        for (int i = 0; i < N; ++i) occ_dst[((size_t)q * n + p) * N + i] = socc[((size_t)k * SP + p) * N + i];
}

#endif  // __HIPCC__
