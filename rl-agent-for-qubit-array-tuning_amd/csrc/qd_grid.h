// qd_grid.h -- stateless 2-D scans on any nx x ny GRID of points along two direction vectors over the 2N controls
// (qd_scan_grid): the reference model layer's do2d_open(x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points) over
// GateVoltageComposer.do2d (GateVoltageComposer.py:224-255), which takes the two point counts from the caller.  A grid is a
// line's slot (qd_line.h) with two scalars: nx*ny points in a slot of its OWN size, Rl x Rl records with Rl =
// qd_line_side(nx*ny), record p = y*nx + x, the tail inert.  The front kernel here fills the records in the hand-over form
// of the tile search; the redo instantiation of the per-pixel search, the ground-state kernels, the telegraph chain, the
// sensor stage, the pack of qd_line.h and the percentile kernel then run on the slot with the geometry (Rl, Rl*Rl) as DATA:
// none of them is changed.  What a grid needs of its own: gather (around qd_slot_copy, qd_query.h), front and a latching walk
// that is reset at every row start (one lane per slot and row, rows of nx points); qd_k_query_write (qd_query.h) hands the
// packed rows out as [ny][nx].  qd_grid_voltages and qd_grid_record are __host__ __device__, so the CPU tier checks them
// (tests/hosttest_grid).
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
// the frame, vpp and tc by qd_control_voltages (qd_query.h), the tail of qd_affine_voltages.  With nx = ny =
// R these are the bits of qd_affine_voltages; with ny = 1 and dy = 0 those of qd_line_voltages (sy = y_lo is finite, and a
// sum with +-0 changes no bits but those of -0, as qd_line.h says of row 0 of an affine scan).
// ---------------------------------------------------------------------------
template <int N>
QD_HD void qd_grid_voltages(const double* par, const double* st, QdGridAxesPtr axes, int nx, int ny, int x, int y,
                            double* v_ext, double* vpp, double* tc) {
    constexpr int G = N + 1, V = 2 * N;
    const QdLayout L = qd_layout(N);
    const double sx = qd_linspace(axes->x_lo, axes->x_hi, nx, x);
    const double sy = qd_linspace(axes->y_lo, axes->y_hi, ny, y);
    double W[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const double w0 = i < N ? st[L.s_gate_v + i] : (i == N ? st[L.s_sensor_gt] : st[L.s_barrier_v + (i - G)]);
        W[i] = fma(sy, axes->dy[i], fma(sx, axes->dx[i], w0));
    }
    qd_control_voltages<N>(par, st, axes->frame, W, v_ext, vpp, tc);
}

// ---------------------------------------------------------------------------
// Record j of a slot: point (j / nx, j % nx) of the grid (true: vpp and tc are in the record, vd, ncont and isa come back for
// the hand-over), or, from nx*ny on, the inert all-zero record of a line's slot (false): qd_slot_record (qd_line.h).
// ---------------------------------------------------------------------------
template <int N>
QD_HD bool qd_grid_record(const double* par, const double* st, QdGridAxesPtr axes, int nx, int ny, int j, QdPixelRec* rec,
                          double* v_ext, double* vd, double* ncont, double* isa) {
    return qd_slot_record<N>(par, j < nx * ny, rec, v_ext, vd, ncont, isa, [&](double* ve, double* vpp, double* tc) {
        const int y = j / nx;
        qd_grid_voltages<N>(par, st, axes, nx, ny, j - y * nx, y, ve, vpp, tc);
    });
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

#define QD_GRID_BLOCK 128
// slots in flight per launch at the most (qdsim.h: QD_GRID_SLOTS), as a line's
#define QD_GRID_MAX_SLOTS QD_LINE_MAX_SLOTS

// ---------------------------------------------------------------------------
// gather: slot k (query base + k) <- parameter and state block of env env_of_query[base + k] with the query applied
// (qd_slot_copy, qd_query.h: the base point, the virtual gate matrix, the constant peak width); axes[k] <- ranges,
// directions, counts and frame.  The Kalman block is copied as it is: the descriptor reaches the front kernel as an
// argument, and no kernel behind it reads the block.  A query that is not live renders a clamped env (the write kernel
// skips it).  grid = cnt, block = QD_GRID_BLOCK.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(QD_GRID_BLOCK)
qd_k_grid_gather(QdAffineQuery Q, int base, int B, int N, int nx, int ny, const double* __restrict__ params,
                 const double* __restrict__ state, double* __restrict__ sparams, double* __restrict__ sstate,
                 QdGridAxes* __restrict__ axes) {
    const int k = blockIdx.x, q = base + k, V = 2 * N;
    qd_slot_copy<QD_GRID_BLOCK>(Q, q, k, B, qd_layout(N), params, state, sparams, sstate, 0);
    QdGridAxes* A = axes + k;
    for (int i = threadIdx.x; i < 2 * QD_MAXN; i += QD_GRID_BLOCK) {
        A->dx[i] = i < V ? Q.dir[((size_t)q * 2 + 0) * V + i] : 0.0;
        A->dy[i] = i < V ? Q.dir[((size_t)q * 2 + 1) * V + i] : 0.0;
    }
    if (threadIdx.x == 0) {
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

#endif  // __HIPCC__
