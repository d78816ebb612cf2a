// qd_groundstate.h -- ground state of H = diag(F) + H_t over the K kept charge states of a pixel (K = num_charge_states,
// 1..32, default 32; reference: hamiltonian_build.py:12-45, 75-137, 460-483 and
// ground_state.py:149-162, where a dense K x K eigh is called per pixel and only column 0 is used).  The candidate
// stage hands over a list of KC >= K states (KC = 8, 16, 32), in (E, idx) order whenever K < KC; the first K slots are
// the kept states and nothing here reads a slot >= K.
//
// Three kernels per launch chunk (qd_kernels.h), the image cut into batches of QD_GS_PPB pixels with one slab of
// scratch per batch:
//
//   A  STRUCTURE (qd_k_gs_structure), one pixel per half-wave, one basis state per lane (qd_ground_structure):
//      hop neighbours (states i, j couple over the adjacent pair d iff s_j - s_i = -+e_d +-e_{d+1}; with 4-bit-spaced
//      delta codes that is a plain integer difference of +-15 << 4q: qd_gs_hop), coefficients
//      H_ij = -t_d sqrt(n_from (n_to + 1)) with the occupations of the ROW state (hamiltonian_build.py:125-131),
//      connected components (hopping conserves the total charge, so H is block diagonal; the padding copies of
//      |0..0> are always isolated), Gershgorin pruning (a component whose lower bound min(F - sum|H_ij|) exceeds
//      an upper bound of the ground energy cannot hold the ground state; the upper bound: the lowest 2x2 pair
//      bound of the pixel, qd_gs_pair_bound).  Every surviving component of >= 2 states becomes a TASK: its dense
//      block is written, lower triangle packed, into the batch's slab and its offset appended to the list of its
//      size class; the batch's 64-task tiles are appended to the launch-wide tile list of the class.
//   B  SOLVE (qd_k_gs_solve<class>, one launch per size class with its own register budget), one TASK per lane
//      (qd_eig.h): Householder tridiagonalisation, Laguerre, twisted factorisation; 64 lanes = 64 different blocks
//      of the same size.  (Round 2 ran Lanczos + the serial tridiagonal recurrences with one state per lane: every
//      member lane of a component repeated the identical computation and a wave paid the maximum over its ~11
//      components; plain Lanczos also lost near-degenerate lowest pairs at tc >~ 1e14.)
//   C  SELECT (qd_k_gs_select), one pixel per lane (qd_ground_select): the component with the lowest eigenvalue wins
//      (ties: lowest candidate index), <n> = sum_m x_m^2 s_m, the sensor constant c0.
// Solving block by block is at least as accurate as one dense 32x32 eigh (no rounding-level mixing of different charge
// sectors); exactly-zero couplings do not link states, so tc == 0 gives exact integer occupations.
#pragma once
#include "qd_pixel.h"
#include "qd_eig.h"

#define QD_GS_PPB 256               // pixels per batch (4 waves x 32 iterations x 2 pixels)
// size classes: 2 .. 8 states exactly, 9-10 (solved as 10), 11-12 (as 12), 13-32 (memory solver)
#define QD_GS_NBIN 10
QD_HD constexpr int qd_gs_bin(int s) { return s <= 8 ? s - 2 : (s <= 10 ? 7 : (s <= 12 ? 8 : 9)); }
QD_HD constexpr int qd_gs_bin_min(int bin) { return bin <= 6 ? bin + 2 : (bin == 7 ? 9 : (bin == 8 ? 11 : 13)); }

// Hop test of two states.  ci, cj: their delta codes with one digit (0..3) per nibble, nibble q = dot N-1-q; tcq: bit 4q set
// iff the adjacent pair N-2-q couples.  cj - ci = sum d_k 16^k with |d_k| <= 3, and a base-16 representation with digits in
// -7..7 is unique, so |cj - ci| == 15 << 4q exactly when d_{q+1} = +-1, d_q = -+1 and every other digit agrees: one electron
// moved between the adjacent dots of pair N-2-q.  A difference 15 << tz with tz no multiple of 4 (30 = 2 * 16 - 2, ...) finds
// no bit in tcq.  Equal codes (the same state, the copies of the |0..0> padding): ay = 0, tz = 31, ay >> tz = 0, no hop.
QD_HD unsigned qd_gs_hop(unsigned ci, unsigned cj, unsigned tcq) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned ay;
    asm("v_sad_u32 %0, %1, %2, 0" : "=v"(ay) : "v"(ci), "v"(cj));
#else
    const unsigned ay = ci > cj ? ci - cj : cj - ci;
#endif
    const int tz = __builtin_ctz(ay | 0x80000000u);
    // x == 0 iff ay == 15 << tz (mod 2^32; -15 is odd, so ay = 0 with tz = 31 leaves x = 1 << 31); the verdict is the pair's
    // bit where x == 0 and 0 elsewhere, as a saturating t - x: branch-free on purpose (the compiler otherwise builds a
    // divergent branch per round), and free of compares
    const unsigned x = ay + (0xFFFFFFF1u << tz);
    const unsigned t = (tcq >> tz) & 1u;
    return t > x ? t - x : 0u;
}

// Pruning bound of the structure phase.  F: the diagonal relative to the pixel's lowest free energy (min F = 0).
//   upper bound of the ground energy   ub = min(0, min over the coupled pairs (i, j) of u_ij), u_ij = (F_i + F_j) / 2 - |H_ij|:
//       the 2x2 principal submatrix of the pair has the lowest eigenvalue m - sqrt(d^2 + c^2) <= m - |c| (m the mean, d half the
//       difference of its diagonal), and no eigenvalue of a principal submatrix lies below lambda_min(H) (interlacing); the 0 is
//       the 1x1 submatrix of the lowest state.  No square root: where many components survive the bound 0 (large tc) the
//       couplings dominate the differences of the diagonal and the full 2x2 eigenvalue prunes no further component.
//   margin   2^-40 ||H||_inf, ||H||_inf = max_i (F_i + radius_i) over the pixel's K states (shifted frame: F >= 0).
//   a component of >= 2 states is a task iff its Gershgorin lower bound min(F - radius) <= ub + margin.
// The margin covers the error bars of the eigen-solvers on the pruned component and on the one that attains ub (<= 2e-14 ||A||
// each) and the rounding of radius and u_ij (a few eps ||H||_inf): 2^-40 = 9.1e-13 is more than 20 times their sum.  So every
// component whose COMPUTED eigenvalue could be the lowest of the pixel, or tied for it, is still solved; a task's result does
// not depend on which other tasks exist; and the select phase sees the same winner, the same tie set and the same vector as
// with the bound 0.  Isolated states do not go through this test: qd_ground_select takes lambda = 0 for them, which is right
// iff F <= 0 (a positive margin would admit F > 0).
QD_HD double qd_gs_pair_bound(double Fi, double Fj, double c) { return __builtin_fma(0.5, Fi + Fj, -__builtin_fabs(c)); }
QD_HD double qd_gs_prune_margin(double hnorm) { return 0x1p-40 * hnorm; }
QD_HD bool qd_gs_is_task(double comp_lower, double ub, double margin) { return comp_lower <= ub + margin; }

#if defined(__HIPCC__)

#ifndef QD_NBREG
#define QD_NBREG 6                  // neighbour slots kept in registers; the other 2*(N-1) - 6 live in LDS (8 dots: 21 KB per block)
#endif
#define QD_GS_BLOCK 256
#define QD_LINK_NONE 0xFFFFFFFFu    // state whose component cannot hold the ground state (Gershgorin)
#define QD_LINK_SINGLE 0xFFFFFFFEu  // isolated state that can: T = [F]

// LDS-qualified volatile pointers: a plain `volatile double*` into __shared__ memory stays a generic
// pointer (address-space inference skips volatile accesses) and every access becomes a FLAT load;
// with the address space spelled out they are ds_read / ds_write.
typedef __attribute__((address_space(3))) double qd_lds_double;
typedef volatile qd_lds_double* qd_lds_vptr;
typedef const volatile qd_lds_double* qd_lds_cvptr;

template <int N>
struct QdWaveLds {
    static constexpr int NS = (2 * (N - 1) - QD_NBREG) > 1 ? (2 * (N - 1) - QD_NBREG) : 1;   // a state has at most 2*(N-1) hop neighbours
    double coef[NS][64];            // H_ij of neighbour slot QD_NBREG + s of lane
    unsigned char nidx[NS][64];
    double buf[64];                 // publish buffer for per-component reductions
    double pv[2][16];               // per half: tc[0..N-2] at offset 9; [0], [1]: upper bound and margin of the pruning test
    int pfl[2][8];                  // per half: floor(n_cont) (32 bits: a plunger at 3e4 V has floors beyond a short)
};
struct QdBlockLds {
    unsigned pool_top;              // bump allocator of the batch's slab (doubles)
    unsigned cnt[QD_GS_NBIN];       // tasks per size class
};

// One batch's scratch in HBM/L2:
//   pool   task records: [0] unused, [1] residual (out, validate mode; in: the size, for the padded / memory solvers),
//          [2 ..] packed lower triangle (in), overwritten by x[0..s-1] (out); blocks of > 12 states carry a 4 s workspace
//          (+ a copy of the matrix in validate mode)
//   link   per pixel and state: its component's position in `lists` (size classes back to back), QD_LINK_SINGLE or QD_LINK_NONE;
//          rank: index inside the component
//   lists  per size class: record offsets;  cnt: their lengths
//   lam    the tasks' eigenvalues, dense, same index as `lists`: written coalesced by the solve launches and read by the select
//          kernel with the locality of neighbouring pixels' tasks (reading them out of the records cost a 64-byte sector each)
//   aux    validate mode, per pixel: ||H||_inf (scale of the residual), then the lowest free energy (offset of the eigenvalues)
struct QdSlab {
    double* pool; unsigned* link; unsigned char* rank; unsigned* lists; double* aux; unsigned* cnt; double* lam;
};
// Lists of the size classes, back to back: class b can hold 32 / qd_gs_bin_min(b) tasks per pixel.  Capacities and offsets
// in units of QD_GS_PPB tasks, as tables packed into one word each (5 and 6 bits per class), so that the structure kernel,
// which looks the offset up with a run-time class, shifts a constant instead of summing the capacities with a division
// per class; the static_asserts below tie the tables to that definition.
constexpr int QD_GS_CAP_TAB[QD_GS_NBIN + 1] = {16, 10, 8, 6, 5, 4, 4, 3, 2, 2, 2};
constexpr int QD_GS_OFF_TAB[QD_GS_NBIN + 1] = {0, 16, 26, 34, 40, 45, 49, 53, 56, 58, 60};
constexpr unsigned long long qd_gs_pack_tab(const int* tab, int n, int bits) {
    unsigned long long w = 0;
    for (int b = 0; b < n; ++b) w |= (unsigned long long)tab[b] << (bits * b);
    return w;
}
constexpr unsigned long long QD_GS_CAP_WORD = qd_gs_pack_tab(QD_GS_CAP_TAB, QD_GS_NBIN + 1, 5);
constexpr unsigned long long QD_GS_OFF_WORD = qd_gs_pack_tab(QD_GS_OFF_TAB, QD_GS_NBIN, 6);     // (the total is not packed)
QD_HD constexpr int qd_gs_list_cap(int bin) { return QD_GS_PPB * (int)((QD_GS_CAP_WORD >> (5 * bin)) & 31u); }
QD_HD constexpr int qd_gs_list_off(int bin) {
    return QD_GS_PPB * (bin >= QD_GS_NBIN ? QD_GS_OFF_TAB[QD_GS_NBIN] : (int)((QD_GS_OFF_WORD >> (6 * bin)) & 63u));
}
constexpr bool qd_gs_lists_match_definition() {
    int o = 0;
    for (int b = 0; b <= QD_GS_NBIN; ++b) {
        if (qd_gs_list_off(b) != o || qd_gs_list_cap(b) != QD_GS_PPB * (32 / qd_gs_bin_min(b))) return false;
        o += QD_GS_PPB * (32 / qd_gs_bin_min(b));
    }
    return true;
}
static_assert(qd_gs_lists_match_definition(), "QD_GS_CAP_TAB / QD_GS_OFF_TAB: capacity 32 / qd_gs_bin_min(b) per pixel, offsets their running sum");
__host__ __device__ inline int qd_gs_task_doubles(int s, bool validate) {
    const int ne = s * (s + 1) / 2;
    const int n = 2 + ne + (s > QD_EIG_REG ? 4 * s + (validate ? ne : 0) : 0);
    return (n + 1) & ~1;                                  // records stay 16-byte aligned: the solvers load / store pairs of doubles
}
// worst case per pixel: one component of all 32 states
__host__ __device__ inline size_t qd_gs_pool_doubles(bool validate) { return (size_t)QD_GS_PPB * (size_t)qd_gs_task_doubles(32, validate); }
__host__ __device__ inline size_t qd_gs_slab_bytes(bool validate) {
    size_t b = qd_gs_pool_doubles(validate) * 8;
    b += (size_t)QD_GS_PPB * 32 * 4;                      // link
    b += (size_t)qd_gs_list_off(QD_GS_NBIN) * 4;          // lists
    b += (size_t)QD_GS_PPB * 16;                          // aux
    b += (size_t)QD_GS_PPB * 32;                          // rank
    b += 64;                                              // cnt
    b += (size_t)qd_gs_list_off(QD_GS_NBIN) * 8;          // lam
    return (b + 255) & ~(size_t)255;
}
__host__ __device__ inline QdSlab qd_gs_slab(unsigned char* base, bool validate) {
    QdSlab s;
    s.pool = (double*)base; base += qd_gs_pool_doubles(validate) * 8;
    s.link = (unsigned*)base; base += (size_t)QD_GS_PPB * 32 * 4;
    s.lists = (unsigned*)base; base += (size_t)qd_gs_list_off(QD_GS_NBIN) * 4;
    s.aux = (double*)base; base += (size_t)QD_GS_PPB * 16;
    s.rank = base; base += (size_t)QD_GS_PPB * 32;
    s.cnt = (unsigned*)base; base += 64;
    s.lam = (double*)base;
    return s;
}
// launch-wide tile lists: tile descriptor = batch << 12 | tile index inside the batch's list << 6 | tasks in the tile - 1
__host__ __device__ inline size_t qd_gs_tile_cap(int bin, size_t batches) { return batches * (size_t)((qd_gs_list_cap(bin) + 63) / 64); }
__host__ __device__ inline size_t qd_gs_tile_off(int bin, size_t batches) { size_t o = 0; for (int b = 0; b < bin; ++b) o += qd_gs_tile_cap(b, batches); return o; }

__device__ __forceinline__ unsigned qd_half_ballot(bool p) {
    unsigned long long b = __ballot(p);
    return (unsigned)(b >> (threadIdx.x & 32));
}
// Minimum over the half-wave, in every lane.  Inside a row of 16 lanes the exchange is done by DPP modifiers (a few cycles each,
// where a ds_bpermute round trip through the LDS crossbar costs a dependent ~100): lane ^ 1 and lane ^ 2 as quad permutations;
// then the quads are uniform, and mirroring the 8 lanes (lane i reads 7 - i) hands each quad the other quad's value; then the
// mirror of the 16.  Only the last step, between the two rows of the half, goes through the crossbar.  All 64 lanes are on
// (as for qd_half_rot).  A minimum does not depend on the order, so the result is that of the __shfl_xor butterfly.
#ifndef QD_GS_MIN_DPP
#define QD_GS_MIN_DPP 1             // 0: the butterfly with __shfl_xor alone (diagnostic)
#endif
template <int CTRL>
__device__ __forceinline__ double qd_dpp_f64(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false),
                            __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ double qd_half_min(double v) {
#if QD_GS_MIN_DPP
    v = fmin(v, qd_dpp_f64<0xB1>(v));                      // quad_perm [1, 0, 3, 2]
    v = fmin(v, qd_dpp_f64<0x4E>(v));                      // quad_perm [2, 3, 0, 1]
    v = fmin(v, qd_dpp_f64<0x141>(v));                     // row_half_mirror
    v = fmin(v, qd_dpp_f64<0x140>(v));                     // row_mirror
    return fmin(v, __shfl_xor(v, 16, 32));
#else
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 32));
    return v;
#endif
}
// wave-wide maximum, returned through readfirstlane so that the compiler knows it is uniform: loop bounds
// and slot guards built from it become scalar branches instead of exec-mask juggling
__device__ __forceinline__ int qd_wave_max_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return __builtin_amdgcn_readfirstlane(v);
}

// v of lane (m + J) mod 32 (UP) or (m - J) mod 32 (!UP) of the same half-wave, J a constant: ds_swizzle in rotate mode moves
// the data without an address register (a __shfl spends three instructions on the ds_bpermute address of every round).
// A swizzle reads 0 from a lane that is switched off: the caller runs with all 64 lanes on -- the two halves of a wave work
// in lock step and the clamped duplicate beyond the image is computed, not switched off.
#ifndef QD_GS_ROT_SWIZZLE
#define QD_GS_ROT_SWIZZLE 1         // 0: the same exchange with __shfl (diagnostic)
#endif
template <int J, bool UP>
__device__ __forceinline__ unsigned qd_half_rot(unsigned v) {
#if QD_GS_ROT_SWIZZLE
    return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0xC000 | ((UP ? 0 : 1) << 10) | (J << 5));
#else
    return (unsigned)__shfl((int)v, ((int)(threadIdx.x & 31) + (UP ? J : 32 - J)) & 31, 32);
#endif
}
// rounds J .. 16 of the all-pairs hop test (qd_ground_structure, phase 2), unrolled at compile time
template <int J>
__device__ __forceinline__ void qd_gs_hop_rounds(unsigned ecode, unsigned tcq, unsigned& acc) {
    const unsigned hop = qd_gs_hop(ecode, qd_half_rot<J, true>(ecode), tcq);
    acc |= hop << J;
    if constexpr (J < 16) {                                // (round 16 pairs m with m + 16 from both sides already)
        acc |= qd_half_rot<J, false>(hop) << (32 - J);
        qd_gs_hop_rounds<J + 1>(ecode, tcq, acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Phase A.  rec: this half's pixel record (states, their free energies from the candidate search, tunnel couplings);
// ps: the pixel's slot in the batch; live: false for the clamped duplicate beyond the image (nothing is emitted);
// kept: K, the states of the Hamiltonian (lanes m >= K take no part: their link is QD_LINK_NONE); bound0: prune against
// min F = 0 alone (QD_FLAG_GS_GERSHGORIN_ZERO, the same for the whole launch).
// ---------------------------------------------------------------------------------------------------------------
template <int N, bool VALIDATE>
__device__ __forceinline__ void qd_ground_structure(const QdPixelRec* __restrict__ rec, bool live, int ps, QdWaveLds<N>& W,
                                                    QdBlockLds& S, const QdSlab& sl, int kept, bool bound0) {
    const int lane = threadIdx.x & 63;
    const int m = lane & 31;
    const int hb = lane & 32;
    const unsigned lt = (1u << m) - 1u;
    qd_lds_vptr buf = (qd_lds_vptr)W.buf;

    // ---- 1. my state -------------------------------------------------------
    // pixel-uniform record fields go through LDS once (keeps them out of registers)
    const int hh = hb >> 5;
    if (m >= 9 && m < 9 + N - 1) W.pv[hh][m] = rec->tc[m - 9];
    if (m >= 16 && m < 16 + N) W.pfl[hh][m - 16] = rec->fl[m - 16];
    __builtin_amdgcn_wave_barrier();
    const double* pvv = W.pv[hh];
    const bool inK = m < kept;
    const int nvalid = min(rec->nvalid, kept);
    const bool valid = m < nvalid;
    const unsigned code = valid ? (unsigned)rec->idx[m] : 0u;
    // digit of dot i (base 4, dot 0 most significant) -> nibble N-1-i of ecode: spread the 2-bit digits to 4-bit spacing
    unsigned ecode = code;
    ecode = (ecode | (ecode << 8)) & 0x00FF00FFu;
    ecode = (ecode | (ecode << 4)) & 0x0F0F0F0Fu;
    ecode = (ecode | (ecode << 2)) & 0x33333333u;
    // F_m: the candidate search already evaluated the canonical energy of every kept state, and of the |0..0> padding
    // when fewer than K candidates are valid.  The diagonal enters RELATIVE to the pixel's lowest free energy:
    // H - c I has the same eigenvectors, and the common offset (|F| ~ 1e3..1e5 far from the ground truth, against
    // spreads of O(1)) would cost ~eps |F| in every subtraction.
    const double Fabs = inK ? rec->E[m] : INFINITY;                // (a state beyond K: no part in H, never active)
    const double fshift = qd_half_min(Fabs);
    const double F = Fabs - fshift;

    // ---- 2. hop neighbours -------------------------------------------------
    // pairs whose coupling is exactly zero do not link states (keeps the classical
    // limit tc == 0 exactly diagonal, as a dense eigh of a diagonal matrix would)
    unsigned tcnz = 0;
#pragma unroll
    for (int d = 0; d < N - 1; ++d) tcnz |= (pvv[9 + d] != 0.0 ? 1u : 0u) << d;
    unsigned tcq = 0;                                     // bit 4q set iff pair N-2-q couples (nibble q of ecode is the digit of dot N-1-q)
#pragma unroll
    for (int q = 0; q < N - 1; ++q) tcq |= ((tcnz >> (N - 2 - q)) & 1u) << (4 * q);
    // The relation is symmetric, so every pair is tested once: in round j lane m tests its partner (m + j) mod 32 and hands the
    // verdict to that partner as well (which receives it from lane (m - j) mod 32) -- 16 rounds instead of 32 tests per lane.
    // Both exchanges are rotations of the half-wave by the constant j (qd_half_rot).  The verdicts are collected in the frame
    // of the lane, bit b = partner (m + b) mod 32, with constant shifts, and rotated into place once at the end.
    unsigned acc = 0;
    qd_gs_hop_rounds<1>(ecode, tcq, acc);
    unsigned nbrmask = __builtin_rotateleft32(acc, (unsigned)m);
    // states beyond the valid count (|0..0> padding, and everything from slot K on) neither hop nor are hopped to
    nbrmask = (valid && live) ? (nbrmask & (nvalid >= 32 ? 0xFFFFFFFFu : ((1u << nvalid) - 1u))) : 0u;
#if defined(QD_ABLATE) && QD_ABLATE == 4
    nbrmask = 0;                                          // diagnostic: no hopping at all
#endif
    const int cnt = __popc(nbrmask);
    const int maxcnt = qd_wave_max_int(cnt);
    double radius = 0.0;
    double ubl = 0.0;                                      // min(0, my pairs' u_ij): see qd_gs_pair_bound
    double creg[QD_NBREG];
    unsigned jpack = 0;                                    // the neighbours of the register slots, 5 bits each
    static_assert(5 * QD_NBREG <= 32, "jpack: 5 bits per register slot");
#pragma unroll
    for (int i = 0; i < QD_NBREG; ++i) creg[i] = 0.0;
    {
        buf[lane] = F;                                     // (a neighbour is a valid state: its F is finite)
        __builtin_amdgcn_wave_barrier();
        unsigned rem = nbrmask;
        for (int s = 0; s < maxcnt; ++s) {
            const bool has = rem != 0;
            const int j = has ? __builtin_ctz(rem) : m;
            rem &= rem - 1;
            const unsigned cj = __shfl(ecode, j, 32);
            double c = 0.0;
            if (has) {
                const int Y = (int)cj - (int)ecode;
                const unsigned ay = (unsigned)(Y < 0 ? -Y : Y);
                const int q = __builtin_ctz(ay) >> 2;
                const int d = N - 2 - q;                   // adjacent pair (d, d+1)
                // occupations of the pair's two dots straight from the code's digits and the floors in LDS
                const int nd = W.pfl[hh][d] + (int)((ecode >> (4 * (q + 1))) & 3u) - 1;
                const int nd1 = W.pfl[hh][d + 1] + (int)((ecode >> (4 * q)) & 3u) - 1;
                const double t = pvv[9 + d];
                // Y < 0: s_j = s_i - e_d + e_{d+1} (forward); else backward
                // (integers below 2^26: the float64 product is exact, where the 32-bit one overflows from 46341 electrons on)
                const double prod = (Y < 0) ? (double)nd * (double)(nd1 + 1) : (double)nd1 * (double)(nd + 1);
                double sq_ = 0.0;
                if (prod > 0.0) sq_ = qd_sqrt1(prod);
                c = -t * sq_;
                ubl = fmin(ubl, qd_gs_pair_bound(F, buf[hb + j], c));
            }
            if (s < QD_NBREG) {                            // (s is uniform: scalar branches)
#pragma unroll
                for (int i = 0; i < QD_NBREG; ++i) if (i == s) creg[i] = c;
                jpack |= (unsigned)j << (5 * s);
            } else { W.coef[s - QD_NBREG][lane] = c; W.nidx[s - QD_NBREG][lane] = (unsigned char)j; }
            radius += fabs(c);
        }
        // the pixel's upper bound and margin (qd_gs_pair_bound), parked in LDS over phase 3 like the other pixel-uniform values
        if (!bound0) {                                     // (uniform for the block)
            const double ub = qd_half_min(ubl);
            const double hnorm = -qd_half_min(inK ? -(F + radius) : 0.0);    // (lanes beyond K have F = inf and no part in H)
            if (m == 0) { W.pv[hh][0] = ub; W.pv[hh][1] = qd_gs_prune_margin(hnorm); }
        }
    }

    // ---- 3. connected components (reach masks) -----------------------------
    unsigned seg = (1u << m) | nbrmask;
    for (int guard = 0; guard < 32; ++guard) {
        unsigned nw = seg, rem = nbrmask;
        for (int s = 0; s < maxcnt; ++s) {
            const bool has = rem != 0;
            const int j = has ? __builtin_ctz(rem) : m;
            rem &= rem - 1;
            nw |= __shfl(seg, j, 32);                     // (own mask for exhausted lanes: no change)
        }
        const bool changed = nw != seg;
        seg = nw;
        if (!__any(changed)) break;
    }
    const int ssz = __popc(seg);
    const int r = __popc(seg & lt);                        // my index inside the component
    const int smax = qd_wave_max_int(ssz);

    // ---- 4. Gershgorin pruning ---------------------------------------------
    // A component whose lower bound min(F - radius) exceeds an upper bound of the pixel's ground energy cannot hold the ground
    // state.  Components of >= 2 states: the pair bound with its margin (qd_gs_pair_bound); bound0 (QD_FLAG_GS_GERSHGORIN_ZERO,
    // uniform for the block): min F = 0, as for the isolated states in either case.
    double comp_lower;
    {
        __builtin_amdgcn_wave_barrier();                   // (the loop of phase 2 read the F of other lanes from buf)
        buf[lane] = F - radius;
        __builtin_amdgcn_wave_barrier();
        double acc = INFINITY;
        unsigned mm = seg;
        for (int it = 0; it < smax; ++it) {
            if (mm) { const int b = __builtin_ctz(mm); mm &= mm - 1; acc = fmin(acc, buf[hb + b]); }
        }
        __builtin_amdgcn_wave_barrier();
        comp_lower = acc;
    }
    bool active = live && comp_lower <= 0.0;
    if (!bound0 && ssz > 1) active = live && qd_gs_is_task(comp_lower, pvv[0], pvv[1]);
#if defined(QD_ABLATE) && QD_ABLATE == 3
    const bool solve = false;                              // diagnostic: no tasks
#else
    const bool solve = active && ssz > 1;
#endif
    // trip count of the zero fill below: the largest component that is written (a pruned one writes no block, takes no list
    // slot and its states are linked to nothing)
    const int smax_solve = qd_wave_max_int(solve ? ssz : 0);

    // ---- 5. tasks: one record per surviving component ------------------------
    unsigned base = 0, gi = 0;
    if (solve && r == 0) {
        base = atomicAdd(&S.pool_top, (unsigned)qd_gs_task_doubles(ssz, VALIDATE));
        const int bin = qd_gs_bin(ssz);
        gi = (unsigned)qd_gs_list_off(bin) + atomicAdd(&S.cnt[bin], 1u);
        sl.lists[gi] = base;
        if (ssz > 8) sl.pool[base + 1] = (double)ssz;
    }
    base = (unsigned)__shfl((int)base, __builtin_ctz(seg), 32);
    gi = (unsigned)__shfl((int)gi, __builtin_ctz(seg), 32);
    if (live) {
        sl.link[ps * 32 + m] = solve ? gi : (active ? QD_LINK_SINGLE : QD_LINK_NONE);
        sl.rank[ps * 32 + m] = (unsigned char)r;
        if (VALIDATE) {
            const double hn = -qd_half_min(inK ? -(fabs(Fabs) + radius) : INFINITY);   // ||H||_inf over the K states (unshifted)
            if (m == 0) { sl.aux[ps] = hn; sl.aux[QD_GS_PPB + ps] = fshift; }
        }
    }
    {
        // my row of the lower triangle: couplings to members of lower rank, zeros elsewhere, F on the diagonal
        double* row = sl.pool + base + 2 + (r * (r + 1)) / 2;
        unsigned nrm = 0;                                  // ranks that carry a coupling
        for (int s = 0; s < maxcnt; ++s) {
            if (s < cnt && solve) {
                int j; double c = creg[0];
                if (s >= QD_NBREG) { j = (int)W.nidx[s - QD_NBREG][lane]; c = W.coef[s - QD_NBREG][lane]; }
                else j = (int)((jpack >> (5 * s)) & 31u);
#pragma unroll
                for (int i = 1; i < QD_NBREG; ++i) if (i == s) c = creg[i];
                const int rj = __popc(seg & ((1u << j) - 1u));
                if (rj < r) { row[rj] = c; nrm |= 1u << rj; }
            }
        }
        for (int c = 0; c < smax_solve - 1; ++c)
            if (solve && c < r && !((nrm >> c) & 1u)) row[c] = 0.0;
        if (solve) row[r] = F;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Phase B: one task per lane.  rec: the task's record in the slab.  Returns the Laguerre iterations (statistics).
// ---------------------------------------------------------------------------------------------------------------
template <int S, bool PADDED, bool VALIDATE>
__device__ __forceinline__ int qd_eig_task(double* rec, double& lam) {
    double resid, x[S];
    int its = 0;
    const int sz = PADDED ? (int)rec[1] : S;
    qd_eig_lowest<S, VALIDATE>(rec + 2, lam, x, resid, VALIDATE ? &its : nullptr, sz);
    if (VALIDATE) rec[1] = resid;                          // (the eigenvalue goes to the slab's dense array: qd_k_gs_solve)
    if (sz == S) {
        double2* X2 = reinterpret_cast<double2*>(rec + 2);
#pragma unroll
        for (int i = 0; i + 1 < S; i += 2) X2[i >> 1] = make_double2(x[i], x[i + 1]);
        if (S & 1) rec[2 + S - 1] = x[S - 1];
    } else {
#pragma unroll
        for (int i = 0; i < S; ++i) if (i < sz) rec[2 + i] = x[i];
    }
    return its;
}
// Blocks of 13..32 states (0.1 % of the pixels have one): the same algorithm with run-time loops in the task's record -- a serial
// O(s^3) chain of dependent memory operations, ~1 ms per wave whatever the batch, run on a side stream.  Measured and not kept
// (bench, env-steps/s; this version 11 500-11 600): solving blocks of <= 16 states in an LDS tile ([element][lane], 100 KB per
// wave, one wave per CU): 11 000-11 100 (a tenth of the latency per operation, a twentieth of the waves in flight); listing the
// class's single tasks launch-wide so that its waves are full: 11 400 (64 different records per memory instruction).
template <bool VALIDATE>
__device__ __forceinline__ int qd_eig_task_mem(double* rec, double& lam) {
    const int s = (int)rec[1];
    const int ne = s * (s + 1) / 2;
    double* M = rec + 2;
    double* work = M + ne;
    double* copy = VALIDATE ? work + 4 * s : nullptr;
    if (VALIDATE) for (int e = 0; e < ne; ++e) copy[e] = M[e];
    double resid;
    int its = 0;
    qd_eig_lowest_mem(s, M, work, copy, lam, resid, VALIDATE ? &its : nullptr);
    if (VALIDATE) rec[1] = resid;                          // (the eigenvalue goes to the slab's dense array: qd_k_gs_solve)
    for (int i = 0; i < s; ++i) M[i] = work[3 * s + i];
    return its;
}

// ---------------------------------------------------------------------------------------------------------------
// Phase C: one pixel per lane, over the first KC slots (the structure phase linked the slots K..KC-1 to nothing).
// Returns the occupations, the ground energy (absolute) and, with VALIDATE, the
// relative residual ||H x - lam x||_2 / ||H||_inf of the winning component's eigenpair.  Written as three rounds of
// INDEPENDENT loads (links and energies; eigenvalues; the winner's vector) -- a lane's chain of 64 dependent loads was
// what the first version of this phase spent its time on.
// ---------------------------------------------------------------------------------------------------------------
template <int N, bool VALIDATE, int KC>
__device__ __forceinline__ void qd_ground_select(const QdPixelRec* __restrict__ rec, int ps, const QdSlab& sl,
                                                 double* occ, double& lam_out, double& resid_out) {
    const unsigned* __restrict__ link = sl.link + ps * 32;
    const unsigned char* __restrict__ rank = sl.rank + ps * 32;
    const double* __restrict__ pool = sl.pool;
    const double* __restrict__ lamd = sl.lam;
    const int nvalid = rec->nvalid;
    unsigned lk[KC];
    double lam[KC];
    {
        const uint4* l4 = reinterpret_cast<const uint4*>(link);
#pragma unroll
        for (int q = 0; q < KC / 4; ++q) { const uint4 v = l4[q]; lk[4 * q] = v.x; lk[4 * q + 1] = v.y; lk[4 * q + 2] = v.z; lk[4 * q + 3] = v.w; }
    }
    // eigenvalues are relative to the pixel's lowest free energy; an isolated state that survived the Gershgorin test
    // is a state of exactly that energy (its bound F - 0 must not exceed min F): lambda = 0
#pragma unroll
    for (int m = 0; m < KC; ++m) {
        const bool task = lk[m] < QD_LINK_SINGLE;
        const double lt = lamd[task ? lk[m] : 0u];         // (always a valid address; the value is used for tasks only)
        lam[m] = task ? lt : (lk[m] == QD_LINK_SINGLE ? 0.0 : INFINITY);
    }
    // the lowest component; tie between components (exactly equal energies): the state with the lowest candidate
    // index wins -- the reference order puts it first -- independent of the buffer order
    unsigned idx2[KC / 2];
    {
        const uint4* i4 = reinterpret_cast<const uint4*>(rec->idx);
#pragma unroll
        for (int q = 0; q < KC / 8; ++q) { const uint4 v = i4[q]; idx2[4 * q] = v.x; idx2[4 * q + 1] = v.y; idx2[4 * q + 2] = v.z; idx2[4 * q + 3] = v.w; }
    }
    double best = INFINITY; unsigned bestkey = 0xFFFFFFFFu, wl = QD_LINK_NONE; int bm = 0;
#pragma unroll
    for (int m = 0; m < KC; ++m) {
        const unsigned code = (idx2[m >> 1] >> (16 * (m & 1))) & 0xFFFFu;
        const unsigned key = (m < nvalid) ? code : 0xFFFFFFFEu;
        const bool better = (lam[m] < best) | ((lam[m] == best) & (key < bestkey));
        if (better) { best = lam[m]; bestkey = key; wl = lk[m]; bm = m; }
    }
    const bool wtask = wl < QD_LINK_SINGLE;
    const unsigned woff = wtask ? sl.lists[wl] : 0u;          // the winner's record
    // the winner's vector: one (predicated) load per member state
    unsigned rk8[KC / 4];
    {
        if constexpr (KC >= 16) {
            const uint4* r4 = reinterpret_cast<const uint4*>(rank);
#pragma unroll
            for (int q = 0; q < KC / 16; ++q) { const uint4 v = r4[q]; rk8[4 * q] = v.x; rk8[4 * q + 1] = v.y; rk8[4 * q + 2] = v.z; rk8[4 * q + 3] = v.w; }
        } else {
            const uint2 v = *reinterpret_cast<const uint2*>(rank); rk8[0] = v.x; rk8[1] = v.y;
        }
    }
    double xs[KC];
#pragma unroll
    for (int m = 0; m < KC; ++m) {
        const bool member = wtask ? (lk[m] == wl) : (m == bm);
        const unsigned rk = (rk8[m >> 2] >> (8 * (m & 3))) & 0xFFu;
        double x = 0.0;
        if (member) x = wtask ? pool[woff + 2 + rk] : 1.0;
        xs[m] = x;
    }
    int fl[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { occ[i] = 0.0; fl[i] = rec->fl[i]; }
#pragma unroll
    for (int m = 0; m < KC; ++m) {
        const unsigned code = (idx2[m >> 1] >> (16 * (m & 1))) & 0xFFFFu;
        const double p = (m < nvalid) ? xs[m] * xs[m] : 0.0;          // (the padding lanes are |0..0>)
#pragma unroll
        for (int i = 0; i < N; ++i)
            occ[i] = fma(p, (double)(fl[i] + (int)((code >> (2 * (N - 1 - i))) & 3u) - 1), occ[i]);
    }
    lam_out = best;
    resid_out = 0.0;
    if (VALIDATE) {
        const double hn = sl.aux[ps];
        lam_out = best + sl.aux[QD_GS_PPB + ps];
        if (wtask) resid_out = pool[woff + 1] / (hn > 0.0 ? hn : 1.0);
    }
}

#endif  // __HIPCC__
