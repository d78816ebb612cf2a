/*
 * qdsim.h -- C ABI of libqdsim.so, the MI355X-native batched replacement for the
 * per-step charge-stability simulation of QADAPT (edwindn/rl-agent-for-qubit-
 * array-tuning).  Plain C, plain pointers and sizes, no torch types; every
 * function returns 0 on success or a QD_ERR_* code (text via qd_last_error).
 *
 * The reference has no FFI (it is 100 % Python); each entry point below names
 * the Python interface it stands in for (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes stub a maintainer adds on the reference side.
 *
 * Memory contract: all `*_dev` pointers are DEVICE memory owned by the caller
 * (e.g. torch.Tensor.data_ptr()) and must stay valid until the stream work that
 * uses them has finished.  `stream` is a hipStream_t passed as void* (NULL =
 * default stream).  A handle is bound to one GPU and is not thread-safe (the
 * RLlib env runner that calls the reference is single-threaded as well).
 *
 * Batch layout: B environments of the same n_dot (N) and resolution (R).
 *   C = N-1 CSD channels, P = R*R pixels, G = N+1 gates (plungers + sensor).
 *   agent order everywhere: plunger_0..plunger_{N-1}, barrier_0..barrier_{N-2}.
 */
#ifndef QDSIM_H
#define QDSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QD_OK 0
#define QD_ERR_ARG 1          /* bad argument / unsupported configuration        */
#define QD_ERR_HIP 2          /* a HIP runtime call failed                        */
#define QD_ERR_STATE 3        /* call order violated (e.g. outputs not bound)     */
#define QD_ERR_NOMEM 4

#define QD_FLAG_VALIDATE 1    /* keep per-pixel candidate records and occupations  */
#define QD_FLAG_PIXEL_SEARCH 2 /* a9 by the per-pixel search only (default: one search per 8x8 pixel tile where the
                                 grid is fine enough, with an exact per-pixel redo pass; same results, A/B switch) */
#define QD_FLAG_RETIRED_TILE_FUSED 4  /* was QD_FLAG_TILE_FUSED (round 2: experimental fused tile kernel, 3x slower than the
                                 default pipeline); the kernel is gone and qd_create refuses the flag with QD_ERR_ARG */
#define QD_FLAG_GS_GERSHGORIN_ZERO 8  /* ground-state stage: discard a hop component only when its Gershgorin lower bound exceeds
                                 min F = 0 (default: the pixel's lowest 2x2 pair bound (F_i + F_j) / 2 - |H_ij|, with a margin
                                 of 2^-40 ||H||_inf, which leaves fewer components to solve; same results bit for bit,
                                 A/B switch; qd_get_solver_stats counts the tasks) */

/* Stochastic stages.  The generators are counter-based Philox streams, so
 * results are reproducible per (rng_seed, global env id, observation number, channel, pixel)
 * but NOT comparable sample-by-sample with the reference's numpy global RNG. */
#define QD_NOISE_SENSOR 1     /* white + telegraph noise on the sensor potential
                                 (TunnelCoupledChargeSensed.py:354; qarray WhiteNoise/TelegraphNoise) */
#define QD_NOISE_RADIAL 2     /* distance-dependent image noise / white-noise replacement
                                 (qarray_base_class.py:444-493)                     */
#define QD_NOISE_LATCH 4      /* charge latching along the raster (ground_state.py:164; qarray
                                 LatchingModel, source absent: UNVERIFIED restatement)     */

typedef struct qd_handle qd_handle;

/* Mirrors the env_config.yaml / constructor knobs of QuantumDeviceEnv
 * (src/qadapt/environment/env.py:38-127, 350-462, 779-787). */
typedef struct qd_config {
    int32_t struct_size;          /* = sizeof(qd_config), for ABI checks          */
    int32_t n_dot;                /* N, 2..8                                       */
    int32_t resolution;           /* R (env_config.yaml simulator.resolution)     */
    int32_t batch;                /* B environments held by this handle            */
    int32_t max_steps;            /* truncation horizon (simulator.max_steps)     */
    int32_t env_chunk;            /* envs per scratch chunk, 0 = choose            */
    int32_t flags;                /* QD_FLAG_*                                     */
    int32_t noise_flags;          /* QD_NOISE_* (0 = deterministic parity mode)           */
    double gate_ramp_start;       /* reward.gate_ramp_start                        */
    double gate_quadratic_start;  /* reward.gate_quadratic_start                   */
    double barrier_ramp_start;    /* reward.barrier_ramp_start                     */
    double kalman_prior_mean;     /* env.py:781                                    */
    double kalman_prior_variance; /* env.py:782                                    */
    double kalman_prior_mean_nnn; /* env.py:786                                    */
    double kalman_variance_threshold; /* capacitance_model.variance_threshold     */
    double kalman_process_noise;  /* capacitance_model.process_noise               */
    uint64_t rng_seed;            /* Philox key for the stochastic stages; the two 32-bit halves are XOR-folded into ONE
                                     32-bit key word (seeds that differ only by such a fold give the same streams)      */
    int64_t env_id_offset;        /* global id of env 0 (multi-GPU shards); the second key word is the low 32 bits of
                                     env_id_offset + env index: global env ids are taken modulo 2^32                    */
    /* config variants reachable from env_config.yaml (env.py:393-441, 553-563, 592-618, 861-876) */
    int32_t use_deltas;           /* simulator.use_deltas: gate actions are increments (env.py:864-867) */
    int32_t sparse_reward;        /* reward.sparse_reward (env.py:393-414)         */
    int32_t gate_curve_type;      /* QD_CURVE_* (reward.gate_curve_type, env.py:430-441) */
    int32_t update_method;        /* QD_UPDATE_KALMAN / QD_UPDATE_DIRECT (KalmanUpdater.py / DirectUpdater.py) */
    int32_t cnn_outputs;          /* 3: [NN, NNN_right, NNN_left]; 2: legacy nearest_neighbour [RL, LR] (env.py:592-618) */
    int32_t num_charge_states;    /* K, latched_model.num_charge_states (qarray_config.yaml:129): kept charge states per
                                     pixel, 1..32; 0 = 32 (the field was reserved0: zeroed callers keep the default).  The
                                     K lowest by (E, index), padded with |0..0> when fewer are valid; H is K x K.
                                     QD_ALL_CHARGE_STATES(m) (negative): the untruncated space, see below.
                                     qd_create returns QD_ERR_ARG above 32 and for an unsupported full space            */
    double delta_max;             /* simulator.delta_max                           */
    double gate_curve_exponent;   /* reward.gate_curve_exponent                    */
    double plunger_radius;        /* reward.plunger_radius        (sparse)         */
    double outer_plunger_radius;  /* reward.outer_plunger_radius  (sparse)         */
    double outer_plunger_reward_max; /* reward.outer_plunger_reward_max (sparse)  */
    double barrier_radius;        /* reward.barrier_radius        (sparse)         */
} qd_config;

/* num_charge_states = QD_ALL_CHARGE_STATES(m), m >= 1: the reference's num_charge_states = None (ground_state.py:79-83)
 * with max_charge_carriers = m.  Every pixel uses all M = (m + 1)^N states with 0..m carriers per dot (reference order:
 * base m + 1, dot 0 the most significant digit) and the ground state of the whole M x M Hamiltonian; no continuous
 * ground state and no candidate search run.  Supported while M <= 512, no total-charge sector holds more than 64
 * states, m <= 15 and N m + 1 <= 32 (m = 4: N = 2 and 3; m = 3: up to N = 4; m = 2: up to N = 5; m = 1: up to N = 7);
 * other (N, m) are QD_ERR_ARG.  Sectors of 33..64 states are solved one per wavefront (csrc/qd_eig_wave.h) and counted
 * in qd_get_solver_stats' out16[14].  In this mode qd_get_candidates returns
 * QD_ERR_ARG (there is no per-pixel list), qd_get_occupations / qd_get_eigen work as usual, and qd_time_kernels reports
 * 0 for the tile search and the redo pass. */
#define QD_ALL_CHARGE_STATES(m) (-(m))

#define QD_CURVE_CONSTANT 0
#define QD_CURVE_POLYNOMIAL 1
#define QD_CURVE_EXPONENTIAL 2
#define QD_CURVE_LINEAR 3
#define QD_UPDATE_KALMAN 0
#define QD_UPDATE_DIRECT 1

/* Sizes (in float64 elements) of the per-env parameter and state blocks whose
 * layout is documented in csrc/qd_common.h (mirrored by qadapt_hip/layout.py). */
int qd_param_block_doubles(int n_dot);
int qd_state_block_doubles(int n_dot);
/* Writes the 31 layout integers (see qadapt_hip/layout.py LAYOUT_FIELDS). */
int qd_layout_query(int n_dot, int32_t* out31);

/* QuantumDeviceEnv.__init__ (env.py:38-132): allocates device state for B envs
 * on GPU `device`; Kalman filters start at their priors (env.py:779-787). */
/* On failure after the handle was allocated (QD_ERR_HIP / QD_ERR_NOMEM), *out is still set: read the message with
 * qd_last_error and release the partial handle with qd_destroy. */
int qd_create(const qd_config* cfg, int device, qd_handle** out);
int qd_destroy(qd_handle* h);
const char* qd_last_error(const qd_handle* h);

/* Output tensors written by qd_observe (all float32, caller-owned device memory):
 *   global_image   [B][R][R][C]    obs["image"]            (env.py:471-509)
 *   plunger_images [B][N][R][R][2] per-agent plunger view  (multi_agent_wrapper.py:311-350)
 *   barrier_images [B][C][R][R][1] per-agent barrier view
 *   voltages       [B][2N-1]       normalised gate then barrier voltages (env.py:511-532)
 * Any pointer may be NULL to skip that output. */
int qd_bind_outputs(qd_handle* h, float* global_image_dev, float* plunger_images_dev,
                    float* barrier_images_dev, float* voltages_dev);

/* QuantumDeviceEnv.reset's device construction (env.py:160-222) for `n` envs:
 * uploads parameter blocks and initial state blocks (HOST pointers, n rows each)
 * built by the host-side sampler; step counters return to 0.  The Kalman state
 * is NOT touched (the reference never resets it, env.py:130) unless
 * reset_kalman != 0. */
int qd_load_episodes(qd_handle* h, const int32_t* env_ids_host, int n, const double* params_host,
                     const double* state_host, int reset_kalman, void* stream);

/* QuantumDeviceEnv.step lines env.py:260-285: clip + rescale the actions
 * [B][2N-1] (gates then barriers, float32), reward against the PREVIOUS ground
 * truth, step counter and truncation flag.  rewards_dev [B][2N-1] float64,
 * truncated_dev [B] uint8. */
int qd_apply_actions(qd_handle* h, const float* actions_dev, double* rewards_dev,
                     uint8_t* truncated_dev, void* stream);

/* QarrayBaseClass._get_obs + QuantumDeviceEnv._normalise_obs +
 * MultiAgentEnvWrapper._extract_agent_observation
 * (qarray_base_class.py:171-229, env.py:471-534, multi_agent_wrapper.py:311-383)
 * for the listed envs (env_ids_dev == NULL: all B).  Writes the bound outputs. */
int qd_observe(qd_handle* h, const int32_t* env_ids_dev, int n, void* stream);

/* QuantumDeviceEnv._update_virtual_gate_matrix (env.py:537-622) with the CNN's
 * outputs supplied by the caller: values/log_vars [B][C][3] float32 (indexed by
 * env id, not by list position).  Kalman update (KalmanUpdater.py:92-213), VGM
 * (qarray_base_class.py:904-942) and, if recompute_ground_truth != 0, the new
 * ground truth (env.py:298-305; reset() skips this, env.py:233). */
int qd_update_capacitance(qd_handle* h, const int32_t* env_ids_dev, int n, const float* values_dev,
                          const float* log_vars_dev, int recompute_ground_truth, void* stream);

/* One whole QuantumDeviceEnv.step for all B envs = qd_apply_actions +
 * qd_observe + qd_update_capacitance(recompute_ground_truth = 1). */
int qd_step(qd_handle* h, const float* actions_dev, const float* values_dev,
            const float* log_vars_dev, double* rewards_dev, uint8_t* truncated_dev, void* stream);

/* Episode-end snapshot (what the reference's step() returns for a truncating env before its reset() replaces the
 * device, multi_agent_wrapper.py:485-584, env.py:240-315): slot i of every destination receives env env_ids_dev[i]'s
 *   global_dst   [n][R][R][C]      \
 *   plunger_dst  [n][N][R][R][2]    | float32, the bound outputs (layouts as at qd_bind_outputs)
 *   barrier_dst  [n][C][R][R][1]    |
 *   voltages_dst [n][2N-1]         /
 *   state_dst    [n][qd_state_block_doubles]  float64
 *   params_dst   [n][qd_param_block_doubles]  float64
 *   steps_dst    [n]               int32 step counter
 * all compact, caller-owned device memory.  Any destination may be NULL, and so may an output that was never bound:
 * that part is skipped.  n == 0 does nothing; n > B, or env_ids_dev == NULL with n > 0, is QD_ERR_ARG; ids outside
 * [0, B) are skipped (their slots are left untouched).  One kernel launch, stream-ordered on `stream`; the host is
 * never synchronised.  Called between qd_update_capacitance and qd_load_episodes it keeps the final observation and
 * state of the envs an automatic reset is about to replace. */
int qd_snapshot(qd_handle* h, const int32_t* env_ids_dev, int n,
                float* global_dst, float* plunger_dst, float* barrier_dst, float* voltages_dst,
                double* state_dst, double* params_dst, int32_t* steps_dst, void* stream);

/* Stateless probe scans: QarrayBaseClass._get_obs(gate_voltages, barrier_voltages, sensor_voltage) asked as a side
 * question (qarray_base_class.py:171-229; its users outside step() are map_device_range.py, map_full_device_range.py,
 * gui/image_generator.py:136 and the dataset generator).  Renders nq queries in one call; every pointer is caller-owned
 * DEVICE memory, the call is stream-ordered on `stream` and never synchronises the host.
 *   env_of_query_dev [nq]      int32, each in [0, B): query q uses that env's parameter block and its CURRENT virtual
 *                              gate matrix and origin; everything else comes from the query
 *   gate_v_dev       [nq][N]   virtual gate voltages, as _get_obs takes them
 *   barrier_v_dev    [nq][N-1]
 *   sensor_v_dev     [nq]      or NULL: 0.0, as sensor_voltage=None
 *   window_dev       [nq]      half-widths of the scan window, or NULL: the env's own window
 *   raw_dst          [nq][C][P]    float64 unnormalised signal, layout of qd_get_raw; may be NULL
 *   image_dst        [nq][R][R][C] float32, normalised per query with its own 0.5 / 99.5 percentiles, as the
 *                                  global_image of qd_observe; may be NULL
 *   plohi_dst        [nq][2]       those percentiles; may be NULL
 * qd_probe is DETERMINISTIC: every launch runs with noise flags 0 whatever the handle's noise_flags are (no sensor noise,
 * no radial noise, no latching); qd_probe_ex below runs the stochastic stages on the queries.  The hot kernels are the
 * ones qd_observe runs, on probe copies of the parameter and state blocks, so a probe at an env's own voltages, sensor voltage and window equals
 * the raw signal, percentiles and image of a noise-free qd_observe bit for bit.
 * The call changes nothing that qd_step, qd_observe or any qd_get_* function can see: not the state blocks, step
 * counters or Kalman state, not the bound outputs, raw signal or percentiles of the last observe, not the observation
 * serial of qd_get_rng_state or the telegraph chains.  nq may exceed B and many queries may name one env; queries run in
 * launch chunks of qd_chunk_envs.  Scratch (per query in flight: a parameter copy, a state block, C*P doubles of signal)
 * is allocated by the first probe and freed by qd_destroy; handles that never probe allocate nothing.  That first
 * call allocates with hipMalloc, which may wait for the device: "never synchronises" holds from the second probe on.
 * nq == 0 does nothing.  QD_ERR_ARG, found without reading the device: nq < 0, env_of_query_dev, gate_v_dev or
 * barrier_v_dev NULL.  An id outside [0, B) leaves its destination slots untouched, as at qd_snapshot.  A handle created
 * with QD_FLAG_VALIDATE answers QD_ERR_STATE: its record, occupation and eigenvalue buffers hold B envs and belong to
 * the last observe.  Works for num_charge_states 1..32 and in the full charge-state space.
 * qd_probe(...) is qd_probe_ex(..., NULL, stream). */
int qd_probe(qd_handle* h, const int32_t* env_of_query_dev, int nq, const double* gate_v_dev,
             const double* barrier_v_dev, const double* sensor_v_dev, const double* window_dev,
             double* raw_dst, float* image_dst, double* plohi_dst, void* stream);

/* Probe scans with the stochastic stages and the occupations.  In the reference the stateless _get_obs is not
 * deterministic: it runs the configured sensor noise, the radial noise or white-noise replacement and the latching model
 * exactly as a step does (qarray_base_class.py:171-229, 444-493, TunnelCoupledChargeSensed.py:354, ground_state.py:164),
 * and its point function returns (signal, n_open).  The ten data arguments are those of qd_probe; opts == NULL is
 * qd_probe, bit for bit.
 *   noise_flags   the QD_NOISE_* stages to run on the queries, whatever the handle was created with (0: none)
 *   serial        the observation-number word of the Philox counter.  The caller owns it: two probes with the same
 *                 serial, stream_base and query index draw the same numbers.  A step's serial (qd_get_rng_state) counts
 *                 up from 1 and never reaches 2^63, so side questions should set the top bit: they then never share a
 *                 stream with a step
 *   stream_base   query q draws from the streams of global env id stream_base + q (low 32 bits), keyed by the handle's
 *                 folded rng_seed
 *   occ_dst       [nq][C][P][N] float64 DEVICE, layout of qd_get_occupations, or NULL: the occupations the signal was
 *                 formed from, after latching if QD_NOISE_LATCH ran.  A channel that the radial stage replaced by white
 *                 noise is never solved: its occupations are NaN.  Ids outside [0, B) leave their slots untouched.
 *                 Asking for them only adds stores: the raw signal keeps the bits of a probe without occ_dst
 * Per launch chunk the order is qd_observe's, on the probe buffers: gather, telegraph chains (SENSOR), candidate search
 * and ground state (a replaced channel is skipped as in a step), latching (LATCH; one lane per raster row,
 * csrc/qd_latch.h, same bits as the step's one-thread walk), sensor stage, percentiles, write.
 * Contracts:
 *   chunk independence   a query's results do not depend on qd_chunk_envs
 *   nothing of the envs moves   state blocks, step counters, Kalman state, bound outputs, qd_get_raw,
 *                        qd_get_occupations, qd_get_rng_state and the envs' telegraph words are as before the call
 *   equivalence with a step   nq = B, env_of_query = 0..B-1, each env's own gate and barrier voltages and sensor slot,
 *                        window_dev = NULL, noise_flags = the handle's, stream_base = env_id_offset, serial = S: raw,
 *                        percentiles and image have the bits of the qd_observe whose observation number
 *                        (qd_get_rng_state afterwards) is S, and with QD_NOISE_LATCH occ_dst has the bits of
 *                        qd_get_occupations in every channel that was not replaced
 * Scratch beyond qd_probe's, per query in flight: C*P*N doubles of occupations from the first call with QD_NOISE_LATCH or
 * occ_dst, C*ceil(P/64) telegraph words from the first call with QD_NOISE_SENSOR; handles that never ask allocate
 * nothing more than qd_probe does.  QD_ERR_ARG, found without touching the device, besides qd_probe's: a struct_size
 * that is not sizeof(qd_probe_opts), a noise_flags bit outside QD_NOISE_SENSOR | QD_NOISE_RADIAL | QD_NOISE_LATCH.
 * A QD_FLAG_VALIDATE handle answers QD_ERR_STATE.  Channel sub-ranges, asymmetric windows and a virtual gate matrix
 * or noise centre per query are not built for probes; qd_scan2d below renders one image over any two controls and
 * ranges, with a virtual gate matrix per query. */
typedef struct qd_probe_opts {
    int32_t  struct_size;   /* = sizeof(qd_probe_opts) */
    int32_t  noise_flags;   /* QD_NOISE_* stages to run on the queries; 0 = none.  Independent of the handle's noise_flags */
    uint64_t serial;        /* the observation-number word of the Philox counter */
    int64_t  stream_base;   /* query q draws from the streams of global env id stream_base + q (mod 2^32) */
    double*  occ_dst;       /* [nq][C][P][N] float64 DEVICE, layout of qd_get_occupations; or NULL */
} qd_probe_opts;
int qd_probe_ex(qd_handle* h, const int32_t* env_of_query_dev, int nq, const double* gate_v_dev,
                const double* barrier_v_dev, const double* sensor_v_dev, const double* window_dev,
                double* raw_dst, float* image_dst, double* plohi_dst, const qd_probe_opts* opts, void* stream);

/* Point evaluation: TunnelCoupledChargeSensed.charge_sensor_open(vg, vb) -> (signal, n_open) and ground_state_open(vg, vb)
 * (TunnelCoupledChargeSensed.py:312-380, ground_state.py:24-166) at arbitrary PHYSICAL voltages, np points in one call:
 * line cuts, plunger-versus-barrier scans, scans of non-adjacent pairs, simplex vertices, the occupations at one voltage.
 * Points come in ng groups; group g evaluates rows group_start_host[g] .. group_start_host[g + 1] on the device (parameter
 * block) of env group_env_host[g].  An env may be named by many groups.
 *   group_env_host   [ng]        int32, HOST, each in [0, B)
 *   group_start_host [ng + 1]    int64, HOST, non-decreasing, >= 0; np = group_start_host[ng]
 *   vg_dev           [np][N+1]   physical gate voltages, sensor gate last, as charge_sensor_open takes them: no virtual
 *                                gate matrix and no origin are applied
 *   vb_dev           [np][N-1]   barrier voltages
 *   gamma_host       [ng]        HOST, the peak width of each group's sensor signal, or NULL: each env's own
 *                                coulomb_peak_width (scal[1] of its parameter block)
 *   signal_dst       [np]        float64 sensor signal, sum over the 10 peaks; may be NULL
 *   occ_dst          [np][N]     float64 expectation occupations <n>; may be NULL
 * vg_dev, vb_dev, signal_dst and occ_dst are caller-owned DEVICE memory; rows before group_start_host[0] and past np are
 * neither read nor written.  The call is stream-ordered on `stream` and DETERMINISTIC, as probes are: no sensor noise, no
 * radial noise, no latching, whatever the handle's noise_flags.  A point takes the place of a pixel: its record is filled
 * from the caller's voltages, then the per-pixel candidate search, the ground-state kernels and the sensor expression of
 * qd_observe run on it, so a point at the voltages of a scan's pixel has the bits of that pixel in a noise-free scan of a
 * QD_FLAG_PIXEL_SEARCH handle with a constant peak width.  The voltage-dependent capacitance model applies as in scans.
 * The occupations have the bits qd_get_occupations gives for that pixel on a QD_FLAG_VALIDATE handle.  Those two paths
 * solve the kept states in different orders when num_charge_states is 8, 16 or 32 (a product handle keeps the search
 * order, a validate handle the reference order by (E, index)) and their eigenvectors differ by rounding; so with both
 * destinations given the signal is solved first, the records are sorted and the ground-state stage runs again for the
 * occupations.  With one destination, or any other num_charge_states, it runs once.
 * The call changes nothing that qd_step, qd_observe, qd_probe or any qd_get_* function can see.
 * Points run in slots of C*P (one env each; a group takes ceil(n / (C*P)) slots, the last one padded with records that
 * cost neither a search nor an eigen task), at most min(qd_chunk_envs, QD_POINTS_SLOTS) slots per launch.  Scratch (per
 * slot in flight: a parameter copy, a state block, C*P doubles of sensor constants, C*P*N doubles of occupations -- 1.8 MB
 * at 8 dots and 64x64, so about 117 MB at most) is allocated by the first call with hipMalloc and freed by qd_destroy.
 * QD_ERR_ARG, found without reading the device: group_env_host, group_start_host, vg_dev or vb_dev NULL, ng < 0,
 * group_start_host decreasing or negative, an env id outside [0, B).  QD_ERR_STATE: a QD_FLAG_VALIDATE handle (as
 * qd_probe), and a handle in the full charge-state space, whose structure kernel synthesises its own voltages (a point
 * front end for it is not built).  ng == 0 or np == group_start_host[0] does nothing.  Works for num_charge_states 1..32. */
#define QD_POINTS_SLOTS 64
int qd_eval_points(qd_handle* h, const int32_t* group_env_host, const int64_t* group_start_host, int ng,
                   const double* vg_dev, const double* vb_dev, const double* gamma_host,
                   double* signal_dst, double* occ_dst, void* stream);

/* Stateless 2-D scans over ANY two controls, each over its own [lo, hi]: the reference model layer's
 * do2d_open(x_gate, x_min, x_max, ..., y_gate, ...) and GateVoltageComposer.do2d(..., gate_voltages, add_full_crosstalk)
 * (GateVoltageComposer.py:170-211) for nq queries in one call -- a non-adjacent plunger pair, a plunger against a barrier,
 * a sensor-gate sweep, one channel where a caller needs one and not N-1, a scan under a hypothetical virtual gate matrix --
 * with the measurement stages of a step (sensor noise, latching) and its normalisation.
 * Controls are indexed in the order of the model's voltage vector: 0..N-1 the plungers, N the sensor gate, N+1..2N-1 the
 * barriers.  With W[2N] = [gate_v, sensor_v, barrier_v] of the query, pixel (row y, column x) has
 * W[ax] = linspace(x_lo, x_hi, R)[x] and W[ay] = linspace(y_lo, y_hi, R)[y]: x is the first axis and runs along columns.
 *   QD_SCAN_VIRTUAL   the model sees VGM W[0:N+1] + origin for the gates and W[N+1:] for the barriers, VGM the env's
 *                     current virtual gate matrix or the query's
 *   QD_SCAN_PHYSICAL  the model sees W: no matrix and no origin, as qd_eval_points takes its voltages
 *   env_of_query_dev [nq]      int32, the env whose device (parameter block, virtual gate matrix) renders query q
 *   axes_dev         [nq][2]   int32 (ax, ay)
 *   range_dev        [nq][4]   x_lo, x_hi, y_lo, y_hi; lo > hi sweeps downwards, lo == hi repeats a 1-D sweep
 *   gate_v_dev       [nq][N], barrier_v_dev [nq][N-1], sensor_v_dev [nq] or NULL (0.0): the controls that are not swept
 *   raw_dst          [nq][P]    float64 unnormalised signal; may be NULL
 *   image_dst        [nq][R][R] float32, normalised per query with its own 0.5 / 99.5 percentiles; may be NULL
 *   plohi_dst        [nq][2]    those percentiles; may be NULL
 * opts (NULL: virtual frame, deterministic):
 *   frame         QD_SCAN_VIRTUAL or QD_SCAN_PHYSICAL, for all queries of the call
 *   noise_flags   QD_NOISE_SENSOR | QD_NOISE_LATCH stages to run.  QD_NOISE_RADIAL is QD_ERR_ARG: the reference defines its
 *                 centre only for the env's own adjacent-pair observation
 *   serial, stream_base   as in qd_probe_opts: the caller owns the serial, query q draws from the streams of global env
 *                 id stream_base + q; the channel word of the Philox counter is 0
 *   vgm_dev       [nq][N+1][N+1] row-major or NULL: the env's current matrix (virtual frame only)
 *   gamma_dev     [nq] peak widths, or NULL: with two virtual plungers as axes the rule of a step on those two plungers'
 *                 base voltages (vary_peak_width handles; the env's constant otherwise), else the env's constant
 *   occ_dst       [nq][P][N] float64 or NULL: the occupations the signal was formed from (after latching, if it ran)
 * A query occupies one slot of the scan buffers with ONE channel image.  The two search kernels run with the scan front
 * end (csrc/qd_pixel.h qd_scan_voltages; the tile search learns the affine model of v' from lane differences and does not
 * know which controls are swept); structure, solve, select, latching rows, telegraph chains, sensor stage and percentiles
 * are the kernels of a step or probe.  With ax = c, ay = c + 1, x_lo = fl(v_c - w), x_hi = fl(v_c + w) (likewise y) and the
 * virtual frame the front end performs the operations of a probe's in the same order: raw equals channel c of qd_probe
 * with window w bit for bit (image and percentiles too where C = 1), and with noise channel 0 equals qd_probe_ex.
 * On a QD_FLAG_PIXEL_SEARCH handle raw equals qd_eval_points at the pixels' voltages bit for bit.
 * Stream-ordered with no host wait after the first call, which allocates the scratch (per query in flight: a parameter
 * copy, a state block, an axes descriptor, P doubles of signal; P*N doubles of occupations and ceil(P/64) telegraph words
 * from the first call that needs them) with hipMalloc; qd_destroy frees it.  nq may exceed B; queries run in chunks of
 * qd_chunk_envs and results do not depend on the chunking.  The call changes nothing that qd_step, qd_observe, qd_probe*,
 * qd_eval_points or any qd_get_* function can see.
 * QD_ERR_ARG, found without reading the device: NULL env_of_query_dev, axes_dev, range_dev, gate_v_dev or barrier_v_dev,
 * nq < 0, a struct_size that is not sizeof(qd_scan_opts), an unknown frame, vgm_dev with the physical frame, a noise bit
 * outside SENSOR | LATCH.  Axes arrive on the device: an axis outside [0, 2N), ax == ay or an env id outside [0, B) makes
 * the query inert, its destination slots are left untouched.  QD_ERR_STATE: QD_FLAG_VALIDATE handles and handles in the
 * full charge-state space, as qd_eval_points refuses them.  Radial noise and more than two swept controls are not
 * built; Rx != Ry is qd_scan_grid's (without the tile search). */
#define QD_SCAN_VIRTUAL 0
#define QD_SCAN_PHYSICAL 1
typedef struct qd_scan_opts {
    int32_t  struct_size;   /* = sizeof(qd_scan_opts) */
    int32_t  frame;         /* QD_SCAN_VIRTUAL 0 / QD_SCAN_PHYSICAL 1 */
    int32_t  noise_flags;   /* QD_NOISE_SENSOR | QD_NOISE_LATCH; 0 = none */
    int32_t  reserved;
    uint64_t serial;        /* the observation-number word of the Philox counter */
    int64_t  stream_base;   /* query q draws from the streams of global env id stream_base + q (mod 2^32) */
    const double* vgm_dev;  /* [nq][G][G] or NULL: the env's current matrix (virtual frame only) */
    const double* gamma_dev;/* [nq] or NULL */
    double*  occ_dst;       /* [nq][P][N] or NULL */
} qd_scan_opts;
int qd_scan2d(qd_handle* h, const int32_t* env_of_query_dev, int nq, const int32_t* axes_dev, const double* range_dev,
              const double* gate_v_dev, const double* barrier_v_dev, const double* sensor_v_dev, double* raw_dst,
              float* image_dst, double* plohi_dst, const qd_scan_opts* opts, void* stream);

/* Stateless 2-D scans along two DIRECTION VECTORS over the 2N controls: the axes a double-dot experiment is plotted in --
 * detuning e{i}_{j} (+1 on plunger i, -1 on plunger j) against the on-site axis U{i}_{j} (1/sqrt(2) on both), as the
 * reference's GateVoltageComposer builds them (GateVoltageComposer.py:35-84) -- a plunger with a compensating barrier, a
 * sweep along a ground-truth direction, and qd_scan2d itself as the special case of two unit vectors; with the measurement
 * stages of a step (sensor noise, latching), the tile search and the normalisation, none of which a grid sent through
 * qd_eval_points gets.
 * Controls are indexed as in qd_scan2d.  With W0[2N] = [gate_v, sensor_v, barrier_v] of the query (the BASE POINT: unlike
 * the composer's crosstalk-free do2d, the controls that are not swept keep the query's voltages and the origin is added
 * once), sx = linspace(x_lo, x_hi, R)[x] and sy = linspace(y_lo, y_hi, R)[y], pixel (row y, column x) has
 *   W[i] = fma(sy, dy[i], fma(sx, dx[i], W0[i]))      i = 0..2N-1
 * and the model sees W through the frame as in qd_scan2d (QD_SCAN_VIRTUAL: VGM W[0:N+1] + origin and W[N+1:];
 * QD_SCAN_PHYSICAL: W).  With dx = e_ax, dy = e_ay and W0[ax] = W0[ay] = 0 every result has the bits of qd_scan2d(ax, ay)
 * (with gamma_dev given: see below).
 *   env_of_query_dev [nq]          int32, the env whose device renders query q
 *   dir_dev          [nq][2][2N]   dx then dy of query q.  A zero vector is legal: it repeats a 1-D sweep.  Non-finite
 *                                  coefficients are NOT looked for: they give non-finite voltages and an undefined image
 *   range_dev        [nq][4]       x_lo, x_hi, y_lo, y_hi of the two scalars sx, sy; lo > hi sweeps downwards
 *   gate_v_dev       [nq][N], barrier_v_dev [nq][N-1], sensor_v_dev [nq] or NULL (0.0): the base point
 *   raw_dst, image_dst, plohi_dst  as in qd_scan2d; each may be NULL
 * opts (NULL: virtual frame, deterministic): the fields of qd_scan_opts with the same meaning, except
 *   gamma_dev     [nq] peak widths, or NULL: the env's constant coulomb_peak_width.  The vary_peak_width rule of a step is
 *                 a function of the swept plunger PAIR; an affine axis has no pair, so the rule is not applied
 * A query occupies one slot of the scan buffers (those of qd_scan2d) with ONE channel image; the two search kernels run with
 * the affine front end (csrc/qd_pixel.h qd_affine_voltages), everything behind them is the kernels of a step or probe.
 * On a QD_FLAG_PIXEL_SEARCH handle raw equals qd_eval_points at the pixels' voltages bit for bit.
 * Stream-ordered with no host wait after the first call, which allocates the scratch with hipMalloc (per query in flight:
 * what qd_scan2d keeps -- a parameter copy, a state block, P doubles of signal, 2 of percentiles; P*N doubles of occupations
 * and ceil(P/64) telegraph words from the first call that needs them -- shared with qd_scan2d, and one descriptor of
 * 4 + 4*8 doubles and the frame, 296 bytes); qd_destroy frees it.  Calls of qd_scan2d and qd_scan_affine on one handle
 * belong on one stream.  nq may exceed B; queries run in chunks of qd_chunk_envs and results do not depend on the chunking.
 * The call changes nothing that qd_step, qd_observe, qd_probe*, qd_scan2d, qd_eval_points or any qd_get_* function can see.
 * QD_ERR_ARG, found without reading the device: NULL env_of_query_dev, dir_dev, range_dev, gate_v_dev or barrier_v_dev,
 * nq < 0, a struct_size that is not sizeof(qd_scan_affine_opts), an unknown frame, vgm_dev with the physical frame, a noise
 * bit outside SENSOR | LATCH (the radial stage is centred on the env's own adjacent-pair observation).  An env id outside
 * [0, B) makes the query inert, its destination slots are left untouched.  QD_ERR_STATE: QD_FLAG_VALIDATE handles and
 * handles in the full charge-state space, as qd_scan2d refuses them.  Radial noise and more than two axes are not built;
 * Rx != Ry is qd_scan_grid's (without the tile search). */
typedef struct qd_scan_affine_opts {
    int32_t  struct_size;   /* = sizeof(qd_scan_affine_opts) */
    int32_t  frame;         /* QD_SCAN_VIRTUAL 0 / QD_SCAN_PHYSICAL 1 */
    int32_t  noise_flags;   /* QD_NOISE_SENSOR | QD_NOISE_LATCH; 0 = none */
    int32_t  reserved;
    uint64_t serial;        /* the observation-number word of the Philox counter */
    int64_t  stream_base;   /* query q draws from the streams of global env id stream_base + q (mod 2^32) */
    const double* vgm_dev;  /* [nq][G][G] or NULL: the env's current matrix (virtual frame only) */
    const double* gamma_dev;/* [nq] or NULL: the env's constant peak width */
    double*  occ_dst;       /* [nq][P][N] or NULL */
} qd_scan_affine_opts;
int qd_scan_affine(qd_handle* h, const int32_t* env_of_query_dev, int nq, const double* dir_dev, const double* range_dev,
                   const double* gate_v_dev, const double* barrier_v_dev, const double* sensor_v_dev, double* raw_dst,
                   float* image_dst, double* plohi_dst, const qd_scan_affine_opts* opts, void* stream);

/* Stateless dense 1-D sweeps along one DIRECTION VECTOR over the 2N controls: the reference model layer's
 * do1d_open(gate, min, max, points) over GateVoltageComposer.do1d (GateVoltageComposer.py:35-84, 213-222) for P{i}, vP{i},
 * e{i}_{j}, U{i}_{j} or any mixed-control direction, nq lines of n_points points in one call, with the measurement stages of a
 * step (sensor noise, latching ALONG the sweep) and a normalisation per line.  A line sent through qd_eval_points occupies a
 * whole slot of C*P records and is deterministic only; qd_scan_affine with a zero dy renders the same line R times.
 * Controls are indexed as in qd_scan2d.  With W0[2N] = [gate_v, sensor_v, barrier_v] of the query (the BASE POINT, as in
 * qd_scan_affine) and s = linspace(lo, hi, n_points)[t], point t has
 *   W[i] = fma(s, d[i], W0[i])      i = 0..2N-1
 * and the model sees W through the frame as in qd_scan2d.  The front end (csrc/qd_line.h qd_line_voltages) performs the
 * operations of qd_scan_affine's in the same order: with dx = d, dy = 0 and R = n_points, row 0 of that scan has the bits of
 * the line on a QD_FLAG_PIXEL_SEARCH handle, with noise too under the same serial and stream base (row 0 of an image and a
 * line share the point indices, the start of the telegraph chain and the latching walk).  raw equals qd_eval_points at the
 * points' voltages bit for bit.
 *   env_of_query_dev [nq]       int32, the env whose device renders query q
 *   n_points                    points per line, 1..P of the handle, the same for all queries of the call
 *   dir_dev          [nq][2N]   the direction d of query q.  The zero vector is legal: it repeats the base point.
 *                               Non-finite coefficients are NOT looked for
 *   range_dev        [nq][2]    lo, hi of the scalar s; lo > hi sweeps downwards, lo == hi repeats a point
 *   gate_v_dev       [nq][N], barrier_v_dev [nq][N-1], sensor_v_dev [nq] or NULL (0.0): the base point
 *   raw_dst          [nq][n]    float64 unnormalised signal; may be NULL
 *   image_dst        [nq][n]    float32, normalised per line with its own 0.5 / 99.5 percentiles (all zero for a constant
 *                               line); may be NULL
 *   plohi_dst        [nq][2]    those percentiles; may be NULL
 * opts (NULL: virtual frame, deterministic): the fields of qd_scan_affine_opts with the same meaning, except
 *   occ_dst       [nq][n][N] float64 or NULL: the occupations the signal was formed from (after latching, if it ran)
 *   noise_flags   QD_NOISE_LATCH walks the line as ONE row of n points: the held state starts at point 0 and is never reset
 *                 (an image resets it at every row start), the Philox counter of point t is t.  QD_NOISE_SENSOR: the
 *                 telegraph chain starts at point 0, white noise is keyed by the point index; the channel word is 0
 * A query occupies one slot of its OWN size: Rl x Rl records with Rl = ceil(sqrt(n)), record p = point p, the Rl*Rl - n tail
 * records inert (all zero: no search, no eigen task).  With n <= P, Rl <= R.  Per launch: gather, telegraph chain, the line
 * front kernel (records in the hand-over form of the tile search), the redo instantiation of the per-pixel search, the
 * ground-state kernels, the latching walk, the sensor stage, a pack of the n leading values of each slot into a dense row,
 * the percentile kernel, the write -- the kernels of a step with the slot geometry as data, four small kernels of the
 * line's own (csrc/qd_line.h) and the scans' write kernel (csrc/qd_query.h).  Slots in flight per launch: what lane 0's record buffer (qd_chunk_envs * C * P records) and
 * slabs hold, floor(qd_chunk_envs * C * P / Rl^2) and floor(slab capacity / ceil(Rl^2 / 256)), at most QD_LINE_SLOTS.
 * Stream-ordered with no host wait after the first call, which allocates the scratch with hipMalloc (per slot in flight: a
 * parameter copy, a state block, Rl^2 + n doubles of signal, 2 of percentiles, one descriptor of 2 + 2*8 doubles and the
 * frame, 152 bytes; Rl^2*N doubles of occupations and ceil(Rl^2/64) telegraph words from the first call that needs them --
 * 11.3 KB per 64-point line at 8 dots with everything, 46 MB for 4096 of them); a later call with more slots or longer lines grows it (hipFree waits
 * for the device); qd_destroy frees it.  Calls of qd_scan1d belong on the stream qd_scan2d and qd_scan_affine use on that
 * handle.  nq may exceed B, many queries may name one env, and results do not depend on how queries fall into launches.
 * The call changes nothing that qd_step, qd_observe, qd_probe*, qd_scan2d, qd_scan_affine, qd_eval_points or any qd_get_*
 * function can see.
 * QD_ERR_ARG, found without reading the device: NULL env_of_query_dev, dir_dev, range_dev, gate_v_dev or barrier_v_dev,
 * nq < 0, n_points outside 1..P, a struct_size that is not sizeof(qd_scan1d_opts), an unknown frame, vgm_dev with the
 * physical frame, a noise bit outside SENSOR | LATCH (the radial stage is centred on the env's own adjacent-pair
 * observation).  An env id outside [0, B) makes the query inert, its destination slots are left untouched.  QD_ERR_STATE:
 * QD_FLAG_VALIDATE handles and handles in the full charge-state space, as qd_scan2d refuses them.  nq == 0 does nothing.
 * Radial noise, lines longer than P, different lengths within one call and eigenvalues per point are not built. */
#define QD_LINE_SLOTS 4096
typedef struct qd_scan1d_opts {
    int32_t  struct_size;   /* = sizeof(qd_scan1d_opts) */
    int32_t  frame;         /* QD_SCAN_VIRTUAL 0 / QD_SCAN_PHYSICAL 1 */
    int32_t  noise_flags;   /* QD_NOISE_SENSOR | QD_NOISE_LATCH; 0 = none */
    int32_t  reserved;
    uint64_t serial;        /* the observation-number word of the Philox counter */
    int64_t  stream_base;   /* query q draws from the streams of global env id stream_base + q (mod 2^32) */
    const double* vgm_dev;  /* [nq][G][G] or NULL: the env's current matrix (virtual frame only) */
    const double* gamma_dev;/* [nq] or NULL: the env's constant peak width */
    double*  occ_dst;       /* [nq][n][N] or NULL */
} qd_scan1d_opts;
int qd_scan1d(qd_handle* h, const int32_t* env_of_query_dev, int nq, int n_points, const double* dir_dev,
              const double* range_dev, const double* gate_v_dev, const double* barrier_v_dev, const double* sensor_v_dev,
              double* raw_dst, float* image_dst, double* plohi_dst, const qd_scan1d_opts* opts, void* stream);

/* Stateless 2-D scans on any nx x ny GRID of points along two DIRECTION VECTORS over the 2N controls: the reference model
 * layer's do2d_open(x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points) over GateVoltageComposer.do2d
 * (GateVoltageComposer.py:224-255), which takes the two point counts from the caller -- a detuning axis at 128 points
 * against a barrier at 16, a coarse 24 x 24 preview on a 64 x 64 handle, a thin band around a transition -- nq grids in one
 * call, at the cost of their point count, with the measurement stages of a step (sensor noise, latching along every row)
 * and one normalisation per grid.  A grid sent through qd_eval_points is deterministic only, is not normalised and takes a
 * whole slot of C*P records per group.
 * Controls are indexed as in qd_scan2d.  With W0[2N] = [gate_v, sensor_v, barrier_v] of the query (the BASE POINT, as in
 * qd_scan_affine), sx = linspace(x_lo, x_hi, nx)[x] and sy = linspace(y_lo, y_hi, ny)[y], point (row y, column x) has
 *   W[i] = fma(sy, dy[i], fma(sx, dx[i], W0[i]))      i = 0..2N-1
 * and the model sees W through the frame as in qd_scan2d.  The front end (csrc/qd_grid.h qd_grid_voltages) performs the
 * operations of qd_scan_affine's in the same order.  Held bit for bit:
 *   1. nx = ny = R of the handle: raw, occupations, percentiles and image equal qd_scan_affine with the same arguments on a
 *      QD_FLAG_PIXEL_SEARCH handle, with noise too under the same serial and stream_base (Rl = R: point indices, telegraph
 *      chain and row walks coincide).
 *   2. ny = 1, dy = 0: every output equals qd_scan1d with n_points = nx, d = dx, [lo, hi] = [x_lo, x_hi], noise included.
 *   3. raw equals qd_eval_points at the points' voltages on any handle; occ_dst equals it under the conditions qd_scan1d
 *      documents.
 *   env_of_query_dev [nq]          int32, the env whose device renders query q
 *   nx, ny                         columns and rows, nx >= 1, ny >= 1, nx*ny <= P of the handle, the same for all queries
 *   dir_dev          [nq][2][2N]   dx then dy of query q, as qd_scan_affine.  Zero vectors are legal
 *   range_dev        [nq][4]       x_lo, x_hi, y_lo, y_hi; lo > hi sweeps downwards, lo == hi repeats a point
 *   gate_v_dev       [nq][N], barrier_v_dev [nq][N-1], sensor_v_dev [nq] or NULL (0.0): the base point
 *   raw_dst          [nq][ny][nx]  float64 unnormalised signal; may be NULL
 *   image_dst        [nq][ny][nx]  float32, normalised with ONE 0.5 / 99.5 percentile pair per grid (all zero for a
 *                                  constant grid); may be NULL
 *   plohi_dst        [nq][2]       those percentiles; may be NULL
 * opts (NULL: virtual frame, deterministic): the fields of qd_scan_affine_opts in the same order with the same meaning, except
 *   occ_dst       [nq][ny][nx][N] float64 or NULL: the occupations the signal was formed from (after latching, if it ran)
 *   noise_flags   QD_NOISE_LATCH: the held state is reset at every row start; row y is walked as qd_latch_row on the nx
 *                 points from y*nx, the Philox counter of a point is y*nx + x.  QD_NOISE_SENSOR: the telegraph chain runs
 *                 over the slot's Rl*Rl states from point 0, as a line's; white noise is keyed by the point index
 *                 p = y*nx + x; the channel word is 0.  QD_NOISE_RADIAL is QD_ERR_ARG
 *   gamma_dev     [nq] or NULL: the env's constant peak width (the width is constant, as in qd_scan_affine)
 * A query occupies one slot of its OWN size: Rl x Rl records with Rl = ceil(sqrt(nx*ny)), record p = y*nx + x, the
 * Rl*Rl - nx*ny tail records inert, as in a line's slot.  Per launch: gather, telegraph chain, the grid front kernel, the
 * redo instantiation of the per-pixel search, the ground-state kernels, the latching walk (one lane per slot and row), the
 * sensor stage, the pack of the nx*ny leading values into a dense row, the percentile kernel, the write -- the kernels of a
 * step with the slot geometry as data, qd_scan1d's pack, the scans' write kernel (csrc/qd_query.h) and three small kernels of
 * the grid's own (csrc/qd_grid.h).  The tile
 * search does not run: its tiles are cut from R x R images.  Slots in flight per launch: those of a line of nx*ny points, at
 * most QD_GRID_SLOTS.  Stream-ordered with no host wait after the first call.  The scratch is qd_scan1d's (a call of either
 * grows it for both; hipFree waits for the device) and one descriptor per slot in flight of 4 + 4*8 doubles, the two
 * counts and the frame, 304 bytes, allocated by the first call, grown by a later one with more slots, freed by qd_destroy.
 * Calls of qd_scan_grid belong on the stream qd_scan2d, qd_scan_affine and qd_scan1d use on that handle: it shares its
 * buffers with qd_scan1d and lane 0's records with all of them.  nq may exceed B, many queries may name one env, and results
 * do not depend on how queries fall into launches.  The call changes nothing that qd_step, qd_observe, qd_probe*, qd_scan2d,
 * qd_scan_affine, qd_scan1d, qd_eval_points or any qd_get_* function can see.
 * QD_ERR_ARG, found without reading the device and before the state of the handle is looked at: NULL env_of_query_dev,
 * dir_dev, range_dev, gate_v_dev or barrier_v_dev, nq < 0, nx < 1, ny < 1 or nx*ny > P, a struct_size that is not
 * sizeof(qd_scan_grid_opts), an unknown frame, vgm_dev with the physical frame, a noise bit outside SENSOR | LATCH.  An env id
 * outside [0, B) makes the query inert, its destination slots are left untouched.  QD_ERR_STATE: QD_FLAG_VALIDATE handles
 * and handles in the full charge-state space, as qd_scan2d refuses them.  nq == 0 does nothing.
 * Grids of more than P points, different shapes within one call, the tile search on a rectangular slot and radial noise
 * are not built. */
#define QD_GRID_SLOTS 4096
typedef struct qd_scan_grid_opts {
    int32_t  struct_size;   /* = sizeof(qd_scan_grid_opts) */
    int32_t  frame;         /* QD_SCAN_VIRTUAL 0 / QD_SCAN_PHYSICAL 1 */
    int32_t  noise_flags;   /* QD_NOISE_SENSOR | QD_NOISE_LATCH; 0 = none */
    int32_t  reserved;
    uint64_t serial;        /* the observation-number word of the Philox counter */
    int64_t  stream_base;   /* query q draws from the streams of global env id stream_base + q (mod 2^32) */
    const double* vgm_dev;  /* [nq][G][G] or NULL: the env's current matrix (virtual frame only) */
    const double* gamma_dev;/* [nq] or NULL: the env's constant peak width */
    double*  occ_dst;       /* [nq][ny][nx][N] or NULL */
} qd_scan_grid_opts;
int qd_scan_grid(qd_handle* h, const int32_t* env_of_query_dev, int nq, int nx, int ny, const double* dir_dev,
                 const double* range_dev, const double* gate_v_dev, const double* barrier_v_dev, const double* sensor_v_dev,
                 double* raw_dst, float* image_dst, double* plohi_dst, const qd_scan_grid_opts* opts, void* stream);

/* The CLOSED regime: the dot array is isolated from its reservoirs and holds exactly n_charge carriers -- the reference model
 * class's ground_state_closed / charge_sensor_closed (qd_eval_points_closed) and do1d_closed / do2d_closed
 * (qd_scan_grid_closed; TunnelCoupledChargeSensed.py:256-268, 291-309, 382-426).  The reference's own ground-state half is
 * not defined there; the definition built here (DESIGN "closed regime") is the open algorithm restricted to one total-charge
 * sector.  With the front end of the open call (vpp, tc, the voltage-dependent-capacitance scales, the scaled v'):
 *   centre   m = argmin (n - v')^T A (n - v') over n >= 0, sum(n) = Q, A = cdd_inv[:N,:N], by a primal active-set iteration
 *   kept     the K = num_charge_states lowest by (E, index) of c = floor(m) + delta, delta in {-1,0,1,2}^N, c >= 0,
 *            sum(c) = Q, with the canonical energy and index of the open search, in the reference order
 * (csrc/qd_closed.h, one kernel in the place of the open search's); fewer than K candidates (always at 2 and 3 dots) give
 * an nv x nv problem.  The ground-state kernels and the noise-free sensor expression then run unchanged; the tunnelling
 * Hamiltonian conserves the total charge, so the occupations sum to n_charge.
 *
 * qd_eval_points_closed takes the arguments of qd_eval_points and
 *   n_charge_host    [ng]        HOST int32, the total charge of each group, 0..32767
 *   states_dst       [np][K][N]  DEVICE int32 or NULL: the kept states of every point in list order, zeros behind the
 *                                candidates found
 * The lists are in the reference order as they come, so signal and occupations come from one run of the ground-state stage.
 * qd_scan_grid_closed takes the arguments of qd_scan_grid and
 *   n_charge_dev     [nq]        DEVICE int32, the total charge of each query, 0..32767
 * It runs qd_scan_grid's slot loop with the one kernel exchanged, so a closed grid in the physical frame equals
 * qd_eval_points_closed at the grid's voltages bit for bit in occupations and raw signal.  opts->noise_flags != 0 is QD_ERR_ARG:
 * latching and sensor noise in the closed regime are not built.
 * Both calls are stateless and stream-ordered, share scratch and stream discipline with their open siblings and change
 * nothing that any other call can see.  QD_ERR_ARG: what the open sibling refuses, a NULL n_charge array, an n_charge outside
 * 0..32767 (qd_scan_grid_closed reads n_charge_dev back for this check and waits for `stream` once per call).  QD_ERR_STATE:
 * QD_FLAG_VALIDATE handles and handles in the full charge-state space, as the open siblings.  qd_step, the tile search, the
 * full space and the noise stages have no closed form here. */
int qd_eval_points_closed(qd_handle* h, const int32_t* group_env_host, const int64_t* group_start_host, int ng,
                          const double* vg_dev, const double* vb_dev, const double* gamma_host, const int32_t* n_charge_host,
                          double* signal_dst, double* occ_dst, int32_t* states_dst, void* stream);
int qd_scan_grid_closed(qd_handle* h, const int32_t* env_of_query_dev, int nq, int nx, int ny, const double* dir_dev,
                        const double* range_dev, const double* gate_v_dev, const double* barrier_v_dev,
                        const double* sensor_v_dev, const int32_t* n_charge_dev, double* raw_dst, float* image_dst,
                        double* plohi_dst, const qd_scan_grid_opts* opts, void* stream);

/* ENERGY LEVELS per point: qd_eval_points_ex is qd_eval_points / qd_eval_points_closed with an options struct that can also
 * ask for the lowest eigenvalues of every point's Hamiltonian (csrc/qd_levels.h, one kernel, one point per wavefront).
 *   Kept states.   For a point with kept list s_0 .. s_{K-1} (K = num_charge_states) the search leaves indices, floors, the
 *                  number of valid candidates nvalid, the tunnel couplings and the energies E.  Let nv = min(nvalid, K).
 *   Hamiltonian.   H = diag(E_0 .. E_{nv-1}) + H_t over those nv states: the reference's matrix of hamiltonian_build.py:75-137
 *                  with the |0..0> PADDING COPIES LEFT OUT (they are always isolated and would only add copies of one
 *                  diagonal entry).  E is the search's canonical energy, absolute, with the 1 / s_a factor of the
 *                  voltage-dependent capacitance model included.
 *   Levels.        level[k], k = 0 .. L-1, is the k-th smallest eigenvalue of H counted with multiplicity; k >= nv gives +inf.
 *                  L = n_levels is in 1 .. QD_LEVELS_MAX.  Equal eigenvalues come back bitwise equal, and level[k] <=
 *                  level[k + 1] always.  Accuracy: 1e-12 ||H||_inf, the bar of the ground-state solvers.
 *   Norm.          hnorm = ||H||_inf = max_i (|E_i| + sum_j |H_ij|), unshifted.
 *   Resolvability. The project's measure is rel_gap = (level[1] - level[0]) / hnorm: below about 1e-9 float64 does not
 *                  resolve the ground vector, and the point's occupations and signal are round-off, here as in the
 *                  reference's eigh.  (A spectrum that includes the padding copies reports gap 0 wherever |0..0> is the
 *                  ground state of a short list; this one does not.)
 *   Truncation.    The levels are those of the reference's TRUNCATED K-state Hamiltonian, not of the infinite system: an
 *                  excited level is only as good as the kept list around the ground state.
 *   Closed regime. With n_charge_host the same definition applies on the closed list (one total-charge sector, nvalid = nv).
 * The levels kernel runs right behind the search, on the list as the search left it and before anything reorders it, so
 * repeated calls give the same bits.  opts == NULL or n_levels == 0 launches exactly what qd_eval_points (n_charge_host NULL)
 * or qd_eval_points_closed launches, with the same bits.  With signal_dst == occ_dst == NULL and n_levels > 0 the
 * ground-state stage is not launched at all.  Stateless and stream-ordered as its siblings.
 * QD_ERR_ARG: what the siblings refuse; opts->struct_size != sizeof(qd_points_opts); n_levels outside 0..QD_LEVELS_MAX;
 * n_levels > 0 with levels_dst NULL; states_dst without n_charge_host.  QD_ERR_STATE: QD_FLAG_VALIDATE handles and handles in
 * the full charge-state space, as the siblings.  Levels over a grid are qd_scan_grid_levels below.  Eigenvectors of excited
 * levels, noisy or latched points and levels inside qd_step, probes, scans and lines are not built. */
#define QD_LEVELS_MAX 8
typedef struct qd_points_opts {
    int32_t struct_size;            /* = sizeof(qd_points_opts) */
    int32_t n_levels;               /* 0: none */
    const double*  gamma_host;      /* as qd_eval_points' gamma */
    const int32_t* n_charge_host;   /* NULL: open regime; else the closed regime, as qd_eval_points_closed */
    int32_t* states_dst;            /* closed regime only, as qd_eval_points_closed */
    double*  levels_dst;            /* [points][n_levels], device */
    double*  hnorm_dst;             /* [points], device, may be NULL */
} qd_points_opts;
int qd_eval_points_ex(qd_handle* h, const int32_t* group_env_host, const int64_t* group_start_host, int ng,
                      const double* vg_dev, const double* vb_dev, double* signal_dst, double* occ_dst,
                      const qd_points_opts* opts, void* stream);

/* FINITE TEMPERATURE per point: qd_eval_points_thermal is qd_eval_points / qd_eval_points_closed with the thermal state
 * rho = exp(-H / kT) / Z in place of the ground state (csrc/qd_thermal.h, one kernel, one point per wavefront).
 *   Hamiltonian.   The H of qd_eval_points_ex above: diag(E_0 .. E_{nv-1}) + H_t over the nv = min(nvalid, K) valid kept states,
 *                  the |0..0> padding copies left out (a copy would carry Boltzmann weight of its own).
 *   kT.            kT_host[g] > 0 and finite, one per group, in the energy units of the levels of qd_eval_points_ex.  The
 *                  reference's conversion from its temperature field, as written, is kT = 8.617333262145e-5 * T.
 *   Populations.   With H V = V diag(lam), w_k = exp(-(lam_k - lam_min) / kT) / Z:  P_m = sum_k w_k V[m,k]^2 is the
 *                  probability of kept state s_m.  A weight that underflows to zero is expected.  At an exact degeneracy
 *                  the state is the equal mixture: no point needs the rel_gap exemption of the ground state.  Pairs
 *                  whose coupling is exactly zero never mix: tc == 0 gives the classical Boltzmann distribution.
 *   Outputs.       occ_dst [points][N]: <n_d> = sum_m P_m s_m[d].  signal_dst [points]: the noise-free sensor signal of
 *                  qd_eval_points evaluated at those occupations (c0 = 2 b + a (2 (Ns - v''_s) + 1), ten Lorentzians).
 *                  opts->var_dst [points][N]: sum_m P_m (s_m[d] - <n_d>)^2.  opts->ztail_dst [points]: the normalised
 *                  weight w of the HIGHEST of the nv levels.  Any of the four may be NULL.
 *   Truncation.    The state is that of the reference's TRUNCATED K-state Hamiltonian, not of the infinite system.  ztail is
 *                  the caller's check: where it is not negligible (against the accuracy wanted of <n>), states outside the
 *                  kept list would carry weight too, and K kept states are too few for this kT.
 *   Accuracy.      Populations within 4 (1e-12 ||H - min(diag H)||_inf + 1e-13 ||H||_inf) min(1 / kT, 1 / (lam_1 - lam_0))
 *                  of an eigh of the oracle's matrix (tests/thermal_helpers.py).
 * The call runs on the slot loop of its siblings (same slots, QD_POINTS_SLOTS, same scratch); the thermal kernel takes the
 * place of the ground-state stage, on the list as the search left it, once: signal and occupations come from one solve.
 * opts == NULL: the open regime and each env's own peak width.  Stateless, stream-ordered, deterministic: repeated calls
 * give the same bits, and nothing any other call can see changes.
 * QD_ERR_ARG (decided on the host, before anything is launched): what the siblings refuse; kT_host NULL; a kT that is not
 * finite or not > 0; opts->struct_size != sizeof(qd_thermal_opts).  QD_ERR_STATE: QD_FLAG_VALIDATE handles and handles in the
 * full charge-state space, as the siblings.  Grids at a temperature are qd_scan_grid_thermal below.  Temperature inside
 * qd_step, probes, scans and lines, noisy or latched thermal points and eigenvectors returned to the caller are not built. */
typedef struct qd_thermal_opts {
    int32_t struct_size;            /* = sizeof(qd_thermal_opts) */
    int32_t reserved;               /* 0 */
    const double*  gamma_host;      /* as qd_eval_points' gamma */
    const int32_t* n_charge_host;   /* NULL: open regime; else the closed regime, as qd_eval_points_closed */
    double* var_dst;                /* [points][N], device, may be NULL */
    double* ztail_dst;              /* [points], device, may be NULL */
} qd_thermal_opts;
int qd_eval_points_thermal(qd_handle* h, const int32_t* group_env_host, const int64_t* group_start_host, int ng,
                           const double* vg_dev, const double* vb_dev, const double* kT_host,
                           double* signal_dst, double* occ_dst, const qd_thermal_opts* opts, void* stream);

/* CHARGE RESPONSE per point: qd_eval_points_response is qd_eval_points_thermal plus the derivatives of the thermal
 * occupations and of the signal at the point (csrc/qd_response.h, an epilogue of the thermal kernel in a kernel of its own).
 *   Model.         The H, kT and populations of qd_eval_points_thermal.  The kept list is held FIXED: the response is the
 *                  derivative of the TRUNCATED K-state model at this point, not of the infinite system (see Truncation above);
 *                  across a voltage where the kept set changes it is the derivative of the model on this side.
 *   chi_dst        [points][N][2N-1].  Columns 0..N-1: d<n_i>/d(eps_k) for H + eps_k n_k; symmetric, negative semidefinite,
 *                  -cov(n_i, n_k) / kT exactly when every tc is zero.  Columns N..2N-2: d<n_i>/d(ln tc_d); a pair with
 *                  tc_d == 0 gives an exact zero column.  A point with one valid state gives zeros.
 *   jac_dst        [points][N][2N]: d<n_i>/dv_j over v = (vg[0..N], vb[0..N-2]) = sum_k chi[i][k] Lam[k][j] +
 *                  sum_d chi[i][N+d] Gam[d][j], Lam = -2 cdd_inv[:N,:N] cgd[:N], Gam[d][j] = -alpha_d d(vb_eff_d)/dv_j.
 *   dsignal_dst    [points][2N]: dS/dv_j = S'(c0) dc0/dv_j with the c0 and S of qd_eval_points_thermal,
 *                  dc0/dv_j = 2 sum_i A[N][i] (jac[i][j] - cgd[i][j]) - 2 A[N][N] cgd[N][j].  Ns = rint(v''_s) is piecewise
 *                  constant and its jumps are not differentiated; the peak width gamma is taken as constant.
 *   Accuracy.      tests/response_helpers.py: chi within 8 n_max^2 (1e-12 hs + 1e-13 hn) min(1/kT, 1/g)^2 + 1e-12 n_max^2 / kT.
 * Any of the three may be NULL; with all three NULL (or opts NULL) the call launches exactly what qd_eval_points_thermal
 * launches, with the same bits.  signal_dst, occ_dst, var_dst and ztail_dst have the bits of qd_eval_points_thermal in
 * every case.  Open and closed regime, the slot loop, checks and scratch of the siblings.
 * QD_ERR_ARG and QD_ERR_STATE: what qd_eval_points_thermal refuses, and, when a response destination is given, QD_ERR_STATE
 * when a named env carries the voltage-dependent capacitance model (its per-point scale factors make Lam depend on v; that chain rule is not built).
 * Grids are qd_scan_grid_response below.  Not built: the response on lines, scans, probes and in qd_step, and a separate
 * T = 0 path (the ground-state response is the kT -> 0 limit of this one). */
typedef struct qd_response_opts {
    int32_t struct_size;            /* = sizeof(qd_response_opts) */
    int32_t reserved;               /* 0 */
    const double*  gamma_host;      /* as qd_eval_points' gamma */
    const int32_t* n_charge_host;   /* NULL: open regime; else the closed regime, as qd_eval_points_closed */
    double* var_dst;                /* [points][N], device, may be NULL */
    double* ztail_dst;              /* [points], device, may be NULL */
    double* chi_dst;                /* [points][N][2N-1], device, may be NULL */
    double* jac_dst;                /* [points][N][2N], device, may be NULL */
    double* dsignal_dst;            /* [points][2N], device, may be NULL */
} qd_response_opts;
int qd_eval_points_response(qd_handle* h, const int32_t* group_env_host, const int64_t* group_start_host, int ng,
                            const double* vg_dev, const double* vb_dev, const double* kT_host,
                            double* signal_dst, double* occ_dst, const qd_response_opts* opts, void* stream);

/* FINITE TEMPERATURE on a grid: qd_scan_grid_thermal is qd_scan_grid / qd_scan_grid_closed with the thermal state of
 * qd_eval_points_thermal at every point in place of the ground state -- the thermally broadened charge-stability diagram.
 * It takes the arguments of qd_scan_grid and
 *   kT_dev         [nq] DEVICE float64: kT of each query, finite and > 0, in the units of qd_eval_points_thermal.  The call reads
 *                  it back for this check and waits for `stream` once, as qd_scan_grid_closed does for n_charge_dev
 *   topts          NULL: the open regime, no further outputs.  n_charge_dev [nq] DEVICE int32 or NULL: the closed regime of
 *                  qd_scan_grid_closed.  var_dst [nq][ny][nx][N], ztail_dst [nq][ny][nx] DEVICE float64 or NULL: the variances
 *                  of the occupations and the normalised weight of the highest kept level, as qd_eval_points_thermal defines them
 * Hamiltonian, populations, truncation and accuracy are those of qd_eval_points_thermal.  raw, image, plohi and opts->occ_dst are
 * those of the thermal state: the sensor expression at <n>, the grid's own percentiles of that signal.
 * The call runs qd_scan_grid's slot loop with ONE kernel exchanged: the thermal grid kernel of csrc/qd_thermal_blocks.h, one
 * point per wavefront, takes the place of the ground-state kernels.  Its solver is not the one of qd_eval_points_thermal: the Jacobi
 * iteration runs inside the connected components of the coupling pattern only (states of different components never mix;
 * exact zeros do not link), so a sweep has as many rounds as the largest component needs, not as the whole list.  The two
 * calls agree within the sum of their tolerances at the same voltages and are NOT bitwise equal in the open regime.  A closed
 * list is one total-charge sector, which hops connect: one component, so the closed regime runs the kernel on the whole-block
 * solver of qd_eval_points_thermal, and a closed thermal grid in the physical frame equals that call at the grid's voltages
 * bit for bit, as qd_scan_grid_closed equals qd_eval_points_closed.  Results do not depend on how queries fall into launches,
 * and repeated calls give the same bits.
 * Noise: QD_NOISE_SENSOR is allowed in the open regime (the sensor stage reads the thermal c0 alone).  QD_NOISE_LATCH is
 * QD_ERR_ARG: the latching model holds an integer configuration, and a thermal mean has none.
 * QD_ERR_ARG: what qd_scan_grid refuses; kT_dev NULL; a kT that is not finite or not > 0; topts->struct_size !=
 * sizeof(qd_grid_thermal_opts); QD_NOISE_LATCH; any noise flag together with n_charge_dev; an n_charge outside 0..32767.
 * QD_ERR_STATE: QD_FLAG_VALIDATE handles and handles in the full charge-state space.  Stateless and stream-ordered as its
 * siblings, on their scratch; nothing any other call can see changes.  Temperature in qd_scan1d, qd_scan2d, qd_scan_affine,
 * probes and qd_step and latched thermal points are not built.  Levels over a grid are qd_scan_grid_levels below. */
typedef struct qd_grid_thermal_opts {
    int32_t struct_size;            /* = sizeof(qd_grid_thermal_opts) */
    int32_t reserved;               /* 0 */
    const int32_t* n_charge_dev;    /* NULL: open regime; else [nq], the closed regime, as qd_scan_grid_closed */
    double* var_dst;                /* [nq][ny][nx][N], device, may be NULL */
    double* ztail_dst;              /* [nq][ny][nx], device, may be NULL */
} qd_grid_thermal_opts;
int qd_scan_grid_thermal(qd_handle* h, const int32_t* env_of_query_dev, int nq, int nx, int ny, const double* dir_dev,
                         const double* range_dev, const double* gate_v_dev, const double* barrier_v_dev,
                         const double* sensor_v_dev, const double* kT_dev, double* raw_dst, float* image_dst,
                         double* plohi_dst, const qd_scan_grid_opts* opts, const qd_grid_thermal_opts* topts, void* stream);

/* CHARGE RESPONSE on a grid: qd_scan_grid_response is qd_scan_grid_thermal plus, at every point, the derivatives of
 * qd_eval_points_response -- the lock-in charge-stability diagram dS/dV along the sweep axis, and the slopes d<n_i>/dV_j along a
 * transition line.  It takes the arguments of qd_scan_grid_thermal, with ropts in place of topts:
 *   n_charge_dev, var_dst, ztail_dst   as in qd_grid_thermal_opts
 *   chi_dst        [nq][ny][nx][N][2N-1], jac_dst [nq][ny][nx][N][2N], dsignal_dst [nq][ny][nx][2N]: chi, the jacobian and dS/dv
 *                  as qd_eval_points_response defines them, over the PHYSICAL voltages v = (vg[0..N], vb[0..N-2]), in either frame
 *   docc_axes_dst  [nq][ny][nx][N][2] = jacobian . (u_x, u_y);  dsignal_axes_dst [nq][ny][nx][2] = dsignal . (u_x, u_y):
 *                  the derivatives along the two axes of the grid, per unit of the axis scalars sx, sy (not per pixel).
 *                  u = dv/ds is the physical direction of one step of the scalar: the direction vector itself in the physical
 *                  frame; in the virtual frame u[:G] = vgm u_dir[:G] with the slot's virtual gate matrix (the query's vgm_dev
 *                  if given, else the env's) and u[G:] = dir[G:].  All sums run over j = 0 .. 2N-1 in index order with fma.
 * DEVICE float64, any subset may be NULL.  With all five NULL (or ropts NULL) the call launches exactly what
 * qd_scan_grid_thermal launches.  raw, image, plohi, opts->occ_dst, var_dst and ztail_dst have the bits of
 * qd_scan_grid_thermal under the same arguments in every case.  The slope S'(c0) is taken at the c0 of the thermal state with
 * the slot's constant peak width (opts->gamma_dev if given); QD_NOISE_SENSOR is allowed in the open regime as in
 * qd_scan_grid_thermal, and the response is that of the NOISELESS expression: its bits do not depend on noise_flags.
 * The call runs qd_scan_grid_thermal's launches with the thermal kernel exchanged for the one of csrc/qd_response_blocks.h.  Open
 * regime: the epilogue runs inside the hop components that the per-component thermal solver found (G = V^T X V and D o G are
 * block diagonal over them; only Z and <X> are global); it agrees with qd_eval_points_response at the same voltages within the
 * sum of both tolerances, not bit for bit.  Closed regime: one component, the whole-block solver and epilogue of
 * qd_eval_points_response, and in the physical frame chi, jac and dsignal equal that call at the grid's voltages bit for bit.
 * QD_ERR_ARG and QD_ERR_STATE: what qd_scan_grid_thermal refuses (QD_NOISE_LATCH included); ropts->struct_size !=
 * sizeof(qd_grid_response_opts); and, when a response destination is given, QD_ERR_STATE for a live query whose env carries the
 * voltage-dependent capacitance model (the call reads env_of_query_dev back for this check).  Not built: the response in
 * qd_scan1d, qd_scan2d, qd_scan_affine, probes and qd_step, and latched thermal points. */
typedef struct qd_grid_response_opts {
    int32_t struct_size;            /* = sizeof(qd_grid_response_opts) */
    int32_t reserved;               /* 0 */
    const int32_t* n_charge_dev;    /* NULL: open regime; else [nq], the closed regime, as qd_scan_grid_closed */
    double* var_dst;                /* [nq][ny][nx][N], device, may be NULL */
    double* ztail_dst;              /* [nq][ny][nx], device, may be NULL */
    double* chi_dst;                /* [nq][ny][nx][N][2N-1], device, may be NULL */
    double* jac_dst;                /* [nq][ny][nx][N][2N], device, may be NULL */
    double* dsignal_dst;            /* [nq][ny][nx][2N], device, may be NULL */
    double* docc_axes_dst;          /* [nq][ny][nx][N][2], device, may be NULL */
    double* dsignal_axes_dst;       /* [nq][ny][nx][2], device, may be NULL */
} qd_grid_response_opts;
int qd_scan_grid_response(qd_handle* h, const int32_t* env_of_query_dev, int nq, int nx, int ny, const double* dir_dev,
                          const double* range_dev, const double* gate_v_dev, const double* barrier_v_dev,
                          const double* sensor_v_dev, const double* kT_dev, double* raw_dst, float* image_dst,
                          double* plohi_dst, const qd_scan_grid_opts* opts, const qd_grid_response_opts* ropts, void* stream);

/* ENERGY LEVELS on a grid: qd_scan_grid_levels is qd_scan_grid / qd_scan_grid_closed that also hands out the lowest eigenvalues
 * and ||H||_inf of qd_eval_points_ex at every point -- the gap map levels[1] - levels[0] over, say, detuning x barrier, and
 * rel_gap = gap / hnorm, the validity mask of the T = 0 diagram.  It takes the arguments of qd_scan_grid and
 *   lopts          required.  n_levels in 1..QD_LEVELS_MAX.  n_charge_dev [nq] DEVICE int32 or NULL: the closed regime of
 *                  qd_scan_grid_closed.  levels_dst [nq][ny][nx][n_levels] DEVICE float64, required; hnorm_dst [nq][ny][nx]
 *                  DEVICE float64 or NULL.
 * Hamiltonian, levels (+inf from nv on, non-decreasing, equal eigenvalues bitwise equal), norm, truncation and the accuracy
 * of 1e-12 ||H||_inf are those of qd_eval_points_ex.
 * The call runs qd_scan_grid's slot loop with ONE kernel added: the levels grid kernel of csrc/qd_levels_blocks.h, one point
 * per wavefront, right behind the search and BEFORE the ground-state stage, on the list as the search left it.  Every other
 * launch is that of qd_scan_grid or qd_scan_grid_closed, so raw, image, plohi and opts->occ_dst equal those calls bit for bit
 * under the same arguments, sensor noise and latching in the open regime included; the levels do not depend on the noise
 * flags.  raw_dst, image_dst and plohi_dst may be NULL where qd_scan_grid allows it.
 * Open regime: the solver is not the one of qd_eval_points_ex.  The Householder tridiagonalisation runs inside the connected
 * components of the coupling pattern, all components at once (states of different components never couple; exact zeros do
 * not link), and the multisection runs on the components' tridiagonals laid side by side.  The two calls agree within the
 * sum of their bars, 2e-12 hnorm, at the same voltages and are NOT bitwise equal.  A closed list is one total-charge sector,
 * which hops connect: one component, so the closed regime runs the kernel on the whole-block solver of qd_eval_points_ex, and
 * a closed levels grid in the physical frame equals that call at the grid's voltages bit for bit.  (Measured ahead of the
 * whole-block solver in the open regime: 4 and 8 dots at K = 8 and 32; other N and K are unmeasured.)  Results do
 * not depend on how queries fall into launches, and repeated calls give the same bits.  A query with an env id outside
 * 0..B-1 writes no row.
 * QD_ERR_ARG: what qd_scan_grid or (with n_charge_dev) qd_scan_grid_closed refuse; lopts NULL; lopts->struct_size !=
 * sizeof(qd_grid_levels_opts); n_levels outside 1..QD_LEVELS_MAX; levels_dst NULL.  QD_ERR_STATE: QD_FLAG_VALIDATE handles
 * and handles in the full charge-state space.  Stateless and stream-ordered as its siblings, on their scratch; nothing any
 * other call can see changes.  Eigenvectors or occupations of excited levels and levels in qd_scan1d, qd_scan2d,
 * qd_scan_affine, probes and qd_step are not built. */
typedef struct qd_grid_levels_opts {
    int32_t struct_size;            /* = sizeof(qd_grid_levels_opts) */
    int32_t n_levels;               /* 1 .. QD_LEVELS_MAX */
    const int32_t* n_charge_dev;    /* NULL: open regime; else [nq], the closed regime, as qd_scan_grid_closed */
    double* levels_dst;             /* [nq][ny][nx][n_levels], device, required */
    double* hnorm_dst;              /* [nq][ny][nx], device, may be NULL */
} qd_grid_levels_opts;
int qd_scan_grid_levels(qd_handle* h, const int32_t* env_of_query_dev, int nq, int nx, int ny, const double* dir_dev,
                        const double* range_dev, const double* gate_v_dev, const double* barrier_v_dev,
                        const double* sensor_v_dev, double* raw_dst, float* image_dst, double* plohi_dst,
                        const qd_scan_grid_opts* opts, const qd_grid_levels_opts* lopts, void* stream);

/* Stitches one channel of nx*ny probe signals into one composite image on the device (map_device_range.py:134-170,
 * map_full_device_range.py:168-194).  raw_dev [nx*ny][C][P] as qd_probe wrote it, query index i*ny + j for scan (i, j);
 * composite_dst [ny*R][nx*R] float32; both DEVICE memory, stream-ordered, no host wait.
 *   QD_MAP_GLOBAL    scan (i, j) at rows j*R.., columns i*R..; ONE 0.5 / 99.5 percentile pair (numpy 'linear') over the
 *                    whole composite, exact (a radix select spread over the grid, same keys and interpolation as the
 *                    per-env percentiles); (z - p_lo) / (p_hi - p_lo) clipped to [0, 1], all zero when p_hi <= p_lo.
 *                    plohi_dst [2] or NULL.
 *   QD_MAP_PER_SCAN  every scan normalised with its own percentiles; row blocks flipped (block ny-1-j holds scan j).
 *                    plohi_dst [nx*ny][2] or NULL.
 * QD_ERR_ARG: NULL raw_dev or composite_dst, nx or ny < 1, more than 65535 scans, nx*ny*P >= 2^32 (the select counts in
 * 32 bits), channel outside [0, C), unknown mode.
 * Scratch (nx*ny*P doubles) is allocated on first use, grown on demand and freed by qd_destroy.  A call that allocates
 * or grows it (the first, and any with more scans than every call before) uses hipMalloc / hipFree and WAITS for the
 * device; all other calls are stream-ordered without a host wait. */
#define QD_MAP_GLOBAL 0
#define QD_MAP_PER_SCAN 1
int qd_probe_compose(qd_handle* h, const double* raw_dev, int nx, int ny, int channel, int mode,
                     float* composite_dst, double* plohi_dst, void* stream);
/* Timing hook of scripts/probe_rate.py: mean HIP-event duration over `iters` runs of the 0.5 / 99.5 percentiles of the n
 * doubles at z_dev, by the grid-wide select of QD_MAP_GLOBAL (single_block 0) or by one block of the per-env percentile
 * kernel (single_block 1); out_dev [2] receives the percentiles.  n < 2^32. */
int qd_time_select(qd_handle* h, const double* z_dev, long long n, int single_block, int iters,
                   double* out_dev, float* mean_ms, void* stream);

/* Validation / checkpoint access (blocking copies to HOST memory).
 *   state_host [B][qd_state_block_doubles], steps_host [B] int32
 *   raw_host   [B][C][P] float64 unnormalised sensor signal of the last observe
 *   plohi_host [B][2]    the 0.5 / 99.5 percentiles used
 *   occ_host   [B][C][P][N] float64 expectation occupations   (QD_FLAG_VALIDATE)
 *   states_host [B][C][P][32][N] int32 kept charge states      (QD_FLAG_VALIDATE): slots 0..K-1 the K kept states in
 *                                  the reference order, |0..0> padding included; slots K..31 are -1 */
int qd_get_state(qd_handle* h, double* state_host, int32_t* steps_host);
int qd_set_state(qd_handle* h, const double* state_host, const int32_t* steps_host);
int qd_get_raw(qd_handle* h, double* raw_host, double* plohi_host);
int qd_get_occupations(qd_handle* h, double* occ_host);
int qd_get_candidates(qd_handle* h, int32_t* states_host);
/* eig_host [B][C][P][2] float64 (QD_FLAG_VALIDATE): per pixel the ground energy of the K-state
 * Hamiltonian (K = num_charge_states; M x M in the full space) (what jnp.linalg.eigh returns first, ground_state.py:150) and the relative residual
 * ||H x - lambda x||_2 / ||H||_inf of the eigenpair the occupations were formed from. */
int qd_get_eigen(qd_handle* h, double* eig_host);
/* Counters of the tile-shared candidate search since qd_create (QD_FLAG_VALIDATE): tiles searched, tiles handed
 * whole to the per-pixel search, single pixels redone, sum of superset sizes, pixels redone for < KC valid states
 * (KC = 8, 16 or 32: the smallest of them >= K);
 * [8 + r]: tiles handed over by reason r (1 ranges, 2 seeds, 3 frontier overflow, 4 too few leaves, 5 superset size). */
int qd_get_search_stats(qd_handle* h, uint64_t* out16);
/* Counters of the ground-state kernel's eigen-solver phase since qd_create (QD_FLAG_VALIDATE): tasks (hop components of
 * >= 2 states solved), sum of their Laguerre iterations, 64-task wave tiles, sum over tiles of the largest iteration count
 * in the tile; [4 + k]: tasks of size class k (2, 3, .. 8 states, then 9..32). */
int qd_get_solver_stats(qd_handle* h, uint64_t* out16);
/* Checkpointing of the stochastic stages (SURVEY 5 "expose RNG seeds/counters"): the Philox
 * counter word that numbers the observations rendered so far by this handle. */
int qd_get_rng_state(const qd_handle* h, uint64_t* obs_serial);
int qd_set_rng_state(qd_handle* h, uint64_t obs_serial);

/* Timing hooks for bench.py: `iters` back-to-back launches over ONE launch chunk (qd_chunk_envs envs) on the current
 * data, mean duration in milliseconds measured with HIP events on `stream`.
 *   qd_time_candidates_kernel  the whole candidate search (tile search + per-pixel redo pass)
 *   qd_time_ground_kernel      the whole ground-state stage (structure + the solve launches + select)
 *   qd_time_kernels            each kernel (group) by itself; out[QD_TIMED_KERNELS] in the order of qd_timed_kernel_name:
 *                              tile search, per-pixel redo pass, ground-state structure, the solve launches of all size
 *                              classes together, ground-state select. */
#define QD_TIMED_KERNELS 5
int qd_time_ground_kernel(qd_handle* h, int iters, float* mean_ms, void* stream);
int qd_time_candidates_kernel(qd_handle* h, int iters, float* mean_ms, void* stream);
int qd_time_kernels(qd_handle* h, int iters, float* mean_ms_out, void* stream);
const char* qd_timed_kernel_name(int k);
/* Number of env-steps one launch of the hot kernels covers (scratch chunk). */
int qd_chunk_envs(const qd_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* QDSIM_H */
