/*
 * qgym.h -- C ABI of the MI355X-native batched env.step() path (libqgym.so).
 *
 * This is the drop-in boundary for qiskit-gym's Rust `env.step()` hot path.  The reference
 * exposes each environment to its callers through the `twisterl::rl::env::Env` trait
 * (implemented at rust/src/envs/clifford.rs:285-382, linear_function.rs:259-365,
 * permutation.rs:148-257, pauli.rs:492-720 of the reference) and to Python through PyO3 classes
 * registered in rust/src/lib.rs:24-31.  A Rust (or cgo / ctypes) host binds the functions below
 * instead; INTEGRATION.md shows the `impl Env` shim a maintainer would add.
 *
 * Two flavours:
 *   qg_vec_*  a batch of B independent environments resident in one GPU's HBM, stepped by one
 *             kernel launch per `step` (new surface: the reference has no vector env, every
 *             method is the batched counterpart of one trait method and cites it);
 *   qg_env_*  one environment with exactly the trait's method set (a batch of 1 on the same
 *             kernels), for callers that hold a `Box<dyn Env>`.
 *
 * Conventions: plain pointers and sizes only.  Pointers named *_dev are device pointers on the
 * handle's GPU; `stream` is a `hipStream_t` passed as `void*` (NULL = the null stream).  All
 * qg_vec_* device work is enqueued on `stream` and returns without synchronising unless stated.
 * Every function returns QG_OK (0) or a negative qg_status; qg_last_error() gives the message
 * (thread-local).  There is no CPU fallback: without a visible gfx950 device creation fails.
 */
#ifndef QGYM_H
#define QGYM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: + qg_comm_* / learner-shard entry points, qg_vec_step_host, qg_vec_observe_*_host (additions only: version-1 callers keep working)
 * 3: + qg_vec_track_dense, qg_comm_p2p_reset, qg_plan_query, qg_vec_reset_done_step, qg_env_pool_clear, qg_vec_copy_envs, qg_beam_select,
 *      qg_beam_merge, qg_beam_seen_bytes, qg_vec_twists, qg_twist_expand_packed, qg_vec_observe_twisted, qg_untwist_actions,
 *      qg_policy_head_logp, qg_policy_mid_head_logp, qg_twist_pack_words, qg_vec_observe_twisted_words, qg_beam_advance, qg_mcts_forest_bytes,
 *      qg_mcts_select, qg_mcts_backup, qg_mcts_decide, qg_mcts_rebase, qg_search_plan_query, qg_mcts_select_many,
 *      qg_mcts_backup_many, qg_az_pack_scratch_bytes, qg_az_pack (additions only) */
#define QG_ABI_VERSION 3

typedef enum {
    QG_OK = 0,
    QG_ERR_INVALID = -1,     /* bad argument (PyValueError in the reference's ctor path) */
    QG_ERR_TYPE = -2,        /* malformed gate (PyTypeError, common.rs:51-76) */
    QG_ERR_UNSUPPORTED = -3, /* outside the limits documented in DESIGN.md */
    QG_ERR_DEVICE = -4,      /* HIP runtime failure / no GPU */
    QG_ERR_PANIC = -5        /* the reference would have panicked (singular inverse, malformed Pauli state, ...) */
} qg_status;

/* rust/src/envs/common.rs:19-29 (enum order) */
typedef enum { QG_H = 0, QG_S = 1, QG_SDG = 2, QG_SX = 3, QG_SXDG = 4, QG_CX = 5, QG_CZ = 6, QG_SWAP = 7 } qg_gate_kind;

/* the four `impl Env` blocks; numbering shared with the oracle */
typedef enum { QG_PERMUTATION = 0, QG_LINEAR_FUNCTION = 1, QG_CLIFFORD = 2, QG_PAULI = 3 } qg_env_kind;

typedef struct {
    int32_t kind; /* qg_gate_kind */
    int32_t q0;
    int32_t q1; /* ignored for one-qubit gates */
} qg_gate;

/* Constructor arguments of Py{Clifford,LinearFunction,Permutation,Pauli}Env::new
 * (clifford.rs:401-426, linear_function.rs:384-410, permutation.rs:277-303, pauli.rs:743-778). */
typedef struct {
    int32_t env_kind; /* qg_env_kind */
    int32_t num_qubits;
    int32_t difficulty;
    int32_t depth_slope;
    int32_t max_depth;
    /* MetricsWeights (metrics.rs:150-166) */
    float w_n_cnots, w_n_layers_cnots, w_n_layers, w_n_gates;
    int32_t add_inverts;
    int32_t add_perms;
    int32_t track_solution;
    /* PauliEnv only */
    int32_t max_rotations;
    int32_t pauli_diff_scale;
    int32_t final_pauli_layers; /* < 0: None -> max_rotations + 2 (pauli.rs:760) */
    float num_qubits_decay;
    float pauli_layer_reward;
} qg_config;

/* Fill the reference's defaults for `env_kind` (clifford.rs:420-422, metrics.rs:157-166,
 * envs/synthesis.py:182-204,380-412). */
void qg_config_default(qg_config *cfg, int32_t env_kind, int32_t num_qubits);

const char *qg_last_error(void);
int qg_abi_version(void);
/* Number of visible gfx950 devices (0 when none / no driver). Never fails. */
int qg_device_count(void);

/* Parse one gate given as (name, indices) -- the FromPyObject of common.rs:46-100: name is
 * trimmed and matched case-insensitively; wrong arity / unknown name -> QG_ERR_INVALID with the
 * reference's message. */
int qg_gate_parse(const char *name, const int64_t *indices, size_t n_indices, qg_gate *out);

/* ------------------------------------------------------------------------------------------
 * Batched environments
 * ---------------------------------------------------------------------------------------- */
typedef struct qg_vec qg_vec;

/* Formats understood by qg_vec_set_state / qg_vec_get_state. */
typedef enum {
    QG_FMT_I64 = 0,   /* the trait's `set_state(Vec<i64>)` wire format per env (clifford.rs:299-304:
                         D*D entries, >0 => 1; permutation.rs:168-173: N entries; pauli.rs:517-552:
                         [rot_count, 4N^2 tableau, (len, chars...)*], fixed stride per env) */
    QG_FMT_U8 = 1,    /* dense 0/1 bytes in observation layout (the Gym int8 observation): D*D bytes per env.
                         Permutation: N bytes, one per entry, exactly as QG_FMT_PACKED (not the N*N one-hot
                         observation), for qg_vec_set_state and qg_vec_get_state alike.  PauliEnv: get_state
                         only, the 2N x 2N tableau */
    QG_FMT_PACKED = 2 /* bit-packed rows, reference row order: row r of env e is word e*D + r;
                         word = uint32 when D <= 32 else uint64; bit c = entry (r, c).
                         Permutation: one uint8 per entry. */
} qg_state_format;

/* Action tensor element type for qg_vec_step / qg_vec_rollout. */
typedef enum { QG_ACT_I32 = 0, QG_ACT_I64 = 1 } qg_action_dtype;

typedef struct {
    int32_t env_kind;
    int32_t num_qubits;
    int32_t num_actions;   /* Env::num_actions (clifford.rs:289) */
    int32_t obs_rows;      /* Env::obs_shape (clifford.rs:291-294, pauli.rs:505-507) */
    int32_t obs_cols;
    int32_t device;
    uint64_t batch;
    uint32_t packed_word_bytes;   /* 4 or 8 (1 for Permutation) */
    uint32_t packed_words_per_env; /* D (N for Permutation) */
    uint64_t packed_env_stride_bytes; /* stride of one env in the resident packed state */
    /* resident device buffers (owned by the handle; valid until destroy) */
    void *state_dev;    /* resident packed state, layout in DESIGN.md section 3 */
    float *reward_dev;  /* [B] Env::reward   (clifford.rs:355) */
    uint8_t *done_dev;  /* [B] Env::is_final (clifford.rs:353) */
    uint8_t *success_dev; /* [B] Env::success (clifford.rs:357-359) */
    int32_t *depth_dev; /* [B] remaining depth */
    uint32_t *error_dev; /* [B] sticky per-env fault bits (QG_FAULT_*) */
} qg_vec_info;

#define QG_FAULT_SINGULAR 1u     /* inverse of a singular matrix requested (clifford.rs:155 panic) */
#define QG_FAULT_ZERO_WEIGHT 2u  /* weight-0 rotation in the front layer (pauli_network.rs:114 unwrap) */
#define QG_FAULT_BAD_STATE 4u    /* set_state produced an unusable state: an out-of-range PermutationEnv entry (the reference indexes out
                                    of bounds, permutation.rs:241-243), or -- with add_inverts only -- a repeated entry, which has no inverse;
                                    without add_inverts a vector with repeated entries runs as in the reference (permutation.rs:168-173) */
#define QG_FAULT_SOLUTION_OVERFLOW 8u /* track_solution: more entries than an episode can produce were logged (the
                                    log holds the max_depth steps an episode can last -- PauliEnv: plus one entry per
                                    rotation; the reference's Vec grows without bound when a caller keeps stepping a
                                    finished env) */

/* Build B environments, all in the constructor state (identity, depth 1, success, reward 1.0;
 * clifford.rs:214-245), on GPU `device`. */
int qg_vec_create(const qg_config *cfg, const qg_gate *gates, size_t n_gates, uint64_t batch, int device, qg_vec **out);
void qg_vec_destroy(qg_vec *v);
int qg_vec_get_info(const qg_vec *v, qg_vec_info *out);

/* Make the handle keep its per-env result arrays in caller-owned device memory (e.g. tensors of
 * the learner's framework) instead of its own: reward f32[B], done u8[B], success u8[B],
 * depth i32[B].  Current contents are carried over.  The caller keeps the memory alive until the
 * handle is destroyed or re-bound; NULL leaves that array where it is.  Synchronises. */
int qg_vec_bind_outputs(qg_vec *v, float *reward_dev, uint8_t *done_dev, uint8_t *success_dev, int32_t *depth_dev);

/* Env::set_difficulty / get_difficulty (clifford.rs:296-297) -- one value for the whole batch, read when a reset is enqueued.
 * A launch captured by the caller into a graph keeps the difficulty it was captured with. */
int qg_vec_set_difficulty(qg_vec *v, int64_t difficulty);
int64_t qg_vec_get_difficulty(const qg_vec *v);

/* Env::set_state for every env (clifford.rs:299-304): states + e*stride_elems is env e's record in
 * `format`; depth := max_depth, metrics zeroed, reward := success ? 1 : 0, inverted := false.
 * `on_device` != 0: `states` is a device pointer.  Host input is staged and copied on `stream`. */
int qg_vec_set_state(qg_vec *v, const void *states, int format, size_t stride_elems, int on_device, void *stream);
/* Inverse of the above for inspection / checkpointing (QG_FMT_I64 of a PauliEnv returns the
 * tableau only). */
int qg_vec_get_state(qg_vec *v, void *out, int format, size_t stride_elems, int on_device, void *stream);
/* Env::clone, batched (clifford.rs:179, linear_function.rs:154, permutation.rs:29 derive(Clone); pauli.rs:307-337): env dst_idx[i] of `dst`
 * becomes a copy of env src_idx[i] of `src`, i < n.  Copied: everything a clone carries -- the state, depth, reward, is_final, success,
 * inverted, the fault word, the incremental solved masks, both halves of the solution log and their lengths, the layer-metric records, and
 * PauliEnv's rotations, DAG order, phases and current_perm_idx -- so a copy and its source step identically under the same actions and
 * coins.  A tracked dense observation of `dst` (qg_vec_track_dense) gets the copied envs' rows rewritten.
 * A copy carries state, not RNG position: later draws of dst env j (add_inverts coins, PauliEnv observe permutations, resets) come from
 * j's own counter streams of the `dst` handle, as every batched draw does.
 * `src` and `dst` (may be the same handle): same constructor arguments and device (the rule of qg_env_clone's pool), else QG_ERR_INVALID.
 * src_idx_dev / dst_idx_dev: device arrays of n uint32; dst_idx_dev NULL = 0 .. n-1.  Sources may repeat; destinations may not; when
 * dst == src no index may be both a destination and a source.  Entries with an index out of range are skipped (the host cannot see device
 * indices without a synchronisation).  Afterwards the list of finished envs is what qg_vec_set_state leaves: the next qg_vec_reset_done
 * resets exactly the envs whose flag is set.  Stream-ordered, one launch, capturable into a hipGraph. */
int qg_vec_copy_envs(qg_vec *dst, const qg_vec *src, const uint32_t *src_idx_dev, const uint32_t *dst_idx_dev, uint64_t n, void *stream);

/* Env::reset for every env (clifford.rs:306-319).  The reference draws `difficulty` uniform
 * actions from an unseedable RNG; here draw t of env e is
 *   action = mulhi64(splitmix64(seed ^ splitmix64(e * 0x9E3779B97F4A7C15 + t)), num_actions)
 * so the oracle can replay it.  (PauliEnv: see qg_vec_pauli_reset_from.) */
int qg_vec_reset(qg_vec *v, uint64_t seed, void *stream);
/* Env::reset for the envs whose episode is over (done flag set) only; the others are untouched.
 * Lets a GPU-resident collector run episode after episode without a host round trip; pass a
 * fresh seed per call (e.g. a step counter) so successive episodes of an env differ. */
int qg_vec_reset_done(qg_vec *v, uint64_t seed, void *stream);
/* qg_vec_reset_done(v, reset_seed) followed by qg_vec_step(v, actions_dev, ...) -- the auto-reset collection loop's pair of calls -- with the
 * results of exactly those two calls (rewards_dev / dones_dev: optional per-step outputs as in qg_vec_rollout).  ONE launch from the second
 * call of a session on for: CliffordEnv N <= 16 with any options (add_inverts included, while every env is symplectic and no dense observation
 * is tracked with it), CliffordEnv 16 < N <= 32 and LinearFunctionEnv 8 < N <= 64 without add_inverts, and always for LinearFunctionEnv N <= 8 /
 * PermutationEnv N <= 16: the reset's workgroups (the finished envs' scrambles) and the step's workgroups (every other env) share the grid, and an
 * env that was reset takes its first step on the wave / lane that finished its scramble.  Everything else -- and the first call of a session,
 * whose list has to be compacted from the flags -- is the two calls; so is a configuration whose episodes are so short that a large share of
 * the batch finishes in every step (there the two launches are as fast or faster).  qg_plan_query(QG_PLAN_RESET_DONE_STEP) says which. */
int qg_vec_reset_done_step(qg_vec *v, uint64_t reset_seed, const void *actions_dev, int action_dtype, const uint8_t *coins_dev, float *rewards_dev,
                           uint8_t *dones_dev, void *stream);
/* Capturing these calls into a caller's hipGraph: once qg_vec_reset_done is in use on a handle, a single qg_vec_step (and the sampling +
 * step calls) leaves the list of the envs it finished for the reset that follows, so that reset needs no compaction launch.  The list
 * lives on the device and every launch that appends to it expects it empty; what the host believes about it only holds within one
 * "session" -- one stream capture, or eager execution on a handle none of whose list launches was ever captured.  The library
 * therefore (a) zeroes the list (a captured memset) before the first appending launch of every capture and compacts the `done` flags
 * itself at the first qg_vec_reset_done of every capture, (b) after any capture, trusts no list in eager calls (they compact every
 * time), and (c) bounds every append by the batch size on the device.  Any order of replays, eager steps and eager resets gives the
 * results of the same calls made eagerly; the cheapest graph is the one that captures step and reset_done together. */
/* Device clock for launches that are replayed from a captured hipGraph (kernel arguments, hence
 * seeds and RNG counters, are baked into a graph).  While set, every kernel of this handle adds
 * *clock_dev to its RNG counter: reset / reset_done draw with seed + 0x9E3779B9 * clock, the
 * add_inverts coin and the PauliEnv permutation draw use counter + clock.  The owner of the graph
 * advances the clock (a device-side add inside the graph) between replays.  NULL detaches.  The
 * word must stay valid while attached.  Synchronises and drops cached rollout graphs. */
int qg_vec_set_clock(qg_vec *v, const uint64_t *clock_dev);
/* Stream ordering without a system-scope fence: everything enqueued on `waiter_stream` after this call
 * runs after everything enqueued on `producer_stream` before it (hipEventRecord + hipStreamWaitEvent with
 * hipEventDisableTiming | hipEventDisableSystemFence).  For side-stream work next to the step stream
 * (the multi-GPU observation all-gather). */
int qg_stream_wait_stream(void *waiter_stream, void *producer_stream);
/* The handle's host-side RNG counters: the next step's add_inverts coin is drawn with counter
 * `step_index` (it advances by one per step) and the next PauliEnv observe() permutation with
 * `observe_index`.  A caller that replays graphs sets them to the position inside the graph so
 * that eager and replayed launches draw alike (effective counter = this + the device clock). */
int qg_vec_set_counters(qg_vec *v, uint64_t step_index, uint64_t observe_index);
/* Seed of the handle's own counter-RNG streams: the add_inverts coin (clifford.rs:266 `gen_bool(0.5)`) and PauliEnv's
 * observe() permutation draw (pauli.rs:657-662), when they are not supplied by the caller.  Handles start with one fixed
 * seed (reproducible runs); a host that wants the reference's thread_rng behaviour -- independent streams per env object
 * and per clone -- gives every handle its own seed. */
int qg_vec_set_seed(qg_vec *v, uint64_t seed);
/* Global index of this handle's env 0 in every counter-RNG draw (reset scramble, coins, PauliEnv targets and permutations):
 * env e draws as env `first_env + e`.  A handle that holds the shard [first_env, first_env + batch) of a larger batch --
 * one rank of a multi-GPU job, SURVEY 8e: GPU g owns envs [g*B/G, (g+1)*B/G) -- then draws exactly what the unsharded
 * batch would, so a sharded run is bit-identical to the single-GPU run of the whole batch.  Default 0. */
int qg_vec_set_env_base(qg_vec *v, uint64_t first_env);
uint64_t qg_vec_get_env_base(const qg_vec *v);
/* Same as qg_vec_reset, with the draws supplied: actions_dev[t*B + e], t < n_draws (int32). */
int qg_vec_reset_with(qg_vec *v, const int32_t *actions_dev, size_t n_draws, void *stream);

/* Env::step for every env (clifford.rs:321-347): one kernel launch.
 *   actions_dev[B]  element type `action_dtype`; out-of-range (incl. negative) = "no gate" but
 *                   depth still decrements (clifford.rs:324,342)
 *   coins_dev[B]    the gen_bool(0.5) draws of maybe_random_invert (clifford.rs:266); NULL = use
 *                   the handle's counter RNG when add_inverts is set; ignored otherwise
 * Results land in the resident reward/done/success/depth buffers (qg_vec_info). */
int qg_vec_step(qg_vec *v, const void *actions_dev, int action_dtype, const uint8_t *coins_dev, void *stream);

/* The same step with HOST buffers (batched flavour, host-pointer variant): actions_host[B] (and coins_host[B] or NULL) are
 * copied to the device, the step runs, and reward / is_final / success are copied back into rewards_host f32[B], dones_host u8[B],
 * success_host u8[B] (each may be NULL) -- all enqueued on `stream` with hipMemcpyAsync, nothing synchronises: with pinned buffers
 * (hipHostMalloc / hipHostRegister) the call returns at once and the outputs are valid after qg_vec_sync(v, stream); pageable buffers
 * work too (the runtime then stages the copies).  The input buffers must stay untouched until the stream has passed the call.
 * When every buffer passed is pinned AND device-mapped (the default of hipHostMalloc; hipHostRegister with hipHostRegisterMapped) and the
 * output buffers are 16-byte aligned, no copy is made at all: the step kernel reads actions / coins in host memory and one kernel writes
 * the outputs there (same contract, a quarter of the time: tools/bench_step_host.py). */
int qg_vec_step_host(qg_vec *v, const void *actions_host, int action_dtype, const uint8_t *coins_host, float *rewards_host, uint8_t *dones_host,
                     uint8_t *success_host, void *stream);

/* T consecutive steps.  actions_dev[t*B + e]; optional per-step outputs rewards_dev[t*B + e],
 * dones_dev[t*B + e] (NULL = only the final values in the resident buffers).
 *   fused == 0: T single-step launches replayed from a cached hipGraph (same results and same
 *               memory traffic as T qg_vec_step calls, without T host launches)
 *   fused != 0: one launch that keeps each env's state in registers across the T steps */
int qg_vec_rollout(qg_vec *v, const void *actions_dev, int action_dtype, size_t n_steps, const uint8_t *coins_dev,
                   float *rewards_dev, uint8_t *dones_dev, int fused, void *stream);

/* Graph rollout whose step t reads the action slice t % period of actions_dev[period][B]: n_steps
 * single-step launches over a small ring of action buffers -- the access pattern of a policy that
 * rewrites one resident action buffer every step (cache-hot), where qg_vec_rollout streams a
 * [n_steps][B] tensor from HBM. */
int qg_vec_rollout_ring(qg_vec *v, const void *actions_dev, int action_dtype, size_t n_steps, size_t period, void *stream);

/* Env::observe for every env, densified the way the Gym adapter does it (adapters.py:50-54):
 * out_dev[e * obs_rows*obs_cols + r*obs_cols + c] in {0,1}, int8. */
int qg_vec_observe_dense(qg_vec *v, int8_t *out_dev, void *stream);
/* Keep the dense observation RESIDENT: from this call on, dense_dev[B * obs_rows * obs_cols] (caller-owned device memory, 16-byte aligned,
 * alive until the handle is destroyed or the tracking is detached with dense_dev == NULL) always holds what qg_vec_observe_dense would
 * write, in stream order after every call that changes states.  What the Gym adapter does after every step (adapters.py:62-72 calls
 * `_full_obs`, :50-54) costs a full D * D-byte rewrite per env; a gate changes the rows of at most two qubits, so the one-step kernel
 * rewrites just those rows (<= 4 rows of D bytes: 128 of CliffordEnv 16q's 1 024 bytes) in the launch that applies the gate.  Resets of
 * finished envs (qg_vec_reset_done) rewrite those envs; launches that cannot track it (add_inverts, fused rollouts, the policy kernels)
 * are followed by one full rewrite on the same stream.  Handles whose matrix has 16 or 32 rows held as 32-bit words (CliffordEnv
 * N = 8, 16; LinearFunctionEnv N = 16, 32): QG_ERR_UNSUPPORTED otherwise.  Drop cached expectations: rollout graphs are keyed by it. */
int qg_vec_track_dense(qg_vec *v, int8_t *dense_dev, void *stream);
/* Bit-packed observation in QG_FMT_PACKED layout (what the multi-GPU all-gather moves): qg_vec_info.packed_words_per_env
 * words of packed_word_bytes per env, one word per observation row, bit c = column c.  PauliEnv (thread-per-env family,
 * at most 64 observation columns): one 64-bit word per row of the [2N, 2N + max_rotations] observation; the call counts
 * as one Env::observe, i.e. it draws the add_perms permutation like qg_vec_observe_dense does. */
int qg_vec_observe_packed(qg_vec *v, void *out_dev, void *stream);
/* Host-pointer variants of the two calls above: the observation is written to a buffer of the handle and copied to out_host on `stream`
 * (hipMemcpyAsync; valid after qg_vec_sync(v, stream), pinned memory for a truly asynchronous copy).  Sizes: B * obs_rows * obs_cols bytes,
 * resp. B * packed_words_per_env * packed_word_bytes. */
int qg_vec_observe_dense_host(qg_vec *v, int8_t *out_host, void *stream);
int qg_vec_observe_packed_host(qg_vec *v, void *out_host, void *stream);
/* Env::masks (clifford.rs:349-351): out_dev[e*num_actions + a] = !success[e] */
int qg_vec_masks(qg_vec *v, uint8_t *out_dev, void *stream);

/* PauliEnv: rebuild every env from an explicit target, the deterministic tail of
 * PauliEnv::reset (pauli.rs:573-585).  tableaus: [B, 2N*2N] uint8 (host), labels: per env
 * `n_rot[e]` Pauli labels of N characters each, concatenated without separators. */
int qg_vec_pauli_reset_from(qg_vec *v, const uint8_t *tableaus, const char *labels, const int32_t *n_rot, void *stream);

/* PauliEnv with add_perms: observe() draws one of the coupling map's qubit automorphisms per env,
 * permutes the observation with it and remembers it so that the next step() un-permutes the
 * action (pauli.rs:594-599, 653-665).  qg_vec_observe_dense draws from the handle's counter RNG;
 * this variant takes the draws explicitly: perm_idx_dev[B] (int32, reduced mod the number of
 * perms), or NULL for the RNG. */
int qg_vec_pauli_observe_dense(qg_vec *v, int8_t *out_dev, const int32_t *perm_idx_dev, void *stream);
/* number of (qubit, action) permutation pairs of a PauliEnv batch (0 when add_perms is off) */
int qg_vec_pauli_num_perms(const qg_vec *v);

/* Diagnostics: the kernel device clock -- how long a launch's waves were on the machine, measured by the waves themselves (no profiler, no host
 * clock).  slots_dev: n_slots x waves_per_slot records {uint64 entry, uint64 exit} in device memory (16-byte aligned), zeroed by the caller;
 * ticks of the device's constant-rate counter (qg_kernel_clock_rate_khz: 100 MHz on gfx950).  After the call the k-th step / observation kernel
 * launched through this handle (eager, or captured into a graph: a replay stamps the slots its launches were captured with) has its wave w write
 * record w of slot k (waves past waves_per_slot write nothing: size it to the largest grid, batch / 32 covers every stamped kernel); the launch's
 * duration is max(exit) - min(entry) over the records with exit != 0.  Launches past n_slots and kernels without stamps (export and
 * fused-rollout kernels, the 64-bit-row and lane-group resets) leave their slot untouched.  Stamped: the one-step kernels (qm_step1 / q64_step1 /
 * qm_inv2 / q64_inv2 / word_step / lfd_step / ptile_step1c), the resets qm_init / word_init / ptile_generate / ptile_reset_tree (one slot each),
 * qm_reset_step / word_reset_step and the dense observation rewrite (qm_dense_stream).  A wave with a slot waits for its own loads and
 * stores before its exit stamp, so exit - entry covers the memory traffic of the launch; a launch WITHOUT a slot pays one scalar instruction.
 * n_slots = 0 detaches.  Drops cached rollout graphs. */
int qg_vec_set_kernel_clock(qg_vec *v, uint64_t *slots_dev, size_t n_slots, uint32_t waves_per_slot);
/* ticks per millisecond of that counter on `device` (hipDeviceAttributeWallClockRate), or a negative status */
int qg_kernel_clock_rate_khz(int device);

/* Blocks until everything enqueued on `stream` by this handle has finished; returns
 * QG_ERR_PANIC if any env has a fault bit set. */
int qg_vec_sync(qg_vec *v, void *stream);

/* Solution log (Env::solution, clifford.rs:376-381 / pauli.rs:685-719) of env e, host side.
 * Returns the length (may exceed cap) or a negative status.  Entries are kept as 32-bit words on
 * the device.  CliffordEnv, LinearFunctionEnv and PermutationEnv spend bit 31 of the word on the
 * `solution_inv` flag, so an entry is exact up to 2^31 - 2: an out-of-range action that CliffordEnv
 * and LinearFunctionEnv log verbatim like the reference (clifford.rs:334-340) is reported exactly
 * up to that value; larger and negative ones are reported as UINT64_MAX (what `-1 as usize` is).
 * PermutationEnv and PauliEnv log in-range actions only (permutation.rs:210-216, pauli.rs:612-626).
 * The log holds the first max_depth pushes of an episode (PauliEnv: max_depth + one per rotation):
 * a later push is dropped, sets QG_FAULT_SOLUTION_OVERFLOW in the env's word and leaves the logged
 * entries as they are -- the list is then a prefix, in push order, of the reference's (PauliEnv: of
 * whole steps, a gate with the rotations it released; nothing is logged behind a dropped step). */
int64_t qg_vec_solution(qg_vec *v, uint64_t env, uint64_t *out, size_t cap);
/* The same for EVERY env with one copy of the log: out[e * cap + i] = entry i of env e's list (entries beyond cap dropped), lens[e] = its
 * full length (what twisterl's collector does per episode with Env::solution, here once per batch).  Host pointers; synchronises. */
int qg_vec_solutions(qg_vec *v, uint64_t *out, size_t cap, int64_t *lens);

/* ------------------------------------------------------------------------------------------
 * Collector support: the device-side steps between observe() and step() when a policy network
 * is in the loop.  The reference runs these on the CPU inside twisterl's collector
 * (rl/synthesis.py:128-138; collecting parameters gamma / lambda, rl/configs.py:134-144,219-220).
 * The free functions work on the calling thread's current HIP device.
 * ---------------------------------------------------------------------------------------- */
typedef enum { QG_DT_I8 = 0, QG_DT_F32 = 1, QG_DT_BF16 = 2, QG_DT_F16 = 3 } qg_dtype;

/* Env::observe densified (adapters.py:50-54) straight into the dtype the policy network reads:
 * out_dev[e * obs_rows*obs_cols + r*obs_cols + c] in {0, 1} as `out_dtype`. */
int qg_vec_observe_dense_as(qg_vec *v, void *out_dev, int out_dtype, void *stream);
/* Dense {0,1} tensor from QG_FMT_PACKED rows (e.g. the gathered observation of other ranks, or
 * the packed observations a rollout buffer keeps): n_rows words of `word_bytes` (4 / 8: bit c =
 * column c; 1: PermutationEnv, the byte is the set column) -> out_dev[row * cols + c]. */
int qg_expand_packed(const void *packed_dev, int word_bytes, uint64_t n_rows, uint32_t cols, void *out_dev, int out_dtype, void *stream);
/* The int8 {0,1} observation of qg_vec_observe_dense (n_elems entries) in another dtype -- for
 * a PauliEnv observation taken once (observe() may draw a permutation) that has no row-word form, so it
 * is taken once and widened. */
int qg_widen_dense(const int8_t *obs_dev, uint64_t n_elems, void *out_dev, int out_dtype, void *stream);
/* One categorical draw per env from softmax(logits[e, 0:num_actions]) by an exponential race on
 * the counter RNG: base = rng(seed ^ 0x73616D70, e, counter + *clock_dev) (clock_dev may be NULL);
 * u[a] = ((hash32(base, a) >> 9) + 0.5) *
 * 2^-23; action = argmin -log(u[a]) / exp(logit[a] - max) (kernels_collect.hip states hash32).
 * logits_dev: [batch, ld] of `logits_dtype` (f32 / bf16 / f16), ld >= num_actions.  mask_dev:
 * [batch, num_actions] (1 = allowed; Env::masks) or NULL.  Outputs (each may be NULL except
 * actions): action, log-prob of it, entropy of the row, and values_dev[e] = logits[e, value_col]
 * (value_col >= 0: a value head computed by the same GEMM as the logits).
 * Logits: every finite value of the dtype (f16 up to +-65504, bf16 / f32 up to their largest: a logit - max that overflows counts as
 * probability 0), any num_actions >= 1.  A -inf logit is a masked action, exactly as a 0 in mask_dev: probability 0, never drawn, p log p
 * = 0 in the entropy.  A row without a live action (mask all 0, or every logit -inf) gives action 0, log-prob 0, entropy 0.  exp(logit - max)
 * is the hardware's: it is 0 from about 87 below the maximum on, and such an action is not drawn either (its probability is below 2e-38).
 * Ties of the race keys go to the lower action index.  Outside the contract: a row that holds NaN or +inf.  The call still terminates
 * and writes an action in [0, num_actions) -- an action whose key is NaN is never the winner, a row in which no key is an ordered
 * finite number gives action 0 -- but log-prob and entropy of such a row are unspecified (NaN, or the 0 of the empty row). */
int qg_sample_actions(const void *logits_dev, int logits_dtype, uint64_t ld, uint64_t batch, uint32_t num_actions, const uint8_t *mask_dev,
                      uint64_t seed, uint64_t counter, const uint64_t *clock_dev, void *actions_dev, int action_dtype, float *logp_dev,
                      float *entropy_dev, int32_t value_col, float *values_dev, void *stream);
/* The selection step of a beam search: from the `width` beams x num_actions actions of every group keep the `width` best continuations as
 * (parent env, action) pairs -- src_idx_dev of qg_vec_copy_envs and actions_dev of qg_vec_step.  Group g owns the `width` consecutive slots
 * g*width .. g*width + width-1 of a batch of n_groups*width envs.  logp_dev: [batch, ld] of `logp_dtype` (f32 / bf16 / f16), ld >= num_actions,
 * the per-action score of each slot (normally log_softmax of the policy's logits); cum_dev f32[batch]: each slot's score so far; live_dev
 * u8[batch]: != 0 where the slot holds a beam.  The rules (tests/beammodel.py restates them in numpy; results agree bit for bit):
 *   - A candidate is (live slot b, action a < num_actions) with score cum[b] + (float)logp[b, a]: one f32 addition, round to nearest, not
 *     contracted with anything.  A candidate whose score is NaN or -inf does not exist (a caller masks an action by scoring it -inf).
 *   - The candidates of a group are ordered by score descending (-0 = +0), ties by slot ascending, then by action ascending.  No randomness;
 *     the result does not depend on the launch geometry.
 *   - Output slot j of the group (env g*width + j) receives candidate j: parent_dev = the BATCH-WIDE env index of its slot, actions_dev = its
 *     action, cum_out_dev = its score (the sum's own bits), live_out_dev = 1.  Slots past the number of candidates get parent = their own
 *     index, action = num_actions (out of range: "no gate", clifford.rs:324), cum_out = -inf, live_out = 0.
 *   - Inputs and outputs may not alias.
 * Limits: width <= 64 and width * num_actions <= 14 336 (64 beams x 224 actions: a group's candidates live in 56 KiB of one workgroup's LDS),
 * n_groups * width < 2^32; QG_ERR_UNSUPPORTED beyond, QG_ERR_INVALID for null pointers, zero sizes, ld < num_actions or an unknown dtype.
 * Stream-ordered on `stream`, one launch (one workgroup per group), no synchronisation, capturable into a hipGraph. */
int qg_beam_select(const void *logp_dev, int logp_dtype, uint64_t ld, uint32_t num_actions, uint64_t n_groups, uint32_t width,
                   const float *cum_dev, const uint8_t *live_dev, uint32_t *parent_dev, void *actions_dev, int action_dtype,
                   float *cum_out_dev, uint8_t *live_out_dev, void *stream);
/* Which beams of a group hold a state the group has already got: the merge step of a beam search.  Groups as in qg_beam_select: group g owns
 * slots g*width .. g*width + width-1 of a batch of n_groups*width envs.  words_dev: the batch's QG_FMT_PACKED observation as
 * qg_vec_observe_packed writes it, [batch, words_per_env] words of word_bytes (1, 4 or 8) each -- any words will do, the kernel knows no env.
 *
 * The state key.  With w_0 .. w_{n-1} the n = words_per_env words of one env, each zero-extended to 64 bits, and splitmix64 the function of
 * the reset draws above (x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31),
 *   key = splitmix64( n ^ ( sum_i splitmix64( w_i ^ splitmix64(i + 1) )  mod 2^64 ) ),     and a key of 0 is replaced by 0x9E3779B97F4A7C15
 * (the sum wraps, so no order of summation shows; 0 is left to mean "empty" in the history).  Two envs hold "the same state" exactly when
 * their keys are equal.  Two different states share a key with probability about 2^-64 per pair; such a collision can only drop a beam, never
 * produce a wrong solution: the env, not this kernel, decides what solves a target.
 *
 * The rules (tests/beammerge_model.py restates them in numpy; results agree bit for bit), with cum_dev f32[batch] the slots' scores so far
 * and live_dev u8[batch] != 0 where a slot holds a beam:
 *   1. A live slot whose cum has no order word -- NaN or -inf, as for a candidate of qg_beam_select -- is dropped and counted nowhere.
 *   2. Revisit: a live slot whose key is in its group's history is dropped, and counted in dropped[g][0].
 *   3. Duplicate: among the remaining live slots of a group that share a key exactly one survives, the one with the largest cum in
 *      qg_beam_select's order (-0 = +0), ties to the lowest slot.  The others are dropped, and counted in dropped[g][1].
 *   4. live_out_dev u8[batch] = 1 for the survivors and 0 for every other slot (a slot that was not live stays 0).  It may not alias live_dev.
 *   5. The survivors' keys enter the group's history in ascending slot order.  A history holds at most seen_cap distinct keys; once it is
 *      full further keys are not recorded (the search goes on and only prunes less).  Nothing is ever removed.
 *   6. No randomness; the result does not depend on the launch geometry.
 * keys_out_dev (optional) u64[batch]: the key of every slot, live or not.  dropped_dev (optional) u32[n_groups][2]: ADDED to by every call.
 * seen_dev (optional): the groups' histories, qg_beam_seen_bytes(n_groups, seen_cap) bytes, 8-byte aligned, opaque; all-zero bytes are the empty
 * history (the caller clears it with a memset on its stream), and one buffer goes with one (n_groups, seen_cap).  NULL: merge within the call
 * only (rule 2 never applies, rule 5 does nothing).  Every call scans the group's history, so a call costs time in proportion to the keys held.
 * Limits: width <= 64 and words_per_env * word_bytes <= 2048 (a group's words are then at most 128 KiB), n_groups < 2^31, seen_cap < 2^32;
 * QG_ERR_UNSUPPORTED beyond, QG_ERR_INVALID for a null required pointer, a zero size (seen_cap too, when seen_dev is given), a word_bytes other
 * than 1 / 4 / 8, a misaligned buffer or aliased live arrays.  Stream-ordered on `stream`, one launch (one workgroup per group), no
 * synchronisation, capturable into a hipGraph. */
size_t qg_beam_seen_bytes(uint64_t n_groups, uint64_t seen_cap);
int qg_beam_merge(const void *words_dev, int word_bytes, uint32_t words_per_env, uint64_t n_groups, uint32_t width, const float *cum_dev,
                  const uint8_t *live_dev, void *seen_dev, uint64_t seen_cap, uint8_t *live_out_dev, uint64_t *keys_out_dev,
                  uint32_t *dropped_dev, void *stream);
/* What a beam search does with the results of a step, between qg_vec_step and qg_beam_merge: the beams' returns, every group's winner, which
 * beams go on -- and, on request, the bound: a beam that can no longer beat its group's winner is hopeless.  Groups as in qg_beam_select:
 * group g owns slots g*width .. g*width + width-1 of a batch of n_groups*width envs.
 * Operands, all on the device.  In: parent_dev i32[batch] (qg_beam_select's), ret_in_dev f32[batch] the returns before the step, reward_dev
 * f32[batch], success_dev / done_dev u8[batch] the step's results.  In and out: live_dev u8[batch] != 0 where a slot holds a beam, best_dev
 * f32[n_groups] the return of each group's winner (-inf without one), found_dev u8[n_groups] != 0 where a group has a winner.  Out: ret_out_dev
 * f32[batch], win_src_dev i32[n_groups] (src_idx_dev of the qg_vec_copy_envs that saves the winners), group_live_dev u8[n_groups].
 * bounded_dev (optional) i32[n_groups]: ADDED to by every call.  `skip`: what win_src says where a group's winner stays (a caller passes an
 * index qg_vec_copy_envs skips, e.g. batch).  `bonus`: the most a beam's return can still grow by.  `mode`: a qg_bound_mode.
 * The rules, per group g, in this order (tests/beambound_model.py restates them in numpy; results agree bit for bit):
 *   1. For a slot b with live[b] != 0: r[b] = ret_in[parent[b]] + reward[b], one f32 addition, round to nearest, not contracted with
 *      anything, and ret_out[b] = r[b] (the sum's own bits).  A slot that is not live gets ret_out[b] = 0, and its parent, reward, success
 *      and done are not read.  parent[b] is a batch-wide env index; one outside [0, batch) is outside the contract (it is not followed: r[b]
 *      is then NaN).
 *   2. solved[b] = live[b] && success[b].  The pick j is the solved slot of the largest r in qg_beam_select's order (-0 = +0; an r of NaN
 *      or -inf is no pick), the lowest slot among equals.  If there is a pick and r[j] > best[g] -- strictly, as floats -- then best[g] =
 *      r[j] (its own bits), found[g] = 1 and win_src[g] = g*width + j.  Otherwise win_src[g] = skip, and best[g] and found[g] stay.
 *   3. live[b] = live[b] && !done[b].
 *   4. With mode != QG_BOUND_NONE and found[g] != 0 after rule 2: hopeful[b] = live[b] && (r[b] + bonus > best[g]) -- the sum one f32
 *      addition of its own, against the best[g] rule 2 left; r[b] + bonus == best[g] is hopeless, and so is a NaN.  QG_BOUND_STOP: if no slot
 *      of the group is hopeful, every live[b] of the group becomes 0; else nothing changes.  QG_BOUND_PRUNE: live[b] = hopeful[b].
 *      bounded[g] grows by the number of beams ended this way.  A group with found[g] == 0 is never touched, nor is any with QG_BOUND_NONE.
 *   5. live_dev is written back as 0 / 1, and group_live[g] = the number of slots of the group still live.
 *   6. No randomness; the result does not depend on the launch geometry.
 * Why QG_BOUND_STOP changes no result of a search whose step rewards are at most `bonus` in total from any state on (CliffordEnv,
 * LinearFunctionEnv, PermutationEnv with metrics weights >= 0: 1.0 for reaching the target, minus penalties): f32 addition is monotone, so no
 * descendant of b ever holds a return above fl(r[b] + bonus); rule 2 replaces a winner only on a strictly greater return; best only rises.
 * ret_out_dev may not alias ret_in_dev (a slot's parent is another slot).  Limits: width <= 64 (one lane of a wave per slot), n_groups * width
 * < 2^31; QG_ERR_UNSUPPORTED beyond, QG_ERR_INVALID for a null required pointer, width 0, an unknown mode, a misaligned 32-bit array or
 * ret_out_dev == ret_in_dev.  Stream-ordered on `stream`, one launch (one wave per group, several groups per workgroup), plain loads and
 * stores only, no synchronisation, capturable into a hipGraph. */
typedef enum { QG_BOUND_NONE = 0, QG_BOUND_STOP = 1, QG_BOUND_PRUNE = 2 } qg_bound_mode;
int qg_beam_advance(uint64_t n_groups, uint32_t width, const int32_t *parent_dev, const float *ret_in_dev, const float *reward_dev,
                    const uint8_t *success_dev, const uint8_t *done_dev, uint8_t *live_dev, float *best_dev, uint8_t *found_dev,
                    float *ret_out_dev, int32_t *win_src_dev, uint8_t *group_live_dev, int32_t *bounded_dev, int32_t skip, float bonus, int mode,
                    void *stream);
/* The tree of a PUCT search (MCTS): one tree per target, rebuilt for every decision unless the caller rebases it (qg_mcts_rebase), in plain arrays the caller owns -- the kernels know no
 * env and no policy.  A forest of n_trees trees of at most cap nodes over num_actions actions is a struct of device arrays:
 *   per (tree m, node j), index m*cap + j:  parent i32 (-1 for node 0) | reward f32, the reward of the step into the node | value f32, the
 *       value head at the node, 0 for a terminal node | visits i32 | wsum f32 | terminal u8, the env's `done`
 *   per (tree, node, action), index (m*cap + j)*num_actions + a:  child i32 (-1 = not expanded) | prior f32
 *   per tree:  n_nodes i32
 * Node 0 is the root.  A node's env is expected in a pool of n_trees*cap envs at index m*cap + j ("pool index"); for a search of N
 * simulations per decision cap = N + 1, more where trees are carried from decision to decision.  qg_mcts_forest_bytes is what the arrays take together.
 * The rules (tests/mctsmodel.py restates them in numpy; results agree bit for bit):
 *   root       qg_mcts_backup in mode QG_MCTS_ROOT, per tree from logp_dev[m*ld + a] and values_dev[m]: prior[0][a] = expf(logp), child[0][a]
 *              = -1, terminal[0] = done_dev[m] != 0 (0 where done_dev is NULL), value[0] = values[m] (0 if terminal), visits[0] = 1,
 *              parent[0] = -1, reward[0] = wsum[0] = 0, n_nodes = 1.
 *   selection  qg_mcts_select, one descent per tree from node 0.  At a terminal node x the descent ends there and nothing is expanded.
 *              Otherwise every action a < num_actions with c = child[x][a] gets
 *                  Q = c >= 0 ? wsum[c] / f32(visits[c]) : value[x]          n_a = c >= 0 ? visits[c] : 0
 *                  U = ((c_puct * prior[x][a]) * sqrtf(f32(visits[x]))) / f32(1 + n_a)          score = Q + U
 *              each operation one IEEE f32 operation rounded to nearest, in this order (no contraction; the plain `/` and sqrtf of the
 *              build, which are the correctly rounded ones -- not __fsqrt_rn, which here is the native approximation).  The greatest score
 *              wins (-0 = +0), ties go to the lowest action; scores are finite by contract and a NaN score is no candidate.  If the
 *              winner has a child the descent goes on there; else it ends with (x, a) and the new node is j = n_nodes.
 *              Out, i32[n_trees] each: src = pool index of x; dst = pool index of the new node, or n_trees*cap (out of range: what
 *              qg_vec_copy_envs skips) where nothing is expanded; act = a, or num_actions ("no gate") where nothing is expanded; leaf =
 *              the node the backup starts from: the new node, or x at a terminal node or where no action is a candidate, or -1 where the
 *              tree makes no simulation that counts: finished_dev[m] != 0 (optional u8[n_trees]: the tree's real env is final), or a bound
 *              or a range check below was hit.
 *   backup     qg_mcts_backup in mode QG_MCTS_BACKUP, from qg_mcts_select's four outputs and the results of the expansion (logp_dev,
 *              values_dev, reward_dev f32[n_trees], done_dev u8[n_trees]: the new node's env after its step).  leaf < 0: nothing.  Where
 *              act < num_actions the node j = n_nodes is linked -- child[x][a] = j, parent[j] = x, reward[j], terminal[j] = done,
 *              value[j] = values (0 if terminal), prior[j][.] = expf(logp), child[j][.] = -1, visits[j] = 0, wsum[j] = 0, n_nodes += 1.
 *              Then G = value[leaf], and every node y != 0 from the leaf up gets G = reward[y] + G (one f32 addition), visits[y] += 1,
 *              wsum[y] += G; the root gets visits[0] += 1.
 * Safety: a descent makes at most cap levels and a walk at most cap steps, and both must move strictly (child > node > parent); every
 * index read from the forest (a child, a parent, n_nodes, src, dst, leaf) is range-checked before it is used, an expansion must name node
 * n_nodes < cap over an edge without a child.  A check that fails ends that tree's work for the call: qg_mcts_select gives leaf = -1 (act =
 * num_actions, dst out of range), qg_mcts_backup returns from that tree (after a broken parent link: without counting the root).
 * logp_dev: rows of ld >= num_actions floats, columns past num_actions are not read.  Limits: num_actions <= 256 (four actions per lane),
 * 2 <= cap <= 8192 (qg_mcts_select keeps a tree's visits and wsum in LDS, so a level of the descent is one dependent trip to memory),
 * n_trees*cap < 2^31 - 1; QG_ERR_UNSUPPORTED beyond, QG_ERR_INVALID for a null required pointer, a zero size, ld < num_actions, an unknown
 * mode or a misaligned 32-bit array.  Stream-ordered on `stream`, one launch each (one wave per tree, several trees per workgroup), plain
 * loads and stores only, no host reads, no synchronisation, capturable into a hipGraph.
 *   decision   qg_mcts_decide, after a decision's simulations: the root's visit counts and the move they give.  It writes nothing into the
 *              forest (tests/mctssample_model.py restates it in integers; results agree bit for bit).
 *     counts   For every action a < num_actions with c = child[0][a]: n_a = visits[c] where c is a child of this tree's root, that is
 *              0 < c < n_nodes; n_a = 0 where c < 0 (not expanded).  A child index c >= 0 outside that range, n_nodes outside [1, cap] or
 *              a negative visits value ends the tree's work for the call: move = num_actions and every count 0.  Nothing read from the
 *              forest is used as an index before it is range-checked.
 *     QG_MCTS_MOST_VISITED   the action of the greatest n_a among the expanded edges (c > 0), the lowest action among equals -- one 64-lane
 *              max of n_a << 32 | ~a; num_actions where the root has no child.
 *     QG_MCTS_SAMPLE   total = sum of the n_a (at most cap - 1 in a tree the kernels built; summed in 64 bits, so exact whatever the
 *              arrays hold).  total = 0 gives the answer of QG_MCTS_MOST_VISITED.  Otherwise r = mulhi64(rng_draw(seed ^ 0x6D637473, m,
 *              counter), total) with m the tree index -- the counter RNG and the integer draw of qg_vec_reset, 0 <= r < total -- and the
 *              move is the lowest action a with n_0 + ... + n_a > r, the sums in action order.  Integer arithmetic throughout: the
 *              result is exact and does not depend on the launch geometry; an action with n_a = 0 is never drawn, and action a is drawn
 *              for n_a of the total values of r.
 *     finished_dev   optional u8[n_trees]: a tree whose real env is final gets move = num_actions and is otherwise treated alike.
 *     counts_dev     optional i32[n_trees][counts_ld], counts_ld >= num_actions: the row of n_a (the training target of an AlphaZero-style
 *              learner), written for finished trees too; columns past num_actions are not written.
 *              move_dev i32[n_trees].  QG_ERR_INVALID for an unknown mode, a null move_dev, a misaligned array or counts_ld <
 *              num_actions with counts_dev given; the forest's limits and error codes are those above.  One launch, one wave per tree.
 *   rebase     qg_mcts_rebase, between two decisions: the subtree below the chosen move becomes the tree, in place, so the next decision
 *              starts from the simulations already spent there (an env's step must be deterministic for that to be valid search work).
 *              tests/mctsreuse_model.py restates it in numpy; results agree bit for bit.  move_dev i32[n_trees] (qg_mcts_decide's);
 *              finished_dev optional u8[n_trees]; env_src_dev i32[n_trees*cap], written in full: the src_idx of the qg_vec_copy_envs call
 *              that moves the node envs into a second pool (new pool index <- old pool index; none = n_trees*cap, which that call skips).
 *              Per tree m, with n = n_nodes[m], a = move_dev[m]:
 *     finished     finished_dev[m] != 0: the forest is untouched, env_src[m*cap + j] = none for every j < cap.
 *     nothing to carry   n outside [1, cap], a outside [0, num_actions) or c = child[0][a] outside (0, n): the forest is untouched,
 *              env_src[m*cap + j] = m*cap + j for j < n (for j < cap where n > cap, for no j where n < 1), none for every other j.
 *     kept     Otherwise node c is kept, and a node j, c < j < n, iff the chain j -> parent[j] -> ... reaches c exactly, every link
 *              strictly below the one before it and >= 0; a chain that breaks, or passes below c, keeps nothing.  No node <= c but c.
 *     renumbering   The new index j' of a kept node is the number of kept nodes below j: the order stays, c becomes 0.
 *     fields   reward, value, visits, wsum, terminal and the prior row move unchanged to j'; parent[j'] is the new index of the old
 *              parent; a child entry c2 becomes its new index where 0 <= c2 < n and c2 is kept, else -1.  The new root gets parent = -1,
 *              reward = 0, wsum = 0 and keeps everything else -- its visits are, by the backup rule, 1 + the simulations below it: a
 *              root's count.
 *     sizes    n_nodes[m] = the number of kept nodes; env_src[m*cap + j'] = m*cap + j for every kept node, none for j' >= n_nodes.
 *              Array entries at node indices >= the new n_nodes mean nothing.
 *              The rules are total: any forest content gives a defined result, every index read from the forest is range-checked before
 *              it is used and every loop is bounded by cap.  The parents and the table of new indices live in LDS (8 bytes per node, the
 *              launch sizing of qg_mcts_select); the renumbering is a ballot and a popcount per slice of 64 nodes; nodes move in
 *              ascending order, every load of a trip before its first store, which is what makes the compaction safe in place (j' <= j).
 *              A full tree has a defined meaning in qg_mcts_select: the simulation that wants to expand gets leaf = -1 and does not
 *              count.  Limits and error codes are those of qg_mcts_select; a null or misaligned move_dev or env_src_dev is
 *              QG_ERR_INVALID.  One launch, one wave per tree, plain vector loads and stores, no host reads, no synchronisation,
 *              capturable.
 *   several leaves per launch   qg_mcts_select_many and qg_mcts_backup_many: k descents per tree in one launch each, so a decision of N
 *              simulations takes ceil(N / k) rounds of launches on a leaf batch k times as large.  tests/mctsmany_model.py restates both in
 *              numpy; results agree bit for bit.  stride >= k is the row length of the per-descent arrays: entry m*stride + i of src, dst,
 *              act, leaf (i32[n_trees*stride]), of values, reward, done and row m*stride + i of logp belong to descent i of tree m.
 *     qg_mcts_select_many   Per tree, n0 = n_nodes at entry.  The call keeps an OVERLAY, a copy of the tree's (visits, wsum) that starts as
 *              the forest's, and makes descents i = 0 .. k-1 in that order.  Each is qg_mcts_select's descent -- the scores, the order of
 *              the f32 operations, the ties, the terminal rule and the range checks (children against n0) -- with three differences:
 *                overlay        visits and wsum are read from the overlay.
 *                pending edges  an edge (x, a) that an earlier descent of this call chose for expansion is no candidate, exactly like an
 *                               action whose score is a NaN: two descents of one call never expand the same edge and no descent enters a
 *                               node that does not exist yet.  With no candidate left at x the existing rule applies: leaf = x, act =
 *                               num_actions, nothing is expanded, the simulation counts.
 *                numbering      the e-th descent of the call that expands (e = 0, 1, ...) names node j = n0 + e; j >= cap refuses the
 *                               descent as a full tree does: leaf = -1, act = num_actions, dst = n_trees*cap, src the node it stood on,
 *                               and its edge is not pending.
 *              After descent i every node y it stood on, the root through the node it ended on -- also when it was refused for a full
 *              tree -- gets overlay visits[y] += 1, and every such y != 0 overlay wsum[y] = wsum[y] - virtual_loss, one f32 subtraction.
 *              (A descent stands on no node twice, so the kernel applies this as the descent leaves each node, its scores taken.)
 *              A failed range check ends the tree's work for the call: that descent gets leaf = -1 with src the node it stood on, and
 *              every later descent of the tree is not made.  A descent that is not made -- after a failed check, i in [k, stride), every
 *              entry of a tree with finished_dev[m] != 0 or n0 outside [1, cap] -- is written as src = m*cap, dst = n_trees*cap, act =
 *              num_actions, leaf = -1, so every call writes all four arrays in full.  Nothing is written into the forest.
 *     qg_mcts_backup_many   Per tree, for i = 0 .. k-1 in that order, the QG_MCTS_BACKUP rule of qg_mcts_backup with every check it has,
 *              on entry m*stride + i.  n_nodes grows as the expansions are linked, so the i-th expanding entry must name the then-current
 *              n_nodes, which qg_mcts_select_many's numbering does.  An entry that fails a check is skipped and later entries go on (an
 *              expansion that was skipped makes the next one's j = n_nodes check fail by itself); n_nodes outside [1, cap] at entry
 *              skips the tree.
 *              With k = stride = 1 both calls give exactly what qg_mcts_select and qg_mcts_backup give, for any forest content and any
 *              virtual_loss; after a select / backup pair the forest's visits of every node that existed at entry equal the overlay's
 *              (in a tree none of whose descents was refused: a refused descent leaves virtual visits and no real ones).
 *              Limits: 1 <= k <= stride <= 64 (the pending edges live in the lanes of the tree's wave, the overlay is qg_mcts_select's
 *              LDS copy), virtual_loss finite and >= 0, n_trees*stride < 2^31 - 1: QG_ERR_INVALID beyond; the forest's own limits and
 *              error codes as above.  One launch each, one wave per tree, plain vector loads and stores, no atomics, no host reads,
 *              capturable.  In the backup a location that a later entry reads after an earlier one stored it has one lane that does
 *              both (child[x][a]: lane a % 64; the per-node fields and the walk: lane 0). */
typedef struct qg_mcts_forest {
    int32_t *parent;
    float *reward;
    float *value;
    int32_t *visits;
    float *wsum;
    uint8_t *terminal;
    int32_t *child;
    float *prior;
    int32_t *n_nodes;
    uint64_t n_trees;
    uint32_t cap, num_actions;
} qg_mcts_forest;
typedef enum { QG_MCTS_ROOT = 0, QG_MCTS_BACKUP = 1 } qg_mcts_mode;
size_t qg_mcts_forest_bytes(uint64_t n_trees, uint32_t cap, uint32_t num_actions);
int qg_mcts_select(const qg_mcts_forest *forest, float c_puct, const uint8_t *finished_dev, int32_t *src_dev, int32_t *dst_dev, int32_t *act_dev,
                   int32_t *leaf_dev, void *stream);
int qg_mcts_backup(const qg_mcts_forest *forest, int mode, const int32_t *src_dev, const int32_t *dst_dev, const int32_t *act_dev,
                   const int32_t *leaf_dev, const float *logp_dev, uint64_t ld, const float *values_dev, const float *reward_dev,
                   const uint8_t *done_dev, void *stream);
typedef enum { QG_MCTS_MOST_VISITED = 0, QG_MCTS_SAMPLE = 1 } qg_mcts_decide_mode;
int qg_mcts_decide(const qg_mcts_forest *forest, int mode, uint64_t seed, uint64_t counter, const uint8_t *finished_dev,
                   int32_t *move_dev, int32_t *counts_dev, uint64_t counts_ld, void *stream);
int qg_mcts_rebase(const qg_mcts_forest *forest, const int32_t *move_dev, const uint8_t *finished_dev, int32_t *env_src_dev, void *stream);
int qg_mcts_select_many(const qg_mcts_forest *forest, float c_puct, float virtual_loss, uint32_t k, uint32_t stride, const uint8_t *finished_dev,
                        int32_t *src_dev, int32_t *dst_dev, int32_t *act_dev, int32_t *leaf_dev, void *stream);
int qg_mcts_backup_many(const qg_mcts_forest *forest, uint32_t k, uint32_t stride, const int32_t *src_dev, const int32_t *dst_dev,
                        const int32_t *act_dev, const int32_t *leaf_dev, const float *logp_dev, uint64_t ld, const float *values_dev,
                        const float *reward_dev, const uint8_t *done_dev, void *stream);
/* Self-play samples: qg_az_pack turns the log of a finished batch of sampled tree searches into the dense batch an AlphaZero-style learner
 * reads (the reference's twisterl.rl.AZ collects the same three things per decision: observation, visit distribution, return).  Episodes end
 * at different decisions, so a [T][E] log is mostly dead rows; the call compacts the live decisions in a fixed order, normalises the counts
 * and computes the value target on the way.  Like the search kernels it knows no env and no policy.  tests/azmodel.py restates the rules
 * in numpy; results agree bit for bit.  T decisions, E episodes, A = num_actions; everything is on the device.
 *   in    counts_dev i32[T][E][counts_ld], counts_ld >= A, columns past A are never read: the rows qg_mcts_decide wrote;
 *         reward_dev f32[T][E]: the reward of the real env's step at decision t;  live_dev u8[T][E]: != 0 where episode e made decision t;
 *         move_dev i32[T][E];  words_dev optional, [T][E][W] words of word_bytes in {1, 4, 8}: the packed observation before the move, as
 *         qg_vec_observe_packed writes it;  capacity >= 1.
 *   out   n_dev i32[3]; index_dev i32[capacity]; z_dev f32[capacity]; move_out_dev i32[capacity]; pi_dev f32[capacity][pi_ld], pi_ld >= A;
 *         words_out_dev [capacity][W] (required with words_dev).  scratch_dev: qg_az_pack_scratch_bytes(T, E) bytes, the caller's, 4-aligned.
 *   1 rows     total(t,e) = the sum over a < A of counts[t][e][a], in 64-bit integers.  A row is BAD if any count is negative or total >=
 *              2^24 (f32(total) would not be exact).  It is VALID iff live != 0, it is not bad and total > 0.  The counts of a row that is
 *              not live are never read.
 *   2 value    G(T,e) = 0; for t = T-1 .. 0: G(t,e) = reward[t][e] + G(t+1,e) where live[t][e] != 0, else G(t,e) = G(t+1,e).  The sum is
 *              one f32 addition, round to nearest, contracted with nothing: the undiscounted return to go in the order of the backup's
 *              G = reward[y] + G, what the value head is taken for inside the tree.  A decision that is live but not valid still
 *              contributes its reward; live need not be monotone in t.
 *   3 order    The rank of a valid (t,e) is the number of valid (t',e') with t'*E + e' < t*E + e.  It is written iff rank < capacity.
 *   4 sample   At its rank: index = t*E + e; z = G(t,e), its own bits; move_out = move[t][e], copied as it stands; pi[a] =
 *              f32(counts[a]) / f32(total) for a < A, one correctly rounded f32 division each (the plain `/` of qg_mcts_select); the W
 *              words copied.  Columns [A, pi_ld) and every entry at a rank >= n[0] are not written.
 *   5 n        n = { min(valid, capacity), valid, the number of live rows that are bad }, written in full by every call.
 *   6          No randomness; the result does not depend on the launch geometry.  Inputs, outputs and scratch may not alias.
 * Four launches on `stream` (mark the rows and count per chunk of 256 items; the returns, a lane per episode; one workgroup scans the
 * per-chunk counts; write), no host reads, no synchronisation, capturable into a hipGraph.  The prefix sum is ballots and popcounts within
 * a wave, LDS across a workgroup's waves and the scratch array of per-chunk counts between launches: no workgroup waits for another, no
 * atomics, plain vector loads and stores only.  A row of counts is read by one wave, four actions per lane, once to mark it and, if valid
 * and of rank < capacity, once more to write pi.
 * Limits: A <= 256, T*E < 2^31 - 1, W*word_bytes <= 2048: QG_ERR_UNSUPPORTED beyond.  QG_ERR_INVALID for a null required pointer, a zero
 * size (T, E, A, capacity; W with words_dev), counts_ld < A, pi_ld < A, a word_bytes other than 1, 4, 8, a misaligned 32-bit array (words:
 * to word_bytes) or words_dev without words_out_dev.  qg_az_pack_scratch_bytes gives 8 bytes per item + 8 per chunk, 0 beyond the limits. */
size_t qg_az_pack_scratch_bytes(uint64_t T, uint64_t E);
int qg_az_pack(const int32_t *counts_dev, uint64_t counts_ld, const float *reward_dev, const uint8_t *live_dev, const int32_t *move_dev,
               const void *words_dev, int word_bytes, uint32_t W, uint64_t T, uint64_t E, uint32_t num_actions, uint64_t capacity,
               int32_t *n_dev, int32_t *index_dev, float *z_dev, int32_t *move_out_dev, float *pi_dev, uint64_t pi_ld, void *words_out_dev,
               void *scratch_dev, void *stream);
/* Twists, batched: the symmetries of the coupling map as views of the observation (Env::twists, clifford.rs:370-372; symmetry.rs:205-295).
 * For CliffordEnv, LinearFunctionEnv and PermutationEnv twist t is a pair: obs_perms[t] over the flat dense observation (rows * cols entries)
 * and act_perms[t] over the actions.  THE DEFINITION, proved on the oracle env for every kind, twist and action (tests/test_twist_views.py):
 *   view:    view_t(obs)[i] = obs[obs_perms[t][i]]                    -- a GATHER through obs_perms (the gather form holds; the scatter form,
 *                                                                        out[obs_perms[t][i]] = obs[i], fails for every automorphism that is
 *                                                                        not an involution, e.g. the rotations of a ring)
 *   action:  an action a chosen on the view is the real action act_perms[t][a]   (PauliEnv's own convention, pauli.rs:596)
 *   equivariance, for every state s, twist t, action a:
 *            view_t(observe(step(s, act_perms[t][a]))) == observe(step(set_state(view_t(observe(s))), a))
 * so a policy may look at a target through any twist, choose there, and the un-twisted action does to the real env what the chosen one
 * does to the viewed one.
 *
 * qg_vec_twists: Env::twists of the batch's configuration with the contract of qg_env_twists (and the same host code): returns the number of
 * twists; obs_perms_out[n * obs_size], act_perms_out[n * num_actions] are filled when non-NULL (count first, then fill).  0 when add_perms
 * is off, always 0 for PauliEnv (pauli.rs:675-679: it permutes inside observe / step). */
int64_t qg_vec_twists(const qg_vec *v, int64_t *obs_perms_out, int64_t *act_perms_out);
/* The view of a packed observation: out_dev[e * rows*cols + i] = element obs_perms[twist_idx[e]][i] of what qg_expand_packed would write for env
 * e, as `out_dtype` (int8, f16, bf16, f32).  packed_dev: the batch's QG_FMT_PACKED observation as qg_vec_observe_packed writes it, [batch, rows]
 * words of word_bytes (4 / 8: bit c = column c; 1: the byte is the set column); obs_perms_dev int32 [n_twists, rows*cols]; twist_idx_dev
 * int32 [batch].  Like qg_beam_merge the kernel knows no env: any words and any table will do (the table need not be a permutation).  A
 * twist_idx[e] outside [0, n_twists) gives env e its untwisted observation (the host cannot see device indices); a table entry outside
 * [0, rows*cols) reads as 0.  Limits: rows * word_bytes <= 2048 (an env's words live in LDS), batch < 2^31, n_twists * rows * cols < 2^31;
 * QG_ERR_UNSUPPORTED beyond.  QG_ERR_INVALID for a null pointer, a zero size, cols that do not fit the word (> 8 * word_bytes; > 256 for bytes),
 * an unknown dtype or word_bytes, or a buffer not aligned to its element size.  Output made of whole 16-byte chunks per env (rows*cols*element
 * size a multiple of 16, out_dev and obs_perms_dev 16-byte aligned) is written with 16-byte stores, a wave 1 KiB at a time; other shapes one
 * element per thread.  Stream-ordered on `stream`, one launch, no synchronisation, capturable into a hipGraph. */
int qg_twist_expand_packed(const void *packed_dev, int word_bytes, uint64_t batch, uint32_t rows, uint32_t cols, const int32_t *obs_perms_dev,
                           uint32_t n_twists, const int32_t *twist_idx_dev, void *out_dev, int out_dtype, void *stream);
/* The handle's own path: qg_vec_observe_packed into a buffer of the handle, then the view through the handle's obs_perms (two launches).  The
 * table is uploaded once, by the first call (which therefore may not be made inside a stream capture; later ones may), and is owned by the
 * handle.  QG_ERR_INVALID on a handle without twists (add_perms off, or a PauliEnv). */
int qg_vec_observe_twisted(qg_vec *v, const int32_t *twist_idx_dev, void *out_dev, int out_dtype, void *stream);
/* The same view as packed words, the [batch, rows] uint64 format qg_policy_embed_words reads (a packed -> packed bit gather): bit c of
 * out_dev[e * rows_out + r] = element obs_perms[twist_idx[e]][r * cols + c] of what qg_expand_packed would write for env e (r < rows,
 * c < cols); bits c >= cols are 0, and so are the words rows <= r < rows_out -- padding, so that a caller reaches the even row count
 * qg_policy_embed_words asks for whatever the env's.  The input contract is qg_twist_expand_packed's: words of 1, 4 or 8 bytes (1: the byte is
 * the set column), any table, an entry outside [0, rows*cols) reads as 0, a twist_idx[e] outside [0, n_twists) gives the untwisted
 * observation.  The output is always 64-bit words, so byte words, 32-bit words and odd row counts reach the words first layer this way.
 * Limits: cols <= 64, rows * word_bytes <= 2048, rows <= rows_out <= 2 * rows + 2, batch < 2^31, n_twists * rows * cols < 2^31;
 * QG_ERR_UNSUPPORTED beyond.  QG_ERR_INVALID for a null pointer, a zero size, an unknown word_bytes, cols that do not fit the word, words or
 * tables not aligned to their element size, out_dev not 8-byte aligned.  A wave makes one output word per ballot and writes 64 of them
 * as 512 contiguous bytes; the result does not depend on the launch geometry.  Stream-ordered, one launch, no synchronisation, capturable. */
int qg_twist_pack_words(const void *packed_dev, int word_bytes, uint64_t batch, uint32_t rows, uint32_t cols, const int32_t *obs_perms_dev,
                        uint32_t n_twists, const int32_t *twist_idx_dev, uint64_t *out_dev, uint32_t rows_out, void *stream);
/* The handle's own path, the words sibling of qg_vec_observe_twisted: qg_vec_observe_packed into the handle's buffer, then qg_twist_pack_words
 * through the handle's obs_perms -- the one table both calls share (whichever is called first uploads it, outside a stream capture).
 * out_dev: uint64 [batch, rows_out].  QG_ERR_INVALID on a handle without twists. */
int qg_vec_observe_twisted_words(qg_vec *v, const int32_t *twist_idx_dev, uint64_t *out_dev, uint32_t rows_out, void *stream);
/* out[e] = act_perms[twist_idx[e]][actions[e]]: actions chosen on views -> real actions.  actions_dev / out_dev: [batch] of `action_dtype`
 * (qg_action_dtype; may be the same array), act_perms_dev int32 [n_twists, num_actions].  An action outside [0, num_actions) passes through
 * unchanged (the "no gate" parking action of the search loops, clifford.rs:324), and so does every action of an env whose twist_idx is outside
 * [0, n_twists).  One thread per env; stream-ordered, one launch, capturable. */
int qg_untwist_actions(const void *actions_dev, int action_dtype, uint64_t batch, uint32_t num_actions, const int32_t *act_perms_dev,
                       uint32_t n_twists, const int32_t *twist_idx_dev, void *out_dev, void *stream);
/* Generalised advantage estimation over a [n_steps, batch] rollout (f32, done_t = the episode ended
 * with step t): delta_t = r_t + gamma*V_{t+1}*(1-done_t) - V_t, A_t = delta_t +
 * gamma*lambda*(1-done_t)*A_{t+1}, returns = A + V.  last_values_dev: V after the last step
 * (NULL = 0); returns_dev may be NULL. */
int qg_gae(const float *rewards_dev, const float *values_dev, const uint8_t *dones_dev, const float *last_values_dev, float gamma,
           float gae_lambda, size_t n_steps, uint64_t batch, float *advantages_dev, float *returns_dev, void *stream);

/* The policy's first layer computed straight from the resident bit-packed state (no dense observation
 * is written or read): out[e, n] = act(sum_k obs[e, k] * W[n, k] + bias[n]) in bf16, obs = Env::observe
 * densified and flattened as in qg_vec_observe_dense_as -- the Linear(prod(obs_shape) -> hidden) that opens
 * the reference's policy network (rl/configs.py:531-607; examples/models/ *.pt).  Handles whose rows are resident uint32
 * words only (CliffordEnv N <= 16, LinearFunctionEnv 8 < N <= 32 with or without add_inverts; QG_ERR_UNSUPPORTED otherwise);
 * hidden % 64 == 0.
 * qg_vec_pack_embedding re-orders W ([hidden, ld] of f32 / bf16, ld >= obs_rows*obs_cols) into the k order
 * the kernel's in-register bit expansion produces (qg_vec_embed_packed_bytes bytes; repeat after every
 * optimiser step); qg_vec_embed runs the layer: bias_dev f32 [hidden] or NULL, relu != 0 applies max(0, .),
 * out_dev bf16 [batch, ld_out], 16-byte aligned, ld_out >= hidden and a multiple of 8. */
size_t qg_vec_embed_packed_bytes(const qg_vec *v, uint32_t hidden);
int qg_vec_pack_embedding(qg_vec *v, const void *weight_dev, int weight_dtype, uint64_t ld, uint32_t hidden, void *packed_dev, void *stream);
int qg_vec_embed(qg_vec *v, const void *packed_dev, const float *bias_dev, uint32_t hidden, int relu, void *out_dev, uint64_t ld_out, void *stream);
/* qg_vec_observe_packed(v, obs_packed_dev, stream) and qg_vec_embed(...) of the same state: the observation a rollout stores and the
 * first layer of the policy that acts on it.  One launch for small batches (the layer's kernel holds the bits it would export), the
 * two launches otherwise; results are those of the two calls. */
int qg_vec_embed_observe(qg_vec *v, const void *packed_dev, const float *bias_dev, uint32_t hidden, int relu, void *out_dev, uint64_t ld_out,
                         void *obs_packed_dev, void *stream);

/* The same first layer from packed observation WORDS instead of a handle's resident state: words_dev = [batch, rows] uint64,
 * bit c of word r = observation entry (r, c) -- what qg_vec_observe_packed writes for handles with 64-bit row words (PauliEnv:
 * 2N rows of 2N + max_rotations columns; CliffordEnv N > 16; LinearFunctionEnv N > 32), a packed rollout buffer, or another
 * rank's all-gathered shard, so the learner side never unpacks either.  rows even, cols <= 64, hidden % 128 == 0
 * (qg_policy_embed_words_packed_bytes returns 0 otherwise); W is [hidden, ld] with ld >= rows*cols, k = r*cols + c as in
 * qg_vec_observe_dense_as; words 16-byte aligned; output as qg_vec_embed.  The weights stream through LDS, so K is not limited. */
size_t qg_policy_embed_words_packed_bytes(uint32_t rows, uint32_t cols, uint32_t hidden);
int qg_policy_pack_embed_words(const void *weight_dev, int weight_dtype, uint64_t ld, uint32_t rows, uint32_t cols, uint32_t hidden, void *packed_dev,
                               void *stream);
int qg_policy_embed_words(const uint64_t *words_dev, uint64_t batch, uint32_t rows, uint32_t cols, const void *packed_dev, const float *bias_dev,
                          uint32_t hidden, int relu, void *out_dev, uint64_t ld_out, void *stream);

/* The policy's last layer and the categorical draw in one kernel: logits[e, a] = sum_k h[e, k] W[a, k] + b[a] stay in
 * registers and go straight into the exponential race of qg_sample_actions (same counter RNG, hash and tie rule, so
 * the same seed / counter / clock give the same draw for the same logits); outputs as there, values_dev[e] = the value
 * head W[value_row] . h[e] + b[value_row].  h_dev: bf16 [batch, ld_h], 16-byte aligned, ld_h % 8 == 0.  Limits
 * (qg_policy_head_packed_bytes returns 0 outside them): num_actions <= 222, in_features % 64 == 0, <= 512, packed head
 * <= 144 KiB.  qg_policy_pack_head re-orders W ([rows, ld] f32 / bf16) and the bias ([rows], same dtype, or NULL)
 * into MFMA fragment order: rows 0..num_actions-1 are the actions, row value_row (>= 0, any index) the value head.
 * Logits (this call and the qg_policy_mid_head_sample / qg_vec_mid_head_sample_step family): finite, |logit| <= 1e37 so that logit - max
 * stays finite.  The padding rows that fill the last 32-action tile carry a bias of -1e30, and a logit below -1e29 is a MASKED action, as
 * -inf is for qg_sample_actions: qg_policy_pack_head stores a bias at or below -1e30 (-inf, the dtype's lowest value used as a mask) as
 * -1e30 -- -inf itself has no two-term bf16 form -- and a row whose largest logit lies below -1e29 has no live action: action 0, log-prob 0,
 * entropy 0.  The bias is carried as two bf16 terms (16 significant bits); weights are bf16.  NaN and +inf (in W, the bias or h) are
 * outside the contract, with the rule of qg_sample_actions: the call terminates, the action lies in [0, num_actions), a NaN logit never
 * wins, log-prob and entropy of such a row are unspecified. */
size_t qg_policy_head_packed_bytes(uint32_t num_actions, uint32_t in_features);
/* after_mid != 0: pack for qg_policy_mid_head_sample (whose head fragments come out of an accumulator tile in a permuted k order) */
int qg_policy_pack_head(const void *weight_dev, const void *bias_dev, int dtype, uint64_t ld, uint32_t in_features, uint32_t num_actions,
                        int32_t value_row, int after_mid, void *packed_dev, void *stream);
int qg_policy_head_sample(const void *h_dev, uint64_t ld_h, uint64_t batch, uint32_t in_features, const void *packed_dev, uint32_t num_actions,
                          uint64_t seed, uint64_t counter, const uint64_t *clock_dev, void *actions_dev, int action_dtype, float *logp_dev,
                          float *entropy_dev, float *values_dev, void *stream);
/* The layer before the head as well: h2 = relu(h W2^T + b2) (mid_features = 256 outputs, in_features % 32 == 0, <= 2048) feeds the head
 * from registers -- with qg_vec_embed in front, the reference's default policy (rl/configs.py:531-607) runs forward and samples
 * without a tensor library and without writing an observation, h2 or logits.  qg_policy_pack_mid packs W2 [mid_features, ld] / b2;
 * the head must be packed with after_mid = 1. */
size_t qg_policy_mid_packed_bytes(uint32_t in_features, uint32_t mid_features);
int qg_policy_pack_mid(const void *weight_dev, const void *bias_dev, int dtype, uint64_t ld, uint32_t in_features, uint32_t mid_features,
                       void *packed_dev, void *stream);
int qg_policy_mid_head_sample(const void *h_dev, uint64_t ld_h, uint64_t batch, uint32_t in_features, const void *packed_mid_dev, uint32_t mid_features,
                              const void *packed_head_dev, uint32_t num_actions, uint64_t seed, uint64_t counter, const uint64_t *clock_dev, void *actions_dev,
                              int action_dtype, float *logp_dev, float *entropy_dev, float *values_dev, void *stream);
/* The deterministic twins of qg_policy_head_sample / qg_policy_mid_head_sample: the same kernels with another epilogue, which writes the
 * whole row of log-probabilities and the arg-max instead of one draw -- what a greedy or a beam search asks of the policy (the rows go
 * straight into qg_beam_select).  Operands, packing (qg_policy_pack_head without / with after_mid, qg_policy_pack_mid), limits, alignment
 * rules and the choice between the small-batch and the large-batch kernel are those of the _sample call; the logit contract is the one
 * stated above qg_policy_head_packed_bytes.  There is no seed, counter or clock: for a given batch size and device the result depends on
 * the operands alone (no atomics, no order that varies from launch to launch).  The small-batch and the large-batch kernel -- chosen by batch
 * size, in_features and the device's CU count, as for the _sample call -- add the terms of s below in different orders, so the same row can
 * differ between the two in the last bits of logf(s), and with it in every log-prob of the row and the entropy: equal up to the rounding of
 * that sum, not bit for bit (the _sample call's log-prob and entropy behave the same way).  The rules:
 *   - With m = the row's largest logit and s = sum_a exp(logit[a] - m) (the hardware's exp2 of (logit - m) * log2(e), as in the draw; f32),
 *     logp_rows_dev[e * ld_logp + a] = (logit[a] - m) - logf(s) for a < num_actions: two f32 subtractions, nothing contracted -- the very
 *     expression, operand order and bits of the log-prob the _sample call reports for an action it drew, and entropy_dev / values_dev are
 *     that call's bits as well.
 *   - A masked action (logit below -1e29: a bias at or below -1e30, -inf, the dtype's lowest) gets -inf, which qg_beam_select reads as "no
 *     such candidate".  An action that is merely far below the maximum (exp flushes to 0 from about 87 on) keeps its finite value.
 *   - actions_dev[e] = the action of the largest logit, equal logits to the lowest action index; padding rows and the value row never win.
 *     best_logp_dev[e] = the log-prob of that action, the bits of logp_rows_dev[e * ld_logp + action].
 *   - A row without a live action (largest logit below -1e29) gives action 0, best log-prob 0, entropy 0 and a row of -inf: the empty row of
 *     the _sample call.
 *   - NaN and +inf are outside the contract as there: the call terminates and the action lies in [0, num_actions).
 * logp_rows_dev: f32 [batch, ld_logp], ld_logp >= num_actions (QG_ERR_INVALID otherwise).  Columns num_actions .. ld_logp-1 and rows >= batch
 * are never written.  A row base and stride that are multiples of 16 bytes get 16-byte stores, any 4-byte aligned layout works.  EVERY
 * output pointer may be NULL: without logp_rows_dev no row is written (the arg-max-only step of a greedy search); all five NULL is
 * QG_ERR_INVALID.  Limits beyond the fused head: QG_ERR_UNSUPPORTED, as for the _sample call.  Stream-ordered on `stream`, one launch, no
 * synchronisation, capturable into a hipGraph. */
int qg_policy_head_logp(const void *h_dev, uint64_t ld_h, uint64_t batch, uint32_t in_features, const void *packed_dev, uint32_t num_actions,
                        float *logp_rows_dev, uint64_t ld_logp, void *actions_dev, int action_dtype, float *best_logp_dev,
                        float *entropy_dev, float *values_dev, void *stream);
int qg_policy_mid_head_logp(const void *h_dev, uint64_t ld_h, uint64_t batch, uint32_t in_features, const void *packed_mid_dev, uint32_t mid_features,
                            const void *packed_head_dev, uint32_t num_actions, float *logp_rows_dev, uint64_t ld_logp, void *actions_dev,
                            int action_dtype, float *best_logp_dev, float *entropy_dev, float *values_dev, void *stream);
/* qg_policy_mid_head_sample followed, in the same launch, by Env::step of handle `v` with the action it drew (the lane that holds an env's draw
 * gathers / scatters that env's rows like qg_vec_step does: same results, one launch less per collection step), and by the compaction of
 * the envs whose episode ended with this step: the next qg_vec_reset_done finds its list ready and launches only the reset itself.
 * batch, num_actions, the device clock and the env outputs are the handle's; rewards_dev / dones_dev: per-step outputs as in
 * qg_vec_rollout (may be NULL).  TILE-layout handles (CliffordEnv N <= 16 with or without add_inverts -- the coin is the handle's counter
 * RNG, as in qg_vec_step without coins; LinearFunctionEnv 8 < N <= 32 without add_inverts); QG_ERR_UNSUPPORTED otherwise.  Where the step
 * cannot ride in the sampling kernel (add_inverts beyond the small-batch kernel, or a state that is not symplectic) the call issues
 * the env's own step launch after it: same results. */
int qg_vec_mid_head_sample_step(qg_vec *v, const void *h_dev, uint64_t ld_h, uint32_t in_features, const void *packed_mid_dev, uint32_t mid_features,
                                const void *packed_head_dev, uint64_t seed, uint64_t counter, void *actions_dev, int action_dtype, float *logp_dev,
                                float *entropy_dev, float *values_dev, float *rewards_dev, uint8_t *dones_dev, void *stream);
/* ... and by qg_vec_reset_done(v, reset_seed): the envs whose episode ended with this step start their next one (clifford.rs:306-318)
 * before the call returns to the stream -- inside the same launch for small batches, as the reset's own launch otherwise; results are
 * those of the two calls.  A collection loop that uses it needs no qg_vec_reset_done of its own after the first step. */
int qg_vec_mid_head_sample_step_reset(qg_vec *v, const void *h_dev, uint64_t ld_h, uint32_t in_features, const void *packed_mid_dev, uint32_t mid_features,
                                      const void *packed_head_dev, uint64_t seed, uint64_t counter, void *actions_dev, int action_dtype, float *logp_dev,
                                      float *entropy_dev, float *values_dev, float *rewards_dev, uint8_t *dones_dev, uint64_t reset_seed, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU hand-over (BASELINE.json north_star: "batches shard trivially over the 8 GPUs of one node with an RCCL all-gather
 * over xGMI only for the observation tensor handed back to the learner").  One process (or thread) per GPU; rank r
 * of W owns the contiguous env range [r*B, (r+1)*B) of one batch of W*B envs (qg_vec_set_env_base makes its draws those of the
 * whole batch).  Env::step (clifford.rs:321-347) touches one env only, so stepping needs no exchange; what crosses GPUs is what
 * the reference's collector reads from every env after a step -- Env::observe (clifford.rs:361-368), Env::reward (:355),
 * Env::is_final (:353), Env::success (:357-359) -- as ONE flat shard per rank:
 *
 *   [ obs: B * packed_words_per_env * packed_word_bytes (qg_vec_observe_packed) | pad to 4 | reward: f32[B] |
 *     is_final: u8[B] | pad to 4 | success: u8[B] | pad to 16 ]
 *
 * Two transports: ncclAllGather of librccl.so.1 (loaded on the first qg_comm_init, not a link-time dependency), and a direct
 * write in which every rank copies its shard into a window in each peer's HBM over xGMI (hipIpc-shared, one link per peer) and
 * raises a per-source flag -- no collective library on the data path.  A gathered buffer is W consecutive shards, rank order =
 * env order.
 * ---------------------------------------------------------------------------------------- */
typedef struct qg_comm qg_comm;
#define QG_COMM_ID_BYTES 128   /* = NCCL_UNIQUE_ID_BYTES */
#define QG_P2P_HANDLE_BYTES 64 /* = HIP_IPC_HANDLE_SIZE */
#define QG_COMM_MAX_WORLD 16

typedef struct {
    uint64_t batch;          /* envs in the shard */
    uint64_t bytes;          /* size of one rank's shard (multiple of 16) = stride between ranks in a gathered buffer */
    uint64_t obs_offset;     /* 0 */
    uint64_t obs_bytes;      /* batch * packed_words_per_env * packed_word_bytes */
    uint64_t reward_offset;  /* f32[batch] */
    uint64_t final_offset;   /* u8[batch]  Env::is_final */
    uint64_t success_offset; /* u8[batch]  Env::success */
} qg_shard_layout;

/* Layout of one rank's shard for this handle (same for every rank that holds the same env kind and batch). */
int qg_vec_learner_shard_layout(const qg_vec *v, qg_shard_layout *out);
/* Write this handle's shard to shard_dev (qg_shard_layout.bytes, 16-byte aligned): two launches on `stream` (the packed
 * observation as qg_vec_observe_packed writes it -- for a PauliEnv this counts as one observe() -- and the three per-env arrays). */
int qg_vec_pack_learner_shard(qg_vec *v, void *shard_dev, void *stream);

/* Rank 0 calls qg_comm_unique_id and hands the 128 bytes to every rank by whatever channel the host has (ncclGetUniqueId). */
int qg_comm_unique_id(uint8_t id_out[QG_COMM_ID_BYTES]);
/* Collective over all ranks: ncclCommInitRank on GPU `device`.  world == 1 is allowed. */
int qg_comm_init(const uint8_t id[QG_COMM_ID_BYTES], int rank, int world, int device, qg_comm **out);
/* A communicator without RCCL, for the direct-write transport only (handles are exchanged by the host: qg_comm_p2p_export /
 * qg_comm_p2p_open).  Not collective. */
int qg_comm_init_local(int rank, int world, int device, qg_comm **out);
/* With the direct-write transport, call it only when every rank is done with every window (a barrier of the host's own): peers write into this
 * rank's window and this rank holds mappings of theirs. */
void qg_comm_destroy(qg_comm *c);
int qg_comm_rank(const qg_comm *c);
int qg_comm_world(const qg_comm *c);

/* qg_vec_pack_learner_shard into a buffer of the communicator, then ncclAllGather of it into out_dev
 * (world * qg_shard_layout.bytes), both on `stream`: stream-ordered after the steps enqueued before it. */
int qg_vec_gather_learner_shard(qg_vec *v, qg_comm *c, void *out_dev, void *stream);
/* The same, double buffered and overlapped with what `stream` does next: submit snapshots the shard on `stream` (the pack
 * launches) and hands the PREVIOUS snapshot to ncclAllGather on the communicator's own stream; flush hands over the last one.  The
 * hand-over goes through the host (wait for the snapshot's event, then enqueue the collective), not through a stream-to-stream
 * event wait, which on ROCm 7 / MI355X slows every later hipGraph replay on the stepping stream by ~40 % (tools/gather_probe.py);
 * the host therefore runs at most one snapshot ahead of the device.  latest waits for the most recently handed-over collective
 * and returns its buffer (owned by the communicator, valid until two more submits), or NULL in *gathered_dev when none exists. */
int qg_comm_gather_submit(qg_comm *c, qg_vec *v, void *stream);
int qg_comm_gather_flush(qg_comm *c);
int qg_comm_gather_latest(qg_comm *c, const void **gathered_dev);

/* Direct write.  Set-up, once per communicator: every rank allocates its window (header + 2 parities x world x shard_bytes of
 * uncached device memory), the hipIpc handles are exchanged, every rank maps the others' windows.  qg_comm_p2p_connect does all
 * three over the communicator's RCCL (collective); without RCCL the host calls qg_comm_p2p_export on every rank, moves the
 * QG_P2P_HANDLE_BYTES to every other rank itself (rank order) and calls qg_comm_p2p_open (a rank never opens its own handle). */
int qg_comm_p2p_connect(qg_comm *c, uint64_t shard_bytes);
int qg_comm_p2p_export(qg_comm *c, uint64_t shard_bytes, uint8_t handle_out[QG_P2P_HANDLE_BYTES]);
int qg_comm_p2p_open(qg_comm *c, const uint8_t *handles /* [world][QG_P2P_HANDLE_BYTES] */);
/* Epoch k (1, 2, ...; the k-th call on every rank): pack this handle's shard, copy it into slot `rank` of parity k & 1 of every
 * rank's window (own included) and store k to the per-source arrival flag there; all on `stream`.  Before overwriting a parity
 * the kernel waits (bounded) for that peer's release of epoch k - 2. */
int qg_vec_push_learner_shard(qg_vec *v, qg_comm *c, void *stream);
/* Enqueue on `stream` the wait for every rank's epoch-k arrival in this rank's window (k = the k-th call) and return the
 * gathered buffer of that epoch (world * shard_bytes, inside the window): work enqueued on `stream` afterwards may read it. */
int qg_comm_p2p_wait(qg_comm *c, const void **gathered_dev, void *stream);
/* Enqueue on `stream` the release of the epoch last waited for: its parity may be overwritten by the push of epoch k + 2. */
int qg_comm_p2p_release(qg_comm *c, void *stream);
/* Synchronise `stream` and report a peer that did not arrive / release within the deadline (QG_ERR_DEVICE), else QG_OK.
 * Deadlines: a push whose target parity was not released in time SKIPS that peer (no copy, no arrival flag: the peer's wait runs into its
 * own deadline rather than reading a torn shard) and raises a sticky error; while it is set, pushes write to nobody.  qg_comm_p2p_wait
 * returns its pointer either way: a caller that may have lost a peer checks before it trusts an epoch. */
int qg_comm_p2p_check(qg_comm *c, void *stream);
/* Restart the direct-write transport after an error: call on EVERY rank between two barriers of the host's own (all streams drained, no
 * push in flight anywhere).  Synchronises `stream`, clears the error word, this rank's window header and both epoch counters. */
int qg_comm_p2p_reset(qg_comm *c, void *stream);

/* ------------------------------------------------------------------------------------------
 * Which kernel would run.  The library picks a state layout and a kernel family from the env kind, the sizes and the options (DESIGN.md
 * section 2); this query answers from the same decision functions the launch paths call (csrc/qgym_plan.hpp) and needs no GPU, so a test can
 * pin the table.  `arg`: QG_PLAN_ROLLOUT_FUSED: number of steps T; QG_PLAN_RESET_DONE: length of the list of finished envs.
 * `nonsymplectic` != 0: some env holds a state not known to be symplectic (set_state of an arbitrary matrix with add_inverts).
 * name_out receives a short name ("TILE", "qm_step1_kernel", "scramble_tree", "qm_dense_stream_kernel", ...).  Returns QG_OK, or the status
 * qg_vec_create would return for this configuration (QG_ERR_UNSUPPORTED beyond the limits).
 * ---------------------------------------------------------------------------------------- */
typedef enum {
    QG_PLAN_LAYOUT = 0,         /* the resident state layout */
    QG_PLAN_STEP = 1,           /* qg_vec_step */
    QG_PLAN_ROLLOUT_FUSED = 2,  /* qg_vec_rollout(fused = 1) of `arg` steps */
    QG_PLAN_RESET_DONE = 3,     /* qg_vec_reset_done with `arg` finished envs, cfg->difficulty draws each */
    QG_PLAN_OBSERVE_DENSE = 4,  /* qg_vec_observe_dense into a 16-byte-aligned buffer */
    QG_PLAN_OBSERVE_PACKED = 5, /* qg_vec_observe_packed */
    QG_PLAN_STATE_I64 = 6,      /* qg_vec_get_state / set_state in QG_FMT_I64 */
    QG_PLAN_TRACK_DENSE = 7,    /* qg_vec_track_dense: "in-step", "refresh" (a full rewrite after every step) or unsupported */
    QG_PLAN_RESET_DONE_STEP = 8, /* qg_vec_reset_done_step: the one-launch kernel, or "two launches" */
    QG_PLAN_COPY_ENVS = 9        /* qg_vec_copy_envs: "copy_envs_kernel [rows x w ...]", the state regions of a tile it walks */
} qg_plan_op;
int qg_plan_query(const qg_config *cfg, uint64_t batch, uint32_t num_actions, int op, uint64_t arg, int nonsymplectic, char *name_out, size_t cap);

/* The launch geometry of the search kernels, from the same functions their launchers call (csrc/qgym_plan.hpp); needs no GPU.  No result
 * depends on it -- the kernels give the same answer whatever way the work is dealt to waves -- so a test pins which shapes reach which
 * bracket (tests/test_search_dispatch.py).  Returns the number asked for, or a negative status: QG_ERR_INVALID for an unknown op or a zero
 * size, QG_ERR_UNSUPPORTED beyond the kernel's limits (cap > 8192, num_actions > 256, width > 64, width * num_actions > 14 336; qg_beam_merge's
 * limit on an env's bytes is not checked here: the word size is no argument). */
typedef enum {
    QG_SEARCH_PLAN_MCTS_TREES = 0,   /* a = cap: trees (waves) per workgroup of qg_mcts_select and qg_mcts_rebase, min(4, 65536 / (8 cap)) */
    QG_SEARCH_PLAN_REBASE_SLICES = 1, /* a = num_actions: K = ceil(num_actions / 64) of qg_mcts_rebase's row pass */
    QG_SEARCH_PLAN_REBASE_ROWS = 2,  /* a = num_actions: the kept nodes' rows it moves per trip, 16 / K */
    QG_SEARCH_PLAN_BEAM_SELECT_WAVES = 3, /* a = width, b = num_actions: 1, 2, 4 or 8 for width * num_actions <= 1024, <= 2048, <= 6144, above */
    QG_SEARCH_PLAN_BEAM_MERGE_WAVES = 4   /* a = width, b = words_per_env, c = seen_cap (0: no history): 1 where a * b <= 512 and c <= 512, else 4 */
} qg_search_plan_op;
int64_t qg_search_plan_query(int op, uint64_t a, uint64_t b, uint64_t c);

/* ------------------------------------------------------------------------------------------
 * Scalar environment: the `Env` trait method for method (clifford.rs:285-382): a batch of one on the same kernels.  A call that changes the
 * state costs one kernel launch and one stream synchronisation where the layout keeps a resident dense observation (16- / 32-row matrices: the
 * step kernel rewrites the changed rows of the pinned observation itself), one more launch elsewhere; results and the fault word land in a pinned
 * block the getters read as plain loads.  This flavour exists for API parity -- throughput comes from qg_vec_* (README: 5.7e4 env-steps/s per host
 * thread, 1.9e5 on 32 threads -- the HIP runtime's own launch rate -- against 1e10 batched).
 * qg_env_destroy parks the handle (device buffers, stream, pinned block) in a process-wide pool for the next qg_env_clone of an env with
 * the same constructor arguments -- at most 64 per configuration, 256 in all; beyond that it frees.  qg_env_pool_clear releases the pool
 * (call it at teardown, or when a configuration will not be cloned again).
 * ---------------------------------------------------------------------------------------- */
typedef struct qg_env qg_env;

int qg_env_create(const qg_config *cfg, const qg_gate *gates, size_t n_gates, int device, qg_env **out);
int qg_env_clone(const qg_env *e, qg_env **out); /* Env: DynClone */
/* seed of the env's own RNG streams (see qg_vec_set_seed); a clone starts with its source's seed and counters */
int qg_env_set_seed(qg_env *e, uint64_t seed);
void qg_env_destroy(qg_env *e);
void qg_env_pool_clear(void);
int64_t qg_env_num_actions(const qg_env *e);
int qg_env_obs_shape(const qg_env *e, int64_t out[2]);
int qg_env_set_difficulty(qg_env *e, int64_t d);
int64_t qg_env_get_difficulty(const qg_env *e);
int qg_env_set_state(qg_env *e, const int64_t *state, size_t n);
int qg_env_reset(qg_env *e, uint64_t seed);
int qg_env_step(qg_env *e, int64_t action);
/* step with the inversion coin supplied (parity runs with add_inverts) */
int qg_env_step_coin(qg_env *e, int64_t action, int coin);
int64_t qg_env_masks(const qg_env *e, uint8_t *out, size_t cap);
int qg_env_is_final(const qg_env *e);
float qg_env_reward(const qg_env *e);
int qg_env_success(const qg_env *e);
/* ascending flat indices of set observation entries; returns the count */
int64_t qg_env_observe(qg_env *e, int64_t *out, size_t cap);
int qg_env_track_solution(const qg_env *e);
/* Env::solution; entries and capacity as for qg_vec_solution: exact up to 2^31 - 2 (bit 31 of the stored word is the `solution_inv`
 * flag), UINT64_MAX beyond and for negative actions; PermutationEnv and PauliEnv log in-range actions only. */
int64_t qg_env_solution(const qg_env *e, uint64_t *out, size_t cap);
/* twists(): (obs_perms, act_perms) (clifford.rs:370-372).  Returns the number of twists;
 * obs_perms_out[n * obs_size], act_perms_out[n * num_actions] when non-NULL. */
int64_t qg_env_twists(const qg_env *e, int64_t *obs_perms_out, int64_t *act_perms_out);

#ifdef __cplusplus
}
#endif
#endif /* QGYM_H */
