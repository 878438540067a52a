/*
 * srlx.h -- C ABI of libsrlx.so, the MI355X (gfx950) native data path behind the
 * SRL (pocokhc/simple_distributed_rl) Memory / Worker / Trainer plugin surface.
 *
 * Conventions
 *   - every entry point returns an int status (SRLX_OK == 0, negative = error); no
 *     exceptions cross the ABI; srlx_last_error() returns a thread-local message.
 *   - handles are opaque, owned by the caller, created on ONE HIP device.
 *   - `on_device` = 0: array arguments are HOST pointers; the call stages them through
 *     pinned memory, runs on `stream` and returns after the results are in the host arrays.
 *     `on_device` = 1: array arguments are DEVICE pointers on the handle's device; the call
 *     only enqueues work on `stream` (no host synchronisation, HIP-graph capturable).
 *     `on_device` = 2 (srlx_per_add / _sample / _update; round 6): HOST pointers, asynchronous -- the arguments are copied
 *     into a device-visible pinned slot that the kernel reads over the link: add / update return without synchronising (later
 *     calls on the stream are ordered behind them), sample synchronises once and has no copy commands.  Arguments that do not
 *     fit a 16 KB slot take the synchronous path.
 *   - `stream` is a hipStream_t passed as void* (NULL = HIP's default stream, which is also
 *     PyTorch's default stream).
 *   - calls on one handle must be serialised by the caller (the Python shim holds a lock),
 *     matching the reference, whose memory is only ever touched under the GIL
 *     (srl/base/run/play_mp.py:248-286).
 *
 * Each group cites the reference interface it replaces (paths relative to the
 * reference repository root).  The reference-side binding a maintainer would add is
 * shown in INTEGRATION.md.
 */
#ifndef SRLX_H
#define SRLX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRLX_VERSION 1

#define SRLX_OK 0
#define SRLX_ERR_INVALID (-1)            /* bad argument */
#define SRLX_ERR_HIP (-2)                /* a HIP runtime call failed (see srlx_last_error) */
#define SRLX_ERR_NOMEM (-3)
#define SRLX_ERR_UNIFORMS_EXHAUSTED (-4) /* sample(): retries consumed the whole uniform stream */
#define SRLX_ERR_UNSUPPORTED (-5)

const char *srlx_last_error(void);
int srlx_version(void);
/* A HIP stream of priority level -1 (high) / 0 (normal) / 1 (low), non-blocking.  The device engines run the ACTORS' side on a low-priority stream: HIP keeps
 * one pool of hardware queues per level, and a HIP graph replays its branches on normal-priority internal streams -- on a pool of its own the actors' stream
 * never queues behind an update's branch (what the reference's actor / trainer PROCESSES get for free: play_mp.py:471-642). */
int srlx_stream_create(int priority_level, void **out_stream);
int srlx_stream_destroy(void *stream);
/* Measurement aid: one-thread launch writing the device's constant-rate wall clock (wall_clock64: 100 MHz) into d_buf[index]; capturable into HIP graphs. */
int srlx_debug_stamp(uint64_t *d_buf, int index, void *stream);
int srlx_device_count(int *out_count);
/* name (e.g. "gfx950"), CU count and total HBM bytes of a device */
int srlx_device_info(int device, char *arch_name, int arch_name_len, int *cu_count, int64_t *hbm_bytes);

/* ------------------------------------------------------------------------------------
 * Proportional prioritized replay (GPU-resident sum-tree)
 *
 * Replaces: srl/rl/memories/priority_memories/proportional_memory.py:13-205
 *           (SumTree + ProportionalMemory) and its pybind11 twin
 *           srl/rl/memories/priority_memories/cpp_module/src/proportional_memory.cpp:14-248,
 *           behind IPriorityMemory (srl/rl/memories/priority_memories/imemory.py:7-34).
 *
 * The tree is the reference's implicit heap: 2*capacity-1 float64 nodes, leaf slot j is
 * node j+capacity-1, parent(i) = (i-1)/2 -- LOGICALLY; in HBM three levels share a 128-byte
 * line.  `sample` returns logical TREE indices (what the reference hands back as update_args).  Tree contents are bit-identical to the reference
 * after the same call sequence: updates propagate fp64 deltas to ancestors in call order.
 * ------------------------------------------------------------------------------------ */
typedef struct srlx_per srlx_per_t;

/* how the `prio` array of add/update is to be interpreted */
#define SRLX_PRIO_NONE 0 /* add only: priority=None -> current max_priority (proportional_memory.py:121-122) */
#define SRLX_PRIO_F64 1  /* float64 values, p = (|x|+eps)^alpha in fp64 (:124; :172 with float64/int/list input) */
#define SRLX_PRIO_F32 2  /* float32 values, p = (|x|+eps)^alpha evaluated in float32 like numpy (:172), widened */
#define SRLX_PRIO_RAW 3  /* float64 values already transformed by the caller (_restore_skip, :123) */

/* ProportionalMemory.__init__ / clear  (proportional_memory.py:96-115; cpp :100-121) */
int srlx_per_create(srlx_per_t **out, int64_t capacity, double alpha, double beta_initial, double beta_steps,
                    int has_duplicate, double epsilon, int device);
int srlx_per_destroy(srlx_per_t *h);
/* switch the duplicate rule of later srlx_per_sample calls (the shim completes a batch WITH duplicates when a has_duplicate=False draw
 * cannot be satisfied: the reference does the same after 9999 tries per draw, proportional_memory.py:146-158) */
int srlx_per_set_has_duplicate(srlx_per_t *h, int has_duplicate);
/* d_counter (device int64, caller-owned, NULL to switch off): every device-side srlx_per_update call adds 1 to it -- the learner's
 * train_count (trainer.py: `self.train_count += 1` after the priority write-back, model_torch.py:113-122) kept on the device without
 * a launch of its own.  Launches queued after the update see the new value. */
int srlx_per_set_update_counter(srlx_per_t *h, int64_t *d_counter);
/* every later APPENDING srlx_per_add also adds 1 to these int64 device counters (either may be NULL), inside its own launch: an engine's ring position and the
 * counter of its policy generator advance with the add that closes a lock-step instead of in launches of their own (readers ran in earlier launches). */
int srlx_per_set_add_counters(srlx_per_t *h, int64_t *d_counter0, int64_t *d_counter1);
int srlx_per_clear(srlx_per_t *h, void *stream);
/* length() (:117-118).  Host mirror; exact as long as adds go through srlx_per_add. */
int64_t srlx_per_length(const srlx_per_t *h);
int64_t srlx_per_capacity(const srlx_per_t *h);

/* add() x n  (:120-129, SumTree.add :71-79).  Equivalent to n sequential reference add()
 * calls writing ring slots write, write+1, ... (mod capacity).  prio may be NULL for
 * SRLX_PRIO_NONE.  n <= capacity. */
int srlx_per_add(srlx_per_t *h, int64_t n, const void *prio, int prio_kind, int on_device, void *stream);

/* sample()  (:131-169, SumTree._retrieve :56-66).
 *   uniforms[0..n_uniforms): the values the reference's random.random() calls (:147) would
 *     return, in order; one per descent attempt, so n_uniforms >= batch_size and more if
 *     zero-priority or duplicate draws are rejected (:150-157).
 *   step       : beta schedule input (:138-140); if d_step != NULL (device int64) it is read
 *                on the device instead (graph-capturable).
 *   out_idx    : int64[batch_size] tree indices
 *   out_w      : float64[batch_size] IS weights / max (may be NULL)
 *   out_w32    : float32[batch_size] same, cast as PriorityReplayBuffer.sample does
 *                (srl/rl/memories/priority_replay_buffer.py:235) (may be NULL)
 *   out_used   : int64[1] number of uniforms consumed, or -1 if the stream was exhausted.
 * on_device=0 additionally returns SRLX_ERR_UNIFORMS_EXHAUSTED in that case. */
int srlx_per_sample(srlx_per_t *h, int64_t batch_size, int64_t step, const int64_t *d_step, const double *uniforms,
                    int64_t n_uniforms, int64_t *out_idx, double *out_w, float *out_w32, int64_t *out_used,
                    int on_device, void *stream);
/* The host loop of the reference's memory -- add one item, sample, update (srl/rl/memories/priority_replay_buffer.py:205-258; tests/quick/rl/memories/speedtest.py:15-58)
 * -- as ONE launch per sample: `n_add` <= min(16, capacity) adds queued since the tree was last observed (host values: final leaf priorities with SRLX_PRIO_RAW, or
 * add_values = NULL with SRLX_PRIO_NONE) are applied inside the sampling launch, in order, exactly like srlx_per_add would; uniforms in and results out travel through a
 * device-visible pinned slot and the host spins on a completion flag the kernel stores last (no stream synchronisation).  batch_size <= n_uniforms <= 8192; a draw
 * whose uniforms and results do not fit one 16 KB slot (pad(8 n_uniforms) + 2 pad(8 batch_size) + pad(4 batch_size) + 512 bytes, pad rounding up to 256: up
 * to batch_size = 544 when n_uniforms = batch_size) takes srlx_per_add + srlx_per_sample(on_device = 0) instead, with the same results.  More adds than
 * min(16, capacity) is SRLX_ERR_INVALID, before anything runs.  Host pointers; results as srlx_per_sample(on_device = 0); SRLX_OK and
 * SRLX_ERR_UNIFORMS_EXHAUSTED both mean the adds were applied. */
int srlx_per_sample_after_adds(srlx_per_t *h, int64_t n_add, const double *add_values, int add_kind, int64_t batch_size, int64_t step, const double *uniforms,
                               int64_t n_uniforms, int64_t *out_idx, double *out_w, float *out_w32, int64_t *out_used, void *stream);
/* The same with the uniforms given as consecutive MT19937 outputs, two 32-bit words per uniform -- what `random.getrandbits(64 * n).to_bytes(8 * n, "little")` yields
 * and `random.random()` would have consumed (CPython: (a >> 5) * 2^26 + (b >> 6)) / 2^53 of consecutive outputs a, b): the host shim hands the generator's raw
 * words over instead of building n Python floats.  Any batch_size <= n_uniforms <= 8192, inside a slot or not; same limits on the adds.  out_slots (or NULL): the
 * data slot of every index (tree index - (capacity - 1)). */
int srlx_per_sample_after_adds_mt(srlx_per_t *h, int64_t n_add, const double *add_values, int add_kind, int64_t batch_size, int64_t step,
                                  const uint32_t *mt_words, int64_t n_uniforms, int64_t *out_idx, double *out_w, float *out_w32,
                                  int64_t *out_used, int64_t *out_slots, void *stream);
/* The learner's call without the launch that draws its uniforms: uniform j is what srlx_rng_uniform(seed, d_counter, n_uniforms, u)
 * would have put into u[j], and *d_counter advances the same way -- results identical to that call followed by
 * srlx_per_sample(..., u, n_uniforms, ..., on_device = 1).  Device pointers only; n_uniforms within the single-workgroup sampler's range. */
int srlx_per_sample_keyed(srlx_per_t *h, int64_t batch_size, const int64_t *d_step, uint64_t seed, int64_t *d_counter, int64_t n_uniforms,
                          int64_t *d_out_idx, double *d_out_w, float *d_out_w32, int64_t *d_out_used, void *stream);

/* update()  (:171-177, SumTree.update :81-86).  indices are tree indices from sample();
 * duplicates inside one call see each other's writes in list order, as in the reference. */
int srlx_per_update(srlx_per_t *h, int64_t n, const int64_t *indices, const void *prio, int prio_kind, int on_device,
                    void *stream);

/* update() of the n CONSECUTIVE ring slots first_slot, first_slot+1, ... (mod capacity) in slot order:
 * identical in effect to srlx_per_update with indices first_slot+capacity-1, ... but processed by the
 * bulk contiguous-run kernels (O(n log n) work instead of the general kernel's O(n^2 log n)). */
int srlx_per_set_range(srlx_per_t *h, int64_t first_slot, int64_t n, const void *prio, int prio_kind, int on_device,
                       void *stream);

/* backup()/restore()  (:179-205).  tree_host: 2*capacity-1 float64 (HOST pointers always). */
int srlx_per_backup(srlx_per_t *h, double *max_priority, int64_t *size, int64_t *write, double *tree_host);
int srlx_per_restore(srlx_per_t *h, double max_priority, int64_t size, int64_t write, const double *tree_host);
/* restore() from a backup of a different capacity (:195-205): clear, then re-add the
 * first old_size leaves of the old tree with _restore_skip. */
int srlx_per_restore_resized(srlx_per_t *h, int64_t old_capacity, int64_t old_size, const double *old_tree_host);

/* raw device view of the tree in its BLOCKED physical layout (16 doubles per 128-byte block, see
 * csrc/srlx_per.hip struct Tree); n_doubles = allocated doubles.  Use backup() for heap order. */
int srlx_per_tree_ptr(srlx_per_t *h, void **d_tree, int64_t *n_doubles);
/* device struct { double max_priority; int64 size; int64 write; int64 pad; } */
/* *d_out (device double) = max_priority as of this point of the stream: what `add(batch, None)` would use (proportional_memory.py:121-122) -- for callers that
 * assemble final priorities themselves (the engines' actor-side initial priorities, rainbow.py:389-398) and add them as SRLX_PRIO_RAW. */
int srlx_per_max_priority(srlx_per_t *h, double *d_out, void *stream);
int srlx_per_state_ptr(srlx_per_t *h, void **d_state);
/* re-read size/write from the device after HIP-graph replays that contained adds */
int srlx_per_refresh(srlx_per_t *h, void *stream);

/* SRLX_PRIO_NONE with a validity mask (uint8[n]): p = mask ? max_priority : 0.  Used by the
 * vectorised actor, where the ring position holding an episode's terminal frame has no transition. */
#define SRLX_PRIO_NONE_MASKED 4
/* add only, float32[n] ESTIMATES of |td| made on the actor side (rainbow.py:389-398; srlx_store_actor_td): x >= 0 -> p = (|x| + eps)^alpha on the widened value
 * (proportional_memory.py:124), x = -1 -> the current max_priority (priority = None), x = -2 -> 0 (the lock-step completed no item for the lane). */
#define SRLX_PRIO_EST_F32 5

/* ------------------------------------------------------------------------------------
 * Counter-based device RNG (the vectorised path has no reference stream to match; the
 * single-env plugin path keeps drawing from Python's `random`).  out[i] = u53(mix(seed, *d_counter, i));
 * afterwards *d_counter += 1.  Restated for tests in oracle/hot_path_oracle.py:rng_uniform.
 * ------------------------------------------------------------------------------------ */
int srlx_rng_uniform(uint64_t seed, int64_t *d_counter, int64_t n, double *d_out, void *stream);
/* rows frames of frame_bytes each, gathered through a frame-offset table (byte offsets from d_frame_base, -1 = none) into d_out[rows][frame_bytes], and the
 * table re-based onto d_out (d_rel_off[row] = row * frame_bytes, or -1): a sampled batch as ONE message from a replay rank to a learner rank -- the
 * device-path counterpart of the batches the reference's memory process puts on its queue (srl/base/run/play_mp_memory.py:253-351). */
int srlx_pack_frames(const uint8_t *d_frame_base, const int64_t *d_frame_off, int64_t rows, int64_t frame_bytes, uint8_t *d_out, int64_t *d_rel_off, void *stream);
/* A keyed pseudo-random permutation of 0..n-1 (int64), key = (seed, *d_counter); advances *d_counter by one.  Device state only: replayable inside a
 * HIP graph (the PPO engine's minibatch shuffles -- the role of the reference's per-epoch shuffle of the collected batch, srl/algorithms/ppo/ppo.py). */
int srlx_rng_permutation(uint64_t seed, int64_t *d_counter, int64_t n, int64_t *d_out, void *stream);
/* `count` permutations [count][n] in one launch: what `count` successive calls would have written (*d_counter + 0 .. count - 1); *d_counter += count. */
int srlx_rng_permutations(uint64_t seed, int64_t *d_counter, int64_t n, int count, int64_t *d_out, void *stream);

/* ------------------------------------------------------------------------------------
 * Device-resident transition store for E lock-stepped environments (uint8 or float32 frames).
 *
 * Replaces, for the vectorised engine: WorkerRun frame stacking + tracking ring
 * (srl/base/rl/worker_run.py:310-358,548-610, srl/base/spaces/box.py:303-312), the Rainbow
 * worker's n-step item assembly incl. terminal padding (srl/algorithms/rainbow/rainbow.py:331-400),
 * the zlib/pickle item storage of PriorityReplayBuffer (srl/rl/memories/priority_replay_buffer.py:205-217,242-243)
 * and the list->ndarray batch assembly of calc_target_q (rainbow.py:190-194).
 *
 * Layout: frames [E][ring_len][obs_elems] (one n-step window is contiguous), scalars [E][ring_len].
 * All envs share one ring position p that advances once per srlx_store_commit_step.  PER slot
 * j <-> (env j % E, item time j / E); PER capacity = E * item_len, item_len = ring_len - (n_step + window).
 * ------------------------------------------------------------------------------------ */
typedef struct srlx_store srlx_store_t;
#define SRLX_OBS_U8 0  /* uint8 frames, presented to the network as float32 u8/255 (image_processor.py:140-142) */
#define SRLX_OBS_F32 1 /* float32 observations, copied */

int srlx_store_create(srlx_store_t **out, int64_t n_envs, int64_t ring_len, int64_t obs_elems, int obs_dtype, int window,
                      int n_step, int n_actions, int reward_clip, uint64_t seed, int device);
int srlx_store_destroy(srlx_store_t *h);
int64_t srlx_store_item_len(const srlx_store_t *h);   /* ring_len - (n_step + window) */
int64_t srlx_store_per_capacity(const srlx_store_t *h); /* n_envs * item_len */
/* start: write every env's first observation (device [E][obs_elems]) at position 0 */
int srlx_store_reset_all(srlx_store_t *h, const void *d_first_obs, void *stream);
/* policy input at the current position: out float32 [E][window][obs_elems] (oldest frame first,
 * zeros before the episode start: worker_run.py:277 default states + box.py:303-312) */
int srlx_store_stack_current(srlx_store_t *h, float *d_out, void *stream);
/* one lock-step commit (rainbow.py:331-352 add_tracking): action/reward/terminated/done of the
 * step taken at p, next observation -> p+1.  Envs whose previous step was `done` are in their reset
 * step: position p (the terminal frame) is marked as holding no transition and d_next_obs is their new
 * episode's first frame.  Also emits the validity mask uint8[E] of the items that became complete
 * (position p-(n_step-1)) for srlx_per_add(..., SRLX_PRIO_NONE_MASKED). */
int srlx_store_commit_step(srlx_store_t *h, const int32_t *d_actions, const float *d_rewards, const uint8_t *d_terminated,
                           const uint8_t *d_done, const void *d_next_obs, uint8_t *d_item_mask, void *stream);
/* The same commit as ONE launch with two options (the round-4 lock-step):
 *   d_next_frame_table  int64 [E][window] or NULL: the frame-offset table of the NEXT policy pass (what srlx_store_frame_table_current would write after
 *                       the position has advanced), so the next pass needs no launch of its own for it (uint8 stores; window-1 float32 stores too -- every
 *                       frame-offset table and gather of this header counts elements, so a float32 ring's offsets index float32 observations)
 *   advance             1: p advances inside the launch (srlx_store_commit_step = this with NULL, 1); 0: p stays and the caller advances it later --
 *                       srlx_store_advance, or srlx_per_set_add_counters on the position view (srlx_store_views).  Ring slot p + 1 and the scalars of p are
 *                       referenced by no stored item, so with advance = 0 the commit may run while a learner still reads the ring; p itself feeds the
 *                       learner's item lookup and must not move under it.
 *   d_bump              int64 device counter or NULL: advanced by one when the launch's last block is done (the counter of the policy generator that
 *                       srlx_qnet_forward_u8_policy only reads) */
int srlx_store_commit_step_ex(srlx_store_t *h, const int32_t *d_actions, const float *d_rewards, const uint8_t *d_terminated, const uint8_t *d_done,
                              const void *d_next_obs, uint8_t *d_item_mask, int64_t *d_next_frame_table, int advance, int64_t *d_bump, void *stream);
/* The commit of a lock-step that arrived as PACKED RECORDS (what actor ranks ship to a learner rank; replaces the unpickling of queued items in the reference's
 * trainer-side drain thread, srl/base/run/play_mp.py:248-286): environment e is lane e % envs_per_record of record e / envs_per_record; a record =
 * [action int32 x per | reward float32 x per | terminated uint8 x per | done uint8 x per | extra float32 x per x extra_floats], records record_stride bytes apart;
 * d_next_obs is the frames of all E environments in environment order.  d_est_records (or NULL): a packed buffer of the same shape whose FIRST extra field holds
 * actor-side initial-priority estimates (srl/algorithms/rainbow/rainbow.py:389-398) for the items THIS commit completes; d_est_out float32 [E] receives them, -2
 * where the commit completed no item, -1 (= "use max_priority") without d_est_records -- the array srlx_per_add(SRLX_PRIO_EST_F32) takes. */
int srlx_store_commit_step_packed(srlx_store_t *h, const uint8_t *d_records, int64_t record_stride, int64_t envs_per_record, int extra_floats, const void *d_next_obs,
                                  uint8_t *d_item_mask, const uint8_t *d_est_records, float *d_est_out, int advance, void *stream);
/* The commit at an EXPLICIT ring position (the host's count of commits) that leaves the device-resident position alone: a store whose tree add runs one lock-step
 * behind its ring commit (device/rainbow.py: the add of lock-step t rides on a side branch of update t + 1, off the lock-step's serial tail) keeps the device
 * position as the LEARNER's view -- it advances with the tree add (srlx_per_set_add_counters), so sampled leaves always resolve against the ring the tree
 * describes -- while the actors' commits run ahead of it by one.  Such a store needs one spare ring slot: srlx_store_set_item_slack(h, 1) right after
 * srlx_store_create (item_len = ring_len - (n_step + window) - slack; the slot a commit overwrites then belongs to no item even of the older view). */
int srlx_store_commit_step_at(srlx_store_t *h, int64_t position, const int32_t *d_actions, const float *d_rewards, const uint8_t *d_terminated, const uint8_t *d_done,
                              const void *d_next_obs, uint8_t *d_item_mask, int64_t *d_next_frame_table, int64_t *d_bump, void *stream);
int srlx_store_set_item_slack(srlx_store_t *h, int slack);
int srlx_store_advance(srlx_store_t *h, void *stream);
/* device views: int64 position p; uint8 needs_reset[E]; int32 step_in_episode[E] (of position p) */
int srlx_store_views(srlx_store_t *h, void **d_pos, void **d_needs_reset, void **d_step_in_ep);
/* sampled PER tree indices -> training batch (rainbow.py:190-194 + terminal padding :354-372):
 *   obs      float32 [B][n_step+1][window][obs_elems]
 *   actions  int32   [B][n_step]      rewards float32 [B][n_step]    terminated float32 [B][n_step] */
int srlx_store_gather_nstep(srlx_store_t *h, int64_t batch, const int64_t *d_tree_idx, float *d_obs, int32_t *d_actions,
                            float *d_rewards, float *d_terminated, void *stream);

/* epsilon-greedy over a batch of Q rows (rainbow.py:301-329, dqn.py:192-211):
 *   u[e][0] < eps[e] -> the floor(u[e][1]*n_valid)-th valid action, else first argmax of q with
 *   invalid actions at -inf.  invalid: uint8 [E][A] or NULL. */
int srlx_policy_epsilon_greedy(int64_t n_envs, int n_actions, const float *d_q, const float *d_eps, const double *d_u,
                               const uint8_t *d_invalid, int32_t *d_actions, void *stream);

/* synthetic 84x84-style environment batch: i.i.d. uint8 frames, reward in
 * {-1,0,1}, episodes of episode_len steps ending `terminated`. Reads the store's reset/step state. */
int srlx_synth_env_step(srlx_store_t *h, int64_t episode_len, void *d_next_obs, float *d_rewards, uint8_t *d_terminated,
                        uint8_t *d_done, void *stream);
/* The same at an EXPLICIT ring position (the host's count of commits; < 0: the device-resident position): for a store whose device position is the learner's view
 * and trails the actors' commits by one lock-step (srlx_store_commit_step_at) -- the environments belong to the actors' side and must see the actors' position. */
int srlx_synth_env_step_at(srlx_store_t *h, int64_t position, int64_t episode_len, void *d_next_obs, float *d_rewards, uint8_t *d_terminated, uint8_t *d_done,
                           void *stream);

/* Episode ledger of E device-resident environments, one call per lock-step BEFORE the commit.
 * Replaces the per-step host bookkeeping of srl/base/env/env_run.py:334-352 (step counter, episode reward sums) and
 * srl/base/run/core_play.py:200-214 (episode_rewards_list / last_episode_* at episode end).
 *   d_skip      uint8 [E] or NULL: lanes that did not take an environment step in this lock-step (the store's
 *               needs_reset view: they only received the first frame of their next episode)
 *   d_ep_return float32 [E], d_ep_len int32 [E]: running return / length of every environment (caller zeroes them once)
 *   d_ring      float32 [ring_cap][2]: (return, length) of finished episodes, appended in environment order: episode number k
 *               (counted from the ledger's start) sits in slot k % ring_cap.  When one call ends more than ring_cap episodes,
 *               only its newest ring_cap are written -- the same ring as if all had been, one after the other
 *   d_totals   32 bytes: int64 episodes finished, int64 environment steps, float64 sum of returns, int64 sum of lengths */
int srlx_episode_account(int64_t n_envs, const float *d_rewards, const uint8_t *d_done, const uint8_t *d_skip, float *d_ep_return,
                         int32_t *d_ep_len, float *d_ring, int64_t ring_cap, void *d_totals, void *stream);

/* Frame preprocessing on the device (replaces srl/rl/processors/image_processor.py:104-151: cv2.cvtColor RGB2GRAY, the trimming slice,
 * cv2.resize INTER_LINEAR, the 0to1 / -1to1 normalisation) for a batch of uint8 images [n][src_h][src_w][src_channels]:
 *   to_gray      3 channels -> 1 with OpenCV's 14-bit coefficients
 *   trim_*       the window rows [top, bottom) x columns [left, right) (0, 0, src_h, src_w = no trimming)
 *   out_h/out_w  bilinear resize with OpenCV's 8-bit fixed-point arithmetic (== the window size: no resize)
 *   d_out_u8     uint8 [n][out_h][out_w][c] (what the frame ring stores) and / or
 *   d_out_f32    float32 of the same shape, normalize 0: as is, 1: / max_val ("0to1"), 2: * 2 / max_val - 1 ("-1to1") */
int srlx_image_preprocess(int64_t n_images, int src_h, int src_w, int src_channels, const uint8_t *d_src, int to_gray, int trim_top, int trim_left,
                          int trim_bottom, int trim_right, int out_h, int out_w, uint8_t *d_out_u8, float *d_out_f32, int normalize, double max_val, void *stream);

/* ------------------------------------------------------------------------------------
 * Fused learner arithmetic
 *
 * srlx_nstep_td_huber_priority replaces, in one launch: the numpy n-step/retrace target of
 * CommonInterfaceParameter.calc_target_q (srl/algorithms/rainbow/rainbow.py:226-287), the
 * selected-Q + HuberLoss(target*w, q*w) of Trainer.train (srl/algorithms/rainbow/model_torch.py:103-105),
 * its gradient w.r.t. the online Q rows (seed for backward) and the new priorities |target - q| (:113).
 *   q_on_next, q_tg_next : float32 [B][n][A]  online / target net on states s_1..s_n
 *   q_on_0               : float32 [B][A]     online net on s_0 (requires grad on the torch side)
 *   actions int32 [B][n], rewards/terminated float32 [B][n], invalid_next uint8 [B][n][A] or NULL
 *   weights float32 [B] (IS weights)
 * outputs: target f32 [B], loss f32 [1], grad_q0 f32 [B][A], priorities f32 [B]
 * n_step <= 32.  The n discounted terms of the target are added in numpy's order (:285 np.sum: one after another below 8 terms,
 * 8 partial sums and then the tail from 8 up): without rescale the target is the reference's float32 result bit for bit.
 * Without double DQN a step whose actions are ALL invalid reads -inf from the masked target net, as the reference does (:248-251).
 * ------------------------------------------------------------------------------------ */
int srlx_nstep_td_huber_priority(int64_t batch, int n_step, int n_actions, const float *d_q_on_next,
                                 const float *d_q_tg_next, const float *d_q_on_0, const int32_t *d_actions,
                                 const float *d_rewards, const float *d_terminated, const uint8_t *d_invalid_next,
                                 const float *d_weights, double discount, double retrace_h, int enable_double_dqn,
                                 int enable_rescale, float *d_target, float *d_loss, float *d_grad_q0,
                                 float *d_priorities, void *stream);
/* Same, with the online network's Q rows of s_0..s_n in ONE buffer float32 [B][n+1][A] -- what a single forward over
 * all states of the sampled items produces (row 0 = s_0, rows 1..n = s_1..s_n): no strided copies in front of it. */
int srlx_nstep_td_huber_priority_packed(int64_t batch, int n_step, int n_actions, const float *d_q_on_all,
                                        const float *d_q_tg_next, const int32_t *d_actions, const float *d_rewards,
                                        const float *d_terminated, const uint8_t *d_invalid_next, const float *d_weights,
                                        double discount, double retrace_h, int enable_double_dqn, int enable_rescale,
                                        float *d_target, float *d_loss, float *d_grad_q0, float *d_priorities, void *stream);

/* 1-step (double-)DQN target (srl/algorithms/dqn/dqn.py:144-176, rainbow_nomultisteps.py:10-43):
 * invalid next actions are masked with min(q) of the WHOLE batch, not -inf (dqn.py:160,164).
 *   q_on_next/q_tg_next f32 [B][A]; rewards f32 [B]; undone f32 [B]; out target f32 [B]
 *   f64_accum=1: dqn.py:171 (int `undone` array promotes the expression to float64, cast at :176);
 *   f64_accum=0: rainbow_nomultisteps.py:38 (all float32).
 *   d_discount_per_sample (f32 [B], NULL = use `discount`): Agent57_light's per-actor gamma,
 *   srl/algorithms/agent57_light/agent57_light.py:218-268 (`undone` is its `dones` = int(not terminated));
 *   float32 arithmetic, requires f64_accum=0. */
int srlx_dqn_target(int64_t batch, int n_actions, const float *d_q_on_next, const float *d_q_tg_next,
                    const float *d_rewards, const float *d_undone, const uint8_t *d_invalid_next, double discount,
                    const float *d_discount_per_sample, int enable_double_dqn, int enable_rescale, int f64_accum,
                    float *d_target, void *stream);

/* torch.optim.Adam(params, lr) .step() (srl/algorithms/rainbow/model_torch.py:71,109; dqn/model_torch.py:75,119) for up
 * to 24 float32 parameter tensors in one launch.  The four pointer arrays and numels are HOST arrays of n_tensors
 * entries (device pointers, 16-byte aligned; exp_avg / exp_avg_sq are the optimizer state, zero before the first step);
 * *d_step = optimizer steps already taken (device scalar, so the call is HIP-graph replayable; the caller increments it). */
int srlx_adam_step(int n_tensors, float *const *d_params, const float *const *d_grads, float *const *d_exp_avg,
                   float *const *d_exp_avg_sq, const int64_t *numels, double lr, double beta1, double beta2, double eps,
                   const int64_t *d_step, void *stream);

/* GAE reverse scan per environment (srl/algorithms/ppo/ppo.py:389-404): for each env, episodes are
 * delimited by done[t]; the last step of an episode uses delta = r - V (no bootstrap, :396-397).
 *   rewards, values, done(uint8) laid out [T][E]; out advantages f32 [T][E].
 *   last_values f32 [E] bootstraps a horizon cut that is not an episode end (NULL = no bootstrap,
 *   which is what the reference does for every episode end, truncation included). */
int srlx_gae_scan(int64_t n_envs, int64_t horizon, const float *d_rewards, const float *d_values, const uint8_t *d_done,
                  const float *d_last_values, double discount, double gae_lambda, float *d_adv, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Rank-based prioritised replay: srl/rl/memories/priority_memories/rankbased_memory.py:13-77.
 * Which ranks are drawn depends only on N, alpha and numpy's generator and stays on the host (bit-identical
 * np.random.choice); the data-dependent half -- np.argsort(-priorities[:N]) on EVERY sample (:47) -- is a descending
 * radix sort of (priority, index) pairs in HBM + a gather of the drawn ranks.  The order is that of
 * np.argsort(-priorities[:N], kind="stable"): NaN -- what an add without a priority stores (:33-40) -- ranks last as in
 * numpy, whatever its sign or payload; -0.0 equals +0.0; ties, NaNs among themselves included, are in index order (lower
 * index first).  numpy's default introsort leaves ties unspecified: results agree with it wherever the priorities are distinct.
 *   srlx_rank_set        : add (:33-40, d_idx NULL: slots (start + i) % capacity, n <= capacity) / update (:60-62, distinct
 *                          indices inside the capacity) of float32 priorities
 *   srlx_rank_select     : out[i] = index of the ranks[i]-th largest of priorities[0..n_live)
 *   srlx_rank_priorities : device pointer of the float32 [capacity] priority array (backup / restore, :64-77)
 * ------------------------------------------------------------------------------------------------ */
typedef struct srlx_rank srlx_rank_t;
int srlx_rank_create(srlx_rank_t **out, int64_t capacity, int device);
int srlx_rank_destroy(srlx_rank_t *h);
int srlx_rank_set(srlx_rank_t *h, int64_t n, const int64_t *d_idx, const float *d_val, int64_t start, void *stream);
int srlx_rank_select(srlx_rank_t *h, int64_t n_live, int64_t n, const int64_t *d_ranks, int64_t *d_out, void *stream);
int srlx_rank_priorities(srlx_rank_t *h, float **d_prio);

/* ------------------------------------------------------------------------------------------------
 * PPO on the vectorised path (BASELINE config 5).  The reference module needs TensorFlow
 * (srl/algorithms/ppo/ppo.py:6-7) and cannot be imported in the build container: parity UNPINNED, restated
 * from the cited lines and checked against oracle/hot_path_oracle.py + torch autograd.
 *   srlx_ppo_normal_act  : ppo.py:316-339 + srl/rl/tf/distributions/normal_dist_block.py:13-20,64-74,144-149:
 *       action = loc + exp(clip(log_scale)) * N(0,1)  (keyed counter RNG, *d_counter += 1), per-dimension
 *       log-probability floored at log(1e-6) (ppo.py:322); deterministic != 0: action = loc (evaluation, :318-319).
 *       All arrays f32 [n] (n = envs x action_dim).
 *   srlx_ppo_loss_normal : compute_train_loss (ppo.py:102-169) for a Normal policy, forward + gradient seeds.
 *       loc/log_scale/action/old_logpi f32 [B][action_dim]; advantage/v/v_target/old_v f32 [B];
 *       baseline_advantage: advantage -= stop_gradient(v) (:121-122); surrogate_clip 1 = "clip" (:127-137),
 *       0 = "" (:148-149) ("kl": srlx_ppo_loss_normal_kl / srlx_ppo_loss_categorical_kl below);
 *       losses f32 [3] = policy, value, entropy as the reference reports them;
 *       grad_loc/grad_log_scale f32 [B][action_dim], grad_v f32 [B] = d(policy+value+entropy)/d(.)
 *   srlx_ppo_loss_logpi  : the same given the policy head's log-probabilities f32 [B][n_logpi]
 *       (Categorical: n_logpi = 1, the taken action); returns d loss / d new_logpi and d loss / d v.
 *   srlx_pendulum_step   : Pendulum-shaped synthetic environments (obs (cos th, sin th, thdot), one torque in
 *       [-2, 2], reward -(th^2 + .1 thdot^2 + .001 u^2), time limit `episode_len` -> done + auto-reset).
 *       state f32 [E][2], step_in_episode i32 [E], action f32 [E], obs f32 [E][3], reward f32 [E], done u8 [E].
 * ------------------------------------------------------------------------------------------------ */
int srlx_ppo_normal_act(int64_t n, const float *d_loc, const float *d_log_scale, double log_scale_min, double log_scale_max,
                        uint64_t seed, int64_t *d_counter, int deterministic, float *d_action, float *d_logprob, void *stream);
int srlx_ppo_loss_normal(int64_t batch, int action_dim, const float *d_loc, const float *d_log_scale, double log_scale_min,
                         double log_scale_max, const float *d_action, const float *d_old_logpi, const float *d_advantage,
                         const float *d_v, const float *d_v_target, const float *d_old_v, int baseline_advantage,
                         int surrogate_clip, double policy_clip_range, int enable_value_clip, double value_clip_range,
                         double value_loss_weight, double entropy_weight, float *d_losses, float *d_grad_loc,
                         float *d_grad_log_scale, float *d_grad_v, void *stream);
int srlx_ppo_loss_logpi(int64_t batch, int n_logpi, const float *d_new_logpi, const float *d_old_logpi, const float *d_advantage,
                        const float *d_v, const float *d_v_target, const float *d_old_v, int baseline_advantage,
                        int surrogate_clip, double policy_clip_range, int enable_value_clip, double value_clip_range,
                        double value_loss_weight, double entropy_weight, float *d_losses, float *d_grad_logpi, float *d_grad_v,
                        void *stream);
int srlx_pendulum_step(int64_t n_envs, float *d_state, int32_t *d_step_in_episode, const float *d_action, int64_t episode_len,
                       uint64_t seed, int64_t *d_counter, float *d_obs, float *d_reward, uint8_t *d_done, void *stream);

/* ------------------------------------------------------------------------------------------------
 * PPO's actor-critic in libsrlx (round 6): the network of srl/algorithms/ppo/ppo.py:55-99 with the reference's default blocks
 * (config.py:47: hidden (64, 64), value (64,), policy (64,); Normal head: loc + log_scale layers) -- forward, loss, backward, clip and
 * Adam -- so that an iteration is ~50 launches instead of ~1700 framework kernels.  Parameters: ONE float32 vector in the order of
 * `ActorCritic.parameters()` (weights [out][in]): w1 [64][obs], b1, w2 [64][64], b2, wv [64][64], bv, wvo [1][64], bvo, wp [64][64], bp,
 * wloc [A][64], bloc, wls [A][64], bls; obs_dim <= 8, action_dim <= 4.  float32, fmaf accumulation in ascending input order.
 *   srlx_ppo_net_param_count    : length of that vector (-1: geometry not covered).
 *   srlx_ppo_net_forward        : v f32 [n], loc / log_scale f32 [n][A] of obs f32 [n][obs_dim] (evaluation, tests, environments
 *       stepped by the host side).
 *   srlx_ppo_net_rollout        : ppo.py:316-339 (policy) + the environment + :389-404 (GAE) for `horizon` steps of `n_envs`
 *       (a multiple of 16) Pendulum-shaped environments in ONE launch: the arithmetic of srlx_ppo_normal_act (key: act_seed,
 *       *d_act_counter + t, 2 (env x A + dim)), srlx_pendulum_step (env_seed, *d_env_counter + t) and srlx_gae_scan; both counters
 *       advance by `horizon`.  env_obs f32 [E][3] = the observation it starts from and (afterwards) ends at; b_obs f32 [T+1][E][3],
 *       b_act / b_logp f32 [T][E][A], b_val / b_rew / b_adv f32 [T][E], b_done u8 [T][E], last_v f32 [E] = V(s_T),
 *       episode_return f32 [E] (running), finished f32 [2] += (sum of finished episodes' returns, their count).
 *   srlx_ppo_net_minibatch      : one minibatch of compute_train_loss (:102-169) + backward: rows i64 [minibatch] index the flattened
 *       [T x E] buffers (b_val = the rollout's values = old_v); partials f32 [srlx_ppo_net_partials_floats]: scratch; grad f32
 *       [param_count] = d loss / d parameters (sums in a fixed order: deterministic); losses f32 [3] or NULL.
 *   srlx_ppo_net_adam           : the gradient (read only) scaled by grad_scale (1 / world size behind a data-parallel all-reduce); global-norm clip
 *       (max_grad_norm, 0 = off: torch.nn.utils.clip_grad_norm_, ppo.py:240-241); torch.optim.Adam step; d_step int64 [2]: [0] += 1 (steps
 *       taken), [1] = the launch's arrival counter (zero it once; it is zero again behind every call).
 * ------------------------------------------------------------------------------------------------ */
int srlx_ppo_net_param_count(int obs_dim, int action_dim);
int srlx_ppo_net_partials_floats(int obs_dim, int action_dim);
int srlx_ppo_net_rollout_max_horizon(int action_dim); /* longest horizon srlx_ppo_net_rollout takes (its per-step records live in the workgroup's LDS) */
int srlx_ppo_net_forward(int64_t n, int obs_dim, int action_dim, const float *d_params, const float *d_obs, float *d_v, float *d_loc,
                         float *d_log_scale, void *stream);
int srlx_ppo_net_rollout(int64_t n_envs, int64_t horizon, int action_dim, const float *d_params, float *d_env_state,
                         int32_t *d_step_in_episode, float *d_env_obs, int64_t episode_len, uint64_t env_seed, int64_t *d_env_counter,
                         uint64_t act_seed, int64_t *d_act_counter, double log_scale_min, double log_scale_max, double discount,
                         double gae_lambda, float *d_b_obs, float *d_b_act, float *d_b_logp, float *d_b_val, float *d_b_rew,
                         uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return, float *d_finished, void *stream);
int srlx_ppo_net_minibatch(int64_t minibatch, const int64_t *d_rows, int obs_dim, int action_dim, const float *d_params,
                           const float *d_b_obs, const float *d_b_act, const float *d_b_logp, const float *d_b_adv,
                           const float *d_b_v_target, const float *d_b_val, double log_scale_min, double log_scale_max,
                           int baseline_advantage, int surrogate_clip, double policy_clip_range, int enable_value_clip,
                           double value_clip_range, double value_loss_weight, double entropy_weight, float *d_partials, float *d_grad,
                           float *d_losses, void *stream);
int srlx_ppo_net_adam(int obs_dim, int action_dim, float *d_params, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq,
                      int64_t *d_step, double lr, double beta1, double beta2, double eps, double max_grad_norm, double grad_scale,
                      void *stream);

/* ------------------------------------------------------------------------------------------------
 * Discrete-action PPO on the vectorised path: a categorical policy head and a self-resetting CartPole (BASELINE config 1's
 * environment).  Parity UNPINNED like the whole PPO row (the reference's PPO needs TensorFlow); restated from the cited lines
 * and checked against tests/ppo_cat_reference.py + torch autograd.  The exact arithmetic: csrc/srlx_ppo_math.h.
 *   srlx_ppo_categorical_act     : ppo.py:316-324 + srl/rl/tf/distributions/categorical_dist_block.py (CategoricalDist.sample /
 *       mode / log_prob): logits f32 [rows][n_actions] -> action i32 [rows] by inverse CDF over the float32 softmax with ONE keyed
 *       uniform per row (seed, *d_counter, row), *d_counter += 1; logprob f32 [rows] of the taken action floored at log(1e-6)
 *       (ppo.py:324).  deterministic != 0: the first maximum (:318-319), no draw, d_counter may be NULL.
 *   srlx_cartpole_autoreset_step : envs/cartpole.py:step (the reference reaches CartPole-v1 through srl/base/env/gym_user_wrapper.py)
 *       for E lanes, float64 state [E][4], steps / episodes i32 [E] as srlx_cartpole_step keeps them; a lane whose step ends its
 *       episode (termination, or steps >= max_steps) returns reward 1, done 1 and starts its next episode in the same call: d_obs
 *       f32 [E][4] is then that episode's first observation (reset key: (seed ^ 0xCA27901E, lane << 32 | episode, k), as
 *       srlx_cartpole_step).  A finished episode is never bootstrapped, truncation included (ppo.py:396-397).
 * The fused network with this head (srlx_ppo_net.hip): the trunk of srlx_ppo_net_*, in -> 64 -> 64 -> {64 -> V, 64 -> n logits}
 * (ppo.py:55-99 with a CategoricalDistBlock); parameters in `ActorCritic.parameters()` order: w1, b1, w2, b2, wv, bv, wvo, bvo, wp, bp,
 * wlogit [n][64], blogit [n]; obs_dim 1..8, n_actions 2..8 (the heads table's eight policy slots per row).
 *   srlx_ppo_cat_param_count / _partials_floats / _rollout_max_horizon : as their srlx_ppo_net_ counterparts (-1: not covered).
 *   srlx_ppo_cat_forward   : v f32 [n], logits f32 [n][n_actions] of obs f32 [n][obs_dim].
 *   srlx_ppo_cat_rollout   : ppo.py:316-324 (policy) + CartPole + :389-404 (GAE) for `horizon` steps of `n_envs` (a multiple of 16)
 *       environments in ONE launch: the arithmetic of srlx_ppo_categorical_act (key: act_seed, *d_act_counter + t, env),
 *       srlx_cartpole_autoreset_step and srlx_gae_scan run step by step; *d_act_counter += horizon.  env_obs f32 [E][4]; b_obs f32
 *       [T+1][E][4], b_act i32 [T][E], b_logp / b_val / b_rew / b_adv f32 [T][E], b_done u8 [T][E], last_v, episode_return, finished as
 *       srlx_ppo_net_rollout.
 *   srlx_ppo_cat_minibatch : compute_train_loss (:102-169) with new_logpi = log_softmax(logits)[action] + backward, as
 *       srlx_ppo_net_minibatch (entropy term of the taken action only, :166; d loss / d logit_k = g_lp ((k == a) - p_k)).
 *   srlx_ppo_cat_adam      : srlx_ppo_net_adam over this head's parameter vector (the same reduction and clip + Adam kernels).
 * ------------------------------------------------------------------------------------------------ */
int srlx_ppo_categorical_act(int64_t rows, int n_actions, const float *d_logits, uint64_t seed, int64_t *d_counter, int deterministic,
                             int32_t *d_action, float *d_logprob, void *stream);
int srlx_cartpole_autoreset_step(int64_t n_envs, double *d_state, int32_t *d_steps, int32_t *d_episodes, const int32_t *d_actions,
                                 int64_t max_steps, uint64_t seed, float *d_obs, float *d_reward, uint8_t *d_done, void *stream);
int srlx_ppo_cat_param_count(int obs_dim, int n_actions);
int srlx_ppo_cat_partials_floats(int obs_dim, int n_actions);
int srlx_ppo_cat_rollout_max_horizon(int n_actions);
int srlx_ppo_cat_forward(int64_t n, int obs_dim, int n_actions, const float *d_params, const float *d_obs, float *d_v, float *d_logits,
                         void *stream);
int srlx_ppo_cat_rollout(int64_t n_envs, int64_t horizon, int n_actions, const float *d_params, double *d_env_state, int32_t *d_steps,
                         int32_t *d_episodes, float *d_env_obs, int64_t max_steps, uint64_t env_seed, uint64_t act_seed,
                         int64_t *d_act_counter, double discount, double gae_lambda, float *d_b_obs, int32_t *d_b_act, float *d_b_logp,
                         float *d_b_val, float *d_b_rew, uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return,
                         float *d_finished, void *stream);
int srlx_ppo_cat_minibatch(int64_t minibatch, const int64_t *d_rows, int obs_dim, int n_actions, const float *d_params,
                           const float *d_b_obs, const int32_t *d_b_act, const float *d_b_logp, const float *d_b_adv,
                           const float *d_b_v_target, const float *d_b_val, int baseline_advantage, int surrogate_clip,
                           double policy_clip_range, int enable_value_clip, double value_clip_range, double value_loss_weight,
                           double entropy_weight, float *d_partials, float *d_grad, float *d_losses, void *stream);
int srlx_ppo_cat_adam(int obs_dim, int n_actions, float *d_params, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq, int64_t *d_step,
                      double lr, double beta1, double beta2, double eps, double max_grad_norm, double grad_scale, void *stream);

/* ------------------------------------------------------------------------------------------------
 * What a ppo.Config asks of the engine beyond the network (srl/algorithms/ppo/config.py:43-110): a learning-rate schedule, the
 * batch baselines of the advantage, reward / state clips and the action rescale.  All of it stays on the device: the update's
 * HIP graph is captured once and follows the schedule by itself.
 *   srlx_lr_schedule_t     : LRSchedulerConfig (srl/rl/schedulers/lr_scheduler.py:5-140) as plain data: kind, decay_steps,
 *       decay_rate, min_lr, up to SRLX_LR_MAX_BOUNDARIES piecewise boundaries with one more value than boundaries.
 *   srlx_lr_factor         : HOST arithmetic (no device needed): *out = the multiplier of `lr` at optimiser step `step` (0-based),
 *       LRSchedulerConfig.factor restated -- step: rate ** (step // decay_steps); exp: rate ** (step / decay_steps); cosine:
 *       (1 - a) / 2 (1 + cos(pi min(step, decay_steps) / decay_steps)) + a, a = min_lr / lr; piecewise: values[#{b: step > b}] / lr;
 *       warmup_steps is not part of `factor`.  float64.  SRLX_ERR_INVALID: unknown kind, decay_steps <= 0, too many boundaries, lr <= 0.
 *   srlx_ppo_net_adam_sched / srlx_ppo_cat_adam_sched : srlx_ppo_*_adam with the rate lr * factor(schedule, d_step[0], lr), evaluated
 *       inside the launch from the step count it reads from device memory (the kernel's integer power for "step" is within a few ulp
 *       of pow()): optimiser step k (0-based) runs at factor(k), as `optimizer.step(); lr_scheduler.step()` under a LambdaLR does.
 *       srlx_ppo_*_adam is the constant schedule of the same kernel (its instantiation without the schedule's code and arguments; a constant
 *       srlx_lr_schedule_t launches that one too): bit for bit.
 *   srlx_ppo_adv_baseline  : baseline_type "ave" / "std" / "normal" (ppo.py:222-233) over ONE minibatch: mean and POPULATION standard
 *       deviation of b_adv[rows[0 .. minibatch)] (two passes, float64 sums in a fixed order: deterministic), then d_out[rows[i]] =
 *       adv - mean (SRLX_PPO_BASELINE_AVE), adv / (std + 1e-8) (_STD), (adv - mean) / (std + 1e-8) (_NORMAL) as float32; d_out is a second
 *       [T x E] buffer, entries outside `rows` are not touched.  Up to 16 workgroups that each compute the whole statistics (no grid-wide exchange) and
 *       transform their own slice.  The minibatch launch then
 *       takes d_out as its d_b_adv, while d_b_v_target keeps reading the untouched advantages.
 *   srlx_ppo_env_opts_t    : the rollout's options; NULL = all off.  reward clip: the clipped reward goes to b_rew and the GAE
 *       records, episode_return / finished keep the raw reward (ppo.py:374-379 clips what the trainer sees); state clip: every
 *       observation row the network reads and every row of b_obs, the first included (env_obs is written back clipped: the clip is
 *       idempotent), never the environment's state; action rescale (Normal head only): the environment's step receives
 *       action * action_scale + action_offset (a multiply, then an add), b_act / b_logp keep the policy's action (ppo.py:336).
 *   srlx_ppo_net_rollout_ex / srlx_ppo_cat_rollout_ex : srlx_ppo_*_rollout with these options; the plain entry points are the
 *       all-off case of the same kernel (instantiated without the options' code, which an all-off struct launches too): bit for bit.
 * ------------------------------------------------------------------------------------------------ */
#define SRLX_LR_CONSTANT 0
#define SRLX_LR_STEP 1
#define SRLX_LR_EXP 2
#define SRLX_LR_COSINE 3
#define SRLX_LR_PIECEWISE 4
#define SRLX_LR_MAX_BOUNDARIES 8
typedef struct {
    int32_t kind;         /* SRLX_LR_* */
    int32_t n_boundaries; /* piecewise: 0 .. SRLX_LR_MAX_BOUNDARIES */
    int64_t decay_steps;
    double decay_rate;
    double min_lr;
    int64_t boundaries[SRLX_LR_MAX_BOUNDARIES];
    double values[SRLX_LR_MAX_BOUNDARIES + 1]; /* learning rates (not factors), n_boundaries + 1 of them */
} srlx_lr_schedule_t;

#define SRLX_PPO_BASELINE_AVE 1
#define SRLX_PPO_BASELINE_STD 2
#define SRLX_PPO_BASELINE_NORMAL 3

typedef struct {
    int32_t reward_clip; /* != 0: on */
    float reward_lo, reward_hi;
    int32_t state_clip;
    float state_lo, state_hi;
    float action_scale, action_offset; /* (1, 0): off */
} srlx_ppo_env_opts_t;

int srlx_lr_factor(const srlx_lr_schedule_t *schedule, int64_t step, double lr, double *out);
int srlx_ppo_net_adam_sched(int obs_dim, int action_dim, float *d_params, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq,
                            int64_t *d_step, double lr, const srlx_lr_schedule_t *schedule, double beta1, double beta2, double eps,
                            double max_grad_norm, double grad_scale, void *stream);
int srlx_ppo_cat_adam_sched(int obs_dim, int n_actions, float *d_params, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq,
                            int64_t *d_step, double lr, const srlx_lr_schedule_t *schedule, double beta1, double beta2, double eps,
                            double max_grad_norm, double grad_scale, void *stream);
int srlx_ppo_adv_baseline(int64_t minibatch, const int64_t *d_rows, const float *d_b_adv, int mode, float *d_out, void *stream);
int srlx_ppo_net_rollout_ex(int64_t n_envs, int64_t horizon, int action_dim, const float *d_params, float *d_env_state,
                            int32_t *d_step_in_episode, float *d_env_obs, int64_t episode_len, uint64_t env_seed, int64_t *d_env_counter,
                            uint64_t act_seed, int64_t *d_act_counter, double log_scale_min, double log_scale_max, double discount,
                            double gae_lambda, float *d_b_obs, float *d_b_act, float *d_b_logp, float *d_b_val, float *d_b_rew,
                            uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return, float *d_finished,
                            const srlx_ppo_env_opts_t *opts, void *stream);
int srlx_ppo_cat_rollout_ex(int64_t n_envs, int64_t horizon, int n_actions, const float *d_params, double *d_env_state, int32_t *d_steps,
                            int32_t *d_episodes, float *d_env_obs, int64_t max_steps, uint64_t env_seed, uint64_t act_seed,
                            int64_t *d_act_counter, double discount, double gae_lambda, float *d_b_obs, int32_t *d_b_act, float *d_b_logp,
                            float *d_b_val, float *d_b_rew, uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return,
                            float *d_finished, const srlx_ppo_env_opts_t *opts, void *stream);

/* ------------------------------------------------------------------------------------------------
 * PPO's adaptive-KL surrogate (surrogate_type "kl": srl/algorithms/ppo/ppo.py:138-146, :279-287; srl/rl/tf/functions.py:86-103).
 * Per element the policy term is ratio * adv - beta * kl with no ratio clip; kl is KL(old || new) against the distribution the
 * policy acted with.  Categorical: sum_k q_k log(q_k / p_k) with both sides clipped to [1e-10, 1] (the clip passes the gradient
 * inside its bounds, bounds included); Normal, per dimension: (ls2 - ls1) + (exp(2 ls1) + (m1 - m2)^2) / 2 exp(-2 ls2) - 1/2 with
 * ls2 the new log-scale clamped to [log_scale_min, log_scale_max] (the gradient reaches the raw log-scale inside that range only)
 * and ls1 the old one as clamped at acting time.  The exact float32 arithmetic: csrc/srlx_ppo_math.h; tests/ppo_kl_reference.py.
 * beta is ONE float32 in device memory (d_kl_beta; the reference starts it at 0.5).  The launch that forms a minibatch's losses
 * adapts it: kl_mean = mean of kl over all elements; kl_mean < target / 1.5: beta /= 2; else kl_mean > target * 1.5 and beta < 10:
 * beta *= 2 (compared in double against thresholds formed on the host in double; halving and doubling are exact: the halving stops
 * at the smallest normal float32, 1.18e-38, where a float32 would start to lose bits and then reach 0 for good).  No host read, no
 * added launch: the next minibatch reads the adapted value through stream order, and a captured graph follows it.
 * losses f32 [5] = policy, value, entropy (as the other entry points report them), kl_mean, beta as adapted.
 *   srlx_ppo_normal_act_dist / srlx_ppo_categorical_act_dist : srlx_ppo_normal_act / srlx_ppo_categorical_act (same draws, same bits)
 *       which also write the acting distribution: old_loc / old_log_scale f32 [n] (the log-scale clamped), probs f32 [rows][n_actions]
 *       (expf of the float32 log-softmax: the values the sampler sums).
 *   srlx_ppo_loss_normal_kl      : srlx_ppo_loss_normal under "kl": old_loc / old_log_scale f32 [B][action_dim] beside old_logpi.
 *   srlx_ppo_loss_categorical_kl : logits f32 [B][n_actions] (2 <= n_actions <= 8), action i32 [B], old_logpi f32 [B], old_probs f32
 *       [B][n_actions]; returns d loss / d logits f32 [B][n_actions] and d loss / d v.  Both loss kernels run as one workgroup that
 *       sums in a fixed order: deterministic.
 *   srlx_ppo_net_rollout_kl / srlx_ppo_cat_rollout_kl : srlx_ppo_*_rollout_ex (opts may be NULL) which also record the acting
 *       distribution of every step: b_loc / b_log_scale f32 [T][E][A], b_probs f32 [T][E][n_actions]; every other output bit for bit.
 *   srlx_ppo_net_minibatch_kl / srlx_ppo_cat_minibatch_kl : srlx_ppo_*_minibatch under "kl": the old distribution is gathered through
 *       `rows` like b_logp; partials f32 [srlx_ppo_*_kl_partials_floats] (a fourth loss sum per workgroup); the gradient reduction
 *       launch adapts *d_kl_beta and writes losses [5] (NULL: beta is adapted all the same).
 * ------------------------------------------------------------------------------------------------ */
int srlx_ppo_normal_act_dist(int64_t n, const float *d_loc, const float *d_log_scale, double log_scale_min, double log_scale_max,
                             uint64_t seed, int64_t *d_counter, int deterministic, float *d_action, float *d_logprob, float *d_old_loc,
                             float *d_old_log_scale, void *stream);
int srlx_ppo_categorical_act_dist(int64_t rows, int n_actions, const float *d_logits, uint64_t seed, int64_t *d_counter,
                                  int deterministic, int32_t *d_action, float *d_logprob, float *d_probs, void *stream);
int srlx_ppo_loss_normal_kl(int64_t batch, int action_dim, const float *d_loc, const float *d_log_scale, double log_scale_min,
                            double log_scale_max, const float *d_action, const float *d_old_logpi, const float *d_old_loc,
                            const float *d_old_log_scale, const float *d_advantage, const float *d_v, const float *d_v_target,
                            const float *d_old_v, int baseline_advantage, int enable_value_clip, double value_clip_range,
                            double value_loss_weight, double entropy_weight, double adaptive_kl_target, float *d_kl_beta,
                            float *d_losses, float *d_grad_loc, float *d_grad_log_scale, float *d_grad_v, void *stream);
int srlx_ppo_loss_categorical_kl(int64_t batch, int n_actions, const float *d_logits, const int32_t *d_action, const float *d_old_logpi,
                                 const float *d_old_probs, const float *d_advantage, const float *d_v, const float *d_v_target,
                                 const float *d_old_v, int baseline_advantage, int enable_value_clip, double value_clip_range,
                                 double value_loss_weight, double entropy_weight, double adaptive_kl_target, float *d_kl_beta,
                                 float *d_losses, float *d_grad_logits, float *d_grad_v, void *stream);
int srlx_ppo_net_kl_partials_floats(int obs_dim, int action_dim);
int srlx_ppo_cat_kl_partials_floats(int obs_dim, int n_actions);
int srlx_ppo_net_rollout_kl(int64_t n_envs, int64_t horizon, int action_dim, const float *d_params, float *d_env_state,
                            int32_t *d_step_in_episode, float *d_env_obs, int64_t episode_len, uint64_t env_seed, int64_t *d_env_counter,
                            uint64_t act_seed, int64_t *d_act_counter, double log_scale_min, double log_scale_max, double discount,
                            double gae_lambda, float *d_b_obs, float *d_b_act, float *d_b_logp, float *d_b_val, float *d_b_rew,
                            uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return, float *d_finished,
                            float *d_b_loc, float *d_b_log_scale, const srlx_ppo_env_opts_t *opts, void *stream);
int srlx_ppo_cat_rollout_kl(int64_t n_envs, int64_t horizon, int n_actions, const float *d_params, double *d_env_state, int32_t *d_steps,
                            int32_t *d_episodes, float *d_env_obs, int64_t max_steps, uint64_t env_seed, uint64_t act_seed,
                            int64_t *d_act_counter, double discount, double gae_lambda, float *d_b_obs, int32_t *d_b_act, float *d_b_logp,
                            float *d_b_val, float *d_b_rew, uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return,
                            float *d_finished, float *d_b_probs, const srlx_ppo_env_opts_t *opts, void *stream);
int srlx_ppo_net_minibatch_kl(int64_t minibatch, const int64_t *d_rows, int obs_dim, int action_dim, const float *d_params,
                              const float *d_b_obs, const float *d_b_act, const float *d_b_logp, const float *d_b_adv,
                              const float *d_b_v_target, const float *d_b_val, const float *d_b_loc, const float *d_b_log_scale,
                              double log_scale_min, double log_scale_max, int baseline_advantage, int enable_value_clip,
                              double value_clip_range, double value_loss_weight, double entropy_weight, double adaptive_kl_target,
                              float *d_kl_beta, float *d_partials, float *d_grad, float *d_losses, void *stream);
int srlx_ppo_cat_minibatch_kl(int64_t minibatch, const int64_t *d_rows, int obs_dim, int n_actions, const float *d_params,
                              const float *d_b_obs, const int32_t *d_b_act, const float *d_b_logp, const float *d_b_adv,
                              const float *d_b_v_target, const float *d_b_val, const float *d_b_probs, int baseline_advantage,
                              int enable_value_clip, double value_clip_range, double value_loss_weight, double entropy_weight,
                              double adaptive_kl_target, float *d_kl_beta, float *d_partials, float *d_grad, float *d_losses,
                              void *stream);

/* ------------------------------------------------------------------------------------------------
 * Never-Give-Up intrinsic reward + Agent57_light priorities
 *
 * srlx_ngu_t: one bounded episodic memory per environment, [E][emb_dim][capacity] float32 in HBM
 * (replaces `collections.deque(maxlen=episodic_memory_capacity)` of numpy vectors,
 * srl/algorithms/agent57_light/agent57_light.py:310-311).
 *   srlx_ngu_episodic_reward : agent57_light.py:473-513 for every environment at once: distances of the
 *       new embedding to every stored one, the k nearest, pseudo-count reward, then append (the oldest
 *       entry is dropped when full).  d_emb f32 [E][emb_dim]; d_reset u8 [E] (NULL = none) empties an
 *       environment's memory BEFORE the query (`on_reset`, :310-311); d_active u8 [E] (NULL = all) skips
 *       environments entirely; d_reward f32 [E].  1 <= k <= 16.
 *   srlx_ngu_reset           : empty every memory.
 *   srlx_ngu_counts          : device pointer of the int64 [E] append counters (live = min(count, capacity)).
 *   srlx_ngu_lifelong_reward : agent57_light.py:515-529, min(max(1 + mean((t-p)^2), 1), L) per row of
 *       d_target/d_train f32 [n][dim].
 *   srlx_agent57_priority    : srl/algorithms/agent57_light/model_torch.py:442,367-373:
 *       td = target - q[action]; priorities = |td_ext + beta[actor] * td_int| (d_target_int NULL: |td_ext|).
 *       d_td_ext / d_td_int (nullable) receive the signed TD errors.  d_q_ext == d_q_int == NULL: d_target_* already
 *       hold TD errors (Agent57's per-sequence means, srl/algorithms/agent57/model_torch.py:388-391).
 * ------------------------------------------------------------------------------------------------ */
typedef struct srlx_ngu srlx_ngu_t;
int srlx_ngu_create(srlx_ngu_t **out, int64_t n_envs, int emb_dim, int64_t capacity, int k, double epsilon,
                    double cluster_distance, double pseudo_counts, int device);
int srlx_ngu_destroy(srlx_ngu_t *h);
int srlx_ngu_reset(srlx_ngu_t *h, void *stream);
int srlx_ngu_counts(srlx_ngu_t *h, int64_t **d_counts);
int srlx_ngu_episodic_reward(srlx_ngu_t *h, const float *d_emb, const uint8_t *d_reset, const uint8_t *d_active,
                             float *d_reward, void *stream);
int srlx_ngu_lifelong_reward(int64_t n, int dim, const float *d_target, const float *d_train, double lifelong_max,
                             float *d_reward, void *stream);
/* Agent57 (LSTM, sequence replay) learner arithmetic after the forwards, srl/algorithms/agent57/agent57.py:301-379
 * (calc_target_q: double-DQN gains with the actor's gamma, greedy-policy retrace coefficients, backward target
 * recursion) + model_torch.py:469-492 (selected Q, HuberLoss(target*w, q*w) over [seq][batch], mean TD error):
 *   q / q_target f32 [B][S+1][A] (online / target network over the S+1 in-sequence states), actions i32 [B][S],
 *   rewards / dones f32 [B][S] (dones = 0 after a terminal step), invalid_next u8 [B][S][A] or NULL,
 *   discounts / weights f32 [B];  out: target f32 [S][B], loss f32 [1], grad_q f32 [B][S+1][A] = d loss / d q,
 *   td_mean f32 [B] = mean_t(q[a_t] - target_t);  scratch >= 2*B*S floats. */
int srlx_agent57_seq_td(int64_t batch, int seq_len, int n_actions, const float *d_q, const float *d_q_target,
                        const int32_t *d_actions, const float *d_rewards, const float *d_dones, const uint8_t *d_invalid_next,
                        const float *d_discounts, const float *d_weights, double retrace_h, int enable_double_dqn,
                        int enable_rescale, float *d_target, float *d_loss, float *d_grad_q, float *d_td_mean, float *d_scratch,
                        void *stream);
/* Sliding-window UCB meta-controller of Agent57(_light), one per device-resident environment (replaces the per-actor-process
 * controller of srl/algorithms/agent57_light/agent57_light.py:317-353).  State (caller-allocated device arrays): ring_arm int32
 * [E][window], ring_reward f32 [E][window], head int32 [E] (0), n_recent int32 [E] (0), count int32 [E][N] (ALL ONES), sum f64 [E][N]
 * (0), arm int32 [E] (-1).  Environments with done[e] != 0 (NULL = all) book `episode_reward[e]` for their current arm and choose the
 * next: arms 0..N-1 in order first, then with u[e][0] < epsilon the arm floor(u[e][1] * N), else the UCB maximiser with ties broken by
 * u[e][2].  u: f64 [E][3] uniforms. */
int srlx_agent57_ucb_step(int64_t n_envs, int n_arms, int window, int32_t *d_ring_arm, float *d_ring_reward, int32_t *d_head, int32_t *d_n_recent,
                          int32_t *d_count, double *d_sum, int32_t *d_arm, const uint8_t *d_done, const float *d_episode_reward, const double *d_u,
                          double epsilon, double beta, void *stream);
int srlx_agent57_priority(int64_t batch, int n_actions, const float *d_target_ext, const float *d_q_ext,
                          const float *d_target_int, const float *d_q_int, const int32_t *d_actions,
                          const int32_t *d_actor_idx, const float *d_beta_list, float *d_td_ext, float *d_td_int,
                          float *d_priorities, void *stream);

/* Frame-offset tables: byte offsets of uint8 frames inside the ring (-1 = all-zero history), consumed by
 * srlx_qnet_forward_u8 so that the first convolution reads the ring directly.
 *   srlx_store_obs_base            : device pointer of the frame ring (+ bytes per frame)
 *   srlx_store_frame_table_current : int64 [E][window] for the policy step at the current position
 *   srlx_store_gather_items        : like srlx_store_gather_nstep, but instead of float32 pixels it emits
 *                                    int64 [B][k_count][window] offsets of states k_begin..k_begin+k_count-1
 *   srlx_store_gather_obs          : float32 [B][k_count][window][obs_elems] pixels of a state range of the
 *                                    items located by the preceding gather_items call (same stream)
 *   srlx_store_gather_train        : the hand-written training pass's gather in ONE launch: n-step scalars as in
 *                                    gather_nstep, int64 [B][n+1][window] offsets of s_0..s_n (online network) and,
 *                                    if not NULL, int64 [B][n][window] offsets of s_1..s_n (target network) */
int srlx_store_obs_base(srlx_store_t *h, void **d_base, int64_t *frame_bytes);
/* sampled tree indices -> (environment, ring slot of the item's first transition, ring slot of the transition before it or -1 when the
 * item starts an episode): lets an engine gather per-step fields it keeps in its own [ring slot][env] arrays (Agent57's UVFA inputs) */
int srlx_store_locate(srlx_store_t *h, int64_t batch, const int64_t *d_tree_idx, int64_t *d_env, int64_t *d_slot, int64_t *d_prev_slot, void *stream);
int srlx_store_frame_table_current(srlx_store_t *h, int64_t *d_out, void *stream);
int srlx_store_gather_items(srlx_store_t *h, int64_t batch, const int64_t *d_tree_idx, int k_begin, int k_count, int64_t *d_frame_off,
                            int32_t *d_actions, float *d_rewards, float *d_terminated, void *stream);
int srlx_store_gather_train(srlx_store_t *h, int64_t batch, const int64_t *d_tree_idx, int64_t *d_frame_off_all, int64_t *d_frame_off_next,
                            int32_t *d_actions, float *d_rewards, float *d_terminated, void *stream);
/* srlx_per_sample_keyed + srlx_store_gather_train as ONE launch: the learner's draw (proportional_memory.py:131-169), then the location, n-step scalars
 * (rainbow.py:190-194 with the terminal padding of :354-372) and frame-offset tables of the drawn items of `store`, whose leaf j is this tree's slot j.  Up to 64
 * items; device pointers only; outputs as the two calls'. */
int srlx_per_sample_gather_train(srlx_per_t *h, srlx_store_t *store, int64_t batch_size, const int64_t *d_step, uint64_t seed, int64_t *d_counter, int64_t n_uniforms,
                                 int64_t *d_out_idx, float *d_out_w32, int64_t *d_out_used, int64_t *d_frame_off_all, int64_t *d_frame_off_next, int32_t *d_actions,
                                 float *d_rewards, float *d_terminated, void *stream);
/* Actor-side initial priorities (rainbow.py:389-398: a distributed worker hands `abs(calc_target_q([batch]) - q[action])` to memory.add): for the E items the LAST
 * commit completed -- PER slots first_slot .. first_slot + E - 1 (mod per_capacity), lane e's item in slot first_slot + e -- the n-step / retrace TD of
 * rainbow.py:226-287 on CACHED Q rows: d_q_hist f32 [n_step + 1][E][n_actions] is a ring over the acting passes, row (base_slot + k) mod (n_step + 1) holds
 * Q(s_k) of the item's k-th state (the online rows stand in for the target network's).  d_est[e] = |target - Q(s_0, a_0)|, or -1 when an episode ends inside
 * the item's window (its last states were never evaluated by an actor: the caller uses max_priority), or -2 when d_item_mask[e] == 0 (no item).  Feeds
 * srlx_per_add(..., SRLX_PRIO_EST_F32). */
int srlx_store_actor_td(srlx_store_t *h, int64_t first_slot, int64_t per_capacity, const float *d_q_hist, int base_slot, const uint8_t *d_item_mask, double discount,
                        double retrace_h, int enable_double_dqn, int enable_rescale, float *d_est, void *stream);
int srlx_store_gather_obs(srlx_store_t *h, int64_t batch, int k_begin, int k_count, float *d_obs, void *stream);

/* ------------------------------------------------------------------------------------
 * Q-network inference on the matrix cores: float32 in, float32 out, float32 accumulation everywhere.
 * Arithmetic: v_mfma_f32_32x32x2_f32 (products of two float32 operands), except where a float32 product is evaluated
 * on the 16x faster 16-bit pipe as a sum of EXACT partial products, each exact in the float32 accumulator.  FORWARD passes of the 84x84x4 geometry
 * (round 6): two float16 parts per operand, x = hi + lo / 2048 with hi = f16(x), lo = f16((x - hi) * 2048) -- 22 significand bits, lo a normal float16
 * wherever hi is -- on v_mfma_f32_32x32x16_f16: conv1 (the uint8 pixel is one float16, the filter two parts: two products), conv2 / conv3 and the first
 * dense layer (three of the four products, the cross terms in a 2^11-scaled accumulator; the dropped one is below 2^-24 |a b|).  BACKWARD GEMMs: three bf16
 * parts per operand on v_mfma_f32_32x32x16_bf16, six of the nine products (gradients live below float16's normal range).  Q-values agree with the
 * all-float32 pipe to float32 round-off (3e-7 of max |Q| against float64 for either; the tolerance promised against the reference is 1e-5).  The float16
 * split holds activations up to 65 504: srlx_qnet_range_flags reports a pass that met a larger one.
 *
 * Environment switches: A/B arms of the numeric paths, each on when its variable starts with '1'.  Read once per process, when a Q-network first needs one.
 *   SRLX_CONV_BF16X3    the fused convolution kernel's products on three bf16 parts (six of the nine products; rounds 3-5), whose range is
 *                       float32's, instead of two float16 parts
 *   SRLX_CONV1_F32      every convolution on the float32 matrix pipe
 *   SRLX_CONV23_F32     conv2 / conv3 on the float32 matrix pipe; conv1 then runs on three bf16 parts (implies SRLX_CONV_BF16X3)
 *   SRLX_FC1_F32        the first dense layer on the float32 matrix pipe
 *   SRLX_NO_FUSED_CONV  the three-launch convolution path instead of the fused kernel (the Python engines read it too: they must agree)
 *   SRLX_NO_CONV_PLANES the fused kernel writes float32 activations, and a split pass makes the first dense layer's operand planes
 *
 * Replaces the no-grad forwards of the reference's torch modules -- DQNImageBlock
 * (srl/rl/torch_/blocks/dqn_image_block.py:10-67) + DuelingNetworkBlock
 * (srl/rl/torch_/blocks/dueling_network.py:8-59) behind pred_q / pred_target_q
 * (srl/algorithms/rainbow/model_torch.py:55-67) -- for the actor's policy step and the
 * learner's online/target evaluation of s_1..s_n.
 *   dueling_type: 0 "average", 1 "max", 2 "" (naive), 3 no dueling -- DQN's plain head q = W2 relu(h) + b2
 *   (srl/algorithms/dqn/model_torch.py:17-29) over ALL 2*hidden units of the first dense layer (a DQN layer of width W is
 *   a handle with hidden = W / 2).  With 3 the a2 entries of srlx_qnet_bind carry W2 [A][2*hidden] and b2 [A], and the
 *   v2 entries are not read (bind any valid pointer; their gradient buffers are not written, their packed ranges are empty).
 *   The published sets, the fused policy, srlx_qnet_backward_u8 / _td_u8 and the fused Adam serve it; srlx_qnet_bind_uvfa,
 *   srlx_qnet_bind_noisy and srlx_qnet_set_head_mode(h, 1, ...) refuse it.
 *   srlx_qnet_bind: 12 device pointers to float32 parameters that the kernels read IN PLACE (no copy;
 *   they must stay valid and may be updated between calls):
 *     conv1.weight [F][window][8][8]      conv1.bias
 *     conv2.weight [2F][4][4][F]  (torch channels_last memory of a [2F][F][4][4] weight)   conv2.bias
 *     conv3.weight [2F][3][3][2F] (channels_last)                                         conv3.bias
 *     fc1.weight [2*hidden][flat]: rows 0..hidden-1 = V head, the rest = A head; columns in NHWC
 *                flatten order (pixel-major, channel-minor)                                fc1.bias
 *     v2.weight [1][hidden]  v2.bias   a2.weight [A][hidden]  a2.bias
 *   srlx_qnet_forward_u8 : input = uint8 frames + offset table [batch][window]
 *   srlx_qnet_forward_f32: input = float32 [batch][window][H][W] (channels first)
 *   output float32 [batch][n_actions]
 * ------------------------------------------------------------------------------------ */
typedef struct srlx_qnet srlx_qnet_t;
int srlx_qnet_create(srlx_qnet_t **out, int in_h, int in_w, int window, int filters, int hidden, int n_actions, int dueling_type, int64_t max_batch,
                     int device);
int srlx_qnet_destroy(srlx_qnet_t *h);
int srlx_qnet_bind(srlx_qnet_t *h, const float *const *d_params);
int srlx_qnet_forward_u8(srlx_qnet_t *h, int64_t batch, const uint8_t *d_frame_base, const int64_t *d_frame_off, float *d_q, void *stream);
/* Two handles' srlx_qnet_forward_u8 as THREE launches (the learner update's online pass over s_0..s_n and its target pass over s_1..s_n, which share nothing but the
 * ring): both convolution passes in one launch, both first dense layers in one, both heads in one -- each workgroup runs the code of its own pass, so both handles
 * are left exactly as their own srlx_qnet_forward_u8 leaves them (Q-values bit for bit, kept activations of a training handle, operand planes, partial sums, range
 * flag, packing state).  The envelope: both handles 84 x 84 x 4 with 32 filters on the float16-split convolution kernel, valid operand planes with
 * srlx_qnet_set_planes_small and 1..128 rows each, plain (not NoisyLinear) dueling heads of the same width with at most 8 actions, no UVFA columns, no fused policy,
 * no probe armed.  *applied = 1: done; *applied = 0: outside the envelope -- nothing was launched and no handle was touched, the caller runs the two passes itself. */
int srlx_qnet_forward_pair_u8(srlx_qnet_t *h_a, int64_t rows_a, const int64_t *d_frame_off_a, float *d_q_a, srlx_qnet_t *h_b, int64_t rows_b,
                              const int64_t *d_frame_off_b, float *d_q_b, const uint8_t *d_frame_base, int *applied, void *stream);
/* The batched Worker.policy step as one call (srl/algorithms/rainbow/rainbow.py:301-329 behind srl/base/rl/worker_run.py:316-322): srlx_qnet_forward_u8 whose head
 * kernel also selects the actions -- epsilon-greedy exactly as srlx_policy_epsilon_greedy would on the Q rows with the uniforms srlx_rng_uniform(seed, d_counter,
 * 2 * batch, u) would write (row e uses u[2 e], u[2 e + 1]).  *d_counter is READ only: advance it once per pass yourself (srlx_store_commit_step_ex's d_bump does).
 *   d_eps float32 [batch], d_invalid uint8 [batch][n_actions] or NULL, d_actions int32 [batch], d_q_copy float32 [batch][n_actions] or NULL (a second copy of Q) */
int srlx_qnet_forward_u8_policy(srlx_qnet_t *h, int64_t batch, const uint8_t *d_frame_base, const int64_t *d_frame_off, float *d_q, const float *d_eps, uint64_t seed,
                                const int64_t *d_counter, const uint8_t *d_invalid, int32_t *d_actions, float *d_q_copy, void *stream);
/* Weights handed from a learner to the actors that share its GPU without a copy on the lock-step's serial tail (the role of the parameter board the reference's
 * trainer publishes and its actors poll, srl/base/run/play_mp.py:289-303,151-165; there a pickled state_dict, here two device-resident parameter sets):
 *   srlx_qnet_actor_sets_enable   an actor handle gets two sets of everything a policy pass reads (packed convolution filters, the first dense layer as bf16
 *                                 operand planes, biases and head vectors)
 *   srlx_qnet_publish             (d_bump: an int64 device counter the launch advances by one, or NULL -- the update's step count, once every reader is done)
 *                                 packs h_src's convolution filters for its own next forwards (they then skip the packing launch until
 *                                 srlx_qnet_weights_changed) and, with h_actor, writes set `set` in the same launch; with_fc1 != 0 also splits the first dense
 *                                 layer's weight into the set's planes (the out-of-band publish: start-up, restore, a target sync)
 *   srlx_qnet_fuse_adam_fc1_planes  the fused Adam epilogue of srlx_qnet_fuse_adam_fc1 ALSO writes the updated weight as planes to d_planes_out (an actor set's,
 *                                 srlx_qnet_actor_set_planes); NULL switches it off
 *   srlx_qnet_actor_set_select    the next forwards of the actor handle read set 0 / 1 (-1: its bound parameters again)
 *   srlx_qnet_set_pack_sticky     a forward's packed filters stay valid until srlx_qnet_weights_changed (a target network: weights change at a sync only)
 *   srlx_qnet_weights_changed     the bound tensors were written by somebody else: packed filters and operand planes derived from them are stale */
int srlx_qnet_actor_sets_enable(srlx_qnet_t *h);
int srlx_qnet_actor_set_planes(srlx_qnet_t *h, int set, void **d_planes);
int srlx_qnet_actor_set_select(srlx_qnet_t *h, int set);
int srlx_qnet_publish(srlx_qnet_t *h_src, srlx_qnet_t *h_actor, int set, int with_fc1, int64_t *d_bump, void *stream);
/* The replay's priority write-back (rainbow/model_torch.py:113-114: memory.update(batch, priorities)) as part of the backward pass: with a sink set, every
 * srlx_qnet_backward_td_u8 / _backward_u8 launches srlx_per_update(per, n, d_indices, d_priorities, prio_kind, on_device = 1) first thing on its weight-gradient
 * branch -- right behind the kernel that produced the priorities, beside the gradient kernels -- instead of the caller doing it after the optimiser step.
 * The branch joins the caller's stream before the call's last launch, so the tree is updated when the backward returns to the caller's stream order.
 * per = NULL removes the sink.  Pointers are device pointers that must stay valid (captured into HIP graphs with the pass). */
int srlx_qnet_set_priority_sink(srlx_qnet_t *h, srlx_per_t *per, int64_t n, const int64_t *d_indices, const void *d_priorities, int prio_kind);
/* a caller-owned HIP event (hipEvent_t, NULL: none) the priority sink's branch waits for before its write-back: a learner rank that commits incoming
 * transitions BESIDE its update (device/dist.py: tree add on a side stream between the update's draw and its write-back) records it behind the add, so the
 * tree sees draw -> add -> write-back in that order whatever the streams do */
int srlx_qnet_set_sink_wait(srlx_qnet_t *h, void *event);
/* ... and one recorded on that branch right BEHIND the write-back: whatever must see the written-back priorities -- the NEXT update's draw, which an engine runs
 * here, beside the rest of the backward pass, instead of at the head of the next update (device/rainbow.py) -- waits for it */
int srlx_qnet_set_sink_done(srlx_qnet_t *h, void *event);
/* ... and a caller-owned stream (hipStream_t, NULL: none) the write-back is launched on instead of the weight-gradient branch, behind the kernel that produced the
 * priorities (and the wait event, if any).  For a learner rank whose write-back waits for a long ingest: the weight gradients then do not queue behind that wait.
 * The CALLER joins that stream (the event of srlx_qnet_set_sink_done is recorded behind the write-back). */
int srlx_qnet_set_sink_stream(srlx_qnet_t *h, void *stream);
/* on != 0: a backward pass enqueues the first kernel of its data-gradient chain BEFORE the launches of its weight-gradient branch (default: behind them).  No
 * effect on results or on eager execution order constraints; under stream capture it decides which of the graph's internal streams the critical chain stays on
 * (finding 14). */
int srlx_qnet_set_main_first(srlx_qnet_t *h, int on);
/* splits = 2: conv3's data-gradient GEMM of the backward pass is split over K in two (twice the workgroups, each half as long; the pad fold adds the two partial
 * slabs) -- for a handle that has the GPU to itself (a learner-only rank), where one workgroup per CU is a serial chain; 1: one pass over K (default).  The sum over K
 * associates differently: results agree to float32 rounding, not bit for bit, with the unsplit pass. */
int srlx_qnet_set_dgrad_split(srlx_qnet_t *h, int splits);

/* a caller-owned HIP event (hipEvent_t, NULL: none) recorded on the backward pass's stream right behind its head kernel: with srlx_qnet_backward_td_u8 the TD
 * targets, loss and new priorities exist from there on, so the priority write-back (srlx_per_update) can run beside the gradient kernels on another stream */
int srlx_qnet_set_td_event(srlx_qnet_t *h, void *event);
/* Measurement aid (tools/lockstep_phases.py): with a buffer set, every backward pass launches srlx_debug_stamp at fixed points -- d_buf[16] head kernel done,
 * [17] first dense layer's data gradient, [18] conv3's data gradient + fold, [19] conv2's data gradient + fold, [20] conv1's weight gradient (caller's stream);
 * [21] priority sink, [22] conv3's weight gradient + reduction, [23] conv2's, [24] the first dense layer's (weight-gradient branch); every forward pass of the
 * handle: [10] convolutions, [11] first dense layer, [12] head.  NULL: none (production). */
int srlx_qnet_set_stamp_buffer(srlx_qnet_t *h, uint64_t *d_buf);
/* Where a backward pass launches the first dense layer's Adam-fused weight gradient (the update's largest kernel: 240 MB): 0 = last on the weight-gradient
 * branch (default), 1 = first on it, 2 = on a branch of its own as soon as the data gradient has read the weights.  2 makes a captured update three
 * branches wide: use it only with the actors on a stream of another priority level (srlx_stream_create). */
int srlx_qnet_set_fc1_branch(srlx_qnet_t *h, int order);
int srlx_qnet_fuse_adam_fc1_planes(srlx_qnet_t *h, void *d_planes_out);
int srlx_qnet_set_pack_sticky(srlx_qnet_t *h, int on);
/* splits > 0: the chip-filling first-dense-layer launches of a handle with operand planes use half-CU workgroups (256 threads, 72 KB of LDS, `splits` K splits:
 * a steady stream of short workgroups that leaves room for a learner's kernels on every compute unit); 0 (default): CU-filling workgroups, the fastest form alone. */
int srlx_qnet_set_fc1_neighbour(srlx_qnet_t *h, int splits);
/* a learner's handle: operand planes also for its passes of one row tile (<= 128 rows: the convolution kernel writes float32 act3 AND planes; first dense layer on
 * the one-row-tile kernel k_fc1_planes_rows with the staging-split GEMM's split-K shape: bit-identical results; on = 2: on the half-CU kernel padded to its tile
 * instead -- measurements only; launches of 129-511 rows stay on the staging-split GEMM); d_weight_planes = BORROWED planes of the bound weight (an actor set's, srlx_qnet_actor_set_planes:
 * the set the last update published holds the online network's current weight) or NULL for the handle's own (srlx_qnet_refresh_fc1_planes) */
int srlx_qnet_set_planes_small(srlx_qnet_t *h, int on, const void *d_weight_planes);
int srlx_qnet_weights_changed(srlx_qnet_t *h);
/* The image block alone (DQNImageBlock, srl/rl/torch_/blocks/dqn_image_block.py:29-54: three convolutions with replicate padding + ReLU) for
 * networks whose dense part is not the dueling head of this handle (Agent57_light's UVFA Q-networks, its embedding and RND networks,
 * agent57_light/model_torch.py:35-64,98-131,160-193): d_features = float32 [batch][OH3*OW3][2*filters] -- the post-ReLU conv3 output in
 * PIXEL-major order (torch's `flatten` of the NCHW tensor is channel-major: transpose the last two axes).  Only entries 0..5 of
 * srlx_qnet_bind are read. */
int srlx_qnet_forward_convs_u8(srlx_qnet_t *h, int64_t batch, const uint8_t *d_frame_base, const int64_t *d_frame_off, float *d_features, void *stream);
/* Measurement hook: the NEXT forward on this handle records the two caller-owned HIP events (hipEvent_t) on its stream right
 * around the dominant kernel -- the one k_convnet_fused launch of the Atari geometry (the filter-packing launch before it excluded), or the
 * conv2 + conv3 launches of k_gemm<AConv> elsewhere -- so that bench.py can time that kernel live, on the stream it runs on.  NULL events
 * switch it off. */
int srlx_qnet_set_probe(srlx_qnet_t *h, void *ev_start, void *ev_end);
/* the same for the first dense layer's GEMM launch (FC1: the second-largest kernel of a lock-step) */
int srlx_qnet_set_probe_fc1(srlx_qnet_t *h, void *ev_start, void *ev_end);
/* ... and the KERNEL's own span (round 5): d_span[0] / d_span[1] (pre-set by the caller to UINT64_MAX / 0) receive min(first workgroup in) / max(last workgroup out)
 * of the device's 100 MHz wall clock for the NEXT operand-planes first-dense-layer launch -- what rocprofv3's kernel trace reports as that kernel's duration, without
 * the queue wait an event bracket on the launch stream includes when other streams hold the compute units. */
int srlx_qnet_set_fc1_span(srlx_qnet_t *h, uint64_t *d_span);
/* The first dense layer of chip-filling launches (>= 512 rows, a multiple of 128: the actors' policy pass) on PRE-SPLIT operands.  The layer evaluates
 * float32 x float32 as three exact products of two float16 parts per operand; by default both operands are split while staging, in every workgroup, every
 * K-slab.  A handle with planes enabled keeps its weight as the two parts ([K/32][unit][2][4][8 f16]: the float32's own 4 bytes per value), the convolution kernel writes its output
 * in the same form, and the GEMM runs without conversions (bit-identical results).  The planes are a CACHE of the float32 weight: after every change of
 * the weight call srlx_qnet_refresh_fc1_planes (d_src_wf = NULL: split the bound weight; otherwise split `d_src_wf`, and when d_copy_dst != NULL also
 * write the float32 values there -- the per-lock-step refresh of an actor's private copy of the online network, play_mp.py:121-165, and its planes in
 * one pass), or srlx_qnet_invalidate_fc1_planes to fall back to the staging split until the next refresh. */
int srlx_qnet_enable_fc1_planes(srlx_qnet_t *h);
int srlx_qnet_refresh_fc1_planes(srlx_qnet_t *h, const float *d_src_wf, float *d_copy_dst, void *stream);
int srlx_qnet_invalidate_fc1_planes(srlx_qnet_t *h);
/* measurement aid: d_phase_stamps = device uint64 [8 waves][8] (or NULL to switch off): the fused convolution kernel's workgroup 0
 * records its shader clock at the phase boundaries (start, frames issued, staged, conv1 done, barrier, conv2 done, barrier, end) */
int srlx_qnet_set_debug(srlx_qnet_t *h, void *d_phase_stamps);
/* Round 6: the fused convolution kernel evaluates its float32 products as three exact products of two float16 parts per operand (x = hi + lo / 2048).  An
 * activation above 65 504 does not fit; the kernel then sets bit (layer - 1) of a device word of the handle instead of failing silently.  *out_bits = that word
 * (blocking device-to-host copy: call where the host has synchronised; the host side raises, device/qnet.py:check_ranges).  SRLX_CONV_BF16X3=1 (the
 * environment switches above) avoids the limit. */
int srlx_qnet_range_flags(srlx_qnet_t *h, int *out_bits);
/* For tests that compare two ways of running a forward pass: what the pass left in the handle.  what 0..8: the device buffer act1, act2, act3, h1 (post-ReLU hidden
 * layer of a training handle), activation planes, split-K partial sums, packed filters, transposed filters of conv3 / conv2 -> *d_ptr (BORROWED; NULL where the
 * handle owns none) and its size *n in float32 elements (the planes: float16 elements).  what 100: host-side state as bits of *n: 1 the last forward built the
 * transposed filters, 2 packed filters valid, 4 activation planes fresh, 8 weight planes valid, 16 the pass continued into the dense layers, 32 partial sums used. */
int srlx_qnet_inspect(srlx_qnet_t *h, int what, void **d_ptr, int64_t *n);
/* Training on the vectorised path (replaces `loss.backward()` + the framework forward it needs,
 * srl/algorithms/rainbow/model_torch.py:103-109):
 *   srlx_qnet_enable_training : from now on every forward keeps its post-ReLU hidden layer, and gradient scratch for up
 *       to max_train_batch (<= 64) samples is allocated.  Covers the DQN image block with 32 filters, dueling "average"/"".
 *   srlx_qnet_backward_u8     : given d loss / d Q  f32 [batch][n_actions] for the samples at rows 0, stride, 2*stride, ...
 *       of the LAST srlx_qnet_forward_u8 on this handle (same d_frame_base / d_frame_off), writes every parameter
 *       gradient into d_grads[12] (same order and memory layouts as srlx_qnet_bind: the torch parameters' own layouts).
 *   srlx_qnet_fuse_adam_fc1   : the first dense layer's weight [2*hidden][flat] holds 97 % of the network's parameters.  With its
 *       Adam state bound here (d_exp_avg / d_exp_avg_sq in the weight's layout, d_steps_taken = device scalar of optimiser steps
 *       already applied, the same one srlx_adam_step reads), srlx_qnet_backward_u8 applies `optimizer.step()` (model_torch.py:109)
 *       to that tensor inside its weight-gradient kernel: d_grads[6] is NOT written and the caller's srlx_adam_step must leave the
 *       tensor out.  d_exp_avg = NULL unbinds.  Refused for NoisyLinear handles (the sigma gradient needs the weight gradient). */
int srlx_qnet_enable_training(srlx_qnet_t *h, int64_t max_train_batch);
int srlx_qnet_fuse_adam_fc1(srlx_qnet_t *h, float *d_exp_avg, float *d_exp_avg_sq, double lr, double beta1, double beta2, double eps,
                            const int64_t *d_steps_taken);
/* srlx_qnet_fuse_adam_rest (round 5; after srlx_qnet_fuse_adam_fc1, whose hyper-parameters and step count it uses): `optimizer.step()` (model_torch.py:109) for
 * EVERY OTHER tensor inside the launch that finishes its gradient -- the convolution weights and biases in the epilogue of their gradient reductions, the first
 * dense layer's bias and the head's second layers in the small-vector range of the packing launch of srlx_qnet_publish -- so that no optimiser launch is left on
 * the update's tail (srlx_adam_step is then not called at all).  The three arrays are indexed like the gradient list of srlx_qnet_backward_u8 (entry 6 ignored);
 * every later backward pass must be handed the same gradient buffers, and EVERY backward pass must be followed by srlx_qnet_publish(h, ...) (which completes the
 * step; the next backward pass fails loudly otherwise).  The arithmetic is srlx_adam_step's, element by element: bit-equal results.  d_grads == NULL: off. */
int srlx_qnet_fuse_adam_rest(srlx_qnet_t *h, const float *const *d_grads, float *const *d_exp_avg, float *const *d_exp_avg_sq);
int srlx_qnet_backward_u8(srlx_qnet_t *h, int64_t batch, int64_t sample_stride, const uint8_t *d_frame_base, const int64_t *d_frame_off,
                          const float *d_grad_q, float *const *d_grads, void *stream);
/* The image block alone (networks whose dense part is not this handle's dueling head: Agent57_light's UVFA Q-networks, embedding and RND networks --
 * srl/algorithms/agent57_light/model_torch.py:18-117): given d loss / d features f32 [batch][pixels * channels] (the layout srlx_qnet_forward_convs_u8
 * returns; rows = the samples at rows 0, stride, 2*stride, ... of the LAST forward on this training-enabled handle), the ReLU mask of the kept
 * activations is applied and the convolution part of loss.backward() (model_torch.py:437-439) runs: d_grads[0..5] = conv1 w, b, conv2 w, b, conv3 w, b in
 * each parameter's own memory layout.  Same kernels, streams and fixed summation orders as the convolution half of srlx_qnet_backward_u8: run to run
 * the gradients are bit-identical. */
int srlx_qnet_backward_convs_u8(srlx_qnet_t *h, int64_t batch, int64_t sample_stride, const uint8_t *d_frame_base, const int64_t *d_frame_off,
                                const float *d_grad_features, float *const *d_grads, void *stream);
/* srlx_nstep_td_huber_priority_packed + srlx_qnet_backward_u8 in one call (one launch less on the learner's chain): the head kernel of
 * the backward pass evaluates the TD target / Huber loss / gradient seed / priorities itself (arguments and results as in
 * srlx_nstep_td_huber_priority_packed, bit-equal; d_q_on_all = the [batch][n_step+1][n_actions] output of the LAST forward on this handle,
 * i.e. sample_stride = n_step + 1) and back-propagates that seed. */
int srlx_qnet_backward_td_u8(srlx_qnet_t *h, int64_t batch, int n_step, const uint8_t *d_frame_base, const int64_t *d_frame_off, const float *d_q_on_all,
                             const float *d_q_tg_next, const int32_t *d_actions, const float *d_rewards, const float *d_terminated,
                             const uint8_t *d_invalid_next, const float *d_weights, double discount, double retrace_h, int enable_double_dqn,
                             int enable_rescale, float *d_target, float *d_loss, float *d_grad_q0, float *d_priorities, float *const *d_grads, void *stream);
int srlx_qnet_forward_f32(srlx_qnet_t *h, int64_t batch, const float *d_obs_nchw, float *d_q, void *stream);
/* The image block over float32 frame SEQUENCES of thousands of rows (Agent57's in-block: srl/rl/torch_/blocks/dqn_image_block.py:29-54 as
 * srl/algorithms/agent57/model_torch.py:39-87 calls it on [B * S] states), on a handle used the way srlx_qnet_forward_convs_u8's callers use it (entries 0..5 of
 * srlx_qnet_bind are read).  Every row count takes the same launches, float32 MFMA with fixed summation orders: results are bit-identical run to run.
 *   srlx_qnet_forward_convs_f32    : d_frames f32 [rows][H][W][C] (channels LAST, C = the handle's `window`, 1..4; C = 1 is the bytes of a channels-first stack);
 *       row r of the features at d_features + r * ld_features: 2 F * OH3 * OW3 floats in torch's flatten order (channel-major); ld_features >= that, columns behind
 *       the features are not touched (the rows may be the first columns of wider rows, an LSTM's input).  rows <= max_batch, <= 65536.  The post-ReLU activations
 *       of the LAST forward stay in the handle (NHWC) for the backward pass.
 *   srlx_qnet_seq_training_bytes   : host arithmetic, no device: the bytes srlx_qnet_enable_seq_training(h, max_rows) allocates on a handle of this geometry,
 *       or -1 outside the envelope: filters = 32, square frames, H a multiple of 4 in 8..84, 1..4 channels, 1 <= max_rows <= 65536.
 *   srlx_qnet_enable_seq_training  : gradient scratch for up to max_rows (<= max_batch) gradient rows; *bytes_allocated (may be NULL) = what was allocated.  Not
 *       combined with srlx_qnet_enable_training on one handle.
 *   srlx_qnet_backward_convs_f32   : d loss / d features of ALL `rows` rows of the LAST srlx_qnet_forward_convs_f32 on this handle (same d_frames; rows in the
 *       same channel-major order, row stride ld_grad >= the feature count); applies the ReLU mask of the kept activations and writes d_grads[0..5] = conv1 w, b,
 *       conv2 w, b, conv3 w, b in each parameter's own memory layout (conv2 / conv3 channels_last, as srlx_qnet_bind reads them).  Weight gradients: the rows are cut
 *       into ceil(rows / ceil(rows / 256)) parts of consecutive rows, a part adds its rows in row order, the parts are added in part order -- one summation order per
 *       element, no atomics: two calls on the same data give bit-equal gradients.  One stream, one launch per stage. */
int srlx_qnet_forward_convs_f32(srlx_qnet_t *h, int64_t rows, const float *d_frames, float *d_features, int64_t ld_features, void *stream);
int64_t srlx_qnet_seq_training_bytes(int in_h, int in_w, int channels, int filters, int64_t max_rows);
int srlx_qnet_enable_seq_training(srlx_qnet_t *h, int64_t max_rows, int64_t *bytes_allocated);
int srlx_qnet_backward_convs_f32(srlx_qnet_t *h, int64_t rows, const float *d_frames, const float *d_grad_features, int64_t ld_grad, float *const *d_grads,
                                 void *stream);
/* Several networks over the SAME frames (round 6; Agent57_light evaluates five networks on the state a lock-step has just produced: the two UVFA Q-networks of the next
 * Worker.policy, agent57_light.py:355-363, and the embedding / RND networks of the intrinsic reward, :383-391):
 *   srlx_qnet_forward_convs_multi_u8 : the image blocks of `n` <= 8 inference handles (84 x 84 x 4, operand planes valid, batch >= 512 in multiples of 128) as ONE
 *       launch of n x batch workgroups -- one ramp and one tail instead of n; each handle is left with fresh operand planes;
 *   srlx_qnet_forward_dense_planes   : a handle's dense layers (first dense layer on the planes + its head: dueling / hidden-layer mode, UVFA terms) on those planes --
 *       together the two calls give what srlx_qnet_forward_u8 gives, bit for bit. */
int srlx_qnet_forward_convs_multi_u8(srlx_qnet_t *const *hs, int n, int64_t batch, const uint8_t *d_frame_base, const int64_t *d_frame_off, void *stream);
int srlx_qnet_forward_dense_planes(srlx_qnet_t *h, int64_t batch, float *d_q, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Agent57_light's five networks on srlx_qnet handles (round 6; SURVEY 8 a18, BASELINE configs[3]).
 * Replaces srl/algorithms/agent57_light/model_torch.py:18-117 (QNetwork with UVFA inputs, _EmbeddingNetwork, _LifelongNetwork), :244-255 (four Adams) and
 * :384-443 (_update_q) -- through round 5 the dense parts ran in torch (hipBLASLt + ATen elementwise).
 *   srlx_qnet_bind_uvfa       : a Q-network's UVFA inputs (:35-64: previous extrinsic reward, previous intrinsic reward, one-hot previous action, one-hot actor,
 *       concatenated BEHIND the image features).  Their columns of the dueling block's two first layers are kept apart from the image columns as
 *       d_wx float32 [n_cols][2 * hidden] (COLUMN-major: unit u of column c at c * 2 * hidden + u; units 0..hidden-1 = value stream, the rest = advantage stream) and
 *       enter the layer as rank-1 terms in the head kernel: reward * column, one column per one-hot.  col_* = first column of an input or -1 (input absent).
 *       Before srlx_qnet_actor_sets_enable: a published set carries a copy of the columns.
 *   srlx_qnet_set_uvfa_inputs : the per-row inputs of the next forward / backward passes, device arrays indexed by the forward's row (float32 rewards, int32 indices;
 *       NULL where the input is absent).  BORROWED until replaced (captured into HIP graphs with the passes).
 *   srlx_qnet_fuse_adam_uvfa  : gradient buffer of the columns (same layout; every backward pass writes it, beside the data-gradient chain) and, with Adam state
 *       (after srlx_qnet_fuse_adam_rest), their optimiser step in the packing launch of srlx_qnet_publish.
 *   srlx_qnet_set_td_extras   : the TD prologue of srlx_qnet_backward_td_u8 with a per-sample discount float32 [batch] (the sampled actor's gamma,
 *       agent57_light.py:263; n_step = 1 makes the prologue exactly calc_target_q :218-268) and the SIGNED TD error target - q float32 [batch] (:442).
 *   srlx_qnet_set_head_mode   : mode 1 = the handle ends behind the first dense layer (the embedding block :78 and the lifelong networks' hidden block :111): `d_q` of
 *       the forward entry points is float32 [batch][out_cols], the first out_cols post-ReLU units (a layer narrower than the GEMM's tile is padded with zero rows);
 *       d_ln_w / d_ln_b != NULL: nn.LayerNorm over all 2 * hidden units first (:112, inference only).  srlx_qnet_backward_u8 then takes d loss / d that output
 *       [batch][out_cols]; d_grads[8..11] are ignored (bind small dummies).  mode 0 = the dueling head.
 * ------------------------------------------------------------------------------------------------ */
int srlx_qnet_bind_uvfa(srlx_qnet_t *h, const float *d_wx, int n_cols, int col_ext, int col_int, int col_action, int n_action_in, int col_actor, int n_actor);
int srlx_qnet_set_uvfa_inputs(srlx_qnet_t *h, const float *d_r_ext, const float *d_r_int, const int32_t *d_action, const int32_t *d_actor);
int srlx_qnet_fuse_adam_uvfa(srlx_qnet_t *h, float *d_grad_wx, float *d_exp_avg, float *d_exp_avg_sq);
int srlx_qnet_set_td_extras(srlx_qnet_t *h, const float *d_discount_per_sample, float *d_td_signed);
int srlx_qnet_set_head_mode(srlx_qnet_t *h, int mode, int out_cols, const float *d_ln_w, const float *d_ln_b, double ln_eps);
/* Agent57_light around its networks, one launch each (csrc/srlx_agent57.hip):
 *   srlx_agent57_policy         : Worker.policy (agent57_light.py:355-375) for E environments: q = q_ext + beta[arm] * q_int, epsilon[arm]-greedy with the keyed uniforms
 *       (seed, *d_counter, 2 e / 2 e + 1) like srlx_qnet_forward_u8_policy (the counter is only read).  d_arm = NULL: evaluation (test_beta / test_epsilon, :294-297).
 *   srlx_agent57_post_step      : Worker.on_step's bookkeeping (:377-432): the item fields the frame store does not keep (rows of the caller's [ring slot][env] arrays:
 *       actor, previous action, previous rewards, intrinsic reward = episodic * lifelong :383-391), then previous action / rewards and the episode reward of the lanes
 *       that took a step (d_reset_lane == 0).
 *   srlx_agent57_begin_episodes : Worker.on_reset (:288-311) for the lanes in d_done (NULL: all): random previous action (keyed: seed, *d_counter, lane), zero previous
 *       rewards and episode reward; d_reset_lane (or NULL) := d_done, d_live_lane (or NULL) := !d_done.
 *   srlx_agent57_gather_inputs  : change_batches_format (:165-216) for a drawn batch located by srlx_store_locate: the online network's rows interleaved (2 b = s_0 with the
 *       inputs of model_torch.py:427-433, 2 b + 1 = s_1 with :294-299), the target network's rows (s_1), discount[b] = discount_list[actor] (:287), r_int[b].
 *   srlx_agent57_emb_tail       : the embedding network behind its two embeddings (model_torch.py:87-95) + MSE against the one-hot action (:343) + backward + Adam (:345-347)
 *       in ONE single-workgroup launch.  d_emb float32 [2 batch][emb_dim] (rows 2 b = f(s), 2 b + 1 = f(s')); the four pointer tables are HOST arrays of 6 device
 *       pointers: out_block weight [hidden][2 emb_dim], its bias, LayerNorm weight, bias, out_block_out1 weight [n_actions][hidden], its bias; d_exp_avg = NULL:
 *       gradients only.  d_steps_taken = optimiser steps already applied (device scalar).  Out: d_loss [1], d_grad_emb [2 batch][emb_dim].
 *   srlx_agent57_rnd_tail       : the predictor's LayerNorm (:112,116) + MSE against the target network's output (:357) + backward + Adam for the LayerNorm parameters;
 *       d_hidden / d_target = the predictor's post-ReLU hidden layer / the target network's output, `batch` rows of `dim` floats row_stride floats apart; d_mirror_* (or NULL) receive the updated LayerNorm parameters once more (the copy the actors
 *       read next). */
int srlx_agent57_policy(int64_t n_envs, int n_actions, const float *d_q_ext, const float *d_q_int, const int32_t *d_arm, const float *d_beta_list, const float *d_eps_list,
                        double test_beta, double test_epsilon, uint64_t seed, const int64_t *d_counter, int32_t *d_actions, float *d_q_out, void *stream);
int srlx_agent57_post_step(int64_t n_envs, const int32_t *d_actions, const int32_t *d_arm, const float *d_rewards, const uint8_t *d_reset_lane, const float *d_episodic,
                           const float *d_lifelong, int32_t *d_prev_action, float *d_prev_r_ext, float *d_prev_r_int, float *d_episode_reward, float *d_x_r_int,
                           float *d_x_prev_r_ext, float *d_x_prev_r_int, int32_t *d_x_actor, int32_t *d_x_prev_action, void *stream);
int srlx_agent57_begin_episodes(int64_t n_envs, int n_actions, const uint8_t *d_done, uint64_t seed, const int64_t *d_counter, int32_t *d_prev_action, float *d_prev_r_ext,
                                float *d_prev_r_int, float *d_episode_reward, uint8_t *d_reset_lane, uint8_t *d_live_lane, void *stream);
int srlx_agent57_gather_inputs(int64_t batch, int64_t n_envs, const int64_t *d_loc_env, const int64_t *d_loc_slot, const int32_t *d_actions, const float *d_rewards,
                               const float *d_x_r_int, const float *d_x_prev_r_ext, const float *d_x_prev_r_int, const int32_t *d_x_actor, const int32_t *d_x_prev_action,
                               const float *d_discount_list, float *d_on_r_ext, float *d_on_r_int, int32_t *d_on_action, int32_t *d_on_actor, float *d_tg_r_ext,
                               float *d_tg_r_int, int32_t *d_tg_action, int32_t *d_tg_actor, float *d_discount, float *d_r_int, void *stream);
/* Multi-GPU (BASELINE configs[3]: 7 actor GPUs + 1 learner GPU; replaces the pickled 11-field items of srl/base/run/play_mp.py:76-118 and their unpickling in the
 * trainer's drain thread, :248-286):
 *   srlx_agent57_pack_record   : an actor rank's lock-step as ONE packed record uint8 [(10 + 4 * 5) * n_envs] in the layout srlx_store_commit_step_packed takes with
 *       extra_floats = 5: [action | reward | terminated | done | (intrinsic reward, arm, previous action, previous extrinsic reward, previous intrinsic reward) per lane].
 *   srlx_agent57_unpack_fields : the learner rank's inverse for the five fields: environment g = lane g % envs_per_record of record g / envs_per_record; they land
 *       in row (*d_position mod ring_len) of the learner's [ring slot][environment] arrays -- the slot the ring commit of the same slab writes; the position is read
 *       on the device (srlx_store_views), so the launch replays inside a captured update.  Records are record_stride bytes apart: record_stride >= 30 *
 *       envs_per_record, envs_per_record % 4 == 0 and record_stride % 4 == 0 (the float fields of every record are read as aligned floats). */
int srlx_agent57_pack_record(int64_t n_envs, const int32_t *d_actions, const float *d_rewards, const uint8_t *d_terminated, const uint8_t *d_done, const float *d_x_r_int,
                             const int32_t *d_x_actor, const int32_t *d_x_prev_action, const float *d_x_prev_r_ext, const float *d_x_prev_r_int, uint8_t *d_record, void *stream);
int srlx_agent57_unpack_fields(int64_t n_records, int64_t envs_per_record, const uint8_t *d_records, int64_t record_stride, const int64_t *d_position, int64_t ring_len,
                               float *d_x_r_int, int32_t *d_x_actor, int32_t *d_x_prev_action, float *d_x_prev_r_ext, float *d_x_prev_r_int, void *stream);
int srlx_agent57_emb_tail(int64_t batch, int emb_dim, int hidden, int n_actions, const float *d_emb, const int32_t *d_actions, float *const *d_params, float *const *d_grads,
                          float *const *d_exp_avg, float *const *d_exp_avg_sq, double ln_eps, double lr, double beta1, double beta2, double eps, const int64_t *d_steps_taken,
                          float *d_loss, float *d_grad_emb, void *stream);
int srlx_agent57_rnd_tail(int64_t batch, int dim, int64_t row_stride, const float *d_hidden, const float *d_target, float *d_ln_w, float *d_ln_b, float *d_grad_ln_w, float *d_grad_ln_b,
                          float *d_exp_avg_w, float *d_exp_avg_sq_w, float *d_exp_avg_b, float *d_exp_avg_sq_b, float *d_mirror_w, float *d_mirror_b, double ln_eps, double lr,
                          double beta1, double beta2, double eps, const int64_t *d_steps_taken, float *d_loss, float *d_grad_hidden, void *stream);

/* NoisyLinear dense layers (replaces srl/rl/torch_/modules/noisy_linear.py:26-52, the dense layers of the reference's
 * rainbow.Config.set_atari_config(), rainbow.py:116-148): W = w_mu + w_sigma * eps, b = b_mu + b_sigma * eps, eps ~ N(0,1)
 * independent per element, ONE draw per forward call shared by all its rows.
 *   srlx_qnet_bind_noisy      : d_sigma[6] = sigma tensors of {fc1 weight [2*hidden][flat], fc1 bias, v2 weight, v2 bias, a2 weight,
 *       a2 bias}, same layouts as the mu tensors given to srlx_qnet_bind (entries 6..11).  From then on every forward first
 *       materialises the effective tensors of a fresh draw (keyed counter generator: eps is a function of (seed, draw id, tensor,
 *       element), so the backward pass regenerates it).
 *   srlx_qnet_redraw_rows     : re-evaluates the dense layers with ANOTHER fresh draw for rows 0, stride, 2*stride, ... of the last
 *       forward and overwrites their q rows -- the reference's train step evaluates q_online(s_1..s_n) and q_online(s_0) in two
 *       forward calls, i.e. under two draws (rainbow.py:220, model_torch.py:103); the backward pass then belongs to this draw.
 *   srlx_qnet_bind_noisy_grads: gradient tensors of the six sigmas; srlx_qnet_backward_u8 fills them (d_grads[6..11] are then the
 *       gradients of the mu tensors).
 *   srlx_qnet_noisy_effective : copies an effective tensor (0 fc1 weight .. 5 a2 bias) into d_out (device, may be NULL) and reports
 *       its element count and the id of the draw it holds (tests, diagnostics). */
int srlx_qnet_bind_noisy(srlx_qnet_t *h, const float *const *d_sigma, uint64_t seed);
int srlx_qnet_bind_noisy_grads(srlx_qnet_t *h, float *const *d_grad_sigma);
int srlx_qnet_redraw_rows(srlx_qnet_t *h, int64_t rows, int64_t row_stride, float *d_q, void *stream);
int srlx_qnet_noisy_effective(srlx_qnet_t *h, int which, float *d_out, int64_t *n_elems, int64_t *draw_id, void *stream);

/* DQN's Q-network for flat observations (srl/algorithms/dqn/model_torch.py:17-29: in_block -> hidden_block (MLP) -> out_layer), srlx_mlpq.hip.
 * obs_dim D = 1..256 float32 elements, n_layers = 1..3 Linear + ReLU layers (the input value block's layers, then the hidden block's) of widths[l] = 32..512 units
 * (multiples of 32), out_layer Linear to n_actions = 2..32.  Plain float32 arithmetic.
 *   srlx_mlpq_create       : max_rows = most rows of one srlx_mlpq_forward; max_batch = most items of one srlx_mlpq_train_step (<= 256; 0: the handle never trains)
 *   srlx_mlpq_bind         : d_params[2 * (n_layers + 1)] = weight [out][in], bias [out] of every layer in the reference's key order (in_block, hidden_block, out_layer)
 *   srlx_mlpq_bind_grads   : gradient tensors of the same shapes (NULL table: none); srlx_mlpq_train_step writes them
 *   srlx_mlpq_bind_adam    : exp_avg / exp_avg_sq of every parameter: srlx_mlpq_train_step then takes torch's Adam step (srlx_adam_math.h) in the launch that
 *                            finishes each gradient
 *   srlx_mlpq_forward      : Q of `rows` observations, row r at d_obs + d_row_offsets[r] (NULL: + r * D); d_q [rows][A] may be NULL.  d_actions != NULL: the
 *                            epsilon-greedy action of every row in the same launch, k_head's rule (srlx_policy_epsilon_greedy on the uniforms
 *                            srlx_rng_uniform(seed, counter, 2 * rows) would write); the counter is read, not advanced
 *   srlx_mlpq_train_step   : one DQN update (dqn.py:144-176, model_torch.py:89-131) in two launches: online forward over s_0 / s_1, target forward over s_1, the
 *                            1-step (double) target, IS-weighted Huber loss, d loss / d q, priorities |target - q|, backward through every layer, Adam.
 *                            d_offsets int64 [B][2] = element offsets of s_0, s_1 from d_obs_base (the store's frame_off_all at window 1, n_step 1); actions /
 *                            rewards / terminated / weights as srlx_per_sample_gather_train writes them; d_steps_taken = Adam steps already taken (device
 *                            scalar, not advanced here).  Outputs: d_q0 [B][A] (online Q of s_0 before the step), d_target, d_priorities [B], d_loss [1].
 *                            Gradient sums run in item order: two runs on the same inputs are bit-identical.
 *   srlx_mlpq_publish      : every parameter of `src` into `dst` (online -> target, online -> an actor copy), one launch
 * Rainbow's network on the same kernels (srl/algorithms/rainbow/model_torch.py:15-29: in_block -> MLP over layer_sizes[:-1] -> DuelingNetworkBlock):
 *   srlx_mlpq_create_dueling : n_trunk = 0..2 Linear + ReLU layers of trunk_widths[l] = 32..512 units (multiples of 32; the input value block's layers, then the
 *                            hidden block's layer_sizes[:-1]; 0: the head reads the observation row), then the dueling head (srl/rl/torch_/blocks/
 *                            dueling_network.py:8-59) with dueling_units H = 32..512 (multiples of 32) in each branch, dueling_type 0 "average" / 1 "",
 *                            n_actions 2..32, max_batch <= 256, max_nstep = 1..7 (the longest item of srlx_mlpq_train_nstep).  Anything else: an error before
 *                            any device call.  srlx_mlpq_bind / _bind_grads / _bind_adam take 2 * n_trunk + 8 tensors on such a handle, in the reference's
 *                            state_dict order: the trunk layers (weight, bias), v_layers.0 ([H][in], [H]), v_layers.2 ([1][H], [1]), adv_layers.0,
 *                            adv_layers.2 ([A][H], [A]).  srlx_mlpq_forward and srlx_mlpq_publish serve both kinds of handle.  In LDS the two branches' hidden
 *                            rows share one buffer (the value row is reduced to its scalar first): the row stride stays max width + 1.
 *   srlx_mlpq_train_nstep  : one Rainbow update (rainbow.py:185-287, model_torch.py:85-122) in two launches, on a dueling or a plain handle: 16 / (n + 1) items
 *                            per workgroup, online forward over s_0..s_n, target forward over s_1..s_n, the n-step retrace target of srlx_td_math.h:td_rows
 *                            (numpy's float32 order, float32(discount ** m) from the host; with `rescale` both value transforms in float64), IS-weighted
 *                            Huber loss, priorities, backward through the head (d adv_k = g ((k == a_0) - 1/A), "": g (k == a_0); d v = g) and the trunk, Adam.
 *                            d_offsets int64 [B][n + 1] (the store's frame_off_all at window 1), actions / rewards / terminated [B][n].  No invalid-action
 *                            mask.  Outputs as srlx_mlpq_train_step; bit-reproducible.  On a plain handle at n = 1, retrace_h = 1 every output, gradient and
 *                            post-Adam parameter is bit-equal to srlx_mlpq_train_step's.
 * NoisyLinear layers on a dueling handle (srl/rl/torch_/modules/noisy_linear.py:8-52: W = w_mu + w_sigma * eps, b = b_mu + b_sigma * eps, eps iid N(0, 1), drawn
 * anew on every forward call and shared by all rows of the call; rainbow.Config(enable_noisy_dense=True)):
 *   srlx_mlpq_bind_noisy   : d_sigma[2 * n_trunk + 8] in srlx_mlpq_bind's order; a layer is noisy iff both of its entries (weight sigma, bias sigma) are non-NULL.
 *                            The four head layers must be noisy; trunk layers may be plain, but only as a prefix (the input value block).  The tensors given to
 *                            srlx_mlpq_bind are then the mu tensors.  The handle allocates its effective tensors (two sets when it trains) and a device-resident
 *                            draw counter starting at 0.  A plain (srlx_mlpq_create) handle refuses: DQN has no noisy form.
 *   srlx_mlpq_bind_noisy_grads / _adam : the sigmas' gradient tensors (NULL table: none) and exp_avg / exp_avg_sq, tables in the same order (entries of plain
 *                            tensors are ignored); Adam's hyper-parameters are srlx_mlpq_bind_adam's, which comes first.
 *   The generator: eps(seed, draw, tensor index, element) = srlx_noise_math.h:noisy_eps_pair, a pure function (Box-Muller on srlx::rng_u64; elements 2 j and
 *                            2 j + 1 share one evaluation).  One launch (k_mlpq_noisy_eff) writes mu + sigma * eps of every noisy tensor; every other kernel
 *                            reads the effective tensors like plain weights.
 *   The draw-id contract: a handle's passes consume consecutive ids from its counter.  srlx_mlpq_forward on a noisy handle consumes 1.
 *                            srlx_mlpq_train_nstep consumes 2 on the online handle (id: the pass over s_1..s_n, id + 1: the pass over s_0, whose gradient is
 *                            taken) and 1 on the target handle, whatever double_dqn is.  The ids are read from device memory, so a captured update replays with
 *                            fresh noise.  A counter is advanced by the launch BEHIND the one that reads it (the acting kernel, the learner kernel), never by
 *                            a launch whose other workgroups still read it.  The sigma gradients d loss / d sigma = d loss / d W * eps regenerate eps from the
 *                            id the s_0 pass used, which the materialising launch recorded.
 *   srlx_mlpq_forward      : effective tensors of a fresh draw (one added launch), otherwise unchanged; a noisy net acts greedily (rainbow.py:305-309): the caller
 *                            passes eps = 0 rows.
 *   srlx_mlpq_train_nstep  : three launches on noisy handles: the three draws, the learner kernel (the online pass split: rows of s_0 under draw id + 1 with
 *                            their kept planes, rows of s_1..s_n under draw id; the target pass under the target's draw and its own sigmas; the backward chain
 *                            through the s_0 effective weights), and the gradient / Adam launch, where the thread that sums d loss / d W of an element also
 *                            writes g_mu = g, g_sigma = g * eps and takes both Adam steps.  With every sigma 0 the outputs, mu gradients and post-Adam mu are the
 *                            plain dueling handle's bits.  Refused: a noisy online handle with a plain target or the reverse, neither sigma gradients nor sigma
 *                            Adam state bound.  srlx_mlpq_train_step refuses noisy handles.
 *   srlx_mlpq_publish      : copies the sigmas too (a second launch); refuses a noisy source with a plain destination and the reverse
 *   srlx_mlpq_noisy_draw   : synchronises the device; *set_next (may be NULL) becomes the id the next pass uses; *next_out (may be NULL) receives that id
 *   srlx_mlpq_noisy_eps    : writes eps(seed of the handle, draw, param_index, .) of one noisy tensor into d_out (its shape): the noise of a step, known before
 *                            the step runs
 *
 * Categorical DQN (C51; srl/algorithms/c51/c51.py:23-142: in_block -> hidden_block (MLP) -> Dense(A * N) reshaped to [A][N], a softmax over the N atoms of the
 * support linspace(v_min, v_max, N), Q = the expectation; srlx_c51_math.h holds the arithmetic once and states its precision):
 *   srlx_mlpq_create_categorical : a plain handle whose out_layer has n_actions * n_atoms rows (row a * n_atoms + j: atom j of action a).  obs_dim 1..256,
 *                            n_layers 1..3 of 32..512 units in multiples of 32, n_actions 2..32, n_atoms 2..256, n_actions * n_atoms <= 512, v_min < v_max both
 *                            finite, max_batch <= 256; anything else is an error before any device call.  srlx_mlpq_bind / _bind_grads / _bind_adam /
 *                            _publish take the 2 * (n_layers + 1) tensors of a plain handle.  srlx_mlpq_forward writes the EXPECTATIONS where Q rows go
 *                            (d_q [rows][n_actions]) and selects actions on them by the same keyed rule.  srlx_mlpq_train_step, srlx_mlpq_train_nstep and
 *                            srlx_mlpq_bind_noisy refuse such a handle.
 *   srlx_mlpq_train_categorical : one C51 update (c51.py:70-142) in two launches: 8 items per workgroup, ONE online pass over s_0 and s_1 (there is no target
 *                            network, :91), the greedy next action by expectation, the projected target distribution, the clipped cross-entropy and its seeds,
 *                            the backward chain; then srlx_mlpq_train_step's gradient / Adam launch.  d_offsets int64 [B][2], actions i32 [B], rewards /
 *                            terminated f32 [B].  Outputs: d_q0 [B][n_actions] expectations of s_0, d_p0 [B][n_atoms] the softmax of a_0's logits, d_m
 *                            [B][n_atoms] the projected target, d_loss [1] the batch mean, d_item_loss [B] the items' cross-entropies (they stand where the
 *                            priorities stand: a uniform memory ignores the values and counts the update).  Bit-reproducible.  Refuses any other handle.
 *   srlx_c51_loss          : the same item arithmetic in one launch on logits f32 [B][n_actions * n_atoms] of s' and s that the caller computed (the plugin
 *                            trainer's torch forward): d_m / d_p0 [B][n_atoms], d_grad_logits [B][n_actions * n_atoms] = d mean-loss / d logits of s (zero outside
 *                            a_0's atoms), d_loss [1].  On the same logits every output is srlx_mlpq_train_categorical's bits.
 * Batch CartPole (envs/cartpole.py:step; srlx_mlpq.hip): float64 state [E][4], steps / episodes int32 [E].  A lane whose d_needs_reset entry is set (the store's
 * needs_reset view, srlx_store_views) starts its next episode instead of stepping: state uniform in [-0.05, 0.05]^4 from (seed, lane, episode of the lane), its
 * first observation in d_obs, reward / terminated / done 0.  d_needs_reset NULL: every lane starts an episode (actions and scalar outputs may be NULL).
 * Otherwise one Euler step: reward 1, terminated outside +-12 degrees / +-2.4, done = terminated or step count >= max_steps; d_obs [E][4] float32. */
typedef struct srlx_mlpq srlx_mlpq_t;
int srlx_mlpq_create(srlx_mlpq_t **out, int obs_dim, int n_layers, const int *widths, int n_actions, int64_t max_rows, int64_t max_batch, int device);
int srlx_mlpq_destroy(srlx_mlpq_t *h);
int srlx_mlpq_bind(srlx_mlpq_t *h, float *const *d_params);
int srlx_mlpq_bind_grads(srlx_mlpq_t *h, float *const *d_grads);
int srlx_mlpq_bind_adam(srlx_mlpq_t *h, float *const *d_exp_avg, float *const *d_exp_avg_sq, double lr, double beta1, double beta2, double eps);
int srlx_mlpq_forward(srlx_mlpq_t *h, int64_t rows, const float *d_obs, const int64_t *d_row_offsets, float *d_q, const float *d_eps, uint64_t seed,
                      const int64_t *d_counter, int32_t *d_actions, void *stream);
int srlx_mlpq_train_step(srlx_mlpq_t *h, const srlx_mlpq_t *target, int64_t batch, const float *d_obs_base, const int64_t *d_offsets, const int32_t *d_actions,
                         const float *d_rewards, const float *d_terminated, const float *d_weights, double discount, int double_dqn, int rescale,
                         const int64_t *d_steps_taken, float *d_q0, float *d_target, float *d_loss, float *d_priorities, void *stream);
int srlx_mlpq_publish(const srlx_mlpq_t *src, srlx_mlpq_t *dst, void *stream);
int srlx_mlpq_create_dueling(srlx_mlpq_t **out, int obs_dim, int n_trunk, const int *trunk_widths, int dueling_units, int dueling_type, int n_actions,
                             int64_t max_rows, int64_t max_batch, int max_nstep, int device);
int srlx_mlpq_train_nstep(srlx_mlpq_t *h, const srlx_mlpq_t *target, int64_t batch, int n, const float *d_obs_base, const int64_t *d_offsets,
                          const int32_t *d_actions, const float *d_rewards, const float *d_terminated, const float *d_weights, double discount, double retrace_h,
                          int double_dqn, int rescale, const int64_t *d_steps_taken, float *d_q0, float *d_target, float *d_loss, float *d_priorities, void *stream);
int srlx_mlpq_bind_noisy(srlx_mlpq_t *h, float *const *d_sigma, uint64_t seed);
int srlx_mlpq_bind_noisy_grads(srlx_mlpq_t *h, float *const *d_grad_sigma);
int srlx_mlpq_bind_noisy_adam(srlx_mlpq_t *h, float *const *d_exp_avg, float *const *d_exp_avg_sq);
int srlx_mlpq_noisy_draw(srlx_mlpq_t *h, const int64_t *set_next, int64_t *next_out);
int srlx_mlpq_noisy_eps(srlx_mlpq_t *h, int64_t draw, int param_index, float *d_out, void *stream);
int srlx_mlpq_create_categorical(srlx_mlpq_t **out, int obs_dim, int n_layers, const int *widths, int n_actions, int n_atoms, double v_min, double v_max,
                                 int64_t max_rows, int64_t max_batch, int device);
int srlx_mlpq_train_categorical(srlx_mlpq_t *h, int64_t batch, const float *d_obs_base, const int64_t *d_offsets, const int32_t *d_actions, const float *d_rewards,
                                const float *d_terminated, double discount, const int64_t *d_steps_taken, float *d_q0, float *d_p0, float *d_m, float *d_loss,
                                float *d_item_loss, void *stream);
int srlx_c51_loss(int64_t batch, int n_actions, int n_atoms, double v_min, double v_max, double discount, const float *d_logits_next, const float *d_logits_0,
                  const int32_t *d_actions, const float *d_rewards, const float *d_terminated, float *d_m, float *d_p0, float *d_grad_logits, float *d_loss,
                  void *stream);
int srlx_cartpole_step(int64_t n_envs, double *d_state, int32_t *d_steps, int32_t *d_episodes, const uint8_t *d_needs_reset, const int32_t *d_actions,
                       int64_t max_steps, uint64_t seed, float *d_obs, float *d_reward, uint8_t *d_terminated, uint8_t *d_done, void *stream);

/* ---- Agent57's recurrent layer (srlx_lstm.hip) ----------------------------------------------------------------------------------------------------------
 * One-layer, unidirectional, batch_first LSTM in float32 with torch.nn.LSTM's parameter layout (srl/algorithms/agent57/model_torch.py:39-46,74-75):
 *   w_ih [4 H][I], w_hh [4 H][H], b_ih [4 H], b_hh [4 H]; gate rows in the order i, f, g, o (rows g H .. g H + H - 1 belong to gate g).
 *   x [B][T][I], y [B][T][H] (row b T + t), h0 / c0 / h_n / c_n [B][H] (torch's (1, B, H) without the leading 1).  All tensors dense.
 *   i, f, o = 1 / (1 + expf(-pre)), g = tanhf(pre), c_t = f c_{t-1} + i g, h_t = o tanhf(c_t); pre = x_t W_ih^T + b_ih + b_hh + h_{t-1} W_hh^T.
 * Envelope (validated before any device call; a violation returns SRLX_ERR_INVALID and srlx_last_error() names lstm): B 1..256, T 1..256, I 1..16384,
 * H a multiple of 16 in 16..512.  h0, w_hh, y and scratch must be 16-byte aligned.
 *   srlx_lstm_workspace_floats : floats of the training workspace (gate activations [B T][4 H], then cell states [B T][H]: 5 B T H) when `training`, 0
 *                                otherwise (a pass without gradient keeps nothing); -1 outside the envelope.  Host arithmetic.
 *   srlx_lstm_scratch_floats   : floats of the scratch buffer of either call (the input projection or dG [B T][4 H], then the dc carry [B][H]); -1 outside
 *                                the envelope.  Host arithmetic.  A forward and the backward that belongs to it may share one scratch buffer.
 *   srlx_lstm_forward          : 1 + T launches.  One dense GEMM projects every time step's input, then one launch per step adds h_{t-1} W_hh^T, runs the
 *                                cell in its epilogue and writes h_t into y[b][t], where step t + 1 reads it.  With `workspace` it also stores the gate
 *                                activations and c_t for srlx_lstm_backward; with NULL (burn-in, target pass, acting) it stores neither and c_n carries the
 *                                running cell state.  y, h_n and c_n are the same bits either way.  h0 / c0 must not alias h_n / c_n.
 *   srlx_lstm_backward         : T launches (t = T-1 .. 0: dh_t = dy[:, t] + dG_{t+1} W_hh, the pointwise backward into the pre-activation gate gradients
 *                                dG_t and the dc carry), one more for dh0 when asked, then dx = dG W_ih (when asked), dw_ih = dG^T x, dw_hh = dG^T h_prev
 *                                and db_ih = db_hh = column sums of dG.  dh_n / dc_n (gradients of the final state) may be NULL (zero); dx, dh0, dc0 may be
 *                                NULL (not wanted).  Outputs are overwritten, not accumulated.  Every sum over B T runs in a fixed order without atomics: two
 *                                calls on the same inputs give the same bits. */
int64_t srlx_lstm_workspace_floats(int64_t B, int64_t T, int64_t I, int64_t H, int training);
int64_t srlx_lstm_scratch_floats(int64_t B, int64_t T, int64_t I, int64_t H, int training);
int srlx_lstm_forward(int64_t B, int64_t T, int64_t I, int64_t H, const float *x, const float *h0, const float *c0, const float *w_ih, const float *w_hh,
                      const float *b_ih, const float *b_hh, float *y, float *h_n, float *c_n, float *workspace, float *scratch, void *stream);
int srlx_lstm_backward(int64_t B, int64_t T, int64_t I, int64_t H, const float *x, const float *h0, const float *c0, const float *w_ih, const float *w_hh,
                       const float *y, const float *workspace, const float *dy, const float *dh_n, const float *dc_n, float *dx, float *dw_ih, float *dw_hh,
                       float *db_ih, float *db_hh, float *dh0, float *dc0, float *scratch, void *stream);

/* ---- Agent57 sequence store (srlx_seqstore.hip) ---------------------------------------------------------------------------------------------------------
 * Batch assembly of Agent57's sequence replay (srl/algorithms/agent57/agent57.py:652-663 stores the window; model_torch.py's `train` rebuilds the batch on the
 * host) from device-resident arrays the CALLER owns (device/sequence_store.py keeps them as torch tensors); the entry point is stateless.
 *   ring    f32 [frame_capacity][frame_stride]: every distinct observation once; frame_stride >= frame_elems, padded by the caller to a multiple of 4 floats
 *           so that rows start on 16 bytes.  Row offsets are 64-bit (100 000 frames of 84 x 84 floats are 2.8 GB).
 *   records i32 [seq_capacity][record_stride]: one packed record per stored sequence, in dwords (L = burnin + sequence_length + 1, S = sequence_length):
 *             [0, L)            frame table i32: the ring row of every step's observation; -1 = an all-zero frame (episode padding)
 *             [L, 2L)           action indices i32
 *             [2L, 3L), [3L,4L) r_ext, r_int f32
 *             [4L, 4L+S)        undone f32 (0 after a terminal step)
 *             4L+S              actor index i32
 *             then 4 H          h_ext, c_ext, h_int, c_int f32 [H] each: both networks' recurrent state at the window head
 *             then S A bytes    next-step invalid-action mask u8 [S][A]
 *           srlx_seq_record_dwords(L, S, A, H) is that length rounded up to a multiple of 4 (host arithmetic; -1 outside the envelope).
 *   slots   i64 [B]: the records to gather (repeats allowed).  A slot outside [0, seq_capacity), or a table entry outside [-1, frame_capacity), reads nothing and
 *           yields zeros: the kernel never dereferences an index it was not given room for.
 * Outputs, dense, in the layouts the trainer feeds its networks: states f32 [B][L][frame_elems], actions i64 [B][L], r_ext / r_int f32 [B][L], dones f32 [B][S],
 * invalid u8 [B][S][A], actor i64 [B], h_ext / c_ext / h_int / c_int f32 [B][H].
 * One launch, no atomics, no scratch.  Rows move as 16-byte accesses when frame_elems and frame_stride are multiples of 4 and ring and states are 16-byte aligned,
 * as dwords otherwise (chosen per launch).  Envelope, validated before any device call (a violation returns SRLX_ERR_INVALID and srlx_last_error() names
 * srlx_seq_gather): B 1..1024, L 2..513, 1 <= S < L, A 1..64, H 1..1024, frame_elems 1..2^20, frame_stride >= frame_elems, frame_capacity 1..2^31-1,
 * seq_capacity >= 1, record_stride >= srlx_seq_record_dwords, no NULL pointer. */
#define SRLX_SEQ_MAX_B 1024
#define SRLX_SEQ_MAX_L 513
#define SRLX_SEQ_MAX_A 64
#define SRLX_SEQ_MAX_H 1024
#define SRLX_SEQ_MAX_FRAME_ELEMS 1048576
#define SRLX_SEQ_MAX_FRAME_CAPACITY 2147483647
int64_t srlx_seq_record_dwords(int64_t L, int64_t S, int64_t A, int64_t H);
int srlx_seq_gather(int64_t B, int64_t L, int64_t S, int64_t A, int64_t H, int64_t frame_elems, int64_t frame_stride, int64_t frame_capacity, int64_t seq_capacity,
                    int64_t record_stride, const int64_t *d_slots, const float *d_ring, const int32_t *d_records, float *d_states, int64_t *d_actions,
                    float *d_r_ext, float *d_r_int, float *d_dones, uint8_t *d_invalid, int64_t *d_actor, float *d_h_ext, float *d_c_ext, float *d_h_int,
                    float *d_c_int, void *stream);

/* ---- Agent57 lane sequence ring (srlx_seqstore.hip) ---------------------------------------------------------------------------------------------------------
 * The sequence replay of E lock-stepped lanes (device/sequence_store.py: LaneSequenceStore; device/agent57.py).  Every per-step field is stored ONCE, time-major,
 * in rings the CALLER owns, position t of all lanes in row t % T; both entry points are stateless.
 *   ring_frames  f32 [T][E][frame_stride]: the observation of (position, lane); frame_stride >= frame_elems, a multiple of 4 floats for 16-byte rows
 *   ring_scalars i32 [T][E][8]: action i32, r_ext f32, r_int f32, undone f32, actor index i32, age i32, two zero dwords.  age = steps since the lane's episode
 *                began, 0 on the episode's first observation
 *   ring_invalid u8  [T][E][A]: next-step invalid-action mask
 *   ring_hidden  f32 [T][E][4][H]: h_ext, c_ext, h_int, c_int as they were BEFORE the networks consumed that position's observation
 * srlx_seq_lane_push writes position t of all E lanes in one launch: frames f32 [E][frame_elems], action / actor i32 [E], r_ext / r_int / undone f32 [E], invalid u8
 * [E][A] (NULL: none), the four recurrent vectors f32 [E][H] each, first u8 [E].  A lane with first[e] != 0 (and every lane at t = 0) only delivers a new
 * episode's first frame: its entry keeps the frame and the actor index and otherwise reads like the padding before an episode -- rewards 0, undone 1, a keyed pad
 * action, zero recurrent state, no invalid action, age 0.  Every other lane gets age = age[t - 1] + 1, read from the ring.
 * srlx_seq_lane_gather turns B descriptors (i64 [B][3]: lane e, absolute position t of the window's last real entry, flush offset k in 0..L-1) into the outputs of
 * srlx_seq_gather, in one launch.  Entry l of window (e, t, k) is lane position p = t - (L - 1) + l + k:
 *   p > t               (after the end)            zero frame, rewards 0, undone 0, no invalid action, pad action
 *   t - p > age[t][e]   (before the episode start) zero frame, rewards 0, undone 1, no invalid action, pad action; at l = 0 zero recurrent state
 *   otherwise           the ring's entry of position p
 * with pad action = rng_u64(seed, e, p) % A (srlx_common.h; the same seed in both calls), so a pad keeps its value in every window that contains it.  dones and
 * invalid are the last S entries, actor is actor[t][e], the recurrent state is entry 0's.  A descriptor outside e in [0, E), t >= 0, 0 <= k < L reads nothing and
 * yields zeros.  That position p is still in the ring (t - p < T pushes ago) is the caller's ledger's business; a stale one reads other data, never other memory.
 * No atomics, no LDS, plain vector stores; rows move as 16-byte accesses when frame_elems and frame_stride are multiples of 4 and both frame pointers are 16-byte
 * aligned, as dwords otherwise (per launch).  Envelope, validated before any device call (SRLX_ERR_INVALID, srlx_last_error() names the entry point): B, L, S, A, H,
 * frame_elems, frame_stride as srlx_seq_gather; E 1..65536; T >= L (push: >= 2) with T * E <= 2^31-1; t >= 0; no NULL pointer but push's invalid. */
#define SRLX_SEQ_MAX_LANES 65536
int srlx_seq_lane_push(int64_t E, int64_t A, int64_t H, int64_t frame_elems, int64_t frame_stride, int64_t T, int64_t t, uint64_t seed, const float *d_frames,
                       const int32_t *d_action, const float *d_r_ext, const float *d_r_int, const float *d_undone, const int32_t *d_actor, const uint8_t *d_invalid,
                       const float *d_h_ext, const float *d_c_ext, const float *d_h_int, const float *d_c_int, const uint8_t *d_first, float *d_ring_frames,
                       int32_t *d_ring_scalars, uint8_t *d_ring_invalid, float *d_ring_hidden, void *stream);
int srlx_seq_lane_gather(int64_t B, int64_t L, int64_t S, int64_t A, int64_t H, int64_t E, int64_t T, int64_t frame_elems, int64_t frame_stride, uint64_t seed,
                         const int64_t *d_desc, const float *d_ring_frames, const int32_t *d_ring_scalars, const uint8_t *d_ring_invalid, const float *d_ring_hidden,
                         float *d_states, int64_t *d_actions, float *d_r_ext, float *d_r_int, float *d_dones, uint8_t *d_invalid, int64_t *d_actor, float *d_h_ext,
                         float *d_c_ext, float *d_h_int, float *d_c_int, void *stream);

/* ---- R2D2 sequence target (srlx_r2d2.hip) -----------------------------------------------------------------------------------------------------------------
 * R2D2's learner arithmetic after the forwards, srl/algorithms/r2d2/r2d2.py:152-209 and the per-sequence mean of :204, in one entry point:
 *   q / q_target f32 [B][S+1][A] (online / target network over the S+1 in-sequence states), actions i32 [B][S] (0 <= a < A), mu f32 [B][S] (the acting
 *   probabilities), rewards f32 [B][S], dones u8 [B][S] (1 = the step terminated), invalid u8 [B][S+1][A] or NULL (entry t masks the policy at step t,
 *   :194-199; entry t + 1 masks the next-state selection, :177), weights f32 [B];
 *   out: target f32 [B][S]; loss f32 [1] = Huber(delta 1) of target * w against q[a] * w, mean over B S; grad_q f32 [B][S+1][A] = d loss / d q, every entry
 *   written, the last step's rows zero (:149-150); td_mean f32 [B] = mean over t of gain_t - q_t[a_t], signed (the memory takes the absolute value).
 * Per (row, step): the selecting row is the online q[t+1] with enable_double_dqn, else q_target[t+1], invalid actions at -inf, the FIRST maximum wins
 * (np.argmax); the value is q_target[t+1][argmax], unmasked; gain = reward on a terminal step, else reward + discount * value, with inverse_rescaling on the
 * value before the discount and rescaling on the gain (terminal steps too) when enable_rescale.  Walking t = S-1 .. 0: target_t = gain_t + retrace * next_td;
 * only with enable_retrace, next_td = gain_t - q_t[a_t] and retrace *= discount * (retrace_h * min(1, pi_t[a_t] / mu_t)), where pi_t is the greedy
 * distribution over the valid actions of q_t (1 / number of maxima on a maximum, 0 elsewhere); retrace starts at 1 and is never reset inside a window;
 * without enable_retrace next_td stays 0.
 * The chain of every (row, step) -- gain, both rescalings, ratio, recursion, Huber term -- runs in double, as the reference's Python floats do, and is rounded
 * to float32 on output (a row's loss term crosses to the summing launch as one float32).  Gains, argmax and pi are computed in parallel over (b, t); one
 * thread per row walks the recursion over S values in LDS.  Two launches, no scratch, no atomics: loss and TD means are summed in a fixed order and two calls
 * on the same inputs give the same bits.
 * Envelope, validated before any device call (a violation returns SRLX_ERR_INVALID and srlx_last_error() names r2d2_seq_td): B 1..SRLX_SEQ_MAX_B,
 * S 1..SRLX_SEQ_MAX_L - 1, A 1..SRLX_SEQ_MAX_A, no NULL pointer except invalid, discount and retrace_h finite and >= 0. */
int srlx_r2d2_seq_td(int64_t batch, int seq_len, int n_actions, const float *d_q, const float *d_q_target, const int32_t *d_actions, const float *d_mu,
                     const float *d_rewards, const uint8_t *d_dones, const uint8_t *d_invalid, const float *d_weights, double discount, double retrace_h,
                     int enable_retrace, int enable_double_dqn, int enable_rescale, float *d_target, float *d_loss, float *d_grad_q, float *d_td_mean,
                     void *stream);

/* ---- R2D2 lane sequence ring (srlx_seqstore.hip) ------------------------------------------------------------------------------------------------------------
 * The actor side and the sequence replay of E lock-stepped R2D2 lanes (device/sequence_store.py: R2D2LaneStore; device/r2d2.py).  Three stateless entry points on
 * arrays the CALLER owns; no atomics, no LDS, plain vector stores, launched on the stream they are given.
 *
 * srlx_r2d2_policy: per row e, funcs.calc_epsilon_greedy_probs followed by funcs.random_choice_by_probs (srl/rl/functions.py:183-214, r2d2.py:283-291), in
 * double as the reference's Python floats.  q f32 [E][A], eps f32 [E], u f64 [E] in [0, 1), invalid u8 [E][A] or NULL (a byte != 0 marks an invalid action);
 * out: actions i32 [E], mu f32 [E].  Over the valid actions: q_max and n_max compare the float32 values; p_a = eps / n_valid, plus (1 - eps) / n_max on a
 * maximum; total = sum of p_a in action order; r = u * total; the action is the first valid a with r <= acc (acc the running sum in action order);
 * mu = (float)p_a.  Two departures from the reference: invalid actions (weight 0) are skipped by the walk (the reference returns action 0 at u = 0 whether or
 * not it is valid), and a row with no valid action yields action 0 and mu 1 (the reference divides by zero).  One work-item per row.
 * Envelope: n_envs 1..SRLX_SEQ_MAX_LANES, n_actions 1..SRLX_SEQ_MAX_A, no NULL pointer but invalid.
 *
 * The ring, position t of all lanes in row t % T:
 *   ring_frames  f32 [T][E][frame_stride]: the observation o_p of (position, lane); frame_stride >= frame_elems, a multiple of 4 floats for 16-byte rows
 *   ring_scalars i32 [T][E][8]: action i32, mu f32, reward f32, done i32 (0 / 1), age i32, three zero dwords: the transition that led INTO o_p (done = the
 *                step terminated); age = steps since the lane's episode began, 0 on the episode's first observation
 *   ring_invalid u8  [T][E][A]: the invalid-action mask OF o_p
 *   ring_hidden  f32 [T][E][2][H]: h, c as they were BEFORE the network consumed o_p
 * srlx_r2d2_lane_push writes position t of all E lanes in one launch: frames f32 [E][frame_elems], action i32 [E], mu / reward f32 [E], done u8 [E], invalid u8
 * [E][A] (NULL: none), h / c f32 [E][H], first u8 [E].  A lane with first[e] != 0 (and every lane at t = 0) delivers an episode's first observation: the entry
 * keeps the frame AND the invalid mask and otherwise reads like the padding before an episode -- a keyed pad action, mu = (float)(1.0 / A), reward 0, done 0,
 * zero recurrent state, age 0.  Every other lane gets age = age[t - 1] + 1, read from the ring.
 * srlx_r2d2_lane_gather turns B descriptors (i64 [B][3]: lane e, absolute position t of the window's last real entry, flush offset k in 0..S-1) into the tensors
 * of r2d2.SequenceBatch (L = burnin + S + 1): states f32 [B][L][frame_elems], actions i32 [B][S], probs / rewards f32 [B][S], dones u8 [B][S], invalid u8
 * [B][S+1][A], h / c f32 [B][H].  Entry l of window (e, t, k) is lane position p = t - (L - 1) + l + k:
 *   p > t               (after the end)            zero frame; pad action, mu (float)(1.0 / A), reward 0, done 1; no invalid action
 *   t - p > age[t][e]   (before the episode start) zero frame; pad action, mu (float)(1.0 / A), reward 0, done 0; no invalid action; at l = 0 zero recurrent state
 *   otherwise           the ring's entry of position p (an episode's first position carries its pad transition, real frame and real mask from the push)
 * with pad action = rng_u64(seed, e, p) % A (the key of the Agent57 ring).  The S transition fields are entries L-S..L-1, the S + 1 masks entries L-S-1..L-1, and
 * (h, c) are entry 0's.  A descriptor outside e in [0, E), t >= 0, 0 <= k < S reads nothing and yields zeros.  A position is reduced mod T only once it is
 * known to be >= 0.  That position p is still in the ring is the caller's ledger's business; a stale one reads other data, never other memory.
 * Rows move as 16-byte accesses when frame_elems and frame_stride are multiples of 4 and both frame pointers are 16-byte aligned, as dwords otherwise (per
 * launch); several loads are in flight before the first store.  Envelope, validated before any device call (SRLX_ERR_INVALID, srlx_last_error() names the entry
 * point): B, L, S, A, H, frame_elems, frame_stride as srlx_seq_gather; E 1..SRLX_SEQ_MAX_LANES; T >= L (push: >= 2) with T * E <= 2^31-1; t >= 0; no NULL
 * pointer but push's invalid. */
int srlx_r2d2_policy(int64_t n_envs, int64_t n_actions, const float *d_q, const float *d_eps, const double *d_u, const uint8_t *d_invalid, int32_t *d_actions,
                     float *d_mu, void *stream);
int srlx_r2d2_lane_push(int64_t E, int64_t A, int64_t H, int64_t frame_elems, int64_t frame_stride, int64_t T, int64_t t, uint64_t seed, const float *d_frames,
                        const int32_t *d_action, const float *d_mu, const float *d_reward, const uint8_t *d_done, const uint8_t *d_invalid, const float *d_h,
                        const float *d_c, const uint8_t *d_first, float *d_ring_frames, int32_t *d_ring_scalars, uint8_t *d_ring_invalid, float *d_ring_hidden,
                        void *stream);
int srlx_r2d2_lane_gather(int64_t B, int64_t L, int64_t S, int64_t A, int64_t H, int64_t E, int64_t T, int64_t frame_elems, int64_t frame_stride, uint64_t seed,
                          const int64_t *d_desc, const float *d_ring_frames, const int32_t *d_ring_scalars, const uint8_t *d_ring_invalid,
                          const float *d_ring_hidden, float *d_states, int32_t *d_actions, float *d_probs, float *d_rewards, uint8_t *d_dones, uint8_t *d_invalid,
                          float *d_h, float *d_c, void *stream);

/* ---- Discrete soft actor-critic on flat observations (srlx_sacd.hip; srl/algorithms/sac/sac_tf_discrete.py:158-243) -----------------------------
 * Five MLPs in float32, torch layouts ([out][in] weights): the policy  state [D] -> n_policy x (Linear + ReLU) -> Linear(A)  and, four times (q1 online, q1
 * target, q2 online, q2 target), the Q-network  concat(state [D], one-hot action [A]) -> n_q x (Linear + ReLU) -> Linear(1).
 * Envelope, validated before any device call (SRLX_ERR_INVALID; srlx_last_error() names the entry point): D 1..256, A 2..16, each block 1..3 layers of 32..512
 * units in multiples of 32, max_batch 1..256.  Every tensor is float32; every sum accumulates in float64 and is rounded to float32 once.
 *   srlx_sacd_scratch_floats : floats of device scratch a handle of this shape owns; -1 outside the envelope.  Host arithmetic.
 *   srlx_sacd_bind           : the parameter tensors by address, each network as (weight, bias) per layer in state-dict order, the networks in the order policy,
 *                              q1 online, q1 target, q2 online, q2 target: 2 (n_policy + 1) + 4 * 2 (n_q + 1) pointers; and log_alpha (one float).
 *   srlx_sacd_bind_grads     : the caller's gradient tensors of policy, q1 online, q2 online (same order and shapes) and of log_alpha.  Every update writes
 *                              them before its Adam step reads them.
 *   srlx_sacd_bind_adam      : exp_avg / exp_avg_sq of policy, q1 online, q2 online and, as the last entry, log_alpha; the optimiser steps already taken
 *                              (host int64 [4]: policy, q1, q2, alpha; the handle counts on from there, srlx_sacd_steps reads them); torch's Adam
 *                              (srlx_adam_math.h).  Binding again restarts an optimiser from the counts given.
 *   srlx_sacd_update         : the whole update of one batch in five launches (states / next states f32 [B][D], actions i32 [B], rewards f32 [B], dones u8 [B]):
 *                                0. alpha = expf(log_alpha), one value for the whole call
 *                                1. y = r + (1 - done) discount sum_a p'[a] (min(q1_target, q2_target)(s', e_a) - alpha logp'[a]),  logp' = z' - logsumexp(z')
 *                                2. q1, q2: loss = mean_b (y - q(s, e_a_b))^2, one Adam step each at lr_q
 *                                3. qv[a] = min(q1, q2)(s, e_a) after step 2; p = softmax(policy(s)), L = log(clip(p, 1e-7, 1)), entropy = -sum_a p L,
 *                                   policy_loss = mean_b sum_a p (alpha L - qv); gradient through p and L, none where the clip is active; Adam at lr_policy
 *                                4. auto_scale: alpha_loss = -mean_b(alpha (target_entropy - entropy_b)) = d alpha_loss / d log_alpha; Adam at lr_alpha
 *                                5. hard_sync: target = online; otherwise target = (float)(1 - tau) * target + (float)tau * online, two products and one add
 *                              Outputs: y, q1, q2, entropy f32 [B]; scalars f32 [5] = q1_loss, q2_loss, policy_loss, alpha_loss (0 without auto_scale), alpha.
 *                              No atomics, every sum in a fixed order: equal inputs give equal bits.
 *   srlx_sacd_forward        : n rows of states -> logits f32 [n][A] (NULL: not wanted) and min(q1, q2)(s, e_a) f32 [n][A] (NULL: not wanted) of the online
 *                              (target = 0) or the target (1) Q-networks.  Needs srlx_sacd_bind only. */
typedef struct srlx_sacd srlx_sacd_t;
int64_t srlx_sacd_scratch_floats(int obs_dim, int n_actions, int n_policy, const int *policy_widths, int n_q, const int *q_widths, int64_t max_batch);
int srlx_sacd_create(srlx_sacd_t **out, int obs_dim, int n_actions, int n_policy, const int *policy_widths, int n_q, const int *q_widths, int64_t max_batch,
                     int device);
int srlx_sacd_destroy(srlx_sacd_t *h);
int srlx_sacd_bind(srlx_sacd_t *h, float *const *d_params, float *d_log_alpha);
int srlx_sacd_bind_grads(srlx_sacd_t *h, float *const *d_grads, float *d_grad_log_alpha);
int srlx_sacd_bind_adam(srlx_sacd_t *h, float *const *d_exp_avg, float *const *d_exp_avg_sq, const int64_t *steps_taken, double beta1, double beta2, double eps);
int srlx_sacd_steps(const srlx_sacd_t *h, int64_t *steps_taken);
int srlx_sacd_update(srlx_sacd_t *h, int64_t batch, const float *d_states, const int32_t *d_actions, const float *d_next_states, const float *d_rewards,
                     const uint8_t *d_dones, double lr_policy, double lr_q, double lr_alpha, double discount, double tau, int hard_sync, int auto_scale,
                     double target_entropy, float *d_y, float *d_q1, float *d_q2, float *d_entropy, float *d_scalars, void *stream);
int srlx_sacd_forward(srlx_sacd_t *h, int64_t n, const float *d_states, int target, float *d_logits, float *d_qmin, void *stream);

/* ---- Discrete soft actor-critic: the device engine's two launches outside the update (srlx_sacd.hip) --------------------------------------------
 *   srlx_sacd_act        : the Worker's policy() (algorithms/sac.py:334-338) for n_rows lanes in ONE launch.  Row r is the D floats at d_obs_base +
 *                          d_row_offsets[r] (offsets in floats, as srlx_mlpq_forward takes them: the store's frame table at window 1; NULL: + r * D).
 *                          U[r * A + a] is the value srlx_rng_uniform(seed, *d_counter, n_rows * A, .) would write at that index; *d_counter is read, not
 *                          advanced.  While *d_counter < random_until: action = min(A - 1, (int)floor(U[r * A] * A)).  Otherwise, in float64:
 *                          u = 1e-6 + (1 - 1e-6) U, score_a = (double)z_a - log(-log(u)), action = the FIRST maximum.  The logits z are the policy's, bit for
 *                          bit what srlx_sacd_forward(target = 0) writes for the same rows.  d_logits f32 [n_rows][A] and d_scores f64 [n_rows][A] are
 *                          optional (NULL) and, when asked for, written in both phases; with neither, the random phase does not run the network.  Needs
 *                          srlx_sacd_bind only and no scratch sized by max_batch.  No atomics: equal inputs give equal bits.  Envelope, validated before
 *                          any device call (SRLX_ERR_INVALID; srlx_last_error() names sacd_act): a bound handle, n_rows 1..65536, random_until >= 0,
 *                          non-NULL d_obs_base, d_counter and d_actions.
 *   srlx_sacd_ring_batch : the items of a draw as srlx_sacd_update's tensors, stateless, ONE launch.  Inputs as srlx_per_sample_gather_train /
 *                          srlx_store_gather_train write them at window 1, n-step 1: offsets i64 [B][2] (s, s'; in floats), actions i32 [B], rewards and
 *                          terminated f32 [B].  Outputs: states and next states f32 [B][D], one-hot actions f32 [B][A] (exact 0 / 1), done u8 [B]
 *                          (terminated != 0).  d_rewards is already the update's [B] tensor: required, not copied.  Rows move as 16-byte accesses when D is a
 *                          multiple of 4 and the base pointers and the item's offsets are 16-byte aligned.  Envelope: B 1..256, D 1..256, A 2..16, no NULL
 *                          pointer (srlx_last_error() names sacd_ring_batch). */
int srlx_sacd_act(srlx_sacd_t *h, int64_t n_rows, const float *d_obs_base, const int64_t *d_row_offsets, uint64_t seed, const int64_t *d_counter,
                  int64_t random_until, int32_t *d_actions, float *d_logits, double *d_scores, void *stream);
int srlx_sacd_ring_batch(int64_t B, int D, int A, const float *d_obs_base, const int64_t *d_offsets, const int32_t *d_actions, const float *d_rewards,
                         const float *d_terminated, float *d_states, float *d_next_states, float *d_onehot, uint8_t *d_done, void *stream);

/* ---- V-PPO on flat observations (srlx_vppo.hip; srl/algorithms/ppo_v/torch_model.py:111-178) ----------------------------------------------------
 * One actor-critic MLP in float32, torch layouts ([out][in] weights): a trunk  state [D] -> n_trunk x (Linear + ReLU)  (input value block + hidden block), a value
 * branch  n_value x (Linear + ReLU) -> Linear(1)  and a policy branch  n_policy x (Linear + ReLU) -> the head: head = 0 categorical, Linear(n_out) logits;
 * head = 1 Normal, Linear(n_out) locs and Linear(n_out) log-scales.  K = 1 (categorical) or n_out (Normal) log-probabilities per row, N = B K.
 * Envelope, validated before any device call (SRLX_ERR_INVALID; srlx_last_error() names the entry point): D 1..256, trunk 1..3 layers, value and policy block
 * 0..2 layers each, every layer 32..512 units in multiples of 32, categorical n_out 2..16, Normal n_out 1..8, max_batch 1..256.  Every tensor is float32; every
 * sum over a layer's inputs or over the batch accumulates in float64 and is rounded to float32 once; a row's own arithmetic is float32 (srlx_vppo_math.h).
 *   srlx_vppo_scratch_floats : floats of device scratch a handle of this shape owns; -1 outside the envelope.  Host arithmetic.
 *   srlx_vppo_bind           : the parameter tensors by address in state-dict order: (weight, bias) of every trunk layer, every value-block layer, the value
 *                              out layer, every policy-block layer, the head (logits; or locs, then log-scales): 2 (n_trunk + n_value + 1 + n_policy + 1 or 2).
 *   srlx_vppo_bind_grads     : the caller's gradient tensors (same order and shapes), twice: d_grads receives the gradients after the norm clip (what Adam
 *                              reads, torch's p.grad after clip_grad_norm_), d_raw_grads the gradients before it.  Every update writes both.
 *   srlx_vppo_bind_adam      : exp_avg / exp_avg_sq (same order) and the optimiser steps already taken (the handle counts on from there, srlx_vppo_steps
 *                              reads the count; -1 on a NULL handle); torch's Adam (srlx_adam_math.h).  Binding again restarts the optimiser from that count.
 *   srlx_vppo_update         : the whole step of one batch in three launches.  Inputs: states / next states f32 [B][D]; actions i32 [B] (categorical) or f32
 *                              [B][K] (Normal, the value before tanh); old log-probabilities f32 [B][K]; rewards, not-terminated, total rewards f32 [B].
 *                                1. v = value(s), n_v = value(s'); q = r + (not_terminated discount) n_v; adv = q - v (a constant)
 *                                2. categorical: p = softmax(logits), lp = log(clamp(p_a, 1e-7, 1)); gradient d lp / d logit_k = (k == a) - p_k where
 *                                   p_a >= 1e-7, none below.  Normal: ls = clamp(raw log-scale, log_scale_lo, log_scale_hi) (gradient on the closed interval),
 *                                   u = (a_j - loc_j) / exp(ls_j), lp_j = -0.5 log(2 pi) - ls_j - 0.5 u^2, and with `squashed` every lp_j loses
 *                                   sum_i log(clamp(1 - tanh(a_i)^2, 1e-10, 1)) (float64; constant in the parameters)
 *                                3. ratio_j = exp(lp_j - old_j) (a constant in the value losses)
 *                                4. loss_value = mean_N huber_1(ratio_j q - v), loss_v_align = mean_N (ratio_j total_reward - v)^2; v is the target argument
 *                                   and takes the gradient: -(d) or -sign(d), and -2 (ratio_j total_reward - v)
 *                                5. loss_policy = -mean_N min(ratio_j adv, clamp(ratio_j, (float)(1 - clip), (float)(1 + clip)) adv); d / d ratio_j = adv on
 *                                   the closed interval and where ratio_j adv is the smaller product, 0 elsewhere
 *                                6. entropy_weight > 0: loss_e = mean_B sum_j exp(lp_j) lp_j, gradient (exp(lp_j) lp_j + exp(lp_j)) / B; otherwise loss_e = 0
 *                                7. loss = loss_value + loss_align_coeff loss_v_align + loss_policy + entropy_weight loss_e; every parameter gradient is a
 *                                   sum over the batch in row order (d_raw_grads)
 *                                8. norm = sqrt(sum of all squared gradient entries) (float64 sum, float32 result); coef = min(1, max_grad_norm /
 *                                   (norm + 1e-6)) in float32; d_grads = d_raw_grads * coef, always
 *                                9. one Adam step at lr on d_grads
 *                              Outputs: v, n_v f32 [B]; new_logpi f32 [B][K]; scalars f32 [5] = loss_value, loss_v_align, loss_policy, loss_e, norm.
 *                              No atomics, every sum in a fixed order: equal inputs give equal bits.
 *   srlx_vppo_forward        : n rows of states -> v f32 [n] (NULL: not wanted) and the head's outputs (NULL: not wanted): d_head0 f32 [n][n_out] logits
 *                              or locs, d_head1 f32 [n][n_out] the log-scales clamped to [log_scale_lo, log_scale_hi] (Normal only, and then required with
 *                              d_head0).  The same chains as the update's: v bit for bit what srlx_vppo_update writes for the same rows.  Needs
 *                              srlx_vppo_bind only. */
typedef struct srlx_vppo srlx_vppo_t;
int64_t srlx_vppo_scratch_floats(int obs_dim, int head, int n_out, int n_trunk, const int *trunk_widths, int n_value, const int *value_widths, int n_policy,
                                 const int *policy_widths, int64_t max_batch);
int srlx_vppo_create(srlx_vppo_t **out, int obs_dim, int head, int n_out, int n_trunk, const int *trunk_widths, int n_value, const int *value_widths, int n_policy,
                     const int *policy_widths, int64_t max_batch, int device);
int srlx_vppo_destroy(srlx_vppo_t *h);
int srlx_vppo_bind(srlx_vppo_t *h, float *const *d_params);
int srlx_vppo_bind_grads(srlx_vppo_t *h, float *const *d_grads, float *const *d_raw_grads);
int srlx_vppo_bind_adam(srlx_vppo_t *h, float *const *d_exp_avg, float *const *d_exp_avg_sq, int64_t steps_taken, double beta1, double beta2, double eps);
int64_t srlx_vppo_steps(const srlx_vppo_t *h);
int srlx_vppo_update(srlx_vppo_t *h, int64_t batch, const float *d_states, const float *d_next_states, const void *d_actions, const float *d_old_logpi,
                     const float *d_rewards, const float *d_not_terminated, const float *d_total_rewards, double lr, double discount, double clip_range,
                     double entropy_weight, double loss_align_coeff, double max_grad_norm, int squashed, double log_scale_lo, double log_scale_hi, float *d_v,
                     float *d_n_v, float *d_new_logpi, float *d_scalars, void *stream);
int srlx_vppo_forward(srlx_vppo_t *h, int64_t n, const float *d_states, double log_scale_lo, double log_scale_hi, float *d_v, float *d_head0, float *d_head1,
                      void *stream);

/* ---- V-PPO: the device engine's launches outside the update (srlx_vppo.hip, srlx_vppo_lanes.hip) -------------------------------------------------
 *   srlx_vppo_act : the Worker's policy() (algorithms/ppo_v.py, discrete branch, training) for n_rows lanes in ONE launch, on a categorical handle; needs
 *                   srlx_vppo_bind only.  Rows are dense f32 [n_rows][D].  The pass is trunk and policy branch (the Worker throws v away); a row's logits are
 *                   bit for bit what srlx_vppo_forward writes into d_head0 for the same rows, whatever rows share a workgroup.
 *                   U0 = u53(rng_u64(seed, *d_counter, 2 r)), U1 = u53(rng_u64(seed, *d_counter, 2 r + 1)) (what srlx_rng_uniform writes at those indices);
 *                   *d_counter is read, not advanced.
 *                     U0 < epsilon : a = min(A - 1, (int)floor(U1 A)), logp = (float)log(1.0 / A)
 *                     otherwise    : float64 w_k = exp((double)z_k - max z), c_k the running sum in action order, a = the first k with U1 c_{A-1} < c_k
 *                                    (A - 1 if rounding leaves none); logp = the update's own float32 form, log(clamp(softmax(z)_a, 1e-7, 1)) -- with unchanged
 *                                    parameters srlx_vppo_update's new_logpi equals it to the bit.  Not floored at log(1e-6): the store's push does that.
 *                   Outputs: d_actions i32 [n], d_logp f32 [n]; optional (NULL): d_logits f32 [n][A], d_cdf f64 [n][A] (the c_k).  No atomics.
 *                   Envelope, validated before any device call (SRLX_ERR_INVALID; srlx_last_error() names vppo_act): a bound categorical handle, n_rows
 *                   1..65536, epsilon in [0, 1], non-NULL d_obs, d_counter, d_actions, d_logp.
 * The episode store: a tracking ring [R][E] (R = max_episode_steps + 2; row p = the observation each lane acted on at lock-step p with that step's action,
 * log-probability, reward, not-terminated, done; s' of row p is row p + 1; per lane the running episode length and the needs_reset byte) and an item ring of
 * `capacity` items (s, s', action, old log-probability, reward, not-terminated, total reward) in which the item with sequence number q lives in slot
 * q % capacity, as ReplayBuffer.add leaves it.  Envelope of create: lanes 1..4096, D 1..256, max_episode_steps 1..4094, capacity 1..2^24, discount in [0, 1].
 *   srlx_vppo_lanes_reset  : empties both structures and takes the lanes' first observations f32 [E][D] as row 0.
 *   srlx_vppo_lanes_push   : one lock-step, TWO launches (the close places a lane's items behind those of the closing lanes before it, so it reads every
 *                            lane's length and done flag: a launch boundary orders that behind all lanes' stores).  Inputs: actions i32 [E], log-probabilities
 *                            f32 [E] (floored at (float)log(1e-6) here), rewards f32 [E], terminated and done u8 [E], next observations f32 [E][D] (into row
 *                            p + 1).  A lane whose needs_reset byte is set stores nothing: the lock-step only delivers its new first observation.  needs_reset
 *                            becomes done; *d_policy_counter (NULL: none) gains 1.  Every lane whose step was done closes its episode of n steps: walking them
 *                            backwards, total = reward + discount * total in float64, one chain in the Worker's order, rounded to float32 at the store; the n
 *                            items are appended in that reversed order, the closing lanes in lane order.  Of the S items a lock-step adds only the last
 *                            `capacity` are written (what a sequential ring would hold).  A lane that stores more than max_episode_steps steps without
 *                            closing sets the sticky error word (srlx_vppo_lanes_count) and drops them; the rest of that episode is dropped too (the lane's
 *                            length reads -1 until its next first observation), so no item with a return cut short reaches the ring.  No atomics.
 *   srlx_vppo_lanes_sample : `batch` (1..256, <= capacity) distinct slots uniformly from [0, N), N = min(capacity, added), by Floyd's algorithm: for
 *                            i = 0..batch-1, j = N - batch + i, t = min(j, (int64)floor(U_i (j + 1))), U_i = u53(rng_u64(seed, draw, i)) with `draw` the
 *                            number of samples since the reset; take t, or j if t is already chosen.  Then the items as srlx_vppo_update's dense tensors:
 *                            states and next states f32 [B][D], actions i32 [B], old log-probabilities, rewards, not-terminated, total rewards f32 [B], and the
 *                            slots i64 [B].  Two launches; rows move as 16-byte accesses where D % 4 == 0.  N < batch sets the error word to 2.
 *   srlx_vppo_lanes_count  : synchronises `stream` and reads the item count (items ever added) and the error word.
 *   srlx_vppo_lanes_views  : device pointers for tests and the engine: 0 obs ring, 1 action, 2 logp, 3 reward, 4 not-terminated, 5 done, 6 lengths, 7
 *                            needs_reset, 8 item s, 9 item s', 10 item action, 11 item logp, 12 item reward, 13 item not-terminated, 14 item total, 15 the
 *                            two count words; and the current row.
 *   srlx_vppo_lanes_read   : synchronises `stream` and copies one whole view (numbered as above) to host memory; `bytes` must be the view's size. */
int srlx_vppo_act(srlx_vppo_t *h, int64_t n_rows, const float *d_obs, uint64_t seed, const int64_t *d_counter, double epsilon, int32_t *d_actions, float *d_logp,
                  float *d_logits, double *d_cdf, void *stream);
typedef struct srlx_vppo_lanes srlx_vppo_lanes_t;
int srlx_vppo_lanes_create(srlx_vppo_lanes_t **out, int64_t n_lanes, int obs_dim, int64_t max_episode_steps, int64_t capacity, double discount, int device);
int srlx_vppo_lanes_destroy(srlx_vppo_lanes_t *h);
int srlx_vppo_lanes_reset(srlx_vppo_lanes_t *h, const float *d_first_obs, void *stream);
int srlx_vppo_lanes_push(srlx_vppo_lanes_t *h, const int32_t *d_actions, const float *d_logp, const float *d_rewards, const uint8_t *d_terminated, const uint8_t *d_done,
                         const float *d_next_obs, int64_t *d_policy_counter, void *stream);
int srlx_vppo_lanes_sample(srlx_vppo_lanes_t *h, int64_t batch, uint64_t seed, float *d_states, float *d_next_states, int32_t *d_actions, float *d_old_logpi,
                           float *d_rewards, float *d_not_terminated, float *d_total_rewards, int64_t *d_slots, void *stream);
int srlx_vppo_lanes_count(srlx_vppo_lanes_t *h, int64_t *added, int32_t *error, void *stream);
int srlx_vppo_lanes_views(srlx_vppo_lanes_t *h, void **views, int64_t *current_row);
int srlx_vppo_lanes_read(srlx_vppo_lanes_t *h, int view, int64_t bytes, void *host_dst, void *stream);

/* ---- V-PPO: the device engine on the Normal head (srlx_vppo.hip, srlx_vppo_lanes.hip) --------------------------------------------------------------
 *   srlx_vppo_act_normal : the Worker's policy() (algorithms/ppo_v.py, NpArraySpace branch, training) for n_rows lanes in ONE launch, on a Normal handle of K
 *                   action elements; needs srlx_vppo_bind only.  Rows are dense f32 [n_rows][D].  The pass is trunk and policy branch; a row's loc and clamped
 *                   log-scale are bit for bit what srlx_vppo_forward writes into d_head0 / d_head1, whatever rows share a workgroup.
 *                   Row r reads 2 K + 1 keyed uniforms u53(rng_u64(seed, *d_counter, i)): U0 at i = (2 K + 1) r; for element j, Ua at i + 1 + 2 j and Ub at
 *                   i + 2 + 2 j.  *d_counter is read, not advanced.  z_j = sqrt(-2 log(1 - Ua)) cos(2 pi Ub) in float64.
 *                     U0 < epsilon : loc_j = 0, sd_j = (float)noise_scale, ls_j = (float)log(noise_scale), for every element of the row
 *                     otherwise    : loc_j the head's loc, ls_j its log-scale clamped to [log_scale_lo, log_scale_hi], sd_j = expf(ls_j)
 *                   a_j = (float)((double)loc_j + (double)sd_j z_j), the value BEFORE tanh.  logp_j is the update's own float32 form from the stored a_j:
 *                   u = (a_j - loc_j) / sd_j, (-0.5 log(2 pi) - ls_j - 0.5 u u) - corr, corr the row's float64 sum of log(clamp(1 - tanh(a_i)^2, 1e-10, 1))
 *                   when `squashed`, else 0 -- on the policy branch, with unchanged parameters, srlx_vppo_update's new_logpi equals it to the bit on every
 *                   element.  Not floored at log(1e-6): the store's push does that.  The environment's action, float64 rounded to float32 and then clipped to
 *                   [low_j, high_j]: low_j + (x + 1) / 2 (high_j - low_j) with x = tanh(a_j) when squashed, x = a_j when plain.
 *                   Outputs: d_actions, d_logp, d_env_actions f32 [n][K]; optional (NULL): d_loc and d_log_scale f32 [n][K] (the head's, together), d_z f64
 *                   [n][K].  d_low / d_high: f32 [K] device arrays.  No atomics.
 *                   Envelope, validated before any device call (SRLX_ERR_INVALID; srlx_last_error() names vppo_act_normal): a bound Normal handle, n_rows
 *                   1..65536, epsilon in [0, 1], noise_scale positive and finite, squashed 0 or 1, ordered clamp ends, non-NULL required pointers.
 *   srlx_vppo_lanes_create_normal / _push_normal / _sample_normal : the episode store above with K = action_dim (1..8) float32 action elements and K
 *                   log-probabilities per step: the tracking ring's action and log-probability views are [R][E][K], the item ring's [capacity][K]; push
 *                   takes actions and log-probabilities f32 [E][K] and floors EACH log-probability at (float)log(1e-6); sample writes actions and old
 *                   log-probabilities f32 [B][K].  Everything else -- the ring, needs_reset, the two launches, the float64 return chain, the count, S >
 *                   capacity, the sticky error, Floyd's draw, count / views / read -- is the categorical store's, one set of kernels.  Each kind of handle
 *                   refuses the other kind's push and sample (SRLX_ERR_INVALID).
 *   srlx_pendulum_lane_step : Pendulum-v1 (envs/pendulum.py) for E lanes under srlx_cartpole_step's contract: float64 state [E][2] (th, thdot), steps and
 *                   episodes i32 [E], torques f32 [E]; outputs obs f32 [E][3] (cos th, sin th, thdot), reward, terminated (always 0), done (steps >=
 *                   max_steps).  The step is envs/pendulum.py:step in float64, line for line (the reward from the state before the step).  A lane whose
 *                   needs_reset byte is set only receives its next episode's first observation: th = -pi + 2 pi U_0, thdot = -1 + 2 U_1, U_k =
 *                   u53(rng_u64(seed ^ 0x50454E44554C554D, lane << 32 | episode, k)); its reward, terminated and done read 0.  NULL torques (or NULL
 *                   needs_reset) reset every lane; the scalar outputs may then be NULL. */
int srlx_vppo_act_normal(srlx_vppo_t *h, int64_t n_rows, const float *d_obs, uint64_t seed, const int64_t *d_counter, double epsilon, double noise_scale, int squashed,
                         double log_scale_lo, double log_scale_hi, const float *d_low, const float *d_high, float *d_actions, float *d_logp, float *d_env_actions,
                         float *d_loc, float *d_log_scale, double *d_z, void *stream);
int srlx_vppo_lanes_create_normal(srlx_vppo_lanes_t **out, int64_t n_lanes, int obs_dim, int64_t max_episode_steps, int64_t capacity, double discount, int action_dim,
                                  int device);
int srlx_vppo_lanes_push_normal(srlx_vppo_lanes_t *h, const float *d_actions, const float *d_logp, const float *d_rewards, const uint8_t *d_terminated,
                                const uint8_t *d_done, const float *d_next_obs, int64_t *d_policy_counter, void *stream);
int srlx_vppo_lanes_sample_normal(srlx_vppo_lanes_t *h, int64_t batch, uint64_t seed, float *d_states, float *d_next_states, float *d_actions, float *d_old_logpi,
                                  float *d_rewards, float *d_not_terminated, float *d_total_rewards, int64_t *d_slots, void *stream);
int srlx_pendulum_lane_step(int64_t n_envs, double *d_state, int32_t *d_steps, int32_t *d_episodes, const uint8_t *d_needs_reset, const float *d_torques,
                            int64_t max_steps, uint64_t seed, float *d_obs, float *d_reward, uint8_t *d_terminated, uint8_t *d_done, void *stream);

/* ---- NoT_SAC on flat observations (srlx_notsac.hip; srl/algorithms/sac_not/torch_model.py:131-191) -------------------------------------------------
 * A handle is one shape: observations of obs_dim (1..256) floats; head 0 = Gumbel with n_out (2..16) actions, head 1 = Normal with n_out (1..8) action elements;
 * a policy block and a q block of 1..3 ReLU layers of 32..512 units in multiples of 32 each; act_emb_units (32..512 in multiples of 32) with obs_dim +
 * act_emb_units <= 512 (the concatenated row is the widest row in LDS); max_batch 1..256.  Everything else is refused at create.  Tensors stay float32; every
 * sum over a layer's inputs or over the batch accumulates in float64 and is rounded to float32 once; exp, tanh, SiLU, softmax and the Gumbel transform are
 * evaluated in float64 (srlx_notsac_math.h).  No atomics: equal inputs give equal bits, and a row's outputs do not depend on the rows that share its workgroup
 * (by default an update runs one row per workgroup; see srlx_notsac_set_rows_per_workgroup).
 *   srlx_notsac_scratch_floats : floats of device scratch a handle of this shape owns; -1 outside the envelope.  Host arithmetic.
 *   srlx_notsac_bind           : the parameter tensors by address, n_tensors of them: the policy's in parameters() order ((weight, bias) of every policy-block
 *                                layer, then of the head's Linear: logits, or locs and then log-scales), then the Q-network's ((weight, bias) of act_block's
 *                                Linear [E][n_out], of every q-block layer -- the first reads obs_dim + E inputs -- and of q_out).  A count that is not the
 *                                shape's is refused and leaves the handle as it was.
 *   srlx_notsac_bind_grads     : the caller's gradient tensors (same order and shapes), twice: d_grads receives the gradients after their network's norm clip
 *                                (what Adam reads), d_raw_grads those before it.
 *   srlx_notsac_bind_adam      : exp_avg / exp_avg_sq (same order) and the optimiser steps already taken by BOTH optimisers (the handle counts on from there,
 *                                srlx_notsac_steps reads the count).
 *   srlx_notsac_update         : the whole step of one batch in six launches, nothing synchronises.  Inputs: states / next states f32 [B][D]; actions i32 [B]
 *                                (Gumbel: the index of the stored one-hot's maximum) or f32 [B][K] (Normal: as stored, after tanh when squashed); rewards,
 *                                not_terminated, total_rewards f32 [B]; noise f32 [2][B][n_out]: standard normals (Normal) or uniforms in [0, 1) (Gumbel), plane
 *                                0 for the target's next action, plane 1 for the policy step.
 *                                  a' = tanh(loc(s') + exp(clamp(ls(s'))) e0) (no tanh unless squashed), or the one-hot of the first maximum of logits(s') +
 *                                  gumbel(u0), gumbel(u) = -log(-log(u + 1e-6) + 1e-6);  target = r + not_terminated * discount * Q(s', a');
 *                                  loss_q = mean Huber(target - Q(s, a)), loss_q_align = mean (total_reward - Q(s, a))^2, both with their gradient on Q(s, a);
 *                                  the Q-network's gradient of loss_q + loss_align_coeff * loss_q_align, its norm, clip_grad_norm_(max_grad_norm), Adam(lr);
 *                                  a = the same sample from the policy on s with plane 1, or softmax(logits(s) + gumbel(u1));
 *                                  loss_policy = -mean Q(s, a) through the Q-network ALREADY STEPPED; the policy's gradient (the log-scale's is zero outside
 *                                  the clamp's closed interval), its norm, the clip, Adam(lr).
 *                                Outputs: q, target_q f32 [B]; next_action, pi_action f32 [B][n_out]; scalars f32 [5] = loss_q, loss_q_align, loss_policy, the
 *                                Q-network's and the policy's gradient norm before their clips.
 *   srlx_notsac_set_rows_per_workgroup : the launch shape of the row kernels and of srlx_notsac_forward: 1, 2, 4, 8 or 16 rows per workgroup, or 0 for the
 *                                default: the smallest of those that keeps the launch within 256 workgroups, which is 1 for every update (B <= 256) and more
 *                                only for a forward call of more than 256 rows.  It changes the launch shape and never a bit (tests/test_notsac_gpu.py holds
 *                                updates at 16 rows per workgroup to the bits of the default); there for measurements and tests.
 *   srlx_notsac_forward        : n rows of states -> the head's outputs (NULL: not wanted): d_head0 f32 [n][n_out] logits or locs, d_head1 the CLAMPED
 *                                log-scales (Normal only); and, for d_actions f32 [n][n_out] (one-hot or soft rows on the Gumbel head), d_q f32 [n] = Q(s, a)
 *                                (both NULL: not wanted).  The same chains as the update's.  Needs srlx_notsac_bind only. */
typedef struct srlx_notsac srlx_notsac_t;
int64_t srlx_notsac_scratch_floats(int obs_dim, int head, int n_out, int n_policy, const int *policy_widths, int n_q, const int *q_widths, int act_emb_units,
                                   int64_t max_batch);
int srlx_notsac_create(srlx_notsac_t **out, int obs_dim, int head, int n_out, int n_policy, const int *policy_widths, int n_q, const int *q_widths, int act_emb_units,
                       int64_t max_batch, int device);
int srlx_notsac_destroy(srlx_notsac_t *h);
int srlx_notsac_bind(srlx_notsac_t *h, int n_tensors, float *const *d_params);
int srlx_notsac_bind_grads(srlx_notsac_t *h, int n_tensors, float *const *d_grads, float *const *d_raw_grads);
int srlx_notsac_bind_adam(srlx_notsac_t *h, int n_tensors, float *const *d_exp_avg, float *const *d_exp_avg_sq, int64_t steps_taken, double beta1, double beta2,
                          double eps);
int srlx_notsac_set_rows_per_workgroup(srlx_notsac_t *h, int rows);
int64_t srlx_notsac_steps(const srlx_notsac_t *h);
int srlx_notsac_update(srlx_notsac_t *h, int64_t batch, const float *d_states, const float *d_next_states, const void *d_actions, const float *d_rewards,
                       const float *d_not_terminated, const float *d_total_rewards, const float *d_noise, double lr, double discount, double loss_align_coeff,
                       double max_grad_norm, int squashed, double log_scale_lo, double log_scale_hi, float *d_q, float *d_target_q, float *d_next_action,
                       float *d_pi_action, float *d_scalars, void *stream);
int srlx_notsac_forward(srlx_notsac_t *h, int64_t n, const float *d_states, double log_scale_lo, double log_scale_hi, float *d_head0, float *d_head1,
                        const float *d_actions, float *d_q, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SRLX_H */
