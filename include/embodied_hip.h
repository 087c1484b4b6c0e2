/* embodied_hip.h — C ABI of libembodied_hip.so (MI355X / gfx950).
 *
 * The reference (danijar/embodied) has no FFI: its boundary is a set of
 * duck-typed Python protocols (embodied/core/base.py:1-73) implemented in numpy.
 * This library is the native layer the MI355X build puts UNDER the same Python
 * classes (embodied_amd.Driver / Replay / selectors / streams / scans).  Every
 * entry point below names the reference code whose work it takes over.
 *
 * Conventions
 *   - every function returns int32 status: 0 ok, <0 error; the message of the
 *     last error on the calling thread is emb_last_error();
 *   - no exceptions and no C++/torch types cross the ABI: plain pointers, sizes;
 *   - device pointers are caller-owned (hipMalloc / torch storage); every launch
 *     goes to the caller's `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - handles are internally locked: add / sample / update may be called from
 *     different host threads (reference: tests/test_replay.py:306-357);
 *   - "host" arrays are ordinary CPU memory, "device" arrays are HBM;
 *   - step ids are 20 bytes: 16-byte big-endian chunk uid || 4-byte big-endian
 *     row-in-chunk (embodied/core/replay.py:90-91).
 */
#ifndef EMBODIED_HIP_H_
#define EMBODIED_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with hidden visibility: what this header declares is all
 * it exports (169 functions). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* 3 (round 4): + emb_configure, emb_scan_lambda_multi, emb_replay_carry_publish,
 * emb_replay_settle; emb_replay_profile_report which = 3.  Additions only: a
 * caller written against version 2 runs unchanged.                             */
/* 4 (round 5): + emb_replay_sample_heads, emb_direct_*.  Additions only.        */
/* 5 (round 6): + emb_comm_exchange_gather, emb_direct_allgather,
 * emb_direct_exchange_gather (additions); emb_configure refuses names that are
 * no knob; a time-out inside emb_direct_* is fatal for the communicator.
 * Still 5: + emb_normalize, emb_normalize_launches, emb_ppo_targets,
 * emb_ppo_targets_launches, emb_scan_lambda_cont, emb_dreamer_targets,
 * emb_dreamer_targets_launches, emb_twohot_stats, emb_twohot_loss,
 * emb_twohot_grad, emb_twohot_launches, emb_onehot_kl, emb_onehot_kl_grad,
 * emb_onehot_kl_launches, emb_policy_loss, emb_policy_loss_grad,
 * emb_policy_loss_launches, emb_optim_table, emb_optim_norms, emb_optim_update,
 * emb_optim_metrics, emb_optim_launches, emb_norm_act, emb_norm_act_grad,
 * emb_norm_act_launches, emb_gru_gate, emb_gru_gate_grad, emb_gru_gate_launches,
 * emb_philox_uniform, emb_onehot_sample, emb_onehot_sample_grad,
 * emb_onehot_sample_launches, emb_recon_loss, emb_recon_loss_grad,
 * emb_recon_loss_launches, emb_normal_policy_loss, emb_normal_policy_loss_grad,
 * emb_normal_sample, emb_philox_normal, emb_normal_policy_launches,
 * emb_block_linear_plan, emb_stat_rows, emb_stat_rows_launches, emb_mean_fill,
 * emb_optim_grad_norms, emb_optim_adam_update, emb_slow_table, emb_slow_update,
 * emb_optim_update_slow, emb_optim_adam_update_slow, emb_pool_norm_act,
 * emb_pool_norm_act_grad, emb_norm_act_upsample, emb_norm_act_upsample_grad,
 * emb_conv_stage_launches, emb_dict_concat, emb_dict_concat_launches
 * (additions only).                                                         */
#define EMB_ABI_VERSION 5

#define EMB_OK 0
#define EMB_ERR_INVALID (-1)   /* bad argument / state                         */
#define EMB_ERR_HIP (-2)       /* a HIP runtime call failed                     */
#define EMB_ERR_EMPTY (-3)     /* sampling from an empty selector               */
#define EMB_ERR_POOL_FULL (-4) /* chunk pool exhausted: grow it and retry       */
#define EMB_ERR_NOT_FOUND (-5) /* unknown key                                   */
#define EMB_ERR_INTERNAL (-6)

#define EMB_STEPID_BYTES 20

/* dtype codes (emb_mask_actions, emb_obs_stack) */
#define EMB_U8 0
#define EMB_I8 1
#define EMB_I16 2
#define EMB_I32 3
#define EMB_I64 4
#define EMB_F16 5
#define EMB_BF16 6
#define EMB_F32 7
#define EMB_F64 8
#define EMB_BOOL 9

#define EMB_LAYOUT_SAME 0           /* (N, P, C) as stored by the envs          */
#define EMB_LAYOUT_CHANNELS_FIRST 1 /* (N, C, P)                                */

#define EMB_MODE_TRAIN 0
#define EMB_MODE_REPORT 1
#define EMB_MODE_EVAL 2

typedef struct emb_rng emb_rng_t;
typedef struct emb_tree emb_tree_t;
typedef struct emb_selector emb_selector_t;
typedef struct emb_replay emb_replay_t;

const char* emb_last_error(void);
int32_t emb_abi_version(void);

/* Tuning knobs (INTEGRATION.md lists them: EMB_SPAN_MOVER, EMB_DEFER_INDEX,
 * EMB_DEFER_MAX_GAP_US, EMB_ARGS_BAR, ...; csrc/knobs.h holds the list).  Each
 * is read once, by the first call that needs it, from emb_configure's value or
 * else from the environment variable of the same name.  emb_configure after
 * that first use is refused (EMB_ERR_INVALID): a setting is never half in
 * effect; a name that is no knob of the library is refused as well (ABI 5: a
 * retired or misspelt knob is an error, not a silent no-op).  value NULL
 * withdraws an earlier emb_configure.  The reference has no counterpart (its knobs are
 * Python config fields); this replaces "export EMB_...=" for host programs. */
int32_t emb_configure(const char* name, const char* value);
int32_t emb_device_count(int32_t* count);

/* A HIP stream whose kernels may use `n_cus` compute units only, beginning with
 * unit `first_cu` (ABI 5).  For a learner that samples / scans / writes back
 * beside the Driver's latency-bound step kernels (the reference dispatches its
 * train step asynchronously too, embodied/jax/agent.py:286-294): a sample gather
 * that fills every CU makes the step's small kernels queue behind it; confined
 * to a share of the chip it runs beside them.  The replay's movers size their
 * persistent grids by the stream's share.  The driver numbers compute units
 * round-robin over XCDs and shader engines, so a range is spread evenly.
 * emb_stream_destroy for streams made here only.                               */
int32_t emb_stream_create_on_cus(int32_t first_cu, int32_t n_cus, void** stream_out);
int32_t emb_stream_destroy(void* stream);

/* ---- numpy-compatible PRNG ------------------------------------------------
 * Replaces numpy.random.default_rng as used by selectors.py:34,42,240,305,212
 * and the per-batch seeds of embodied/jax/agent.py:405-408.  `words` is the
 * SeedSequence entropy: a Python int seed split into little-endian u32 words
 * (a list seed concatenates its elements' words).                            */
int32_t emb_rng_create(const uint32_t* words, int32_t n_words, emb_rng_t** out);
int32_t emb_rng_integers(emb_rng_t* rng, int64_t high, int64_t count, int64_t* out);
int32_t emb_rng_random(emb_rng_t* rng, int64_t count, double* out);
int32_t emb_rng_choice(emb_rng_t* rng, const double* p, int32_t k, int64_t count, int64_t* out);
int32_t emb_rng_destroy(emb_rng_t* rng);
/* ndarray.sum() of a contiguous float64 vector (pairwise), selectors.py:296. */
int32_t emb_np_sum(const double* values, int64_t n, double* out);

/* ---- SampleTree (selectors.py:231-354) ------------------------------------ */
int32_t emb_tree_create(int32_t branching, uint64_t seed, emb_tree_t** out);
int32_t emb_tree_insert(emb_tree_t* tree, int64_t key, double uprob);
int32_t emb_tree_remove(emb_tree_t* tree, int64_t key);
int32_t emb_tree_update(emb_tree_t* tree, int64_t key, double uprob);
int32_t emb_tree_sample(emb_tree_t* tree, int64_t* key);
int32_t emb_tree_len(emb_tree_t* tree, int64_t* n);
int32_t emb_tree_root_sum(emb_tree_t* tree, double* total);
/* leaf depths (root = 0) and node count incl. leaves: what the reference's
 * tests/test_sampletree.py:18-58 inspect.                                    */
int32_t emb_tree_shape(emb_tree_t* tree, int64_t cap, int64_t* depths, int64_t* n_leaves,
                       int64_t* n_nodes);
int32_t emb_tree_destroy(emb_tree_t* tree);

/* ---- selectors (selectors.py:7-228): __call__/__len__/__setitem__/__delitem__
 * /prioritize.  Item keys are int64 (Replay's itemid counter).              */
int32_t emb_selector_create_fifo(emb_selector_t** out);
int32_t emb_selector_create_uniform(uint64_t seed, emb_selector_t** out);
int32_t emb_selector_create_prioritized(double exponent, double initial, int32_t zero_on_sample,
                                        double maxfrac, int32_t branching, uint64_t seed,
                                        emb_selector_t** out);
/* members: name-sorted, zero fractions already dropped (selectors.py:205-211);
 * the mixture shares the members, which stay valid handles of their own.     */
int32_t emb_selector_create_mixture(emb_selector_t* const* members, const float* fractions,
                                    int32_t n, uint64_t seed, emb_selector_t** out);
/* Recency (embodied/core/selectors.py:60-125): age-biased draws from a b-ary
 * table of normalised block masses.  `table` = the levels of the reference's
 * `_build(uprobs)` (:107-125) one after the other, level l as bfactor^l rows of
 * bfactor probabilities (table_len = sum over levels); `entries` = len(uprobs).
 * One Generator.choice per level and draw (:98-105, with the one-token repair
 * DESIGN.md 6 describes), age scaled while fewer than `entries` items are held
 * (:77-79), a vanished age drawn again (:75-88 sleeps and retries).            */
int32_t emb_selector_create_recency(const double* table, int64_t table_len, int32_t depth,
                                    int32_t bfactor, int64_t entries, uint64_t seed,
                                    emb_selector_t** out);
/* a caller-implemented selector (any Python object with the protocol).       */
typedef struct {
  void* user;
  int64_t (*sample)(void* user);
  int64_t (*size)(void* user);
  void (*insert)(void* user, int64_t key, const uint8_t* stepids, int32_t n_steps);
  void (*remove)(void* user, int64_t key);
  void (*prioritize)(void* user, const uint8_t* stepids, const double* prios, int64_t n); /* may be NULL */
} emb_selector_callbacks_t;
int32_t emb_selector_create_callback(const emb_selector_callbacks_t* cb, emb_selector_t** out);
int32_t emb_selector_insert(emb_selector_t* sel, int64_t key, const uint8_t* stepids, int32_t n_steps);
int32_t emb_selector_remove(emb_selector_t* sel, int64_t key);
int32_t emb_selector_sample(emb_selector_t* sel, int64_t* key);
int32_t emb_selector_len(emb_selector_t* sel, int64_t* n);
int32_t emb_selector_prioritize(emb_selector_t* sel, const uint8_t* stepids, const double* prios, int64_t n);
int32_t emb_selector_destroy(emb_selector_t* sel);

/* ---- Replay (embodied/core/replay.py, chunk.py) ---------------------------
 * Payload lives in a caller-owned device chunk pool: for key k a buffer of
 * (n_slots * chunksize) rows of rowbytes[k] bytes.  The library keeps the
 * integer state (items, FIFO, chunk refcounts, online queue, selector) on the
 * host and moves rows with HIP kernels.                                      */
typedef struct {
  int64_t length;     /* Replay(length=...)                replay.py:16-21     */
  int64_t capacity;   /* in items; 0 = unbounded                              */
  int64_t chunksize;  /*                                    chunk.py:13        */
  int64_t n_slots;    /* chunk slots in the device pool                       */
  int32_t online;     /*                                    replay.py:39-42    */
  int32_t reserved;
  uint64_t uid_hi;    /* high 64 bits of chunk uids (replica id)              */
  /* Sharded pools (0/1 = off): worker w belongs to owner w / workers_per_owner,
   * whose chunks only use slots [o, o+1) * n_slots / owners.                 */
  int64_t owners;
  int64_t workers_per_owner;
} emb_replay_config_t;

/* selector may be NULL: Uniform(seed), as replay.py:26.                      */
int32_t emb_replay_create(const emb_replay_config_t* cfg, emb_selector_t* selector,
                          uint64_t seed, emb_replay_t** out);
int32_t emb_replay_destroy(emb_replay_t* rep);
/* Column schema, discovered from the first add (chunk.py:43-47).  Keys named
 * "stepid" (20 B), "is_first", "is_last" (1 B) get their reference meaning.  */
int32_t emb_replay_set_keys(emb_replay_t* rep, int32_t n_keys, const char* const* names,
                            const int64_t* rowbytes, void* const* pools);
/* After the caller re-allocated a larger pool (rows copied by the caller).   */
int32_t emb_replay_grow(emb_replay_t* rep, int64_t n_slots, void* const* pools);

/* Host-only index steps (no GPU needed; bit-exact with the reference):
 * add_index    = bookkeeping of Replay.add for n steps, one per workers[i], in
 *                order (replay.py:77-118); rows_out[i] = pool row to write,
 *                stepids_out = n x 20 bytes; new_chunks_out = chunks this call
 *                opened in RECYCLED slots (slots an evicted chunk had held).  A
 *                caller that batches the payload writes must, whenever it is
 *                non-zero, write out what it had batched BEFORE this call ahead
 *                of this call's rows: rows still waiting for the old chunk and
 *                rows of the new one would otherwise meet in one launch.
 * sample_index = `batch` sequence draws (replay.py:121-127,151-169,193-214):
 *                rows_out[batch*length] pool rows, online_out[batch] flags,
 *                workers_out[batch] the worker stream of each sequence.
 * resolve      = Replay.update's decode of stepid[i,0] -> `count` pool rows
 *                (replay.py:139-149,216-235); evicted -> rows -1, found 0.   */
int32_t emb_replay_add_index(emb_replay_t* rep, int64_t n, const int64_t* workers,
                             int32_t* rows_out, uint8_t* stepids_out, int32_t* new_chunks_out);
int32_t emb_replay_sample_index(emb_replay_t* rep, int64_t batch, int32_t mode,
                                int32_t* rows_out, uint8_t* online_out, int64_t* workers_out);
int32_t emb_replay_resolve(emb_replay_t* rep, int64_t n, const uint8_t* stepids, int64_t count,
                           int32_t* rows_out, uint8_t* found_out);
int32_t emb_replay_prioritize(emb_replay_t* rep, const uint8_t* stepids, const double* prios,
                              int64_t n);
int32_t emb_replay_len(emb_replay_t* rep, int64_t* items);
int32_t emb_replay_sampler_len(emb_replay_t* rep, int64_t* n);
/* Windows queued by online mode (replay.py:114-118) that the next train-mode
 * samples will serve before the selector is asked.                           */
int32_t emb_replay_online_pending(emb_replay_t* rep, int64_t* n);
int32_t emb_replay_free_slots(emb_replay_t* rep, int64_t* n);
/* out = {items, chunks, streams, inserts, samples, updates} (replay.py:58-74) */
int32_t emb_replay_stats(emb_replay_t* rep, int64_t out[6], int32_t reset);

/* Fused device steps: index + row table upload + ONE kernel launch.
 * add:    src[k] = device (n, rowbytes[k]) for every key except "stepid",
 *         which the library synthesises (entry ignored).   Replay.add
 * sample: dst[k] = device (batch, length, rowbytes[k]); is_first / is_last are
 *         annotated in flight (replay.py:277-292); online_out[batch] and
 *         first_stepids_out[batch*20] (host, optional) receive the online-queue
 *         flags and stepid[:,0] without a device read-back.   Replay.sample
 * update: stepids = host (B, 20) first step of each row; key_ids/src select the
 *         columns to overwrite, src[j] = device (B, T, rowbytes).  Replay.update */
int32_t emb_replay_add(emb_replay_t* rep, int64_t n, const int64_t* workers,
                       const void* const* src, void* stream);
/* Replay.add with the Driver's action mask fused in (driver.py:72-74,84-87 +
 * replay.py:77-118): the n_masked keys masked_keys[j] (replay key ids, dtype
 * codes masked_dtypes[j] = EMB_U8 .. EMB_BOOL) are stored as src * !is_last[row] in
 * their own dtype (a real multiply: -x -> -0.0, NaN stays NaN), and the same
 * masked values are written to masked_out[j] (device (n, rowbytes), may be
 * NULL): the actions the next env step receives.  is_last = device uint8/bool
 * (n).  One launch instead of mask + insert. */
int32_t emb_replay_add_masked(emb_replay_t* rep, int64_t n, const int64_t* workers,
                              const void* const* src, int32_t n_masked,
                              const int32_t* masked_keys, const int32_t* masked_dtypes,
                              void* const* masked_out, const void* is_last, void* stream);

/* Early insert: the vectorised step's observation keys go to their pool rows
 * BEFORE the policy runs, in the launch that builds the policy batch, so that
 * every frame is read once (driver.py:65 np.stack + jax/agent.py:230 layout /
 * dtype change + replay.py:77-118 / chunk.py:41-50 row copy in one pass).
 *
 * obs_stack_insert = emb_obs_stack(frames -> dst as `spec` says) and, when the
 * rows of the next add of exactly `workers` (one step each) are known — every
 * worker already has an open chunk and is listed once — the same launch also
 * writes: the frames to the pool rows of key `frame_key`, every other key k
 * with src[k] != NULL and rowbytes <= 256 (device (n, rowbytes[k]): reward,
 * flags ...; at most 8) and the step ids.  Nothing in the index changes: a
 * worker's next row is the cursor of its open chunk, and no item can reach a
 * row before it is published.  *token_out = a non-zero token if the early
 * insert happened, 0 if the call only did the obs stack (unknown worker, odd
 * frame shape, src[frame_key] != frames).
 *
 * publish = emb_replay_add_masked for the same step.  With the token of the
 * early insert, the same workers and stream, keys whose src[k] is the buffer
 * the early insert copied from are not copied again; what is left (the action)
 * goes out with a 56-byte-argument launch when it is a single small key.  With
 * token 0, or when anything does not match, publish is add_masked.            */
typedef struct emb_obs_spec {
  int64_t pixels, channels;     /* frames are (n, pixels, channels) uint8           */
  int32_t layout, out_dtype;    /* EMB_LAYOUT_*, EMB_U8 / EMB_F16 / EMB_BF16 / EMB_F32 */
  float scale, offset;          /* float outputs: value * scale + offset            */
} emb_obs_spec_t;
int32_t emb_replay_obs_stack_insert(emb_replay_t* rep, int64_t n, const int64_t* workers,
                                    int32_t frame_key, const void* frames,
                                    const emb_obs_spec_t* spec, void* dst, const void* const* src,
                                    void* stream, uint64_t* token_out);
int32_t emb_replay_publish(emb_replay_t* rep, int64_t n, const int64_t* workers,
                           const void* const* src, int32_t n_masked, const int32_t* masked_keys,
                           const int32_t* masked_dtypes, void* const* masked_out,
                           const void* is_last, uint64_t token, void* stream);

/* Carried publish (round 4).  With the early insert in use, what a publish has
 * left is usually one small masked key (the action): a launch of its own whose
 * only cost is its place in the chain of dependent launches of an env step.
 * emb_replay_carry_publish(rep, 1) lets emb_replay_publish skip that launch when
 * the caller passes a NULL masked_out for the key (nobody needs the masked
 * values back -- Driver: the env takes unmasked actions together with `reset`,
 * driver.py:72-75): the key is written, masked, by the NEXT
 * emb_replay_obs_stack_insert launch on the same stream, or by a launch of its
 * own before any other call reads or writes the pool (sample, update, add,
 * gather / scatter rows, chunk bookkeeping, grow all settle it first).
 * Contract while it is enabled: the key's source buffer of a publish stays
 * unchanged until the next call on this replay that launches (its early insert,
 * or anything that settles).  The is_last flags need not: a publish is carried
 * only when the step's early insert stored that very flag buffer as the
 * replay's `is_last` key, and the mask then reads the stored rows -- an env that
 * rewrites its flag outputs in place on the next step is fine.
 * emb_replay_settle(rep) settles explicitly (before the caller moves the pool,
 * reads it directly or frees the source).  Results are identical to an
 * immediate publish.                                                            */
int32_t emb_replay_carry_publish(emb_replay_t* rep, int32_t enable);
int32_t emb_replay_settle(emb_replay_t* rep);
int32_t emb_replay_sample(emb_replay_t* rep, int64_t batch, int32_t mode, void* const* dst,
                          uint8_t* online_out, uint8_t* first_stepids_out, void* stream);
/* The same with per-key head lengths: key k receives only the first
 * key_len[k] steps of every sampled sequence, dst[k] is (batch, key_len[k],
 * rowbytes[k]); 0 (or `length`) = the whole sequence, key_len NULL = all whole.
 * For keys whose consumer reads only the head of the window -- the reference's
 * DreamerV3 takes x[:, :K] (K = replay_context) of the sampled enc/ dyn/ dec/
 * latents (dreamerv3/agent.py:322-331) and its _assemble_batch already copies a
 * [start, stop) sub-range (embodied/core/replay.py:255-275).  Index draws,
 * PRNG stream and the is_first / is_last annotation (computed over the whole
 * sequence, then cut) are those of emb_replay_sample: every key equals the
 * full sample's [:, :key_len[k]].                                              */
int32_t emb_replay_sample_heads(emb_replay_t* rep, int64_t batch, int32_t mode, void* const* dst,
                                const int32_t* key_len, uint8_t* online_out,
                                uint8_t* first_stepids_out, void* stream);
/* The same with the batch side cut into groups of `group` sequences whose
 * starts are `group_stride` bytes (a multiple of 16) apart: dst[k] is key k's
 * place inside group 0, sequence s of key k lands at dst[k] + (s / group) *
 * group_stride + (s % group) * length * rowbytes[k].  This is the layout of a
 * packed batch cut into one block per destination rank, so that the DP-slice
 * exchange of SURVEY.md 8e (the reference assembles per-process slices into the
 * global batch, embodied/jax/internal.py:145-152) is ONE all-to-all.         */
int32_t emb_replay_sample_grouped(emb_replay_t* rep, int64_t batch, int32_t mode,
                                  void* const* dst, int32_t group, int64_t group_stride,
                                  uint8_t* online_out, uint8_t* first_stepids_out, void* stream);
int32_t emb_replay_update(emb_replay_t* rep, int64_t B, int64_t T, const uint8_t* stepids,
                          int32_t n_keys, const int32_t* key_ids, const void* const* src,
                          void* stream);
/* emb_replay_update (replay.py:129-149: stepids = the B first step ids
 * stepid[i, 0], decoded on the host; a window whose chunk was evicted is
 * skipped; where windows overlap the last occurrence wins) with the source in
 * the grouped layout of emb_replay_sample_grouped: sequence s of key k is read
 * from src[k] + (s / group) * group_stride + (s % group) * T * rowbytes[k]
 * (group_stride a multiple of 16; group = 0: identical to emb_replay_update).
 * The layout an all-gather of per-rank packed slices delivers: every rank
 * writes the whole batch back with one launch straight from the receive
 * buffer (replay.py:129-149 run on the global batch, as the reference's
 * train step does after assembling it, embodied/jax/internal.py:145-152).    */
int32_t emb_replay_update_grouped(emb_replay_t* rep, int64_t B, int64_t T,
                                  const uint8_t* first_stepids, int32_t n_keys,
                                  const int32_t* key_ids, const void* const* src, int32_t group,
                                  int64_t group_stride, void* stream);
/* Sharded pools (owners > 1): this process holds owner `owner`'s slot range of
 * the pool only (set_keys received a virtual base).  A bound handle treats every
 * window outside that range as rows -1 in the write-backs and gathers it plans
 * (emb_replay_sample*, emb_replay_update*, emb_replay_gather_rows,
 * emb_replay_scatter_rows): nothing is read or written there and the window's
 * destination bytes are left as they are.  A window is one worker's chunk
 * chain (replay.py:77-118), so it never spans owners.  owner = -1 unbinds.   */
int32_t emb_replay_bind_owner(emb_replay_t* rep, int64_t owner);
/* Move rows given an explicit host row table (multi-GPU owner-side gather,
 * fused sample+windowing, load from disk).  gather: a NULL dst[k] skips key k;
 * the flag annotation applies per `seq_len` rows.                             */
int32_t emb_replay_gather_rows(emb_replay_t* rep, const int32_t* rows, int64_t n_rows,
                               int64_t seq_len, void* const* dst, void* stream);
int32_t emb_replay_scatter_rows(emb_replay_t* rep, const int32_t* rows, int64_t n_rows,
                                int32_t n_keys, const int32_t* key_ids, const void* const* src,
                                void* stream);

/* Callers that add/update and sample from DIFFERENT streams (actor stream +
 * learner stream, run/parallel.py's split in one process) enable this: pool
 * writes and reads are then ordered across streams with events.             */
int32_t emb_replay_multistream(emb_replay_t* rep, int32_t enable);

/* HIP-event timing of the gather launches issued through this handle (on their
 * own stream): total milliseconds and launch count since the last reset.
 * enable = 1 stamps every gather, n > 1 every n-th one (a stamped launch costs
 * the host more than a plain one), 0 switches the stamps off.                */
int32_t emb_replay_profile(emb_replay_t* rep, int32_t enable);
int32_t emb_replay_profile_read(emb_replay_t* rep, int64_t* launches, double* total_ms,
                                int32_t reset);
/* The same counters per launch kind, with the name of the kernel the last
 * stamped launch of that kind ran (as a profiler prints it, without namespaces):
 * which = 0 the sample gathers, 1 the write-backs of emb_replay_update (stamped
 * at the same rate while profiling is on), 2 no kernel: `launches` = the
 * emb_replay_publish calls that handed their index bookkeeping to the library's
 * helper thread (total_ms: how many early inserts took predicted rows instead of
 * waiting for it); which = 3: carried publishes that rode in the next early
 * insert (total_ms: all carried publishes).  kernel_out may be NULL.            */
int32_t emb_replay_profile_report(emb_replay_t* rep, int32_t which, int64_t* launches,
                                  double* total_ms, int32_t reset, char* kernel_out,
                                  int32_t kernel_cap);

/* Checkpoint support (replay.py:294-388): chunk table in/out.
 * complete_all closes every worker's open chunk (replay.py:297-299); it needs
 * one free slot per open chunk (emb_replay_open_chunks) and fails with
 * EMB_ERR_POOL_FULL, leaving the index unchanged, when they are not there.
 * reserve_uids: chunk serials below `serial` are not issued (chunk files of an
 * earlier run in the same directory keep their ids: chunk.py:15-16 draws
 * random UUIDs, this build counts).                                          */
int32_t emb_replay_complete_all(emb_replay_t* rep);
int32_t emb_replay_open_chunks(emb_replay_t* rep, int64_t* n);
int32_t emb_replay_reserve_uids(emb_replay_t* rep, uint64_t serial);
int32_t emb_replay_chunks(emb_replay_t* rep, int64_t cap, uint64_t* uid, uint64_t* succ,
                          int64_t* fill, int64_t* slot, int64_t* time_ms, int64_t* n);
int32_t emb_replay_load_chunk(emb_replay_t* rep, uint64_t uid, uint64_t succ, int64_t fill,
                              int64_t time_ms, int64_t* slot);
int32_t emb_replay_load_items(emb_replay_t* rep, uint64_t uid, int64_t amount);

/* ---- Driver-side kernels (embodied/core/driver.py:55-87) ------------------ */
/* np.stack of per-env frames into the policy batch (driver.py:65) fused with
 * the layout/dtype change the agent applies next (jax/agent.py:230):
 * src = device (n_envs_total, pixels, channels) u8 slab; batch row j reads env
 * env_ids[j] (host int32[n], NULL = identity).                               */
int32_t emb_obs_stack(const void* src, const int32_t* env_ids, int64_t n, int64_t pixels,
                      int64_t channels, int32_t layout, int32_t out_dtype, float scale,
                      float offset, void* dst, void* stream);
/* emb_mask_actions that also tells the HOST when it is done (ABI 5): `flag`, a
 * 32-bit word in pinned, device-mapped host memory, receives `seq` once every row
 * has been stored (system-scope release behind the stores).  With `out` in pinned
 * memory as well this is how the Driver brings the next step's masked actions
 * (driver.py:72-75) down to its env processes: the host reads one word instead of
 * recording and waiting for an event.  `counter`: a zeroed 32-bit device word of
 * the caller's, zero again afterwards; one launch at a time per counter.        */
int32_t emb_mask_actions_notify(const void* act, void* out, int64_t n, int64_t row_elems,
                                int32_t dtype, const void* is_last, void* counter, void* flag,
                                uint32_t seq, void* stream);

/* dst[0 .. bytes) = src[0 .. bytes) by a KERNEL on `stream` (ABI 5).  `src` may be
 * pinned, device-mapped host memory: the Driver brings a piece of its shared
 * observation slab (embodied/core/driver.py:17-25,61-65: what env processes wrote)
 * to the device this way while other env processes are still stepping -- a copy
 * through the DMA engines costs ~10 us of set-up per call on this system, a kernel
 * that reads across PCIe does not.  Any alignment.                              */
int32_t emb_copy_bytes(const void* src, void* dst, int64_t bytes, void* stream);

/* acts zeroed where is_last (driver.py:72-74,84-87): out = act * ~is_last as a
 * real multiply in `dtype`; act, out (n, row_elems), out may alias act.      */
int32_t emb_mask_actions(const void* act, void* out, int64_t n, int64_t row_elems,
                         int32_t dtype, const void* is_last, void* stream);
/* Per-env policy carry rows by env id (embodied/jax/agent.py:173-181,
 * run/parallel.py:94-104): dst[j] = table[ids[j]] / table[ids[j]] = src[j].  */
int32_t emb_rows_gather(const void* table, int64_t rowbytes, const int32_t* ids, int64_t n,
                        void* dst, void* stream);
int32_t emb_rows_scatter(void* table, int64_t rowbytes, const int32_t* ids, int64_t n,
                         const void* src, void* stream);
/* Sequence windowing (streams.py:133-138): src (B, total, rowbytes) ->
 * dst (B, count, rowbytes) = src[:, start:start+count].                      */
int32_t emb_window(const void* src, void* dst, int64_t batch, int64_t total, int64_t start,
                   int64_t count, int64_t rowbytes, void* stream);
/* The same for every key of a batch in ONE launch: src[k] (B, total, rowbytes[k])
 * -> dst[k] (B, count, rowbytes[k]).                                          */
int32_t emb_window_keys(int32_t n_keys, const void* const* src, void* const* dst,
                        const int64_t* rowbytes, int64_t batch, int64_t total, int64_t start,
                        int64_t count, void* stream);

/* ---- return scans, float32 on device ------------------------------------- */
/* PPO GAE (ppo/agent.py:188-201): rew,val (B,T) f32; last,term (B,T) u8 ->
 * adv,tar (B,T-1).  live_scale = 1 - 1/hor.                                  */
int32_t emb_scan_gae(const void* rew, const void* val, const void* last, const void* term,
                     int64_t B, int64_t T, float live_scale, float lam, void* adv, void* tar,
                     void* stream);
/* The same with rew / last / term read straight out of a grouped packed batch
 * (emb_replay_sample_grouped, or the buffer a DP-slice all-to-all delivered):
 * row b of a key starts (b / group) * group_stride + (b % group) * T * itemsize
 * bytes into it; val, adv and tar are dense.  group = 0: identical to
 * emb_scan_gae.                                                               */
int32_t emb_scan_gae_grouped(const void* rew, const void* val, const void* last, const void* term,
                             int64_t B, int64_t T, float live_scale, float lam, void* adv,
                             void* tar, int64_t group, int64_t group_stride, void* stream);
/* DreamerV3 lambda-return (dreamerv3/agent.py:482-490) -> ret (B,T-1).       */
int32_t emb_scan_lambda(const void* last, const void* term, const void* rew, const void* boot,
                        int64_t B, int64_t T, float disc, float lam, void* ret, void* stream);
/* The lambda-return as imag_loss calls it (dreamerv3/agent.py:401-405,482-490):
 * last = 0 and term = 1 - con, with con (B,T) float32 the continue head's
 * PROBABILITY (emb_scan_lambda reads one-byte flags: every con < 1 would be
 * terminal).  Per step, in the reference's operations: term = 1 - con[t+1],
 * live = (1 - term) * disc, ret[t] = rew[t+1] + (1 - lam) * live * boot[t+1]
 * + live * lam * ret[t+1], seeded with boot[:, -1].  rew, con, boot (B,T) ->
 * ret (B,T-1), contiguous float32 on device.
 * EMB_ERR_INVALID before any launch: a NULL pointer, B < 0, T < 2 with B > 0,
 * B * T > 2^31 - 1.  B = 0: EMB_OK, nothing is launched.                       */
int32_t emb_scan_lambda_cont(const void* rew, const void* con, const void* boot, int64_t B, int64_t T,
                             float disc, float lam, void* ret, void* stream);
/* Several lambda-return problems of one train step in ONE launch: DreamerV3
 * computes the replay returns (B,T) and the imagined returns (B*K,H+1) in the
 * same step (dreamerv3/agent.py:401-405 imag_loss, :464-466 repl_loss, both
 * through lambda_return :482-490); at those sizes each scan is launch latency.
 * Same arithmetic as emb_scan_lambda per problem.  Up to 4 problems with rows of
 * at most 257 steps share a launch; anything else runs one launch each.        */
typedef struct emb_lambda_problem {
  const void* last; const void* term; const void* rew; const void* boot; void* ret;
  int64_t B, T;
  float disc, lam;
} emb_lambda_problem_t;
int32_t emb_scan_lambda_multi(int32_t n_problems, const emb_lambda_problem_t* problems, void* stream);
/* Director critic target, time-major (director/agent.py:430-445): rew (T-1,B),
 * cont,value (T,B) -> ret (T-1,B).  discount = 1 - 1/horizon.                */
int32_t emb_scan_director(const void* rew, const void* cont, const void* value, int64_t T,
                          int64_t B, float discount, float lam, void* ret, void* stream);

/* Director manager steps (director/hierarchy.py:240-256), time-major: windows
 * of k steps; reward (T-1,B) f32 [shifted by one step inside], cont (T,B) f32 ->
 * reward_out (T/k-1,B) = mean of cumprod(cont)-weighted rewards per window,
 * cont_out (T/k,B) = product of cont per window.  Either output may be NULL.  */
int32_t emb_abstract_traj(const void* reward, const void* cont, int64_t T, int64_t B, int32_t k,
                          void* reward_out, void* cont_out, void* stream);

/* ---- running return normaliser, float32 on device -------------------------
 * The reference's Normalize (embodied/jax/utils.py:16-91: DreamerV3's retnorm /
 * valnorm / advnorm, the advantage normaliser of the PPO loss) for ONE replica,
 * as one kernel launch of one workgroup.  `state` is five float32 words of
 * DEVICE memory that the caller owns and zeroes once:
 *   [0] mean | lo   [1] sqrs | hi   [2] corr   [3] offset   [4] scale
 * update != 0: the running statistics take one EMA step
 * (1 - rate) * var + rate * value from x[0 .. n) (contiguous float32 on device):
 *   EMB_NORM_MEANSTD  value = mean(x), mean(x * x)   (accumulated in float64)
 *   EMB_NORM_PERC     value = the perclo-th and perchi-th percentile with numpy's
 *                     "linear" method: pos = q / 100 * (n - 1) in double, the
 *                     two neighbouring order statistics selected exactly
 *                     (radix select), a + (b - a) * frac
 * and, with `debias`, corr moves towards 1.  Then, always (utils.py:59-74):
 *   corr = debias ? 1 / max(rate, state[2]) : 1
 *   MEANSTD  offset = mean * corr,  scale = max(limit, sqrt(relu(sqrs * corr - offset^2)))
 *   PERC     offset = lo * corr,    scale = max(limit, hi * corr - offset)
 * out != NULL: the same launch also writes
 *   out[i] = (x[i] - (sub ? sub[i] : offset)) / scale     (out may be x)
 * Nothing returns to the host: no synchronisation, no allocation.  Up to 16384
 * values stay in LDS; more are re-read from global memory by the same launch.
 * EMB_ERR_INVALID before any launch: a NULL config / state (or x with n > 0),
 * n < 0, an unknown impl, rate outside [0, 1], a percentile outside [0, 100],
 * update with n = 0, sub without out.                                          */
#define EMB_NORM_NONE 0      /* emb_dreamer_targets only: no normaliser, (offset, scale) = (0, 1) */
#define EMB_NORM_MEANSTD 1
#define EMB_NORM_PERC 2
typedef struct emb_normalize_config {
  int32_t impl;      /* EMB_NORM_MEANSTD | EMB_NORM_PERC                        */
  int32_t debias;
  double rate, limit;   /* as given: 1 - rate is formed in double, then each is rounded to float32 */
  double perclo, perchi;
} emb_normalize_config_t;
int32_t emb_normalize(const emb_normalize_config_t* config, const void* x, int64_t n, void* state,
                      int32_t update, const void* sub, void* out, void* stream);
/* Kernel launches emb_normalize has issued in this process, counted where the
 * kernel is launched.                                                         */
int32_t emb_normalize_launches(int64_t* count);

/* ---- fused PPO targets, float32 on device --------------------------------
 * The top of ppo_loss (ppo/agent.py:188-210) as ONE kernel launch of one
 * workgroup, in place of emb_scan_gae, two emb_normalize and the array ops
 * between them.  Both normalisers must be EMB_NORM_MEANSTD (PPO's own:
 * ppo/configs.yaml:99-100); their state words are those of emb_normalize.
 *   agent.py:191-192  (voffset, vscale) = valnorm's stats BEFORE the step,
 *                     val = pred * vscale + voffset
 *   agent.py:194-201  GAE over rew, val (B,T) f32 and last, term (B,T) u8 ->
 *                     adv, tar (B,T-1); live_scale = 1 - 1/hor
 *   agent.py:203      update != 0: valnorm takes its EMA step from tar (utils.py:44-57)
 *   agent.py:204-206  tar_normed (B,T) = clip((tar - voffset') / vscale', +-tarclip)
 *                     with a last column of +0.0; tarclip = 0: no clip
 *   agent.py:209-210  update != 0: advnorm steps from adv;
 *                     adv_normed (B,T-1) = (adv - aoffset) / ascale
 * Words 0-2 of both states are written with update != 0 only, words 3-4
 * (offset, scale) always.  The batch sums are accumulated in float64, as
 * emb_normalize's.  Correct at every B >= 1, T >= 2 and alignment; fast while one
 * workgroup suits B * T (a few thousand values).
 * EMB_ERR_INVALID before any launch: a NULL config or state, one state given
 * twice, B < 0, T < 2 with B > 0, B * T > 2^31 - 1, a NULL input or output with
 * B > 0, an impl other than EMB_NORM_MEANSTD, rate outside [0, 1], tarclip < 0.
 * B = 0: EMB_OK, nothing is launched.                                           */
int32_t emb_ppo_targets(const emb_normalize_config_t* valnorm, const emb_normalize_config_t* advnorm,
                        const void* rew, const void* pred, const void* last, const void* term, int64_t B,
                        int64_t T, float live_scale, float lam, float tarclip, int32_t update, void* adv,
                        void* tar, void* tar_normed, void* adv_normed, void* valnorm_state,
                        void* advnorm_state, void* stream);
/* Kernel launches emb_ppo_targets has issued in this process, counted where the
 * kernel is launched.                                                         */
int32_t emb_ppo_targets_launches(int64_t* count);

/* ---- fused DreamerV3 imagination targets, float32 on device ---------------
 * imag_loss's targets (dreamerv3/agent.py:397-419) as ONE kernel launch of one
 * workgroup, in place of emb_scan_lambda_cont, up to three emb_normalize and the
 * array ops between them.  retnorm must be EMB_NORM_PERC; valnorm and advnorm
 * are each EMB_NORM_MEANSTD or none (a NULL config or impl EMB_NORM_NONE: its
 * state is not read, (offset, scale) = (0, 1)); dreamerv3/configs.yaml:111-113
 * ships perc / none / none.  State words are those of emb_normalize.
 *   agent.py:397-400  (voffset, vscale) = valnorm's stats BEFORE the step,
 *                     tarval = pred * vscale + voffset; `pred` (N,T) is the
 *                     prediction that serves as the target value (the slow
 *                     critic's with slowtar)
 *   agent.py:401-402  weight (N,T) = cumprod(disc * con, 1) / disc, the products
 *                     taken left to right, one rounding each (numpy.cumprod)
 *   agent.py:403-405  ret (N,T-1) = the lambda-return of emb_scan_lambda_cont
 *                     over rew, con, boot = tarval
 *   agent.py:407-408  retnorm(ret, update) -> (roffset, rscale) AFTER the step,
 *                     adv (N,T-1) = (ret - tarval[:, :-1]) / rscale
 *   agent.py:409-410  advnorm(adv, update), adv_normed = (adv - aoffset) / ascale
 *   agent.py:417-419  valnorm(ret, update), tar_padded (N,T) =
 *                     (ret - voffset') / vscale' with a +0.0 last column
 * Words 0-2 of every present state are written with update != 0 only, words 3-4
 * (offset, scale) always.  The percentiles are selected exactly, the batch sums
 * accumulated in float64, both by the device code of emb_normalize.
 * One workgroup holds the returns' sort keys: N * (T-1) <= 16 384.
 * EMB_ERR_INVALID before any launch: a NULL retnorm config or state, retnorm
 * not EMB_NORM_PERC, valnorm or advnorm EMB_NORM_PERC, a mean-std normaliser
 * with a NULL state, two states that are read given the same address, N < 0,
 * T < 2, a NULL input or output with N > 0, N * (T-1) > 16 384 (then:
 * emb_scan_lambda_cont + emb_normalize), rate outside [0, 1], a percentile
 * outside [0, 100].  N = 0: EMB_OK, nothing is launched.                        */
int32_t emb_dreamer_targets(const emb_normalize_config_t* retnorm, const emb_normalize_config_t* valnorm,
                            const emb_normalize_config_t* advnorm, const void* rew, const void* con,
                            const void* pred, int64_t N, int64_t T, float disc, float lam, int32_t update,
                            void* ret, void* weight, void* adv, void* adv_normed, void* tar_padded,
                            void* ret_state, void* val_state, void* adv_state, void* stream);
/* Kernel launches emb_dreamer_targets has issued in this process, counted where
 * the kernel is launched.                                                      */
int32_t emb_dreamer_targets_launches(int64_t* count);

/* ---- the symexp_twohot head, float32 arithmetic on device -----------------
 * DreamerV3's reward and value heads (embodied/jax/heads.py:132-144 builds the
 * bins, embodied/jax/outs.py:273-330 is the distribution): what sits on both
 * sides of emb_dreamer_targets -- its `pred` argument is value.pred(), its
 * tar_padded goes into value.loss (dreamerv3/agent.py:398-399,420-422).
 * `logits` is (rows, n) contiguous on device, dtype EMB_F32 or EMB_BF16 (bfloat16
 * is widened in registers; the reference computes in float32, outs.py:276);
 * `bins` n float32 on device, non-decreasing (the caller's promise: the library
 * counts, it does not sort; heads.py:141-143 gives an even n the neighbours
 * 0.0, -0.0); lse, pred, loss, gout, every target: `rows` float32 on device.
 * One kernel launch each:
 *   emb_twohot_stats  outs.py:280,285-309,328-329: lse = max + log(sum(exp(x - max)))
 *                     and pred = sum over the mirrored pairs
 *                     p[i] * b[i] + p[n-1-i] * b[n-1-i], each pair formed before
 *                     any other addition, plus the middle bin for odd n, with
 *                     p = exp(x - max) / sum: uniform logits over antisymmetric
 *                     bins give exactly 0.0.  One pass over the logits.
 *   emb_twohot_loss   outs.py:311-330 for k targets (host array of k device
 *                     pointers) with k host coefficients:
 *                       below = #(bins <= t) - 1, above = n - #(bins > t), both
 *                       clipped to [0, n-1]; equal indices: weights 0.5 / 0.5 on
 *                       the one bin, else w_below = |b[above] - t| / total,
 *                       w_above = |b[below] - t| / total
 *                       loss[r] = sum_k coefs[k] * -(w_below * (x[below] - lse)
 *                                                   + w_above * (x[above] - lse))
 *                     Two logits per row and target are read, not the row.  A NaN
 *                     target gives NaN (n > 1), one beyond an outer bin that bin
 *                     with weight 1.
 *   emb_twohot_grad   the gradient of that sum with respect to the logits,
 *                       grad[r, i] = gout[r] * (sum(coefs) * exp(x[r, i] - lse[r])
 *                                               - sum_k coefs[k] * twohot_k[r, i])
 *                     written in the logits' dtype: one read of the logits, one
 *                     write of the gradient.
 * No atomics: the same bits run to run.
 * EMB_ERR_INVALID before any launch: an unknown dtype, rows < 0, n outside
 * 1 .. 1024, rows * n > 2^31 - 1, k outside 1 .. 4, a NULL targets or coefs
 * array, and with rows > 0 any NULL pointer.  rows = 0: EMB_OK, nothing is
 * launched.                                                                    */
int32_t emb_twohot_stats(const void* logits, int32_t dtype, int64_t rows, int64_t n, const void* bins, void* lse,
                         void* pred, void* stream);
int32_t emb_twohot_loss(const void* logits, int32_t dtype, int64_t rows, int64_t n, const void* bins,
                        const void* lse, const void* const* targets, const float* coefs, int32_t k, void* loss,
                        void* stream);
int32_t emb_twohot_grad(const void* logits, int32_t dtype, int64_t rows, int64_t n, const void* bins,
                        const void* lse, const void* const* targets, const float* coefs, int32_t k, const void* gout,
                        void* grad, void* stream);
/* Kernel launches the three entry points above have issued in this process,
 * counted where the kernels are launched.                                      */
int32_t emb_twohot_launches(int64_t* count);

/* ---- the RSSM's KL pair over one-hot latents, float32 arithmetic on device --
 * DreamerV3's world-model loss, RSSM.loss (dreamerv3/rssm.py:123-132), over
 * _dist = Agg(OneHot(logits, unimix), 1, sum) (dreamerv3/rssm.py:173-176,
 * embodied/jax/outs.py:40-76 Agg, embodied/jax/outs.py:208-263 Categorical and
 * OneHot).  `post` and `prior` are (rows, stoch, classes) contiguous on device,
 * dtype EMB_F32 or EMB_BF16 (bfloat16 is widened in registers; the reference
 * computes in float32, outs.py:211); kl, ent_post, ent_prior, dyn, rep, g_rep,
 * g_dyn: `rows` float32 on device.  Per group of `classes` logits
 *   p = (1 - unimix) * softmax(post) + unimix / classes       (outs.py:212-216)
 *   q = the same of prior;  unimix == 0: p = softmax(post), log p = log_softmax
 * and per row, summed over the stoch groups in one fixed order,
 *   kl = sum p (log p - log q)                                (outs.py:236-240)
 *   ent_post = -sum p log p, ent_prior = -sum q log q         (outs.py:230-234)
 * (p sums to 1 up to rounding, so the reference's second softmax over log p is
 * the identity and is not repeated).  One kernel launch each:
 *   emb_onehot_kl       rssm.py:125-132: one read of post and prior.  dyn and
 *                       rep have the same forward value (sg only routes
 *                       gradients): both receive max(kl, free_nats), or kl where
 *                       free_nats == 0 (rssm.py:127); either may be NULL.
 *   emb_onehot_kl_grad  the gradients of that pair in the logits' dtype:
 *                         grad_post  = g_rep * f * d kl / d post
 *                         grad_prior = g_dyn * f * d kl / d prior
 *                       f the gradient of rssm.py:128-129's maximum from the
 *                       saved `kl`: 1 where kl > free_nats, 0 where kl <
 *                       free_nats, 1/2 at equality (jnp.maximum's), NaN for a NaN
 *                       kl; free_nats == 0: 1.  grad_post or grad_prior may be
 *                       NULL: that side is not written and its g not read.
 * No atomics: the same bits run to run.
 * EMB_ERR_INVALID before any launch: an unknown dtype, rows < 0, stoch < 1,
 * classes outside 1 .. 256, more than 2^31 - 1 logits, unimix outside [0, 1),
 * free_nats < 0, and with rows > 0 a NULL required pointer (for the gradient:
 * both outputs NULL, or an output without its g).  rows = 0: EMB_OK, nothing
 * is launched.                                                                 */
int32_t emb_onehot_kl(const void* post, const void* prior, int32_t dtype, int64_t rows, int64_t stoch,
                      int64_t classes, float unimix, float free_nats, void* kl, void* ent_post, void* ent_prior,
                      void* dyn, void* rep, void* stream);
int32_t emb_onehot_kl_grad(const void* post, const void* prior, int32_t dtype, int64_t rows, int64_t stoch,
                           int64_t classes, float unimix, float free_nats, const void* kl, const void* g_rep,
                           const void* g_dyn, void* grad_post, void* grad_prior, void* stream);
/* Kernel launches the two entry points above have issued in this process,
 * counted where the kernels are launched.                                      */
int32_t emb_onehot_kl_launches(int64_t* count);

/* ---- the actor's loss over a categorical policy, float32 arithmetic on device
 * DreamerV3's imag_loss, dreamerv3/agent.py:411-415:
 *   logpi = sum_k policy[k].logp(sg(act[k]))[:, :-1]
 *   ents  = policy[k].entropy()[:, :-1]
 *   policy_loss = sg(weight[:, :-1]) * -(logpi * sg(adv_normed) + actent * ents)
 * for one action key (the loss is linear in logpi and ents: the sum over keys
 * is the sum of one call per key), policy[k] = Agg(Categorical(logits, unimix),
 * dims, sum) (embodied/jax/heads.py:90-91, 101-110; embodied/jax/outs.py:40-76
 * Agg, embodied/jax/outs.py:208-234 Categorical).  `logits` is (N, T, groups,
 * classes) contiguous on device, dtype EMB_F32 or EMB_BF16 (widened in
 * registers; the reference computes in float32, outs.py:211); `act` (N, T,
 * groups) int32 on device, or NULL (no action: logpi = 0 and its gradient 0).
 * `drop` is 0 or 1, the reference's [:, :-1] taken inside the launch: an output
 * row r = (n, t), t < T - drop, reads the logits' row n * T + t, and the last step
 * of every n is not read.  adv, loss, logpi, ent and gout are (N, T - drop)
 * float32 on device; `weight` is float32 read at n * weight_stride + t, so (N, T)
 * as emb_dreamer_targets writes it (stride T) and (N, T - drop) both go.  adv
 * and weight may be NULL: 1.  Per group of `classes` logits
 *   p = (1 - unimix) * softmax(x) + unimix / classes, logp = log p (outs.py:212-216)
 *   unimix == 0: p = softmax(x), logp = log_softmax(x), in the log domain
 * and per output row, summed over the groups in one fixed order,
 *   logpi = sum_g logp[g, act[g]]      (outs.py:226-228, 63-64; the action is
 *           compared with the class index, never an address: one outside
 *           [0, classes) adds 0, as jax.nn.one_hot)
 *   ent   = sum_g -sum_k p_k logp_k    (outs.py:230-234, 69-71)
 *   loss  = weight * -(logpi * adv + actent * ent)            (agent.py:413-414)
 * One kernel launch each:
 *   emb_policy_loss       one read of the logits; `loss` may be NULL (not written).
 *   emb_policy_loss_grad  grad (N, T, groups, classes) in the logits' dtype =
 *                         gout * d loss / d logits, the closed form from one more
 *                         read (nothing the forward wrote is used); the rows of
 *                         a dropped step are written as zeros; a row with a NaN
 *                         or +inf logit or a group of -inf is NaN throughout.
 * No atomics: the same bits run to run.
 * EMB_ERR_INVALID before any launch: an unknown dtype, N or T < 0, drop not 0 or
 * 1, groups < 1, classes outside 1 .. 256, more than 2^31 - 1 logits, unimix
 * outside [0, 1), a non-finite actent, and with work to do a NULL logits, logpi,
 * ent, gout or grad, or a weight_stride below T - drop.  No output rows (N = 0
 * or T - drop = 0): emb_policy_loss launches nothing; emb_policy_loss_grad
 * launches nothing without logits (N * T = 0) and otherwise writes the zeros.  */
int32_t emb_policy_loss(const void* logits, const void* act, int32_t dtype, int64_t N, int64_t T, int32_t drop,
                        int64_t groups, int64_t classes, float unimix, float actent, const void* adv,
                        const void* weight, int64_t weight_stride, void* loss, void* logpi, void* ent, void* stream);
int32_t emb_policy_loss_grad(const void* logits, const void* act, int32_t dtype, int64_t N, int64_t T, int32_t drop,
                             int64_t groups, int64_t classes, float unimix, float actent, const void* adv,
                             const void* weight, int64_t weight_stride, const void* gout, void* grad, void* stream);
/* Kernel launches the two entry points above have issued in this process,
 * counted where the kernels are launched.                                      */
int32_t emb_policy_loss_launches(int64_t* count);

/* ---- the learner's optimizer step, float32 arithmetic on device
 * The reference's chain, dreamerv3/agent.py:342-379, over every parameter tensor
 * at once:
 *   clip_by_agc        embodied/jax/opt.py:109-123
 *   scale_by_rms       embodied/jax/opt.py:126-143
 *   scale_by_momentum  embodied/jax/opt.py:146-164
 *   optax.add_decayed_weights, scale_by_learning_rate (agent.py:361-378) and
 *   optax.apply_updates (opt.py:62),
 * and the metrics of embodied/jax/opt.py:64-79.  Per tensor, t the number of this
 * update counted from 1, the caller handing over omb = 1 - beta and c = 1 -
 * beta^t, each formed in double and rounded once:
 *   unorm = ||g||2, pnorm = ||p||2                             (opt.py:116-117)
 *   g1 = g * (1 / maximum(1, unorm / (agc * maximum(pmin, pnorm))))   agc == 0: g
 *   nu = beta2 * nu + omb2 * (g1 * g1)                         (opt.py:136-137)
 *   u  = g1 / (sqrt(nu / c2) + eps)                            (opt.py:138-140)
 *   mu = omb1 * u + beta1 * mu                                 (opt.py:156)
 *   m  = mu / c1, nesterov: (omb1 * u + beta1 * mu) / c1       (opt.py:157-161)
 *   upd = (m + wd * p where the tensor decays, else m) * -lr   (agent.py:365, 378)
 *   p  = p + upd
 * `maximum` hands a NaN on: one NaN in a tensor's gradient makes its p, nu and mu
 * NaN throughout; an infinity and no NaN gives the scale 0, g1 = 0 for the finite
 * elements and NaN for the infinite ones; no other tensor is touched.
 *
 * Work is cut into chunks of one tensor each.  emb_optim_table (host only, no
 * HIP call) writes what the kernels read through two device pointers:
 *   table   one record of `record_bytes` per tensor, from addrs (tensors, 4) =
 *           the device addresses of p, g, nu, mu (float32; g bfloat16 with
 *           EMB_OPTIM_BF16), counts (tensors) elements each, 0 .. 2^31 - 1, and
 *           flags (tensors) of EMB_OPTIM_BF16 | EMB_OPTIM_DECAY
 *   chunks  one 8-byte record per chunk (`chunk_capacity` = what `chunks` holds)
 * Either may be NULL (not written); n_chunks, chunk_size (elements per chunk) and
 * record_bytes receive their values where not NULL.  The caller copies both to
 * the device, and the table again whenever an address changes.  A tensor whose
 * p, g, nu and mu start at the same element offset modulo 4 is read and written
 * in 16-byte vectors with scalar ragged ends; any other alignment goes scalar.
 *   emb_optim_norms    launch 1: every chunk's sum g^2 and sum p^2 into `partials`,
 *                      (4, n_chunks) float32 on device
 *   emb_optim_update   launch 2: every workgroup sums its tensor's partials in a
 *                      fixed order, forms the scale and updates its chunk in
 *                      place; leaves sum upd^2 and sum p_new^2 per chunk behind
 *   emb_optim_metrics  one launch of one workgroup: out (4,) float32 on device =
 *                      grad_norm (optax.global_norm of the raw gradients),
 *                      grad_rms, update_rms, param_rms (embodied/jax/nets.py:120-124
 *                      over `count` elements; the parameters after the update)
 * No atomics, and no workgroup waits for another: the same bits run to run.
 * EMB_ERR_INVALID before any launch: sizes outside their ranges, an address that
 * is null or not aligned to its element, unknown flags, a chunk map that is too
 * small, a non-finite lr, a beta outside [0, 1), omb or c outside (0, 1], a
 * negative or non-finite eps, agc, pmin or wd, and with n_chunks > 0 a NULL
 * pointer.  n_chunks = 0: norms and update launch nothing.                     */
#define EMB_OPTIM_BF16 1
#define EMB_OPTIM_DECAY 2
int32_t emb_optim_table(const int64_t* addrs, const int64_t* counts, const int32_t* flags, int64_t tensors,
                        void* table, void* chunks, int64_t chunk_capacity, int64_t* n_chunks, int64_t* chunk_size,
                        int64_t* record_bytes);
int32_t emb_optim_norms(const void* table, const void* chunks, int64_t n_chunks, void* partials, void* stream);
int32_t emb_optim_update(const void* table, const void* chunks, int64_t n_chunks, void* partials, float lr, float beta1,
                         float omb1, float c1, float beta2, float omb2, float c2, float eps, float agc, float pmin,
                         float wd, int32_t nesterov, void* stream);
int32_t emb_optim_metrics(const void* partials, int64_t n_chunks, int64_t count, void* out, void* stream);
/* The PPO learner's chain, ppo/agent.py:114-124, on the same table, chunk map and
 * partials (emb_optim_table builds them; emb_optim_metrics serves it unchanged):
 *   optax.clip_by_global_norm, optax.scale_by_adam (eps_root = 0),
 *   optax.add_decayed_weights, optax.scale_by_learning_rate, optax.apply_updates.
 * All float32, t the number of this update counted from 1, omb = 1 - beta and
 * c = 1 - beta^t formed in double by the caller and rounded once:
 *   gnorm = sqrt(sum over EVERY tensor of sum g^2)            optax.global_norm
 *   g1  = g if clip == 0 or gnorm < clip, else (g / gnorm) * clip
 *   mu  = beta1 * mu + omb1 * g1
 *   nu  = beta2 * nu + omb2 * (g1 * g1)
 *   u   = (mu / c1) / (sqrt(nu / c2) + eps)
 *   upd = (u + wd * p where the tensor decays, else u) * -lr ;  p = p + upd
 * The select is on gnorm < clip: a NaN in ANY gradient makes p, mu and nu NaN in
 * EVERY tensor (the reference's behaviour, unlike the per-tensor containment of
 * the chain above); an infinity and no NaN gives g / inf * clip, 0 for the finite
 * elements and NaN for the infinite ones.
 *   emb_optim_grad_norms   launch 1: every chunk's sum g^2 into row 0 of
 *                          `partials`; the parameters are not read
 *   emb_optim_adam_update  launch 2: every workgroup sums row 0 over all chunks
 *                          in one fixed order (the same bits and the same clip
 *                          decision everywhere), then updates its chunks in
 *                          place; leaves sum upd^2 and sum p_new^2 per chunk in
 *                          rows 2 and 3
 * No atomics.  EMB_ERR_INVALID before any launch: a NULL table, chunk map or
 * partials, n_chunks outside 1 .. 2^31 - 1, a non-finite lr, a beta outside
 * [0, 1), omb or c outside (0, 1], a negative or non-finite clip, eps or wd.  */
int32_t emb_optim_grad_norms(const void* table, const void* chunks, int64_t n_chunks, void* partials, void* stream);
int32_t emb_optim_adam_update(const void* table, const void* chunks, int64_t n_chunks, void* partials, float lr,
                              float beta1, float omb1, float c1, float beta2, float omb2, float c2, float eps,
                              float clip, float wd, void* stream);
/* The slow (EMA) copy of a set of float32 tensors, the reference's SlowModel
 * (embodied/jax/utils.py:94-127; dreamerv3/agent.py:142 `self.slowval.update()`),
 * per element, float32, two rounded products and one rounded sum:
 *   dst = mix * src + omm * dst                                 (utils.py:118)
 * The caller hands over mix = the rate as float32 and omm = 1 - mix FORMED IN
 * float32, as the reference forms it on a float32 scalar, and decides on the host
 * whether this is an update step (utils.py:117, count % every == 0): on any other
 * step it calls nothing.  A NaN or an infinity in src or dst stays in its element.
 *   emb_slow_table   host only, no HIP call; as emb_optim_table: one record of
 *                    `record_bytes` per tensor from addrs (tensors, 2) = the device
 *                    addresses of dst and src and counts (tensors), one 8-byte
 *                    record per chunk into `chunks`.  A tensor whose src is 16-byte
 *                    aligned where dst is takes 16-byte accesses with scalar
 *                    ragged ends, any other goes scalar.  dst == src is refused.
 *   emb_slow_update  one launch over such a table: reads 8 and writes 4 bytes per
 *                    element.  n_chunks = 0 launches nothing.
 *   emb_optim_update_slow, emb_optim_adam_update_slow
 *                    emb_optim_update / emb_optim_adam_update with the slow copy
 *                    written in the same launch from the p_new it holds in
 *                    registers: `slow` is (tensors,) uint64 on device, the address
 *                    of each table entry's slow copy or 0 for none (the tensor is
 *                    then updated as by the plain entry point); d = mix * p_new +
 *                    omm * d at the same element index.  p, nu, mu and the
 *                    partials receive the same bits as from the plain entry point.
 *                    The caller guarantees that a slow copy is float32 of its
 *                    tensor's size, 4-byte aligned, and overlaps nothing else in
 *                    the table.
 * EMB_ERR_INVALID before any launch: what emb_optim_table, emb_optim_update and
 * emb_optim_adam_update refuse, a NULL `slow`, mix outside [0, 1], omm not finite
 * or outside [0, 1].                                                           */
int32_t emb_slow_table(const int64_t* addrs, const int64_t* counts, int64_t tensors, void* table, void* chunks,
                       int64_t chunk_capacity, int64_t* n_chunks, int64_t* record_bytes);
int32_t emb_slow_update(const void* table, const void* chunks, int64_t n_chunks, float mix, float omm, void* stream);
int32_t emb_optim_update_slow(const void* table, const void* chunks, int64_t n_chunks, void* partials, float lr,
                              float beta1, float omb1, float c1, float beta2, float omb2, float c2, float eps, float agc,
                              float pmin, float wd, int32_t nesterov, const void* slow, float mix, float omm,
                              void* stream);
int32_t emb_optim_adam_update_slow(const void* table, const void* chunks, int64_t n_chunks, void* partials, float lr,
                                   float beta1, float omb1, float c1, float beta2, float omb2, float c2, float eps,
                                   float clip, float wd, const void* slow, float mix, float omm, void* stream);
/* Kernel launches the eight launching entry points above (emb_optim_norms to
 * emb_optim_adam_update_slow; the two table builders launch nothing) have issued
 * in this process, counted where the kernels are launched.                     */
int32_t emb_optim_launches(int64_t* count);

/* ---- Norm followed by the activation, float32 arithmetic on device
 * embodied/jax/nets.py:361-399 (Norm.__call__) and then embodied/jax/nets.py:26-39
 * (act): what follows every Linear, BlockLinear and Conv2D of DreamerV3's
 * networks -- inside RSSM._core four times (dreamerv3/rssm.py:141-151), once in
 * _observe (dreamerv3/rssm.py:83-85) and twice in _prior (dreamerv3/rssm.py:163-165).
 * `x` and `out` are (rows, units) contiguous on device, dtype EMB_F32 or EMB_BF16
 * (widened in registers); `scale` and `shift` are (units,) float32 on device, or
 * NULL: ones / zeros.  Per row, every operation in float32 and on its own:
 *   EMB_NORM_RMS    y = x * (rsqrt(mean(x^2) + eps) * scale)          (nets.py:383-386)
 *   EMB_NORM_LAYER  y = (x - mean) * (rsqrt(max(0, mean(x^2) - mean^2) + eps) * scale)
 *                       + shift          (nets.py:388-395: the one-pass variance)
 *   out = act(y): EMB_ACT_NONE, EMB_ACT_SILU y sigmoid(y), EMB_ACT_GELU the tanh
 *         approximation (jax.nn.gelu's default), EMB_ACT_RELU max(y, 0)
 * The activation works on the float32 y and the result is rounded once at the
 * store; the reference rounds y to the compute dtype first (nets.py:398).
 * EMB_NORM_RMS ignores `shift`.
 *   emb_norm_act       one launch; x is read once.
 *   emb_norm_act_grad  dx (rows, units) in the dtype of x -- gout's too -- and
 *                      dscale, dshift (units,) float32, each NULL or written, all
 *                      recomputed from x.  With dscale or dshift every workgroup
 *                      leaves its rows' column sums in `partials` (float32 on
 *                      device, `partial_floats` of them: at least 2 * P * units
 *                      with P = min(ceil(rows / (units <= 1024 ? 4 : 1)), 512)) and
 *                      a second launch adds them in a fixed order; without, one
 *                      launch and `partials` is not used.
 * No atomics: the same bits run to run.  A row whose mean(x^2) is NaN or
 * infinite is NaN throughout in out and dx, and touches no other row; dscale and
 * dshift sum over it.
 * EMB_ERR_INVALID before any launch: an unknown dtype, impl or act, rows < 0,
 * units outside 1 .. 16384, more than 2^31 - 1 elements, a negative or non-finite
 * eps, and with rows > 0 a NULL x, out or gout, no output at all, or partials
 * that are NULL or too small.  rows = 0: EMB_OK, nothing is launched or written. */
#define EMB_NORM_RMS 0
#define EMB_NORM_LAYER 1
#define EMB_ACT_NONE 0
#define EMB_ACT_SILU 1
#define EMB_ACT_GELU 2
#define EMB_ACT_RELU 3
int32_t emb_norm_act(const void* x, const void* scale, const void* shift, int32_t dtype, int64_t rows, int64_t units,
                     int32_t impl, int32_t act, float eps, void* out, void* stream);
int32_t emb_norm_act_grad(const void* x, const void* scale, const void* shift, const void* gout, int32_t dtype,
                          int64_t rows, int64_t units, int32_t impl, int32_t act, float eps, void* dx, void* dscale,
                          void* dshift, void* partials, int64_t partial_floats, void* stream);
/* Kernel launches the two entry points above have issued in this process,
 * counted where the kernels are launched.                                      */
int32_t emb_norm_act_launches(int64_t* count);

/* ---- the tails of the convolution stages: pool + Norm + act, Norm + act + upsample
 * Encoder.__call__, dreamerv3/rssm.py:238-241 (the default, strided = False):
 * after the stage's Conv2D a 2x2 max pool (rssm.py:239-240), Norm and act
 * (rssm.py:241).  Decoder.__call__, dreamerv3/rssm.py:327, 336-338, 346: act(Norm)
 * and then every pixel repeated 2x2 (rssm.py:336, jnp's element-by-element
 * repeat) in front of the next Conv2D.  Norm and act are embodied/jax/nets.py:361-399
 * and embodied/jax/nets.py:26-39, with emb_norm_act's impl, act, eps, scale and
 * shift and its float32 arithmetic, rounded once at the store.  Tensors are
 * channels last, contiguous on device, EMB_F32 or EMB_BF16; `x` is (images, H, W, C).
 *   emb_pool_norm_act        out (images, H/2, W/2, C) = act(Norm(max of the 2x2
 *                            window)), one launch.  The max propagates a NaN.
 *   emb_pool_norm_act_grad   gout as out, dx as x: the pooled row and its
 *                            statistics recomputed from x, its gradient g formed
 *                            as emb_norm_act_grad does, and per window and channel
 *                            g / count where x equals the max (count: how many of
 *                            the four do) and 0 elsewhere.
 *   emb_norm_act_upsample    out (images, 2H, 2W, C), out[n, 2h+i, 2w+j] =
 *                            act(Norm(x[n, h, w])) for i, j in {0, 1}; one launch,
 *                            x read once, four rows written.
 *   emb_norm_act_upsample_grad  gout as out, dx as x: the four rows of gout added
 *                            in float32 as ((0,0) + (0,1)) + ((1,0) + (1,1)), then
 *                            emb_norm_act_grad's row.
 * dscale, dshift, partials as emb_norm_act_grad: with either, every workgroup
 * leaves its column sums in `partials` (at least 2 * P * C float32, P =
 * min(ceil(pixels / (256 / L)), 1024) with pixels = images * H/2 * W/2 for the
 * pool and images * H * W for the upsample, L = 8, 16, 32, 64 lanes per pixel for
 * C <= 64, 128, 256, 1024) and a second launch adds them in a fixed order.
 * No atomics: the same bits run to run.  A pixel whose (pooled) row has a NaN
 * or infinite mean(x^2) is NaN throughout in out and in its window of dx and
 * touches no other pixel; dscale and dshift sum over it.
 * EMB_ERR_INVALID before any launch: an unknown dtype, impl or act, images < 0,
 * H or W below 1, for the pool an odd H or W, C outside 1 .. 1024, more than
 * 2^31 - 1 elements in the larger tensor, a negative or non-finite eps, and with
 * images > 0 a NULL x, out or gout, no output at all, or partials that are NULL
 * or too small.  images = 0: EMB_OK, nothing is launched or written.           */
int32_t emb_pool_norm_act(const void* x, const void* scale, const void* shift, int32_t dtype, int64_t images, int64_t H,
                          int64_t W, int64_t C, int32_t impl, int32_t act, float eps, void* out, void* stream);
int32_t emb_pool_norm_act_grad(const void* x, const void* scale, const void* shift, const void* gout, int32_t dtype,
                               int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act, float eps,
                               void* dx, void* dscale, void* dshift, void* partials, int64_t partial_floats,
                               void* stream);
int32_t emb_norm_act_upsample(const void* x, const void* scale, const void* shift, int32_t dtype, int64_t images,
                              int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act, float eps, void* out,
                              void* stream);
int32_t emb_norm_act_upsample_grad(const void* x, const void* scale, const void* shift, const void* gout,
                                   int32_t dtype, int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl,
                                   int32_t act, float eps, void* dx, void* dscale, void* dshift, void* partials,
                                   int64_t partial_floats, void* stream);
/* Kernel launches the four entry points above have issued in this process,
 * counted where the kernels are launched.                                      */
int32_t emb_conv_stage_launches(int64_t* count);

/* ---- the blocked GRU gate of the RSSM, float32 arithmetic on device
 * The tail of RSSM._core, dreamerv3/rssm.py:152-159: `x` (rows, 3 * deter) is what
 * the `dyngru` BlockLinear leaves, `deter` and `out` are (rows, deter), all
 * contiguous on device in one dtype, EMB_F32 or EMB_BF16.  `blocks` divides
 * deter, h = deter / blocks; for block k and j < h (rssm.py:153-154)
 *   reset  = sigmoid(x[r, 3hk + j])                                (rssm.py:155)
 *   cand   = tanh(reset * x[r, 3hk + h + j])                       (rssm.py:156)
 *   update = sigmoid(x[r, 3hk + 2h + j] - 1)                       (rssm.py:157)
 *   out[r, hk + j] = update * cand + (1 - update) * deter[r, hk + j]   (rssm.py:158)
 * rounded once at the store.  The split is index arithmetic: nothing is copied.
 *   emb_gru_gate       one launch.
 *   emb_gru_gate_grad  one launch: dx (rows, 3 * deter) and ddeter (rows, deter)
 *                      from x, deter and gout (rows, deter), in their dtype;
 *                      either may be NULL (not written).
 * Elementwise: a saturated gate gives finite values and a zero or tiny gradient, a
 * NaN touches the output element and the gradient elements it feeds.
 * EMB_ERR_INVALID before any launch: an unknown dtype, rows < 0, deter < 1, a
 * `blocks` below 1 or that does not divide deter, more than 2^31 - 1 elements of
 * x, and with rows > 0 a NULL input or no output.  rows = 0: EMB_OK, nothing is
 * launched.                                                                    */
int32_t emb_gru_gate(const void* x, const void* deter, int32_t dtype, int64_t rows, int64_t width, int64_t blocks,
                     void* out, void* stream);
int32_t emb_gru_gate_grad(const void* x, const void* deter, const void* gout, int32_t dtype, int64_t rows,
                          int64_t width, int64_t blocks, void* dx, void* ddeter, void* stream);
/* Kernel launches the two entry points above have issued in this process,
 * counted where the kernels are launched.                                      */
int32_t emb_gru_gate_launches(int64_t* count);

/* ---- BlockLinear, the RSSM's block-diagonal product: the launch plan
 * `dynhid{i}` and `dyngru` of RSSM._core (dreamerv3/rssm.py:135-159) are
 * BlockLinear layers (embodied/jax/nets.py:254-281): x (rows, g * I), kernel W
 * (g, I, O), bias (g * O,),
 *   out[r, k O + o]  = sum_i x[r, k I + i] W[k, i, o] + bias[k O + o]   (nets.py:269-277)
 *   dx[r, k I + i]   = sum_o gout[r, k O + o] W[k, i, o]
 *   dW[k, i, o]      = sum_r x[r, k I + i] gout[r, k O + o],  dbias[k O + o] = sum_r gout[r, k O + o].
 * There are no kernels for it in this library yet; this is the host-side plan
 * they are to be launched by, exported so that it can be held on a CPU first.
 *   emb_block_linear_plan    the geometry of the three launches (forward, dx, dW +
 *                            dbias) for a shape and a mask of the outputs wanted:
 *                            grids, passes of the row loop, row splits of dW and
 *                            the workspace bytes for their partial sums.  Needs
 *                            no GPU and makes no HIP call.
 * EMB_ERR_INVALID: plan NULL, outputs no mask of EMB_BLOCK_LINEAR_*, rows < 0, g,
 * I or O below 1, g above 65535, I or O no multiple of 8 (16-byte rows of
 * bfloat16), more than 2^31 - 1 elements of x, out or W, or, where dW or dbias is
 * asked for, of workspace.  rows = 0: EMB_OK, all zeros.                       */
#define EMB_BLOCK_LINEAR_OUT 1
#define EMB_BLOCK_LINEAR_DX 2
#define EMB_BLOCK_LINEAR_DW 4
#define EMB_BLOCK_LINEAR_DBIAS 8
typedef struct emb_block_linear_launch {
  int64_t grid_x, grid_y, grid_z, block; /* all zero: not launched                    */
  int64_t passes;                        /* trips of a workgroup's row loop            */
  int64_t row_tile;                      /* rows a workgroup takes per trip            */
  int64_t col_tile, col_tiles;           /* output columns per workgroup, and how many */
  int64_t k_tile, k_steps;               /* of the other axis (summed, or I for dW)    */
} emb_block_linear_launch_t;
typedef struct emb_block_linear_plan {
  emb_block_linear_launch_t forward, grad_x, grad_w; /* grad_w: grid_z = splits, rows summed */
  int64_t splits, split_rows;  /* row splits of dW / dbias, rows of each (multiple of row_tile) */
  int64_t launches_grad_w;     /* 1, or 2 with more than one split                     */
  int64_t sum_grid_x;          /* the second launch's grid (block 256), 0 without      */
  int64_t workspace_bytes;     /* partial sums of dW / dbias, 0 with one split         */
  int64_t workspace_max_multiple; /* workspace_bytes <= this * bytes of dW, always     */
} emb_block_linear_plan_t;
int32_t emb_block_linear_plan(int64_t rows, int64_t g, int64_t I, int64_t O, int32_t outputs,
                              emb_block_linear_plan_t* plan);

/* ---- the draw of a one-hot latent or a discrete action, float32 arithmetic on device
 * DreamerV3 samples its stochastic state once per step of RSSM._observe and
 * RSSM.imagine, `self._dist(logit).sample(seed)` (dreamerv3/rssm.py:87, 100), and
 * the actor's action the same way (dreamerv3/agent.py:18, 126, 192), over OneHot /
 * Categorical (embodied/jax/outs.py:208-224 Categorical.__init__, pred, sample;
 * 243-254 OneHot.pred, sample; 265-270 _onehot_with_grad).  `logits` is
 * (rows, groups, classes), contiguous on device, EMB_F32 or EMB_BF16; group
 * g = row * groups + group.  Per group
 *   p = (1 - unimix) softmax(x) + unimix / classes                  (outs.py:212-216)
 *   u = uniform[g] (float32, in [0, 1)) or, with uniform NULL, Philox4x32-10 with
 *       key (seed & 0xffffffff, seed >> 32) and counter (g & 0xffffffff, g >> 32,
 *       offset & 0xffffffff, offset >> 32): u = (word 0 >> 8) * 2^-24.  The draw
 *       depends on (seed, offset, g) and on nothing else.
 *   EMB_SAMPLE_DRAW  index = the smallest k with p_k > 0 and C_k > u * C_last, C the
 *                    inclusive float32 prefix sum of p in class order; if rounding
 *                    leaves none, the last class with p > 0      (outs.py:222-224)
 *   EMB_SAMPLE_PRED  index = argmax(x), the first on ties; no uniform (outs.py:219-220)
 *   index[g]         int32; may be NULL
 *   onehot[g, :]     the logits' dtype, exactly 0 or 1: the value of
 *                    sg(onehot) + (probs - sg(probs)), outs.py:267-269; may be NULL
 * A group holding a NaN or +inf logit, or nothing but -inf, gets index -1 and a
 * one-hot row of NaN (a gradient of NaN); no other group is touched.  One kernel
 * launch each:
 *   emb_philox_uniform      out[i] = u(seed, offset, first + i), i < count, float32.
 *   emb_onehot_sample       the index and / or the one-hot.
 *   emb_onehot_sample_grad  grad (rows, groups, classes) in the logits' dtype from
 *                           gout, the gradient w.r.t. the one-hot, in that dtype:
 *                           (1 - unimix) s (gout - sum_k s_k gout_k), s = softmax(x),
 *                           the straight-through term of outs.py:268-269; it does not
 *                           depend on the draw.
 * `seed` and `offset` are passed by value: a captured graph replays the draw it
 * captured; fresh draws inside a graph come through `uniform`.
 * EMB_ERR_INVALID before any launch: an unknown dtype or mode, rows or count < 0,
 * groups < 1, classes outside 1 .. 256, more than 2^31 - 1 logits, unimix outside
 * [0, 1), and with work to do a NULL logits, gout, grad or out, or index and
 * onehot both NULL.  rows = 0 or count = 0: EMB_OK, nothing is launched.       */
#define EMB_SAMPLE_DRAW 0
#define EMB_SAMPLE_PRED 1
int32_t emb_philox_uniform(uint64_t seed, uint64_t offset, uint64_t first, int64_t count, void* out, void* stream);
int32_t emb_onehot_sample(const void* logits, int32_t dtype, int64_t rows, int64_t groups, int64_t classes,
                          float unimix, int32_t mode, uint64_t seed, uint64_t offset, const void* uniform,
                          void* index, void* onehot, void* stream);
int32_t emb_onehot_sample_grad(const void* logits, const void* gout, int32_t dtype, int64_t rows, int64_t groups,
                               int64_t classes, float unimix, void* grad, void* stream);
/* Kernel launches the three entry points above have issued in this process,
 * counted where the kernels are launched.                                      */
int32_t emb_onehot_sample_launches(int64_t* count);

/* ---- the reconstruction terms of the world-model loss, float32 arithmetic on device
 * Three terms of DreamerV3's loss (dreamerv3/agent.py:170-182) are sums of
 * elementwise errors over the trailing `units` elements of a row:
 *   the image loss    Agg(MSE(sigmoid(x)), 3, sum) against f32(frame) / 255
 *                     (dreamerv3/rssm.py:349, 353-356; agent.py:181)
 *   the vector loss   Agg(MSE(x, symlog), 1, sum)  (embodied/jax/heads.py:127-130,
 *                     embodied/jax/outs.py:129-141, embodied/jax/nets.py symlog)
 *   the continue head Binary(logit).loss(con)      (agent.py:177, outs.py:189-201)
 * under Agg (outs.py:40-58).  `x` is (rows, units) contiguous on device, EMB_F32 or
 * EMB_BF16; `target` the same shape in EMB_F32, EMB_BF16 or EMB_U8.  Per element
 * t = float32(target) / div in float32 (div = 255 for frames, 1 otherwise), and
 * with s(x) = 1 / (1 + exp(-x)), ls(x) = min(x, 0) - log1p(exp(-|x|)), g = gout[row]:
 *   EMB_RECON_MSE          loss = sum (x - t)^2                 grad = 2 (x - t) g
 *   EMB_RECON_MSE_SYMLOG   loss = sum (x - sign(t) log1p|t|)^2  grad = 2 (x - symlog t) g
 *   EMB_RECON_SIGMOID_MSE  loss = sum (s(x) - t)^2              grad = 2 (s(x) - t) s(x) (1 - s(x)) g
 *   EMB_RECON_BINARY       loss = sum -(t ls(x) + (1 - t) ls(-x))   grad = (s(x) - t) g
 * One kernel launch each, no atomics, the same bits from run to run and whatever
 * the alignment of the pointers:
 *   emb_recon_loss       loss (rows,) float32, each row summed in a fixed order.
 *   emb_recon_loss_grad  grad (rows, units) in the dtype of x from gout (rows,) float32.
 * A NaN or infinite x makes its own row's loss and its own gradient element NaN
 * and touches no other row.  Pointers may start on any multiple of their element
 * size.  EMB_ERR_INVALID before any launch: an unknown dtype or op, div not
 * positive and finite, rows < 0, units < 1, more than 2^31 - 1 elements, and with
 * work to do a NULL or misaligned pointer.  rows = 0: EMB_OK, nothing is launched. */
#define EMB_RECON_MSE 0
#define EMB_RECON_MSE_SYMLOG 1
#define EMB_RECON_SIGMOID_MSE 2
#define EMB_RECON_BINARY 3
int32_t emb_recon_loss(const void* x, int32_t x_dtype, const void* target, int32_t target_dtype, float div,
                       int64_t rows, int64_t units, int32_t op, void* loss, void* stream);
int32_t emb_recon_loss_grad(const void* x, int32_t x_dtype, const void* target, int32_t target_dtype, float div,
                            int64_t rows, int64_t units, int32_t op, const void* gout, void* grad, void* stream);
/* Kernel launches the two entry points above have issued in this process,
 * counted where the kernels are launched.                                      */
int32_t emb_recon_loss_launches(int64_t* count);

/* ---- the continuous policy head: Normal logp, entropy, policy loss and draw on device
 * The actor's loss of DreamerV3's imagination (dreamerv3/agent.py:411-415) for a
 * continuous action key, whose policy is Agg(Normal(mean, stddev), dims, sum)
 * (embodied/jax/outs.py:40-76 Agg, 161-186 Normal) as Head.bounded_normal and
 * Head.normal_logstd build it (embodied/jax/heads.py:146-162).  `mean_raw` and
 * `std_raw` are the two linear layers' outputs, (N, T, A) contiguous on device,
 * both EMB_F32 or both EMB_BF16 (the arithmetic is float32); `act` is (N, T, A)
 * float32 or NULL (no action: logpi = 0).  Per element
 *   EMB_NORMAL_BOUNDED  mean = tanh(m), std = (hi - lo) sigmoid(s + 2) + lo   (heads.py:150-152)
 *   EMB_NORMAL_LOGSTD   mean = m,       std = exp(s)                           (heads.py:161)
 *   z = (act - mean) / std
 *   logp_a = -z^2 / 2 - log(std) - log(2 pi) / 2                              (outs.py:174-176)
 *   ent_a  = log(2 pi std^2) / 2 + 1 / 2                                      (outs.py:178-179)
 * and per output row r = (n, t), t < T - drop, summed over the A action dimensions
 * in an order that A alone fixes (outs.py:63-64, 69-71):
 *   logpi = sum_a logp_a,  ent = sum_a ent_a
 *   loss  = weight[n * weight_stride + t] * -(logpi * adv[r] + actent * ent)
 * `adv` (N, T - drop) and `weight` are float32 constants; either may be NULL: 1.
 * `drop` is 0 or 1, the reference's [:, :-1]: a dropped step is not read.  One
 * kernel launch each, no atomics, the same bits from run to run and whatever the
 * alignment of the pointers:
 *   emb_normal_policy_loss       loss, logpi, ent (N, T - drop) float32; each may be
 *                                NULL (not written), not all three.
 *   emb_normal_policy_loss_grad  grad_mean, grad_std (N, T, A) in the inputs' dtype =
 *                                gout[r] * d loss[r] / d (m, s), the closed form
 *                                  d / d m_a = -w g adv (z / std) dmean/dm
 *                                  d / d s_a = -w g (adv (z^2 - 1) + actent) / std dstd/ds
 *                                from one more read of the inputs; a dropped step's
 *                                rows are written as zeros; T - drop may be 0.
 *   emb_normal_sample            act[e] = mean_e + std_e * eps_e (outs.py:170-172),
 *                                (rows, A) float32; eps (rows, A) float32 or, with eps
 *                                NULL, the draw below at e = row * A + a.
 *   emb_philox_normal            out[i] = eps(seed, offset, first + i), i < count: the
 *                                Philox4x32-10 block keyed as emb_philox_uniform's,
 *                                u1 = ((word 0 >> 8) + 1) * 2^-24 in (0, 1],
 *                                u2 = (word 1 >> 8) * 2^-24,
 *                                eps = sqrt(-2 ln u1) cos(2 pi u2).  It depends on
 *                                (seed, offset, e) and on nothing else.
 * `seed` and `offset` are passed by value: a captured graph replays the draw it
 * captured; fresh noise inside a graph comes through `eps`.
 * A NaN in m, s or act of a kept step makes that row's three outputs and its
 * gradient rows NaN and touches no other row.  EMB_NORMAL_BOUNDED stays finite
 * for m, s = +-1e4 (std is (hi - lo) * 0 + lo or (hi - lo) * 1 + lo, the gradient
 * to m exactly 0); EMB_NORMAL_LOGSTD returns what the float32 arithmetic above
 * returns when exp overflows (+-inf or NaN), confined to the row.
 * EMB_ERR_INVALID before any launch: an unknown dtype or kind, N, T, rows or
 * count < 0, drop outside {0, 1}, A outside 1 .. 256 (emb_normal_sample: A < 1),
 * more than 2^31 - 1 elements, EMB_NORMAL_BOUNDED without finite hi >= lo > 0, a
 * non-finite actent, weight_stride < T - drop, and with work to do a NULL input,
 * gradient, act or out, or loss, logpi and ent all NULL.  No output rows:
 * emb_normal_policy_loss launches nothing; emb_normal_policy_loss_grad still
 * writes its zeros unless N * T = 0.                                            */
#define EMB_NORMAL_BOUNDED 0
#define EMB_NORMAL_LOGSTD 1
int32_t emb_normal_policy_loss(const void* mean_raw, const void* std_raw, const void* act, int32_t dtype, int64_t N,
                               int64_t T, int32_t drop, int64_t A, int32_t kind, float lo, float hi, float actent,
                               const void* adv, const void* weight, int64_t weight_stride, void* loss, void* logpi,
                               void* ent, void* stream);
int32_t emb_normal_policy_loss_grad(const void* mean_raw, const void* std_raw, const void* act, int32_t dtype,
                                    int64_t N, int64_t T, int32_t drop, int64_t A, int32_t kind, float lo, float hi,
                                    float actent, const void* adv, const void* weight, int64_t weight_stride,
                                    const void* gout, void* grad_mean, void* grad_std, void* stream);
int32_t emb_normal_sample(const void* mean_raw, const void* std_raw, int32_t dtype, int64_t rows, int64_t A,
                          int32_t kind, float lo, float hi, uint64_t seed, uint64_t offset, const void* eps, void* act,
                          void* stream);
int32_t emb_philox_normal(uint64_t seed, uint64_t offset, uint64_t first, int64_t count, void* out, void* stream);
/* Kernel launches the four entry points above have issued in this process,
 * counted where the kernels are launched.                                      */
int32_t emb_normal_policy_launches(int64_t* count);

/* ---- device metrics: many small reductions in one launch, float32 on device --
 * The scalar book-keeping of a DreamerV3 train step.  One kernel family serves
 *   dreamerv3/agent.py:424-442  the metrics of imag_loss: adv.mean(), adv.std(),
 *                               |adv|.mean(), the means of rew, con, val, slowval,
 *                               tar_normed, weight and of every ents[k]; mean,
 *                               min, max and (|.| >= 1).mean() of
 *                               ret_normed = (ret - roffset) / rscale
 *   dreamerv3/agent.py:239-240  loss/{k} = v.mean() and
 *                               loss = sum([v.mean() * scales[k] ...])
 * in place of 25 to 30 torch launches each way.
 *
 * An entry is a float32 matrix view: `x`, rows >= 1, cols >= 1 and a row stride
 * in elements >= cols (x[:, :-1] of a contiguous (N, T) is cols = T - 1,
 * stride = T: no copy).  With a mode other than EMB_STAT_NONE the statistics are
 * those of x' = x * scale + offset (EMB_STAT_MUL_ADD) or (x - offset) / scale
 * (EMB_STAT_SUB_DIV, a true division), float32 operations in that order, where
 * `affine` is the DEVICE address of the float32 pair (offset, scale), read by
 * the kernel: words 3-4 of an emb_normalize state go in as they are.
 * emb_stat_rows gives every entry one workgroup, which writes
 *   out[e, 0] mean    out[e, 1] std (population, jnp.std)    out[e, 2] mean |x'|
 *   out[e, 3] min     out[e, 4] max    out[e, 5] rate = count(|x'| >= 1) / n
 * Sums are float64 in a fixed order without atomics: the same bits run to run
 * for the same inputs at the same addresses (a contiguous entry on a 16-byte
 * boundary is read with 16-byte loads, any other with 4-byte loads, which may
 * round a sum differently).  min and max return a NaN that is there (jnp.min,
 * jnp.max); a NaN never counts toward rate; a NaN or infinity in entry e
 * changes row e only.  One launch per EMB_STAT_MAX_ENTRIES entries; `out` is
 * (count, EMB_STAT_VALUES) float32.
 * `total` (NULL: none), agent.py:240: one more workgroup of the same launch
 * reduces every entry again and writes total[0] = 0 + out[0, 0] * weight_0 +
 * out[1, 0] * weight_1 + ..., float32, left to right as Python's sum(); it reads
 * no other workgroup's result, so its bits do not depend on their order.
 * EMB_ERR_INVALID before any HIP call: count < 0, and with count > 0 a NULL
 * `entries` or `out`, rows or cols < 1, stride < cols, an entry of more than
 * 2^31 - 1 elements, an unknown mode, a NULL `x` (or `affine` where the mode
 * reads it), an address off 4 bytes, `total` with more than
 * EMB_STAT_MAX_ENTRIES entries.  count = 0: EMB_OK, nothing is launched.        */
#define EMB_STAT_NONE 0
#define EMB_STAT_MUL_ADD 1
#define EMB_STAT_SUB_DIV 2
#define EMB_STAT_MAX_ENTRIES 48
#define EMB_STAT_VALUES 6
typedef struct emb_stat_entry {
  const void* x;
  const void* affine;
  int64_t rows, cols, stride;
  int32_t mode;
  float weight;
} emb_stat_entry_t;
int32_t emb_stat_rows(const emb_stat_entry_t* entries, int64_t count, void* out, void* total, void* stream);
/* The backward of agent.py:239-240: out_k[i] = (g[0] * scale_k) / n_k for every
 * element of every entry, `g` the device address of the float32 gradient of the
 * loss; one launch per EMB_STAT_MAX_ENTRIES entries.  EMB_ERR_INVALID before
 * any HIP call: count < 0, and with count > 0 a NULL `entries`, `g` or `out`, an
 * address off 4 bytes, n < 1 or n > 2^31 - 1.                                   */
typedef struct emb_fill_entry {
  void* out;
  int64_t n;
  float scale;
  int32_t reserved;
} emb_fill_entry_t;
int32_t emb_mean_fill(const emb_fill_entry_t* entries, int64_t count, const void* g, void* stream);
/* Kernel launches the two entry points above have issued in this process,
 * counted where the kernels are launched.                                      */
int32_t emb_stat_rows_launches(int64_t* count);

/* ---- device DictConcat: one-hot, squish, masks and concat in one launch ------
 * The first step of the world model's sequential scan and the head of the
 * Encoder.  One launch serves
 *   embodied/jax/nets.py:467-500  nn.DictConcat: per key available, mask, one_hot
 *                                 or squish, the cast, mask again, reshape; then
 *                                 concatenate
 *   embodied/jax/nets.py:80-99    available with bdims
 *   embodied/jax/nets.py:59-60    symlog(x) = sign(x) log1p(|x|)
 *   dreamerv3/rssm.py:76-79       mask(action, ~reset) in front of and behind it
 *   dreamerv3/rssm.py:97          the same DictConcat in RSSM.imagine
 *   dreamerv3/rssm.py:137         action /= sg(max(1, |action|))
 *   dreamerv3/rssm.py:216-220     DictConcat(vspace, 1, squish=symlog) of the Encoder
 * in place of twenty to thirty torch launches for a dict of two keys.
 *
 * `out` is (rows, width), EMB_F32 or EMB_BF16, its rows `out_stride` elements
 * apart (a column slice of a wider matrix is out_stride > width).  Entry k is a
 * contiguous (rows, elements) device array `x` of dtype EMB_F32, EMB_BF16,
 * EMB_I32, EMB_I64, EMB_U8 or EMB_BOOL that fills the columns [first, first +
 * span) of every row; the spans of the table tile [0, width) in any order.
 * Per row r and key k
 *   m = every element of x[r] != -inf (EMB_F32, EMB_BF16: a NaN is there) or
 *       != -1 (EMB_I32, EMB_I64); always for EMB_U8 and EMB_BOOL
 *   EMB_DICT_ONEHOT  span = elements * classes, column first + e * classes + c is
 *                    1 where m and x[r, e] == c, else 0.  The index is compared,
 *                    never used as an address: one outside [0, classes) gives
 *                    zeros (jax.nn.one_hot), and an EMB_I64 value beyond the
 *                    int32 range is outside, it is not wrapped (the reference's
 *                    astype(int32) never sees one: JAX runs without x64).
 *   EMB_DICT_NONE    span = elements, column first + e is x[r, e] as float32
 *                    where m, else 0
 *   EMB_DICT_SYMLOG  the same of sign(x) log1p(|x|)
 * `reset` (NULL: none) is one byte per row, uint8 or bool: a row whose byte is
 * not 0 is written as zeros (both masks of rssm.py:76-79).  With `unit` != 0
 * every continuous value v is stored as v / max(1, |v|) (rssm.py:137); one-hot
 * values pass.  Arithmetic is float32, rounded once at the store: the reference
 * divides after rounding, and for every finite v the two give the same bits
 * (|v| <= 1 stores the rounded v, anything else +-1).
 * No atomics: the same bits run to run.  16-byte stores wherever a row's own
 * address allows, element stores before and behind them.
 * EMB_ERR_INVALID before any HIP call, rows = 0 included: count outside
 * 1 .. EMB_DICT_MAX_KEYS, a NULL `table`, `out` or `x`, an unknown dtype or
 * kind, elements < 1, classes outside 1 .. 16 384, one-hot of a float input,
 * squish of an integer input, an address off its element size, spans that
 * overlap or do not tile [0, width), width outside 1 .. 16 384, out_stride <
 * width, rows < 0 or rows * out_stride > 2^31 - 1.  rows = 0: EMB_OK, nothing
 * is launched.                                                                */
#define EMB_DICT_ONEHOT 0
#define EMB_DICT_NONE 1
#define EMB_DICT_SYMLOG 2
#define EMB_DICT_MAX_KEYS 16
typedef struct emb_dict_entry {
  const void* x;
  int32_t dtype;    /* EMB_F32, EMB_BF16, EMB_I32, EMB_I64, EMB_U8, EMB_BOOL */
  int32_t kind;     /* EMB_DICT_*                                          */
  int32_t elements; /* per row                                             */
  int32_t classes;  /* EMB_DICT_ONEHOT only                                */
  int32_t first;    /* the key's first output column                       */
  int32_t reserved;
} emb_dict_entry_t;
int32_t emb_dict_concat(const emb_dict_entry_t* table, int64_t count, int64_t rows, int64_t width, void* out,
                        int64_t out_stride, int32_t out_dtype, const void* reset, int32_t unit, void* stream);
/* Kernel launches emb_dict_concat has issued in this process, counted where the
 * kernel is launched.                                                          */
int32_t emb_dict_concat_launches(int64_t* count);

/* ----------------------------------------------------------- collectives --
 * The two exchange steps of the sharded path on RCCL directly (xGMI inside one
 * node), for hosts that do not go through torch.distributed:
 *   trajectories  -> one all-gather of the packed (B, L, S) byte block per rank
 *                    (or all-to-all of its per-rank blocks: the DP slice)
 *   gradients     -> all-reduce (sum or mean) of one flat buffer
 *                    (embodied/jax/opt.py:52-54's pmean)
 * RCCL is opened with dlopen at the first call (the library itself does not
 * link against it).  Rank 0 makes the 128-byte id, the caller hands it to the
 * other ranks by whatever means it has (file, socket, torch.distributed
 * store), every rank calls emb_comm_init with the device it uses current.
 * Collectives are asynchronous on `stream`; buffers are caller-owned.         */
typedef struct emb_comm emb_comm_t;
#define EMB_COMM_ID_BYTES 128
int32_t emb_comm_unique_id(uint8_t* id_out /* [EMB_COMM_ID_BYTES] */);
int32_t emb_comm_init(const uint8_t* id, int32_t rank, int32_t world, emb_comm_t** out);
int32_t emb_comm_allgather_traj(emb_comm_t* comm, const void* send, void* recv,
                                int64_t bytes_per_rank, void* stream);
int32_t emb_comm_allreduce_grads(emb_comm_t* comm, void* buf, int64_t count, int32_t mean,
                                 void* stream);
/* The same with the element type named (EMB_F16 / EMB_BF16 / EMB_F32 / EMB_F64):
 * bf16 gradients halve the bytes on the links.                  */
int32_t emb_comm_allreduce_grads_as(emb_comm_t* comm, void* buf, int64_t count, int32_t dtype,
                                    int32_t mean, void* stream);
/* DP-slice exchange (SURVEY.md 8e "only its DP slice via all-to-all"): `send`
 * and `recv` hold `world` blocks of bytes_per_rank bytes; block r of `send`
 * goes to rank r, block r of `recv` arrives from rank r (block `rank` is a
 * local copy).  One fused group of RCCL point-to-point transfers.            */
int32_t emb_comm_alltoall_slices(emb_comm_t* comm, const void* send, void* recv,
                                 int64_t bytes_per_rank, void* stream);
/* Normaliser statistics over the data-parallel ranks (embodied/jax/utils.py:76-88;
 * used by the agents' return / advantage / value normalisers, ppo/agent.py:35-36,
 * dreamerv3/agent.py:70-72).
 * allgather_returns: every rank's `count` float32 values -> recv[world * count],
 *   rank order: the `perc` normaliser's jax.lax.all_gather in front of
 *   jnp.percentile (utils.py:83-88).
 * pmean_scalars: in-place mean over the ranks of `count` float32 values: the
 *   jax.lax.pmean of Normalize._mean (utils.py:76-81).                         */
int32_t emb_comm_allgather_returns(emb_comm_t* comm, const void* send, void* recv, int64_t count,
                                   void* stream);
int32_t emb_comm_pmean_scalars(emb_comm_t* comm, void* values, int64_t count, void* stream);

/* One train step's exchange, asynchronous on the communicator's OWN stream so
 * that it overlaps what the caller queues next (the reference hands train
 * outputs out one step late for the same reason, embodied/jax/agent.py:286-294):
 * the collectives start after everything queued on `after_stream` so far --
 * first the slices (bytes_per_rank > 0), then the gradients (count > 0).
 * emb_comm_wait makes `stream` wait for the exchange issued last; buffers stay
 * the caller's and must live until then.  Host cost: two event records and two
 * stream waits per train step, whatever the number of collectives.            */
int32_t emb_comm_exchange(emb_comm_t* comm, void* after_stream, const void* slices_send,
                          void* slices_recv, int64_t bytes_per_rank, void* grads, int64_t count,
                          int32_t dtype, int32_t mean);
/* The same with the trajectory ALL-GATHER in front of the gradients instead of the
 * DP-slice all-to-all (north_star's "RCCL all-gather of trajectories"; the
 * reference assembles every process's batch slice into the global batch,
 * embodied/jax/internal.py:145-152): `traj_send` = this rank's bytes_per_rank
 * bytes, `traj_recv` = world * bytes_per_rank bytes in rank order.  (ABI 5)    */
int32_t emb_comm_exchange_gather(emb_comm_t* comm, void* after_stream, const void* traj_send,
                                 void* traj_recv, int64_t bytes_per_rank, void* grads,
                                 int64_t count, int32_t dtype, int32_t mean);
int32_t emb_comm_wait(emb_comm_t* comm, void* stream);
int32_t emb_comm_destroy(emb_comm_t* comm);

/* ---- synthetic vector env (benchmark / test input) ---------- */
/* Episode logic of embodied/envs/dummy.py:38-48 for n device-resident envs;
 * counters = device int32[2][2n] state in two generations: the step reads
 * generation `turn` (0/1) and writes the other one (the caller alternates);
 * reset = device u8[n] or NULL.                                               */
int32_t emb_synth_env_step(void* image, void* reward, void* is_first, void* is_last,
                           void* is_terminal, int64_t n, int64_t frame_bytes, int64_t env0,
                           int64_t episode_len, const void* reset, void* counters,
                           int32_t turn, void* stream);
/* The same step with the Driver's action mask (driver.py:72-75) inside the
 * launch: `act` = the policy's raw actions, device (n, row_bytes) of `dtype`
 * (EMB_U8 ...); the launch also stores act * !reset[e], a real multiply in
 * `dtype`, to `masked_out` -- the env's input -- and the env uses nothing but
 * that product.  `reset` must be given (the Driver passes the previous step's
 * is_last).  Keys: those emb_env_mask_supported accepts (1..256 elements per
 * row: what a carried publish takes, emb_replay_carry_publish); anything else
 * is EMB_ERR_INVALID.  No extra launch: with emb_replay_carry_publish an env
 * step is two dependent launches instead of three.                             */
int32_t emb_synth_env_step_masked(void* image, void* reward, void* is_first, void* is_last,
                                  void* is_terminal, int64_t n, int64_t frame_bytes,
                                  int64_t env0, int64_t episode_len, const void* reset,
                                  void* counters, int32_t turn, const void* act,
                                  void* masked_out, int64_t row_bytes, int32_t dtype,
                                  void* stream);
/* 1 if an action key of this row size and dtype can be masked inside a device
 * env's step launch (and carried by the replay), else 0.                        */
int32_t emb_env_mask_supported(int64_t row_bytes, int32_t dtype);
/* The masked step's arguments as one block (emb_synth_env_step_fused).          */
typedef struct {
  void *image, *reward, *is_first, *is_last, *is_terminal;
  int64_t n, frame_bytes, env0, episode_len;
  const void* reset;
  void* counters;
  const void* act;
  void* masked_out;
  int64_t row_bytes;
  int32_t turn, dtype;
} emb_synth_step_t;
/* The masked step AND the early insert of the step it produces
 * (emb_replay_obs_stack_insert with frames = env->image) in ONE launch: the
 * workgroup that generates a frame slice stores it to the env's image buffer,
 * to its pool row and, cast as `spec` says, to the policy batch `dst`; reward
 * and flags go to the env's buffers and to their pool rows from registers; the
 * carried publish rides along.  An env step is one launch instead of two.
 * The other arguments are emb_replay_obs_stack_insert's; `src[k]` of an
 * observation key is the env's buffer for it.
 *   *token_out != 0: launched; go on with emb_replay_publish(token) as after
 *     emb_replay_obs_stack_insert.  The policy batch is in `dst`.
 *   *token_out == 0 (and EMB_OK): nothing was launched and neither handle nor
 *     env state changed -- the rows of the step are not predicted (the helper
 *     thread would have to be waited for) or EMB_STEP_FUSED=0 is set.  Make the
 *     two launches (emb_synth_env_step_masked, emb_replay_obs_stack_insert).
 *   EMB_ERR_INVALID, nothing launched: the launch cannot take this step at all
 *     -- the plan fails the early insert's own checks, frames are not 4-channel
 *     uint8 in env->image, a narrow key's source is not one of the env's four
 *     output buffers (reward as 4-byte rows, the flags as 1-byte rows), the flag
 *     buffers are not within 32-bit offsets of `reward`, or the action key is
 *     not one emb_env_mask_supported accepts.  Two launches, as before.        */
int32_t emb_synth_env_step_fused(emb_replay_t* rep, int64_t n, const int64_t* workers, int32_t frame_key,
                                 const emb_synth_step_t* env, const emb_obs_spec_t* spec, void* dst,
                                 const void* const* src, void* stream, uint64_t* token_out);

/* ---- direct xGMI schedule (round 5) ----------------------------------------
 * The two collectives of a train step -- the gradient all-reduce
 * (embodied/jax/opt.py:52-54) and the DP-slice all-to-all
 * (embodied/jax/internal.py:145-152) -- without RCCL: every rank writes its
 * peers' shares straight into their memory (hipIpc handles of one uncached,
 * fine-grained allocation per rank), all n-1 peers at once, one xGMI link each; flags in that
 * memory order the steps (csrc/direct_comm.hip states the schedule).  One node,
 * at most 8 ranks, one GPU per rank (or several ranks on one GPU: the tests).
 *
 * create: max_reduce_bytes = the largest gradient buffer, max_block_bytes = the
 *         largest all-to-all / all-gather block (bytes per rank); every wait
 *         inside a kernel gives up after timeout_ms.  A time-out is FATAL for
 *         the communicator (RCCL would keep waiting; a bounded wait must not
 *         turn into a silently wrong gradient): the kernel that gave up writes
 *         no result and raises no peer's flag, every later kernel returns at
 *         once and every later call of allreduce / alltoall / allgather /
 *         exchange / wait returns an error (the word is read from host-mapped
 *         memory, no synchronisation); emb_direct_status synchronises and
 *         reports it.  Choose timeout_ms like a collective watchdog (minutes),
 *         not like a latency bound.
 * handle / connect: each rank's 64-byte handle reaches every other rank by the
 *         caller's means (a process-group all-gather, a file); connect takes all
 *         `world` handles in rank order.
 * allreduce / alltoall / allgather: asynchronous on `stream`; same order of
 *         calls on every rank.  Results: the sum is taken in rank order in f32 by
 *         the rank that owns the shard and broadcast, so every rank holds the
 *         same bits.  The all-reduce buffer must be 16-byte aligned.  allgather
 *         (ABI 5): this rank's bytes_per_rank bytes reach every peer, all n-1
 *         links at once; recv = world * bytes_per_rank bytes in rank order.
 * exchange / exchange_gather / wait: emb_comm_exchange[_gather]'s contract on
 *         the transport's own stream.                                         */
#define EMB_DIRECT_HANDLE_BYTES 64
typedef struct emb_direct emb_direct_t;
int32_t emb_direct_create(int32_t rank, int32_t world, int64_t max_reduce_bytes,
                          int64_t max_block_bytes, int32_t timeout_ms, emb_direct_t** out);
int32_t emb_direct_handle(emb_direct_t* d, uint8_t* handle_out);
int32_t emb_direct_connect(emb_direct_t* d, const uint8_t* handles);
int32_t emb_direct_allreduce(emb_direct_t* d, void* buf, int64_t count, int32_t dtype,
                             int32_t mean, void* stream);
int32_t emb_direct_alltoall(emb_direct_t* d, const void* send, void* recv,
                            int64_t bytes_per_rank, void* stream);
int32_t emb_direct_exchange(emb_direct_t* d, void* after_stream, const void* slices_send,
                            void* slices_recv, int64_t bytes_per_rank, void* grads,
                            int64_t count, int32_t dtype, int32_t mean);
int32_t emb_direct_allgather(emb_direct_t* d, const void* send, void* recv,
                             int64_t bytes_per_rank, void* stream);
int32_t emb_direct_exchange_gather(emb_direct_t* d, void* after_stream, const void* traj_send,
                                   void* traj_recv, int64_t bytes_per_rank, void* grads,
                                   int64_t count, int32_t dtype, int32_t mean);
int32_t emb_direct_wait(emb_direct_t* d, void* stream);
/* The watchdog of the launches from now on (a short one while a set-up is being
 * checked, minutes for the job itself).  (ABI 5)                               */
int32_t emb_direct_set_timeout(emb_direct_t* d, int32_t timeout_ms);
int32_t emb_direct_status(emb_direct_t* d, int32_t* timed_out);
int32_t emb_direct_destroy(emb_direct_t* d);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* EMBODIED_HIP_H_ */
