/*
 * zbot_ppo.h — C ABI of the post-rollout PPO inputs,
 * exported by libzbot_hip.so next to the engine (include/zbot.h).
 *
 * Replaces ksim 0.1.99's PPO input computation (un-vendored ksim/task/ppo.py
 * `compute_ppo_inputs` [U]; its caller is PPOTask after the rollout scan whose
 * per-step critic values come from get_ppo_variables, train.py:1683-1729):
 *
 *   values_shifted[t] = values[t+1]            (t < T-1)
 *                     = bootstrap[e] or values[T-1]   (t = T-1; ksim uses the
 *                                               last value as bootstrap [U])
 *   mask[t]  = 1 - done[t]
 *   next[t]  = success[t] ? values[t] : values_shifted[t] * mask[t]   [U]
 *   delta[t] = reward[t] + gamma * next[t] - values[t]
 *   gae[t]   = fma((gamma * lam) * mask[t], gae[t+1], delta[t])  (reverse
 *              scan, gae[T] = 0; one rounding per step)
 *   value_targets[t] = gae[t] + values[t]
 *   advantages = (gae - mean(gae)) / (std(gae) + eps)   (normalize_advantages,
 *                population std over the whole batch — every env, every step,
 *                every rank)
 *
 * Layout: every [T, n] array is time-major with the env axis contiguous, i.e.
 * exactly the buffers zb_step writes when the caller hands it row t of a
 * [T, n] reward / done rollout buffer. Values are the critic outputs for the
 * same rows. All pointers are device pointers; calls are asynchronous on
 * `stream` and allocate nothing (graph-capturable).
 *
 * Determinism: the batch moments are sums in fp64 over a fixed pairwise tree
 * whose leaves are envs (per-env time sums first, in an order fixed by T:
 * oracle/zb_oracle_ppo.c zbo_gae).
 * When every rank holds the same power-of-two number of envs (a multiple of
 * ZB_GAE_ENVS_PER_BLOCK), combining the per-rank moments with
 * zb_moments_combine in rank order reproduces the single-GPU tree bit for
 * bit, so normalized advantages do not depend on the world size.
 */
#ifndef ZBOT_PPO_H
#define ZBOT_PPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZB_GAE_ENVS_PER_BLOCK 32  /* envs per workgroup of zb_gae (leaf group of the moment tree) */

/* Number of fp64 words of the `partials` scratch zb_gae needs for n envs. */
size_t zb_gae_partials_words(int n);

/*
 * GAE + value targets over a [T, n] rollout.
 *   reward, values  [T, n] fp32      done [T, n] uint8
 *   success         [T, n] uint8 (nullable: no successful terminations)
 *   bootstrap       [n] fp32 (nullable: values[T-1], ksim's convention [U])
 *   gae_out         [T, n] fp32  unnormalized GAE (may alias nothing else)
 *   value_targets   [T, n] fp32  (nullable)
 *   partials        [zb_gae_partials_words(n)] fp64 scratch (nullable: no
 *                   moments); filled with per-block (sum, sum of squares)
 *   moments_out     [2] fp64 (nullable): (sum, sum of squares) of gae over
 *                   this call's T*n elements, reduced over `partials` by the
 *                   fixed pairwise tree. Requires partials.
 */
int zb_gae(const float* reward, const float* values, const uint8_t* done, const uint8_t* success,
           const float* bootstrap, int T, int n, float gamma, float lam, float* gae_out,
           float* value_targets, double* partials, double* moments_out, void* stream);

/*
 * Pairwise-tree combine of `k` (sum, sum of squares) pairs stored as
 * moments[2*k] (device, fp64) into out[2] (device). Used for the per-rank
 * moments after an all-gather (rank order), so every rank normalizes with
 * the same bits.
 */
int zb_moments_combine(const double* moments, int k, double* out, void* stream);

/*
 * advantages[i] = (gae[i] - mean) / (std + eps) for i < count, where
 * mean = moments[0] / total, std = sqrt(max(moments[1] / total - mean^2, 0))
 * and `total` is the number of elements the moments cover (T * n_global).
 * In place when advantages == gae.
 */
int zb_adv_normalize(const float* gae, float* advantages, long long count, const double* moments,
                     double total, float eps, void* stream);

/*
 * ---- Learner: PPO loss seeds, global-norm clip and AdamW ----
 *
 * The three steps of an optimizer step around the networks' backward pass
 * (include/zbot_policy.h "Training"):
 *
 *   zb_policy_actor_train / zb_policy_critic_train       log_prob, values
 *   zb_ppo_loss                                          -> d_log_prob, d_value, sums
 *   zb_policy_actor_backward / zb_policy_critic_backward -> one flat gradient per network
 *   zb_grad_sqnorm (one per network)                     -> sqnorms[k]
 *     (several ranks: an all-gather of the gradient and zb_grad_combine instead, which sums the
 *      ranks' gradients and returns the sum's squared norm)
 *   zb_adamw_step  (one per network, the same sqnorms)   params, m, v in place
 *   zb_policy_set_params
 *
 * Element arithmetic: include/zbot_learner_math.h, whose operation order is
 * the definition. The loss is ksim's PPO loss [U] as zbot_amd.learner.ppo_loss
 * states it (clipped surrogate on the log-probs summed over the 20 joints,
 * clipped value loss, means over `total` rows; no entropy term); the update is
 * optax.clip_by_global_norm -> optax.adamw [U] (train.py:1314-1324).
 *
 * All pointers are device pointers; every call is asynchronous on `stream`,
 * allocates nothing and synchronizes nothing. Bad arguments return ZB_EARG and
 * launch nothing.
 *
 * Reduction tree: every sum (the four loss sums over rows, the squared norm
 * over elements) is the balanced pairwise tree over its leaves in index order,
 * zero-padded to a power of two, combined in fp64; the root is then added to
 * +0.0 (so a sum of negative zeros reads +0 whatever the padding). Adding
 * zeros is exact, so the result depends neither on the launch shape nor, for
 * power-of-two shards combined in rank order, on the world size. No
 * floating-point atomics anywhere.
 *
 * The *_host functions take host pointers, run the same header and the same
 * tree on the CPU, and are the bit reference of the kernels.
 */
#define ZB_LOSS_ROWS_PER_BLOCK 256     /* rows (leaves) per partial of zb_ppo_loss */
#define ZB_SQNORM_ELEMS_PER_BLOCK 4096 /* elements (leaves) per partial of zb_grad_sqnorm */

/* fp64 words of the `partials` scratch zb_ppo_loss needs for a [T, n] batch (0: bad size). */
size_t zb_ppo_loss_partials_words(int T, int n);

/*
 * PPO loss seeds and sums over the T*n rows of a [T, n] minibatch.
 *   log_prob, old_log_prob    [T, n, 20] fp32
 *   advantages, values, old_values, value_targets  [T, n] fp32
 *   total          rows the means run over: T*n here, T*n_global when ranks share a batch
 *   d_log_prob     [T, n, 20] fp32: d loss / d log_prob (the same value for a row's 20 joints)
 *   d_value        [T, n] fp32: d loss / d values
 *   partials       [zb_ppo_loss_partials_words(T, n)] fp64 scratch
 *   sums_out       [4] fp64 over this call's rows: sum S, sum Vt, sum [|ratio - 1| > clip_param],
 *                  sum ((ratio - 1) - log ratio). loss = -sums[0] / total
 *                  + value_loss_coef * 0.5 * sums[1] / total; sums[2] / total is the clip
 *                  fraction, sums[3] / total an approximate KL.
 * T >= 1, n >= 1, T*n <= 2^28, total > 0, clip_param >= 0, log_clip_value >= 0. Outputs alias no input.
 */
int zb_ppo_loss(const float* log_prob, const float* old_log_prob, const float* advantages, const float* values,
                const float* old_values, const float* value_targets, int T, int n, double total, float clip_param,
                float value_loss_coef, int use_clipped_value_loss, float log_clip_value, float* d_log_prob,
                float* d_value, double* partials, double* sums_out, void* stream);
int zb_ppo_loss_host(const float* log_prob, const float* old_log_prob, const float* advantages, const float* values,
                     const float* old_values, const float* value_targets, int T, int n, double total,
                     float clip_param, float value_loss_coef, int use_clipped_value_loss, float log_clip_value,
                     float* d_log_prob, float* d_value, double* sums_out);

/* fp64 words of the `partials` scratch zb_grad_sqnorm needs for `count` elements. */
size_t zb_sqnorm_partials_words(size_t count);

/*
 * out[0] = sum_i grad[i]^2 (fp64; the square of an fp32 value is exact there), by the tree above.
 * 1 <= count <= 2^32.
 */
int zb_grad_sqnorm(const float* grad, size_t count, double* partials, double* out, void* stream);
int zb_grad_sqnorm_host(const float* grad, size_t count, double* out);

/*
 * The gradient sum over ranks, by the tree above instead of a collective's own order: `parts` is
 * [world][count] fp32, densely packed (the destination of an all-gather of every rank's flat
 * gradient, row r from rank r). For every i < count
 *   grad[i] = (float)(tree over the world leaves (double)parts[r][i], r ascending)
 * i.e. the leaves zero-padded to a power of two, combined in fp64 by the balanced pairwise tree,
 * the root added to +0.0 and rounded to fp32 once. Every rank that holds the same `parts` gets the
 * same bits, whatever ring or tree moved them.
 *   partials   [zb_sqnorm_partials_words(count)] fp64 scratch
 *   sq_out     [1] fp64: bit for bit what zb_grad_sqnorm returns on the `grad` just written (the
 *              same leaves and tree; the combined gradient is read once, not twice)
 * 1 <= world <= ZB_COMBINE_MAX_WORLD, 1 <= count <= 2^32; grad must not overlap parts. Rows are read
 * in 16-byte accesses when parts, grad and every row start are 16-byte aligned, else in 4-byte ones.
 */
#define ZB_COMBINE_MAX_WORLD 64
int zb_grad_combine(const float* parts, int world, size_t count, float* grad, double* partials, double* sq_out,
                    void* stream);
int zb_grad_combine_host(const float* parts, int world, size_t count, float* grad, double* sq_out);

/*
 * One AdamW step behind the global-norm clip, in place on param, m, v [count] (fp32):
 *   N = sqrt(sqnorms[0] + ... + sqnorms[k-1])  (fp64, index order): the joint norm of k gradients,
 *       e.g. the actor's and the critic's, each from zb_grad_sqnorm;
 *   scale = (float)(max_grad_norm / N) if max_grad_norm > 0 and N > max_grad_norm, else exactly 1;
 *   zbl_adamw (zbot_learner_math.h) on elements 0 .. count - frozen_tail - 1.
 * The last `frozen_tail` elements of param, m and v are left untouched (the actor's 20 mean
 * offsets, constants of the model). `step` >= 1 is the number of this step, counted by the caller;
 * the bias corrections 1 - beta^step are formed from it on the host in fp64. beta1 and beta2 are
 * doubles because 1 - beta is formed from them too, in fp64, and rounded once (zbot_learner_math.h). It is passed by value:
 * a captured graph replays the step number it was captured with, so capture would freeze the bias
 * correction; launch this call outside a graph, or re-capture per step.
 * 1 <= k <= 64, 0 <= beta < 1, lr, eps, weight_decay >= 0.
 */
int zb_adamw_step(float* param, const float* grad, float* m, float* v, size_t count, size_t frozen_tail,
                  const double* sqnorms, int k, float max_grad_norm, float lr, double beta1, double beta2, float eps,
                  float weight_decay, int step, void* stream);
int zb_adamw_step_host(float* param, const float* grad, float* m, float* v, size_t count, size_t frozen_tail,
                       const double* sqnorms, int k, float max_grad_norm, float lr, double beta1, double beta2,
                       float eps, float weight_decay, int step);

/*
 * ---- Minibatches: the keyed permutation and the gather that cuts a minibatch ----
 *
 * A PPO pass visits the rollout's n envs in minibatches. With shuffling, minibatch k of pass
 * `epoch` is positions [k batch, (k + 1) batch) of the permutation
 *   p(i) = zbf_perm_index(seed, epoch, n, i)      (include/zbot_fmath.h; integers only, the same
 *                                                  bits on host and device)
 * ksim shuffles with its own RNG [U]; this law is this library's.
 *
 * zb_minibatch_gather moves every array of one minibatch in one launch: for every item and every
 * t < rows, j < count
 *   dst[t][j][:] = src[t][p(lo + j)][:]           (p the identity when shuffle == 0)
 * The source of an item is [rows][n][row_bytes] with an explicit stride between time rows
 * (src_t_stride_bytes >= 0: the first T rows of a [T + 1, n, 50] buffer are an item; a carry is
 * rows = 1); the destination is dense [rows][count][row_bytes]. src == NULL zero-fills (row 0 of
 * `reset` in a first rollout). Each item moves in the widest of 16-, 8-, 4- and 1-byte accesses
 * that divides its row_bytes, both pointers and (with rows > 1) its stride. Sources and
 * destinations must not overlap.
 *
 * `items` is a host array (read during the call, passed to the kernel by value); the pointers in
 * it are device pointers (host pointers for zb_minibatch_gather_host). Asynchronous on `stream`,
 * nothing allocated, nothing synchronized. Bad arguments (a null items / dst, n_items outside
 * 1 .. ZB_GATHER_MAX_ITEMS, n < 1, lo < 0, count < 1, lo + count > n, rows < 1, row_bytes outside
 * 1 .. ZB_GATHER_MAX_ROW_BYTES, a negative stride) return ZB_EARG and launch nothing.
 */
#define ZB_GATHER_MAX_ITEMS 16
#define ZB_GATHER_MAX_ROW_BYTES (1 << 24) /* per env and time row */

typedef struct ZbGatherItem {
  const void* src;            /* [rows][n][row_bytes], time stride src_t_stride_bytes; NULL: zeros */
  void* dst;                  /* [rows][count][row_bytes], dense */
  int32_t rows;
  int32_t row_bytes;
  int64_t src_t_stride_bytes;
} ZbGatherItem;

/* perm[i] = zbf_perm_index(seed, epoch, n, i) for i < n (n >= 1). For callers and tests: the
   gather evaluates the permutation itself. */
int zb_minibatch_perm(uint64_t seed, uint32_t epoch, int n, int32_t* perm, void* stream);
int zb_minibatch_perm_host(uint64_t seed, uint32_t epoch, int n, int32_t* perm);

int zb_minibatch_gather(const ZbGatherItem* items, int n_items, int n, int lo, int count, int shuffle,
                        uint64_t seed, uint32_t epoch, void* stream);
int zb_minibatch_gather_host(const ZbGatherItem* items, int n_items, int n, int lo, int count, int shuffle,
                             uint64_t seed, uint32_t epoch);

/*
 * ---- Chunked minibatches: the gather of truncated BPTT with stored carries ----
 * Added in ABI version 6 (zb_minibatch_gather_seq, zb_minibatch_gather_seq_host).
 *
 * A rollout of T steps is cut into C = T / seq_len chunks of L = seq_len steps, and every env of
 * a minibatch contributes its C chunks as C sequences: the networks then run on [L, C count]
 * instead of [T, count]. The envs of the minibatch are the same as without chunks: positions
 * [lo, lo + count) of the same permutation p over the n envs.
 *
 * zb_minibatch_gather_seq is zb_minibatch_gather with one more law. cut[k] != 0 marks item k as a
 * time item: its rows (= T, a multiple of seq_len) are cut in chunks, and for l < L, c < C,
 * j < count
 *   dst[l][c count + j][:] = src[c L + l][p(lo + j)][:]
 * with dst dense [L][C count][row_bytes] (the same bytes in all as [rows][count][row_bytes]).
 * cut[k] == 0 leaves item k to zb_minibatch_gather's law dst[r][j] = src[r][p(lo + j)]: the
 * carries stored at the chunk starts are such an item with rows = C, whose destination
 * [C][count][...] read as C count sequences has the same column order q = c count + j; a
 * whole-run carry is one with rows = 1. Column q of every item is so chunk c of env p(lo + j).
 * With seq_len == rows a time item moves as in zb_minibatch_gather.
 *
 * Everything else is zb_minibatch_gather's: the explicit source time stride, src == NULL
 * zero-fills, the access width per item, `items` and `cut` host arrays read during the call,
 * asynchronous on `stream`, nothing allocated. Bad arguments (zb_minibatch_gather's, a null cut,
 * seq_len < 1, a time item whose rows are no multiple of seq_len) return ZB_EARG and launch
 * nothing.
 */
int zb_minibatch_gather_seq(const ZbGatherItem* items, const int32_t* cut, int n_items, int seq_len, int n, int lo,
                            int count, int shuffle, uint64_t seed, uint32_t epoch, void* stream);
int zb_minibatch_gather_seq_host(const ZbGatherItem* items, const int32_t* cut, int n_items, int seq_len, int n,
                                 int lo, int count, int shuffle, uint64_t seed, uint32_t epoch);

/*
 * ---- Rollout summary: every sum a rollout's telemetry needs, in one fixed-order reduction ----
 * Added in ABI version 5 (zb_rollout_summary_partials_words, zb_rollout_summary,
 * zb_rollout_summary_host).
 *
 * One pass over the T*n rows of a finished rollout, in (t, env) order, into ZB_SUMMARY_WORDS fp64
 * words (zbot_amd.metrics.rollout_telemetry turns them into means, rates and the explained
 * variance):
 *
 *   ZB_SUM_TERMS + i        sum of reward term i (i < 12, include/zbot.h ZB_T_*)
 *   ZB_SUM_CMD_TERMS + i    sum of command term i (i < 5, include/zbot_command.h)
 *   ZB_SUM_REWARD, _SQ      sum of reward, of reward^2
 *   ZB_SUM_DONE, _SUCCESS   number of rows with done != 0, with success != 0
 *   ZB_SUM_LOG_PROB         sum over rows of the row's log-prob: its 20 joints, the first converted
 *                           to fp64 and the others added to it in joint order in fp64
 *   ZB_SUM_VALUE, _SQ       sum of value, of value^2
 *   ZB_SUM_TARGET, _SQ      sum of value target, of target^2
 *   ZB_SUM_RESIDUAL_SQ      sum of (target - value)^2
 *   ZB_SUM_ROWS             the row count T*n (a leaf of 1.0 per row)
 *   28 .. 31                +0.0
 *
 * A leaf is formed in fp64 from the fp32 (or uint8) inputs: squares and the difference are taken
 * after the conversion. The words of a null plane are +0.0. Every word is reduced over the rows by
 * the "Reduction tree" above (balanced pairwise tree, zero-padded to a power of two, adjacent pairs
 * first, fp64, root + 0.0; no floating-point atomics): a workgroup reduces ZB_LOSS_ROWS_PER_BLOCK
 * rows for all words at once into one partial of ZB_SUMMARY_WORDS words, and a second,
 * single-workgroup launch runs the tree over the partials.
 *
 *   reward_terms   [T, n, 12] fp32 (nullable)     command_terms [T, n, 5] fp32 (nullable)
 *   reward         [T, n] fp32                    done [T, n] uint8; success [T, n] uint8 (nullable)
 *   log_prob       [T, n, 20] fp32 (nullable)
 *   values, value_targets  [T, n] fp32 (nullable, both or neither)
 *   partials       [zb_rollout_summary_partials_words(T, n)] fp64 scratch
 *   sums_out       [ZB_SUMMARY_WORDS] fp64
 * T >= 1, n >= 1, T*n <= 2^28. A workgroup's share of a plane is contiguous and starts on a multiple
 * of 16 bytes from the plane's start, so each plane whose pointer is 16-byte aligned is read in
 * 16-byte accesses (whatever its row size: 48, 20, 80, 4 bytes or 1), the others in 4-byte ones
 * (single bytes for the uint8 planes). Device pointers; asynchronous on `stream`, nothing
 * allocated, nothing synchronized; bad arguments return ZB_EARG and launch nothing. The host twin
 * takes host pointers, forms the same leaves and runs the same tree: the kernel's bit reference.
 */
#define ZB_SUMMARY_WORDS 32
#define ZB_SUM_TERMS 0
#define ZB_SUM_CMD_TERMS 12
#define ZB_SUM_REWARD 17
#define ZB_SUM_REWARD_SQ 18
#define ZB_SUM_DONE 19
#define ZB_SUM_SUCCESS 20
#define ZB_SUM_LOG_PROB 21
#define ZB_SUM_VALUE 22
#define ZB_SUM_VALUE_SQ 23
#define ZB_SUM_TARGET 24
#define ZB_SUM_TARGET_SQ 25
#define ZB_SUM_RESIDUAL_SQ 26
#define ZB_SUM_ROWS 27
#define ZB_SUM_USED 28 /* words below this index carry a sum */

/* fp64 words of the `partials` scratch zb_rollout_summary needs for a [T, n] rollout (0: bad size). */
size_t zb_rollout_summary_partials_words(int T, int n);

int zb_rollout_summary(const float* reward_terms, const float* command_terms, const float* reward,
                       const uint8_t* done, const uint8_t* success, const float* log_prob, const float* values,
                       const float* value_targets, int T, int n, double* partials, double* sums_out, void* stream);
int zb_rollout_summary_host(const float* reward_terms, const float* command_terms, const float* reward,
                            const uint8_t* done, const uint8_t* success, const float* log_prob, const float* values,
                            const float* value_targets, int T, int n, double* sums_out);

#ifdef __cplusplus
}
#endif
#endif /* ZBOT_PPO_H */
