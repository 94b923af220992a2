/*
 * zbot_policy.h — C ABI of the GRU policy/value networks in the rollout loop
 * (SURVEY.md §8f row f1), exported by libzbot_hip.so next to the engine.
 *
 * Replaces, for N environments at once (train.py, ZbotWalkingTask):
 *   Actor.forward + MixtureOfGaussians sample / mode / log_prob
 *       train.py:885-967 (Actor), :1616-1643 (run_actor), :1737-1763
 *       (sample_action), :1683-1729 (get_ppo_variables' log_probs)
 *   Critic.forward   train.py:970-1023 (Critic), :1645-1681 (run_critic)
 * with hidden_size 128, depth 5, num_mixtures 5, min_std 0.01, max_std 1.0,
 * var_scale 1.0 (train.py:1068-1079, 1604-1614, 1040-1057).
 *
 * Per layer (equinox GRUCell, un-vendored equinox [U]):
 *   ig = W_ih x + b        hg = W_hh h
 *   r = sigmoid(ig_r + hg_r)   z = sigmoid(ig_z + hg_z)
 *   n = tanh(ig_n + r * (hg_n + b_n))      h' = n + z * (h - n)
 * Every matrix-vector product is the k-ordered fp32 fmaf chain the matrix
 * cores compute (v_mfma_f32_32x32x2_f32), so the GPU is bit-identical to the
 * CPU oracle (oracle/zb_oracle_policy.c), transcendental functions included
 * (include/zbot_fmath.h).
 *
 * Parameters are passed in equinox's natural layout, fp32, concatenated:
 *   input_proj.weight [H][I], input_proj.bias [H],
 *   per layer l < D: weight_ih [3H][H], weight_hh [3H][H], bias [3H], bias_n [H],
 *   output_proj.weight [O][H], output_proj.bias [O]
 * (zb_policy_param_count gives the total). Gate order r, z, n.
 *
 * Layouts (device, row-major): obs [T][n][I]; carry [n][D][H] (read and
 * written in place); reset [T][n] uint8 (nullable: carry zeroed before step
 * t for envs with reset[t][e] != 0 — pass the engine's done flags, which mark
 * envs whose observation is already the next episode's first);
 * actions [T][n][20]; log_prob [T][n][20] (per joint); value [T][n].
 */
#ifndef ZBOT_POLICY_H
#define ZBOT_POLICY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZB_POL_HIDDEN 128
#define ZB_POL_DEPTH 5
#define ZB_POL_MIX 5
#define ZB_POL_JOINTS 20
#define ZB_POL_ACTOR_IN 50     /* NUM_ACTOR_INPUTS train.py:51 */
#define ZB_POL_CRITIC_IN 484   /* NUM_CRITIC_INPUTS train.py:52 */
#define ZB_POL_ACTOR_OUT 300   /* NUM_JOINTS * 3 * num_mixtures train.py:934-938 */
#define ZB_POL_ENVS_PER_BLOCK 32   /* envs per workgroup (two 16-row matrix-core tiles) */

#define ZB_POL_ACTOR 0
#define ZB_POL_CRITIC 1

/* actor modes */
#define ZB_POL_SAMPLE 0        /* action_dist.sample(seed) -> actions (out) */
#define ZB_POL_MODE 1          /* action_dist.mode() (argmax=True) -> actions (out) */
#define ZB_POL_EVAL 2          /* log_prob of the given actions (in) */

#define ZB_RNG_POLICY 5u       /* RNG purpose of the action sample (engine uses 1-4) */
#define ZB_RNG_SHUFFLE 6u      /* RNG purpose of the minibatch permutation (zbot_fmath.h zbf_perm_index) */

typedef struct ZbPolicy ZbPolicy;

/* Number of fp32 parameters of an actor (kind 0) or critic (kind 1). */
size_t zb_policy_param_count(int kind);

/* Upload `params` (host, natural layout above) to `device`, packed into
 * matrix-core fragment order. */
int zb_policy_create(int kind, const float* params, size_t n_params, int device, ZbPolicy** out);
int zb_policy_destroy(ZbPolicy* p);

/* Kernel layout of the handle's launches (bit-identical results either way):
 *   ZB_POL_LAYOUT_BLOCK  32 envs x 8 waves a workgroup, 89 KB (actor) / 116 KB (critic) of LDS:
 *                        the fastest alone on the GPU;
 *   ZB_POL_LAYOUT_WAVE   16 envs on one wave, <= 20 KB of LDS: a workgroup fits the slot of one
 *                        zb_step wave, so its launches fill the slots a concurrent step launch
 *                        frees (env groups on their own streams).
 * The default is ZB_POL_LAYOUT_BLOCK, or the environment's ZB_POLICY_LAYOUT=wave|block at
 * zb_policy_create. */
#define ZB_POL_LAYOUT_BLOCK 0
#define ZB_POL_LAYOUT_WAVE 1
#define ZB_POL_LAYOUT_WAVE2 2 /* the one-wave layout's unit tiles split over two waves (2 slots, 19 KB) */
#define ZB_POL_LAYOUT_WAVE4 3 /* ... over four waves (4 slots, 19 KB) */
int zb_policy_set_layout(ZbPolicy* p, int layout);

/* Persistent launches (round 5; default on): with the block layout a call over T steps is ONE launch
 * that runs the recurrence over the T steps with each layer's carry in registers (HBM sees the carry
 * once on entry and once after step T-1) instead of T launches. Bit-identical either way; 0 = one
 * launch per step. The slot-sized layouts always launch per step. No reference counterpart: ksim
 * scans the critic over the trajectory (get_ppo_variables, train.py:1683-1729). */
int zb_policy_set_persistent(ZbPolicy* p, int on);

/*
 * Actor over T consecutive steps of n envs (T = 1 in the rollout loop).
 *   mode ZB_POL_SAMPLE / ZB_POL_MODE: actions written; ZB_POL_EVAL: read.
 *   log_prob (nullable) receives log N-mixture(action) per joint.
 * Sampling draws are keyed by (seed, global env id = env_offset + e, step =
 * step0 + t): a pure function of its inputs, independent of n and sharding.
 */
int zb_policy_actor(ZbPolicy* p, const float* obs, int T, int n, float* carry, const uint8_t* reset, int mode,
                    uint64_t seed, int env_offset, uint32_t step0, float* actions, float* log_prob, void* stream);

/* Critic over T consecutive steps: value [T][n]. */
int zb_policy_critic(ZbPolicy* p, const float* obs, int T, int n, float* carry, const uint8_t* reset, float* value,
                     void* stream);

/*
 * ---- Training: activation-saving forward and the vector-Jacobian product ----
 *
 * The learner's half of PPO (get_ppo_variables differentiates through the GRU scan,
 * train.py:1683-1729). None of these entry points changes what the inference entry points
 * compute. All pointers are device pointers; every call is asynchronous on `stream`, allocates
 * nothing, and returns an error code instead of launching on a bad argument (a scratch buffer
 * smaller than zb_policy_train_scratch_words is one). They always run the 32-env block layout.
 *
 *   reset[t][e] zeroes the carry before step t as in inference, and the gradient through time is
 *   cut at the same place (train.py:1719-1723). carry0 [n][D][H] is read-only data: it gets no
 *   gradient. The actor's trailing 20 mean offsets (JOINT_BIASES, train.py:963) are constants:
 *   their grad entries are written as 0.
 *
 * Scratch (fp32 words, K = T n rows): what the training forward saves per (t, env) — the input
 * projection, and per layer the old carry, r, z, n, W_hn h + b_n and the output h'; the actor's
 * 300 raw head outputs — then what backward adds — per layer (da_r, da_z, da_n, da_n r), the
 * gradient of the input projection's output and of the raw head outputs — and the split-K
 * partials of the parameter gradient. Nothing is recomputed in backward but the mixture head.
 *
 * Reduction order of the parameter gradient (two identical calls return identical bits; no
 * floating-point atomics): the K rows, in (t, env) order, are cut into C = min(32, ceil(K / 512))
 * chunks of ceil(K / C) rows rounded up to a multiple of 16. A chunk's rows are taken in sub-chains
 * of 512 rows: for every weight gradient element each sub-chain is one matrix-core chain from 0
 * over its rows in row order (v_mfma_f32_16x16x4_f32: 4 rows a step), and the chunk's partial is
 * the sub-chain sums added in order, ((s0 + s1) + s2) + ... A bias gradient element is one fp64
 * matrix-core chain over the whole chunk (v_mfma_f64_16x16x4_f64), rounded to fp32 once. The C
 * chunk partials p[0..31] (p[c] = 0 for c >= C) are then combined by the fixed tree
 * p[c] += p[c + s] for s = 16, 8, 4, 2, 1.
 */

/* fp32 words of scratch a (kind, T, n) training forward writes and its backward reads (0 on a bad argument) */
size_t zb_policy_train_scratch_words(int kind, int T, int n);

/* Replace the handle's parameters from a DEVICE buffer in the natural layout (zb_policy_param_count
 * floats): repacked on the GPU into the forward's fragment order and backward's transposed packs. */
int zb_policy_set_params(ZbPolicy* p, const float* params, size_t n_params, void* stream);

/* Training forward: the arithmetic and bits of zb_policy_actor(mode = ZB_POL_EVAL) / zb_policy_critic
 * over T steps, with carry0 [n][D][H] read-only and the activations saved to scratch. */
int zb_policy_actor_train(ZbPolicy* p, const float* obs, int T, int n, const float* carry0, const uint8_t* reset,
                          const float* actions, float* log_prob, float* scratch, size_t scratch_words, void* stream);
int zb_policy_critic_train(ZbPolicy* p, const float* obs, int T, int n, const float* carry0, const uint8_t* reset,
                           float* value, float* scratch, size_t scratch_words, void* stream);

/* VJP after the training forward of the same arguments and scratch:
 * grad [param_count] (natural layout, overwritten) = d(sum d_log_prob * log_prob) / d params
 * (d_log_prob [T][n][20]; critic: d_value [T][n]). */
int zb_policy_actor_backward(ZbPolicy* p, const float* obs, int T, int n, const float* carry0, const uint8_t* reset,
                             const float* actions, const float* d_log_prob, float* scratch, size_t scratch_words,
                             float* grad, void* stream);
int zb_policy_critic_backward(ZbPolicy* p, const float* obs, int T, int n, const float* carry0, const uint8_t* reset,
                              const float* d_value, float* scratch, size_t scratch_words, float* grad, void* stream);

/*
 * ---- Network shape: GRU depth and mixture count per handle ----
 *
 * train.py's config opens with hidden_size, depth and num_mixtures (train.py:1065-1076; Model, Actor and
 * Critic take them, :898-944, :977-1013, :1604-1614). Everything above is the default shape (128, 5, 5).
 * A shaped handle has D = depth GRU layers and, for the actor, O = 60 * num_mixtures outputs ordered
 * means [20][m], stds [20][m], logits [20][m] (train.py:955-958); the critic has one output whatever
 * num_mixtures is (it is range-checked for both kinds). The parameter layout is the one at the top of this
 * file with these D and O: H I + H + D (6 H^2 + 4 H) + O H + O floats, plus 20 for the actor. The carry is
 * [n][depth][128]. Every entry point above takes a shaped handle and means the same thing on it.
 *
 *   hidden_size  128 only. The wave count of a workgroup (H / 16), the gate-tile indices, the fragment
 *                groups and every LDS tile are built on it; any other value is refused with ZB_EARG and
 *                "hidden_size" in zb_last_error.
 *   depth        1 .. ZB_POL_MAX_DEPTH, num_mixtures 1 .. ZB_POL_MAX_MIX; outside: ZB_EARG, field named.
 *
 * Kernels. A default-shape handle without ZB_POL_SHAPE_GENERIC launches exactly the kernels of
 * zb_policy_create (compiled for depth 5 and 5 mixtures). Every other handle launches the shape-generic
 * set: one instantiation per kernel form with depth and mixture count as runtime values bounded by the
 * two maxima, the same k-ordered chains, epilogue order and reduction order, so at the default shape the
 * two sets return the same bits (forward, training forward and gradient). The generic set exists in the
 * 32-env block layout only, one-step and persistent: zb_policy_set_layout to a slot-sized layout
 * (ZB_POL_LAYOUT_WAVE, _WAVE2, _WAVE4) on such a handle returns ZB_EARG, and such handles ignore the
 * environment's ZB_POLICY_LAYOUT. Their persistent form keeps the carries in memory between steps (each
 * thread reads back the 8 values per layer it wrote), not in registers.
 *
 * Training scratch of a shaped handle: the planes of the default layout with D layers and a raw-head row
 * stride of 60 m rounded up to 16, plus one [D][n][128] plane for the time-direction gradient that the
 * default kernel keeps in registers. Use zb_policy_train_scratch_words_shaped (a flagged default shape
 * needs more words than zb_policy_train_scratch_words says). The reduction order of the parameter
 * gradient is the one above at every shape.
 */
#define ZB_POL_MAX_DEPTH 8
#define ZB_POL_MAX_MIX 8
#define ZB_POL_SHAPE_GENERIC 1u /* flags: run the shape-generic kernels even at the default shape */
typedef struct ZbPolicyShape {
  int32_t struct_bytes;  /* sizeof(ZbPolicyShape) */
  int32_t hidden_size;   /* 128 */
  int32_t depth;         /* 1..ZB_POL_MAX_DEPTH */
  int32_t num_mixtures;  /* 1..ZB_POL_MAX_MIX; read for the actor, range-checked for both */
  uint32_t flags;        /* ZB_POL_SHAPE_GENERIC or 0 */
} ZbPolicyShape;

/* 128, 5, 5, flags 0 */
void zb_policy_default_shape(ZbPolicyShape* shape);
/* parameters of a (kind, shape) network; 0 on a bad kind or shape (zb_last_error names the field) */
size_t zb_policy_param_count_shaped(int kind, const ZbPolicyShape* shape);
/* zb_policy_create with a shape; zb_policy_create is this with zb_policy_default_shape */
int zb_policy_create_shaped(int kind, const ZbPolicyShape* shape, const float* params, size_t n_params, int device,
                            ZbPolicy** out);
int zb_policy_get_shape(const ZbPolicy* p, ZbPolicyShape* shape);
/* scratch words of a shaped handle's training calls (0 on a bad argument) */
size_t zb_policy_train_scratch_words_shaped(int kind, const ZbPolicyShape* shape, int T, int n);

/* Host twins: zb_policy_actor / zb_policy_critic on the CPU, every pointer a host pointer. They are the
 * bit reference of the kernels at every shape: each product the k-ordered fp32 fmaf chain from 0, biases
 * and the GRU update in the kernels' order without contraction, zbot_fmath.h functions and RNG. The
 * backward pass has no host twin (its reference is fp64 autograd). */
int zb_policy_actor_host(const ZbPolicyShape* shape, const float* params, const float* obs, int T, int n, float* carry,
                         const uint8_t* reset, int mode, uint64_t seed, int env_offset, uint32_t step0, float* actions,
                         float* log_prob);
int zb_policy_critic_host(const ZbPolicyShape* shape, const float* params, const float* obs, int T, int n, float* carry,
                          const uint8_t* reset, float* value);

#ifdef __cplusplus
}
#endif
#endif /* ZBOT_POLICY_H */
