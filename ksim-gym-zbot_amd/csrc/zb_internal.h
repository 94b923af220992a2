/*
 * zb_internal.h — declarations shared by the HIP engine (zb_engine.hip) and
 * the C-ABI host code (zb_capi.cpp). Not part of the public ABI.
 */
#ifndef ZB_INTERNAL_H
#define ZB_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zbot.h"
#include "zbot_command.h"
#include "zbot_policy.h"
#include "zbot_ppo.h"
#include "zb_host.h"

/* debug forward dump layout (zb_debug_forward), fp32 words per env */
#define ZB_DBG_QM      0     /* [nv*nv] dense symmetric mass matrix */
#define ZB_DBG_BIAS    1024  /* [nv] qfrc_bias */
#define ZB_DBG_QACCS   1056  /* [nv] qacc_smooth */
#define ZB_DBG_QACC    1088  /* [nv] constrained qacc */
#define ZB_DBG_XPOS    1120  /* [nbody*3] */
#define ZB_DBG_CINERT  1216  /* [nbody*10] */
#define ZB_DBG_CVEL    1536  /* [nbody*6] */
#define ZB_DBG_MISC    1728  /* nefc, ncon, touch_l, touch_r, imu quat(4), gyro(3), acc(3) */
#define ZB_DBG_STRIDE  1760
#define ZB_XJ_STRIDE   (32 * ZB_MAX_DEPTH) /* floats per env of StepArgs::xj */
#define ZB_NSTAMP      20    /* phase-stamp slots of the -DZB_STAMPS build (zb_engine.hip S_*) */

namespace zb {

struct StepArgs {
  const ZbModel* model;     /* device copy, the handle's lane record behind it (zb_host.h LR_OFFSET) */
  const int32_t* topo;      /* [TP_NF][32] per-lane topology (device) */
  const ZbEnvConfig* cfg;   /* device copy */
  int n_envs;
  int env_offset;
  uint64_t seed;
  float* state;             /* [n, ZB_STATE_STRIDE] */
  float* rnd;               /* [n, ZB_RAND_STRIDE] */
  const float* action;      /* [nsteps, n, 20] */
  int nsteps;
  float* obs_actor;
  float* obs_critic;
  float* obs_extra;
  float* reward_terms;
  float* reward;            /* per step reward (nsteps==1) or reward sum (rollout) */
  uint8_t* done;
  uint8_t* success;         /* [n] or null: time-limit end without failure */
  float curriculum;
  float* stats;             /* [n, ZB_NUM_STATS] */
  int32_t* iters;           /* [n] */
  const uint8_t* reset_mask;
  float* dbg;               /* [n, ZB_DBG_STRIDE] */
  /* chunked step (nsteps == 1, step_kernel): the n_substeps of a control step split into
     nchunk work units per pair of envs, taken in chunk-major order from a counter */
  int nchunk;               /* 1: one workgroup per pair runs all substeps */
  uint32_t* sched;          /* [2 + npair]: units taken, pairs finished, per-pair chunks done */
  int32_t* itpart;          /* [n] Newton iterations of the chunks so far */
  int air_mark;             /* first step of a rollout: save its contacts + causal airtime term */
  int solver;               /* ZB_SOLVER_NEWTON / ZB_SOLVER_CG: which kernel instantiation runs */
  int xg;                   /* general colliders (zb_host.h needs_xg): 0 two-sole, 1 two banks, 2 two banks + cylinders / ellipsoids / meshes, 3 / 4 the sole pair, 5 three banks of floor colliders, 6 those and the sole pair's fourth */
  float* xj;                /* xg: [n + 1, banks x ZB_XJ_STRIDE] Jacobian rows of the banks beyond the first (1 to 3 blocks per env; the last env block: ghost teams) */
  int ed;                   /* ZB_F_EULERDAMP: the step kernel integrates the joint damping implicitly */
  int sol_default;          /* the handle's solver fields are the defaults (solver_fields_default): launch_step may
                               run the instantiation that holds them as literals */
  /* velocity commands (include/zbot_command.h), appended so the fields above keep their offsets */
  const ZbCommandConfig* cmd; /* device copy, or null: commands off (the instantiations without the command path) */
  float* cmd_terms;           /* [n, ZB_NUM_CMD_TERMS] unscaled tracking terms of the last step */
};

/* The solver fields of zb_default_config (MuJoCo's opt.tolerance / ls_tolerance defaults, train.py's
   iteration counts). A handle's config never changes after zb_create, so zb_capi.cpp compares it with
   these once per launch on the host copy, and step_kernel<.., DS = true> holds them as literals: its
   solver loops load no config field. Any other value runs the generic instantiation. */
constexpr int SOL_DEFAULT_ITERATIONS = 8;
constexpr int SOL_DEFAULT_LS_ITERATIONS = 8;
constexpr float SOL_DEFAULT_TOLERANCE = 1e-8f;
constexpr float SOL_DEFAULT_LS_TOLERANCE = 0.01f;
inline bool solver_fields_default(const ZbEnvConfig& c) {
  return c.iterations == SOL_DEFAULT_ITERATIONS && c.ls_iterations == SOL_DEFAULT_LS_ITERATIONS &&
         c.tolerance == SOL_DEFAULT_TOLERANCE && c.ls_tolerance == SOL_DEFAULT_LS_TOLERANCE;
}

/* workgroups of step_kernel resident on the device at once (occupancy x CUs) */
int step_resident_blocks(int device, int xg, int solver, int ed);

hipError_t launch_step(const StepArgs& a, hipStream_t s);
hipError_t launch_reset(const StepArgs& a, hipStream_t s);
hipError_t launch_debug_forward(const StepArgs& a, hipStream_t s);
/* exact ksim FeetAirtime row 0 of a marked rollout (a.state, a.cfg, a.n_envs, a.curriculum,
   a.reward = reward row 0 or null, a.reward_terms = terms row 0 or null) */
hipError_t launch_airtime_exact(const StepArgs& a, hipStream_t s);
/* packed [n, 7] commands <-> state rows: in != null writes the envs `mask` selects (null: all), else reads into out */
hipError_t launch_command_copy(float* state, const float* in, float* out, const uint8_t* mask, int n, hipStream_t s);

/* post-rollout PPO inputs (zb_ppo.hip, include/zbot_ppo.h) */
struct GaeArgs {
  const float* reward;      /* [T, n] */
  const float* values;      /* [T, n] */
  const uint8_t* done;      /* [T, n] */
  const uint8_t* success;   /* [T, n] or null */
  const float* bootstrap;   /* [n] or null */
  int T;
  int n;
  float gamma;
  float gl;                 /* gamma * lam, rounded once as the reference does */
  float* gae;               /* [T, n] */
  float* vtarget;           /* [T, n] or null */
  double* partials;         /* [ceil(n / ZB_GAE_ENVS_PER_BLOCK)][2] or null */
};

hipError_t launch_gae(const GaeArgs& a, double* moments_out, hipStream_t s);
hipError_t launch_moments(const double* in, int k, double* out, hipStream_t s);
/* GRU actor / critic, one step (zb_policy.hip, include/zbot_policy.h) */
struct PolicyArgs {
  const float* obs;       /* [n][I] of this step */
  float* carry;           /* [n][depth][hidden], read and written */
  const uint8_t* reset;   /* [n] or null: carry zeroed first */
  int n;
  int mode;               /* ZB_POL_SAMPLE / MODE / EVAL (actor) */
  uint64_t seed;
  int env_offset;
  uint32_t step;
  float* actions;         /* [n][20] (actor) */
  float* log_prob;        /* [n][20] or null (actor) */
  float* value;           /* [n] (critic) */
  const float* wpack;     /* fragment-packed weights */
  const float* bias;      /* biases and head constants */
  int layout;             /* ZB_POL_LAYOUT_BLOCK / ZB_POL_LAYOUT_WAVE */
  int T;                  /* block layout: steps run by one persistent launch (obs / reset / outputs
                             advance by one [n] step each; carry in registers between steps) */
  float* save;            /* training forward (zb_policy_*_train): scratch base, else null; carry is then
                             read-only (carry0) */
};
/* what a launch is given: PolicyArgs, which the default-shape kernels take as it is, and the handle's shape
   (include/zbot_policy.h "Network shape"), which only the shape-generic instantiations take */
struct PolicyArgsG : PolicyArgs {
  int generic;            /* 1: the shape-generic instantiations, which read depth and nmix below */
  int depth, nmix;
};
hipError_t launch_policy(int kind, const PolicyArgsG& a, hipStream_t s);

/* Training scratch (include/zbot_policy.h): planes of K = T n rows in (t, env) order, offsets in
   fp32 words. Per-layer planes are [layer][K][cols]. */
#define ZB_TR_RAW_LD 304     /* row stride of the actor's raw head outputs (300) and their gradient */
#define ZB_TR_DG_LD 512      /* (da_r, da_z, da_n, da_n r) of one layer: dgi = cols 0..383, dgh = 0..255 + 384..511 */
#define ZB_TR_MAX_CHUNKS 32
struct TrainLayout {
  size_t K;
  size_t x0;    /* [K][H] input projection output */
  size_t hp;    /* [D][K][H] carry each layer read (after the reset) */
  size_t r, z, nn, hn, ho; /* [D][K][H] gates, W_hn h + b_n, layer output */
  size_t raw;   /* [K][304] actor */
  size_t dg;    /* [D][K][512] */
  size_t dx0;   /* [K][H] */
  size_t draw;  /* [K][304] actor */
  size_t part;  /* [chunks][param_count] */
  size_t total;
  int chunks;   /* split-K chunks of the parameter gradient */
  int chunk_rows;
  size_t dht;   /* train_layout_shaped only: [D][n][H] d loss / d carry handed to step t - 1 */
};
__host__ __device__ static inline size_t policy_param_count(int kind) {
  const size_t H = ZB_POL_HIDDEN, D = ZB_POL_DEPTH;
  const size_t I = kind == ZB_POL_ACTOR ? ZB_POL_ACTOR_IN : ZB_POL_CRITIC_IN, O = kind == ZB_POL_ACTOR ? ZB_POL_ACTOR_OUT : 1;
  return H * I + H + D * (6 * H * H + 4 * H) + O * H + O + (kind == ZB_POL_ACTOR ? ZB_POL_JOINTS : 0);
}
__host__ __device__ static inline TrainLayout train_layout(int kind, int T, int n) {
  TrainLayout L;
  const size_t H = ZB_POL_HIDDEN, D = ZB_POL_DEPTH, K = (size_t)T * (size_t)n;
  const size_t act = kind == ZB_POL_ACTOR ? K * ZB_TR_RAW_LD : 0;
  size_t o = 0;
  L.K = K;
  L.x0 = o, o += K * H;
  L.hp = o, o += D * K * H;
  L.r = o, o += D * K * H;
  L.z = o, o += D * K * H;
  L.nn = o, o += D * K * H;
  L.hn = o, o += D * K * H;
  L.ho = o, o += D * K * H;
  L.raw = o, o += act;
  L.dg = o, o += D * K * ZB_TR_DG_LD;
  L.dx0 = o, o += K * H;
  L.draw = o, o += act;
  size_t c = (K + 511) / 512;
  c = c < 1 ? 1 : (c > ZB_TR_MAX_CHUNKS ? ZB_TR_MAX_CHUNKS : c);
  L.chunks = (int)c;
  L.chunk_rows = (int)(((K + c - 1) / c + 15) / 16 * 16);
  L.part = o, o += c * policy_param_count(kind);
  L.total = o;
  L.dht = 0;
  return L;
}

/* The layout of a shaped handle's scratch: D layers, a raw-head row stride of 60 m rounded up to 16
   (policy_raw_ld), and the plane dht [D][n][H] in which the generic bptt_kernel hands the
   time-direction gradient of every layer to step t - 1 (the default kernel holds it in registers). */
__host__ __device__ static inline size_t policy_param_count_shaped(int kind, int depth, int nmix) {
  const size_t H = ZB_POL_HIDDEN, D = (size_t)depth;
  const size_t I = kind == ZB_POL_ACTOR ? ZB_POL_ACTOR_IN : ZB_POL_CRITIC_IN;
  const size_t O = kind == ZB_POL_ACTOR ? (size_t)3 * ZB_POL_JOINTS * (size_t)nmix : 1;
  return H * I + H + D * (6 * H * H + 4 * H) + O * H + O + (kind == ZB_POL_ACTOR ? ZB_POL_JOINTS : 0);
}
__host__ __device__ static inline int policy_raw_ld(int nmix) { return (3 * ZB_POL_JOINTS * nmix + 15) / 16 * 16; }
__host__ __device__ static inline TrainLayout train_layout_shaped(int kind, int depth, int nmix, int T, int n) {
  TrainLayout L;
  const size_t H = ZB_POL_HIDDEN, D = (size_t)depth, K = (size_t)T * (size_t)n;
  const size_t act = kind == ZB_POL_ACTOR ? K * (size_t)policy_raw_ld(nmix) : 0;
  size_t o = 0;
  L.K = K;
  L.x0 = o, o += K * H;
  L.hp = o, o += D * K * H;
  L.r = o, o += D * K * H;
  L.z = o, o += D * K * H;
  L.nn = o, o += D * K * H;
  L.hn = o, o += D * K * H;
  L.ho = o, o += D * K * H;
  L.raw = o, o += act;
  L.dg = o, o += D * K * ZB_TR_DG_LD;
  L.dx0 = o, o += K * H;
  L.draw = o, o += act;
  L.dht = o, o += D * (size_t)n * H;
  size_t c = (K + 511) / 512;
  c = c < 1 ? 1 : (c > ZB_TR_MAX_CHUNKS ? ZB_TR_MAX_CHUNKS : c);
  L.chunks = (int)c;
  L.chunk_rows = (int)(((K + c - 1) / c + 15) / 16 * 16);
  L.part = o, o += c * policy_param_count_shaped(kind, depth, nmix);
  L.total = o;
  return L;
}

struct PolicyBwdArgs {
  const float* obs;       /* [T][n][I] */
  const uint8_t* reset;   /* [T][n] or null */
  const float* actions;   /* [T][n][20] (actor) */
  const float* dout;      /* d_log_prob [T][n][20] (actor) / d_value [T][n] (critic) */
  float* scratch;
  float* grad;            /* [param_count] */
  const float* wpack_t;   /* transposed fragment packs: per layer W_ih^T, W_hh^T; then W_out^T (actor) */
  const float* bias;      /* as PolicyArgs::bias */
  int T, n;
};
struct PolicyBwdArgsG : PolicyBwdArgs {
  int generic, depth, nmix; /* as PolicyArgsG */
};
hipError_t launch_policy_backward(int kind, const PolicyBwdArgsG& a, hipStream_t s);
/* device repack of natural-layout parameters into wpack / wpack_t / bias (depth layers, nmix mixtures) */
hipError_t launch_policy_pack(int kind, int depth, int nmix, const float* params, float* wpack, float* wpack_t,
                              float* bias, hipStream_t s);

hipError_t launch_normalize(const float* gae, float* adv, long long count, const double* mom, double total,
                            float eps, hipStream_t s);

/* the learner's loss / norm / AdamW kernels (zb_learner.hip, include/zbot_ppo.h "Learner") */
struct LossArgs {
  const float* log_prob;       /* [rows][20] */
  const float* old_log_prob;   /* [rows][20] */
  const float* advantages;     /* [rows] */
  const float* values;
  const float* old_values;
  const float* value_targets;
  size_t rows;                 /* T n */
  float inv;                   /* (float)(1 / total) */
  float clip_param, value_loss_coef, log_clip_value;
  int use_clipped_value_loss;
  float* d_log_prob;           /* [rows][20] */
  float* d_value;              /* [rows] */
  double* partials;            /* [ceil(rows / ZB_LOSS_ROWS_PER_BLOCK)][4] */
  int vec;                     /* set by the launcher: the [rows][20] arrays are 16-byte aligned */
};
struct AdamArgs {
  float* param;
  const float* grad;
  float* m;
  float* v;
  size_t count, frozen_tail;
  const double* sqnorms;       /* [k] */
  int k;
  float max_grad_norm, lr, eps, wd;
  AdamCoef c;                  /* zb_host.h adam_coefficients */
  int vec;                     /* set by the launcher: all four arrays are 16-byte aligned */
};
hipError_t launch_ppo_loss(LossArgs a, double* sums_out, hipStream_t s);
hipError_t launch_sqnorm(const float* grad, size_t count, double* partials, double* out, hipStream_t s);
hipError_t launch_grad_combine(const float* parts, int world, size_t count, float* grad, double* partials,
                               double* sq_out, bool vec, hipStream_t s);
hipError_t launch_adamw(AdamArgs a, hipStream_t s);

/* the rollout summary (zb_ppo.hip, include/zbot_ppo.h "Rollout summary") */
struct SummaryArgs {
  const float* terms;          /* [rows][12] or null */
  const float* cmd;            /* [rows][5] or null */
  const float* reward;         /* [rows] */
  const uint8_t* done;         /* [rows] */
  const uint8_t* success;      /* [rows] or null */
  const float* log_prob;       /* [rows][20] or null */
  const float* values;         /* [rows] or null */
  const float* targets;        /* [rows] or null, with values */
  size_t rows;                 /* T n */
  double* partials;            /* [ceil(rows / ZB_LOSS_ROWS_PER_BLOCK)][ZB_SUMMARY_WORDS] */
  int vec;                     /* set by the launcher: bit p = plane p (in the order above) is 16-byte aligned */
};
hipError_t launch_rollout_summary(SummaryArgs a, double* sums_out, hipStream_t s);

/* the minibatch kernels (zb_minibatch.hip, include/zbot_ppo.h "Minibatches") */
struct GatherArgs {
  GatherItemDev it[ZB_GATHER_MAX_ITEMS]; /* zb_host.h: the checked items with their access width */
  int n_items, n, lo, count, shuffle;
  uint32_t epoch;
  uint64_t seed;
};
hipError_t launch_minibatch_perm(uint64_t seed, uint32_t epoch, int n, int32_t* perm, hipStream_t s);
hipError_t launch_minibatch_gather(const GatherArgs& a, hipStream_t s);

}  // namespace zb

#endif
