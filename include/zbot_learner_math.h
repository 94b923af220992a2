/*
 * zbot_learner_math.h — the element arithmetic of one PPO optimizer step, shared,
 * source-identical, by the HIP kernels (csrc/zb_learner.hip) and their host twins
 * (csrc/zb_host.cpp: zb_ppo_loss_host, zb_grad_sqnorm_host, zb_adamw_step_host).
 * C ABI: include/zbot_ppo.h "Learner".
 *
 * Like zbot_fmath.h, every function is a fixed sequence of IEEE-754 operations (+ - * /, sqrt,
 * explicit fmaf, zbf_exp), each correctly rounded on gfx950 (hipcc without fast-math flags) and
 * on the host (-ffp-contract=off), so a kernel's result is bit-identical to the host twin's. The
 * operation order written here is the definition of the result, as zbot_ppo.h defines GAE.
 *
 * What it restates: ksim's PPO loss as zbot_amd.learner.ppo_loss writes it ([U], un-vendored
 * ksim/task/ppo.py) together with its derivative with respect to the per-joint log-probs and the
 * values (what torch autograd returns for that function, ties of minimum / maximum included), and
 * optax.clip_by_global_norm -> optax.adamw ([U]; ZbotWalkingTask.get_optimizer, train.py:1314-1324).
 */
#ifndef ZBOT_LEARNER_MATH_H
#define ZBOT_LEARNER_MATH_H

#include "zbot_fmath.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define ZBL_JOINTS 20 /* per-joint log-probs of one row (ZB_POL_JOINTS) */

/* s = sum_j lp[j], j ascending, one fp32 rounding per addition */
ZBF_FN float zbl_joint_sum(const float* lp) {
  float s = lp[0];
  for (int j = 1; j < ZBL_JOINTS; j++) s = s + lp[j];
  return s;
}

typedef struct ZblLossRow {
  float d_log_prob; /* seed of each of the row's 20 per-joint log-probs */
  float d_value;    /* seed of the row's value */
  float surrogate;  /* S: the loss is -sum S / total + c 0.5 sum Vt / total */
  float value_term; /* Vt */
  float clipped;    /* [|ratio - 1| > clip_param] */
  float kl;         /* (ratio - 1) - clamped log ratio */
} ZblLossRow;

/*
 * One row (t, env) of the loss. s, s0: zbl_joint_sum of log_prob / old_log_prob; A: advantage;
 * v, old_v, tgt: value, rollout value, value target; eps = clip_param, L = log_clip_value,
 * c = value_loss_coef, inv = (float)(1.0 / total). In this order, every line one fp32 rounding:
 *
 *   lr    = s - s0
 *   cl    = lr < -L ? -L : (lr > L ? L : lr)
 *   ratio = zbf_exp(cl)
 *   lo    = 1 - eps,  hi = 1 + eps
 *   rc    = ratio < lo ? lo : (ratio > hi ? hi : ratio)
 *   s1    = ratio * A,  s2 = rc * A
 *   S     = s1 < s2 ? s1 : s2
 *   dS    = A  if lo <= ratio <= hi            (minimum's tie: both halves pass)
 *           A  else if s1 < s2                 (the unclipped branch is the minimum)
 *           0  otherwise                       (the clamp passes nothing)
 *   g     = |lr| <= L ? (-(dS * ratio)) * inv : 0          (d ratio / d cl = ratio; the clamp of the
 *                                                            log ratio passes the gradient inside)
 *   d     = v - tgt,  a = d * d
 *   dv    = v - old_v
 *   cv    = dv < -eps ? -eps : (dv > eps ? eps : dv)
 *   vc    = old_v + cv,  dc = vc - tgt,  b = dc * dc
 *   pass  = |dv| <= eps ? dc : 0
 *   clipped value loss:   Vt = a > b ? a : b
 *                         h  = d if a > b,  pass if a < b,  0.5 * (d + pass) if a == b   (maximum's tie)
 *   unclipped:            Vt = a,  h = d
 *   d_value = (c * h) * inv
 *   clipped = |ratio - 1| > eps ? 1 : 0
 *   kl      = (ratio - 1) - cl
 *
 * On a first pass (s == s0 bit for bit, v == old_v): ratio == 1, g == (-A) * inv, h == d exactly.
 */
ZBF_FN void zbl_loss_row(float s, float s0, float A, float v, float old_v, float tgt, float eps, float L, float c,
                         float inv, int use_clipped_value_loss, ZblLossRow* o) {
  const float lr = s - s0;
  const float cl = lr < -L ? -L : (lr > L ? L : lr);
  const float ratio = zbf_exp(cl);
  const float lo = 1.0f - eps, hi = 1.0f + eps;
  const float rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);
  const float s1 = ratio * A, s2 = rc * A;
  const int inside = ratio >= lo && ratio <= hi;
  const float dS = inside ? A : (s1 < s2 ? A : 0.0f);
  const float gr = dS * ratio;
  o->surrogate = s1 < s2 ? s1 : s2;
  o->d_log_prob = fabsf(lr) <= L ? (-gr) * inv : 0.0f;

  const float d = v - tgt;
  const float a = d * d;
  float Vt = a, h = d;
  if (use_clipped_value_loss) {
    const float dv = v - old_v;
    const float cv = dv < -eps ? -eps : (dv > eps ? eps : dv);
    const float vc = old_v + cv;
    const float dc = vc - tgt;
    const float b = dc * dc;
    const float pass = fabsf(dv) <= eps ? dc : 0.0f;
    const float tie = 0.5f * (d + pass);
    Vt = a > b ? a : b;
    h = a > b ? d : (a < b ? pass : tie);
  }
  o->value_term = Vt;
  const float ch = c * h;
  o->d_value = ch * inv;
  const float rm1 = ratio - 1.0f;
  o->clipped = fabsf(rm1) > eps ? 1.0f : 0.0f;
  o->kl = rm1 - cl;
}

/*
 * optax.clip_by_global_norm's factor from k squared norms (fp64, index order):
 *   N = sqrt(sqnorms[0] + sqnorms[1] + ... )
 *   scale = (float)(max_grad_norm / N)  if max_grad_norm > 0 and N > max_grad_norm,  else exactly 1
 * (torch's clip_grad_norm_ scales by max / (N + 1e-6) instead, and also when N <= max.)
 */
ZBF_FN float zbl_clip_scale(const double* sqnorms, int k, float max_grad_norm) {
  double s = 0.0;
  for (int i = 0; i < k; i++) s = s + sqnorms[i];
  const double N = sqrt(s);
  const double mx = (double)max_grad_norm;
  return (max_grad_norm > 0.0f && N > mx) ? (float)(mx / N) : 1.0f;
}

/*
 * AdamW on one element (optax.adamw: decoupled weight decay, eps outside the square root).
 * The caller forms in fp64, from beta1 / beta2 as doubles, and rounds once: beta1, beta2,
 * omb1 = (float)(1 - beta1), omb2 = (float)(1 - beta2), bc1 = (float)(1 - beta1^step),
 * bc2 = (float)(1 - beta2^step). (1 - (float)0.999 is 1.3e-5 away from 0.001: the complement must
 * not be taken of a rounded beta.)
 * In this order, every line one fp32 rounding (fmaf: one for the fused pair):
 *
 *   g   = scale * grad
 *   m   = fmaf(beta1, m, omb1 * g)
 *   v   = fmaf(beta2, v, (omb2 * g) * g)
 *   mh  = m / bc1,  vh = v / bc2
 *   u   = mh / (sqrtf(vh) + eps)
 *   u   = fmaf(wd, p, u)
 *   p   = fmaf(-lr, u, p)
 *
 * scale == 1 leaves g == grad bit for bit, so an unclipped step equals one with the clip off.
 */
ZBF_FN void zbl_adamw(float* p, float* m, float* v, float grad, float scale, float lr, float beta1, float omb1,
                      float beta2, float omb2, float bc1, float bc2, float eps, float wd) {
  const float g = scale * grad;
  const float a1 = omb1 * g;
  const float a2 = (omb2 * g) * g;
  const float mn = fmaf(beta1, *m, a1);
  const float vn = fmaf(beta2, *v, a2);
  const float mh = mn / bc1;
  const float vh = vn / bc2;
  const float den = sqrtf(vh) + eps;
  float u = mh / den;
  u = fmaf(wd, *p, u);
  *p = fmaf(-lr, u, *p);
  *m = mn;
  *v = vn;
}

#endif /* ZBOT_LEARNER_MATH_H */
