/*
 * zbot_command.h — velocity commands: the joystick task's command law and its tracking rewards,
 * shared source-identical by the step kernel (csrc/zb_engine.hip) and the host twins
 * (csrc/zb_host.cpp: zb_command_initial_host, zb_command_next_host, zb_command_rewards_host).
 *
 * Reference anchors
 *   UnifiedCommand                     train.py:189-261 (the law; ranges and switch_prob have no
 *                                      reference values: the reference never instantiates it)
 *   LinearVelocityTrackingReward       train.py:278-313
 *   L1LinearVelocityTrackingReward     train.py:317-363
 *   AngularVelocityTrackingReward      train.py:367-386
 *   XYOrientationReward                train.py:390-412
 *   BaseHeightReward                   train.py:469-482
 *   heading back-spin of the IMU       train.py:860-867
 *   xax.quat_to_euler / euler_to_quat / rotate_vector_by_quat are un-vendored: the standard ZYX
 *   forms are restated here [U]. The jax RNG stream cannot be matched, so the draw
 *   law below is this library's own [U].
 *
 * The command of an env is seven fp32 words, [vx, vy, wz, heading, bh, rx, ry], in the free tail
 * of its state row (ZB_S_CMD), so zb_get_state / zb_set_state carry it.
 *
 * Ordering (one control step t of zb_step / zb_rollout, commands on):
 *   1. the reward of step t reads cmd_t, the command in the observation that a_t answered, on the
 *      post-step state the other twelve terms read: qvel[0:3], body 1's xquat, xpos[1].z;
 *   2. cmd_{t+1} = next(cmd_t) at the post-step base quaternion (qpos[3:7]), drawn at counter
 *      rng_step; an env that terminates under auto-reset (and every env of a masked zb_reset)
 *      takes the initial command of its new episode at the reset pose, drawn at the episode
 *      counter;
 *   3. the observation written at the end of step t carries cmd_{t+1}: actor slots 44..49 =
 *      [c0, c1, c3, c4, c5, c6], critic 450..456 = all seven, and the IMU quaternion is spun back
 *      by the heading c3 before the hemisphere flip and the EMA.
 * All draws are keyed by the global env id, so sharding does not change them.
 *
 * Every function is a fixed sequence of fp32 operations without multiply-add contraction. The
 * sampled components and the switch decision use + - * and compares only, so the device and the
 * host agree bit for bit on them; heading and the reward terms go through atan2f / asinf /
 * sincosf / expf and agree to rounding (DESIGN.md §4q has the contract).
 */
#ifndef ZBOT_COMMAND_H
#define ZBOT_COMMAND_H

#include <math.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZB_CMD_WORDS        7    /* == ZB_NUM_CMD */
#define ZB_S_CMD            176  /* [7] state words 176..182: vx, vy, wz, heading, bh, rx, ry */
#define ZB_C_VX             0
#define ZB_C_VY             1
#define ZB_C_WZ             2
#define ZB_C_HEADING        3
#define ZB_C_BH             4
#define ZB_C_RX             5
#define ZB_C_RY             6

/* obs_extra, commands on: body 1's xquat as the terms of the step read it (off: 0, as the rest of
   the tail past ZB_X_END) */
#define ZB_X_CMD_XQUAT      67   /* [4] */

#define ZB_NUM_CMD_TERMS    5
#define ZB_CT_LINVEL        0    /* LinearVelocityTrackingReward */
#define ZB_CT_LINVEL_L1     1    /* L1LinearVelocityTrackingReward */
#define ZB_CT_YAW           2    /* AngularVelocityTrackingReward (tracks the heading) */
#define ZB_CT_XY_ORIENT     3    /* XYOrientationReward */
#define ZB_CT_BASE_HEIGHT   4    /* BaseHeightReward */

/* RNG purpose of the command draws (zb_engine.hip P_*), and the draw indices k under it: a pair of
   uniforms per index. The initial command of an episode draws at the episode counter, the per-step
   switch and redraw at rng_step, under disjoint indices. */
#define ZB_RNG_CMD          5u
#define ZB_CMD_K_RESET      0u   /* k = 0..3: (mode, vx) (vy, wz) (bh, bh_standing) (rx, ry) */
#define ZB_CMD_K_SWITCH     4u   /* first word: the switch uniform */
#define ZB_CMD_K_REDRAW     8u   /* k = 8..11: as ZB_CMD_K_RESET, for a switched command */

typedef struct ZbCommandConfig {
  int32_t  struct_bytes;
  float    vx_range[2];           /* m/s, robot frame */
  float    vy_range[2];
  float    wz_range[2];           /* rad/s */
  float    bh_range[2];           /* base height offset from standard_height while moving, m */
  float    bh_standing_range[2];  /* ... while standing */
  float    rx_range[2];           /* commanded roll while standing, rad */
  float    ry_range[2];           /* commanded pitch while standing, rad */
  float    switch_prob;           /* per control step */
  float    dead_zone;             /* 0.09 train.py:215-217: |vx|, |vy|, |wz| below it become 0 */
  float    term_scale[ZB_NUM_CMD_TERMS];          /* 0: computed and reported, not rewarded */
  int32_t  term_by_curriculum[ZB_NUM_CMD_TERMS];
  float    linvel_error_scale;        /* 0.25 train.py:281 */
  float    yaw_error_scale;           /* 0.25 train.py:370 */
  float    xy_orient_error_scale;     /* 0.25 train.py:393 */
  float    base_height_error_scale;   /* 0.25 train.py:472 */
  float    stand_still_threshold;     /* 1e-2 train.py:285,323 */
  float    l1_slope;                  /* 1.0  train.py:320 */
  float    l1_target_bonus;           /* 2.0  train.py:324 */
  float    standard_height;           /* 0.27 train.py:473 */
  float    pad[1];
} ZbCommandConfig;

#ifdef __cplusplus
}
#endif

#if defined(__HIPCC__)
#define ZBC_FN __host__ __device__ static inline
#else
#define ZBC_FN static inline
#endif
/* no multiply-add contraction inside the functions below (the host twins are built with
   -ffp-contract=off; hipcc would otherwise fuse lo + (hi - lo) * u). Block scope: the including
   unit's own code keeps its setting */
#if defined(__clang__)
#define ZBC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ZBC_NO_CONTRACT
#endif

/* cos and sin of the yaw of q = (w, x, y, z) (xax.quat_to_euler's ZYX yaw [U]), without the angle:
   yaw = atan2(a, b) with a = 2 (w z + x y), b = 1 - 2 (y^2 + z^2) on the normalised quaternion, so
   (cos, sin) = (b, a) / |(a, b)|; the degenerate a = b = 0 (pitch of a right angle) is yaw 0 */
ZBC_FN void zbc_yaw_ab(const float q_[4], float* a_out, float* b_out) {
  ZBC_NO_CONTRACT
  const float n = sqrtf(q_[0] * q_[0] + q_[1] * q_[1] + q_[2] * q_[2] + q_[3] * q_[3]);
  const float inv = n > 0.0f ? 1.0f / n : 0.0f;
  const float w = q_[0] * inv, x = q_[1] * inv, y = q_[2] * inv, z = q_[3] * inv;
  *a_out = 2.0f * (w * z + x * y);
  *b_out = 1.0f - 2.0f * (y * y + z * z);
}
ZBC_FN float zbc_yaw(const float q[4]) {
  float a, b;
  zbc_yaw_ab(q, &a, &b);
  return atan2f(a, b);
}
ZBC_FN void zbc_yaw_cs(const float q[4], float* c_out, float* s_out) {
  ZBC_NO_CONTRACT
  float a, b;
  zbc_yaw_ab(q, &a, &b);
  const float h = sqrtf(a * a + b * b);
  *c_out = h > 0.0f ? b / h : 1.0f;
  *s_out = h > 0.0f ? a / h : 0.0f;
}
/* roll and pitch of q (xax.quat_to_euler [U]; zb_engine.hip quat_roll_pitch is the same form) */
ZBC_FN void zbc_roll_pitch(const float q_[4], float* roll, float* pitch) {
  ZBC_NO_CONTRACT
  const float n = sqrtf(q_[0] * q_[0] + q_[1] * q_[1] + q_[2] * q_[2] + q_[3] * q_[3]);
  const float inv = n > 0.0f ? 1.0f / n : 0.0f;
  const float w = q_[0] * inv, x = q_[1] * inv, y = q_[2] * inv, z = q_[3] * inv;
  *roll = atan2f(2.0f * (w * x + y * z), 1.0f - 2.0f * (x * x + y * y));
  float sp = 2.0f * (w * y - z * x);
  sp = sp < -1.0f ? -1.0f : (sp > 1.0f ? 1.0f : sp);
  *pitch = asinf(sp);
}
/* xax.euler_to_quat(roll, pitch, 0) [U]: (cr cp, sr cp, cr sp, -sr sp) */
ZBC_FN void zbc_rp_quat(float roll, float pitch, float q[4]) {
  ZBC_NO_CONTRACT
  const float cr = cosf(0.5f * roll), sr = sinf(0.5f * roll);
  const float cp = cosf(0.5f * pitch), sp = sinf(0.5f * pitch);
  q[0] = cr * cp;
  q[1] = sr * cp;
  q[2] = cr * sp;
  q[3] = -(sr * sp);
}

ZBC_FN float zbc_lerp(const float r[2], float u) {
  ZBC_NO_CONTRACT
  return r[0] + (r[1] - r[0]) * u;
}

/* UnifiedCommand.initial_command from eight uniforms u (mode, vx, vy, wz, bh, bh_standing, rx, ry)
   and the base yaw. mode = floor(6 u0) clipped to 5: 0 forward, 1 sideways, 2 rotate, 3 omni,
   4 and 5 stand. */
ZBC_FN void zbc_initial(const ZbCommandConfig* c, const float u[8], float yaw, float ctrl_dt, float out[7]) {
  ZBC_NO_CONTRACT
  int mode = (int)(6.0f * u[0]);
  mode = mode > 5 ? 5 : mode;
  float vx = zbc_lerp(c->vx_range, u[1]);
  float vy = zbc_lerp(c->vy_range, u[2]);
  float wz = zbc_lerp(c->wz_range, u[3]);
  const float bh = zbc_lerp(c->bh_range, u[4]);
  const float bhs = zbc_lerp(c->bh_standing_range, u[5]);
  const float rx = zbc_lerp(c->rx_range, u[6]);
  const float ry = zbc_lerp(c->ry_range, u[7]);
  const float dz = c->dead_zone;
  vx = fabsf(vx) < dz ? 0.0f : vx;
  vy = fabsf(vy) < dz ? 0.0f : vy;
  wz = fabsf(wz) < dz ? 0.0f : wz;
  const int stand = mode >= 4;
  out[ZB_C_VX] = (mode == 0 || mode == 3) ? vx : 0.0f;
  out[ZB_C_VY] = (mode == 1 || mode == 3) ? vy : 0.0f;
  out[ZB_C_WZ] = (mode == 2 || mode == 3) ? wz : 0.0f;
  out[ZB_C_BH] = stand ? bhs : bh;
  out[ZB_C_RX] = stand ? rx : 0.0f;
  out[ZB_C_RY] = stand ? ry : 0.0f;
  out[ZB_C_HEADING] = yaw + ctrl_dt * out[ZB_C_WZ]; /* one step of the yaw rate ahead, train.py:240 */
}

/* UnifiedCommand.__call__: the heading integrates the yaw rate; with probability switch_prob
   (u_switch < switch_prob) the command is a fresh initial command at the current yaw.
   Returns whether it switched. */
ZBC_FN int zbc_next(const ZbCommandConfig* c, const float prev[7], float u_switch, const float u[8], float yaw,
                    float ctrl_dt, float out[7]) {
  ZBC_NO_CONTRACT
  float fresh[7];
  zbc_initial(c, u, yaw, ctrl_dt, fresh);
  const int sw = u_switch < c->switch_prob;
  for (int k = 0; k < 7; k++) out[k] = sw ? fresh[k] : prev[k];
  const float cont = prev[ZB_C_HEADING] + prev[ZB_C_WZ] * ctrl_dt;
  out[ZB_C_HEADING] = sw ? fresh[ZB_C_HEADING] : cont;
  return sw;
}

/* The five tracking terms, unscaled. cmd: the command the action answered; vel: qvel[0:3] (world
   frame); xquat: body 1's orientation; height: xpos[1].z. */
ZBC_FN void zbc_rewards(const ZbCommandConfig* c, const float cmd[7], const float xquat[4], const float vel[3],
                        float height, float t[ZB_NUM_CMD_TERMS]) {
  ZBC_NO_CONTRACT
  float cy, sy;
  zbc_yaw_cs(xquat, &cy, &sy);
  const float c0 = cmd[ZB_C_VX], c1 = cmd[ZB_C_VY], c2 = cmd[ZB_C_WZ];
  const int still = sqrtf(c0 * c0 + c1 * c1 + c2 * c2) < c->stand_still_threshold;
  {
    /* the robot-frame command turned into the world frame by the base yaw alone */
    const float gx = cy * c0 - sy * c1, gy = sy * c0 + cy * c1;
    const float dx = vel[0] - gx, dy = vel[1] - gy;
    const float e = sqrtf(dx * dx + dy * dy);
    const float err = still ? e : 2.0f * (e * e);
    t[ZB_CT_LINVEL] = expf(-err / c->linvel_error_scale);
  }
  {
    /* the world velocity turned into the robot frame by the base yaw alone; L1 error */
    const float rx = cy * vel[0] + sy * vel[1], ry = cy * vel[1] - sy * vel[0];
    const float walk = fabsf(rx - c0) + fabsf(ry - c1);
    const float stand = fabsf(rx) + fabsf(ry);
    t[ZB_CT_LINVEL_L1] = c->l1_target_bonus - c->l1_slope * (still ? stand : walk);
  }
  {
    /* <yaw quat, heading quat> = cos((yaw - heading) / 2); error 1 - dot^2 = (1 - cos(yaw - heading)) / 2 */
    const float h = cmd[ZB_C_HEADING];
    const float ch = cosf(h), sh = sinf(h);
    const float e = 0.5f * (1.0f - (cy * ch + sy * sh));
    t[ZB_CT_YAW] = expf(-e / c->yaw_error_scale);
  }
  {
    float roll, pitch, qb[4], qc[4];
    zbc_roll_pitch(xquat, &roll, &pitch);
    zbc_rp_quat(roll, pitch, qb);
    zbc_rp_quat(cmd[ZB_C_RX], cmd[ZB_C_RY], qc);
    const float d = qb[0] * qc[0] + qb[1] * qc[1] + qb[2] * qc[2] + qb[3] * qc[3];
    const float e = 1.0f - d * d;
    t[ZB_CT_XY_ORIENT] = expf(-e / c->xy_orient_error_scale);
  }
  t[ZB_CT_BASE_HEIGHT] = expf(-fabsf(height - (cmd[ZB_C_BH] + c->standard_height)) / c->base_height_error_scale);
}

/* the terms' weighted sum added to the step's reward (level: the curriculum scalar) */
ZBC_FN float zbc_reward_sum(const ZbCommandConfig* c, const float t[ZB_NUM_CMD_TERMS], float level) {
  ZBC_NO_CONTRACT
  float total = 0.0f;
  for (int i = 0; i < ZB_NUM_CMD_TERMS; i++) {
    const float sc = c->term_scale[i] * (c->term_by_curriculum[i] ? level : 1.0f);
    total = total + sc * t[i];
  }
  return total;
}

#endif /* ZBOT_COMMAND_H */
