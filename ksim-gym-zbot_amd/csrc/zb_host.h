/*
 * zb_host.h — host-only pieces of the C ABI (zb_host.cpp): model / config validation, the
 * per-lane team topology zb_create uploads, the thread-local error string. No HIP here, so the
 * same source builds under the host sanitizers (csrc/sanitize.mk, tests/test_sanitizers.py).
 * Not part of the public ABI.
 */
#ifndef ZB_HOST_H
#define ZB_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "zbot.h"
#include "zbot_command.h"
#include "zbot_policy.h"
#include "zbot_ppo.h"

namespace zb {

/* per-lane topology of a team (32 lanes), built once by zb_create from the model
   (zb_capi.cpp build_topology) and read by the kernels' make_ctx: field-major
   [TP_NF][32] int32 */
enum {
  TP_BPAR, TP_BDEP, TP_BJT, TP_BDOFADR, TP_BLAST, TP_NCH, TP_CH0, TP_CH1, TP_LVL_LO, TP_LVL_HI,
  TP_DDEP, TP_DBODY, TP_QADR, TP_ACT, TP_ROWMASK, TP_ROWMASK2, TP_ROWMASK3, TP_DK0, TP_DFREE, TP_CHD, TP_CPS, TP_CLN, TP_NF
};
constexpr int TOPO_LANES = 32;
constexpr int TOPO_NROOT = 6;  /* root dof chain (the free joint), zb_engine.hip NROOT */
constexpr int TOPO_NGEOM = 2;  /* geoms per contact-row bank, zb_engine.hip NGEOM */
constexpr int TOPO_MAXBD = 8;  /* deepest body, zb_engine.hip MAXBD */

/* The handle's lane record, built once by zb_create (build_lane_record) and read by the step kernels
   that take it (zb_engine.hip CONST_REC): the model rows that the substep body reads per team lane
   and waited for on the spot, in the order of the phases that read them. It lies behind the model's
   device copy, LR_OFFSET bytes from its start, so a kernel needs no pointer of its own for it.
   Plane-major: plane p holds one 16-byte row per lane, [LR_NPLANE][32][4] fp32, so a wave fetches
   a plane with one global_load_dwordx3 / x4 over 512 contiguous bytes, and a phase's part (whole
   planes: 16-byte aligned and padded) with one load per plane. Values are copied, never computed:
   every bit is the model's. A model never changes after zb_create, so the
   record is never rebuilt.
     com_crb_m's part, rows of body bb = l if 1 <= l < nbody, else 0, and of the body of dof l,
     bj = TP_DBODY[l] if it is >= 0, else 0 (the indices the kernel forms):
       LR_CRB_IPOS_MASS  body_ipos[bb][0..2], body_mass[bb][0]
       LR_CRB_IQUAT      body_iquat[bb]     LR_CRB_INERTIA  body_inertia[bb]
       LR_CRB_DAXIS      jnt_axis[bj]       LR_CRB_DPOS     jnt_pos[bj]
     the actuation's part, of the actuator a = TP_ACT[l] of dof l (a < 0: a row of zeros, not read):
       LR_ACT            act_ctrlrange[a][0], act_ctrlrange[a][1], act_gear[a], 0
   kinematics' rows (body_pos, body_quat, jnt_pos, jnt_axis) are not in it: its loads are covered
   already (profiles/mem_wait_phases.json). */
enum {
  LR_CRB_IPOS_MASS, LR_CRB_IQUAT, LR_CRB_INERTIA, LR_CRB_DAXIS, LR_CRB_DPOS, LR_NCRB,
  LR_CRB = 0, LR_ACT = LR_NCRB, /* first plane of each part; LR_CRB_* count from LR_CRB */
  LR_NPLANE = LR_ACT + 1
};
constexpr int LR_PLANE_FLOATS = TOPO_LANES * 4;
constexpr int LR_PLANE_BYTES = LR_PLANE_FLOATS * 4;
constexpr int LR_FLOATS = LR_NPLANE * LR_PLANE_FLOATS;
constexpr size_t LR_OFFSET = (sizeof(ZbModel) + 15) / 16 * 16; /* of the record in the model's device buffer */
/* requires check_model(m) == ZB_OK and t = build_topology(m) */
void build_lane_record(const ZbModel* m, const int32_t t[TP_NF][TOPO_LANES], float rec[LR_FLOATS]);

/* fail(): record the message for zb_last_error() and return `code` */
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
/* ZB_OK, or ZB_EARG / ZB_EMODEL with the reason in zb_last_error() */
int check_model(const ZbModel* m);
int check_cfg(const ZbEnvConfig* c);
/* zb_set_command_config's check: struct_bytes, finite fields, lo <= hi, switch_prob in [0, 1] */
int check_command_config(const ZbCommandConfig* c);
/* the model needs the general-collider kernels (anything but exactly two box soles) */
int needs_xg(const ZbModel* m); /* 0 two-sole, 1 general colliders, 2 with cylinders / ellipsoids / meshes, 3 the sole pair alone, 4 the sole pair beside up to two other colliders, 5 more than two colliders beyond the soles (two floor banks), 6 the sole pair beside more than two (two floor banks and the pair's) */
/* floor colliders beyond the soles that a substep holds before the overflow flag is set (zb_bank_cap) */
int bank_cap(const ZbModel* m);
/* requires check_model(m) == ZB_OK */
void build_topology(const ZbModel* m, int32_t t[TP_NF][TOPO_LANES]);

/* argument checks of the learner entry points (include/zbot_ppo.h "Learner"), shared by the
   device entry points (zb_capi.cpp) and their host twins: ZB_OK or ZB_EARG */
int check_loss_args(const char* what, const void* const* ptrs, int nptrs, int T, int n, double total,
                    float clip_param, float log_clip_value);
int check_sqnorm_args(const char* what, const void* grad, size_t count, const void* out);
/* zb_grad_combine / _host: the check, and the access width the kernel reads rows in: 16 bytes when
   parts, grad and (with more than one row) the row stride count * 4 are multiples of 16, else 4 */
int check_combine_args(const char* what, const float* parts, int world, size_t count, const float* grad,
                       const void* sq_out);
int combine_width(const float* parts, int world, size_t count, const float* grad);
int check_adamw_args(const char* what, const void* param, const void* grad, const void* m, const void* v,
                     size_t count, size_t frozen_tail, const void* sqnorms, int k, float max_grad_norm, float lr,
                     double beta1, double beta2, float eps, float weight_decay, int step);
/* zb_rollout_summary / _host (include/zbot_ppo.h "Rollout summary"); `partials` is checked when
   need_partials (the device entry point) */
int check_summary_args(const char* what, const void* reward, const void* done, const void* values,
                       const void* value_targets, int T, int n, const void* partials, int need_partials,
                       const void* sums_out);
/* the scalars both sides derive on the host, here only (zb_capi.cpp is built with relaxed flags):
   (float)(1 / total); AdamW's (float)beta, (float)(1 - beta), (float)(1 - beta^step), in fp64 */
float inv_total(double total);
struct AdamCoef { float beta1, omb1, beta2, omb2, bc1, bc2; };
AdamCoef adam_coefficients(double beta1, double beta2, int step);

/* a ZbPolicyShape (include/zbot_policy.h "Network shape"): ZB_OK, or ZB_EARG with the field named */
int check_policy_shape(const char* what, int kind, const ZbPolicyShape* shape);

/* zb_minibatch_gather / _host (include/zbot_ppo.h "Minibatches"): the argument check, which also
   fills out[n_items] with each item and the access width it moves in: the widest of 16, 8, 4, 1
   bytes that divides row_bytes, both addresses and, with more than one row, the time stride */
struct GatherItemDev {
  const char* src;
  char* dst;
  int rows, row_bytes, width;
  int chunk; /* 0, or zb_minibatch_gather_seq's seq_len for a time item (fills the padding in front of stride) */
  long long stride;
};
int check_gather_args(const char* what, const ZbGatherItem* items, int n_items, int n, int lo, int count,
                      GatherItemDev* out);
/* zb_minibatch_gather_seq / _host: check_gather_args, then seq_len and the time items' rows */
int check_gather_seq_args(const char* what, const ZbGatherItem* items, const int32_t* cut, int n_items, int seq_len,
                          int n, int lo, int count, GatherItemDev* out);

}  // namespace zb

#endif
