/*
 * zb_host.cpp — the host-only half of the C ABI (include/zbot.h): the error string, the
 * train.py default configuration, model / config validation and the per-lane team topology;
 * and the learner's host twins (include/zbot_ppo.h "Learner": zb_ppo_loss_host,
 * zb_grad_sqnorm_host, zb_adamw_step_host), the CPU bit reference of csrc/zb_learner.hip; and
 * the minibatch twins ("Minibatches": zb_minibatch_perm_host, zb_minibatch_gather_host), that of
 * csrc/zb_minibatch.hip; and the velocity commands' twins (include/zbot_command.h:
 * zb_command_initial_host, zb_command_next_host, zb_command_rewards_host), built on the header the
 * step kernel includes; and the rollout summary's twin ("Rollout summary":
 * zb_rollout_summary_host), the bit reference of zb_ppo.hip's summary kernels.
 * Plain C++ (no HIP): the product library links it, and csrc/sanitize.mk builds it with the host
 * sanitizers for tests/test_sanitizers.py.
 */
#include <cmath>
#include <cstdlib>
#include "zb_host.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "zbot_command.h"
#include "zbot_fmath.h"
#include "zbot_learner_math.h"
#include "zbot_ppo.h"

namespace zb {

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

static bool in(int v, int lo, int hi) { return v >= lo && v < hi; } /* lo <= v < hi */

/* Every integer the kernels use as an index lies inside the array it indexes, so that no field of
   a model handed to zb_create can send a kernel outside its model copy, LDS rows or team lanes
   (an out-of-bounds access in a kernel faults the GPU). Counts first, then each table over the
   entries the engine reads. Found necessary by the mutation driver zb_host_selftest.cpp. */
static int check_indices(const ZbModel* m) {
  if (!in(m->nbody, 2, ZB_MAX_BODY + 1) || !in(m->nv, 1, ZB_MAX_DOF + 1) || !in(m->nq, 1, ZB_MAX_QPOS + 1) ||
      !in(m->nu, 0, ZB_MAX_ACT + 1) || !in(m->ngeom, 0, ZB_MAX_GEOM + 1) || !in(m->nsite, 0, ZB_MAX_SITE + 1) ||
      !in(m->max_depth, 1, ZB_MAX_DEPTH + 1) || !in(m->nlevel, 0, ZB_MAX_DEPTH + 1))
    return fail(ZB_EMODEL, "model counts out of range (nbody=%d nv=%d nq=%d nu=%d ngeom=%d nsite=%d depth=%d nlevel=%d)",
                m->nbody, m->nv, m->nq, m->nu, m->ngeom, m->nsite, m->max_depth, m->nlevel);
  const int NB = m->nbody, NV = m->nv, NQ = m->nq;
  if (m->body_parent[0] != -1) return fail(ZB_EMODEL, "body 0 (world) must have parent -1");
  for (int b = 0; b < NB; b++) {
    if (b > 0 && !in(m->body_parent[b], 0, b)) return fail(ZB_EMODEL, "body %d: parent %d not an earlier body", b, m->body_parent[b]);
    const int jt = m->body_jnttype[b];
    if (jt != ZB_JNT_NONE && jt != ZB_JNT_FREE && jt != ZB_JNT_HINGE) return fail(ZB_EMODEL, "body %d: joint type %d", b, jt);
    if (!in(m->body_depth[b], 0, 16) || !in(m->body_dofadr[b], -1, NV) || !in(m->body_dofnum[b], 0, 7) ||
        !in(m->body_qposadr[b], -1, NQ) || !in(m->body_lastdof[b], -1, NV) || !in(m->body_nchild[b], 0, 9))
      return fail(ZB_EMODEL, "body %d: a depth / dof / qpos index out of range", b);
    if (m->body_dofadr[b] >= 0 && m->body_dofadr[b] + m->body_dofnum[b] > NV)
      return fail(ZB_EMODEL, "body %d: dofs [%d, %d) past nv", b, m->body_dofadr[b], m->body_dofadr[b] + m->body_dofnum[b]);
    for (int c = 0; c < 8; c++)
      if (!in(m->body_child[b][c], -1, NB)) return fail(ZB_EMODEL, "body %d: child %d out of range", b, c);
  }
  for (int k = 0; k < NV; k++) {
    if (!in(m->dof_body[k], 1, NB) || !in(m->dof_parent[k], -1, k) || !in(m->dof_depth[k], 0, m->max_depth) ||
        !in(m->dof_qposadr[k], -1, NQ) || !in(m->dof_act[k], -1, m->nu) || !in(m->dof_rowoff[k], 0, 248 - 8) ||
        (m->dof_limited[k] != 0 && m->dof_limited[k] != 1))
      return fail(ZB_EMODEL, "dof %d: a body / parent / depth / qpos / actuator / row index out of range", k);
    for (int d = 0; d < ZB_MAX_DEPTH; d++)
      if (!in(m->dof_anc[k][d], -1, NV)) return fail(ZB_EMODEL, "dof %d: ancestor at depth %d out of range", k, d);
    if (m->dof_anc[k][m->dof_depth[k]] != k) return fail(ZB_EMODEL, "dof %d: not its own ancestor at its depth", k);
  }
  for (int a = 0; a < m->nu; a++)
    if (!in(m->act_dof[a], 0, NV)) return fail(ZB_EMODEL, "actuator %d: dof %d out of range", a, m->act_dof[a]);
  for (int g = 0; g < m->ngeom; g++)
    if (!in(m->geom_body[g], 1, NB) || !in(m->geom_lastdof[g], -1, NV) ||
        m->geom_lastdof[g] != m->body_lastdof[m->geom_body[g]])
      return fail(ZB_EMODEL, "geom %d: body / dof out of range", g);
  for (int s = 0; s < m->nsite; s++)
    if (!in(m->site_body[s], 0, NB)) return fail(ZB_EMODEL, "site %d: body %d out of range", s, m->site_body[s]);
  if (!in(m->site_imu, 0, m->nsite) || !in(m->site_left_foot, 0, m->nsite) || !in(m->site_right_foot, 0, m->nsite) ||
      !in(m->body_base, 1, NB) || !in(m->body_left_foot, 1, NB) || !in(m->body_right_foot, 1, NB) ||
      !in(m->geom_left_foot, 0, m->ngeom) || !in(m->geom_right_foot, 0, m->ngeom))
    return fail(ZB_EMODEL, "a named site / body / geom index is out of range");
  if (!in(m->max_body_depth, 0, 16) || !in(m->mrow_size, 0, 248 - 8 + 1))
    return fail(ZB_EMODEL, "max_body_depth %d / mrow_size %d out of range", m->max_body_depth, m->mrow_size);
  for (int d = 0; d < 16; d++)
    if (!in(m->depth_maxchild[d], 0, 9)) return fail(ZB_EMODEL, "depth_maxchild[%d] out of range", d);
  for (int l = 0; l < m->nlevel; l++) {
    if (!in(m->level_nmem[l], 0, 9)) return fail(ZB_EMODEL, "level %d: %d members", l, m->level_nmem[l]);
    for (int i = 0; i < m->level_nmem[l]; i++)
      if (!in(m->level_mem[l][i], 0, NV)) return fail(ZB_EMODEL, "level %d member %d out of range", l, i);
  }
  return ZB_OK;
}

int check_model(const ZbModel* m) {
  if (m->magic != ZB_MODEL_MAGIC) return fail(ZB_EARG, "model magic mismatch");
  if (m->version != ZB_MODEL_VERSION) return fail(ZB_EARG, "model version %d != %d", m->version, ZB_MODEL_VERSION);
  if (m->struct_bytes != (int32_t)sizeof(ZbModel))
    return fail(ZB_EARG, "model struct_bytes %d != %zu (layout mismatch)", m->struct_bytes, sizeof(ZbModel));
  if (int rc = check_indices(m)) return rc;
  if (m->nskip_geom != 0)
    return fail(ZB_EMODEL, "the source model has %d colliding geoms the engine does not collide with the floor (it "
                           "collides the 2 box soles): compile_model(..., drop_colliders=True) to simulate without "
                           "them knowingly", m->nskip_geom);
  if (m->nskip_pair != 0)
    return fail(ZB_EMODEL, "the source model collides %d pairs of its own geoms with each other; the engine "
                           "collides the robot with itself only as the two box soles against each other: "
                           "compile_model(..., drop_self_contacts=True) to simulate without them knowingly",
                m->nskip_pair);
  if (m->nbody > 32 || m->nv > 32 || m->nq > ZB_MAX_QPOS)
    return fail(ZB_EMODEL, "model too large for a 32-lane team (nbody=%d nv=%d nq=%d)", m->nbody, m->nv, m->nq);
  /* colliders: banks of 32 contact-row lanes, 16 rows (4 contacts x 4 pyramid edges) per geom; the
     first bank holds geoms 0-1 (the soles), the second the first two others within reach of the floor
     each substep (zb_engine.hip select_bank2), a third the next two where the model has more than two
     others; the sole pair's half rows take the bank after the floor colliders' (needs_xg, bank_cap) */
  if (m->ngeom < 1 || m->ngeom > ZB_MAX_GEOM)
    return fail(ZB_EMODEL, "ngeom=%d: 1 to %d floor colliders", m->ngeom, ZB_MAX_GEOM);
  for (int g = 0; g < m->ngeom; g++) {
    const int ty = m->geom_type[g];
    const int nsz = (ty == ZB_GEOM_BOX || ty == ZB_GEOM_ELLIPSOID) ? 3
                    : (ty == ZB_GEOM_CAPSULE || ty == ZB_GEOM_CYLINDER) ? 2
                    : (ty == ZB_GEOM_SPHERE || ty == ZB_GEOM_MESH) ? 1 : 0;
    if (nsz == 0)
      return fail(ZB_EMODEL, "geom %d: type %d (mesh 7, box 6, cylinder 5, ellipsoid 4, capsule 3, sphere 2)", g, ty);
    for (int k = 0; k < nsz; k++)
      if (!(m->geom_size[g][k] > 0.f)) return fail(ZB_EMODEL, "geom %d: size[%d] must be positive", g, k);
    if (ty == ZB_GEOM_MESH) {
      /* the hull's vertices: a range of the pool, within the kernel's per-mesh limit */
      const int adr = m->geom_vertadr[g], num = m->geom_vertnum[g];
      if (num < 1 || num > ZB_MAX_MESHV || adr < 0 || adr + num > ZB_MAX_MESHVERT)
        return fail(ZB_EMODEL, "geom %d: mesh vertices [%d, %d + %d) (1 to %d hull vertices in a pool of %d)", g, adr,
                    adr, num, ZB_MAX_MESHV, ZB_MAX_MESHVERT);
      for (int i = adr; i < adr + num; i++)
        for (int k = 0; k < 3; k++)
          if (!std::isfinite(m->mesh_vert[i][k])) return fail(ZB_EMODEL, "geom %d: mesh vertex %d not finite", g, i - adr);
    }
  }
  if (m->max_depth > ZB_MAX_DEPTH) return fail(ZB_EMODEL, "dof depth %d > %d", m->max_depth, ZB_MAX_DEPTH);
  if (m->npair < 0 || m->npair > 1) return fail(ZB_EMODEL, "npair=%d: the sole pair at most", m->npair);
  if (m->npair == 1) {
    /* the sole pair (zb_engine.hip pair_rows): the two box soles (geoms 0 and 1, the touch sensors'),
       on two different limbs (its contact rows are one half-row per limb chain); with other floor
       colliders beside them its rows take a bank of their own (XG 4, XG 6) */
    const int g1 = m->pair_geom[0], g2 = m->pair_geom[1];
    if (m->ngeom < 2 || !((g1 == 0 && g2 == 1) || (g1 == 1 && g2 == 0)))
      return fail(ZB_EMODEL, "the sole pair collides the two soles, geoms 0 and 1 (ngeom=%d, pair %d-%d)",
                  m->ngeom, g1, g2);
    if (m->geom_type[0] != ZB_GEOM_BOX || m->geom_type[1] != ZB_GEOM_BOX)
      return fail(ZB_EMODEL, "the sole pair collides two boxes (box-box)");
    int head[2];
    for (int k = 0; k < 2; k++) {
      int d = m->body_lastdof[m->geom_body[k]];
      if (d < 6) return fail(ZB_EMODEL, "sole %d hangs off the base: the pair needs both on limbs", k);
      while (m->dof_parent[d] >= 6) d = m->dof_parent[d];
      head[k] = d;
    }
    if (head[0] == head[1]) return fail(ZB_EMODEL, "the two soles of the pair are on one limb");
    if (!(m->pair_friction[0] >= 0.f) || !(m->pair_solref[0] > 0.f) || !(m->pair_solimp[1] > 0.f))
      return fail(ZB_EMODEL, "the sole pair's friction / solref / solimp are invalid");
  }
  if (m->nu != ZB_NJ || m->nbody != ZB_NBODY_TASK)
    return fail(ZB_EMODEL, "task layout needs nu=%d nbody=%d (got %d, %d)", ZB_NJ, ZB_NBODY_TASK, m->nu, m->nbody);
  if (m->body_jnttype[1] != ZB_JNT_FREE) return fail(ZB_EMODEL, "body 1 must carry the free joint");
  int maxbd = 0;
  for (int b = 0; b < m->nbody; b++) {
    if (m->body_depth[b] > maxbd) maxbd = m->body_depth[b];
    int nch = 0;
    for (int c = 1; c < m->nbody; c++)
      if (m->body_parent[c] == b) nch++;
    if (nch > 8) return fail(ZB_EMODEL, "body %d has %d children (max 8)", b, nch);
    /* subtree sums are chain suffix sums below the base (zb_engine.hip subtree_sum) */
    if (b != 1 && nch > 1) return fail(ZB_EMODEL, "body %d branches (%d children): only the base may", b, nch);
  }
  if (maxbd > 15) return fail(ZB_EMODEL, "body depth %d > 15", maxbd);
  /* dof tree shape the factorization relies on (zb_engine.hip factor_ldl):
     a root chain 0..R-1 (R <= 6, one dof per top elimination level) and
     unbranched limb chains of consecutive dofs hanging off dof R-1 */
  int nroot = 0;
  for (int k = 0; k < 6 && k < m->nlevel; k++) {
    const int lv = m->nlevel - 1 - k;
    if (m->level_nmem[lv] == 1 && m->level_mem[lv][0] == k && m->dof_depth[k] == k) nroot++;
    else break;
  }
  if (nroot != 6) return fail(ZB_EMODEL, "dof tree: the free joint's 6 dofs must form the root chain (got %d)", nroot);
  if (m->nv != 6 + ZB_NJ) return fail(ZB_EMODEL, "task layout needs nv=%d (got %d)", 6 + ZB_NJ, m->nv);
  /* the depths the engine is compiled for (zb_engine.hip MAXBD, MAXDD / NLIMBLV): the pointer-jumping
     passes cover bodies up to depth 8 and limb chains up to 6 dofs below the 6 root dofs */
  if (maxbd > TOPO_MAXBD || m->max_depth > 12 || m->nlevel > 12)
    return fail(ZB_EMODEL, "body depth %d (max %d), dof depth %d (max 12), %d levels (max 12)", maxbd, TOPO_MAXBD,
                m->max_depth, m->nlevel);
  for (int k = nroot; k < m->nv; k++) {
    const int p = m->dof_parent[k];
    int nchild_prev = 0;
    for (int j = nroot; j < m->nv; j++) nchild_prev += (m->dof_parent[j] == k - 1);
    const bool head = p == nroot - 1;
    const bool cont = p == k - 1 && k - 1 >= nroot && nchild_prev == 1;
    if (!head && !cont)
      return fail(ZB_EMODEL, "dof %d: limbs must be unbranched chains of consecutive dofs off dof %d", k, nroot - 1);
  }
  return ZB_OK;
}

int needs_xg(const ZbModel* m) {
  /* the sole pair: alone with the soles (XG 3, the second bank holds the pair's rows), or beside other
     floor colliders: up to two of them in one floor bank and a third bank for the pair's rows (XG 4),
     more than two in two floor banks, as XG 5 holds them, and a fourth bank for the pair's rows (XG 6) */
  if (m->npair > 0) return m->ngeom == 2 ? 3 : m->ngeom <= 4 ? 4 : 6;
  /* ZB_FORCE_XG=1 (profiling only): the two-sole model on the general-collider instantiation, whose
     second bank then stays empty, to time that kernel's overhead on the headline's work */
  const char* fx = getenv("ZB_FORCE_XG");
  if (m->ngeom == 2 && m->geom_type[0] == ZB_GEOM_BOX && m->geom_type[1] == ZB_GEOM_BOX)
    return (fx && fx[0] == '1') ? 1 : 0;
  /* more than two colliders beyond the soles: the second and third banks both hold floor colliders,
     the first four within reach of the floor each substep (XG 5, every collider type compiled) */
  if (m->ngeom > 4) return 5;
  for (int g = 0; g < m->ngeom; g++)
    if (m->geom_type[g] == ZB_GEOM_CYLINDER || m->geom_type[g] == ZB_GEOM_ELLIPSOID || m->geom_type[g] == ZB_GEOM_MESH)
      return 2;
  return 1;
}

int bank_cap(const ZbModel* m) {
  /* the floor banks beyond the soles' hold two colliders each: one bank up to two such colliders
     (needs_xg 1, 2, 4), two banks for more (5, 6); exactly the soles: none */
  if (m->ngeom <= 2) return 0;
  return m->ngeom <= 4 ? 2 : 4;
}

int check_cfg(const ZbEnvConfig* c) {
  if (c->struct_bytes != (int32_t)sizeof(ZbEnvConfig))
    return fail(ZB_EARG, "config struct_bytes %d != %zu", c->struct_bytes, sizeof(ZbEnvConfig));
  if (c->n_substeps < 1 || c->iterations < 0 || c->ls_iterations < 0 || !(c->dt > 0.f))
    return fail(ZB_EARG, "invalid solver/timestep configuration");
  if (c->solver != (int32_t)ZB_SOLVER_NEWTON && c->solver != (int32_t)ZB_SOLVER_CG)
    return fail(ZB_EARG, "unknown solver %d", c->solver);
  return ZB_OK;
}

/* The per-lane roles of a 32-lane team (body lane, dof lane, limb-chain position, contact
   rows holding the dof, actuator), computed once here instead of by every wave at the top
   of every launch. Field-major [TP_NF][32]; the checks of check_model hold. */
int check_command_config(const ZbCommandConfig* c) {
  if (!c) return fail(ZB_EARG, "command config: null");
  if (c->struct_bytes != (int32_t)sizeof(ZbCommandConfig))
    return fail(ZB_EARG, "command config: struct_bytes %d != %zu", c->struct_bytes, sizeof(ZbCommandConfig));
  /* every fp32 field is finite (the flags between term_scale and the parameters are integers) */
  const float* f = &c->vx_range[0];
  const float* const flags = reinterpret_cast<const float*>(&c->term_by_curriculum[0]);
  const float* const end = reinterpret_cast<const float*>(c + 1);
  for (; f < end; f++) {
    if (f >= flags && f < flags + ZB_NUM_CMD_TERMS) continue;
    if (!std::isfinite(*f))
      return fail(ZB_EARG, "command config: non-finite field at byte %d", (int)((const char*)f - (const char*)c));
  }
  const struct { const char* name; const float* r; } ranges[] = {
      {"vx_range", c->vx_range}, {"vy_range", c->vy_range}, {"wz_range", c->wz_range}, {"bh_range", c->bh_range},
      {"bh_standing_range", c->bh_standing_range}, {"rx_range", c->rx_range}, {"ry_range", c->ry_range}};
  for (const auto& r : ranges)
    if (r.r[0] > r.r[1] || !std::isfinite(r.r[1] - r.r[0]))
      return fail(ZB_EARG, "command config: %s lo %g > hi %g (or a width beyond fp32)", r.name, r.r[0], r.r[1]);
  if (!(c->switch_prob >= 0.f && c->switch_prob <= 1.f))
    return fail(ZB_EARG, "command config: switch_prob %g outside [0, 1]", c->switch_prob);
  if (c->dead_zone < 0.f) return fail(ZB_EARG, "command config: dead_zone %g < 0", c->dead_zone);
  const struct { const char* name; float v; } pos[] = {{"linvel_error_scale", c->linvel_error_scale},
                                                       {"yaw_error_scale", c->yaw_error_scale},
                                                       {"xy_orient_error_scale", c->xy_orient_error_scale},
                                                       {"base_height_error_scale", c->base_height_error_scale}};
  for (const auto& q : pos)
    if (!(q.v > 0.f)) return fail(ZB_EARG, "command config: %s %g must be > 0", q.name, q.v);
  return ZB_OK;
}

void build_topology(const ZbModel* m, int32_t t[zb::TP_NF][zb::TOPO_LANES]) {
  const int NB = ZB_NBODY_TASK, NV = 6 + ZB_NJ;
  memset(t, 0, sizeof(int32_t) * TP_NF * TOPO_LANES);
  int nch_of[TOPO_LANES], bdep_of[TOPO_LANES];
  for (int l = 0; l < TOPO_LANES; l++) {
    const bool isb = l < NB;
    t[TP_BPAR][l] = isb ? m->body_parent[l] : 0;
    t[TP_BDEP][l] = bdep_of[l] = isb ? m->body_depth[l] : 1000;
    t[TP_BJT][l] = isb ? m->body_jnttype[l] : ZB_JNT_NONE;
    t[TP_BDOFADR][l] = isb ? m->body_dofadr[l] : -1;
    t[TP_BLAST][l] = isb ? m->body_lastdof[l] : -1;
    int nch = 0;
    uint32_t ch0 = 0, ch1 = 0;
    for (int b = 1; b < NB; b++)
      if (isb && m->body_parent[b] == l && nch < 8) {
        if (nch < 4) ch0 |= (uint32_t)b << (8 * nch);
        else ch1 |= (uint32_t)b << (8 * (nch - 4));
        nch++;
      }
    t[TP_NCH][l] = nch_of[l] = nch;
    t[TP_CH0][l] = (int32_t)ch0;
    t[TP_CH1][l] = (int32_t)ch1;
  }
  /* per body depth: the largest child count among the bodies at that depth (4 bits each) */
  uint64_t lv = 0;
  for (int d = 0; d <= TOPO_MAXBD && d < 16; d++) {
    int mx = 0;
    for (int l = 0; l < TOPO_LANES; l++)
      if (bdep_of[l] == d && nch_of[l] > mx) mx = nch_of[l];
    lv |= (uint64_t)(mx & 0xf) << (4 * d);
  }
  for (int l = 0; l < TOPO_LANES; l++) {
    t[TP_LVL_LO][l] = (int32_t)(uint32_t)lv;
    t[TP_LVL_HI][l] = (int32_t)(uint32_t)(lv >> 32);
    const bool isd = l < NV;
    const int ddep = isd ? m->dof_depth[l] : 0;
    const int dbody = isd ? m->dof_body[l] : 0;
    t[TP_DDEP][l] = ddep;
    t[TP_DBODY][l] = dbody;
    t[TP_QADR][l] = isd ? m->dof_qposadr[l] : -1;
    int act = -1;
    for (int a = 0; a < m->nu; a++)
      if (isd && m->act_dof[a] == l) act = a;
    t[TP_ACT][l] = act;
    uint32_t desc = 0;
    for (int k = 0; k < NV; k++)
      if (isd && k != l && m->dof_depth[k] > ddep && m->dof_anc[k][ddep] == l) desc |= 1u << k;
    /* contact rows of geom g: bank g / 2, lanes 16 (g % 2) .. + 15 */
    uint32_t rm[2] = {0u, 0u};
    for (int g = 0; g < m->ngeom && g < 2 * TOPO_NGEOM; g++) {
      const int kd = m->body_lastdof[m->geom_body[g]];
      if (isd && kd >= 0 && (kd == l || ((desc >> kd) & 1u))) rm[g / 2] |= 0xFFFFu << (16 * (g % 2));
    }
    uint32_t rp = 0u;
    if (m->npair > 0) {
      /* the sole pair's rows (the second bank with the soles alone, XG 3; a third bank beside other
         floor colliders, XG 4): lanes 0-15 the half rows on geom2's limb (+J), lanes 16-31 those on
         geom1's limb (-J); the root dofs' columns cancel, so a limb dof only */
      for (int h = 0; h < 2; h++) {
        const int kd = m->body_lastdof[m->geom_body[m->pair_geom[1 - h]]];
        if (isd && l >= 6 && kd >= 0 && (kd == l || ((desc >> kd) & 1u))) rp |= 0xFFFFu << (16 * h);
      }
      if (m->ngeom == 2) {
        rm[1] = rp;
        rp = 0u;
      }
    }
    t[TP_ROWMASK][l] = (int32_t)rm[0];
    t[TP_ROWMASK2][l] = (int32_t)rm[1];
    t[TP_ROWMASK3][l] = (int32_t)rp;
    t[TP_DK0][l] = isd ? l - m->body_dofadr[dbody] : 0;
    t[TP_DFREE][l] = (isd && m->body_jnttype[dbody] == ZB_JNT_FREE) ? 1 : 0;
    int hd = -1, ln = 0;
    if (isd && l >= TOPO_NROOT) {
      hd = l;
      while (m->dof_parent[hd] >= TOPO_NROOT) hd = m->dof_parent[hd];
      int k = hd;
      while (k + 1 < NV && m->dof_parent[k + 1] == k) k++;
      ln = k - hd + 1;
    }
    t[TP_CHD][l] = hd;
    t[TP_CPS][l] = hd >= 0 ? l - hd : 0;
    t[TP_CLN][l] = ln;
  }
}

/* The handle's lane record (zb_host.h LR_*): the model rows com_crb_m() and forward()'s actuation read
   per team lane, copied into plane-major 16-byte rows. The row indices are the ones the kernel forms
   (zb_engine.hip: body l or 0 off the bodies; the dof's body from the topology table or 0; the dof's
   actuator). Copies only: memcpy of whole rows, plain assignments for single values. */
void build_lane_record(const ZbModel* m, const int32_t t[zb::TP_NF][zb::TOPO_LANES], float rec[zb::LR_FLOATS]) {
  static_assert(TOPO_LANES == ZB_MAX_BODY, "a body row per lane");
  const int NB = ZB_NBODY_TASK;
  memset(rec, 0, sizeof(float) * LR_FLOATS);
  auto row = [&](int plane, int l) { return rec + (size_t)plane * LR_PLANE_FLOATS + 4 * l; };
  for (int l = 0; l < TOPO_LANES; l++) {
    const int bb = (l >= 1 && l < NB) ? l : 0;
    const int bj = t[TP_DBODY][l] < 0 ? 0 : t[TP_DBODY][l];
    memcpy(row(LR_CRB + LR_CRB_IPOS_MASS, l), m->body_ipos[bb], 12);
    row(LR_CRB + LR_CRB_IPOS_MASS, l)[3] = m->body_mass[bb][0];
    memcpy(row(LR_CRB + LR_CRB_IQUAT, l), m->body_iquat[bb], 16);
    memcpy(row(LR_CRB + LR_CRB_INERTIA, l), m->body_inertia[bb], 16);
    memcpy(row(LR_CRB + LR_CRB_DAXIS, l), m->jnt_axis[bj], 16);
    memcpy(row(LR_CRB + LR_CRB_DPOS, l), m->jnt_pos[bj], 16);
    const int a = t[TP_ACT][l];
    if (a >= 0) {
      memcpy(row(LR_ACT, l), m->act_ctrlrange[a], 8);
      row(LR_ACT, l)[2] = m->act_gear[a];
    }
  }
}

/* ---- learner (include/zbot_ppo.h "Learner"): argument checks and the host twins' tree ---- */

int check_loss_args(const char* what, const void* const* ptrs, int nptrs, int T, int n, double total,
                    float clip_param, float log_clip_value) {
  for (int i = 0; i < nptrs; i++)
    if (!ptrs[i]) return fail(ZB_EARG, "%s: null pointer (argument %d of its arrays)", what, i + 1);
  if (T < 1 || n < 1) return fail(ZB_EARG, "%s: bad size (T=%d n=%d)", what, T, n);
  if ((unsigned long long)T * (unsigned long long)n > (1ull << 28))
    return fail(ZB_EARG, "%s: T n = %llu rows exceed 2^28", what, (unsigned long long)T * n);
  if (!(total > 0.0)) return fail(ZB_EARG, "%s: total must be > 0", what);
  if (!(clip_param >= 0.f) || !(log_clip_value >= 0.f))
    return fail(ZB_EARG, "%s: clip_param / log_clip_value must be >= 0", what);
  return ZB_OK;
}

int check_sqnorm_args(const char* what, const void* grad, size_t count, const void* out) {
  if (!grad || !out) return fail(ZB_EARG, "%s: null pointer", what);
  if (count < 1 || (unsigned long long)count > (1ull << 32))
    return fail(ZB_EARG, "%s: count = %zu (1 to 2^32)", what, count);
  return ZB_OK;
}

int check_combine_args(const char* what, const float* parts, int world, size_t count, const float* grad,
                       const void* sq_out) {
  if (!parts || !grad || !sq_out) return fail(ZB_EARG, "%s: null pointer", what);
  if (world < 1 || world > ZB_COMBINE_MAX_WORLD)
    return fail(ZB_EARG, "%s: world = %d (1 to %d)", what, world, ZB_COMBINE_MAX_WORLD);
  if (count < 1 || (unsigned long long)count > (1ull << 32))
    return fail(ZB_EARG, "%s: count = %zu (1 to 2^32)", what, count);
  const uintptr_t p0 = (uintptr_t)parts, p1 = p0 + (uintptr_t)world * count * sizeof(float);
  const uintptr_t g0 = (uintptr_t)grad, g1 = g0 + count * sizeof(float);
  if (g0 < p1 && p0 < g1) return fail(ZB_EARG, "%s: grad overlaps parts", what);
  return ZB_OK;
}

int combine_width(const float* parts, int world, size_t count, const float* grad) {
  uintptr_t bits = (uintptr_t)parts | (uintptr_t)grad;
  if (world > 1) bits |= (uintptr_t)(count * sizeof(float)); /* the stride between row starts */
  return !(bits & 15) ? 16 : 4;
}

int check_adamw_args(const char* what, const void* param, const void* grad, const void* m, const void* v,
                     size_t count, size_t frozen_tail, const void* sqnorms, int k, float max_grad_norm, float lr,
                     double beta1, double beta2, float eps, float weight_decay, int step) {
  if (!param || !grad || !m || !v || !sqnorms) return fail(ZB_EARG, "%s: null pointer", what);
  if (count < 1 || (unsigned long long)count > (1ull << 32))
    return fail(ZB_EARG, "%s: count = %zu (1 to 2^32)", what, count);
  if (frozen_tail > count) return fail(ZB_EARG, "%s: frozen_tail %zu > count %zu", what, frozen_tail, count);
  if (k < 1 || k > 64) return fail(ZB_EARG, "%s: k = %d norms (1 to 64)", what, k);
  if (step < 1) return fail(ZB_EARG, "%s: step = %d (the first step is 1)", what, step);
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
    return fail(ZB_EARG, "%s: beta1 / beta2 must lie in [0, 1)", what);
  if (!(lr >= 0.f) || !(eps >= 0.f) || !(weight_decay >= 0.f) || max_grad_norm != max_grad_norm)
    return fail(ZB_EARG, "%s: lr / eps / weight_decay must be >= 0, max_grad_norm a number", what);
  return ZB_OK;
}

int check_gather_args(const char* what, const ZbGatherItem* items, int n_items, int n, int lo, int count,
                      GatherItemDev* out) {
  if (!items) return fail(ZB_EARG, "%s: null items", what);
  if (n_items < 1 || n_items > ZB_GATHER_MAX_ITEMS)
    return fail(ZB_EARG, "%s: n_items = %d (1 to %d)", what, n_items, ZB_GATHER_MAX_ITEMS);
  if (n < 1 || lo < 0 || count < 1 || (long long)lo + (long long)count > (long long)n)
    return fail(ZB_EARG, "%s: envs [%d, %d + %d) of n = %d", what, lo, lo, count, n);
  for (int k = 0; k < n_items; k++) {
    const ZbGatherItem& it = items[k];
    if (!it.dst) return fail(ZB_EARG, "%s: item %d: null dst", what, k);
    if (it.rows < 1 || it.row_bytes < 1 || it.row_bytes > ZB_GATHER_MAX_ROW_BYTES)
      return fail(ZB_EARG, "%s: item %d: rows = %d, row_bytes = %d", what, k, it.rows, it.row_bytes);
    if (it.src_t_stride_bytes < 0) return fail(ZB_EARG, "%s: item %d: negative stride", what, k);
    uintptr_t bits = (uintptr_t)it.row_bytes | (uintptr_t)it.dst;
    if (it.src) {
      bits |= (uintptr_t)it.src;
      if (it.rows > 1) bits |= (uintptr_t)it.src_t_stride_bytes;
    }
    GatherItemDev& o = out[k];
    o.src = (const char*)it.src;
    o.dst = (char*)it.dst;
    o.rows = it.rows;
    o.row_bytes = it.row_bytes;
    o.stride = (long long)it.src_t_stride_bytes;
    o.width = !(bits & 15) ? 16 : (!(bits & 7) ? 8 : (!(bits & 3) ? 4 : 1));
    o.chunk = 0;
  }
  return ZB_OK;
}

int check_gather_seq_args(const char* what, const ZbGatherItem* items, const int32_t* cut, int n_items, int seq_len,
                          int n, int lo, int count, GatherItemDev* out) {
  if (int rc = check_gather_args(what, items, n_items, n, lo, count, out)) return rc;
  if (!cut) return fail(ZB_EARG, "%s: null cut", what);
  if (seq_len < 1) return fail(ZB_EARG, "%s: seq_len = %d (at least 1)", what, seq_len);
  for (int k = 0; k < n_items; k++) {
    if (!cut[k]) continue;
    if (out[k].rows % seq_len)
      return fail(ZB_EARG, "%s: item %d: rows = %d is no multiple of seq_len = %d", what, k, out[k].rows, seq_len);
    out[k].chunk = seq_len;
  }
  return ZB_OK;
}

int check_summary_args(const char* what, const void* reward, const void* done, const void* values,
                       const void* value_targets, int T, int n, const void* partials, int need_partials,
                       const void* sums_out) {
  if (T < 1) return fail(ZB_EARG, "%s: T = %d (at least 1)", what, T);
  if (n < 1) return fail(ZB_EARG, "%s: n = %d (at least 1)", what, n);
  if ((unsigned long long)T * (unsigned long long)n > (1ull << 28))
    return fail(ZB_EARG, "%s: T * n = %d * %d rows (at most 2^28)", what, T, n);
  if (!reward) return fail(ZB_EARG, "%s: null reward", what);
  if (!done) return fail(ZB_EARG, "%s: null done", what);
  if (!values != !value_targets)
    return fail(ZB_EARG, "%s: %s without %s (both or neither)", what, values ? "values" : "value_targets",
                values ? "value_targets" : "values");
  if (need_partials && !partials) return fail(ZB_EARG, "%s: null partials", what);
  if (!sums_out) return fail(ZB_EARG, "%s: null sums_out", what);
  return ZB_OK;
}

float inv_total(double total) { return (float)(1.0 / total); }

AdamCoef adam_coefficients(double beta1, double beta2, int step) {
  AdamCoef c;
  c.beta1 = (float)beta1;
  c.omb1 = (float)(1.0 - beta1);
  c.beta2 = (float)beta2;
  c.omb2 = (float)(1.0 - beta2);
  c.bc1 = (float)(1.0 - std::pow(beta1, (double)step));
  c.bc2 = (float)(1.0 - std::pow(beta2, (double)step));
  return c;
}

/* The balanced pairwise tree over leaves [lo, lo + len), len a power of two, of which the first
   `count` exist (the rest are +0.0): leaf(i) for a single leaf, left + right otherwise. */
template <typename Leaf>
static double tree_sum(const Leaf& leaf, size_t lo, size_t len, size_t count) {
  if (lo >= count) return 0.0;
  if (len == 1) return leaf(lo);
  const double a = tree_sum(leaf, lo, len / 2, count);
  const double b = tree_sum(leaf, lo + len / 2, len / 2, count);
  return a + b;
}
template <typename Leaf>
static double tree_root(const Leaf& leaf, size_t count) {
  size_t len = 1;
  while (len < count) len <<= 1;
  return tree_sum(leaf, 0, len, count) + 0.0;
}

int check_policy_shape(const char* what, int kind, const ZbPolicyShape* s) {
  if (kind != ZB_POL_ACTOR && kind != ZB_POL_CRITIC) return fail(ZB_EARG, "%s: unknown kind %d", what, kind);
  if (!s) return fail(ZB_EARG, "%s: null shape", what);
  if (s->struct_bytes != (int32_t)sizeof(ZbPolicyShape))
    return fail(ZB_EARG, "%s: struct_bytes %d, this library's ZbPolicyShape has %zu", what, s->struct_bytes,
                sizeof(ZbPolicyShape));
  if (s->hidden_size != ZB_POL_HIDDEN)
    return fail(ZB_EARG, "%s: hidden_size %d: only %d is built (the workgroup and every LDS tile are sized on it)",
                what, s->hidden_size, ZB_POL_HIDDEN);
  if (s->depth < 1 || s->depth > ZB_POL_MAX_DEPTH)
    return fail(ZB_EARG, "%s: depth %d outside 1..%d", what, s->depth, ZB_POL_MAX_DEPTH);
  if (s->num_mixtures < 1 || s->num_mixtures > ZB_POL_MAX_MIX)
    return fail(ZB_EARG, "%s: num_mixtures %d outside 1..%d", what, s->num_mixtures, ZB_POL_MAX_MIX);
  if (s->flags & ~ZB_POL_SHAPE_GENERIC) return fail(ZB_EARG, "%s: unknown flags 0x%x", what, s->flags);
  return ZB_OK;
}

}  // namespace zb

using zb::fail;

extern "C" {

int zb_ppo_loss_host(const float* log_prob, const float* old_log_prob, const float* advantages, const float* values,
                     const float* old_values, const float* value_targets, int T, int n, double total,
                     float clip_param, float value_loss_coef, int use_clipped_value_loss, float log_clip_value,
                     float* d_log_prob, float* d_value, double* sums_out) {
  const void* ptrs[] = {log_prob, old_log_prob, advantages, values, old_values, value_targets, d_log_prob, d_value, sums_out};
  if (int rc = zb::check_loss_args("zb_ppo_loss_host", ptrs, 9, T, n, total, clip_param, log_clip_value)) return rc;
  const size_t rows = (size_t)T * (size_t)n;
  const float inv = zb::inv_total(total);
  std::vector<ZblLossRow> r(rows);
  for (size_t i = 0; i < rows; i++) {
    const float s = zbl_joint_sum(log_prob + i * ZBL_JOINTS), s0 = zbl_joint_sum(old_log_prob + i * ZBL_JOINTS);
    zbl_loss_row(s, s0, advantages[i], values[i], old_values[i], value_targets[i], clip_param, log_clip_value,
                 value_loss_coef, inv, use_clipped_value_loss, &r[i]);
    for (int j = 0; j < ZBL_JOINTS; j++) d_log_prob[i * ZBL_JOINTS + j] = r[i].d_log_prob;
    d_value[i] = r[i].d_value;
  }
  sums_out[0] = zb::tree_root([&](size_t i) { return (double)r[i].surrogate; }, rows);
  sums_out[1] = zb::tree_root([&](size_t i) { return (double)r[i].value_term; }, rows);
  sums_out[2] = zb::tree_root([&](size_t i) { return (double)r[i].clipped; }, rows);
  sums_out[3] = zb::tree_root([&](size_t i) { return (double)r[i].kl; }, rows);
  return ZB_OK;
}

int zb_grad_sqnorm_host(const float* grad, size_t count, double* out) {
  if (int rc = zb::check_sqnorm_args("zb_grad_sqnorm_host", grad, count, out)) return rc;
  out[0] = zb::tree_root([&](size_t i) { const double g = (double)grad[i]; return g * g; }, count);
  return ZB_OK;
}

int zb_grad_combine_host(const float* parts, int world, size_t count, float* grad, double* sq_out) {
  if (int rc = zb::check_combine_args("zb_grad_combine_host", parts, world, count, grad, sq_out)) return rc;
  for (size_t i = 0; i < count; i++)
    grad[i] = (float)zb::tree_root([&](size_t r) { return (double)parts[r * count + i]; }, (size_t)world);
  sq_out[0] = zb::tree_root([&](size_t i) { const double g = (double)grad[i]; return g * g; }, count);
  return ZB_OK;
}

int zb_rollout_summary_host(const float* reward_terms, const float* command_terms, const float* reward,
                            const uint8_t* done, const uint8_t* success, const float* log_prob, const float* values,
                            const float* value_targets, int T, int n, double* sums_out) {
  if (int rc = zb::check_summary_args("zb_rollout_summary_host", reward, done, values, value_targets, T, n, nullptr, 0,
                                      sums_out))
    return rc;
  const size_t rows = (size_t)T * (size_t)n;
  for (int w = 0; w < ZB_SUMMARY_WORDS; w++) sums_out[w] = 0.0;
  if (reward_terms)
    for (int k = 0; k < 12; k++)
      sums_out[ZB_SUM_TERMS + k] = zb::tree_root([&](size_t i) { return (double)reward_terms[i * 12 + k]; }, rows);
  if (command_terms)
    for (int k = 0; k < ZB_NUM_CMD_TERMS; k++)
      sums_out[ZB_SUM_CMD_TERMS + k] =
          zb::tree_root([&](size_t i) { return (double)command_terms[i * ZB_NUM_CMD_TERMS + k]; }, rows);
  sums_out[ZB_SUM_REWARD] = zb::tree_root([&](size_t i) { return (double)reward[i]; }, rows);
  sums_out[ZB_SUM_REWARD_SQ] = zb::tree_root([&](size_t i) { const double r = (double)reward[i]; return r * r; }, rows);
  sums_out[ZB_SUM_DONE] = zb::tree_root([&](size_t i) { return done[i] ? 1.0 : 0.0; }, rows);
  if (success) sums_out[ZB_SUM_SUCCESS] = zb::tree_root([&](size_t i) { return success[i] ? 1.0 : 0.0; }, rows);
  if (log_prob)
    sums_out[ZB_SUM_LOG_PROB] = zb::tree_root(
        [&](size_t i) {
          const float* p = log_prob + i * ZBL_JOINTS;
          double s = (double)p[0];
          for (int j = 1; j < ZBL_JOINTS; j++) s = s + (double)p[j];
          return s;
        },
        rows);
  if (values) {
    sums_out[ZB_SUM_VALUE] = zb::tree_root([&](size_t i) { return (double)values[i]; }, rows);
    sums_out[ZB_SUM_VALUE_SQ] = zb::tree_root([&](size_t i) { const double v = (double)values[i]; return v * v; }, rows);
    sums_out[ZB_SUM_TARGET] = zb::tree_root([&](size_t i) { return (double)value_targets[i]; }, rows);
    sums_out[ZB_SUM_TARGET_SQ] =
        zb::tree_root([&](size_t i) { const double g = (double)value_targets[i]; return g * g; }, rows);
    sums_out[ZB_SUM_RESIDUAL_SQ] = zb::tree_root(
        [&](size_t i) { const double d = (double)value_targets[i] - (double)values[i]; return d * d; }, rows);
  }
  sums_out[ZB_SUM_ROWS] = zb::tree_root([](size_t) { return 1.0; }, rows);
  return ZB_OK;
}

int zb_adamw_step_host(float* param, const float* grad, float* m, float* v, size_t count, size_t frozen_tail,
                       const double* sqnorms, int k, float max_grad_norm, float lr, double beta1, double beta2,
                       float eps, float weight_decay, int step) {
  if (int rc = zb::check_adamw_args("zb_adamw_step_host", param, grad, m, v, count, frozen_tail, sqnorms, k,
                                    max_grad_norm, lr, beta1, beta2, eps, weight_decay, step))
    return rc;
  const zb::AdamCoef c = zb::adam_coefficients(beta1, beta2, step);
  const float scale = zbl_clip_scale(sqnorms, k, max_grad_norm);
  for (size_t i = 0; i < count - frozen_tail; i++)
    zbl_adamw(&param[i], &m[i], &v[i], grad[i], scale, lr, c.beta1, c.omb1, c.beta2, c.omb2, c.bc1, c.bc2, eps, weight_decay);
  return ZB_OK;
}

int zb_minibatch_perm_host(uint64_t seed, uint32_t epoch, int n, int32_t* perm) {
  if (!perm || n < 1) return fail(ZB_EARG, "zb_minibatch_perm_host: null perm or n = %d", n);
  for (int i = 0; i < n; i++) perm[i] = (int32_t)zbf_perm_index(seed, epoch, (uint32_t)n, (uint32_t)i);
  return ZB_OK;
}

/* both gathers on checked items: source row t = c L + l of an item cut in chunks of L = chunk rows
   (C = rows / L of them) lands in destination row l C + c, any other row t in row t */
static void gather_host(const zb::GatherItemDev* it, int n_items, int n, int lo, int count, int shuffle,
                        uint64_t seed, uint32_t epoch) {
  std::vector<uint32_t> p((size_t)count);
  for (int j = 0; j < count; j++)
    p[j] = shuffle ? zbf_perm_index(seed, epoch, (uint32_t)n, (uint32_t)(lo + j)) : (uint32_t)(lo + j);
  for (int k = 0; k < n_items; k++) {
    const size_t rb = (size_t)it[k].row_bytes;
    const int L = it[k].chunk, C = L ? it[k].rows / L : 0;
    for (int t = 0; t < it[k].rows; t++) {
      const int dt = L ? (t % L) * C + t / L : t;
      for (int j = 0; j < count; j++) {
        char* d = it[k].dst + ((size_t)dt * (size_t)count + (size_t)j) * rb;
        if (it[k].src)
          memcpy(d, it[k].src + (size_t)t * (size_t)it[k].stride + (size_t)p[j] * rb, rb);
        else
          memset(d, 0, rb);
      }
    }
  }
}

int zb_minibatch_gather_host(const ZbGatherItem* items, int n_items, int n, int lo, int count, int shuffle,
                             uint64_t seed, uint32_t epoch) {
  zb::GatherItemDev it[ZB_GATHER_MAX_ITEMS];
  if (int rc = zb::check_gather_args("zb_minibatch_gather_host", items, n_items, n, lo, count, it)) return rc;
  gather_host(it, n_items, n, lo, count, shuffle, seed, epoch);
  return ZB_OK;
}

int zb_minibatch_gather_seq_host(const ZbGatherItem* items, const int32_t* cut, int n_items, int seq_len, int n,
                                 int lo, int count, int shuffle, uint64_t seed, uint32_t epoch) {
  zb::GatherItemDev it[ZB_GATHER_MAX_ITEMS];
  if (int rc = zb::check_gather_seq_args("zb_minibatch_gather_seq_host", items, cut, n_items, seq_len, n, lo, count, it))
    return rc;
  gather_host(it, n_items, n, lo, count, shuffle, seed, epoch);
  return ZB_OK;
}

/* ---- velocity commands: the host twins of the step kernel's command path ---- */
static void command_uniforms(uint64_t seed, uint32_t k0, uint32_t env, uint32_t ctr, float u[8]) {
  for (uint32_t k = 0; k < 4; k++) {
    uint32_t a, b;
    zbf_rng_bits(seed, ZB_RNG_CMD, k0 + k, env, ctr, &a, &b);
    u[2 * k] = zbf_u01(a);
    u[2 * k + 1] = zbf_u01(b);
  }
}

size_t zb_command_config_struct_bytes(void) { return sizeof(ZbCommandConfig); }

int zb_command_config_check(const ZbCommandConfig* cfg) { return zb::check_command_config(cfg); }

/* ---- shaped policy handles: the shape's checks and the host twins of the forward kernels (zb_policy.hip) ---- */

void zb_policy_default_shape(ZbPolicyShape* s) {
  if (!s) return;
  s->struct_bytes = (int32_t)sizeof(ZbPolicyShape);
  s->hidden_size = ZB_POL_HIDDEN;
  s->depth = ZB_POL_DEPTH;
  s->num_mixtures = ZB_POL_MIX;
  s->flags = 0;
}

size_t zb_policy_param_count_shaped(int kind, const ZbPolicyShape* s) {
  if (zb::check_policy_shape("zb_policy_param_count_shaped", kind, s) != ZB_OK) return 0;
  const size_t H = ZB_POL_HIDDEN, D = (size_t)s->depth;
  const size_t I = kind == ZB_POL_ACTOR ? ZB_POL_ACTOR_IN : ZB_POL_CRITIC_IN;
  const size_t O = kind == ZB_POL_ACTOR ? (size_t)3 * ZB_POL_JOINTS * (size_t)s->num_mixtures : 1;
  return H * I + H + D * (6 * H * H + 4 * H) + O * H + O + (kind == ZB_POL_ACTOR ? ZB_POL_JOINTS : 0);
}

namespace {

struct PolNet {
  const float *win, *bin, *wih[ZB_POL_MAX_DEPTH], *whh[ZB_POL_MAX_DEPTH], *b[ZB_POL_MAX_DEPTH], *bn[ZB_POL_MAX_DEPTH];
  const float *wout, *bout, *mean_bias;
  int I, O, D, nm;
};

PolNet pol_net(const float* P, int kind, const ZbPolicyShape* s) {
  constexpr int H = ZB_POL_HIDDEN;
  PolNet n;
  n.I = kind == ZB_POL_ACTOR ? ZB_POL_ACTOR_IN : ZB_POL_CRITIC_IN;
  n.D = s->depth;
  n.nm = s->num_mixtures;
  n.O = kind == ZB_POL_ACTOR ? 3 * ZB_POL_JOINTS * n.nm : 1;
  const float* p = P;
  n.win = p, p += (size_t)H * n.I;
  n.bin = p, p += H;
  for (int l = 0; l < n.D; l++) {
    n.wih[l] = p, p += (size_t)3 * H * H;
    n.whh[l] = p, p += (size_t)3 * H * H;
    n.b[l] = p, p += 3 * H;
    n.bn[l] = p, p += H;
  }
  n.wout = p, p += (size_t)n.O * H;
  n.bout = p, p += n.O;
  n.mean_bias = kind == ZB_POL_ACTOR ? p : nullptr;
  return n;
}

/* the matrix cores' chain: from 0, k ascending, one fmaf a step */
float pol_dot(const float* x, const float* w, int K) {
  float acc = 0.0f;
  for (int k = 0; k < K; k++) acc = fmaf(x[k], w[k], acc);
  return acc;
}

/* one env, one step, in policy_kernel's order: (chain + bias) for the input gates, the bare chain for the
   hidden gates, r / z from (ig + b) + hg, n from (ig + b) + r (hg + b_n), h' = n + z (h - n); carry [D][H]
   updated in place, out [O] = chain + bias */
void pol_forward(const PolNet& nt, const float* obs, float* carry, float* out) {
  constexpr int H = ZB_POL_HIDDEN;
  float x[H], xn[H];
  for (int u = 0; u < H; u++) x[u] = pol_dot(obs, nt.win + (size_t)u * nt.I, nt.I) + nt.bin[u];
  for (int l = 0; l < nt.D; l++) {
    float* h = carry + (size_t)l * H;
    for (int u = 0; u < H; u++) {
      float ig[3], hg[3];
      for (int g = 0; g < 3; g++) {
        ig[g] = pol_dot(x, nt.wih[l] + (size_t)(g * H + u) * H, H) + nt.b[l][g * H + u];
        hg[g] = pol_dot(h, nt.whh[l] + (size_t)(g * H + u) * H, H);
      }
      const float r = zbf_sigmoid(ig[0] + hg[0]);
      const float z = zbf_sigmoid(ig[1] + hg[1]);
      const float nn = zbf_tanh(ig[2] + r * (hg[2] + nt.bn[l][u]));
      xn[u] = nn + z * (h[u] - nn);
    }
    memcpy(h, xn, sizeof xn);
    memcpy(x, xn, sizeof xn);
  }
  for (int c = 0; c < nt.O; c++) out[c] = pol_dot(x, nt.wout + (size_t)c * H, H) + nt.bout[c];
}

int pol_host_check(const char* what, int kind, const ZbPolicyShape* s, const float* params, const float* obs, int T,
                   int n, const float* carry, int env_offset) {
  if (int rc = zb::check_policy_shape(what, kind, s)) return rc;
  if (T < 0 || n < 0 || env_offset < 0) return fail(ZB_EARG, "%s: bad size (T=%d n=%d offset=%d)", what, T, n, env_offset);
  if (T == 0 || n == 0) return 1;
  if (!params || !obs || !carry) return fail(ZB_EARG, "%s: null params, obs or carry", what);
  return ZB_OK;
}

}  // namespace

int zb_policy_actor_host(const ZbPolicyShape* s, const float* params, const float* obs, int T, int n, float* carry,
                         const uint8_t* reset, int mode, uint64_t seed, int env_offset, uint32_t step0, float* actions,
                         float* log_prob) {
  const int rc = pol_host_check("zb_policy_actor_host", ZB_POL_ACTOR, s, params, obs, T, n, carry, env_offset);
  if (rc != ZB_OK) return rc == 1 ? ZB_OK : rc;
  if (!actions) return fail(ZB_EARG, "zb_policy_actor_host: null actions");
  if (mode != ZB_POL_SAMPLE && mode != ZB_POL_MODE && mode != ZB_POL_EVAL)
    return fail(ZB_EARG, "zb_policy_actor_host: unknown mode %d", mode);
  constexpr int H = ZB_POL_HIDDEN, NJ = ZB_POL_JOINTS;
  const PolNet nt = pol_net(params, ZB_POL_ACTOR, s);
  const int nm = nt.nm;
  std::vector<float> out((size_t)nt.O);
  for (int t = 0; t < T; t++)
    for (int e = 0; e < n; e++) {
      float* ce = carry + (size_t)e * nt.D * H;
      if (reset && reset[(size_t)t * n + e]) memset(ce, 0, sizeof(float) * nt.D * H);
      pol_forward(nt, obs + ((size_t)t * n + e) * ZB_POL_ACTOR_IN, ce, out.data());
      float* act = actions + ((size_t)t * n + e) * NJ;
      for (int j = 0; j < NJ; j++) {
        float mu[ZB_POL_MAX_MIX], sd[ZB_POL_MAX_MIX], lg[ZB_POL_MAX_MIX];
        for (int m = 0; m < nm; m++) {
          mu[m] = out[j * nm + m] + nt.mean_bias[j];
          const float sp = (zbf_softplus(out[NJ * nm + j * nm + m]) + 0.01f) * 1.0f;
          sd[m] = sp < 1.0f ? sp : 1.0f;
          lg[m] = out[2 * NJ * nm + j * nm + m];
        }
        if (mode != ZB_POL_EVAL)
          act[j] = zbf_mix_sample_n(mu, sd, lg, nm, mode == ZB_POL_MODE, seed, ZB_RNG_POLICY, (uint32_t)j,
                                    (uint32_t)(NJ + j), (uint32_t)(env_offset + e), step0 + (uint32_t)t);
        if (log_prob) log_prob[((size_t)t * n + e) * NJ + j] = zbf_mix_log_prob_n(mu, sd, lg, nm, act[j]);
      }
    }
  return ZB_OK;
}

int zb_policy_critic_host(const ZbPolicyShape* s, const float* params, const float* obs, int T, int n, float* carry,
                          const uint8_t* reset, float* value) {
  const int rc = pol_host_check("zb_policy_critic_host", ZB_POL_CRITIC, s, params, obs, T, n, carry, 0);
  if (rc != ZB_OK) return rc == 1 ? ZB_OK : rc;
  if (!value) return fail(ZB_EARG, "zb_policy_critic_host: null value");
  constexpr int H = ZB_POL_HIDDEN;
  const PolNet nt = pol_net(params, ZB_POL_CRITIC, s);
  for (int t = 0; t < T; t++)
    for (int e = 0; e < n; e++) {
      float* ce = carry + (size_t)e * nt.D * H;
      if (reset && reset[(size_t)t * n + e]) memset(ce, 0, sizeof(float) * nt.D * H);
      pol_forward(nt, obs + ((size_t)t * n + e) * ZB_POL_CRITIC_IN, ce, value + (size_t)t * n + e);
    }
  return ZB_OK;
}

int zb_command_initial_host(const ZbCommandConfig* cfg, uint64_t seed, const uint32_t* env, const uint32_t* counter,
                            const float* quat, float ctrl_dt, int n, float* out) {
  if (int rc = zb::check_command_config(cfg)) return rc;
  if (n < 0 || (n > 0 && (!env || !counter || !quat || !out)))
    return fail(ZB_EARG, "zb_command_initial_host: null pointer or n = %d", n);
  for (int i = 0; i < n; i++) {
    float u[8];
    command_uniforms(seed, ZB_CMD_K_RESET, env[i], counter[i], u);
    zbc_initial(cfg, u, zbc_yaw(quat + 4 * (size_t)i), ctrl_dt, out + 7 * (size_t)i);
  }
  return ZB_OK;
}

int zb_command_next_host(const ZbCommandConfig* cfg, uint64_t seed, const uint32_t* env, const uint32_t* counter,
                         const float* prev, const float* quat, float ctrl_dt, int n, float* out, uint8_t* switched) {
  if (int rc = zb::check_command_config(cfg)) return rc;
  if (n < 0 || (n > 0 && (!env || !counter || !prev || !quat || !out)))
    return fail(ZB_EARG, "zb_command_next_host: null pointer or n = %d", n);
  for (int i = 0; i < n; i++) {
    float u[8], cmd[7];
    uint32_t a, b;
    zbf_rng_bits(seed, ZB_RNG_CMD, ZB_CMD_K_SWITCH, env[i], counter[i], &a, &b);
    command_uniforms(seed, ZB_CMD_K_REDRAW, env[i], counter[i], u);
    const int sw = zbc_next(cfg, prev + 7 * (size_t)i, zbf_u01(a), u, zbc_yaw(quat + 4 * (size_t)i), ctrl_dt, cmd);
    memcpy(out + 7 * (size_t)i, cmd, sizeof cmd); /* out may be prev */
    if (switched) switched[i] = (uint8_t)sw;
  }
  return ZB_OK;
}

int zb_command_rewards_host(const ZbCommandConfig* cfg, const float* cmd, const float* quat, const float* vel,
                            const float* height, int n, float* out) {
  if (int rc = zb::check_command_config(cfg)) return rc;
  if (n < 0 || (n > 0 && (!cmd || !quat || !vel || !height || !out)))
    return fail(ZB_EARG, "zb_command_rewards_host: null pointer or n = %d", n);
  for (int i = 0; i < n; i++)
    zbc_rewards(cfg, cmd + 7 * (size_t)i, quat + 4 * (size_t)i, vel + 3 * (size_t)i, height[i],
                out + ZB_NUM_CMD_TERMS * (size_t)i);
  return ZB_OK;
}

void zb_default_command_config(ZbCommandConfig* c) {
  if (!c) return;
  memset(c, 0, sizeof *c);
  c->struct_bytes = (int32_t)sizeof(ZbCommandConfig);
  c->dead_zone = 0.09f;
  c->linvel_error_scale = 0.25f;
  c->yaw_error_scale = 0.25f;
  c->xy_orient_error_scale = 0.25f;
  c->base_height_error_scale = 0.25f;
  c->stand_still_threshold = 1e-2f;
  c->l1_slope = 1.0f;
  c->l1_target_bonus = 2.0f;
  c->standard_height = 0.27f;
}

const char* zb_last_error(void) { return zb::g_err.c_str(); }

int zb_bank_cap(const ZbModel* model) { return model ? zb::bank_cap(model) : 0; }

void zb_default_config(ZbEnvConfig* c) {
  if (!c) return;
  memset(c, 0, sizeof *c);
  const double PI = 3.14159265358979323846;
  c->struct_bytes = (int32_t)sizeof(ZbEnvConfig);
  c->flags = ZB_F_OBS_NOISE | ZB_F_AUTORESET;
  c->n_substeps = 20;
  c->iterations = 8;
  c->ls_iterations = 8;
  c->dt = 0.001f;
  c->ctrl_dt = 0.02f;
  c->tolerance = 1e-8f;
  c->ls_tolerance = 0.01f;
  c->solver = (int32_t)ZB_SOLVER_CG; /* MJX's CG, as ksim's model setup selects it [U] */
  c->imu_noise_std = (float)(PI / 180.0);
  c->acc_noise_std = 0.5f;
  c->reset_qvel_scale = 0.01f;
  c->max_episode_sec = 80.f;
  c->lag_range[0] = 0.f; c->lag_range[1] = 0.1f;
  c->bad_z[0] = 0.05f; c->bad_z[1] = 0.5f;
  c->max_tilt_rad = (float)(60.0 * PI / 180.0);
  c->push_linvel[0] = 0.1f; c->push_linvel[1] = 0.1f; c->push_linvel[2] = 0.05f;
  c->push_interval[0] = 2.f; c->push_interval[1] = 4.f;
  c->push_vel_range[0] = 0.05f; c->push_vel_range[1] = 0.15f;
  const float scales[ZB_NUM_TERMS] = {1.0f, 1.0f, 5.0f, 0.3f, -2.0f, 0.3f, 2.5f, 0.3f, -0.5f, -0.5f, -0.05f, -2.0f};
  const int by_cur[ZB_NUM_TERMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1};
  for (int i = 0; i < ZB_NUM_TERMS; i++) {
    c->reward_scale[i] = scales[i];
    c->reward_by_curriculum[i] = by_cur[i];
  }
  c->feet_airtime_touchdown_penalty = 0.3f;
  c->naive_forward_clip_max = 0.2f;
  c->feet_orient_error_scale = 0.25f;
  c->feet_too_close_threshold = 0.12f;
  c->touch_threshold = 0.1f;
  c->stay_alive_balance = 10.f;
  c->rand_mass[0] = 0.95f; c->rand_mass[1] = 1.15f;
  c->rand_armature[0] = 1.0f; c->rand_armature[1] = 1.05f;
  c->rand_damping[0] = 0.95f; c->rand_damping[1] = 1.05f;
  c->rand_friction[0] = 0.5f; c->rand_friction[1] = 1.5f;
  c->rand_qpos0[0] = (float)(-2.0 * PI / 180.0); c->rand_qpos0[1] = (float)(2.0 * PI / 180.0);
  c->rand_floor_mu[0] = 0.3f; c->rand_floor_mu[1] = 1.5f;
  c->rand_imu_tilt_std = (float)(5.0 * PI / 180.0);
  c->rand_imu_yaw_std = (float)(1.0 * PI / 180.0);
  c->rand_imu_pos_std = 0.005f;
}

}  // extern "C"
