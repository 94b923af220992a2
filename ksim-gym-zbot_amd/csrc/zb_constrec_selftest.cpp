/*
 * zb_constrec_selftest.cpp — host-sanitizer driver for the lane record builder of zb_host.cpp
 * (build_lane_record; layout in zb_host.h LR_*). Built by `make constrec_selftest` with
 * -fsanitize=address,undefined and run on the CPU (tests/test_const_records_host.py).
 *
 *   zb_constrec_selftest <model.bin> [<model.bin> ...]
 *
 * Each file holds the raw ZbModel bytes compile_model() produces (the default and the limbs model in
 * the test). Per model the driver validates it, builds the team topology and the record into a heap
 * block of exactly LR_FLOATS floats (a write past it is an ASan report), and checks
 *   - every word of every row, bit for bit, against the ZbModel row it has to come from, with the
 *     row indices formed here as the kernel forms them (body l or 0 off the bodies; the body of
 *     dof l or 0; the actuator of dof l);
 *   - the layout: whole 16-byte rows, every part starting on a plane boundary, 32 rows per plane,
 *     parts in phase order without gaps, the record's offset behind the model. (The limbs model
 *     differs from the default one in its colliders only, so the two records are equal.)
 * Prints one summary line per model.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zb_host.h"

static bool read_file(const char* path, void* dst, size_t bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  size_t got = fread(dst, 1, bytes, f);
  int extra = fgetc(f);
  fclose(f);
  return got == bytes && extra == EOF;
}

static long bad = 0;
/* `n` words of the record row (plane, lane) against `src`, as bits */
static void expect_row(const float* rec, int plane, int l, const float* src, int n, const char* what) {
  const float* row = rec + (size_t)plane * zb::LR_PLANE_FLOATS + 4 * l;
  if (memcmp(row, src, sizeof(float) * n) != 0) {
    fprintf(stderr, "plane %d lane %d: %s differs from the model's row\n", plane, l, what);
    bad++;
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s model.bin [model.bin ...]\n", argv[0]);
    return 2;
  }
  static_assert(zb::LR_PLANE_BYTES % 16 == 0 && zb::LR_PLANE_FLOATS == 4 * zb::TOPO_LANES, "16-byte rows, one per lane");
  static_assert(zb::LR_CRB == 0 && zb::LR_ACT == zb::LR_CRB + zb::LR_NCRB && zb::LR_NPLANE == zb::LR_ACT + 1,
                "parts in phase order, whole planes, no gap");
  static_assert(zb::LR_OFFSET % 16 == 0 && zb::LR_OFFSET >= sizeof(ZbModel) && zb::LR_OFFSET < sizeof(ZbModel) + 16,
                "the record starts on the first 16-byte boundary behind the model");
  static_assert(zb::LR_FLOATS * sizeof(float) == (size_t)zb::LR_NPLANE * zb::LR_PLANE_BYTES, "record size");
  for (int f = 1; f < argc; f++) {
    ZbModel* m = new ZbModel;
    if (!read_file(argv[f], m, sizeof *m)) {
      fprintf(stderr, "cannot read %s as ZbModel (%zu B)\n", argv[f], sizeof(ZbModel));
      return 2;
    }
    if (zb::check_model(m) != ZB_OK) {
      fprintf(stderr, "%s fails validation: %s\n", argv[f], zb_last_error());
      return 1;
    }
    static int32_t topo[zb::TP_NF][zb::TOPO_LANES];
    zb::build_topology(m, topo);
    float* rec = static_cast<float*>(malloc(sizeof(float) * zb::LR_FLOATS)); /* exact size: ASan guards both ends */
    memset(rec, 0xA5, sizeof(float) * zb::LR_FLOATS);
    zb::build_lane_record(m, topo, rec);
    if (reinterpret_cast<uintptr_t>(rec) % 16 != 0) {
      fprintf(stderr, "record block not 16-byte aligned\n");
      bad++;
    }
    const long before = bad;
    for (int l = 0; l < zb::TOPO_LANES; l++) {
      const int bb = (l >= 1 && l < m->nbody) ? l : 0;
      const int dof_body = l < m->nv ? m->dof_body[l] : 0;
      const int bj = dof_body < 0 ? 0 : dof_body;
      const float ipos_mass[4] = {m->body_ipos[bb][0], m->body_ipos[bb][1], m->body_ipos[bb][2], m->body_mass[bb][0]};
      expect_row(rec, zb::LR_CRB + zb::LR_CRB_IPOS_MASS, l, ipos_mass, 4, "body_ipos / body_mass");
      expect_row(rec, zb::LR_CRB + zb::LR_CRB_IQUAT, l, m->body_iquat[bb], 4, "body_iquat");
      expect_row(rec, zb::LR_CRB + zb::LR_CRB_INERTIA, l, m->body_inertia[bb], 4, "body_inertia");
      expect_row(rec, zb::LR_CRB + zb::LR_CRB_DAXIS, l, m->jnt_axis[bj], 4, "jnt_axis of the dof's body");
      expect_row(rec, zb::LR_CRB + zb::LR_CRB_DPOS, l, m->jnt_pos[bj], 4, "jnt_pos of the dof's body");
      int a = -1; /* the actuator that drives dof l */
      for (int k = 0; k < m->nu; k++)
        if (l < m->nv && m->act_dof[k] == l) a = k;
      const float zero[4] = {0.f, 0.f, 0.f, 0.f};
      const float act[4] = {a < 0 ? 0.f : m->act_ctrlrange[a][0], a < 0 ? 0.f : m->act_ctrlrange[a][1],
                            a < 0 ? 0.f : m->act_gear[a], 0.f};
      expect_row(rec, zb::LR_ACT, l, a < 0 ? zero : act, 4, "act_ctrlrange / act_gear of the dof's actuator");
    }
    /* no word kept the fill pattern: every row of every plane was written */
    const uint32_t* w = reinterpret_cast<const uint32_t*>(rec);
    for (int i = 0; i < zb::LR_FLOATS; i++)
      if (w[i] == 0xA5A5A5A5u) {
        fprintf(stderr, "word %d of the record was never written\n", i);
        bad++;
        break;
      }
    printf("zb_constrec_selftest %s: %d planes x %d lanes, %ld mismatches\n", argv[f], (int)zb::LR_NPLANE,
           (int)zb::TOPO_LANES, bad - before);
    free(rec);
    delete m;
  }
  if (bad) return 1;
  printf("zb_constrec_selftest ok: %d models\n", argc - 1);
  return 0;
}
