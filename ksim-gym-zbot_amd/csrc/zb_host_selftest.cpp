/*
 * zb_host_selftest.cpp — host-sanitizer driver for zb_host.cpp (host code under
 * -fsanitize=address,undefined; built by csrc/sanitize.mk, run by tests/test_sanitizers.py).
 *
 *   zb_host_selftest <model.bin> <config.bin> [mutations]
 *
 * The model / config are the raw ZbModel / ZbEnvConfig bytes compile_model() and default_config()
 * produce. The driver validates them (expects ZB_OK), builds the team topology, and then feeds
 * check_model / check_cfg `mutations` corrupted copies: one to four 32-bit words of the struct
 * replaced by small integers, boundary values or random bits (deterministic xorshift). Every
 * copy that passes validation is handed to build_topology, which must then stay inside the
 * model's arrays: an out-of-bounds index the validation let through is an ASan / UBSan report
 * (-fsanitize=bounds sees the fixed-size member arrays). The velocity commands' host twins
 * (include/zbot_command.h) get the same treatment: a joystick ZbCommandConfig with one word
 * corrupted goes to zb_command_config_check, and every copy that passes runs
 * zb_command_initial_host / _next_host / _rewards_host over a small batch whose outputs must then
 * lie where the law puts them. Last, zb_rollout_summary_host (include/zbot_ppo.h) reads planes
 * allocated to the byte at sizes around its tree's powers of two, with every subset of the nullable
 * planes, so a read past a plane's end is an ASan report; its counts must be the exact integers
 * and its bad arguments refused. Prints one summary line.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "zb_host.h"
#include "zbot_ppo.h"

static bool read_file(const char* path, void* dst, size_t bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  size_t got = fread(dst, 1, bytes, f);
  int extra = fgetc(f);
  fclose(f);
  return got == bytes && extra == EOF;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s model.bin config.bin [mutations]\n", argv[0]);
    return 2;
  }
  const long mutations = argc > 3 ? atol(argv[3]) : 20000;
  ZbModel* model = new ZbModel;
  ZbEnvConfig cfg;
  if (!read_file(argv[1], model, sizeof *model) || !read_file(argv[2], &cfg, sizeof cfg)) {
    fprintf(stderr, "cannot read %s / %s as ZbModel (%zu B) / ZbEnvConfig (%zu B)\n", argv[1], argv[2],
            sizeof(ZbModel), sizeof(ZbEnvConfig));
    return 2;
  }
  if (zb::check_model(model) != ZB_OK || zb::check_cfg(&cfg) != ZB_OK) {
    fprintf(stderr, "the unmodified model / config fail validation: %s\n", zb_last_error());
    return 1;
  }
  static int32_t topo[zb::TP_NF][zb::TOPO_LANES];
  zb::build_topology(model, topo);
  long roots = 0;
  for (int l = 0; l < zb::TOPO_LANES; l++) roots += topo[zb::TP_DFREE][l];
  if (roots != 6) {
    fprintf(stderr, "topology: %ld free-joint dof lanes, expected 6\n", roots);
    return 1;
  }
  ZbEnvConfig dflt;
  zb_default_config(&dflt);
  if (memcmp(&dflt, &cfg, sizeof cfg) != 0) fprintf(stderr, "note: config differs from zb_default_config\n");

  const size_t words = sizeof(ZbModel) / 4;
  const int32_t specials[] = {-1, 0, 1, 2, 5, 6, 7, 12, 13, 25, 26, 27, 31, 32, 33, 40, 64, 127, 255, 1000,
                              -1000, 0x7fffffff, (int32_t)0x80000000};
  const int nspecial = (int)(sizeof specials / sizeof specials[0]);
  long accepted = 0, rejected = 0;
  ZbModel* m = new ZbModel;
  for (long it = 0; it < mutations; it++) {
    memcpy(m, model, sizeof *m);
    uint32_t* w = reinterpret_cast<uint32_t*>(m);
    const int k = 1 + (int)(next_u64() % 4);
    for (int j = 0; j < k; j++) {
      /* keep the header (magic, version, struct_bytes) mostly intact so the deep checks run */
      size_t at = (size_t)(next_u64() % words);
      if (at < 3 && (next_u64() & 7)) at = 3 + (size_t)(next_u64() % (words - 3));
      const uint64_t r = next_u64();
      switch (r % 3) {
        case 0: w[at] = (uint32_t)specials[(r >> 8) % nspecial]; break;
        case 1: w[at] = (uint32_t)((int32_t)((r >> 8) % 80) - 8); break;
        default: w[at] = (uint32_t)(r >> 16); break;
      }
    }
    if (zb::check_model(m) == ZB_OK) {
      accepted++;
      zb::build_topology(m, topo);
    } else {
      rejected++;
    }
    ZbEnvConfig c = cfg;
    uint32_t* cw = reinterpret_cast<uint32_t*>(&c);
    cw[next_u64() % (sizeof c / 4)] = (uint32_t)next_u64();
    (void)zb::check_cfg(&c);
  }
  /* the command twins */
  ZbCommandConfig cc;
  zb_default_command_config(&cc);
  const float ranges[7][2] = {{-0.3f, 0.8f}, {-0.4f, 0.4f}, {-1.f, 1.f}, {-0.05f, 0.02f}, {-0.08f, 0.f}, {-0.2f, 0.2f},
                              {-0.25f, 0.15f}};
  memcpy(cc.vx_range, ranges, sizeof ranges);
  cc.switch_prob = 0.25f;
  if (zb_command_config_check(&cc) != ZB_OK) {
    fprintf(stderr, "the joystick command config fails validation: %s\n", zb_last_error());
    return 1;
  }
  const int nb = 64;
  std::vector<uint32_t> env(nb), ctr(nb);
  std::vector<float> quat(4 * nb), cmd(7 * nb), nxt(7 * nb), vel(3 * nb), hz(nb), terms(ZB_NUM_CMD_TERMS * nb);
  std::vector<uint8_t> sw(nb);
  long cmd_accepted = 0, cmd_rejected = 0;
  for (long it = 0; it < mutations / 8 + 1; it++) {
    ZbCommandConfig c = cc;
    if (it > 0) reinterpret_cast<uint32_t*>(&c)[next_u64() % (sizeof c / 4)] = (uint32_t)next_u64();
    if (zb_command_config_check(&c) != ZB_OK) {
      cmd_rejected++;
      continue;
    }
    cmd_accepted++;
    for (int i = 0; i < nb; i++) {
      env[i] = (uint32_t)next_u64();
      ctr[i] = (uint32_t)next_u64();
      float n2 = 0.f;
      for (int k = 0; k < 4; k++) {
        quat[4 * i + k] = (float)((double)(next_u64() >> 11) / 9007199254740992.0 * 2.0 - 1.0);
        n2 += quat[4 * i + k] * quat[4 * i + k];
      }
      if (n2 < 1e-3f) quat[4 * i] = 1.f;
      for (int k = 0; k < 3; k++) vel[3 * i + k] = (float)((double)(next_u64() >> 11) / 9007199254740992.0 - 0.5);
      hz[i] = 0.05f + 0.4f * (float)((double)(next_u64() >> 11) / 9007199254740992.0);
    }
    const uint64_t seed = next_u64();
    if (zb_command_initial_host(&c, seed, env.data(), ctr.data(), quat.data(), 0.02f, nb, cmd.data()) != ZB_OK ||
        zb_command_next_host(&c, seed, env.data(), ctr.data(), cmd.data(), quat.data(), 0.02f, nb, nxt.data(),
                             sw.data()) != ZB_OK ||
        zb_command_rewards_host(&c, nxt.data(), quat.data(), vel.data(), hz.data(), nb, terms.data()) != ZB_OK) {
      fprintf(stderr, "a command twin rejected a validated config: %s\n", zb_last_error());
      return 1;
    }
    for (int i = 0; i < nb; i++) {
      const float* v = &cmd[7 * i];
      const bool in_x = v[0] == 0.f || (v[0] >= c.vx_range[0] && v[0] <= c.vx_range[1]);
      const bool in_y = v[1] == 0.f || (v[1] >= c.vy_range[0] && v[1] <= c.vy_range[1]);
      const bool in_w = v[2] == 0.f || (v[2] >= c.wz_range[0] && v[2] <= c.wz_range[1]);
      if (!in_x || !in_y || !in_w || sw[i] > 1) {
        fprintf(stderr, "command %d outside its ranges: %g %g %g (switched %d)\n", i, v[0], v[1], v[2], sw[i]);
        return 1;
      }
      if (!sw[i] && memcmp(&nxt[7 * i], v, 3 * sizeof(float)) != 0) {
        fprintf(stderr, "command %d changed without a switch\n", i);
        return 1;
      }
    }
  }
  /* the rollout summary's twin */
  const int shapes[][2] = {{1, 1}, {3, 85}, {4, 64}, {1, 257}, {7, 33}, {3, 259}};
  long summaries = 0;
  for (const auto& sh : shapes) {
    const int T = sh[0], n = sh[1];
    const size_t rows = (size_t)T * (size_t)n;
    for (int mask = 0; mask < 32; mask++) {
      auto plane = [&](size_t width) {
        std::vector<float> v(rows * width);
        for (float& x : v) x = (float)((double)(next_u64() >> 11) / 9007199254740992.0 * 2.0 - 1.0);
        return v;
      };
      const std::vector<float> terms = plane(12), cterms = plane(ZB_NUM_CMD_TERMS), rew = plane(1), lp = plane(20),
                               val = plane(1), tgt = plane(1);
      std::vector<uint8_t> done(rows), succ(rows);
      double ndone = 0.0, nsucc = 0.0;
      for (size_t i = 0; i < rows; i++) {
        done[i] = (uint8_t)(next_u64() % 4 == 0 ? 1 + next_u64() % 255 : 0);
        succ[i] = (uint8_t)(done[i] && (next_u64() & 1));
        ndone += done[i] ? 1.0 : 0.0;
        nsucc += succ[i] ? 1.0 : 0.0;
      }
      double sums[ZB_SUMMARY_WORDS];
      if (zb_rollout_summary_host(mask & 1 ? terms.data() : nullptr, mask & 2 ? cterms.data() : nullptr, rew.data(),
                                  done.data(), mask & 4 ? succ.data() : nullptr, mask & 8 ? lp.data() : nullptr,
                                  mask & 16 ? val.data() : nullptr, mask & 16 ? tgt.data() : nullptr, T, n,
                                  sums) != ZB_OK) {
        fprintf(stderr, "zb_rollout_summary_host refused %d x %d, planes 0x%x: %s\n", T, n, mask, zb_last_error());
        return 1;
      }
      if (sums[ZB_SUM_ROWS] != (double)rows || sums[ZB_SUM_DONE] != ndone ||
          sums[ZB_SUM_SUCCESS] != (mask & 4 ? nsucc : 0.0) || sums[ZB_SUM_USED] != 0.0 ||
          (!(mask & 16) && sums[ZB_SUM_RESIDUAL_SQ] != 0.0)) {
        fprintf(stderr, "zb_rollout_summary_host %d x %d, planes 0x%x: wrong counts\n", T, n, mask);
        return 1;
      }
      if (zb_rollout_summary_host(nullptr, nullptr, rew.data(), done.data(), nullptr, nullptr, val.data(), nullptr, T, n,
                                  sums) != ZB_EARG ||
          zb_rollout_summary_host(nullptr, nullptr, rew.data(), nullptr, nullptr, nullptr, nullptr, nullptr, T, n,
                                  sums) != ZB_EARG ||
          zb_rollout_summary_host(nullptr, nullptr, rew.data(), done.data(), nullptr, nullptr, nullptr, nullptr, 0, n,
                                  sums) != ZB_EARG) {
        fprintf(stderr, "zb_rollout_summary_host accepted a bad argument\n");
        return 1;
      }
      summaries++;
    }
  }
  printf("zb_host_selftest ok: %ld mutations, %ld accepted, %ld rejected, words %zu; command configs %ld accepted, "
         "%ld rejected; %ld rollout summaries\n", mutations, accepted, rejected, words, cmd_accepted, cmd_rejected,
         summaries);
  delete m;
  delete model;
  return 0;
}
