"""Measurement definitions shared by bench.py and the tests."""

from __future__ import annotations

from . import cstructs as cs

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s)
FP32_PEAK_TFLOPS = 157.3  # MI355X FP32 vector peak (MI355X_MICROARCH.md)


def bytes_per_env_step(extras: bool = False, terms: bool = True, stats: bool = True) -> int:
    """Algorithmic HBM bytes one env-step of zb_step moves, from the layouts in
    include/zbot_layout.h: the env's action row in, its state row in and out,
    its observation / reward / done outputs, and the episode-statistics
    read-modify-write. The model descriptor (11.5 KB, shared by all envs and
    cache-resident) is not counted per env."""
    f = 4
    b = cs.NJ * f  # action
    b += 2 * cs.STATE_STRIDE * f  # state row read + write
    b += (cs.OBS_ACTOR + cs.OBS_CRITIC) * f
    if extras:
        b += cs.OBS_EXTRA * f
    if terms:
        b += cs.NUM_TERMS * f
    b += f + 1  # reward (fp32) + done (u8)
    if stats:
        b += 2 * cs.NUM_STATS * f + 4  # stats read+write, solver-iteration counter
    return b


def rollout_telemetry(sums, cfg, level: float, command_config=None, stats=None, ctrl_dt: float = 0.02) -> dict:
    """What a rollout did, from the 32 sums of ppo.rollout_summary (cs.SUM_*; over several ranks:
    the sums after dist.reduce_fixed_order). Returns 0-d float64 tensors on `sums`' device; nothing
    is synchronised. With rows = sums[SUM_ROWS]:

      terms/<name>, terms_scaled/<name>   for cs.TERM_NAMES: the term's mean per env-step, and
                       reward_scale[i] * (level if reward_by_curriculum[i] else 1) * mean, its share
                       of the mean reward (cfg: the engine's ZbEnvConfig);
      the same two for cs.CMD_TERM_NAMES with command_config's term_scale / term_by_curriculum (the
                       weights of zbc_reward_sum); absent without a command config;
      reward, reward_std      mean and population standard deviation of the per-step reward;
      done_rate               episode ends per env-step; failures = done - success and
                              time_limits = success, as counts;
      entropy_estimate        - sum of log-probs / rows: the Monte-Carlo estimate of the policy's
                              entropy on the actions it sampled;
      value_mean, explained_variance   1 - mean (target - value)^2 / var(target), NaN where the
                              targets have no variance;
      with stats (engine.get_stats(): the [n, 4] window): episodes (finished in the window), and the
                              mean episode_return and episode_length (seconds) over them, NaN
                              when none finished.
    A plane the summary did not get reads as zeros here (its sums are +0.0)."""
    import torch  # noqa: PLC0415

    if sums.dim() != 1 or sums.numel() < cs.SUMMARY_WORDS or sums.dtype != torch.float64:
        raise ValueError(f"sums must be a float64 tensor of {cs.SUMMARY_WORDS} words, got {sums.dtype} "
                         f"{tuple(sums.shape)}")
    rows = sums[cs.SUM_ROWS]
    out = {}
    weights = [(cs.TERM_NAMES, cs.SUM_TERMS, cfg.reward_scale, cfg.reward_by_curriculum)]
    if command_config is not None:
        weights.append((cs.CMD_TERM_NAMES, cs.SUM_CMD_TERMS, command_config.term_scale,
                        command_config.term_by_curriculum))
    for names, base, scale, by_curriculum in weights:
        for i, name in enumerate(names):
            mean = sums[base + i] / rows
            out[f"terms/{name}"] = mean
            out[f"terms_scaled/{name}"] = mean * (float(scale[i]) * (float(level) if by_curriculum[i] else 1.0))
    mean_r = sums[cs.SUM_REWARD] / rows
    out["reward"] = mean_r
    out["reward_std"] = torch.sqrt(torch.clamp(sums[cs.SUM_REWARD_SQ] / rows - mean_r * mean_r, min=0.0))
    out["done_rate"] = sums[cs.SUM_DONE] / rows
    out["failures"] = sums[cs.SUM_DONE] - sums[cs.SUM_SUCCESS]
    out["time_limits"] = sums[cs.SUM_SUCCESS] + 0.0
    out["entropy_estimate"] = -sums[cs.SUM_LOG_PROB] / rows
    out["value_mean"] = sums[cs.SUM_VALUE] / rows
    mean_t = sums[cs.SUM_TARGET] / rows
    var_t = sums[cs.SUM_TARGET_SQ] / rows - mean_t * mean_t
    ev = 1.0 - (sums[cs.SUM_RESIDUAL_SQ] / rows) / var_t
    out["explained_variance"] = torch.where(var_t > 0.0, ev, torch.full_like(ev, float("nan")))
    if stats is not None:
        if stats.dim() != 2 or stats.shape[1] != cs.NUM_STATS:
            raise ValueError(f"stats must be [n, {cs.NUM_STATS}], got {tuple(stats.shape)}")
        s = stats.to(sums.device).double().sum(0)
        episodes = s[cs.ST_DONE]
        out["episodes"] = episodes
        out["episode_return"] = s[cs.ST_RETURN] / episodes  # 0 / 0: NaN when no episode finished
        out["episode_length"] = s[cs.ST_LENGTH] * float(ctrl_dt) / episodes
    return out


def command_term_means(terms) -> dict:
    """Per-term means over the envs of the unscaled tracking terms [n, 5] of a step
    (engine.get_command_terms(); include/zbot_command.h), under the names of cs.CMD_TERM_NAMES:
    0-d tensors on the terms' device, nothing synchronised."""
    if terms.dim() != 2 or terms.shape[1] != cs.NUM_CMD_TERMS:
        raise ValueError(f"terms must be [n, {cs.NUM_CMD_TERMS}], got {tuple(terms.shape)}")
    m = terms.double().mean(0)
    return {name: m[i] for i, name in enumerate(cs.CMD_TERM_NAMES)}
