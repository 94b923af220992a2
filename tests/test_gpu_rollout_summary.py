"""Rollout telemetry on the GPU: zb_rollout_summary against its host twin bit for bit (every shape,
pointer combination and alignment path); PolicyRollout.run(record_terms=True) changes no other
output and its terms explain the reward; Trainer.validate() leaves training where it was, and
Trainer(telemetry=True) trains the same weights. 64 envs, T = 8 throughout."""

import numpy as np
import pytest
import torch

import command_ref as R
import summary_cases as SC
from zbot_amd import cstructs as cs
from zbot_amd import default_config, ppo
from zbot_amd.curriculum import EpisodeLengthCurriculum
from zbot_amd.engine import ZbError
from zbot_amd.policy import ACTOR, CRITIC, MODE, init_params

pytestmark = pytest.mark.gpu
N, T, BATCH, PASSES, SEED = 64, 8, 32, 2, 5
LEVEL = 0.7
CMD_SCALES = dict(linvel_tracking=1.0, linvel_tracking_l1=0.3, yaw_tracking=0.5, xy_orientation=0.2, base_height=0.5)
CUR = EpisodeLengthCurriculum(min_level_steps=1, increase_threshold=0.05, decrease_threshold=0.01)


# ---- the kernel against its twin ----

def dev(p):
    return {k: (None if v is None else torch.from_numpy(v.copy()).cuda()) for k, v in p.items()}


def gpu_sums(d, **kw):
    return ppo.rollout_summary(d["reward"], d["done"], d["success"], reward_terms=d["reward_terms"],
                               command_terms=d["command_terms"], log_prob=d["log_prob"], values=d["values"],
                               value_targets=d["value_targets"], **kw)


def host_sums(p):
    return ppo.rollout_summary_host(p["reward"], p["done"], p["success"], reward_terms=p["reward_terms"],
                                    command_terms=p["command_terms"], log_prob=p["log_prob"], values=p["values"],
                                    value_targets=p["value_targets"])


def same_bits(got, want):
    got, want = got.cpu().numpy(), want.numpy()
    assert got.shape == want.shape == (cs.SUMMARY_WORDS,)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)


@pytest.mark.parametrize("T_,n_,combo", [(T_, n_, c) for T_, n_ in SC.SHAPES for c in SC.COMBOS])
def test_kernel_equals_twin(T_, n_, combo):
    p = SC.planes_case(T_, n_, combo)
    same_bits(gpu_sums(dev(p)), host_sums(p))


def test_more_than_one_finishing_pass():
    """1025 workgroups: the finishing kernel's second pass and its carry (1024 partials a pass)."""
    T_, n_ = 1, 1024 * 256 + 3
    rng = np.random.default_rng(3)
    r = (rng.standard_normal((T_, n_)) * 10.0 ** rng.uniform(-3, 3, (T_, n_))).astype(np.float32)
    d = (rng.random((T_, n_)) < 0.1).astype(np.uint8)
    same_bits(ppo.rollout_summary(torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda()),
              ppo.rollout_summary_host(r, d))


@pytest.mark.parametrize("T_,n_", [(3, 85), (3, 259)])
def test_views_at_odd_element_offsets(T_, n_):
    """Every plane a view that starts one element into its buffer: the float planes are then 4 bytes
    off a 16-byte boundary and the uint8 planes 1 byte: the 4-byte and the single-byte paths."""
    p = SC.planes_case(T_, n_)
    d = {}
    for k, v in p.items():
        buf = torch.zeros(v.size + 1, dtype=torch.uint8 if v.dtype == np.uint8 else torch.float32, device="cuda")
        buf[1:].copy_(torch.from_numpy(v.copy()).reshape(-1))
        d[k] = buf[1:].view(*v.shape)
        assert d[k].data_ptr() % 16 != 0 and d[k].is_contiguous()
    same_bits(gpu_sums(d), host_sums(p))
    # mixed: the [T, n, 5] and uint8 planes off, the others aligned
    a = dev(p)
    for k in ("command_terms", "done", "success"):
        a[k] = d[k]
    same_bits(gpu_sums(a), host_sums(p))


def test_extremes_and_negative_zeros():
    p = SC.extremes_case()
    got = gpu_sums(dev(p))
    same_bits(got, host_sums(p))
    assert float(got[cs.SUM_REWARD]) == 0.0 and not np.signbit(got.cpu().numpy()[cs.SUM_REWARD])


def test_buffers_are_checked_and_reused():
    p = SC.planes_case(1, 257)
    d = dev(p)
    want = host_sums(p)
    words = 2 * cs.SUMMARY_WORDS
    out = torch.full((cs.SUMMARY_WORDS,), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ZbError, match="partials"):  # one workgroup's worth for two: refused, nothing launched
        gpu_sums(d, out=out, partials=torch.zeros(words - 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ZbError, match="partials"):
        gpu_sums(d, out=out, partials=torch.zeros(words, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    part = torch.zeros(words, dtype=torch.float64, device="cuda")
    assert gpu_sums(d, out=out, partials=part).data_ptr() == out.data_ptr()
    same_bits(out, want)
    same_bits(gpu_sums(d), want)  # the cached scratch, twice
    same_bits(gpu_sums(d), want)


# ---- recording the terms ----

def make_engine(kind, cmodel, command, solver="cg"):
    from zbot_amd.engine import EnvGroups, HipEngine

    cfg = default_config(solver=solver, push=True, randomize=True, autoreset=True, max_episode_sec=0.06)
    eng = HipEngine(cmodel, cfg, N, seed=2) if kind == "engine" else EnvGroups(cmodel, cfg, N, groups=2, seed=2)
    cc = R.joystick(0.25, CMD_SCALES, by_curriculum=("yaw_tracking", "base_height")) if command else None
    if cc is not None:
        eng.set_command_config(cc)
    return eng, cfg, cc


def rollout_pair(kind, cmodel, command):
    from zbot_amd import policy as P

    outs = []
    for record in (False, True):
        eng, cfg, cc = make_engine(kind, cmodel, command)
        actor = P.GruPolicy(ACTOR, init_params(ACTOR, seed=8))
        critic = P.GruPolicy(CRITIC, init_params(CRITIC, seed=9))
        ro = P.PolicyRollout(eng, actor, seed=SEED, curriculum=LEVEL)
        kw = dict(record_terms=True) if record else {}
        outs.append(ro.run(T, record_critic=True, critic=critic, critic_carry=critic.initial_carry(N), **kw))
        torch.cuda.synchronize()
        state = eng.get_state()
        outs[-1]["_state"] = state
    return outs[0], outs[1], cfg, cc


@pytest.fixture(scope="module", params=[("engine", False), ("engine", True), ("groups", False), ("groups", True)],
                ids=lambda p: f"{p[0]}-{'commands' if p[1] else 'plain'}")
def recorded(request, cmodel):
    return rollout_pair(request.param[0], cmodel, request.param[1]) + (request.param[1],)


def test_recording_changes_nothing_else(recorded):
    plain, rec, _, _, command = recorded
    assert int(plain["done"].sum()) > 0 and int(plain["success"].sum()) > 0  # resets are in the run
    assert set(rec) - set(plain) == ({"reward_terms", "command_terms"} if command else {"reward_terms"})
    for k in plain:
        assert torch.equal(plain[k], rec[k]), k
    assert tuple(rec["reward_terms"].shape) == (T, N, cs.NUM_TERMS)
    if command:
        assert tuple(rec["command_terms"].shape) == (T, N, cs.NUM_CMD_TERMS)
        assert bool(rec["command_terms"].abs().sum() > 0)


def test_terms_explain_the_reward(recorded):
    """Per row |reward - sum_i s_i term_i| <= 24 * 2^-24 * sum_i |s_i term_i| over the 12 + 5 scaled
    terms, row 0 after the airtime patch included: 17 products and 17 additions in fp32, the
    scale x level product, and the patch's extra product and addition, each within 2^-24 relative
    of a partial sum that sum_i |s_i term_i| (1 + small) bounds. The right side is formed in float64
    from the float32 terms and scales."""
    _, rec, cfg, cc, command = recorded
    w = [cfg.reward_scale[i] * (LEVEL if cfg.reward_by_curriculum[i] else 1.0) for i in range(cs.NUM_TERMS)]
    scaled = rec["reward_terms"].double() * torch.tensor(w, dtype=torch.float64, device="cuda")
    if command:
        wc = [cc.term_scale[i] * (LEVEL if cc.term_by_curriculum[i] else 1.0) for i in range(cs.NUM_CMD_TERMS)]
        scaled = torch.cat([scaled, rec["command_terms"].double() * torch.tensor(wc, dtype=torch.float64,
                                                                                  device="cuda")], dim=2)
    err = (rec["reward"].double() - scaled.sum(2)).abs()
    bound = 24 * 2.0 ** -24 * scaled.abs().sum(2)
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"terms explain the reward: worst |err| / bound = {worst:.3f}, row 0: "
          f"{float((err[0] / bound[0].clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), worst
    # the summary over the recorded rollout: the reward word is the fp64 tree of out["reward"], the counts exact
    sums = ppo.rollout_summary(rec["reward"], rec["done"], rec["success"], reward_terms=rec["reward_terms"],
                               command_terms=rec.get("command_terms"), log_prob=rec["log_prob"],
                               values=rec["value"], value_targets=rec["value"])
    leaves = rec["reward"].double().reshape(-1, 1).cpu().numpy()
    assert float(sums[cs.SUM_REWARD]) == float(SC.tree_numpy(leaves)[0])
    assert float(sums[cs.SUM_DONE]) == float(rec["done"].sum())
    assert float(sums[cs.SUM_SUCCESS]) == float(rec["success"].sum())
    assert float(sums[cs.SUM_ROWS]) == T * N and float(sums[cs.SUM_RESIDUAL_SQ]) == 0.0
    host = {k: (None if rec.get(k) is None else rec[k].cpu().numpy()) for k in
            ("reward", "done", "success", "reward_terms", "command_terms", "log_prob")}
    v = rec["value"].cpu().numpy()
    same_bits(sums, ppo.rollout_summary_host(host["reward"], host["done"], host["success"],
                                             reward_terms=host["reward_terms"], command_terms=host["command_terms"],
                                             log_prob=host["log_prob"], values=v, value_targets=v))


def test_mode_rollout_is_deterministic(cmodel):
    from zbot_amd import policy as P

    acts = []
    for seed in (SEED, SEED + 1):  # the action seed does not matter to the mode
        eng, _, _ = make_engine("engine", cmodel, False)
        ro = P.PolicyRollout(eng, P.GruPolicy(ACTOR, init_params(ACTOR, seed=8)), seed=seed, curriculum=LEVEL)
        acts.append(ro.run(4, mode=MODE)["actions"])
    assert torch.equal(acts[0], acts[1])


# ---- the Trainer ----

def make_trainer(kind, cmodel, command, **kw):
    from zbot_amd import policy as P
    from zbot_amd.train import Trainer

    eng, _, cc = make_engine(kind, cmodel, False, solver="newton")
    if command:
        cc = R.joystick(0.25, CMD_SCALES, by_curriculum=("yaw_tracking", "base_height"))
    actor = P.GruPolicy(ACTOR, init_params(ACTOR, seed=8))
    critic = P.GruPolicy(CRITIC, init_params(CRITIC, seed=9))
    return Trainer(eng, actor, critic, rollout_steps=T, num_passes=PASSES, batch_size=BATCH, seed=SEED, shuffle=True,
                   curriculum=CUR, command_config=cc, **kw)


def snap(tr):
    torch.cuda.synchronize()
    sd = tr.learner.state_dict()
    out = {f"{net}.{k}": sd[net][k] for net in ("actor", "critic") for k in ("params", "m", "v")}
    out["reward"] = tr.last_rollout["reward"].clone()
    out["state"] = tr.eng.get_state()
    out["rand"] = tr.eng.get_rand()
    return out, (tr.level, tr.cur_state.steps, sd["step"], sd["epoch"], tr.iteration, tr.rollout.step_count)


def same(a, b):
    (ta, sa), (tb, sb) = a, b
    assert sa == sb, (sa, sb)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k


def telemetry_keys(command):
    names = cs.TERM_NAMES + (cs.CMD_TERM_NAMES if command else ())
    keys = {f"{form}/{name}" for form in ("terms", "terms_scaled") for name in names}
    return keys | {"reward", "reward_std", "done_rate", "failures", "time_limits", "entropy_estimate", "value_mean",
                   "explained_variance", "episodes", "episode_return", "episode_length"}


@pytest.mark.parametrize("kind,command", [("engine", False), ("groups", True)])
def test_validation_leaves_training_alone(kind, command, cmodel):
    a = make_trainer(kind, cmodel, command)
    b = make_trainer(kind, cmodel, command)
    c = make_trainer(kind, cmodel, command, telemetry=True)
    a.step()
    v1 = a.validate()
    v2 = a.validate(mode="mode")
    v3 = a.validate(mode="mode")
    ma = a.step()
    b.step()
    mb = b.step()
    same(snap(a), snap(b))
    assert ma["episode_length"] == mb["episode_length"] and torch.equal(ma["reward"], mb["reward"])
    assert "telemetry" not in mb
    # validation: every key, finite where it must be, deterministic in mode "mode"
    for v in (v1, v2):
        assert set(v) == telemetry_keys(command)
        assert all(t.dtype == torch.float64 and t.dim() == 0 and t.is_cuda for t in v.values())
        assert float(v["done_rate"]) > 0 and float(v["episodes"]) > 0
        assert float(v["failures"]) + float(v["time_limits"]) == float(v["done_rate"]) * T * N
    assert set(v2) == set(v3)
    for k in v2:
        assert torch.equal(v2[k], v3[k]) or (bool(torch.isnan(v2[k])) and bool(torch.isnan(v3[k]))), k
    # a sampled validation rollout is the rollout the next step() starts with: the same mean reward
    assert abs(float(v1["reward"]) - float(ma["reward"])) <= 1e-5 * max(1.0, abs(float(ma["reward"])))
    # telemetry=True: the same weights, and the dict
    mc = None
    for _ in range(2):
        mc = c.step()
    same(snap(c), snap(b))
    tel = mc["telemetry"]
    assert set(tel) == telemetry_keys(command)
    torch.cuda.synchronize()
    assert abs(float(tel["reward"]) - float(mb["reward"])) <= 1e-6 * max(1.0, abs(float(mb["reward"])))
    out = c.last_rollout
    assert float(tel["done_rate"]) == float(out["done"].sum()) / (T * N)
    assert float(tel["time_limits"]) == float(out["success"].sum())
    scaled = sum(float(tel[f"terms_scaled/{n}"]) for n in cs.TERM_NAMES + (cs.CMD_TERM_NAMES if command else ()))
    assert scaled == pytest.approx(float(tel["reward"]), rel=1e-5, abs=1e-6)
    assert np.isfinite(float(tel["entropy_estimate"])) and np.isfinite(float(tel["explained_variance"]))
    with pytest.raises(ZbError):
        a.validate(mode="greedy")
