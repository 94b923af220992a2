"""zbot_amd.train.Trainer on the GPU: the iteration is the blocks wired by hand, runs are
reproducible, and a run continued from state_dict() in fresh engine and policy handles equals the
uninterrupted one bit for bit. 64 envs, T = 8, batch 32, 2 passes; the model, config and weights
are the ones tests/test_gpu_policy.py rolls out with. The curriculum moves after one update at a
level and at a 0.05 s episode length, so the level changes inside the runs and its state is part
of what a resume has to restore.
"""

import io

import pytest
import torch

from zbot_amd import default_config, ppo
from zbot_amd.curriculum import EpisodeLengthCurriculum, rollout_episode_length
from zbot_amd.policy import ACTOR, CRITIC, init_params

pytestmark = pytest.mark.gpu
N, T, BATCH, PASSES, SEED = 64, 8, 32, 2, 5
CUR = EpisodeLengthCurriculum(min_level_steps=1, increase_threshold=0.05, decrease_threshold=0.01)


def make_engine(kind, cmodel):
    from zbot_amd.engine import EnvGroups, HipEngine

    cfg = default_config(solver="newton")
    return HipEngine(cmodel, cfg, N, seed=2) if kind == "engine" else EnvGroups(cmodel, cfg, N, groups=2, seed=2)


def make_trainer(kind, cmodel, weights=(8, 9), **kw):
    from zbot_amd import policy as P
    from zbot_amd.train import Trainer

    actor = P.GruPolicy(ACTOR, init_params(ACTOR, seed=weights[0]))
    critic = P.GruPolicy(CRITIC, init_params(CRITIC, seed=weights[1]))
    return Trainer(make_engine(kind, cmodel), actor, critic, rollout_steps=T, num_passes=PASSES, batch_size=BATCH,
                   seed=SEED, shuffle=True, curriculum=CUR, **kw)


def snap(tr):
    torch.cuda.synchronize()
    sd = tr.learner.state_dict()
    out = {f"{net}.{k}": sd[net][k] for net in ("actor", "critic") for k in ("params", "m", "v")}
    out["reward"] = tr.last_rollout["reward"].clone()
    return out, (tr.level, tr.cur_state.steps, sd["step"], sd["epoch"], tr.iteration)


def same(a, b):
    (ta, sa), (tb, sb) = a, b
    assert sa == sb, (sa, sb)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k


@pytest.mark.parametrize("kind", ["engine", "groups"])
def test_reproducible_and_resumable(kind, cmodel):
    a = make_trainer(kind, cmodel)
    snaps, levels = [], []
    for _ in range(4):
        m = a.step()
        levels.append(m["level"])
        snaps.append(snap(a))
    assert m["iteration"] == 4 and len(set(levels)) > 1  # the curriculum moved
    assert snaps[3][1][2:] == (4 * PASSES * (N // BATCH), 4 * PASSES, 4)
    assert not torch.equal(snaps[0][0]["actor.params"], snaps[1][0]["actor.params"])
    # two fresh Trainers from the same seeds: identical bits over 3 iterations
    b = make_trainer(kind, cmodel)
    for i in range(3):
        b.step()
        same(snap(b), snaps[i])
    # 2 iterations, save, load into fresh engine and handles (created from other weights), 2 more
    c = make_trainer(kind, cmodel)
    c.step()
    c.step()
    f = io.BytesIO()
    torch.save(c.state_dict(), f)
    del c
    f.seek(0)
    d = make_trainer(kind, cmodel, weights=(1, 2))
    d.load_state_dict(torch.load(f, weights_only=False))
    assert d.iteration == 2
    for i in (2, 3):
        d.step()
        same(snap(d), snaps[i])


def test_step_equals_the_wiring_by_hand(cmodel):
    from zbot_amd import policy as P
    from zbot_amd.learner import HipPpoLearner

    kw = dict(learning_rate=1e-3, max_grad_norm=0.5, weight_decay=1e-4)
    tr = make_trainer("engine", cmodel, **kw)
    m = tr.step()
    got = snap(tr)
    # by hand
    eng = make_engine("engine", cmodel)
    actor = P.GruPolicy(ACTOR, init_params(ACTOR, seed=8))
    critic = P.GruPolicy(CRITIC, init_params(CRITIC, seed=9))
    level = CUR.initial_state().level
    ro = P.PolicyRollout(eng, actor, seed=SEED, curriculum=level)
    eng.get_stats(clear=True)
    ro.reset()
    carry0 = ro.carry.clone()
    ccarry = critic.initial_carry(N)
    ccarry0 = ccarry.clone()
    out = ro.run(T, record_critic=True, critic=critic, critic_carry=ccarry)
    inputs = ppo.compute_ppo_inputs(out["value"], out["reward"], out["done"], out["success"], bootstrap=out["value_next"])
    ln = HipPpoLearner(shuffle_seed=SEED, **kw)
    sums = ln.update(out, inputs, actor, critic, carry0, ccarry0, reset=None, num_passes=PASSES, batch_size=BATCH)
    length = rollout_episode_length(eng.get_stats(), eng.get_state(), out["done"][T - 1], 0.02)
    state = CUR.update(CUR.initial_state(), length)
    torch.cuda.synchronize()
    sd = ln.state_dict()
    for net in ("actor", "critic"):
        for k in ("params", "m", "v"):
            assert torch.equal(got[0][f"{net}.{k}"], sd[net][k]), (net, k)
    assert torch.equal(got[0]["reward"], out["reward"])
    assert torch.equal(tr.actor.params_tensor(), actor.params_tensor())
    assert (tr.level, tr.cur_state.steps) == (state.level, state.steps)
    # the metrics are the returned sums' means
    assert m["iteration"] == 1 and m["level"] == level and m["episode_length"] == length
    assert len(m["sums"]) == len(sums) == PASSES * (N // BATCH)
    for x, y in zip(m["sums"], sums):
        assert torch.equal(x, y)
    assert torch.equal(m["loss"], torch.stack([HipPpoLearner.loss(s) for s in sums]))
    assert torch.equal(m["clip_fraction"], torch.stack([s[2] / s[4] for s in sums]))
    assert torch.equal(m["approx_kl"], torch.stack([s[3] / s[4] for s in sums]))
    assert torch.equal(m["reward"], out["reward"].mean())
    assert m["loss"].is_cuda and m["reward"].is_cuda and torch.isfinite(m["loss"]).all()
