"""Truncated BPTT with stored carries on the GPU: the chunked gather kernel, the carries
PolicyRollout.run(carry_every=) stores, both learners' update(seq_len=) and Trainer(seq_len=).

Bars: the gather equals its host twin byte for byte (tests/test_seq_chunks_host.py holds the twin to
the law); the stored carries are the bits the networks reach from the entry carry; with unchanged
weights the chunked forward gives back the rollout's log-probs and values bit for bit, so the first
step's clipped count and KL sum are exactly 0; HipPpoLearner.update(seq_len=) is the library calls
written out by hand on a minibatch cut with torch indexing; seq_len == T is the whole-sequence path
bit for bit; against PpoLearner the bound of tests/test_gpu_learner_update.py (1 % of the learning
rate on the elements whose gradient reaches 1e-3 of the largest).
"""

import io
import os
from datetime import timedelta

import numpy as np
import pytest
import torch

from test_gpu_learner_update import compare_case, fresh_nets, pol  # noqa: F401 - fixtures
from test_seq_chunks_host import env_index, random_array
from zbot_amd import default_config, ppo
from zbot_amd.curriculum import EpisodeLengthCurriculum
from zbot_amd.policy import ACTOR, CRITIC, EVAL, PolicyShape, init_params

pytestmark = pytest.mark.gpu
NJ = 20
# elements per row: obs_critic 1936 B and actions 80 B (16-byte accesses), obs_actor 200 B (8), values 4 B, flags 1 B
ROWS = ((484, np.float32), (50, np.float32), (20, np.float32), (1, np.float32), (1, np.uint8))
CUR = EpisodeLengthCurriculum(min_level_steps=1, increase_threshold=0.05, decrease_threshold=0.01)


# ---- 1. the gather kernel ----

def _dev(a, offset):
    """A device copy of a numpy array; offset: its storage starts 4 bytes past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    pad = 4 // t.element_size()
    buf = torch.zeros(t.numel() + pad, dtype=t.dtype, device="cuda")
    out = buf[pad:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("shuffle_seed", [None, 11])
@pytest.mark.parametrize("lo,count", [(0, 33), (16, 17), (32, 1)])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_gather_equals_the_host_twin(L, lo, count, shuffle_seed, offset):
    T, n, epoch = 6, 33, 2
    Cn = T // L
    rng = np.random.default_rng(1000 * L + 10 * lo + count)
    srcs = [random_array(rng, (T + 1, n, F) if F == 50 else (T, n, F), dt) for F, dt in ROWS]  # obs_actor: [T + 1]
    srcs += [random_array(rng, (Cn, n, 5, 128), np.float32), random_array(rng, (1, n, 5, 128), np.float32)]
    shapes = [(L, Cn * count, F) for F, _ in ROWS] + [(Cn, count, 5, 128), (1, count, 5, 128)]
    host = [np.full(s, 0x5A, x.dtype) for s, x in zip(shapes, srcs)]
    hz, hz1 = np.full((L, Cn * count), 9, np.uint8), np.full((1, count), 9, np.uint8)  # null sources
    nt = len(ROWS)  # the first nt items are time items, then the chunk carries and a whole-run carry
    mark = lambda pairs: [p + (True,) if k < nt else p for k, p in enumerate(pairs)]  # noqa: E731
    ppo.gather_minibatch_host(mark(list(zip(srcs, host))) + [(None, hz, True), (None, hz1)], n, lo, count, shuffle_seed=shuffle_seed,
                              epoch=epoch, seq_len=L)
    dsrc = [_dev(x, offset) for x in srcs]
    ddst = [_dev(np.full(s, 0x33, x.dtype), offset) for s, x in zip(shapes, srcs)]
    dz, dz1 = _dev(np.full((L, Cn * count), 9, np.uint8), offset), _dev(np.full((1, count), 9, np.uint8), offset)
    ppo.gather_minibatch(mark(list(zip(dsrc, ddst))) + [(None, dz, True), (None, dz1)], n, lo, count, shuffle_seed=shuffle_seed,
                         epoch=epoch, seq_len=L)
    torch.cuda.synchronize()
    for h, d, s in zip(host + [hz, hz1], ddst + [dz, dz1], shapes + [hz.shape, hz1.shape]):
        assert d.cpu().numpy().tobytes() == h.tobytes(), s
    # spot check against the law itself: column c count + j of the observations is chunk c of env idx[j]
    idx = env_index(n, lo, count, shuffle_seed, epoch)
    got = ddst[0].cpu().numpy()
    for c in range(Cn):
        assert got[:, c * count:(c + 1) * count].tobytes() == np.ascontiguousarray(srcs[0][c * L:(c + 1) * L][:, idx]).tobytes()


def test_gather_refusals_launch_nothing():
    import ctypes as C

    from zbot_amd.engine import load_library

    lib = load_library()
    T, n, count = 6, 8, 4
    src = torch.ones(T, n, 3, device="cuda")
    dst = torch.full((T, count, 3), 7.0, device="cuda")
    arr = (ppo.ZbGatherItem * 1)(ppo.ZbGatherItem(src.data_ptr(), dst.data_ptr(), T, 12, n * 12))
    cut = (C.c_int32 * 1)(1)
    for L in (4, 0, -1):
        assert lib.zb_minibatch_gather_seq(arr, cut, 1, L, n, 0, count, 1, 0, 0, None) == -1
        assert b"seq_len" in lib.zb_last_error()
    assert lib.zb_minibatch_gather_seq(arr, None, 1, 2, n, 0, count, 1, 0, 0, None) == -1
    assert lib.zb_minibatch_gather_seq(arr, cut, 1, 2, n, 5, count, 1, 0, 0, None) == -1
    torch.cuda.synchronize()
    assert torch.all(dst == 7.0)
    assert lib.zb_minibatch_gather_seq(arr, cut, 1, 2, n, 0, count, 1, 0, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.all(dst == 1.0)


# ---- helpers: the law in torch indexing ----

def chunk_t(x, T, L, idx):
    """[>= T, n, ...] -> [L, C b, ...]: column c b + j is rows c L .. c L + L - 1 of env idx[j]."""
    y = x[:T].index_select(1, idx)
    tail = tuple(y.shape[2:])
    return y.reshape((T // L, L, len(idx)) + tail).transpose(0, 1).reshape((L, (T // L) * len(idx)) + tail).contiguous()


def unchunk_t(y, T, L, b):
    """chunk_t's inverse for idx = arange(b): [L, C b, ...] -> [T, b, ...]."""
    tail = tuple(y.shape[2:])
    return y.reshape((L, T // L, b) + tail).transpose(0, 1).reshape((T, b) + tail).contiguous()


def chunk_carry(x, idx):
    """[C, n, depth, 128] -> [C b, depth, 128]."""
    y = x.index_select(1, idx)
    return y.reshape((-1,) + tuple(y.shape[2:])).contiguous()


def env_idx(n, lo, count, seed, epoch):
    return torch.from_numpy(env_index(n, lo, count, seed, epoch)).cuda()


def reset_rows(prev_done, done, T):
    r = torch.zeros(T, done.shape[1], dtype=torch.uint8, device="cuda")
    if prev_done is not None:
        r[0] = prev_done
    r[1:] = done[:T - 1]
    return r


# ---- 2. the rollout's chunk carries ----

def _engine(kind, cmodel, n, max_episode_sec=0.06):
    from zbot_amd.engine import EnvGroups, HipEngine

    cfg = default_config(solver="newton", max_episode_sec=max_episode_sec)
    return HipEngine(cmodel, cfg, n, seed=2) if kind == "engine" else EnvGroups(cmodel, cfg, n, groups=2, seed=2)


def _two_runs(pol, kind, cmodel, actor, critic, n, T, carry_every):  # noqa: F811
    """A run of T steps, then the run under test: its row 0 resets with the first run's last done flags."""
    ro = pol.PolicyRollout(_engine(kind, cmodel, n), actor, seed=5)
    cc = critic.initial_carry(n)
    ro.run(T, record_critic=True, critic=critic, critic_carry=cc)
    entry, centry, prev = ro.carry.clone(), cc.clone(), ro.done.clone()
    kw = {} if carry_every is None else dict(carry_every=carry_every)
    out = ro.run(T, record_critic=True, critic=critic, critic_carry=cc, **kw)
    torch.cuda.synchronize()
    return out, entry, centry, prev, ro.carry.clone(), cc.clone()


@pytest.mark.parametrize("kind,shaped", [("engine", False), ("groups", False), ("engine", True)],
                         ids=["engine", "groups", "engine-depth2x3-critic1"])
def test_rollout_stores_the_carries_at_chunk_starts(pol, cmodel, kind, shaped):  # noqa: F811
    n, T, L = 64, 6, 2
    sa, sc = (PolicyShape(2, 3), PolicyShape(1)) if shaped else (PolicyShape(), PolicyShape())

    def nets():
        return (pol.GruPolicy(ACTOR, init_params(ACTOR, seed=8, shape=sa), shape=sa),
                pol.GruPolicy(CRITIC, init_params(CRITIC, seed=9, shape=sc), shape=sc))

    plain, *_ = _two_runs(pol, kind, cmodel, *nets(), n, T, None)
    actor, critic = nets()
    out, entry, centry, prev, end, cend = _two_runs(pol, kind, cmodel, actor, critic, n, T, L)
    assert set(out) - set(plain) == {"actor_carry_chunks", "critic_carry_chunks"}
    for k in plain:
        assert torch.equal(plain[k], out[k]), k
    ac, ccs = out["actor_carry_chunks"], out["critic_carry_chunks"]
    assert tuple(ac.shape) == (T // L, n, sa.depth, 128) and tuple(ccs.shape) == (T // L, n, sc.depth, 128)
    # the fixture: a reset row on a chunk's first row and one inside a chunk, and carries that are not all zero
    rs = reset_rows(prev, out["done"], T)
    rows = rs.any(1).cpu().numpy()
    assert rows[0::L].any() and rows[1::L].any(), rows
    assert bool(entry.any()) and bool(rs[0].any())
    assert torch.equal(ac[0], entry) and torch.equal(ccs[0], centry)
    crs = rs.clone()
    crs[0] = 0  # the in-loop critic resets nothing at t = 0
    for c in range(1, T // L + 1):
        carry, ccarry = entry.clone(), centry.clone()
        actor.actor(out["obs_actor"][:c * L], carry, reset=rs[:c * L], mode=EVAL, actions=out["actions"][:c * L])
        critic.critic(out["obs_critic"][:c * L], ccarry, reset=crs[:c * L])
        torch.cuda.synchronize()
        want, cwant = (ac[c], ccs[c]) if c < T // L else (end, None)
        assert torch.equal(carry, want), c
        if cwant is not None:
            assert torch.equal(ccarry, cwant), c
    assert not torch.equal(ac[1], ac[0]) and not torch.equal(ccs[1], ccs[0])


def test_carry_every_must_divide(pol, cmodel):  # noqa: F811
    actor = pol.GruPolicy(ACTOR, init_params(ACTOR, seed=8))
    ro = pol.PolicyRollout(_engine("engine", cmodel, 4), actor, seed=5)
    for bad in (4, 0, -2, 1.5):
        with pytest.raises(ppo.ZbError, match="carry_every"):
            ro.run(6, carry_every=bad)
    out = ro.run(6, carry_every=3)  # no critic: the actor's chunks alone
    assert "critic_carry_chunks" not in out and tuple(out["actor_carry_chunks"].shape) == (2, 4, 5, 128)


# ---- the learner fixtures ----

def _rollout(pol, cmodel, T, n, carry_every):  # noqa: F811
    """A first rollout after reset() (row 0 carries no reset) with episodes of 3 steps: reset row 3."""
    from zbot_amd.engine import HipEngine

    eng = HipEngine(cmodel, default_config(solver="newton", max_episode_sec=0.06), n, seed=2)
    pa, pc = init_params(ACTOR, seed=8), init_params(CRITIC, seed=9)
    actor, critic = pol.GruPolicy(ACTOR, pa), pol.GruPolicy(CRITIC, pc)
    ro = pol.PolicyRollout(eng, actor, seed=5)
    ro.reset()
    carry0 = ro.carry.clone()
    ccarry = critic.initial_carry(n)
    ccarry0 = ccarry.clone()
    out = ro.run(T, record_critic=True, critic=critic, critic_carry=ccarry, carry_every=carry_every)
    reset = reset_rows(None, out["done"], T)
    inputs = ppo.compute_ppo_inputs(out["value"], out["reward"], out["done"], out["success"], bootstrap=out["value_next"])
    torch.cuda.synchronize()
    assert bool(reset[3].any())
    out = {k: v.clone() for k, v in out.items()}
    return dict(T=T, n=n, out=out, inputs=inputs, carry0=carry0, ccarry0=ccarry0, reset=reset, pa=pa, pc=pc)


@pytest.fixture(scope="module")
def rollout6(pol, cmodel):  # noqa: F811
    """n = 33, T = 6 with the carries of every step stored: the chunk carries of L are every L-th row."""
    return _rollout(pol, cmodel, 6, 33, 1)


@pytest.fixture(scope="module")
def rollout4(pol, cmodel):  # noqa: F811
    """n = 33, T = 4, chunks of 2: minibatches of 16 envs are 16, 16 and 1 envs, 32, 32 and 2 sequences."""
    return _rollout(pol, cmodel, 4, 33, 2)


def with_chunks(r, L):
    out = dict(r["out"])
    for k in ("actor_carry_chunks", "critic_carry_chunks"):
        out[k] = r["out"][k][::L].contiguous()
    return dict(r, out=out)


# ---- 3. the exact first pass ----

@pytest.mark.parametrize("seed", [None, 7])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_first_pass_reproduces_the_rollout(pol, rollout6, L, seed):  # noqa: F811
    from zbot_amd.learner import _ShuffledMinibatches

    r = with_chunks(rollout6, L)
    T, n = r["T"], r["n"]
    actor, critic = fresh_nets(pol, r)
    for lo, count in ((0, 17), (17, 16)):
        mb = _ShuffledMinibatches().cut_chunks(torch, r["out"], r["inputs"], r["reset"], T, n, lo, count, seed, 0, L)
        lp, _ = actor.actor_train(mb["obs_a"], mb["acts"], mb["ca"], mb["rs"])
        v, _ = critic.critic_train(mb["obs_c"], mb["cc"], mb["rs"])
        _, _, sums = ppo.ppo_loss_grad(lp, mb["old_lp"], mb["adv"], v, mb["old_v"], mb["vt"])
        torch.cuda.synchronize()
        assert tuple(lp.shape) == (L, (T // L) * count, NJ)
        assert torch.equal(lp, mb["old_lp"]) and torch.equal(v, mb["old_v"])
        assert sums[2].item() == 0.0 and sums[3].item() == 0.0
        # and the gathered arrays are the law on the rollout
        idx = env_idx(n, lo, count, seed, 0)
        assert torch.equal(mb["old_lp"], chunk_t(r["out"]["log_prob"], T, L, idx))
        assert torch.equal(mb["ca"], chunk_carry(r["out"]["actor_carry_chunks"], idx))
        assert torch.equal(mb["rs"], chunk_t(r["reset"], T, L, idx))
    assert bool(r["out"]["actor_carry_chunks"][-1].any())  # not a run of zero carries


# ---- 4. and 5. HipPpoLearner.update(seq_len=) ----

def run_update(learner, r, actor, critic, **kw):
    return learner.update(r["out"], r["inputs"], actor, critic, r["carry0"], r["ccarry0"], reset=r["reset"], **kw)


def state_equal(a, b):
    return all(torch.equal(a[net][k], b[net][k]) for net in ("actor", "critic") for k in ("params", "m", "v"))


@pytest.mark.parametrize("seed", [None, 13])
def test_seq_len_of_the_whole_rollout_is_todays_path(pol, rollout4, seed):  # noqa: F811
    from zbot_amd.learner import HipPpoLearner

    r = rollout4
    res = []
    for kw in ({}, dict(seq_len=r["T"])):
        for drop in (False, True):  # seq_len = T reads no chunk carries
            if drop and not kw:
                continue
            rr = dict(r, out={k: v for k, v in r["out"].items() if not k.endswith("_chunks")}) if drop else r
            actor, critic = fresh_nets(pol, r)
            ln = HipPpoLearner(learning_rate=3e-4, max_grad_norm=1e-3, weight_decay=1e-5, shuffle_seed=seed)
            sums = run_update(ln, rr, actor, critic, num_passes=2, batch_size=16, **kw)
            torch.cuda.synchronize()
            res.append((ln.state_dict(), sums))
    for sd, sums in res[1:]:
        assert state_equal(sd, res[0][0])
        assert len(sums) == len(res[0][1]) and all(torch.equal(x, y) for x, y in zip(sums, res[0][1]))


def by_hand_chunks(pol, r, L, num_passes, batch_size, lr, max_norm, wd, seed):  # noqa: F811
    """HipPpoLearner.update(seq_len=L)'s library calls written out, the minibatch cut by torch indexing."""
    actor, critic = fresh_nets(pol, r)
    T, n, out, inp = r["T"], r["n"], r["out"], r["inputs"]
    st = {}
    for net, h in (("a", actor), ("c", critic)):
        p = h.params_tensor()
        st[net] = [p, torch.zeros_like(p), torch.zeros_like(p)]
    sq = torch.zeros(2, dtype=torch.float64, device="cuda")
    step, all_sums = 0, []
    for epoch in range(num_passes):
        for lo in range(0, n, batch_size):
            idx = env_idx(n, lo, min(n, lo + batch_size) - lo, seed, epoch)
            cut = lambda x: chunk_t(x, T, L, idx)  # noqa: E731
            obs_a, acts, obs_c, rs = cut(out["obs_actor"]), cut(out["actions"]), cut(out["obs_critic"]), cut(r["reset"])
            ca, cc = chunk_carry(out["actor_carry_chunks"], idx), chunk_carry(out["critic_carry_chunks"], idx)
            lp, sa = actor.actor_train(obs_a, acts, ca, rs)
            v, sc = critic.critic_train(obs_c, cc, rs)
            d_lp, d_v, sums = ppo.ppo_loss_grad(lp, cut(out["log_prob"]), cut(inp.advantages_t), v, cut(out["value"]),
                                                cut(inp.value_targets_t))
            gc = critic.critic_backward(obs_c, cc, rs, d_v, sc)
            ga = actor.actor_backward(obs_a, acts, ca, rs, d_lp, sa)
            ppo.grad_sqnorm(ga, out=sq[0:1])
            ppo.grad_sqnorm(gc, out=sq[1:2])
            step += 1
            ppo.adamw_step(*st["a"][:1], ga, *st["a"][1:], sq, step, lr, max_grad_norm=max_norm, weight_decay=wd,
                           frozen_tail=NJ)
            ppo.adamw_step(*st["c"][:1], gc, *st["c"][1:], sq, step, lr, max_grad_norm=max_norm, weight_decay=wd)
            actor.set_params(st["a"][0])
            critic.set_params(st["c"][0])
            all_sums.append(sums.clone())
    torch.cuda.synchronize()
    return st, all_sums


@pytest.mark.parametrize("seed", [None, 13])
def test_update_equals_the_calls_by_hand(pol, rollout4, seed):  # noqa: F811
    from zbot_amd.learner import HipPpoLearner

    r, L = rollout4, 2
    lr, mx, wd = 3e-4, 1e-3, 1e-5  # a maximum the gradient norm exceeds, so that the clip scales
    st, sums_hand = by_hand_chunks(pol, r, L, 2, 16, lr, mx, wd, seed)
    actor, critic = fresh_nets(pol, r)
    ln = HipPpoLearner(learning_rate=lr, max_grad_norm=mx, weight_decay=wd, shuffle_seed=seed)
    # the entry carries are not read on this path: poison them
    sums = ln.update(r["out"], r["inputs"], actor, critic, torch.full_like(r["carry0"], float("nan")),
                     torch.full_like(r["ccarry0"], float("nan")), reset=r["reset"], num_passes=2, batch_size=16, seq_len=L)
    torch.cuda.synchronize()
    assert len(sums) == 6 and ln.step == 6 and ln.epoch == 2
    for a, b in zip(sums, sums_hand):
        assert torch.equal(a[:4], b)
    assert [float(s[4]) for s in sums] == [64.0, 64.0, 4.0] * 2  # the rows T b, whatever the chunks
    assert float(sums[0][2]) == 0.0 and float(sums[0][3]) == 0.0  # the first step: ratio exactly 1
    sd = ln.state_dict()
    for net, key in (("actor", "a"), ("critic", "c")):
        for name, x in zip(("params", "m", "v"), st[key]):
            assert torch.equal(sd[net][name], x), (net, name)
            assert torch.isfinite(x).all()
    assert torch.equal(actor.params_tensor(), sd["actor"]["params"])
    # reset=None builds the same rows (a first rollout: row 0 zeros, row t done[t - 1])
    a2, c2 = fresh_nets(pol, r)
    l2 = HipPpoLearner(learning_rate=lr, max_grad_norm=mx, weight_decay=wd, shuffle_seed=seed)
    l2.update(r["out"], r["inputs"], a2, c2, r["carry0"], r["ccarry0"], reset=None, num_passes=2, batch_size=16, seq_len=L)
    assert state_equal(l2.state_dict(), sd)
    # truncation changes the gradient: not the whole-sequence result
    a3, c3 = fresh_nets(pol, r)
    l3 = HipPpoLearner(learning_rate=lr, max_grad_norm=mx, weight_decay=wd, shuffle_seed=seed)
    run_update(l3, r, a3, c3, num_passes=2, batch_size=16, seq_len=r["T"])
    torch.cuda.synchronize()
    assert not torch.equal(l3.state_dict()["actor"]["m"], sd["actor"]["m"])


# ---- 6. against the torch learner ----

def test_one_step_against_the_torch_learner(pol):  # noqa: F811
    """tests/test_gpu_learner_update.py's construction and bound at T = 4, L = 2: the chunk carries are
    synthetic, of the fixture's carry scale (row 0 is the fixture's carry itself)."""
    from zbot_amd.learner import HipPpoLearner, PpoLearner, TrainablePolicy
    from zbot_amd.ppo import PPOInputs

    c = compare_case()
    T, n, L = c["T"], c["n"], 2
    Cn = T // L
    lr = 3e-4
    rng = np.random.default_rng(77)
    d = lambda k: torch.from_numpy(c[k]).cuda()  # noqa: E731
    chunks = {}
    for k in ("carry_a", "carry_c"):
        extra = (0.5 * rng.normal(size=(Cn - 1,) + c[k].shape)).astype(np.float32)
        chunks[k] = torch.from_numpy(np.concatenate([c[k][None], extra])).cuda()
    idx = torch.arange(n, device="cuda")
    ch = lambda x: chunk_t(x, T, L, idx)  # noqa: E731
    obs_a, acts, obs_c, rs = ch(d("obs_a")), ch(d("actions")), ch(d("obs_c")), ch(d("reset"))
    ca, cc = chunk_carry(chunks["carry_a"], idx), chunk_carry(chunks["carry_c"], idx)
    probe_a, probe_c = pol.GruPolicy(ACTOR, c["Pa"]), pol.GruPolicy(CRITIC, c["Pc"])
    lp_ch, sa = probe_a.actor_train(obs_a, acts, ca, rs)
    v_ch, sc = probe_c.critic_train(obs_c, cc, rs)
    lp, v = unchunk_t(lp_ch, T, L, n), unchunk_t(v_ch, T, L, n)
    ro = dict(obs_actor=d("obs_a"), actions=d("actions"), obs_critic=d("obs_c"), log_prob=lp + d("dlp"), value=v + d("dv"),
              actor_carry_chunks=chunks["carry_a"], critic_carry_chunks=chunks["carry_c"])
    inputs = PPOInputs(advantages_t=d("adv"), value_targets_t=v + d("dtgt"), gae_t=None, returns_t=None)
    # the gradient that decides which elements are compared: the library's own, on the chunks
    d_lp, d_v, _ = ppo.ppo_loss_grad(lp_ch, ch(ro["log_prob"]), ch(inputs.advantages_t), v_ch, ch(ro["value"]),
                                     ch(inputs.value_targets_t))
    grads = dict(actor=probe_a.actor_backward(obs_a, acts, ca, rs, d_lp, sa).clone(),
                 critic=probe_c.critic_backward(obs_c, cc, rs, d_v, sc).clone())

    def one_step(cls, wrap):
        a, k = pol.GruPolicy(ACTOR, c["Pa"]), pol.GruPolicy(CRITIC, c["Pc"])
        cls(learning_rate=lr).update(ro, inputs, wrap(a), wrap(k), d("carry_a"), d("carry_c"), reset=d("reset"),
                                     num_passes=1, batch_size=n, seq_len=L)
        torch.cuda.synchronize()
        return dict(actor=a.params_tensor().double(), critic=k.params_tensor().double())

    hip = one_step(HipPpoLearner, lambda h: h)
    ref = one_step(PpoLearner, TrainablePolicy)
    for net, p0 in (("actor", c["Pa"]), ("critic", c["Pc"])):
        live = p0.size - (NJ if net == "actor" else 0)
        g = grads[net][:live].abs()
        mask = g >= 1e-3 * g.max()
        share = mask.double().mean().item()
        p0d = torch.from_numpy(p0).cuda().double()
        dh, dr = (hip[net] - p0d)[:live][mask], (ref[net] - p0d)[:live][mask]
        worst = (dh - dr).abs().max().item()
        print(f"VSTORCH-CHUNKS {net} compared share={share:.3f} max |dp_hip - dp_torch| = {worst:.3e} = "
              f"{worst / lr:.2e} lr; max |dp| = {dh.abs().max().item():.3e}")
        assert share >= 0.5
        assert worst <= 0.01 * lr
        assert dh.abs().max().item() > 0.5 * lr  # the step did move them
    assert torch.equal(hip["actor"][-NJ:], ref["actor"][-NJ:])


# ---- 7. Trainer(seq_len=) ----

TN, TT, TBATCH, TPASSES, TSEED = 64, 6, 32, 2, 5


def make_trainer(kind, cmodel, weights=(8, 9), **kw):
    from zbot_amd import policy as P
    from zbot_amd.train import Trainer

    actor = P.GruPolicy(ACTOR, init_params(ACTOR, seed=weights[0]))
    critic = P.GruPolicy(CRITIC, init_params(CRITIC, seed=weights[1]))
    # episodes of 5 or 6 steps: the reset rows move through the chunks from one iteration to the next
    return Trainer(_engine(kind, cmodel, TN, max_episode_sec=0.1), actor, critic, rollout_steps=TT, num_passes=TPASSES,
                   batch_size=TBATCH, seed=TSEED, shuffle=True, curriculum=CUR, **kw)


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
def test_trainer_reproducible_and_resumable(kind, cmodel):
    from zbot_amd.engine import ZbError

    a = make_trainer(kind, cmodel, seq_len=2)
    snaps = []
    for _ in range(3):
        m = a.step()
        snaps.append(snap(a))
    assert tuple(a.last_rollout["actor_carry_chunks"].shape) == (3, TN, 5, 128)
    assert bool(a.last_rollout["done"].any())  # episodes ended inside the runs
    assert float(m["sums"][0][4]) == TT * TBATCH
    assert not torch.equal(snaps[0][0]["actor.params"], snaps[1][0]["actor.params"])
    b = make_trainer(kind, cmodel, seq_len=2)
    for i in range(3):
        b.step()
        same(snap(b), snaps[i])
    b.validate()  # records no chunk carries and leaves the Trainer where it was
    a.step()
    b.step()
    same(snap(a), snap(b))
    c = make_trainer(kind, cmodel, seq_len=2)
    c.step()
    c.step()
    sd = c.state_dict()
    assert sd["seq_len"] == 2
    f = io.BytesIO()
    torch.save(sd, f)
    del c
    f.seek(0)
    d = make_trainer(kind, cmodel, weights=(1, 2), seq_len=2)
    d.load_state_dict(torch.load(f, weights_only=False))
    assert d.iteration == 2
    d.step()
    same(snap(d), snaps[2])
    e = make_trainer(kind, cmodel, seq_len=3)
    with pytest.raises(ZbError, match="seq_len"):
        e.load_state_dict(sd)


@pytest.mark.parametrize("kind", ["engine", "groups"])
def test_trainer_seq_len_of_the_whole_rollout_is_todays_path(kind, cmodel):
    from zbot_amd.engine import ZbError

    a, b = make_trainer(kind, cmodel), make_trainer(kind, cmodel, seq_len=TT)
    for _ in range(2):
        a.step()
        b.step()
        same(snap(a), snap(b))
    assert "actor_carry_chunks" not in b.last_rollout and "seq_len" not in a.state_dict()
    # a different result with chunks: the option does something
    c = make_trainer(kind, cmodel, seq_len=2)
    c.step()
    c.step()
    assert not torch.equal(snap(c)[0]["actor.params"], snap(a)[0]["actor.params"])
    with pytest.raises(ZbError, match="seq_len"):
        make_trainer(kind, cmodel, seq_len=4)
    # seq_len = T and None are one spelling: the states load into each other (load drops last_rollout: done last)
    sd_b = b.state_dict()
    assert "seq_len" not in sd_b and b.seq_len is None
    a.load_state_dict(sd_b)
    b.load_state_dict(a.state_dict())


# ---- 8. two ranks ----

WORLD, N_LOCAL = 2, 32
KW = dict(learning_rate=1e-3, max_grad_norm=0.5, weight_decay=1e-4)  # a maximum the gradient norm exceeds
TIMEOUT = timedelta(seconds=60)


def _seq_rank(rank, world, port, outdir):
    import torch.distributed as dist

    from zbot_amd import compile_model
    from zbot_amd import policy as P
    from zbot_amd.engine import HipEngine, ZbError
    from zbot_amd.train import Trainer

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
    g = dist.group.WORLD

    def trainer(seq_len):
        eng = HipEngine(compile_model(), default_config(solver="newton", max_episode_sec=0.1), N_LOCAL,
                        env_offset=N_LOCAL * rank, seed=2)
        actor = P.GruPolicy(ACTOR, init_params(ACTOR, seed=8))
        critic = P.GruPolicy(CRITIC, init_params(CRITIC, seed=9))
        return Trainer(eng, actor, critic, rollout_steps=TT, num_passes=TPASSES, batch_size=TBATCH, seed=TSEED,
                       shuffle=True, curriculum=CUR, group=g, seq_len=seq_len, **KW)

    refused = ""
    try:
        trainer(2 if rank == 0 else 3)
    except ZbError as e:
        refused = str(e)
    tr = trainer(2)
    for _ in range(2):
        m = tr.step()
    torch.cuda.synchronize()
    sd = tr.learner.state_dict()
    out = {f"{net}.{k}": sd[net][k].cpu() for net in ("actor", "critic") for k in ("params", "m", "v")}
    out["sums"] = torch.stack(m["sums"]).cpu()
    out["handle"] = tr.actor.params_tensor().cpu()
    out["refused"] = refused
    # the learner's own agreement, were the Trainers' skipped. Neither rank passes the seq_len = 2 it
    # has agreed on: check_ranks asks the other ranks only about a shape that is new to it
    try:
        tr.learner.check_ranks(N_LOCAL, TT, TBATCH, TPASSES, seq_len=1 if rank == 0 else 3)
        out["learner_refused"] = ""
    except ZbError as e:
        out["learner_refused"] = str(e)
    torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks(tmp_path):
    from test_gpu_dp_trainer import spawn

    assert torch.cuda.is_available()
    spawn(_seq_rank, WORLD, str(tmp_path))
    a, b = (torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(WORLD))
    for k in a:
        if k.endswith((".params", ".m", ".v")) or k in ("sums", "handle"):
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["handle"], a["actor.params"]) and torch.isfinite(a["actor.params"]).all()
    assert torch.all(a["sums"][:, 4] == TT * TBATCH)
    for r in (a, b):
        assert "seq_len" in r["refused"] and "seq_len" in r["learner_refused"], r["refused"]


# ---- 9. refusals ----

def test_refusals_name_their_cause(pol, rollout4):  # noqa: F811
    from zbot_amd.engine import ZbError
    from zbot_amd.learner import HipPpoLearner, PpoLearner, TrainablePolicy

    r = rollout4
    out = r["out"]

    def update(cls, ro, seq_len):
        actor, critic = fresh_nets(pol, r)
        wrap = TrainablePolicy if cls is PpoLearner else (lambda h: h)
        return cls().update(ro, r["inputs"], wrap(actor), wrap(critic), r["carry0"], r["ccarry0"], reset=r["reset"],
                            num_passes=1, batch_size=16, seq_len=seq_len)

    for cls in (HipPpoLearner, PpoLearner):
        for bad in (3, 0, -1, 8):
            with pytest.raises(ZbError, match="seq_len"):
                update(cls, out, bad)
        for name in ("actor_carry_chunks", "critic_carry_chunks"):
            with pytest.raises(ZbError, match=name):
                update(cls, {k: v for k, v in out.items() if k != name}, 2)
        with pytest.raises(ZbError, match="actor_carry_chunks"):    # C = 4 rows for seq_len = 2
            update(cls, dict(out, actor_carry_chunks=out["actor_carry_chunks"].repeat(2, 1, 1, 1)), 2)
        with pytest.raises(ZbError, match="actor_carry_chunks"):    # the rows of seq_len = 2 for seq_len = 1
            update(cls, out, 1)
        with pytest.raises(ZbError, match="critic_carry_chunks"):   # depth 4
            update(cls, dict(out, critic_carry_chunks=out["critic_carry_chunks"][:, :, :4].contiguous()), 2)
        with pytest.raises(ZbError, match="actor_carry_chunks"):    # another env count
            update(cls, dict(out, actor_carry_chunks=out["actor_carry_chunks"][:, :32].contiguous()), 2)
