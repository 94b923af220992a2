"""The learner's loss, gradient norm and AdamW kernels (csrc/zb_learner.hip, include/zbot_ppo.h
"Learner") and zbot_amd.learner.HipPpoLearner over them, on the GPU.

Kernel bar: the bits of the host twins (zb_ppo_loss_host, zb_grad_sqnorm_host, zb_adamw_step_host),
which tests/test_learner_host.py holds to fp64 torch on the CPU; same fixtures and shapes
(tests/learner_cases.py). Every kernel test also runs from storage that is not 16-byte aligned,
where the kernels take their scalar path.

Learner bar: HipPpoLearner.update equals, bit for bit, the same library calls made by hand; against
PpoLearner (torch loss, clip and AdamW over the same backward kernels), one step from the same
weights moves every parameter whose gradient is at least 1e-3 of its network's largest by the
same amount within 1 % of the learning rate (a relative gradient difference d moves Adam's first
step by at most lr d / 4; below the threshold that step is a sign function of noise).
"""

import ctypes as C

import numpy as np
import pytest
import torch

import learner_cases as LC
from zbot_amd import ppo
from zbot_amd.policy import ACTOR, CRITIC, init_params

pytestmark = pytest.mark.gpu
NJ, D, H = 20, 5, 128
LOSS_KEYS = ("log_prob", "old_log_prob", "advantages", "values", "old_values", "value_targets")


@pytest.fixture(scope="module")
def pol():
    from zbot_amd import policy as P

    assert torch.cuda.is_available()
    return P


def dev(x, misalign=False):
    """A device copy of a numpy array; misalign: at an address that is 4 but not 16 bytes aligned."""
    t = torch.from_numpy(np.array(x))  # a copy: the shared fixtures are read-only
    if not misalign:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def gpu_loss(c, use_clip, misalign=False, total=None):
    ins = [dev(c[k], misalign) for k in LOSS_KEYS]
    T, n = c["T"], c["n"]
    d_lp = dev(np.zeros((T, n, NJ), np.float32), misalign)
    d_lp, d_v, sums = ppo.ppo_loss_grad(*ins, total=total, clip_param=LC.EPS, value_loss_coef=LC.COEF,
                                        use_clipped_value_loss=use_clip, log_clip_value=LC.L_CLIP, d_log_prob=d_lp)
    torch.cuda.synchronize()
    return d_lp.cpu().numpy(), d_v.cpu().numpy(), sums.cpu().numpy()


def host_loss(c, use_clip, total=None):
    return ppo.ppo_loss_grad_host(*(c[k] for k in LOSS_KEYS), total=total, clip_param=LC.EPS, value_loss_coef=LC.COEF,
                                  use_clipped_value_loss=use_clip, log_clip_value=LC.L_CLIP)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("use_clip", [True, False])
@pytest.mark.parametrize("T,n", LC.LOSS_SHAPES)
def test_loss_bits_of_the_host_twin(T, n, use_clip, misalign):
    c = LC.loss_case(T, n)
    got, want = gpu_loss(c, use_clip, misalign), host_loss(c, use_clip)
    for name, g, w in zip(("d_log_prob", "d_value", "sums"), got, want):
        assert same_bits(g, w), (name, np.max(np.abs(g.astype(np.float64) - w)))
    again = gpu_loss(c, use_clip, misalign)
    assert all(same_bits(x, y) for x, y in zip(got, again))  # two identical calls, identical bits


@pytest.mark.parametrize("T,n", LC.LOSS_SHAPES)
def test_loss_first_pass_bits(T, n):
    c = LC.first_pass_case(T, n)
    got, want = gpu_loss(c, True), host_loss(c, True)
    assert all(same_bits(g, w) for g, w in zip(got, want))
    assert got[2][2] == 0.0 and got[2][3] == 0.0
    got2, want2 = gpu_loss(c, True, total=8.0 * T * n), host_loss(c, True, total=8.0 * T * n)
    assert all(same_bits(g, w) for g, w in zip(got2, want2))
    assert same_bits(got2[0], got[0] * np.float32(0.125))  # `total` only scales the seeds


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("count", LC.SQNORM_COUNTS)
def test_sqnorm_bits_of_the_host_twin(count, misalign):
    g = LC.sqnorm_case(count)
    gd = dev(g, misalign)
    a = ppo.grad_sqnorm(gd)
    b = ppo.grad_sqnorm(gd)
    torch.cuda.synchronize()
    want = np.float64(ppo.grad_sqnorm_host(g))
    assert same_bits(a.cpu().numpy()[0], want) and same_bits(b.cpu().numpy()[0], want)


def gpu_adamw(c, max_norm, misalign=False):
    p = dev(c["param"], misalign)
    m0 = np.zeros(LC.ADAM_COUNT, np.float32)
    v0 = np.zeros(LC.ADAM_COUNT, np.float32)
    m0[-LC.ADAM_TAIL:], v0[-LC.ADAM_TAIL:] = 3.0, 5.0
    m, v = dev(m0, misalign), dev(v0, misalign)
    sq = torch.zeros(2, dtype=torch.float64, device="cuda")
    out = []
    for i, (g, o) in enumerate(zip(c["grads"], c["other"])):
        gd = dev(g, misalign)
        ppo.grad_sqnorm(gd, out=sq[0:1])
        ppo.grad_sqnorm(dev(o), out=sq[1:2])
        ppo.adamw_step(p, gd, m, v, sq, 1 + i, LC.ADAM_LR, max_grad_norm=max_norm, weight_decay=LC.ADAM_WD,
                       frozen_tail=LC.ADAM_TAIL)
        torch.cuda.synchronize()
        out.append((p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()))
    return out


def host_adamw(c, max_norm):
    p = c["param"].copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    m[-LC.ADAM_TAIL:], v[-LC.ADAM_TAIL:] = 3.0, 5.0
    out = []
    for i, (g, o) in enumerate(zip(c["grads"], c["other"])):
        sq = np.array([ppo.grad_sqnorm_host(g), ppo.grad_sqnorm_host(o)])
        ppo.adamw_step_host(p, g, m, v, sq, 1 + i, LC.ADAM_LR, max_grad_norm=max_norm, weight_decay=LC.ADAM_WD,
                            frozen_tail=LC.ADAM_TAIL)
        out.append((p.copy(), m.copy(), v.copy()))
    return out


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("case", ["under", "over"])
def test_adamw_bits_of_the_host_twin(case, misalign):
    """param, m and v over three steps; count = 4099 is no multiple of 4 and frozen_tail = 20 ends the
    live range at 4079, inside a float4."""
    c = LC.adam_case()
    got, want = gpu_adamw(c, LC.ADAM_MAX_NORM[case], misalign), host_adamw(c, LC.ADAM_MAX_NORM[case])
    for s in range(LC.ADAM_STEPS):
        for name, g, w in zip(("param", "m", "v"), got[s], want[s]):
            assert same_bits(g, w), (s + 1, name, np.max(np.abs(g.astype(np.float64) - w)))
    live = LC.ADAM_COUNT - LC.ADAM_TAIL
    assert same_bits(got[-1][0][live:], c["param"][live:])
    assert np.all(got[-1][1][live:] == 3.0) and np.all(got[-1][2][live:] == 5.0)
    again = gpu_adamw(c, LC.ADAM_MAX_NORM[case], misalign)
    assert all(same_bits(x, y) for a, b in zip(got, again) for x, y in zip(a, b))


def test_argument_checks():
    """Refused calls return ZB_EARG and launch nothing: the outputs keep their fill."""
    from zbot_amd.engine import load_library

    L = load_library()
    T, n = 3, 37
    c = LC.loss_case(T, n)
    ins = [dev(c[k]) for k in LOSS_KEYS]
    d_lp, d_v = torch.full((T, n, NJ), 7.0, device="cuda"), torch.full((T, n), 7.0, device="cuda")
    part = torch.full((int(L.zb_ppo_loss_partials_words(T, n)),), 7.0, dtype=torch.float64, device="cuda")
    sums = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    assert L.zb_ppo_loss_partials_words(0, n) == 0 and L.zb_ppo_loss_partials_words(T, n) == 4
    fl = C.c_float

    def loss(ptrs=None, T_=T, n_=n, total=float(T * n), outs=None):
        ptrs = [x.data_ptr() for x in ins] if ptrs is None else ptrs
        outs = [d_lp.data_ptr(), d_v.data_ptr(), part.data_ptr(), sums.data_ptr()] if outs is None else outs
        return L.zb_ppo_loss(*ptrs, T_, n_, total, fl(LC.EPS), fl(LC.COEF), 1, fl(LC.L_CLIP), *outs, None)

    for i in range(6):
        p = [x.data_ptr() for x in ins]
        p[i] = None
        assert loss(ptrs=p) == -1
    for i in range(4):
        o = [d_lp.data_ptr(), d_v.data_ptr(), part.data_ptr(), sums.data_ptr()]
        o[i] = None
        assert loss(outs=o) == -1
    assert loss(T_=0) == -1 and loss(T_=-2) == -1 and loss(n_=0) == -1
    assert loss(total=0.0) == -1 and loss(total=-1.0) == -1

    g = dev(LC.sqnorm_case(4099))
    sq_part, sq = torch.full((2,), 7.0, dtype=torch.float64, device="cuda"), torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    assert L.zb_grad_sqnorm(None, g.numel(), sq_part.data_ptr(), sq.data_ptr(), None) == -1
    assert L.zb_grad_sqnorm(g.data_ptr(), g.numel(), None, sq.data_ptr(), None) == -1
    assert L.zb_grad_sqnorm(g.data_ptr(), g.numel(), sq_part.data_ptr(), None, None) == -1
    assert L.zb_grad_sqnorm(g.data_ptr(), 0, sq_part.data_ptr(), sq.data_ptr(), None) == -1

    a = LC.adam_case()
    p, m, v = dev(a["param"]), torch.zeros(LC.ADAM_COUNT, device="cuda"), torch.zeros(LC.ADAM_COUNT, device="cuda")
    gr = dev(a["grads"][0])

    def adam(ptrs=None, count=LC.ADAM_COUNT, tail=LC.ADAM_TAIL, k=2, step=1, sqp=sq.data_ptr()):
        ptrs = [p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr()] if ptrs is None else ptrs
        return L.zb_adamw_step(*ptrs, count, tail, sqp, k, fl(1.0), fl(1e-3), 0.9, 0.999, fl(1e-8), fl(0.0), step, None)

    for i in range(4):
        q = [p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr()]
        q[i] = None
        assert adam(ptrs=q) == -1
    assert adam(sqp=None) == -1 and adam(step=0) == -1 and adam(tail=LC.ADAM_COUNT + 1) == -1
    assert adam(k=0) == -1 and adam(count=0, tail=0) == -1
    torch.cuda.synchronize()
    assert torch.all(d_lp == 7) and torch.all(d_v == 7) and torch.all(part == 7) and torch.all(sums == 7)
    assert torch.all(sq_part == 7) and torch.all(sq == 7)
    assert np.array_equal(p.cpu().numpy(), a["param"]) and not m.any() and not v.any()
    with pytest.raises(ppo.ZbError):
        ppo.ppo_loss_grad(*(x.cpu() for x in ins))
    with pytest.raises(ppo.ZbError):
        ppo.adamw_step(p, gr, m[:-1], v, sq, 1, 1e-3)


# ---- HipPpoLearner ----

@pytest.fixture(scope="module")
def rollout(pol, cmodel):
    """A real small rollout, as test_gpu_policy_train.py::test_rollout_ties_to_learner builds one, at
    n = 33, T = 4: minibatches of 16 envs are 16, 16 and 1."""
    from zbot_amd import default_config
    from zbot_amd.engine import HipEngine

    T, n = 4, 33
    eng = HipEngine(cmodel, default_config(solver="newton"), n, seed=2)
    pa, pc = init_params(ACTOR, seed=8), init_params(CRITIC, seed=9)
    actor, critic = pol.GruPolicy(ACTOR, pa), pol.GruPolicy(CRITIC, pc)
    ro = pol.PolicyRollout(eng, actor, seed=5)
    ro.reset()
    carry0 = ro.carry.clone()
    ccarry = critic.initial_carry(n)
    ccarry0 = ccarry.clone()
    out = ro.run(T, record_critic=True, critic=critic, critic_carry=ccarry)
    reset = torch.zeros(T, n, dtype=torch.uint8, device="cuda")
    reset[1:] = out["done"][:T - 1]
    inputs = ppo.compute_ppo_inputs(out["value"], out["reward"], out["done"], out["success"],
                                    bootstrap=out["value_next"])
    torch.cuda.synchronize()
    out = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    return dict(T=T, n=n, out=out, inputs=inputs, carry0=carry0, ccarry0=ccarry0, reset=reset, pa=pa, pc=pc)


def fresh_nets(pol, r):
    return pol.GruPolicy(ACTOR, r["pa"]), pol.GruPolicy(CRITIC, r["pc"])


def by_hand(pol, r, num_passes, batch_size, lr, max_norm, wd):
    """HipPpoLearner.update's sequence of library calls, written out."""
    actor, critic = fresh_nets(pol, r)
    T, n, out, inp = r["T"], r["n"], r["out"], r["inputs"]
    st = {}
    for net, h in (("a", actor), ("c", critic)):
        p = h.params_tensor()
        st[net] = [p, torch.zeros_like(p), torch.zeros_like(p)]
    sq = torch.zeros(2, dtype=torch.float64, device="cuda")
    step, all_sums = 0, []
    for _ in range(num_passes):
        for lo in range(0, n, batch_size):
            hi = min(n, lo + batch_size)
            cut = lambda x: x[:T, lo:hi].contiguous()  # noqa: E731
            obs_a, acts, obs_c, rs = cut(out["obs_actor"]), cut(out["actions"]), cut(out["obs_critic"]), cut(r["reset"])
            ca, cc = r["carry0"][lo:hi].contiguous(), r["ccarry0"][lo:hi].contiguous()
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
    return st, all_sums, actor, critic


def run_update(learner, r, actor, critic, **kw):
    return learner.update(r["out"], r["inputs"], actor, critic, r["carry0"], r["ccarry0"], reset=r["reset"], **kw)


def test_update_equals_the_calls_by_hand(pol, rollout):
    from zbot_amd.learner import HipPpoLearner, TrainablePolicy

    r = rollout
    lr, mx, wd = 3e-4, 1e-3, 1e-5  # a maximum the gradient norm exceeds, so that the clip scales (checked below)
    st, sums_hand, _, _ = by_hand(pol, r, 2, 16, lr, mx, wd)
    actor, critic = fresh_nets(pol, r)
    ln = HipPpoLearner(learning_rate=lr, max_grad_norm=mx, weight_decay=wd)
    sums = run_update(ln, r, actor, critic, num_passes=2, batch_size=16)
    torch.cuda.synchronize()
    assert len(sums) == 6 and ln.step == 6  # 2 passes x (16 + 16 + 1 envs)
    for a, b in zip(sums, sums_hand):
        assert torch.equal(a[:4], b)
    assert [float(s[4]) for s in sums] == [64.0, 64.0, 4.0] * 2 and all(float(s[5]) == 0.5 for s in sums)
    sd = ln.state_dict()
    for net, key in (("actor", "a"), ("critic", "c")):
        for name, x in zip(("params", "m", "v"), st[key]):
            assert torch.equal(sd[net][name], x), (net, name)
    assert torch.equal(actor.params_tensor(), sd["actor"]["params"])  # the handle runs the new weights
    assert torch.equal(sd["actor"]["params"][-NJ:], torch.from_numpy(r["pa"][-NJ:]).cuda())
    assert not sd["actor"]["m"][-NJ:].any() and not sd["actor"]["v"][-NJ:].any()
    assert not torch.equal(sd["actor"]["params"], torch.from_numpy(r["pa"]).cuda())
    # the clip did scale: the first step's joint norm exceeds the maximum
    # (checked on the by-hand gradients' norms through a second, unclipped run)
    st0, _, _, _ = by_hand(pol, r, 1, 16, lr, 0.0, wd)
    st1, _, _, _ = by_hand(pol, r, 1, 16, lr, mx, wd)
    assert not torch.equal(st0["a"][1], st1["a"][1])
    # TrainablePolicy wrappers are taken too and follow their handles
    a2, c2 = fresh_nets(pol, r)
    ta, tc = TrainablePolicy(a2), TrainablePolicy(c2)
    ln2 = HipPpoLearner(learning_rate=lr, max_grad_norm=mx, weight_decay=wd)
    run_update(ln2, r, ta, tc, num_passes=2, batch_size=16)
    torch.cuda.synchronize()
    assert torch.equal(ta.param.detach(), sd["actor"]["params"]) and torch.equal(tc.param.detach(), sd["critic"]["params"])
    assert torch.equal(a2.params_tensor(), sd["actor"]["params"])
    first = HipPpoLearner.loss(sums[0])
    assert first.dtype == torch.float64 and torch.isfinite(first)


WEIGHT_SCALE = 2.0


def compare_case(T=4, n=33, seed=21):
    """The minibatch of the comparison with PpoLearner: synthetic observations as
    test_gpu_policy_train.py's cases, and a second-pass flavour: the old log-probs and values are the
    networks' own outputs plus noise (dlp, dv), so ratios differ from 1 and some rows clip. The
    weights are WEIGHT_SCALE x their initialisation: at the initialisation's scale the gradient
    shrinks by about half per GRU layer on its way down, and only 40 % (actor) / 22 % (critic) of the
    elements reach 1e-3 of their network's largest. Checked with the fp64 torch gradient of ppo_loss
    through tests/policy_torch.py on the CPU: at this fixture 86 % (actor) and 69 % (critic) do."""
    rng = np.random.default_rng(seed)
    f = lambda x: x.astype(np.float32)  # noqa: E731
    reset = np.zeros((T, n), np.uint8)
    reset[0, 0::3] = 1
    reset[2, 1::3] = 1
    Pa, Pc = init_params(ACTOR, seed=3), init_params(CRITIC, seed=4)
    Pa[:-NJ] *= WEIGHT_SCALE
    Pc *= WEIGHT_SCALE
    return dict(T=T, n=n, Pa=Pa, Pc=Pc,
                obs_a=f(rng.normal(size=(T, n, 50))), obs_c=f(rng.normal(size=(T, n, 484))),
                carry_a=f(0.5 * rng.normal(size=(n, D, H))), carry_c=f(0.5 * rng.normal(size=(n, D, H))),
                actions=f(0.4 * rng.normal(size=(T, n, NJ))), reset=reset, adv=f(rng.normal(size=(T, n))),
                dlp=f(0.01 * rng.normal(size=(T, n, NJ))), dv=f(0.1 * rng.normal(size=(T, n))),
                dtgt=f(0.5 * rng.normal(size=(T, n))))


def test_one_step_against_the_torch_learner(pol):
    from zbot_amd.learner import HipPpoLearner, PpoLearner, TrainablePolicy
    from zbot_amd.ppo import PPOInputs

    c = compare_case()
    T, n = c["T"], c["n"]
    lr = 3e-4
    d = lambda k: torch.from_numpy(c[k]).cuda()  # noqa: E731
    probe_a, probe_c = pol.GruPolicy(ACTOR, c["Pa"]), pol.GruPolicy(CRITIC, c["Pc"])
    lp, sa = probe_a.actor_train(d("obs_a"), d("actions"), d("carry_a"), d("reset"))
    v, sc = probe_c.critic_train(d("obs_c"), d("carry_c"), d("reset"))
    ro = dict(obs_actor=d("obs_a"), actions=d("actions"), obs_critic=d("obs_c"), log_prob=lp + d("dlp"), value=v + d("dv"))
    inputs = PPOInputs(advantages_t=d("adv"), value_targets_t=v + d("dtgt"), gae_t=None, returns_t=None)
    # the gradient that decides which elements are compared: the library's own
    d_lp, d_v, _ = ppo.ppo_loss_grad(lp, ro["log_prob"], inputs.advantages_t, v, ro["value"], inputs.value_targets_t)
    grads = dict(actor=probe_a.actor_backward(d("obs_a"), d("actions"), d("carry_a"), d("reset"), d_lp, sa).clone(),
                 critic=probe_c.critic_backward(d("obs_c"), d("carry_c"), d("reset"), d_v, sc).clone())

    def one_step(cls, wrap):
        a, k = pol.GruPolicy(ACTOR, c["Pa"]), pol.GruPolicy(CRITIC, c["Pc"])
        args = (wrap(a), wrap(k))
        cls(learning_rate=lr).update(ro, inputs, *args, d("carry_a"), d("carry_c"), reset=d("reset"), num_passes=1,
                                     batch_size=n)
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
        print(f"VSTORCH {net} compared share={share:.3f} max |dp_hip - dp_torch| = {worst:.3e} = {worst / lr:.2e} lr; "
              f"max |dp| = {dh.abs().max().item():.3e}")
        assert share >= 0.5
        assert worst <= 0.01 * lr
        assert dh.abs().max().item() > 0.5 * lr  # the step did move them
    assert torch.equal(hip["actor"][-NJ:], ref["actor"][-NJ:])  # the constants stay with both


def test_state_dict_round_trip(pol, rollout):
    from zbot_amd.learner import HipPpoLearner

    r = rollout
    kw = dict(num_passes=1, batch_size=16)
    a1, c1 = fresh_nets(pol, r)
    l1 = HipPpoLearner()
    run_update(l1, r, a1, c1, **kw)
    run_update(l1, r, a1, c1, **kw)
    sd = l1.state_dict()
    saved = {net: {k: t.clone() for k, t in sd[net].items()} for net in ("actor", "critic")}
    run_update(l1, r, a1, c1, **kw)
    a2, c2 = fresh_nets(pol, r)  # a new process would create its handles from any weights
    l2 = HipPpoLearner()
    l2.load_state_dict(sd)
    run_update(l2, r, a2, c2, **kw)
    torch.cuda.synchronize()
    s1, s2 = l1.state_dict(), l2.state_dict()
    assert s1["step"] == s2["step"] == 9
    for net in ("actor", "critic"):
        for k in ("params", "m", "v"):
            assert torch.equal(s1[net][k], s2[net][k]), (net, k)
            assert torch.equal(sd[net][k], saved[net][k])  # a state dict is a copy: later updates leave it alone
            assert not torch.equal(s1[net][k], saved[net][k])
    assert torch.equal(a2.params_tensor(), s1["actor"]["params"])


def test_it_learns(pol, rollout):
    """20 updates on a fixed rollout lower loss(sums)."""
    from zbot_amd.learner import HipPpoLearner

    r = rollout
    actor, critic = fresh_nets(pol, r)
    ln = HipPpoLearner(learning_rate=1e-3)
    losses = []
    for _ in range(20):
        sums = run_update(ln, r, actor, critic, num_passes=1, batch_size=r["n"])
        losses.append(HipPpoLearner.loss(sums[0]))
    losses = [x.item() for x in losses]
    assert losses[-1] < losses[0], losses
    assert torch.isfinite(actor.params_tensor()).all() and torch.isfinite(critic.params_tensor()).all()
