"""Training the GRU actor / critic on the GPU: the activation-saving forward, the backward pass
(include/zbot_policy.h "Training", csrc/zb_policy_train.hip) and zbot_amd.learner over them.

Forward bar: the bits of the inference entry points. Gradient bar: per parameter tensor,
err(g) = max|g - g64| / max|g64| against the fp64 torch restatement's autograd gradient
(tests/policy_torch.py, pinned to the oracle by tests/test_policy_torch_ref.py), held to
C_BOUND x the error the same restatement makes when it runs in fp32 on the CPU: the GPU is another
fp32 evaluation of the same sums in another order. C_BOUND is the smallest power of two that is at
least twice the worst ratio measured on the MI355X (DESIGN.md §4m has the table).

Shapes: T = 4, n = 33 (two workgroups, the second with one live env; a persistent loop with
carried dh; K = T n = 132 is no multiple of 16) with resets at t = 0 for some envs, at t = 2 for
others and none for the rest; and T = 1, n = 1. The gradient tests add the sizes at which the weight
gradient takes another path: K = 600 rows (two split-K chunks) and K = 16 500 (32 chunks of 528 rows,
each summed as a 512-row and a 16-row sub-chain).
"""

import numpy as np
import pytest
import torch

import policy_torch as PT
from zbot_amd.policy import ACTOR, CRITIC, EVAL, MODE, init_params, param_count

pytestmark = pytest.mark.gpu
D, H, NJ = 5, 128, 20
C_BOUND = 8.0  # err_gpu <= C_BOUND * err_ref32 per tensor; worst measured ratio 3.75 (critic rnn1.weight_ih)
STD_BIAS_SCALE = 12.0  # spreads the raw std outputs over both sides of the max_std clip


@pytest.fixture(scope="module")
def pol():
    from zbot_amd import policy as P

    assert torch.cuda.is_available()
    return P


def actor_params(seed=3):
    """Actor parameters whose std block of output_proj.bias is scaled so both branches of the
    max_std clip (train.py:961) are taken."""
    P = init_params(ACTOR, seed=seed)
    off = param_count(ACTOR) - NJ - 300  # output_proj.bias
    P[off + 100:off + 200] *= STD_BIAS_SCALE
    return P


def make_case(kind, T, n, seed):
    rng = np.random.default_rng(seed)
    I = 50 if kind == ACTOR else 484
    c = dict(kind=kind, T=T, n=n, P=actor_params() if kind == ACTOR else init_params(CRITIC, seed=4))
    c["obs"] = rng.normal(size=(T, n, I)).astype(np.float32)
    c["carry0"] = (0.5 * rng.normal(size=(n, D, H))).astype(np.float32)
    reset = np.zeros((T, n), np.uint8)
    if T >= 3:
        reset[0, 0::3] = 1   # envs 0, 3, ...: at t = 0
        reset[2, 1::3] = 1   # envs 1, 4, ...: at t = 2 (env 31 among them); the rest: none
    c["reset"] = reset
    c["actions"] = (0.4 * rng.normal(size=(T, n, NJ))).astype(np.float32)
    c["dout"] = rng.normal(size=(T, n, NJ) if kind == ACTOR else (T, n)).astype(np.float32)
    return c


def cpu_grad(c, dtype):
    """Autograd gradient of sum(dout * output) through the torch restatement, on the CPU."""
    t = lambda x: torch.from_numpy(x).to(dtype)  # noqa: E731
    P = t(c["P"]).requires_grad_()
    r = torch.from_numpy(c["reset"])
    if c["kind"] == ACTOR:
        out = PT.actor_log_prob(P, t(c["obs"]), t(c["carry0"]), r, t(c["actions"]))
    else:
        out = PT.critic_value(P, t(c["obs"]), t(c["carry0"]), r)
    (g,) = torch.autograd.grad((out * t(c["dout"])).sum(), P)
    return g.double().numpy()


_CASES = {}


def case(kind, T, n):
    """The inputs and CPU references of one (kind, T, n), computed once and left unchanged."""
    key = (kind, T, n)
    if key not in _CASES:
        c = make_case(kind, T, n, seed=100 * kind + 10 * T + n)
        c["g64"] = cpu_grad(c, torch.float64)
        c["g32"] = cpu_grad(c, torch.float32)
        _CASES[key] = c
    return _CASES[key]


def gpu_run(pol, c, P=None, obs=None, dout=None, net=None):
    """Training forward + backward on the GPU -> (output, grad, carry0 after, net)."""
    kind = c["kind"]
    net = net or pol.GruPolicy(kind, c["P"] if P is None else P)
    d = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    o, c0, r = d(c["obs"] if obs is None else obs), d(c["carry0"]), d(c["reset"])
    do = d(c["dout"] if dout is None else dout)
    if kind == ACTOR:
        a = d(c["actions"])
        out, scratch = net.actor_train(o, a, c0, r)
        g = net.actor_backward(o, a, c0, r, do, scratch)
    else:
        out, scratch = net.critic_train(o, c0, r)
        g = net.critic_backward(o, c0, r, do, scratch)
    torch.cuda.synchronize()
    return out.cpu().numpy(), g.cpu().numpy(), c0.cpu().numpy(), net


SHAPES = [(4, 33), (1, 1)]


@pytest.mark.parametrize("T,n", SHAPES)
@pytest.mark.parametrize("kind", [ACTOR, CRITIC])
def test_forward_identity(pol, kind, T, n):
    """The training forward returns the bits of the inference entry points and leaves carry0 alone."""
    c = case(kind, T, n)
    out, _, c0_after, net = gpu_run(pol, c)
    d = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    carry = d(c["carry0"])
    if kind == ACTOR:
        _, ref = net.actor(d(c["obs"]), carry, reset=d(c["reset"]), mode=EVAL, actions=d(c["actions"]), log_prob=True)
    else:
        ref = net.critic(d(c["obs"]), carry, reset=d(c["reset"]))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out, ref.cpu().numpy())
    np.testing.assert_array_equal(c0_after, c["carry0"])
    assert not np.array_equal(carry.cpu().numpy(), c["carry0"])  # inference did advance its carry


def tensor_errors(c, g):
    """{tensor name: (err_gpu, err_ref32)} with err = max|g - g64| / max|g64| over the tensor."""
    actor = c["kind"] == ACTOR
    out, i = {}, 0
    for name, shp in zip(PT.names(actor), PT.shapes(actor)):
        k = int(np.prod(shp))
        ref = c["g64"][i:i + k]
        scale = np.max(np.abs(ref))
        assert scale > 0, f"{name}: the reference gradient is all zero"
        out[name] = (np.max(np.abs(g[i:i + k] - ref)) / scale, np.max(np.abs(c["g32"][i:i + k] - ref)) / scale)
        i += k
    return out, i


# + two split-K chunks (actor, K = 600); 32 chunks of two sub-chains each (critic, K = 16 500)
GRAD_CASES = [(k, T, n) for k in (ACTOR, CRITIC) for T, n in SHAPES] + [(ACTOR, 4, 150), (CRITIC, 3, 5500)]


@pytest.mark.parametrize("kind,T,n", GRAD_CASES)
def test_gradient_parity(pol, kind, T, n):
    c = case(kind, T, n)
    _, g, _, _ = gpu_run(pol, c)
    assert np.isfinite(g).all()
    errs, used = tensor_errors(c, g.astype(np.float64))
    bad = []
    for name, (eg, er) in errs.items():
        print(f"GRADERR kind={kind} T={T} n={n} {name} err_gpu={eg:.3e} err_ref32={er:.3e} ratio={eg / max(er, 1e-300):.2f}")
        if not eg <= C_BOUND * er:
            bad.append((name, eg, er))
    assert not bad, bad
    if kind == ACTOR:
        assert used == g.size - NJ
        assert np.all(g[used:] == 0.0)  # JOINT_BIASES are constants
        assert np.all(c["g64"][used:] != 0.0)  # ... that the loss does depend on


def test_std_clip_fixture_takes_both_branches():
    """At least a tenth of the (t, env, joint, mixture) std entries clipped at max_std and at
    least a tenth not, on the CPU helper: test_gradient_parity[actor] covers both gradients."""
    c = case(ACTOR, 4, 33)
    t = lambda x: torch.from_numpy(x).double()  # noqa: E731
    with torch.no_grad():
        P = t(c["P"])
        _, _, _, unclipped = PT.head(P, PT.trunk(P, True, t(c["obs"]), t(c["carry0"]), torch.from_numpy(c["reset"])))
    frac = unclipped.double().mean().item()
    assert 0.1 <= frac <= 0.9, frac


def test_reset_cuts_the_gradient(pol):
    """Upstream only at t = 3 of an env reset at t = 2: its observations before the reset cannot
    matter, bit for bit."""
    c = case(ACTOR, 4, 33)
    e = 31
    assert c["reset"][2, e] == 1 and c["reset"][3, e] == 0
    dout = np.zeros_like(c["dout"])
    dout[3, e] = c["dout"][3, e]
    obs2 = c["obs"].copy()
    obs2[0:2, e] = np.random.default_rng(5).normal(size=(2, 50)).astype(np.float32)
    _, g1, _, net = gpu_run(pol, c, dout=dout)
    _, g2, _, _ = gpu_run(pol, c, dout=dout, obs=obs2, net=net)
    assert np.any(g1 != 0)
    np.testing.assert_array_equal(g1, g2)
    obs3 = c["obs"].copy()
    obs3[2, e] += 1.0  # after the reset it does matter
    _, g3, _, _ = gpu_run(pol, c, dout=dout, obs=obs3, net=net)
    assert not np.array_equal(g1, g3)


@pytest.mark.parametrize("kind,T,n", [(ACTOR, 4, 33), (CRITIC, 4, 33), (CRITIC, 3, 5500)])
def test_backward_is_deterministic(pol, kind, T, n):
    c = case(kind, T, n)
    _, g1, _, net = gpu_run(pol, c)
    _, g2, _, _ = gpu_run(pol, c, net=net)
    np.testing.assert_array_equal(g1, g2)


def test_argument_checks(pol):
    """An undersized scratch, a handle of the other kind and a wrong parameter count are errors
    returned before anything is launched."""
    T, n = 2, 3
    actor, critic = pol.GruPolicy(ACTOR), pol.GruPolicy(CRITIC)
    L = actor.L
    words = actor.train_scratch_words(T, n)
    assert words > 0 and L.zb_policy_train_scratch_words(7, T, n) == 0
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    obs, acts, lp, c0 = z(T, n, 50), z(T, n, NJ), z(T, n, NJ), z(n, D, H)
    scratch, grad = z(words), torch.full((param_count(ACTOR),), 7.0, device="cuda")

    def fwd(h, sw):
        return L.zb_policy_actor_train(h, obs.data_ptr(), T, n, c0.data_ptr(), None, acts.data_ptr(), lp.data_ptr(),
                                       scratch.data_ptr(), sw, None)

    def bwd(h, sw):
        return L.zb_policy_actor_backward(h, obs.data_ptr(), T, n, c0.data_ptr(), None, acts.data_ptr(), lp.data_ptr(),
                                          scratch.data_ptr(), sw, grad.data_ptr(), None)

    assert fwd(actor.h, words) == 0
    assert fwd(actor.h, words - 1) != 0 and bwd(actor.h, words - 1) != 0
    assert fwd(critic.h, words) != 0 and bwd(critic.h, words) != 0
    p = z(param_count(ACTOR) + 1)
    assert L.zb_policy_set_params(actor.h, p.data_ptr(), param_count(ACTOR) + 1, None) != 0
    assert L.zb_policy_set_params(actor.h, p.data_ptr(), param_count(ACTOR) - 1, None) != 0
    torch.cuda.synchronize()
    assert torch.all(grad == 7.0)  # no refused call wrote the gradient
    with pytest.raises(pol.ZbError):
        actor.set_params(p)
    with pytest.raises(pol.ZbError):
        critic.actor_train(obs, acts, c0)


@pytest.mark.parametrize("kind", [ACTOR, CRITIC])
def test_set_params_round_trip(pol, kind):
    """After set_params(p2) a handle computes what a fresh handle created from p2 computes, in
    inference and in the gradient (the device repack equals the host's, transposed packs included)."""
    c = case(kind, 4, 33)
    p2 = actor_params(seed=11) if kind == ACTOR else init_params(CRITIC, seed=12)
    moved = pol.GruPolicy(kind, c["P"])
    moved.set_params(torch.from_numpy(p2).cuda())
    fresh = pol.GruPolicy(kind, p2)
    assert torch.equal(moved.params_tensor(), fresh.params_tensor())
    d = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    outs = []
    for net in (moved, fresh):
        carry = d(c["carry0"])
        if kind == ACTOR:
            a, lp = net.actor(d(c["obs"]), carry, reset=d(c["reset"]), mode=MODE, log_prob=True)
            outs.append((a.cpu(), lp.cpu(), carry.cpu()))
        else:
            outs.append((net.critic(d(c["obs"]), carry, reset=d(c["reset"])).cpu(), carry.cpu()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    _, g_moved, _, _ = gpu_run(pol, c, net=moved)
    _, g_fresh, _, _ = gpu_run(pol, c, net=fresh)
    np.testing.assert_array_equal(g_moved, g_fresh)


@pytest.mark.parametrize("kind", [ACTOR, CRITIC])
def test_it_learns(pol, kind):
    """20 AdamW steps through TrainablePolicy lower the loss on a fixed batch."""
    from zbot_amd.learner import TrainablePolicy

    c = case(kind, 4, 33)
    d = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    tp = TrainablePolicy(pol.GruPolicy(kind, c["P"]))
    opt = torch.optim.AdamW(tp.parameters(), lr=1e-3)
    obs, c0, r, acts = d(c["obs"]), d(c["carry0"]), d(c["reset"]), d(c["actions"])
    targets = d(c["dout"]) if kind == CRITIC else None
    losses = []
    for _ in range(20):
        if kind == ACTOR:
            loss = -tp.log_prob(obs, acts, c0, r).sum(-1).mean()
        else:
            loss = torch.nn.functional.mse_loss(tp.value(obs, c0, r), targets)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    assert torch.isfinite(tp.param).all()
    assert obs.grad is None and c0.grad is None


def test_rollout_ties_to_learner(pol, cmodel):
    """The learner reproduces the rollout's in-loop log-probs bit for bit (the first-pass PPO ratio
    is exactly 1), and one PpoLearner.update changes the weights the rollout handle runs."""
    from zbot_amd import default_config, ppo
    from zbot_amd.engine import HipEngine
    from zbot_amd.learner import PpoLearner, TrainablePolicy

    T, n = 4, 64
    eng = HipEngine(cmodel, default_config(solver="newton"), n, seed=2)
    actor = pol.GruPolicy(ACTOR, init_params(ACTOR, seed=8))
    critic = pol.GruPolicy(CRITIC, init_params(CRITIC, seed=9))
    ro = pol.PolicyRollout(eng, actor, seed=5)
    ro.reset()
    carry0 = ro.carry.clone()
    ccarry = critic.initial_carry(n)
    ccarry0 = ccarry.clone()
    out = ro.run(T, record_critic=True, critic=critic, critic_carry=ccarry)
    reset = torch.zeros(T, n, dtype=torch.uint8, device="cuda")  # row 0: a fresh trajectory resets nothing
    reset[1:] = out["done"][:T - 1]
    ta, tc = TrainablePolicy(actor), TrainablePolicy(critic)
    lp = ta.log_prob(out["obs_actor"][:T], out["actions"], carry0, reset)
    v = tc.value(out["obs_critic"], ccarry0, reset)
    torch.cuda.synchronize()
    assert torch.equal(lp.detach(), out["log_prob"])
    assert torch.equal(v.detach(), out["value"])
    ratio = (lp.detach().sum(-1) - out["log_prob"].sum(-1)).exp()
    assert torch.all(ratio == 1.0)

    inputs = ppo.compute_ppo_inputs(out["value"], out["reward"], out["done"], out["success"],
                                    bootstrap=out["value_next"])
    before_a, before_c = ta.param.detach().clone(), tc.param.detach().clone()
    probe_obs, probe_carry = out["obs_actor"][0].clone(), carry0.clone()
    acts_before, _ = actor.actor(probe_obs, probe_carry.clone(), mode=MODE)
    losses = PpoLearner().update(out, inputs, ta, tc, carry0, ccarry0, reset=reset, num_passes=1, batch_size=32)
    assert len(losses) == 2 and all(torch.isfinite(x) for x in losses)
    assert torch.isfinite(ta.param).all() and torch.isfinite(tc.param).all()
    assert not torch.equal(ta.param.detach(), before_a) and not torch.equal(tc.param.detach(), before_c)
    assert torch.equal(ta.param.detach()[-NJ:], before_a[-NJ:])  # the mean offsets stay constants
    assert torch.equal(actor.params_tensor(), ta.param.detach())
    acts_after, _ = actor.actor(probe_obs, probe_carry.clone(), mode=MODE)
    torch.cuda.synchronize()
    assert not torch.equal(acts_before, acts_after)
