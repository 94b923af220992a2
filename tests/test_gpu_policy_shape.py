"""Shaped policy handles on the GPU (include/zbot_policy.h "Network shape"): GRU depth and
mixture count as runtime values of the shape-generic kernels.

Forward bar: the bits of the host twins zb_policy_actor_host / zb_policy_critic_host
(tests/test_policy_shape_host.py pins those to the oracle at the default shape and to the fp64 helper
elsewhere). At the default shape the generic kernels also return the bits of the specialised ones, the
gradient included (the reduction order is the header's at every shape). Gradient bar at the other shapes:
tests/test_gpu_policy_train.py's, per parameter tensor err_gpu <= C * err_ref32 against the fp64 autograd
of tests/policy_shape_torch.py, C = 8 as there unless a shape's worst measured ratio exceeds 4 (GRADERR
lines; DESIGN.md §4r has the table).

Shapes (depth, mixtures): (1, 1) no next-layer prefetch and 60 outputs in 4 tiles for 8 waves; (2, 3) 180
outputs with a partial last tile; (8, 8) both maxima, 480 outputs in exactly 30 tiles; (5, 5) with the generic
flag. Sizes as the existing tests chose them: n = 1; n = 33 (two workgroups, the second with one env); T = 3
for the persistent form; K = 4 x 150 for two split-K chunks.
"""

import io

import numpy as np
import pytest
import torch

import policy_shape_torch as PS
from zbot_amd import policy as P
from zbot_amd.engine import ZbError
from zbot_amd.policy import ACTOR, CRITIC, EVAL, MODE, SAMPLE, PolicyShape

pytestmark = pytest.mark.gpu
H, NJ = 128, 20
SHAPES = [(1, 1, False), (2, 3, False), (8, 8, False), (5, 5, True)]  # depth, mixtures, generic flag
STD_BIAS_SCALE = 12.0  # spreads the raw std outputs over both sides of the max_std clip
# err_gpu <= C * err_ref32 per tensor, by shape; 8 is tests/test_gpu_policy_train.py's (worst ratio 3.75 there)
C_BOUND = {(1, 1): 8.0, (2, 3): 8.0, (8, 8): 8.0}


def dev(x):
    return torch.from_numpy(x).cuda()


def params(kind, depth, mix, seed):
    sh = PolicyShape(depth, mix)
    prm = P.init_params(kind, seed=seed, shape=sh)
    if kind == ACTOR:
        off = prm.size - NJ - 60 * mix  # output_proj.bias: its std block
        prm[off + 20 * mix:off + 40 * mix] *= STD_BIAS_SCALE
    return sh, prm


def inputs(kind, T, n, depth, seed):
    rng = np.random.default_rng(seed)
    obs = rng.normal(size=(T, n, 50 if kind == ACTOR else 484)).astype(np.float32)
    carry = (0.5 * rng.normal(size=(n, depth, H))).astype(np.float32)
    reset = (rng.random((T, n)) < 0.2).astype(np.uint8)
    acts = (0.4 * rng.normal(size=(T, n, NJ))).astype(np.float32)
    return obs, carry, reset, acts


def persist_modes(T):
    return (True, False) if T > 1 else (True,)


@pytest.mark.parametrize("depth,mix,generic", SHAPES)
@pytest.mark.parametrize("n,T,mode", [(1, 1, SAMPLE), (33, 3, SAMPLE), (70, 2, EVAL), (33, 3, MODE)])
def test_actor_forward_bits(depth, mix, generic, n, T, mode):
    sh, prm = params(ACTOR, depth, mix, seed=3)
    obs, carry, reset, acts = inputs(ACTOR, T, n, depth, seed=10 * n + T + depth)
    kw = dict(mode=mode, seed=9, env_offset=3)
    a_h, lp_h, c_h = P.actor_host(prm, obs, carry, reset=reset, step0=5, log_prob=True, shape=sh,
                                  actions=acts if mode == EVAL else None, **kw)
    net = P.GruPolicy(ACTOR, prm, shape=sh, generic=generic)
    assert net.shape == sh
    for persistent in persist_modes(T):
        net.set_persistent(persistent)
        c = dev(carry)
        a, lp = net.actor(dev(obs), c, reset=dev(reset), step=5, log_prob=True,
                          actions=dev(acts) if mode == EVAL else None, **kw)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(a.cpu().numpy(), a_h)
        np.testing.assert_array_equal(lp.cpu().numpy(), lp_h)
        np.testing.assert_array_equal(c.cpu().numpy(), c_h)


@pytest.mark.parametrize("depth,mix,generic", SHAPES)
@pytest.mark.parametrize("n,T", [(5, 2), (33, 3)])
def test_critic_forward_bits(depth, mix, generic, n, T):
    sh, prm = params(CRITIC, depth, mix, seed=4)
    obs, carry, reset, _ = inputs(CRITIC, T, n, depth, seed=10 * n + T + depth)
    v_h, c_h = P.critic_host(prm, obs, carry, reset=reset, shape=sh)
    net = P.GruPolicy(CRITIC, prm, shape=sh, generic=generic)
    for persistent in persist_modes(T):
        net.set_persistent(persistent)
        c = dev(carry)
        v = net.critic(dev(obs), c, reset=dev(reset))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(v.cpu().numpy(), v_h)
        np.testing.assert_array_equal(c.cpu().numpy(), c_h)


def train_run(net, obs, carry, reset, acts, dout):
    """Training forward + backward -> (output, grad, carry0 afterwards)."""
    o, c0, r, do = dev(obs), dev(carry), dev(reset), dev(dout)
    if net.kind == ACTOR:
        a = dev(acts)
        out, scratch = net.actor_train(o, a, c0, r)
        g = net.actor_backward(o, a, c0, r, do, scratch)
    else:
        out, scratch = net.critic_train(o, c0, r)
        g = net.critic_backward(o, c0, r, do, scratch)
    torch.cuda.synchronize()
    return out.cpu(), g.cpu(), c0.cpu().numpy()


def dout_of(kind, T, n, seed=77):
    return np.random.default_rng(seed).normal(size=(T, n, NJ) if kind == ACTOR else (T, n)).astype(np.float32)


@pytest.mark.parametrize("kind", [ACTOR, CRITIC])
def test_generic_equals_specialised(kind):
    """A (5, 5) handle with generic=True and a plain default handle, same parameters: the same bits for
    inference, the training forward and the full gradient (4 x 33, and 4 x 150: two split-K chunks)."""
    sh, prm = params(kind, 5, 5, seed=6)
    gen, plain = P.GruPolicy(kind, prm, shape=sh, generic=True), P.GruPolicy(kind, prm)
    assert gen.train_scratch_words(4, 33) > plain.train_scratch_words(4, 33)  # the plane the generic bptt adds
    for n in (33, 150):
        obs, carry, reset, acts = inputs(kind, 4, n, 5, seed=n)
        res = []
        for net in (gen, plain):
            c = dev(carry)
            if kind == ACTOR:
                a, lp = net.actor(dev(obs), c, reset=dev(reset), mode=SAMPLE, seed=2, log_prob=True)
                inf = (a.cpu(), lp.cpu(), c.cpu())
            else:
                inf = (net.critic(dev(obs), c, reset=dev(reset)).cpu(), c.cpu())
            res.append(inf + train_run(net, obs, carry, reset, acts, dout_of(kind, 4, n))[:2])
        for x, y in zip(*res):
            assert torch.equal(x, y)
        assert res[0][-1].abs().max() > 0


@pytest.mark.parametrize("depth,mix", [(1, 1), (2, 3), (8, 8)])
@pytest.mark.parametrize("kind", [ACTOR, CRITIC])
def test_training_forward_identity(kind, depth, mix):
    """actor_train log-probs are actor(EVAL)'s bits, critic_train values are critic's, carry0 is left alone."""
    T, n = 4, 33
    sh, prm = params(kind, depth, mix, seed=3)
    obs, carry, reset, acts = inputs(kind, T, n, depth, seed=5)
    net = P.GruPolicy(kind, prm, shape=sh)
    out, _, c0 = train_run(net, obs, carry, reset, acts, dout_of(kind, T, n))
    c = dev(carry)
    if kind == ACTOR:
        _, ref = net.actor(dev(obs), c, reset=dev(reset), mode=EVAL, actions=dev(acts), log_prob=True)
    else:
        ref = net.critic(dev(obs), c, reset=dev(reset))
    torch.cuda.synchronize()
    assert torch.equal(out, ref.cpu())
    np.testing.assert_array_equal(c0, carry)


_GRAD = {}


def grad_case(kind, depth, mix, T, n):
    """Inputs and the CPU fp64 / fp32 autograd gradients of one case, computed once and left unchanged."""
    key = (kind, depth, mix, T, n)
    if key not in _GRAD:
        sh, prm = params(kind, depth, mix, seed=3)
        obs, carry, _, acts = inputs(kind, T, n, depth, seed=100 * kind + 10 * T + n)
        reset = np.zeros((T, n), np.uint8)
        if T >= 3:
            reset[0, 0::3] = 1
            reset[2, 1::3] = 1
        dout = dout_of(kind, T, n)
        c = dict(sh=sh, prm=prm, obs=obs, carry=carry, reset=reset, acts=acts, dout=dout)
        for name, dt in (("g64", torch.float64), ("g32", torch.float32)):
            t = lambda x: torch.from_numpy(x).to(dt)  # noqa: E731, B023
            f = t(prm).requires_grad_()
            if kind == ACTOR:
                out = PS.actor_log_prob(f, depth, mix, t(obs), t(carry), torch.from_numpy(reset), t(acts))
            else:
                out = PS.critic_value(f, depth, t(obs), t(carry), torch.from_numpy(reset))
            (g,) = torch.autograd.grad((out * t(dout)).sum(), f)
            c[name] = g.double().numpy()
        _GRAD[key] = c
    return _GRAD[key]


GRAD_CASES = ([(ACTOR, d, m, 4, 33) for d, m in ((1, 1), (2, 3), (8, 8))] + [(ACTOR, 2, 3, 1, 1), (ACTOR, 2, 3, 4, 150)]
              + [(CRITIC, 1, 1, 4, 33), (CRITIC, 8, 1, 4, 33)])


@pytest.mark.parametrize("kind,depth,mix,T,n", GRAD_CASES)
def test_gradient_parity(kind, depth, mix, T, n):
    c = grad_case(kind, depth, mix, T, n)
    net = P.GruPolicy(kind, c["prm"], shape=c["sh"])
    _, g, _ = train_run(net, c["obs"], c["carry"], c["reset"], c["acts"], c["dout"])
    g = g.numpy().astype(np.float64)
    assert np.isfinite(g).all()
    bound = C_BOUND.get((depth, mix), 8.0)
    actor = kind == ACTOR
    bad, i = [], 0
    for name, shp in zip(PS.names(actor, depth), PS.shapes(actor, depth, mix)):
        k = int(np.prod(shp))
        ref = c["g64"][i:i + k]
        scale = np.max(np.abs(ref))
        assert scale > 0, f"{name}: the reference gradient is all zero"
        eg, er = np.max(np.abs(g[i:i + k] - ref)) / scale, np.max(np.abs(c["g32"][i:i + k] - ref)) / scale
        print(f"GRADERR kind={kind} depth={depth} mix={mix} T={T} n={n} {name} err_gpu={eg:.3e} err_ref32={er:.3e} "
              f"ratio={eg / max(er, 1e-300):.2f}")
        if not eg <= bound * er:
            bad.append((name, eg, er))
        if actor and mix == 1 and name.startswith("output_proj"):
            # one component: softmax(logit) = 1 whatever the logit, so the logit rows get exactly nothing
            rows = g[i:i + k].reshape(shp)[2 * NJ:3 * NJ]
            assert rows.size and not rows.any(), name
        i += k
    assert not bad, bad
    if actor:
        assert i == g.size - NJ and not g[i:].any()  # JOINT_BIASES are constants


@pytest.mark.parametrize("depth,mix", [(1, 1), (2, 3), (8, 8)])
def test_std_clip_fixture_takes_both_branches(depth, mix):
    c = grad_case(ACTOR, depth, mix, 4, 33)
    t = lambda x: torch.from_numpy(x).double()  # noqa: E731
    with torch.no_grad():
        f = t(c["prm"])
        raw = PS.trunk(f, True, depth, mix, t(c["obs"]), t(c["carry"]), torch.from_numpy(c["reset"]))
        frac = PS.head(f, depth, mix, raw)[3].double().mean().item()
    assert 0.1 <= frac <= 0.9, frac


def test_backward_is_deterministic_at_the_maxima():
    c = grad_case(ACTOR, 8, 8, 4, 33)
    net = P.GruPolicy(ACTOR, c["prm"], shape=c["sh"])
    args = (c["obs"], c["carry"], c["reset"], c["acts"], c["dout"])
    g1, g2 = train_run(net, *args)[1], train_run(net, *args)[1]
    assert torch.equal(g1, g2) and g1.abs().max() > 0


def test_refusals():
    sh = PolicyShape(2, 3)
    net = P.GruPolicy(ACTOR, shape=sh)
    with pytest.raises(ZbError, match="block layout"):
        net.set_layout(P.LAYOUT_WAVE)
    with pytest.raises(ZbError, match="block layout"):
        P.GruPolicy(ACTOR, generic=True).set_layout(P.LAYOUT_WAVE2)
    net.set_layout(P.LAYOUT_BLOCK)
    n = 3
    with pytest.raises(ZbError, match="carry"):
        net.actor(torch.zeros(n, 50, device="cuda"), torch.zeros(n, 5, H, device="cuda"))
    with pytest.raises(ZbError, match="hidden_size"):
        P.GruPolicy(ACTOR, shape=PolicyShape(2, 3, 256))
    with pytest.raises(ZbError, match="depth"):
        P.GruPolicy(CRITIC, shape=PolicyShape(9, 1))
    T = 2
    words = net.train_scratch_words(T, n)
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    obs, acts, lp, c0, scratch = z(T, n, 50), z(T, n, NJ), z(T, n, NJ), z(n, 2, H), z(words)
    L = net.L
    call = lambda sw: L.zb_policy_actor_train(net.h, obs.data_ptr(), T, n, c0.data_ptr(), None, acts.data_ptr(),  # noqa: E731
                                              lp.data_ptr(), scratch.data_ptr(), sw, None)
    assert call(words) == 0 and call(words - 1) == -1  # ZB_EARG, nothing launched
    assert "scratch" in L.zb_last_error().decode()
    torch.cuda.synchronize()


def make_engine(cmodel):
    from zbot_amd import default_config
    from zbot_amd.engine import HipEngine

    return HipEngine(cmodel, default_config(solver="newton"), 64, seed=2)


def test_policy_rollout_with_a_shaped_actor(cmodel):
    runs = []
    for _ in range(2):
        sh = PolicyShape(2, 3)
        ro = P.PolicyRollout(make_engine(cmodel), P.GruPolicy(ACTOR, P.init_params(ACTOR, 8, sh), shape=sh), seed=5)
        out = ro.run(4)
        torch.cuda.synchronize()
        assert ro.carry.shape == (64, 2, H)
        runs.append({k: out[k].cpu() for k in ("obs_actor", "actions", "log_prob", "reward")})
    for k, x in runs[0].items():
        assert torch.isfinite(x).all() and torch.equal(x, runs[1][k]), k


def test_trainer_with_shaped_networks(cmodel):
    """Actor (2, 3), critic depth 3: one step, state_dict() into a fresh Trainer, a second step on both gives
    the same parameters bit for bit; default-shape handles refuse the state."""
    from zbot_amd.train import Trainer

    sa, sc = PolicyShape(2, 3), PolicyShape(3, 1)

    def make(seeds, shapes=(sa, sc)):
        actor = P.GruPolicy(ACTOR, P.init_params(ACTOR, seeds[0], shapes[0]), shape=shapes[0])
        critic = P.GruPolicy(CRITIC, P.init_params(CRITIC, seeds[1], shapes[1]), shape=shapes[1])
        return Trainer(make_engine(cmodel), actor, critic, rollout_steps=8, num_passes=1, batch_size=32, seed=5)

    a = make((8, 9))
    a.step()
    sd = a.state_dict()
    assert sd["shapes"]["actor"]["depth"] == 2 and sd["shapes"]["critic"]["depth"] == 3
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    sd = torch.load(f, weights_only=False)
    b = make((1, 2))
    b.load_state_dict(sd)
    a.step()
    b.step()
    torch.cuda.synchronize()
    for net in ("actor", "critic"):
        pa, pb = a.learner.state_dict()[net]["params"], b.learner.state_dict()[net]["params"]
        assert torch.isfinite(pa).all() and torch.equal(pa, pb), net
    assert not torch.equal(a.actor.params_tensor().cpu(), torch.from_numpy(P.init_params(ACTOR, 8, sa)))
    with pytest.raises(ZbError, match="shape"):
        make((1, 2), shapes=(None, None)).load_state_dict(sd)
