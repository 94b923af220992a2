"""The minibatch kernels (csrc/zb_minibatch.hip, include/zbot_ppo.h "Minibatches") and the learners'
shuffle_seed over them, on the GPU.

Kernel bar: the permutation equals the host twin's, and the gather equals torch.index_select on the
host permutation, bit for bit, at every access width. Learner bar: shuffling is data movement only
(a shuffled update equals an unshuffled update of the rollout permuted beforehand, bit for bit);
HipPpoLearner and PpoLearner shuffle alike; and shuffle_seed=None is still the by-hand sequence of
tests/test_gpu_learner_update.py.
"""

import numpy as np
import pytest
import torch

from test_gpu_learner_update import by_hand, compare_case, fresh_nets, pol, rollout, run_update  # noqa: F401 - fixtures
from zbot_amd import ppo
from zbot_amd.policy import ACTOR, CRITIC

pytestmark = pytest.mark.gpu
NJ = 20
# floats per row: obs_critic 1936 B, obs_actor 200 B, actions 80 B, values 4 B; and the 1-byte done flags
ROWS = ((484, torch.float32), (50, torch.float32), (20, torch.float32), (1, torch.float32), (1, torch.uint8))


@pytest.mark.parametrize("n", [1, 33, 4097, 65536])
def test_device_permutation_equals_the_host_twin(n):
    for seed, epoch in ((0, 0), (2**63 + 11, 2**32 - 1), (5, 3)):
        got = ppo.minibatch_perm(n, seed, epoch, device="cuda").cpu().numpy()
        assert np.array_equal(got, ppo.minibatch_perm_host(n, seed, epoch)), (n, seed, epoch)


def _tensor(shape, dtype, offset, gen):
    """A random device tensor; offset: its storage starts 4 bytes past a 16-byte boundary."""
    numel = int(np.prod(shape))
    if dtype == torch.uint8:
        host = torch.randint(0, 256, (numel,), dtype=torch.uint8, generator=gen)
        pad = 4
    else:
        host = torch.randn(numel, generator=gen)
        pad = 1
    if not offset:
        return host.cuda().view(shape)
    buf = torch.zeros(numel + pad, dtype=dtype, device="cuda")
    out = buf[pad:].view(shape)
    out.copy_(host.view(shape))
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("shuffle_seed", [None, 11])
@pytest.mark.parametrize("lo,count", [(0, 33), (16, 17), (32, 1)])
def test_gather_equals_index_select(lo, count, shuffle_seed, offset):
    T, n, epoch = 3, 33, 2
    gen = torch.Generator().manual_seed(100 * lo + count)
    srcs = [_tensor((T + 1, n, F) if F == 50 else (T, n, F), dt, offset, gen) for F, dt in ROWS]  # obs_actor: [T + 1]
    dsts = [_tensor((T, count, F), dt, offset, gen) for F, dt in ROWS]
    carry, cdst = _tensor((n, 5, 128), torch.float32, offset, gen), _tensor((count, 5, 128), torch.float32, offset, gen)
    zdst = torch.full((1, count), 9, dtype=torch.uint8, device="cuda")
    items = list(zip(srcs, dsts)) + [(carry[None], cdst[None]), (None, zdst)]
    ppo.gather_minibatch(items, n, lo, count, shuffle_seed=shuffle_seed, epoch=epoch)
    torch.cuda.synchronize()
    if shuffle_seed is None:
        idx = torch.arange(lo, lo + count)
    else:
        idx = torch.from_numpy(ppo.minibatch_perm_host(n, shuffle_seed, epoch)[lo:lo + count].astype(np.int64))
    for s, d in zip(srcs, dsts):
        want = torch.index_select(s[:T].cpu(), 1, idx)
        assert d.cpu().numpy().tobytes() == want.contiguous().numpy().tobytes(), (tuple(s.shape), s.dtype)
        if shuffle_seed is None:
            assert torch.equal(d, s[:T, lo:lo + count])  # the slice
    assert torch.equal(cdst.cpu(), torch.index_select(carry.cpu(), 0, idx))
    assert not zdst.any()


def test_gather_argument_checks():
    """Refused calls return ZB_EARG and launch nothing: a pre-filled destination keeps its fill."""
    from zbot_amd.engine import load_library

    L = load_library()
    T, n, count = 2, 8, 4
    src = torch.ones(T, n, 3, device="cuda")
    dst = torch.full((T, count, 3), 7.0, device="cuda")
    ok = ppo.ZbGatherItem(src.data_ptr(), dst.data_ptr(), T, 12, n * 12)

    def call(items, n_items=1, n_=n, lo=0, count_=count):
        arr = (ppo.ZbGatherItem * len(items))(*items)
        return L.zb_minibatch_gather(arr, n_items, n_, lo, count_, 1, 0, 0, None)

    assert call([ok], lo=5) == -1 and call([ok], lo=-1) == -1 and call([ok], count_=0) == -1
    assert call([ok], lo=2**31 - 2) == -1 and call([ok], n_=0) == -1
    assert call([ok], n_items=0) == -1 and call([ok] * 17, n_items=17) == -1
    assert L.zb_minibatch_gather(None, 1, n, 0, count, 1, 0, 0, None) == -1
    assert call([ppo.ZbGatherItem(src.data_ptr(), None, T, 12, n * 12)]) == -1
    assert call([ok, ppo.ZbGatherItem(src.data_ptr(), None, T, 12, n * 12)], n_items=2) == -1
    assert call([ppo.ZbGatherItem(src.data_ptr(), dst.data_ptr(), 0, 12, n * 12)]) == -1
    assert call([ppo.ZbGatherItem(src.data_ptr(), dst.data_ptr(), T, 0, n * 12)]) == -1
    assert call([ppo.ZbGatherItem(src.data_ptr(), dst.data_ptr(), T, 12, -12)]) == -1
    perm = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    assert L.zb_minibatch_perm(0, 0, 0, perm.data_ptr(), None) == -1 and L.zb_minibatch_perm(0, 0, 4, None, None) == -1
    torch.cuda.synchronize()
    assert torch.all(dst == 7.0) and torch.all(perm == 7)
    with pytest.raises(ppo.ZbError):
        ppo.gather_minibatch([(src.cpu(), dst.cpu())], n, 0, count)
    with pytest.raises(ppo.ZbError):
        ppo.gather_minibatch([(src, dst.transpose(0, 1))], n, 0, count)
    with pytest.raises(ppo.ZbError):
        ppo.gather_minibatch([(src, dst)], n, 0, count, shuffle_seed=-1)
    with pytest.raises(ppo.ZbError):
        ppo.gather_minibatch([(src, dst)], n, 0, count, shuffle_seed=1, epoch=2**32)
    torch.cuda.synchronize()
    assert torch.all(dst == 7.0)
    assert call([ok]) == 0
    torch.cuda.synchronize()
    assert torch.all(dst == 1.0)


# ---- the learners' shuffle_seed ----

def _permuted(r, perm):
    """The rollout fixture with its env axis, both carries and the reset rows permuted."""
    from zbot_amd.ppo import PPOInputs

    p = torch.from_numpy(perm.astype(np.int64)).cuda()
    per_env = ("obs_critic_next", "value_next")  # [n, ...]; every other array is [T or T + 1, n, ...]
    out = {k: v.index_select(0 if k in per_env else 1, p) for k, v in r["out"].items()}
    inp = r["inputs"]
    inputs = PPOInputs(*(x.index_select(1, p) for x in (inp.advantages_t, inp.value_targets_t, inp.gae_t, inp.returns_t)))
    return dict(r, out=out, inputs=inputs, carry0=r["carry0"].index_select(0, p), ccarry0=r["ccarry0"].index_select(0, p),
                reset=r["reset"].index_select(1, p))


def test_shuffle_is_data_movement_only(pol, rollout):
    from zbot_amd.learner import HipPpoLearner

    r, seed = rollout, 13
    kw = dict(learning_rate=3e-4, max_grad_norm=1e-3, weight_decay=1e-5)
    a1, c1 = fresh_nets(pol, r)
    l1 = HipPpoLearner(shuffle_seed=seed, **kw)
    sums1 = run_update(l1, r, a1, c1, num_passes=1, batch_size=16)
    perm = ppo.minibatch_perm_host(r["n"], seed, 0)
    assert not np.array_equal(perm, np.arange(r["n"]))
    a2, c2 = fresh_nets(pol, r)
    l2 = HipPpoLearner(**kw)
    sums2 = run_update(l2, _permuted(r, perm), a2, c2, num_passes=1, batch_size=16)
    torch.cuda.synchronize()
    assert len(sums1) == len(sums2) == 3 and l1.epoch == 1 and l1.step == 3
    for x, y in zip(sums1, sums2):
        assert torch.equal(x, y)
    s1, s2 = l1.state_dict(), l2.state_dict()
    for net in ("actor", "critic"):
        for k in ("params", "m", "v"):
            assert torch.equal(s1[net][k], s2[net][k]), (net, k)
    # and it is not the unshuffled update of the unpermuted rollout
    a3, c3 = fresh_nets(pol, r)
    l3 = HipPpoLearner(**kw)
    run_update(l3, r, a3, c3, num_passes=1, batch_size=16)
    assert not torch.equal(l3.state_dict()["actor"]["params"], s1["actor"]["params"])
    # reset=None builds the same rows inside the gather (row 0 zeros, row t done[t - 1])
    a4, c4 = fresh_nets(pol, r)
    l4 = HipPpoLearner(shuffle_seed=seed, **kw)
    l4.update(r["out"], r["inputs"], a4, c4, r["carry0"], r["ccarry0"], reset=None, num_passes=1, batch_size=16)
    assert torch.equal(l4.state_dict()["actor"]["params"], s1["actor"]["params"])
    # a second pass takes the next permutation, and the state dict carries the pass count
    run_update(l1, r, a1, c1, num_passes=1, batch_size=16)
    sd = l1.state_dict()
    assert sd["epoch"] == 2 and sd["step"] == 6
    l5 = HipPpoLearner(shuffle_seed=seed, **kw)
    old = {k: v for k, v in sd.items() if k != "epoch"}
    l5.load_state_dict(old)
    assert l5.epoch == 0
    l5.load_state_dict(sd)
    assert l5.epoch == 2


def test_both_learners_shuffle_alike(pol):
    """test_one_step_against_the_torch_learner's rule over one pass of two shuffled minibatches
    (17 + 16 envs): on the elements whose gradient is at least 1e-3 of their network's largest, the
    two learners' parameter changes differ by at most 1 % of the learning rate.

    The gradient the rule reads is the first optimizer step's: an element is compared when its
    gradient on the pass's first minibatch (the library's, at the initial weights) reaches 1e-3 of
    that gradient's largest. Adam's first step moves an element by lr g1 / (|g1| + eps): a sign
    function of rounding error where g1 is noise, however large the element's gradient over the
    whole batch is. From the second step on the move is lr m / (sqrt(v) + eps) with m and v
    carrying g1, so a gradient difference d between the learners moves it by about lr d / |g1|:
    small wherever g1 is above the threshold, whatever g2 is. Masked by the whole-batch gradient
    the actor's worst gap measured 0.11 lr (printed below as `whole-batch mask`, with the gap on
    the elements above the threshold in both minibatches: 2.2e-4 lr actor, 9.9e-5 lr critic); that is
    the first step's sign effect and not a disagreement about the minibatches, whose bits
    test_shuffle_is_data_movement_only pins."""
    from zbot_amd.learner import HipPpoLearner, PpoLearner, TrainablePolicy
    from zbot_amd.ppo import PPOInputs

    c = compare_case()
    T, n, lr, seed = c["T"], c["n"], 3e-4, 4
    d = lambda k: torch.from_numpy(c[k]).cuda()  # noqa: E731
    probe_a, probe_c = pol.GruPolicy(ACTOR, c["Pa"]), pol.GruPolicy(CRITIC, c["Pc"])
    lp, sa = probe_a.actor_train(d("obs_a"), d("actions"), d("carry_a"), d("reset"))
    v, sc = probe_c.critic_train(d("obs_c"), d("carry_c"), d("reset"))
    ro = dict(obs_actor=d("obs_a"), actions=d("actions"), obs_critic=d("obs_c"), log_prob=lp + d("dlp"), value=v + d("dv"))
    inputs = PPOInputs(advantages_t=d("adv"), value_targets_t=v + d("dtgt"), gae_t=None, returns_t=None)
    d_lp, d_v, _ = ppo.ppo_loss_grad(lp, ro["log_prob"], inputs.advantages_t, v, ro["value"], inputs.value_targets_t)
    grads = dict(actor=probe_a.actor_backward(d("obs_a"), d("actions"), d("carry_a"), d("reset"), d_lp, sa).clone(),
                 critic=probe_c.critic_backward(d("obs_c"), d("carry_c"), d("reset"), d_v, sc).clone())

    def one_pass(cls, wrap):
        a, k = pol.GruPolicy(ACTOR, c["Pa"]), pol.GruPolicy(CRITIC, c["Pc"])
        ln = cls(learning_rate=lr, shuffle_seed=seed)
        out = ln.update(ro, inputs, wrap(a), wrap(k), d("carry_a"), d("carry_c"), reset=d("reset"), num_passes=1,
                        batch_size=17)
        torch.cuda.synchronize()
        assert len(out) == 2 and ln.epoch == 1
        return dict(actor=a.params_tensor().double(), critic=k.params_tensor().double())

    # each step's own gradient: the two minibatches, cut by the same gather, at the initial weights
    from zbot_amd.learner import _ShuffledMinibatches

    step_grads = []
    for lo, count in ((0, 17), (17, 16)):
        mb = _ShuffledMinibatches().cut(torch, ro, inputs, d("carry_a"), d("carry_c"), d("reset"), T, n, lo, count, seed, 0)
        lp_k, sa_k = probe_a.actor_train(mb["obs_a"], mb["acts"], mb["ca"], mb["rs"])
        v_k, sc_k = probe_c.critic_train(mb["obs_c"], mb["cc"], mb["rs"])
        dl, dv, _ = ppo.ppo_loss_grad(lp_k, mb["old_lp"], mb["adv"], v_k, mb["old_v"], mb["vt"])
        step_grads.append(dict(actor=probe_a.actor_backward(mb["obs_a"], mb["acts"], mb["ca"], mb["rs"], dl, sa_k).clone(),
                               critic=probe_c.critic_backward(mb["obs_c"], mb["cc"], mb["rs"], dv, sc_k).clone()))

    hip = one_pass(HipPpoLearner, lambda h: h)
    ref = one_pass(PpoLearner, TrainablePolicy)
    for net, p0 in (("actor", c["Pa"]), ("critic", c["Pc"])):
        live = p0.size - (NJ if net == "actor" else 0)
        p0d = torch.from_numpy(p0).cuda().double()
        gap = ((hip[net] - p0d) - (ref[net] - p0d))[:live].abs()
        g = grads[net][:live].abs()
        whole = g >= 1e-3 * g.max()
        print(f"VSTORCH-SHUFFLED {net} whole-batch mask: share={whole.double().mean().item():.3f} "
              f"max gap = {gap[whole].max().item() / lr:.2e} lr")
        both = torch.ones_like(whole)
        for sg in step_grads:
            gk = sg[net][:live].abs()
            both &= gk >= 1e-3 * gk.max()
        print(f"VSTORCH-SHUFFLED {net} both-minibatches mask: share={both.double().mean().item():.3f} "
              f"max gap = {gap[both].max().item() / lr:.2e} lr")
        # where both steps' gradients are above the threshold the bound holds without the argument above
        assert both.any() and gap[both].max().item() <= 0.01 * lr
        g1 = step_grads[0][net][:live].abs()
        mask = g1 >= 1e-3 * g1.max()
        share = mask.double().mean().item()
        dh, dr = (hip[net] - p0d)[:live][mask], (ref[net] - p0d)[:live][mask]
        worst = (dh - dr).abs().max().item()
        print(f"VSTORCH-SHUFFLED {net} compared share={share:.3f} max |dp_hip - dp_torch| = {worst:.3e} = "
              f"{worst / lr:.2e} lr; max |dp| = {dh.abs().max().item():.3e}")
        # the fixture's guard as in the one-step test: over half of each network's elements carry a
        # whole-batch gradient above the threshold. A minibatch of half the envs concentrates the
        # gradient (measured first-step shares: actor 0.85, critic 0.40), so the compared set is
        # asked to be at least a quarter of the network: never a sliver, tens of thousands of elements
        assert whole.double().mean().item() >= 0.5
        assert share >= 0.25
        assert worst <= 0.01 * lr
        assert dh.abs().max().item() > 0.5 * lr
    assert torch.equal(hip["actor"][-NJ:], ref["actor"][-NJ:])


def test_no_seed_is_the_sequence_by_hand(pol, rollout):
    """shuffle_seed=None: the untouched path, still the explicit calls of test_gpu_learner_update.by_hand."""
    from zbot_amd.learner import HipPpoLearner

    r = rollout
    lr, mx, wd = 3e-4, 1e-3, 1e-5
    st, sums_hand, _, _ = by_hand(pol, r, 2, 16, lr, mx, wd)
    actor, critic = fresh_nets(pol, r)
    ln = HipPpoLearner(learning_rate=lr, max_grad_norm=mx, weight_decay=wd, shuffle_seed=None)
    sums = run_update(ln, r, actor, critic, num_passes=2, batch_size=16)
    torch.cuda.synchronize()
    assert len(sums) == len(sums_hand) == 6
    for a, b in zip(sums, sums_hand):
        assert torch.equal(a[:4], b)
    sd = ln.state_dict()
    for net, key in (("actor", "a"), ("critic", "c")):
        for name, x in zip(("params", "m", "v"), st[key]):
            assert torch.equal(sd[net][name], x), (net, name)
