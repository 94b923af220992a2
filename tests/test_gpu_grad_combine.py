"""zb_grad_combine on the GPU (csrc/zb_learner.hip grad_combine_kernel): the sum over
ranks of an all-gathered gradient by the fixed fp64 tree, and the squared norm of the sum.

Kernel bar: the bits of the host twin zb_grad_combine_host, which tests/test_grad_combine_host.py
holds to an independent restatement of the tree; from 16-byte aligned storage (16-byte accesses when
the row stride allows them too) and from storage 4 bytes past a 16-byte boundary (4-byte accesses).

Gradient bar: two shards' gradients combined by the kernel against the one-process gradient over
the same envs, both measured against the fp64 torch restatement (tests/policy_torch.py) with §4m's
err = max|g - g64| / max|g64| per parameter tensor: the combined gradient stays within
max(8 err_ref32, 2 err_one). 8 is §4m's contract for an fp32 evaluation of the same sums in another
order; err_one is the one-process HIP gradient's own error, and 2 allows for the other split-K
partition of the same rows (each shard's K = 132 rows are summed apart, then added in fp64).
"""

import numpy as np
import pytest
import torch

import combine_cases as CC
import test_gpu_policy_train as TPT
from zbot_amd import ppo
from zbot_amd.policy import ACTOR, CRITIC, param_count

pytestmark = pytest.mark.gpu
WORLDS = (1, 2, 3, 8)
# one element; a chunk and one element; the two networks' gradients (neither a multiple of 4096)
COUNTS = (1, 4097, param_count(ACTOR), param_count(CRITIC))
# from storage 4 bytes past a 16-byte boundary: the same counts, and the actor's made odd like the
# others, so that rows alternate their alignment
CASES = [(c, False) for c in COUNTS] + [(c, True) for c in COUNTS + (param_count(ACTOR) + 1,)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev(x, misalign):
    """A device copy of a numpy array; misalign: 4 bytes past a 16-byte boundary."""
    t = torch.from_numpy(np.array(x))
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + t.numel()].view(t.shape) if misalign else buf[:t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == (4 if misalign else 0) and out.is_contiguous()
    return out


def run(parts, misalign):
    world, count = parts.shape
    p = dev(parts, misalign)
    g = dev(np.full(count, 7, np.float32), misalign)
    out, sq = ppo.grad_combine(p, out=g)
    assert out is g
    norm = ppo.grad_sqnorm(g)
    torch.cuda.synchronize()
    return g.cpu().numpy(), sq.cpu().numpy(), norm.cpu().numpy()


@pytest.mark.parametrize("count,misalign", CASES)
@pytest.mark.parametrize("world", WORLDS)
def test_bits_of_the_host_twin(world, count, misalign):
    parts = CC.parts_case(world, count)
    want_g, want_sq = ppo.grad_combine_host(parts)
    g, sq, norm = run(parts, misalign)
    assert same_bits(g, want_g), np.max(np.abs(g.astype(np.float64) - want_g))
    assert same_bits(sq[0], np.float64(want_sq))
    assert same_bits(sq, norm)  # what zb_grad_sqnorm returns on the gradient just written
    g2, sq2, _ = run(parts, misalign)
    assert same_bits(g, g2) and same_bits(sq, sq2)  # two identical calls, identical bits


def test_default_outputs_and_aligned_rows():
    """count a multiple of 4: every row start is 16-byte aligned and whole chunks move as float4."""
    parts = CC.parts_case(3, 3 * 4096)
    out, sq = ppo.grad_combine(torch.from_numpy(np.array(parts)).cuda())
    torch.cuda.synchronize()
    want_g, want_sq = ppo.grad_combine_host(parts)
    assert same_bits(out.cpu().numpy(), want_g) and sq.cpu().numpy()[0] == want_sq
    assert out.cpu().numpy()[CC.cancel_index(3 * 4096)] == 1.0


def test_refused_calls_touch_nothing():
    from zbot_amd.engine import load_library

    L = load_library()
    count = 4097
    parts = dev(CC.parts_case(3, count), False)
    grad = torch.full((count,), 7.0, device="cuda")
    part = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    sq = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")

    def call(p=parts.data_ptr(), world=3, n=count, g=grad.data_ptr(), pt=part.data_ptr(), s=sq.data_ptr()):
        return L.zb_grad_combine(p, world, n, g, pt, s, None)

    assert call(world=0) == -1 and call(world=65) == -1 and call(world=-3) == -1
    assert call(n=0) == -1 and call(n=(1 << 32) + 1) == -1
    assert call(p=None) == -1 and call(g=None) == -1 and call(pt=None) == -1 and call(s=None) == -1
    assert call(g=parts.data_ptr() + 4 * count) == -1  # grad is row 1 of parts
    torch.cuda.synchronize()
    assert torch.all(grad == 7) and torch.all(part == 7) and torch.all(sq == 7)
    with pytest.raises(ppo.ZbError):
        ppo.grad_combine(parts, out=parts[1])
    with pytest.raises(ppo.ZbError):
        ppo.grad_combine(parts, out=grad[:-1])
    with pytest.raises(ppo.ZbError):
        ppo.grad_combine(parts[0])
    assert call() == 0
    torch.cuda.synchronize()
    assert same_bits(grad.cpu().numpy(), ppo.grad_combine_host(CC.parts_case(3, count))[0])


@pytest.mark.parametrize("kind", [ACTOR, CRITIC])
def test_two_shard_gradient_against_one_process(kind):
    """§4m's fixture at 4 x 66 envs, in shards of 33: one minibatch holding everything, no shuffle."""
    from zbot_amd import policy as P

    T, n, half = 4, 66, 33
    c = TPT.make_case(kind, T, n, seed=100 * kind + 10 * T + n)
    c["g64"], c["g32"] = TPT.cpu_grad(c, torch.float64), TPT.cpu_grad(c, torch.float32)
    net = P.GruPolicy(kind, c["P"])
    _, g_one, _, _ = TPT.gpu_run(P, c, net=net)
    rows = []
    for lo in (0, half):
        s = dict(c)
        for k in ("obs", "reset", "actions", "dout"):
            s[k] = np.ascontiguousarray(c[k][:, lo:lo + half])
        s["carry0"] = np.ascontiguousarray(c["carry0"][lo:lo + half])
        rows.append(TPT.gpu_run(P, s, net=net)[1])
    g, _ = ppo.grad_combine(torch.from_numpy(np.stack(rows)).cuda())
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    e_dp, _ = TPT.tensor_errors(c, g.astype(np.float64))
    e_one, _ = TPT.tensor_errors(c, g_one.astype(np.float64))
    bad = []
    for name in e_dp:
        (ed, er), eo = e_dp[name], e_one[name][0]
        bound = max(TPT.C_BOUND * er, 2.0 * eo)
        print(f"DPGRADERR kind={kind} {name} err_dp={ed:.3e} err_one={eo:.3e} err_ref32={er:.3e} "
              f"dp/ref32={ed / max(er, 1e-300):.2f} dp/one={ed / max(eo, 1e-300):.2f}")
        if not ed <= bound:
            bad.append((name, ed, eo, er))
    assert not bad, bad
    if kind == ACTOR:
        assert np.all(g[-TPT.NJ:] == 0.0)  # the constants' gradient stays exactly 0 through the sum
