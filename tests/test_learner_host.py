"""The learner's loss, gradient norm and AdamW on the CPU: the host twins of csrc/zb_learner.hip
(zb_ppo_loss_host, zb_grad_sqnorm_host, zb_adamw_step_host; include/zbot_ppo.h "Learner"), which run
include/zbot_learner_math.h and the same fp64 tree as the kernels and are their bit reference
(tests/test_gpu_learner_update.py). No GPU needed.

Accuracy bar, the project's (tests/test_gpu_policy_train.py): err(x) = max|x - x64| / max|x64| per
output against the fp64 torch evaluation on the CPU (autograd of learner.ppo_loss; torch.optim.AdamW
after optax's clip rule in fp64), held to C x the error the same torch function makes in fp32 on
the CPU. C is the smallest power of two that is at least twice the worst ratio measured
(DESIGN.md §4n has the tables).
"""

import ctypes as C

import numpy as np
import pytest
import torch

import learner_cases as LC
from zbot_amd import engine as E
from zbot_amd import learner as LN
from zbot_amd import ppo

C_LOSS = 16.0  # worst measured ratio 6.04 (the scalar loss at 3 x 37, clipped value loss)
C_ADAM = 4.0   # worst measured ratio 1.09 (m after step 3, norm over the maximum)


@pytest.fixture(scope="module", autouse=True)
def lib():
    E.build_library()
    return E.load_library()


def torch_loss(c, dtype, use_clip):
    """(d_log_prob, d_value, loss) of learner.ppo_loss by autograd on the CPU, as float64 numpy."""
    t = lambda k, g=False: torch.from_numpy(np.array(c[k])).to(dtype).requires_grad_(g)  # noqa: E731
    lp, v = t("log_prob", True), t("values", True)
    loss = LN.ppo_loss(lp, t("old_log_prob"), t("advantages"), v, t("old_values"), t("value_targets"),
                       clip_param=LC.EPS, value_loss_coef=LC.COEF, use_clipped_value_loss=use_clip,
                       log_clip_value=LC.L_CLIP)
    g_lp, g_v = torch.autograd.grad(loss, (lp, v))
    return g_lp.double().numpy(), g_v.double().numpy(), np.float64(loss.item())


def host_loss(c, use_clip, total=None):
    d_lp, d_v, sums = ppo.ppo_loss_grad_host(c["log_prob"], c["old_log_prob"], c["advantages"], c["values"],
                                             c["old_values"], c["value_targets"], total=total, clip_param=LC.EPS,
                                             value_loss_coef=LC.COEF, use_clipped_value_loss=use_clip,
                                             log_clip_value=LC.L_CLIP)
    return d_lp, d_v, sums


def err(x, x64):
    scale = np.max(np.abs(x64))
    assert scale > 0
    return float(np.max(np.abs(np.asarray(x, np.float64) - x64)) / scale)


@pytest.mark.parametrize("T,n", LC.LOSS_SHAPES)
def test_fixture_reaches_every_branch(T, n):
    c = LC.loss_case(T, n)
    assert not LC.violations(c).any()
    q = LC.row_quantities(c)
    active = np.abs(q["dv"]) > LC.EPS
    if active.any():
        print(f"FIXTURE T={T} n={n} min|a-b| where the clip is active = {np.abs(q['a'] - q['b'])[active].min():.3e}")
    if (T, n) != (1, 1):
        empty = [k for k, m in LC.regimes(c).items() if not m.any()]
        assert not empty, empty


@pytest.mark.parametrize("use_clip", [True, False])
@pytest.mark.parametrize("T,n", LC.LOSS_SHAPES)
def test_loss_against_fp64_autograd(T, n, use_clip):
    c = LC.loss_case(T, n)
    ref64, ref32 = torch_loss(c, torch.float64, use_clip), torch_loss(c, torch.float32, use_clip)
    d_lp, d_v, sums = host_loss(c, use_clip)
    total = float(T * n)
    loss = -sums[0] / total + LC.COEF * 0.5 * sums[1] / total
    bad = []
    for name, x, x64, x32 in zip(("d_log_prob", "d_value", "loss"), (d_lp, d_v, loss), ref64, ref32):
        e, e32 = err(x, x64), err(x32, x64)
        print(f"LOSSERR T={T} n={n} clip={int(use_clip)} {name} err={e:.3e} err_ref32={e32:.3e} "
              f"ratio={e / max(e32, 1e-300):.2f}")
        assert e32 > 0, f"{name}: the fp32 torch error is exactly 0: change this case's seed"
        if not e <= C_LOSS * e32:
            bad.append((name, e, e32))
    assert not bad, bad
    # every joint of a row gets the row's seed
    assert np.array_equal(d_lp, np.repeat(d_lp[..., :1], LC.NJ, axis=-1))
    # the diagnostics: the clipped count is an integer, the KL term is the sum of (ratio - 1) - cl
    q = LC.row_quantities(c)
    assert sums[2] == np.count_nonzero(np.abs(q["ratio"] - 1) > LC.EPS)
    kl = (q["ratio"] - 1) - np.clip(q["lr"], -LC.L_CLIP, LC.L_CLIP)
    assert abs(sums[3] - kl.sum()) <= 1e-5 * np.abs(kl).sum() + 1e-6


def test_total_scales_the_seeds():
    """`total` is the row count of the mean: a batch shared by two ranks halves every seed (a power
    of two: bit for bit) and leaves the sums alone."""
    c = LC.loss_case(3, 37)
    a, b = host_loss(c, True), host_loss(c, True, total=2.0 * 3 * 37)
    assert np.array_equal(a[0] * np.float32(0.5), b[0]) and np.array_equal(a[1] * np.float32(0.5), b[1])
    assert np.array_equal(a[2], b[2])


@pytest.mark.parametrize("T,n", LC.LOSS_SHAPES)
def test_first_pass_identities(T, n):
    """log_prob is old_log_prob bit for bit and values == old_values: the ratio is exactly 1, nothing is
    clipped, and the seeds are -A inv and c (v - tgt) inv, inv = (float)(1 / total). The reference is that
    expression in float32, left to right; 1 ulp is the float32 spacing at the reference. (Against an exact
    reference d_value's two roundings, of v - tgt and of the product, could differ by more than one
    spacing for any fp32 evaluation, so the fp32 expression is the reference this identity can mean.)"""
    c = LC.first_pass_case(T, n)
    d_lp, d_v, sums = host_loss(c, True)
    assert sums[2] == 0.0 and sums[3] == 0.0
    inv = np.float32(1.0 / (T * n))
    want_lp = (-c["advantages"]) * inv
    want_v = (np.float32(LC.COEF) * (c["values"] - c["value_targets"])) * inv
    assert want_lp.dtype == np.float32 and want_v.dtype == np.float32
    assert np.all(np.abs(d_lp - want_lp[..., None]) <= np.spacing(np.abs(want_lp))[..., None])
    assert np.all(np.abs(d_v - want_v) <= np.spacing(np.abs(want_v)))
    assert np.array_equal(host_loss(c, False)[1], d_v)  # v == old_v: both value losses agree


@pytest.mark.parametrize("count", LC.SQNORM_COUNTS)
def test_sqnorm_against_numpy(count):
    """The square of an fp32 value is exact in fp64 and the tree has fewer than 20 levels of 2^-53."""
    g = LC.sqnorm_case(count)
    want = np.sum(g.astype(np.float64) ** 2)
    got = ppo.grad_sqnorm_host(g)
    print(f"SQNORM count={count} rel err={abs(got - want) / want:.3e}")
    assert abs(got - want) <= 1e-13 * want
    assert got == ppo.grad_sqnorm_host(torch.from_numpy(g.copy()))  # a CPU tensor is taken too


def optax_scale64(sq, max_norm):
    N = np.sqrt(np.sum(np.asarray(sq, np.float64)))
    return max_norm / N if (max_norm > 0 and N > max_norm) else 1.0


def torch_adamw(c, dtype, max_norm):
    """[(param, m, v) after step 1, 2, 3] of torch.optim.AdamW on the live elements, gradients scaled
    by optax.clip_by_global_norm's factor formed in fp64; as float64 numpy."""
    live = LC.ADAM_COUNT - LC.ADAM_TAIL
    p = torch.from_numpy(c["param"][:live].copy()).to(dtype).requires_grad_()
    opt = torch.optim.AdamW([p], lr=LC.ADAM_LR, weight_decay=LC.ADAM_WD, eps=ppo.ADAM_EPS,
                            betas=(ppo.ADAM_BETA1, ppo.ADAM_BETA2))
    out = []
    for g, o in zip(c["grads"], c["other"]):
        sq = [np.sum(g.astype(np.float64) ** 2), np.sum(o.astype(np.float64) ** 2)]
        scale = torch.tensor(optax_scale64(sq, max_norm), dtype=torch.float64).to(dtype)
        p.grad = torch.from_numpy(g[:live].copy()).to(dtype) * scale
        opt.step()
        st = opt.state[p]
        out.append(tuple(x.detach().double().numpy().copy() for x in (p, st["exp_avg"], st["exp_avg_sq"])))
    return out


def host_adamw(c, max_norm, step0=1):
    """[(param, m, v) after each step] of zb_adamw_step_host over the whole arrays (tail included)."""
    p = c["param"].copy()
    m, v = np.full_like(p, 0.0), np.full_like(p, 0.0)
    m[-LC.ADAM_TAIL:], v[-LC.ADAM_TAIL:] = 3.0, 5.0  # the frozen tail of m and v is not ours to touch either
    out = []
    for i, (g, o) in enumerate(zip(c["grads"], c["other"])):
        sq = np.array([ppo.grad_sqnorm_host(g), ppo.grad_sqnorm_host(o)])
        ppo.adamw_step_host(p, g, m, v, sq, step0 + i, LC.ADAM_LR, max_grad_norm=max_norm, weight_decay=LC.ADAM_WD,
                            frozen_tail=LC.ADAM_TAIL)
        out.append((p.copy(), m.copy(), v.copy()))
    return out


@pytest.mark.parametrize("case", ["under", "over"])
def test_adamw_against_torch_fp64(case):
    c = LC.adam_case()
    mx = LC.ADAM_MAX_NORM[case]
    N = np.sqrt(sum(np.sum(x.astype(np.float64) ** 2) for x in (c["grads"][0], c["other"][0])))
    assert (N < mx) if case == "under" else (N > mx)
    ref64, ref32, got = torch_adamw(c, torch.float64, mx), torch_adamw(c, torch.float32, mx), host_adamw(c, mx)
    live = LC.ADAM_COUNT - LC.ADAM_TAIL
    bad = []
    for s in range(LC.ADAM_STEPS):
        for name, x, x64, x32 in zip(("param", "m", "v"), got[s], ref64[s], ref32[s]):
            e, e32 = err(x[:live], x64), err(x32, x64)
            print(f"ADAMERR case={case} step={s + 1} {name} err={e:.3e} err_ref32={e32:.3e} "
                  f"ratio={e / max(e32, 1e-300):.2f}")
            assert e32 > 0
            if not e <= C_ADAM * e32:
                bad.append((s + 1, name, e, e32))
        # the frozen tail of param, m and v is bit-unchanged
        assert np.array_equal(got[s][0][live:], c["param"][live:])
        assert np.all(got[s][1][live:] == 3.0) and np.all(got[s][2][live:] == 5.0)
    assert not bad, bad
    if case == "under":  # scale is exactly 1: the bits of a call with the clip off
        off = host_adamw(c, 0.0)
        for a, b in zip(got, off):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
    else:
        assert not np.array_equal(got[0][0], host_adamw(c, 0.0)[0][0])


def test_argument_checks(lib):
    """Null pointers, T <= 0, total <= 0, step < 1, frozen_tail > count and k < 1 are errors that touch nothing."""
    c = LC.loss_case(3, 37)
    T, n = 3, 37
    ins = [np.array(c[k]) for k in ("log_prob", "old_log_prob", "advantages", "values", "old_values", "value_targets")]
    d_lp, d_v, sums = np.full((T, n, LC.NJ), 7, np.float32), np.full((T, n), 7, np.float32), np.full(4, 7.0)
    fl = C.c_float

    def loss(ptrs=None, T_=T, n_=n, total=float(T * n), outs=None):
        ptrs = [x.ctypes.data for x in ins] if ptrs is None else ptrs
        outs = [d_lp.ctypes.data, d_v.ctypes.data, sums.ctypes.data] if outs is None else outs
        return lib.zb_ppo_loss_host(*ptrs, T_, n_, total, fl(LC.EPS), fl(LC.COEF), 1, fl(LC.L_CLIP), *outs)

    for i in range(6):
        p = [x.ctypes.data for x in ins]
        p[i] = None
        assert loss(ptrs=p) == -1  # ZB_EARG
    for i in range(3):
        o = [d_lp.ctypes.data, d_v.ctypes.data, sums.ctypes.data]
        o[i] = None
        assert loss(outs=o) != 0
    assert loss(T_=0) != 0 and loss(T_=-1) != 0 and loss(n_=0) != 0
    assert loss(total=0.0) != 0 and loss(total=-1.0) != 0 and loss(total=float("nan")) != 0
    assert b"total" in lib.zb_last_error()
    assert np.all(d_lp == 7) and np.all(d_v == 7) and np.all(sums == 7)
    assert loss() == 0 and not np.any(d_v == 7)

    g, out = LC.sqnorm_case(4099), np.full(1, 7.0)
    assert lib.zb_grad_sqnorm_host(None, g.size, out.ctypes.data) != 0
    assert lib.zb_grad_sqnorm_host(g.ctypes.data, g.size, None) != 0
    assert lib.zb_grad_sqnorm_host(g.ctypes.data, 0, out.ctypes.data) != 0
    assert out[0] == 7.0

    a = LC.adam_case()
    p0 = a["param"].copy()
    p, m, v, sq = p0.copy(), np.zeros_like(p0), np.zeros_like(p0), np.array([1.0, 2.0])
    gr = a["grads"][0]

    def adam(ptrs=None, count=p.size, tail=LC.ADAM_TAIL, k=2, step=1, sqp=sq.ctypes.data):
        ptrs = [p.ctypes.data, gr.ctypes.data, m.ctypes.data, v.ctypes.data] if ptrs is None else ptrs
        return lib.zb_adamw_step_host(*ptrs, count, tail, sqp, k, fl(1.0), fl(1e-3), 0.9, 0.999, fl(1e-8),
                                      fl(0.0), step)

    for i in range(4):
        q = [p.ctypes.data, gr.ctypes.data, m.ctypes.data, v.ctypes.data]
        q[i] = None
        assert adam(ptrs=q) != 0
    assert adam(sqp=None) != 0
    assert adam(step=0) != 0 and adam(step=-3) != 0
    assert adam(tail=p.size + 1) != 0
    assert adam(k=0) != 0 and adam(k=-1) != 0
    assert adam(count=0, tail=0) != 0
    assert np.array_equal(p, p0) and not m.any() and not v.any()
    assert adam(tail=p.size) == 0  # everything frozen: a valid no-op
    assert np.array_equal(p, p0) and not m.any() and not v.any()
    assert adam() == 0 and not np.array_equal(p, p0)
