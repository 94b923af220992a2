"""Fixtures shared by tests/test_learner_host.py (CPU) and tests/test_gpu_learner_update.py (GPU):
the loss batches that cycle their rows through every branch of zbl_loss_row
(include/zbot_learner_math.h), and the AdamW sequences. Built once per key and left unchanged.

Loss rows: the target log ratio of row i cycles over LR_TARGETS (inside the clip, outside it on
both sides, beyond log_clip_value on both sides) with +-0.02 jitter, spread evenly over the 20
joints; the value offset v - old_v cycles over V_OFFSETS (inside the value clip, outside on both
sides) with +-0.02 jitter; the advantage's sign is random, so either sign meets either side.
7 and 5 are coprime: every pair of regimes occurs.

Every row keeps away from the branch boundaries (checked in fp64 by check_fixture, distances set
by the issue this feature answers): ||lr| - L| >= 0.1, |ratio - (1 +- eps)| >= 0.01,
||v - old_v| - eps| >= 0.01, and |a - b| >= 1e-4 where the value clip is active; rows that
violate one are redrawn.
"""

import numpy as np

NJ = 20
EPS, L_CLIP, COEF = 0.2, 10.0, 0.5
LR_TARGETS = (0.0, 0.05, -0.05, 0.4, -0.4, 12.0, -12.0)
V_OFFSETS = (0.0, 0.05, -0.05, 0.5, -0.5)
LOSS_SHAPES = [(3, 37), (2, 700), (1, 1)]

_LOSS = {}


def row_quantities(c):
    """fp64 per-row quantities of a loss case, from its float32 arrays."""
    d = lambda k: c[k].astype(np.float64)  # noqa: E731
    lr = d("log_prob").sum(-1) - d("old_log_prob").sum(-1)
    ratio = np.exp(np.clip(lr, -L_CLIP, L_CLIP))
    dv = d("values") - d("old_values")
    vc = d("old_values") + np.clip(dv, -EPS, EPS)
    a, b = (d("values") - d("value_targets")) ** 2, (vc - d("value_targets")) ** 2
    return dict(lr=lr, ratio=ratio, dv=dv, a=a, b=b, A=d("advantages"))


def violations(c):
    """Boolean [T, n]: rows closer to a branch boundary than the fixture allows."""
    q = row_quantities(c)
    bad = np.abs(np.abs(q["lr"]) - L_CLIP) < 0.1
    bad |= np.abs(q["ratio"] - (1 + EPS)) < 0.01
    bad |= np.abs(q["ratio"] - (1 - EPS)) < 0.01
    bad |= np.abs(np.abs(q["dv"]) - EPS) < 0.01
    bad |= (np.abs(q["dv"]) > EPS) & (np.abs(q["a"] - q["b"]) < 1e-4)
    return bad


def regimes(c):
    """{name: boolean [T, n]} of the branches the fixture has to reach."""
    q = row_quantities(c)
    inlog = np.abs(q["lr"]) <= L_CLIP
    hi, lo = inlog & (q["ratio"] > 1 + EPS), inlog & (q["ratio"] < 1 - EPS)
    vout = np.abs(q["dv"]) > EPS
    return {
        "ratio inside": inlog & ~hi & ~lo,
        "ratio above, A > 0": hi & (q["A"] > 0), "ratio above, A < 0": hi & (q["A"] < 0),
        "ratio below, A > 0": lo & (q["A"] > 0), "ratio below, A < 0": lo & (q["A"] < 0),
        "log ratio above L": q["lr"] > L_CLIP, "log ratio below -L": q["lr"] < -L_CLIP,
        "value inside": ~vout, "value outside, a > b": vout & (q["a"] > q["b"]),
        "value outside, a < b": vout & (q["a"] < q["b"]),
    }


def _draw_rows(rng, idx):
    """Rows with flat indices idx -> dict of float32 arrays [len(idx), ...]."""
    k = len(idx)
    old_lp = rng.normal(-1.0, 0.5, size=(k, NJ))
    target = np.array(LR_TARGETS)[idx % len(LR_TARGETS)] + rng.uniform(-0.02, 0.02, size=k)
    lp = old_lp + (target / NJ)[:, None]
    old_v = rng.normal(size=k)
    v = old_v + np.array(V_OFFSETS)[idx % len(V_OFFSETS)] + rng.uniform(-0.02, 0.02, size=k)
    sign = np.where(rng.random(k) < 0.5, -1.0, 1.0)
    adv = sign * (0.2 + np.abs(rng.normal(size=k)))
    tgt = old_v + rng.normal(scale=0.7, size=k)
    f = lambda x: x.astype(np.float32)  # noqa: E731
    return dict(log_prob=f(lp), old_log_prob=f(old_lp), advantages=f(adv), values=f(v), old_values=f(old_v),
                value_targets=f(tgt))


def loss_case(T, n, seed=None):
    """The loss batch of one shape: float32 arrays [T, n, 20] / [T, n]."""
    key = (T, n, seed)
    if key in _LOSS:
        return _LOSS[key]
    if seed is None:
        # 1 x 1: with the default seed fp32 torch's d_value has error exactly 0 against fp64 (one
        # row, total = 1: v - tgt is exact), which leaves the error bar undefined; 13 is the first
        # seed from 11 upward at which none of the three fp32 torch errors is 0
        seed = {(1, 1): 13}.get((T, n), 1000 * T + n)
    rng = np.random.default_rng(seed)
    rows = T * n
    c = {k: x.reshape((T, n) + x.shape[1:]) for k, x in _draw_rows(rng, np.arange(rows)).items()}
    for _ in range(100):
        bad = np.flatnonzero(violations(c).reshape(-1))
        if bad.size == 0:
            break
        new = _draw_rows(rng, bad)
        for k in c:
            c[k].reshape((rows,) + c[k].shape[2:])[bad] = new[k]
    assert not violations(c).any()
    for x in c.values():
        x.setflags(write=False)
    c["T"], c["n"] = T, n
    _LOSS[key] = c
    return c


def first_pass_case(T, n):
    """A first optimizer pass: log_prob is old_log_prob bit for bit and values == old_values."""
    c = dict(loss_case(T, n))
    c["log_prob"] = c["old_log_prob"]
    c["values"] = c["old_values"]
    return c


# ---- AdamW sequences ----
ADAM_COUNT, ADAM_TAIL, ADAM_STEPS, ADAM_OTHER = 4099, 20, 3, 1000
ADAM_LR, ADAM_WD = 3e-4, 1e-2
ADAM_MAX_NORM = {"under": 2.0, "over": 0.1}  # the joint norm is about 1e-2 sqrt(5099) = 0.71

_ADAM = {}


def adam_case(seed=7):
    """Initial param / m / v and ADAM_STEPS gradients of 1e-2 normal with 50 exact zeros each (the
    slots backward writes as 0), plus the squared norm of a second network's gradient
    (ADAM_OTHER elements) that only enters the joint clip norm."""
    if seed in _ADAM:
        return _ADAM[seed]
    rng = np.random.default_rng(seed)
    c = dict(param=rng.normal(size=ADAM_COUNT).astype(np.float32), grads=[], other=[])
    for _ in range(ADAM_STEPS):
        g = (1e-2 * rng.normal(size=ADAM_COUNT)).astype(np.float32)
        g[rng.choice(ADAM_COUNT - ADAM_TAIL, size=50, replace=False)] = 0.0
        c["grads"].append(g)
        c["other"].append((1e-2 * rng.normal(size=ADAM_OTHER)).astype(np.float32))
    for x in [c["param"]] + c["grads"] + c["other"]:
        x.setflags(write=False)
    _ADAM[seed] = c
    return c


SQNORM_COUNTS = [1, 4099, 70001]


def sqnorm_case(count):
    return (1e-2 * np.random.default_rng(count).normal(size=count)).astype(np.float32)
