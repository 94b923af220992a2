"""Fixtures of the rollout summary (zb_rollout_summary, include/zbot_ppo.h "Rollout summary"), shared
by tests/test_rollout_summary_host.py and tests/test_gpu_rollout_summary.py, and an independent
restatement of its leaves and its tree on numpy float64."""

import functools

import numpy as np

from zbot_amd import cstructs as cs

SHAPES = ((1, 1), (3, 85), (4, 64), (1, 257), (7, 33), (3, 259))  # T x n: 1, 255, 256, 257, 231, 777 rows
# which nullable planes are present
COMBOS = {
    "all": dict(terms=True, cmd=True, success=True, lp=True, values=True),
    "bare": dict(terms=False, cmd=False, success=False, lp=False, values=False),
    "terms_values": dict(terms=True, cmd=False, success=True, lp=False, values=True),
    "cmd_lp": dict(terms=False, cmd=True, success=False, lp=True, values=False),
}
PLANES = ("reward_terms", "command_terms", "reward", "done", "success", "log_prob", "values", "value_targets")


@functools.lru_cache(maxsize=None)
def _planes(T: int, n: int) -> dict:
    rng = np.random.default_rng(100 * T + n)
    f = lambda *s: (rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 3, s)).astype(np.float32)  # noqa: E731
    p = dict(reward_terms=f(T, n, cs.NUM_TERMS), command_terms=f(T, n, cs.NUM_CMD_TERMS), reward=f(T, n),
             done=(rng.random((T, n)) < 0.2).astype(np.uint8), log_prob=f(T, n, 20), values=f(T, n),
             value_targets=f(T, n))
    p["success"] = (p["done"] * (rng.random((T, n)) < 0.5)).astype(np.uint8)
    p["done"][0, 0] = 7  # any non-zero byte counts once
    for a in p.values():
        a.setflags(write=False)
    return p


def planes_case(T: int, n: int, combo: str = "all") -> dict:
    """The eight planes of a [T, n] rollout (read-only, cached), None where `combo` leaves one out."""
    p, c = _planes(T, n), COMBOS[combo]
    on = dict(reward_terms=c["terms"], command_terms=c["cmd"], success=c["success"], log_prob=c["lp"],
              values=c["values"], value_targets=c["values"])
    return {k: (p[k] if on.get(k, True) else None) for k in PLANES}


def extremes_case(T: int = 3, n: int = 85) -> dict:
    """planes_case with a reward plane of negative zeros and term / value planes that mix 1e30, 1e-30
    and -0.0 (their squares overflow float32, not float64)."""
    p = {k: (None if v is None else v.copy()) for k, v in planes_case(T, n).items()}
    p["reward"][:] = -0.0
    big = np.array([1e30, -1e30, 1e-30, -1e-30, -0.0, 1.0], np.float32)
    for k in ("reward_terms", "command_terms", "values", "value_targets", "log_prob"):
        flat = p[k].reshape(-1)
        flat[:] = big[np.arange(flat.size) % big.size]
    p["value_targets"][:] = np.roll(p["value_targets"].reshape(-1), 1).reshape(T, n)
    return p


def leaves_numpy(p: dict) -> np.ndarray:
    """[rows, 32] float64: the header's leaf of every row and word (absent planes: +0.0)."""
    T, n = p["reward"].shape
    rows = T * n
    x = np.zeros((rows, cs.SUMMARY_WORDS), np.float64)
    d = lambda a: a.reshape(rows, -1).astype(np.float64)  # noqa: E731
    if p["reward_terms"] is not None:
        x[:, cs.SUM_TERMS:cs.SUM_TERMS + cs.NUM_TERMS] = d(p["reward_terms"])
    if p["command_terms"] is not None:
        x[:, cs.SUM_CMD_TERMS:cs.SUM_CMD_TERMS + cs.NUM_CMD_TERMS] = d(p["command_terms"])
    r = d(p["reward"])[:, 0]
    x[:, cs.SUM_REWARD], x[:, cs.SUM_REWARD_SQ] = r, r * r
    x[:, cs.SUM_DONE] = (p["done"].reshape(rows) != 0)
    if p["success"] is not None:
        x[:, cs.SUM_SUCCESS] = (p["success"].reshape(rows) != 0)
    if p["log_prob"] is not None:
        lp = d(p["log_prob"])
        s = lp[:, 0].copy()
        for j in range(1, lp.shape[1]):  # joint order, in float64
            s = s + lp[:, j]
        x[:, cs.SUM_LOG_PROB] = s
    if p["values"] is not None:
        v, g = d(p["values"])[:, 0], d(p["value_targets"])[:, 0]
        x[:, cs.SUM_VALUE], x[:, cs.SUM_VALUE_SQ] = v, v * v
        x[:, cs.SUM_TARGET], x[:, cs.SUM_TARGET_SQ] = g, g * g
        x[:, cs.SUM_RESIDUAL_SQ] = (g - v) * (g - v)
    x[:, cs.SUM_ROWS] = 1.0
    return x


def tree_numpy(leaves: np.ndarray) -> np.ndarray:
    """The header's reduction tree over axis 0, all words at once: zero-padded to a power of two,
    adjacent pairs first, in float64; root + 0.0."""
    rows = leaves.shape[0]
    p = 1
    while p < rows:
        p <<= 1
    a = np.zeros((p,) + leaves.shape[1:], np.float64)
    a[:rows] = leaves
    while a.shape[0] > 1:
        a = a[0::2] + a[1::2]
    return a[0] + 0.0
