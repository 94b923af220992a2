"""zb_rollout_summary_host (include/zbot_ppo.h "Rollout summary") and metrics.rollout_telemetry on
the CPU: the host twin against a numpy restatement of the header's leaves and tree, bit for bit;
against math.fsum within the pairwise-summation bound; its argument checks; and the telemetry's
closed forms on hand-made sums. No GPU needed."""

import math

import numpy as np
import pytest
import torch

import command_ref as R
import summary_cases as SC
from zbot_amd import default_config, ppo
from zbot_amd import cstructs as cs
from zbot_amd import engine as E
from zbot_amd.metrics import rollout_telemetry

CASES = [(T, n, c) for T, n in SC.SHAPES for c in SC.COMBOS]


@pytest.fixture(scope="module")
def lib():
    E.build_library()
    return E.load_library()


def host_sums(p):
    return ppo.rollout_summary_host(p["reward"], p["done"], p["success"], reward_terms=p["reward_terms"],
                                    command_terms=p["command_terms"], log_prob=p["log_prob"], values=p["values"],
                                    value_targets=p["value_targets"]).numpy()


@pytest.mark.parametrize("T,n,combo", CASES)
def test_twin_is_the_headers_tree(lib, T, n, combo):
    """Word for word the bits of the restated tree; the counts are the exact integers; each sum lies
    within the pairwise-summation bound of the correctly rounded sum of its leaves.

    The bound: a balanced pairwise tree over N leaves has depth L = ceil(log2 N), and every leaf
    passes through at most L additions, each with a relative error of at most u = 2^-53, so
    |tree - exact| <= ((1 + u)^L - 1) sum |leaf| = (L u + O(u^2)) sum |leaf| (Higham, Accuracy and
    Stability of Numerical Algorithms, 4.2). math.fsum returns the exact sum rounded once: it lies
    within u |exact| <= u sum |leaf| of it. The two together, and the O(u^2) term, are inside
    (L + 1) u sum |leaf|. The zero padding adds exactly and root + 0.0 is exact."""
    p = SC.planes_case(T, n, combo)
    got = host_sums(p)
    leaves = SC.leaves_numpy(p)
    want = SC.tree_numpy(leaves)
    assert got.dtype == np.float64 and got.shape == (cs.SUMMARY_WORDS,)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    rows = T * n
    assert got[cs.SUM_ROWS] == rows
    assert got[cs.SUM_DONE] == int((p["done"] != 0).sum())
    assert got[cs.SUM_SUCCESS] == (0 if p["success"] is None else int((p["success"] != 0).sum()))
    assert not got[cs.SUM_USED:].any() and not np.signbit(got[cs.SUM_USED:]).any()
    depth = math.ceil(math.log2(rows)) if rows > 1 else 0
    for w in range(cs.SUM_USED):
        exact = math.fsum(leaves[:, w])
        bound = (depth + 1) * 2.0 ** -53 * math.fsum(np.abs(leaves[:, w]))
        assert abs(got[w] - exact) <= bound, (w, got[w], exact, bound)
    if combo == "bare":  # the words of absent planes are +0.0
        absent = [w for w in range(cs.SUM_USED) if w not in (cs.SUM_REWARD, cs.SUM_REWARD_SQ, cs.SUM_DONE, cs.SUM_ROWS)]
        assert not got[absent].any() and not np.signbit(got[absent]).any()


def test_extremes_and_negative_zeros(lib):
    """1e30 and 1e-30 side by side, squares beyond float32, and a plane of -0.0 whose sum reads +0."""
    p = SC.extremes_case()
    got = host_sums(p)
    assert np.array_equal(got.view(np.uint64), SC.tree_numpy(SC.leaves_numpy(p)).view(np.uint64))
    assert got[cs.SUM_REWARD] == 0.0 and not np.signbit(got[cs.SUM_REWARD])
    assert np.isfinite(got).all() and got[cs.SUM_VALUE_SQ] > 1e59


def _call(lib, p, T, n, **over):
    ptr = {k: (None if v is None else v.ctypes.data) for k, v in p.items()}
    out = np.full(cs.SUMMARY_WORDS, 7.0)
    ptr["sums_out"] = out.ctypes.data
    ptr.update(over)
    rc = lib.zb_rollout_summary_host(*(ptr[k] for k in SC.PLANES), T, n, ptr["sums_out"])
    return rc, lib.zb_last_error().decode(), out


@pytest.mark.parametrize("over,T,n,word", [
    (dict(), 0, 85, "T = 0"),
    (dict(), 3, 0, "n = 0"),
    (dict(), -1, 85, "T = -1"),
    (dict(), 1 << 15, (1 << 13) + 1, "2^28"),
    (dict(reward=None), 3, 85, "reward"),
    (dict(done=None), 3, 85, "done"),
    (dict(sums_out=None), 3, 85, "sums_out"),
    (dict(values=None), 3, 85, "value_targets without values"),
    (dict(value_targets=None), 3, 85, "values without value_targets"),
])
def test_bad_arguments_name_the_field(lib, over, T, n, word):
    rc, msg, out = _call(lib, SC.planes_case(3, 85), T, n, **over)
    assert rc == -1 and word in msg and "zb_rollout_summary_host" in msg, (rc, msg)  # ZB_EARG
    assert (out == 7.0).all()  # nothing written


def test_device_entry_checks_before_any_launch(lib):
    """zb_rollout_summary refuses the same arguments, and a null partials, on the host: no device
    is touched (this test runs without one)."""
    p = SC.planes_case(3, 85)
    ptr = [p[k].ctypes.data for k in SC.PLANES]  # never dereferenced: every call is refused
    out = np.zeros(cs.SUMMARY_WORDS)
    assert lib.zb_rollout_summary(*ptr, 3, 85, None, out.ctypes.data, None) == -1
    assert "partials" in lib.zb_last_error().decode()
    assert lib.zb_rollout_summary(*ptr, 0, 85, out.ctypes.data, out.ctypes.data, None) == -1
    assert "T = 0" in lib.zb_last_error().decode()
    ptr[SC.PLANES.index("done")] = None
    assert lib.zb_rollout_summary(*ptr, 3, 85, out.ctypes.data, out.ctypes.data, None) == -1
    assert "done" in lib.zb_last_error().decode()
    words = lib.zb_rollout_summary_partials_words
    assert [words(1, 1), words(4, 64), words(1, 257), words(0, 4), words(4, 0), words(1 << 15, 1 << 14)] == \
        [32, 32, 64, 0, 0, 0]
    assert words(1 << 14, 1 << 14) == 32 << 20


def test_python_wrappers_check_shapes():
    p = SC.planes_case(3, 85)
    with pytest.raises(E.ZbError, match="log_prob"):
        ppo.rollout_summary_host(p["reward"], p["done"], log_prob=p["log_prob"][:, :, :19].copy())
    with pytest.raises(E.ZbError, match="both or neither"):
        ppo.rollout_summary_host(p["reward"], p["done"], values=p["values"])
    with pytest.raises(E.ZbError, match="done"):
        ppo.rollout_summary_host(p["reward"], p["done"].astype(np.float32))
    with pytest.raises(E.ZbError, match="GPU"):
        ppo.rollout_summary(torch.zeros(3, 85), torch.zeros(3, 85, dtype=torch.uint8))


def test_header_and_binding_agree_on_the_words():
    import os
    import re

    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zbot_ppo.h")).read()
    c = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ZB_(SUM\w+)\s+(\d+)", txt)}
    assert len(c) == 15
    for name, v in c.items():
        assert getattr(cs, name) == v, name
    assert ppo.SUMMARY_WORDS == cs.SUMMARY_WORDS == 32


def _sums(**w):
    s = torch.zeros(cs.SUMMARY_WORDS, dtype=torch.float64)
    for k, v in w.items():
        s[k if isinstance(k, int) else getattr(cs, k)] = v
    return s


def test_telemetry_closed_forms():
    cfg = default_config()
    cc = R.joystick(0.25, dict(linvel_tracking=1.5, yaw_tracking=0.5, xy_orientation=0.25, base_height=2.0),
                    by_curriculum=("linvel_tracking",))
    level, rows = 0.5, 8.0
    s = _sums(SUM_ROWS=rows, SUM_REWARD=4.0, SUM_REWARD_SQ=10.0, SUM_DONE=3.0, SUM_SUCCESS=1.0, SUM_LOG_PROB=-16.0,
              SUM_VALUE=2.0, SUM_VALUE_SQ=6.0, SUM_TARGET=8.0, SUM_TARGET_SQ=40.0, SUM_RESIDUAL_SQ=16.0)
    for i in range(cs.NUM_TERMS):
        s[cs.SUM_TERMS + i] = float(i + 1)
    for i in range(cs.NUM_CMD_TERMS):
        s[cs.SUM_CMD_TERMS + i] = -float(i + 1)
    stats = torch.zeros(4, cs.NUM_STATS)
    stats[:, cs.ST_RETURN] = torch.tensor([1.0, 2.0, 0.0, 3.0])
    stats[:, cs.ST_LENGTH] = torch.tensor([10.0, 20.0, 0.0, 30.0])
    stats[:, cs.ST_DONE] = torch.tensor([1.0, 1.0, 0.0, 1.0])
    t = rollout_telemetry(s, cfg, level, command_config=cc, stats=stats, ctrl_dt=0.02)
    assert all(v.dtype == torch.float64 and v.dim() == 0 for v in t.values())
    for i, name in enumerate(cs.TERM_NAMES):
        mean = (i + 1) / rows
        assert float(t[f"terms/{name}"]) == mean
        w = cfg.reward_scale[i] * (level if cfg.reward_by_curriculum[i] else 1.0)
        assert float(t[f"terms_scaled/{name}"]) == pytest.approx(w * mean, rel=1e-15)
    for i, name in enumerate(cs.CMD_TERM_NAMES):
        mean = -(i + 1) / rows
        assert float(t[f"terms/{name}"]) == mean
        w = cc.term_scale[i] * (level if cc.term_by_curriculum[i] else 1.0)
        assert float(t[f"terms_scaled/{name}"]) == pytest.approx(w * mean, rel=1e-15)
    assert float(t["terms_scaled/linvel_tracking"]) == pytest.approx(1.5 * 0.5 * -1 / 8)
    assert float(t["reward"]) == 0.5 and float(t["reward_std"]) == 1.0  # sqrt(10/8 - 1/4)
    assert float(t["done_rate"]) == 3 / 8 and float(t["failures"]) == 2.0 and float(t["time_limits"]) == 1.0
    assert float(t["entropy_estimate"]) == 2.0
    assert float(t["value_mean"]) == 0.25
    assert float(t["explained_variance"]) == 0.5  # var(target) = 40/8 - 1 = 4; 1 - (16/8) / 4
    assert float(t["episodes"]) == 3.0 and float(t["episode_return"]) == 2.0
    assert float(t["episode_length"]) == pytest.approx(20 * 0.02)
    # no command config, no stats: no such keys
    t = rollout_telemetry(s, cfg, level)
    assert "terms/linvel_tracking" not in t and "episodes" not in t and len(t) == 2 * cs.NUM_TERMS + 8


def test_explained_variance_is_nan_at_constant_targets():
    s = _sums(SUM_ROWS=4.0, SUM_TARGET=8.0, SUM_TARGET_SQ=16.0, SUM_VALUE=4.0, SUM_VALUE_SQ=6.0, SUM_RESIDUAL_SQ=5.0)
    t = rollout_telemetry(s, default_config(), 1.0)
    assert math.isnan(float(t["explained_variance"]))
    assert float(t["value_mean"]) == 1.0
    stats = torch.zeros(3, cs.NUM_STATS)  # no episode finished in the window
    t = rollout_telemetry(s, default_config(), 1.0, stats=stats)
    assert float(t["episodes"]) == 0.0 and math.isnan(float(t["episode_return"]))
    with pytest.raises(ValueError):
        rollout_telemetry(s.float(), default_config(), 1.0)
