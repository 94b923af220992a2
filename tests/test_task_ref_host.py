"""The restatement of the step end (tests/task_ref.py) against both CPU oracles on the edge set
(tests/task_cases.py), and the conditions the edge set itself must meet. No GPU.

This is where the restatement is shown to be right: tests/test_gpu_task_edges.py then holds the engine to it.
The conditions are on the inputs (how far a rung ends from its threshold, that both outcomes occur),
taken from the oracles alone; a rung that misses one is moved, the condition stays.
"""

import numpy as np
import pytest

import task_cases as TC
import task_ref as TR
from zbot_amd import cstructs as cs

_CACHE = {}


def stepped(O, cm, variant, solver, level, **kw):
    """(config, case, fp32 oracle step, fp64 oracle step) of the edge set, autoreset off; computed once."""
    key = (variant, solver, level, tuple(sorted(kw.items())))
    if key not in _CACHE:
        cfg = TC.config(variant, solver=solver, autoreset=False, **kw)
        case = TC.build(O, cm, cfg)
        _CACHE[key] = (cfg, case, TC.oracle_step(O, cm, cfg, case, level), TC.oracle_step(O, cm, cfg, case, level, "f64"))
    return _CACHE[key]


@pytest.mark.parametrize("level", TC.LEVELS)
@pytest.mark.parametrize("solver", ["cg", "newton"])
@pytest.mark.parametrize("variant", ["default", "lowz"])
def test_restatement_matches_both_oracles(cmodel, oracle_mod, variant, solver, level):
    cfg, case, r32, r64 = stepped(oracle_mod, cmodel, variant, solver, level)
    d32, d64 = r32.out["done"].astype(bool), r64.out["done"].astype(bool)
    # the two oracles part on `done` only at the time limit's edge (4000 x 0.02f: 80.0f, 79.9999982 in double)
    assert set(np.flatnonzero(d32 != d64).tolist()) <= set(TC.EP_EDGE)
    for name, r in (("f32", r32), ("f64", r64)):
        rs = TR.restate(cfg, cmodel.cmodel, case.state, r.state, level, reward=r.out["reward"])
        # the fp32 law is the expectation: against the fp64 oracle, leave out the envs it decides otherwise
        keep = np.ones(case.n, bool) if name == "f32" else d32 == d64
        assert (~keep).sum() <= 3
        np.testing.assert_array_equal(rs["done"][keep], r.out["done"].astype(bool)[keep])
        np.testing.assert_array_equal(rs["success"][keep], r.out["success"].astype(bool)[keep])
        np.testing.assert_array_equal(rs["airtime"][keep], r.state[keep, cs.S_AIRTIME:cs.S_AIRTIME + 2])
        np.testing.assert_array_equal(rs["prev_cont"], r.state[:, cs.S_PREV_CONT:cs.S_PREV_CONT + 2])
        np.testing.assert_array_equal(rs["ep_steps"], TR.u32(r.state[:, cs.S_EP_STEPS]))
        np.testing.assert_array_equal(rs["rng_step"], TR.u32(r.state[:, cs.S_RNG_STEP]))
        np.testing.assert_array_equal(rs["stats"][keep], r.stats[keep])
        terms = r.out["reward_terms"].astype(np.float64)
        for k in ("simple_single_foot_contact", "feet_airtime", "feet_too_close", "naive_forward"):
            np.testing.assert_array_equal(rs[k], terms[:, cs.TERM_NAMES.index(k)], err_msg=k)
        for k in TR.RESTATED:
            got = terms[:, cs.TERM_NAMES.index(k)]
            # fp64 oracle: its outputs are float32 words (half an ulp) of fp64 values; the fp32 oracle computes the
            # term in under twenty fp32 operations: 8 ulps at max(1, |term|), the engine's bound
            bound = 1e-8 + 4 * 2.0 ** -23 * np.abs(rs[k]) if name == "f64" else 8 * TR.ulps(rs[k])
            err = np.abs(got - rs[k])
            assert (err[keep] <= bound[keep]).all(), (name, k, float(err.max()), int(err.argmax()))
        total = TR.reward_sum(cfg, terms, level)
        assert (np.abs(total - r.out["reward"]) <= 16 * TR.ulps(TR.reward_sum(cfg, terms, level, magnitude=True))).all()
        # the running return advances by exactly the reward, and the observation's words are the state's
        ret = (case.state[:, cs.S_EP_RETURN] + r.out["reward"]).astype(np.float32)
        if name == "f32":
            np.testing.assert_array_equal(r.state[:, cs.S_EP_RETURN], ret)
        ox = r.out["obs_extra"]
        np.testing.assert_array_equal(r.state[:, cs.S_TOUCH:cs.S_TOUCH + 2], ox[:, cs.X_TOUCH:cs.X_TOUCH + 2])
        feet = ox[:, cs.X_FEET_POS:cs.X_FEET_POS + 6].astype(np.float64)
        dist = np.linalg.norm(feet[:, :3] - feet[:, 3:], axis=1)
        assert np.abs(dist - r.state[:, cs.S_FEET_DIST]).max() <= 8 * 2.0 ** -23 * 0.25  # 8 ulps of a length under 0.25


def test_time_limit_follows_the_fp32_product(cmodel, oracle_mod):
    """4000 steps of float32(0.02) s reach float32(80): an env entering the step with S_EP_STEPS 3999 ends
    (and succeeds) by the fp32 law, which the engine states; in double the product is 79.9999982."""
    cfg, case, r32, r64 = stepped(oracle_mod, cmodel, "default", "cg", 1.0)
    assert np.float32(4000) * np.float32(cfg.ctrl_dt) >= np.float32(cfg.max_episode_sec)
    assert not 4000 * float(np.float32(cfg.ctrl_dt)) >= 80.0
    e = TC.G["ep_steps"]
    assert r32.out["done"][e].tolist() == [0, 0, 1, 1] and r32.out["success"][e].tolist() == [0, 0, 1, 1]
    assert r64.out["done"][e].tolist() == [0, 0, 0, 1]
    rs = TR.restate(cfg, cmodel.cmodel, case.state, r64.state)
    assert rs["done"][e].tolist() == [0, 0, 1, 1]  # the restatement takes the decision in float32 from any state


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_edge_set_conditions(cmodel, oracle_mod, solver):
    cfg, case, r32, r64 = stepped(oracle_mod, cmodel, "default", solver, 1.0)
    G = TC.G
    d32, d64 = r32.out["done"].astype(bool), r64.out["done"].astype(bool)
    np.testing.assert_array_equal(d32, TC.EXPECT_DONE)
    np.testing.assert_array_equal(r32.out["success"].astype(bool), TC.EXPECT_SUCCESS)
    rest = np.setdiff1d(np.arange(case.n), TC.EP_EDGE)
    np.testing.assert_array_equal(d32[rest], d64[rest])
    for r in (r32, r64):
        z = r.state[G["z"], 2].astype(np.float64)
        assert np.abs(z - cfg.bad_z[1]).min() >= TC.Z_MARGIN, z
        for k in ("tilt_x", "tilt_y"):
            upz = TR.up_z(r.state[G[k], 3:7]).astype(np.float64)
            assert np.abs(upz - np.cos(cfg.max_tilt_rad)).min() >= TC.UPZ_MARGIN, (k, upz)
        # lifted rungs touch nothing
        lifted = G["z"] + G["tilt_x"] + G["tilt_y"] + G["vx"]
        assert not r.state[lifted, cs.S_TOUCH:cs.S_TOUCH + 2].any()
    # both outcomes on every ladder
    for k in ("z", "tilt_x", "tilt_y", "ep_steps"):
        assert 0 < d32[G[k]].sum() < len(G[k]), k
    terms = r32.out["reward_terms"]
    clip = np.float32(cfg.naive_forward_clip_max)
    nf, vx = terms[G["vx"], cs.TERM_NAMES.index("naive_forward")], r32.state[G["vx"], cs.S_QVEL]
    assert (nf == clip).sum() >= 2 and (nf < clip).sum() >= 2 and (nf < 0).any() and (vx > clip).sum() >= 2
    assert case.state[G["vx"][2], cs.S_QVEL] == clip
    assert terms[G["feet_dist"], cs.TERM_NAMES.index("feet_too_close")].tolist() == [1, 1, 0, 0]
    # every discrete term takes each of its values on at least two envs
    for k in TR.DISCRETE:
        col = terms[:, cs.TERM_NAMES.index(k)]
        vals = (col != 0) if k == "feet_airtime" else col
        u, cnt = np.unique(vals, return_counts=True)
        assert len(u) >= 2 and cnt.min() >= 2, (k, u, cnt)
    rs = TR.restate(cfg, cmodel.cmodel, case.state, r32.state)
    td = rs["touchdown"][G["touch"]]
    assert {tuple(x) for x in td.tolist()} == {(True, False), (False, True), (True, True), (False, False)}
    grew = rs["airtime"] > case.state[:, cs.S_AIRTIME:cs.S_AIRTIME + 2]
    assert grew[G["touch"]].any() and (case.state[G["touch"], cs.S_AIRTIME:cs.S_AIRTIME + 2][grew[G["touch"]]] > 0).any()
    for e in G["air_trunc"] + G["air_fail"]:  # a foot in the air on a step that ends the episode
        assert case.state[e, cs.S_AIRTIME:cs.S_AIRTIME + 2].max() > 0 and d32[e] and not rs["airtime"][e].any()
    assert d32[G["fail_trunc"]].all() and rs["trunc"][G["fail_trunc"]].all() and rs["fail"][G["fail_trunc"]].all()
    assert not r32.out["success"][G["fail_trunc"]].any()
    # wave placement of the terminating envs: env 2k is team 0 of wave k, env 2k + 1 team 1
    pairs = [(bool(d32[2 * k]), bool(d32[2 * k + 1])) for k in range(case.n // 2)]
    assert {(True, True), (True, False), (False, True), (False, False)} <= set(pairs)
    assert pairs[G["team0"][0] // 2] == (True, False) and pairs[G["team1"][0] // 2] == (False, True)
    assert pairs[G["both"][0] // 2] == (True, True)
    assert case.n % 2 == 1 and d32[case.n - 1] and G["last"] == [case.n - 1]


def test_lowz_variant_crosses_the_lower_bound(cmodel, oracle_mod):
    cfg, case, r32, r64 = stepped(oracle_mod, cmodel, "lowz", "cg", 1.0)
    z = r32.state[TC.G["z"], 2]
    d = r32.out["done"][TC.G["z"]].astype(bool)
    np.testing.assert_array_equal(d, z < np.float32(cfg.bad_z[0]))
    assert 0 < d.sum() < len(d) and (z < cfg.bad_z[1]).all()
    rest = np.setdiff1d(np.arange(case.n), TC.EP_EDGE)
    np.testing.assert_array_equal(r32.out["done"][rest], r64.out["done"][rest])
    for r in (r32, r64):
        assert np.abs(r.state[TC.G["z"], 2].astype(np.float64) - cfg.bad_z[0]).min() >= TC.Z_MARGIN


def test_maxerr_fails_on_nonfinite_output():
    """The one-step contract's bookkeeping (test_gpu_parity.MaxErr): a NaN row counts as over the bound, and a
    non-finite output fails the report even on an env that is exempt from the loose limit."""
    from test_gpu_parity import MaxErr

    ref = np.zeros((4, 3))
    ok = MaxErr("finite")
    ok.add("x", ref + 1e-7, ref, 1e-6)
    ok.report()
    for bad in (np.nan, np.inf):
        got = ref.copy()
        got[2, 1] = bad
        err = MaxErr("nonfinite", budget=1)
        err.add("x", got, ref, 1e-6, ref64=ref, exempt={2})
        assert err.nout["x"] == 1 and err.take_over() == [2]
        with pytest.raises(AssertionError, match="non-finite"):
            err.report()
        err = MaxErr("nonfinite, no budget", budget=0)
        err.add("x", got, ref, 1e-6)
        assert err.bad
    flat = MaxErr("vector")
    flat.add("r", np.array([0.0, np.nan]), np.zeros(2), 1e-6)
    assert flat.nout["r"] == 1 and flat.nonfinite


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_push_timer_rungs(cmodel, oracle_mod, solver):
    """With pushes on, S_PUSH_TIMER = float32(ctrl_dt) fires (timer - ctrl_dt <= 0), the float32 above it does
    not, 0.01 does; both oracles agree, and a fired timer is redrawn from push_interval."""
    cfg, case, r32, r64 = stepped(oracle_mod, cmodel, "default", solver, 1.0, push=True)
    for r in (r32, r64):
        new, old = r.state[:, cs.S_PUSH_TIMER], case.state[:, cs.S_PUSH_TIMER]
        fired = new > old
        assert {e: bool(fired[e]) for e in TC.G["push"]} == TC.PUSH_FIRES
        assert fired.sum() == 2 and (new[fired] >= cfg.push_interval[0]).all()
        np.testing.assert_array_equal(new[~fired], (old - np.float32(cfg.ctrl_dt))[~fired])
