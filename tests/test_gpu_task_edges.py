"""The step end of the HIP step kernel at its edges: terminations at their thresholds, every reward
branch, the carried words, the statistics, auto-reset, the push timer, the ghost pass, terminations
inside a rollout launch, the flag word, a NaN env. One to four control steps on at most 64 envs.

(a) against the stated law: tests/task_ref.py (a plain numpy restatement, shown right on the CPU by
    tests/test_task_ref_host.py) applied to the engine's OWN state before and after the step. Decisions,
    discrete terms, counters and statistics exactly; the restated float terms within 8 fp32 ulps of
    max(1, |term|) = 9.5e-7 (each is under twenty fp32 operations from the state words, and the kernel's
    approximate reciprocal and rsqrt add an ulp or two each); the reward within 16 ulps of
    max(1, sum |scale term|) of the weighted sum of the engine's own terms.
(b) against the oracle from the same inputs, under test_gpu_parity's one-step contract, unchanged.
(c) auto-reset with pushes and randomization against the oracle.
(d) the ghost pass (the team whose wave partner resets) leaves no trace: bit-equal to a run whose
    partners do not terminate.
(e) terminations inside a rollout launch: bit-equal to single steps.
(f) the flag word (ZB_S_NAN) of an env does not depend on whether its wave partner terminated.
(g) a NaN env terminates, resets to a finite state and leaves the other envs' bits alone.

Measured on MI355X (pytest -s, profiles/task_edges_gpu.log), the largest error over the variants of (a):
in fp32 ulps of max(1, |x|), nine variants: stay_alive 0.01, linear_velocity_penalty_y 0.30, the three joint
penalties 0.01, upright 0.35 and naive_forward_orientation 0.31 (commands on, against X_CMD_XQUAT), reward
1.45 of the 16 allowed. (b) on the edge set: Newton qpos 1.2e-7, reward 4.8e-7; CG within 1.4x an env's
sensitivity. (c) reset envs: qpos 3.0e-8, rand row 1.2e-7, observations 4.2e-6.
"""

import numpy as np
import pytest

import task_cases as TC
import task_ref as TR
from test_gpu_parity import (CG_BUDGET, CG_LOOSE, CG_SLACK, ONE_STEP_TOL, MaxErr, boundary_envs, engine, one_step_outputs,
                             oracle_sensitivity, oracle_steps, print_budget_envs)
from zbot_amd import cstructs as cs

pytestmark = pytest.mark.gpu
LEVEL = 0.7
OUTS = ("obs_actor", "obs_critic", "obs_extra", "reward_terms", "reward", "done", "success")


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_MODELS = {}


def model(kind, cmodel):
    if kind == "default":
        return cmodel
    if kind not in _MODELS:
        import collider_util as U
        from zbot_amd import compile_model

        _MODELS[kind] = compile_model({"limbs": U.limbs_desc, "many": U.many_desc}[kind]())
    return _MODELS[kind]


_CASES = {}


def edge_set(O, cm, kind, variant, **kw):
    """The edge set on a config (the oracle's warm-up depends on the model, the randomization and the
    integrator, not on the solver fields the variants of (a) change); built once per key."""
    key = (kind, variant, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = TC.build(O, cm, TC.config(variant, **kw))
    return _CASES[key]


def step_once(torch, eng, state, rand, action, level=1.0):
    """set_state / set_rand, clear the statistics, one step: every output, the state and the statistics."""
    eng.set_state(torch.from_numpy(state.copy()))
    eng.set_rand(torch.from_numpy(rand.copy()))
    eng.get_stats(clear=True)
    out = eng.step(torch.from_numpy(action).cuda(), curriculum=level)
    torch.cuda.synchronize()
    eng.check()
    res = {k: out[k].cpu().numpy().copy() for k in OUTS}
    res["state"] = eng.get_state().cpu().numpy()
    res["stats"] = eng.get_stats().cpu().numpy()
    res["rand"] = eng.get_rand().cpu().numpy()
    return res


# ------------------------------------------------------------------ (a) the stated law
LAW_VARIANTS = {
    "cg": dict(),
    "newton": dict(solver="newton"),
    "cg_iterations4": dict(iterations=4),
    "cg_eulerdamp": dict(eulerdamp=True),
    "cg_commands": dict(commands=True),
    "cg_chunks4": dict(chunks=4),
    "cg_limbs": dict(kind="limbs"),
    "newton_limbs": dict(kind="limbs", solver="newton"),
    "cg_lowz": dict(variant="lowz"),
}
_MEASURED = {}


@pytest.mark.parametrize("name", list(LAW_VARIANTS))
def test_engine_obeys_the_stated_law(torch_gpu, cmodel, oracle_mod, name):
    torch = torch_gpu
    v = dict(LAW_VARIANTS[name])
    kind, variant, commands, chunks = v.pop("kind", "default"), v.pop("variant", "default"), v.pop("commands", False), v.pop("chunks", 0)
    cm = model(kind, cmodel)
    case = edge_set(oracle_mod, cm, kind, variant, autoreset=False, eulerdamp=v.get("eulerdamp", False))
    cfg = TC.config(variant, autoreset=False, **v)
    eng = engine(cm, cfg, case.n, seed=TC.SEED)
    if commands:
        import command_ref as R

        eng.set_command_config(R.joystick())  # every term scale 0: computed and reported, not rewarded
    if chunks:
        eng.set_step_chunks(chunks)
    g = step_once(torch, eng, case.state, case.rand, case.action, LEVEL)
    rs = TR.restate(cfg, cm.cmodel, case.state, g["state"], LEVEL, reward=g["reward"])
    terms = g["reward_terms"].astype(np.float64)
    col = {k: terms[:, i] for i, k in enumerate(cs.TERM_NAMES)}
    # decisions, discrete terms, carried words, statistics: exact
    np.testing.assert_array_equal(g["done"].astype(bool), rs["done"])
    np.testing.assert_array_equal(g["success"].astype(bool), rs["success"])
    if kind == "default" and variant == "default":
        np.testing.assert_array_equal(g["done"].astype(bool), TC.EXPECT_DONE)
        np.testing.assert_array_equal(g["success"].astype(bool), TC.EXPECT_SUCCESS)
    for k in ("simple_single_foot_contact", "feet_airtime", "feet_too_close", "naive_forward"):
        np.testing.assert_array_equal(col[k], rs[k], err_msg=k)
    st = g["state"]
    np.testing.assert_array_equal(st[:, cs.S_AIRTIME:cs.S_AIRTIME + 2], rs["airtime"])
    np.testing.assert_array_equal(st[:, cs.S_PREV_CONT:cs.S_PREV_CONT + 2], rs["prev_cont"])
    np.testing.assert_array_equal(TR.u32(st[:, cs.S_EP_STEPS]), rs["ep_steps"])
    np.testing.assert_array_equal(TR.u32(st[:, cs.S_RNG_STEP]), rs["rng_step"])
    np.testing.assert_array_equal(st[:, cs.S_EPISODE], case.state[:, cs.S_EPISODE])
    np.testing.assert_array_equal(st[:, cs.S_EP_RETURN], (case.state[:, cs.S_EP_RETURN] + g["reward"]).astype(np.float32))
    np.testing.assert_array_equal(g["stats"], rs["stats"].astype(np.float32))
    np.testing.assert_array_equal(st[:, cs.S_TOUCH:cs.S_TOUCH + 2], g["obs_extra"][:, cs.X_TOUCH:cs.X_TOUCH + 2])
    assert not st[:, cs.S_NAN].view(np.uint32).any()
    # restated float terms: 8 ulps of max(1, |term|)
    worst = {}
    for k in ("stay_alive", "linear_velocity_penalty_y", "straight_leg_penalty", "ankle_knee_penalty", "arm_pose_penalty"):
        worst[k] = float((np.abs(col[k] - rs[k]) / TR.ulps(rs[k])).max())
    if commands:
        ot = TR.orientation_terms(g["obs_extra"][:, cs.X_CMD_XQUAT:cs.X_CMD_XQUAT + 4])
        for k, want in ot.items():
            worst[k] = float((np.abs(col[k] - want) / TR.ulps(want)).max())
    total, mag = TR.reward_sum(cfg, terms, LEVEL), TR.reward_sum(cfg, terms, LEVEL, magnitude=True)
    worst["reward"] = float((np.abs(g["reward"] - total) / TR.ulps(mag)).max())
    _MEASURED[name] = worst
    print(f"\n[law {name}] max error in fp32 ulps of max(1, |x|): " + ", ".join(f"{k} {x:.2f}" for k, x in worst.items()))
    for k, x in worst.items():
        assert x <= (16 if k == "reward" else 8), (k, x)


# ------------------------------------------------------------------ (b), (c) against the oracle
def contract_step(torch, O, cm, cfg, case, solver, name):
    """One step of the engine and of both oracles from the case's state under test_gpu_parity's one-step
    contract (MaxErr with ONE_STEP_TOL; CG: + CG_SLACK x the env's sensitivity, CG_BUDGET, CG_LOOSE), every
    output of one_step_outputs; done and success exact. Returns (engine result, fp32 oracle env, its outputs)."""
    n, cg = case.n, solver == "cg"
    env = O.OracleEnv(cm.cmodel, cfg, n, seed=TC.SEED)
    env.state[:], env.rand[:] = case.state, case.rand
    eng = engine(cm, cfg, n, seed=TC.SEED)
    ref, ref64 = oracle_steps(O, cm, cfg, env, case.action, TC.SEED)
    ref32 = {k: want for k, _, want in one_step_outputs(env.state, ref, env.state, ref)}
    # the fp64 oracle takes the time limit in double (tests/task_ref.py): where it decides otherwise its step is
    # no measure of this step's conditioning, so those envs get no fp32 / fp64 slack at all
    odd = TC.oracle_step(O, cm, cfg, case, precision="f64").out["done"] != ref["done"]
    assert set(np.flatnonzero(odd).tolist()) <= set(TC.EP_EDGE)
    for key in ref32:
        ref64[key] = np.where(odd.reshape((-1,) + (1,) * (np.ndim(ref32[key]) - 1)), ref32[key], ref64[key])
    sens = oracle_sensitivity(O, cm, cfg, case.state, case.rand, case.action, TC.SEED, ref32) if cg else {}
    g = step_once(torch, eng, case.state, case.rand, case.action)
    np.testing.assert_array_equal(g["done"], ref["done"])
    np.testing.assert_array_equal(g["success"], ref["success"])
    err = MaxErr(name, **(dict(budget=CG_BUDGET, loose=CG_LOOSE, max_ill=n, k_slack=CG_SLACK) if cg else {}))
    for key, got, want in one_step_outputs(g["state"], g, env.state, ref):
        err.add(key, got, want, *ONE_STEP_TOL[key], ref64=ref64[key], sens=sens.get(key), exempt=boundary_envs(ref64))
    print_budget_envs(err, 0, eng, env, ref64, g["state"])
    err.report()
    return g, env, ref


@pytest.mark.parametrize("variant", ["default", "lowz"])
@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_edge_set_against_oracle(torch_gpu, cmodel, oracle_mod, solver, variant):
    """Every output of the step on the edge set, the three terms the restatement cannot reach included."""
    cfg = TC.config(variant, solver=solver, autoreset=False)
    case = edge_set(oracle_mod, cmodel, "default", variant, autoreset=False, eulerdamp=False)
    g, env, ref = contract_step(torch_gpu, oracle_mod, cmodel, cfg, case, solver, f"edge set {solver} {variant}")
    if variant == "default":
        np.testing.assert_array_equal(g["done"].astype(bool), TC.EXPECT_DONE)
    for w in (cs.S_EP_STEPS, cs.S_RNG_STEP, cs.S_EPISODE):
        np.testing.assert_array_equal(TR.u32(g["state"][:, w]), TR.u32(env.state[:, w]))
    np.testing.assert_array_equal(g["state"][:, cs.S_AIRTIME:cs.S_AIRTIME + 2], env.state[:, cs.S_AIRTIME:cs.S_AIRTIME + 2])


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_autoreset_and_push_against_oracle(torch_gpu, cmodel, oracle_mod, solver):
    kw = dict(push=True, randomize=True, autoreset=True)
    cfg = TC.config("default", solver=solver, **kw)
    case = edge_set(oracle_mod, cmodel, "default", "default", **kw)
    g, env, ref = contract_step(torch_gpu, oracle_mod, cmodel, cfg, case, solver, f"auto-reset {solver}")
    d = TC.EXPECT_DONE
    np.testing.assert_array_equal(g["done"].astype(bool), d)
    np.testing.assert_array_equal(g["success"].astype(bool), TC.EXPECT_SUCCESS)
    st, ost = g["state"], env.state
    for w in (cs.S_EPISODE, cs.S_EP_STEPS, cs.S_RNG_STEP):
        np.testing.assert_array_equal(TR.u32(st[:, w]), TR.u32(ost[:, w]))
    assert (TR.u32(st[d, cs.S_EP_STEPS]) == 0).all() and (TR.u32(st[d, cs.S_EPISODE]) == TR.u32(case.state[d, cs.S_EPISODE]) + 1).all()
    # statistics: the counts against the oracle, the sums by the engine's own law (the reward's bound is (b)'s)
    for w in (cs.ST_LENGTH, cs.ST_DONE):
        np.testing.assert_array_equal(g["stats"][:, w], env.stats[:, w])
    np.testing.assert_array_equal(g["stats"][:, cs.ST_REWARD], g["reward"])
    ret = (case.state[:, cs.S_EP_RETURN] + g["reward"]).astype(np.float32)
    np.testing.assert_array_equal(g["stats"][:, cs.ST_RETURN], np.where(d, ret, np.float32(0)))
    # the reset state: the goldens' bound for final_rand
    tight = dict(qpos=slice(0, 27), qvel=slice(32, 58), lag=slice(cs.S_IMU_LAG, cs.S_IMU_LAG + 1),
                 push_timer=slice(cs.S_PUSH_TIMER, cs.S_PUSH_TIMER + 1))
    worst = {k: float(np.abs(st[d, s].astype(np.float64) - ost[d, s]).max()) for k, s in tight.items()}
    worst["rand"] = float(np.abs(g["rand"][d].astype(np.float64) - env.rand[d]).max())
    assert np.abs(env.rand[d] - case.rand[d]).max() > 1e-3  # the rows were resampled
    for k in ("obs_actor", "obs_critic", "obs_extra"):
        e = float(np.abs(g[k][d].astype(np.float64) - ref[k][d]).max())
        print(f"[auto-reset {solver}] reset observation {k}: {e:.2e}")
        assert e <= ONE_STEP_TOL[k][0], (k, e)
    print(f"[auto-reset {solver}] reset envs, max |error|: " + ", ".join(f"{k} {x:.2e}" for k, x in worst.items()))
    assert all(x <= 1e-6 for x in worst.values()), worst
    assert np.isfinite(st[d]).all() and not st[:, cs.S_AIRTIME:cs.S_AIRTIME + 2][d].any()
    # push rungs: who fired, read from the new timer (a fired timer is redrawn from push_interval >= 2 s)
    alive = ~d
    fired, ofired = st[:, cs.S_PUSH_TIMER] > case.state[:, cs.S_PUSH_TIMER], ost[:, cs.S_PUSH_TIMER] > case.state[:, cs.S_PUSH_TIMER]
    np.testing.assert_array_equal(fired[alive], ofired[alive])
    assert {e: bool(fired[e]) for e in TC.G["push"]} == TC.PUSH_FIRES
    np.testing.assert_array_equal(st[alive & ~fired, cs.S_PUSH_TIMER],
                                  (case.state[:, cs.S_PUSH_TIMER] - np.float32(cfg.ctrl_dt))[alive & ~fired])


# ------------------------------------------------------------------ (d) the ghost pass
@pytest.mark.parametrize("kind", ["default", "limbs"])
@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_ghost_pass_is_discarded(torch_gpu, cmodel, oracle_mod, solver, kind):
    """Handle A: the edge set with auto-reset, so a wave with one terminating team runs the other as a ghost
    through the reset's forward(). Handle B: the same states with every terminating env replaced by a plain
    one (no wave runs the extra pass). The surviving envs' state rows and outputs are the same bits."""
    torch = torch_gpu
    cm = model(kind, cmodel)
    cfg = TC.config("default", solver=solver, autoreset=True)
    case = edge_set(oracle_mod, cm, kind, "default", autoreset=True)
    ends = TC.EXPECT_DONE
    calm = case.state.copy()
    calm[ends] = case.state[21]  # a plain standing env (the RNG is keyed by the env id, not by the row)
    A = step_once(torch, engine(cm, cfg, case.n, seed=TC.SEED), case.state, case.rand, case.action)
    B = step_once(torch, engine(cm, cfg, case.n, seed=TC.SEED), calm, case.rand, case.action)
    np.testing.assert_array_equal(A["done"].astype(bool), ends)
    assert not B["done"].any()
    partner = np.arange(case.n) ^ 1
    partner[partner >= case.n] = case.n - 1
    ghosts = np.flatnonzero(~ends & ends[partner])
    assert (ghosts % 2 == 0).sum() >= 2 and (ghosts % 2 == 1).sum() >= 2  # either team of a wave
    alive = np.flatnonzero(~ends)
    for k in ("state", "stats") + OUTS:
        np.testing.assert_array_equal(A[k][alive].view(np.uint32 if A[k].dtype == np.float32 else A[k].dtype),
                                      B[k][alive].view(np.uint32 if B[k].dtype == np.float32 else B[k].dtype), err_msg=k)


# ------------------------------------------------------------------ (e) terminations inside a rollout launch
@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_rollout_with_terminations_equals_steps(torch_gpu, cmodel, oracle_mod, solver):
    """T = 4 with failures forced at step 0 and time limits at step 2 (S_EP_STEPS 47 of the 50 a 1 s episode
    has): rollout() leaves the bits of four step() calls, its reward_sum is the fp32 running sum of the
    steps' rewards, and three chunks per step change nothing."""
    torch = torch_gpu
    n, T = 32, 4
    cfg = TC.config("default", solver=solver, max_episode_sec=1.0)
    env = oracle_mod.OracleEnv(cmodel.cmodel, cfg, n, seed=9)
    env.reset()
    for t in range(20):
        env.step(oracle_mod.synthetic_actions(cmodel.cmodel, 9, n, 0, t))
    st = env.state.copy()
    fails, limits = [3, 8, 12, 13, 31], [5, 10, 20, 21]
    st[fails, 2] = 0.7
    for e in limits:
        st[e:e + 1, cs.S_EP_STEPS].view(np.uint32)[:] = 47
    acts = np.stack([oracle_mod.synthetic_actions(cmodel.cmodel, 9, n, 0, 100 + t) for t in range(T)])
    A = torch.from_numpy(acts).cuda()
    res = {}
    for chunks in (0, 3):
        a, b = engine(cmodel, cfg, n, seed=9), engine(cmodel, cfg, n, seed=9)
        for eng in (a, b):
            eng.set_state(torch.from_numpy(st.copy()))
            eng.get_stats(clear=True)
            if chunks:
                eng.set_step_chunks(chunks)
        rew, done, succ = [], [], []
        for t in range(T):
            o = a.step(A[t])
            torch.cuda.synchronize()
            rew.append(o["reward"].cpu().numpy().copy())
            done.append(o["done"].cpu().numpy().copy())
            succ.append(o["success"].cpu().numpy().copy())
        rsum = torch.zeros(n, device="cuda")
        ob = b.rollout(A, reward_sum=rsum)
        torch.cuda.synchronize()
        a.check()
        b.check()
        done, succ = np.stack(done).astype(bool), np.stack(succ).astype(bool)
        if not chunks:
            assert done[0, fails].all() and not succ[0, fails].any() and done[0].sum() == len(fails)
            assert done[2, limits].all() and succ[2, limits].all() and done[2].sum() == len(limits)
            assert not done[1].any() and not done[3].any()
        run = np.zeros(n, np.float32)
        for r in rew:
            run = (run + r).astype(np.float32)
        got = dict(state=a.get_state().cpu().numpy(), stats=a.get_stats().cpu().numpy(), reward_sum=run,
                   **{k: a.outputs()[k].cpu().numpy() for k in ("obs_actor", "obs_critic", "done", "success")})
        roll = dict(state=b.get_state().cpu().numpy(), stats=b.get_stats().cpu().numpy(), reward_sum=rsum.cpu().numpy(),
                    **{k: ob[k].cpu().numpy() for k in ("obs_actor", "obs_critic", "done", "success")})
        for k in got:
            np.testing.assert_array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                                          roll[k].view(np.uint32) if roll[k].dtype == np.float32 else roll[k],
                                          err_msg=f"{k}, chunks {chunks}")
        res[chunks] = got
    for k in res[0]:
        np.testing.assert_array_equal(res[0][k], res[3][k], err_msg=f"{k}: 3 chunks vs the automatic choice")


# ------------------------------------------------------------------ (f) the flag word and the partner
def overflow_ladder(O, cm, cfg_of):
    """Start heights of a robot lying face down and falling at 0.5 m/s (0.5 mm per substep, 0.1 mm per rung):
    (state rows [16, 192], action row, per rung: the largest count of colliders within reach of the floor
    over the 20 substep-start poses with the bound widened by 1e-5, and the count at the post-step pose
    with the bound narrowed by 1e-5). The poses are the oracle's after k = 0..20 substeps (a control
    step of k substeps); collider_util.bank2_candidates states the kernel's bound in float64."""
    import collider_util as U

    R = 16
    base = O.OracleEnv(cm.cmodel, cfg_of(20), 2, seed=TC.SEED)
    base.reset()
    for t in range(5):
        base.step(O.synthetic_actions(cm.cmodel, TC.SEED, 2, 0, t))
    st = np.tile(base.state[:1], (R, 1))
    st[:, 3:7] = np.array([np.cos(np.pi / 4), 0, np.sin(np.pi / 4), 0], np.float32)
    st[:, 2] = (0.0872 + 0.0001 * np.arange(R)).astype(np.float32)
    st[:, cs.S_QVEL:cs.S_QVEL + 26] = 0.0
    st[:, cs.S_QVEL + 2] = -0.5
    a = O.synthetic_actions(cm.cmodel, TC.SEED, 1, 0, 100)
    margin = float(cm.cmodel.floor_margin)
    count = lambda q, m: np.array([len(U.bank2_candidates(cm, x.astype(np.float64), m)) for x in q])  # noqa: E731
    before = count(st[:, :27], margin + 1e-5)
    for k in range(1, 21):
        e = O.OracleEnv(cm.cmodel, cfg_of(k), R, seed=TC.SEED)
        e.state[:] = st
        e.rand[:] = base.rand[:1]
        out = e.step(np.tile(a, (R, 1)))
        assert not out["done"].any()
        if k < 20:
            before = np.maximum(before, count(e.state[:, :27], margin + 1e-5))
    after = count(e.state[:, :27], margin - 1e-5)
    return st, a[0], base, before, after


def test_flags_do_not_depend_on_the_partner(torch_gpu, cmodel, oracle_mod):
    """An env whose colliders within reach exceed the banks at the post-step pose alone (a pose its own step
    never collides at) must not show an overflow because its wave partner reset and it ran the extra
    forward() as a ghost: ZB_S_NAN is the same word whether the partner terminates (A) or not (B)."""
    from zbot_amd import default_config
    from zbot_amd.engine import bank_cap

    torch = torch_gpu
    cm = model("many", cmodel)
    cap = bank_cap(cm)

    def cfg_of(k):
        c = default_config(solver="cg", ctrl_dt=k * 0.001)
        c.max_tilt_rad = np.pi  # a lying robot goes on: only BadZ's upper bound ends an episode here
        c.bad_z[0] = -1.0
        return c

    rows, act, base, before, after = overflow_ladder(oracle_mod, cm, cfg_of)
    premise = np.flatnonzero((before <= cap) & (after > cap))
    print(f"\n[flags] colliders within reach, cap {cap}: max over the substep-start poses {before.tolist()}, "
          f"at the post-step pose {after.tolist()}; premise rungs {premise.tolist()}")
    assert len(premise) >= 3
    R = len(rows)
    n = 2 * R
    rung_env = np.array([2 * i if i < R // 2 else 2 * i + 1 for i in range(R)])  # team 0 for half the rungs, team 1 for the rest
    st = np.tile(base.state[1:2], (n, 1))  # the partners: a standing robot
    st[rung_env] = rows
    a = np.tile(oracle_mod.synthetic_actions(cm.cmodel, TC.SEED, 1, 0, 100), (n, 1))
    a[rung_env] = act
    rand = np.tile(base.rand[:1], (n, 1))
    up = st.copy()
    up[rung_env ^ 1, 2] = 0.7  # the partners of handle A end their episode
    cfg = cfg_of(20)
    A = step_once(torch, engine(cm, cfg, n, seed=TC.SEED), up, rand, a)
    B = step_once(torch, engine(cm, cfg, n, seed=TC.SEED), st, rand, a)
    assert A["done"][rung_env ^ 1].all() and not A["done"][rung_env].any() and not B["done"].any()
    fa, fb = A["state"][rung_env, cs.S_NAN].view(np.uint32), B["state"][rung_env, cs.S_NAN].view(np.uint32)
    print(f"[flags] ZB_S_NAN of the rungs, partner terminates {fa.tolist()}, partner goes on {fb.tolist()}")
    np.testing.assert_array_equal(fa, fb)
    assert not fb[premise].any()  # no substep of these rungs' own step overflowed
    assert fb.any() and (fb[fb != 0] == 6).all() and (before[fb != 0] > cap).all()  # the lower rungs overflow in their own step
    np.testing.assert_array_equal(A["state"][rung_env].view(np.uint32), B["state"][rung_env].view(np.uint32))


# ------------------------------------------------------------------ (g) a NaN env
def test_nan_env_terminates_and_does_not_spread(torch_gpu, cmodel, oracle_mod):
    """One env's base height is NaN: it ends its episode as a failure, raises `nonfinite`, and resets to a
    finite state with finite observations; the other three envs (its wave partner among them) keep the
    bits of a run without the NaN.

    Read before running it: no address and no loop bound of step_kernel comes from a float of the state.
    zb_engine.hip converts no float to an integer anywhere (its only casts to int are of bit fields: pj_lane,
    childof, the chunk scheduler's unit index); its four `while` loops run over a row bitmask (add_rows),
    the integer solver iteration count (the Newton and CG iterations, `it < ...`) and the control step's own
    loop, which `continue`s on the integer substep counter and leaves on the bools resetting / ghost /
    done_reset; lanes and rows are picked by ballots of comparisons (a NaN compares false) and __ffs."""
    from zbot_amd.engine import state_flags

    torch = torch_gpu
    n, bad = 4, 2
    cfg = TC.config("default")
    env = oracle_mod.OracleEnv(cmodel.cmodel, cfg, n, seed=TC.SEED)
    env.reset()
    for t in range(10):
        env.step(oracle_mod.synthetic_actions(cmodel.cmodel, TC.SEED, n, 0, t))
    st = env.state.copy()
    a = oracle_mod.synthetic_actions(cmodel.cmodel, TC.SEED, n, 0, 100)
    clean = step_once(torch, engine(cmodel, cfg, n, seed=TC.SEED), st, env.rand, a)
    st_nan = st.copy()
    st_nan[bad, 2] = np.nan
    eng = engine(cmodel, cfg, n, seed=TC.SEED)
    g = step_once(torch, eng, st_nan, env.rand, a)
    assert g["done"].tolist() == [0, 0, 1, 0] and g["success"].tolist() == [0, 0, 0, 0]
    fl = state_flags(torch.from_numpy(g["state"]))
    assert fl["nonfinite"].tolist() == [False, False, True, False]
    row = g["state"][bad].copy()
    row[cs.S_NAN] = 0.0  # the flag word is bits, not a float
    assert np.isfinite(row).all()
    for k in ("obs_actor", "obs_critic", "obs_extra"):
        assert np.isfinite(g[k][bad]).all(), k
    others = [e for e in range(n) if e != bad]
    for k in ("state", "stats") + OUTS:
        x, y = g[k][others], clean[k][others]
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                      y.view(np.uint32) if y.dtype == np.float32 else y, err_msg=k)
