"""Record the HIP engine's bits with friction-loss rows in all three zones of one wave (needs the
GPU): tests/golden/slot_diet_<case>.npz.

    python tests/golden/make_slot_diet.py [--out DIR] [--lib libzbot_hip.so] [case ...]

mj_constraintUpdate's friction-loss row has three zones: jar <= -R fl (force +fl), jar >= +R fl
(force -fl) and the linear zone between them. The other fixtures start from rest, where nearly every
row sits in the linear zone; a rewrite of eval_fric's selects (update_constraint_lane, rows_cost, the
warm start) that mixes up two arms would pass them. These cases give every hinge a velocity of
about 1 rad/s, which spreads the rows of one wave over all three zones, beside the dofs of the free
joint, which have no friction loss (fl = 0):

  n1_<solver>    n = 1: one env, the wave's second team a ghost. Default config.
  pair_<solver>  n = 2, [A, B]: A lifted 0.1 m (airborne at the start, no contact row), B set down on
                 the floor (its soles' lowest point 1 mm inside: in contact from the start) with one
                 limited hinge 0.05 rad past its range (the joint-limit row in one env of the wave
                 only). No observation
                 noise and no automatic reset, so that nothing depends on the env index: the test
                 replays [A, B] and [B, A] against the one fixture, the rows swapped.
  n3_<solver>    n = 3, [A, B, A2]: two waves, the second with a ghost. The pair's config.
  generic_cg     the pair with iterations = 3: the generic kernel (solver fields read from the
                 handle), not the default-fields copy.

Zones are checked on the CPU twin (oracle.OracleEnv stepped through the same actions from the same
state and randomization rows): at every pre-step state the oracle's constraint problem
(oracle.constraint_problem, no control) gives each friction-loss row's jar = J qacc - aref at its
solution. main() and the replay refuse a case in which a wave does not hold all three zones in one
and the same step, or, for the pair cases, in which A has a contact row at the start, B never gets
one, or the limit row is missing.

The fixtures were recorded with the library of commit 132bf6a ("Velocity commands: UnifiedCommand
and tracking rewards in step kernel"), the parent of the change that cut the CG wave's non-VALU
issue slots, before any kernel edit. What the engine-bit families share is in tests/bit_fixtures.py.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/, when run as a script
import bit_fixtures as F  # noqa: E402
import collider_util as U  # noqa: E402
from zbot_amd import default_config  # noqa: E402

FAMILY, MAX_KB = "slot_diet", 100
STEPS = 3
LIMIT_JOINT = ("left_elbow_roll", 1)  # env B: past the upper bound
VEL_SIGMA = 1.0  # rad/s, in steps of 1/32
LIFT = 0.1  # m above the reset height (airborne for every step of a case; 0.5 m would terminate the env)

CASES = {}
for _i, _sv in enumerate(("cg", "newton")):
    CASES[f"n1_{_sv}"] = dict(seed=61 + _i, solver=_sv, layout="B")
    CASES[f"pair_{_sv}"] = dict(seed=63 + _i, solver=_sv, layout="AB", plain=True)
    CASES[f"n3_{_sv}"] = dict(seed=65 + _i, solver=_sv, layout="ABA", plain=True)
CASES["generic_cg"] = dict(seed=67, solver="cg", layout="AB", plain=True, iterations=3)


def case_cfg(kw):
    extra = dict(obs_noise=False, autoreset=False) if kw.get("plain") else {}
    if "iterations" in kw:
        extra["iterations"] = kw["iterations"]
    return default_config(solver=kw["solver"], **extra)


def inputs(name):
    kw = CASES[name]
    return {"noise_q": F.action_noise(kw["seed"], STEPS, len(kw["layout"]))}


def start_state(cm, kw, st):
    """Reset state rows `st` [n, S_END] moved to the case's start: hinge velocities for every env,
    A lifted, B with one hinge past its limit; the warm start zero."""
    st = st.copy()
    n = len(kw["layout"])
    vel = np.float32(VEL_SIGMA) * F.noise(kw["seed"] + 1000, (n, 20)).astype(np.float32) / np.float32(32.0)
    for e, kind in enumerate(kw["layout"]):
        st[e] = st[0]  # the same reset row for every env: A and B differ only as described
        F.at_rest(cm, st[e])
        st[e, F.qvel_cols(cm)][6:] = vel[e]  # past the free joint's six dofs
        if kind == "A":
            F.lift(st[e], LIFT)
        else:
            F.set_past(cm, st[e], *LIMIT_JOINT)
            # down to the floor: the soles' lowest point 1 mm below it
            F.lift(st[e], -(U.lowest_point(cm, st[e, F.qpos_cols(cm)].astype(np.float64)) + 1e-3))
    return st


def run_layout(cm, kw, noise_q, start, same_rand, lib_path=None, swap=False):
    """One engine of the case's layout through its steps, from start(cm, kw, reset rows); the arrays a
    fixture keeps. same_rand: every env gets randomization row 0 (else its own)."""
    data = {"noise_q": noise_q}
    data.update(F.run(cm, case_cfg(kw), len(kw["layout"]), kw["seed"], F.actions(cm, noise_q),
                      start=lambda st: start(cm, kw, st), rand="row0" if same_rand else "own", lib_path=lib_path,
                      swap=swap, per_step=(*F.PER_STEP, "states"), final=("start_state", "start_rand", "last")))
    return data


def run_case(name, noise_q=None, lib_path=None, swap=False):
    """The arrays of one case, keyed as in its fixture. `noise_q`: the fixture's own (a replay)."""
    cm = F.model()
    if noise_q is None:
        noise_q = inputs(name)["noise_q"]
    return run_layout(cm, CASES[name], noise_q, start_state, True, lib_path, swap), cm


def row_zones(cm, cfg, q, v):
    """Friction-loss rows of the oracle's problem at (q, v) by zone at its solution: (below -R fl,
    above +R fl, linear), then the joint-limit rows and the contact rows."""
    import oracle as O  # noqa: PLC0415

    p = O.constraint_problem(cm.cmodel, cfg, q, v, precision="f32")
    fr = p["type"] == 0
    jar = p["J"] @ p["qacc"] - p["aref"]
    rf = p["R"] * p["floss"]
    lo, hi = fr & (jar <= -rf), fr & (jar >= rf)
    return (int(lo.sum()), int(hi.sum()), int((fr & ~lo & ~hi).sum()), int((p["type"] == 1).sum()),
            int((p["type"] == 2).sum()))


def twin_zones(name, cm, data):
    """[STEPS, n, 5] row_zones of the CPU twin's pre-step states along the case's actions."""
    kw = CASES[name]
    cfg = case_cfg(kw)
    n = len(kw["layout"])
    _, env, actions = F.cpu_twin(cm, cfg, kw["seed"], data)
    z = np.zeros((STEPS, n, 5), np.int64)
    for t in range(STEPS):
        for e in range(n):
            z[t, e] = row_zones(cm, cfg, env.state[e, F.qpos_cols(cm)], env.state[e, F.qvel_cols(cm)])
        env.step(actions[t])
    return z


def check_zones(name, cm, data) -> None:
    """The case's premise, on the CPU twin."""
    kw = CASES[name]
    z = twin_zones(name, cm, data)
    n = z.shape[1]
    nofl = sum(1 for d in range(cm.nv) if float(cm.cmodel.dof_frictionloss[d]) == 0.0)
    assert nofl == 6 and cm.nv - nofl == 20, f"{name}: {nofl} dofs without friction loss"
    print(f"  {name}: (below, above, linear, limit rows, contact rows) per step and env {z.tolist()}")
    for w in range(0, n, 2):
        wave = z[:, w:w + 2, :3].sum(1)  # [STEPS, 3]
        assert (wave > 0).all(1).any(), f"{name}: envs {w}.. never hold all three zones in one step: {wave.tolist()}"
    for e, kind in enumerate(kw["layout"]):
        if kind == "A":
            assert z[0, e, 4] == 0 and z[0, e, 3] == 0, f"{name}: env {e} (A) starts with contact or limit rows"
        else:
            assert z[0, e, 3] == 1, f"{name}: env {e} (B) starts with {z[0, e, 3]} limit rows"
            assert z[:, e, 4].max() > 0, f"{name}: env {e} (B) never in contact"
    if "A" in kw["layout"] and "B" in kw["layout"]:
        both = [(z[t, 0, 4] == 0) != (z[t, 1, 4] == 0) for t in range(STEPS)]
        assert any(both), f"{name}: no step with one env of the first wave in contact and one airborne"


def check_case(name, data, cm, zones=True) -> None:
    """What makes the fixture worth having, on the run that is about to be recorded (or replayed)."""
    assert np.isfinite(data["states"][:, :, F.motion_cols(cm)]).all(), f"{name}: non-finite state"
    assert (data["solver_iters"] > 0).all(), f"{name}: a step without a solver iteration"
    assert not data["done"].any(), f"{name}: an env terminated"
    if zones:
        check_zones(name, cm, data)


if __name__ == "__main__":
    F.main(sys.modules[__name__])
