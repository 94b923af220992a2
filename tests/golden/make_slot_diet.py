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
issue slots, before any kernel edit.
"""

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "ksim-gym-zbot_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_engine_bits as G  # noqa: E402
import make_smooth_bits as S  # noqa: E402

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
    from zbot_amd import default_config  # noqa: PLC0415

    extra = dict(obs_noise=False, autoreset=False) if kw.get("plain") else {}
    if "iterations" in kw:
        extra["iterations"] = kw["iterations"]
    return default_config(solver=kw["solver"], **extra)


def case_noise(kw):
    z = np.random.default_rng(kw["seed"]).standard_normal((STEPS, len(kw["layout"]), 20))
    return np.clip(np.rint(z * 32.0), -127, 127).astype(np.int8)


def start_state(cm, kw, st):
    """Reset state rows `st` [n, S_END] moved to the case's start: hinge velocities for every env,
    A lifted, B with one hinge past its limit; the warm start zero."""
    import collider_util as U  # noqa: PLC0415
    from zbot_amd import cstructs as cs  # noqa: PLC0415

    st = st.copy()
    n = len(kw["layout"])
    z = np.random.default_rng(kw["seed"] + 1000).standard_normal((n, 20))
    vel = (np.float32(VEL_SIGMA) * np.clip(np.rint(z * 32.0), -127, 127).astype(np.float32) / np.float32(32.0))
    for e, kind in enumerate(kw["layout"]):
        st[e] = st[0]  # the same reset row for every env: A and B differ only as described
        st[e, 32:58] = 0.0
        st[e, 38:58] = vel[e]
        if kind == "A":
            st[e, 2] += np.float32(LIFT)
        else:
            b = S.hinge(cm, LIMIT_JOINT[0])
            st[e, b.qposadr] = np.float32(b.jrange[1] + S.PAST)
            # down to the floor: the soles' lowest point 1 mm below it
            st[e, 2] -= np.float32(U.lowest_point(cm, st[e, :27].astype(np.float64)) + 1e-3)
    st[:, cs.S_QACCW:cs.S_QACCW + 32] = 0.0
    return st


def run_engine(cm, cfg, kw, actions, lib_path=None, swap=False):
    """One engine through the case's steps; the arrays a fixture keeps. swap: envs in reverse order
    (state rows, randomization rows and actions), the results reversed back."""
    import torch  # noqa: PLC0415
    from zbot_amd.engine import HipEngine  # noqa: PLC0415

    n = len(kw["layout"])
    eng = HipEngine(cm, cfg, n, seed=kw["seed"], lib_path=lib_path)
    eng.reset()
    st = start_state(cm, kw, eng.get_state().cpu().numpy())
    rnd = eng.get_rand().cpu().numpy()
    rnd[:] = rnd[0]
    o = slice(None, None, -1) if swap else slice(None)
    eng.set_state(torch.from_numpy(np.ascontiguousarray(st[o])))
    eng.set_rand(torch.from_numpy(np.ascontiguousarray(rnd[o])))
    rows = {"reward": [], "done": [], "success": [], "solver_iters": [], "states": []}
    out = None
    for a in actions:
        out = eng.step(torch.from_numpy(np.ascontiguousarray(a[o])).cuda())
        torch.cuda.synchronize()
        for k in ("reward", "done", "success"):
            rows[k].append(out[k].cpu().numpy()[o].copy())
        rows["solver_iters"].append(eng.solver_iters().cpu().numpy()[o].copy())
        rows["states"].append(eng.get_state().cpu().numpy()[o].copy())
    d = {k: np.stack(v) for k, v in rows.items()}
    d["start_state"] = st
    d["start_rand"] = rnd
    for k, v in out.items():
        d[f"last_{k}"] = v.cpu().numpy()[o].copy()
    return d


def run_case(name, noise_q=None, lib_path=None, swap=False):
    """The arrays of one case, keyed as in its fixture. `noise_q`: the fixture's own (a replay)."""
    from zbot_amd import compile_model  # noqa: PLC0415

    kw = CASES[name]
    cm = compile_model()
    if noise_q is None:
        noise_q = case_noise(kw)
    actions = G.case_actions(cm, noise_q)
    data = {"noise_q": noise_q}
    data.update(run_engine(cm, case_cfg(kw), kw, actions, lib_path=lib_path, swap=swap))
    return data, cm


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
    import oracle as O  # noqa: PLC0415

    O.build()
    kw = CASES[name]
    cfg = case_cfg(kw)
    n = len(kw["layout"])
    env = O.OracleEnv(cm.cmodel, cfg, n, seed=kw["seed"])
    env.reset()
    env.state[:] = data["start_state"]
    env.rand[:] = data["start_rand"]
    actions = G.case_actions(cm, data["noise_q"])
    z = np.zeros((STEPS, n, 5), np.int64)
    for t in range(STEPS):
        for e in range(n):
            z[t, e] = row_zones(cm, cfg, env.state[e, :27], env.state[e, 32:58])
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
    assert np.isfinite(data["states"][:, :, :58]).all(), f"{name}: non-finite state"
    assert (data["solver_iters"] > 0).all(), f"{name}: a step without a solver iteration"
    assert not data["done"].any(), f"{name}: an env terminated"
    if zones:
        check_zones(name, cm, data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", help="case names to (re)generate; default: all")
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--lib", default=None, help="the library to record with (default: the product build)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for name in CASES:
        if a.cases and name not in a.cases:
            continue
        data, cm = run_case(name, lib_path=a.lib and os.path.abspath(a.lib))
        check_case(name, data, cm)
        path = os.path.join(a.out, f"slot_diet_{name}.npz")
        np.savez_compressed(path, **data)
        kb = os.path.getsize(path) / 1024
        assert kb < 100, f"{path}: {kb:.0f} KB"
        print(f"{name}: {len(data)} arrays, {kb:.0f} KB")


if __name__ == "__main__":
    main()
