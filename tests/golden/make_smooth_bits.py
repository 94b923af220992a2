"""Record the HIP engine's bits on two paths the engine_bits fixtures do not reach (needs the GPU):
tests/golden/smooth_bits_<case>.npz.

    python tests/golden/make_smooth_bits.py [--out DIR] [--lib libzbot_hip.so] [case ...]

make_engine_bits.py pins the engine on walking and touching robots. By construction those runs
have contact rows in every wave and no joint past its range, so two paths of the once-per-substep
code stay dark: a joint-limit row (make_constraints' r.anyl branch, row_params on a dof row, the
solvers' limit terms) and a wave with no constraint row at all (forward() skips the solver and
keeps qacc_smooth). These cases start in them:

  limit_*       after reset, set_state() puts one limited hinge of each env 0.05 rad past its
                dof_range (env 0 and 2 past the upper bound, env 1 past the lower one).
  air_*         every env starts with its base 0.5 m above the reset height. Free fall over four
                control steps is about 3 cm, so no sole reaches the floor margin.
  airmix_*      the same with the even envs airborne and the odd ones on the floor: one team of a
                wave has rows, its partner has none.
  *_nofloss     the airborne cases again on a copy of the default model whose servos have no friction
                loss. The default model has a friction-loss row on every hinge, so an airborne env
                of it still has dof rows and runs the solver; without them an airborne wave has no
                row and takes the path that skips the solver (solver_iters stays 0, which main()
                checks on the recorded run).

The airborne cases run with autoreset off: the base starts above the task's height bound, and an
automatic reset after the first control step would put the robot back on the floor.

Every case runs four control steps with n = 2 and again with n = 3 (the second wave's other team
is the ghost copy past n), with the CG and the Newton kernels. It keeps what make_engine_bits.py
keeps. main() refuses to write a case whose premise fails; both premises are checked on the CPU
(tests/collider_util.contacts() is empty for an airborne start; the chosen dof is limited and its
start angle lies outside its range). What the engine-bit families share is in tests/bit_fixtures.py.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/, when run as a script
import bit_fixtures as F  # noqa: E402
import collider_util as U  # noqa: E402
from zbot_amd import default_config  # noqa: E402

FAMILY, MAX_KB = "smooth_bits", 300
STEPS = 4
SIZES = (("", 2), ("odd_", 3))
N = 3  # envs of the largest engine
LIFT = 0.5  # m above the reset height
# env -> (joint, +1: past the upper bound, -1: past the lower one)
LIMIT_JOINTS = (("left_elbow_roll", 1), ("right_shoulder_roll", -1), ("right_knee_pitch", 1))

CASES = {}
for _sv in ("cg", "newton"):
    CASES[f"limit_{_sv}"] = dict(seed=31, solver=_sv, start="limit")
    CASES[f"air_{_sv}"] = dict(seed=32, solver=_sv, start="air")
    CASES[f"airmix_{_sv}"] = dict(seed=33, solver=_sv, start="airmix")
    CASES[f"air_{_sv}_nofloss"] = dict(seed=34, solver=_sv, start="air", nofloss=True)
    CASES[f"airmix_{_sv}_nofloss"] = dict(seed=35, solver=_sv, start="airmix", nofloss=True)


def inputs(name):
    return {"noise_q": F.action_noise(CASES[name]["seed"], STEPS, N)}


def airborne(start, e) -> bool:
    return start == "air" or (start == "airmix" and e % 2 == 0)


def start_state(cm, start, st):
    """The reset state rows `st` [n, S_END] moved to the case's start (velocities and warm start zero)."""
    st = st.copy()
    for e in range(st.shape[0]):
        if start == "limit":
            F.set_past(cm, st[e], *LIMIT_JOINTS[e])
        elif airborne(start, e):
            F.lift(st[e], LIFT)
    return F.at_rest(cm, st)


def check_start(name, cm, st) -> None:
    """The case's premise on the start state, on the CPU."""
    kw = CASES[name]
    m = cm.cmodel
    for e in range(st.shape[0]):
        q = st[e, F.qpos_cols(cm)].astype(np.float64)
        ncon = sum(len(cons) for cons in U.contacts(cm, q, margin=float(m.floor_margin)))
        if kw["start"] == "limit":
            joint, side = LIMIT_JOINTS[e]
            b = F.hinge(cm, joint)
            d = b.dofadr
            assert m.dof_limited[d] == 1, f"{name}: {joint} is not limited"
            lo, hi = float(m.dof_range[d][0]), float(m.dof_range[d][1])
            ang = float(st[e, b.qposadr])
            assert (ang > hi) if side > 0 else (ang < lo), f"{name}: env {e} {joint} at {ang} is inside [{lo}, {hi}]"
            others = [h for h in cm.bodies if h.jnt_type == 3 and h is not b and h.jrange is not None
                      and not (h.jrange[0] <= float(st[e, h.qposadr]) <= h.jrange[1])]
            assert not others, f"{name}: env {e} has further joints past their range"
        elif airborne(kw["start"], e):
            assert ncon == 0, f"{name}: env {e} starts airborne with {ncon} floor contacts"
        else:
            low = U.lowest_point(cm, q)
            assert low < 2e-3, f"{name}: env {e} starts {low} m above the floor"
    if kw.get("nofloss"):
        assert all(float(m.dof_frictionloss[d]) == 0.0 for d in range(cm.nv)), f"{name}: friction loss left"


def run_case(name, noise_q=None, lib_path=None):
    """The arrays of one case, keyed as in its fixture. `noise_q`: the fixture's own (a replay)."""
    kw = CASES[name]
    cm = F.model("nofloss" if kw.get("nofloss") else None)
    cfg = default_config(solver=kw["solver"], autoreset=kw["start"] == "limit")
    if noise_q is None:
        noise_q = inputs(name)["noise_q"]
    data = {"noise_q": noise_q}
    for tag, n in SIZES:
        data.update(F.tagged(tag, F.run(cm, cfg, n, kw["seed"], F.actions(cm, noise_q), lib_path=lib_path,
                                        start=lambda st: start_state(cm, kw["start"], st),
                                        final=("start_state", "final_state", "final_rand", "last"))))
    return data, cm


def check_case(name, data, cm) -> None:
    """What makes the fixture worth having, on the run that is about to be recorded."""
    kw = CASES[name]
    for tag, _ in SIZES:
        assert np.isfinite(data[tag + "final_state"][:, F.motion_cols(cm)]).all(), f"{name}: non-finite state"
        check_start(name, cm, data[tag + "start_state"])
        it = data[tag + "solver_iters"]
        print(f"  {name} {tag or 'n2_'}solver_iters per step: {it.tolist()}")
        if kw["start"] == "limit":
            assert (it > 0).all(), f"{name}: a step without a solver iteration"
        if kw.get("nofloss"):
            air = np.array([airborne(kw["start"], e) for e in range(it.shape[1])])
            assert (it[:, air] == 0).all(), f"{name}: an airborne env without friction loss ran the solver"
            assert (it[:, ~air] > 0).all(), f"{name}: an env on the floor ran no solver iteration"


if __name__ == "__main__":
    F.main(sys.modules[__name__])
