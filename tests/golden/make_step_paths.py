"""Record the HIP engine's bits on the step kernel's paths that the other fixtures leave dark (needs
the GPU): tests/golden/step_paths_<case>.npz.

    python tests/golden/make_step_paths.py [--out DIR] [--lib libzbot_hip.so] [case ...]

engine_bits, smooth_bits and const_staging pin 64-env runs, n = 2 and 3, resets and ghost passes,
the limit row in every env of a wave, and non-default solver fields. Three things stay open that a
rewrite of the solver loop's lane bookkeeping or of the step end can get wrong:

  n1_*          n = 1: the wave's second team is a ghost copy of env 0 for the whole launch and
                stores nothing. CG and Newton, four control steps. No env terminates (checked on
                the done flags), so the only ghost is the team past n.
  limit_one_cg  n = 2 with one limited hinge of env 0 0.05 rad past its range and env 1 inside all
                of its ranges: the wave takes the line search's copy with the joint-limit row while
                one team's row is absent. Two control steps. Checked on debug_forward's row counts
                of the start state: rows beyond the contacts' and the friction-loss rows are 1 for
                env 0 and 0 for env 1.
  outputs_cg    n = 2, one control step from the same start on three engines: every output
                (`full`), without obs_extra (`noextra`, step(extras=False)) and without
                reward_terms (`noterms`, step(terms=False)). A null pointer switches that output's
                stores off at the step end; the buffer then keeps its zeros (checked) and every
                other output keeps its bits.

Observation noise stays on and autoreset stays on, as in the headline configuration. main() refuses
to write a case whose premise fails. What the engine-bit families share is in tests/bit_fixtures.py.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/, when run as a script
import bit_fixtures as F  # noqa: E402
from zbot_amd import default_config  # noqa: E402

FAMILY, MAX_KB = "step_paths", 100
LIMIT_JOINT = ("left_elbow_roll", 1)  # env 0 of limit_one_cg: past the upper bound
OUTPUT_MODES = (("full_", dict()), ("noextra_", dict(extras=False)), ("noterms_", dict(terms=False)))

CASES = {
    "n1_cg": dict(seed=41, solver="cg", n=1, steps=4),
    "n1_newton": dict(seed=42, solver="newton", n=1, steps=4),
    "limit_one_cg": dict(seed=43, solver="cg", n=2, steps=2, limit_one=True),
    "outputs_cg": dict(seed=44, solver="cg", n=2, steps=1, modes=True),
}


def inputs(name):
    kw = CASES[name]
    return {"noise_q": F.action_noise(kw["seed"], kw["steps"], kw["n"])}


def start_state(cm, kw, st):
    """The reset state rows `st`, env 0 moved past its joint limit for limit_one_cg."""
    st = st.copy()
    if kw.get("limit_one"):
        F.set_past(cm, st[0], *LIMIT_JOINT)
    return st


def extra_rows(cm, dbg):
    """Per env: constraint rows beyond the contacts' four each and the friction-loss rows."""
    nfl = sum(1 for d in range(cm.nv) if float(cm.cmodel.dof_frictionloss[d]) > 0.0)
    nefc = dbg[:, F.DBG_MISC + 0].astype(np.int64)
    ncon = dbg[:, F.DBG_MISC + 1].astype(np.int64)
    return nefc - 4 * ncon - nfl, nefc, ncon


def run_mode(cm, cfg, kw, actions, lib_path=None, **step_kw):
    """One engine through the case's steps; the arrays a fixture keeps (every output buffer)."""
    r = F.Run(cm, cfg, kw["n"], kw["seed"], actions, start=lambda st: start_state(cm, kw, st), lib_path=lib_path,
              step_kw=step_kw, final=("start_state", "final_state", "last"))
    # the buffers a switched-off output leaves alone start from zeros
    for k in ("obs_extra", "reward_terms"):
        getattr(r.eng, k).zero_()
    d = {}
    if kw.get("limit_one"):
        st = r.torch.from_numpy(r.start_state)
        d["start_dbg_misc"] = r.eng.debug_forward(st).cpu().numpy()[:, F.DBG_MISC:F.DBG_MISC + 2].copy()
        r.eng.set_state(st)
    d.update(r.run())
    return d


def run_case(name, noise_q=None, lib_path=None):
    """The arrays of one case, keyed as in its fixture. `noise_q`: the fixture's own (a replay)."""
    kw = CASES[name]
    cm = F.model()
    cfg = default_config(solver=kw["solver"])
    if noise_q is None:
        noise_q = inputs(name)["noise_q"]
    data = {"noise_q": noise_q}
    for tag, step_kw in (OUTPUT_MODES if kw.get("modes") else (("", dict()),)):
        data.update(F.tagged(tag, run_mode(cm, cfg, kw, F.actions(cm, noise_q), lib_path, **step_kw)))
    return data, cm


def check_case(name, data, cm) -> None:
    """The case takes its path, on the run that is about to be recorded (or replayed)."""
    kw = CASES[name]
    tags = [t for t, _ in OUTPUT_MODES] if kw.get("modes") else [""]
    for tag in tags:
        assert np.isfinite(data[tag + "final_state"][:, F.motion_cols(cm)]).all(), f"{name}: non-finite state"
        assert (data[tag + "solver_iters"] > 0).all(), f"{name}: a step without a solver iteration"
    if kw["n"] == 1:
        assert data["done"].shape == (kw["steps"], 1) and not data["done"].any(), f"{name}: env 0 terminated"
    if kw.get("limit_one"):
        dbg = np.zeros((kw["n"], F.DBG_MISC + 2), np.float32)
        dbg[:, F.DBG_MISC:] = data["start_dbg_misc"]
        extra, nefc, ncon = extra_rows(cm, dbg)
        print(f"  {name}: nefc {nefc.tolist()} ncon {ncon.tolist()} rows beyond contacts and friction loss {extra.tolist()}")
        assert extra.tolist() == [1, 0], f"{name}: limit rows per env {extra.tolist()}, wanted [1, 0]"
        assert not data["done"].any(), f"{name}: an env terminated"
    if kw.get("modes"):
        assert data["full_last_obs_extra"].any() and data["full_last_reward_terms"].any(), f"{name}: full outputs empty"
        assert not data["noextra_last_obs_extra"].any(), f"{name}: extras=False wrote obs_extra"
        assert data["noextra_last_reward_terms"].any()
        assert not data["noterms_last_reward_terms"].any(), f"{name}: terms=False wrote reward_terms"
        assert data["noterms_last_obs_extra"].any()
        for k in ("last_obs_actor", "last_obs_critic", "last_reward", "last_done", "final_state"):
            for tag in ("noextra_", "noterms_"):
                assert np.array_equal(data[tag + k], data["full_" + k], equal_nan=True), f"{name}: {tag}{k} moved"


if __name__ == "__main__":
    F.main(sys.modules[__name__])
