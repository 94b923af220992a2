"""Record the HIP engine's own output bits (needs the GPU): tests/golden/engine_bits_<case>.npz.

    python tests/golden/make_engine_bits.py [--out DIR] [--lib libzbot_hip.so] [case ...]

The other goldens pin the CPU oracle, and the engine is held to them within a tolerance. These
pin the engine itself, bit for bit, so that a change meant to leave every rounding alone (fewer
instructions, another schedule) can be told from one that does not. tests/test_gpu_engine_bits.py
replays every case and compares with array_equal.

A case runs 64 envs from reset with a fixed seed, and its first three envs again as an engine of
n = 3 (an odd n: the last wave's second team is the ghost copy past n). It keeps the actions' noise
(int8, in steps of 1/32: the float32 actions follow from it exactly), the
per-step reward / done / success / solver_iters() rows, get_state() and get_rand() after the last
step and every output of the last step. The collider and sole-pair cases start from states in
which the rows in question exist (tests/collider_util.py), set with set_state() after the reset.

Regenerating: when a change alters the engine's rounding on purpose, check it against the
oracle-based tests first (tests/test_gpu_parity.py, tests/test_gpu_colliders.py), then run this
script on the GPU at that commit and commit the new files together with the change; main() refuses
to write a case that lost what makes it worth having (an episode end, a solve below the iteration
cap, second-bank rows, a contact in every extra contact-row bank of the case's kernel: bank_envs).
What the engine-bit families share is in tests/bit_fixtures.py.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/, when run as a script
import bit_fixtures as F  # noqa: E402
import collider_util as U  # noqa: E402
from zbot_amd import default_config  # noqa: E402

FAMILY, MAX_KB = "engine_bits", 300
N = 64
N_ODD = 3  # the first three envs again, alone

CASES = {
    # (a) the headline kernel: CG, the default model
    "cg": dict(steps=40, seed=21),
    # (b) mj_Euler's implicit damping (the ED kernels)
    "cg_eulerdamp": dict(steps=40, seed=22, eulerdamp=True),
    # (c) pushes and per-env domain randomization
    "cg_push_rand": dict(steps=40, seed=23, push=True, randomize=True),
    # (d) Newton
    "newton": dict(steps=8, seed=24, solver="newton"),
    # (e) the second contact-row bank: floor colliders beyond the soles, from touching states
    "cg_limbs": dict(steps=8, seed=25, model="zbot_like_limbs.xml", start="touching"),
    "cg_many": dict(steps=8, seed=26, model="zbot_like_many.xml", start="touching"),
    # (f) the sole pair, from states with the soles crossed
    "cg_sole_pair": dict(steps=8, seed=27, model="sole_pair", start="crossing"),
    # (g) the kernels no case above runs: the cylinder / ellipsoid rules (XG 2), the pair beside one
    # and two floor banks (XG 4, 6), the nine colliders with the unfolded solve_cg masks, and Newton
    # (hessian_factor, hsolve_pair) with every kind of extra bank. The pair models lie or stand on
    # the floor with the soles crossed. check_case counts, per extra bank, the envs that fill it
    "cg_cyl": dict(steps=8, seed=28, model="zbot_like_cyl.xml", start="touching"),
    "cg_limbs_pair": dict(steps=8, seed=29, model="limbs_pair", start="crossing_touching"),
    "cg_many_pair": dict(steps=8, seed=30, model="many_pair", start="crossing_touching"),
    "cg_many_eulerdamp": dict(steps=8, seed=31, model="zbot_like_many.xml", start="touching", eulerdamp=True),
    "newton_limbs": dict(steps=8, seed=32, solver="newton", model="zbot_like_limbs.xml", start="touching"),
    "newton_many": dict(steps=8, seed=33, solver="newton", model="zbot_like_many.xml", start="touching"),
    "newton_sole_pair": dict(steps=8, seed=34, solver="newton", model="sole_pair", start="crossing_touching"),
    "newton_many_pair": dict(steps=8, seed=35, solver="newton", model="many_pair", start="crossing_touching"),
}
# the cases recorded before the per-bank count existed: their fixtures stay, check_case only prints it
BANKS_PRINTED_ONLY = ("cg_limbs", "cg_many", "cg_sole_pair")


def inputs(name):
    kw = CASES[name]
    return {"noise_q": F.action_noise(kw["seed"], kw["steps"], N)}


def start_qpos(cm, start, seed):
    """[N, 27] qpos of a case that does not start from the reset state (None: it does)."""
    if start is None:
        return None
    if start == "touching":
        return U.touching_states(cm, N, seed).astype(np.float32)
    if start == "crossing_touching":
        return U.crossing_touching_states(cm, N, seed).astype(np.float32)
    return U.crossing_states(cm, N, seed, air=False).astype(np.float32)


def second_bank_envs(cm, qpos) -> int:
    """Envs whose start state has a floor contact on a collider beyond the two soles."""
    return sum(any(len(cons) > 0 for cons in U.contacts(cm, q.astype(np.float64))[2:]) for q in qpos)


def bank_envs(cm, cfg, qpos) -> list[tuple[str, int]]:
    """Per extra contact-row bank of the model's kernel, in bank order: what it holds and how many
    envs' start states put a contact into it. A floor bank takes two of the colliders beyond the
    soles within reach of the floor, in geom order (collider_util.bank2_candidates; a model with at
    most two such colliders has one floor bank, any other two), and is filled by a floor contact on
    one of its two (collider_util.contacts); the sole pair has the bank after the floor banks, filled
    when the oracle's constraint rows hold a contact row without root columns (the pair's only).
    The oracle is the repository's own CPU one (oracle/oracle.py, its libraries built by
    __graft_entry__.build() or on first use by oracle.build()); nothing outside the tree is read."""
    m = cm.cmodel
    q64 = [q.astype(np.float64) for q in qpos]
    out = []
    if m.ngeom > 2:
        cand = [U.bank2_candidates(cm, q) for q in q64]
        con = [U.contacts(cm, q, margin=float(m.floor_margin)) for q in q64]
        for b in range(1 if m.ngeom <= 4 else 2):
            out.append((f"floor bank {b + 1}", sum(any(len(con[e][g]) > 0 for g in cand[e][2 * b:2 * b + 2])
                                                   for e in range(len(q64)))))
    if m.npair:
        import oracle as O  # noqa: PLC0415

        O.build()
        rows = [O.constraint_problem(m, cfg, q, np.zeros(cm.nv, np.float32), precision="f64") for q in qpos]
        out.append(("sole pair", sum(bool(((p["type"] == 2) & (np.abs(p["J"][:, :6]).max(1) == 0)).any()) for p in rows)))
    return out


def run_case(name, noise_q=None, lib_path=None):
    """The arrays of one case, keyed as in its fixture. `noise_q`: the fixture's own (a replay)."""
    kw = CASES[name]
    cm = F.model(kw.get("model"))
    cfg = default_config(solver=kw.get("solver", "cg"), eulerdamp=kw.get("eulerdamp", False),
                         push=kw.get("push", False), randomize=kw.get("randomize", False))
    if noise_q is None:
        noise_q = inputs(name)["noise_q"]
    qpos = start_qpos(cm, kw.get("start"), kw["seed"])
    data = {"noise_q": noise_q}
    for tag, n in (("", N), ("odd_", N_ODD)):
        data.update(F.tagged(tag, F.run(cm, cfg, n, kw["seed"], F.actions(cm, noise_q), start=F.rest_at(cm, qpos),
                                        lib_path=lib_path, final=("final_state", "final_rand", "last"))))
    return data, cm, cfg, qpos


def check_case(name, data, cm, cfg, qpos) -> None:
    """What makes the fixture worth having, on the run that is about to be recorded."""
    kw = CASES[name]
    assert np.isfinite(data["final_state"][:, F.motion_cols(cm)]).all(), f"{name}: non-finite state"
    if name == "cg":
        # a control step: n_substeps solves of at most cfg.iterations iterations (a reset pass adds one)
        cap = cfg.n_substeps * cfg.iterations
        ends = int(data["done"].sum())
        below = int((data["solver_iters"] < cap).sum())
        print(f"  {name}: {ends} episode ends, {below} of {data['solver_iters'].size} env-steps below the cap total {cap}")
        assert ends >= 1, f"{name}: no episode end in {kw['steps']} steps (the reset and ghost passes did not run)"
        assert below >= 1, f"{name}: every solve ran to the iteration cap"
    if kw.get("start") == "touching":
        nb = second_bank_envs(cm, qpos)
        print(f"  {name}: {nb} of {N} envs start with second-bank rows")
        assert nb >= 1, f"{name}: no env has rows in the second bank"
    if kw.get("start") is not None:
        banks = bank_envs(cm, cfg, qpos)
        print(f"  {name}: envs that start with a contact in " + ", ".join(f"{what}: {k} of {N}" for what, k in banks))
        if name not in BANKS_PRINTED_ONLY:
            assert all(k >= 1 for _, k in banks), f"{name}: a bank of its kernel stays empty ({banks})"


if __name__ == "__main__":
    F.main(sys.modules[__name__])
