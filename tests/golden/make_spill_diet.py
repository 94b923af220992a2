"""Record the HIP engine's bits on the CG wave's exit paths (needs the GPU):
tests/golden/spill_diet_<case>.npz.

    python tests/golden/make_spill_diet.py [--out DIR] [--lib libzbot_hip.so] [case ...]

The CG line search evaluates its slope up to eight times per call, and the two teams of a wave (two
envs) leave it after different numbers of evaluations. A rewrite of how a wave leaves (the exec
regions of the unrolled evaluations, alpha and the bracket kept per lane) can mix up the lanes of a
team that is done with those of one that still searches, and the other fixtures do not say which
exits they hold. These cases do, three control steps each from touching states:

  pair_cg     n = 2, [A, B] as in make_slot_diet.py: A lifted 0.1 m (airborne, no contact row), B on
              the floor with one limited hinge past its range (the wave runs the line search's copy
              with the joint-limit row, one team's row absent). Every hinge moves at about 1 rad/s.
              No observation noise and no automatic reset, so that nothing depends on the env index:
              the test replays [A, B] and [B, A] against the one fixture, the rows swapped.
  n1_cg       n = 1, [B]: the wave's second team is the ghost past n. Default config.
  n3_cg       n = 3, [A, B, A]: two waves, the second with a ghost. The pair's config.
  generic_cg  the pair with iterations = 3: the generic CG kernel (solver fields read from the handle),
              which the change this fixture was made for must leave untouched.
  reset_cg    n = 3, [B, H, B] under the default config (observation noise and automatic reset on): H
              starts 0.5 m above the reset height, past the task's height bound, so it terminates at
              the first control step and runs the ghost pass and the reset re-entry inside the window.
  rest_cg     n = 2, [F, B] on a copy of the default model without gravity: F floats at rest with every
              servo holding its target, so that its smooth force, its rows' values and the solver's
              gradient are exact zeros and every line search of it returns at its entry test (the
              slope is not negative), beside a team that searches. The pair's config; replayed in
              both orders.

The premises are checked on the CPU twin: oracle.OracleEnv stepped through the same actions from the
same state and randomization rows, and at every pre-step state a float64 replay of the oracle's CG
(zb_oracle.c solve_cg / line_search, the same statements) on oracle.constraint_problem's rows, which
counts the evaluations of every line search (0: returned at its entry test). main() and the test
refuse the fixtures unless
  - the counts hold 1, 2, a value from 3 to 7, and the cap of 8;
  - some wave has its two teams leave the same iteration's line search after different counts;
  - rest_cg's F returns at the entry test (count 0, no iteration) while its partner searches;
  - A starts without contact or limit row and B with one limit row and, at some step, contact rows,
    one env of a wave in contact while the other is airborne;
  - reset_cg's H, and no other env, terminates at the first control step (the twin's done flags and
    the recorded ones);
  - n = 1 and n = 3 are among the sizes.
The twin's counts are a premise about the states, not a bit reference: the engine solves the same
problems in float32 and with its servo torques, and may take an evaluation more or less somewhere.

The fixtures were recorded with the library of commit 57ba670 ("Policy shape per handle: GRU depth
and mixture count in HIP"), the parent of the change to the line search's exit path, before any
kernel edit. What the engine-bit families share is in tests/bit_fixtures.py.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/, when run as a script
import bit_fixtures as F  # noqa: E402
import make_slot_diet as D  # noqa: E402  (the A and B rows, the pair's config, the layout's run)
from zbot_amd import cstructs as cs  # noqa: E402

FAMILY, MAX_KB = "spill_diet", 100
STEPS = 3
HIGH = 0.5  # m above the reset height: past the task's height bound

CASES = {
    "pair_cg": dict(seed=65, layout="AB", plain=True),
    "n1_cg": dict(seed=64, layout="B"),
    "n3_cg": dict(seed=63, layout="ABA", plain=True),
    "generic_cg": dict(seed=65, layout="AB", plain=True, iterations=3),
    "reset_cg": dict(seed=66, layout="BHB"),
    "rest_cg": dict(seed=67, layout="FB", plain=True, nogravity=True),
}
for _kw in CASES.values():
    _kw["solver"] = "cg"
SWAPPED = [n for n, kw in CASES.items() if kw.get("plain") and len(kw["layout"]) == 2]



def case_model(kw):
    return F.model("nogravity" if kw.get("nogravity") else None)


def inputs(name):
    kw = CASES[name]
    q = F.action_noise(kw["seed"], STEPS, len(kw["layout"]))
    for e, kind in enumerate(kw["layout"]):
        if kind == "F":
            q[:, e] = 0  # the held target: the joint biases themselves
    return {"noise_q": q}


def start_state(cm, kw, st):
    """Reset state rows `st` moved to the case's start. A, B: make_slot_diet.start_state. H: B lifted
    HIGH. F: at rest 0.1 m above the reset height, every hinge and its servo's plan at the joint bias
    (the action of zero noise), the warm start zero."""
    lay = kw["layout"]
    out = D.start_state(cm, dict(kw, layout="".join("A" if k == "A" else "B" for k in lay)), st)
    m = cm.cmodel
    for e, kind in enumerate(lay):
        if kind == "H":
            F.lift(out[e], HIGH)
        elif kind == "F":
            out[e] = st[0]
            F.lift(out[e], D.LIFT)
            out[e, cs.S_QVEL:cs.S_QACCW] = 0.0
            out[e, cs.S_QACCW:cs.S_PLAN_POS] = 0.0
            for a in range(m.nu):
                tgt = np.float32(m.joint_bias[a])
                out[e, m.dof_qposadr[m.act_dof[a]]] = tgt
                out[e, cs.S_PLAN_POS + a] = tgt
                out[e, cs.S_PLAN_VEL + a] = 0.0
                out[e, cs.S_PLAN_TAU + a] = 0.0
    return out


def run_case(name, noise_q=None, lib_path=None, swap=False):
    """The arrays of one case, keyed as in its fixture. `noise_q`: the fixture's own (a replay). A case
    that is not `plain` keeps every env's own randomization row."""
    kw = CASES[name]
    cm = case_model(kw)
    if noise_q is None:
        noise_q = inputs(name)["noise_q"]
    return D.run_layout(cm, kw, noise_q, start_state, bool(kw.get("plain")), lib_path, swap), cm


# ---- the CPU twin's line searches ----

def _efc(typ, Dr, R, fl, jar):
    """zb_oracle.c efc_eval over the rows: (cost, force)."""
    cost, force = 0.0, np.zeros_like(jar)
    for r in range(len(jar)):
        if typ[r] == 0:
            rf = R[r] * fl[r]
            if jar[r] <= -rf:
                force[r] = fl[r]
                cost += -fl[r] * (0.5 * rf + jar[r])
                continue
            if jar[r] >= rf:
                force[r] = -fl[r]
                cost += fl[r] * (jar[r] - 0.5 * rf)
                continue
        elif not jar[r] < 0:
            continue
        force[r] = -Dr[r] * jar[r]
        cost += 0.5 * Dr[r] * jar[r] * jar[r]
    return cost, force


def ls_counts(p, qaccw, cfg, meaninertia):
    """Evaluations of every line search of zb_oracle.c's solve_cg on the problem `p`
    (oracle.constraint_problem), in float64: one entry per iteration, 0 for a line search that
    returned at its entry test."""
    M = p["qM"].astype(np.float64)
    if not np.allclose(M, M.T):
        M = np.tril(M) + np.tril(M, -1).T
    nv = M.shape[0]
    J, Dr, R, aref, fl = (p[k].astype(np.float64) for k in ("J", "D", "R", "aref", "floss"))
    typ = p["type"]
    if len(Dr) == 0:
        return []
    qs = p["qacc_smooth"].astype(np.float64)
    fs = M @ qs

    def total(x):
        return 0.5 * (M @ x - fs) @ (x - qs) + _efc(typ, Dr, R, fl, J @ x - aref)[0]

    x = np.asarray(qaccw, np.float64)[:nv].copy()
    if total(x) > total(qs):
        x = qs.copy()
    Ma, jar = M @ x, J @ x - aref
    scale = 1.0 / (meaninertia * max(nv, 1))

    def update():
        c, f = _efc(typ, Dr, R, fl, jar)
        return 0.5 * (Ma - fs) @ (x - qs) + c, Ma - fs - J.T @ f

    cost, grad = update()
    mg = np.linalg.solve(M, grad)
    search = -mg
    counts = []
    for _ in range(cfg.iterations):
        Mv, Jv = M @ search, J @ search
        c1, c2 = search @ (Ma - fs), search @ Mv

        def ev(alpha):
            g1, g2 = c1 + alpha * c2, c2
            xx = jar + alpha * Jv
            for r in range(len(xx)):
                if Jv[r] == 0:
                    continue
                if typ[r] == 0:
                    rf = R[r] * fl[r]
                    if xx[r] <= -rf:
                        g1 -= fl[r] * Jv[r]
                        continue
                    if xx[r] >= rf:
                        g1 += fl[r] * Jv[r]
                        continue
                elif not xx[r] < 0:
                    continue
                g1 += Dr[r] * xx[r] * Jv[r]
                g2 += Dr[r] * Jv[r] * Jv[r]
            return g1, g2

        d1, d2 = ev(0.0)
        if not d1 < 0 or not d2 > 0:
            counts.append(0)
            break
        gtol = cfg.ls_tolerance * (-d1)
        lo, hi, alpha, n = 0.0, -1.0, -d1 / d2, 0
        for _k in range(cfg.ls_iterations):
            d1, d2 = ev(alpha)
            n += 1
            if abs(d1) <= gtol:
                break
            if d1 < 0:
                lo = alpha
            else:
                hi = alpha
            an = alpha - d1 / d2
            if not an > lo or (hi >= 0 and not an < hi):
                an = 0.5 * (lo + (hi if hi >= 0 else 2 * alpha))
            alpha = an
        counts.append(n)
        if alpha == 0:
            break
        x, Ma, jar = x + alpha * search, Ma + alpha * Mv, jar + alpha * Jv
        old, gold, mgold = cost, grad, mg
        cost, grad = update()
        if scale * (old - cost) < cfg.tolerance or scale * np.sqrt(grad @ grad) < cfg.tolerance:
            break
        mg = np.linalg.solve(M, grad)
        beta = max((grad @ (mg - mgold)) / max(gold @ mgold, 1e-15), 0.0)
        search = -mg + beta * search
    return counts


def twin(name, data):
    """The CPU twin along the case: (counts[t][e]: ls_counts of the pre-step states; rows [STEPS, n, 2]:
    limit rows and contact rows there; done [STEPS, n])."""
    kw = CASES[name]
    cm, cfg = case_model(kw), D.case_cfg(kw)
    n = len(kw["layout"])
    O, env, actions = F.cpu_twin(cm, cfg, kw["seed"], data)
    counts, rows, done = [], np.zeros((STEPS, n, 2), np.int64), np.zeros((STEPS, n), bool)
    for t in range(STEPS):
        row = []
        for e in range(n):
            w = env.state[e, cs.S_QACCW:cs.S_QACCW + cm.nv]
            p = O.constraint_problem(cm.cmodel, cfg, env.state[e, F.qpos_cols(cm)], env.state[e, F.qvel_cols(cm)], qaccw=w,
                                     precision="f32")
            row.append(ls_counts(p, w, cfg, float(cm.cmodel.meaninertia)))
            rows[t, e] = int((p["type"] == 1).sum()), int((p["type"] == 2).sum())
        counts.append(row)
        done[t] = env.step(actions[t])["done"] != 0
    return counts, rows, done


def differing_exits(counts, n):
    """(step, wave, iteration) where the wave's two teams both search and leave after different counts."""
    out = []
    for t, row in enumerate(counts):
        for w in range(0, n - 1, 2):
            for k, (a, b) in enumerate(zip(row[w], row[w + 1])):
                if a != b and a > 0 and b > 0:
                    out.append((t, w // 2, k))
    return out


def check_twin(name, data):
    """The case's premises on the CPU twin; returns the set of evaluation counts it holds and whether
    one of its waves leaves a line search at two different counts."""
    kw = CASES[name]
    lay = kw["layout"]
    n = len(lay)
    counts, rows, done = twin(name, data)
    print(f"  {name}: evaluations per line search, per step and env {counts}")
    print(f"  {name}: (limit rows, contact rows) per step and env {rows.tolist()}  done {done.astype(int).tolist()}")
    for e, kind in enumerate(lay):
        if kind == "A":
            assert rows[0, e, 0] == 0 and rows[0, e, 1] == 0, f"{name}: env {e} (A) starts with limit or contact rows"
        elif kind in "BH":
            assert rows[0, e, 0] == 1, f"{name}: env {e} ({kind}) starts with {rows[0, e, 0]} limit rows"
        if kind == "B":
            assert rows[:, e, 1].max() > 0, f"{name}: env {e} (B) never in contact"
        if kind == "H":
            assert done[0, e], f"{name}: env {e} (H) does not terminate at the first control step"
            assert rows[0, e, 1] == 0, f"{name}: env {e} (H) starts in contact"
        else:
            assert not done[:, e].any(), f"{name}: env {e} ({kind}) terminated"
        if kind == "F":
            assert all(c == [0] for c in (counts[t][e] for t in range(STEPS))), \
                f"{name}: env {e} (F) searches: {[counts[t][e] for t in range(STEPS)]}"
            assert (rows[:, e] == 0).all(), f"{name}: env {e} (F) has limit or contact rows"
            o = e ^ 1
            assert all(len(counts[t][o]) > 0 and counts[t][o][0] > 0 for t in range(STEPS)), f"{name}: F's partner does not search"
    if "A" in lay and "B" in lay:
        mixed = [(rows[t, 0, 1] == 0) != (rows[t, 1, 1] == 0) for t in range(STEPS)]
        assert any(mixed), f"{name}: no step with one env of the first wave in contact and one airborne"
        assert rows[0, 0, 0] != rows[0, 1, 0], f"{name}: the first wave's teams both have a limit row, or neither"
    held = {c for row in counts for env in row for c in env}
    return held, bool(differing_exits(counts, n))


def check_all(held, differ, sizes) -> None:
    """The premises that the fixtures hold together. held, differ: per case, from check_twin."""
    every = set().union(*held.values())
    print(f"  evaluation counts held: {sorted(every)}; waves with differing exits in {sorted(k for k, v in differ.items() if v)}")
    assert {0, 1, 2, 8} <= every, f"the fixtures hold the evaluation counts {sorted(every)}: 0, 1, 2 and 8 are wanted"
    assert every & {3, 4, 5, 6, 7}, f"the fixtures hold the evaluation counts {sorted(every)}: none from 3 to 7"
    assert any(differ.values()), "no wave leaves a line search at two different counts"
    assert {1, 3} <= set(sizes), f"sizes {sorted(sizes)}: n = 1 and n = 3 are wanted"


def check_case(name, data) -> None:
    """On the run that is about to be recorded (or replayed): finite, and the recorded flags."""
    kw = CASES[name]
    assert np.isfinite(data["states"][:, :, F.motion_cols(case_model(kw))]).all(), f"{name}: non-finite state"
    for e, kind in enumerate(kw["layout"]):
        if kind == "H":
            assert data["done"][0, e], f"{name}: env {e} (H) did not terminate at the first control step"
        else:
            assert not data["done"][:, e].any(), f"{name}: env {e} ({kind}) terminated"
        if kind == "F":
            assert (data["solver_iters"][:, e] == 0).all(), f"{name}: env {e} (F) ran solver iterations"
        elif kind != "H":
            assert (data["solver_iters"][:, e] > 0).all(), f"{name}: env {e} ({kind}): a step without a solver iteration"


def record(names, lib_path=None):
    held, differ = {}, {}
    for name in names:
        data, _ = run_case(name, lib_path=lib_path)
        check_case(name, data)
        held[name], differ[name] = check_twin(name, data)
        yield name, data
    if len(names) == len(CASES):
        check_all(held, differ, {len(kw["layout"]) for kw in CASES.values()})


if __name__ == "__main__":
    F.main(sys.modules[__name__])
