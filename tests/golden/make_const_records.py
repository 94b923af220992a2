"""Record the HIP engine's bits per model, for the per-handle constant records (needs the GPU):
tests/golden/const_records_<case>.npz and const_records_handles.npz.

    python tests/golden/make_const_records.py [--out DIR] [--lib libzbot_hip.so] [case ...]

zb_create repacks the model rows that the substep body reads per lane into a record of the handle's
own (csrc/zb_host.h, "lane record"). The other engine-bit fixtures would not see a record built
wrongly for a model other than the default, or one left over from another handle. These were
recorded with the library of the commit before the records existed, whose kernels read the model
itself; tests/test_gpu_const_records.py replays them and compares with array_equal.

A case is one model and configuration: CG and Newton, n = 2 (one full wave) and n = 3 (a wave with
an idle team), three control steps from the touching states of tests/collider_util.py. main()
refuses to write a case in which an env starts without a floor contact: the constraint rows' loads
have to run from the first substep on.

  default, limbs, many, cyl, mesh   the default model and the four collider assets (many: the second
                                    compilation unit)
  eulerdamp                         the implicit-damping kernels
  randomize                         per-env parameters, which live in EnvL::par and not in the record

const_records_handles.npz holds the default and the limbs model (CG, n = 3), each recorded alone,
for the tests with two handles alive at once and with a handle created after another was destroyed.

Regenerating: as for make_engine_bits.py, on the GPU at the commit whose bits are meant.
"""

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "ksim-gym-zbot_amd"), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_const_staging as S  # noqa: E402

NMAX = 3
SIZES = (2, 3)
STEPS = 3
SEED = 55
SOLVERS = ("cg", "newton")
KEYS = ("state", "reward", "done", "solver_iters")
CASES = {
    "default": dict(),
    "limbs": dict(model="zbot_like_limbs.xml"),
    "many": dict(model="zbot_like_many.xml"),
    "cyl": dict(model="zbot_like_cyl.xml"),
    "mesh": dict(model="zbot_like_mesh.xml"),
    "eulerdamp": dict(eulerdamp=True),
    "randomize": dict(randomize=True),
}
HANDLES = ("default", "limbs")  # const_records_handles.npz: CG, n = NMAX
LIB = None  # another build of the library to record from (--lib); None: the product library


def noise():
    """[STEPS, NMAX, 20] int8: N(0, 1) in steps of 1/32 (the fixtures keep it; the actions follow exactly)."""
    z = np.random.default_rng(SEED).standard_normal((STEPS, NMAX, 20))
    return np.clip(np.rint(z * 32.0), -127, 127).astype(np.int8)


def start_qpos(case):
    """[NMAX, 27] float32 touching states of the case's model."""
    import collider_util as U  # noqa: PLC0415

    return U.touching_states(S.model(CASES[case].get("model")), NMAX, SEED).astype(np.float32)


def contact_counts(case, qpos):
    """Per env: floor contacts of the start state, over all colliders."""
    import collider_util as U  # noqa: PLC0415

    cm = S.model(CASES[case].get("model"))
    return [sum(len(c) for c in U.contacts(cm, q.astype(np.float64))) for q in qpos]


class Run:
    """One handle of n envs at its start state; step() takes the next control step and keeps its rows."""

    def __init__(self, case, solver, n, noise_q, qpos):
        import torch  # noqa: PLC0415
        from zbot_amd import cstructs as cs  # noqa: PLC0415
        from zbot_amd import default_config  # noqa: PLC0415
        from zbot_amd.engine import HipEngine  # noqa: PLC0415

        kw = CASES[case]
        self.torch = torch
        cm = S.model(kw.get("model"))
        cfg = default_config(solver=solver, eulerdamp=kw.get("eulerdamp", False), randomize=kw.get("randomize", False))
        self.acts = S.actions(cm, noise_q)[:, :n]
        self.eng = HipEngine(cm, cfg, n, seed=SEED, lib_path=LIB)
        self.eng.reset()
        st = self.eng.get_state().cpu().numpy()
        st[:, :27] = qpos[:n]
        st[:, 32:58] = 0.0
        st[:, cs.S_QACCW:cs.S_QACCW + 32] = 0.0
        self.eng.set_state(torch.from_numpy(st))
        self.rows = {k: [] for k in KEYS}
        self.t = 0

    def step(self):
        torch = self.torch
        out = self.eng.step(torch.from_numpy(np.ascontiguousarray(self.acts[self.t])).cuda())
        self.t += 1
        torch.cuda.synchronize()
        self.rows["state"].append(self.eng.get_state().cpu().numpy())
        self.rows["reward"].append(out["reward"].cpu().numpy().copy())
        self.rows["done"].append(out["done"].cpu().numpy().copy())
        self.rows["solver_iters"].append(self.eng.solver_iters().cpu().numpy())

    def result(self):
        return {k: np.stack(v) for k, v in self.rows.items()}


def run_alone(case, solver, n, noise_q, qpos):
    r = Run(case, solver, n, noise_q, qpos)
    for _ in range(STEPS):
        r.step()
    return r.result()


def run_case(case, solver, noise_q, qpos):
    """{"<solver>_n<n>_<key>": array} of one case and solver."""
    data = {}
    for n in SIZES:
        for k, v in run_alone(case, solver, n, noise_q, qpos).items():
            data[f"{solver}_n{n}_{k}"] = v
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", help="case names to (re)generate; default: all, and the handles file")
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--lib", default=None, help="record from this build of the library instead of the product one")
    a = ap.parse_args()
    global LIB
    LIB = os.path.abspath(a.lib) if a.lib else None
    os.makedirs(a.out, exist_ok=True)
    noise_q = noise()
    for case in CASES:
        if a.cases and case not in a.cases:
            continue
        qpos = start_qpos(case)
        ncon = contact_counts(case, qpos)
        print(f"  {case}: floor contacts of the start states {ncon}")
        assert min(ncon) >= 1, f"{case}: an env starts without a contact row ({ncon})"
        data = {"noise_q": noise_q, "qpos": qpos}
        for solver in SOLVERS:
            data.update(run_case(case, solver, noise_q, qpos))
            st = data[f"{solver}_n{NMAX}_state"]
            assert np.isfinite(st[:, :, :58]).all(), f"{case} {solver}: non-finite state"
            assert (data[f"{solver}_n{NMAX}_solver_iters"][0] > 0).all(), f"{case} {solver}: a first step without a solver iteration"
        path = os.path.join(a.out, f"const_records_{case}.npz")
        np.savez_compressed(path, **data)
        kb = os.path.getsize(path) / 1024
        assert kb < 100, f"{path}: {kb:.0f} KB"
        print(f"{case}: {len(data)} arrays, {kb:.0f} KB")
    if not a.cases:
        data = {"noise_q": noise_q}
        for h in HANDLES:
            data[f"qpos_{h}"] = start_qpos(h)
            for k, v in run_alone(h, "cg", NMAX, noise_q, data[f"qpos_{h}"]).items():
                data[f"{h}_{k}"] = v
        assert any(not np.array_equal(data[f"default_{k}"], data[f"limbs_{k}"]) for k in KEYS), \
            "the limbs handle computes what the default handle does"
        path = os.path.join(a.out, "const_records_handles.npz")
        np.savez_compressed(path, **data)
        print(f"handles: {len(data)} arrays, {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
