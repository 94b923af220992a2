"""Record the HIP engine's output bits under non-default solver settings and with several handles
in one process (needs the GPU): tests/golden/const_staging_<solver>.npz and const_staging_handles.npz.

    python tests/golden/make_const_staging.py [--out DIR] [--lib libzbot_hip.so]

The other engine-bit fixtures all run the default solver settings with one model per process. A
library that treats values fixed for a handle's life specially (a kernel specialised for the
default solver fields of ZbEnvConfig, a copy of ZbModel rows kept outside the handle's buffers)
could serve one handle what belongs to another, and those fixtures would not see it.
These pin what a handle computes when its settings differ from the defaults and from its
neighbour's. tests/test_gpu_const_staging.py replays them and compares with array_equal.

Every run starts from the touching states of tests/collider_util.py (contact rows exist from the
first substep on, so the solver iterates), takes two control steps and keeps the state, reward, done
and solver_iters rows. n = 2 and n = 3: the odd count runs the ghost team of the last wave.

Regenerating: as for make_engine_bits.py, on the GPU at the commit whose bits are meant, after the
oracle-based tests have passed.
"""

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "ksim-gym-zbot_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

NMAX = 3
SIZES = (2, 3)
STEPS = 2
SEED = 31
SIGMA = 0.2

# the solver fields a case sets (every other field: default_config())
CONFIGS = {
    "default": {},
    "it3_ls2": dict(iterations=3, ls_iterations=2),
    "tol_neg": dict(tolerance=-1.0),
    "lstol": dict(ls_tolerance=0.3),
    "ls1": dict(ls_iterations=1),
    "it3": dict(iterations=3),
}
SOLVER_CASES = ("it3_ls2", "tol_neg", "lstol", "ls1")
SOLVERS = ("cg", "newton")
# the handles of const_staging_handles.npz, each recorded alone: (config, model); CG, n = 3
HANDLES = {
    "default": ("default", None),
    "it3": ("it3", None),
    "limbs": ("default", "zbot_like_limbs.xml"),
    "it3_limbs": ("it3", "zbot_like_limbs.xml"),
}
KEYS = ("state", "reward", "done", "solver_iters")
LIB = None  # another build of the library to record from (--lib); None: the product library

_models = {}


def model(name=None):
    if name not in _models:
        from zbot_amd import compile_model  # noqa: PLC0415
        from zbot_amd.mjcf import load_mjcf  # noqa: PLC0415

        _models[name] = compile_model() if name is None else compile_model(
            load_mjcf(os.path.join(ROOT, "ksim-gym-zbot_amd", "assets", name)))
    return _models[name]


def config(name, solver="cg"):
    from zbot_amd import default_config  # noqa: PLC0415

    kw = CONFIGS[name]
    cfg = default_config(solver=solver, **{k: v for k, v in kw.items() if k in ("iterations", "ls_iterations")})
    for k in ("tolerance", "ls_tolerance"):
        if k in kw:
            setattr(cfg, k, kw[k])
    return cfg


def noise():
    """[STEPS, NMAX, 20] int8: N(0, 1) in steps of 1/32 (the fixtures keep it; the actions follow exactly)."""
    z = np.random.default_rng(SEED).standard_normal((STEPS, NMAX, 20))
    return np.clip(np.rint(z * 32.0), -127, 127).astype(np.int8)


def start_qpos(model_name=None):
    """[NMAX, 27] float32 touching states of the model."""
    import collider_util as U  # noqa: PLC0415

    return U.touching_states(model(model_name), NMAX, SEED).astype(np.float32)


def actions(cm, noise_q):
    bias = np.array([cm.cmodel.joint_bias[i] for i in range(20)], np.float32)
    return bias + np.float32(SIGMA) * (noise_q.astype(np.float32) / np.float32(32.0))


class Run:
    """One handle of n envs at its start state; step() takes the next control step and keeps its rows."""

    def __init__(self, cfg_name, solver, model_name, n, noise_q, qpos):
        import torch  # noqa: PLC0415
        from zbot_amd import cstructs as cs  # noqa: PLC0415
        from zbot_amd.engine import HipEngine  # noqa: PLC0415

        self.torch = torch
        cm = model(model_name)
        self.acts = actions(cm, noise_q)[:, :n]
        self.eng = HipEngine(cm, config(cfg_name, solver), n, seed=SEED, lib_path=LIB)
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


def run_alone(cfg_name, solver, model_name, n, noise_q, qpos):
    r = Run(cfg_name, solver, model_name, n, noise_q, qpos)
    for _ in range(STEPS):
        r.step()
    return r.result()


def run_solver_cases(solver, noise_q, qpos):
    """{"<case>_n<n>_<key>": array} of every non-default solver setting, for one solver."""
    data = {}
    for name in SOLVER_CASES:
        for n in SIZES:
            for k, v in run_alone(name, solver, None, n, noise_q, qpos).items():
                data[f"{name}_n{n}_{k}"] = v
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--lib", default=None, help="record from this build of the library instead of the product one")
    a = ap.parse_args()
    global LIB
    LIB = os.path.abspath(a.lib) if a.lib else None
    os.makedirs(a.out, exist_ok=True)
    noise_q = noise()
    qpos = {m: start_qpos(m) for m in (None, "zbot_like_limbs.xml")}
    cap = config("default").n_substeps
    for solver in SOLVERS:
        data = run_solver_cases(solver, noise_q, qpos[None])
        # what makes the fixture worth having: the settings change what the solver does
        it3 = data["it3_ls2_n3_solver_iters"]
        full = data["tol_neg_n3_solver_iters"]
        assert np.isfinite(data["tol_neg_n3_state"][:, :, :58]).all(), f"{solver}: non-finite state"
        assert (it3 <= 3 * cap + 3).all() and (it3 > 0).all(), f"{solver}: iterations=3 not honoured: {it3}"
        assert (full > it3).all(), f"{solver}: tolerance=-1 ran no longer than iterations=3"
        for other in ("lstol", "ls1"):
            assert not np.array_equal(data[f"{other}_n3_state"], data["tol_neg_n3_state"]), f"{solver}: {other} changed nothing"
        data["noise_q"], data["qpos"] = noise_q, qpos[None]
        path = os.path.join(a.out, f"const_staging_{solver}.npz")
        np.savez_compressed(path, **data)
        print(f"{solver}: {len(data)} arrays, {os.path.getsize(path) / 1024:.0f} KB")
    data = {"noise_q": noise_q, "qpos": qpos[None], "qpos_limbs": qpos["zbot_like_limbs.xml"]}
    for h, (cfg_name, model_name) in HANDLES.items():
        for k, v in run_alone(cfg_name, "cg", model_name, NMAX, noise_q, qpos[model_name]).items():
            data[f"{h}_{k}"] = v
    # an env that starts tipped over ends its episode in the first step and carries the reset state
    # from then on, whatever the handle: the step's reward and iteration count tell the handles apart
    for other in ("it3", "limbs"):
        assert any(not np.array_equal(data[f"default_{k}"], data[f"{other}_{k}"]) for k in KEYS), \
            f"handle {other} computes what the default handle does"
    path = os.path.join(a.out, "const_staging_handles.npz")
    np.savez_compressed(path, **data)
    print(f"handles: {len(data)} arrays, {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
