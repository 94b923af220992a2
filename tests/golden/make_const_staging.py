"""Record the HIP engine's output bits under non-default solver settings and with several handles
in one process (needs the GPU): tests/golden/const_staging_<solver>.npz and const_staging_handles.npz.

    python tests/golden/make_const_staging.py [--out DIR] [--lib libzbot_hip.so] [cg | newton | handles ...]

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
oracle-based tests have passed. What the engine-bit families share is in tests/bit_fixtures.py.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/, when run as a script
import bit_fixtures as F  # noqa: E402
import collider_util as U  # noqa: E402
from zbot_amd import default_config  # noqa: E402

FAMILY, MAX_KB = "const_staging", 100
NMAX = 3
SIZES = (2, 3)
STEPS = 2
SEED = 31

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
FIXTURES = (*SOLVERS, "handles")


def config(name, solver="cg"):
    kw = CONFIGS[name]
    cfg = default_config(solver=solver, **{k: v for k, v in kw.items() if k in ("iterations", "ls_iterations")})
    for k in ("tolerance", "ls_tolerance"):
        if k in kw:
            setattr(cfg, k, kw[k])
    return cfg


def start_qpos(model_name=None):
    """[NMAX, 27] float32 touching states of the model."""
    return U.touching_states(F.model(model_name), NMAX, SEED).astype(np.float32)


def inputs(name):
    d = {"noise_q": F.action_noise(SEED, STEPS, NMAX), "qpos": start_qpos()}
    if name == "handles":
        d["qpos_limbs"] = start_qpos("zbot_like_limbs.xml")
    return d


def handle(cfg_name, solver, model_name, n, noise_q, qpos, lib_path=None):
    """One handle of n envs at rest at `qpos`: a bit_fixtures.Run, stepped by the caller."""
    cm = F.model(model_name)
    return F.Run(cm, config(cfg_name, solver), n, SEED, F.actions(cm, noise_q), start=F.rest_at(cm, qpos),
                 lib_path=lib_path, per_step=KEYS)


def handle_alone(h, inputs, lib_path=None):
    """The handle `h` of const_staging_handles.npz; inputs: inputs("handles"), or the fixture itself."""
    cfg_name, model_name = HANDLES[h]
    qpos = inputs["qpos_limbs" if model_name else "qpos"]
    return handle(cfg_name, "cg", model_name, NMAX, inputs["noise_q"], qpos, lib_path)


def run_solver_cases(solver, noise_q, qpos, lib_path=None):
    """{"<case>_n<n>_<key>": array} of every non-default solver setting, for one solver."""
    data = {}
    for name in SOLVER_CASES:
        for n in SIZES:
            data.update(F.tagged(f"{name}_n{n}_", handle(name, solver, None, n, noise_q, qpos, lib_path).run()))
    return data


def check_solver_cases(solver, data) -> None:
    """What makes the fixture worth having: the settings change what the solver does."""
    cap = config("default").n_substeps
    it3 = data["it3_ls2_n3_solver_iters"]
    full = data["tol_neg_n3_solver_iters"]
    assert np.isfinite(data["tol_neg_n3_state"][:, :, F.motion_cols(F.model())]).all(), f"{solver}: non-finite state"
    assert (it3 <= 3 * cap + 3).all() and (it3 > 0).all(), f"{solver}: iterations=3 not honoured: {it3}"
    assert (full > it3).all(), f"{solver}: tolerance=-1 ran no longer than iterations=3"
    for other in ("lstol", "ls1"):
        assert not np.array_equal(data[f"{other}_n3_state"], data["tol_neg_n3_state"]), f"{solver}: {other} changed nothing"


def check_handles(data) -> None:
    # an env that starts tipped over ends its episode in the first step and carries the reset state
    # from then on, whatever the handle: the step's reward and iteration count tell the handles apart
    for other in ("it3", "limbs"):
        assert any(not np.array_equal(data[f"default_{k}"], data[f"{other}_{k}"]) for k in KEYS), \
            f"handle {other} computes what the default handle does"


def record(names, lib_path=None):
    for name in names:
        data = inputs(name)
        if name == "handles":
            for h in HANDLES:
                data.update(F.tagged(f"{h}_", handle_alone(h, data, lib_path).run()))
            check_handles(data)
        else:
            data.update(run_solver_cases(name, data["noise_q"], data["qpos"], lib_path))
            check_solver_cases(name, data)
        yield name, data


if __name__ == "__main__":
    F.main(sys.modules[__name__])
