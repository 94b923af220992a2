"""Record the HIP engine's bits per model, for the per-handle constant records (needs the GPU):
tests/golden/const_records_<case>.npz and const_records_handles.npz.

    python tests/golden/make_const_records.py [--out DIR] [--lib libzbot_hip.so] [case | handles ...]

zb_create repacks the model rows that the substep body reads per lane into a record of the handle's
own (csrc/zb_host.h, "lane record"). The other engine-bit fixtures would not see a record built
wrongly for a model other than the default, or one left over from another handle. These were
recorded with the library of the commit before the records existed, whose kernels read the model
itself; tests/test_gpu_const_records.py replays them and compares with array_equal.

A case is one model and configuration: CG and Newton, n = 2 (one full wave) and n = 3 (a wave with
an idle team), three control steps from the touching states of tests/collider_util.py. record()
refuses to write a case in which an env starts without a floor contact: the constraint rows' loads
have to run from the first substep on.

  default, limbs, many, cyl, mesh   the default model and the four collider assets (many: the second
                                    compilation unit)
  eulerdamp                         the implicit-damping kernels
  randomize                         per-env parameters, which live in EnvL::par and not in the record

const_records_handles.npz holds the default and the limbs model (CG, n = 3), each recorded alone,
for the tests with two handles alive at once and with a handle created after another was destroyed.

Regenerating: as for make_engine_bits.py, on the GPU at the commit whose bits are meant. What the
engine-bit families share is in tests/bit_fixtures.py.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/, when run as a script
import bit_fixtures as F  # noqa: E402
import collider_util as U  # noqa: E402
from zbot_amd import default_config  # noqa: E402

FAMILY, MAX_KB = "const_records", 100
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
FIXTURES = (*CASES, "handles")


def start_qpos(case):
    """[NMAX, 27] float32 touching states of the case's model."""
    return U.touching_states(F.model(CASES[case].get("model")), NMAX, SEED).astype(np.float32)


def inputs(name):
    d = {"noise_q": F.action_noise(SEED, STEPS, NMAX)}
    d.update({f"qpos_{h}": start_qpos(h) for h in HANDLES} if name == "handles" else {"qpos": start_qpos(name)})
    return d


def contact_counts(case, qpos):
    """Per env: floor contacts of the start state, over all colliders."""
    cm = F.model(CASES[case].get("model"))
    return [sum(len(c) for c in U.contacts(cm, q.astype(np.float64))) for q in qpos]


def handle(case, solver, n, noise_q, qpos, lib_path=None):
    """One handle of n envs at rest at `qpos`: a bit_fixtures.Run, stepped by the caller."""
    kw = CASES[case]
    cm = F.model(kw.get("model"))
    cfg = default_config(solver=solver, eulerdamp=kw.get("eulerdamp", False), randomize=kw.get("randomize", False))
    return F.Run(cm, cfg, n, SEED, F.actions(cm, noise_q), start=F.rest_at(cm, qpos), lib_path=lib_path, per_step=KEYS)


def handle_alone(h, inputs, lib_path=None):
    """The handle `h` of const_records_handles.npz; inputs: inputs("handles"), or the fixture itself."""
    return handle(h, "cg", NMAX, inputs["noise_q"], inputs[f"qpos_{h}"], lib_path)


def run_case(case, solver, noise_q, qpos, lib_path=None):
    """{"<solver>_n<n>_<key>": array} of one case and solver."""
    data = {}
    for n in SIZES:
        data.update(F.tagged(f"{solver}_n{n}_", handle(case, solver, n, noise_q, qpos, lib_path).run()))
    return data


def record(names, lib_path=None):
    for name in names:
        data = inputs(name)
        if name == "handles":
            for h in HANDLES:
                data.update(F.tagged(f"{h}_", handle_alone(h, data, lib_path).run()))
            assert any(not np.array_equal(data[f"default_{k}"], data[f"limbs_{k}"]) for k in KEYS), \
                "the limbs handle computes what the default handle does"
        else:
            ncon = contact_counts(name, data["qpos"])
            print(f"  {name}: floor contacts of the start states {ncon}")
            assert min(ncon) >= 1, f"{name}: an env starts without a contact row ({ncon})"
            for solver in SOLVERS:
                data.update(run_case(name, solver, data["noise_q"], data["qpos"], lib_path))
                st = data[f"{solver}_n{NMAX}_state"]
                assert np.isfinite(st[:, :, F.motion_cols(F.model())]).all(), f"{name} {solver}: non-finite state"
                assert (data[f"{solver}_n{NMAX}_solver_iters"][0] > 0).all(), f"{name} {solver}: a first step without a solver iteration"
        yield name, data


if __name__ == "__main__":
    F.main(sys.modules[__name__])
