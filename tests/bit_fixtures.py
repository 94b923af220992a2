"""What the engine-bit fixture families share (tests/golden/make_<family>.py and their replay tests).

A family records the HIP engine's own output bits into tests/golden/<family>_<name>.npz at the commit
before a change that must keep every rounding, and its test replays them with array_equal. A family
module holds what is its own: FAMILY, MAX_KB, its CASES table (FIXTURES where the file names are not
the case names), inputs(name) (what is drawn for a fixture: the action noise, start poses), its start
state, its config, the rows it keeps and its premise checks: run_case(name, ...) and check_case(name,
*its result), which main() runs before it writes a file, or a record(names, lib_path) of its own
where the checks span several cases or files. Everything else is here, once: the import paths, the
action noise, the model cache, the state-row edits, the engine loop (Run), the comparison and the
command line. Test infrastructure only.
"""

import argparse
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GOLDEN = os.path.join(TESTS, "golden")
# a generator run as a script starts with tests/golden alone; pytest has the first three from conftest.py
for _p in (os.path.join(ROOT, "ksim-gym-zbot_amd"), os.path.join(ROOT, "oracle"), TESTS, GOLDEN):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import collider_util as U  # noqa: E402
from zbot_amd import compile_model  # noqa: E402
from zbot_amd import cstructs as cs  # noqa: E402

SIGMA = 0.2  # of the actions around the joint biases
PAST = 0.05  # rad past a hinge's range
DBG_MISC = 1728  # csrc/zb_internal.h ZB_DBG_MISC: debug_forward's nefc, ncon, ...
PER_STEP = ("reward", "done", "success", "solver_iters")


# ---- inputs ----

def noise(seed, shape):
    """int8 N(0, 1) in steps of 1/32: what a fixture keeps of its draws (float32 follows exactly)."""
    z = np.random.default_rng(seed).standard_normal(shape)
    return np.clip(np.rint(z * 32.0), -127, 127).astype(np.int8)


def action_noise(seed, steps, n):
    return noise(seed, (steps, n, cs.NJ))


def actions(cm, noise_q):
    """[steps, n, 20] float32: the joint biases + SIGMA N(0, 1), exact in float32 from the int8 noise."""
    bias = np.array([cm.cmodel.joint_bias[i] for i in range(cs.NJ)], np.float32)
    return bias + np.float32(SIGMA) * (noise_q.astype(np.float32) / np.float32(32.0))


_models = {}


def model(key=None):
    """The compiled model of `key`, compiled once: None (the default model), an asset XML name, a
    collider_util descriptor (sole_pair, limbs_pair, many_pair), or the default description without
    friction loss (nofloss) or without gravity (nogravity)."""
    if key not in _models:
        from zbot_amd.mjcf import load_mjcf  # noqa: PLC0415
        from zbot_amd.model import load_description  # noqa: PLC0415

        if key is None:
            d = None
        elif key.endswith(".xml"):
            d = load_mjcf(os.path.join(ROOT, "ksim-gym-zbot_amd", "assets", key))
        elif key in ("nofloss", "nogravity"):
            d = load_description()
            if key == "nofloss":
                for sc in d["servo_classes"].values():
                    sc["frictionloss"] = 0.0
            else:
                d.setdefault("option", {})["gravity"] = [0.0, 0.0, 0.0]
        else:
            d = getattr(U, key + "_desc")()
        _models[key] = compile_model(d)
    return _models[key]


# ---- state rows [n, STATE_STRIDE] ----

def qpos_cols(cm):
    return slice(cs.S_QPOS, cs.S_QPOS + cm.nq)


def qvel_cols(cm):
    return slice(cs.S_QVEL, cs.S_QVEL + cm.nv)


def motion_cols(cm):
    """qpos through qvel: what a premise check wants finite."""
    return slice(cs.S_QPOS, cs.S_QVEL + cm.nv)


def at_rest(cm, st):
    """Velocities and the solver's warm start zero, in place."""
    st[..., qvel_cols(cm)] = 0.0
    st[..., cs.S_QACCW:cs.S_PLAN_POS] = 0.0
    return st


def rest_at(cm, qpos):
    """start= of a Run whose envs stand still at the rows of `qpos` (None: they stay as reset left them)."""
    if qpos is None:
        return None

    def start(st):
        st[:, qpos_cols(cm)] = qpos[:len(st)]
        return at_rest(cm, st)

    return start


def lift(row, dz):
    """One state row's base moved up by dz (m, rounded to float32 first)."""
    row[cs.S_QPOS + 2] += np.float32(dz)


def hinge(cm, joint):
    return next(b for b in cm.bodies if b.jnt_name == joint)


def set_past(cm, row, joint, side=1):
    """One state row's limited hinge `joint` PAST its upper (side > 0) or lower bound."""
    b = hinge(cm, joint)
    row[cs.S_QPOS + b.qposadr] = np.float32(b.jrange[1] + PAST if side > 0 else b.jrange[0] - PAST)


# ---- the engine loop ----

class Run:
    """One handle of n envs at its start state and randomization rows; step() takes the next control
    step and keeps its rows, result() adds what is kept at the end.

    start: reset state rows -> start state rows (None: no set_state). rand: None leaves the
    randomization rows alone, "own" writes every env's own back, "row0" gives every env row 0's.
    swap: the envs in reverse order on the device (state rows, randomization rows, actions), every
    kept row reversed back. step_kw: keywords of HipEngine.step. per_step: outputs of step(),
    "solver_iters", and "state" / "states" for get_state() (None: all of them). final: of
    "start_state", "start_rand", "final_state", "final_rand" and "last" (every output of the last
    step as last_<output>)."""

    def __init__(self, cm, cfg, n, seed, acts, start=None, rand=None, lib_path=None, swap=False, step_kw=None,
                 per_step=PER_STEP, final=()):
        import torch  # noqa: PLC0415
        from zbot_amd.engine import HipEngine  # noqa: PLC0415

        self.torch = torch
        self.acts = acts[:, :n]
        self.o = slice(None, None, -1) if swap else slice(None)
        self.step_kw, self.final = step_kw or {}, final
        self.eng = HipEngine(cm, cfg, n, seed=seed, lib_path=lib_path)
        self.eng.reset()
        self.start_state = None if start is None else start(self.eng.get_state().cpu().numpy())
        self.start_rand = None if rand is None else self.eng.get_rand().cpu().numpy()
        if rand == "row0":
            self.start_rand[:] = self.start_rand[0]
        if start is not None:
            self.eng.set_state(self.to_device(self.start_state))
        if rand is not None:
            self.eng.set_rand(self.to_device(self.start_rand))
        self.rows = {k: [] for k in per_step or (*self.eng.outputs(), "solver_iters", "state")}
        self.out = None
        self.t = 0

    def to_device(self, rows):
        return self.torch.from_numpy(np.ascontiguousarray(rows[self.o])).cuda()

    def to_host(self, t):
        return t.cpu().numpy()[self.o].copy()

    def step(self):
        self.out = self.eng.step(self.to_device(self.acts[self.t]), **self.step_kw)
        self.t += 1
        self.torch.cuda.synchronize()
        for k, v in self.rows.items():
            v.append(self.to_host(self.eng.solver_iters() if k == "solver_iters"  # of this launch
                                  else self.eng.get_state() if k in ("state", "states") else self.out[k]))

    def result(self):
        d = {k: np.stack(v) for k, v in self.rows.items()}
        for k in self.final:
            if k == "last":
                d.update({f"last_{o}": self.to_host(v) for o, v in self.out.items()})
            elif k.startswith("start_"):
                d[k] = getattr(self, k)
            else:
                d[k] = self.to_host(self.eng.get_state() if k == "final_state" else self.eng.get_rand())
        return d

    def run(self):
        while self.t < len(self.acts):
            self.step()
        return self.result()


def run(*args, **kw):
    return Run(*args, **kw).run()


def cpu_twin(cm, cfg, seed, data):
    """The CPU twin of a recorded run, for premise checks: (the oracle module, an oracle.OracleEnv at
    the run's start_state and start_rand rows, the actions of its noise_q)."""
    import oracle as O  # noqa: PLC0415

    O.build()
    st = data["start_state"]
    env = O.OracleEnv(cm.cmodel, cfg, len(st), seed=seed)
    env.reset()
    env.state[:, :st.shape[1]] = st
    env.rand[:] = data["start_rand"]
    return O, env, actions(cm, data["noise_q"])


# ---- fixtures ----

def tagged(tag, d):
    return {tag + k: v for k, v in d.items()}


def names(fam):
    """The fixtures of a family module: <FAMILY>_<name>.npz."""
    return tuple(fam.FIXTURES if hasattr(fam, "FIXTURES") else fam.CASES)


def load(family, name):
    return np.load(os.path.join(GOLDEN, f"{family}_{name}.npz"))


def differing(got, want, keys=None, prefix=""):
    """The arrays of `got` (or its `keys`) that are not, bit for bit, want[prefix + key]."""
    return [k for k in (got if keys is None else keys) if not np.array_equal(got[k], want[prefix + k], equal_nan=True)]


@pytest.fixture(scope="module")
def torch_gpu():
    import torch  # noqa: PLC0415

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def record(fam, names, lib_path=None):
    """(name, data) of every fixture in `names`, each checked on its premises before it is handed out.
    A family whose checks span several cases or files has a record(names, lib_path) of its own."""
    if hasattr(fam, "record"):
        yield from fam.record(names, lib_path)
        return
    for name in names:
        data, *context = fam.run_case(name, lib_path=lib_path)
        fam.check_case(name, data, *context)
        yield name, data


def main(fam):
    ap = argparse.ArgumentParser(description=fam.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", help=f"fixtures to (re)generate, of {', '.join(names(fam))}; default: all")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--lib", default=None, help="record from this build of the library instead of the product one")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    todo = [n for n in names(fam) if not a.cases or n in a.cases]
    for name, data in record(fam, todo, a.lib and os.path.abspath(a.lib)):
        path = os.path.join(a.out, f"{fam.FAMILY}_{name}.npz")
        np.savez_compressed(path, **data)
        kb = os.path.getsize(path) / 1024
        assert kb < fam.MAX_KB, f"{path}: {kb:.0f} KB"
        print(f"{name}: {len(data)} arrays, {kb:.0f} KB")
