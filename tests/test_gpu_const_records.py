"""The per-handle constant records hold the handle's own model, bit for bit
(tests/golden/const_records_*.npz).

zb_create repacks the model rows that the step kernel's substep body reads per lane into a record
owned by the handle (csrc/zb_host.h LR_*, built by zb_host.cpp build_lane_record), and the kernels
that take it read the record where they read the model before. The fixtures were recorded by
tests/golden/make_const_records.py with the library of the commit before the records existed. A
record built wrongly for some model, or stale for a model other than the one its handle was created
with, moves bits here (array_equal):

  - per model and configuration (the default model, the four collider assets, implicit damping,
    per-env randomization), CG and Newton, n = 2 and n = 3, three control steps from touching states;
  - two handles with different models alive at once, stepped A, B, A, B;
  - a handle created after another with a different model was stepped and destroyed.
"""

import gc
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_const_records as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def load(name):
    return np.load(os.path.join(HERE, "golden", f"const_records_{name}.npz"))


@pytest.mark.parametrize("solver", G.SOLVERS)
@pytest.mark.parametrize("case", list(G.CASES))
def test_model_case(torch_gpu, case, solver):
    want = load(case)
    ncon = G.contact_counts(case, want["qpos"])
    assert min(ncon) >= 1, f"{case}: an env starts without a contact row ({ncon})"
    got = G.run_case(case, solver, want["noise_q"], want["qpos"])
    assert sorted(got) == sorted(k for k in want.files if k.startswith(solver + "_"))
    bad = [k for k in got if not np.array_equal(got[k], want[k], equal_nan=True)]
    assert not bad, f"{case} {solver}: arrays that differ from the recorded bits: {bad}"


def handle_run(want, h):
    return G.Run(h, "cg", G.NMAX, want["noise_q"], want[f"qpos_{h}"])


def differing(got, want, prefix):
    return [k for k in G.KEYS if not np.array_equal(got[k], want[f"{prefix}_{k}"], equal_nan=True)]


def test_two_models_interleaved(torch_gpu):
    want = load("handles")
    ra, rb = handle_run(want, "default"), handle_run(want, "limbs")
    for _ in range(G.STEPS):
        ra.step()
        rb.step()
    for h, r in (("default", ra), ("limbs", rb)):
        bad = differing(r.result(), want, h)
        assert not bad, f"handle {h} beside the other model's: differs from its run alone in {bad}"


@pytest.mark.parametrize("first,second", [("default", "limbs"), ("limbs", "default")])
def test_handle_created_after_another_model_was_destroyed(torch_gpu, first, second):
    want = load("handles")
    a = handle_run(want, first)
    a.step()
    del a
    gc.collect()  # HipEngine.__del__: zb_destroy
    b = handle_run(want, second)
    for _ in range(G.STEPS):
        b.step()
    bad = differing(b.result(), want, second)
    assert not bad, f"the {second} handle created after the {first} one differs from its recorded bits in {bad}"
