"""Values fixed for a handle's life must stay that handle's own (tests/golden/const_staging_*.npz).

The library picks a step kernel per launch from the handle's host copy of the config: handles whose
solver fields are the defaults run a copy of the kernel that holds them as literals
(zb_internal.h solver_fields_default, zb_engine.hip SOL_LITERAL), every other handle the generic
kernel that reads them from its config buffer. The other engine-bit fixtures run the default solver
settings with one model per process, where a choice made for the wrong handle, or a value kept from
another handle, would show nothing. These replay tests/golden/make_const_staging.py's recordings
bit for bit (array_equal):

  - non-default iterations / ls_iterations / tolerance / ls_tolerance, CG and Newton, n = 2 and 3;
  - two handles alive at once on one stream, stepped A, B, A, B, with different settings and with
    different models: each must compute what it computes alone;
  - a handle created after another one was stepped and destroyed, with other settings and model.
"""

import gc
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_const_staging as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def load(name):
    return np.load(os.path.join(HERE, "golden", f"const_staging_{name}.npz"))


def differing(got, want, prefix):
    return [k for k in G.KEYS if not np.array_equal(got[k], want[f"{prefix}_{k}"], equal_nan=True)]


@pytest.mark.parametrize("solver", G.SOLVERS)
def test_non_default_solver_fields(torch_gpu, solver):
    want = load(solver)
    got = G.run_solver_cases(solver, want["noise_q"], want["qpos"])
    assert sorted(got) == sorted(k for k in want.files if k not in ("noise_q", "qpos"))
    bad = [k for k in got if not np.array_equal(got[k], want[k], equal_nan=True)]
    assert not bad, f"{solver}: arrays that differ from the recorded bits: {bad}"


def handle_run(want, h):
    cfg_name, model_name = G.HANDLES[h]
    return G.Run(cfg_name, "cg", model_name, G.NMAX, want["noise_q"], want["qpos_limbs" if model_name else "qpos"])


@pytest.mark.parametrize("a,b", [("default", "it3"), ("default", "limbs")])
def test_two_handles_interleaved(torch_gpu, a, b):
    want = load("handles")
    ra, rb = handle_run(want, a), handle_run(want, b)
    for _ in range(G.STEPS):
        ra.step()
        rb.step()
    for h, r in ((a, ra), (b, rb)):
        bad = differing(r.result(), want, h)
        assert not bad, f"handle {h} beside {b if h == a else a}: differs from its run alone in {bad}"


def test_handle_created_after_another_was_destroyed(torch_gpu):
    want = load("handles")
    first = handle_run(want, "default")
    first.step()
    del first
    gc.collect()  # HipEngine.__del__: zb_destroy
    second = handle_run(want, "it3_limbs")
    for _ in range(G.STEPS):
        second.step()
    bad = differing(second.result(), want, "it3_limbs")
    assert not bad, f"the second handle differs from its recorded bits in {bad}"
