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

import bit_fixtures as F
import pytest
from bit_fixtures import torch_gpu  # noqa: F401

import make_const_staging as G  # isort: skip  (tests/golden: on the path once bit_fixtures is imported)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("solver", G.SOLVERS)
def test_non_default_solver_fields(torch_gpu, solver):
    want = F.load(G.FAMILY, solver)
    got = G.run_solver_cases(solver, want["noise_q"], want["qpos"])
    assert sorted(got) == sorted(k for k in want.files if k not in ("noise_q", "qpos"))
    bad = F.differing(got, want)
    assert not bad, f"{solver}: arrays that differ from the recorded bits: {bad}"


@pytest.mark.parametrize("a,b", [("default", "it3"), ("default", "limbs")])
def test_two_handles_interleaved(torch_gpu, a, b):
    want = F.load(G.FAMILY, "handles")
    ra, rb = G.handle_alone(a, want), G.handle_alone(b, want)
    for _ in range(G.STEPS):
        ra.step()
        rb.step()
    for h, r in ((a, ra), (b, rb)):
        bad = F.differing(r.result(), want, G.KEYS, h + "_")
        assert not bad, f"handle {h} beside {b if h == a else a}: differs from its run alone in {bad}"


def test_handle_created_after_another_was_destroyed(torch_gpu):
    want = F.load(G.FAMILY, "handles")
    first = G.handle_alone("default", want)
    first.step()
    del first
    gc.collect()  # HipEngine.__del__: zb_destroy
    second = G.handle_alone("it3_limbs", want)
    for _ in range(G.STEPS):
        second.step()
    bad = F.differing(second.result(), want, G.KEYS, "it3_limbs_")
    assert not bad, f"the second handle differs from its recorded bits in {bad}"
