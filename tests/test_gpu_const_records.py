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

import bit_fixtures as F
import pytest
from bit_fixtures import torch_gpu  # noqa: F401

import make_const_records as G  # isort: skip  (tests/golden: on the path once bit_fixtures is imported)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("solver", G.SOLVERS)
@pytest.mark.parametrize("case", list(G.CASES))
def test_model_case(torch_gpu, case, solver):
    want = F.load(G.FAMILY, case)
    ncon = G.contact_counts(case, want["qpos"])
    assert min(ncon) >= 1, f"{case}: an env starts without a contact row ({ncon})"
    got = G.run_case(case, solver, want["noise_q"], want["qpos"])
    assert sorted(got) == sorted(k for k in want.files if k.startswith(solver + "_"))
    bad = F.differing(got, want)
    assert not bad, f"{case} {solver}: arrays that differ from the recorded bits: {bad}"


def test_two_models_interleaved(torch_gpu):
    want = F.load(G.FAMILY, "handles")
    ra, rb = G.handle_alone("default", want), G.handle_alone("limbs", want)
    for _ in range(G.STEPS):
        ra.step()
        rb.step()
    for h, r in (("default", ra), ("limbs", rb)):
        bad = F.differing(r.result(), want, G.KEYS, h + "_")
        assert not bad, f"handle {h} beside the other model's: differs from its run alone in {bad}"


@pytest.mark.parametrize("first,second", [("default", "limbs"), ("limbs", "default")])
def test_handle_created_after_another_model_was_destroyed(torch_gpu, first, second):
    want = F.load(G.FAMILY, "handles")
    a = G.handle_alone(first, want)
    a.step()
    del a
    gc.collect()  # HipEngine.__del__: zb_destroy
    b = G.handle_alone(second, want)
    for _ in range(G.STEPS):
        b.step()
    bad = F.differing(b.result(), want, G.KEYS, second + "_")
    assert not bad, f"the {second} handle created after the {first} one differs from its recorded bits in {bad}"
