"""The HIP engine against its own recorded bits (tests/golden/engine_bits_<case>.npz).

Each case of tests/golden/make_engine_bits.py is replayed with the fixture's action noise and every
stored array compared with array_equal: the per-step reward / done / success / solver_iters rows,
the final state and RNG rows and every output of the last step, for 64 envs and for the first
three envs alone. The cases cover the CG and Newton kernels of the default model, the implicit
damping, pushes with domain randomization, the second contact-row bank of the limbs and the
nine-collider model and the sole pair, and every kind of extra bank (one or two floor banks, the
cylinder / ellipsoid rules, the pair alone and beside them) under both solvers.

A change that is meant to keep every rounding (fewer instructions, another schedule, another
build flag) passes unchanged. A change that alters rounding on purpose regenerates the fixtures on
the GPU, after the oracle-based tests have passed, and commits them with the change:

    python tests/golden/make_engine_bits.py
"""

import bit_fixtures as F
import pytest
from bit_fixtures import torch_gpu  # noqa: F401

import make_engine_bits as G  # isort: skip  (tests/golden: on the path once bit_fixtures is imported)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(G.CASES))
def test_engine_reproduces_recorded_bits(torch_gpu, name):
    want = F.load(G.FAMILY, name)
    got, *_ = G.run_case(name, noise_q=want["noise_q"])
    assert sorted(got) == sorted(want.files)
    bad = F.differing(got, want)
    assert not bad, f"{name}: arrays that differ from the recorded bits: {bad}"
