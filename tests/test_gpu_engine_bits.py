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

import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_engine_bits as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.parametrize("name", list(G.CASES))
def test_engine_reproduces_recorded_bits(torch_gpu, name):
    want = np.load(os.path.join(HERE, "golden", f"engine_bits_{name}.npz"))
    got, *_ = G.run_case(name, noise_q=want["noise_q"])
    assert sorted(got) == sorted(want.files)
    bad = [k for k in want.files if not np.array_equal(got[k], want[k], equal_nan=True)]
    assert not bad, f"{name}: arrays that differ from the recorded bits: {bad}"
