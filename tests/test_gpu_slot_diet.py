"""The step kernel's bits with friction-loss rows in all three zones of one wave.

Fixtures (tests/golden/slot_diet_<case>.npz, tests/golden/make_slot_diet.py): n = 1, 2 and 3 envs,
three control steps, CG and Newton in their default-fields kernels and the generic CG kernel
(iterations = 3). Every hinge moves at about 1 rad/s, so that one wave holds friction-loss rows below
-R fl, above +R fl and in the linear zone at once, beside the free joint's dofs without friction
loss; the pair cases put an airborne env beside one in contact that also has the wave's only
joint-limit row. Every stored array is compared with array_equal.

The pair cases are replayed twice, as [A, B] and as [B, A]: both must give the fixture's rows (the
second one's swapped back), which pins the upper team's lanes to the same bits as the lower one's.

The premises (all three zones in one wave and step, A airborne, B in contact, one limit row) are
checked on the CPU twin by the generator and again here, without the GPU.

The fixtures were recorded with the library of commit 132bf6a, the parent of the change that cut the
CG wave's non-VALU issue slots. A change meant to keep every rounding passes unchanged.
"""

import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_slot_diet as D  # noqa: E402


def _fixture(name):
    return np.load(os.path.join(HERE, "golden", f"slot_diet_{name}.npz"))


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.parametrize("name", list(D.CASES))
def test_fixture_holds_every_zone(name):
    """On the CPU twin: the recorded start states and actions put every zone into one wave."""
    from zbot_amd import compile_model

    want = _fixture(name)
    D.check_zones(name, compile_model(), {k: want[k] for k in ("start_state", "start_rand", "noise_q")})


def _replay(name, swap):
    want = _fixture(name)
    got, cm = D.run_case(name, noise_q=want["noise_q"], swap=swap)
    D.check_case(name, got, cm, zones=False)
    assert sorted(got) == sorted(want.files)
    bad = [k for k in want.files if not np.array_equal(got[k], want[k], equal_nan=True)]
    assert not bad, f"{name} (swapped: {swap}): arrays that differ from the recorded bits: {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(D.CASES))
def test_engine_reproduces_slot_diet(torch_gpu, name):
    _replay(name, swap=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, kw in D.CASES.items() if kw["layout"] == "AB"])
def test_swapped_pair_gives_swapped_rows(torch_gpu, name):
    _replay(name, swap=True)
