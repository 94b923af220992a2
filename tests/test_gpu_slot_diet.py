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

import bit_fixtures as F
import pytest
from bit_fixtures import torch_gpu  # noqa: F401

import make_slot_diet as D  # isort: skip  (tests/golden: on the path once bit_fixtures is imported)


@pytest.mark.parametrize("name", list(D.CASES))
def test_fixture_holds_every_zone(name):
    """On the CPU twin: the recorded start states and actions put every zone into one wave."""
    want = F.load(D.FAMILY, name)
    D.check_zones(name, F.model(), {k: want[k] for k in ("start_state", "start_rand", "noise_q")})


def _replay(name, swap):
    want = F.load(D.FAMILY, name)
    got, cm = D.run_case(name, noise_q=want["noise_q"], swap=swap)
    D.check_case(name, got, cm, zones=False)
    assert sorted(got) == sorted(want.files)
    bad = F.differing(got, want)
    assert not bad, f"{name} (swapped: {swap}): arrays that differ from the recorded bits: {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(D.CASES))
def test_engine_reproduces_slot_diet(torch_gpu, name):
    _replay(name, swap=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, kw in D.CASES.items() if kw["layout"] == "AB"])
def test_swapped_pair_gives_swapped_rows(torch_gpu, name):
    _replay(name, swap=True)
