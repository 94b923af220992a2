"""The step kernel's bits on the CG wave's exit paths.

Fixtures (tests/golden/spill_diet_<case>.npz, tests/golden/make_spill_diet.py): n = 1, 2 and 3 envs,
three control steps from touching states, the CG default-fields kernel and the generic CG kernel
(iterations = 3). Together they hold line searches that end after 1, 2, 3 to 7 and the cap of 8
evaluations, a wave whose two teams leave the same line search after different counts, a team whose
every line search returns at its entry test beside one that searches, a team in the line search's
joint-limit copy beside one without the row, an airborne env beside one in contact, an env that
terminates at the first control step (the ghost pass and the reset re-entry), and a ghost team past
n. Every stored array is compared with array_equal.

The plain pairs are replayed twice, as [A, B] and as [B, A]: both must give the fixture's rows (the
second one's swapped back), which pins the upper team's lanes to the same bits as the lower one's.

The premises are checked on the CPU twin by the generator and again here, without the GPU.

The fixtures were recorded with the library of commit 57ba670, the parent of the change to the line
search's exit path. A change meant to keep every rounding passes unchanged.
"""

import bit_fixtures as F
import pytest
from bit_fixtures import torch_gpu  # noqa: F401

import make_spill_diet as P  # isort: skip  (tests/golden: on the path once bit_fixtures is imported)


@pytest.fixture(scope="module")
def twins():
    """check_twin of every fixture, once: {case: (counts held, a wave with differing exits)}."""
    out = {}
    for name in P.CASES:
        want = F.load(P.FAMILY, name)
        out[name] = P.check_twin(name, {k: want[k] for k in ("start_state", "start_rand", "noise_q")})
    return out


@pytest.mark.parametrize("name", list(P.CASES))
def test_fixture_holds_its_case(twins, name):
    """On the CPU twin: the recorded start states and actions take the case's paths (check_twin
    asserts them), and the recorded flags agree."""
    want = F.load(P.FAMILY, name)
    P.check_case(name, {k: want[k] for k in ("states", "done", "solver_iters")})
    assert name in twins


def test_fixtures_hold_every_exit(twins):
    """Together: 0, 1, 2, 3 to 7 and 8 evaluations, differing exits in one wave, n = 1 and n = 3."""
    P.check_all({k: v[0] for k, v in twins.items()}, {k: v[1] for k, v in twins.items()},
                {F.load(P.FAMILY, name)["start_state"].shape[0] for name in P.CASES})


def _replay(name, swap):
    want = F.load(P.FAMILY, name)
    got, _ = P.run_case(name, noise_q=want["noise_q"], swap=swap)
    P.check_case(name, got)
    assert sorted(got) == sorted(want.files)
    bad = F.differing(got, want)
    assert not bad, f"{name} (swapped: {swap}): arrays that differ from the recorded bits: {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(P.CASES))
def test_engine_reproduces_spill_diet(torch_gpu, name):
    _replay(name, swap=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", P.SWAPPED)
def test_swapped_pair_gives_swapped_rows(torch_gpu, name):
    _replay(name, swap=True)
