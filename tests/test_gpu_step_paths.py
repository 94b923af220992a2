"""The step kernel on the paths its other bit fixtures leave dark, and a team-symmetry property.

Fixtures (tests/golden/step_paths_<case>.npz, tests/golden/make_step_paths.py): n = 1 (one live
team beside a ghost for the whole launch; CG and Newton), n = 2 with a joint-limit row in exactly
one of the two envs (the wave takes the line search's limit copy with one team's row absent), and
one control step with every output, without obs_extra and without reward_terms (the step end's
output switches). Every stored array is compared with array_equal, and the generator's own path
checks (done flags, debug_forward's row counts, untouched buffers) run again on the replay.

The fixtures were recorded at commit 4c8e7fd ("Step kernel: extra contact-row banks as one array
and one table"), the parent of the change that trimmed the CG loop's and the step end's executed
instructions, before any kernel edit. A change meant to keep every rounding passes unchanged; one
that alters rounding on purpose regenerates them on the GPU after the oracle-based tests pass:

    python tests/golden/make_step_paths.py

Team symmetry (no fixture): the two envs of a wave sit in lanes 0-31 and 32-63. With nothing that
depends on the env index (no observation noise, no automatic reset), stepping the states [A, B]
and [B, A] must give every output row swapped, bit for bit. It catches a cross-lane rewrite that
treats the upper team differently. A and B differ where the solver's copies differ: B has a limited
hinge past its range (a joint-limit row), A has none.
"""

import bit_fixtures as F
import numpy as np
import pytest
from bit_fixtures import torch_gpu  # noqa: F401

import make_step_paths as P  # isort: skip  (tests/golden: on the path once bit_fixtures is imported)

pytestmark = pytest.mark.gpu

SYM_STEPS = 3


@pytest.mark.parametrize("name", list(P.CASES))
def test_engine_reproduces_step_paths(torch_gpu, name):
    want = F.load(P.FAMILY, name)
    got, cm = P.run_case(name, noise_q=want["noise_q"])
    P.check_case(name, got, cm)
    assert sorted(got) == sorted(want.files)
    bad = F.differing(got, want)
    assert not bad, f"{name}: arrays that differ from the recorded bits: {bad}"


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_teams_are_symmetric(torch_gpu, solver):
    from zbot_amd import default_config

    cm = F.model()
    cfg = default_config(solver=solver, obs_noise=False, autoreset=False)

    def start(st):
        # B: the reset state of env 1 with one limited hinge past its upper bound; A: env 0's reset state
        F.set_past(cm, st[1], *P.LIMIT_JOINT)
        assert not np.array_equal(st[0, F.motion_cols(cm)], st[1, F.motion_cols(cm)])
        return st

    # every output, solver_iters and the state of every step, of [A, B] and of [B, A] with its rows swapped back
    ab, ba = (F.run(cm, cfg, 2, 51, F.actions(cm, F.action_noise(52, SYM_STEPS, 2)), start=start, rand="own",
                    swap=swap, per_step=None) for swap in (False, True))
    for t in range(SYM_STEPS):
        assert not ab["done"][t].any(), "an env terminated: the reset draws depend on the env index"
        assert (ab["solver_iters"][t] > 0).all()
        bad = [k for k in ab if not np.array_equal(ab[k][t], ba[k][t], equal_nan=True)]
        assert not bad, f"{solver} step {t}: outputs that are not the swapped rows: {bad}"
