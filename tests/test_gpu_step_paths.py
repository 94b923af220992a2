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

import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_step_paths as P  # noqa: E402

pytestmark = pytest.mark.gpu

SYM_STEPS = 3


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.parametrize("name", list(P.CASES))
def test_engine_reproduces_step_paths(torch_gpu, name):
    want = np.load(os.path.join(HERE, "golden", f"step_paths_{name}.npz"))
    got, cm = P.run_case(name, noise_q=want["noise_q"])
    P.check_case(name, got, cm)
    assert sorted(got) == sorted(want.files)
    bad = [k for k in want.files if not np.array_equal(got[k], want[k], equal_nan=True)]
    assert not bad, f"{name}: arrays that differ from the recorded bits: {bad}"


def _run_pair(torch, cm, cfg, st, rnd, actions):
    from zbot_amd.engine import HipEngine

    eng = HipEngine(cm, cfg, 2, seed=51)
    eng.reset()
    eng.set_state(torch.from_numpy(st))
    eng.set_rand(torch.from_numpy(rnd))
    rows = []
    for a in actions:
        out = eng.step(torch.from_numpy(np.ascontiguousarray(a)).cuda())
        torch.cuda.synchronize()
        d = {k: v.cpu().numpy().copy() for k, v in out.items()}
        d["solver_iters"] = eng.solver_iters().cpu().numpy()
        d["state"] = eng.get_state().cpu().numpy()
        rows.append(d)
    return rows


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_teams_are_symmetric(torch_gpu, solver):
    torch = torch_gpu
    from zbot_amd import compile_model, default_config
    from zbot_amd.engine import HipEngine

    cm = compile_model()
    cfg = default_config(solver=solver, obs_noise=False, autoreset=False)
    eng = HipEngine(cm, cfg, 2, seed=51)
    eng.reset()
    st = eng.get_state().cpu().numpy()
    rnd = eng.get_rand().cpu().numpy()
    del eng
    # B: the reset state of env 1 with one limited hinge past its upper bound; A: env 0's reset state
    b = P.S.hinge(cm, P.LIMIT_JOINT[0])
    st[1, b.qposadr] = np.float32(b.jrange[1] + P.S.PAST)
    assert not np.array_equal(st[0, :58], st[1, :58])
    actions = P.G.case_actions(cm, P.case_noise(SYM_STEPS, 2, 52))
    ab = _run_pair(torch, cm, cfg, st, rnd, actions)
    ba = _run_pair(torch, cm, cfg, st[::-1].copy(), rnd[::-1].copy(), actions[:, ::-1])
    for t in range(SYM_STEPS):
        assert not ab[t]["done"].any(), "an env terminated: the reset draws depend on the env index"
        assert (ab[t]["solver_iters"] > 0).all()
        bad = [k for k in ab[t] if not np.array_equal(ab[t][k], ba[t][k][::-1], equal_nan=True)]
        assert not bad, f"{solver} step {t}: outputs that are not the swapped rows: {bad}"
