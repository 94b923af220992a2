"""The HIP engine against its recorded bits on a joint-limit row and on waves without rows
(tests/golden/smooth_bits_<case>.npz).

tests/test_gpu_engine_bits.py pins the engine on runs that always have contact rows and never a
joint past its range. The cases of tests/golden/make_smooth_bits.py start in the two paths those
leave out: one limited hinge of each env 0.05 rad past its dof_range (the r.anyl path of
make_constraints / row_params and the solvers' limit terms), and envs 0.5 m above the reset height
(every env of a wave, or one team of it), on the default model and on a copy without friction loss,
where an airborne wave has no constraint row at all and forward() skips the solver. Each case runs
four control steps with n = 2 and n = 3, with the CG and the Newton kernels, and every stored array
is compared with array_equal.

The fixtures were recorded at commit 3a9cd9f ("PPO update in the library: loss seeds, global-norm
clip, AdamW in HIP"), the parent of the change that trimmed the once-per-substep phases of the
step kernel, before any kernel edit. A change meant to keep every rounding passes unchanged; one
that alters rounding on purpose regenerates them on the GPU after the oracle-based tests pass:

    python tests/golden/make_smooth_bits.py
"""

import bit_fixtures as F
import pytest
from bit_fixtures import torch_gpu  # noqa: F401

import make_smooth_bits as S  # isort: skip  (tests/golden: on the path once bit_fixtures is imported)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(S.CASES))
def test_engine_reproduces_smooth_bits(torch_gpu, name):
    want = F.load(S.FAMILY, name)
    got, cm = S.run_case(name, noise_q=want["noise_q"])
    for tag, _ in S.SIZES:
        S.check_start(name, cm, got[tag + "start_state"])
    assert sorted(got) == sorted(want.files)
    bad = F.differing(got, want)
    assert not bad, f"{name}: arrays that differ from the recorded bits: {bad}"
