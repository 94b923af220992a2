"""The engine-bit generators still draw the inputs that their committed fixtures were recorded from.

The replay tests feed a fixture's own action noise (and, for the two const families, its start
poses) back into the engine, so they would not notice a generator whose case table, seeds or draws
had drifted: the next recording would silently start from other inputs. Here every input that a
family's inputs(name) regenerates from its case table is compared, bit for bit, with the array of
the same name in tests/golden/<family>_<name>.npz, and the fixture files of a family are exactly
the names its module lists. No GPU: nothing is stepped.
"""

import glob
import importlib
import os

import bit_fixtures as F
import numpy as np
import pytest

FAMILIES = ("engine_bits", "smooth_bits", "const_staging", "step_paths", "const_records", "slot_diet", "spill_diet")
MODULES = {fam: importlib.import_module("make_" + fam) for fam in FAMILIES}


def is_input(key):
    return key == "noise_q" or key == "qpos" or key.startswith("qpos_")


@pytest.mark.parametrize("family,name", [(fam, name) for fam, mod in MODULES.items() for name in F.names(mod)])
def test_regenerated_inputs_equal_recorded(family, name):
    want = F.load(family, name)
    got = MODULES[family].inputs(name)
    assert sorted(got) == sorted(k for k in want.files if is_input(k))
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), f"{family}_{name}: {k} is not the recorded one"


@pytest.mark.parametrize("family", FAMILIES)
def test_fixture_files_are_the_listed_ones(family):
    assert MODULES[family].FAMILY == family
    files = glob.glob(os.path.join(F.GOLDEN, family + "_*.npz"))
    assert sorted(os.path.basename(f) for f in files) == sorted(f"{family}_{name}.npz" for name in F.names(MODULES[family]))
