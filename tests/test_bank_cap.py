"""How many floor colliders beyond the soles a substep holds (zb_bank_cap, engine.bank_cap): two per
floor bank, one bank for models with up to two such colliders, two banks for more, with or without
the sole pair (the pair's half rows have a bank of their own, the XG 6 kernels beside two floor
banks). And the states of tests/test_gpu_pair_banks.py hold the cases those tests are about. No GPU
needed."""

import numpy as np
import pytest

import collider_util as U
from zbot_amd import compile_model

N_ENVS, STATE_SEED = 64, 11


def pair_beside_three_desc() -> dict:
    """many_desc cut to five colliders (the soles, the right leg's thigh and shin, the left thigh) with
    the sole pair."""
    d = U.many_desc()
    d["geoms"] = [g for g in d["geoms"] if g["name"].endswith("_foot_sole")
                  or g["name"] in ("right_thigh", "right_shin", "left_thigh")]
    d["self_pairs"] = [["left_foot_sole", "right_foot_sole"]]
    return d


CAPS = [
    ("default", None, 0),
    ("sole_pair", U.sole_pair_desc, 0),
    ("limbs", U.limbs_desc, 2),
    ("limbs_pair", U.limbs_pair_desc, 2),
    ("many", U.many_desc, 4),
    ("many_pair", U.many_pair_desc, 4),
    ("pair_beside_three", pair_beside_three_desc, 4),
]


@pytest.mark.parametrize("name,desc,cap", CAPS, ids=[c[0] for c in CAPS])
def test_bank_cap_per_model(name, desc, cap):
    from zbot_amd.engine import bank_cap, build_library

    build_library()
    cm = compile_model(desc()) if desc else compile_model()
    if name == "pair_beside_three":
        assert cm.cmodel.ngeom == 5 and cm.cmodel.npair == 1
    assert bank_cap(cm) == cap
    assert bank_cap(cm.cmodel) == cap


def pair_bank_cases(cm, n=N_ENVS, seed=STATE_SEED):
    """The crossing, touching states of the many + pair model and, per env, the colliders beyond the
    soles within reach of the floor (the engine's selection bound) and whether the third or fourth of
    them, in geom order, has a floor contact: (qpos [n, 27], candidates per env, bool [n])."""
    q = U.crossing_touching_states(cm, n, seed)
    margin = float(cm.cmodel.floor_margin)
    cand = [U.bank2_candidates(cm, q[e]) for e in range(n)]
    deep = np.zeros(n, bool)
    for e in range(n):
        con = U.contacts(cm, q[e], margin=margin)
        deep[e] = any(len(con[g]) > 0 for g in cand[e][2:4])
    return q, cand, deep


def test_pair_bank_states_contain_the_cases():
    cm = compile_model(U.many_pair_desc())
    _, cand, deep = pair_bank_cases(cm)
    ncand = np.array([len(c) for c in cand])
    second_floor_bank = ((ncand == 3) | (ncand == 4)) & deep
    print(f"\n[pair banks states] candidates per env {np.bincount(ncand).tolist()}; {int(((ncand == 3) | (ncand == 4)).sum())} "
          f"envs with 3-4, {int(second_floor_bank.sum())} of them with a contact on the third or fourth; "
          f"{int((ncand > 4).sum())} over four")
    assert second_floor_bank.sum() >= 6
    assert (ncand > 4).sum() >= 1
    assert (ncand <= 4).sum() >= 48
