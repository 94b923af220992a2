"""zbot_amd.train.Trainer with a velocity command config (include/zbot_command.h): the per-term
metrics are finite, and a run continued from state_dict() in fresh engine and policy handles equals
the uninterrupted one bit for bit, command sequence included. 64 envs, T = 8, two iterations and
one more.
"""

import io

import pytest
import torch

import command_ref as R
from zbot_amd import cstructs as cs
from zbot_amd import default_config
from zbot_amd.policy import ACTOR, CRITIC, init_params

pytestmark = pytest.mark.gpu
N, T, BATCH, PASSES, SEED = 64, 8, 32, 2, 5
SCALES = dict(linvel_tracking=1.0, yaw_tracking=0.5, base_height=0.5)


def make_trainer(cmodel, weights=(8, 9), command=True):
    from zbot_amd import policy as P
    from zbot_amd.engine import HipEngine
    from zbot_amd.train import Trainer

    actor = P.GruPolicy(ACTOR, init_params(ACTOR, seed=weights[0]))
    critic = P.GruPolicy(CRITIC, init_params(CRITIC, seed=weights[1]))
    cc = R.joystick(0.25, SCALES, by_curriculum=("yaw_tracking",)) if command else None
    return Trainer(HipEngine(cmodel, default_config(), N, seed=2), actor, critic, rollout_steps=T, num_passes=PASSES,
                   batch_size=BATCH, seed=SEED, shuffle=True, command_config=cc)


def snap(tr):
    torch.cuda.synchronize()
    sd = tr.learner.state_dict()
    out = {f"{net}.{k}": sd[net][k] for net in ("actor", "critic") for k in ("params", "m", "v")}
    out["reward"] = tr.last_rollout["reward"].clone()
    out["commands"] = tr.eng.get_commands()
    return out


def test_trainer_with_commands_resumes_bit_for_bit(cmodel):
    a = make_trainer(cmodel)
    first = None
    for _ in range(2):
        m = a.step()
        first = a.last_rollout["reward"].clone() if first is None else first
        assert set(m["command_terms"]) == set(cs.CMD_TERM_NAMES)
        assert all(bool(torch.isfinite(v)) for v in m["command_terms"].values())
    assert a.eng.get_commands().abs().sum() > 0
    f = io.BytesIO()
    torch.save(a.state_dict(), f)
    a.step()
    want = snap(a)
    # a Trainer without a config reports no command terms, and earns another reward from the same seeds
    plain = make_trainer(cmodel, command=False)
    mp = plain.step()
    assert "command_terms" not in mp
    assert not torch.equal(plain.last_rollout["reward"], first)
    f.seek(0)
    b = make_trainer(cmodel, weights=(1, 2), command=False)  # the state brings the command config
    b.load_state_dict(torch.load(f, weights_only=False))
    assert b.iteration == 2 and bytes(b.command_config) == bytes(a.command_config)
    b.step()
    got = snap(b)
    for k in want:
        assert torch.equal(got[k], want[k]), k
