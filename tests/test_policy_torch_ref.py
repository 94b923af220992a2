"""The torch restatement of Actor / Critic (tests/policy_torch.py) against the CPU oracle.

policy_torch is the autograd reference of the HIP backward pass; this pins its fp64 forward to
oracle/zb_oracle_policy.c — the chain the GPU forward is bit-exact against — at the tolerance
test_policy.py::test_oracle_matches_float64_restatement holds its numpy restatement to.
"""

import numpy as np
import pytest
import torch

import policy_torch as PT
from zbot_amd.policy import ACTOR, CRITIC, EVAL, init_params

H, D, NJ = 128, 5, 20


@pytest.mark.parametrize("kind", [ACTOR, CRITIC])
def test_fp64_helper_matches_oracle(oracle_mod, kind):
    I = 50 if kind == ACTOR else 484
    P = init_params(kind, seed=5)
    rng = np.random.default_rng(12)
    T, n = 3, 5
    obs = rng.normal(size=(T, n, I)).astype(np.float32)
    carry0 = (0.5 * rng.normal(size=(n, D, H))).astype(np.float32)
    reset = np.zeros((T, n), np.uint8)
    reset[0, 1] = reset[1, 2] = reset[2, 4] = reset[2, 2] = 1
    acts = (0.3 * rng.normal(size=(T, n, NJ))).astype(np.float32)
    f64 = lambda x: torch.from_numpy(x).double()  # noqa: E731
    with torch.no_grad():
        if kind == ACTOR:
            _, lp, _ = oracle_mod.policy_actor(P, obs, carry0, reset, mode=EVAL, actions=acts, log_prob=True)
            got = PT.actor_log_prob(f64(P), f64(obs), f64(carry0), torch.from_numpy(reset), f64(acts))
            np.testing.assert_allclose(lp, got.numpy(), rtol=1e-4, atol=2e-4)
        else:
            val, _ = oracle_mod.policy_critic(P, obs, carry0, reset)
            got = PT.critic_value(f64(P), f64(obs), f64(carry0), torch.from_numpy(reset))
            np.testing.assert_allclose(val, got.numpy(), rtol=1e-5, atol=2e-5)


def test_reset_cuts_the_helper_gradient():
    """Nothing before a reset reaches the gradient of what comes after it (train.py:1719-1723)."""
    P = torch.from_numpy(init_params(CRITIC, seed=2)).double().requires_grad_()
    g = torch.Generator().manual_seed(0)
    obs = torch.randn(3, 2, 484, generator=g, dtype=torch.float64)
    c0 = torch.randn(2, D, H, generator=g, dtype=torch.float64)
    reset = torch.tensor([[0, 0], [0, 0], [1, 0]], dtype=torch.uint8)
    grads = []
    for o in (obs, torch.cat([obs[:2] + torch.tensor([1.0, 0.0])[None, :, None], obs[2:]])):
        v = PT.critic_value(P, o, c0, reset)
        grads.append(torch.autograd.grad(v[2, 0], P)[0])
    assert torch.equal(grads[0], grads[1])
