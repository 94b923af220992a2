"""Torch restatement of train.py's Actor / Critic forward over T steps (helper, not a test).

Actor.forward / Critic.forward (train.py:943-950, 1011-1017) with equinox's GRUCell [U], the
carry reset of get_ppo_variables (train.py:1719-1723) and ksim's MixtureOfGaussians log-prob [U]
with the std clip of train.py:961, in plain differentiable torch ops at the dtype of the
parameter tensor handed in. It is the autograd reference of the HIP backward pass
(tests/test_gpu_policy_train.py) and the baseline of scripts/learner_timing.py;
tests/test_policy_torch_ref.py pins its fp64 forward to the CPU oracle.
"""

import math

import torch

H, D, NJ, NM = 128, 5, 20, 5
ACTOR_IN, CRITIC_IN, ACTOR_OUT = 50, 484, 300


def names(actor: bool):
    """Parameter tensor names in natural-layout order (without the actor's constant tail)."""
    out = ["input_proj.weight", "input_proj.bias"]
    for l in range(D):
        out += [f"rnn{l}.weight_ih", f"rnn{l}.weight_hh", f"rnn{l}.bias", f"rnn{l}.bias_n"]
    return out + ["output_proj.weight", "output_proj.bias"]


def shapes(actor: bool):
    I, O = (ACTOR_IN, ACTOR_OUT) if actor else (CRITIC_IN, 1)
    out = [(H, I), (H,)]
    for _ in range(D):
        out += [(3 * H, H), (3 * H, H), (3 * H,), (H,)]
    return out + [(O, H), (O,)]


def split(flat, actor: bool):
    """{name: view} of a flat natural-layout parameter tensor (+ 'mean_bias' for the actor)."""
    out, i = {}, 0
    for name, shp in zip(names(actor), shapes(actor)):
        k = math.prod(shp)
        out[name] = flat[i:i + k].reshape(shp)
        i += k
    if actor:
        out["mean_bias"] = flat[i:i + NJ]
        i += NJ
    assert i == flat.numel()
    return out


def trunk(flat, actor: bool, obs, carry0, reset):
    """obs [T, n, I], carry0 [n, D, H], reset [T, n] (bool / uint8) or None -> output_proj [T, n, O]."""
    p = split(flat, actor)
    T = obs.shape[0]
    h = [carry0[:, l] for l in range(D)]
    outs = []
    for t in range(T):
        if reset is not None:
            keep = (reset[t] == 0).to(flat.dtype)[:, None]
            h = [x * keep for x in h]
        x = obs[t] @ p["input_proj.weight"].T + p["input_proj.bias"]
        for l in range(D):
            ig = x @ p[f"rnn{l}.weight_ih"].T + p[f"rnn{l}.bias"]
            hg = h[l] @ p[f"rnn{l}.weight_hh"].T
            r = torch.sigmoid(ig[:, :H] + hg[:, :H])
            z = torch.sigmoid(ig[:, H:2 * H] + hg[:, H:2 * H])
            nn = torch.tanh(ig[:, 2 * H:] + r * (hg[:, 2 * H:] + p[f"rnn{l}.bias_n"]))
            x = nn + z * (h[l] - nn)
            h[l] = x
        outs.append(x @ p["output_proj.weight"].T + p["output_proj.bias"])
    return torch.stack(outs)


def head(flat, out):
    """out [..., 300] -> (mu, sd, logits, unclipped) each [..., 20, 5] (train.py:952-965)."""
    mb = split(flat, True)["mean_bias"]
    lead = out.shape[:-1]
    mu = out[..., :100].reshape(*lead, NJ, NM) + mb[:, None]
    s = torch.nn.functional.softplus(out[..., 100:200].reshape(*lead, NJ, NM)) + 0.01
    sd = torch.clamp(s, max=1.0)
    lg = out[..., 200:300].reshape(*lead, NJ, NM)
    return mu, sd, lg, s < 1.0


def mix_log_prob(mu, sd, lg, a):
    logw = torch.log_softmax(lg, dim=-1)
    z = (a[..., None] - mu) / sd
    return torch.logsumexp(logw - 0.5 * z * z - torch.log(sd) - 0.5 * math.log(2 * math.pi), dim=-1)


def actor_log_prob(flat, obs, carry0, reset, actions):
    """[T, n, 20] per-joint log-probs of `actions`."""
    mu, sd, lg, _ = head(flat, trunk(flat, True, obs, carry0, reset))
    return mix_log_prob(mu, sd, lg, actions)


def critic_value(flat, obs, carry0, reset):
    """[T, n] values."""
    return trunk(flat, False, obs, carry0, reset)[..., 0]
