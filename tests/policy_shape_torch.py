"""tests/policy_torch.py with the network shape as an argument (helper, not a test).

The same operations in the same order with `depth` GRU layers and `mixtures` components per joint in
place of the constants 5 and 5, so at (5, 5) the fp64 results are policy_torch's to the bit
(tests/test_policy_shape_host.py checks that). It is the autograd reference of the shaped handles'
backward pass (tests/test_gpu_policy_shape.py) and the fp64 reference of their host twins.
"""

import math

import torch

H, NJ = 128, 20
ACTOR_IN, CRITIC_IN = 50, 484


def names(actor: bool, depth: int):
    out = ["input_proj.weight", "input_proj.bias"]
    for l in range(depth):
        out += [f"rnn{l}.weight_ih", f"rnn{l}.weight_hh", f"rnn{l}.bias", f"rnn{l}.bias_n"]
    return out + ["output_proj.weight", "output_proj.bias"]


def shapes(actor: bool, depth: int, mixtures: int):
    I, O = (ACTOR_IN, 3 * NJ * mixtures) if actor else (CRITIC_IN, 1)
    out = [(H, I), (H,)]
    for _ in range(depth):
        out += [(3 * H, H), (3 * H, H), (3 * H,), (H,)]
    return out + [(O, H), (O,)]


def split(flat, actor: bool, depth: int, mixtures: int):
    """{name: view} of a flat natural-layout parameter tensor (+ 'mean_bias' for the actor)."""
    out, i = {}, 0
    for name, shp in zip(names(actor, depth), shapes(actor, depth, mixtures)):
        k = math.prod(shp)
        out[name] = flat[i:i + k].reshape(shp)
        i += k
    if actor:
        out["mean_bias"] = flat[i:i + NJ]
        i += NJ
    assert i == flat.numel()
    return out


def trunk(flat, actor: bool, depth: int, mixtures: int, obs, carry0, reset, carry_out=None):
    """obs [T, n, I], carry0 [n, depth, H], reset [T, n] or None -> output_proj [T, n, O]. carry_out: a list
    that receives the final carry [n, depth, H]."""
    p = split(flat, actor, depth, mixtures)
    T = obs.shape[0]
    h = [carry0[:, l] for l in range(depth)]
    outs = []
    for t in range(T):
        if reset is not None:
            keep = (reset[t] == 0).to(flat.dtype)[:, None]
            h = [x * keep for x in h]
        x = obs[t] @ p["input_proj.weight"].T + p["input_proj.bias"]
        for l in range(depth):
            ig = x @ p[f"rnn{l}.weight_ih"].T + p[f"rnn{l}.bias"]
            hg = h[l] @ p[f"rnn{l}.weight_hh"].T
            r = torch.sigmoid(ig[:, :H] + hg[:, :H])
            z = torch.sigmoid(ig[:, H:2 * H] + hg[:, H:2 * H])
            nn = torch.tanh(ig[:, 2 * H:] + r * (hg[:, 2 * H:] + p[f"rnn{l}.bias_n"]))
            x = nn + z * (h[l] - nn)
            h[l] = x
        outs.append(x @ p["output_proj.weight"].T + p["output_proj.bias"])
    if carry_out is not None:
        carry_out.append(torch.stack(h, dim=1))
    return torch.stack(outs)


def head(flat, depth: int, mixtures: int, out):
    """out [..., 60 m] -> (mu, sd, logits, unclipped) each [..., 20, m] (train.py:952-965)."""
    mb = split(flat, True, depth, mixtures)["mean_bias"]
    lead = out.shape[:-1]
    k = NJ * mixtures
    mu = out[..., :k].reshape(*lead, NJ, mixtures) + mb[:, None]
    s = torch.nn.functional.softplus(out[..., k:2 * k].reshape(*lead, NJ, mixtures)) + 0.01
    sd = torch.clamp(s, max=1.0)
    lg = out[..., 2 * k:3 * k].reshape(*lead, NJ, mixtures)
    return mu, sd, lg, s < 1.0


def mix_log_prob(mu, sd, lg, a):
    logw = torch.log_softmax(lg, dim=-1)
    z = (a[..., None] - mu) / sd
    return torch.logsumexp(logw - 0.5 * z * z - torch.log(sd) - 0.5 * math.log(2 * math.pi), dim=-1)


def actor_log_prob(flat, depth: int, mixtures: int, obs, carry0, reset, actions, carry_out=None):
    """[T, n, 20] per-joint log-probs of `actions`."""
    mu, sd, lg, _ = head(flat, depth, mixtures, trunk(flat, True, depth, mixtures, obs, carry0, reset, carry_out))
    return mix_log_prob(mu, sd, lg, actions)


def critic_value(flat, depth: int, obs, carry0, reset, carry_out=None):
    """[T, n] values."""
    return trunk(flat, False, depth, 1, obs, carry0, reset, carry_out)[..., 0]
