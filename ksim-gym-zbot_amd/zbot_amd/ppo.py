"""Post-rollout PPO inputs on the GPU.

Mirrors ksim 0.1.99's ``compute_ppo_inputs`` (un-vendored ksim/task/ppo.py
[U]) — the step PPOTask runs on a finished rollout, after get_ppo_variables
(train.py:1683-1729) has produced the critic values:

    inputs = compute_ppo_inputs(values_t, rewards_t, dones_t, successes_t,
                                decay_gamma=0.99, gae_lambda=0.95,
                                normalize_advantages=True)
    inputs.advantages_t, inputs.value_targets_t, inputs.gae_t, inputs.returns_t

All arrays are [T, n] torch device tensors, time-major with the env axis
contiguous — the buffers zb_step fills when handed row t of a rollout buffer.
The arithmetic runs in libzbot_hip.so (include/zbot_ppo.h); there is no
PyTorch or CPU fallback.

Multi-GPU: each rank holds its own envs. The advantage mean/std are global:
every rank's (sum, sum of squares) is all-gathered (RCCL over xGMI; gloo on
CPU in the tests) and combined in rank order by the same pairwise tree the
kernel uses, so normalized advantages are bit-identical on every rank and —
for power-of-two env counts per rank — independent of the world size.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from .engine import ZbError, _check, load_library

DEFAULT_GAMMA = 0.99  # ksim PPOConfig.gamma default [U]
DEFAULT_LAMBDA = 0.95  # ksim PPOConfig.lam default [U]
ADV_EPS = 1e-6  # (gae - mean) / (std + 1e-6) [U]


@dataclass
class PPOInputs:
    advantages_t: object
    value_targets_t: object
    gae_t: object
    returns_t: object


def _stream(torch, dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _as(t, dtype, dev, torch):
    if t is None:
        return None
    if t.dtype != dtype or t.device != dev or not t.is_contiguous():
        t = t.to(device=dev, dtype=dtype).contiguous()
    return t


def gae(rewards_t, values_t, dones_t, decay_gamma: float = DEFAULT_GAMMA, gae_lambda: float = DEFAULT_LAMBDA,
        successes_t=None, bootstrap=None, with_moments: bool = True):
    """GAE + value targets on the GPU -> (gae [T, n], value_targets [T, n], moments [2] fp64 or None)."""
    import torch  # noqa: PLC0415

    L = load_library()
    dev = values_t.device
    if dev.type != "cuda":
        raise ZbError("ppo.gae runs on the GPU (libzbot_hip.so); got tensors on " + str(dev))
    T, n = values_t.shape
    rewards_t = _as(rewards_t, torch.float32, dev, torch)
    values_t = _as(values_t, torch.float32, dev, torch)
    dones_t = _as(dones_t, torch.uint8, dev, torch)
    successes_t = _as(successes_t, torch.uint8, dev, torch)
    bootstrap = _as(bootstrap, torch.float32, dev, torch)
    for name, t in (("rewards_t", rewards_t), ("dones_t", dones_t), ("successes_t", successes_t)):
        if t is not None and tuple(t.shape) != (T, n):
            raise ZbError(f"{name} must be [{T}, {n}], got {tuple(t.shape)}")
    if bootstrap is not None and tuple(bootstrap.shape) != (n,):
        raise ZbError(f"bootstrap must be [{n}]")
    g = torch.empty(T, n, dtype=torch.float32, device=dev)
    vt = torch.empty(T, n, dtype=torch.float32, device=dev)
    part = mom = None
    if with_moments:
        part = torch.empty(max(int(L.zb_gae_partials_words(n)), 2), dtype=torch.float64, device=dev)
        mom = torch.empty(2, dtype=torch.float64, device=dev)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _check(L.zb_gae(p(rewards_t), p(values_t), p(dones_t), p(successes_t), p(bootstrap), T, n,
                    C.c_float(decay_gamma), C.c_float(gae_lambda), p(g), p(vt), p(part), p(mom),
                    _stream(torch, dev)))
    return g, vt, mom


def pairwise_tree_host(pairs):
    """The kernel's rank-combine tree on host fp64 values ([k, 2] -> [2]); used for CPU (gloo) tensors."""
    import torch  # noqa: PLC0415

    a = [[float(x[0]), float(x[1])] for x in pairs.tolist()]
    p = 1
    while p < len(a):
        p <<= 1
    a += [[0.0, 0.0]] * (p - len(a))
    s = 1
    while s < p:
        for i in range(0, p - s, 2 * s):
            a[i] = [a[i][0] + a[i + s][0], a[i][1] + a[i + s][1]]
        s <<= 1
    return torch.tensor(a[0] if a else [0.0, 0.0], dtype=torch.float64)


def combine_moments(moments, group=None):
    """Global (sum, sum^2) from per-rank moments: all-gather + rank-order pairwise tree (every rank)."""
    import torch  # noqa: PLC0415
    import torch.distributed as dist  # noqa: PLC0415

    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return moments
    world = dist.get_world_size(group)
    parts = [torch.zeros_like(moments) for _ in range(world)]
    dist.all_gather(parts, moments, group=group)
    stacked = torch.stack(parts).contiguous()
    if stacked.device.type != "cuda":
        # gloo on CPU tensors: the same tree on the host, handed back on the caller's device
        return pairwise_tree_host(stacked).to(moments.device)
    out = torch.empty(2, dtype=torch.float64, device=stacked.device)
    _check(load_library().zb_moments_combine(stacked.data_ptr(), world, out.data_ptr(),
                                             _stream(torch, stacked.device)))
    return out


def global_count(local: int, group=None) -> int:
    import torch.distributed as dist  # noqa: PLC0415

    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return local
    import torch  # noqa: PLC0415

    t = torch.tensor([local], dtype=torch.int64)
    if dist.get_backend(group) == "nccl":
        t = t.cuda()
    dist.all_reduce(t, group=group)
    return int(t.item())


def normalize(gae_t, moments, total: float, eps: float = ADV_EPS, out=None):
    """(gae - mean) / (std + eps) with mean/std from global moments over `total` elements."""
    import torch  # noqa: PLC0415

    dev = gae_t.device
    if dev.type != "cuda":
        raise ZbError("ppo.normalize runs on the GPU (libzbot_hip.so)")
    if (not isinstance(moments, torch.Tensor) or moments.dtype != torch.float64 or moments.numel() != 2
            or moments.device != dev or not moments.is_contiguous()):
        # the kernel dereferences moments[0..1] on the device: a host pointer would fault the GPU
        raise ZbError(f"moments must be a contiguous float64 tensor of 2 elements on {dev}")
    if gae_t.dtype != torch.float32 or not gae_t.is_contiguous():
        raise ZbError("gae_t must be a contiguous float32 tensor")
    if out is None:
        out = torch.empty_like(gae_t)
    elif (out.dtype != torch.float32 or out.device != dev or not out.is_contiguous()
          or out.numel() != gae_t.numel()):
        raise ZbError(f"out must be a contiguous float32 tensor of {gae_t.numel()} elements on {dev}")
    _check(load_library().zb_adv_normalize(gae_t.data_ptr(), out.data_ptr(), gae_t.numel(), moments.data_ptr(),
                                           float(total), C.c_float(eps), _stream(torch, dev)))
    return out


def compute_ppo_inputs(values_t, rewards_t, dones_t, successes_t=None, decay_gamma: float = DEFAULT_GAMMA,
                       gae_lambda: float = DEFAULT_LAMBDA, normalize_advantages: bool = True,
                       monte_carlo_returns: bool = False, bootstrap=None, group=None) -> PPOInputs:
    """ksim-shaped entry point (argument names follow ksim's compute_ppo_inputs [U])."""
    if monte_carlo_returns:
        raise ZbError("monte_carlo_returns is not built (ksim's default is False [U])")
    g, vt, mom = gae(rewards_t, values_t, dones_t, decay_gamma, gae_lambda, successes_t, bootstrap,
                     with_moments=normalize_advantages)
    adv = g
    if normalize_advantages:
        gm = combine_moments(mom, group)
        total = global_count(g.numel(), group)
        adv = normalize(g, gm, total)
    return PPOInputs(advantages_t=adv, value_targets_t=vt, gae_t=g, returns_t=vt)


# ---- the learner's three steps around the backward pass (include/zbot_ppo.h "Learner") ----
# zbot_amd.learner's defaults (ksim PPOConfig [U]; optax.adamw [U]), repeated here because learner imports this module
_CLIP_PARAM, _VALUE_LOSS_COEF, _USE_CLIPPED_VALUE_LOSS, _LOG_CLIP_VALUE = 0.2, 0.5, True, 10.0
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8  # optax.adamw's defaults [U], torch.optim.AdamW's too
JOINTS = 20


def _f32_dev(t, dev, torch, name):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
        raise ZbError(f"{name} must be a contiguous float32 tensor on {dev}")
    return t


def _f64_dev(t, dev, torch, name, numel):
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != dev or not t.is_contiguous()
            or t.numel() < numel):
        raise ZbError(f"{name} must be a contiguous float64 tensor of at least {numel} elements on {dev}")
    return t


def ppo_loss_grad(log_prob, old_log_prob, advantages, values, old_values, value_targets, total: float | None = None,
                  clip_param: float = _CLIP_PARAM, value_loss_coef: float = _VALUE_LOSS_COEF,
                  use_clipped_value_loss: bool = _USE_CLIPPED_VALUE_LOSS, log_clip_value: float = _LOG_CLIP_VALUE,
                  d_log_prob=None, d_value=None, sums=None, partials=None):
    """zb_ppo_loss: the seeds of learner.ppo_loss's gradient and its sums, on the GPU, asynchronously.

    log_prob / old_log_prob [T, n, 20]; advantages, values, old_values, value_targets [T, n] (float32,
    contiguous, one device). total: rows the means run over (default T n).
    -> (d_log_prob [T, n, 20], d_value [T, n], sums [4] float64: sum S, sum Vt, sum clipped, sum kl);
    loss = -sums[0] / total + value_loss_coef * 0.5 * sums[1] / total. The optional outputs and the
    `partials` scratch are reused when given (sums may be longer than 4: the first 4 are written)."""
    import torch  # noqa: PLC0415

    L = load_library()
    dev = log_prob.device
    if dev.type != "cuda":
        raise ZbError("ppo.ppo_loss_grad runs on the GPU (libzbot_hip.so); ppo_loss_grad_host is the CPU twin")
    if log_prob.dim() != 3 or log_prob.shape[2] != JOINTS:
        raise ZbError(f"log_prob must be [T, n, {JOINTS}], got {list(log_prob.shape)}")
    T, n, _ = log_prob.shape
    _f32_dev(log_prob, dev, torch, "log_prob")
    if tuple(_f32_dev(old_log_prob, dev, torch, "old_log_prob").shape) != (T, n, JOINTS):
        raise ZbError(f"old_log_prob must be [{T}, {n}, {JOINTS}]")
    for name, t in (("advantages", advantages), ("values", values), ("old_values", old_values),
                    ("value_targets", value_targets)):
        if tuple(_f32_dev(t, dev, torch, name).shape) != (T, n):
            raise ZbError(f"{name} must be [{T}, {n}], got {tuple(t.shape)}")
    if d_log_prob is None:
        d_log_prob = torch.empty(T, n, JOINTS, dtype=torch.float32, device=dev)
    elif _f32_dev(d_log_prob, dev, torch, "d_log_prob").numel() != T * n * JOINTS:
        raise ZbError(f"d_log_prob must hold {T * n * JOINTS} elements")
    if d_value is None:
        d_value = torch.empty(T, n, dtype=torch.float32, device=dev)
    elif _f32_dev(d_value, dev, torch, "d_value").numel() != T * n:
        raise ZbError(f"d_value must hold {T * n} elements")
    words = int(L.zb_ppo_loss_partials_words(T, n))
    partials = (torch.empty(max(words, 1), dtype=torch.float64, device=dev) if partials is None
                else _f64_dev(partials, dev, torch, "partials", words))
    sums = torch.empty(4, dtype=torch.float64, device=dev) if sums is None else _f64_dev(sums, dev, torch, "sums", 4)
    _check(L.zb_ppo_loss(log_prob.data_ptr(), old_log_prob.data_ptr(), advantages.data_ptr(), values.data_ptr(),
                         old_values.data_ptr(), value_targets.data_ptr(), T, n, float(T * n if total is None else total),
                         C.c_float(clip_param), C.c_float(value_loss_coef), 1 if use_clipped_value_loss else 0,
                         C.c_float(log_clip_value), d_log_prob.data_ptr(), d_value.data_ptr(), partials.data_ptr(),
                         sums.data_ptr(), _stream(torch, dev)))
    return d_log_prob, d_value, sums


def grad_sqnorm(grad, out=None, partials=None):
    """zb_grad_sqnorm: sum of squares of a float32 device tensor -> out [1] float64 (fixed fp64 tree)."""
    import torch  # noqa: PLC0415

    L = load_library()
    dev = grad.device
    if dev.type != "cuda":
        raise ZbError("ppo.grad_sqnorm runs on the GPU (libzbot_hip.so); grad_sqnorm_host is the CPU twin")
    _f32_dev(grad, dev, torch, "grad")
    words = int(L.zb_sqnorm_partials_words(grad.numel()))
    partials = (torch.empty(max(words, 1), dtype=torch.float64, device=dev) if partials is None
                else _f64_dev(partials, dev, torch, "partials", words))
    out = torch.empty(1, dtype=torch.float64, device=dev) if out is None else _f64_dev(out, dev, torch, "out", 1)
    _check(L.zb_grad_sqnorm(grad.data_ptr(), grad.numel(), partials.data_ptr(), out.data_ptr(), _stream(torch, dev)))
    return out


SUMMARY_WORDS = 32  # ZB_SUMMARY_WORDS
_SUMMARY_PLANES = (("reward_terms", 12), ("command_terms", 5), ("reward", 0), ("done", 0), ("success", 0),
                   ("log_prob", JOINTS), ("values", 0), ("value_targets", 0))  # name, trailing axis (0: none)
_summary_partials: dict = {}  # (device, words) -> scratch, reused between calls on one stream


def _summary_shapes(planes: dict, shape_of):
    """(T, n) of the planes of a rollout summary, each checked against [T, n(, k)]."""
    if planes["reward"] is None or planes["done"] is None:
        raise ZbError("rollout_summary needs reward and done")
    if (planes["values"] is None) != (planes["value_targets"] is None):
        raise ZbError("rollout_summary: values and value_targets go together (both or neither)")
    rs = tuple(shape_of(planes["reward"]))
    if len(rs) != 2 or rs[0] < 1 or rs[1] < 1:
        raise ZbError(f"reward must be [T, n] with T, n >= 1, got {list(rs)}")
    T, n = rs
    for name, k in _SUMMARY_PLANES:
        t = planes[name]
        want = (T, n, k) if k else (T, n)
        if t is not None and tuple(shape_of(t)) != want:
            raise ZbError(f"{name} must be {list(want)}, got {list(shape_of(t))}")
    return T, n


def rollout_summary(reward, done, success=None, reward_terms=None, command_terms=None, log_prob=None, values=None,
                    value_targets=None, out=None, partials=None):
    """zb_rollout_summary: the 32 fp64 sums of a rollout (cstructs.SUM_*; include/zbot_ppo.h "Rollout
    summary") by the fixed pairwise tree over the T n rows in (t, env) order, on the GPU,
    asynchronously on the current stream. reward [T, n] float32, done / success [T, n] uint8,
    reward_terms [T, n, 12], command_terms [T, n, 5], log_prob [T, n, 20], values / value_targets
    [T, n] float32 (both or neither): contiguous device tensors (views at any element offset are
    fine); the words of an absent plane are +0.0. -> out [32] float64. `out` and the `partials`
    scratch are reused when given; without `partials` one scratch per device and size is kept and
    reused (calls on different streams of a device should pass their own)."""
    import torch  # noqa: PLC0415

    L = load_library()
    if not isinstance(reward, torch.Tensor):
        raise ZbError("reward must be a float32 device tensor")
    dev = reward.device
    if dev.type != "cuda":
        raise ZbError("ppo.rollout_summary runs on the GPU (libzbot_hip.so); rollout_summary_host is the CPU twin")
    planes = dict(reward_terms=reward_terms, command_terms=command_terms, reward=reward, done=done, success=success,
                  log_prob=log_prob, values=values, value_targets=value_targets)
    T, n = _summary_shapes(planes, lambda t: t.shape)
    for name, _ in _SUMMARY_PLANES:
        t = planes[name]
        if t is None:
            continue
        dt = torch.uint8 if name in ("done", "success") else torch.float32
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ZbError(f"{name} must be a contiguous {dt} tensor on {dev}")
    words = int(L.zb_rollout_summary_partials_words(T, n))
    if words == 0:
        raise ZbError(f"rollout_summary: T * n = {T} * {n} rows (1 to 2^28)")
    if partials is None:
        partials = _summary_partials.get((dev, words))
        if partials is None:
            partials = _summary_partials[(dev, words)] = torch.empty(words, dtype=torch.float64, device=dev)
    else:
        _f64_dev(partials, dev, torch, "partials", words)
    out = (torch.empty(SUMMARY_WORDS, dtype=torch.float64, device=dev) if out is None
           else _f64_dev(out, dev, torch, "out", SUMMARY_WORDS))
    p = lambda name: None if planes[name] is None else planes[name].data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        _check(L.zb_rollout_summary(*(p(name) for name, _ in _SUMMARY_PLANES), T, n, partials.data_ptr(),
                                    out.data_ptr(), _stream(torch, dev)))
    return out[:SUMMARY_WORDS]


def rollout_summary_host(reward, done, success=None, reward_terms=None, command_terms=None, log_prob=None,
                         values=None, value_targets=None):
    """zb_rollout_summary_host: the same leaves and the same tree on the CPU (numpy arrays or CPU
    tensors in, a float64 tensor [32] out): the kernel's bit reference."""
    import numpy as np  # noqa: PLC0415
    import torch  # noqa: PLC0415

    planes = dict(reward_terms=reward_terms, command_terms=command_terms, reward=reward, done=done, success=success,
                  log_prob=log_prob, values=values, value_targets=value_targets)
    for name, _ in _SUMMARY_PLANES:
        if planes[name] is not None:
            planes[name] = _host(planes[name], np.uint8 if name in ("done", "success") else np.float32, name)
    T, n = _summary_shapes(planes, lambda a: a.shape)
    out = np.empty(SUMMARY_WORDS, np.float64)
    _check(load_library().zb_rollout_summary_host(
        *(None if planes[name] is None else planes[name].ctypes.data for name, _ in _SUMMARY_PLANES), T, n,
        out.ctypes.data))
    return torch.from_numpy(out)


COMBINE_MAX_WORLD = 64  # ZB_COMBINE_MAX_WORLD


def grad_combine(parts, out=None, sq_out=None, partials=None):
    """zb_grad_combine: the sum over ranks of an all-gathered gradient, by the fixed fp64 tree in rank
    order. parts [world, count] float32 on the device, contiguous (zbot_amd.dist.all_gather_rows'
    destination) -> (out [count] float32, sq_out [1] float64): the sum rounded to float32 once, and
    the bits grad_sqnorm(out) would return. `out` must not overlap `parts`; the optional outputs and
    the `partials` scratch (as grad_sqnorm's) are reused when given."""
    import torch  # noqa: PLC0415

    L = load_library()
    dev = parts.device
    if dev.type != "cuda":
        raise ZbError("ppo.grad_combine runs on the GPU (libzbot_hip.so); grad_combine_host is the CPU twin")
    if _f32_dev(parts, dev, torch, "parts").dim() != 2:
        raise ZbError(f"parts must be [world, count], got {list(parts.shape)}")
    world, count = parts.shape
    if out is None:
        out = torch.empty(count, dtype=torch.float32, device=dev)
    elif _f32_dev(out, dev, torch, "out").numel() != count:
        raise ZbError(f"out must hold {count} elements")
    words = int(L.zb_sqnorm_partials_words(count))
    partials = (torch.empty(max(words, 1), dtype=torch.float64, device=dev) if partials is None
                else _f64_dev(partials, dev, torch, "partials", words))
    sq_out = (torch.empty(1, dtype=torch.float64, device=dev) if sq_out is None
              else _f64_dev(sq_out, dev, torch, "sq_out", 1))
    with torch.cuda.device(dev):
        _check(L.zb_grad_combine(parts.data_ptr(), int(world), int(count), out.data_ptr(), partials.data_ptr(),
                                 sq_out.data_ptr(), _stream(torch, dev)))
    return out, sq_out


def grad_combine_host(parts):
    """zb_grad_combine_host: the same trees on the CPU, the kernel's bit definition.
    parts [world, count] float32 (numpy or a CPU tensor) -> (grad [count] float32 numpy, squared norm float)."""
    import numpy as np  # noqa: PLC0415

    p = _host(parts, np.float32, "parts")
    if p.ndim != 2:
        raise ZbError(f"parts must be [world, count], got {list(p.shape)}")
    grad, sq = np.empty(p.shape[1], np.float32), np.empty(1, np.float64)
    _check(load_library().zb_grad_combine_host(p.ctypes.data, p.shape[0], p.shape[1], grad.ctypes.data, sq.ctypes.data))
    return grad, float(sq[0])


def adamw_step(param, grad, m, v, sqnorms, step: int, lr: float, max_grad_norm: float = 0.0,
               weight_decay: float = 0.0, frozen_tail: int = 0, beta1: float = ADAM_BETA1, beta2: float = ADAM_BETA2,
               eps: float = ADAM_EPS) -> None:
    """zb_adamw_step: one AdamW step of `param`, `m`, `v` (float32 device tensors, in place) behind the
    global-norm clip over all of `sqnorms` (float64 device tensor of k squared norms; max_grad_norm
    0: no clip). The last `frozen_tail` elements stay as they are. `step` counts from 1."""
    import torch  # noqa: PLC0415

    dev = param.device
    if dev.type != "cuda":
        raise ZbError("ppo.adamw_step runs on the GPU (libzbot_hip.so); adamw_step_host is the CPU twin")
    for name, t in (("param", param), ("grad", grad), ("m", m), ("v", v)):
        if _f32_dev(t, dev, torch, name).numel() != param.numel():
            raise ZbError(f"{name} must hold {param.numel()} elements")
    k = sqnorms.numel()
    _f64_dev(sqnorms, dev, torch, "sqnorms", 1)
    _check(load_library().zb_adamw_step(param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), param.numel(),
                                        int(frozen_tail), sqnorms.data_ptr(), k, C.c_float(max_grad_norm),
                                        C.c_float(lr), float(beta1), float(beta2), C.c_float(eps),
                                        C.c_float(weight_decay), int(step), _stream(torch, dev)))


# ---- minibatches: the keyed permutation and the fused gather (include/zbot_ppo.h "Minibatches") ----
GATHER_MAX_ITEMS = 16  # ZB_GATHER_MAX_ITEMS


class ZbGatherItem(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int32), ("row_bytes", C.c_int32),
                ("src_t_stride_bytes", C.c_int64)]


def _perm_args(n, seed, epoch):
    n, seed, epoch = int(n), int(seed), int(epoch)
    if n < 1 or not 0 <= seed < 1 << 64 or not 0 <= epoch < 1 << 32:
        raise ZbError(f"minibatch permutation: n >= 1, a 64-bit seed and a 32-bit epoch, got {n}, {seed}, {epoch}")
    return n, seed, epoch


def minibatch_perm(n: int, seed: int, epoch: int = 0, device=None):
    """zb_minibatch_perm: perm[i] = zbf_perm_index(seed, epoch, n, i), an int32 device tensor [n]: the
    order in which pass `epoch` of a learner with shuffle_seed=seed visits the n envs."""
    import torch  # noqa: PLC0415

    n, seed, epoch = _perm_args(n, seed, epoch)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ZbError("ppo.minibatch_perm runs on the GPU (libzbot_hip.so); minibatch_perm_host is the CPU twin")
    out = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(load_library().zb_minibatch_perm(seed, epoch, n, out.data_ptr(), _stream(torch, dev)))
    return out


def minibatch_perm_host(n: int, seed: int, epoch: int = 0):
    """zb_minibatch_perm_host: the same permutation on the CPU, an int32 numpy array [n]."""
    import numpy as np  # noqa: PLC0415

    n, seed, epoch = _perm_args(n, seed, epoch)
    out = np.empty(n, np.int32)
    _check(load_library().zb_minibatch_perm_host(seed, epoch, n, out.ctypes.data))
    return out


def _gather_table(items, n, count, describe, seq_len=None):
    """The ZbGatherItem array of `items`, pairs (src, dst): dst [rows, count, ...] dense, src
    [>= rows, n, ...] with the same trailing shape and dtype, dense below its first axis (any stride
    along it), or None for zeros. `describe(x)` -> (address, shape, strides in bytes, itemsize, dtype).
    With seq_len = L also the int32 `cut` array of zb_minibatch_gather_seq: an item given as a triple
    (src, dst, True) is a time item, dst [L, C count, ...], of rows = L C cut in chunks; a pair is not."""
    items = list(items)
    if not 1 <= len(items) <= GATHER_MAX_ITEMS:
        raise ZbError(f"gather_minibatch takes 1 to {GATHER_MAX_ITEMS} items, got {len(items)}")
    table = (ZbGatherItem * len(items))()
    cut = None if seq_len is None else (C.c_int32 * len(items))()  # the plain gather does what it always did
    for k, item in enumerate(items):
        if len(item) not in (2, 3):
            raise ZbError(f"item {k}: (src, dst), or (src, dst, True) for a time item cut in chunks of seq_len")
        src, dst = item[0], item[1]
        dp, dshape, dstr, isz, ddt = describe(dst)
        chunks = 1
        if len(item) == 3 and item[2]:
            if cut is None:
                raise ZbError(f"item {k} is marked as a time item to be cut in chunks, but no seq_len is given")
            if len(dshape) < 2 or dshape[0] != seq_len or dshape[1] < count or dshape[1] % count:
                raise ZbError(f"item {k}: a time item's dst must be [seq_len = {seq_len}, C x {count}, ...], got "
                              f"{list(dshape)}")
            chunks = dshape[1] // count
            cut[k] = 1
        elif len(dshape) < 2 or dshape[1] != count or dshape[0] < 1:
            raise ZbError(f"item {k}: dst must be [rows, {count}, ...], got {list(dshape)}")
        dense = [isz] * len(dshape)
        for a in range(len(dshape) - 2, -1, -1):
            dense[a] = dense[a + 1] * dshape[a + 1]
        if any(st != dn for st, dn, sz in zip(dstr, dense, dshape) if sz != 1):  # a size-1 axis has no stride
            raise ZbError(f"item {k}: dst must be contiguous")
        rows, row_bytes = dshape[0] * chunks, dense[1]
        sp, stride = None, 0
        if src is not None:
            sp, sshape, sstr, _, sdt = describe(src)
            if (sdt != ddt or len(sshape) != len(dshape) or sshape[0] < rows or sshape[1] != n
                    or tuple(sshape[2:]) != tuple(dshape[2:])):
                raise ZbError(f"item {k}: src {list(sshape)} {sdt} does not feed dst {list(dshape)} {ddt} over "
                              f"{n} envs" + (f" in {chunks} chunks of seq_len={seq_len}" if cut is not None and cut[k] else ""))
            if any(st != dn for st, dn, sz in zip(sstr[1:], dense[1:], sshape[1:]) if sz != 1) or sstr[0] < 0:
                raise ZbError(f"item {k}: src must be dense below its first axis")
            stride = sstr[0] if rows > 1 else 0
        table[k] = ZbGatherItem(sp, dp, rows, row_bytes, stride)
    return table, cut


def _seq_len(seq_len):
    if seq_len is None:
        return None
    if int(seq_len) != seq_len or int(seq_len) < 1:
        raise ZbError(f"gather_minibatch: seq_len must be an integer >= 1, got {seq_len!r}")
    return int(seq_len)


def gather_minibatch(items, n: int, lo: int, count: int, shuffle_seed: int | None = None, epoch: int = 0,
                     seq_len: int | None = None) -> None:
    """zb_minibatch_gather: one launch that cuts every array of a minibatch. For each pair (src, dst)
    of `items` (device tensors; at most 16) and every t < rows, j < count:
    dst[t, j] = src[t, p(lo + j)], p = minibatch_perm(n, shuffle_seed, epoch), or the identity (a
    slice) when shuffle_seed is None. dst is [rows, count, ...], contiguous; src is [>= rows, n, ...]
    of the same dtype and trailing shape, dense below its first axis (the first T rows of a [T + 1]
    buffer, or any stride along time), or None, which fills dst with zeros. A per-env array such as
    a carry goes in as src[None], dst[None]. Asynchronous on the current stream; allocates nothing
    on the device.

    seq_len = L (zb_minibatch_gather_seq, truncated BPTT): an item given as (src, dst, True) is a time
    item, dst [L, C count, ...], whose T = L C source rows are cut in C chunks,
    dst[l, c count + j] = src[c L + l, p(lo + j)]; a pair (src, dst) moves as above (the carries stored
    at the chunk starts: src [C, n, ...], dst [C, count, ...], then viewed as the C count sequences'
    carry0)."""
    import torch  # noqa: PLC0415

    items = list(items)
    dev = items[0][1].device if items else None
    if dev is None or dev.type != "cuda":
        raise ZbError("ppo.gather_minibatch runs on the GPU (libzbot_hip.so); gather_minibatch_host is the CPU twin")

    def describe(x):
        if not isinstance(x, torch.Tensor) or x.device != dev:
            raise ZbError(f"gather_minibatch: every tensor must live on {dev}")
        isz = x.element_size()
        return x.data_ptr(), tuple(x.shape), tuple(s * isz for s in x.stride()), isz, x.dtype

    n, seed, epoch = _perm_args(n, 0 if shuffle_seed is None else shuffle_seed, epoch)
    seq_len = _seq_len(seq_len)
    table, cut = _gather_table(items, n, int(count), describe, seq_len)
    shuffle = 0 if shuffle_seed is None else 1
    with torch.cuda.device(dev):
        if seq_len is None:
            _check(load_library().zb_minibatch_gather(table, len(table), n, int(lo), int(count), shuffle, seed, epoch,
                                                      _stream(torch, dev)))
        else:
            _check(load_library().zb_minibatch_gather_seq(table, cut, len(table), seq_len, n, int(lo), int(count),
                                                          shuffle, seed, epoch, _stream(torch, dev)))


def gather_minibatch_host(items, n: int, lo: int, count: int, shuffle_seed: int | None = None, epoch: int = 0,
                          seq_len: int | None = None) -> None:
    """zb_minibatch_gather_host (with seq_len: zb_minibatch_gather_seq_host): gather_minibatch on numpy
    arrays (or CPU tensors), in place on each dst."""
    import numpy as np  # noqa: PLC0415

    def describe(x):
        if hasattr(x, "detach"):
            if x.device.type != "cpu":
                raise ZbError("gather_minibatch_host takes CPU tensors or numpy arrays")
            x = x.detach().numpy()
        if not isinstance(x, np.ndarray):
            raise ZbError("gather_minibatch_host takes CPU tensors or numpy arrays")
        return x.ctypes.data, x.shape, x.strides, x.itemsize, x.dtype

    n, seed, epoch = _perm_args(n, 0 if shuffle_seed is None else shuffle_seed, epoch)
    seq_len = _seq_len(seq_len)
    table, cut = _gather_table(list(items), n, int(count), describe, seq_len)
    shuffle = 0 if shuffle_seed is None else 1
    if seq_len is None:
        _check(load_library().zb_minibatch_gather_host(table, len(table), n, int(lo), int(count), shuffle, seed, epoch))
    else:
        _check(load_library().zb_minibatch_gather_seq_host(table, cut, len(table), seq_len, n, int(lo), int(count),
                                                           shuffle, seed, epoch))


def _host(a, dtype, name, writable=False):
    """A contiguous numpy view of a CPU tensor or numpy array (no copy: the twins write in place)."""
    import numpy as np  # noqa: PLC0415

    if hasattr(a, "detach"):
        if a.device.type != "cpu":
            raise ZbError(f"{name}: the host twins take CPU tensors or numpy arrays")
        a = a.detach().numpy()
    if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous or (writable and not a.flags.writeable):
        raise ZbError(f"{name} must be a contiguous {np.dtype(dtype).name} array")
    return a


def ppo_loss_grad_host(log_prob, old_log_prob, advantages, values, old_values, value_targets,
                       total: float | None = None, clip_param: float = _CLIP_PARAM,
                       value_loss_coef: float = _VALUE_LOSS_COEF,
                       use_clipped_value_loss: bool = _USE_CLIPPED_VALUE_LOSS, log_clip_value: float = _LOG_CLIP_VALUE):
    """zb_ppo_loss_host: ppo_loss_grad on the CPU (numpy in, numpy out), the kernels' bit reference."""
    import numpy as np  # noqa: PLC0415

    lp = _host(log_prob, np.float32, "log_prob")
    if lp.ndim != 3 or lp.shape[2] != JOINTS:
        raise ZbError(f"log_prob must be [T, n, {JOINTS}]")
    T, n, _ = lp.shape
    olp = _host(old_log_prob, np.float32, "old_log_prob")
    rest = [_host(x, np.float32, nm) for nm, x in (("advantages", advantages), ("values", values),
                                                    ("old_values", old_values), ("value_targets", value_targets))]
    if olp.shape != lp.shape or any(x.shape != (T, n) for x in rest):
        raise ZbError(f"shapes must be [{T}, {n}, {JOINTS}] and [{T}, {n}]")
    d_lp, d_v, sums = np.empty((T, n, JOINTS), np.float32), np.empty((T, n), np.float32), np.empty(4, np.float64)
    _check(load_library().zb_ppo_loss_host(lp.ctypes.data, olp.ctypes.data, *(x.ctypes.data for x in rest), T, n,
                                           float(T * n if total is None else total), C.c_float(clip_param),
                                           C.c_float(value_loss_coef), 1 if use_clipped_value_loss else 0,
                                           C.c_float(log_clip_value), d_lp.ctypes.data, d_v.ctypes.data,
                                           sums.ctypes.data))
    return d_lp, d_v, sums


def grad_sqnorm_host(grad) -> float:
    """zb_grad_sqnorm_host: the same tree on the CPU."""
    import numpy as np  # noqa: PLC0415

    g = _host(grad, np.float32, "grad")
    out = np.empty(1, np.float64)
    _check(load_library().zb_grad_sqnorm_host(g.ctypes.data, g.size, out.ctypes.data))
    return float(out[0])


def adamw_step_host(param, grad, m, v, sqnorms, step: int, lr: float, max_grad_norm: float = 0.0,
                    weight_decay: float = 0.0, frozen_tail: int = 0, beta1: float = ADAM_BETA1,
                    beta2: float = ADAM_BETA2, eps: float = ADAM_EPS) -> None:
    """zb_adamw_step_host: adamw_step on the CPU, in place on param, m, v."""
    import numpy as np  # noqa: PLC0415

    p, mm, vv = (_host(x, np.float32, nm, writable=True) for nm, x in (("param", param), ("m", m), ("v", v)))
    g = _host(grad, np.float32, "grad")
    sq = np.ascontiguousarray(np.asarray(sqnorms, dtype=np.float64).reshape(-1))
    if not (g.size == mm.size == vv.size == p.size):
        raise ZbError(f"grad, m and v must hold {p.size} elements")
    _check(load_library().zb_adamw_step_host(p.ctypes.data, g.ctypes.data, mm.ctypes.data, vv.ctypes.data, p.size,
                                             int(frozen_tail), sq.ctypes.data, sq.size, C.c_float(max_grad_norm),
                                             C.c_float(lr), float(beta1), float(beta2), C.c_float(eps),
                                             C.c_float(weight_decay), int(step)))
