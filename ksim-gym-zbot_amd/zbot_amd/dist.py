"""Multi-GPU sharding of environments.

Rank r of W owns global envs [r*N, (r+1)*N); every RNG stream is keyed by the
global env id, so per-env results do not depend on W. The rollout's only
collective is a tiny per-rollout reduction of episode statistics: each rank sums
its env partials in fixed env order, the partials are all-gathered (RCCL over
xGMI on GPUs, gloo on CPU) and summed in fixed rank order on every rank, which
makes the result bit-reproducible whatever ring/tree RCCL picks.

The PPO update follows the same rule: all_gather_rows only moves
every rank's gradient, and the sum over ranks is ppo.grad_combine's fixed tree.
"""

from __future__ import annotations

import os


def shard(global_envs: int, world: int, rank: int) -> tuple[int, int]:
    """(env_offset, n_envs) of `rank` for an even split."""
    if global_envs % world:
        raise ValueError(f"{global_envs} envs do not split evenly over {world} ranks")
    n = global_envs // world
    return rank * n, n


def reduce_fixed_order(part, group=None):
    """A per-rank float64 partial -> the sum over ranks, the same bits on every rank: all_gather
    (RCCL over xGMI on GPUs, gloo on CPU) and a rank-order sum, whatever algorithm the collective
    picks. Without an initialised process group: the partial itself."""
    import torch  # noqa: PLC0415
    import torch.distributed as dist  # noqa: PLC0415

    if not dist.is_available() or not dist.is_initialized():
        return part
    world = dist.get_world_size(group)
    parts = [torch.zeros_like(part) for _ in range(world)]
    dist.all_gather(parts, part, group=group)
    total = parts[0].clone()
    for p in parts[1:]:
        total += p
    return total


_stage = {}  # (group, world, count, dtype) -> (host part, host rows): all_gather_rows' gloo staging buffers


def all_gather_rows(part, out, group=None):
    """Every rank's flat tensor `part` [count] into the preallocated `out` [world, count]: row r is
    rank r's tensor, on every rank. Only moves data (the sum over rows is ppo.grad_combine's), on the
    current stream, with no allocation after the first call of a shape. Under `nccl` (RCCL) this is
    all_gather_into_tensor. Under gloo CPU tensors are gathered as they are and device tensors (the
    one-GPU rehearsal, ranks sharing a GPU) are staged through host buffers kept per shape, which
    synchronises the stream: a rehearsal's price, not the product path's. Without an initialised
    process group: a copy into row 0."""
    import torch  # noqa: PLC0415
    import torch.distributed as dist  # noqa: PLC0415

    from .engine import ZbError  # noqa: PLC0415

    live = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if live else 1
    count = part.numel()
    if (part.dim() != 1 or not part.is_contiguous() or not out.is_contiguous() or tuple(out.shape) != (world, count)
            or out.dtype != part.dtype or out.device != part.device):
        raise ZbError(f"all_gather_rows: part [count] and out [{world}, count] of one dtype and device, contiguous; "
                      f"got {list(part.shape)} and {list(out.shape)}")
    if not live:
        out[0].copy_(part)
    elif dist.get_backend(group) == "nccl":
        dist.all_gather_into_tensor(out, part, group=group)
    elif part.device.type == "cpu":
        dist.all_gather(list(out.unbind(0)), part, group=group)
    else:
        key = (group, world, count, part.dtype)
        if key not in _stage:
            _stage[key] = (torch.empty(count, dtype=part.dtype).pin_memory(),
                           torch.empty(world, count, dtype=part.dtype).pin_memory())
        hp, ho = _stage[key]
        hp.copy_(part)  # waits for the stream's work on `part`
        dist.all_gather(list(ho.unbind(0)), hp, group=group)
        out.copy_(ho, non_blocking=True)
    return out


def agree(values, what: str, group=None) -> None:
    """Raise ZbError unless every rank of `group` passed the same `values` (integers below 2^63), naming
    the first that differs. One small all_gather; nothing without an initialised group."""
    import torch  # noqa: PLC0415
    import torch.distributed as dist  # noqa: PLC0415

    from .engine import ZbError  # noqa: PLC0415

    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    names = list(values)
    t = torch.tensor([int(values[k]) for k in names], dtype=torch.int64)
    if dist.get_backend(group) == "nccl":
        t = t.cuda()
    rows = [torch.zeros_like(t) for _ in range(dist.get_world_size(group))]
    dist.all_gather(rows, t, group=group)
    rows = torch.stack(rows).cpu()
    for j, k in enumerate(names):
        if not bool((rows[:, j] == rows[0, j]).all()):
            raise ZbError(f"{what}: the ranks disagree on {k}: {rows[:, j].tolist()} (rank order)")


def reduce_episode_stats(stats_local, group=None):
    """[n_local, 4] per-env statistics -> [4] float64 global sums (every rank)."""
    return reduce_fixed_order(stats_local.double().sum(0), group=group)


def dist_env() -> tuple[int, int, int]:
    """(rank, local_rank, world) from the torchrun environment."""
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")),
            int(os.environ.get("WORLD_SIZE", "1")))
