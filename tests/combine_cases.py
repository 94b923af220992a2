"""Fixtures of the gradient combine (zb_grad_combine, include/zbot_ppo.h "Learner"), shared by
tests/test_grad_combine_host.py and tests/test_gpu_grad_combine.py, and an independent restatement
of its tree on numpy float64."""

import functools

import numpy as np

CANCEL = (1e8, 1.0, -1e8)  # fp32 in rank order: (1e8 + 1) - 1e8 = 0; the fp64 tree: exactly 1


def cancel_index(count: int) -> int:
    return count // 2


@functools.lru_cache(maxsize=None)
def _parts(world: int, count: int) -> np.ndarray:
    rng = np.random.default_rng(1000 * world + count)
    # magnitudes spread over six decades between ranks and elements, so the order of the sum shows
    p = (rng.standard_normal((world, count)) * 10.0 ** rng.uniform(-3, 3, (world, count))).astype(np.float32)
    if world >= 3:
        i = cancel_index(count)
        p[:, i] = 0.0
        p[:3, i] = CANCEL
    if count > 3:
        p[:, 1] = -0.0  # a column of negative zeros: root + 0.0 reads +0
    p.setflags(write=False)
    return p


def parts_case(world: int, count: int) -> np.ndarray:
    """[world, count] float32, read-only and cached: every rank's gradient."""
    return _parts(world, count)


def tree_numpy(parts: np.ndarray) -> np.ndarray:
    """The header's reduction tree over axis 0, all columns at once: leaves in rank order as float64,
    zero-padded to a power of two, adjacent pairs first; root + 0.0; one rounding to float32."""
    world, count = parts.shape
    p = 1
    while p < world:
        p <<= 1
    a = np.zeros((p, count), np.float64)
    a[:world] = parts.astype(np.float64)
    while a.shape[0] > 1:
        a = a[0::2] + a[1::2]
    return (a[0] + 0.0).astype(np.float32)
