"""The keyed minibatch permutation (include/zbot_fmath.h zbf_perm_index) and the host twin of the
fused minibatch gather (include/zbot_ppo.h "Minibatches"), on the CPU. tests/test_gpu_minibatch.py
holds the kernels to these bits.
"""

import ctypes as C

import numpy as np
import pytest

from zbot_amd import engine as E
from zbot_amd import ppo

SIZES = (1, 2, 3, 5, 8, 33, 128, 129, 512, 1000, 65536)
KEYS = ((0, 0), (0, 1), (7, 0), (2**63 + 11, 2**32 - 1), (123456789, 40))
# rows of the arrays a minibatch moves: obs_critic 1936 B (16-B accesses), obs_actor 200 B (8-B),
# actions 80 B (16-B), values 4 B, done flags 1 B; and an odd size that only bytes divide
ROWS = ((484, np.float32), (50, np.float32), (20, np.float32), (1, np.float32), (1, np.uint8), (7, np.uint8))


@pytest.fixture(scope="module", autouse=True)
def lib():
    E.build_library()
    return E.load_library()


@pytest.mark.parametrize("n", SIZES)
def test_it_is_a_permutation(n):
    for seed, epoch in KEYS:
        p = ppo.minibatch_perm_host(n, seed, epoch)
        assert p.dtype == np.int32 and p.shape == (n,)
        assert np.array_equal(np.sort(p), np.arange(n)), (n, seed, epoch)
        assert np.array_equal(p, ppo.minibatch_perm_host(n, seed, epoch))


def test_it_differs_between_epochs_and_seeds():
    base = ppo.minibatch_perm_host(128, 0, 0)
    assert not np.array_equal(base, np.arange(128))
    seen = {base.tobytes()}
    for seed, epoch in ((0, 1), (0, 2), (1, 0), (2, 0), (1, 1)):
        p = ppo.minibatch_perm_host(128, seed, epoch)
        assert p.tobytes() not in seen, (seed, epoch)
        seen.add(p.tobytes())
    # small n is mixed too: the Feistel half-width has a floor of 4 bits
    assert any(ppo.minibatch_perm_host(2, 0, e)[0] == 1 for e in range(16))
    assert len({ppo.minibatch_perm_host(3, 0, e).tobytes() for e in range(64)}) == 6


def test_uniformity_at_n8():
    """n = 8, seed 0, epochs 0 .. 7999: each of the 64 (position, value) counts is binomial(8000, 1/8),
    mean 1000, standard deviation 29.6; all must lie within 5 standard deviations, 1000 +- 150."""
    cnt = np.zeros((8, 8), np.int64)
    pos = np.arange(8)
    for e in range(8000):
        cnt[pos, ppo.minibatch_perm_host(8, 0, e)] += 1
    chi2 = float(((cnt - 1000.0) ** 2 / 1000.0).sum())
    print(f"PERM n=8 counts min {cnt.min()} max {cnt.max()} chi2 {chi2:.1f}")
    assert cnt.min() >= 850 and cnt.max() <= 1150, (cnt.min(), cnt.max())


def test_perm_argument_checks(lib):
    out = np.full(4, 7, np.int32)
    assert lib.zb_minibatch_perm_host(0, 0, 0, out.ctypes.data) == -1
    assert lib.zb_minibatch_perm_host(0, 0, -3, out.ctypes.data) == -1
    assert lib.zb_minibatch_perm_host(0, 0, 4, None) == -1
    assert np.all(out == 7)
    with pytest.raises(ppo.ZbError):
        ppo.minibatch_perm_host(0, 0, 0)
    with pytest.raises(ppo.ZbError):
        ppo.minibatch_perm_host(4, -1, 0)


def _sources(T, n, rng, pad=0):
    """One [T + pad, n, F] source per row class (the first T rows are the item), random bytes."""
    out = []
    for F, dt in ROWS:
        raw = rng.integers(0, 256, size=(T + pad, n, F * np.dtype(dt).itemsize), dtype=np.uint8)
        out.append(np.ascontiguousarray(raw).view(dt).reshape(T + pad, n, F))
    return out


@pytest.mark.parametrize("shuffle_seed", [None, 5])
@pytest.mark.parametrize("T,n,lo,count", [(3, 33, 0, 33), (3, 33, 16, 17), (3, 33, 32, 1), (1, 33, 4, 9), (4, 5, 1, 3)])
def test_gather_host_equals_fancy_indexing(T, n, lo, count, shuffle_seed):
    rng = np.random.default_rng(T * 1000 + n + lo)
    srcs = _sources(T, n, rng, pad=1)  # [T + 1] buffers: the source rows end before the buffer does
    dsts = [np.full((T, count) + s.shape[2:], 0x5A, s.dtype) if s.dtype == np.uint8 else
            np.full((T, count) + s.shape[2:], -1.0, s.dtype) for s in srcs]
    carry = rng.normal(size=(n, 5, 128)).astype(np.float32)  # rows = 1
    cdst = np.zeros((count, 5, 128), np.float32)
    strided = rng.normal(size=(2 * T, n, 6)).astype(np.float32)[::2]  # a time stride of two rows
    sdst = np.zeros((T, count, 6), np.float32)
    zdst = np.full((1, count), 9, np.uint8)  # null source
    items = list(zip(srcs, dsts)) + [(carry[None], cdst[None]), (strided, sdst), (None, zdst)]
    ppo.gather_minibatch_host(items, n, lo, count, shuffle_seed=shuffle_seed, epoch=3)
    idx = np.arange(lo, lo + count) if shuffle_seed is None else ppo.minibatch_perm_host(n, shuffle_seed, 3)[lo:lo + count]
    for s, d in zip(srcs, dsts):
        assert d.tobytes() == np.ascontiguousarray(s[:T, idx]).tobytes(), (s.shape, s.dtype)
    assert np.array_equal(cdst, carry[idx])
    assert np.array_equal(sdst, strided[:, idx])
    assert not zdst.any()


def test_gather_host_misaligned_pointers():
    """Source and destination 4 bytes off a 16-byte boundary: the 16- and 8-byte rows move as words."""
    T, n, lo, count = 3, 33, 16, 17
    rng = np.random.default_rng(1)
    idx = ppo.minibatch_perm_host(n, 9, 0)[lo:lo + count]
    for F in (484, 50, 20, 1):
        sbuf, dbuf = np.zeros(T * n * F + 1, np.float32), np.zeros(T * count * F + 1, np.float32)
        s, d = sbuf[1:].reshape(T, n, F), dbuf[1:].reshape(T, count, F)
        s[...] = rng.normal(size=s.shape)
        ppo.gather_minibatch_host([(s, d)], n, lo, count, shuffle_seed=9)
        assert np.array_equal(d, s[:, idx]) and dbuf[0] == 0


def test_gather_argument_checks(lib):
    T, n, count = 2, 8, 4
    src, dst = np.ones((T, n, 3), np.float32), np.full((T, count, 3), 7.0, np.float32)
    ok = ppo.ZbGatherItem(src.ctypes.data, dst.ctypes.data, T, 12, n * 12)

    def call(items, n_items=1, n_=n, lo=0, count_=count):
        arr = (ppo.ZbGatherItem * len(items))(*items)
        return lib.zb_minibatch_gather_host(arr, n_items, n_, lo, count_, 1, 0, 0)

    assert call([ok], lo=5) == -1            # lo + count > n
    assert call([ok], lo=-1) == -1
    assert call([ok], count_=0) == -1
    assert call([ok], n_=0, count_=0) == -1
    assert call([ok], lo=2**31 - 2, count_=4) == -1   # no overflow of lo + count
    assert call([ok], n_items=0) == -1
    assert call([ok] * 17, n_items=17) == -1  # over ZB_GATHER_MAX_ITEMS
    assert lib.zb_minibatch_gather_host(None, 1, n, 0, count, 1, 0, 0) == -1
    assert call([ppo.ZbGatherItem(src.ctypes.data, None, T, 12, n * 12)]) == -1
    assert call([ppo.ZbGatherItem(src.ctypes.data, dst.ctypes.data, 0, 12, n * 12)]) == -1
    assert call([ppo.ZbGatherItem(src.ctypes.data, dst.ctypes.data, T, 0, n * 12)]) == -1
    assert call([ppo.ZbGatherItem(src.ctypes.data, dst.ctypes.data, T, 12, -12)]) == -1
    assert call([ok, ppo.ZbGatherItem(src.ctypes.data, None, T, 12, n * 12)], n_items=2) == -1  # nothing moved
    assert np.all(dst == 7.0)
    assert b"zb_minibatch_gather_host" in lib.zb_last_error()
    assert call([ok]) == 0 and np.all(dst == 1.0)
    assert C.sizeof(ppo.ZbGatherItem) == 32
    # the Python form refuses what the table cannot describe
    with pytest.raises(ppo.ZbError):
        ppo.gather_minibatch_host([(src, dst[:, :, :2])], n, 0, count)
    with pytest.raises(ppo.ZbError):
        ppo.gather_minibatch_host([(src.astype(np.float64), dst)], n, 0, count)
    with pytest.raises(ppo.ZbError):
        ppo.gather_minibatch_host([(src, dst)] * 17, n, 0, count)
    # seed and epoch are range-checked as minibatch_perm_host checks them: no silent wrap to another permutation
    with pytest.raises(ppo.ZbError):
        ppo.gather_minibatch_host([(src, dst)], n, 0, count, shuffle_seed=-1)
    with pytest.raises(ppo.ZbError):
        ppo.gather_minibatch_host([(src, dst)], n, 0, count, shuffle_seed=1, epoch=2**32)
    with pytest.raises(ppo.ZbError):
        ppo.gather_minibatch_host([(src, dst)], n, 0, count, shuffle_seed=2**64)
    assert np.all(dst == 1.0)
