"""The host twin of the chunked minibatch gather (include/zbot_ppo.h "Chunked minibatches",
zb_minibatch_gather_seq_host) against its law written in numpy indexing, on the CPU.
tests/test_gpu_seq_chunks.py holds the kernel to these bits.

The law: a time item's T = C L source rows are cut in C chunks of L rows, and for l < L, c < C,
j < count  dst[l][c count + j] = src[c L + l][p(lo + j)]; any other item keeps
dst[r][j] = src[r][p(lo + j)].
"""

import ctypes as C

import numpy as np
import pytest

from zbot_amd import engine as E
from zbot_amd import ppo

# elements per row and dtype: row_bytes 1, 4, 200 (8-byte accesses) and 16
ROWS = ((1, np.uint8), (1, np.float32), (50, np.float32), (4, np.float32))


@pytest.fixture(scope="module", autouse=True)
def lib():
    E.build_library()
    return E.load_library()


def env_index(n, lo, count, shuffle_seed, epoch):
    if shuffle_seed is None:
        return np.arange(lo, lo + count)
    return ppo.minibatch_perm_host(n, shuffle_seed, epoch)[lo:lo + count].astype(np.int64)


def chunked(src, T, L, idx):
    """The law for a time item: src [>= T, n, ...] -> [L, C count, ...]."""
    Cn, count = T // L, len(idx)
    want = np.empty((L, Cn * count) + src.shape[2:], src.dtype)
    for c in range(Cn):
        for l in range(L):  # noqa: E741
            for j in range(count):
                want[l, c * count + j] = src[c * L + l, idx[j]]
    return want


def random_array(rng, shape, dtype):
    raw = rng.integers(0, 256, size=int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=np.uint8)
    return raw.view(dtype).reshape(shape)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("shuffle_seed", [None, 5])
@pytest.mark.parametrize("lo,count", [(0, 5), (1, 3), (4, 1)])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_host_twin_equals_the_law(L, lo, count, shuffle_seed):
    T, n, epoch = 6, 5, 3
    Cn = T // L
    rng = np.random.default_rng(100 * L + 10 * lo + count)
    srcs = [random_array(rng, (T + 1, n, F), dt) for F, dt in ROWS]  # [T + 1] buffers: the item is the first T rows
    dsts = [np.full((L, Cn * count, F), 0x5A, dt) for F, dt in ROWS]
    strided = random_array(rng, (2 * T, n, 6), np.float32)[::2]      # a time stride of two rows
    sdst = np.zeros((L, Cn * count, 6), np.float32)
    carries = random_array(rng, (Cn, n, 2, 128), np.float32)         # rows = C: the carries at the chunk starts
    cdst = np.zeros((Cn, count, 2, 128), np.float32)
    whole = random_array(rng, (n, 3), np.float32)                    # rows = 1
    wdst = np.zeros((count, 3), np.float32)
    zdst = np.full((L, Cn * count), 9, np.uint8)                     # a null source, cut like the others
    z1 = np.full((1, count), 9, np.uint8)                            # and one that is not a time item
    items = [(s, d, True) for s, d in zip(srcs, dsts)] + [(strided, sdst, True), (carries, cdst), (whole[None], wdst[None]),
                                                           (None, zdst, True), (None, z1)]
    ppo.gather_minibatch_host(items, n, lo, count, shuffle_seed=shuffle_seed, epoch=epoch, seq_len=L)
    idx = env_index(n, lo, count, shuffle_seed, epoch)
    for s, d in zip(srcs, dsts):
        assert same_bytes(d, chunked(s, T, L, idx)), (s.shape, s.dtype)
    assert same_bytes(sdst, chunked(strided, T, L, idx))
    assert same_bytes(cdst, carries[:, idx]) and same_bytes(wdst, whole[idx])
    assert not zdst.any() and not z1.any()
    # column q = c count + j of every item is chunk c of env idx[j]: the carries read as C count sequences
    seq_carry = cdst.reshape(Cn * count, 2, 128)
    for c in range(Cn):
        for j in range(count):
            assert same_bytes(seq_carry[c * count + j], carries[c, idx[j]])
            assert same_bytes(dsts[2][:, c * count + j], srcs[2][c * L:(c + 1) * L, idx[j]])


def _table(pairs, T, n):
    arr = (ppo.ZbGatherItem * len(pairs))()
    for k, (s, d) in enumerate(pairs):
        rb = s[0, 0].nbytes
        arr[k] = ppo.ZbGatherItem(s.ctypes.data, d.ctypes.data, T, rb, n * rb)
    return arr


@pytest.mark.parametrize("shuffle", [0, 1])
def test_seq_len_of_the_whole_run_is_the_plain_gather(lib, shuffle):
    """cut items with seq_len == rows: the bytes of zb_minibatch_gather_host."""
    T, n, lo, count = 6, 5, 1, 3
    rng = np.random.default_rng(7)
    srcs = [random_array(rng, (T, n, F), dt) for F, dt in ROWS]
    a = [np.full((T, count, F), 0x5A, dt) for F, dt in ROWS]
    b = [np.full((T, count, F), 0x33, dt) for F, dt in ROWS]
    cut = (C.c_int32 * len(srcs))(*([1] * len(srcs)))
    assert lib.zb_minibatch_gather_seq_host(_table(list(zip(srcs, a)), T, n), cut, len(srcs), T, n, lo, count, shuffle,
                                            11, 2) == 0
    assert lib.zb_minibatch_gather_host(_table(list(zip(srcs, b)), T, n), len(srcs), n, lo, count, shuffle, 11, 2) == 0
    for x, y in zip(a, b):
        assert same_bytes(x, y)
    # and through the Python form, marked as time items or not
    for mark in ((True,), ()):
        c = [np.zeros((T, count, F), dt) for F, dt in ROWS]
        ppo.gather_minibatch_host([(s, d) + mark for s, d in zip(srcs, c)], n, lo, count,
                                  shuffle_seed=11 if shuffle else None, epoch=2, seq_len=T)
        for x, y in zip(c, b):
            assert same_bytes(x, y)


def test_refusals_name_the_argument(lib):
    T, n, count = 6, 8, 4
    src, dst = np.ones((T, n, 3), np.float32), np.full((T, count, 3), 7.0, np.float32)
    ok = ppo.ZbGatherItem(src.ctypes.data, dst.ctypes.data, T, 12, n * 12)

    def call(items, cut=(1,), n_items=1, L=2, n_=n, lo=0, count_=count):
        arr = (ppo.ZbGatherItem * len(items))(*items)
        cu = None if cut is None else (C.c_int32 * len(items))(*(list(cut) * len(items))[:len(items)])
        return lib.zb_minibatch_gather_seq_host(arr, cu, n_items, L, n_, lo, count_, 1, 0, 0)

    for L in (4, 5, 7):  # T % L != 0
        assert call([ok], L=L) == -1
        assert b"seq_len" in lib.zb_last_error() and b"zb_minibatch_gather_seq_host" in lib.zb_last_error()
    for L in (0, -2):    # L < 1, whether or not an item is cut
        assert call([ok], L=L) == -1 and b"seq_len" in lib.zb_last_error()
        assert call([ok], cut=(0,), L=L) == -1 and b"seq_len" in lib.zb_last_error()
    assert call([ok], cut=None) == -1 and b"cut" in lib.zb_last_error()
    assert call([ok], cut=(0,), L=4) == 0  # an item that is not cut need not divide
    dst[...] = 7.0
    # the plain gather's bad arguments
    assert call([ok], lo=5) == -1 and b"envs" in lib.zb_last_error()
    assert call([ok], lo=-1) == -1 and call([ok], count_=0) == -1 and call([ok], n_=0, count_=0) == -1
    assert call([ok], lo=2**31 - 2) == -1
    assert call([ok], n_items=0) == -1 and b"n_items" in lib.zb_last_error()
    assert call([ok] * 17, n_items=17) == -1
    assert lib.zb_minibatch_gather_seq_host(None, (C.c_int32 * 1)(1), 1, 2, n, 0, count, 1, 0, 0) == -1
    assert b"items" in lib.zb_last_error()
    assert call([ppo.ZbGatherItem(src.ctypes.data, None, T, 12, n * 12)]) == -1 and b"dst" in lib.zb_last_error()
    assert call([ppo.ZbGatherItem(src.ctypes.data, dst.ctypes.data, 0, 12, n * 12)]) == -1
    assert call([ppo.ZbGatherItem(src.ctypes.data, dst.ctypes.data, T, 0, n * 12)]) == -1
    assert b"row_bytes" in lib.zb_last_error()
    assert call([ppo.ZbGatherItem(src.ctypes.data, dst.ctypes.data, T, 12, -12)]) == -1 and b"stride" in lib.zb_last_error()
    assert call([ok, ppo.ZbGatherItem(src.ctypes.data, dst.ctypes.data, T, 12, n * 12)], n_items=2, L=4) == -1
    assert np.all(dst == 7.0)  # a refused call moves nothing
    assert call([ok]) == 0 and np.all(dst == 1.0)
    # the Python form: seq_len itself, and a destination that is neither [L, C count] nor [rows, count]
    d2 = np.zeros((2, 3 * count, 3), np.float32)
    for bad in (0, -1, 1.5):
        with pytest.raises(ppo.ZbError, match="seq_len"):
            ppo.gather_minibatch_host([(src, d2, True)], n, 0, count, seq_len=bad)
    with pytest.raises(ppo.ZbError, match="seq_len"):
        ppo.gather_minibatch_host([(src, d2, True)], n, 0, count, seq_len=3)       # dst has 2 rows, not 3
    with pytest.raises(ppo.ZbError, match="seq_len"):
        ppo.gather_minibatch_host([(src, d2[:, :10], True)], n, 0, count, seq_len=2)  # 10 columns: no multiple of count
    with pytest.raises(ppo.ZbError, match="seq_len"):
        ppo.gather_minibatch_host([(src, np.zeros((2, 4 * count, 3), np.float32), True)], n, 0, count, seq_len=2)  # 8 > T rows
    with pytest.raises(ppo.ZbError, match="seq_len"):
        ppo.gather_minibatch_host([(src, d2, True)], n, 0, count)                # a time item without seq_len
    with pytest.raises(ppo.ZbError, match=r"\[rows, 4"):
        ppo.gather_minibatch_host([(src, d2)], n, 0, count, seq_len=2)            # unmarked: the plain gather's error
    ppo.gather_minibatch_host([(src, d2, True)], n, 0, count, seq_len=2)
    assert np.all(d2 == 1.0)
