"""The multi-rank gradient combine on the CPU: zb_grad_combine_host, the bit definition
of csrc/zb_learner.hip's grad_combine_kernel, against an independent restatement of the header's
reduction tree; zbot_amd.dist.all_gather_rows and the learner's cross-rank checks over gloo. No GPU
needed: the spawned ranks exchange CPU tensors only.
"""

import ctypes as C
import os
import re
import socket
from datetime import timedelta

import numpy as np
import pytest
import torch

import combine_cases as CC
from zbot_amd import engine as E
from zbot_amd import ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = (1, 2, 3, 5, 8, 64)
COUNTS = (1, 7, 4096, 4097, 12289)
TIMEOUT = timedelta(seconds=60)


@pytest.fixture(scope="module", autouse=True)
def lib():
    E.build_library()
    return E.load_library()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("world", WORLDS)
def test_host_twin_is_the_tree(world, count):
    parts = CC.parts_case(world, count)
    grad, sq = ppo.grad_combine_host(parts)
    assert same_bits(grad, CC.tree_numpy(parts))
    # the same tree by ppo.pairwise_tree_host (host floats, one column at a time) on a few columns
    for i in sorted({0, 1 % count, CC.cancel_index(count), count - 1}):
        col = np.stack([parts[:, i].astype(np.float64), np.zeros(world)], 1)
        want = np.float32(float(ppo.pairwise_tree_host(torch.from_numpy(col))[0]) + 0.0)
        assert same_bits(grad[i], want), (i, grad[i], want)
    if world >= 3:
        # rank order is visible in fp32 and gone after the fp64 tree
        i = CC.cancel_index(count)
        fp32 = np.float32(0)
        for r in range(world):
            fp32 = np.float32(fp32 + parts[r, i])
        assert fp32 == 0.0 and grad[i] == 1.0
    if count > 3:
        assert grad[1] == 0.0 and not np.signbit(grad[1])  # a sum of negative zeros reads +0
    # the norm is grad_sqnorm's of the gradient just written
    assert same_bits(np.float64(sq), np.float64(ppo.grad_sqnorm_host(grad)))
    assert sq > 0


def test_world_one_is_the_row():
    parts = CC.parts_case(1, 4097)
    grad, _ = ppo.grad_combine_host(parts)
    assert np.array_equal(grad, parts[0])  # -0.0 == +0.0 here: the one bit the tree's + 0.0 changes


def test_refused_calls(lib):
    parts = np.array(CC.parts_case(3, 7))
    grad, sq = np.full(7, 7, np.float32), np.full(1, 7.0)

    def call(p=parts.ctypes.data, world=3, count=7, g=grad.ctypes.data, s=sq.ctypes.data):
        return lib.zb_grad_combine_host(p, world, count, g, s)

    assert call(world=0) == -1 and call(world=65) == -1  # ZB_EARG
    assert b"world" in lib.zb_last_error()
    assert call(world=-1) == -1 and call(count=0) == -1 and call(count=(1 << 32) + 1) == -1
    assert call(p=None) == -1 and call(g=None) == -1 and call(s=None) == -1
    # grad inside parts (any row) is refused; directly behind the last row it is not an overlap
    assert call(g=parts.ctypes.data) == -1 and call(g=parts.ctypes.data + 4 * 20) == -1
    assert b"overlap" in lib.zb_last_error()
    assert np.all(grad == 7) and sq[0] == 7.0
    buf = np.zeros(4 * 7, np.float32)
    buf[:21] = parts.reshape(-1)
    assert lib.zb_grad_combine_host(buf.ctypes.data, 3, 7, buf.ctypes.data + 4 * 21, sq.ctypes.data) == 0
    assert same_bits(buf[21:], CC.tree_numpy(parts))
    assert call() == 0 and same_bits(grad, CC.tree_numpy(parts))
    # the device entry point checks before it launches: no GPU is touched by a refused call
    part = np.zeros(1)
    for w in (0, 65):
        assert lib.zb_grad_combine(parts.ctypes.data, w, 7, grad.ctypes.data, part.ctypes.data, sq.ctypes.data, None) == -1
    assert lib.zb_grad_combine(parts.ctypes.data, 3, 7, grad.ctypes.data, None, sq.ctypes.data, None) == -1
    with pytest.raises(E.ZbError):
        ppo.grad_combine(torch.zeros(2, 5))  # a CPU tensor: the kernel runs on the GPU only


def test_abi_exports_and_binding(lib):
    txt = open(os.path.join(ROOT, "include", "zbot_ppo.h")).read()
    syms = set(re.findall(r"\b(zb_[a-z_]+)\s*\(", txt))
    assert {"zb_grad_combine", "zb_grad_combine_host"} <= syms
    for s in ("zb_grad_combine", "zb_grad_combine_host"):
        assert hasattr(lib, s), f"libzbot_hip.so does not export {s}"
        assert getattr(lib, s).restype is C.c_int
    assert lib.zb_grad_combine.argtypes == [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]
    assert lib.zb_grad_combine_host.argtypes == [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
    m = re.search(r"#define ZB_COMBINE_MAX_WORLD\s+(\d+)", txt)
    assert m and int(m.group(1)) == ppo.COMBINE_MAX_WORLD == 64


# ---- spawned gloo ranks, CPU tensors only ----

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
    return dist


def _gather_rank(rank, world, port, outdir):
    dist = _init(rank, world, port)
    from zbot_amd.dist import all_gather_rows
    from zbot_amd.engine import ZbError

    count = 1031
    out = torch.full((world, count), -1.0)
    got = all_gather_rows(torch.full((count,), float(rank)), out, dist.group.WORLD)
    assert got is out
    ptr = out.data_ptr()
    all_gather_rows(torch.full((count,), float(rank)), out, dist.group.WORLD)  # again, into the same storage
    assert out.data_ptr() == ptr
    f64 = all_gather_rows(torch.tensor([rank + 0.5, -rank], dtype=torch.float64),
                          torch.empty(world, 2, dtype=torch.float64), dist.group.WORLD)
    try:
        all_gather_rows(torch.zeros(count), torch.zeros(world + 1, count), dist.group.WORLD)
        refused = False
    except ZbError:
        refused = True
    np.savez(os.path.join(outdir, f"rows{rank}.npz"), out=out.numpy(), f64=f64.numpy(), refused=refused)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_all_gather_rows_gloo(world, tmp_path):
    import torch.multiprocessing as mp

    mp.start_processes(_gather_rank, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    want = np.repeat(np.arange(world, dtype=np.float32)[:, None], 1031, 1)
    for r in range(world):
        z = np.load(tmp_path / f"rows{r}.npz")
        assert np.array_equal(z["out"], want)  # row r holds rank r, on every rank
        assert np.array_equal(z["f64"], np.array([[k + 0.5, -k] for k in range(world)], np.float64))
        assert bool(z["refused"])


def test_all_gather_rows_without_a_group():
    from zbot_amd.dist import all_gather_rows

    part = torch.arange(5, dtype=torch.float32)
    assert torch.equal(all_gather_rows(part, torch.zeros(1, 5)), part[None])
    with pytest.raises(E.ZbError):
        all_gather_rows(part, torch.zeros(2, 5))


def _check_rank(rank, world, port, outdir):
    dist = _init(rank, world, port)
    from zbot_amd.engine import ZbError
    from zbot_amd.learner import HipPpoLearner

    def attempt(name, learner, *shape):
        try:
            learner.check_ranks(*shape)
            msg = ""
        except ZbError as e:
            msg = str(e)
        with open(os.path.join(outdir, f"{name}{rank}.txt"), "w") as f:
            f.write(msg)

    g = dist.group.WORLD
    ln = HipPpoLearner(shuffle_seed=5, group=g)
    assert (ln.world, ln.rank) == (world, rank)
    assert ln.rank_seed() == (5 + 0x9E3779B97F4A7C15 * rank) % (1 << 64)
    # a learner agrees once per update shape, so every attempt gets a learner that has not agreed yet
    attempt("ok", ln, 32, 8, 32, 2)                    # n_local, T, batch_size, num_passes
    attempt("batch", HipPpoLearner(shuffle_seed=5, group=g), 32, 8, 33, 2)      # 33 is no multiple of 2
    attempt("T", HipPpoLearner(shuffle_seed=5, group=g), 32, 8 + rank, 32, 2)   # rollouts of different lengths
    attempt("seed", HipPpoLearner(shuffle_seed=5 + rank, group=g), 32, 8, 32, 2)
    attempt("lr", HipPpoLearner(shuffle_seed=5, learning_rate=3e-4 * (1 + rank), group=g), 32, 8, 32, 2)
    # a state saved by one process is refused by a learner over two ranks, and the other way round
    z = torch.zeros(3)
    sd = dict(step=1, epoch=1, actor=dict(params=z, m=z, v=z), critic=dict(params=z, m=z, v=z))
    for name, learner, state in (("load1", ln, sd), ("load2", HipPpoLearner(shuffle_seed=5), dict(sd, world=2))):
        try:
            learner.load_state_dict(state)
            msg = ""
        except ZbError as e:
            msg = str(e)
        with open(os.path.join(outdir, f"{name}{rank}.txt"), "w") as f:
            f.write(msg)
    ln.load_state_dict(dict(sd, world=2))
    dist.barrier()
    dist.destroy_process_group()


def test_learner_checks_across_ranks(tmp_path):
    """batch_size % W, and a mismatch of T, the seed or the learning rate between ranks, raise ZbError
    on every rank (none waits for another); no GPU call is made."""
    import torch.multiprocessing as mp

    mp.start_processes(_check_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    for r in range(2):
        msg = {k: open(tmp_path / f"{k}{r}.txt").read() for k in ("ok", "batch", "T", "seed", "lr", "load1", "load2")}
        assert msg["ok"] == ""
        assert "multiple" in msg["batch"]
        assert "disagree on T" in msg["T"] and "[8, 9]" in msg["T"]
        assert "shuffle_seed" in msg["seed"] and "learning_rate" in msg["lr"]
        assert "rank" in msg["load1"] and "rank" in msg["load2"]


def test_one_process_learner_has_no_group():
    from zbot_amd.learner import HipPpoLearner

    ln = HipPpoLearner(shuffle_seed=7)
    assert (ln.world, ln.rank, ln.group) == (1, 0, None) and ln.rank_seed() == 7
    assert HipPpoLearner().rank_seed() is None
    ln.check_ranks(32, 8, 33, 2)  # one process: any batch size, no collective
