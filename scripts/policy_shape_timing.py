"""Timings behind DESIGN.md §4r (shaped policy handles) -> profiles/policy_shape_timing.json.

    python scripts/policy_shape_timing.py [--rounds 3] [--parent-lib PATH] [--out profiles/policy_shape_timing.json]

Per configuration, two numbers: one one-step actor launch at 8192 envs, and one actor gradient evaluation
(training forward + backward) at 128 envs x 200 steps. Configurations: the default handle, (5, 5) with the
generic flag, (2, 5), (5, 1), (8, 8); and, with --parent-lib, a default handle of another build of the library
(the parent commit's) through the same calls. Every measurement runs in a process of its own (two builds of
the library do not load together), the configurations alternate within a round, and a round's figure is the
median of its repetitions, so the file holds one figure per configuration per round: compare the rounds'
ranges, not single numbers. Last, one Trainer iteration at train.py's size (512 envs x 200 steps, batch 128,
4 passes) with both networks at depth 2 against depth 5.
"""

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ksim-gym-zbot_amd"))

N_STEP, N_TRAIN, T_TRAIN = 8192, 128, 200


def timed(torch, fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def measure_raw(lib_path):
    """A default-shape actor through the C ABI as the parent commit has it (works on either build)."""
    import numpy as np
    import torch

    from zbot_amd.policy import ACTOR, init_params

    L = C.CDLL(lib_path)
    vp = C.c_void_p
    L.zb_policy_create.argtypes = [C.c_int, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.POINTER(vp)]
    L.zb_policy_actor.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_uint64, C.c_int, C.c_uint32, vp, vp, vp]
    L.zb_policy_train_scratch_words.argtypes = [C.c_int, C.c_int, C.c_int]
    L.zb_policy_train_scratch_words.restype = C.c_size_t
    L.zb_policy_actor_train.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.zb_policy_actor_backward.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_size_t, vp, vp]
    prm = init_params(ACTOR, seed=1)
    h = vp()
    assert L.zb_policy_create(ACTOR, prm.ctypes.data_as(C.POINTER(C.c_float)), prm.size, 0, C.byref(h)) == 0
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    obs, carry, act = r(N_STEP, 50), torch.zeros(N_STEP, 5, 128, device="cuda"), torch.empty(N_STEP, 20, device="cuda")

    def step():
        assert L.zb_policy_actor(h, obs.data_ptr(), 1, N_STEP, carry.data_ptr(), None, 0, 0, 0, 0, act.data_ptr(), None,
                                 stream) == 0

    T, n = T_TRAIN, N_TRAIN
    words = L.zb_policy_train_scratch_words(ACTOR, T, n)
    o, a, d, c0 = r(T, n, 50), 0.4 * r(T, n, 20), r(T, n, 20), 0.5 * r(n, 5, 128)
    lp, scr, grad = torch.empty(T, n, 20, device="cuda"), torch.empty(words, device="cuda"), torch.empty(prm.size, device="cuda")

    def train():
        assert L.zb_policy_actor_train(h, o.data_ptr(), T, n, c0.data_ptr(), None, a.data_ptr(), lp.data_ptr(),
                                       scr.data_ptr(), words, stream) == 0
        assert L.zb_policy_actor_backward(h, o.data_ptr(), T, n, c0.data_ptr(), None, a.data_ptr(), d.data_ptr(),
                                          scr.data_ptr(), words, grad.data_ptr(), stream) == 0

    return dict(step_ms=timed(torch, step, 20, 200), grad_ms=timed(torch, train, 3, 10))


def measure_shaped(depth, mix, generic):
    import torch

    from zbot_amd import policy as P

    sh = P.PolicyShape(depth, mix)
    net = P.GruPolicy(P.ACTOR, P.init_params(P.ACTOR, 1, sh), shape=sh, generic=generic)
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    obs, carry, act = r(N_STEP, 50), net.initial_carry(N_STEP), torch.empty(N_STEP, 20, device="cuda")
    step = lambda: net.actor(obs, carry, actions=act)  # noqa: E731
    T, n = T_TRAIN, N_TRAIN
    o, a, d, c0 = r(T, n, 50), 0.4 * r(T, n, 20), r(T, n, 20), 0.5 * r(n, depth, 128)
    scr = torch.empty(net.train_scratch_words(T, n), device="cuda")
    grad = torch.empty(net.n_params, device="cuda")

    def train():
        net.actor_train(o, a, c0, None, scr)
        net.actor_backward(o, a, c0, None, d, scr, grad)

    return dict(step_ms=timed(torch, step, 20, 200), grad_ms=timed(torch, train, 3, 10))


def measure_trainer(depth):
    import torch

    from zbot_amd import compile_model, default_config
    from zbot_amd import policy as P
    from zbot_amd.engine import HipEngine
    from zbot_amd.train import Trainer

    sh = P.PolicyShape(depth, 5)
    eng = HipEngine(compile_model(), default_config(), 512, seed=2)
    tr = Trainer(eng, P.GruPolicy(P.ACTOR, P.init_params(P.ACTOR, 8, sh), shape=sh),
                 P.GruPolicy(P.CRITIC, P.init_params(P.CRITIC, 9, sh), shape=sh), rollout_steps=200, num_passes=4,
                 batch_size=128, seed=5)
    return dict(iteration_ms=timed(torch, tr.step, 1, 3))


def child(spec):
    kind = spec["kind"]
    if kind == "raw":
        out = measure_raw(spec["lib"])
    elif kind == "shaped":
        out = measure_shaped(spec["depth"], spec["mix"], spec["generic"])
    else:
        out = measure_trainer(spec["depth"])
    print("RESULT " + json.dumps(out))


def run_child(spec):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(spec)], capture_output=True,
                       text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"measurement {spec} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_shape_timing.json"))
    a = ap.parse_args()
    if a.child:
        child(json.loads(a.child))
        return
    from zbot_amd.engine import LIB_PATH

    specs = {"default": dict(kind="raw", lib=LIB_PATH)}
    if a.parent_lib:
        specs["default_parent_build"] = dict(kind="raw", lib=os.path.abspath(a.parent_lib))
    specs["5x5_generic"] = dict(kind="shaped", depth=5, mix=5, generic=True)
    for d, m in ((2, 5), (5, 1), (8, 8)):
        specs[f"{d}x{m}"] = dict(kind="shaped", depth=d, mix=m, generic=False)
    specs["trainer_depth5"] = dict(kind="trainer", depth=5)
    specs["trainer_depth2"] = dict(kind="trainer", depth=2)
    res = {k: [] for k in specs}
    for _ in range(a.rounds):
        for k, s in specs.items():
            res[k].append(run_child(s))
            print(k, res[k][-1], flush=True)
    out = dict(what="ms per call, one figure per round (each the median of its repetitions; a process per measurement, "
                    "configurations alternating within a round)",
               step="one one-step actor launch, 8192 envs", grad="actor training forward + backward, 128 envs x 200 steps",
               iteration="one Trainer.step(), 512 envs x 200 steps, batch 128, 4 passes, actor and critic at the depth",
               rounds=a.rounds, results=res)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
