#!/usr/bin/env python3
"""One training iteration of zbot_amd.train.Trainer at train.py's own size (512 envs x 200 steps,
batch 128, 4 passes; train.py:1770-1775), split by phase, on one GPU.

  phases   2 warm-up iterations, then 5 timed ones with device events around the phases of
           Trainer.step(): the rollout (actor, zb_step and the in-loop critic), the PPO inputs, and
           the update (16 optimizer steps). After each timed iteration the update's 16 minibatch
           gathers are replayed alone on the same rollout (one zb_minibatch_gather launch each)
           between two events. Median (min - max) in ms per phase and each phase's share of their
           sum; `iteration_ms` is the host wall time of step(), which adds the curriculum's
           synchronisation and the host's own work.
  gather   the update of the last rollout with shuffle_seed=None (seven torch slice copies, two
           carry slices and a reset slice per minibatch) against a seed (the fused gather), on two
           learners with their own network handles, one warm-up each, then alternating, 5 rounds.
           The two do not run the same minibatches (that is what the seed changes), only the same
           amount of work.

    python scripts/train_loop_timing.py --out profiles/train_loop_timing.json
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ksim-gym-zbot_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--groups", type=int, default=1, help="env groups of the rollout (1: one HipEngine)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from zbot_amd import compile_model, default_config
    from zbot_amd import learner as LN
    from zbot_amd import policy as P
    from zbot_amd.engine import EnvGroups, HipEngine
    from zbot_amd.train import Trainer

    if not torch.cuda.is_available():
        raise SystemExit("train_loop_timing needs a GPU: there is no CPU path to time")
    n, T = a.envs, a.steps
    cm, cfg = compile_model(), default_config()
    eng = HipEngine(cm, cfg, n, seed=1) if a.groups == 1 else EnvGroups(cm, cfg, n, groups=a.groups, seed=1)
    pa, pc = P.init_params(P.ACTOR, seed=1), P.init_params(P.CRITIC, seed=2)
    tr = Trainer(eng, P.GruPolicy(P.ACTOR, pa), P.GruPolicy(P.CRITIC, pc), rollout_steps=T, num_passes=a.passes,
                 batch_size=a.batch, seed=3, shuffle=True, ctrl_dt=float(cfg.ctrl_dt))
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    names = ("rollout", "ppo_inputs", "update")

    def gathers_alone():
        """The update's minibatch gathers on the last rollout, without the steps between them."""
        out, inp = tr.last_rollout, tr.last_inputs
        carry, ccarry = tr.rollout.carry, tr.critic_carry  # any carries: the gather moves bytes
        e0, e1 = ev(), ev()
        e0.record()
        for epoch in range(a.passes):
            for lo in range(0, n, a.batch):
                tr.learner._mb.cut(torch, out, inp, carry, ccarry, None, T, n, lo, min(n, lo + a.batch) - lo, 3, epoch)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {k: [] for k in names + ("gathers", "iteration")}
    for it in range(a.warmup + a.repeats):
        tr.timing = {k: (ev(), ev()) for k in names}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = tr.step()
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        g = gathers_alone()
        if it >= a.warmup:
            for k in names:
                times[k].append(tr.timing[k][0].elapsed_time(tr.timing[k][1]))
            times["gathers"].append(g)
            times["iteration"].append(wall)
        print(json.dumps(dict(iteration=m["iteration"], level=m["level"], episode_length=m["episode_length"],
                              wall_ms=wall, loss=float(m["loss"][-1]))), flush=True)
    tr.timing = None
    stat = lambda t: dict(median=statistics.median(t), min=min(t), max=max(t))  # noqa: E731
    res = dict(device=torch.cuda.get_device_name(0), envs=n, steps=T, batch=a.batch, passes=a.passes, groups=a.groups,
               solver="cg", warmup=a.warmup, repeats=a.repeats,
               optimizer_steps=a.passes * ((n + a.batch - 1) // a.batch))
    res["phases_ms"] = {k: stat(times[k]) for k in names}
    total = sum(res["phases_ms"][k]["median"] for k in names)
    res["phase_share"] = {k: res["phases_ms"][k]["median"] / total for k in names}
    res["gathers_ms"] = stat(times["gathers"])
    res["gathers_share_of_update"] = res["gathers_ms"]["median"] / res["phases_ms"]["update"]["median"]
    res["iteration_ms"] = stat(times["iteration"])
    print(json.dumps({k: res[k] for k in ("phases_ms", "phase_share", "gathers_ms", "iteration_ms")}), flush=True)

    # second leg: the same rollout's update through torch slices and through the fused gather
    out, inp = tr.last_rollout, tr.last_inputs
    carry, ccarry = tr.rollout.carry.clone(), tr.critic_carry.clone()
    legs = {}
    for name, seed in (("slices", None), ("gather", 3)):
        legs[name] = (LN.HipPpoLearner(shuffle_seed=seed), P.GruPolicy(P.ACTOR, pa), P.GruPolicy(P.CRITIC, pc))

    def update(name):
        ln, act, cri = legs[name]
        e0, e1 = ev(), ev()
        e0.record()
        ln.update(out, inp, act, cri, carry, ccarry, reset=None, num_passes=a.passes, batch_size=a.batch)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for name in legs:
        update(name)
    ut = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name in legs:
            ut[name].append(update(name))
    res["update_ms"] = {name: stat(t) for name, t in ut.items()}
    res["gather_minus_slices_ms"] = res["update_ms"]["gather"]["median"] - res["update_ms"]["slices"]["median"]
    print(json.dumps(dict(update_ms=res["update_ms"], gather_minus_slices_ms=res["gather_minus_slices_ms"])), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
