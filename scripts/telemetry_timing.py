"""Timings behind DESIGN.md §4t (rollout telemetry) -> profiles/telemetry_timing.json.

    python scripts/telemetry_timing.py [--rounds 3] [--parent-root PATH] [--out profiles/telemetry_timing.json]

One Trainer iteration at train.py's size (512 envs x 200 steps, batch 128, 4 passes) three ways:
telemetry=False, telemetry=True and, with --parent-root, the parent commit's Trainer (PATH: a
checkout of the parent commit with its library built; its package is imported instead of this
one). And ppo.rollout_summary alone, every plane present, at 200 x 512 and 256 x 8192 rows, plus
Trainer.validate() at the same size. Device events around each call; every measurement runs in a
process of its own (two builds of the library do not load together), the configurations alternate
within a round, and a round's figure is the median of its repetitions: compare the rounds' ranges,
not single numbers.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, BATCH, PASSES = 512, 200, 128, 4


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


def make_trainer(**kw):
    from zbot_amd import compile_model, default_config
    from zbot_amd import policy as P
    from zbot_amd.engine import HipEngine
    from zbot_amd.train import Trainer

    eng = HipEngine(compile_model(), default_config(), N, seed=2)
    return Trainer(eng, P.GruPolicy(P.ACTOR, P.init_params(P.ACTOR, 8)), P.GruPolicy(P.CRITIC, P.init_params(P.CRITIC, 9)),
                   rollout_steps=T, num_passes=PASSES, batch_size=BATCH, seed=5, **kw)


def measure_trainer(telemetry):
    import torch

    tr = make_trainer(**({"telemetry": True} if telemetry else {}))
    return dict(iteration_ms=timed(torch, tr.step, 1, 3))


def measure_validate():
    import torch

    tr = make_trainer()
    tr.step()
    return dict(validate_ms=timed(torch, tr.validate, 1, 3))


def measure_summary(T_, n_):
    import torch

    from zbot_amd import ppo

    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    done = (torch.rand(T_, n_, device="cuda", generator=g) < 0.01).to(torch.uint8)
    planes = dict(reward_terms=r(T_, n_, 12), command_terms=r(T_, n_, 5), log_prob=r(T_, n_, 20), values=r(T_, n_),
                  value_targets=r(T_, n_))
    reward, out = r(T_, n_), torch.empty(32, dtype=torch.float64, device="cuda")
    fn = lambda: ppo.rollout_summary(reward, done, done, out=out, **planes)  # noqa: E731
    bytes_read = T_ * n_ * (4 * (12 + 5 + 20 + 3) + 2)
    ms = timed(torch, fn, 20, 200)
    return dict(summary_ms=ms, gb_per_s=bytes_read / ms * 1e-6)


def child(spec):
    sys.path.insert(0, os.path.join(spec.get("root") or ROOT, "ksim-gym-zbot_amd"))
    kind = spec["kind"]
    if kind == "trainer":
        out = measure_trainer(spec["telemetry"])
    elif kind == "validate":
        out = measure_validate()
    else:
        out = measure_summary(spec["T"], spec["n"])
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
    ap.add_argument("--parent-root")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "telemetry_timing.json"))
    a = ap.parse_args()
    if a.child:
        child(json.loads(a.child))
        return
    specs = {"trainer_telemetry_off": dict(kind="trainer", telemetry=False)}
    if a.parent_root:
        specs["trainer_parent_commit"] = dict(kind="trainer", telemetry=False, root=os.path.abspath(a.parent_root))
    specs["trainer_telemetry_on"] = dict(kind="trainer", telemetry=True)
    specs["validate"] = dict(kind="validate")
    specs["summary_200x512"] = dict(kind="summary", T=200, n=512)
    specs["summary_256x8192"] = dict(kind="summary", T=256, n=8192)
    res = {k: [] for k in specs}
    for _ in range(a.rounds):
        for k, s in specs.items():
            res[k].append(run_child(s))
            print(k, res[k][-1], flush=True)
    out = dict(what="ms per call, one figure per round (each the median of its repetitions; a process per measurement, "
                    "configurations alternating within a round)",
               iteration=f"one Trainer.step(), {N} envs x {T} steps, batch {BATCH}, {PASSES} passes",
               validate="one Trainer.validate() at the same size",
               summary="one ppo.rollout_summary, all eight planes (162 B a row), T x n rows; gb_per_s: bytes read / time",
               rounds=a.rounds, results=res)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
