#!/usr/bin/env python3
"""zb_grad_combine against the bytes it moves, and what the data-parallel path adds to an optimizer step.

On one GPU, device events around each call, `--warmup` runs and then the median and range of `--repeats`:
  combine   ppo.grad_combine at world = 8 over the actor's parameter count: reads 4 world count bytes,
            writes 4 count; the time is set beside 4 (world + 1) count bytes. The buffers are a few MB
            and stay in the L2 / Infinity Cache between runs: the figure is a cache-resident one, not
            an HBM stream.
  sqnorm    ppo.grad_sqnorm over the same count: the launch the combine replaces.
  dp_step   at world 1 through RCCL (a one-rank `nccl` group): per network all_gather_rows of the
            gradient and grad_combine of the gathered rows, both networks, against the two
            grad_sqnorm launches of a one-process step. The difference is what the path adds to a
            step before any second GPU exists; multi-GPU scaling cannot be measured on one GPU.

    python scripts/grad_combine_timing.py --out profiles/grad_combine_timing.json
"""

import argparse
import json
import os
import statistics
import sys
from datetime import timedelta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ksim-gym-zbot_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-rccl", action="store_true", help="skip the dp_step leg (no process group is created)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from zbot_amd import policy as P
    from zbot_amd import ppo
    from zbot_amd.dist import all_gather_rows

    if not torch.cuda.is_available():
        raise SystemExit("grad_combine_timing needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    counts = dict(actor=P.param_count(P.ACTOR), critic=P.param_count(P.CRITIC))
    g = torch.Generator(device="cpu").manual_seed(3)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), rounds=len(ms))

    count = counts["actor"]
    parts = torch.randn(a.world, count, generator=g).to(dev)
    grad = torch.empty(count, device=dev)
    sq = torch.zeros(2, dtype=torch.float64, device=dev)
    part = torch.empty(int(ppo.load_library().zb_sqnorm_partials_words(count)), dtype=torch.float64, device=dev)
    res = dict(device=torch.cuda.get_device_name(0), world=a.world, count=count, warmup=a.warmup)
    res["combine"] = timed(lambda: ppo.grad_combine(parts, out=grad, sq_out=sq[0:1], partials=part))
    nbytes = 4 * (a.world + 1) * count
    res["combine"].update(bytes=nbytes, gb_per_s=nbytes / (res["combine"]["median_ms"] * 1e-3) / 1e9,
                          note="buffers of a few MB, cache-resident between runs")
    res["sqnorm"] = timed(lambda: ppo.grad_sqnorm(grad, out=sq[0:1], partials=part))
    res["sqnorm"].update(bytes=4 * count)

    if not a.no_rccl:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev, timeout=timedelta(seconds=60))
        grp = dist.group.WORLD
        buf = {}
        for k, (net, cnt) in enumerate(counts.items()):
            buf[net] = dict(k=k, grad=torch.randn(cnt, generator=g).to(dev), rows=torch.empty(1, cnt, device=dev),
                            out=torch.empty(cnt, device=dev),
                            part=torch.empty(int(ppo.load_library().zb_sqnorm_partials_words(cnt)), dtype=torch.float64,
                                             device=dev))

        def dp():
            for b in buf.values():
                all_gather_rows(b["grad"], b["rows"], grp)
                ppo.grad_combine(b["rows"], out=b["out"], sq_out=sq[b["k"]:b["k"] + 1], partials=b["part"])

        def single():
            for b in buf.values():
                ppo.grad_sqnorm(b["grad"], out=sq[b["k"]:b["k"] + 1], partials=b["part"])

        res["dp_step"] = dict(backend=dist.get_backend(grp), world=1, gather_and_combine=timed(dp), two_sqnorm=timed(single))
        res["dp_step"]["added_ms"] = (res["dp_step"]["gather_and_combine"]["median_ms"]
                                      - res["dp_step"]["two_sqnorm"]["median_ms"])
        dist.destroy_process_group()

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
