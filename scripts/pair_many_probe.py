"""C2 rates of the nine-collider model with and without the sole pair, and of the limbs + pair model,
in one process (needs a GPU). The three runs use bench.py's own C2 settings and timing
(bench_general_colliders, bench_variant): 8192 envs, the CG solver, two env groups.

  many       assets/zbot_like_many.xml: two banks of floor colliders (the XG 5 kernels)
  many_pair  the same description whose soles also collide with each other: the pair's rows in a
             bank of their own beside the floor colliders' (the XG 6 kernels; before them the XG 4
             kernels, whose one floor bank holds two colliders)
  limbs_pair assets/zbot_like_limbs.xml with the sole pair (the XG 4 kernels)

Prints one JSON line: the three env-step rates and how many envs of the many_pair run ever had more
colliders beyond the soles within reach of the floor than its banks hold (the run replayed on one
handle: the same bits).

    python scripts/pair_many_probe.py [--steps K] [--warmup W]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ksim-gym-zbot_amd")]
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--solver", default="cg", choices=["newton", "cg"])
    ap.add_argument("--groups", type=int, default=2)
    args = ap.parse_args()
    import torch
    from zbot_amd import compile_model, default_config
    from zbot_amd.engine import HipEngine
    from zbot_amd.mjcf import load_mjcf

    conf = bench.CONFIGS["c2"]
    n, seed, G = conf["envs"], 0, max(1, args.groups)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = default_config(push=conf["push"], randomize=conf["randomize"], solver=args.solver)
    assets = os.path.join(ROOT, "ksim-gym-zbot_amd", "assets")
    pair = [["left_foot_sole", "right_foot_sole"]]

    many = bench.bench_general_colliders(cfg, n, args.steps, args.warmup, dev, 0, 1, seed, G, "zbot_like_many.xml")
    mdesc = load_mjcf(os.path.join(assets, "zbot_like_many.xml"))
    mdesc["self_pairs"] = pair
    cm_mp = compile_model(mdesc)
    many_pair = bench.bench_variant(cm_mp, cfg, "the sole pair beside the nine-collider model's seven others", "", n,
                                    args.steps, args.warmup, dev, 0, 1, seed, G)
    ldesc = load_mjcf(os.path.join(assets, "zbot_like_limbs.xml"))
    ldesc["self_pairs"] = pair
    limbs_pair = bench.bench_variant(compile_model(ldesc), cfg, "the sole pair beside the limbs model's two others", "", n,
                                     args.steps, args.warmup, dev, 0, 1, seed, G)
    # the many_pair run again on one handle (the same reset, actions and step count, so the same bits)
    eng = HipEngine(cm_mp, cfg, n, device=dev.index, seed=seed)
    acts = bench._synthetic_actions(n, 64, dev, 1234, 0.05)
    eng.reset()
    for t in range(args.warmup + args.steps):
        eng.step(acts[t % 64], extras=False)
    over = int(eng.flags()["bank_overflow"].sum().item())
    print(json.dumps({
        "probe": "pair_many", "envs": n, "solver": args.solver, "groups": G, "steps": args.steps, "warmup": args.warmup,
        "many_env_steps_per_s": many["env_steps_per_s"], "many_bank_overflow_envs": many.get("bank2_overflow_envs"),
        "many_pair_env_steps_per_s": many_pair["env_steps_per_s"], "many_pair_bank_overflow_envs": over,
        "limbs_pair_env_steps_per_s": limbs_pair["env_steps_per_s"],
    }))


if __name__ == "__main__":
    main()
