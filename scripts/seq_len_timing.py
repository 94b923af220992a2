"""Timings behind DESIGN.md §4u (truncated BPTT on rollout chunks) -> profiles/seq_len_timing.json.

    python scripts/seq_len_timing.py [--rounds 3] [--parent-root PATH] [--skip PARTS] [--out profiles/seq_len_timing.json]

1. One Trainer iteration at train.py's size (512 envs x 200 steps, batch 128, 4 passes) with
   seq_len None, 100, 50, 25 and 10, and its rollout / update split from Trainer.timing; with
   --parent-root also the parent commit's Trainer (PATH: a checkout of the parent commit with its
   library built; its package is imported instead of this one). The 16 whole-sequence gathers of one
   update are timed in both builds too (the gather's device code is shared with the chunked one).
2. One gradient evaluation of the actor and of the critic at [T', n'] = [200, 128], [100, 256],
   [50, 512], [25, 1024]: the 25 600 rows of one minibatch as chunks; the training forward and the
   backward call apart (device events), and the per-kernel split (forward, head, BPTT, weight gradients)
   from one rocprofv3 kernel trace per shape, in a run of its own: kernel time, without launch gaps.
3. The cosine between the first optimizer step's actor gradient at each seq_len and at seq_len = T, on
   one real rollout of that size.
Device events around each call; every measurement runs in a process of its own (two builds of the
library do not load together), the configurations alternate within a round, and a round's figure is
the median of its repetitions: compare the rounds' ranges, not single numbers. Parts left out with
--skip (trainer, gathers, grad, split, cosine) keep the results an existing --out file holds for them.
"""

import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, BATCH, PASSES = 512, 200, 128, 4
SEQ_LENS = (100, 50, 25, 10)
GRAD_SHAPES = ((200, 128), (100, 256), (50, 512), (25, 1024))


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


def measure_trainer(seq_len):
    import torch

    tr = make_trainer(**({} if seq_len is None else {"seq_len": seq_len}))
    tr.step()
    torch.cuda.synchronize()
    tr.timing = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                 for k in ("rollout", "ppo_inputs", "update")}
    rows = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.step()
        b.record()
        b.synchronize()
        rows.append(dict(iteration_ms=a.elapsed_time(b), **{f"{k}_ms": s.elapsed_time(e) for k, (s, e) in tr.timing.items()}))
    return {k: statistics.median(r[k] for r in rows) for k in rows[0]}


def measure_gathers():
    """The 16 whole-sequence gathers of one update (zb_minibatch_gather), on a real rollout: the items
    HipPpoLearner cuts per minibatch (seven [T, n] arrays, both carries, the reset rows built in the
    gather), through ppo.gather_minibatch."""
    import torch

    from zbot_amd import ppo

    tr = make_trainer()
    tr.step()
    ro, inp = tr.last_rollout, tr.last_inputs
    ca, cc = tr.rollout.carry.clone(), tr.critic_carry.clone()
    src = [ro["obs_actor"], ro["actions"], ro["obs_critic"], ro["log_prob"], ro["value"], inp.advantages_t,
           inp.value_targets_t]
    dst = [torch.empty((T, BATCH) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device) for x in src]
    dca, dcc = torch.empty_like(ca[:BATCH]), torch.empty_like(cc[:BATCH])
    rs = torch.empty(T, BATCH, dtype=torch.uint8, device=ca.device)
    items = list(zip(src, dst)) + [(ca[None], dca[None]), (cc[None], dcc[None]), (None, rs[:1]), (ro["done"], rs[1:])]

    def fn():
        for epoch in range(PASSES):
            for lo in range(0, N, BATCH):
                ppo.gather_minibatch(items, N, lo, BATCH, shuffle_seed=5, epoch=epoch)

    return dict(gathers_ms=timed(torch, fn, 3, 20))


TRACED_EVALUATIONS = 5


def measure_grad(kind_name, T_, n_, traced=False):
    import torch

    from zbot_amd import policy as P

    kind = P.ACTOR if kind_name == "actor" else P.CRITIC
    dev = torch.device("cuda", 0)
    I = P.ACTOR_IN if kind == P.ACTOR else P.CRITIC_IN
    g = torch.Generator(device="cpu").manual_seed(7)
    obs = torch.randn(T_, n_, I, generator=g).to(dev)
    carry0 = (0.5 * torch.randn(n_, P.DEPTH, P.HIDDEN, generator=g)).to(dev)
    reset = (torch.rand(T_, n_, generator=g) < 0.01).to(torch.uint8).to(dev)
    acts = (0.4 * torch.randn(T_, n_, P.JOINTS, generator=g)).to(dev)
    dout = torch.randn(*((T_, n_, P.JOINTS) if kind == P.ACTOR else (T_, n_)), generator=g).to(dev)
    net = P.GruPolicy(kind, P.init_params(kind, seed=1))
    scratch = torch.empty(net.train_scratch_words(T_, n_), dtype=torch.float32, device=dev)
    grad = torch.empty(P.param_count(kind), dtype=torch.float32, device=dev)

    def fwd():
        if kind == P.ACTOR:
            net.actor_train(obs, acts, carry0, reset, scratch=scratch)
        else:
            net.critic_train(obs, carry0, reset, scratch=scratch)

    def bwd():
        if kind == P.ACTOR:
            net.actor_backward(obs, acts, carry0, reset, dout, scratch, grad=grad)
        else:
            net.critic_backward(obs, carry0, reset, dout, scratch, grad=grad)

    def both():
        fwd()
        bwd()

    if traced:  # under the kernel trace: a fixed number of evaluations, nothing timed here
        for _ in range(TRACED_EVALUATIONS):
            both()
        torch.cuda.synchronize()
        return dict(evaluations=TRACED_EVALUATIONS)
    fwd()
    return dict(forward_ms=timed(torch, fwd, 2, 7), backward_ms=timed(torch, bwd, 2, 7), evaluation_ms=timed(torch, both, 2, 7))


def chunks_of(x, L, cols):
    """[>= T, n, ...] -> [L, C b, ...], column c b + j = rows c L .. c L + L - 1 of env cols[j]: the chunk law in torch."""
    y = x[:T].index_select(1, cols)
    tail = tuple(y.shape[2:])
    return y.reshape((T // L, L, len(cols)) + tail).transpose(0, 1).reshape((L, (T // L) * len(cols)) + tail).contiguous()


def measure_cosine():
    """The first optimizer step's actor gradient on one real rollout: every seq_len against seq_len = T.
    The first minibatch of the first pass, cut by the chunk law in torch indexing; with the weights
    that collected the rollout the ratio is exactly 1, so the value arguments of the loss do not
    reach d_log_prob."""
    import torch

    from zbot_amd import compile_model, default_config, ppo
    from zbot_amd import policy as P
    from zbot_amd.engine import HipEngine

    eng = HipEngine(compile_model(), default_config(), N, seed=2)
    actor, critic = P.GruPolicy(P.ACTOR, P.init_params(P.ACTOR, 8)), P.GruPolicy(P.CRITIC, P.init_params(P.CRITIC, 9))
    ro = P.PolicyRollout(eng, actor, seed=5, curriculum=0.5)
    # the carries of every step: those of any seq_len are every seq_len-th row
    out = ro.run(T, record_critic=True, critic=critic, critic_carry=critic.initial_carry(N), carry_every=1)
    inp = ppo.compute_ppo_inputs(out["value"], out["reward"], out["done"], out["success"], bootstrap=out["value_next"])
    reset = torch.zeros(T, N, dtype=torch.uint8, device="cuda")
    reset[1:] = out["done"][:T - 1]
    cols = ppo.minibatch_perm(N, 5, 0)[:BATCH].long()
    grads = {}
    for L in (T,) + SEQ_LENS:
        c = lambda x: chunks_of(x, L, cols)  # noqa: E731
        obs, acts, rs = c(out["obs_actor"]), c(out["actions"]), c(reset)
        carry = out["actor_carry_chunks"][::L].index_select(1, cols).reshape(-1, P.DEPTH, P.HIDDEN).contiguous()
        lp, scr = actor.actor_train(obs, acts, carry, rs)
        assert torch.equal(lp, c(out["log_prob"]))  # the rollout's own log-probs: ratio exactly 1
        d_lp, _, _ = ppo.ppo_loss_grad(lp, c(out["log_prob"]), c(inp.advantages_t), c(out["value"]), c(out["value"]),
                                       c(inp.value_targets_t))
        grads[L] = actor.actor_backward(obs, acts, carry, rs, d_lp, scr).double().clone()
    ref = grads[T][:-P.JOINTS]
    res = {f"cosine_seq_len_{L}": float(torch.dot(g[:-P.JOINTS], ref) / (g[:-P.JOINTS].norm() * ref.norm()))
           for L, g in grads.items()}
    res.update({f"norm_ratio_seq_len_{L}": float(g[:-P.JOINTS].norm() / ref.norm()) for L, g in grads.items()})
    return res


# kernel-name substrings, the backward's kernels first: their argument types may hold the word "policy"
KERNEL_GROUPS = (("head", ("head_kernel",)), ("bptt", ("bptt_kernel",)), ("wgrad", ("wgrad_kernel", "wreduce_kernel")),
                 ("forward", ("policy_kernel", "policy_wave_kernel")))


def measure_split(net, T_, n_):
    """Kernel time per evaluation and group, from rocprofv3's kernel statistics of a traced child."""
    spec = dict(kind="grad", net=net, T=T_, n=n_, traced=True)
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable,
                            os.path.abspath(__file__), "--child", json.dumps(spec)], capture_output=True, text=True,
                           timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            raise SystemExit(f"kernel trace {spec} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        with open(files[0], newline="") as f:
            rows = list(csv.DictReader(f))
    out = {g: 0.0 for g in ("forward", "head", "bptt", "wgrad", "other")}
    if not rows or "Name" not in rows[0] or "TotalDurationNs" not in rows[0]:
        raise SystemExit(f"kernel statistics without the columns Name / TotalDurationNs: {list(rows[0]) if rows else rows}")
    for r in rows:
        name, total_ms = r["Name"], float(r["TotalDurationNs"]) * 1e-6
        group = next((g for g, keys in KERNEL_GROUPS if any(k in name for k in keys)), "other")
        out[group] += total_ms / TRACED_EVALUATIONS
    res = {f"{g}_ms": v for g, v in out.items()}
    res["other_kernels"] = sorted({r["Name"][:60] for r in rows
                                   if not any(k in r["Name"] for _, keys in KERNEL_GROUPS for k in keys)})
    return res


def child(spec):
    sys.path.insert(0, os.path.join(spec.get("root") or ROOT, "ksim-gym-zbot_amd"))
    kind = spec["kind"]
    if kind == "trainer":
        out = measure_trainer(spec["seq_len"])
    elif kind == "gathers":
        out = measure_gathers()
    elif kind == "grad":
        out = measure_grad(spec["net"], spec["T"], spec["n"], spec.get("traced", False))
    else:
        out = measure_cosine()
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
    ap.add_argument("--skip", default="", help="comma separated: trainer, gathers, grad, split, cosine")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_len_timing.json"))
    a = ap.parse_args()
    if a.child:
        child(json.loads(a.child))
        return
    skip = set(filter(None, a.skip.split(",")))
    specs = {}
    parent = os.path.abspath(a.parent_root) if a.parent_root else None
    if "trainer" not in skip:
        specs["trainer_seq_len_none"] = dict(kind="trainer", seq_len=None)
        if parent:
            specs["trainer_parent_commit"] = dict(kind="trainer", seq_len=None, root=parent)
        for L in SEQ_LENS:
            specs[f"trainer_seq_len_{L}"] = dict(kind="trainer", seq_len=L)
    if "gathers" not in skip:
        specs["gathers"] = dict(kind="gathers")
        if parent:
            specs["gathers_parent_commit"] = dict(kind="gathers", root=parent)
    if "grad" not in skip:
        for net in ("actor", "critic"):
            for T_, n_ in GRAD_SHAPES:
                specs[f"grad_{net}_{T_}x{n_}"] = dict(kind="grad", net=net, T=T_, n=n_)
    res = {}
    if os.path.exists(a.out):  # the parts skipped in this run keep what an earlier one measured
        with open(a.out) as f:
            res = json.load(f).get("results", {})
    res.update({k: [] for k in specs})
    for _ in range(a.rounds):
        for k, s in specs.items():
            res[k].append(run_child(s))
            print(k, res[k][-1], flush=True)
    def write():
        out = dict(what="ms per call, one figure per round (each the median of its repetitions; a process per "
                        "measurement, configurations alternating within a round)",
                   trainer=f"one Trainer.step(), {N} envs x {T} steps, batch {BATCH}, {PASSES} passes; rollout / "
                           "ppo_inputs / update from Trainer.timing",
                   gathers=f"the {PASSES * (N // BATCH)} whole-sequence gathers of one update, in one timed call",
                   grad="one gradient evaluation at [T', n']: the training forward, the backward call, and both together",
                   split="kernel time per gradient evaluation at [T', n'] from a kernel trace: the training forward, the "
                         "head, the BPTT kernel, the weight gradients with their reduction, everything else",
                   first_step_actor_gradient="cosine between the actor gradient of the first minibatch at seq_len and at "
                                             f"seq_len = {T} (whole sequences), the loss seeds of ratio 1; norm_ratio: "
                                             "their norms' ratio",
                   rounds=a.rounds, results=res)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    write()  # what is measured so far survives a failure of a later part
    if "cosine" not in skip:
        res["first_step_actor_gradient"] = [run_child(dict(kind="cosine"))]
        print(res["first_step_actor_gradient"][-1], flush=True)
        write()
    if "split" not in skip:  # after the timed rounds, alone: a trace slows what runs beside it
        for net in ("actor", "critic"):
            for T_, n_ in GRAD_SHAPES:
                k = f"split_{net}_{T_}x{n_}"
                res[k] = [measure_split(net, T_, n_)]
                print(k, res[k][-1], flush=True)
        write()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
