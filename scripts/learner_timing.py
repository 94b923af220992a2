#!/usr/bin/env python3
"""Training forward + backward of the GRU actor / critic: the HIP path against torch autograd.

Times, on one GPU, one gradient evaluation (forward over T steps + the VJP) of
  hip    zb_policy_*_train + zb_policy_*_backward (include/zbot_policy.h "Training")
  torch  the fp32 torch restatement (tests/policy_torch.py: forward + backward()) on the same GPU,
         i.e. what a user would run without this library's backward pass. It is reference code, not
         the code under test, and is run as it is.
at train.py's minibatch (128 envs x 200 steps, train.py:1771, 1775: 4 s of 0.02 s control steps)
and at 1024 x 200. Both paths are warmed up at every shape, then timed alternately (hip, torch, hip,
...) with device events around each evaluation; medians with min / max are reported, and both
gradients are compared at the timed size with the same restatement in fp64 on the GPU
(max |g - g64| / max |g64| over the whole gradient).

FLOP count of one gradient evaluation per env-step (FMA = 2), matrix products only, with
F = 2 (I H + D 6 H^2 + H O) the forward's count (policy.FLOP_ACTOR / FLOP_CRITIC):
  forward F  +  backward's transposed products 2 (D 6 H^2 + H O)  +  weight gradients F
  = 3 F - 2 I H
(the observations get no gradient, so the input projection has no transposed product). The share
of peak is that count over the hip time over the f32 matrix-core peak, 157.3 TFLOP/s: an
end-to-end figure of the whole evaluation, not one kernel's.

    python scripts/learner_timing.py --out profiles/learner_timing.json
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ksim-gym-zbot_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_F32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128x200,1024x200", help="envs x steps, comma separated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import policy_torch as PT
    from zbot_amd import policy as P

    if not torch.cuda.is_available():
        raise SystemExit("learner_timing needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    results = []
    for size in a.sizes.split(","):
        n, T = (int(x) for x in size.split("x"))
        for kind, name in ((P.ACTOR, "actor"), (P.CRITIC, "critic")):
            I, O = P._dims(kind)
            H, D = P.HIDDEN, P.DEPTH
            fwd = 2 * (I * H + D * 6 * H * H + H * O)
            assert fwd == (P.FLOP_ACTOR if kind == P.ACTOR else P.FLOP_CRITIC)
            flop = (3 * fwd - 2 * I * H) * n * T
            g = torch.Generator(device="cpu").manual_seed(7)
            prm = torch.from_numpy(P.init_params(kind, seed=1))
            obs = torch.randn(T, n, I, generator=g).to(dev)
            carry0 = (0.5 * torch.randn(n, D, H, generator=g)).to(dev)
            reset = (torch.rand(T, n, generator=g) < 0.01).to(torch.uint8).to(dev)
            acts = (0.4 * torch.randn(T, n, P.JOINTS, generator=g)).to(dev)
            dout = torch.randn(*((T, n, P.JOINTS) if kind == P.ACTOR else (T, n)), generator=g).to(dev)
            net = P.GruPolicy(kind, prm.numpy())
            scratch = torch.empty(net.train_scratch_words(T, n), dtype=torch.float32, device=dev)
            grad = torch.empty(P.param_count(kind), dtype=torch.float32, device=dev)
            flat = prm.to(dev).requires_grad_()

            def hip():
                if kind == P.ACTOR:
                    net.actor_train(obs, acts, carry0, reset, scratch=scratch)
                    return net.actor_backward(obs, acts, carry0, reset, dout, scratch, grad=grad)
                net.critic_train(obs, carry0, reset, scratch=scratch)
                return net.critic_backward(obs, carry0, reset, dout, scratch, grad=grad)

            def ref():
                flat.grad = None
                if kind == P.ACTOR:
                    out = PT.actor_log_prob(flat, obs, carry0, reset, acts)
                else:
                    out = PT.critic_value(flat, obs, carry0, reset)
                (out * dout).sum().backward()
                return flat.grad

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            for _ in range(a.warmup):
                hip()
                ref()
            torch.cuda.synchronize()
            th, tr = [], []
            for _ in range(a.repeats):
                th.append(timed(hip))
                tr.append(timed(ref))
            gh, gr = hip().clone(), ref().clone()
            torch.cuda.synchronize()
            live = gh.numel() - (P.JOINTS if kind == P.ACTOR else 0)
            # both against the same restatement in fp64 on the GPU: max |g - g64| / max |g64|
            f64 = prm.to(dev).double().requires_grad_()
            if kind == P.ACTOR:
                o64 = PT.actor_log_prob(f64, obs.double(), carry0.double(), reset, acts.double())
            else:
                o64 = PT.critic_value(f64, obs.double(), carry0.double(), reset)
            (g64,) = torch.autograd.grad((o64 * dout.double()).sum(), f64)
            del o64
            scale = g64[:live].abs().max()
            err_hip = ((gh[:live].double() - g64[:live]).abs().max() / scale).item()
            err_ref = ((gr[:live].double() - g64[:live]).abs().max() / scale).item()
            mh, mr = statistics.median(th), statistics.median(tr)
            row = dict(net=name, envs=n, steps=T, hip_ms=dict(median=mh, min=min(th), max=max(th)),
                       torch_ms=dict(median=mr, min=min(tr), max=max(tr)), torch_over_hip=mr / mh,
                       flop_per_env_step=3 * fwd - 2 * I * H, flop=flop, hip_tflops=flop / (mh * 1e-3) / 1e12,
                       hip_fraction_of_f32_mfma_peak=flop / (mh * 1e-3) / PEAK_F32_MFMA,
                       scratch_mib=scratch.numel() * 4 / 2**20, hip_err_vs_fp64=err_hip, torch_err_vs_fp64=err_ref,
                       repeats=a.repeats, warmup=a.warmup)
            print(json.dumps(row), flush=True)
            results.append(row)
            del scratch, net
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), peak_f32_mfma_flops=PEAK_F32_MFMA, rows=results), f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
