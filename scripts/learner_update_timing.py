#!/usr/bin/env python3
"""One PPO optimizer step: HipPpoLearner (every step in libzbot_hip.so) against PpoLearner (torch loss,
clip and AdamW around the same HIP forward / backward kernels), and the three new steps alone.

At train.py's minibatch (128 envs x 200 steps, train.py:1771, 1775), on one GPU:
  step    one update(..., num_passes=1, batch_size=envs) of each learner: training forwards, loss,
          backward passes, norm, AdamW, set_params. The two learners are warmed up, then timed
          alternately (torch, hip, torch, ...) with device events around each update.
  stages  the three steps include/zbot_ppo.h "Learner" adds, alone, against their torch counterparts:
            loss   zb_ppo_loss            | learner.ppo_loss forward + autograd to d_log_prob, d_value
            norm   2 x zb_grad_sqnorm     | torch.nn.utils.clip_grad_norm_ over both networks
            adamw  2 x zb_adamw_step      | torch.optim.AdamW.step over both networks
          (the clip's scaling of the gradient is part of zb_adamw_step on the hip side and of
          clip_grad_norm_ on the torch side). Same protocol.
Medians with (min - max) of the timed rounds; `hip_stage_share` is the sum of the three hip stage
medians over the hip step median.

    python scripts/learner_update_timing.py --out profiles/learner_update_timing.json
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ksim-gym-zbot_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="128x200", help="envs x steps")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--first", default="torch", choices=("torch", "hip"), help="which learner each round times first")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from zbot_amd import learner as LN
    from zbot_amd import policy as P
    from zbot_amd import ppo

    if not torch.cuda.is_available():
        raise SystemExit("learner_update_timing needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    n, T = (int(x) for x in a.size.split("x"))
    g = torch.Generator(device="cpu").manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    D, H, NJ = P.DEPTH, P.HIDDEN, P.JOINTS
    obs_a, obs_c = rn(T, n, P.ACTOR_IN), rn(T, n, P.CRITIC_IN)
    carry_a, carry_c = 0.5 * rn(n, D, H), 0.5 * rn(n, D, H)
    reset = (torch.rand(T, n, generator=g) < 0.01).to(torch.uint8).to(dev)
    acts = 0.4 * rn(T, n, NJ)
    pa, pc = P.init_params(P.ACTOR, seed=1), P.init_params(P.CRITIC, seed=2)

    def nets():
        return P.GruPolicy(P.ACTOR, pa), P.GruPolicy(P.CRITIC, pc)

    # a second-pass flavoured batch: the rollout's log-probs / values are the networks' own plus noise
    probe_a, probe_c = nets()
    lp0, _ = probe_a.actor_train(obs_a, acts, carry_a, reset)
    v0, _ = probe_c.critic_train(obs_c, carry_c, reset)
    rollout = dict(obs_actor=obs_a, actions=acts, obs_critic=obs_c, log_prob=lp0 + 0.01 * rn(T, n, NJ),
                   value=v0 + 0.1 * rn(T, n))
    inputs = ppo.PPOInputs(advantages_t=rn(T, n), value_targets_t=v0 + 0.5 * rn(T, n), gae_t=None, returns_t=None)
    del probe_a, probe_c
    torch.cuda.empty_cache()

    ha, hc = nets()
    hip_learner = LN.HipPpoLearner()
    ta, tc = (LN.TrainablePolicy(x) for x in nets())
    torch_learner = LN.PpoLearner()

    def hip_step():
        hip_learner.update(rollout, inputs, ha, hc, carry_a, carry_c, reset=reset, num_passes=1, batch_size=n)

    def torch_step():
        torch_learner.update(rollout, inputs, ta, tc, carry_a, carry_c, reset=reset, num_passes=1, batch_size=n)

    # the stages alone
    cnt_a, cnt_c = P.param_count(P.ACTOR), P.param_count(P.CRITIC)
    grad_a, grad_c = 1e-2 * rn(cnt_a), 1e-2 * rn(cnt_c)
    d_lp, d_v = torch.empty(T, n, NJ, device=dev), torch.empty(T, n, device=dev)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    lpart = torch.empty(int(ppo.load_library().zb_ppo_loss_partials_words(T, n)), dtype=torch.float64, device=dev)
    sq = torch.zeros(2, dtype=torch.float64, device=dev)
    spart = [torch.empty(int(ppo.load_library().zb_sqnorm_partials_words(c)), dtype=torch.float64, device=dev)
             for c in (cnt_a, cnt_c)]
    st = [[torch.from_numpy(p).to(dev), torch.zeros(p.size, device=dev), torch.zeros(p.size, device=dev)]
          for p in (pa, pc)]
    tpar = [torch.nn.Parameter(torch.from_numpy(p).to(dev)) for p in (pa, pc)]
    opt = torch.optim.AdamW(tpar, lr=LN.DEFAULT_LEARNING_RATE, weight_decay=LN.DEFAULT_WEIGHT_DECAY)
    lp_leaf, v_leaf = lp0.clone().requires_grad_(), v0.clone().requires_grad_()
    step = [0]

    def hip_loss():
        ppo.ppo_loss_grad(lp0, rollout["log_prob"], inputs.advantages_t, v0, rollout["value"], inputs.value_targets_t,
                          d_log_prob=d_lp, d_value=d_v, sums=sums, partials=lpart)

    def torch_loss():
        loss = LN.ppo_loss(lp_leaf, rollout["log_prob"], inputs.advantages_t, v_leaf, rollout["value"],
                           inputs.value_targets_t)
        torch.autograd.grad(loss, (lp_leaf, v_leaf))

    def hip_norm():
        ppo.grad_sqnorm(grad_a, out=sq[0:1], partials=spart[0])
        ppo.grad_sqnorm(grad_c, out=sq[1:2], partials=spart[1])

    def torch_norm():
        tpar[0].grad, tpar[1].grad = grad_a.clone(), grad_c.clone()
        torch.nn.utils.clip_grad_norm_(tpar, LN.DEFAULT_MAX_GRAD_NORM)

    def hip_adamw():
        step[0] += 1
        for (p, m, v), gr, tail in zip(st, (grad_a, grad_c), (NJ, 0)):
            ppo.adamw_step(p, gr, m, v, sq, step[0], LN.DEFAULT_LEARNING_RATE, max_grad_norm=LN.DEFAULT_MAX_GRAD_NORM,
                           weight_decay=LN.DEFAULT_WEIGHT_DECAY, frozen_tail=tail)

    def torch_adamw():
        opt.step()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def race(first, second):
        """Warm both up, then alternate first, second, first, ... -> (times of first, of second)."""
        for _ in range(a.warmup):
            first()
            second()
        torch.cuda.synchronize()
        t1, t2 = [], []
        for _ in range(a.repeats):
            t1.append(timed(first))
            t2.append(timed(second))
        return t1, t2

    stat = lambda t: dict(median=statistics.median(t), min=min(t), max=max(t))  # noqa: E731
    res = dict(device=torch.cuda.get_device_name(0), envs=n, steps=T, warmup=a.warmup, repeats=a.repeats)
    if a.first == "torch":
        tt, th = race(torch_step, hip_step)
    else:
        th, tt = race(hip_step, torch_step)
    res["first"] = a.first
    res["step_ms"] = dict(torch=stat(tt), hip=stat(th))
    print(json.dumps(dict(step_ms=res["step_ms"])), flush=True)
    hip_norm()  # sq holds real norms before AdamW is timed; torch_norm leaves .grad for opt.step
    torch_norm()
    res["stages_ms"] = {}
    for name, tf, hf in (("loss", torch_loss, hip_loss), ("norm", torch_norm, hip_norm), ("adamw", torch_adamw, hip_adamw)):
        tt, th = race(tf, hf)
        res["stages_ms"][name] = dict(torch=stat(tt), hip=stat(th))
        print(json.dumps({name: res["stages_ms"][name]}), flush=True)
    for side in ("torch", "hip"):
        res[f"{side}_stage_share"] = (sum(res["stages_ms"][k][side]["median"] for k in res["stages_ms"])
                                      / res["step_ms"][side]["median"])
    print(json.dumps(dict(torch_stage_share=res["torch_stage_share"], hip_stage_share=res["hip_stage_share"])))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
