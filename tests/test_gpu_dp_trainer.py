"""zbot_amd.train.Trainer over a process group: two spawned ranks share cuda:0 and
exchange over gloo (RCCL needs one GPU per rank; the one-GPU rehearsal of tests/test_gpu_distributed.py).
Rank r owns envs [32 r, 32 r + 32); T = 8, global batch 32, 2 passes, shuffle on, HipEngine, and
tests/test_gpu_trainer.py's curriculum, which moves after the second iteration.

One spawned run of 3 iterations is shared by the tests (every rank saves what they compare):
  1. iteration 1's rollout and PPO inputs on rank r are rows [32 r, 32 r + 32) of a one-process
     Trainer over 64 envs: the shard invariants of the engine, the sampler and the advantage moments;
  2. after 2 iterations both ranks hold the same params, m, v, level and returned sums;
  3. iteration 1's update replayed in this process from both ranks' saved rollouts, with the library
     calls written out and the two gradients stacked into ppo.grad_combine, gives the ranks' bits;
  4. a second spawned run continues from the state saved after iteration 2, in fresh handles made
     from other weights, and arrives at the uninterrupted run's iteration 3;
  5. a one-rank `nccl` group (RCCL) gives the bits of group=None, and all_gather_rows through RCCL
     returns the row it was given.
Every process group is created with a 60 s timeout: a rank that diverges ends in an error.
"""

import os
import socket
from datetime import timedelta

import pytest
import torch

from zbot_amd import default_config, ppo
from zbot_amd.curriculum import EpisodeLengthCurriculum
from zbot_amd.policy import ACTOR, CRITIC, JOINTS, init_params

pytestmark = pytest.mark.gpu
WORLD, N_LOCAL, T, BATCH, PASSES, SEED, ENGINE_SEED = 2, 32, 8, 32, 2, 5, 2
KW = dict(learning_rate=1e-3, max_grad_norm=0.5, weight_decay=1e-4)  # a maximum the gradient norm exceeds
CUR = EpisodeLengthCurriculum(min_level_steps=1, increase_threshold=0.05, decrease_threshold=0.01)
TIMEOUT = timedelta(seconds=60)
STRIDE = 0x9E3779B97F4A7C15
NETS = ("actor", "critic")
ROLLOUT_KEYS = ("obs_actor", "actions", "log_prob", "reward", "done", "success", "obs_critic", "value", "value_next")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def make_trainer(n, env_offset=0, weights=(8, 9), group=None):
    from zbot_amd import compile_model
    from zbot_amd import policy as P
    from zbot_amd.engine import HipEngine
    from zbot_amd.train import Trainer

    eng = HipEngine(compile_model(), default_config(solver="newton"), n, env_offset=env_offset, seed=ENGINE_SEED)
    actor = P.GruPolicy(ACTOR, init_params(ACTOR, seed=weights[0]))
    critic = P.GruPolicy(CRITIC, init_params(CRITIC, seed=weights[1]))
    return Trainer(eng, actor, critic, rollout_steps=T, num_passes=PASSES, batch_size=BATCH, seed=SEED, shuffle=True,
                   curriculum=CUR, group=group, **KW)


def snap(tr, m):
    """What two runs that should agree are compared on, as CPU tensors and numbers."""
    torch.cuda.synchronize()
    sd = tr.learner.state_dict()
    out = {f"{net}.{k}": sd[net][k].cpu() for net in NETS for k in ("params", "m", "v")}
    out["handle.actor"], out["handle.critic"] = tr.actor.params_tensor().cpu(), tr.critic.params_tensor().cpu()
    out["sums"] = torch.stack(m["sums"]).cpu()
    out["reward_mean"] = m["reward"].double().cpu()
    out["meta"] = (tr.level, tr.cur_state.steps, sd["step"], sd["epoch"], sd["world"], tr.iteration, m["level"],
                   m["episode_length"])
    return out


def same(a, b, skip=()):
    assert a["meta"] == b["meta"], (a["meta"], b["meta"])
    for k in a:
        if k != "meta" and k not in skip:
            assert torch.equal(a[k], b[k]), k


def _dp_rank(rank, world, port, outdir, resume):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
    from zbot_amd.engine import ZbError

    g = dist.group.WORLD
    path = lambda name: os.path.join(outdir, f"{name}_rank{rank}.pt")  # noqa: E731
    if not resume:
        tr = make_trainer(N_LOCAL, env_offset=N_LOCAL * rank, group=g)
        for it in (1, 2, 3):
            m = tr.step()
            torch.save(snap(tr, m), path(f"snap{it}"))
            if it == 1:
                ro = {k: tr.last_rollout[k].cpu() for k in ROLLOUT_KEYS}
                ro["advantages"], ro["value_targets"] = tr.last_inputs.advantages_t.cpu(), tr.last_inputs.value_targets_t.cpu()
                torch.save(ro, path("rollout1"))
            if it == 2:
                torch.save(tr.state_dict(), path("state2"))
    else:
        sd = torch.load(path("state2"), weights_only=False)
        assert (sd["world"], sd["rank"], sd["learner"]["world"]) == (world, rank, world)
        tr = make_trainer(N_LOCAL, env_offset=N_LOCAL * rank, weights=(1, 2), group=g)
        refused = []
        one = {k: v for k, v in sd.items() if k not in ("world", "rank")}  # as a one-process Trainer saves it
        one["learner"] = {k: v for k, v in sd["learner"].items() if k != "world"}
        for bad in (one, dict(sd, world=1), dict(sd, rank=1 - rank), dict(sd, learner=one["learner"])):
            try:
                tr.load_state_dict(bad)
                refused.append(False)
            except ZbError:
                refused.append(True)
        assert refused == [True] * 4, refused
        tr = make_trainer(N_LOCAL, env_offset=N_LOCAL * rank, weights=(1, 2), group=g)
        tr.load_state_dict(sd)
        assert tr.iteration == 2
        m = tr.step()
        torch.save(snap(tr, m), path("resumed3"))
    try:  # an engine that does not own this rank's envs is refused before any collective
        make_trainer(N_LOCAL, env_offset=N_LOCAL * rank + 1, group=g)
        raise AssertionError("a wrong env_offset was accepted")
    except ZbError:
        pass
    dist.barrier()
    dist.destroy_process_group()


def spawn(fn, nprocs, *args):
    import torch.multiprocessing as mp

    mp.start_processes(fn, args=(nprocs, _free_port()) + args, nprocs=nprocs, join=True, start_method="spawn")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The shared two-rank run: {name: [rank 0's, rank 1's]} and the directory it saved into."""
    assert torch.cuda.is_available()
    d = tmp_path_factory.mktemp("dp")
    spawn(_dp_rank, WORLD, str(d), False)
    names = ("snap1", "snap2", "snap3", "rollout1")
    out = {k: [torch.load(d / f"{k}_rank{r}.pt", weights_only=False) for r in range(WORLD)] for k in names}
    out["dir"] = d
    return out


def test_shards_equal_one_process(run):
    tr = make_trainer(WORLD * N_LOCAL)
    m = tr.step()
    torch.cuda.synchronize()
    ro, inp = tr.last_rollout, tr.last_inputs
    for r in range(WORLD):
        got, rows = run["rollout1"][r], slice(N_LOCAL * r, N_LOCAL * (r + 1))
        for k in ("reward", "done", "success", "actions", "log_prob", "value"):
            assert torch.equal(got[k], ro[k][:, rows].cpu()), (r, k)
        assert torch.equal(got["advantages"], inp.advantages_t[:, rows].cpu()), r
        assert torch.equal(got["value_targets"], inp.value_targets_t[:, rows].cpu()), r
        # the metrics that are global: the same episode length, and the reward mean over all ranks
        # (float64 sums over 32 + 32 envs against one over 64: the same value up to the order of the sum)
        assert run["snap1"][r]["meta"][-1] == pytest.approx(m["episode_length"], rel=1e-12)
        want = ro["reward"].double().sum() / ro["reward"].numel()
        assert abs(run["snap1"][r]["reward_mean"].item() - want.item()) <= 1e-12 * abs(want.item()) + 1e-300
    assert not torch.equal(run["rollout1"][0]["reward"], run["rollout1"][1]["reward"])


def test_ranks_agree(run):
    for it in (1, 2, 3):
        a, b = run[f"snap{it}"]
        same(a, b)
        for net in NETS:
            assert torch.equal(a[f"{net}.params"], a[f"handle.{net}"])  # the handles run the learner's weights
    s1, s2, s3 = (run[f"snap{it}"][0] for it in (1, 2, 3))
    steps = PASSES * (N_LOCAL * WORLD // BATCH)
    assert s2["meta"][2:6] == (2 * steps, 2 * PASSES, WORLD, 2)
    assert s2["meta"][0] != s1["meta"][0] and s3["meta"][6] == s2["meta"][0]  # the level moved, for both ranks alike
    assert not torch.equal(s1["actor.params"], s2["actor.params"])
    assert s2["sums"].shape == (steps, 6) and torch.all(s2["sums"][:, 4] == T * BATCH)  # the global row count
    assert torch.isfinite(s3["sums"]).all() and torch.isfinite(s3["actor.params"]).all()


def test_update_by_hand(run):
    """Iteration 1's update from both ranks' saved rollouts, every library call written out."""
    from zbot_amd import policy as P
    from zbot_amd.learner import _ShuffledMinibatches
    from zbot_amd.ppo import PPOInputs

    actor = P.GruPolicy(ACTOR, init_params(ACTOR, seed=8))
    critic = P.GruPolicy(CRITIC, init_params(CRITIC, seed=9))
    shard = []
    for r in range(WORLD):
        ro = {k: v.cuda() for k, v in run["rollout1"][r].items()}
        shard.append(dict(ro=ro, inp=PPOInputs(ro["advantages"], ro["value_targets"], None, None),
                          cut=_ShuffledMinibatches(), seed=(SEED + STRIDE * r) % (1 << 64)))
    assert shard[0]["seed"] == SEED and shard[1]["seed"] != SEED
    ca0, cc0 = actor.initial_carry(N_LOCAL), critic.initial_carry(N_LOCAL)  # a first rollout starts from these
    st = {}
    for net, h in zip(NETS, (actor, critic)):
        p = h.params_tensor()
        st[net] = [p, torch.zeros_like(p), torch.zeros_like(p)]
    sq = torch.zeros(2, dtype=torch.float64, device="cuda")
    b = BATCH // WORLD
    step, all_sums = 0, []
    for epoch in range(PASSES):
        for lo in range(0, N_LOCAL, b):
            ga, gc, sums = [], [], []
            for s in shard:
                mb = s["cut"].cut(torch, s["ro"], s["inp"], ca0, cc0, None, T, N_LOCAL, lo, b, s["seed"], epoch)
                lp, sa = actor.actor_train(mb["obs_a"], mb["acts"], mb["ca"], mb["rs"])
                v, sc = critic.critic_train(mb["obs_c"], mb["cc"], mb["rs"])
                d_lp, d_v, sm = ppo.ppo_loss_grad(lp, mb["old_lp"], mb["adv"], v, mb["old_v"], mb["vt"],
                                                  total=T * b * WORLD)
                gc.append(critic.critic_backward(mb["obs_c"], mb["cc"], mb["rs"], d_v, sc).clone())
                ga.append(actor.actor_backward(mb["obs_a"], mb["acts"], mb["ca"], mb["rs"], d_lp, sa).clone())
                sums.append(sm.clone())
            g_a, _ = ppo.grad_combine(torch.stack(ga), sq_out=sq[0:1])
            g_c, _ = ppo.grad_combine(torch.stack(gc), sq_out=sq[1:2])
            step += 1
            ppo.adamw_step(st["actor"][0], g_a, *st["actor"][1:], sq, step, KW["learning_rate"],
                           max_grad_norm=KW["max_grad_norm"], weight_decay=KW["weight_decay"], frozen_tail=JOINTS)
            ppo.adamw_step(st["critic"][0], g_c, *st["critic"][1:], sq, step, KW["learning_rate"],
                           max_grad_norm=KW["max_grad_norm"], weight_decay=KW["weight_decay"])
            actor.set_params(st["actor"][0])
            critic.set_params(st["critic"][0])
            all_sums.append(sums[0] + sums[1])  # rank order
    torch.cuda.synchronize()
    # the ranks' first permutations differ: they do not shuffle alike
    assert not torch.equal(ppo.minibatch_perm(N_LOCAL, shard[0]["seed"], 0), ppo.minibatch_perm(N_LOCAL, shard[1]["seed"], 0))
    for r in range(WORLD):
        got = run["snap1"][r]
        for net in NETS:
            for name, x in zip(("params", "m", "v"), st[net]):
                assert torch.equal(got[f"{net}.{name}"], x.cpu()), (r, net, name)
        assert torch.equal(got["sums"][:, :4], torch.stack(all_sums).cpu())


def test_resume(run):
    spawn(_dp_rank, WORLD, str(run["dir"]), True)
    for r in range(WORLD):
        same(torch.load(run["dir"] / f"resumed3_rank{r}.pt", weights_only=False), run["snap3"][r])


def _rccl_rank(rank, world, port, outdir):
    import torch.distributed as dist

    from zbot_amd.dist import all_gather_rows

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=TIMEOUT)
    g = dist.group.WORLD
    a, b = make_trainer(N_LOCAL, group=g), make_trainer(N_LOCAL)
    assert (a.world, a.rank, a.learner.group) == (1, 0, None)  # one rank: the learner issues no collective
    for _ in range(2):
        sa, sb = snap(a, a.step()), snap(b, b.step())
        same(sa, sb)
        assert sa["reward_mean"].dtype == sb["reward_mean"].dtype
    grad = a.learner._buf["actor"]["grad"]
    rows = all_gather_rows(grad, torch.zeros(1, grad.numel(), device=dev), g)
    torch.cuda.synchronize()
    assert dist.get_backend(g) == "nccl" and torch.equal(rows[0], grad) and bool(grad.any())
    with open(os.path.join(outdir, "rccl_ok"), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_world_one_through_rccl(tmp_path):
    assert torch.cuda.is_available()
    spawn(_rccl_rank, 1, str(tmp_path))
    assert (tmp_path / "rccl_ok").read_text() == "ok"
