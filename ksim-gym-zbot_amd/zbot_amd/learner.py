"""The learner's half of PPO: gradients through the GRU actor / critic, and the update.

Mirrors what ksim's PPOTask does with train.py's model after a rollout:
get_ppo_variables (train.py:1683-1729) scans both networks over the trajectory and is
differentiated through, the loss is ksim's PPO loss (un-vendored ksim/task/ppo.py [U]) and the
optimizer is ZbotWalkingTask.get_optimizer (train.py:1314-1324).

The hot path — the activation-saving forward and the backward pass through 5 GRU layers x T
steps — runs in libzbot_hip.so (include/zbot_policy.h "Training"); there is no PyTorch or CPU
fallback for it. In PpoLearner the loss and the optimizer are ordinary torch; HipPpoLearner runs
the same update with those steps in the library too (include/zbot_ppo.h "Learner"), and the torch
path stays as the second implementation it is compared with:

    actor, critic = GruPolicy(ACTOR, ...), GruPolicy(CRITIC, ...)
    ta, tc = TrainablePolicy(actor), TrainablePolicy(critic)
    lp = ta.log_prob(obs, actions, carry0, reset)      # [T, n, 20], bits of actor.actor(mode=EVAL)
    v = tc.value(obs_critic, carry0_c, reset)          # [T, n]
    ppo_loss(lp, old_lp, adv, v, old_v, targets).backward()   # -> ta.param.grad, tc.param.grad

`TrainablePolicy.param` is one flat torch.nn.Parameter in the natural layout. Whenever it has
changed (an optimizer step), the next forward pushes it to the handle, which keeps serving
PolicyRollout with the updated weights.
"""

from __future__ import annotations

import struct

from .engine import ZbError
from .policy import ACTOR, JOINTS, GruPolicy

# ZbotWalkingTaskConfig (train.py:1079-1090) and the launch line (train.py:1771-1775)
DEFAULT_LEARNING_RATE = 3e-4    # train.py:1080
DEFAULT_MAX_GRAD_NORM = 2.0     # train.py:1084
DEFAULT_WEIGHT_DECAY = 1e-5     # train.py:1088
DEFAULT_NUM_PASSES = 4          # train.py:1773
DEFAULT_BATCH_SIZE = 128        # train.py:1771: envs per minibatch
# ksim PPOConfig defaults [U]
DEFAULT_CLIP_PARAM = 0.2        # [U]
DEFAULT_VALUE_LOSS_COEF = 0.5   # [U]
DEFAULT_USE_CLIPPED_VALUE_LOSS = True  # [U]
DEFAULT_LOG_CLIP_VALUE = 10.0   # [U] bound on the log ratio before exp
RANK_SEED_STRIDE = 0x9E3779B97F4A7C15  # rank r shuffles with (shuffle_seed + r x this) mod 2^64


def _function():
    """The autograd function, built on first use (torch is imported lazily, as in policy.py)."""
    import torch  # noqa: PLC0415

    class _Net(torch.autograd.Function):
        @staticmethod
        def forward(ctx, param, tp, obs, actions, carry0, reset):  # noqa: ARG004 - param carries the graph edge
            pol = tp.policy
            if pol.kind == ACTOR:
                out, scratch = pol.actor_train(obs, actions, carry0, reset)
            else:
                out, scratch = pol.critic_train(obs, carry0, reset)
            ctx.tp, ctx.args, ctx.scratch = tp, (obs, actions, carry0, reset), scratch
            ctx.pushed = tp._pushed
            return out

        @staticmethod
        def backward(ctx, d_out):
            tp = ctx.tp
            if tp._pushed != ctx.pushed:
                raise ZbError("the parameters were pushed to the handle between forward and backward")
            obs, actions, carry0, reset = ctx.args
            pol = tp.policy
            if pol.kind == ACTOR:
                g = pol.actor_backward(obs, actions, carry0, reset, d_out.contiguous(), ctx.scratch)
            else:
                g = pol.critic_backward(obs, carry0, reset, d_out.contiguous(), ctx.scratch)
            ctx.scratch = None
            return g, None, None, None, None, None

    return _Net


class TrainablePolicy:
    """A GruPolicy handle with its parameters as one flat torch.nn.Parameter (natural layout of
    include/zbot_policy.h, on the handle's device). log_prob / value are differentiable with
    respect to `param` only: observations, actions, carry0 and reset are data (their gradient is
    None), carry0 is not modified, and reset cuts the gradient through time where it zeroes the
    carry. The actor's trailing 20 mean offsets are constants: their gradient is exactly 0."""

    def __init__(self, policy: GruPolicy):
        import torch  # noqa: PLC0415

        self.torch = torch
        self.policy = policy
        self.param = torch.nn.Parameter(policy.params_tensor())
        self._pushed = self.param._version  # version of `param` the handle holds
        # JOINT_BIASES (train.py:963) are not trained: an optimizer's weight decay must not move them
        self._const = self.param.detach()[-JOINTS:].clone() if policy.kind == ACTOR else None
        self._fn = _function()

    def parameters(self):
        return [self.param]

    def sync(self) -> None:
        """Push `param` to the handle if it changed since the last push."""
        if self._pushed != self.param._version:
            if self._const is not None:
                with self.torch.no_grad():
                    self.param[-JOINTS:] = self._const
            self.policy.set_params(self.param.detach())
            self._pushed = self.param._version

    def log_prob(self, obs, actions, carry0, reset=None):
        """[T, n, 20] per-joint log-probs of `actions` (actor): the bits of actor.actor(mode=EVAL)."""
        if self.policy.kind != ACTOR:
            raise ZbError("log_prob() on a critic")
        self.sync()
        return self._fn.apply(self.param, self, obs, actions, carry0, reset)

    def value(self, obs, carry0, reset=None):
        """[T, n] values (critic): the bits of critic.critic."""
        if self.policy.kind == ACTOR:
            raise ZbError("value() on an actor")
        self.sync()
        return self._fn.apply(self.param, self, obs, None, carry0, reset)


def ppo_loss(log_prob, old_log_prob, advantages, values, old_values, value_targets,
             clip_param: float = DEFAULT_CLIP_PARAM, value_loss_coef: float = DEFAULT_VALUE_LOSS_COEF,
             use_clipped_value_loss: bool = DEFAULT_USE_CLIPPED_VALUE_LOSS,
             log_clip_value: float = DEFAULT_LOG_CLIP_VALUE):
    """ksim's PPO loss [U] in plain torch: the clipped surrogate on the per-joint log-probs summed
    over joints, plus value_loss_coef x the (clipped) value loss; means over [T, n].

    log_prob / old_log_prob [T, n, 20]; advantages, values, old_values, value_targets [T, n].
    The entropy bonus is out of scope: a mixture of Gaussians has no closed-form entropy (ksim's
    default entropy_coef only matters with a distribution that provides one)."""
    import torch  # noqa: PLC0415

    log_ratio = (log_prob.sum(-1) - old_log_prob.sum(-1)).clamp(-log_clip_value, log_clip_value)
    ratio = log_ratio.exp()
    surrogate = torch.minimum(ratio * advantages, ratio.clamp(1.0 - clip_param, 1.0 + clip_param) * advantages)
    policy_loss = -surrogate.mean()
    if use_clipped_value_loss:
        clipped = old_values + (values - old_values).clamp(-clip_param, clip_param)
        value_loss = 0.5 * torch.maximum((values - value_targets) ** 2, (clipped - value_targets) ** 2).mean()
    else:
        value_loss = 0.5 * ((values - value_targets) ** 2).mean()
    return policy_loss + value_loss_coef * value_loss


class _ShuffledMinibatches:
    """The minibatches of a learner with a shuffle seed: minibatch k of pass `epoch` is positions
    [k batch, (k + 1) batch) of ppo.minibatch_perm(n, seed, epoch), cut by one ppo.gather_minibatch
    launch (every array of the minibatch, both carries and the reset rows) into buffers kept per
    minibatch shape, so a steady-state step allocates nothing for them."""

    KEYS = (("obs_a", "obs_actor"), ("acts", "actions"), ("obs_c", "obs_critic"), ("old_lp", "log_prob"),
            ("old_v", "value"))

    def __init__(self):
        self._buf = {}

    def cut(self, torch, rollout, ppo_inputs, actor_carry0, critic_carry0, reset, T, n, lo, count, seed, epoch) -> dict:
        from . import ppo  # noqa: PLC0415

        src = {k: rollout[name] for k, name in self.KEYS}
        src["adv"], src["vt"] = ppo_inputs.advantages_t, ppo_inputs.value_targets_t
        dev = src["acts"].device
        key = (T, count, dev) + tuple((tuple(x.shape[2:]), x.dtype) for x in src.values())
        key += (tuple(actor_carry0.shape[1:]), tuple(critic_carry0.shape[1:]))  # [depth, 128] of each network
        b = self._buf.get(key)
        if b is None:
            b = {k: torch.empty((T, count) + tuple(x.shape[2:]), dtype=x.dtype, device=dev) for k, x in src.items()}
            b["rs"] = torch.empty(T, count, dtype=torch.uint8, device=dev)
            b["ca"], b["cc"] = torch.empty_like(actor_carry0[:count]), torch.empty_like(critic_carry0[:count])
            self._buf[key] = b
        items = [(x, b[k]) for k, x in src.items()]
        items += [(actor_carry0[None], b["ca"][None]), (critic_carry0[None], b["cc"][None])]
        if reset is not None:
            items.append((reset, b["rs"]))  # uint8: the learners convert once per update()
        else:  # row 0: no reset; row t: done[t - 1]
            items.append((None, b["rs"][:1]))
            if T > 1:
                items.append((rollout["done"], b["rs"][1:]))
        ppo.gather_minibatch(items, n, lo, count, shuffle_seed=seed, epoch=epoch)
        return b

    def cut_chunks(self, torch, rollout, ppo_inputs, reset, T, n, lo, count, seed, epoch, seq_len) -> dict:
        """The same minibatch as C = T / seq_len sequences of L = seq_len steps per env (truncated
        BPTT), by one ppo.gather_minibatch(seq_len=) launch: every [T, n] array as
        [L, C count], column c count + j chunk c of env p(lo + j); "ca" / "cc" [C count, depth, 128]
        the carries the rollout stored at the chunk starts; "rs" from `reset` [T, n] uint8, whose row
        c L lands in row 0 of chunk c. seed None: env order."""
        from . import ppo  # noqa: PLC0415

        L, C = seq_len, T // seq_len
        src = {k: rollout[name] for k, name in self.KEYS}
        src["adv"], src["vt"] = ppo_inputs.advantages_t, ppo_inputs.value_targets_t
        src["rs"] = reset
        ca, cc = rollout["actor_carry_chunks"], rollout["critic_carry_chunks"]
        dev = src["acts"].device
        key = ("chunks", L, C, count, dev) + tuple((tuple(x.shape[2:]), x.dtype) for x in src.values())
        key += (tuple(ca.shape[2:]), tuple(cc.shape[2:]))
        b = self._buf.get(key)
        if b is None:
            b = {k: torch.empty((L, C * count) + tuple(x.shape[2:]), dtype=x.dtype, device=dev) for k, x in src.items()}
            b["ca"] = torch.empty((C * count,) + tuple(ca.shape[2:]), dtype=ca.dtype, device=dev)
            b["cc"] = torch.empty((C * count,) + tuple(cc.shape[2:]), dtype=cc.dtype, device=dev)
            self._buf[key] = b
        items = [(x, b[k], True) for k, x in src.items()]  # the time items, cut in chunks
        items += [(ca, b["ca"].view((C, count) + tuple(ca.shape[2:]))), (cc, b["cc"].view((C, count) + tuple(cc.shape[2:])))]
        ppo.gather_minibatch(items, n, lo, count, shuffle_seed=seed, epoch=epoch, seq_len=L)
        return b


def _chunk_count(rollout, T: int, n: int, seq_len, actor: GruPolicy, critic: GruPolicy):
    """update(seq_len=)'s checks. None: the whole-sequence path (seq_len None or T). Else C = T / seq_len,
    after checking that the rollout carries both networks' chunk carries [C, n, depth, 128]
    (PolicyRollout.run(carry_every=seq_len) with the in-loop critic)."""
    if seq_len is None:
        return None
    if int(seq_len) != seq_len or seq_len < 1 or T % int(seq_len):
        raise ZbError(f"seq_len={seq_len!r} must be an integer >= 1 that divides the rollout's T = {T}")
    if int(seq_len) == T:
        return None
    C = T // int(seq_len)
    for name, h in (("actor_carry_chunks", actor), ("critic_carry_chunks", critic)):
        x = rollout.get(name)
        if x is None:
            raise ZbError(f"seq_len={seq_len} needs rollout[{name!r}]: run the rollout with carry_every={seq_len}"
                          + (" and the in-loop critic" if h.kind != ACTOR else ""))
        if tuple(x.shape) != (C, n, h.shape.depth, 128) or not x.is_contiguous():
            raise ZbError(f"rollout[{name!r}] must be a contiguous [C = T / seq_len = {C}, n = {n}, depth = "
                          f"{h.shape.depth}, 128] tensor, got {list(x.shape)}")
    return C


def _reset_rows(torch, rollout, reset, T, n):
    """update()'s `reset` as [T, n] uint8: the given rows, or row 0 zeros and row t done[t - 1]."""
    if reset is None:
        reset = torch.zeros(T, n, dtype=torch.uint8, device=rollout["actions"].device)
        reset[1:] = rollout["done"][:T - 1]
    elif reset.dtype != torch.uint8:
        reset = reset.to(torch.uint8)
    return reset


class PpoLearner:
    """num_passes x env-axis minibatches of AdamW steps behind a global-norm clip
    (train.py:1314-1324, 1771-1773). shuffle_seed=None: contiguous env slices in env order on every
    pass; a seed: each pass's minibatches follow a keyed permutation of the envs."""

    def __init__(self, learning_rate: float = DEFAULT_LEARNING_RATE, max_grad_norm: float = DEFAULT_MAX_GRAD_NORM,
                 weight_decay: float = DEFAULT_WEIGHT_DECAY, shuffle_seed: int | None = None):
        import torch  # noqa: PLC0415

        self.torch = torch
        self.learning_rate, self.max_grad_norm, self.weight_decay = learning_rate, max_grad_norm, weight_decay
        self.actor = self.critic = self.opt = None
        # None: contiguous env slices in env order. A seed: pass `epoch`'s minibatches follow
        # ppo.minibatch_perm(n, shuffle_seed, epoch), the same law as HipPpoLearner's
        self.shuffle_seed = shuffle_seed
        self.epoch = 0                   # passes taken
        self._mb = _ShuffledMinibatches()

    def update(self, rollout: dict, ppo_inputs, actor: TrainablePolicy, critic: TrainablePolicy, actor_carry0,
               critic_carry0, reset=None, num_passes: int = DEFAULT_NUM_PASSES, batch_size: int = DEFAULT_BATCH_SIZE,
               seq_len: int | None = None, **loss_kw) -> list:
        """One PPO update of `actor` and `critic` on a finished rollout (the optimizer state is kept
        between updates of the same pair).

        rollout: PolicyRollout.run(T, record_critic=True, critic=...)'s dict (obs_actor, actions,
        log_prob, obs_critic, value). ppo_inputs: zbot_amd.ppo.compute_ppo_inputs' result
        (advantages_t, value_targets_t). actor_carry0 / critic_carry0 [n, depth, 128]: the carries as
        they were before the run. reset [T, n]: the rows the run reset its carries with (row 0:
        the previous run's last done flags or None -> zeros; row t: done[t - 1]).
        Minibatches are contiguous env slices of `batch_size` in env order, or with a shuffle_seed
        the same positions of the pass's keyed permutation (ksim shuffles them with its own RNG
        [U]). Returns the losses, one per optimizer step.

        seq_len = L < T (a divisor of T): truncated BPTT with stored carries. The
        same envs per minibatch, each as its T / L chunks of L steps; the networks run on
        [L, (T / L) b] from rollout["actor_carry_chunks"] / ["critic_carry_chunks"]
        (PolicyRollout.run(carry_every=L)), which are data: no gradient crosses a chunk start, and
        actor_carry0 / critic_carry0 are not read. seq_len None or T: the whole sequences, as ever."""
        torch = self.torch
        if self.opt is None or actor is not self.actor or critic is not self.critic:
            self.actor, self.critic = actor, critic
            # optax.adamw's eps is 1e-8 like torch's; its weight decay is decoupled like torch's AdamW
            self.opt = torch.optim.AdamW([actor.param, critic.param], lr=self.learning_rate,
                                         weight_decay=self.weight_decay)
        T = rollout["actions"].shape[0]
        n = rollout["actions"].shape[1]
        if _chunk_count(rollout, T, n, seq_len, actor.policy, critic.policy) is not None:
            return self._update_gathered(rollout, ppo_inputs, actor_carry0, critic_carry0, reset, T, n, num_passes,
                                         batch_size, loss_kw, seq_len=int(seq_len))
        if self.shuffle_seed is not None:
            return self._update_gathered(rollout, ppo_inputs, actor_carry0, critic_carry0, reset, T, n, num_passes,
                                         batch_size, loss_kw)
        if reset is None:
            reset = torch.zeros(T, n, dtype=torch.uint8, device=rollout["actions"].device)
            reset[1:] = rollout["done"][:T - 1]
        losses = []
        for _ in range(num_passes):
            for lo in range(0, n, batch_size):
                hi = min(n, lo + batch_size)

                def cut(x):
                    return x[:T, lo:hi].contiguous()

                lp = self.actor.log_prob(cut(rollout["obs_actor"]), cut(rollout["actions"]),
                                         actor_carry0[lo:hi].contiguous(), cut(reset))
                v = self.critic.value(cut(rollout["obs_critic"]), critic_carry0[lo:hi].contiguous(), cut(reset))
                loss = ppo_loss(lp, cut(rollout["log_prob"]), cut(ppo_inputs.advantages_t), v, cut(rollout["value"]),
                                cut(ppo_inputs.value_targets_t), **loss_kw)
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                torch.nn.utils.clip_grad_norm_([self.actor.param, self.critic.param], self.max_grad_norm)
                self.opt.step()
                losses.append(loss.detach())
        self.epoch += num_passes
        # the handles serve the next rollout with the updated weights
        self.actor.sync()
        self.critic.sync()
        return losses

    def _update_gathered(self, rollout, ppo_inputs, actor_carry0, critic_carry0, reset, T, n, num_passes, batch_size,
                         loss_kw, seq_len=None) -> list:
        """update() on minibatches cut by the gather, the same steps on its buffers: with a shuffle seed
        the positions of the pass's keyed permutation, without one (seq_len alone) env order; with
        seq_len the buffers hold the minibatch in chunks. The pass count advances either way, as in
        update()'s env-slice path."""
        torch = self.torch
        if seq_len is not None:
            reset = _reset_rows(torch, rollout, reset, T, n)  # the chunked gather cuts given rows
        elif reset is not None and reset.dtype != torch.uint8:
            reset = reset.to(torch.uint8)  # reset None: the gather builds the rows itself
        losses = []
        for _ in range(num_passes):
            for lo in range(0, n, batch_size):
                count = min(n, lo + batch_size) - lo
                if seq_len is not None:
                    b = self._mb.cut_chunks(torch, rollout, ppo_inputs, reset, T, n, lo, count, self.shuffle_seed,
                                            self.epoch, seq_len)
                else:
                    b = self._mb.cut(torch, rollout, ppo_inputs, actor_carry0, critic_carry0, reset, T, n, lo, count,
                                     self.shuffle_seed, self.epoch)
                lp = self.actor.log_prob(b["obs_a"], b["acts"], b["ca"], b["rs"])
                v = self.critic.value(b["obs_c"], b["cc"], b["rs"])
                loss = ppo_loss(lp, b["old_lp"], b["adv"], v, b["old_v"], b["vt"], **loss_kw)
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                torch.nn.utils.clip_grad_norm_([self.actor.param, self.critic.param], self.max_grad_norm)
                self.opt.step()
                losses.append(loss.detach())
            self.epoch += 1
        self.actor.sync()
        self.critic.sync()
        return losses


class HipPpoLearner:
    """PpoLearner with every step in libzbot_hip.so (include/zbot_ppo.h "Learner"): per minibatch
    the training forwards, zb_ppo_loss, the backward passes, two zb_grad_sqnorm, two zb_adamw_step
    behind optax's global-norm clip over the joint norm, and zb_policy_set_params. No autograd
    graph and no host synchronisation inside update(); every sum runs over a fixed fp64 tree, so an
    update is bit-reproducible. Same constructor arguments and update() signature as PpoLearner;
    `actor` / `critic` are GruPolicy handles or TrainablePolicy wrappers (whose `param` is brought
    up to date at the end of update()).

    The learner owns, per network, the flat parameters and AdamW's m and v (float32 device tensors,
    natural layout), the step count and the pass count `epoch`; state_dict() / load_state_dict()
    carry them. shuffle_seed: as PpoLearner's (the same permutation, so the two stay comparable).

    group: a torch.distributed process group of W ranks that train one model on W shards of the envs
    (DESIGN.md §4p); None, or a group of one rank: this process alone, no collective. With W > 1
    every rank calls update() with its own rollout of the same shape and the global `batch_size`
    (a multiple of W): minibatch k is positions [k b, (k + 1) b), b = batch_size / W, of each rank's
    own env order (with a seed: the rank's own permutation, keyed by rank_seed()), the loss means run
    over the global rows, and per step and network the ranks' gradients are all-gathered
    (dist.all_gather_rows) and summed in rank order by ppo.grad_combine, which also returns the sum's
    squared norm. Gradient, norms and so params, m and v are the same bits on every rank without a
    broadcast; the ranks must start from the same weights. The returned sums are the global ones."""

    def __init__(self, learning_rate: float = DEFAULT_LEARNING_RATE, max_grad_norm: float = DEFAULT_MAX_GRAD_NORM,
                 weight_decay: float = DEFAULT_WEIGHT_DECAY, shuffle_seed: int | None = None, group=None):
        import torch  # noqa: PLC0415

        self.torch = torch
        self.learning_rate, self.max_grad_norm, self.weight_decay = learning_rate, max_grad_norm, weight_decay
        self.shuffle_seed = shuffle_seed  # None: env slices in env order; a seed: PpoLearner's keyed permutation
        self.group, self.world, self.rank = group, 1, 0
        if group is not None:
            import torch.distributed as dist  # noqa: PLC0415

            self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        if self.world == 1:
            self.group = None  # one rank: today's path, no collective
        self._agreed = None              # the update shape the ranks last agreed on
        self._mb = _ShuffledMinibatches()
        self.actor = self.critic = None  # the GruPolicy handles the state below belongs to
        self.step = 0                    # optimizer steps taken
        self.epoch = 0                   # passes taken: the permutation's second key
        self.state = None                # {"actor": {"params", "m", "v"}, "critic": {...}}
        self._loaded = False             # state came from load_state_dict: the next update pushes it to its handles
        self._buf = {}

    @staticmethod
    def _handle(p) -> GruPolicy:
        return p.policy if isinstance(p, TrainablePolicy) else p

    def rank_seed(self) -> int | None:
        """The seed of this rank's minibatch permutation: (shuffle_seed + 0x9E3779B97F4A7C15 rank)
        mod 2^64. Rank 0's (and a single process's) is shuffle_seed itself; ranks do not shuffle alike."""
        if self.shuffle_seed is None or self.rank == 0:
            return self.shuffle_seed
        return (int(self.shuffle_seed) + RANK_SEED_STRIDE * self.rank) % (1 << 64)

    def check_ranks(self, n_local: int, T: int, batch_size: int, num_passes: int, seq_len: int | None = None) -> None:
        """With several ranks: raise ZbError unless batch_size is a multiple of the world size and all
        ranks agree on (n_local, T, batch_size, num_passes, seq_len, shuffle_seed, learning_rate) - one
        small all_gather, no GPU work over gloo. update() runs it once per such shape. seq_len None
        counts as T: the same path."""
        key = (int(n_local), int(T), int(batch_size), int(num_passes), int(T if seq_len is None else seq_len))
        if self.world == 1 or self._agreed == key:
            return
        from .dist import agree  # noqa: PLC0415

        seed = -1 if self.shuffle_seed is None else int(self.shuffle_seed) % (1 << 64)
        lr = struct.unpack("<q", struct.pack("<d", float(self.learning_rate)))[0]
        agree(dict(n_local=key[0], T=key[1], batch_size=key[2], num_passes=key[3], seq_len=key[4],
                   shuffle=int(seed >= 0),
                   shuffle_seed_low=seed & 0xFFFFFFFF, shuffle_seed_high=(seed >> 32) & 0xFFFFFFFF if seed >= 0 else 0,
                   learning_rate_bits=lr), f"HipPpoLearner over {self.world} ranks", self.group)
        if key[2] % self.world:
            raise ZbError(f"batch_size {key[2]} is the global one: it must be a multiple of the {self.world} ranks")
        self._agreed = key

    def _bind(self, actor: GruPolicy, critic: GruPolicy) -> None:
        torch = self.torch
        if actor.kind != ACTOR or critic.kind == ACTOR:
            raise ZbError("HipPpoLearner.update(actor, critic): an actor and a critic handle, in this order")
        if self._loaded:
            for net, h in (("actor", actor), ("critic", critic)):
                st = self.state[net]
                for k in ("params", "m", "v"):
                    st[k] = st[k].to(device=h.device, dtype=torch.float32).contiguous()
                    if st[k].numel() != h.params_tensor().numel():
                        raise ZbError(f"loaded {net} {k}: {st[k].numel()} elements for this handle")
                h.set_params(st["params"])
            self._loaded = False
        elif self.state is None or actor is not self.actor or critic is not self.critic:
            self.state, self.step, self.epoch = {}, 0, 0
            for net, h in (("actor", actor), ("critic", critic)):
                p = h.params_tensor()
                self.state[net] = dict(params=p, m=torch.zeros_like(p), v=torch.zeros_like(p))
        self.actor, self.critic = actor, critic
        dev = actor.device
        if self._buf.get("dev") != dev:
            from . import ppo  # noqa: PLC0415

            L = ppo.load_library()
            self._buf = dict(dev=dev, sq=torch.zeros(2, dtype=torch.float64, device=dev))
            for net in ("actor", "critic"):
                cnt = self.state[net]["params"].numel()
                self._buf[net] = dict(grad=torch.empty(cnt, dtype=torch.float32, device=dev),
                                      part=torch.empty(max(int(L.zb_sqnorm_partials_words(cnt)), 1),
                                                       dtype=torch.float64, device=dev))
                if self.world > 1:  # the all-gather's destination: every rank's gradient, rank order
                    self._buf[net]["rows"] = torch.empty(self.world, cnt, dtype=torch.float32, device=dev)
            if self.world > 1:
                self._buf["sums"] = torch.empty(self.world, 4, dtype=torch.float64, device=dev)

    def update(self, rollout: dict, ppo_inputs, actor, critic, actor_carry0, critic_carry0, reset=None,
               num_passes: int = DEFAULT_NUM_PASSES, batch_size: int = DEFAULT_BATCH_SIZE,
               seq_len: int | None = None, **loss_kw) -> list:
        """One PPO update, as PpoLearner.update (same arguments, same minibatches in the same order,
        shuffled by the same permutation when both have the same shuffle_seed).
        Returns one float64 device tensor [6] per optimizer step: zb_ppo_loss's four sums (sum S,
        sum Vt, sum clipped, sum kl), then the row count and value_loss_coef the step used; loss(sums)
        forms the scalar loss from it. Nothing is synchronized.
        seq_len: as PpoLearner.update's (truncated BPTT on the rollout's stored chunk carries; the
        loss still runs over the minibatch's T b rows, so the row count in the sums is unchanged)."""
        from . import ppo  # noqa: PLC0415

        torch = self.torch
        wrappers = [p for p in (actor, critic) if isinstance(p, TrainablePolicy)]
        self._bind(self._handle(actor), self._handle(critic))
        act, cri, sa, sc, ba, bc, sq = (self.actor, self.critic, self.state["actor"], self.state["critic"],
                                        self._buf["actor"], self._buf["critic"], self._buf["sq"])
        T = rollout["actions"].shape[0]
        n = rollout["actions"].shape[1]
        W = self.world
        # how a minibatch is cut: in chunks by the chunked gather, by the whole-sequence gather, or as env slices
        if _chunk_count(rollout, T, n, seq_len, act, cri) is not None:
            mode = "chunks"
        else:
            mode = "slices" if self.shuffle_seed is None else "gather"
        if W > 1:
            from .dist import all_gather_rows  # noqa: PLC0415

            self.check_ranks(n, T, batch_size, num_passes, seq_len)
            batch_size //= W  # this rank's share of every minibatch
        seed = self.rank_seed()
        if mode == "chunks" or (mode == "slices" and reset is None):
            reset = _reset_rows(torch, rollout, reset, T, n)
        elif mode == "gather" and reset is not None and reset.dtype != torch.uint8:
            reset = reset.to(torch.uint8)  # reset None: the gather builds the rows itself
        coef = float(loss_kw.get("value_loss_coef", DEFAULT_VALUE_LOSS_COEF))
        out = []
        for _ in range(num_passes):
            for lo in range(0, n, batch_size):
                hi = min(n, lo + batch_size)

                def cut(x):
                    return x[:T, lo:hi].contiguous()

                if mode != "slices":
                    if mode == "chunks":
                        mb = self._mb.cut_chunks(torch, rollout, ppo_inputs, reset, T, n, lo, hi - lo, seed, self.epoch,
                                                 int(seq_len))
                    else:
                        mb = self._mb.cut(torch, rollout, ppo_inputs, actor_carry0, critic_carry0, reset, T, n, lo,
                                          hi - lo, seed, self.epoch)
                    obs_a, acts, obs_c, rs, ca, cc = mb["obs_a"], mb["acts"], mb["obs_c"], mb["rs"], mb["ca"], mb["cc"]
                    old_lp, adv, old_v, vt = mb["old_lp"], mb["adv"], mb["old_v"], mb["vt"]
                else:
                    obs_a, acts, obs_c, rs = cut(rollout["obs_actor"]), cut(rollout["actions"]), cut(rollout["obs_critic"]), cut(reset)
                    ca, cc = actor_carry0[lo:hi].contiguous(), critic_carry0[lo:hi].contiguous()
                lp, scr_a = act.actor_train(obs_a, acts, ca, rs)
                v, scr_c = cri.critic_train(obs_c, cc, rs)
                sums = torch.empty(6, dtype=torch.float64, device=lp.device)
                total = T * (hi - lo) * W  # the rows of this minibatch on all ranks
                sums[4], sums[5] = float(total), coef
                if mode == "slices":
                    old_lp, adv, old_v, vt = (cut(rollout["log_prob"]), cut(ppo_inputs.advantages_t),
                                              cut(rollout["value"]), cut(ppo_inputs.value_targets_t))
                d_lp, d_v, _ = ppo.ppo_loss_grad(lp, old_lp, adv, v, old_v, vt, sums=sums,
                                                 **(loss_kw if W == 1 else dict(loss_kw, total=total)))
                # the critic first: its saved activations were written last, so more of them are still in
                # the cache (autograd runs PpoLearner's backward passes in this order too)
                cri.critic_backward(obs_c, cc, rs, d_v, scr_c, grad=bc["grad"])
                act.actor_backward(obs_a, acts, ca, rs, d_lp, scr_a, grad=ba["grad"])
                if W == 1:
                    ppo.grad_sqnorm(ba["grad"], out=sq[0:1], partials=ba["part"])
                    ppo.grad_sqnorm(bc["grad"], out=sq[1:2], partials=bc["part"])
                else:  # the sum over ranks in rank order, and its squared norm, the same bits on every rank
                    for k, b in enumerate((ba, bc)):
                        all_gather_rows(b["grad"], b["rows"], self.group)
                        ppo.grad_combine(b["rows"], out=b["grad"], sq_out=sq[k:k + 1], partials=b["part"])
                    g = all_gather_rows(sums[:4], self._buf["sums"], self.group)
                    sums[:4].copy_(g[0])  # then + rank 1, + rank 2, ...: rank order, on the device
                    for r in range(1, W):
                        sums[:4] += g[r]
                self.step += 1
                for st, b, tail in ((sa, ba, JOINTS), (sc, bc, 0)):
                    ppo.adamw_step(st["params"], b["grad"], st["m"], st["v"], sq, self.step, self.learning_rate,
                                   max_grad_norm=self.max_grad_norm, weight_decay=self.weight_decay, frozen_tail=tail)
                act.set_params(sa["params"])
                cri.set_params(sc["params"])
                out.append(sums)
            self.epoch += 1
        for w in wrappers:  # a TrainablePolicy's own copy follows its handle
            with torch.no_grad():
                w.param.copy_(self.state["actor" if w.policy.kind == ACTOR else "critic"]["params"])
            w._pushed = w.param._version
        return out

    @staticmethod
    def loss(sums):
        """The scalar PPO loss of one step from update()'s sums (a float64 device scalar; no sync):
        -sum S / total + value_loss_coef * 0.5 * sum Vt / total, i.e. learner.ppo_loss."""
        return -sums[0] / sums[4] + sums[5] * 0.5 * sums[1] / sums[4]

    def state_dict(self) -> dict:
        """{"step", "epoch", "world", "actor": {"params", "m", "v"}, "critic": {...}} (copies)."""
        if self.state is None:
            raise ZbError("HipPpoLearner.state_dict(): no state yet (no update() and no load_state_dict())")
        return dict(step=self.step, epoch=self.epoch, world=self.world,
                    **{net: {k: t.clone() for k, t in self.state[net].items()} for net in ("actor", "critic")})

    def load_state_dict(self, sd: dict) -> None:
        """Restore state_dict()'s result. The next update() pushes the restored parameters to the
        handles it is given and continues the step count. A state saved at another world size is
        refused: its minibatches were cut differently."""
        if int(sd.get("world", 1)) != self.world:  # a state dict from before the multi-rank update has none
            raise ZbError(f"the state was saved by a learner over {sd.get('world', 1)} rank(s); this one runs over "
                          f"{self.world}")
        self.state = {net: {k: sd[net][k].clone() for k in ("params", "m", "v")} for net in ("actor", "critic")}
        self.step = int(sd["step"])
        self.epoch = int(sd.get("epoch", 0))  # a state dict from before the shuffle has none
        self.actor = self.critic = None
        self._loaded = True
