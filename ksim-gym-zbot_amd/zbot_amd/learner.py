"""The learner's half of PPO: gradients through the GRU actor / critic, and the update.

Mirrors what ksim's PPOTask does with train.py's model after a rollout:
get_ppo_variables (train.py:1683-1729) scans both networks over the trajectory and is
differentiated through, the loss is ksim's PPO loss (un-vendored ksim/task/ppo.py [U]) and the
optimizer is ZbotWalkingTask.get_optimizer (train.py:1314-1324).

The hot path — the activation-saving forward and the backward pass through 5 GRU layers x T
steps — runs in libzbot_hip.so (include/zbot_policy.h "Training"); there is no PyTorch or CPU
fallback for it. The loss and the optimizer are ordinary torch:

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


class PpoLearner:
    """num_passes x env-axis minibatches of AdamW steps behind a global-norm clip
    (train.py:1314-1324, 1771-1773)."""

    def __init__(self, learning_rate: float = DEFAULT_LEARNING_RATE, max_grad_norm: float = DEFAULT_MAX_GRAD_NORM,
                 weight_decay: float = DEFAULT_WEIGHT_DECAY):
        import torch  # noqa: PLC0415

        self.torch = torch
        self.learning_rate, self.max_grad_norm, self.weight_decay = learning_rate, max_grad_norm, weight_decay
        self.actor = self.critic = self.opt = None

    def update(self, rollout: dict, ppo_inputs, actor: TrainablePolicy, critic: TrainablePolicy, actor_carry0,
               critic_carry0, reset=None, num_passes: int = DEFAULT_NUM_PASSES, batch_size: int = DEFAULT_BATCH_SIZE,
               **loss_kw) -> list:
        """One PPO update of `actor` and `critic` on a finished rollout (the optimizer state is kept
        between updates of the same pair).

        rollout: PolicyRollout.run(T, record_critic=True, critic=...)'s dict (obs_actor, actions,
        log_prob, obs_critic, value). ppo_inputs: zbot_amd.ppo.compute_ppo_inputs' result
        (advantages_t, value_targets_t). actor_carry0 / critic_carry0 [n, 5, 128]: the carries as
        they were before the run. reset [T, n]: the rows the run reset its carries with (row 0:
        the previous run's last done flags or None -> zeros; row t: done[t - 1]).
        Minibatches are contiguous env slices of `batch_size` in env order (ksim shuffles them
        with its own RNG [U]). Returns the losses, one per optimizer step."""
        torch = self.torch
        if self.opt is None or actor is not self.actor or critic is not self.critic:
            self.actor, self.critic = actor, critic
            # optax.adamw's eps is 1e-8 like torch's; its weight decay is decoupled like torch's AdamW
            self.opt = torch.optim.AdamW([actor.param, critic.param], lr=self.learning_rate,
                                         weight_decay=self.weight_decay)
        T = rollout["actions"].shape[0]
        n = rollout["actions"].shape[1]
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
        # the handles serve the next rollout with the updated weights
        self.actor.sync()
        self.critic.sync()
        return losses
