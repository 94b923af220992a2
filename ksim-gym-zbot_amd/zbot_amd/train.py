"""The training iteration of the reference's ZbotWalkingTask.launch (train.py:1766-1788), joined
from the library's blocks: rollout with the GRU actor and the in-loop critic, PPO inputs, the PPO
update in HIP, the episode-length curriculum.

    tr = Trainer(engine, actor, critic, rollout_steps=200, num_passes=4, batch_size=128,
                 seed=0, shuffle=True, curriculum=EpisodeLengthCurriculum(), ctrl_dt=0.02, group=None,
                 command_config=None, telemetry=False, seq_len=None, **learner_kw)
    m = tr.step()            # one iteration; returns metrics (telemetry=True: with m["telemetry"])
    v = tr.validate()        # a rollout without an update: its telemetry; the Trainer stays where it was
    sd = tr.state_dict(); tr.load_state_dict(sd)

Several GPUs: one Trainer per rank over its shard of the envs (engine.env_offset = rank x engine.n)
and `group` = the ranks' torch.distributed process group. `batch_size` is then the global one; the
advantage moments, the gradients (summed in rank order by ppo.grad_combine), the loss sums, the
episode length and so the curriculum level are global, and every rank holds the same weights bit for
bit. The state dict stays per rank.

`engine` is a HipEngine or an EnvGroups, `actor` / `critic` are GruPolicy handles; the remaining
keyword arguments go to HipPpoLearner (learning_rate, max_grad_norm, weight_decay). Saving to a file
is the caller's torch.save(tr.state_dict(), path); file formats, logging, the command line and the
viewer are out of scope.

One step(), in order:
  1. open the statistics window: engine.get_stats(clear=True);
  2. snapshot both carries (the learner's carry0 arguments: the carries before the run);
  3. PolicyRollout.run(T, record_critic=True, critic=..., critic_carry=...) at the current level;
  4. ppo.compute_ppo_inputs(value, reward, done, success, bootstrap=value_next);
  5. HipPpoLearner.update(...), `reset` row 0 = the previous iteration's last done flags (none in
     the first), row t = done[t - 1];
  6. curriculum.rollout_episode_length and curriculum.update: the iteration's one host
     synchronisation is that float;
  7. the new level goes to the next rollout.
With seq_len = L < rollout_steps (a divisor of it) the update is truncated BPTT: 3.
runs with carry_every=L, which stores both carries at every chunk start, and 5. with seq_len=L, which
trains on each env's T / L chunks as separate sequences from those stored carries; seq_len None or
rollout_steps is the whole-sequence path, the same launches and bits as without the argument.
With telemetry=True the rollout of 3. also records the reward and command terms, and between 4. and
5. one ppo.rollout_summary on the current stream reduces them, the rewards, the episode ends, the
log-probs, the values and the value targets to 32 sums; telemetry=False issues none
of this.
"""

from __future__ import annotations

import ctypes
import dataclasses

from . import cstructs as cs
from . import ppo
from .curriculum import CurriculumState, EpisodeLengthCurriculum, rollout_episode_length
from .engine import ZbError
from .metrics import command_term_means, rollout_telemetry
from .learner import DEFAULT_BATCH_SIZE, DEFAULT_NUM_PASSES, HipPpoLearner
from .policy import ACTOR, MODE, SAMPLE, GruPolicy, PolicyRollout, PolicyShape

DEFAULT_ROLLOUT_STEPS = 200  # rollout_length_seconds 4.0 / ctrl_dt 0.02 (train.py:1775, 1783)


class Trainer:
    """One training process on one GPU (one rank of `group`, when given): owns the PolicyRollout, the critic's carry, the
    HipPpoLearner and the curriculum state. The seed keys the actor's action samples and, with
    shuffle, the minibatch permutation (shuffle=False: env slices in env order). Everything runs
    on the current stream; two Trainers built from the same seeds, weights and engine seed produce
    the same bits, and so does one continued from state_dict() in a fresh process."""

    def __init__(self, engine, actor: GruPolicy, critic: GruPolicy, rollout_steps: int = DEFAULT_ROLLOUT_STEPS,
                 num_passes: int = DEFAULT_NUM_PASSES, batch_size: int = DEFAULT_BATCH_SIZE, seed: int = 0,
                 shuffle: bool = True, curriculum: EpisodeLengthCurriculum | None = None, ctrl_dt: float = 0.02,
                 group=None, command_config: cs.ZbCommandConfig | None = None, telemetry: bool = False,
                 seq_len: int | None = None, **learner_kw):
        """seq_len: train on chunks of seq_len steps from the carries the rollout stored at the chunk
        starts (truncated BPTT; must divide rollout_steps; None: whole sequences). validate() stores
        none. It is part of state_dict() when set, and the ranks must agree on it; seq_len == rollout_steps
        is None in every one of these respects.
        telemetry: step() also returns "telemetry", metrics.rollout_telemetry of the rollout's
        sums (every reward and command term, how episodes end, the entropy estimate, the explained
        variance, the episode statistics). On several ranks the 32 sums go through
        dist.reduce_fixed_order: every rank then reports the same bits, but they are a rank-order
        sum of per-rank trees, not the tree over all rows: not the bits a single rank over the same
        envs reports. The weights do not depend on it.
        command_config: a config.command_config(...): the engine samples velocity commands
        (include/zbot_command.h) and adds the tracking terms to the reward; step() then reports
        the per-term means. It is set on the engine here and is part of state_dict()."""
        if actor.kind != ACTOR or critic.kind == ACTOR:
            raise ZbError("Trainer(engine, actor, critic): an actor and a critic handle, in this order")
        if rollout_steps < 1 or num_passes < 1 or batch_size < 1:
            raise ZbError("rollout_steps, num_passes and batch_size must be >= 1")
        self.torch = actor.torch
        self.eng, self.actor, self.critic = engine, actor, critic
        self.T, self.num_passes, self.batch_size = int(rollout_steps), int(num_passes), int(batch_size)
        if seq_len is not None and (int(seq_len) != seq_len or seq_len < 1 or self.T % int(seq_len)):
            raise ZbError(f"seq_len={seq_len!r} must be an integer >= 1 that divides rollout_steps = {self.T}")
        # seq_len == rollout_steps is the whole-sequence path: kept as None, so that the ranks' agreement,
        # state_dict() and load_state_dict() see one spelling of it
        self.seq_len = None if seq_len is None or int(seq_len) == self.T else int(seq_len)
        self.seed, self.shuffle, self.ctrl_dt = int(seed), bool(shuffle), float(ctrl_dt)
        self.group, self.world, self.rank = group, 1, 0
        if group is not None:
            import torch.distributed as dist  # noqa: PLC0415

            from .dist import agree  # noqa: PLC0415

            self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
            if int(engine.env_offset) != self.rank * int(engine.n):
                raise ZbError(f"rank {self.rank} of {self.world} owns envs from {self.rank * int(engine.n)}: the engine "
                              f"was created with env_offset {engine.env_offset}")
            agree(dict(seed=self.seed % (1 << 63), shuffle=int(self.shuffle), rollout_steps=self.T,
                       num_passes=self.num_passes, batch_size=self.batch_size, envs_per_rank=int(engine.n),
                       seq_len=0 if self.seq_len is None else self.seq_len),
                  f"Trainer over {self.world} ranks", group)
        self.telemetry = bool(telemetry)
        self.command_config = command_config
        if command_config is not None:
            engine.set_command_config(command_config)  # before the rollout's first reset draws the commands
        self.curriculum = EpisodeLengthCurriculum() if curriculum is None else curriculum
        self.cur_state = self.curriculum.initial_state()
        self.rollout = PolicyRollout(engine, actor, seed=self.seed, curriculum=self.cur_state.level)
        self.critic_carry = critic.initial_carry(engine.n)
        self.learner = HipPpoLearner(shuffle_seed=self.seed if self.shuffle else None, group=group, **learner_kw)
        self.iteration = 0
        self.last_rollout = None  # the last step()'s rollout dict and PPO inputs, for inspection
        self.last_inputs = None
        self.timing = None        # {"rollout": (start, end), ...} torch.cuda.Event pairs: step() records them

    @property
    def level(self) -> float:
        return self.cur_state.level

    def _mark(self, name: str, end: bool) -> None:
        if self.timing is not None:
            self.timing[name][1 if end else 0].record()

    def step(self) -> dict:
        """One training iteration. Returns {"iteration", "level" (the level the rollout ran at),
        "episode_length" (seconds, a float), "reward" (mean per env-step, over all ranks), "loss", "clip_fraction",
        "approx_kl" ([optimizer steps] each), "sums" (HipPpoLearner.update's list), and with a command
        config "command_terms" (metrics.command_term_means of the rollout's last step), and with
        telemetry=True "telemetry" (metrics.rollout_telemetry: a dict of 0-d tensors)}; the tensors are
        on the device and nothing but the episode length is synchronised."""
        torch = self.torch
        ro, T = self.rollout, self.T
        self.eng.get_stats(clear=True)
        if ro.obs is None:
            ro.reset()
        carry0, ccarry0 = ro.carry.clone(), self.critic_carry.clone()
        prev_done = ro.done
        level = self.cur_state.level
        ro.curriculum = level
        self._mark("rollout", False)
        # only what is asked for is passed on: without telemetry and seq_len this is the call it always was
        extra_kw = dict(record_terms=True) if self.telemetry else {}
        if self.seq_len is not None:
            extra_kw["carry_every"] = self.seq_len
        out = ro.run(T, record_critic=True, critic=self.critic, critic_carry=self.critic_carry, **extra_kw)
        self._mark("rollout", True)
        self._mark("ppo_inputs", False)
        inputs = ppo.compute_ppo_inputs(out["value"], out["reward"], out["done"], out["success"],
                                        bootstrap=out["value_next"], group=self.group)
        self._mark("ppo_inputs", True)
        tsums = self._summary(out, inputs) if self.telemetry else None
        reset = None
        if prev_done is not None:
            reset = torch.cat([prev_done[None], out["done"][:T - 1]])
        self._mark("update", False)
        sums = self.learner.update(out, inputs, self.actor, self.critic, carry0, ccarry0, reset=reset,
                                   num_passes=self.num_passes, batch_size=self.batch_size, seq_len=self.seq_len)
        self._mark("update", True)
        stats = self.eng.get_stats()
        length = rollout_episode_length(stats, self.eng.get_state(), out["done"][T - 1], self.ctrl_dt,
                                        group=self.group)
        self.cur_state = self.curriculum.update(self.cur_state, length)
        self.iteration += 1
        self.last_rollout, self.last_inputs = out, inputs
        s = torch.stack(sums)
        reward = out["reward"].mean()
        if self.world > 1:  # the mean over every rank's env-steps: float64 sums, added in rank order
            from .dist import reduce_fixed_order  # noqa: PLC0415

            r = out["reward"]
            tot = reduce_fixed_order(torch.stack([r.double().sum(), torch.tensor(float(r.numel()), dtype=torch.float64,
                                                                               device=r.device)]), group=self.group)
            reward = tot[0] / tot[1]
        extra = {}
        if self.command_config is not None:
            # the rollout's last step, mean over this rank's envs (zbot_amd.metrics)
            extra["command_terms"] = command_term_means(self.eng.get_command_terms())
        if self.telemetry:
            extra["telemetry"] = self._telemetry(tsums, stats, level)
        return dict(iteration=self.iteration, level=level, episode_length=length, reward=reward, **extra,
                    loss=-s[:, 0] / s[:, 4] + s[:, 5] * 0.5 * s[:, 1] / s[:, 4], clip_fraction=s[:, 2] / s[:, 4],
                    approx_kl=s[:, 3] / s[:, 4], sums=sums)

    def _summary(self, out: dict, inputs):
        """ppo.rollout_summary of a recorded rollout and its PPO inputs, on the current stream."""
        return ppo.rollout_summary(out["reward"], out["done"], out["success"], reward_terms=out.get("reward_terms"),
                                   command_terms=out.get("command_terms"), log_prob=out["log_prob"],
                                   values=out["value"], value_targets=inputs.value_targets_t)

    def _telemetry(self, sums, stats, level: float) -> dict:
        """metrics.rollout_telemetry of this rank's sums and statistics window; over several ranks
        both are summed in rank order first (one collective), so every rank returns the same bits."""
        if self.world > 1:
            from .dist import reduce_fixed_order  # noqa: PLC0415

            tot = reduce_fixed_order(self.torch.cat([sums, stats.double().sum(0)]), group=self.group)
            sums, stats = tot[:cs.SUMMARY_WORDS], tot[cs.SUMMARY_WORDS:][None]
        return rollout_telemetry(sums, self.eng.cfg, level, command_config=self.command_config, stats=stats,
                                 ctrl_dt=self.ctrl_dt)

    def validate(self, steps: int | None = None, mode: str = "sample") -> dict:
        """ksim's validation rollout (valid_every_n_steps, train.py:1783): one rollout of `steps`
        control steps (default: rollout_steps) at the current level with no update and no
        curriculum step; returns its telemetry (metrics.rollout_telemetry; the values are the in-loop
        critic's, the value targets ppo.compute_ppo_inputs'). mode "sample" draws actions as training
        does (from the Trainer's seed and step count: the rollout the next step() would start with),
        "mode" takes the mixture's mode: a deterministic rollout, whose log-probs, and with them
        entropy_estimate, are those of the mode actions.

        The Trainer is left exactly where it was: the engine's state rows (which hold the velocity
        commands, the airtime words and the RNG counters) and randomisation rows, the rollout's
        obs, obs_c, done, actor carry and step count and the critic carry are copied before the run
        and put back after it. The statistics window is cleared before the run and read after it;
        step() clears it at its own start, so no iteration loses anything. Works on a HipEngine and
        on an EnvGroups. Over several ranks every rank calls it (the advantage moments and the
        telemetry sums are collectives)."""
        modes = {"sample": SAMPLE, "mode": MODE}
        if mode not in modes:
            raise ZbError(f"validate(mode=...): 'sample' or 'mode', got {mode!r}")
        T = self.T if steps is None else int(steps)
        if T < 1:
            raise ZbError("validate: steps must be >= 1")
        ro, eng = self.rollout, self.eng
        if ro.obs is None:
            ro.reset()
        c = lambda t: None if t is None else t.clone()  # noqa: E731
        state, rand = eng.get_state(), eng.get_rand()
        saved = (c(ro.obs), c(ro.obs_c), c(ro.done), ro.carry.clone(), int(ro.step_count), self.critic_carry.clone(),
                 ro.curriculum)
        level = self.cur_state.level
        ro.curriculum = level
        eng.get_stats(clear=True)
        out = ro.run(T, record_critic=True, critic=self.critic, critic_carry=self.critic_carry, record_terms=True,
                     mode=modes[mode])
        inputs = ppo.compute_ppo_inputs(out["value"], out["reward"], out["done"], out["success"],
                                        bootstrap=out["value_next"], group=self.group)
        tel = self._telemetry(self._summary(out, inputs), eng.get_stats(), level)
        eng.set_state(state)
        eng.set_rand(rand)
        ro.obs, ro.obs_c, ro.done = saved[0], saved[1], saved[2]
        ro.carry.copy_(saved[3])
        ro.step_count = saved[4]
        self.critic_carry.copy_(saved[5])
        ro.curriculum = saved[6]
        return tel

    def state_dict(self) -> dict:
        """Everything a fresh process needs to continue with the same bits (copies): the engine's
        state and randomisation rows, the rollout's current observations, done flags, actor carry
        and step count, the critic carry, both networks' weights, the learner's state (weights, m,
        v, step, epoch; None before the first step), the curriculum state, the iteration count and
        the seeds. The engine
        and the policy handles themselves are the caller's to create: the engine with the same
        model, config, env count and seed (checked on load), the handles from any weights."""
        ro = self.rollout
        if ro.obs is None:
            ro.reset()
        c = lambda t: None if t is None else t.clone()  # noqa: E731
        return dict(
            engine=dict(state=self.eng.get_state(), rand=self.eng.get_rand(), seed=int(self.eng.seed), n=int(self.eng.n)),
            rollout=dict(obs=c(ro.obs), obs_c=c(ro.obs_c), done=c(ro.done), carry=ro.carry.clone(),
                         step_count=int(ro.step_count)),
            critic_carry=self.critic_carry.clone(),
            params=dict(actor=self.actor.params_tensor(), critic=self.critic.params_tensor()),
            shapes=dict(actor=dataclasses.asdict(self.actor.shape), critic=dataclasses.asdict(self.critic.shape)),
            learner=None if self.learner.state is None else self.learner.state_dict(),
            curriculum=dict(level=float(self.cur_state.level), steps=int(self.cur_state.steps)),
            iteration=int(self.iteration), seed=self.seed, shuffle=self.shuffle, world=self.world, rank=self.rank,
            command_config=None if self.command_config is None else bytes(self.command_config),
            **({} if self.seq_len is None else dict(seq_len=self.seq_len)))

    def load_state_dict(self, sd: dict) -> None:
        """Restore state_dict()'s result into this Trainer's engine, handles and learner."""
        torch = self.torch
        dev = self.eng.device
        e = sd["engine"]
        if int(e["n"]) != self.eng.n or int(e["seed"]) != int(self.eng.seed):
            raise ZbError(f"the state is of {e['n']} envs with engine seed {e['seed']}; this engine has {self.eng.n}, "
                          f"seed {self.eng.seed}")
        if int(sd["seed"]) != self.seed or bool(sd["shuffle"]) != self.shuffle:
            raise ZbError(f"the state was trained with seed={sd['seed']}, shuffle={sd['shuffle']}")
        if sd.get("seq_len") != self.seq_len:
            raise ZbError(f"the state was trained with seq_len={sd.get('seq_len')}; this Trainer has seq_len={self.seq_len}")
        if int(sd.get("world", 1)) != self.world or int(sd.get("rank", 0)) != self.rank:
            raise ZbError(f"the state is rank {sd.get('rank', 0)}'s of {sd.get('world', 1)}; this Trainer is rank "
                          f"{self.rank} of {self.world}")
        # the networks' shapes (a state from before shapes existed is of the default one); the critic reads no mixtures
        default = dataclasses.asdict(PolicyShape())
        for net, h in (("actor", self.actor), ("critic", self.critic)):
            want = dict(sd.get("shapes", {}).get(net, default))
            have = dataclasses.asdict(h.shape)
            if net == "critic":
                want.pop("num_mixtures", None), have.pop("num_mixtures", None)
            if want != have:
                raise ZbError(f"the state's {net} has the shape {want}; this Trainer's {net} handle has {have}")
        cc = sd.get("command_config")
        if cc is not None and len(cc) != ctypes.sizeof(cs.ZbCommandConfig):
            raise ZbError(f"the state's command config has {len(cc)} bytes, ZbCommandConfig {ctypes.sizeof(cs.ZbCommandConfig)}")
        self.command_config = None if cc is None else cs.ZbCommandConfig.from_buffer_copy(cc)
        self.eng.set_command_config(self.command_config)
        self.eng.set_state(e["state"])  # the commands are words of the state rows
        self.eng.set_rand(e["rand"])
        ro, r = self.rollout, sd["rollout"]
        to = lambda t: None if t is None else t.to(dev).clone()  # noqa: E731
        ro.obs, ro.obs_c, ro.done = to(r["obs"]), to(r["obs_c"]), to(r["done"])
        ro.carry.copy_(r["carry"])
        ro.step_count = int(r["step_count"])
        self.critic_carry.copy_(sd["critic_carry"])
        self.learner = HipPpoLearner(learning_rate=self.learner.learning_rate, max_grad_norm=self.learner.max_grad_norm,
                                     weight_decay=self.learner.weight_decay,
                                     shuffle_seed=self.seed if self.shuffle else None, group=self.group)
        # the next rollout comes before the next update: the handles need the weights now
        self.actor.set_params(sd["params"]["actor"].to(dev, dtype=torch.float32))
        self.critic.set_params(sd["params"]["critic"].to(dev, dtype=torch.float32))
        if sd["learner"] is not None:
            self.learner.load_state_dict(sd["learner"])
        self.cur_state = CurriculumState(level=float(sd["curriculum"]["level"]), steps=int(sd["curriculum"]["steps"]))
        ro.curriculum = self.cur_state.level
        self.iteration = int(sd["iteration"])
        self.last_rollout = self.last_inputs = None
