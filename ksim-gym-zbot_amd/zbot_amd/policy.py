"""GRU actor / critic of ZbotWalkingTask in the rollout loop.

Mirrors train.py's Model (Actor :885-967, Critic :970-1023, get_model
:1604-1614) and ZbotWalkingTask.run_actor / run_critic / sample_action
(:1616-1681, :1737-1763). The networks run in libzbot_hip.so on the f32
matrix cores (include/zbot_policy.h); there is no PyTorch or CPU fallback.
Training them (the activation-saving forward, the backward pass and a torch
autograd wrapper over both) is zbot_amd.learner.

    actor = GruPolicy(ACTOR, init_params(ACTOR, seed=0))
    carry = actor.initial_carry(n)                          # get_initial_model_carry
    actions, log_prob = actor.actor(obs_actor, carry, reset=done, log_prob=True)   # sample_action
    critic = GruPolicy(CRITIC, init_params(CRITIC, seed=1))
    values = critic.critic(obs_critic_t, critic.initial_carry(n), reset=resets_t)  # [T, n]
    (obs_critic_t[t] is the observation of the state acted in at step t; PolicyRollout records it)

The network shape (train.py's `depth` and `num_mixtures`, train.py:1065-1076) is a property of the
handle: `GruPolicy(ACTOR, init_params(ACTOR, 0, shape), shape=PolicyShape(depth=2, num_mixtures=3))`;
carries are then [n, depth, 128]. `actor_host` / `critic_host` are the CPU bit references at every
shape.

`PolicyRollout` is ksim's rollout loop with the actor in it: per control step
one actor launch then one zb_step launch, rows written straight into [T, n]
buffers on the GPU.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses

import numpy as np

from . import cstructs as cs
from .constants import JOINT_BIASES
from .engine import ZbError, _check, load_library

HIDDEN, DEPTH, MIXTURES, JOINTS = 128, 5, 5, 20
ACTOR_IN, CRITIC_IN, ACTOR_OUT = 50, 484, 300
ACTOR, CRITIC = 0, 1
SAMPLE, MODE, EVAL = 0, 1, 2
LAYOUT_BLOCK, LAYOUT_WAVE, LAYOUT_WAVE2, LAYOUT_WAVE4 = 0, 1, 2, 3  # include/zbot_policy.h ZB_POL_LAYOUT_*
# matrix-core FLOP per env per step (FMA = 2): the roofline unit bench.py reports
FLOP_ACTOR = 2 * (ACTOR_IN * HIDDEN + DEPTH * 6 * HIDDEN * HIDDEN + HIDDEN * ACTOR_OUT)
FLOP_CRITIC = 2 * (CRITIC_IN * HIDDEN + DEPTH * 6 * HIDDEN * HIDDEN + HIDDEN)


MAX_DEPTH, MAX_MIXTURES = cs.POL_MAX_DEPTH, cs.POL_MAX_MIX  # include/zbot_policy.h ZB_POL_MAX_*


@dataclasses.dataclass(frozen=True)
class PolicyShape:
    """train.py's model fields (hidden_size, depth, num_mixtures; train.py:1065-1076) as a property of a
    policy handle (include/zbot_policy.h "Network shape"). depth 1..8, num_mixtures 1..8 (read for the
    actor), hidden_size 128 only; anything else is refused by the library with the field named."""

    depth: int = DEPTH
    num_mixtures: int = MIXTURES
    hidden_size: int = HIDDEN

    def cstruct(self, generic: bool = False) -> cs.ZbPolicyShape:
        return cs.ZbPolicyShape(C.sizeof(cs.ZbPolicyShape), int(self.hidden_size), int(self.depth),
                                int(self.num_mixtures), cs.POL_SHAPE_GENERIC if generic else 0)


def _shape(shape) -> PolicyShape:
    return PolicyShape() if shape is None else shape


def _dims(kind: int, shape: PolicyShape | None = None) -> tuple[int, int]:
    if kind == ACTOR:
        return ACTOR_IN, 3 * JOINTS * _shape(shape).num_mixtures
    if kind == CRITIC:
        return CRITIC_IN, 1
    raise ZbError(f"unknown policy kind {kind}")


def param_count(kind: int, shape: PolicyShape | None = None) -> int:
    I, O = _dims(kind, shape)
    H, D = _shape(shape).hidden_size, _shape(shape).depth
    return H * I + H + D * (6 * H * H + 4 * H) + O * H + O + (JOINTS if kind == ACTOR else 0)


def flop_per_step(kind: int, shape: PolicyShape | None = None) -> int:
    """Matrix-core FLOP per env per step (FMA = 2) of a (kind, shape) network; FLOP_ACTOR / FLOP_CRITIC at
    the default shape."""
    I, O = _dims(kind, shape)
    H, D = _shape(shape).hidden_size, _shape(shape).depth
    return 2 * (I * H + D * 6 * H * H + H * O)


def init_params(kind: int, seed: int = 0, shape: PolicyShape | None = None) -> np.ndarray:
    """Parameters in the natural (equinox) layout of include/zbot_policy.h.

    Initialised like equinox [U]: Linear weight and bias ~ U(-1/sqrt(in), 1/sqrt(in)),
    GRUCell weights and biases ~ U(-1/sqrt(hidden), 1/sqrt(hidden)). The actor's trailing
    20 floats are the JOINT_BIASES mean offsets (train.py:61-82, 960)."""
    I, O = _dims(kind, shape)
    H, D = _shape(shape).hidden_size, _shape(shape).depth
    rng = np.random.default_rng(seed)

    def u(lim, *shape):
        return rng.uniform(-lim, lim, size=shape)

    parts = [u(1 / np.sqrt(I), H, I), u(1 / np.sqrt(I), H)]
    for _ in range(D):
        g = 1 / np.sqrt(H)
        parts += [u(g, 3 * H, H), u(g, 3 * H, H), u(g, 3 * H), u(g, H)]
    parts += [u(1 / np.sqrt(H), O, H), u(1 / np.sqrt(H), O)]
    if kind == ACTOR:
        parts.append(np.array([b for _, b, _ in JOINT_BIASES]))
    out = np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in parts])
    assert out.size == param_count(kind, shape)
    return out


def _host_args(kind, params, obs, carry, reset, shape):
    """Checked, contiguous numpy arguments of the host twins."""
    sh = _shape(shape)
    I, _ = _dims(kind, sh)
    p = np.ascontiguousarray(np.asarray(params, dtype=np.float32).ravel())
    if p.size != param_count(kind, sh):
        raise ZbError(f"{p.size} parameters, expected {param_count(kind, sh)}")
    o = np.ascontiguousarray(obs, dtype=np.float32)
    if o.ndim != 3 or o.shape[2] != I:
        raise ZbError(f"observations must be [T, n, {I}], got {list(o.shape)}")
    T, n, _ = o.shape
    c = np.array(carry, dtype=np.float32, order="C")  # a copy: the twin updates it in place
    if c.shape != (n, sh.depth, sh.hidden_size):
        raise ZbError(f"carry must be [{n}, {sh.depth}, {sh.hidden_size}], got {list(c.shape)}")
    r = None if reset is None else np.ascontiguousarray(np.asarray(reset).reshape(T, n), dtype=np.uint8)
    return sh.cstruct(), p, o, T, n, c, r


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def actor_host(params, obs, carry, reset=None, mode: int = SAMPLE, seed: int = 0, env_offset: int = 0, step0: int = 0,
               actions=None, log_prob: bool = False, shape: PolicyShape | None = None):
    """zb_policy_actor_host: the CPU bit reference of GruPolicy.actor at every shape. obs [T, n, 50],
    carry [n, depth, 128] (not modified) -> (actions [T, n, 20], log_prob [T, n, 20] or None, new carry)."""
    st, p, o, T, n, c, r = _host_args(ACTOR, params, obs, carry, reset, shape)
    if mode == EVAL:
        if actions is None:
            raise ZbError("EVAL needs the actions")
        a = np.array(actions, dtype=np.float32, order="C").reshape(T, n, JOINTS)
    else:
        a = np.zeros((T, n, JOINTS), np.float32)
    lp = np.zeros((T, n, JOINTS), np.float32) if log_prob else None
    _check(load_library().zb_policy_actor_host(C.byref(st), _np_ptr(p), _np_ptr(o), T, n, _np_ptr(c), _np_ptr(r),
                                               int(mode), C.c_uint64(seed), int(env_offset), C.c_uint32(step0),
                                               _np_ptr(a), _np_ptr(lp)))
    return a, lp, c


def critic_host(params, obs, carry, reset=None, shape: PolicyShape | None = None):
    """zb_policy_critic_host: the CPU bit reference of GruPolicy.critic. obs [T, n, 484] -> (value [T, n],
    new carry)."""
    st, p, o, T, n, c, r = _host_args(CRITIC, params, obs, carry, reset, shape)
    v = np.zeros((T, n), np.float32)
    _check(load_library().zb_policy_critic_host(C.byref(st), _np_ptr(p), _np_ptr(o), T, n, _np_ptr(c), _np_ptr(r),
                                                _np_ptr(v)))
    return v, c


class GruPolicy:
    """One actor or critic network on one GPU (a zb_policy handle)."""

    def __init__(self, kind: int, params=None, device: int = 0, seed: int = 0, layout: int | None = None,
                 shape: PolicyShape | None = None, generic: bool = False):
        """shape: the network's PolicyShape (default: depth 5, 5 mixtures). generic: run the shape-generic
        kernels even at the default shape (bit-identical to the default ones; include/zbot_policy.h)."""
        import torch  # noqa: PLC0415

        if not torch.cuda.is_available():
            raise ZbError("GruPolicy needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.torch = torch
        self.L = load_library()
        self.kind = kind
        self.shape = _shape(shape)
        self.generic = bool(generic)
        st = self.shape.cstruct(generic)
        if self.L.zb_policy_param_count_shaped(kind, C.byref(st)) == 0:  # the library names the bad field
            raise ZbError(f"policy shape refused: {self.L.zb_last_error().decode()}")
        self.I, self.O = _dims(kind, self.shape)
        self.n_params = param_count(kind, self.shape)
        self.device = torch.device("cuda", device)
        p = init_params(kind, seed, self.shape) if params is None else np.asarray(params, dtype=np.float32).ravel()
        p = np.ascontiguousarray(p)
        if p.size != self.n_params:
            raise ZbError(f"{p.size} parameters, expected {self.n_params}")
        self.params = p
        self._params_dev = None  # device copy of the natural-layout parameters (params_tensor)
        h = C.c_void_p()
        _check(self.L.zb_policy_create_shaped(kind, C.byref(st), p.ctypes.data_as(C.POINTER(C.c_float)), p.size,
                                              device, C.byref(h)))
        self.h = h
        # the handle's own record: flags says which kernels it runs, and so sizes its training scratch
        self._cshape = cs.ZbPolicyShape()
        _check(self.L.zb_policy_get_shape(self.h, C.byref(self._cshape)))
        if layout is not None:
            self.set_layout(layout)

    def set_layout(self, layout: int) -> None:
        """LAYOUT_BLOCK (32 envs x 8 waves a workgroup) or LAYOUT_WAVE (16 envs on one wave, the size
        of a zb_step wave's slot); bit-identical results (include/zbot_policy.h)."""
        _check(self.L.zb_policy_set_layout(self.h, int(layout)))

    def set_persistent(self, on: bool) -> None:
        """Block layout: a call over T steps as one persistent launch with the carry in registers
        (default), or one launch per step; bit-identical (include/zbot_policy.h)."""
        _check(self.L.zb_policy_set_persistent(self.h, 1 if on else 0))

    def set_params(self, params) -> None:
        """Replace the handle's parameters from a device tensor in the natural layout
        (zb_policy_set_params: repacked on the GPU, asynchronous on the current stream). Every later
        launch of this handle, PolicyRollout's included, runs the new weights."""
        torch = self.torch
        p = self._dev(params.detach().reshape(-1), torch.float32)
        if p.numel() != self.n_params:
            raise ZbError(f"{p.numel()} parameters, expected {self.n_params}")
        _check(self.L.zb_policy_set_params(self.h, p.data_ptr(), p.numel(), self._stream()))
        self._params_dev = p.clone()
        self.params = None  # the host copy is stale: params_tensor() is the record

    def params_tensor(self):
        """The handle's parameters in the natural layout, as a float32 device tensor (a copy)."""
        if self._params_dev is None:
            self._params_dev = self.torch.from_numpy(self.params).to(self.device)
        return self._params_dev.clone()

    def train_scratch_words(self, T: int, n: int) -> int:
        """fp32 words of scratch a (T, n) training forward writes and its backward reads."""
        return int(self.L.zb_policy_train_scratch_words_shaped(self.kind, C.byref(self._cshape), int(T), int(n)))

    def _train_args(self, obs, carry0, reset, scratch):
        torch = self.torch
        o = self._dev(obs, torch.float32)
        if o.dim() != 3 or o.shape[2] != self.I:
            raise ZbError(f"training observations must be [T, n, {self.I}], got {list(o.shape)}")
        T, n, _ = o.shape
        self._check_carry(carry0, n)
        r = None if reset is None else self._dev(reset.reshape(T, n), torch.uint8)
        if scratch is None:
            scratch = torch.empty(self.train_scratch_words(T, n), dtype=torch.float32, device=self.device)
        elif scratch.dtype != torch.float32 or scratch.device != self.device or not scratch.is_contiguous():
            raise ZbError(f"scratch must be a contiguous float32 tensor on {self.device}")
        return o, T, n, r, scratch

    def actor_train(self, obs, actions, carry0, reset=None, scratch=None):
        """Training forward of the actor (zb_policy_actor_train): obs [T, n, 50], actions [T, n, 20],
        carry0 [n, depth, 128] read-only -> (log_prob [T, n, 20] with the bits of actor(mode=EVAL), scratch).
        `scratch` holds the saved activations for actor_backward."""
        if self.kind != ACTOR:
            raise ZbError("actor_train() on a critic handle")
        o, T, n, r, scratch = self._train_args(obs, carry0, reset, scratch)
        a = self._dev(actions.reshape(T, n, JOINTS), self.torch.float32)
        lp = self.torch.empty(T, n, JOINTS, dtype=self.torch.float32, device=self.device)
        _check(self.L.zb_policy_actor_train(self.h, o.data_ptr(), T, n, carry0.data_ptr(),
                                            None if r is None else r.data_ptr(), a.data_ptr(), lp.data_ptr(),
                                            scratch.data_ptr(), scratch.numel(), self._stream()))
        return lp, scratch

    def critic_train(self, obs, carry0, reset=None, scratch=None):
        """Training forward of the critic (zb_policy_critic_train) -> (value [T, n], scratch)."""
        if self.kind != CRITIC:
            raise ZbError("critic_train() on an actor handle")
        o, T, n, r, scratch = self._train_args(obs, carry0, reset, scratch)
        v = self.torch.empty(T, n, dtype=self.torch.float32, device=self.device)
        _check(self.L.zb_policy_critic_train(self.h, o.data_ptr(), T, n, carry0.data_ptr(),
                                             None if r is None else r.data_ptr(), v.data_ptr(), scratch.data_ptr(),
                                             scratch.numel(), self._stream()))
        return v, scratch

    def actor_backward(self, obs, actions, carry0, reset, d_log_prob, scratch, grad=None):
        """VJP of actor_train (zb_policy_actor_backward), after it, on the same arguments and scratch:
        grad [param_count] = d(sum d_log_prob * log_prob) / d params, natural layout."""
        if self.kind != ACTOR:
            raise ZbError("actor_backward() on a critic handle")
        torch = self.torch
        o, T, n, r, scratch = self._train_args(obs, carry0, reset, scratch)
        a = self._dev(actions.reshape(T, n, JOINTS), torch.float32)
        d = self._dev(d_log_prob.reshape(T, n, JOINTS), torch.float32)
        g = self._out(grad, (self.n_params,), torch.float32)
        _check(self.L.zb_policy_actor_backward(self.h, o.data_ptr(), T, n, carry0.data_ptr(),
                                               None if r is None else r.data_ptr(), a.data_ptr(), d.data_ptr(),
                                               scratch.data_ptr(), scratch.numel(), g.data_ptr(), self._stream()))
        return g

    def critic_backward(self, obs, carry0, reset, d_value, scratch, grad=None):
        """VJP of critic_train (zb_policy_critic_backward): grad = d(sum d_value * value) / d params."""
        if self.kind != CRITIC:
            raise ZbError("critic_backward() on an actor handle")
        torch = self.torch
        o, T, n, r, scratch = self._train_args(obs, carry0, reset, scratch)
        d = self._dev(d_value.reshape(T, n), torch.float32)
        g = self._out(grad, (self.n_params,), torch.float32)
        _check(self.L.zb_policy_critic_backward(self.h, o.data_ptr(), T, n, carry0.data_ptr(),
                                                None if r is None else r.data_ptr(), d.data_ptr(), scratch.data_ptr(),
                                                scratch.numel(), g.data_ptr(), self._stream()))
        return g

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            try:
                self.L.zb_policy_destroy(h)
            except Exception:  # noqa: BLE001
                pass
            self.h = None

    def initial_carry(self, n: int):
        """get_initial_model_carry (train.py:1731-1735): zeros [n, depth, hidden] per env."""
        return self.torch.zeros(n, self.shape.depth, HIDDEN, dtype=self.torch.float32, device=self.device)

    def _stream(self) -> int:
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _dev(self, t, dtype):
        if t.dtype != dtype or t.device != self.device or not t.is_contiguous():
            t = t.to(device=self.device, dtype=dtype).contiguous()
        return t

    def _check_carry(self, carry, n):
        D = self.shape.depth
        if (tuple(carry.shape) != (n, D, HIDDEN) or carry.dtype != self.torch.float32
                or carry.device != self.device or not carry.is_contiguous()):
            raise ZbError(f"carry must be a contiguous float32 [{n}, {D}, {HIDDEN}] tensor on {self.device}")

    def _out(self, t, shape, dtype):
        if t is None:
            return self.torch.empty(*shape, dtype=dtype, device=self.device)
        if (t.numel() != int(np.prod(shape)) or t.dtype != dtype or t.device != self.device
                or not t.is_contiguous()):
            raise ZbError(f"output must be a contiguous {dtype} tensor of {int(np.prod(shape))} elements")
        return t.view(*shape)

    def actor(self, obs, carry, reset=None, mode: int = SAMPLE, seed: int = 0, env_offset: int = 0, step: int = 0,
              actions=None, log_prob=False):
        """obs [n, 50] or [T, n, 50]; carry [n, depth, 128] updated in place; reset [n] / [T, n] uint8
        (the engine's done flags: carry zeroed before that step). mode SAMPLE / MODE write `actions`,
        EVAL reads them. log_prob: False, True or an output tensor (per joint, [..., 20]).
        Returns (actions, log_prob or None) shaped like obs."""
        torch = self.torch
        if self.kind != ACTOR:
            raise ZbError("actor() on a critic handle")
        single = obs.dim() == 2
        o = self._dev(obs.unsqueeze(0) if single else obs, torch.float32)
        T, n, I = o.shape
        if I != ACTOR_IN:
            raise ZbError(f"actor observations must have {ACTOR_IN} features, got {I}")
        self._check_carry(carry, n)
        r = None if reset is None else self._dev(reset.reshape(T, n), torch.uint8)
        if mode == EVAL:
            if actions is None:
                raise ZbError("EVAL needs the actions")
            a = self._dev(actions.reshape(T, n, JOINTS), torch.float32)
        else:
            a = self._out(actions, (T, n, JOINTS), torch.float32)
        lp = None
        if log_prob is not False and log_prob is not None:
            lp = self._out(None if log_prob is True else log_prob, (T, n, JOINTS), torch.float32)
        _check(self.L.zb_policy_actor(self.h, o.data_ptr(), T, n, carry.data_ptr(),
                                      None if r is None else r.data_ptr(), int(mode), C.c_uint64(seed), int(env_offset),
                                      C.c_uint32(step), a.data_ptr(), None if lp is None else lp.data_ptr(),
                                      self._stream()))
        if single:
            return a[0], (None if lp is None else lp[0])
        return a, lp

    def critic(self, obs, carry, reset=None, value=None):
        """obs [n, 484] or [T, n, 484]; carry [n, depth, 128] updated in place -> value [n] / [T, n]."""
        torch = self.torch
        if self.kind != CRITIC:
            raise ZbError("critic() on an actor handle")
        single = obs.dim() == 2
        o = self._dev(obs.unsqueeze(0) if single else obs, torch.float32)
        T, n, I = o.shape
        if I != CRITIC_IN:
            raise ZbError(f"critic observations must have {CRITIC_IN} features, got {I}")
        self._check_carry(carry, n)
        r = None if reset is None else self._dev(reset.reshape(T, n), torch.uint8)
        v = self._out(value, (T, n), torch.float32)
        _check(self.L.zb_policy_critic(self.h, o.data_ptr(), T, n, carry.data_ptr(),
                                       None if r is None else r.data_ptr(), v.data_ptr(), self._stream()))
        return v[0] if single else v


class PolicyRollout:
    """ksim's rollout loop with the GRU actor in it (sample_action -> env.step, train.py:1737-1763),
    entirely on the GPU: per control step one actor launch and one zb_step launch, whose rows go
    straight into [T, n] buffers. Episode ends reset the actor carry (get_ppo_variables,
    train.py:1719-1723). `engine` is a HipEngine, or an EnvGroups whose groups each run their own
    actor -> zb_step chain on their own stream (bit-identical: the actor's RNG is keyed by global
    env id)."""

    def __init__(self, engine, actor: GruPolicy, seed: int = 0, curriculum: float = 1.0, stagger: bool = False,
                 exact_airtime: bool = True):
        if actor.kind != ACTOR:
            raise ZbError("PolicyRollout needs an actor")
        self.eng = engine
        self.actor = actor
        self.seed = seed
        self.curriculum = curriculum
        # each run() is one ksim trajectory: its FeetAirtime row 0 is patched to ksim's form
        # (prev contact False at t = 0, airtime roll -> air[T-1]; include/zbot.h
        # zb_feet_airtime_exact). False keeps the fused step's causal row 0.
        self.exact_airtime = exact_airtime
        # with env groups: at the first step of a run(), group g's chain starts after group g-1's
        # first actor launch, offsetting the groups' phases (bit-identical either way)
        self.stagger = stagger
        self.carry = actor.initial_carry(engine.n)
        self.step_count = 0
        self.obs = None
        self.obs_c = None  # critic observation of the current state (known after reset / recording)
        self.done = None

    def reset(self):
        out = self.eng.reset(extras=False)
        self.obs = out["obs_actor"].clone()
        self.obs_c = out["obs_critic"].clone()
        self.carry.zero_()
        self.done = None

    def run(self, T: int, record_critic: bool = False, critic: GruPolicy | None = None,
            critic_carry=None, record_terms: bool = False, mode: int = SAMPLE,
            carry_every: int | None = None) -> dict:
        """T control steps. With record_critic, out["obs_critic"][t] is the critic observation of
        the state the actor acted in at step t (what get_ppo_variables evaluates the critic on,
        train.py:1683-1729) and out["obs_critic_next"] that of the state after step T-1 (the
        bootstrap value's input). out["success"][t] flags the steps whose episode ended at the
        time limit without a failure (ksim's successes_t for compute_ppo_inputs).

        With `critic` (and record_critic), the critic runs inside the loop: V(s_t) right after
        step t's launch, in the same group chain, with `critic_carry` ([n, depth, 128], updated in
        place) reset where the previous step ended an episode (none at t = 0), then the bootstrap
        V(s_T) (reset where step T-1 ended one). out["value"] [T, n] and out["value_next"] [n] are
        bit-identical to critic.critic(out["obs_critic"], carry, reset=[0, done[:-1]]) followed by
        critic.critic(out["obs_critic_next"], carry, reset=done[-1]) after the rollout.

        With record_terms, out["reward_terms"] [T, n, 12] holds every step's unscaled reward terms
        (cs.TERM_NAMES; zb_step's reward_terms output), row 0 with ksim's FeetAirtime term when
        exact_airtime is on, as out["reward"][0] has it; with a command config on the engine,
        out["command_terms"] [T, n, 5] holds the tracking terms (cs.CMD_TERM_NAMES), read with
        zb_get_command_terms on the group's own stream right after each step. Every other output
        keeps its bits. `mode`: SAMPLE, or MODE for the deterministic rollout of the mixture's mode
        (the actor's log-probs are then those of the mode actions).

        With carry_every = L (a divisor of T; truncated BPTT), out["actor_carry_chunks"]
        [T / L, n, depth, 128] row c is the actor carry as it stood before step c L's actor launch,
        i.e. before that step's reset row is applied (row 0: the carry on entry), and with an in-loop
        critic out["critic_carry_chunks"] the same of the critic carry: one copy each per chunk on the
        group's own stream, in front of the launch. Every other output keeps its bits; without it
        nothing is allocated or issued."""
        torch = self.actor.torch
        if mode not in (SAMPLE, MODE):
            raise ZbError("PolicyRollout.run: mode is SAMPLE or MODE")
        if carry_every is not None and (int(carry_every) != carry_every or carry_every < 1 or T % carry_every):
            raise ZbError(f"PolicyRollout.run: carry_every={carry_every!r} must be an integer >= 1 that divides T = {T}")
        n, dev = self.eng.n, self.eng.device
        if self.obs is None:
            self.reset()
        if record_critic and self.obs_c is None:
            raise ZbError("the current state's critic observation is unknown (a run without "
                          "record_critic came before): reset() first")
        f32 = dict(dtype=torch.float32, device=dev)
        obs = torch.empty(T + 1, n, ACTOR_IN, **f32)
        obs[0].copy_(self.obs)
        crit = torch.empty(T + 1, n, CRITIC_IN, **f32) if record_critic else None
        if record_critic:
            crit[0].copy_(self.obs_c)
        acts = torch.empty(T, n, JOINTS, **f32)
        lp = torch.empty(T, n, JOINTS, **f32)
        rew = torch.empty(T, n, **f32)
        done = torch.zeros(T, n, dtype=torch.uint8, device=dev)
        success = torch.zeros(T, n, dtype=torch.uint8, device=dev)
        if critic is not None:
            if not record_critic or critic.kind != CRITIC or critic_carry is None:
                raise ZbError("an in-loop critic needs record_critic=True, a critic handle and its carry")
            critic._check_carry(critic_carry, n)
            val = torch.empty(T + 1, n, **f32)
        terms = cterms = None
        if record_terms:
            terms = torch.empty(T, n, cs.NUM_TERMS, **f32)
            if getattr(self.eng, "command_cfg", None) is not None:
                cterms = torch.empty(T, n, cs.NUM_CMD_TERMS, **f32)
        a_chunks = c_chunks = None
        if carry_every is not None:
            carry_every = int(carry_every)
            a_chunks = torch.empty((T // carry_every,) + tuple(self.carry.shape), **f32)
            if critic is not None:
                c_chunks = torch.empty((T // carry_every,) + tuple(critic_carry.shape), **f32)
        L = self.eng.L
        # an EnvGroups engine runs each group's actor -> zb_step chain on the group's own stream
        # (DESIGN.md §4f); a HipEngine is one group on the current stream
        grouped = hasattr(self.eng, "groups")
        parts = self.eng.groups() if grouped else [(self.eng, None, (0, n))]
        if grouped:
            self.eng.fork()
        if self.exact_airtime:
            for e, _, _ in parts:
                _check(L.zb_mark_rollout_start(e.h))
        for t in range(T):
            for g, (e, s, (lo, hi)) in enumerate(parts):
                with (torch.cuda.stream(s) if s is not None else contextlib.nullcontext()):
                    stream = torch.cuda.current_stream(dev).cuda_stream
                    r = done[t - 1][lo:hi] if t > 0 else (None if self.done is None else self.done[lo:hi])
                    if self.stagger and grouped and t == 0 and g > 0:
                        s.wait_event(prev_actor)
                    if a_chunks is not None and t % carry_every == 0:
                        a_chunks[t // carry_every][lo:hi].copy_(self.carry[lo:hi])
                    self.actor.actor(obs[t][lo:hi], self.carry[lo:hi], reset=r, mode=mode, seed=self.seed,
                                     env_offset=e.env_offset, step=self.step_count, actions=acts[t][lo:hi],
                                     log_prob=lp[t][lo:hi])
                    if self.stagger and grouped and t == 0:
                        prev_actor = torch.cuda.Event()
                        prev_actor.record(s)
                    _check(L.zb_step(e.h, acts[t][lo:hi].data_ptr(), obs[t + 1][lo:hi].data_ptr(),
                                     crit[t + 1][lo:hi].data_ptr() if record_critic else None, None,
                                     terms[t][lo:hi].data_ptr() if record_terms else None,
                                     rew[t][lo:hi].data_ptr(), done[t][lo:hi].data_ptr(),
                                     success[t][lo:hi].data_ptr(), float(self.curriculum), stream))
                    if cterms is not None:
                        _check(L.zb_get_command_terms(e.h, cterms[t][lo:hi].data_ptr(), stream))
                    if self.exact_airtime and t == T - 1:
                        _check(L.zb_feet_airtime_exact(e.h, rew[0][lo:hi].data_ptr(),
                                                       terms[0][lo:hi].data_ptr() if record_terms else None,
                                                       float(self.curriculum), stream))
                    if critic is not None:  # V(s_t): its input crit[t] is ready since step t-1
                        if c_chunks is not None and t % carry_every == 0:
                            c_chunks[t // carry_every][lo:hi].copy_(critic_carry[lo:hi])
                        critic.critic(crit[t][lo:hi], critic_carry[lo:hi],
                                      reset=done[t - 1][lo:hi] if t > 0 else None, value=val[t][lo:hi])
                        if t == T - 1:  # the bootstrap V(s_T)
                            critic.critic(crit[T][lo:hi], critic_carry[lo:hi], reset=done[T - 1][lo:hi],
                                          value=val[T][lo:hi])
                if grouped:
                    self.eng.mark(g)
            self.step_count += 1
        if grouped:
            self.eng.join()
        self.obs = obs[T].clone()
        self.obs_c = crit[T].clone() if record_critic else None
        self.done = done[T - 1].clone()
        out = dict(obs_actor=obs, actions=acts, log_prob=lp, reward=rew, done=done, success=success)
        if record_critic:
            out["obs_critic"] = crit[:T]
            out["obs_critic_next"] = crit[T]
        if critic is not None:
            out["value"] = val[:T]
            out["value_next"] = val[T]
        if record_terms:
            out["reward_terms"] = terms
            if cterms is not None:
                out["command_terms"] = cterms
        if a_chunks is not None:
            out["actor_carry_chunks"] = a_chunks
        if c_chunks is not None:
            out["critic_carry_chunks"] = c_chunks
        return out
