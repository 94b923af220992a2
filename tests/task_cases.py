"""Edge states of the step end (terminations, reward branches, counters, the push timer), shared by
tests/test_task_ref_host.py (CPU: the restatement against both oracles, and the conditions the set must
meet) and tests/test_gpu_task_edges.py (the engine). Test infrastructure only.

61 envs from the oracle's warm standing states (20 control steps after a reset, the recipe of
test_gpu_parity.warm_states); every rung is an edit of state words or of the base pose. The env index
is the layout: its parity is the team of the wave, so the terminating envs are placed to cover a wave
whose two teams end, one whose team 0 alone ends, one whose team 1 alone ends, and the last env of an
odd count (a wave with one live team).

  0..7    z ladder across bad_z[1] = 0.5, in the air (ends 0.472 .. 0.532; 3 stay, 5 end)
  8..13   tilt ladder about x across 60 degrees, lifted to 0.40, base angular velocity 0
  14..19  tilt ladder about y
  20      forced failure (z = 0.7): team 0 alone           21 plain
  22..26  base forward velocity -0.3, 0.1, float32(0.2) (the clip itself), 0.3, 0.6, lifted
  28..31  S_FEET_DIST 0.10, the float32 below 0.12, float32(0.12), 0.14
  32..39  S_TOUCH at touch_threshold (no contact) or one ulp above (contact) x S_PREV_CONT x S_AIRTIME:
          touchdown left / right / both / none, a foot that stays in the air, a lift-off
  40, 41  a foot in the air on a step that ends by the time limit (S_AIRTIME returns to 0)
  42      the same on a step that ends by a failure         43 plain
  44..47  S_EP_STEPS 3997, 3998, 3999, 4000 (80 s at 0.02 s: 3999 ends, by the fp32 product)
  48, 49  failure and time limit in the same step (success 0): by height, by tilt
  50..52  S_PUSH_TIMER float32(0.02) (fires), the float32 above it (does not), 0.01 (fires)
  55      forced failure: team 1 alone    56, 57 forced failures: both teams    60 the last env, forced
  the rest plain.

The "lowz" variant is the same set on a config whose BadZ band is (0.5, 0.9): the z ladder then crosses
the LOWER bound (an env ends when it finishes below 0.5), which no standing robot can reach at the
default 0.05 without also tilting past 60 degrees.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from zbot_amd import cstructs as cs
from zbot_amd import default_config

f32 = np.float32
N = 61
SEED = 7
LEVELS = (1.0, 0.7)
Z_RUNGS = (-0.03, -0.01, -0.003, -0.001, 0.001, 0.003, 0.01, 0.03)  # start = bound + rung + 0.004 (the fall of one step is ~0.002)
TILT_RUNGS = (-3.0, -1.0, -0.3, 0.3, 1.0, 3.0)  # degrees from 60
VX_RUNGS = (-0.3, 0.1, f32(0.2), 0.3, 0.6)
Z_MARGIN = 5e-4  # 5x the flat CG position contract (test_gpu_parity.ONE_STEP_TOL_CG["qpos"])
UPZ_MARGIN = 1e-3
LIFT = 0.40  # base height of the lifted rungs: no collider reaches the floor, below bad_z[1]

G = dict(z=range(0, 8), tilt_x=range(8, 14), tilt_y=range(14, 20), team0=[20], vx=range(22, 27), feet_dist=range(28, 32),
         touch=range(32, 40), air_trunc=[40, 41], air_fail=[42], ep_steps=range(44, 48), fail_trunc=[48, 49],
         push=range(50, 53), team1=[55], both=[56, 57], last=[60])
G = {k: list(v) for k, v in G.items()}
# envs whose S_EP_STEPS is at the time limit's edge: the fp32 law is the expectation (the fp64 oracle differs)
EP_EDGE = sorted(G["air_trunc"] + G["ep_steps"] + G["fail_trunc"])
# done by the stated law at the default config, per env (1 = the episode ends)
EXPECT_DONE = np.zeros(N, bool)
EXPECT_DONE[[3, 4, 5, 6, 7, 11, 12, 13, 17, 18, 19, 20, 40, 41, 42, 46, 47, 48, 49, 55, 56, 57, 60]] = True
EXPECT_SUCCESS = np.zeros(N, bool)
EXPECT_SUCCESS[[40, 41, 46, 47]] = True
PUSH_FIRES = {50: True, 51: False, 52: True}


def config(variant="default", **kw):
    cfg = default_config(**kw)
    if variant == "lowz":
        cfg.bad_z[0], cfg.bad_z[1] = 0.5, 0.9
    else:
        assert variant == "default", variant
    return cfg


def _tilt(axis: int, deg: float) -> np.ndarray:
    h = np.radians(deg) / 2
    q = np.zeros(4)
    q[0], q[1 + axis] = np.cos(h), np.sin(h)
    return q.astype(f32)


def build(O, cm, cfg, n: int = N) -> SimpleNamespace:
    """The edge set on `cfg` (its randomization rows, where cfg randomizes): state [n, 192], rand, the
    action of the step, and the groups (G). n < N keeps the first n envs (not used by the tests)."""
    env = O.OracleEnv(cm.cmodel, cfg, N, seed=SEED)
    env.reset()
    for t in range(20):
        env.step(O.synthetic_actions(cm.cmodel, SEED, N, 0, t))
    st = env.state.copy()
    thr = f32(cfg.touch_threshold)
    T, U = thr, np.nextafter(thr, f32(1))

    def words(e, touch=None, prev=None, air=None, steps=None):
        if touch is not None:
            st[e, cs.S_TOUCH:cs.S_TOUCH + 2] = touch
        if prev is not None:
            st[e, cs.S_PREV_CONT:cs.S_PREV_CONT + 2] = prev
        if air is not None:
            st[e, cs.S_AIRTIME:cs.S_AIRTIME + 2] = air
        if steps is not None:
            st[e:e + 1, cs.S_EP_STEPS].view(np.uint32)[:] = steps

    for e, d in zip(G["z"], Z_RUNGS):
        st[e, 2] = 0.5 + d + 0.004
    for axis, key in ((0, "tilt_x"), (1, "tilt_y")):
        for e, d in zip(G[key], TILT_RUNGS):
            st[e, 2] = LIFT
            st[e, 3:7] = _tilt(axis, 60.0 + d)
            st[e, cs.S_QVEL + 3:cs.S_QVEL + 6] = 0.0
    for e in G["team0"] + G["team1"] + G["both"] + G["last"]:
        st[e, 2] = 0.7
    for e, vx in zip(G["vx"], VX_RUNGS):
        st[e, 2] = LIFT
        st[e, cs.S_QVEL] = vx
    near = f32(cfg.feet_too_close_threshold)
    st[G["feet_dist"], cs.S_FEET_DIST] = [f32(0.10), np.nextafter(near, f32(0)), near, f32(0.14)]
    combos = [((U, T), (0, 0), (0.5, 0.7)),   # touchdown left; the right foot stays in the air
              ((T, U), (0, 0), (0.5, 0.7)),   # touchdown right
              ((U, U), (0, 0), (0.5, 0.7)),   # touchdown on both
              ((U, U), (1, 1), (0.0, 0.0)),   # standing on: none
              ((T, T), (0, 0), (0.5, 0.7)),   # both in the air: none, both airtimes grow
              ((T, T), (1, 1), (0.0, 0.0)),   # lift-off of both
              ((U, T), (1, 0), (0.0, 0.26)),  # one foot down as before, the other still in the air
              ((U, U), (0, 1), (0.1, 0.0))]   # touchdown left after 0.1 s: a negative term
    for e, (touch, prev, air) in zip(G["touch"], combos):
        words(e, touch, prev, air)
    words(40, (T, T), (0, 0), (0.3, 0.44), 3999)
    words(41, (U, T), (1, 0), (0.0, 0.4), 3999)
    words(42, (T, T), (0, 0), (0.2, 0.6))
    st[42, 2] = 0.7
    for e, k in zip(G["ep_steps"], (3997, 3998, 3999, 4000)):
        words(e, steps=k)
    words(48, steps=3999)
    st[48, 2] = 0.7
    words(49, steps=3999)
    st[49, 2] = LIFT
    st[49, 3:7] = _tilt(0, 70.0)
    st[49, cs.S_QVEL + 3:cs.S_QVEL + 6] = 0.0
    dt = f32(cfg.ctrl_dt)
    st[G["push"], cs.S_PUSH_TIMER] = [dt, np.nextafter(dt, f32(1)), f32(0.01)]
    a = O.synthetic_actions(cm.cmodel, SEED, N, 0, 100)
    return SimpleNamespace(state=st[:n].copy(), rand=env.rand[:n].copy(), action=a[:n].copy(), n=n, groups=G)


def oracle_step(O, cm, cfg, case, curriculum: float = 1.0, precision: str = "f32") -> SimpleNamespace:
    """One oracle step of the set: (outputs, the post-step state and rand, the statistics)."""
    env = O.OracleEnv(cm.cmodel, cfg, case.n, seed=SEED, precision=precision)
    env.state[:], env.rand[:] = case.state, case.rand
    out = env.step(case.action, curriculum)
    return SimpleNamespace(out=out, state=env.state.copy(), rand=env.rand.copy(), stats=env.stats.copy(), env=env)
