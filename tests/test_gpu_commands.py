"""Velocity commands in the step kernel (include/zbot_command.h): off is off, the
wiring of the command into the observations, the IMU back-spin, the command law and the tracking
terms against the host twins and the fp64 restatement (tests/command_ref.py), resets, and the same
bits however the envs are run. 66 envs (33 waves; split 33 + 33 each shard ends in a half-empty
wave), 8 steps, observation noise off unless said otherwise.

Error contract of heading and the terms: err <= C_BOUND * err of the float32 restatement, per
quantity over the rows of the test (tests/test_command_host.py has the rule and the measured ratios).
"""

import math

import numpy as np
import pytest

import command_ref as R
from test_command_host import C_BOUND

pytestmark = pytest.mark.gpu

N, T, SEED = 66, 8, 1234
S_CMD, S_EMA, S_LAG, S_RET, S_RNG, S_EPISODE = 176, 156, 160, 167, 169, 172
SAMPLED = [0, 1, 2, 4, 5, 6]
LEVEL = 0.7
SCALES = dict(linvel_tracking=1.5, linvel_tracking_l1=0.25, yaw_tracking=0.75, xy_orientation=-0.5, base_height=2.0)


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_MODELS = {}


def model(kind):
    if kind not in _MODELS:
        from zbot_amd import compile_model

        if kind == "default":
            _MODELS[kind] = compile_model()
        else:
            import collider_util as U

            _MODELS[kind] = compile_model(U.limbs_desc())
    return _MODELS[kind]


def config(solver="cg", eulerdamp=False, **kw):
    from zbot_amd import default_config

    return default_config(solver=solver, obs_noise=False, eulerdamp=eulerdamp, **kw)


def zero_commands():
    from zbot_amd.config import command_config

    z = (0.0, 0.0)
    return command_config(vx_range=z, vy_range=z, wz_range=z, bh_range=z, bh_standing_range=z, rx_range=z, ry_range=z,
                          switch_prob=0.0)


def actions(steps, n=N):
    """Fixed actions: the standing pose's targets with a small per-env, per-step wave."""
    from zbot_amd.constants import JOINT_BIASES

    bias = np.array([b for _, b, _ in JOINT_BIASES], np.float32)
    t, e, j = np.meshgrid(np.arange(steps), np.arange(n), np.arange(20), indexing="ij")
    return (bias + 0.05 * np.sin(0.7 * t + 0.37 * e + 1.3 * j)).astype(np.float32)


def engine(cm, cfg, ccfg=None, n=N, offset=0):
    from zbot_amd.engine import HipEngine

    eng = HipEngine(cm, cfg, n, env_offset=offset, seed=SEED)
    if ccfg is not None:
        eng.set_command_config(ccfg)
    return eng


def snap(torch, eng, out):
    torch.cuda.synchronize()
    d = {k: v.cpu().numpy().copy() for k, v in out.items()}
    d["state"] = eng.get_state().cpu().numpy()
    d["cmd_terms"] = eng.get_command_terms().cpu().numpy()
    d["cmd"] = eng.get_commands().cpu().numpy()
    return d


def run(torch, eng, acts, level=1.0, reset=True):
    """rows[0]: after reset; rows[t + 1]: after step t."""
    rows = [snap(torch, eng, eng.reset())] if reset else []
    for a in acts:
        rows.append(snap(torch, eng, eng.step(torch.from_numpy(a).cuda(), curriculum=level)))
    return rows


def u32(col):
    return np.ascontiguousarray(col).view(np.uint32)


_RUNS = {}


def shared_run(torch, kind, solver, eulerdamp, which):
    """One run of 8 steps per (model, solver, integrator) and command setting, shared by the tests
    that read it: "off" no command config, "joy" the joystick config with switch_prob 0.25 and the
    test scales at curriculum level 0.7."""
    key = (kind, solver, eulerdamp, which)
    if key not in _RUNS:
        ccfg = None if which == "off" else R.joystick(0.25, SCALES, by_curriculum=("yaw_tracking",))
        eng = engine(model(kind), config(solver, eulerdamp), ccfg)
        _RUNS[key] = (run(torch, eng, actions(T), level=LEVEL), ccfg)
    return _RUNS[key]


VARIANTS = [("default", "cg", False), ("limbs", "cg", False), ("limbs", "cg", True)]
VARIANT_IDS = ["default", "limbs", "limbs-eulerdamp"]


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_off_is_off(torch_gpu, solver):
    torch = torch_gpu
    cm, acts = model("default"), actions(T)
    a = run(torch, engine(cm, config(solver)), acts)
    b = run(torch, engine(cm, config(solver), zero_commands()), acts)
    for t, (ra, rb) in enumerate(zip(a, b)):
        keys = ["state", "obs_actor", "obs_critic"] + (["reward", "done"] if t else [])
        bad = [k for k in keys if not np.array_equal(ra[k], rb[k])]
        assert not bad, f"{solver} step {t}: a zero command config changed {bad}"
        ox_a, ox_b = ra["obs_extra"].copy(), rb["obs_extra"].copy()
        assert not ox_a[:, 67:71].any() and np.abs(np.linalg.norm(ox_b[:, 67:71], axis=1) - 1).max() < 1e-5
        ox_b[:, 67:71] = 0
        assert np.array_equal(ox_a, ox_b)
    assert not a[-1]["cmd_terms"].any() and b[-1]["cmd_terms"].all()


@pytest.mark.parametrize("kind,solver,ed", VARIANTS, ids=VARIANT_IDS)
def test_wiring(torch_gpu, kind, solver, ed):
    off, _ = shared_run(torch_gpu, kind, solver, ed, "off")
    joy, _ = shared_run(torch_gpu, kind, solver, ed, "joy")
    switched = 0
    for t, (ro, rj) in enumerate(zip(off, joy)):
        cmd = rj["state"][:, S_CMD:S_CMD + 7]
        assert np.array_equal(cmd, rj["cmd"])
        assert np.array_equal(rj["obs_actor"][:, 44:50], cmd[:, [0, 1, 3, 4, 5, 6]]), t
        assert np.array_equal(rj["obs_critic"][:, 450:457], cmd), t
        assert not ro["obs_actor"][:, 44:50].any() and not ro["obs_critic"][:, 450:457].any()
        # everything else but the IMU quaternion slots is the commands-off run: the physics never reads the command
        oa = np.r_[0:40, 50:50]
        oc = np.r_[0:446, 457:484]
        assert np.array_equal(rj["obs_actor"][:, oa], ro["obs_actor"][:, oa]), t
        assert np.array_equal(rj["obs_critic"][:, oc], ro["obs_critic"][:, oc]), t
        st = np.r_[0:S_EMA, S_LAG:S_RET, S_RET + 1:S_CMD, S_CMD + 7:192]
        assert np.array_equal(rj["state"][:, st], ro["state"][:, st]), t
        if t:
            assert np.array_equal(rj["done"], ro["done"]) and np.array_equal(rj["reward_terms"], ro["reward_terms"])
            switched += int((cmd[:, SAMPLED] != joy[t - 1]["cmd"][:, SAMPLED]).any(1).sum())
    first = joy[0]["cmd"]
    assert (first[:, :3] != 0).any() and (first[:, 5:] != 0).any()
    assert 0 < switched < N * T // 2
    # the heading moved the IMU observation
    assert not np.array_equal(joy[-1]["obs_actor"][:, 40:44], off[-1]["obs_actor"][:, 40:44])


def test_backspin(torch_gpu):
    torch = torch_gpu
    cm, acts, h = model("default"), actions(T), 0.3
    runs = []
    for heading in (0.0, h):
        eng = engine(cm, config(), zero_commands())
        eng.reset()
        st = eng.get_state()
        st[:, S_EMA:S_EMA + 4] = 0  # the filter starts at 0 in both runs, so it is linear in its input
        eng.set_state(st)
        cmd = torch.zeros(N, 7)
        cmd[:, 3] = heading
        eng.set_commands(cmd)
        runs.append(run(torch, eng, acts, reset=False))
    a, b = runs
    lag = a[0]["state"][:, S_LAG].astype(np.float64)[:, None]
    qh = np.array([math.cos(h / 2), 0.0, 0.0, -math.sin(h / 2)])  # yaw(-h)
    worst, prev_a, prev_b = 0.0, np.zeros((N, 4)), np.zeros((N, 4))
    for t, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["state"][:, :58], rb["state"][:, :58])  # qpos, qvel: identical physics
        assert np.all(rb["cmd"][:, 3] == np.float32(h)) and not ra["cmd"].any()
        xa, xb = ra["obs_actor"][:, 40:44].astype(np.float64), rb["obs_actor"][:, 40:44].astype(np.float64)
        # neither run takes the w < 0 flip: the filter's inputs (x_t - lag x_{t-1}) / (1 - lag) keep w well above 0
        for x, p in ((xa, prev_a), (xb, prev_b)):
            assert ((x - lag * p) / (1 - lag))[:, 0].min() > 0.5
        prev_a, prev_b = xa, xb
        w1, x1, y1, z1 = qh
        w2, x2, y2, z2 = xa.T
        want = np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                         w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)
        worst = max(worst, np.abs(xb - want).max())
    print("back-spin: max |B - yaw(-h) x A| =", worst)
    # a handful of fp32 roundings on unit-size values plus the 1e-6 eps of rotate_quat_by_quat
    assert worst <= 1e-5
    assert np.abs(xb - xa).max() > 0.05  # and the spin is there


def test_law_on_the_device(torch_gpu):
    torch = torch_gpu
    from zbot_amd import engine as E

    cm, cfg, steps = model("default"), config(), 16
    ccfg = R.joystick(0.25)
    rows = run(torch, engine(cm, cfg, ccfg), actions(steps))
    env = np.arange(N, dtype=np.uint32)
    err = err32 = 0.0
    nsw = 0
    for t in range(steps):
        before, after = rows[t], rows[t + 1]
        assert not after["done"].any()
        ctr = u32(before["state"][:, S_RNG])
        quat = after["obs_critic"][:, 480:484]
        want, sw = E.command_next_host(ccfg, SEED, env, ctr, before["cmd"], quat, cfg.ctrl_dt)
        assert np.array_equal(after["cmd"][:, SAMPLED], want[:, SAMPLED]), t
        moved = (after["cmd"][:, SAMPLED] != before["cmd"][:, SAMPLED]).any(1)
        assert not (moved & ~sw.astype(bool)).any()
        nsw += int(sw.sum())
        ref64, _ = R.next_keyed(ccfg, SEED, env, ctr, before["cmd"], quat, cfg.ctrl_dt, np.float64)
        ref32, _ = R.next_keyed(ccfg, SEED, env, ctr, before["cmd"], quat, cfg.ctrl_dt, np.float32)
        err = max(err, np.abs(after["cmd"][:, 3] - ref64[:, 3]).max())
        err32 = max(err32, np.abs(ref32[:, 3].astype(np.float64) - ref64[:, 3]).max())
    total, p = N * steps, 0.25
    assert abs(nsw - total * p) <= 5 * math.sqrt(total * p * (1 - p))
    print(f"heading: err {err:.3e} err_ref32 {err32:.3e} ratio {err / err32:.2f}; {nsw} switches")
    assert err <= C_BOUND * err32
    # the reset drew the initial command of episode 0 at the reset pose
    want0 = E.command_initial_host(ccfg, SEED, env, u32(rows[0]["state"][:, S_EPISODE]) - np.uint32(1), rows[0]["obs_critic"][:, 480:484], cfg.ctrl_dt)
    assert np.array_equal(rows[0]["cmd"][:, SAMPLED], want0[:, SAMPLED])
    assert np.abs(rows[0]["cmd"][:, 3] - want0[:, 3]).max() <= 1e-6


@pytest.mark.parametrize("kind,solver,ed", VARIANTS, ids=VARIANT_IDS)
def test_rewards_on_the_device(torch_gpu, kind, solver, ed):
    from zbot_amd import cstructs as cs

    off, _ = shared_run(torch_gpu, kind, solver, ed, "off")
    joy, ccfg = shared_run(torch_gpu, kind, solver, ed, "joy")
    sc = np.array([ccfg.term_scale[i] * (LEVEL if ccfg.term_by_curriculum[i] else 1.0) for i in range(5)])
    sc32 = np.array([np.float32(ccfg.term_scale[i]) * (np.float32(LEVEL) if ccfg.term_by_curriculum[i] else np.float32(1))
                     for i in range(5)], np.float64)
    assert np.count_nonzero(sc) == 5 and sum(ccfg.term_by_curriculum) == 1
    got, r64, r32 = [], [], []
    for t in range(1, T + 1):
        assert not joy[t]["done"].any() and not off[t]["done"].any(), "no row may hide behind the done exclusion"
        ox = joy[t]["obs_extra"]
        args = (joy[t - 1]["cmd"], ox[:, cs.X_CMD_XQUAT:cs.X_CMD_XQUAT + 4], ox[:, cs.X_BASE_LINVEL:cs.X_BASE_LINVEL + 3],
                ox[:, cs.X_BASE_HEIGHT])
        terms = joy[t]["cmd_terms"]
        got.append(terms)
        r64.append(R.rewards(ccfg, *args, np.float64))
        r32.append(R.rewards(ccfg, *args, np.float32))
        # reward_B - reward_A = sum_i scale_i level_i term_i: the kernel rounds each product and each of the five
        # adds (6 roundings of at most sum |s_i t_i|), then the add to the other terms' total (one of |reward_B|)
        delta = joy[t]["reward"].astype(np.float64) - off[t]["reward"].astype(np.float64)
        want = (sc32 * terms.astype(np.float64)).sum(1)
        bound = 2.0**-24 * (6 * np.abs(sc32 * terms).sum(1) + np.abs(joy[t]["reward"]) + np.abs(off[t]["reward"]))
        assert np.all(np.abs(delta - want) <= bound), (t, np.abs(delta - want).max(), bound.min())
        assert np.abs(want).max() > 0.1
    err, err32 = R.contract_ratios(np.concatenate(got), np.concatenate(r64), np.concatenate(r32))
    for name, e, e32 in zip(cs.CMD_TERM_NAMES, err, err32):
        print(f"{kind} {name:20s} err {e:.3e}  err_ref32 {e32:.3e}  ratio {e / e32:.2f}")
    assert np.all(err32 > 0) and np.all(err <= C_BOUND * err32), (err, err32)
    # the episode return carries the command terms too
    assert np.all(joy[T]["state"][:, S_RET] != off[T]["state"][:, S_RET])


def test_resets(torch_gpu):
    torch = torch_gpu
    from zbot_amd import engine as E

    cm, cfg = model("default"), config()
    ccfg = R.joystick(0.25)
    eng = engine(cm, cfg, ccfg)
    r0 = snap(torch, eng, eng.reset())
    k = 17
    st = eng.get_state()
    # env k lies on its front below bad_z[0]: it terminates in this step (a termination, not a fault)
    st[k, 2] = cfg.bad_z[0] - 0.01
    st[k, 3:7] = torch.tensor([math.cos(math.pi / 4), 0.0, math.sin(math.pi / 4), 0.0])
    eng.set_state(st)
    before = snap(torch, eng, eng.outputs())
    r1 = snap(torch, eng, eng.step(torch.from_numpy(actions(1)[0]).cuda()))
    done = r1["done"].astype(bool)
    assert done[k] and done.sum() == 1
    env = np.arange(N, dtype=np.uint32)
    quat = r1["obs_critic"][:, 480:484]
    want, _ = E.command_next_host(ccfg, SEED, env, u32(before["state"][:, S_RNG]), before["cmd"], quat, cfg.ctrl_dt)
    init = E.command_initial_host(ccfg, SEED, env, u32(before["state"][:, S_EPISODE]), quat, cfg.ctrl_dt)
    assert u32(r1["state"][:, S_EPISODE])[k] == u32(before["state"][:, S_EPISODE])[k] + 1
    want[k] = init[k]
    assert np.array_equal(r1["cmd"][:, SAMPLED], want[:, SAMPLED])
    assert np.abs(r1["cmd"][:, 3] - want[:, 3]).max() <= 1e-6
    assert not np.array_equal(init[k, SAMPLED], r0["cmd"][k, SAMPLED])
    assert np.array_equal(r1["obs_critic"][:, 450:457], r1["cmd"])
    # a masked reset redraws only the masked envs
    mask = np.zeros(N, np.uint8)
    mask[[0, 5, k, N - 1]] = 1
    r2 = snap(torch, eng, eng.reset(mask=torch.from_numpy(mask)))
    m = mask.astype(bool)
    assert np.array_equal(r2["cmd"][~m], r1["cmd"][~m])
    init2 = E.command_initial_host(ccfg, SEED, env, u32(r1["state"][:, S_EPISODE]), r2["state"][:, 3:7], cfg.ctrl_dt)
    assert np.array_equal(r2["cmd"][m][:, SAMPLED], init2[m][:, SAMPLED])
    assert np.abs(r2["cmd"][m, 3] - init2[m, 3]).max() <= 1e-6
    assert np.array_equal(r2["obs_critic"][m, 450:457], r2["cmd"][m])


SAME_KEYS = ("state", "reward", "cmd_terms")


def assert_same(got, want, what):
    bad = [k for k in SAME_KEYS if not np.array_equal(got[k], want[k])]
    assert not bad, f"{what}: {bad} differ"


def test_same_bits_however_it_is_run(torch_gpu):
    torch = torch_gpu
    from zbot_amd.engine import EnvGroups

    ref, ccfg = shared_run(torch, "default", "cg", False, "joy")
    cm, cfg, acts = model("default"), config(), actions(T)
    # two handles over envs 0..32 and 33..65
    halves = [run(torch, engine(cm, cfg, ccfg, n=33, offset=o), acts[:, o:o + 33], level=LEVEL) for o in (0, 33)]
    for t in range(T + 1):
        both = {k: np.concatenate([h[t][k] for h in halves]) for k in SAME_KEYS}
        assert_same(both, ref[t], f"two shards, step {t}")
    # one rollout launch of 8 steps
    eng = engine(cm, cfg, ccfg)
    eng.reset()
    rsum = torch.zeros(N, device="cuda")
    eng.rollout(torch.from_numpy(acts).cuda(), curriculum=LEVEL, reward_sum=rsum)
    roll = snap(torch, eng, eng.outputs())
    acc = np.zeros(N, np.float32)
    for t in range(1, T + 1):
        acc = (acc + ref[t]["reward"]).astype(np.float32)
    roll["reward"] = rsum.cpu().numpy()
    assert_same(roll, dict(ref[T], reward=acc), "zb_rollout(8)")
    assert np.array_equal(roll["obs_actor"], ref[T]["obs_actor"])
    # two env groups
    grp = EnvGroups(cm, cfg, N, groups=2, seed=SEED)
    grp.set_command_config(ccfg)
    grp.reset()
    for t in range(T):
        out = grp.step(torch.from_numpy(acts[t]).cuda(), curriculum=LEVEL)
        grp.join()
        torch.cuda.synchronize()
        got = dict(state=grp.get_state().cpu().numpy(), reward=out["reward"].cpu().numpy(),
                   cmd_terms=grp.get_command_terms().cpu().numpy())
        assert_same(got, ref[t + 1], f"two groups, step {t}")
        assert np.array_equal(grp.get_commands().cpu().numpy(), ref[t + 1]["cmd"])
    # four chunks per control step
    eng = engine(cm, cfg, ccfg)
    eng.set_step_chunks(4)
    for t, row in enumerate(run(torch, eng, acts, level=LEVEL)):
        assert_same(row, ref[t], f"4 chunks, step {t}")
    eng.check()
    # the state at step 4 into a fresh handle, then 4 more steps
    eng = engine(cm, cfg, ccfg)
    eng.set_state(torch.from_numpy(ref[4]["state"]))
    for t, row in enumerate(run(torch, eng, acts[4:], level=LEVEL, reset=False)):
        assert_same(row, ref[5 + t], f"resumed at 4, step {5 + t}")


@pytest.mark.parametrize("groups", [1, 2])
def test_task_env_exposes_the_command(torch_gpu, groups):
    torch = torch_gpu
    from zbot_amd import cstructs as cs
    from zbot_amd.constants import COMMAND_NAME
    from zbot_amd.task import ZbotWalkingEnv

    ccfg = R.joystick(0.25, SCALES)
    env = ZbotWalkingEnv(N, seed=SEED, obs_noise=False, model=model("default"), groups=groups, command=ccfg)
    r = env.reset()
    assert torch.equal(r.commands[COMMAND_NAME], env.engine.get_commands())
    r = env.step(torch.from_numpy(actions(1)[0]).cuda())
    cmd = r.commands[COMMAND_NAME]
    torch.cuda.synchronize()
    assert cmd.shape == (N, 7) and torch.equal(cmd, env.engine.get_commands()) and cmd.abs().sum() > 0
    assert set(cs.CMD_TERM_NAMES) <= set(r.reward_terms)
    assert torch.equal(r.reward_terms["base_height"], env.engine.get_command_terms()[:, cs.CT_BASE_HEIGHT])
    assert ZbotWalkingEnv(N, seed=SEED, model=model("default")).reset().commands[COMMAND_NAME].abs().sum() == 0
