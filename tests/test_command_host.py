"""The velocity command law and its tracking terms on the CPU: the host twins of the step
kernel's command path (include/zbot_command.h; zb_command_initial_host, zb_command_next_host,
zb_command_rewards_host) against the fp64 numpy restatement of train.py in tests/command_ref.py.

Error contract of the terms (the rule of §4m): err <= C_BOUND * err of the same
restatement run in numpy float32, per term over the 4096 rows. C_BOUND is the smallest power of two
that is at least twice the worst ratio measured (0.96 for the host twins, 1.37 on the device).
tests/test_gpu_commands.py holds the kernel to the same contract.
"""

import ctypes as C
import math

import numpy as np
import pytest

import command_ref as R
from zbot_amd import cstructs as cs
from zbot_amd import engine as E
from zbot_amd.config import command_config

N = 4096
SEED = 2**40 + 77
CTRL_DT = 0.02
C_BOUND = 4.0
F32 = 2.0**-24  # half an ulp of 1


@pytest.fixture(scope="module", autouse=True)
def lib():
    E.build_library()
    return E.load_library()


def keys():
    rng = np.random.default_rng(5)
    env = rng.integers(0, 2**20, N).astype(np.uint32)
    ctr = rng.integers(0, 2**16, N).astype(np.uint32)
    return env, ctr


def random_quats(rng, n, max_tilt_deg=60.0):
    """Base orientations: any yaw, a tilt of up to max_tilt_deg about a random horizontal axis."""
    yaw = rng.uniform(-math.pi, math.pi, n)
    tilt = rng.uniform(0, math.radians(max_tilt_deg), n)
    ax = rng.uniform(-math.pi, math.pi, n)
    qy = np.stack([np.cos(yaw / 2), np.zeros(n), np.zeros(n), np.sin(yaw / 2)], -1)
    qt = np.stack([np.cos(tilt / 2), np.sin(tilt / 2) * np.cos(ax), np.sin(tilt / 2) * np.sin(ax), np.zeros(n)], -1)
    w1, x1, y1, z1 = qy.T
    w2, x2, y2, z2 = qt.T
    q = np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                  w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)
    return q.astype(np.float32)


def test_struct_size_agrees(lib):
    assert lib.zb_command_config_struct_bytes() == C.sizeof(cs.ZbCommandConfig)
    d = cs.ZbCommandConfig()
    lib.zb_default_command_config(C.byref(d))
    assert d.struct_bytes == C.sizeof(cs.ZbCommandConfig)
    assert (d.dead_zone, d.stand_still_threshold, d.l1_slope, d.l1_target_bonus) == (
        np.float32(0.09), np.float32(1e-2), 1.0, 2.0)
    assert d.standard_height == np.float32(0.27) and d.linvel_error_scale == 0.25
    assert list(d.term_scale) == [0.0] * 5


def test_initial_law():
    cc = R.joystick()
    env, ctr = keys()
    quat = random_quats(np.random.default_rng(1), N)
    got = E.command_initial_host(cc, SEED, env, ctr, quat, CTRL_DT)
    ref, mode = R.initial_keyed(cc, SEED, env, ctr, quat, CTRL_DT, np.float64)
    # every sampled component inside its range, or exactly 0 inside the dead zone
    stand = mode >= 4
    for col, name in ((0, "vx_range"), (1, "vy_range"), (2, "wz_range")):
        v = got[:, col]
        lo, hi = getattr(cc, name)
        assert np.all((v == 0) | ((v >= lo) & (v <= hi) & (np.abs(v) >= cc.dead_zone)))
        assert np.any(v == 0) and np.any(v != 0)
    bh = got[:, 4]
    assert np.all((bh[~stand] >= cc.bh_range[0]) & (bh[~stand] <= cc.bh_range[1]))
    assert np.all((bh[stand] >= cc.bh_standing_range[0]) & (bh[stand] <= cc.bh_standing_range[1]))
    assert np.all((got[stand, 5] >= cc.rx_range[0]) & (got[stand, 5] <= cc.rx_range[1]))
    assert np.all((got[stand, 6] >= cc.ry_range[0]) & (got[stand, 6] <= cc.ry_range[1]))
    assert np.all(got[~stand, 5:] == 0) and np.all(got[stand, :3] == 0)
    # all five command shapes occur, and standing for two of the six mode values
    assert set(np.unique(mode)) == {0, 1, 2, 3, 4, 5}
    shape = (got[:, [0, 1, 2]] != 0).astype(int) @ np.array([1, 2, 4])
    assert {1, 2, 4, 7} <= set(shape[~stand])  # forward, sideways, rotate, omni; the rest stands
    assert np.any(got[stand, 5] != 0)
    p_stand = stand.mean()
    assert abs(p_stand - 2 / 6) < 5 * math.sqrt((2 / 6) * (4 / 6) / N)
    # the components agree with fp64 to fp32 rounding (ranges and values below 1: two roundings)
    sampled = [0, 1, 2, 4, 5, 6]
    assert np.abs(got[:, sampled] - ref[:, sampled]).max() <= 4 * F32
    # heading - yaw - ctrl_dt wz within fp32 rounding of atan2f on [-pi, pi]
    resid = got[:, 3].astype(np.float64) - R.yaw_of(quat, np.float64) - CTRL_DT * got[:, 2].astype(np.float64)
    print("initial: max |heading - yaw - ctrl_dt wz| =", np.abs(resid).max())
    assert np.abs(resid).max() <= 8 * math.pi * F32


def test_switch_count_and_update():
    cc = R.joystick(switch_prob=0.25)
    env, ctr = keys()
    rng = np.random.default_rng(2)
    quat = random_quats(rng, N)
    prev = E.command_initial_host(cc, SEED, env, ctr + 1, quat, CTRL_DT)
    got, sw = E.command_next_host(cc, SEED, env, ctr, prev, quat, CTRL_DT)
    ref, sw_ref = R.next_keyed(cc, SEED, env, ctr, prev, quat, CTRL_DT, np.float64)
    assert np.array_equal(sw.astype(bool), sw_ref)
    k, p = int(sw.sum()), 0.25
    print("switches over", N, "keys:", k)
    assert abs(k - N * p) <= 5 * math.sqrt(N * p * (1 - p))
    keep = ~sw.astype(bool)
    sampled = [0, 1, 2, 4, 5, 6]
    assert np.array_equal(got[keep][:, sampled], prev[keep][:, sampled])
    assert np.array_equal(got[keep, 3], (prev[keep, 3] + prev[keep, 2] * np.float32(CTRL_DT)).astype(np.float32))
    assert np.abs(got[:, sampled] - ref[:, sampled]).max() <= 4 * F32
    assert np.abs(got[:, 3] - ref[:, 3]).max() <= 8 * math.pi * F32
    # switch_prob 0 never switches, 1 always does
    for prob, want in ((0.0, 0), (1.0, N)):
        c2 = R.joystick(switch_prob=prob)
        assert int(E.command_next_host(c2, SEED, env, ctr, prev, quat, CTRL_DT)[1].sum()) == want


def test_same_key_same_command_for_any_batch():
    cc = R.joystick()
    env, ctr = keys()
    quat = random_quats(np.random.default_rng(3), N)
    full = E.command_initial_host(cc, SEED, env, ctr, quat, CTRL_DT)
    nxt, sw = E.command_next_host(cc, SEED, env, ctr, full, quat, CTRL_DT)
    for i in (0, 1, 777, N - 1):
        one = E.command_initial_host(cc, SEED, env[i:i + 1], ctr[i:i + 1], quat[i:i + 1], CTRL_DT)
        assert np.array_equal(one[0], full[i])
        n1, s1 = E.command_next_host(cc, SEED, env[i:i + 1], ctr[i:i + 1], full[i:i + 1], quat[i:i + 1], CTRL_DT)
        assert np.array_equal(n1[0], nxt[i]) and s1[0] == sw[i]
    # the reset draws and the per-step redraws are different streams
    redraw, _ = E.command_next_host(R.joystick(switch_prob=1.0), SEED, env, ctr, full, quat, CTRL_DT)
    assert not np.array_equal(redraw[:, :3], full[:, :3])


def reward_rows():
    """4096 (quat, velocity, height, command) rows: commands from the law (a third stand), a quarter
    of the moving rows scaled to straddle stand_still_threshold, tilts up to 60 degrees, half the
    quaternions negated (w < 0), some of them unnormalised."""
    rng = np.random.default_rng(11)
    cc = R.joystick(scales=dict(linvel_tracking=1.0))
    env, ctr = keys()
    quat = random_quats(rng, N)
    cmd = E.command_initial_host(cc, SEED, env, ctr, quat, CTRL_DT)
    cmd[:, 3] += rng.uniform(-1.0, 1.0, N).astype(np.float32)  # a heading error of up to a radian
    small = rng.random(N) < 0.25
    cmd[small, :3] *= (rng.uniform(0.2, 5.0, small.sum()) * 1e-2
                       / np.maximum(np.linalg.norm(cmd[small, :3], axis=-1), 1e-9)).astype(np.float32)[:, None]
    quat[rng.random(N) < 0.5] *= -1
    quat *= rng.uniform(0.98, 1.02, N).astype(np.float32)[:, None]
    vel = rng.normal(0, 0.4, (N, 3)).astype(np.float32)
    height = rng.uniform(0.05, 0.5, N).astype(np.float32)
    norm = np.linalg.norm(cmd[:, :3], axis=-1)
    assert (norm < cc.stand_still_threshold).sum() > 500 and ((norm > cc.stand_still_threshold) & small).sum() > 300
    assert (quat[:, 0] < 0).sum() > 1000
    tilt = np.degrees(np.arccos(np.clip(1 - 2 * (quat[:, 1] ** 2 + quat[:, 2] ** 2) / (quat ** 2).sum(-1), -1, 1)))
    assert tilt.max() > 55 and tilt.max() <= 60.01
    return cc, cmd, quat, vel, height


def test_rewards_meet_the_contract():
    cc, cmd, quat, vel, height = reward_rows()
    got = E.command_rewards_host(cc, cmd, quat, vel, height)
    ref64 = R.rewards(cc, cmd, quat, vel, height, np.float64)
    ref32 = R.rewards(cc, cmd, quat, vel, height, np.float32)
    err, err32 = R.contract_ratios(got, ref64, ref32)
    for name, e, e32 in zip(cs.CMD_TERM_NAMES, err, err32):
        print(f"{name:20s} err {e:.3e}  err_ref32 {e32:.3e}  ratio {e / e32:.2f}")
    assert np.all(err32 > 0)
    assert np.all(err <= C_BOUND * err32), (err, err32)
    assert np.all((got[:, [0, 2, 3, 4]] > 0) & (got[:, [0, 2, 3, 4]] <= 1 + 1e-6))
    assert got[:, 1].max() <= 2.0


BAD = [
    (dict(struct_bytes=8), "struct_bytes"),
    (dict(vx_range=(0.5, -0.5)), "vx_range"),
    (dict(ry_range=(0.1, 0.0)), "ry_range"),
    (dict(bh_standing_range=(0.0, -0.01)), "bh_standing_range"),
    (dict(switch_prob=-0.01), "switch_prob"),
    (dict(switch_prob=1.5), "switch_prob"),
    (dict(switch_prob=float("nan")), "non-finite"),
    (dict(wz_range=(-1.0, float("inf"))), "non-finite"),
    (dict(standard_height=float("nan")), "non-finite"),
    (dict(yaw_error_scale=0.0), "yaw_error_scale"),
]


@pytest.mark.parametrize("change,text", BAD)
def test_malformed_configs_are_rejected(lib, change, text):
    cc = R.joystick()
    assert lib.zb_command_config_check(C.byref(cc)) == 0
    for k, v in change.items():
        if isinstance(v, tuple):
            getattr(cc, k)[0], getattr(cc, k)[1] = v
        else:
            setattr(cc, k, v)
    assert lib.zb_command_config_check(C.byref(cc)) == -1  # ZB_EARG
    assert text in lib.zb_last_error().decode()
    env = np.zeros(1, np.uint32)
    with pytest.raises(E.ZbError, match=text):
        E.command_initial_host(cc, 0, env, env, np.array([[1, 0, 0, 0]], np.float32), CTRL_DT)


def test_python_constructor_requires_the_ranges():
    with pytest.raises(TypeError):
        command_config(switch_prob=0.1)
    with pytest.raises(ValueError, match="unknown command terms"):
        R.joystick(scales=dict(nonsense=1.0))
    cc = R.joystick(scales=dict(yaw_tracking=0.5), by_curriculum=("yaw_tracking",))
    assert cc.term_scale[cs.CT_YAW] == 0.5 and cc.term_by_curriculum[cs.CT_YAW] == 1
    assert sum(cc.term_scale) == 0.5
