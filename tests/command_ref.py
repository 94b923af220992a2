"""numpy restatement of the velocity command law and its five tracking terms
(include/zbot_command.h), as train.py writes them (UnifiedCommand :189-261, the tracking rewards
:278-412, BaseHeightReward :469-482) with the standard ZYX forms of the un-vendored
xax.quat_to_euler / euler_to_quat / rotate_vector_by_quat. Every function takes the dtype it
computes in: float64 is the reference, float32 the yardstick of the error contract
(tests/test_command_host.py, tests/test_gpu_commands.py). Shared by both; holds no test.
"""

import numpy as np

RNG_CMD, K_RESET, K_SWITCH, K_REDRAW = 5, 0, 4, 8
RANGES = ("vx_range", "vy_range", "wz_range", "bh_range", "bh_standing_range", "rx_range", "ry_range")


def joystick(switch_prob=0.25, scales=None, by_curriculum=()):
    """The joystick config of the tests: every range two-sided and wider than the dead zone."""
    from zbot_amd.config import command_config

    return command_config(vx_range=(-0.3, 0.8), vy_range=(-0.4, 0.4), wz_range=(-1.0, 1.0), bh_range=(-0.05, 0.02),
                          bh_standing_range=(-0.08, 0.0), rx_range=(-0.2, 0.2), ry_range=(-0.25, 0.15),
                          switch_prob=switch_prob, scales=scales, by_curriculum=by_curriculum)


def _rotl(x, r):
    return ((x << np.uint32(r)) | (x >> np.uint32(32 - r))).astype(np.uint32)


def threefry2x32(k0, k1, c0, c1):
    """Random123 threefry2x32-20 on uint32 arrays (zbot_fmath.h zbf_threefry2x32)."""
    with np.errstate(over="ignore"):
        k0, k1, c0, c1 = (np.asarray(v, np.uint32) for v in (k0, k1, c0, c1))
        ks = (k0, k1, np.uint32(0x1BD11BDA) ^ k0 ^ k1)
        x0, x1 = (c0 + k0).astype(np.uint32), (c1 + k1).astype(np.uint32)
        R = (13, 15, 26, 6, 17, 29, 16, 24)
        for blk in range(5):
            for i in range(4):
                x0 = (x0 + x1).astype(np.uint32)
                x1 = _rotl(x1, R[(blk & 1) * 4 + i]) ^ x0
            x0 = (x0 + ks[(blk + 1) % 3]).astype(np.uint32)
            x1 = (x1 + ks[(blk + 2) % 3] + np.uint32(blk + 1)).astype(np.uint32)
    return x0, x1


def uniform2(seed, k, env, ctr):
    """The pair of uniforms of draw k under the command purpose: exact in float32 and float64."""
    k0 = np.uint32((seed & 0xFFFFFFFF) ^ ((RNG_CMD * 0x9E3779B9) & 0xFFFFFFFF))
    k1 = np.uint32(((seed >> 32) & 0xFFFFFFFF) ^ ((k * 0x85EBCA6B) & 0xFFFFFFFF))
    a, b = threefry2x32(k0, k1, env, ctr)
    return (a >> np.uint32(8)).astype(np.float64) / 16777216.0, (b >> np.uint32(8)).astype(np.float64) / 16777216.0


def uniforms8(seed, k0, env, ctr):
    return np.stack([u for k in range(4) for u in uniform2(seed, k0 + k, env, ctr)], axis=-1)


def quat_to_euler(q, dt):
    q = np.asarray(q, dt)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, x, y, z = (q[..., i] for i in range(4))
    two, one = dt(2), dt(1)
    roll = np.arctan2(two * (w * x + y * z), one - two * (x * x + y * y))
    pitch = np.arcsin(np.clip(two * (w * y - z * x), -one, one))
    yaw = np.arctan2(two * (w * z + x * y), one - two * (y * y + z * z))
    return np.stack([roll, pitch, yaw], -1).astype(dt)


def euler_to_quat(e, dt):
    e = np.asarray(e, dt)
    h = dt(0.5)
    cr, sr = np.cos(e[..., 0] * h), np.sin(e[..., 0] * h)
    cp, sp = np.cos(e[..., 1] * h), np.sin(e[..., 1] * h)
    cy, sy = np.cos(e[..., 2] * h), np.sin(e[..., 2] * h)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy], -1).astype(dt)


def rotate_vector_by_quat(v, q, inverse, dt):
    q = np.asarray(q, dt)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, u = q[..., :1], q[..., 1:] * (dt(-1) if inverse else dt(1))
    t = dt(2) * np.cross(u, v)
    return (v + w * t + np.cross(u, t)).astype(dt)


def yaw_of(q, dt):
    return quat_to_euler(q, dt)[..., 2]


def initial(cc, u, yaw, ctrl_dt, dt):
    """UnifiedCommand.initial_command on uniforms u [n, 8] (mode, vx, vy, wz, bh, bhs, rx, ry)."""
    u = np.asarray(u, dt)
    mode = np.minimum(np.floor(dt(6) * u[:, 0]).astype(np.int64), 5)

    def draw(name, col):
        lo, hi = (dt(v) for v in getattr(cc, name))
        return lo + (hi - lo) * u[:, col]

    vx, vy, wz, bh, bhs, rx, ry = (draw(nm, i + 1) for i, nm in enumerate(RANGES))
    dz = dt(cc.dead_zone)
    vx, vy, wz = (np.where(np.abs(v) < dz, dt(0), v) for v in (vx, vy, wz))
    z = np.zeros_like(vx)
    stand = mode >= 4
    cmd = np.stack([np.where((mode == 0) | (mode == 3), vx, z), np.where((mode == 1) | (mode == 3), vy, z),
                    np.where((mode == 2) | (mode == 3), wz, z), z, np.where(stand, bhs, bh), np.where(stand, rx, z),
                    np.where(stand, ry, z)], -1).astype(dt)
    cmd[:, 3] = np.asarray(yaw, dt) + dt(ctrl_dt) * cmd[:, 2]
    return cmd, mode


def initial_keyed(cc, seed, env, ctr, quat, ctrl_dt, dt, k0=K_RESET):
    return initial(cc, uniforms8(seed, k0, env, ctr), yaw_of(quat, dt), ctrl_dt, dt)


def next_keyed(cc, seed, env, ctr, prev, quat, ctrl_dt, dt):
    """UnifiedCommand.__call__: (next command, switched)."""
    prev = np.asarray(prev, dt)
    fresh, _ = initial_keyed(cc, seed, env, ctr, quat, ctrl_dt, dt, K_REDRAW)
    sw = uniform2(seed, K_SWITCH, env, ctr)[0].astype(dt) < dt(cc.switch_prob)
    cont = prev.copy()
    cont[:, 3] = prev[:, 3] + prev[:, 2] * dt(ctrl_dt)
    return np.where(sw[:, None], fresh, cont).astype(dt), sw


def rewards(cc, cmd, xquat, vel, height, dt):
    """The five unscaled terms [n, 5] as train.py writes them."""
    cmd, xquat, vel, height = (np.asarray(v, dt) for v in (cmd, xquat, vel, height))
    n = cmd.shape[0]
    euler = quat_to_euler(xquat, dt)
    zq = euler_to_quat(np.stack([np.zeros(n, dt), np.zeros(n, dt), euler[:, 2]], -1), dt)
    still = np.sqrt((cmd[:, :3] ** 2).sum(-1)) < dt(cc.stand_still_threshold)
    out = np.empty((n, 5), dt)
    # LinearVelocityTrackingReward
    rcmd = np.zeros((n, 3), dt)
    rcmd[:, :2] = cmd[:, :2]
    gcmd = rotate_vector_by_quat(rcmd, zq, False, dt)
    e = np.sqrt(((vel[:, :2] - gcmd[:, :2]) ** 2).sum(-1))
    out[:, 0] = np.exp(-np.where(still, e, dt(2) * e * e) / dt(cc.linvel_error_scale))
    # L1LinearVelocityTrackingReward
    vr = rotate_vector_by_quat(vel, zq, True, dt)[:, :2]
    walk = np.abs(vr - cmd[:, :2]).sum(-1)
    stand = np.abs(vr).sum(-1)
    out[:, 1] = dt(cc.l1_target_bonus) - dt(cc.l1_slope) * np.where(still, stand, walk)
    # AngularVelocityTrackingReward
    tq = euler_to_quat(np.stack([np.zeros(n, dt), np.zeros(n, dt), cmd[:, 3]], -1), dt)
    out[:, 2] = np.exp(-(dt(1) - (tq * zq).sum(-1) ** 2) / dt(cc.yaw_error_scale))
    # XYOrientationReward
    bq = euler_to_quat(np.stack([euler[:, 0], euler[:, 1], np.zeros(n, dt)], -1), dt)
    cq = euler_to_quat(np.stack([cmd[:, 5], cmd[:, 6], np.zeros(n, dt)], -1), dt)
    out[:, 3] = np.exp(-(dt(1) - (cq * bq).sum(-1) ** 2) / dt(cc.xy_orient_error_scale))
    # BaseHeightReward
    out[:, 4] = np.exp(-np.abs(height - (cmd[:, 4] + dt(cc.standard_height))) / dt(cc.base_height_error_scale))
    return out


def contract_ratios(got, ref64, ref32):
    """Per term: max |got - ref64| / max |ref32 - ref64| over the rows (err of the float32 restatement)."""
    e = np.abs(np.asarray(got, np.float64) - ref64).max(0)
    e32 = np.abs(np.asarray(ref32, np.float64) - ref64).max(0)
    return e, e32
