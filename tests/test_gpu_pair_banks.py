"""The sole pair beside two banks of floor colliders on the GPU (the XG 6 kernels): the nine-collider
model whose soles also collide with each other (collider_util.many_pair_desc) holds the first four
colliders beyond the soles within reach of the floor each substep, as the model without the pair
does, and the pair's half rows in a fourth contact-row bank. Against the oracle, which collides all
nine and the pair, from states with the legs crossed, half the robots standing and half lying
(collider_util.crossing_touching_states; tests/test_bank_cap.py shows that these states put a contact
on the third or fourth collider within reach in at least 6 of the 64 envs and more than four within
reach in at least one)."""

import numpy as np
import pytest

import collider_util as U
from test_bank_cap import N_ENVS, STATE_SEED, pair_bank_cases
from zbot_amd import compile_model, default_config
from zbot_amd import cstructs as cs

pytestmark = pytest.mark.gpu

BANK_CAP = 4


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def many_pair():
    """The model and its crossing, touching states with each env's candidates (computed once)."""
    cm = compile_model(U.many_pair_desc())
    cm.variant = "many_pair"
    q, cand, deep = pair_bank_cases(cm)
    ncand = np.array([len(c) for c in cand])
    cm.q, cm.ncand, cm.deep = q, ncand, ((ncand == 3) | (ncand == 4)) & deep
    return cm


def touching_env(O, cm, cfg, seed=STATE_SEED):
    """An oracle env at the module's states, at rest, no warm start (as test_gpu_sole_pair.crossing_env
    prepares the limbs + pair model's)."""
    env = O.OracleEnv(cm.cmodel, cfg, N_ENVS, seed=seed)
    env.reset()
    env.state[:, :27] = cm.q.astype(np.float32)
    env.state[:, 32:58] = 0.0
    env.state[:, cs.S_QACCW:cs.S_QACCW + 32] = 0.0
    return env


@pytest.mark.parametrize("solver", ["newton", "cg"])
def test_debug_forward_matches_oracle(torch_gpu, many_pair, oracle_mod, solver):
    """One forward pass for every env with at most four colliders beyond the soles within reach: contact
    and constraint counts exact (floor colliders of both floor banks + the pair), the constrained
    acceleration and both touch sensors against the fp64 oracle. With a cap of two the envs whose third
    or fourth collider within reach touches the floor would lose those contacts and differ in the counts."""
    torch = torch_gpu
    from test_gpu_sole_pair import tie_member

    from zbot_amd.engine import DBG, HipEngine

    cm = many_pair
    cfg = default_config(solver=solver)
    n = N_ENVS
    env = touching_env(oracle_mod, cm, cfg)
    st = env.state.copy()
    ctrl = (np.random.default_rng(2).normal(size=(n, 20)) * 0.5).astype(np.float32)
    eng = HipEngine(cm, cfg, n)
    g = eng.debug_forward(torch.from_numpy(st), torch.from_numpy(ctrl)).cpu().numpy()
    worst, npair, ties, checked = 0.0, 0, [], []
    for e in range(n):
        if cm.ncand[e] > BANK_CAP:
            continue
        checked.append(e)
        ref = oracle_mod.forward_debug(cm.cmodel, cfg, st[e, :27], st[e, 32:58], ctrl[e], precision="f64")
        got = (int(g[e, DBG["misc"] + 1]), int(g[e, DBG["misc"]]))
        print(f"[pair banks {solver} debug forward] env {e}: {int(cm.ncand[e])} candidates, (ncon, nefc) {got} vs "
              f"{(ref['ncon'], ref['nefc'])}")
        if got != (ref["ncon"], ref["nefc"]):
            # a tie of the box-box manifold selection (test_gpu_sole_pair.test_debug_forward_matches_oracle)
            ref = tie_member(oracle_mod, cm, cfg, st[e], ctrl[e], got)
            assert ref is not None, (e, got)
            ties.append(e)
        p = oracle_mod.constraint_problem(cm.cmodel, cfg, st[e, :27], st[e, 32:58], ctrl[e], precision="f64")
        npair += int(((p["type"] == 2) & (np.abs(p["J"][:, :6]).max(1) == 0)).sum() > 0)
        qa = g[e, DBG["qacc"]:DBG["qacc"] + 26]
        err = np.abs(qa - ref["qacc"]).max() / max(1.0, np.abs(ref["qacc"]).max())
        worst = max(worst, err)
        assert err <= (1e-3 if solver == "newton" else 5e-2), (e, err)
        np.testing.assert_allclose(g[e, DBG["misc"] + 2:DBG["misc"] + 4], ref["touch"], rtol=2e-3, atol=2e-3)
    deep = [e for e in checked if cm.deep[e]]
    print(f"\n[pair banks {solver} debug forward] {len(checked)} of {n} envs within {BANK_CAP} candidates, {len(deep)} of "
          f"them with a contact on the third or fourth ({deep}), {npair} with pair contacts, max relative qacc "
          f"error {worst:.2e}, manifold ties {ties}")
    assert len(ties) <= 2
    assert len(deep) >= 6
    assert len(checked) >= 48


@pytest.mark.parametrize("eulerdamp", [False, True], ids=["explicit", "eulerdamp"])
@pytest.mark.parametrize("solver", ["newton", "cg"])
def test_one_step_matches_oracle(torch_gpu, many_pair, oracle_mod, solver, eulerdamp):
    """Two env-steps, each from the oracle's state: done exact, every output under the sole pair's
    one-step contract for the envs whose step kept within the cap (no overflow flag), the flag on
    every env that starts with more than four within reach, and at least one env that starts with three
    or four ends the first step unflagged."""
    torch = torch_gpu
    from test_gpu_parity import (CG_BUDGET, CG_LOOSE, CG_SLACK, MaxErr, boundary_envs, one_step_outputs, oracle_sensitivity,
                                 oracle_steps)
    from test_gpu_sole_pair import PAIR_TOL

    from zbot_amd.engine import HipEngine

    cm = many_pair
    cfg = default_config(solver=solver, eulerdamp=eulerdamp)
    n = N_ENVS
    cg = solver == "cg"
    env = touching_env(oracle_mod, cm, cfg)
    eng = HipEngine(cm, cfg, n, seed=STATE_SEED)
    kw = dict(budget=CG_BUDGET, loose=CG_LOOSE, max_ill=n, k_slack=CG_SLACK) if cg else {}
    tag = f"pair banks {solver}{' eulerdamp' if eulerdamp else ''}"
    err = MaxErr(f"{tag} one-step (unflagged envs)", **kw)
    for t in range(2):
        st0, rd0 = env.state.copy(), env.rand.copy()
        ncand = np.array([len(U.bank2_candidates(cm, st0[e, :27].astype(np.float64))) for e in range(n)])
        eng.set_state(torch.from_numpy(st0.copy()))
        eng.set_rand(torch.from_numpy(rd0.copy()))
        a = oracle_mod.synthetic_actions(cm.cmodel, STATE_SEED, n, 0, t)
        ref, ref64 = oracle_steps(oracle_mod, cm, cfg, env, a, STATE_SEED)
        ref32 = {k: want for k, _, want in one_step_outputs(env.state, ref, env.state, ref)}
        sens = oracle_sensitivity(oracle_mod, cm, cfg, st0, rd0, a, STATE_SEED, ref32) if cg else {}
        out = eng.step(torch.from_numpy(a).cuda())
        torch.cuda.synchronize()
        gs = eng.get_state().cpu().numpy()
        flag = (gs[:, cs.S_NAN].view(np.int32) & 2) != 0
        keep = ~flag
        print(f"\n[{tag}] step {t}: candidates per env {np.bincount(ncand).tolist()}, {int(keep.sum())} of {n} envs "
              f"without the overflow flag, {int((keep & (ncand >= 3)).sum())} of them started with 3 or 4 within reach")
        np.testing.assert_array_equal(out["done"].cpu().numpy(), ref["done"])
        assert np.array_equal(eng.flags()["bank_overflow"].cpu().numpy(), flag)
        assert flag[ncand > BANK_CAP].all(), "an env that starts with more than the cap is flagged"
        if t == 0:
            assert np.array_equal(ncand, cm.ncand)
            # the step's own bit: the state came in with clear flags, so it equals the sticky one
            assert np.array_equal(eng.flags()["bank_overflow_step"].cpu().numpy(), flag)
            assert (keep & (ncand >= 3) & (ncand <= BANK_CAP)).any(), "an env with 3 or 4 within reach stays unflagged"
        assert keep.sum() >= n // 2
        # boundary envs by their position among the kept ones
        pos = np.cumsum(keep) - 1
        bnd = {int(pos[e]) for e in boundary_envs(ref64) if keep[e]}
        for key, got, want in one_step_outputs(gs, out, env.state, ref):
            sk = sens.get(key)
            err.add(key, got[keep], want[keep], *PAIR_TOL[key], ref64=ref64[key][keep],
                    sens=None if sk is None else np.asarray(sk)[keep], exempt=bnd)
    err.report()


@pytest.mark.parametrize("solver", ["newton", "cg"])
def test_same_bits_however_the_envs_are_run(torch_gpu, many_pair, oracle_mod, solver):
    """6 control steps with pushes from the module's states: one rollout launch, two half-size handles,
    two env groups and the chunked step all leave the state bits of six zb_step calls on one handle."""
    torch = torch_gpu
    from zbot_amd.engine import EnvGroups, HipEngine

    cm = many_pair
    cfg = default_config(solver=solver, push=True)
    n, T, seed = N_ENVS, 6, 4
    A = torch.from_numpy(np.stack([oracle_mod.synthetic_actions(cm.cmodel, seed, n, 0, t, std=0.3)
                                   for t in range(T)])).cuda()
    env = touching_env(oracle_mod, cm, cfg, seed=seed)
    st, rd = torch.from_numpy(env.state.copy()), torch.from_numpy(env.rand.copy())

    def load(h, lo=0, hi=n):
        h.set_state(st[lo:hi].clone())
        h.set_rand(rd[lo:hi].clone())
        return h

    def stepped(h, lo=0, hi=n):
        for t in range(T):
            h.step(A[t, lo:hi].contiguous())
        if hasattr(h, "join"):
            h.join()
        torch.cuda.synchronize()
        return h.get_state().cpu().numpy()

    base = stepped(load(HipEngine(cm, cfg, n, seed=seed)))
    assert np.isfinite(base[:, :58]).all()
    roll = load(HipEngine(cm, cfg, n, seed=seed))
    roll.rollout(A, reward_sum=torch.zeros(n, device="cuda"))
    torch.cuda.synchronize()
    assert np.array_equal(roll.get_state().cpu().numpy(), base), "zb_rollout"
    halves = [stepped(load(HipEngine(cm, cfg, n // 2, env_offset=off, seed=seed), off, off + n // 2), off, off + n // 2)
              for off in (0, n // 2)]
    assert np.array_equal(np.concatenate(halves), base), "two half-size handles"
    assert np.array_equal(stepped(load(EnvGroups(cm, cfg, n, groups=2, seed=seed))), base), "two env groups"
    chunked = load(HipEngine(cm, cfg, n, seed=seed))
    chunked.set_step_chunks(2)
    assert np.array_equal(stepped(chunked), base), "chunked step"


@pytest.mark.parametrize("solver", ["newton", "cg"])
def test_rollout_from_reset_matches_oracle(torch_gpu, many_pair, oracle_mod, solver):
    """test_gpu_sole_pair.test_rollout_from_reset_matches_oracle's contract for the many + pair model: 48
    control steps of 64 envs from reset with the legs driven into each other; the first 3 rewards under
    the one-step contract, done flags exact over the first 16 steps, then the ensemble contract over all
    64 envs. Prints how many envs ever had more than four colliders beyond the soles within reach."""
    torch = torch_gpu
    from test_gpu_parity import GOLDEN_EXACT_STEPS, GOLDEN_TOL, GOLDEN_TOL_CG, MaxErr, golden_ensemble_check
    from test_gpu_sole_pair import crossing_actions

    from zbot_amd.engine import HipEngine

    cm = many_pair
    cfg = default_config(solver=solver)
    n, steps, seed = 64, 48, 13
    acts = crossing_actions(oracle_mod, cm, seed, n, steps)
    e32 = oracle_mod.OracleEnv(cm.cmodel, cfg, n, seed=seed)
    e64 = oracle_mod.OracleEnv(cm.cmodel, cfg, n, seed=seed, precision="f64")
    e32.reset()
    ref_r, ref_d, r64s, touching = [], [], [], 0
    for t in range(steps):
        if t < 8:
            e64.state[:] = e32.state
            e64.rand[:] = e32.rand
            r64s.append(e64.step(acts[t])["reward"].copy())
        o = e32.step(acts[t])
        ref_r.append(o["reward"].copy())
        ref_d.append(o["done"].copy())
        for e in range(0, n, 4):
            p = oracle_mod.constraint_problem(cm.cmodel, cfg, e32.state[e, :27], e32.state[e, 32:58], precision="f64")
            touching += int(((p["type"] == 2) & (np.abs(p["J"][:, :6]).max(1) == 0)).any())
    g = {"reward": np.stack(ref_r), "done": np.stack(ref_d), "final_state": e32.state.copy()}
    eng = HipEngine(cm, cfg, n, seed=seed)
    eng.reset()
    rew, done = [], []
    for t in range(steps):
        o = eng.step(torch.from_numpy(acts[t]).cuda())
        rew.append(o["reward"].cpu().numpy().copy())
        done.append(o["done"].cpu().numpy().copy())
    rew, done = np.stack(rew), np.stack(done)
    over = int(eng.flags()["bank_overflow"].sum().item())
    print(f"\n[pair banks {solver} rollout] envs whose sticky overflow bit is set after {steps} steps: {over} of {n}; "
          f"oracle env-steps with pair contacts (every 4th env): {touching} of {steps * n // 4}")
    assert over <= n // 4
    np.testing.assert_array_equal(done[:GOLDEN_EXACT_STEPS], g["done"][:GOLDEN_EXACT_STEPS])
    err = MaxErr(f"pair banks {solver} rollout from reset")
    tol = GOLDEN_TOL_CG if solver == "cg" else GOLDEN_TOL
    for t in range(3):
        err.add(f"reward[{t}]", rew[t], g["reward"][t], tol["reward"], ref64=r64s[t])
    assert touching > 0
    golden_ensemble_check(f"pair banks {solver}", rew, done, eng.get_state().cpu().numpy(), g)
    err.report()
