"""GPU suite for the Swimmer stepper (k_swimmer_step / k_swimmer_reset of csrc/swimmer_env.h) against the numpy restatement in
tests/swimmer_restatement.py.  As in test_cartchain_hip.py every step is restated from the device's own previous state, so a difference
cannot build up.  The states are not bit-identical (closed-form Cholesky against np.linalg.solve, two libms); the largest relative state
difference per step, |got - want| / max(1, |want|), is measured by run_parity and kept in profiles/swimmer_parity.json; every state
comparison holds at 100x that figure, capped at 1e-9 (section 19's rule: the cap is a condition, not a measurement).

Reward tolerance, derived from the state tolerance e: reward = (x' - x) / 0.04 - cost; a state error e moves x by e * max(1, |x|) on
both ends of the difference, so the reward by at most 2 e max(1, |x|) / 0.04, plus one float32 ulp of the reward (it is stored as
float32)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import swimmer_restatement as sr  # noqa: E402

CAP = 1e-9
F32 = dict(rtol=2.5e-7, atol=1e-12)     # float32 values of float64 quantities that agree to the state tolerance


def state_tol():
    p = json.load(open(os.path.join(ROOT, "profiles", "swimmer_parity.json")))
    return min(100.0 * p["max_rel_state_diff"], CAP)


def _model(**kw):
    from ilswiss_amd.envs.models_swimmer import swimmer
    m = swimmer()
    m.update(kw)
    return m


def _env(ctx, n, seed=3, **kw):
    from ilswiss_amd.envs import HipVectorEnv
    return HipVectorEnv("swimmer", n, seed=seed, ctx=ctx, **kw)


def _rel(got, want):
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def _rew_tol(tol, x_before, x_after, rew):
    x = np.maximum(1.0, np.maximum(np.abs(x_before), np.abs(x_after)))
    return 2.0 * tol * x / 0.04 + np.spacing(np.abs(rew).astype(np.float32)).astype(np.float64)


def _check_step(S, pq, pv, a, gq, gv, obs, rew, tol, keep=None):
    wq, wv, wobs, wrew = S.step(pq, pv, a)
    k = np.ones(len(pq), bool) if keep is None else keep
    worst = max(float(_rel(gq[k], wq[k]).max(initial=0.0)), float(_rel(gv[k], wv[k]).max(initial=0.0)))
    assert worst <= tol, worst
    if obs is not None:
        np.testing.assert_allclose(np.asarray(obs, np.float32), wobs, **F32)
    if rew is not None:
        assert np.all(np.abs(np.asarray(rew, np.float64) - wrew) <= _rew_tol(tol, pq[:, 0], wq[:, 0], wrew))
    return worst


@pytest.mark.gpu
def test_dims_spaces_and_state_round_trip(ctx):
    from ilswiss_amd.envs.vecenv import Box
    S = sr.Swimmer(_model())
    env = _env(ctx, 4)
    assert (env.obs_dim, env.act_dim, env.nq, env.nv, env.discrete_n) == (8, 2, 5, 5, 0)
    ac = env.action_space[0]
    assert isinstance(ac, Box) and ac.shape == (2,) and np.array_equal(ac.low, [-1, -1]) and np.array_equal(ac.high, [1, 1])
    assert env.observation_space[0].shape == (8,)
    obs = env.reset()
    q, v = env.get_state()
    assert np.abs(q).max() <= 0.1 and np.abs(v).max() <= 0.1 and q.std() > 0.02
    np.testing.assert_allclose(obs.astype(np.float32), S.observe(q, v), **F32)
    rng = np.random.default_rng(4)
    q, v = rng.uniform(-0.9, 0.9, (4, 5)), rng.uniform(-3, 3, (4, 5))
    env.set_state(q, v)
    gq, gv = env.get_state()
    assert np.array_equal(gq, q) and np.array_equal(gv, v)
    a = np.zeros((4, 2), np.float32)
    obs, rew, done, _ = env.step(a)
    gq, gv = env.get_state()
    _check_step(S, q, v, a, gq, gv, obs, rew, state_tol())
    assert not done.any()
    env.close()


def run_parity(ctx, tol):
    """70 envs (a partial wavefront), 120 auto-resetting steps with the device's random actions, path limit 50 so that resets happen;
    every step restated from the device's previous state.  Returns the largest relative state difference; asserts everything at `tol`."""
    import ilswiss_amd as ia
    S = sr.Swimmer(_model())
    n, T, maxlen = 70, 120, 50
    env = _env(ctx, n, seed=11)
    env.rollout_stats(reset=True)
    rb = ia.SimpleReplayBuffer(n, 8, 2, ctx=ctx)       # capacity n: step t's record of env i sits at slot i
    pq, pv = env.get_state()
    ep_len, ep_ret = np.zeros(n, int), np.zeros(n)
    worst, episodes, ret_sum = 0.0, 0, 0.0
    for t in range(T):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
        rec = rb._gather(np.arange(n))
        a = rec["actions"]
        assert a.shape == (n, 2) and np.all(np.abs(a) < 1)
        np.testing.assert_allclose(rec["observations"], S.observe(pq, pv), **F32)
        assert not rec["terminals"].any()
        gq, gv = env.get_state()
        ep_len += 1
        end = ep_len >= maxlen
        worst = max(worst, _check_step(S, pq, pv, a, gq, gv, rec["next_observations"], rec["rewards"][:, 0], tol, keep=~end))
        ep_ret += S.step(pq, pv, a)[3]
        assert np.all(np.abs(gq[end]) <= 0.1) and np.all(np.abs(gv[end]) <= 0.1)          # the ended envs were reset
        episodes += int(end.sum()); ret_sum += float(ep_ret[end].sum())
        ep_len[end], ep_ret[end] = 0, 0.0
        pq, pv = gq, gv
    e, r = env.rollout_stats(reset=True)
    assert e == episodes == 2 * n
    np.testing.assert_allclose(r, ret_sum, rtol=1e-6, atol=1e-6)
    env.close()
    return worst


@pytest.mark.gpu
def test_rollout_steps_match_the_restatement(ctx):
    print("largest relative state difference", run_parity(ctx, state_tol()))


@pytest.mark.gpu
def test_block_boundary(ctx):
    S = sr.Swimmer(_model())
    env = _env(ctx, 257, seed=5)
    rng = np.random.default_rng(6)
    for _ in range(3):
        q, v = env.get_state()
        a = rng.uniform(-1, 1, (257, 2)).astype(np.float32)
        obs, rew, _, _ = env.step(a)
        _check_step(S, q, v, a, *env.get_state(), obs, rew, state_tol())
    env.close()


@pytest.mark.gpu
def test_limit_rows_match_the_restatement(ctx):
    S = sr.Swimmer(_model())
    lim = np.radians(100.0)
    sg = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], float)
    q = np.concatenate([np.tile([0.1, -0.2, 0.3], (4, 1)), sg * (lim + np.array([0.01, 0.02]))], 1)
    v = np.concatenate([np.tile([0.1, -0.2, 0.5], (4, 1)), sg * np.array([6.0, 8.0])], 1)
    _, active, f = S.dynamics(q, v, np.zeros((4, 2)))
    assert active.all() and np.all(f > 0.0)            # both rows on at once: the comparison below is not vacuous
    env = _env(ctx, 4, seed=5)
    env.set_state(q, v)
    a = (0.5 * sg).astype(np.float32)                   # the motors push into the limits
    for _ in range(5):
        pq, pv = env.get_state()
        obs, rew, _, _ = env.step(a)
        _check_step(S, pq, pv, a, *env.get_state(), obs, rew, state_tol())
    env.close()


@pytest.mark.gpu
def test_fluid_off_through_the_model_argument(ctx):
    m = _model(density=0.0, viscosity=0.0)
    S = sr.Swimmer(m)
    env = _env(ctx, 8, seed=5, model=m)
    rng = np.random.default_rng(7)
    on = _env(ctx, 8, seed=5)
    on.set_state(*env.get_state())
    for _ in range(20):
        pq, pv = env.get_state()
        a = rng.uniform(-1, 1, (8, 2)).astype(np.float32)
        obs, rew, _, _ = env.step(a)
        on.step(a)
        _check_step(S, pq, pv, a, *env.get_state(), obs, rew, state_tol())
    assert np.abs(on.get_state()[0] - env.get_state()[0]).max() > 1e-3      # the fluid does matter
    env.close(), on.close()


@pytest.mark.gpu
def test_actions_outside_the_box_are_clipped_and_recorded_unmapped(ctx):
    import ilswiss_amd as ia
    env = _env(ctx, 6)
    rng = np.random.default_rng(5)
    q, v = rng.uniform(-0.1, 0.1, (6, 5)), rng.uniform(-1, 1, (6, 5))
    a = np.array([[3.0, -3.0], [1.5, -1.0001], [100.0, -1e6], [0.2, 5.0], [-2.0, 0.1], [1.0, -1.0]], np.float32)
    res = []
    for act in (a, np.clip(a, -1, 1)):
        env.set_state(q, v)
        obs, rew, done, _ = env.step(act)
        res.append((env.get_state(), rew, obs))
    for x, y in zip(res[0], res[1]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    # the record holds the action as the policy gave it
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[32, 32], obs_dim=8, action_dim=2, ctx=ctx)
    rb = ia.SimpleReplayBuffer(6, 8, 2, ctx=ctx)
    env.set_state(q, v)
    env.rollout_step(policy=pol, replay=rb, max_path_length=1000)
    rec = rb._gather(np.arange(6))
    gq, gv = env.get_state()
    _check_step(sr.Swimmer(_model()), q, v, rec["actions"], gq, gv, rec["next_observations"], rec["rewards"][:, 0], state_tol())
    env.close()


@pytest.mark.gpu
def test_path_mode_inserts_whole_episodes(ctx):
    import ilswiss_amd as ia
    n, maxlen = 16, 5
    env = _env(ctx, n, seed=5)
    env.set_path_mode(True)
    rb = ia.SimpleReplayBuffer(1 << 12, 8, 2, ctx=ctx)
    for _ in range(12):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
    size, _ = rb._cursors()
    assert len(rb._traj_endpoints) == 2 * n and size == 2 * n * maxlen
    b = rb._gather(np.arange(size))
    for s, e in rb._traj_endpoints.items():
        rows = np.arange(s, e)
        assert rows.size == maxlen and not b["terminals"][rows].any()
        assert np.array_equal(b["observations"][rows][1:], b["next_observations"][rows][:-1])
        assert np.abs(b["observations"][rows[0]]).max() <= 0.1 + 1e-7          # starts from a reset state
    env.close()


@pytest.mark.gpu
def test_policy_rollout_evaluation_and_ppo_sampling(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.ppo import PPO, ReparamMultivariateGaussianPolicy
    from ilswiss_amd.samplers import DeviceEvalSampler
    n = 16
    env = _env(ctx, n, seed=9)
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[32, 32], obs_dim=8, action_dim=2, ctx=ctx)
    rb = ia.SimpleReplayBuffer(64, 8, 2, ctx=ctx)
    for _ in range(3):
        env.rollout_step(policy=pol, replay=rb, max_path_length=1000)
    size, _ = rb._cursors()
    rec = rb._gather(np.arange(size))
    assert size == 3 * n and all(np.isfinite(rec[k]).all() for k in ("observations", "actions", "rewards", "next_observations"))
    st = DeviceEvalSampler(env, ia.MakeDeterministic(pol), 2 * n * 6, 6).obtain_statistics()
    assert st["Num Paths"] >= n and np.isfinite(st["AverageReturn"]) and st["Test Ep. Len. Max"] == 6 == st["Test Ep. Len. Min"]
    gp = ReparamMultivariateGaussianPolicy([32, 32], 8, 2, conditioned_std=False, hidden_activation="tanh", ctx=ctx)
    vf = ia.FlattenMlp([32, 32], 1, 8, hidden_activation="tanh", ctx=ctx)
    tr = PPO(gp, vf, mini_batch_size=32, update_epoch=1, gae_tau=0.95, max_samples=n * 4)
    assert tr.train_from_rollout(env, 4, max_path_length=1000) == n * 4
    _, obs, act, rew, ends, lastv = tr._roll
    assert obs.numpy().shape == (n * 4, 8) and act.numpy().shape == (n * 4, 2)
    assert np.isfinite(obs.numpy()).all() and np.isfinite(act.numpy()).all() and np.isfinite(rew.numpy()).all()
    env.close()


@pytest.mark.gpu
def test_norm_obs_running_statistics(ctx):
    """Turning norm_obs on feeds the env's current observations (the creation-time reset) to the statistics as their first batch; ten
    steps add ten more.  Mean and variance over all eleven batches against numpy's on the read-back observations."""
    n = 32
    S = sr.Swimmer(_model())
    env = _env(ctx, n, seed=2, norm_obs=True)
    raw = _env(ctx, n, seed=2)
    rng = np.random.default_rng(0)
    seen = [S.observe(*env.get_state()).astype(np.float64)]
    assert env.obs_rms.count == n
    for _ in range(10):
        a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        raw.set_state(*env.get_state())
        seen.append(raw.step(a)[0])
        o = env.step(a)[0]
    m, v, cnt = env.obs_rms.mean, env.obs_rms.var, env.obs_rms.count
    x = np.concatenate(seen)
    assert cnt == 11 * n == len(x)
    # float64 statistics merged batch by batch against numpy's one pass over float32 observations held as float64
    np.testing.assert_allclose(m, x.mean(0), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(v, x.var(0), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(o, np.clip((seen[-1] - m) / np.sqrt(v + np.finfo(np.float32).eps), -10, 10), rtol=1e-5, atol=1e-5)
    env.close(), raw.close()


@pytest.mark.gpu
def test_refusals(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.envs.vecenv import swimmer_struct
    env = _env(ctx, 8, seed=2)
    cat = ia.DiscretePolicy(hidden_sizes=[32, 32], obs_dim=8, action_dim=3, ctx=ctx)
    with pytest.raises(RuntimeError, match="categorical policy on an env with a Box"):
        env.rollout_step(policy=cat, max_path_length=200)
    sh, sc = np.zeros(8), np.ones(8)
    assert ctx.lib.ilsx_vecenv_set_obs_affine(env.h, sh.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p)) != 0
    with pytest.raises(NotImplementedError):
        _env(ctx, 4, obs_shift=sh, obs_scale=sc)
    env.close()
    bad = []
    m = _model(); m["limited"] = [1, 0, 0, 1, 1]; bad.append(m)                     # a limited root degree of freedom
    m = _model(); m["box"] = [(1.0, 0.0, 0.1)] + m["box"][1:]; bad.append(m)        # a non-positive box side
    m = _model(); m["n_link"] = 2; bad.append(m)                                    # a link count the kernels do not exist for
    for _ in range(2):                                                               # create and destroy twice: nothing is left behind
        for m in bad:
            h = C.c_void_p()
            ms = swimmer_struct(m)
            assert ctx.lib.ilsx_vecenv_create_swimmer(ctx.h, C.byref(ms), 4, C.c_uint64(1), C.byref(h)) != 0 and not h.value
        e = _env(ctx, 4)
        e.close()
    h = C.c_void_p()
    assert ctx.lib.ilsx_vecenv_create_classic(ctx.h, 16, 4, C.c_uint64(1), C.byref(h)) != 0 and not h.value


@pytest.mark.gpu
def test_get_envs_builds_training_and_evaluation_envs(ctx):
    from ilswiss_amd.envs import get_env, get_envs
    tr = get_envs(dict(env_name="swimmer", env_num=3, training_env_seed=1), ctx=ctx)
    ev = get_env(dict(env_name="swimmer", eval_env_seed=2), ctx=ctx)
    assert len(tr) == 3 and tr.reset().shape == (3, 8) and ev.reset().shape == (1, 8)
    tr.close(), ev.close()
