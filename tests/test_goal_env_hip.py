"""GPU suite of the device goal env (PointReachTask of csrc/goal_env.h behind HipVectorEnv("point-reach")) and of the epsilon-uniform
branch of the Gaussian exploration strategy (k_explore of csrc/ilsx_env.hip).

The env's oracle is the host class her.PointReachEnv: one step of 300 envs (one full workgroup and a partial one) from states and actions
of tests/her_sample_restatement.py's generator must give the host class's float64 state, its float32 observation row and its reward,
bit for bit.  tests/test_goal_env_cpu.py shows that no input lies within 1e-12 of the threshold in goal distance, so the sparse reward is
compared on every row.  The dense reward leaves the stepper as float32 like every task's reward; it is compared with the float32
roundings of the float64 interval ref * (1 -+ 1e-15) (rounding is monotonic, so this is exactly what rtol 1e-15 on the float64 value
allows to be seen)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import her_sample_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[x.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def step_ref():
    p, g, v, a = R.step_inputs()
    return dict(p=p, g=g, v=v, a=a, sparse=R.host_step(p, g, a), dense=R.host_step(p, g, a, dense=True))


@pytest.mark.parametrize("rtype", ("sparse", "dense"))
def test_one_step_is_the_host_class_step(ctx, step_ref, rtype):
    from ilswiss_amd.envs import HipVectorEnv
    p, g, v, a = (step_ref[k] for k in "pgva")
    p2, v2, rows, rew, dist = step_ref[rtype]
    env = HipVectorEnv("point-reach", R.STEP_N, seed=1, ctx=ctx, env_kwargs=dict(tol=R.TOL, reward_type=rtype))
    assert (env.obs_dim, env.act_dim, env.nq, env.nv, env.d_obs, env.d_goal) == (8, 2, 4, 2, 4, 2)
    env.set_state(np.concatenate([p, g], 1), v)
    obs, r, done, _ = env.step(a)
    q_dev, v_dev = env.get_state()
    assert _same(q_dev[:, :2], p2) and _same(q_dev[:, 2:], g) and _same(v_dev, v2)      # float64 state: exact
    assert _same(obs.astype(np.float32), rows)                                            # float32 observation row: exact
    assert not done.any()
    if rtype == "sparse":
        keep = np.abs(dist - R.TOL) > 1e-12
        assert keep.all()
        np.testing.assert_array_equal(r[keep], rew[keep])
        assert set(np.unique(r)) == {-1.0, 0.0}
    else:
        lo, hi = (rew * (1 + 1e-15)).astype(np.float32), (rew * (1 - 1e-15)).astype(np.float32)    # rew < 0: lo <= hi
        got = r.astype(np.float32)
        print("dense reward: rows that differ from float32(ref):", int((got != rew.astype(np.float32)).sum()))
        assert ((got >= lo) & (got <= hi)).all()
    env.close()


def test_reset_draws():
    """Own contexts: an env's Philox stream id is its context's object counter, so the same seed repeats only on a fresh context."""
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    cs = [ia.Context(0, seed=5), ia.Context(0, seed=5)]
    try:
        e1, e2 = (HipVectorEnv("point-reach", 5, seed=9, ctx=c) for c in cs)
        q1, v1 = e1.get_state()
        assert _same(q1, e2.get_state()[0])                                               # the same seed gives the same draws
        seen = [q1]
        for _ in range(3):
            o1, o2 = e1.reset(), e2.reset()
            assert _same(o1, o2)
            q, v = e1.get_state()
            assert (np.abs(q[:, :2]) <= 0.5).all() and (np.abs(q[:, 2:]) <= 0.8).all() and (v == 0).all()
            assert len({tuple(r) for r in q[:, 2:].tolist()}) == 5                        # goals differ between envs
            assert (np.abs(q[:, 2:] - seen[-1][:, 2:]).max(axis=1) > 0).all()             # ... and between consecutive episodes of one env
            assert _same(o1.astype(np.float32), np.concatenate([q[:, :2], v, q[:, 2:], q[:, :2]], 1).astype(np.float32))
            seen.append(q)
        assert np.abs(np.concatenate(seen)[:, 2:]).max() > 0.5                            # the goal range is wider than the start range
        q0, v0 = e1.get_state()
        o = e1.reset([1, 3])
        q, v = e1.get_state()
        assert _same(q[[0, 2, 4]], q0[[0, 2, 4]]) and _same(v[[0, 2, 4]], v0[[0, 2, 4]])  # the others' state is untouched
        assert (q[[1, 3]] != q0[[1, 3]]).all() and o.shape == (2, 8)
        assert _same(o.astype(np.float32), np.concatenate([q[:, :2], v, q[:, 2:], q[:, :2]], 1).astype(np.float32)[[1, 3]])
        e1.close(), e2.close()
    finally:
        for c in cs:
            c.close()


def test_the_policy_reads_the_observation_and_goal_prefix(ctx):
    """A rollout step with a deterministic policy: the recorded actions are policy(cur_obs[:, :6]) bit for bit — the forward reads the
    6-column prefix of the 8-column rows in place.  70 envs: more than one 16-row tile, a ragged last one."""
    import ilswiss_amd as ia
    from ilswiss_amd import her
    from ilswiss_amd.envs import HipVectorEnv
    from ilswiss_amd.td3 import MlpGaussianNoisePolicy
    n = 70
    env = HipVectorEnv("point-reach", n, seed=2, ctx=ctx)
    pol = her.MlpGaussianAndEpsilonPolicy([64, 64], 4, 2, condition_dim=2, output_activation="tanh", init_w=0.5, ctx=ctx, seed=5)
    rb = ia.SimpleReplayBuffer(256, 8, 2, ctx=ctx)
    q, v = env.get_state()
    cur = np.concatenate([q[:, :2], v, q[:, 2:], q[:, :2]], 1).astype(np.float32)
    env.rollout_step(policy=pol, replay=rb, max_path_length=1000, deterministic=True)
    b = rb._gather(np.arange(n))
    assert _same(np.asarray(b["observations"], np.float32), cur)
    want = pol.get_actions(cur[:, :6], deterministic=True)
    got = np.asarray(b["actions"], np.float32)
    assert _same(got, want) and np.abs(got).max() > 0.05 and len({tuple(r) for r in got.tolist()}) == n
    q2, v2 = env.get_state()
    assert _same(v2, (np.float32(0.1) * np.clip(got, -1, 1)).astype(np.float64))          # ... and they are what the stepper took
    # evaluation goes through the same prefix
    from ilswiss_amd.samplers import DeviceEvalSampler
    st = DeviceEvalSampler(env, ia.MakeDeterministic(pol), n, 3).obtain_statistics()
    assert st["Num Paths"] == n and np.isfinite(st["AverageReturn"]) and env.goal_success().shape == (n,)
    for bad in (MlpGaussianNoisePolicy([64, 64], 8, 2, output_activation="tanh", ctx=ctx), MlpGaussianNoisePolicy([64, 64], 4, 2, ctx=ctx)):
        with pytest.raises(RuntimeError, match="observation . desired_goal = 6 columns"):
            env.rollout_step(policy=bad, max_path_length=1000, deterministic=True)
    env.close()


def test_what_a_goal_env_refuses(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd import _lib, her
    from ilswiss_amd.envs import HipVectorEnv
    from ilswiss_amd.ppo import PPO, ReparamMultivariateGaussianPolicy
    lib = ctx.lib
    env = HipVectorEnv("point-reach", 4, seed=2, ctx=ctx)
    UNSUPPORTED, ARG = _lib.ILSX_ERR_UNSUPPORTED, -1
    assert lib.ilsx_vecenv_obs_norm(env.h, 1, 1) == UNSUPPORTED and b"goal env" in lib.ilsx_last_error()
    assert lib.ilsx_vecenv_obs_norm(env.h, 0, 0) == 0
    sh, sc = np.zeros(8), np.ones(8)
    assert lib.ilsx_vecenv_set_obs_affine(env.h, sh.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p)) == UNSUPPORTED
    pol = her.MlpGaussianAndEpsilonPolicy([64, 64], 4, 2, condition_dim=2, output_activation="tanh", ctx=ctx)
    rb = ia.SimpleReplayBuffer(64, 8, 2, ctx=ctx)
    vp = C.c_void_p
    envs, pis, rbs, mins = (vp * 1)(env.h), (vp * 1)(pol.h), (vp * 1)(rb.h), (C.c_int64 * 1)(0)
    assert lib.ilsx_rollout_steps_lockstep(envs, pis, rbs, 1, 1, 5, mins, 0, 0) == UNSUPPORTED
    st = (C.c_double * 18)()
    assert lib.ilsx_eval_rollouts_lockstep(envs, pis, 1, 5, 1, 4, st) == UNSUPPORTED
    ppo = PPO(ReparamMultivariateGaussianPolicy([64, 64], 8, 2, conditioned_std=False, hidden_activation="tanh", ctx=ctx),
              ia.FlattenMlp([64, 64], 1, 8, hidden_activation="tanh", ctx=ctx), mini_batch_size=16, update_epoch=1, max_samples=64)
    with pytest.raises(RuntimeError, match="goal env"):
        ppo.train_from_rollout(env, 2, 5)
    assert lib.ilsx_eval_rollout(env.h, None, ppo.h, 5, 1, 1, st) == UNSUPPORTED
    # a goal env's constants are refused before anything is allocated
    n0 = C.c_size_t()
    lib.ilsx_debug_ctx_allocs(ctx.h, C.byref(n0))
    for bad in (dict(tol=0.0), dict(tol=float("nan")), dict(step_scale=-0.1), dict(p_range=float("inf")), dict(g_range=0.0), dict(reward_kind=2)):
        m = dict(tol=0.1, step_scale=0.1, p_range=0.5, g_range=0.8, reward_kind=0)
        m.update(bad)
        ms, h = _lib.GoalModel(m["tol"], m["step_scale"], m["p_range"], m["g_range"], m["reward_kind"], 0), vp()
        assert lib.ilsx_vecenv_create_goal(ctx.h, C.byref(ms), 4, C.c_uint64(1), C.byref(h)) == ARG and not h.value, bad
    n1 = C.c_size_t()
    lib.ilsx_debug_ctx_allocs(ctx.h, C.byref(n1))
    assert n1.value == n0.value
    d = C.c_int()
    hop = HipVectorEnv("hopper", 2, seed=1, ctx=ctx)
    assert lib.ilsx_vecenv_goal_dims(hop.h, C.byref(d), C.byref(d)) != 0
    hop.close(), env.close()


# ---------------------------------------------------------------------------------------------- exploration
KW = dict(max_sigma=0.4, min_sigma=0.1, decay_period=1000.0, low=-1.0, high=1.0)


def _explore(env, act, eps, u, t, plain=False):
    from ilswiss_amd import _lib
    a, e = env.ctx.from_numpy(act, np.float32), env.ctx.from_numpy(eps, np.float64)
    if plain:
        _lib.check(env.ctx.lib.ilsx_vecenv_explore(env.h, a.ptr, e.ptr, int(t)))
    else:
        ud = env.ctx.from_numpy(u, np.float64)
        _lib.check(env.ctx.lib.ilsx_vecenv_explore_u(env.h, a.ptr, e.ptr, ud.ptr, int(t)))
    return a.numpy()


def test_epsilon_uniform_branch_of_the_gaussian_strategy(ctx):
    from ilswiss_amd import _lib, her
    from ilswiss_amd.envs import HipVectorEnv
    n, a = 300, 2
    env = HipVectorEnv("point-reach", n, seed=4, ctx=ctx)
    lib = ctx.lib
    assert lib.ilsx_vecenv_set_exploration_epsilon(env.h, 0.3) != 0                       # no Gaussian strategy installed yet
    cfg = _lib.ExploreCfg(1, 0, 0.0, 0.0, KW["max_sigma"], KW["min_sigma"], KW["decay_period"], KW["low"], KW["high"])
    _lib.check(lib.ilsx_vecenv_set_exploration(env.h, C.byref(cfg)))
    assert lib.ilsx_vecenv_set_exploration_epsilon(env.h, 1.5) != 0 and lib.ilsx_vecenv_set_exploration_epsilon(env.h, -0.1) != 0
    rng = np.random.default_rng(11)
    act = np.tanh(rng.normal(0, 1, (n, a))).astype(np.float32)
    eps, u = rng.normal(0, 1, (n, a)), rng.random((n, 1 + a))
    today = _explore(env, act, eps, None, 250, plain=True)                                # epsilon = 0: the strategy as it was
    assert _same(today, R.explore_step(act, eps, u, 0.0, t=250, **KW))
    for e in (0.0, 0.3, 1.0):
        _lib.check(lib.ilsx_vecenv_set_exploration_epsilon(env.h, e))
        got = _explore(env, act, eps, u, 250)
        assert _same(got, R.explore_step(act, eps, u, e, t=250, **KW)), e
        if e == 0.0:
            assert _same(got, today) and _same(_explore(env, act, eps, None, 250, plain=True), today)
        if e == 1.0:
            assert (got >= -1).all() and (got <= 1).all() and len({tuple(r) for r in got.tolist()}) == n
        if e == 0.3:
            assert not _same(got, today)
    # Philox draws: every action in range, no two envs alike, two calls differ
    x, y = (_explore_philox(env, act) for _ in range(2))
    assert (np.abs(x) <= 1).all() and len({tuple(r) for r in x.tolist()}) == n and not _same(x, y)
    # the policy binds its knobs to the env and forwards t
    pol = her.MlpGaussianAndEpsilonPolicy([64, 64], 4, 2, condition_dim=2, epsilon=1.0, max_sigma=0.4, min_sigma=0.1, decay_period=1000,
                                          output_activation="tanh", ctx=ctx)
    pol.install(env)
    pol.set_num_steps_total(250)
    got = _explore(env, act, eps, u, 250)
    assert _same(got, R.explore_step(act, eps, u, 1.0, t=250, **KW))
    env.close()


def _explore_philox(env, act):
    from ilswiss_amd import _lib
    a = env.ctx.from_numpy(act, np.float32)
    _lib.check(env.ctx.lib.ilsx_vecenv_explore_u(env.h, a.ptr, None, None, 250))
    return a.numpy()
