"""GPU suite for the cart-and-poles steppers of the classic-control engine (InvertedPendulum / InvertedDoublePendulum, k_cartchain_step /
k_cartchain_reset of csrc/classic_env.h) against the numpy restatement in tests/cartchain_restatement.py: dims, spaces, state access,
the fused rollout (auto-reset, replay records, episode bookkeeping, the device's random actions), the limit rows, the constraint-force
columns, the action clip, path mode, the device terminal predicates on the device's own records, policy rollouts, evaluation, observation
normalisation and the refusal of a categorical policy.

As in test_pendulum_hip.py the rollout test restates every step from the device's own previous state, so a difference cannot build up.
The states are not bit-identical: the kernel's closed-form Cholesky and np.linalg.solve round differently, and so do the two libms' sin
and cos.  The largest relative state difference per step, |got - want| / max(1, |want|), was measured on the first GPU run and is kept in
profiles/cartchain_parity.json; every state comparison here holds at 100x that figure, capped at 1e-9 (STATE_TOL).  A done flag may
differ from the restatement's only where the restatement's |theta| - 0.2 or y_tip - 1 lies within 4 * STATE_TOL of zero (a relative state
error e moves theta by e * max(1, |theta|) and y_tip by at most 2 * 1.2 * e), for at most 0.5 % of the steps (the issue's wording is
"within that state tolerance"; the factor 4 is the worst case just given).  test_cartchain_cpu.py checks on the restatement, with numpy's
generator in place of the device's Philox draws, that this protocol stays under that share; the first GPU run excused 0 steps."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import cartchain_restatement as cr  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("invertedpendulum", "inverteddoublependulum")
TERM = dict(invertedpendulum="inverted_pendulum", inverteddoublependulum="inverted_double_pendulum")
F32 = dict(rtol=2.5e-7, atol=1e-12)     # float32 values of float64 quantities that agree to STATE_TOL: at most an ulp or two apart


def state_tol():
    p = json.load(open(os.path.join(ROOT, "profiles", "cartchain_parity.json")))
    return min(100.0 * max(p["max_rel_state_diff"].values()), 1e-9)


def _env(ctx, name, n, seed=3, **kw):
    from ilswiss_amd.envs import HipVectorEnv
    return HipVectorEnv(name, n, seed=seed, ctx=ctx, **kw)


def _chain(name):
    from ilswiss_amd.envs.models_cartchain import MODELS_CARTCHAIN
    return cr.CartChain(MODELS_CARTCHAIN[name]())


def _rel(got, want):
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def _in_reset_range(c, q, v):
    if c.n == 2:
        return np.all(np.abs(q) <= 0.01, 1) & np.all(np.abs(v) <= 0.01, 1)
    return np.all(np.abs(q) <= 0.1, 1) & np.all(np.abs(v) < 0.1 * 9.0, 1)      # Box-Muller on 32-bit draws: |z| < sqrt(2 ln 2^33) = 6.8


@pytest.mark.parametrize("name", NAMES)
def test_dims_spaces_and_state_round_trip(ctx, name):
    from ilswiss_amd.envs.vecenv import Box
    c = _chain(name)
    env = _env(ctx, name, 300)
    assert (env.obs_dim, env.act_dim, env.nq, env.nv, env.discrete_n) == (c.obs_dim, 1, c.n, c.n, 0)
    ac = env.action_space[0]
    assert isinstance(ac, Box) and ac.shape == (1,) and np.array_equal(ac.low, [-1.0]) and np.array_equal(ac.high, [1.0])
    assert env.observation_space[0].shape == (c.obs_dim,)
    obs = env.reset()
    q, v = env.get_state()
    assert np.all(_in_reset_range(c, q, v)) and q.std() > (0.004 if c.n == 2 else 0.04)
    if c.n == 3:
        assert 0.08 < v.std() < 0.12 and np.all(obs[:, 8:] == 0.0)       # qvel = 0.1 N(0, 1); no constraint force after a reset
    np.testing.assert_allclose(obs.astype(np.float32), c.observe(q, v), **F32)
    assert not np.array_equal(env.reset(), obs)                            # a new Philox counter: other states
    rng = np.random.default_rng(4)
    q, v = rng.uniform(-0.9, 0.9, (300, c.n)), rng.uniform(-3, 3, (300, c.n))
    env.set_state(q, v)
    gq, gv = env.get_state()
    assert np.array_equal(gq, q) and np.array_equal(gv, v)
    with pytest.raises(NotImplementedError):
        _env(ctx, name, 4, obs_shift=np.zeros(c.obs_dim), obs_scale=np.ones(c.obs_dim))
    env.close()


def run_parity(ctx, name, tol):
    """64 envs, 200 auto-resetting steps with the device's random actions; every step restated from the device's previous state.
    Returns the figures (largest relative state difference, excused done flags, ...); asserts everything at `tol`."""
    import ilswiss_amd as ia
    from ilswiss_amd.envs.terminals import get_terminal_func
    c = _chain(name)
    n, T, maxlen = 64, 200, 1000
    env = _env(ctx, name, n, seed=11)
    env.rollout_stats(reset=True)
    rb = ia.SimpleReplayBuffer(n, c.obs_dim, 1, ctx=ctx)       # capacity n: step t's record of env i sits at slot i
    is_terminal = get_terminal_func(TERM[name])
    ep_len, ep_ret = np.zeros(n, int), np.zeros(n)
    pq, pv = env.get_state()
    pfrc = np.zeros_like(pv)
    worst, excused, pred_excused, episodes, ret_sum, lens = 0.0, 0, 0, 0, 0.0, []
    amin, amax = 1.0, -1.0
    for t in range(T):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
        rec = rb._gather(np.arange(n))
        a = rec["actions"][:, 0]
        assert np.all(a > -1) and np.all(a < 1)                 # Box(-1, 1).sample(), stored unmapped
        amin, amax = min(amin, a.min()), max(amax, a.max())
        wq, wv, wfrc, wobs, wrew, wdone = c.step(pq, pv, a)
        np.testing.assert_allclose(rec["observations"], c.observe(pq, pv, pfrc), **F32, err_msg=f"step {t}")
        np.testing.assert_allclose(rec["next_observations"], wobs, **F32, err_msg=f"step {t}")
        np.testing.assert_allclose(rec["rewards"][:, 0], wrew.astype(np.float32), **F32, err_msg=f"step {t}")
        done = rec["terminals"][:, 0].astype(bool)
        near = np.abs(c.margin(wq)) <= 4.0 * tol
        assert np.array_equal(done[~near], wdone[~near]), t
        excused += int(np.sum(done != wdone))
        # the device predicate (MBPO's labels) on the device's own record
        pred = np.asarray(is_terminal(None, None, rec["next_observations"], ctx=ctx))[:, 0].astype(bool)
        assert np.array_equal(pred[~near], done[~near]), (t, np.abs(c.margin(wq))[pred != done])
        pred_excused += int(np.sum(pred != done))
        ep_len += 1
        ep_ret += wrew
        end = done | (ep_len >= maxlen)
        gq, gv = env.get_state()
        keep = ~end
        worst = max(worst, float(_rel(gq[keep], wq[keep]).max(initial=0.0)), float(_rel(gv[keep], wv[keep]).max(initial=0.0)))
        assert worst <= tol, (t, worst)
        assert np.all(_in_reset_range(c, gq[end], gv[end])), t          # the ended envs were reset ...
        episodes += int(end.sum())
        ret_sum += float(ep_ret[end].sum())
        lens += list(ep_len[end])
        ep_len[end], ep_ret[end] = 0, 0.0
        pq, pv = gq, gv
        pfrc = np.where(end[:, None], 0.0, wfrc)                         # ... and show no constraint force
    e, r = env.rollout_stats(reset=True)
    assert e == episodes and episodes > n                                # random play drops the pole(s) within tens of steps
    np.testing.assert_allclose(r, ret_sum, rtol=1e-9)                    # float64 returns of states that agree to `tol`
    assert amin < -0.95 and amax > 0.95
    assert excused <= 0.005 * n * T and pred_excused <= 0.005 * n * T
    env.close()
    return dict(max_rel_state_diff=worst, excused_done=excused, excused_predicate=pred_excused, steps=n * T, episodes=episodes,
                mean_episode_length=float(np.mean(lens)), mean_return=ret_sum / episodes)


@pytest.mark.parametrize("name", NAMES)
def test_rollout_steps_match_the_restatement(ctx, name):
    fig = run_parity(ctx, name, state_tol())
    print(name, fig)


def limit_cases(name):
    """(q, v, action) rows that switch limit rows on: the slide just inside its upper limit moving out (the row comes on inside the step),
    and for InvertedPendulum the hinge just outside 90 degrees, and both rows at once on either side."""
    if name == "invertedpendulum":
        q = np.array([[0.999, 0.0], [0.0, 1.5709], [1.002, 1.575], [-1.003, -1.58], [0.2, 0.1]])
        v = np.array([[2.0, 0.0], [0.0, 1.0], [1.0, 2.0], [-1.0, -1.0], [0.0, 0.0]])
    else:
        q = np.array([[0.999, 0.05, -0.03], [1.02, 0.3, 0.2], [-1.004, -0.2, 0.4], [0.1, 0.02, 0.01]])
        v = np.array([[2.0, 0.0, 0.0], [1.0, 12.0, -15.0], [-3.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    a = np.where(q[:, 0] > 0.9, 0.9, np.where(q[:, 0] < -0.9, -0.9, 0.0)).astype(np.float32)     # the actuator pushes the cart into its limit
    return q, v, a


def run_limits(ctx, name, tol):
    import ilswiss_amd as ia
    c = _chain(name)
    q, v, a = limit_cases(name)
    n = len(q)
    env = _env(ctx, name, n, seed=5)
    worst = 0.0
    for mode in ("step", "rollout"):
        env.reset()
        env.set_state(q, v)
        wq, wv, wfrc, wobs, wrew, wdone = c.step(q, v, a)
        if mode == "step":
            obs, rew, done, _ = env.step(a.reshape(n, 1))
            obs = obs.astype(np.float32)
        else:       # the fused step with no_terminal: a pole beyond 0.2 rad goes on
            rb = ia.SimpleReplayBuffer(n, c.obs_dim, 1, ctx=ctx)
            env.rollout_step(replay=rb, max_path_length=1000, random_actions=True, no_terminal=True)
            rec = rb._gather(np.arange(n))
            wq, wv, wfrc, wobs, wrew, wdone = c.step(q, v, rec["actions"][:, 0])
            obs, rew, done = rec["next_observations"], rec["rewards"][:, 0], wdone
            assert not rec["terminals"].any()
        gq, gv = env.get_state()
        worst = max(worst, float(_rel(gq, wq).max()), float(_rel(gv, wv).max()))
        assert worst <= tol, (mode, worst)
        np.testing.assert_allclose(obs, wobs, **F32)
        np.testing.assert_allclose(np.asarray(rew, np.float32), wrew.astype(np.float32), **F32)
        assert np.array_equal(np.asarray(done, bool), wdone)
        if mode == "rollout":
            continue
        # the rows are on inside the step in every case but the last; at its last stage the InvertedPendulum cart of case 0 is already on
        # its way back (the row only pushes: f = 0), every other case ends with a row pushing
        assert np.all(np.any(wfrc[1:-1] != 0.0, 1)) and np.all(wfrc[-1] == 0.0) and wq[0, 0] > 1.0
        if c.n == 3:
            assert np.all(obs[:-1, 8] != 0.0) and np.all(obs[:, 9:] == 0.0) and np.all(obs[-1, 8:] == 0.0)
            assert obs[1, 8] == -10.0 and abs(wfrc[1, 0]) > 10.0                     # the +-10 clip on qfrc_constraint ...
            assert np.abs(obs[1, 5:8]).max() == 10.0 and np.abs(wv[1]).max() > 10.0  # ... and on qvel
        else:
            assert np.all(wfrc[2] != 0.0) and np.all(wfrc[3] != 0.0)                 # both rows pushing
    env.close()
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_limit_rows_match_the_restatement(ctx, name):
    print(name, "limit rows: largest relative state difference", run_limits(ctx, name, state_tol()))


@pytest.mark.parametrize("name", NAMES)
def test_builtin_constants_are_the_python_model(ctx, name):
    """ilsx_vecenv_create_classic(kind) fills the model from the library's built-in constants; HipVectorEnv passes models_cartchain.py."""
    import ctypes as C
    from ilswiss_amd import _lib
    from ilswiss_amd.device import as_dev, host_ptr
    from ilswiss_amd.envs import CARTCHAIN
    env = _env(ctx, name, 4, seed=5)
    q, v, a = limit_cases(name)
    q, v, a = q[:4], v[:4], a[:4]
    env.set_state(q, v)
    env.step(a.reshape(4, 1))
    want = env.get_state()
    h = C.c_void_p()
    _lib.check(ctx.lib.ilsx_vecenv_create_classic(ctx.h, CARTCHAIN[name], 4, C.c_uint64(5), C.byref(h)))
    keep, pa = as_dev(ctx, a.reshape(4, 1))
    gq, gv = np.empty_like(q), np.empty_like(v)
    _lib.check(ctx.lib.ilsx_vecenv_set_state(h, host_ptr(np.ascontiguousarray(q)), host_ptr(np.ascontiguousarray(v))))
    _lib.check(ctx.lib.ilsx_vecenv_step(h, pa, None, 4, None, None, None))
    _lib.check(ctx.lib.ilsx_vecenv_get_state(h, host_ptr(gq), host_ptr(gv)))
    ctx.lib.ilsx_vecenv_destroy(h)
    del keep
    assert _rel(gq, want[0]).max() <= 1e-13 and _rel(gv, want[1]).max() <= 1e-13    # the same constants up to the rounding of their derivation
    env.close()


@pytest.mark.parametrize("name", NAMES)
def test_actions_outside_the_box_are_clipped(ctx, name):
    c = _chain(name)
    env = _env(ctx, name, 6)
    rng = np.random.default_rng(5)
    q, v = rng.uniform(-0.1, 0.1, (6, c.n)), rng.uniform(-1, 1, (6, c.n))
    a = np.array([3.0, -3.0, 1.5, -1.0001, 100.0, -1e6], np.float32)
    res = []
    for act in (a, np.clip(a, -1, 1)):
        env.set_state(q, v)
        obs, rew, done, _ = env.step(act.reshape(6, 1))
        res.append((env.get_state(), rew, obs, done))
    for x, y in zip(res[0], res[1]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    wq, wv, *_ = c.step(q, v, a)
    assert _rel(res[0][0][0], wq).max() <= state_tol() and _rel(res[0][0][1], wv).max() <= state_tol()
    env.close()


@pytest.mark.parametrize("name", NAMES)
def test_path_mode_inserts_whole_episodes(ctx, name):
    import ilswiss_amd as ia
    c = _chain(name)
    n, maxlen = 128, 20
    env = _env(ctx, name, n, seed=5)
    env.set_path_mode(True)
    rb = ia.SimpleReplayBuffer(1 << 15, c.obs_dim, 1, ctx=ctx)
    for _ in range(60):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
    size, _ = rb._cursors()
    assert len(rb._traj_endpoints) >= 3 * n and size == sum(e - s for s, e in rb._traj_endpoints.items())
    b = rb._gather(np.arange(size))
    n_term = 0
    for s, e in rb._traj_endpoints.items():
        rows = np.arange(s, e)
        obs, nobs, term = b["observations"][rows], b["next_observations"][rows], b["terminals"][rows, 0]
        assert 1 <= rows.size <= maxlen
        assert np.array_equal(obs[1:], nobs[:-1])                       # one env's consecutive steps
        assert not term[:-1].any() and (term[-1] or rows.size == maxlen)
        n_term += int(term[-1])
        first = obs[0]                                                   # starts from a reset state
        assert (np.abs(first).max() <= 0.01 + 1e-7) if c.n == 2 else (abs(first[0]) <= 0.1 + 1e-7 and np.all(first[8:] == 0.0))
    assert n_term > 0
    env.close()


@pytest.mark.parametrize("name", NAMES)
def test_policy_rollout_and_evaluation(ctx, name):
    import ilswiss_amd as ia
    from ilswiss_amd.samplers import DeviceEvalSampler
    c = _chain(name)
    n = 64
    env = _env(ctx, name, n, seed=9)
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[64, 64], obs_dim=c.obs_dim, action_dim=1, ctx=ctx)
    pol.set_flat_params(pol.get_flat_params() * 3.0)   # a policy whose actions depend on the observation
    rb = ia.SimpleReplayBuffer(n, c.obs_dim, 1, ctx=ctx)
    env.reset()
    pq, pv = env.get_state()
    tol = state_tol()
    for t in range(10):
        env.rollout_step(policy=pol, replay=rb, max_path_length=1000, no_terminal=True)
        rec = rb._gather(np.arange(n))
        a = rec["actions"]
        assert np.all(np.abs(a) <= 1) and a.std() > 1e-3
        wq, wv, _, wobs, wrew, _ = c.step(pq, pv, a[:, 0])
        gq, gv = env.get_state()
        assert _rel(gq, wq).max() <= tol and _rel(gv, wv).max() <= tol
        np.testing.assert_allclose(rec["rewards"][:, 0], wrew.astype(np.float32), **F32)
        pq, pv = gq, gv
    det = ia.MakeDeterministic(pol)
    for p in (det, pol):
        st = DeviceEvalSampler(env, p, 400, 200).obtain_statistics()
        assert st["Num Paths"] >= 2 and np.isfinite(st["AverageReturn"]) and st["AverageReturn"] > 0.0
        assert 1 <= st["Test Ep. Len. Min"] <= st["Test Ep. Len. Max"] <= 200
        assert st["Test Rewards Max"] <= (1.0 if c.n == 2 else 10.0)
        assert -1.0 <= st["Test Actions Min"] <= st["Test Actions Max"] <= 1.0
    env.close()


@pytest.mark.parametrize("name", NAMES)
def test_norm_obs_running_statistics(ctx, name):
    n = 256
    env = _env(ctx, name, n, seed=2, norm_obs=True)
    raw = _env(ctx, name, n, seed=2)
    rms = env.obs_rms
    rng = np.random.default_rng(0)
    for _ in range(3):
        a = rng.uniform(-1, 1, (n, 1)).astype(np.float32)
        raw.set_state(*env.get_state())
        o_raw = raw.step(a)[0]
        o = env.step(a)[0]
        m, v, cnt = rms.mean, rms.var, rms.count
        assert cnt > 0 and np.all(v >= 0) and np.all(v[:4] > 0)
        np.testing.assert_allclose(o, np.clip((o_raw - m) / np.sqrt(v + np.finfo(np.float32).eps), -10, 10), rtol=1e-5, atol=1e-5)
    env.close(), raw.close()


@pytest.mark.parametrize("name", NAMES)
def test_categorical_policy_is_refused(ctx, name):
    import ilswiss_amd as ia
    from ilswiss_amd.samplers import DeviceEvalSampler
    c = _chain(name)
    env = _env(ctx, name, 8, seed=2)
    cat = ia.DiscretePolicy(hidden_sizes=[64, 64], obs_dim=c.obs_dim, action_dim=3, ctx=ctx)
    with pytest.raises(RuntimeError, match="categorical policy on an env with a Box"):
        env.rollout_step(policy=cat, max_path_length=200)
    with pytest.raises(RuntimeError, match="categorical policy on an env with a Box"):
        DeviceEvalSampler(env, ia.MakeDeterministic(cat), 10, 10).obtain_statistics()
    env.close()


def test_envpool_names_build(ctx):
    from ilswiss_amd.envs.envpool import HipEnvPool
    for task, o in (("InvertedPendulum-v2", 4), ("InvertedDoublePendulum-v2", 11)):
        e = HipEnvPool(task, num_envs=3, seed=1, ctx=ctx)
        assert e.obs_dim == o and e.reset().shape == (3, o)
        e.close()
