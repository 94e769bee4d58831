"""GPU suite for the Pendulum stepper of the classic-control engine (csrc/classic_env.h, ILSX_CLASSIC_PENDULUM) against the numpy
restatement of gym 0.22's PendulumEnv behind NormalizedBoxEnv (tests/pendulum_restatement.py): spaces, reset, state access, the fused
rollout (auto-reset, replay records, episode bookkeeping, the device's random actions), the action clip, path mode, policy-driven rollouts,
evaluation, observation normalisation, and the refusal of a categorical policy.

As in test_classic_env_hip.py, the rollout test restates every step from the device's own previous state, so a difference cannot build up.
The reward needs no libm (fmod is exact) and agrees bit for bit on every step; the float64 states agree bit for bit except where ROCm's and
glibc's double sin differ by an ulp, where they agree to 1e-14 relative (measured: 0.40 % of the components over the 300 steps; the bound
is 1 %).  Observations differ only where the states do."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pendulum_restatement as pr  # noqa: E402

pytestmark = pytest.mark.gpu


def _env(ctx, n, seed=3, **kw):
    from ilswiss_amd.envs import HipVectorEnv
    return HipVectorEnv("pendulum", n, seed=seed, ctx=ctx, **kw)


def _state(env):
    q, v = env.get_state()
    return np.stack([q[:, 0], v[:, 0]], 1)   # (theta, theta_dot)


def _set(env, s):
    env.set_state(s[:, :1].copy(), s[:, 1:].copy())


def test_spaces_and_dims(ctx):
    from ilswiss_amd.envs.vecenv import Box
    env = _env(ctx, 64)
    assert (env.obs_dim, env.act_dim, env.nq, env.nv) == (3, 1, 1, 1)
    assert env.discrete_n == 0
    ac = env.action_space[0]
    assert isinstance(ac, Box) and ac.shape == (1,) and np.array_equal(ac.low, [-1.0]) and np.array_equal(ac.high, [1.0])
    assert env.observation_space[0].shape == (3,)
    env.close()


def test_reset_range(ctx):
    env = _env(ctx, 4096)
    obs = env.reset()
    s = _state(env)
    assert np.all(s[:, 0] >= -np.pi) and np.all(s[:, 0] < np.pi) and np.all(s[:, 1] >= -1) and np.all(s[:, 1] < 1)
    assert s[:, 0].std() > 1.5 and s[:, 1].std() > 0.5          # U[-pi, pi): std 1.81; U[-1, 1): 0.577
    assert np.array_equal(obs.astype(np.float32), pr.observe(s))
    obs2 = env.reset()                                             # a new Philox counter: other states
    assert not np.array_equal(obs2, obs)
    env.close()


def test_get_and_set_state(ctx):
    env = _env(ctx, 1000)
    rng = np.random.default_rng(4)
    s = np.stack([rng.uniform(-20, 20, 1000), rng.uniform(-8, 8, 1000)], 1)
    _set(env, s)
    assert np.array_equal(_state(env), s)
    a = rng.uniform(-1, 1, (1000, 1)).astype(np.float32)
    obs, rew, done, _ = env.step(a)
    want, wrew, wobs = pr.pendulum_step(s, a)
    got = _state(env)
    assert np.all(np.abs(got - want) <= 1e-14 * np.maximum(1.0, np.abs(want)))
    same = np.all(got == want, 1)
    assert same.mean() > 0.97   # theta spread over +-20 rad: ~1 % of the sin values differ by an ulp (measured 0.99 agree)
    assert np.array_equal(rew.astype(np.float32), wrew.astype(np.float32)) and not done.any()
    assert np.array_equal(obs[same].astype(np.float32), wobs[same])
    env.close()


def test_rollout_steps_match_restatement_up_to_libm_ulps(ctx):
    import ilswiss_amd as ia
    n, T, maxlen = 4096, 300, 200
    env = _env(ctx, n)
    rng = np.random.default_rng(11)
    s0 = np.stack([rng.uniform(-4 * np.pi, 4 * np.pi, n), rng.uniform(-8, 8, n)], 1)
    _set(env, s0)
    env.rollout_stats(reset=True)
    rb = ia.SimpleReplayBuffer(n, 3, 1, ctx=ctx)   # capacity n: step t's record of env i sits at slot i
    ep_len, ep_ret = np.zeros(n, int), np.zeros(n)
    prev = _state(env)
    episodes, ret_sum, mism, checked, obs_mism = 0, 0.0, 0, 0, 0
    amin, amax = 1.0, -1.0
    for t in range(T):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
        rec = rb._gather(np.arange(n))
        a = rec["actions"][:, 0]
        assert np.all(a > -1) and np.all(a < 1)                    # Box(-1, 1).sample(), stored unmapped
        amin, amax = min(amin, a.min()), max(amax, a.max())
        want, rew, wobs = pr.pendulum_step(prev, a)
        assert np.array_equal(rec["observations"], pr.observe(prev)), t
        assert np.array_equal(rec["rewards"][:, 0], rew.astype(np.float32)), t
        assert not rec["terminals"].any()
        ep_len += 1
        ep_ret += rew
        end = ep_len >= maxlen
        got = _state(env)
        keep = ~end
        # ROCm's double sin and glibc's differ by an ulp on a few arguments: those steps agree to rounding, every other one bit for bit
        assert np.all(np.abs(got[keep] - want[keep]) <= 1e-14 * np.maximum(1.0, np.abs(want[keep]))), t
        mism += int(np.sum(got[keep] != want[keep]))
        checked += int(keep.sum()) * 2
        same = keep & np.all(got == want, 1)
        assert np.array_equal(rec["next_observations"][same], wobs[same]), t
        # the ended envs' post-step states were replaced by resets: their records agree with the restatement to float32 rounding
        np.testing.assert_allclose(rec["next_observations"][end], wobs[end], rtol=0, atol=1e-6)
        obs_mism += int(np.sum(rec["next_observations"][end] != wobs[end]))
        assert np.all(got[end, 0] >= -np.pi) and np.all(got[end, 0] < np.pi) and np.all(np.abs(got[end, 1]) <= 1)
        episodes += int(end.sum())
        ret_sum += float(ep_ret[end].sum())
        ep_len[end], ep_ret[end] = 0, 0.0
        prev = got
    # measured: 9891 of 2.45 M components (0.40 %).  CartPole's bound (0.1 %) does not carry over: its sin / cos see |theta| < 0.21,
    # Pendulum's see the whole circle and beyond (theta is never wrapped), where the two libms disagree more often
    assert mism <= 1e-2 * checked, f"{mism} of {checked} float64 state components differ from the restatement"
    assert obs_mism <= 1e-3 * episodes * 3
    assert amin < -0.99 and amax > 0.99
    e, r = env.rollout_stats(reset=True)
    assert e == episodes == n and episodes > 0
    np.testing.assert_allclose(r, ret_sum, rtol=1e-12)           # a sum of per-env float64 returns in another order
    assert ret_sum / episodes < -100.0                              # random play on Pendulum pays heavily
    env.close()


def test_actions_outside_the_box_are_clipped(ctx):
    env = _env(ctx, 6)
    rng = np.random.default_rng(5)
    s = np.stack([rng.uniform(-3, 3, 6), rng.uniform(-2, 2, 6)], 1)
    a = np.array([3.0, -3.0, 1.5, -1.0001, 100.0, -1e6], np.float32)
    clipped = np.clip(a, -1, 1)
    res = []
    for act in (a, clipped):
        _set(env, s)
        obs, rew, done, _ = env.step(act.reshape(6, 1))
        res.append((_state(env), rew, obs))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    _, wrew, _ = pr.pendulum_step(s, a)
    assert np.array_equal(res[0][1].astype(np.float32), wrew.astype(np.float32))
    env.close()


def test_path_mode_inserts_whole_episodes(ctx):
    import ilswiss_amd as ia
    n, maxlen = 256, 50
    env = _env(ctx, n, seed=5)
    env.set_path_mode(True)
    rb = ia.SimpleReplayBuffer(1 << 16, 3, 1, ctx=ctx)
    for _ in range(120):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
    size, _ = rb._cursors()
    assert size == 2 * n * maxlen and len(rb._traj_endpoints) == 2 * n   # never done: every episode runs to the time limit
    b = rb._gather(np.arange(size))
    for s, e in rb._traj_endpoints.items():
        rows = np.arange(s, e)
        assert rows.size == maxlen
        obs, nobs, term = b["observations"][rows], b["next_observations"][rows], b["terminals"][rows, 0]
        assert np.array_equal(obs[1:], nobs[:-1])                       # one env's consecutive steps
        assert not term.any()
        assert np.all(np.abs(b["actions"][rows, 0]) < 1)
        assert abs(obs[0, 2]) < 1 and abs(np.hypot(obs[0, 0], obs[0, 1]) - 1) < 1e-6   # starts from a reset state
        np.testing.assert_allclose(b["rewards"][rows, 0], pr.pendulum_step(
            np.stack([np.arctan2(obs[:, 1], obs[:, 0]), obs[:, 2]], 1).astype(np.float64), b["actions"][rows])[1], rtol=0, atol=1e-4)
    env.close()


def test_policy_rollout_and_evaluation(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.samplers import DeviceEvalSampler
    n = 64
    env = _env(ctx, n, seed=9)
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[64, 64], obs_dim=3, action_dim=1, ctx=ctx)
    pol.set_flat_params(pol.get_flat_params() * 3.0)   # a policy whose actions depend on the observation
    rb = ia.SimpleReplayBuffer(n, 3, 1, ctx=ctx)
    env.reset()
    prev = _state(env)
    mism = 0
    for t in range(40):
        env.rollout_step(policy=pol, replay=rb, max_path_length=1000)
        rec = rb._gather(np.arange(n))
        a = rec["actions"]
        assert np.all(np.abs(a) <= 1) and a.std() > 1e-3
        want, rew, _ = pr.pendulum_step(prev, a)
        got = _state(env)
        assert np.array_equal(rec["rewards"][:, 0], rew.astype(np.float32))
        assert np.all(np.abs(got - want) <= 1e-14 * np.maximum(1.0, np.abs(want)))
        mism += int(np.sum(got != want))
        prev = got
    assert mism <= 1e-2 * 40 * n * 2
    det = ia.MakeDeterministic(pol)
    for p in (det, pol):
        st = DeviceEvalSampler(env, p, 400, 200).obtain_statistics()
        assert st["Num Paths"] >= 2 and np.isfinite(st["AverageReturn"])
        assert st["Test Ep. Len. Min"] == st["Test Ep. Len. Max"] == 200            # never done: the time limit ends every episode
        assert st["Test Rewards Max"] <= 0.0 and st["Test Rewards Min"] >= -(np.pi ** 2 + 0.1 * 64 + 0.001 * 4) - 1e-4
        assert -1.0 <= st["Test Actions Min"] <= st["Test Actions Max"] <= 1.0
        assert st["AverageReturn"] < 0.0
    env.close()


def test_norm_obs_running_statistics(ctx):
    n = 512
    env = _env(ctx, n, seed=2, norm_obs=True)
    raw = _env(ctx, n, seed=2)
    rms = env.obs_rms
    rng = np.random.default_rng(0)
    for _ in range(3):
        a = rng.uniform(-1, 1, (n, 1)).astype(np.float32)
        _set(raw, _state(env))
        o_raw = raw.step(a)[0]
        o = env.step(a)[0]
        m, v, c = rms.mean, rms.var, rms.count
        assert c > 0 and np.all(v > 0)
        np.testing.assert_allclose(o, np.clip((o_raw - m) / np.sqrt(v + np.finfo(np.float32).eps), -10, 10), rtol=1e-5, atol=1e-5)
    env.close(), raw.close()


def test_categorical_policy_is_refused(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.samplers import DeviceEvalSampler
    env = _env(ctx, 8, seed=2)
    cat = ia.DiscretePolicy(hidden_sizes=[64, 64], obs_dim=3, action_dim=3, ctx=ctx)
    with pytest.raises(RuntimeError, match="categorical policy on an env with a Box"):
        env.rollout_step(policy=cat, max_path_length=200)
    with pytest.raises(RuntimeError, match="categorical policy on an env with a Box"):
        DeviceEvalSampler(env, ia.MakeDeterministic(cat), 10, 10).obtain_statistics()
    env.close()
