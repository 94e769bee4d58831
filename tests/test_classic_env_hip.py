"""GPU suite for the classic-control engine (csrc/classic_env.h): the CartPole stepper against the float64 restatement of gym 0.22's
CartPoleEnv (tests/dsac_restatement.py) through the fused rollout — auto-reset, replay records, episode bookkeeping, random actions —
and path mode with the 1-wide action column.

The rollout test is NOT a bit-identity test over a free-running trajectory: the actions are the device's own uniform draws (read back
from the replay records), and every step is restated from the device's own previous state, so a difference cannot build up.  Within a
step the float64 states agree bit for bit except where ROCm's and glibc's double sin / cos differ by an ulp (measured: 696 of 4.7 M
components over the 300 steps); there they agree to 1e-14 relative, and at most 0.1 % of the components may differ.  Observations,
rewards, dones, episode lengths and returns agree exactly."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from dsac_restatement import cartpole_step  # noqa: E402

pytestmark = pytest.mark.gpu


def _env(ctx, n, seed=3):
    from ilswiss_amd.envs import HipVectorEnv
    return HipVectorEnv("cartpole", n, seed=seed, ctx=ctx)


def _state(env):
    q, v = env.get_state()
    return np.stack([q[:, 0], v[:, 0], q[:, 1], v[:, 1]], 1)   # (x, x_dot, theta, theta_dot)


def test_spaces_dims_and_reset_range(ctx):
    from ilswiss_amd.envs import Discrete
    env = _env(ctx, 4096)
    assert (env.obs_dim, env.act_dim, env.nq, env.nv) == (4, 1, 2, 2)
    assert isinstance(env.action_space[0], Discrete) and env.action_space[0].n == 2
    obs = env.reset()
    s = _state(env)
    assert np.all(s >= -0.05) and np.all(s < 0.05) and s.std() > 0.02
    assert np.array_equal(obs.astype(np.float32), s.astype(np.float32))
    env.close()


def test_rollout_steps_match_restatement_up_to_libm_ulps(ctx):
    import ilswiss_amd as ia
    n, T, maxlen = 4096, 300, 200
    env = _env(ctx, n)
    rng = np.random.default_rng(11)
    s0 = np.stack([rng.uniform(-2.3, 2.3, n), rng.uniform(-1, 1, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-1, 1, n)], 1)
    env.set_state(np.stack([s0[:, 0], s0[:, 2]], 1), np.stack([s0[:, 1], s0[:, 3]], 1))
    env.rollout_stats(reset=True)
    rb = ia.SimpleReplayBuffer(n, 4, 1, ctx=ctx)   # capacity n: step t's record of env i sits at slot i
    ep_len, ep_ret = np.zeros(n, int), np.zeros(n)
    prev = _state(env)
    episodes, ret_sum, acts_seen, mism, checked = 0, 0.0, set(), 0, 0
    for t in range(T):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
        rec = rb._gather(np.arange(n))
        a = rec["actions"][:, 0]
        assert set(np.unique(a).tolist()) <= {0.0, 1.0}
        acts_seen |= set(np.unique(a).tolist())
        want, rew, done = cartpole_step(prev, a.astype(np.int64))
        assert np.array_equal(rec["observations"], prev.astype(np.float32))
        assert np.array_equal(rec["next_observations"], want.astype(np.float32))
        assert np.all(rec["rewards"][:, 0] == 1.0) and np.array_equal(rec["terminals"][:, 0].astype(bool), done)
        ep_len += 1
        ep_ret += rew
        end = done | (ep_len >= maxlen)
        got = _state(env)
        keep = ~end
        mism += int(np.sum(got[keep] != want[keep]))
        checked += int(keep.sum()) * 4
        # the device's double sin / cos (ROCm's libm) and Python's (glibc) differ by an ulp on a few arguments: those steps agree to
        # rounding, every other one bit for bit
        assert np.all(np.abs(got[keep] - want[keep]) <= 1e-14 * np.maximum(1.0, np.abs(want[keep]))), t
        assert np.all(got[end] >= -0.05) and np.all(got[end] < 0.05)
        episodes += int(end.sum())
        ret_sum += float(ep_ret[end].sum())
        ep_len[end], ep_ret[end] = 0, 0.0
        prev = got
    assert mism <= 1e-3 * checked, f"{mism} of {checked} float64 state components differ from the restatement"
    assert acts_seen == {0.0, 1.0}
    e, r = env.rollout_stats(reset=True)
    assert e == episodes and r == ret_sum and episodes > n   # random play ends ~ every 20 steps
    env.close()


def test_path_mode_inserts_whole_episodes(ctx):
    import ilswiss_amd as ia
    n, maxlen = 256, 50
    env = _env(ctx, n, seed=5)
    env.set_path_mode(True)
    rb = ia.SimpleReplayBuffer(1 << 16, 4, 1, ctx=ctx)
    for _ in range(120):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
    size, _ = rb._cursors()
    assert size > 0 and rb._traj_endpoints
    b = rb._gather(np.arange(size))
    for s, e in rb._traj_endpoints.items():
        rows = np.arange(s, e)
        assert 1 <= rows.size <= maxlen
        obs, nobs, term = b["observations"][rows], b["next_observations"][rows], b["terminals"][rows, 0]
        assert np.array_equal(obs[1:], nobs[:-1])                       # one env's consecutive steps
        assert not term[:-1].any() and (term[-1] == 1 or rows.size == maxlen)
        assert set(np.unique(b["actions"][rows, 0]).tolist()) <= {0.0, 1.0}
        assert np.all(np.abs(obs[0]) < 0.05)                            # starts from a reset state
    env.close()


def test_eval_rollout_with_categorical_policy(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.samplers import DeviceEvalSampler
    env = _env(ctx, 16, seed=9)
    pol = ia.DiscretePolicy(hidden_sizes=[64, 64], obs_dim=4, action_dim=2, ctx=ctx)
    pol.set_flat_params(pol.get_flat_params() * 3.0)   # a policy whose actions depend on the observation
    det = ia.MakeDeterministic(pol)
    runs = []
    for p in (det, det, pol):
        st = DeviceEvalSampler(env, p, 400, 200).obtain_statistics()
        assert st["Num Paths"] >= 16 and np.isfinite(st["AverageReturn"])
        assert 1 <= st["Test Ep. Len. Min"] <= st["Test Ep. Len. Max"] <= 200
        assert st["Test Rewards Min"] == st["Test Rewards Max"] == 1.0             # CartPole pays 1 per step, the last one included
        assert st["Test Returns Mean"] == st["Test Ep. Len. Mean"]                 # so a return IS an episode length
        assert 0.0 <= st["Test Actions Min"] <= st["Test Actions Max"] <= 1.0    # indices of Discrete(2)
        runs.append(st)
    # evaluation resets every env from the env's Philox stream at a new counter, so repeats see other start states: the deterministic
    # policy's average return stays in CartPole's range either way, and both runs covered the requested steps
    assert all(r["Num Paths"] * r["Test Ep. Len. Mean"] >= 400 for r in runs)
    env.close()


def test_action_space_kind_must_match_the_policy(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    cart = _env(ctx, 8, seed=2)
    gauss = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[64, 64], obs_dim=4, action_dim=1, ctx=ctx)
    with pytest.raises(RuntimeError, match="continuous policy on an env with a Discrete"):
        cart.rollout_step(policy=gauss, max_path_length=200)
    hop = HipVectorEnv("hopper", 8, seed=2, ctx=ctx)
    cat = ia.DiscretePolicy(hidden_sizes=[64, 64], obs_dim=hop.obs_dim, action_dim=3, ctx=ctx)
    with pytest.raises(RuntimeError, match="categorical policy on an env with a Box"):
        hop.rollout_step(policy=cat, max_path_length=200)
    from ilswiss_amd.samplers import DeviceEvalSampler
    with pytest.raises(RuntimeError, match="categorical policy on an env with a Box"):
        DeviceEvalSampler(hop, ia.MakeDeterministic(cat), 10, 10).obtain_statistics()
    cart.close(), hop.close()
