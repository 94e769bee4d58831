"""GPU suite: k_envg_step / k_env_reset / the fused rollout step against the CPU oracle (float64)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _mk(ctx, name, n, seed=3):
    from ilswiss_amd.envs.vecenv import HipVectorEnv
    return HipVectorEnv(name, n, seed=seed, ctx=ctx)


@pytest.mark.parametrize("name", ["hopper", "walker", "halfcheetah"])
def test_step_matches_oracle(ctx, name):
    from oracle.planar_env import PlanarOracle
    env = _mk(ctx, name, 96)
    P = PlanarOracle(env.model)
    n, nd, na = 96, env.n_dof, env.act_dim
    rng = np.random.default_rng(7)
    obs0 = env.reset()
    q, v = env.get_state()
    # reset noise: init + U(+-0.005) on qpos/qvel (hopper.py:32-40), obs = qpos[1:] + clip(qvel); HalfCheetah: U(+-0.1), 0.1*randn
    nz = env.model["reset_noise"]
    assert np.all(np.abs(q - np.asarray(env.model["init_qpos"])) <= nz)
    if name == "halfcheetah":
        assert 0.07 < v.std() < 0.13 and abs(v.mean()) < 0.02 and np.abs(v).max() > 0.2
    else:
        assert np.all(np.abs(v) <= nz)
    np.testing.assert_allclose(obs0, np.concatenate([q[:, 1:], v], 1), atol=1e-6)
    assert len(np.unique(q[:, 1])) == n  # every env gets its own noise
    # spread the states: some airborne, some in deep contact, some beyond joint limits, some already unhealthy
    q[:, 1] += rng.uniform(-0.05, 0.6, n)
    q[:, 2] += rng.uniform(-0.25, 0.25, n)
    q[:, 3:] += rng.uniform(-1.0, 0.4, (n, nd - 3))
    v += rng.normal(0, 1.5, (n, nd))
    env.set_state(q, v)
    for it in range(4):
        act = rng.uniform(-1.4, 1.4, (n, na)).astype(np.float32)
        obs, rew, done, info = env.step(act)
        q1, v1 = env.get_state()
        for i in range(n):
            qo, vo, oo, ro, do = P.step(q[i].copy(), v[i].copy(), act[i])
            np.testing.assert_allclose(q1[i], qo, rtol=1e-8, atol=1e-9, err_msg=f"qpos env {i} it {it}")
            np.testing.assert_allclose(v1[i], vo, rtol=1e-7, atol=1e-7, err_msg=f"qvel env {i} it {it}")
            np.testing.assert_allclose(obs[i], oo, rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(rew[i], ro, rtol=1e-5, atol=1e-4)
            assert bool(done[i]) == bool(do), (i, it)
        assert info[5]["env_id"] == 5
        q, v = q1, v1
    assert not done.all() and (done.any() or name != "hopper")  # walker's healthy band is wide (walker2d.py:17-20)
    assert not (name == "halfcheetah" and done.any())             # HalfCheetah never terminates
    env.close()


def test_subset_step_and_reset(ctx):
    env = _mk(ctx, "hopper", 32)
    env.reset()
    q0, v0 = env.get_state()
    ids = np.array([3, 17, 30])
    act = np.zeros((3, 3), np.float32)
    obs, rew, done, info = env.step(act, ids)
    q1, v1 = env.get_state()
    moved = np.any(q1 != q0, axis=1)
    assert moved[ids].all() and not np.delete(moved, ids).any()
    assert [i["env_id"] for i in info] == [3, 17, 30] and obs.shape == (3, 11)
    ob = env.reset(ids[:2])
    q2, _ = env.get_state()
    assert np.all(q2[30] == q1[30]) and np.all(q2[3] != q1[3]) and ob.shape == (2, 11)
    env.close()


def test_rollout_step_fills_replay_and_auto_resets(ctx):
    import ilswiss_amd as ia
    n = 256
    env = _mk(ctx, "hopper", n, seed=5)
    rb = ia.SimpleReplayBuffer(10 * n, 11, 3, ctx=ctx)
    pol = ia.ReparamTanhMultivariateGaussianPolicy([64, 64], 11, 3, ctx=ctx, seed=1)
    steps = 40
    for t in range(steps):
        env.rollout_step(policy=pol if t % 2 else None, replay=rb, max_path_length=25, random_actions=(t % 2 == 0))
        if t < 10:
            assert rb.num_steps_can_sample() == min((t + 1) * n, 10 * n)
    assert rb._size == 10 * n and rb._top == (steps * n) % (10 * n)
    episodes, ret_sum = env.rollout_stats()
    assert episodes >= n  # every env hit the 25-step limit or fell at least once
    assert 3.0 < ret_sum / episodes < 40.0
    b = rb._get_batch_using_indices(np.arange(10 * n))
    assert np.all(np.abs(b["actions"]) <= 1.0) and np.isfinite(b["observations"]).all()
    term = b["terminals"].ravel().astype(bool)
    assert 0 < term.sum() < term.size
    # healthy transitions keep z > 0.7 and |angle| < 0.2 in next_obs; terminal ones violate it (hopper.py:19-25)
    nz, nang = b["next_observations"][:, 0], b["next_observations"][:, 1]
    healthy = (nz > 0.7) & (np.abs(nang) < 0.2) & (np.abs(b["next_observations"][:, 1:]) < 100).all(1)
    assert np.array_equal(healthy, ~term)
    # reward formula on stored transitions: alive + forward progress - ctrl cost; |r| is O(1)
    assert np.abs(b["rewards"]).max() < 30
    q, v = env.get_state()
    assert np.isfinite(q).all() and (q[:, 1] > 0.5).all()
    env.close()


@pytest.mark.gpu
def test_scaled_and_minmax_env_wrappers(ctx):
    """ScaledEnv / MinmaxEnv (wrappers.py:53-203) folded into the stepper: reset / step / replay records all carry the mapped
    observation; rewards and dynamics are untouched."""
    from ilswiss_amd.envs.vecenv import EPS, MinmaxEnv, ScaledEnv, get_envs
    from ilswiss_amd.replay import SimpleReplayBuffer
    rng = np.random.default_rng(2)
    mean, std = rng.normal(0, 1, 11), rng.uniform(0.5, 2.0, 11)
    lo = rng.normal(-1, 0.3, 11)
    hi = lo + rng.uniform(1.0, 3.0, 11)
    spec = dict(env_name="hopper", env_num=16, training_env_seed=8)
    raw = get_envs(spec, ctx=ctx)
    for wrapper, kw, f in ((ScaledEnv, dict(obs_mean=mean, obs_std=std), lambda x: (x - mean) / (std + EPS)),
                           (MinmaxEnv, dict(obs_min=lo, obs_max=hi), lambda x: (x - lo) / (hi - lo + EPS))):
        env = get_envs(spec, env_wrapper=wrapper, wrapper_kwargs=kw, ctx=ctx)
        o0 = env.reset()
        q, v = env.get_state()
        raw_obs = np.concatenate([q[:, 1:], np.clip(v, -10, 10)], axis=1)
        np.testing.assert_allclose(o0, f(raw_obs), rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(env.get_unscaled_obs(o0), raw_obs, rtol=1e-5, atol=1e-5)
        for _ in range(3):
            act = rng.uniform(-1, 1, (16, 3)).astype(np.float32)
            raw.set_state(*env.get_state())
            o_r, r_r, d_r, _ = raw.step(act)
            o_w, r_w, d_w, _ = env.step(act)
            np.testing.assert_allclose(o_w, f(o_r), rtol=2e-6, atol=2e-6)
            np.testing.assert_array_equal(r_w, r_r)
            np.testing.assert_array_equal(d_w, d_r)
        # the fused rollout records the mapped observations too
        rb = SimpleReplayBuffer(64, 11, 3, random_seed=0, ctx=ctx)
        q, v = env.get_state()
        before = f(np.concatenate([q[:, 1:], np.clip(v, -10, 10)], axis=1))
        env.rollout_step(replay=rb, random_actions=True, max_path_length=1000)
        batch = rb._gather(np.arange(16))
        np.testing.assert_allclose(batch["observations"], before, rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("name", ["hopper", "walker", "halfcheetah"])
def test_step_is_lane_independent(ctx, name):
    """The same states placed in different lanes / workgroups give bit-identical next states (every env is one lane with a
    private LDS slice: any cross-lane or stale-scratch dependence shows up here), over multi-step trajectories that cross
    contact and joint-limit activation."""
    n_base, copies = 128, 8
    n = n_base * copies
    env = _mk(ctx, name, n, seed=11)
    nd, na = env.n_dof, env.act_dim
    rng = np.random.default_rng(5)
    env.reset()
    q, v = env.get_state()
    qb, vb = q[:n_base].copy(), v[:n_base].copy()
    qb[:, 1] += rng.uniform(-0.05, 0.4, n_base)
    qb[:, 2] += rng.uniform(-0.2, 0.2, n_base)
    qb[:, 3:] += rng.uniform(-0.6, 0.3, (n_base, nd - 3))
    vb += rng.normal(0, 1.5, (n_base, nd))
    perm = [rng.permutation(n_base) for _ in range(copies)]
    idx = np.concatenate(perm)                      # env e holds base state idx[e]
    env.set_state(qb[idx], vb[idx])
    for it in range(6):
        ab = rng.uniform(-1.2, 1.2, (n_base, na)).astype(np.float32)
        env.step(ab[idx])
        q1, v1 = env.get_state()
        assert np.isfinite(q1).all() and np.isfinite(v1).all()
        ref_q, ref_v = np.empty_like(qb), np.empty_like(vb)
        ref_q[perm[0]], ref_v[perm[0]] = q1[:n_base], v1[:n_base]
        np.testing.assert_array_equal(q1, ref_q[idx], err_msg=f"it {it}")
        np.testing.assert_array_equal(v1, ref_v[idx], err_msg=f"it {it}")
    env.close()


def test_limit_activating_mid_step_matches_oracle(ctx):
    """Regression: a Hopper state whose leg joint crosses its upper limit in the second of the four RK4 substeps."""
    from oracle.planar_env import PlanarOracle
    env = _mk(ctx, "hopper", 64)
    P = PlanarOracle(env.model)
    env.reset()
    q, v = env.get_state()
    q[:] = [0.00392835, 1.29935858, -0.0386257, -0.46328653, -0.00914546, 0.19995099]
    v[:] = [0.22292121, 0.45649667, -2.6787209, -1.5525852, 2.26402428, 3.00530967]
    act = np.array([0.59693384, 0.9162253, 0.10651099], np.float32)
    env.set_state(q, v)
    env.step(np.tile(act, (64, 1)))
    q1, v1 = env.get_state()
    qo, vo, *_ = P.step(q[0].copy(), v[0].copy(), act)
    assert qo[4] > 0 > q[0, 4]
    np.testing.assert_allclose(q1, np.tile(qo, (64, 1)), rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(v1, np.tile(vo, (64, 1)), rtol=1e-8, atol=1e-8)
    env.close()


def test_no_terminal_keeps_stepping_an_unhealthy_env(ctx):
    """base_algorithm.py:195-196 overwrites `terminals` before the reset decision at :215: with no_terminal an env that fell is stepped on
    until max_path_length (the fallen states are visited), every stored terminal flag is 0, and episodes end only at the time limit."""
    import ilswiss_amd as ia
    n, T = 128, 40
    env = _mk(ctx, "hopper", n, seed=9)
    rb = ia.SimpleReplayBuffer(2 * T * n, 11, 3, ctx=ctx)
    for t in range(T - 1):
        env.rollout_step(policy=None, replay=rb, max_path_length=T, random_actions=True, no_terminal=True)
    assert env.rollout_stats(reset=False)[0] == 0            # nobody was reset by falling
    b = rb._get_batch_using_indices(np.arange((T - 1) * n))
    assert not b["terminals"].any()
    z, ang = b["next_observations"][:, 0], b["next_observations"][:, 1]
    unhealthy = (z <= 0.7) | (np.abs(ang) >= 0.2)
    assert unhealthy.mean() > 0.2                              # random Hopper falls within ~20 steps: those states ARE in the buffer
    nxt = b["next_observations"].reshape(T - 1, n, 11); cur = b["observations"].reshape(T - 1, n, 11)
    np.testing.assert_array_equal(nxt[:-1], cur[1:])           # one unbroken trajectory per env, through the fall
    env.rollout_step(policy=None, replay=rb, max_path_length=T, random_actions=True, no_terminal=True)
    episodes, _ = env.rollout_stats()
    assert episodes == n                                       # all of them end at the time limit, together
    q, v = env.get_state()
    assert np.isfinite(q).all() and np.isfinite(v).all()
    env.close()


@pytest.mark.parametrize("no_terminal", [False, True])
def test_path_mode_inserts_whole_episodes_in_the_references_order(no_terminal):
    """Path mode of the fused rollout == BaseAlgorithm's bookkeeping (base_algorithm.py:490-519 over simple_replay_buffer.py:78-132):
    samples enter the ring when their episode ends, ended envs in ascending order, contiguous, registered in _traj_endpoints, through
    ring wrap-around.  Expected ring: the reference's cursor logic (oracle.replay) replayed over the transitions an identical env run
    in immediate mode recorded."""
    import ilswiss_amd as ia
    from oracle.replay import ReplayOracle
    n, T, maxlen, cap = 48, 70, 25, 900
    got = {}
    for mode in ("step", "path"):
        c = ia.Context(0, seed=123)
        env = _mk(c, "hopper", n, seed=5)
        rb = ia.SimpleReplayBuffer(T * n if mode == "step" else cap, 11, 3, ctx=c)
        if mode == "path":
            env.set_path_mode(True)
        sizes = []
        for t in range(T):
            env.rollout_step(policy=None, replay=rb, max_path_length=maxlen, random_actions=True, no_terminal=no_terminal)
            sizes.append(rb._size)
        got[mode] = (rb._gather(np.arange(rb._size)), rb._top, rb._size, dict(rb._traj_endpoints), sizes, rb)
    rows, _, _, _, _, _ = got["step"]
    ora = ReplayOracle(cap, 11, 3)
    paths, lens, exp_sizes = [[] for _ in range(n)], np.zeros(n, int), []
    for t in range(T):
        for e in range(n):           # the vec step's samples go to the path builders (base_algorithm.py:490-497)
            i = t * n + e
            paths[e].append(i)
        ended = [e for e in range(n) if rows["terminals"][paths[e][-1], 0] > 0 or len(paths[e]) >= maxlen]
        for e in ended:              # _handle_vec_rollout_ending: ascending env index
            for i in paths[e]:
                ora.add_sample(rows["observations"][i], rows["actions"][i], rows["rewards"][i, 0], rows["terminals"][i, 0] > 0,
                               rows["next_observations"][i])
            ora.terminate_episode()
            paths[e] = []
        exp_sizes.append(ora.size)
    b, top, size, ends, sizes, rb = got["path"]
    assert (top, size) == (ora.top, ora.size) and size == cap            # wrapped
    assert sizes == exp_sizes and sizes[0] == 0                          # unfinished episodes are not sampleable
    assert ends == dict(ora.traj_endpoints) and list(ends) == list(ora.traj_endpoints) and len(ends) > 10
    exp = ora.gather(np.arange(size))
    for k in ("observations", "actions", "rewards", "terminals", "next_observations"):
        np.testing.assert_array_equal(b[k].reshape(exp[k].shape), exp[k], err_msg=k)
    trajs = rb.sample_all_trajs()
    assert len(trajs) == len(ends)
    for tr in trajs[:5]:            # contiguous: next_obs(t) == obs(t+1) inside a trajectory
        np.testing.assert_array_equal(tr["next_observations"][:-1], tr["observations"][1:])


@pytest.mark.parametrize("n_env", [4096, 8192])
def test_config_width_rollout_against_oracle_and_terminal_predicate(ctx, n_env):
    """BASELINE configs 2 / 4 at their own width (4096 / 8192 Hopper envs; VERDICT r3 weak #10: only bench.py ran them).  Five vec-env
    steps from spread-out states: every output finite, `done` == the reference's batched terminal predicate on the post-step observation
    (rlkit/envs/terminals.py HopperTerminal, pinned by g14), and 64 envs sampled across the whole width — first / last wavefronts, both
    halves of the grid — equal oracle.planar_env step for step (the tolerance of test_step_matches_oracle)."""
    from ilswiss_amd.envs.terminals import get_terminal_func
    from oracle.planar_env import PlanarOracle
    env = _mk(ctx, "hopper", n_env, seed=11)
    P = PlanarOracle(env.model)
    rng = np.random.default_rng(n_env)
    env.reset()
    q, v = env.get_state()
    q[:, 1] += rng.uniform(-0.05, 0.5, n_env)
    q[:, 2] += rng.uniform(-0.2, 0.2, n_env)
    q[:, 3:] += rng.uniform(-0.8, 0.3, (n_env, env.n_dof - 3))
    v += rng.normal(0, 1.0, (n_env, env.n_dof))
    env.set_state(q, v)
    pick = np.unique(np.concatenate([np.arange(8), n_env - 1 - np.arange(8), rng.choice(n_env, 48, replace=False)]))[:64]
    term = get_terminal_func("hopper")     # rlkit/envs/terminals.py:6-11 -> HopperTerminalFunc.is_terminal(obs, act, next_obs)
    n_done = 0
    for it in range(5):
        act = rng.uniform(-1.2, 1.2, (n_env, env.act_dim)).astype(np.float32)
        obs, rew, done, _ = env.step(act)
        q1, v1 = env.get_state()
        assert np.isfinite(obs).all() and np.isfinite(rew).all() and np.isfinite(q1).all() and np.isfinite(v1).all()
        pred = np.asarray(term(None, None, np.asarray(obs, np.float32))).reshape(-1).astype(bool)
        # the stepper decides on its float64 state (hopper.py:21-27: unclipped velocities), the predicate on the float32 observation (velocities
        # clipped to +-10): rows within rounding of a threshold, or with a state entry near / past 100, are not comparable
        z, ang = q1[:, 1], q1[:, 2]
        edge = (np.abs(z - 0.7) < 1e-5) | (np.abs(np.abs(ang) - 0.2) < 1e-5) | (np.abs(np.concatenate([q1[:, 2:], v1], 1)).max(1) > 99.0)
        assert np.array_equal(pred[~edge], np.asarray(done, bool)[~edge]), (it, int((pred != np.asarray(done, bool)).sum()))
        n_done += int(np.asarray(done).sum())
        for i in pick:
            qo, vo, oo, ro, do = P.step(q[i].copy(), v[i].copy(), act[i])
            np.testing.assert_allclose(q1[i], qo, rtol=1e-8, atol=1e-9, err_msg=f"qpos env {i} it {it}")
            np.testing.assert_allclose(v1[i], vo, rtol=1e-7, atol=1e-7, err_msg=f"qvel env {i} it {it}")
            np.testing.assert_allclose(obs[i], oo, rtol=1e-5, atol=1e-5)
            assert bool(done[i]) == bool(do), (i, it)
        q, v = q1, v1
    assert 0 < n_done < 5 * n_env          # some fell, not all
    env.close()
