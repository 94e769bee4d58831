"""GPU suite of the vectorised HER loop: path mode of the fused rollout on the goal env, the hindsight sampler that draws in the kernel
(ilsx_her_sample, k_her_sample of csrc/ilsx_replay.hip) against its numpy restatement (tests/her_sample_restatement.py, tied to the
reference buffer by tests/test_goal_env_cpu.py) and against ilsx_her_gather (pinned by golden g22), her.VecHER end to end, and the
allocation count of an env and its ring."""
import csv
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


def _goal_space_env(o, gd, a, reward_type="sparse", thr=0.5):
    from ilswiss_amd.her import Box, DictSpace

    class Env:
        observation_space = DictSpace(observation=Box(-np.ones(o), np.ones(o)), desired_goal=Box(-np.ones(gd), np.ones(gd)),
                                      achieved_goal=Box(-np.ones(gd), np.ones(gd)))
        action_space = Box(-np.ones(a), np.ones(a))
    Env.reward_type, Env.distance_threshold = reward_type, thr
    return Env


def _add_episode(rb, rng, L):
    o, a = rb._observation_dim, rb._action_dim
    ends = np.zeros(L, np.uint8)
    ends[-1] = 1
    rb.add_rows(rng.uniform(-1, 1, (L, o)), rng.uniform(-1, 1, (L, a)), rng.normal(0, 1, L), np.zeros(L, np.uint8), rng.uniform(-1, 1, (L, o)), ends)


def _slots(endpoints, cap):
    """start -> the trajectory's ring slots, in order"""
    return {s: [(s + k) % cap for k in range((e - s) % cap)] for s, e in endpoints.items()}


# ---------------------------------------------------------------------------------------------- path mode
def test_path_mode_fills_the_ring_with_whole_episodes(ctx):
    from ilswiss_amd import her
    from ilswiss_amd.envs import HipVectorEnv
    n, L, cap = 5, 7, 64
    env = HipVectorEnv("point-reach", n, seed=3, ctx=ctx)
    rb = her.DeviceGoalReplayBuffer(cap, env, random_seed=1, ctx=ctx)
    env.set_path_mode(True)
    first_starts = None
    for step in range(1, 41):
        env.rollout_step(replay=rb, max_path_length=L, random_actions=True)
        ends = rb._traj_endpoints
        assert rb.num_steps_can_sample() == min(cap, n * L * (step // L))          # episodes enter the ring when they end, whole
        if step == L:
            first_starts = sorted(ends)
            assert first_starts == [0, 7, 14, 21, 28]
        if step == 2 * L:                                                          # 70 rows in 64 slots: the oldest episode is gone
            assert len(ends) == 9 and 0 not in ends and set(first_starts[1:]) <= set(ends)
    ends = rb._traj_endpoints
    sl = _slots(ends, cap)
    assert len(ends) == 9 and all(len(v) == L for v in sl.values())               # contiguous, length 7
    flat = [x for v in sl.values() for x in v]
    assert len(set(flat)) == len(flat)                                             # ... and disjoint
    assert any(e < s for s, e in ends.items())                                     # one of them wraps the ring
    for s, idx in sl.items():
        b = rb._gather(np.array(idx))
        ob, nob = b["observations"], b["next_observations"]
        assert (ob[:, 4:6] == ob[0, 4:6]).all() and (nob[:, 4:6] == ob[0, 4:6]).all()     # the desired goal is constant inside an episode
        assert _same(nob[:, 6:8], nob[:, 0:2]) and _same(ob[:, 6:8], ob[:, 0:2])          # achieved goal = the observation's p
        assert _same(nob[:-1], ob[1:]) and (b["terminals"] == 0).all()                    # the steps of ONE episode, in order
        d = np.linalg.norm(nob[:, 6:8].astype(np.float64) - nob[:, 4:6].astype(np.float64), axis=1)
        near = np.abs(d - 0.1) < 1e-6
        np.testing.assert_array_equal(b["rewards"][~near, 0], -(d[~near] > 0.1).astype(np.float32))
    goals = {tuple(rb._gather(np.array(idx[:1]))["observations"][0, 4:6]) for idx in sl.values()}
    assert len(goals) == 9                                                         # a new goal every episode
    batch = rb.numpy_batch(rb.random_batch(64))
    assert batch["observations"].shape == (64, 4) and batch["desired_goals"].shape == (64, 2) and np.isfinite(batch["rewards"]).all()
    rb.close(), env.close()


# ---------------------------------------------------------------------------------------------- sampler, explicit uniforms
def _her_sample(ctx, rb, B, n_rel, rtype, d_obs, d_goal, kind, thr, u):
    from ilswiss_amd import _lib
    W, a = d_obs + d_goal, rb._action_dim
    out = [ctx.empty((B, W)), ctx.empty((B, a)), ctx.empty((B,)), ctx.empty((B,)), ctx.empty((B, W))]
    di, dr = ctx.empty((B,), np.int64), ctx.empty((B,), np.int64)
    ud = ctx.from_numpy(u, np.float64) if u is not None else None
    _lib.check(ctx.lib.ilsx_her_sample(rb.h, B, n_rel, rtype, d_obs, d_goal, kind, C.c_float(thr), ud.ptr if ud is not None else None,
                                       *[x.ptr for x in out], di.ptr, dr.ptr))
    return [x.numpy() for x in out], di, dr


def _her_gather(ctx, rb, B, n_rel, relabel_on, d_obs, d_goal, kind, thr, di, dr):
    from ilswiss_amd import _lib
    W, a = d_obs + d_goal, rb._action_dim
    out = [ctx.empty((B, W)), ctx.empty((B, a)), ctx.empty((B,)), ctx.empty((B,)), ctx.empty((B, W))]
    _lib.check(ctx.lib.ilsx_her_gather(rb.h, di.ptr, dr.ptr, B, n_rel, relabel_on, d_obs, d_goal, kind, C.c_float(thr), *[x.ptr for x in out]))
    return [x.numpy() for x in out]


@pytest.mark.parametrize("d_obs,d_goal,a", [(4, 2, 2), (10, 3, 4), (25, 3, 4)])       # the stand-in's dims and the Fetch tasks' dims
def test_sampler_with_explicit_uniforms(ctx, d_obs, d_goal, a):
    """Episodes of 12 (evicted by the wrap), 50, 7, 1, 2 and 16 steps in a ring of 80: the last one wraps (72..79, 0..7)."""
    from ilswiss_amd import her
    cap = 80
    rng = np.random.default_rng(d_obs)
    rb = her.DeviceGoalReplayBuffer(cap, _goal_space_env(d_obs, d_goal, a), random_seed=3, ctx=ctx)
    for L in (12, 50, 7, 1, 2, 16):
        _add_episode(rb, rng, L)
    ends = rb._traj_endpoints
    starts, lens = R.traj_table(ends, cap)
    assert starts.tolist() == [12, 62, 69, 70, 72] and lens.tolist() == [50, 7, 1, 2, 16]
    edge = np.array([[0.0, 0.0, 0.0], [np.nextafter(1.0, 0.0)] * 3, [0.99, 0.0, np.nextafter(1.0, 0.0)], [0.99, 0.5, 0.5], [0.5, 0.5, 0.0]])
    for B in (1, 37, 128):
        u = rng.random((B, 3))
        u[: min(B, len(edge))] = edge[: min(B, len(edge))]
        for n_rel in (0, int(0.8 * B), B):
            for rtype in (1, 2, 0):
                kind, thr = (rtype + B) % 2, 0.7
                got, di, dr = _her_sample(ctx, rb, B, n_rel, rtype, d_obs, d_goal, kind, thr, u)
                idx, rel = R.sample_indices(starts, lens, cap, u, rtype)
                np.testing.assert_array_equal(di.numpy(), idx, err_msg=f"{B} {n_rel} {rtype}")
                np.testing.assert_array_equal(dr.numpy(), rel, err_msg=f"{B} {n_rel} {rtype}")
                want = _her_gather(ctx, rb, B, n_rel, int(rtype != 0), d_obs, d_goal, kind, thr, di, dr)
                for g_, w_, name in zip(got, want, ("obs_cat", "act", "rew", "done", "nobs_cat")):
                    assert _same(g_, w_), (B, n_rel, rtype, name)
                if rtype and n_rel == B and B > 1:      # relabelled rows carry the relabel record's next achieved goal
                    rows = rb._gather(rel)["next_observations"]
                    assert _same(got[0][:, d_obs:], rows[:, d_obs + d_goal:])
    lib = ctx.lib
    o5 = [ctx.empty((4, d_obs + d_goal)), ctx.empty((4, a)), ctx.empty((4,)), ctx.empty((4,)), ctx.empty((4, d_obs + d_goal))]
    p5 = [x.ptr for x in o5]
    f = C.c_float(0.5)
    assert lib.ilsx_her_sample(rb.h, 4, 5, 1, d_obs, d_goal, 0, f, None, *p5, None, None) == -1            # n_relabel outside [0, B]
    assert lib.ilsx_her_sample(rb.h, 4, -1, 1, d_obs, d_goal, 0, f, None, *p5, None, None) == -1
    assert lib.ilsx_her_sample(rb.h, 4, 2, 1, d_obs, d_goal, 2, f, None, *p5, None, None) == -1            # reward_kind outside {0, 1}
    assert lib.ilsx_her_sample(rb.h, 4, 2, 3, d_obs, d_goal, 0, f, None, *p5, None, None) == -1            # relabel_type outside {0, 1, 2}
    assert lib.ilsx_her_sample(rb.h, 4, 2, 1, d_obs + 1, d_goal, 0, f, None, *p5, None, None) == -1        # ring width != d_obs + 2 d_goal
    assert lib.ilsx_her_sample(rb.h, 4, 2, 1, d_obs, d_goal, 0, f, None, *p5, None, None) == 0             # index outputs are optional
    rb.close()


def test_sampler_refusals_of_state_and_width(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd import _lib, her
    lib, f = ctx.lib, C.c_float(0.5)
    rb = her.DeviceGoalReplayBuffer(32, _goal_space_env(4, 2, 2), ctx=ctx)
    o5 = [ctx.empty((4, 6)), ctx.empty((4, 2)), ctx.empty((4,)), ctx.empty((4,)), ctx.empty((4, 6))]
    assert lib.ilsx_her_sample(rb.h, 4, 2, 1, 4, 2, 0, f, None, *[x.ptr for x in o5], None, None) == -4    # no registered trajectory
    rng = np.random.default_rng(0)
    rb.add_rows(rng.uniform(-1, 1, (3, 8)), rng.uniform(-1, 1, (3, 2)), np.zeros(3), np.zeros(3, np.uint8), rng.uniform(-1, 1, (3, 8)))
    assert lib.ilsx_her_sample(rb.h, 4, 2, 1, 4, 2, 0, f, None, *[x.ptr for x in o5], None, None) == -4    # rows, but no finished episode
    rb.terminate_episode()
    assert lib.ilsx_her_sample(rb.h, 4, 2, 1, 4, 2, 0, f, None, *[x.ptr for x in o5], None, None) == 0
    wide = ia.SimpleReplayBuffer(32, 5, 7, ctx=ctx)                                                         # act_dim 7 > d_obs + d_goal 4
    assert lib.ilsx_her_sample(wide.h, 4, 2, 1, 3, 1, 0, f, None, *[x.ptr for x in o5], None, None) == _lib.ILSX_ERR_UNSUPPORTED
    rb.close()


# ---------------------------------------------------------------------------------------------- sampler, Philox
def _check_inside(idx, rel, ends, cap):
    """every idx lies in a registered trajectory, its idx_relabel in the same one at an offset >= its own; returns the trajectory of each row"""
    owner = np.full(cap, -1)
    offs = np.zeros(cap, np.int64)
    for s, sl in _slots(ends, cap).items():
        owner[sl], offs[sl] = s, np.arange(len(sl))
    assert (owner[idx] >= 0).all() and (owner[rel] == owner[idx]).all() and (offs[rel] >= offs[idx]).all()
    return owner[idx]


def test_sampler_with_its_own_draws(ctx):
    from ilswiss_amd import her
    cap, B = 64, 4096
    env = _goal_space_env(4, 2, 2)
    cur = ctx.rng_stream_cursor()
    rb = her.DeviceGoalReplayBuffer(cap, env, random_seed=21, ctx=ctx)
    ctx.rng_stream_cursor(set_to=cur)                      # the second ring takes the first one's Philox stream id: one seed, one stream
    rb2 = her.DeviceGoalReplayBuffer(cap, env, random_seed=21, ctx=ctx)
    for r in (rb, rb2):
        rng = np.random.default_rng(2)
        for _ in range(4):
            _add_episode(r, rng, 10)
    ends = rb._traj_endpoints
    b1 = rb.random_batch(B, return_indices=True)
    i1, r1 = b1["indices"].numpy(), b1["indices_relabel"].numpy()
    o1 = b1["observations"].numpy()
    own = _check_inside(i1, r1, ends, cap)
    counts = np.array([(own == s).sum() for s in ends])
    print("rows per trajectory:", counts.tolist())
    assert (np.abs(counts - 1024) <= 6 * np.sqrt(4096 * 0.25 * 0.75)).all()           # 4 equal trajectories: 1024 +- 166 each
    assert (r1 != i1).any() and len(set(i1.tolist())) == 40
    b2 = rb.random_batch(B, return_indices=True)
    assert not np.array_equal(b2["indices"].numpy(), i1)                              # two calls differ
    c1 = rb2.random_batch(B, return_indices=True)
    assert np.array_equal(c1["indices"].numpy(), i1) and np.array_equal(c1["indices_relabel"].numpy(), r1)   # two rings with one seed agree
    assert _same(c1["observations"].numpy(), o1)
    # a table change between two calls is seen by the next call: one more episode ...
    rng = np.random.default_rng(3)
    _add_episode(rb, rng, 5)
    ends = rb._traj_endpoints
    assert len(ends) == 5
    b = rb.random_batch(B, return_indices=True)
    own = _check_inside(b["indices"].numpy(), b["indices_relabel"].numpy(), ends, cap)
    assert (own == 40).sum() > 500                                                    # the new trajectory (slots 40..44) is drawn from
    # ... then an eviction: 25 more rows wrap the ring over the first trajectory (slots 0..5 of 0..9 are overwritten)
    _add_episode(rb, rng, 25)
    ends = rb._traj_endpoints
    assert 0 not in ends and len(ends) == 5
    b = rb.random_batch(B, return_indices=True)
    own = _check_inside(b["indices"].numpy(), b["indices_relabel"].numpy(), ends, cap)
    assert set(own.tolist()) == set(ends) and not np.isin(b["indices"].numpy(), np.arange(6, 10)).any()
    rb.close(), rb2.close()


# ---------------------------------------------------------------------------------------------- the loop
def _vec_her(ctx, trainer_name, tmp, **alg):
    import ilswiss_amd as ia
    from ilswiss_amd import her
    from ilswiss_amd.envs import HipVectorEnv
    env = HipVectorEnv("point-reach", 64, seed=1, ctx=ctx)
    eval_env = HipVectorEnv("point-reach", 32, seed=10008, ctx=ctx)
    q1, q2 = ia.FlattenMlp([64, 64], 1, 8, ctx=ctx, seed=6), ia.FlattenMlp([64, 64], 1, 8, ctx=ctx, seed=7)
    if trainer_name == "td3":
        pol = her.MlpGaussianAndEpsilonPolicy([64, 64], 4, 2, action_space=env.single_action_space, condition_dim=2, output_activation="tanh",
                                              ctx=ctx, seed=5)
        tr = her.TD3(pol, q1, q2, discount=0.95, policy_lr=1e-3, qf_lr=1e-3, max_batch=128)
    else:
        pol = ia.ReparamTanhMultivariateGaussianPolicy([64, 64], 6, 2, ctx=ctx, seed=5)
        tr = her.SAC(pol, q1, q2, discount=0.95, policy_lr=1e-3, qf_lr=1e-3, max_batch=128)
    kw = dict(batch_size=128, max_path_length=25, replay_buffer_size=20000, num_steps_per_eval=800, eval_deterministic=True,
              num_steps_between_train_calls=64, log_dir=str(tmp))
    kw.update(alg)
    return her.VecHER(tr, env, env, eval_env, pol, **kw), tr


def test_vec_her_learns_to_reach(tmp_path):
    """her.VecHER end to end on 64 device envs, a context of its own.  4 epochs of 55 vec steps; training starts when the first episodes
    are in (vec step 25), then 16 gradient steps per vec step: 196 x 16 = 3136 gradient steps, fewer than the host loop's test spends
    (3500).  The bar is that test's own, on the evaluation's Success Rate."""
    import ilswiss_amd as ia
    from ilswiss_amd import her
    ctx = ia.Context(0, seed=11)
    try:
        np.random.seed(3)
        alg, tr = _vec_her(ctx, "td3", tmp_path / "td3", num_epochs=3, num_steps_per_epoch=64 * 55, min_steps_before_training=64 * 25,
                           num_train_steps_per_train_call=16)
        assert isinstance(alg.replay_buffer, her.DeviceGoalReplayBuffer) and alg.exploration_policy.env is None
        first = alg._eval_collect()["Success Rate"]
        alg.train()
        assert alg.exploration_policy.env is alg.training_env                      # the policy bound its exploration to the device env
        rows = list(csv.DictReader(open(tmp_path / "td3" / "progress.csv")))
        hist = [float(r["Success Rate"]) for r in rows]
        print("success rate before training", first, "per epoch", hist, "gradient steps", alg._n_grad_steps_total)
        assert len(hist) == 4 and 0 < alg._n_grad_steps_total <= 3500
        assert max(hist) >= max(0.6, first + 0.3), (first, hist)
        for col in ("Epoch", "AverageReturn", "Test Returns Mean", "Test Ep. Len. Mean", "Num Paths", "QF1 Loss", "Policy Loss",
                    "Exploration Returns Mean", "Number of train calls total", "Number of gradient steps total", "Number of env steps total",
                    "Number of rollouts total", "Train Time (s)", "Sample Time (s)", "Epoch Time (s)", "Total Train Time (s)", "Success Rate"):
            assert col in rows[0], col
        assert int(float(rows[-1]["Number of env steps total"])) == 4 * 64 * 55 and float(rows[-1]["Num Paths"]) == 32
        assert os.path.exists(tmp_path / "td3" / "params.pkl") and os.path.exists(tmp_path / "td3" / "extra_data.pkl")
        # one epoch of her.SAC through the same loop
        alg2, tr2 = _vec_her(ctx, "sac", tmp_path / "sac", num_epochs=0, num_steps_per_epoch=64 * 40, min_steps_before_training=64 * 25,
                             num_train_steps_per_train_call=4)
        alg2.train()
        assert alg2._n_train_steps_total > 0 and alg2._n_grad_steps_total == 4 * alg2._n_train_steps_total
        for k in ("policy", "qf1", "qf2"):
            assert np.isfinite(tr2.get_params(k)).all(), k
        row = list(csv.DictReader(open(tmp_path / "sac" / "progress.csv")))[0]
        assert 0.0 <= float(row["Success Rate"]) <= 1.0 and np.isfinite(float(row["QF1 Loss"]))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- allocations
def _ctx_allocs(ctx):
    n = C.c_size_t()
    assert ctx.lib.ilsx_debug_ctx_allocs(ctx.h, C.byref(n)) == 0
    return n.value


def _one_life(ctx, pol):
    import ilswiss_amd as ia
    from ilswiss_amd import her
    from ilswiss_amd.envs import HipVectorEnv
    from ilswiss_amd.samplers import DeviceEvalSampler
    env = HipVectorEnv("point-reach", 8, seed=1, ctx=ctx)
    rb = her.DeviceGoalReplayBuffer(512, env, random_seed=1, ctx=ctx)
    env.set_path_mode(True)
    for _ in range(9):
        env.rollout_step(policy=pol, replay=rb, max_path_length=4)                 # exploration bound, episodes staged and inserted
    rb.random_batch(16)                                                            # the trajectory mirror and the batch arrays
    for _ in range(70):
        env.rollout_step(policy=pol, replay=rb, max_path_length=4)                 # > 64 trajectories: the mirror grows
    rb.random_batch(16)
    DeviceEvalSampler(env, ia.MakeDeterministic(pol), 8, 3).obtain_statistics()
    ctx.sync()
    pol.env = None
    rb.close(), env.close()


def test_env_and_ring_give_back_every_device_allocation(ctx):
    from ilswiss_amd import her
    pol = her.MlpGaussianAndEpsilonPolicy([64, 64], 4, 2, condition_dim=2, output_activation="tanh", ctx=ctx)
    _one_life(ctx, pol)
    before = _ctx_allocs(ctx)
    _one_life(ctx, pol)
    after = _ctx_allocs(ctx)
    print(f"context allocations after the first life {before}, after the second {after}")
    assert after == before
