"""GPU suite for what the lane-per-env tasks share (lane_step_frame / lane_reset_frame of csrc/classic_env.h) and for who owns a vec env's
device memory (csrc/ilsx_env.hip).

Compact indexing: stepping a list of env ids runs, lane for lane, the arithmetic that stepping every env runs, so the listed envs' states
and their compact obs / rew / done rows are compared BIT FOR BIT with the same rows of a full step, and the unlisted envs with the state
they had.  No restatement and no tolerance: both sides are the same kernel.  70 envs: one full wavefront and a partial one.

Allocations: one life of an env (create, rollouts of every kind, close) must give back every device allocation it made, the ones made on
first use included.  The count is read after a first life (which also warms what the CONTEXT allocates once and keeps) and after an
identical second one.  The library refuses norm_obs together with a fused replay insert, so the env is created with norm_obs=True, takes
one policy step under it, and has the normalisation turned off before the steps that record."""
import ctypes as C

import numpy as np
import pytest

TASKS = ("cartpole", "pendulum", "invertedpendulum", "inverteddoublependulum", "swimmer")
N, IDS = 70, [69, 0, 33]


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[x.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", TASKS)
def test_stepping_listed_envs_equals_the_same_rows_of_a_full_step(ctx, name):
    from ilswiss_amd.envs import HipVectorEnv
    a_env, b_env = HipVectorEnv(name, N, seed=7, ctx=ctx), HipVectorEnv(name, N, seed=7, ctx=ctx)
    rng = np.random.default_rng(17)
    q0, v0 = a_env.get_state()
    q = q0 + rng.uniform(-0.05, 0.05, q0.shape)   # near the reset state: upright poles, no episode ends in the step
    v = v0 + rng.uniform(-0.05, 0.05, v0.shape)
    a_env.set_state(q, v), b_env.set_state(q, v)
    if a_env.discrete_n:
        act = rng.integers(0, a_env.discrete_n, (N, 1)).astype(np.float32)
    else:
        act = rng.uniform(-1.0, 1.0, (N, a_env.act_dim)).astype(np.float32)
    oa, ra, da, _ = a_env.step(act[IDS], id=IDS)
    ob, rb, db, _ = b_env.step(act)
    qa, va = a_env.get_state()
    qb, vb = b_env.get_state()
    rest = np.setdiff1d(np.arange(N), IDS)
    assert _same(qa[rest], q[rest]) and _same(va[rest], v[rest])          # the unlisted envs kept their state
    assert not _same(qb[rest], q[rest])                                  # ... which a step does change
    assert _same(qa[IDS], qb[IDS]) and _same(va[IDS], vb[IDS])
    assert oa.shape == (3, a_env.obs_dim) and _same(oa, ob[IDS]) and _same(ra, rb[IDS]) and _same(da, db[IDS])   # compact rows, id order
    assert np.isfinite(oa).all() and np.isfinite(ra).all()
    a_env.close(), b_env.close()


def _ctx_allocs(ctx):
    n = C.c_size_t()
    assert ctx.lib.ilsx_debug_ctx_allocs(ctx.h, C.byref(n)) == 0
    return n.value


def _one_life(ctx, name, pol, rb):
    import ilswiss_amd as ia
    from ilswiss_amd import _lib
    from ilswiss_amd.envs import HipVectorEnv
    from ilswiss_amd.samplers import DeviceEvalSampler
    env = HipVectorEnv(name, 8, seed=1, ctx=ctx, norm_obs=True)
    env.rollout_step(policy=pol, max_path_length=4)                       # running statistics and the normalised policy input
    _lib.check(ctx.lib.ilsx_vecenv_obs_norm(env.h, 0, 0))
    env.rollout_step(policy=pol, replay=rb, max_path_length=4)            # fused insert into the ring
    env.rollout_step(policy=pol, replay=rb, max_path_length=4, label_policy=pol)   # relabel step: the label buffer
    env.set_path_mode(True)
    env.rollout_step(policy=pol, replay=rb, max_path_length=4)            # the episode staging area
    env.set_path_mode(False)
    DeviceEvalSampler(env, ia.MakeDeterministic(pol), 8, 3).obtain_statistics()    # the evaluation buffers
    cfg = _lib.ExploreCfg(2, 0, 0.0, 0.15, 0.3, 0.3, 1000.0, -1.0, 1.0)            # an OU process per env
    _lib.check(ctx.lib.ilsx_vecenv_set_exploration(env.h, C.byref(cfg)))
    env.rollout_step(policy=pol, replay=rb, max_path_length=4)
    ctx.sync()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("hopper", "ant", "swimmer"))   # one task of each engine
def test_an_env_gives_back_every_device_allocation(ctx, name):
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    probe = HipVectorEnv(name, 8, seed=1, ctx=ctx)
    o, a = probe.obs_dim, probe.act_dim
    probe.close()
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[32, 32], obs_dim=o, action_dim=a, ctx=ctx)
    rb = ia.SimpleReplayBuffer(256, o, a, ctx=ctx)
    _one_life(ctx, name, pol, rb)
    before = _ctx_allocs(ctx)
    _one_life(ctx, name, pol, rb)
    after = _ctx_allocs(ctx)
    print(f"{name}: context allocations after the first life {before}, after the second {after}")
    assert after == before
