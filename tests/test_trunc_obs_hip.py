"""GPU suite of the truncated-observation 3-D tasks (ant_trunc_obs, humanoid_trunc_obs): each runs in lock-step beside its
full-observation task — same context key, same env seed, same Philox stream id, same actions — and must hand out the full task's first
27 / 45 observation columns, rewards and dones bit for bit, through finished episodes and resets, by explicit steps and by the fused
rollout; and the running observation statistics are sized by the truncated width."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PAIRS = [("ant", "ant_trunc_obs", 27), ("humanoid", "humanoid_trunc_obs", 45)]
STEPS = 25


def _pair(ctx, full, trunc, n=8, seed=3, **kw):
    """the two envs on the same Philox stream id: their reset noise and random actions are the same draws"""
    from ilswiss_amd.envs.vecenv import HipVectorEnv
    cur = ctx.rng_stream_cursor()
    ef = HipVectorEnv(full, n, seed=seed, ctx=ctx, **kw)
    ctx.rng_stream_cursor(set_to=cur)
    et = HipVectorEnv(trunc, n, seed=seed, ctx=ctx, **kw)
    return ef, et


@pytest.mark.parametrize("full,trunc,dim", PAIRS)
def test_lock_step_with_the_full_task(ctx, full, trunc, dim):
    ef, et = _pair(ctx, full, trunc)
    assert et.obs_dim == dim and ef.obs_dim > dim and et.act_dim == ef.act_dim
    assert (et.nq - 2) + et.nv == dim
    of, ot = ef.reset(), et.reset()
    assert ot.shape == (8, dim) and np.array_equal(ot, of[:, :dim])
    rng = np.random.default_rng(21)
    n_done = 0

    def run(steps):
        nonlocal n_done
        for s in range(steps):
            act = rng.uniform(-1, 1, (8, ef.act_dim)).astype(np.float32)
            of, rf, df, _ = ef.step(act)
            ot, rt, dt, _ = et.step(act)
            assert np.array_equal(ot, of[:, :dim]), s
            assert np.array_equal(rt, rf) and np.array_equal(dt, df), s
            qt, vt = et.get_state()
            assert np.array_equal(ot, np.concatenate([qt[:, 2:], vt], 1).astype(np.float32)), s    # it is qpos[2:] | qvel
            ids = np.flatnonzero(df)
            if len(ids):       # finished envs start over, as the sampler does: the reset observations are the same draws
                n_done += len(ids)
                zf, zt = ef.reset(ids), et.reset(ids)
                assert np.array_equal(zt, zf[:, :dim]), s

    run(STEPS)
    if n_done == 0:
        # On this engine an Ant under uniform actions stays inside 0.2 <= z <= 1.0 for 25 steps (checked on the host build of the
        # stepper), so nothing has ended yet: toss half of the envs — lifted past z_max, tilted, spinning — and go on, so that the
        # done and reset paths are compared too.
        assert full == "ant"
        q, v = ef.get_state()
        q[:4, 2] += 0.5
        q[:4, 3:7] += rng.normal(0, 0.3, (4, 4))
        q[:4, 3:7] /= np.linalg.norm(q[:4, 3:7], axis=1, keepdims=True)
        v[:4] += rng.normal(0, 1.5, v[:4].shape)
        ef.set_state(q, v), et.set_state(q, v)
        run(10)
    qf, vf = ef.get_state()
    qt, vt = et.get_state()
    assert np.array_equal(qf, qt) and np.array_equal(vf, vt)      # the state layout and the physics are the full task's
    print(f"{trunc}: {n_done} episodes ended")
    assert n_done > 0      # the done and reset paths were compared
    ef.close(), et.close()


@pytest.mark.parametrize("full,trunc,dim", PAIRS)
def test_fused_rollout_records_match_the_full_task(ctx, full, trunc, dim):
    """the fused step (uniform random actions from the env's own stream, records into a ring, auto-reset on done)"""
    from ilswiss_amd.replay import SimpleReplayBuffer
    ef, et = _pair(ctx, full, trunc)
    rf, rt = SimpleReplayBuffer(400, ef.obs_dim, ef.act_dim, ctx=ctx), SimpleReplayBuffer(400, dim, et.act_dim, ctx=ctx)
    ef.reset(), et.reset()
    for _ in range(STEPS):     # max_path_length 10: every env is reset at least twice, whether or not its episode ends by itself
        ef.rollout_step(replay=rf, max_path_length=10, random_actions=True)
        et.rollout_step(replay=rt, max_path_length=10, random_actions=True)
    ctx.sync()
    a, b = rf.get_all(), rt.get_all()
    assert b["observations"].shape == (8 * STEPS, dim)
    assert np.array_equal(b["observations"], a["observations"][:, :dim])
    assert np.array_equal(b["next_observations"], a["next_observations"][:, :dim])
    assert np.array_equal(b["actions"], a["actions"]) and np.array_equal(b["rewards"], a["rewards"])
    assert np.array_equal(b["terminals"], a["terminals"])
    sf, st = ef.rollout_stats(reset=False), et.rollout_stats(reset=False)
    assert sf[0] == st[0] and st[0] >= 16                        # episodes ended: rows after an auto-reset were compared
    # the return sum is built by one atomicAdd per finished env, eight in one launch: the order of those double adds is the scheduler's and
    # need not be the same in the two kernels, so the sums agree to rounding (<= 200 adds of eps each), not bit for bit; the rewards above do
    assert abs(sf[1] - st[1]) <= 200 * np.finfo(np.float64).eps * float(np.abs(a["rewards"]).sum())
    ef.close(), et.close()


def test_norm_obs_statistics_have_the_truncated_width(ctx):
    from ilswiss_amd.envs.vecenv import HipVectorEnv
    env = HipVectorEnv("humanoid_trunc_obs", 8, seed=3, ctx=ctx, norm_obs=True)
    m0 = env.obs_rms.mean.copy()
    assert m0.shape == (45,)
    env.reset()
    rng = np.random.default_rng(2)
    for _ in range(3):
        obs = env.step(rng.uniform(-1, 1, (8, env.act_dim)).astype(np.float32))[0]
    m1 = env.obs_rms.mean
    assert obs.shape == (8, 45) and np.isfinite(obs).all()
    assert m1.shape == (45,) and env.obs_rms.var.shape == (45,) and env.obs_rms.count > 0
    assert not np.array_equal(m0, m1)       # the statistics moved
    env.close()
