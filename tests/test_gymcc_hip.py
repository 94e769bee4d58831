"""GPU suite for the MountainCarContinuous / MountainCar / Acrobot steppers of the classic-control engine (csrc/classic_env.h,
ILSX_CLASSIC_MOUNTAINCAR_CONT / _MOUNTAINCAR / _ACROBOT) against the numpy restatements of gym 0.22's classes in tests/gymcc_restatement.py:
spaces, reset, state access, one step, the fused rollout (replay records, auto-reset, episode bookkeeping, the device's random actions,
no_terminal, path mode), action handling, discrete SAC on Discrete(3) and SAC-alpha on the continuous car end to end, and the C entry point.

As in test_pendulum_hip.py the rollout is restated every step from the device's own previous state, so nothing builds up.  Rewards need no
libm given `done` and agree bit for bit.  The float64 states agree bit for bit except where ROCm's and glibc's double cos / sin differ by an
ulp; what such a difference can do to a step was measured on the CPU (tests/test_gymcc_cpu.py: every libm result of the restatement moved by
+-1 ulp at random over parity_inputs): largest absolute deviation of a state component MountainCarContinuous 0 (the float32 store absorbs
it), MountainCar 2.22e-16, Acrobot 1.07e-14.  The bound here is 8 x that (gymcc_restatement.ULP_DEV, ULP_FACTOR): 0, 1.78e-15, 8.53e-14.
The two cars, with one cos per step, may differ in at most 1 % of the state components (Pendulum, one sin: 0.40 %); Acrobot, with sixteen
libm calls per step, has no such cap: its share is printed (see DESIGN.md section 24 for the measured figures).  `done` is compared wherever
the restated result is further than the bound from the threshold (at most 0.1 % of the rows may be left out), and some compared rows end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gymcc_restatement as gr  # noqa: E402
from gymcc_restatement import Acrobot, MountainCar, MountainCarCont  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
TASKS = pytest.mark.parametrize("task", list(gr.TASKS.values()), ids=lambda t: t.name)
CARS = (MountainCarCont, MountainCar)


def _bound(task):
    return gr.ULP_FACTOR * gr.ULP_DEV[task.name]


def _env(ctx, task, n, seed=3, **kw):
    from ilswiss_amd.envs import HipVectorEnv
    return HipVectorEnv(task.name, n, seed=seed, ctx=ctx, **kw)


def _state(env):
    return np.concatenate(env.get_state(), 1)


def _set(env, task, s):
    env.set_state(*gr.split(task, s))


def _in_reset_range(task, s):
    if task is Acrobot:
        return np.all(np.abs(s) <= 0.1 + 1e-7)
    return np.all(s[:, 0] >= -0.6 - 1e-7) and np.all(s[:, 0] <= -0.4 + 1e-7) and np.all(s[:, 1] == 0)


def _is_f32(s):
    return np.array_equal(s, s.astype(F32).astype(np.float64))


def _reward_given_done(task, action, done):
    """The reward of a step whose done flag is known: no libm in it."""
    if task is MountainCarCont:
        f = task.force(action).astype(np.float64)
        return np.where(done, 100.0, 0.0) - (f * f) * 0.1
    return np.full(len(done), -1.0) if task is MountainCar else np.where(done, 0.0, -1.0)


# ---------------------------------------------------------------------------------------------------- spaces, reset, state access
@TASKS
def test_spaces_and_dims(ctx, task):
    from ilswiss_amd.envs.vecenv import Box, Discrete
    env = _env(ctx, task, 64)
    assert (env.obs_dim, env.act_dim, env.nq, env.nv, env.n_dof) == (task.obs_dim, 1, task.nq, task.nq, task.nq)
    assert env.discrete_n == task.discrete_n
    ac = env.action_space[0]
    if task.discrete_n:
        assert isinstance(ac, Discrete) and ac.n == 3 and repr(ac) == "Discrete(3)"
    else:
        assert isinstance(ac, Box) and ac.shape == (1,) and np.array_equal(ac.low, [-1.0]) and np.array_equal(ac.high, [1.0])
    assert env.observation_space[0].shape == (task.obs_dim,)
    env.close()


@TASKS
def test_reset_range(ctx, task):
    env = _env(ctx, task, 4096)
    obs = env.reset()
    s = _state(env)
    assert _in_reset_range(task, s)
    if task is Acrobot:
        assert np.all(s.std(0) > 0.05) and _is_f32(s)                 # U(-0.1, 0.1): std 0.0577; reset() rounds to float32
    else:
        assert s[:, 0].std() > 0.05 and abs(s[:, 0].mean() + 0.5) < 0.01
        assert _is_f32(s) == (task is MountainCarCont)                  # the continuous car keeps float32 values, the discrete one float64
    assert np.array_equal(obs.astype(F32), task.observe(s))
    obs2 = env.reset()                                                  # a new Philox counter: other states
    assert not np.array_equal(obs2, obs)
    env.close()


@TASKS
def test_set_state_and_one_step_against_the_restatement(ctx, task):
    n = 1000
    env = _env(ctx, task, n)
    s, a = gr.parity_inputs(task, n, 0)
    _set(env, task, s)
    assert np.array_equal(_state(env), s)
    obs, rew, done, _ = env.step(a)
    want, wrew, wdone = task.step(s, a)
    got = _state(env)
    dev = np.abs(got - want)
    differ = got != want
    print(f"{task.name}: largest state deviation {dev.max()!r} (bound {_bound(task)!r}), {int(differ.sum())} of {differ.size} components differ")
    assert np.all(dev <= _bound(task)), dev.max()
    if task in CARS:
        assert differ.sum() <= 1e-2 * differ.size
    far = gr.done_margin(task, s, a, want) > _bound(task)
    assert (~far).sum() <= 1e-3 * n
    assert np.array_equal(done[far], wdone[far]) and wdone[far].sum() >= 0.05 * n
    assert np.array_equal(rew.astype(F32), _reward_given_done(task, a, done).astype(F32))
    assert np.array_equal(rew[far].astype(F32), wrew[far].astype(F32))
    same = ~differ.any(1)
    assert np.array_equal(obs[same].astype(F32), task.observe(want)[same])
    np.testing.assert_allclose(obs, task.observe(want), rtol=0, atol=1e-6)
    if task is MountainCarCont:
        assert _is_f32(got)
    env.close()


# ---------------------------------------------------------------------------------------------------- the fused rollout
@TASKS
def test_rollout_steps_match_restatement_up_to_libm_ulps(ctx, task):
    import ilswiss_amd as ia
    n, T, maxlen = 1024, 120, 50
    env = _env(ctx, task, n)
    s0, _ = gr.parity_inputs(task, n, 1)
    _set(env, task, s0)
    env.rollout_stats(reset=True)
    rb = ia.SimpleReplayBuffer(n, task.obs_dim, 1, ctx=ctx)   # capacity n: step t's record of env i sits at slot i
    ep_len, ep_ret = np.zeros(n, int), np.zeros(n)
    prev = _state(env)
    episodes, ret_sum, mism, checked, left_out, ended_by_done = 0, 0.0, 0, 0, 0, 0
    seen, amin, amax = set(), 1.0, -1.0
    for t in range(T):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
        rec = rb._gather(np.arange(n))
        a = rec["actions"][:, 0]
        if task.discrete_n:
            seen |= set(a.tolist())
        else:
            assert np.all(a > -1) and np.all(a < 1)                    # Box(-1, 1).sample(), stored unmapped
            amin, amax = min(amin, a.min()), max(amax, a.max())
        want, wrew, wdone = task.step(prev, a)
        term = rec["terminals"][:, 0] != 0
        assert np.array_equal(rec["observations"], task.observe(prev)), t
        assert np.array_equal(rec["rewards"][:, 0], _reward_given_done(task, a, term).astype(F32)), t
        far = gr.done_margin(task, prev, a, want) > _bound(task)
        left_out += int((~far).sum())
        assert np.array_equal(term[far], wdone[far]), t
        ended_by_done += int(term[far].sum())
        ep_len += 1
        ep_ret += _reward_given_done(task, a, term)
        end = term | (ep_len >= maxlen)
        got = _state(env)
        keep = ~end
        assert np.all(np.abs(got[keep] - want[keep]) <= _bound(task)), (t, np.abs(got[keep] - want[keep]).max())
        mism += int(np.sum(got[keep] != want[keep]))
        checked += int(keep.sum()) * got.shape[1]
        same = keep & np.all(got == want, 1)
        assert np.array_equal(rec["next_observations"][same], task.observe(want)[same]), t
        # the ended envs' post-step states were replaced by resets: their records agree with the restatement to float32 rounding
        np.testing.assert_allclose(rec["next_observations"][end], task.observe(want)[end], rtol=0, atol=1e-6)
        assert _in_reset_range(task, got[end])
        episodes += int(end.sum())
        ret_sum += float(ep_ret[end].sum())
        ep_len[end], ep_ret[end] = 0, 0.0
        prev = got
    print(f"{task.name}: {mism} of {checked} float64 state components differ from the restatement ({100.0 * mism / checked:.3f} %), "
          f"{ended_by_done} episodes ended by done, {left_out} rows left out of the done comparison")
    if task in CARS:
        assert mism <= 1e-2 * checked, f"{mism} of {checked} float64 state components differ from the restatement"
    assert left_out <= 1e-3 * n * T
    assert ended_by_done > 0
    if task.discrete_n:
        assert seen == {0.0, 1.0, 2.0}, seen                           # Discrete(3).sample(): every index and no other
    else:
        assert amin < -0.99 and amax > 0.99
    e, r = env.rollout_stats(reset=True)
    assert e == episodes and episodes >= 2 * n
    np.testing.assert_allclose(r, ret_sum, rtol=1e-12, atol=1e-9)     # a sum of per-env float64 returns in another order
    env.close()


@TASKS
def test_no_terminal_keeps_the_episode_going(ctx, task):
    import ilswiss_amd as ia
    n = 256
    env = _env(ctx, task, n)
    s, _ = gr.parity_inputs(task, n, 2)
    _set(env, task, s)
    rb = ia.SimpleReplayBuffer(n, task.obs_dim, 1, ctx=ctx)
    env.rollout_step(replay=rb, max_path_length=50, random_actions=True, no_terminal=True)
    rec = rb._gather(np.arange(n))
    want, _, wdone = task.step(s, rec["actions"][:, 0])
    assert wdone.sum() >= 0.05 * n and not rec["terminals"].any()
    got = _state(env)
    assert np.all(np.abs(got - want) <= _bound(task))                  # nobody was reset, the ended rows included
    assert np.array_equal(rec["rewards"][:, 0], _reward_given_done(task, rec["actions"][:, 0], wdone).astype(F32))   # done still pays
    env.close()


@TASKS
def test_path_mode_inserts_whole_episodes(ctx, task):
    import ilswiss_amd as ia
    n, maxlen = 256, 50
    env = _env(ctx, task, n, seed=5)
    s, _ = gr.parity_inputs(task, n, 3)
    _set(env, task, s)
    env.rollout_stats(reset=True)
    env.set_path_mode(True)
    rb = ia.SimpleReplayBuffer(1 << 16, task.obs_dim, 1, ctx=ctx)
    for _ in range(120):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
    size, _ = rb._cursors()
    episodes, _ = env.rollout_stats(reset=True)
    assert episodes >= 2 * n
    b = rb._gather(np.arange(size))
    covered, short = np.zeros(size, bool), 0
    for s0, e0 in rb._traj_endpoints.items():
        rows = np.arange(s0, e0)
        assert 2 <= rows.size and not covered[rows].any()
        covered[rows] = True
        obs, nobs, term = b["observations"][rows], b["next_observations"][rows], b["terminals"][rows, 0]
        assert rows.size <= maxlen and np.array_equal(obs[1:], nobs[:-1])          # one env's consecutive steps
        assert not term[:-1].any()
        if rows.size < maxlen:
            assert term[-1] != 0                                                    # only done ends an episode early
            short += 1
        a = b["actions"][rows, 0]
        assert np.all(np.isin(a, (0, 1, 2))) if task.discrete_n else np.all(np.abs(a) < 1)
    # an episode of ONE terminal step is in the ring but not in the table: the reference's add_sample registers it and its _advance deletes
    # the entry again (simple_replay_buffer.py:95-98, 228-231), which the library mirrors.  Every row outside the table is such an episode.
    assert np.all(b["terminals"][~covered, 0] != 0) and int((~covered).sum()) == episodes - len(rb._traj_endpoints)
    assert short > 0
    env.close()


# ---------------------------------------------------------------------------------------------------- action handling
def test_actions_outside_the_box_are_clipped(ctx):
    task = MountainCarCont
    env = _env(ctx, task, 6)
    s = gr.parity_inputs(task, 6, 4)[0]
    a = np.array([3.0, -3.0, 1.5, -1.0001, 100.0, -1e6], F32)
    res = []
    for act in (a, np.clip(a, -1, 1)):
        _set(env, task, s)
        obs, rew, done, _ = env.step(act.reshape(6, 1))
        res.append((_state(env), rew, obs, done))
    for x, y in zip(*res):
        assert np.array_equal(x, y)
    _, wrew, _ = task.step(s, a)
    assert np.array_equal(res[0][1].astype(F32), wrew.astype(F32))
    env.close()


def test_wrong_kind_of_policy_is_refused(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.samplers import DeviceEvalSampler
    for task in (MountainCar, Acrobot):
        env = _env(ctx, task, 8, seed=2)
        gauss = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[64, 64], obs_dim=task.obs_dim, action_dim=1, ctx=ctx)
        with pytest.raises(RuntimeError, match="continuous policy on an env with a Discrete"):
            env.rollout_step(policy=gauss, max_path_length=200)
        env.close()
    env = _env(ctx, MountainCarCont, 8, seed=2)
    cat = ia.DiscretePolicy(hidden_sizes=[64, 64], obs_dim=2, action_dim=3, ctx=ctx)
    with pytest.raises(RuntimeError, match="categorical policy on an env with a Box"):
        env.rollout_step(policy=cat, max_path_length=200)
    with pytest.raises(RuntimeError, match="categorical policy on an env with a Box"):
        DeviceEvalSampler(env, ia.MakeDeterministic(cat), 10, 10).obtain_statistics()
    env.close()


# ---------------------------------------------------------------------------------------------------- trainers end to end
def test_discrete_sac_on_discrete3_end_to_end(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.discrete_sac import DiscreteSoftActorCritic
    from ilswiss_amd.samplers import DeviceEvalSampler
    n, hid = 64, [64, 64]
    env = _env(ctx, Acrobot, n, seed=7)
    pol = ia.DiscretePolicy(hidden_sizes=hid, obs_dim=6, action_dim=3, ctx=ctx)
    q1 = ia.FlattenMlp(hidden_sizes=hid, input_size=6, output_size=3, ctx=ctx)
    q2 = ia.FlattenMlp(hidden_sizes=hid, input_size=6, output_size=3, ctx=ctx)
    tr = DiscreteSoftActorCritic(pol, q1, q2, max_batch=64, alpha=0.05, discount=0.95, policy_lr=1e-4, qf_lr=1e-3, reward_scale=1.0,
                                 soft_target_tau=0.005)
    rb = ia.SimpleReplayBuffer(20 * n, 6, 1, ctx=ctx)
    env.reset()
    for _ in range(20):
        env.rollout_step(policy=pol, replay=rb, max_path_length=500)
    size, _ = rb._cursors()
    assert size == 20 * n
    b = rb._gather(np.arange(size))
    assert set(b["actions"][:, 0].tolist()) == {0.0, 1.0, 2.0}          # the categorical head draws all three indices and no other
    assert np.all(np.isin(b["rewards"], (-1.0, 0.0)))
    before = {k: tr.get_flat_params(k).copy() for k in ("policy", "qf1", "qf2", "target_qf1")}
    tr.end_epoch()
    tr.train_from_replay(rb, 5, 64)
    st = tr.get_eval_statistics()
    assert all(np.isfinite(st[k]) for k in ("QF1 Loss", "QF2 Loss", "Policy Loss"))
    for k, v in before.items():
        after = tr.get_flat_params(k)
        assert np.all(np.isfinite(after)) and not np.array_equal(after, v), k
    ev = DeviceEvalSampler(env, ia.MakeDeterministic(pol), 200, 100).obtain_statistics()
    assert ev["Num Paths"] >= n and ev["Test Rewards Min"] == -1.0 and ev["Test Rewards Max"] in (-1.0, 0.0)
    assert ev["Test Actions Min"] >= 0.0 and ev["Test Actions Max"] <= 2.0 and -100.0 <= ev["AverageReturn"] <= 0.0
    env.close()


def test_sac_alpha_on_the_continuous_car_end_to_end(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.samplers import DeviceEvalSampler
    n, hid = 64, [64, 64]
    env = _env(ctx, MountainCarCont, n, seed=7)
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=hid, obs_dim=2, action_dim=1, ctx=ctx)
    q1, q2 = ia.FlattenMlp(hid, 1, 3, ctx=ctx), ia.FlattenMlp(hid, 1, 3, ctx=ctx)
    tr = ia.SoftActorCritic(pol, q1, q2, max_batch=64, reward_scale=1.0, discount=0.99, policy_lr=1e-4, qf_lr=3e-4, alpha_lr=3e-4,
                            soft_target_tau=0.005, alpha=0.2, train_alpha=True, policy_mean_reg_weight=1e-3, policy_std_reg_weight=1e-3)
    rb = ia.SimpleReplayBuffer(20 * n, 2, 1, ctx=ctx)
    env.reset()
    for _ in range(20):
        env.rollout_step(policy=pol, replay=rb, max_path_length=100)
    size, _ = rb._cursors()
    assert size == 20 * n
    b = rb._gather(np.arange(size))
    assert np.all(np.abs(b["actions"]) <= 1) and b["actions"].std() > 1e-3
    f = MountainCarCont.force(b["actions"]).astype(np.float64)
    assert np.array_equal(b["rewards"][:, 0], (np.where(b["terminals"][:, 0] != 0, 100.0, 0.0) - (f * f) * 0.1).astype(F32))
    before = {k: tr.get_flat_params(k).copy() for k in ("policy", "qf1", "qf2")}
    tr.end_epoch()
    tr.train_from_replay(rb, 5, 64)
    st = tr.get_eval_statistics()
    assert all(np.isfinite(st[k]) for k in ("QF1 Loss", "QF2 Loss", "Policy Loss"))
    for k, v in before.items():
        after = tr.get_flat_params(k)
        assert np.all(np.isfinite(after)) and not np.array_equal(after, v), k
    ev = DeviceEvalSampler(env, ia.MakeDeterministic(pol), 200, 100).obtain_statistics()
    assert ev["Num Paths"] >= n and -0.1 - 1e-6 <= ev["Test Rewards Min"] <= ev["Test Rewards Max"] <= 100.0
    assert -1.0 <= ev["Test Actions Min"] <= ev["Test Actions Max"] <= 1.0
    env.close()


# ---------------------------------------------------------------------------------------------------- the C entry point
def test_create_classic_builds_kinds_4_to_6_and_refuses_7(ctx):
    lib = ctx.lib
    for task in gr.TASKS.values():
        h = C.c_void_p()
        assert lib.ilsx_vecenv_create_classic(ctx.h, task.kind, 4, C.c_uint64(5), C.byref(h)) == 0 and h.value
        o, a, n, ne, dn = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        assert lib.ilsx_vecenv_dims(h, C.byref(o), C.byref(a), C.byref(n), C.byref(ne)) == 0
        assert lib.ilsx_vecenv_action_space(h, C.byref(dn)) == 0
        assert (o.value, a.value, n.value, ne.value, dn.value) == (task.obs_dim, 1, task.nq, 4, task.discrete_n)
        lib.ilsx_vecenv_destroy(h)
    h = C.c_void_p()
    assert lib.ilsx_vecenv_create_classic(ctx.h, 7, 4, C.c_uint64(5), C.byref(h)) != 0 and not h.value
