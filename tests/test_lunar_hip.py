"""GPU suite for the LunarLanderContinuous stepper (k_lunar_step / k_lunar_reset of csrc/lunar_env.h) against the numpy restatement in
tests/lunar_restatement.py.  As in test_swimmer_hip.py every step is restated from the device's own previous state and the device's own
recorded action, so a difference cannot build up; the engines' dispersion and the reset draws are taken from the env's Philox stream
(oracle/philox.py) at the coordinates the library used: the env's seed, the stream id the context handed it, and the env's step counter
(1 for the creation-time reset, one more for every reset, step and rollout step after it).

State tolerance.  The states are not bit-identical (two libms, other summation orders); the largest relative state difference per step,
|got - want| / max(1, |want|), over lane-steps whose switch_margin exceeds 1e-9 is measured by run_parity and kept in
profiles/lunar_parity.json; every state comparison holds at 100x that figure, capped at 1e-9 (section 19's rule: the cap is a condition,
not a measurement).  Lane-steps within 1e-9 of a switch (a foot or hull vertex at the terrain, |s0| at 1, a speed at its sleep tolerance)
are left out of the state, observation and reward comparisons and may be at most 0.5 % of all; the restatement's own rollout at this size
and action distribution has 0 of 8400 (tests/test_lunar_cpu.py).  A done or contact flag that differs anywhere else is a failure.

Reward tolerance, derived from the state tolerance e.  shaping = -100 |(s0, s1)| - 100 |(s2, s3)| - 100 |s4| + 10 (s6 + s7); a norm moves
by at most the sum of its components' moves, and with equal contact flags a state error e moves
    s0 by e max(1, |x|) / (W / 2),  s1 by e max(1, |y|) / (H / 2),  s2 by e max(1, |vx|) (W / 2) / FPS,  s3 by e max(1, |vy|) (H / 2) / FPS,
    s4 by e max(1, |theta|),
so shaping(after) by at most 100 times their sum.  shaping(before) is computed on both sides from the same bits; its few roundings are
covered by 1e-13 (|shaping(before)| + |shaping(after)|).  The engine costs are exact functions of the float32 action.  One float32 ulp
of the reward is added because the device stores it as float32.  Terminal rewards (+-100) compare exactly."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import lunar_restatement as lr  # noqa: E402

CAP = 1e-9
SWITCH = 1e-9
F32 = dict(rtol=2.5e-7, atol=1e-12)     # float32 values of float64 quantities that agree to the state tolerance
NAME = "lunarlandercont"


@pytest.fixture(autouse=True)
def _leave_the_stream_cursor_where_it_was(request):
    """The session's context hands every random-drawing object the next Philox stream id.  The tests of this file put the cursor back, so
    that the files that run after it draw from the streams they drew from before this file existed."""
    if "ctx" not in request.fixturenames:
        yield
        return
    ctx = request.getfixturevalue("ctx")
    cursor = ctx.rng_stream_cursor()
    yield
    ctx.rng_stream_cursor(set_to=cursor)


def state_tol():
    p = json.load(open(os.path.join(ROOT, "profiles", "lunar_parity.json")))
    return min(100.0 * p["max_rel_state_diff"], CAP)


def _model(**kw):
    from ilswiss_amd.envs.models_lunar import lunar
    m = lunar()
    m.update(kw)
    return m


class Tracked:
    """A lander env together with the coordinates of its Philox stream."""

    def __init__(self, ctx, n, seed=3, **kw):
        from ilswiss_amd.envs import HipVectorEnv
        self.stream = ctx.rng_stream_cursor()          # the id the next random-drawing object of the context takes
        self.env = HipVectorEnv(NAME, n, seed=seed, ctx=ctx, **kw)
        self.seed, self.n, self.step = seed, n, 1      # the creation-time reset was step 1

    def tick(self):
        self.step += 1
        return self.step

    def dispersion(self, envs=None):
        return lr.draws(self.seed, self.stream, self.step, np.arange(self.n) if envs is None else envs, [14, 15])

    def reset_draws(self, envs=None):
        return lr.draws(self.seed, self.stream, self.step, np.arange(self.n) if envs is None else envs, list(range(14)))


def _rel(got, want):
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def _rew_tol(S, tol, wq, wv, before, after, rew):
    W, H, fps = S.W, S.H, S.fps
    big = lambda x: np.maximum(1.0, np.abs(x))  # noqa: E731
    move = (big(wq[:, 0]) / (W / 2) + big(wq[:, 1]) / (H / 2) + big(wv[:, 0]) * (W / 2) / fps + big(wv[:, 1]) * (H / 2) / fps + big(wq[:, 2]))
    return 100.0 * tol * move + 1e-13 * (np.abs(before) + np.abs(after)) + np.spacing(np.abs(rew).astype(np.float32)).astype(np.float64)


def _check_step(S, pq, pv, a, disp, gq, gv, obs, rew, done, tol, skip=None):
    """One device step against the restatement of it.  skip: lanes whose outcome is not the step's (they were reset afterwards).
    Returns (largest relative state difference over the compared lanes, lanes close to a switch, the restatement's outputs)."""
    want = S.step(pq, pv, a, disp)
    wq, wv, wobs, wrew, wdone, margin, _ = want
    close = margin <= SWITCH
    keep = ~close if skip is None else ~close & ~skip
    worst = max(float(_rel(gq[keep], wq[keep]).max(initial=0.0)), float(_rel(gv[keep], wv[keep]).max(initial=0.0)))
    assert worst <= tol, worst
    live = ~close
    if obs is not None:
        obs = np.asarray(obs, np.float32)
        assert np.array_equal(obs[live][:, 6:], wobs[live][:, 6:])                       # contact flags
        np.testing.assert_allclose(obs[live], wobs[live], **F32)
    if done is not None:
        assert np.array_equal(np.asarray(done, bool)[live], wdone[live])
    if rew is not None:
        rew = np.asarray(rew, np.float64)
        ended = wdone & live
        assert np.array_equal(rew[ended], wrew[ended])                                   # exactly +-100
        before, after = S.shaping(S.observe64(pq, pv)), S.shaping(S.observe64(wq, wv))
        ok = np.abs(rew - wrew) <= _rew_tol(S, tol, wq, wv, before, after, wrew)
        assert np.all(ok[live & ~wdone]), np.abs(rew - wrew)[live & ~wdone].max()
    return worst, close, want


@pytest.mark.gpu
def test_dims_spaces_and_state_round_trip(ctx):
    from ilswiss_amd.envs.vecenv import Box
    S = lr.Lunar(_model())
    T = Tracked(ctx, 4)
    env = T.env
    assert (env.obs_dim, env.act_dim, env.nq, env.nv, env.n_dof, env.discrete_n) == (8, 2, 14, 4, 3, 0)
    ac = env.action_space[0]
    assert isinstance(ac, Box) and ac.shape == (2,) and np.array_equal(ac.low, [-1, -1]) and np.array_equal(ac.high, [1, 1])
    assert env.observation_space[0].shape == (8,)
    tol = state_tol()
    # the creation-time reset and an explicit one, against the stream's draws
    for first in (True, False):
        if not first:
            T.tick()
            obs = env.reset()
        q, v = env.get_state()
        wq, wv = S.reset_from_draws(T.reset_draws())
        assert np.array_equal(q[:, 3:], wq[:, 3:]) and np.all(v[:, 3] == 0.0)            # the terrain is a few products: bit-exact
        assert max(_rel(q, wq).max(), _rel(v, wv).max()) <= tol
        if not first:
            np.testing.assert_allclose(obs.astype(np.float32), S.observe(q, v), **F32)
    rng = np.random.default_rng(4)
    sy = S.terrain_from_heights(rng.uniform(0, S.H / 2, (4, 12)))
    q = np.concatenate([rng.uniform(5, 15, (4, 1)), rng.uniform(8, 12, (4, 1)), rng.uniform(-0.5, 0.5, (4, 1)), sy], 1)
    v = np.concatenate([rng.uniform(-2, 2, (4, 3)), rng.uniform(0, 0.3, (4, 1))], 1)
    env.set_state(q, v)
    gq, gv = env.get_state()
    assert np.array_equal(gq, q) and np.array_equal(gv, v)                                # all 18 columns, bit for bit
    a = rng.uniform(-1, 1, (4, 2)).astype(np.float32)
    T.tick()
    obs, rew, done, _ = env.step(a)
    _check_step(S, q, v, a, T.dispersion(), *env.get_state(), obs, rew, done, tol)
    assert not done.any() and np.all(env.get_state()[1][:, 3] == 0.0)                     # moving: the sleep clock was cleared
    env.close()


def run_parity(ctx, tol, n=70, steps=120, maxlen=50, seed=11):
    """n envs, auto-resetting rollout steps with the device's random actions, path limit maxlen, fused insert into a capacity-n ring;
    every step restated from the device's previous state.  Returns (largest relative state difference over lane-steps away from a
    switch, lane-steps near a switch, lane-steps); asserts everything at `tol`."""
    import ilswiss_amd as ia
    S = lr.Lunar(_model())
    T = Tracked(ctx, n, seed=seed)
    env = T.env
    env.rollout_stats(reset=True)
    rb = ia.SimpleReplayBuffer(n, 8, 2, ctx=ctx)       # capacity n: step t's record of env i sits at slot i
    pq, pv = env.get_state()
    ep_len, ep_ret = np.zeros(n, int), np.zeros(n)
    worst, near, episodes, ret_sum = 0.0, 0, 0, 0.0
    for t in range(steps):
        env.rollout_step(replay=rb, max_path_length=maxlen, random_actions=True)
        T.tick()
        rec = rb._gather(np.arange(n))
        a = rec["actions"]
        assert a.shape == (n, 2) and np.all(np.abs(a) < 1)
        np.testing.assert_allclose(rec["observations"], S.observe(pq, pv), **F32)
        gq, gv = env.get_state()
        dev_done = rec["terminals"][:, 0] != 0
        ep_len += 1
        end = dev_done | (ep_len >= maxlen)
        w, close, want = _check_step(S, pq, pv, a, T.dispersion(), gq, gv, rec["next_observations"], rec["rewards"][:, 0], dev_done, tol, skip=end)
        worst, near = max(worst, w), near + int(close.sum())
        ep_ret += want[3]
        if end.any():                                    # the ended envs were reset at this step's coordinates
            ids = np.flatnonzero(end)
            wq, wv = S.reset_from_draws(T.reset_draws(ids))
            assert np.array_equal(gq[ids, 3:], wq[:, 3:])
            assert max(_rel(gq[ids], wq).max(), _rel(gv[ids], wv).max()) <= tol
        episodes += int(end.sum()); ret_sum += float(ep_ret[end].sum())
        ep_len[end], ep_ret[end] = 0, 0.0
        pq, pv = gq, gv
    e, r = env.rollout_stats(reset=True)
    assert e == episodes and episodes >= (steps // maxlen) * n
    np.testing.assert_allclose(r, ret_sum, rtol=1e-6, atol=1e-6)
    assert near <= 0.005 * n * steps, (near, n * steps)
    env.close()
    return worst, near, n * steps


@pytest.mark.gpu
def test_rollout_steps_match_the_restatement(ctx):
    print("largest relative state difference, lane-steps near a switch, lane-steps:", run_parity(ctx, state_tol()))


@pytest.mark.gpu
def test_block_boundary(ctx):
    print(run_parity(ctx, state_tol(), n=257, steps=20, maxlen=8, seed=5))


@pytest.mark.gpu
def test_listed_envs_step_and_the_rest_stay(ctx):
    S = lr.Lunar(_model())
    n, ids = 64, np.array([63, 0, 17, 40, 5])
    T = Tracked(ctx, n, seed=9)
    env = T.env
    rng = np.random.default_rng(8)
    for _ in range(3):
        q, v = env.get_state()
        a = rng.uniform(-1, 1, (5, 2)).astype(np.float32)
        T.tick()
        obs, rew, done, _ = env.step(a, id=ids)
        gq, gv = env.get_state()
        rest = np.setdiff1d(np.arange(n), ids)
        assert np.array_equal(gq[rest], q[rest]) and np.array_equal(gv[rest], v[rest])
        assert obs.shape == (5, 8)
        _check_step(S, q[ids], v[ids], a, T.dispersion(ids), gq[ids], gv[ids], obs, rew, done, state_tol())
    env.close()


@pytest.mark.gpu
def test_evaluation_freezes_ended_envs(ctx):
    """One evaluation round (one episode per env, ended envs frozen, not reset) under a policy whose weights are all zero: its
    deterministic action is exactly 0, the engines never fire and every lander falls to the ground, where it crashes, falls asleep or
    lies awake until the path limit, so the round can be restated from the reset draws alone.  The restatement runs the whole episode on its own here, so states are compared at 1e-6 (about 75 steps
    of accumulated rounding through one hard touchdown), not at the one-step tolerance; episode lengths and the -100 compare exactly
    unless the restatement's episode passed within 1e-9 of a switch."""
    import ilswiss_amd as ia
    from ilswiss_amd.samplers import DeviceEvalSampler
    S = lr.Lunar(_model())
    n, K = 64, 160
    T = Tracked(ctx, n, seed=21)
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[32, 32], obs_dim=8, action_dim=2, ctx=ctx)
    pol.set_flat_params(np.zeros_like(pol.get_flat_params()))
    st = DeviceEvalSampler(T.env, ia.MakeDeterministic(pol), 1, K).obtain_statistics()
    T.tick()                                             # the round's reset
    q, v = S.reset_from_draws(T.reset_draws())
    alive, length, ret, safe = np.ones(n, bool), np.zeros(n, int), np.zeros(n), np.ones(n, bool)
    fq, fv = q.copy(), v.copy()
    for _ in range(K):
        q2, v2, _, rew, done, margin, _ = S.step(q, v, np.zeros((n, 2), np.float32))
        safe &= ~alive | (margin > SWITCH)
        length += alive; ret += np.where(alive, rew, 0.0)
        fq[alive], fv[alive] = q2[alive], v2[alive]
        alive &= ~done
        q, v = q2, v2
    assert (~alive).mean() > 0.5 and length.min() > 25    # most episodes ended inside the round, none at once
    gq, gv = T.env.get_state()
    assert safe.mean() > 0.9
    assert np.array_equal(gq[:, 3:], fq[:, 3:])
    assert max(_rel(gq[safe], fq[safe]).max(), _rel(gv[safe], fv[safe]).max()) < 1e-6     # frozen where the episode ended
    assert st["Num Paths"] == n
    if safe.all():
        assert st["Test Ep. Len. Max"] == length.max() and st["Test Ep. Len. Min"] == length.min()
        np.testing.assert_allclose(st["AverageReturn"], ret.mean(), rtol=1e-5)    # the device sums the float32 rewards
    T.env.close()


def _scenarios(S):
    """Eight landers placed by hand: (q, v, actions per step as a function of t, what must happen)."""
    m = S.m
    W, H = S.W, S.H
    flat = S.terrain_from_heights(np.full((1, 12), m["helipad_y"]))[0]
    slope = S.terrain_from_heights(np.linspace(6.0, 0.5, 12)[None])[0]
    pad_y = flat[5] - m["foot"][0][1] - 1e-6               # both feet a micrometre inside the pad: at the surface, not ON the switch
    t = np.array([2.0, slope[2] - slope[1]]); t /= np.hypot(*t)
    nrm = np.array([-t[1], t[0]])
    on_line = np.array([3.5, slope[1] + (slope[2] - slope[1]) * 1.5 / 2.0])
    origin = on_line - 1e-3 * nrm - np.array(m["foot"][0])
    rows = [
        ([W / 2, pad_y, 0.0], flat, [0, 0, 0], (0.0, 0.0)),              # 0 landing: +100 after the sleep time
        ([W / 2, pad_y, np.pi / 2], flat, [0, 0, 0], (0.0, 0.0)),        # 1 crash: -100 by game_over
        ([W + 0.01, 10.0, 0.0], flat, [0, 0, 0], (0.0, 0.0)),            # 2 out of bounds at once
        ([0.3, 10.0, 0.0], flat, [-3.1, 0, 0], (0.0, 0.0)),              # 3 drifting out of bounds on the left
        ([8.0, 12.0, 0.0], flat, [0, 0, 0], (0.0, 0.5)),                 # 4 side-engine dead zone: |a1| = 0.5 fires nothing
        ([12.0, 12.0, 0.0], flat, [0, 0, 0], (0.0, 0.5000001)),          # 5 ... and just past it fires
        ([6.0, 12.0, 0.2], flat, [0, 0, 0], (0.0, 0.0)),                 # 6 main engine off at a0 = 0
        ([origin[0], origin[1], 0.0], slope, [0, 0, 0], (0.0, 0.0)),     # 7 one foot in contact on a sloped segment
    ]
    q = np.array([list(p) + list(sy) for p, sy, _, _ in rows])
    v = np.array([list(u) + [0.0] for _, _, u, _ in rows])
    a = np.array([act for _, _, _, act in rows], np.float32)
    return q, v, a


@pytest.mark.gpu
def test_scenarios_through_set_state(ctx):
    S = lr.Lunar(_model())
    q, v, a = _scenarios(S)
    T = Tracked(ctx, 8, seed=2)
    env = T.env
    env.set_state(q, v)
    o0 = S.observe(q, v)
    assert np.array_equal(o0[:, 6:], [[1, 1], [1, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [1, 0]])
    tol = state_tol()
    first_done, first_rew = np.full(8, -1), np.zeros(8)
    want_done = np.full(8, -1)
    rq, rv = q.copy(), v.copy()                          # the restatement's own run, for the step at which each outcome arrives
    fired = None
    for t in range(55):
        pq, pv = env.get_state()
        T.tick()
        obs, rew, done, _ = env.step(a)
        gq, gv = env.get_state()
        fresh = first_done < 0
        _, close, want = _check_step(S, pq, pv, a, T.dispersion(), gq, gv, obs, rew, done, tol, skip=~fresh)
        assert not close[fresh].any()
        if t == 0:
            fired = (S.engines(pq, a, T.dispersion())[2:], rew.copy(), want[3].copy())
        rq, rv, _, _, rdone, _, _ = S.step(rq, rv, a, T.dispersion())
        want_done[(want_done < 0) & rdone] = t
        new = fresh & done
        first_done[new], first_rew[new] = t, rew[new]
    m_power, s_power = fired[0]
    assert np.all(m_power == 0.0) and np.array_equal(s_power > 0, [0, 0, 0, 0, 0, 1, 0, 0])      # the dead zone, a0 = 0
    assert s_power[5] == float(np.float32(0.5000001))
    assert first_rew[0] == 100.0 and 25 <= first_done[0] <= 54                                    # asleep after the sleep time
    assert first_rew[1] == -100.0 and first_rew[2] == -100.0 and first_done[2] == 0 and first_rew[3] == -100.0
    assert np.all(first_done[4:7] < 0)                                                             # the free fliers are still up
    assert np.array_equal(first_done, want_done)                                                   # every outcome at the restatement's step
    env.close()


@pytest.mark.gpu
def test_no_terminal_and_path_mode(ctx):
    import ilswiss_amd as ia
    S = lr.Lunar(_model())
    q, v, a = _scenarios(S)
    # no_terminal is the library's (and the reference's, base_algorithm.py:195-196 ahead of :215) for every task: the stored terminal is
    # forced to 0 and a done env is stepped on; the path limit still ends the episode.  The out-of-bounds lander keeps collecting -100.
    T = Tracked(ctx, 8, seed=4)
    T.env.set_state(q, v)
    T.env.rollout_stats(reset=True)
    rb = ia.SimpleReplayBuffer(8, 8, 2, ctx=ctx)
    for t in range(3):
        T.env.rollout_step(replay=rb, max_path_length=3, random_actions=True, no_terminal=True)
        T.tick()
        rec = rb._gather(np.arange(8))
        assert not rec["terminals"].any() and rec["rewards"][2, 0] == -100.0
        gq, gv = T.env.get_state()
        if t < 2:
            assert np.array_equal(gq[:, 3:], q[:, 3:]) and gq[2, 0] > S.W          # nobody was reset, the lost lander flies on
            assert T.env.rollout_stats(reset=False)[0] == 0
    wq, wv = S.reset_from_draws(T.reset_draws())                                    # the path limit ended all eight
    assert np.array_equal(gq[:, 3:], wq[:, 3:]) and max(_rel(gq, wq).max(), _rel(gv, wv).max()) <= state_tol()
    assert T.env.rollout_stats(reset=True)[0] == 8
    T.env.close()
    # path mode: whole episodes enter the ring when they end; the terminal bit is set where the restatement says done
    T = Tracked(ctx, 8, seed=4)
    env = T.env
    env.set_path_mode(True)
    env.set_state(q, v)
    rb = ia.SimpleReplayBuffer(1 << 10, 8, 2, ctx=ctx)
    maxlen, ends = 12, []
    ep_len = np.zeros(8, int)
    for t in range(30):
        pq, pv = env.get_state()
        env.rollout_step(policy=None, replay=rb, max_path_length=maxlen, random_actions=True)
        T.tick()
        ep_len += 1
        gq, gv = env.get_state()
        # which envs ended: their sleep clock and terrain were redrawn, or the path limit was reached
        ended = (ep_len >= maxlen) | np.any(gq[:, 3:] != pq[:, 3:], 1)
        ends += [(int(i), int(ep_len[i])) for i in np.flatnonzero(ended)]
        ep_len[ended] = 0
    size, _ = rb._cursors()
    assert size == sum(n for _, n in ends) and (2, 1) in ends
    b = rb._gather(np.arange(size))
    # the ring's cursor rule is the reference's (simple_replay_buffer.py add_sample, then _advance): an episode of ONE step that ends
    # with a terminal registers its start and loses it again in the same insert; every other episode is registered
    lengths = sorted(e - s for s, e in rb._traj_endpoints.items())
    assert lengths == sorted(n for _, n in ends if n > 1)
    n_terminal = 0
    for s, e in rb._traj_endpoints.items():
        rows = np.arange(s, e)
        assert np.array_equal(b["observations"][rows][1:], b["next_observations"][rows][:-1])
        assert not b["terminals"][rows[:-1]].any()
        last = rows[-1]
        if b["terminals"][last, 0]:
            n_terminal += 1
            assert abs(b["rewards"][last, 0]) == 100.0 and len(rows) <= maxlen
        else:
            assert len(rows) == maxlen and abs(b["rewards"][last, 0]) != 100.0
    assert n_terminal >= 1                                # the lander that drifts out of bounds
    assert b["terminals"][0, 0] == 1 and b["rewards"][0, 0] == -100.0          # row 0: the one-step episode of the lander that started outside
    env.close()


@pytest.mark.gpu
def test_creation_errors_leak_nothing(ctx):
    from ilswiss_amd.envs.vecenv import lunar_struct
    T = Tracked(ctx, 8, seed=2)
    sh, sc = np.zeros(8), np.ones(8)
    assert ctx.lib.ilsx_vecenv_set_obs_affine(T.env.h, sh.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p)) != 0
    T.env.close()
    n = C.c_size_t()
    assert ctx.lib.ilsx_debug_ctx_allocs(ctx.h, C.byref(n)) == 0
    before = n.value
    bad = [_model(mass=0.0), _model(inertia=-1.0), _model(fps=0.0), _model(frame_skip=0), _model(contact_solref=(0.0, 1.0)),
           _model(contact_solimp=(0.9, 0.0, 0.001)), _model(sleep_lin_tol=0.0), _model(gravity=float("nan")), _model(side_engine_power=float("inf"))]
    for m in bad:
        h = C.c_void_p()
        ms = lunar_struct(m)
        assert ctx.lib.ilsx_vecenv_create_lunar(ctx.h, C.byref(ms), 4, C.c_uint64(1), C.byref(h)) != 0 and not h.value
    ms = lunar_struct(_model())
    ms.foot[1][1] = 0.0                                   # a foot above the hull's bottom, past the Python check
    h = C.c_void_p()
    assert ctx.lib.ilsx_vecenv_create_lunar(ctx.h, C.byref(ms), 4, C.c_uint64(1), C.byref(h)) != 0 and not h.value
    assert ctx.lib.ilsx_vecenv_create_classic(ctx.h, 17, 4, C.c_uint64(1), C.byref(h)) != 0 and not h.value
    for _ in range(50):
        Tracked(ctx, 50, seed=1).env.close()
    assert ctx.lib.ilsx_debug_ctx_allocs(ctx.h, C.byref(n)) == 0
    assert n.value == before


@pytest.mark.gpu
def test_trainers_take_lander_rollouts(ctx):
    """Wiring only: three SAC-V gradient steps on a batch the fused rollout recorded, one PPO update on its own rollout; finite weights."""
    import ilswiss_amd as ia
    from ilswiss_amd.envs import get_env, get_envs
    from ilswiss_amd.ppo import PPO, ReparamMultivariateGaussianPolicy
    from ilswiss_amd.sac_v import SoftActorCriticV
    n = 64
    env = get_envs(dict(env_name=NAME, env_num=n, training_env_seed=1), ctx=ctx)
    ev = get_env(dict(env_name=NAME, eval_env_seed=2), ctx=ctx)
    assert len(env) == n and env.reset().shape == (n, 8) and ev.reset().shape == (1, 8)
    ev.close()
    hid = [32, 32]
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=hid, obs_dim=8, action_dim=2, ctx=ctx)
    q1, q2 = ia.FlattenMlp(hid, 1, 10, ctx=ctx), ia.FlattenMlp(hid, 1, 10, ctx=ctx)
    vf = ia.FlattenMlp(hid, 1, 8, ctx=ctx)
    rb = ia.SimpleReplayBuffer(4 * n, 8, 2, ctx=ctx)
    for _ in range(4):
        env.rollout_step(policy=pol, replay=rb, max_path_length=1000)
    size, _ = rb._cursors()
    batch = rb._gather(np.arange(size))
    assert size == 4 * n and all(np.isfinite(batch[k]).all() for k in batch)
    tr = SoftActorCriticV(pol, q1, q2, vf, max_batch=size, alpha=0.2)
    rng = np.random.default_rng(0)
    for _ in range(3):
        tr.train_step(batch, eps=rng.normal(0, 1, (size, 2)).astype(np.float32))
    assert all(np.isfinite(tr.get_flat_params(k)).all() for k in ("pi", "q1", "q2", "vf"))
    gp = ReparamMultivariateGaussianPolicy(hid, 8, 2, conditioned_std=False, hidden_activation="tanh", ctx=ctx)
    pvf = ia.FlattenMlp(hid, 1, 8, hidden_activation="tanh", ctx=ctx)
    ppo = PPO(gp, pvf, mini_batch_size=n * 4, update_epoch=1, gae_tau=0.95, max_samples=n * 4)
    assert ppo.train_from_rollout(env, 4, max_path_length=1000) == n * 4
    assert np.isfinite(ppo.get_flat_params(0)).all() and np.isfinite(ppo.get_flat_params(1)).all()
    env.close()
