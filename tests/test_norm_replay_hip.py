"""GPU suite for off-policy rollouts with norm_obs: the replay ring of a normalising env records what the policy saw (k_obs_norm_record,
csrc/ilsx_env.hip; contract in DESIGN.md, "Off-policy rollouts with norm_obs").

Every case but the policy ones steps with random_actions=True, so that a TWIN — an env without normalisation created on the same seed with
the context's rng_stream_cursor moved back to the same value, recording into a ring of its own — follows the same raw trajectory.  The twin's
ring holds the raw rows; tests/norm_rollout_restatement.py turns them into the rows the normalising env must have recorded.
70 envs (a full wavefront and a partial one), max_path_length 5, 12 steps: path-limit resets happen in two different steps.  Hopper also
runs at 4096 and 4097 envs, the two sides of the kernel's switch between its two forms.

Tolerance of a normalised column: one float32 ulp of the float64 expectation cast to float32, plus 1e-9 absolute — the device sums a column in
another order than numpy, which moves z by parts in 1e-13 even on a near-constant column, and the cast can then round the other way.  The
statistics: rtol 1e-9 / atol 1e-12 and an exact count, as test_loop_hip.py::test_device_obs_rms_matches_running_mean_std."""
import csv
import ctypes as C
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from norm_rollout_restatement import make_rms, replay_norm_rollout  # noqa: E402

from oracle.envnorm import RunningMeanStd, normalize_obs  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, MPL, T = 70, 5, 12
TASKS = ("hopper", "ant", "pendulum", "cartpole")
KEYS = ("observations", "actions", "rewards", "terminals", "next_observations", "absorbing")
# (task, envs): every task at 70 envs; Hopper also at the two sizes around the kernel's switch from rows held in registers (up to 4096 envs) to
# rows re-read from memory
SHAPES = [(t, 70) for t in TASKS] + [("hopper", 4096), ("hopper", 4097)]
DESYNC = dict(hopper=(2, 0.5), cartpole=(0, 3.0))   # (qpos column, value): a torso angle past Hopper's 0.2 rad, a cart past CartPole's 2.4 m


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[x.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _envs_on_one_stream(ctx, name, kws, seed=11, n=N):
    """One env per keyword set, all on the same seed AND the same Philox stream id: they draw the same resets and the same random actions."""
    from ilswiss_amd.envs import HipVectorEnv
    cur = ctx.rng_stream_cursor()
    out = []
    for kw in kws:
        ctx.rng_stream_cursor(set_to=cur)
        out.append(HipVectorEnv(name, n, seed=seed, ctx=ctx, **kw))
    return out


def _policy_input(env):
    p = C.c_void_p()
    from ilswiss_amd import _lib
    from ilswiss_amd.device import host_ptr
    _lib.check(env.ctx.lib.ilsx_vecenv_cur_obs(env.h, C.byref(p)))
    out = np.empty((env.env_num, env.obs_dim), np.float32)
    _lib.check(env.ctx.lib.ilsx_memcpy_d2h(env.ctx.h, host_ptr(out), p, out.nbytes))
    return out


def _ring(ctx, env, cap=1024):
    import ilswiss_amd as ia
    return ia.SimpleReplayBuffer(cap, env.obs_dim, env.act_dim, ctx=ctx)


def _rows(rb, n_rows):
    b = rb._gather(np.arange(n_rows))
    return {k: np.ascontiguousarray(b[k]) for k in KEYS}


def _close_ulp(got, want64, what):
    want = np.asarray(want64, np.float64).astype(np.float32)
    tol = np.spacing(np.abs(want)).astype(np.float64) + 1e-9
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{what}: {float((got != want).mean()):.4%} of {got.size} elements differ from float32(expectation), worst {diff.max():.3e}")
    assert (diff <= tol).all(), (what, diff.max())


_CACHE = {}


def _scenario(ctx, name, preset=None, update=True, n=N):
    """The runs the cases share, made once per (task, preset): the normalising env with a ring (transition mode), its raw twin, a normalising
    env WITHOUT a ring on the existing chain, and the normalising env in path mode; T random-action steps each.  preset = (mean, var, count)
    given to obs_rms.set before the first step.  update=False: the statistics are never fed (an eval env's setting)."""
    key = (name, preset is not None, update, n)
    if key in _CACHE:
        return _CACHE[key]
    norm_kw = dict(norm_obs=True, update_obs_rms=update)
    env, twin, chain, penv = _envs_on_one_stream(ctx, name, [norm_kw, {}, norm_kw, norm_kw], n=n)
    N = n   # (the module's N is the default)
    o = env.obs_dim
    rms = RunningMeanStd()
    if update:
        rms.update(_policy_input(twin).astype(np.float64))   # turning norm_obs on shows the env's current observations to the statistics
    if name in DESYNC:   # every third env starts outside the task's healthy range: its episode ends in the first step, and from then on
        col, val = DESYNC[name]   # a third of the envs reaches the path limit one step after the others
        q, v = twin.get_state()
        q[::3, col] = val
        for e in (env, twin, chain, penv):
            e.set_state(q, v)
    raw0 = _policy_input(twin)
    if preset is not None:
        mean, var, count = preset(o)
        rms = make_rms(mean, var, count)
        for e in (env, chain, penv):
            e.obs_rms.set(mean, var, count)
    obs_n0 = normalize_obs(raw0.astype(np.float64), rms) + np.zeros((N, o))
    S = dict(name=name, n=n, o=o, a=env.act_dim, obs_n0_dev=_policy_input(env), obs_n0=obs_n0)
    cap = 1024 if T * n < 1024 else 65536
    rb, rbt, rbp = _ring(ctx, env, cap), _ring(ctx, env, cap), _ring(ctx, env, cap)
    penv.set_path_mode(True)
    for t in range(T):
        env.rollout_step(replay=rb, max_path_length=MPL, random_actions=True)
        twin.rollout_step(replay=rbt, max_path_length=MPL, random_actions=True)
        chain.rollout_step(max_path_length=MPL, random_actions=True)
        penv.rollout_step(replay=rbp, max_path_length=MPL, random_actions=True)
    S["rows"], S["raw"] = _rows(rb, T * N), _rows(rbt, T * N)
    S["size"], S["size_twin"] = rb._size, rbt._size
    S["path_rows"], S["path_size"], S["path_endpoints"] = _rows(rbp, max(rbp._size, 1)), rbp._size, rbp._traj_endpoints
    S["last_raw"], S["last_obs_n"] = _policy_input(twin), _policy_input(env)
    S["stats"] = {k: e.obs_rms._get() for k, e in (("ring", env), ("chain", chain), ("path", penv))}
    S["chain_obs_n"] = _policy_input(chain)
    # which envs were reset after which step, and to what: the twin's next policy input differs from the step's own next observation
    steps = []
    for t in range(T):
        nxt = S["raw"]["next_observations"][t * N:(t + 1) * N]
        after = S["raw"]["observations"][(t + 1) * N:(t + 2) * N] if t + 1 < T else S["last_raw"]
        ids = np.nonzero((_bits(nxt) != _bits(after)).any(axis=1))[0]
        steps.append(dict(nobs=nxt.astype(np.float64), reset_ids=ids, reset_obs=after[ids].astype(np.float64)))
    S["steps"] = steps
    S["want"] = replay_norm_rollout(rms, obs_n0, steps, update=update)
    for e in (env, twin, chain, penv):
        e.close()
    _CACHE[key] = S
    return S


def _check_against_restatement(S):
    rows, raw, want, N = S["rows"], S["raw"], S["want"], S["n"]
    assert S["size"] == T * N and S["size_twin"] == T * N
    for k in ("actions", "rewards", "terminals", "absorbing"):
        assert _same(rows[k], raw[k]), k                                  # what the same step writes without normalisation
    n_reset = [len(s["reset_ids"]) for s in S["steps"]]
    print(f"{S['name']}: envs reset after each step {n_reset}, terminal rows {int(raw['terminals'].sum())}")
    assert sum(1 for c in n_reset if c) >= 2                              # path-limit resets in two different steps
    if S["name"] in DESYNC:
        assert sum(1 for c in n_reset if 0 < c < N) >= 3                  # steps in which some envs reset and the others do not
    _close_ulp(rows["observations"], np.concatenate([w["obs"] for w in want]), f"{S['name']} obs")
    _close_ulp(rows["next_observations"], np.concatenate([w["next"] for w in want]), f"{S['name']} next_obs")
    _close_ulp(S["last_obs_n"], want[-1]["obs_n"], f"{S['name']} policy input after the last step")
    m, v, c = S["stats"]["ring"]
    np.testing.assert_allclose(m, want[-1]["mean"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(v, want[-1]["var"], rtol=1e-9, atol=1e-12)
    assert c == want[-1]["count"]


# ---------------------------------------------------------------------------------------------- 1. records against the restatement
@pytest.mark.parametrize("name,N", SHAPES)
def test_records_match_the_restatement(ctx, name, N):
    S = _scenario(ctx, name, n=N)
    _check_against_restatement(S)
    assert _same(S["rows"]["observations"][:N], S["obs_n0_dev"])          # the first segment is, bit for bit, what the policy read
    assert not _same(S["rows"]["observations"], S["raw"]["observations"])
    assert S["stats"]["ring"][2] == N + T * N + sum(len(s["reset_ids"]) for s in S["steps"])


def _tight(o):
    return np.zeros(o), np.full(o, 1e-4), 1


def test_records_are_clipped_at_ten(ctx):
    """Statistics preset to mean 0, var 1e-4, count 1: the policy's first input, and so the first records' observation segment, is clipped
    wherever the raw value is farther than 0.1 from zero (Hopper's height and more).  The first real batch then swamps the count of 1."""
    S = _scenario(ctx, "hopper", preset=_tight)
    _check_against_restatement(S)
    first = S["rows"]["observations"][:N]
    assert (np.abs(first) == 10.0).any(axis=1).all() and (np.abs(first) < 10.0).any()
    assert np.abs(S["rows"]["observations"]).max() <= 10.0 and np.abs(S["rows"]["next_observations"]).max() <= 10.0


def test_statistics_that_are_not_fed(ctx):
    """update_obs_rms off on preset statistics (an eval env's setting): every step normalises, nothing updates — and with var 1e-4 the clip is
    active in both observation segments of every step."""
    S = _scenario(ctx, "hopper", preset=_tight, update=False)
    _check_against_restatement(S)
    m, v, c = S["stats"]["ring"]
    assert c == 1 and (m == 0).all() and (v == 1e-4).all()
    assert (np.abs(S["rows"]["next_observations"]) == 10.0).any(axis=1).all()


# ---------------------------------------------------------------------------------------------- 2. statistics: the existing kernels' bits
@pytest.mark.parametrize("name,N", SHAPES)
def test_statistics_equal_the_no_ring_chain_bit_for_bit(ctx, name, N):
    S = _scenario(ctx, name, n=N)
    for k in ("path", "chain"):
        for got, want in zip(S["stats"][k], S["stats"]["ring"]):
            assert _same(np.asarray(got), np.asarray(want)), k
    # the no-ring path is unchanged: it re-normalises every row under the newest statistics, reset or not
    _close_ulp(S["chain_obs_n"], normalize_obs(S["last_raw"].astype(np.float64), make_rms(*S["stats"]["ring"])), f"{name} no-ring policy input")


# ---------------------------------------------------------------------------------------------- 3. the chain property on the device
@pytest.mark.parametrize("name,N", SHAPES)
def test_next_observation_is_the_next_records_observation(ctx, name, N):
    S = _scenario(ctx, name, n=N)
    rows, want = S["rows"], S["want"]
    kept = reset = 0
    for t in range(T):
        nxt = rows["next_observations"][t * N:(t + 1) * N]
        after = rows["observations"][(t + 1) * N:(t + 2) * N] if t + 1 < T else S["last_obs_n"]
        ids = S["steps"][t]["reset_ids"]
        keep = np.setdiff1d(np.arange(N), ids)
        assert _same(after[keep], nxt[keep]), t                           # the same bits, not normalised again under newer statistics
        kept += keep.size
        if ids.size:
            post = make_rms(want[t]["mean"], want[t]["var"], want[t]["count"])
            _close_ulp(after[ids], normalize_obs(S["steps"][t]["reset_obs"], post), f"{name} reset rows after step {t}")
            assert not _same(after[ids], nxt[ids])
            reset += ids.size
    print(f"{name}: {kept} rows carried over, {reset} rows reset")
    assert kept and reset
    # old rows are never re-normalised: the statistics moved during the run, and the first step's rows still match their own step's
    assert not np.allclose(want[0]["mean"], want[-1]["mean"], rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------- 4. path mode
@pytest.mark.parametrize("name,N", SHAPES)
def test_path_mode_rows_are_the_transition_mode_rows(ctx, name, N):
    S = _scenario(ctx, name, n=N)
    rows = S["rows"]
    start = np.zeros(N, np.int64)                                         # the step each env's running episode began in
    order, endpoints, top = [], {}, 0
    for t in range(T):
        for e in S["steps"][t]["reset_ids"]:                              # ended envs in ascending order, each episode contiguous
            length = t + 1 - start[e]
            order += [(s, e) for s in range(start[e], t + 1)]
            if length > 1 or not rows["terminals"][t * N + e, 0]:         # (add_sample's cursor logic drops a one-sample trajectory that ends
                endpoints[top] = top + length                              # terminal: its start is the slot _advance writes next,
            top += length                                                  # simple_replay_buffer.py:78-108)
            start[e] = t + 1
    assert S["path_size"] == len(order) and len(order) >= N
    idx = np.array([s * N + e for s, e in order])
    for k in KEYS:
        assert _same(S["path_rows"][k][:len(order)], rows[k][idx]), k
    assert S["path_endpoints"] == endpoints


# ---------------------------------------------------------------------------------------------- 5. policy and DAgger
def test_the_recorded_action_is_the_policys_for_the_recorded_observation(ctx):
    import ilswiss_amd as ia
    env, twin = _envs_on_one_stream(ctx, "hopper", [dict(norm_obs=True), {}])
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[64, 64], obs_dim=env.obs_dim, action_dim=env.act_dim, init_w=0.5, ctx=ctx, seed=5)
    rb = _ring(ctx, env)
    raw0 = _policy_input(twin)
    for _ in range(3):
        env.rollout_step(policy=pol, replay=rb, max_path_length=MPL, deterministic=True)
    b = _rows(rb, 3 * N)
    want = pol.get_actions(b["observations"], deterministic=True)
    np.testing.assert_allclose(b["actions"], want, rtol=0, atol=1e-6)
    on_raw = pol.get_actions(raw0, deterministic=True)
    assert np.abs(b["actions"][:N] - on_raw).max() > 1e-2                 # ... and not the policy's for the raw observation
    assert np.abs(want).max() > 0.05 and len({tuple(r) for r in want[:N].tolist()}) == N
    env.close(), twin.close()


def test_the_recorded_label_is_the_experts_for_the_recorded_observation(ctx):
    import ilswiss_amd as ia
    (env,) = _envs_on_one_stream(ctx, "hopper", [dict(norm_obs=True)])
    kw = dict(hidden_sizes=[64, 64], obs_dim=env.obs_dim, action_dim=env.act_dim, init_w=0.5, ctx=ctx)
    pol, expert = ia.ReparamTanhMultivariateGaussianPolicy(seed=5, **kw), ia.ReparamTanhMultivariateGaussianPolicy(seed=6, **kw)
    rb = _ring(ctx, env)
    seen = []
    for _ in range(3):
        seen.append(_policy_input(env))
        env.rollout_step(policy=pol, replay=rb, max_path_length=MPL, label_policy=ia.MakeDeterministic(expert))
    b = _rows(rb, 3 * N)
    assert _same(b["observations"], np.concatenate(seen))
    np.testing.assert_allclose(b["actions"], expert.get_actions(b["observations"], deterministic=True), rtol=0, atol=1e-6)
    assert np.abs(b["actions"] - pol.get_actions(b["observations"], deterministic=True)).max() > 1e-2
    env.close()


# ---------------------------------------------------------------------------------------------- 6. lock-step
def test_lockstep_equals_single_steps(ctx):
    """Two normalising runs through ilsx_rollout_steps_lockstep (six random-action steps while the rings fill, then six deterministic policy
    steps) against the same two runs stepped with ilsx_rollout_step."""
    import ilswiss_amd as ia
    from ilswiss_amd import _lib
    a1, a2 = _envs_on_one_stream(ctx, "hopper", [dict(norm_obs=True)] * 2, seed=3)
    b1, b2 = _envs_on_one_stream(ctx, "hopper", [dict(norm_obs=True)] * 2, seed=4)
    kw = dict(hidden_sizes=[64, 64], obs_dim=a1.obs_dim, action_dim=a1.act_dim, init_w=0.5, ctx=ctx)
    pa, pb = ia.ReparamTanhMultivariateGaussianPolicy(seed=5, **kw), ia.ReparamTanhMultivariateGaussianPolicy(seed=6, **kw)
    rings = [_ring(ctx, a1) for _ in range(4)]
    ra1, ra2, rb1, rb2 = rings
    fill = 6 * N
    vp = C.c_void_p
    envs, pis, rbs, mins = (vp * 2)(a1.h, b1.h), (vp * 2)(pa.h, pb.h), (vp * 2)(ra1.h, rb1.h), (C.c_int64 * 2)(fill, fill)
    _lib.check(ctx.lib.ilsx_rollout_steps_lockstep(envs, pis, rbs, 2, T, MPL, mins, 1, 0))
    for _ in range(T):
        for e, p, r in ((a2, pa, ra2), (b2, pb, rb2)):
            e.rollout_step(policy=p, replay=r, max_path_length=MPL, random_actions=r._size < fill, deterministic=True)
    for (e_l, r_l), (e_s, r_s) in (((a1, ra1), (a2, ra2)), ((b1, rb1), (b2, rb2))):
        assert r_l._size == r_s._size == T * N
        got, want = _rows(r_l, T * N), _rows(r_s, T * N)
        for k in KEYS:
            assert _same(got[k], want[k]), k
        for g, w in zip(e_l.obs_rms._get(), e_s.obs_rms._get()):
            assert _same(np.asarray(g), np.asarray(w))
        assert _same(_policy_input(e_l), _policy_input(e_s))
    assert not _same(_rows(ra1, T * N)["observations"], _rows(rb1, T * N)["observations"])
    for e in (a1, a2, b1, b2):
        e.close()


# ---------------------------------------------------------------------------------------------- 7. allocations
def _ctx_allocs(ctx):
    n = C.c_size_t()
    assert ctx.lib.ilsx_debug_ctx_allocs(ctx.h, C.byref(n)) == 0
    return n.value


def _one_life(ctx, name, pol, rb):
    from ilswiss_amd.envs import HipVectorEnv
    env = HipVectorEnv(name, 8, seed=1, ctx=ctx, norm_obs=True)
    env.rollout_step(policy=pol, replay=rb, max_path_length=4)            # records under normalisation, ring mode
    env.rollout_step(policy=pol, replay=rb, max_path_length=4, label_policy=pol)
    env.set_path_mode(True)
    for _ in range(5):                                                    # ... and path mode: episodes end and reach the ring
        env.rollout_step(policy=pol, replay=rb, max_path_length=4)
    env.set_path_mode(False)
    ctx.sync()
    env.close()


@pytest.mark.parametrize("name", ("hopper", "ant", "swimmer"))   # one task of each engine
def test_a_recording_normalising_env_gives_back_every_allocation(ctx, name):
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


# ---------------------------------------------------------------------------------------------- 8. script plumbing
def test_sac_alpha_script_on_the_pendulum_norm_spec(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "run_scripts"))
    import sac_alpha_exp_script as script
    from _common import flatten_spec
    v = flatten_spec(yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "sac", "sac_pendulum_norm_hip.yaml"))))
    assert v["env_specs"]["vec_env_kwargs"] == {"norm_obs": True}
    v["env_specs"].update(env_num=8, eval_env_num=4)
    v["rl_alg_params"].update(num_epochs=1, num_steps_per_epoch=800, num_steps_between_train_calls=400, num_train_steps_per_train_call=10,
                              num_steps_per_eval=100, max_path_length=100, min_steps_before_training=200, batch_size=64,
                              replay_buffer_size=5000, freq_saving=1)
    alg = script.experiment(v, 0, str(tmp_path))
    rows = list(csv.DictReader(open(tmp_path / "progress.csv")))
    steps = float(rows[-1]["Number of env steps total"])
    assert steps >= 800 and all(np.isfinite(float(r["AverageReturn"])) for r in rows)
    tr, ev = alg.training_env, alg.eval_env
    assert tr.norm_obs and tr.update_obs_rms and ev.norm_obs and not ev.update_obs_rms
    assert tr.obs_rms.count >= steps and ev.obs_rms.count == tr.obs_rms.count
    assert _same(ev.obs_rms.mean, tr.obs_rms.mean) and _same(ev.obs_rms.var, tr.obs_rms.var)
    b = alg.replay_buffer.get_all()
    assert len(b["observations"]) == steps
    for k in ("observations", "next_observations"):
        assert np.isfinite(b[k]).all() and np.abs(b[k]).max() <= 10.0
    print("largest recorded |normalised observation| per column:", np.abs(b["observations"]).max(axis=0))
