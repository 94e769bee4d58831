"""GPU suite for DDPG: the device trainer (ilsx_ddpg_*, csrc/ilsx_ac.hip) against the reference's own DDPG (tests/golden/g31_ddpg.npz),
train_from_replay, snapshots, the device-side exploration strategies (ilsx_vecenv_explore, k_explore in csrc/ilsx_env.hip) against the
reference's OUStrategy / GaussianStrategy traces, the fused rollout with a strategy set, and a short run of run_scripts/ddpg_exp_script.py.

Tolerances as in tests/test_ddpg_cpu.py (those of tests/test_hip_parity.py): losses and statistics rtol 2e-4 / atol 2e-6, parameters 5e-5
absolute, every gradient vector within 1e-4 of ITS largest entry (no absolute floor); strategy traces exact after the float32 cast of the action."""
import csv
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from ddpg_restatement import CASES, GOLDEN, STAT_KEYS, golden_cases  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL, PTOL = 2e-4, 2e-6, 5e-5
NAMES = (("pi", "policy"), ("q", "qf"), ("tpi", "target_policy"), ("tq", "target_qf"))
STAT_NAMES = dict(q_predictions="Q Predictions", q_targets="Q Targets", bellman_errors="Bellman Errors", policy_action="Policy Action")


@pytest.fixture(scope="module")
def cases():
    return golden_cases()


def _build(ctx, c, max_batch=None, **over):
    import ilswiss_amd as ia
    from ilswiss_amd.ddpg import DDPG, MlpPolicy
    pol = MlpPolicy(hidden_sizes=c["hidden"], obs_dim=c["o"], action_dim=c["a"], output_activation="tanh" if c["tanh_out"] else "identity", ctx=ctx)
    qf = ia.FlattenMlp(hidden_sizes=c["hidden"], input_size=c["o"] + c["a"], output_size=1, ctx=ctx)
    pol.set_flat_params(c["pi0"]), qf.set_flat_params(c["q0"])
    return DDPG(pol, qf, max_batch=max_batch or c["B"], **dict(c["kw"], **over))


def _all_params(tr):
    return {name: tr.get_flat_params(name) for _, name in NAMES}


@pytest.mark.parametrize("case", range(len(CASES)))
def test_device_trainer_matches_reference(ctx, cases, case):
    c = cases[case]
    tr = _build(ctx, c)
    idx = dict(pi=c["idx_pi"], q=c["idx_q"], tpi=c["idx_pi"], tq=c["idx_q"])
    for s, b in enumerate(c["batches"]):
        tr.end_epoch()
        tr.train_step(b)
        st = tr.get_eval_statistics()
        got = [st[k] for k in ("QF Loss", "Policy Loss", "Raw Policy Loss", "Preactivation Policy Loss")]
        print(case, s, "losses", got, c[f"s{s}_losses"])
        assert np.allclose(got, c[f"s{s}_losses"], rtol=RTOL, atol=ATOL), (s, got, c[f"s{s}_losses"])
        for k in STAT_KEYS:
            got = [st[f"{STAT_NAMES[k]} {m}"] for m in ("Mean", "Std", "Max", "Min")]
            assert np.allclose(got, c[f"s{s}_{k}"], rtol=RTOL, atol=ATOL), (s, k, got, c[f"s{s}_{k}"])
        if s == 0:   # the first Adam step: exp_avg = (1 - beta_1) * grad
            snap = tr.get_snapshot()
            for k, name in (("q", "qf"), ("pi", "policy")):
                g = snap[name + "_optimizer"]["exp_avg"][idx[k]] / (1.0 - 0.9)
                ref = c["grad_" + k]
                err = np.abs(g - ref).max()
                print(case, "grad", k, err, np.abs(ref).max())
                assert err <= 1e-4 * np.abs(ref).max(), (k, err, np.abs(ref).max())
        if case == 0:   # the hard-update schedule: copies on steps 0 and 2, none on step 1
            p = _all_params(tr)
            for k, name in NAMES:
                assert np.abs(p[name] - c[f"s{s}_{k}"]).max() < PTOL, (s, k)
            if s == 1:
                assert np.array_equal(p["target_qf"], q_after_0) and np.array_equal(p["target_policy"], pi_after_0)
                assert not np.array_equal(p["target_qf"], p["qf"])
            else:
                assert np.array_equal(p["target_qf"], p["qf"]) and np.array_equal(p["target_policy"], p["policy"])
            if s == 0:
                q_after_0, pi_after_0 = p["qf"], p["policy"]
    for k, name in NAMES:
        err = np.abs(tr.get_flat_params(name)[idx[k]] - c[k]).max()
        print(case, "params", k, err)
        assert err < PTOL, (k, err)


def _replay_run(c, n_steps, seed=5):
    import ilswiss_amd as ia
    cx = ia.Context(0, seed=seed)
    try:
        tr = _build(cx, c)
        rb = ia.SimpleReplayBuffer(512, c["o"], c["a"], random_seed=9, ctx=cx)
        rows = {k: np.concatenate([b[k] for b in c["batches"]])[:512] for k in c["batches"][0]}
        rb.add_rows(rows["observations"], rows["actions"], rows["rewards"], rows["terminals"], rows["next_observations"])
        tr.train_from_replay(rb, n_steps, c["B"])
        st = dict(tr.get_eval_statistics())
        return st, _all_params(tr), tr.get_snapshot()["qf_optimizer"]["n_train_steps"]
    finally:
        cx.close()


def test_train_from_replay(cases):
    c = cases[1]
    st3, p3, n3 = _replay_run(c, 3)
    st3b, p3b, _ = _replay_run(c, 3)
    st1, p1, n1 = _replay_run(c, 1)
    assert (n1, n3) == (1, 3)
    assert st3 == st1 and np.isfinite(list(st3.values())).all()       # the statistics are the first batch's
    assert st3 == st3b and all(np.array_equal(p3[k], p3b[k]) for k in p3)   # same seed: bitwise
    assert not np.array_equal(p3["qf"], p1["qf"])


def test_snapshot_round_trip(ctx, cases):
    """At case 0, where the hard-update counter decides whether the step after the restore copies."""
    c = cases[0]
    tr = _build(ctx, c)
    tr.train_step(c["batches"][0])
    tr.train_step(c["batches"][1])
    snap = tr.get_snapshot()
    assert snap["qf_optimizer"]["n_train_steps"] == 2
    tr.train_step(c["batches"][2])   # counter 2: copies
    tr.train_step(c["batches"][0])   # counter 3: does not
    after = _all_params(tr)
    tr2 = _build(ctx, c)
    tr2.load_snapshot(snap)
    tr2.train_step(c["batches"][2])
    assert np.array_equal(tr2.get_flat_params("target_qf"), tr2.get_flat_params("qf"))
    tr2.train_step(c["batches"][0])
    for k, v in after.items():
        assert np.array_equal(tr2.get_flat_params(k), v), k
    assert not np.array_equal(after["target_qf"], after["qf"])


def test_create_refusals(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.ddpg import DDPG, MlpPolicy
    pol = MlpPolicy(hidden_sizes=[64, 64], obs_dim=4, action_dim=2, ctx=ctx)
    with pytest.raises(RuntimeError, match="qf input"):
        DDPG(pol, ia.FlattenMlp(hidden_sizes=[64, 64], input_size=5, output_size=1, ctx=ctx))
    with pytest.raises(RuntimeError, match="min_q_value"):
        DDPG(pol, ia.FlattenMlp(hidden_sizes=[64, 64], input_size=6, output_size=1, ctx=ctx), min_q_value=1.0, max_q_value=0.0)


# ---------------------------------------------------------------------------------------------- exploration strategies
def _explore(env, act, eps, t):
    from ilswiss_amd import _lib
    a = env.ctx.from_numpy(act, np.float32)
    e = env.ctx.from_numpy(eps, np.float64)
    _lib.check(env.ctx.lib.ilsx_vecenv_explore(env.h, a.ptr, e.ptr, int(t)))
    return a.numpy()


def _hopper4(ctx):
    from ilswiss_amd.envs import HipVectorEnv
    env = HipVectorEnv("hopper", 4, seed=3, ctx=ctx)   # 3-wide actions, the width of the golden traces
    env.reset()
    return env


def _age(env):
    """One env step of every env that ends no episode: afterwards no env is at the start of an episode."""
    env.rollout_step(max_path_length=10 ** 6, random_actions=True, no_terminal=True)


def test_explore_ou_matches_reference_trace(ctx):
    from ilswiss_amd.ddpg import OUStrategy, PolicyWrappedWithExplorationStrategy
    g = np.load(GOLDEN)
    mu, theta, mx, mn, dp = g["ou_kw"]
    env = _hopper4(ctx)
    es = OUStrategy(env.single_action_space, mu=mu, theta=theta, max_sigma=mx, min_sigma=mn, decay_period=dp)
    PolicyWrappedWithExplorationStrategy(es, None).install(env)
    want = g["ou_out"].astype(np.float32)
    differs = False
    for k in range(40):
        if k in (13, 29):
            env.reset([0, 1, 2])    # envs 0..2 start an episode: their processes go back to mu, as reset() does in the reference's trace
        got = _explore(env, np.tile(g["ou_raw"][k], (4, 1)), np.tile(g["ou_eps"][k], (4, 1)), 7 * k)
        for e in range(3):
            assert np.array_equal(got[e], want[k]), (k, e, got[e], want[k])
        if k < 13:
            assert np.array_equal(got[3], want[k]), k
        differs = differs or not np.array_equal(got[3], want[k])
        if k == 13:
            assert not np.array_equal(got[3], want[k])   # the env that was not reset carries its state on
        _age(env)
    assert differs
    env.close()


def test_explore_gaussian_matches_reference_trace(ctx):
    from ilswiss_amd.ddpg import GaussianStrategy, PolicyWrappedWithExplorationStrategy
    g = np.load(GOLDEN)
    mx, mn, dp = g["ga_kw"]
    env = _hopper4(ctx)
    PolicyWrappedWithExplorationStrategy(GaussianStrategy(env.single_action_space, max_sigma=mx, min_sigma=mn, decay_period=dp), None).install(env)
    want = g["ga_out"].astype(np.float32)
    for k in range(40):
        got = _explore(env, np.tile(g["ga_raw"][k], (4, 1)), np.tile(g["ga_eps"][k], (4, 1)), 7 * k)
        assert np.array_equal(got, np.tile(want[k], (4, 1))), k
    env.close()


def test_explore_needs_a_strategy(ctx):
    env = _hopper4(ctx)
    with pytest.raises(RuntimeError, match="no exploration strategy"):
        _explore(env, np.zeros((4, 3)), np.zeros((4, 3)), 0)
    env.close()


def _rollout(kind, T=20, deterministic=False, random_actions=False, seed=21, zero_policy=False, t_step=64):
    """A fresh context, a 64-env Pendulum, a tanh MlpPolicy with fixed parameters; T fused rollout steps; the actions of every step."""
    import ctypes as C

    import ilswiss_amd as ia
    from ilswiss_amd import _lib
    from ilswiss_amd.ddpg import MlpPolicy
    from ilswiss_amd.envs import HipVectorEnv
    cx = ia.Context(0, seed=seed)
    try:
        env = HipVectorEnv("pendulum", 64, seed=seed, ctx=cx)
        env.reset()
        pol = MlpPolicy(hidden_sizes=[64, 64], obs_dim=3, action_dim=1, output_activation="tanh", ctx=cx)
        flat = np.random.default_rng(8).normal(0, 0.3, pol.num_params).astype(np.float32)
        pol.set_flat_params(np.zeros_like(flat) if zero_policy else flat)
        if kind is not None:
            cfg = _lib.ExploreCfg(kind, 0, 0.0, 0.15, 0.5, 0.1, 640.0, -1.0, 1.0)
            _lib.check(cx.lib.ilsx_vecenv_set_exploration(env.h, C.byref(cfg)))
        rb = ia.SimpleReplayBuffer(64, 3, 1, ctx=cx)   # capacity n: step t's record of env i sits at slot i
        acts = []
        for t in range(T):
            _lib.check(cx.lib.ilsx_vecenv_set_exploration_t(env.h, t * t_step))
            env.rollout_step(pol, rb, max_path_length=7, random_actions=random_actions, deterministic=deterministic)
            acts.append(rb._gather(np.arange(64))["actions"][:, 0].copy())
        q, v = env.get_state()
        env.close()
        return np.stack(acts), q, v
    finally:
        cx.close()


def test_rollout_with_ou_exploration():
    base, _, _ = _rollout(None, zero_policy=True)
    assert np.all(base == 0.0)                              # tanh(0): what is stored below is the clipped OU state alone
    a, q, v = _rollout(2, zero_policy=True)
    assert np.all(np.abs(a) <= 1.0) and np.abs(a).max() > 0.3
    assert not np.array_equal(a[:, 0], a[:, 1])             # one process per env
    inner = a[0][np.abs(a[0]) < 1.0]                        # (entries on the clip bounds coincide; sigma 0.5 puts ~5 % of the draws there)
    assert len(inner) > 48 and len(np.unique(inner)) == len(inner)
    b, q2, v2 = _rollout(2, zero_policy=True)
    assert np.array_equal(a, b) and np.array_equal(q, q2) and np.array_equal(v, v2)   # same seed: bitwise
    # max_path_length 7: step 7 starts a new episode from mu = 0, so its noise is ONE draw times the annealed sigma (< 0.5), while steps 5
    # and 6 are late in a process with theta 0.15: correlated with each other across the 64 envs (~0.8 by the AR(1) recursion), and not
    # with step 7 (independent draws; the standard error of a correlation of 64 pairs is 0.125)
    corr = lambda x, y: float(np.corrcoef(x, y)[0, 1])  # noqa: E731
    assert corr(a[5], a[6]) > 0.5 and abs(corr(a[6], a[7])) < 0.4
    assert np.abs(a[7]).mean() < np.abs(a[6]).mean()


def test_rollout_ignores_the_strategy_when_deterministic_or_random():
    for kw in (dict(deterministic=True), dict(random_actions=True)):
        plain = _rollout(None, **kw)
        with_ou = _rollout(2, **kw)
        for x, y in zip(plain, with_ou):
            assert np.array_equal(x, y), kw
    plain, with_ou = _rollout(None)[0], _rollout(2)[0]
    assert not np.array_equal(plain, with_ou) and np.all(np.abs(with_ou) <= 1.0)
    gauss = _rollout(1)[0]
    assert not np.array_equal(plain, gauss) and not np.array_equal(gauss, with_ou) and np.all(np.abs(gauss) <= 1.0)


def test_rollout_without_a_strategy_is_unchanged():
    untouched = _rollout(None)
    kind0 = _rollout(0)
    for x, y in zip(untouched, kind0):
        assert np.array_equal(x, y)


def test_wrapper_get_actions(ctx):
    from ilswiss_amd.ddpg import GaussianStrategy, MlpPolicy, PolicyWrappedWithExplorationStrategy
    from ilswiss_amd.envs import HipVectorEnv
    env = HipVectorEnv("pendulum", 64, seed=2, ctx=ctx)
    obs = env.reset()
    pol = MlpPolicy(hidden_sizes=[64, 64], obs_dim=3, action_dim=1, output_activation="tanh", ctx=ctx)
    wp = PolicyWrappedWithExplorationStrategy(GaussianStrategy(env.single_action_space, max_sigma=0.5), pol)
    with pytest.raises(RuntimeError, match="installed"):
        wp.get_actions(obs)
    wp.install(env)
    det = wp.get_actions(obs, deterministic=True)
    assert np.array_equal(det, pol.get_actions(obs, deterministic=True))
    a = wp.get_actions(obs)
    assert a.shape == det.shape and np.all(np.abs(a) <= 1.0) and 0.2 < np.std(a - det) < 0.8   # sigma 0.5, clipped
    assert wp.h is pol.h
    other = HipVectorEnv("pendulum", 64, seed=4, ctx=ctx)
    with pytest.raises(RuntimeError, match="another vec env"):   # a second env would restart the first one's processes on every switch
        other.rollout_step(wp, max_path_length=50)
    wp.install(env)   # the same env again is allowed (restarts its processes, asked for)
    other.close()
    env.close()


def test_run_script_logs_ddpg_statistics(tmp_path):
    import yaml
    sys.path.insert(0, os.path.join(ROOT, "run_scripts"))
    import ddpg_exp_script as script
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "ddpg", "ddpg_pendulum_hip.yaml")))
    from _common import flatten_spec
    v = flatten_spec(spec)
    v["rl_alg_params"].update(num_epochs=1, num_steps_per_epoch=200, num_steps_between_train_calls=100, num_train_steps_per_train_call=20,
                              num_steps_per_eval=200, min_steps_before_training=100, freq_saving=1)
    alg = script.experiment(v, 0, str(tmp_path))
    rows = list(csv.DictReader(open(tmp_path / "progress.csv")))
    assert len(rows) == 2 and rows[-1]["Epoch"] == "1"      # epochs 0 and 1 of 200 steps each
    for k in ("QF Loss", "Policy Loss", "Raw Policy Loss", "Preactivation Policy Loss", "Q Predictions Mean", "Q Targets Std",
              "Bellman Errors Max", "Policy Action Min", "AverageReturn", "Number of env steps total"):
        assert k in rows[-1] and np.isfinite(float(rows[-1][k])), k
    assert float(rows[-1]["Number of env steps total"]) == 400
    assert alg.exploration_policy.env is alg.training_env and alg.exploration_policy.t == 399   # t forwarded before every step
