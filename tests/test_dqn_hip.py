"""GPU suite for DQN / Double DQN: the device trainer (ilsx_dqn_*, csrc/dqn.h) against the reference's own _do_training methods
(tests/golden/g32_dqn.npz), the epsilon-greedy argmax head of ilsx_policy_act, train_from_replay, snapshots across a hard update, the
refusals, a MountainCar rollout and a short run of run_scripts/dqn_exp_script.py."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from dqn_restatement import golden_cases  # noqa: E402

G32 = os.path.join(HERE, "golden", "g32_dqn.npz")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return golden_cases(G32)


def _qf(ctx, c):
    import ilswiss_amd as ia
    qf = ia.FlattenMlp(hidden_sizes=[c["H"]] * 2, input_size=c["o"], output_size=c["n"], ctx=ctx)
    qf.set_flat_params(c["q0"])
    return qf


def _build(ctx, c, max_batch=None):
    import ilswiss_amd as ia
    qf = _qf(ctx, c)
    tr = (ia.DoubleDQN if c["double_q"] else ia.DQN)(qf, max_batch=max_batch or c["B"], **c["kw"])
    tr.set_flat_params("target_qf", c["tq0"])   # the fixture's target net starts from a vector of its own
    return qf, tr


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_device_trainer_matches_reference(ctx, cases, case):
    c = cases[case]
    _, tr = _build(ctx, c)
    idx = c["idx"]
    for s, b in enumerate(c["batches"]):
        tr.end_epoch()
        tr.train_step(b)
        st = tr.get_eval_statistics()
        want = float(c[f"s{s}_qf_loss"])
        print(case, s, "QF Loss", st["QF Loss"], want)
        assert abs(st["QF Loss"] - want) <= 1e-4 * max(1.0, abs(want)), (s, st["QF Loss"], want)
        got = [st[f"Y Predictions {k}"] for k in ("Mean", "Std", "Max", "Min")]
        print(case, s, "Y Predictions", np.abs(np.array(got) - c[f"s{s}_y_pred"]).max())
        assert np.allclose(got, c[f"s{s}_y_pred"], atol=1e-4), (s, got)
        if s == 0:   # the first Adam step: exp_avg = (1 - beta_1) * grad
            g = tr.get_snapshot()["qf_optimizer"]["exp_avg"][idx] / (1.0 - 0.9)
            ref = c["grad_q"]
            print(case, "grad", np.abs(g - ref).max(), np.abs(ref).max())
            assert np.abs(g - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
    for k, name in (("q", "qf"), ("tq", "target_qf")):
        err = np.abs(tr.get_flat_params(name)[idx] - c[k]).max()
        print(case, name, err)
        assert err < 5e-5, (k, err)


def test_deterministic_actions_are_the_golden_argmax(ctx, cases):
    import ilswiss_amd as ia
    for c in cases:
        pol = ia.ArgmaxDiscretePolicy(_qf(ctx, c), epsilon=0.3)
        det = ia.MakeDeterministic(pol).get_actions(c["am_obs"])
        assert det.shape == (64, 1) and np.array_equal(det[:, 0].astype(np.int64), c["argmax"])
        a, info = pol.get_action(c["am_obs"][0], deterministic=True)
        assert a.shape == (1,) and int(a[0]) == c["argmax"][0] and info == {}


def test_epsilon_greedy_frequencies(ctx, cases):
    import ilswiss_amd as ia
    c = cases[1]
    n, N = c["n"], 1 << 20
    assert n == 5
    obs = np.repeat(c["am_obs"][:1], N, axis=0)
    best = int(c["argmax"][0])
    for eps in (0.3, 0.0, 1.0):
        pol = ia.ArgmaxDiscretePolicy(_qf(ctx, c), epsilon=eps)
        a = pol.get_actions(obs)[:, 0]
        assert np.array_equal(a, np.floor(a)) and a.min() >= 0 and a.max() < n
        cnt = np.bincount(a.astype(np.int64), minlength=n)
        p = (1.0 - eps) * (np.arange(n) == best) + eps / n
        sig = np.sqrt(N * p * (1 - p))
        assert np.all(np.abs(cnt - N * p) <= 5 * sig), (eps, cnt / N, p)
        if eps == 0.0:
            assert cnt[best] == N
    a2 = pol.get_actions(obs[:4096])[:, 0]      # the call counter keys the draw: a second call draws anew
    assert not np.array_equal(a2, a[:4096])


def test_train_from_replay_equals_train_step(ctx, cases):
    import ilswiss_amd as ia
    c = cases[3]
    B = 64
    rep = {k: np.repeat(v[:1], B, axis=0) for k, v in c["batches"][0].items()}
    _, t1 = _build(ctx, c, max_batch=B)
    _, t2 = _build(ctx, c, max_batch=B)
    rb = ia.SimpleReplayBuffer(256, c["o"], 1, ctx=ctx)
    rb.add_rows(rep["observations"], rep["actions"], rep["rewards"], rep["terminals"], rep["next_observations"])
    for _ in range(3):   # every row of the ring is the same transition, so every sampled batch is `rep`
        t1.train_step(rep)
    t2.train_from_replay(rb, 3, B)
    for k in ("qf", "target_qf"):
        assert np.array_equal(t1.get_flat_params(k), t2.get_flat_params(k)), k


def test_snapshot_round_trip_lands_the_copy_on_the_same_step(ctx, cases):
    c = cases[2]
    assert c["hard"] and c["kw"]["hard_update_period"] == 2
    _, tr = _build(ctx, c)
    tr.train_step(c["batches"][0])
    snap = tr.get_snapshot()
    assert sorted(snap) == ["qf", "qf_optimizer", "target_qf"] and snap["qf_optimizer"]["n_train_steps"] == 1
    tr.train_step(c["batches"][1])
    assert not np.array_equal(tr.get_flat_params("qf"), tr.get_flat_params("target_qf"))      # counter 1: no copy
    tr.train_step(c["batches"][2])
    after = {k: tr.get_flat_params(k) for k in ("qf", "target_qf")}
    assert np.array_equal(after["qf"], after["target_qf"])                                     # counter 2: copy
    _, fresh = _build(ctx, c)           # a new trainer (counter 0) takes the snapshot
    fresh.load_snapshot(snap)
    for b in c["batches"][1:]:
        fresh.train_step(b)
    for k, v in after.items():
        assert np.array_equal(fresh.get_flat_params(k), v), k


def _td3_with(ctx, pol, q):
    import ctypes as C

    from ilswiss_amd import _lib
    cfg = _lib.Td3Cfg(1.0, 0.99, 1e-3, 1e-3, 2, 0.005, 0.1, 0.5, 1.0, 64, 0, 0.0, 0.0)
    h = C.c_void_p()
    _lib.check(ctx.lib.ilsx_td3_create(ctx.h, C.byref(cfg), pol.h, q[0].h, q[1].h, C.byref(h)))


def test_refusals(ctx, cases):
    import ilswiss_amd as ia
    from ilswiss_amd.discrete_sac import DiscreteSoftActorCritic
    from ilswiss_amd.envs import HipVectorEnv
    c = cases[0]
    _, tr = _build(ctx, c)
    bad = dict(c["batches"][0], actions=np.full((c["B"], 1), float(c["n"]), np.float32))
    with pytest.raises(RuntimeError, match="not an index"):
        tr.train_step(bad)
    with pytest.raises(RuntimeError, match="not an index"):
        tr.train_step(dict(bad, actions=np.full((c["B"], 1), 0.5, np.float32)))
    for eps in (-0.01, 1.01, float("nan")):
        with pytest.raises(RuntimeError, match=r"not in \[0, 1\]"):
            ia.ArgmaxDiscretePolicy(_qf(ctx, c), epsilon=eps)
    marked = ia.ArgmaxDiscretePolicy(ia.FlattenMlp(hidden_sizes=[64, 64], input_size=4, output_size=2, ctx=ctx), 0.1)
    q = [ia.FlattenMlp(hidden_sizes=[64, 64], input_size=6, output_size=1, ctx=ctx) for _ in range(2)]
    with pytest.raises(RuntimeError, match="epsilon-greedy"):
        _td3_with(ctx, marked, q)
    q2 = [ia.FlattenMlp(hidden_sizes=[64, 64], input_size=4, output_size=2, ctx=ctx) for _ in range(2)]
    with pytest.raises(RuntimeError, match="epsilon-greedy"):
        DiscreteSoftActorCritic(marked, q2[0], q2[1])
    cat = ia.DiscretePolicy(hidden_sizes=[64, 64], obs_dim=4, action_dim=2, ctx=ctx)
    with pytest.raises(RuntimeError, match="epsilon-greedy"):
        DiscreteSoftActorCritic(cat, marked.qf, q2[1])
    with pytest.raises(RuntimeError, match="neither categorical nor a noise policy"):
        ia.ArgmaxDiscretePolicy(cat, 0.1)
    with pytest.raises(RuntimeError, match="log-probability"):
        lp = ctx.empty((4,))
        o = ctx.empty((4, 4))
        from ilswiss_amd import _lib
        _lib.check(ctx.lib.ilsx_policy_act(marked.h, o.ptr, 4, 0, None, ctx.empty((4, 1)).ptr, lp.ptr))
    env = HipVectorEnv("mountaincar", 8, seed=2, ctx=ctx)
    gauss = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[64, 64], obs_dim=2, action_dim=1, ctx=ctx)
    with pytest.raises(RuntimeError, match="continuous policy on an env with a Discrete"):     # unchanged
        env.rollout_step(policy=gauss, max_path_length=200)
    env.close()
    box = HipVectorEnv("pendulum", 8, seed=2, ctx=ctx)
    pm = ia.ArgmaxDiscretePolicy(ia.FlattenMlp(hidden_sizes=[64, 64], input_size=3, output_size=3, ctx=ctx), 0.1)
    with pytest.raises(RuntimeError, match="epsilon-greedy policy on an env with a Box"):
        box.rollout_step(policy=pm, max_path_length=200)
    box.close()


def test_mountaincar_rollout_acts_through_the_marked_net(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    n, T = 256, 8
    qf = ia.FlattenMlp(hidden_sizes=[128, 128], input_size=2, output_size=3, ctx=ctx, seed=11)
    p = qf.get_flat_params()
    p[-(128 * 3 + 3):] *= 100.0     # action values well apart
    qf.set_flat_params(p)
    for eps in (0.0, 1.0):
        pol = ia.ArgmaxDiscretePolicy(qf, eps)
        env = HipVectorEnv("mountaincar", n, seed=5, ctx=ctx)
        rb = ia.SimpleReplayBuffer(n * T, 2, 1, ctx=ctx)
        env.reset()
        for _ in range(T):
            env.rollout_step(policy=pol, replay=rb, max_path_length=200)
        size, _ = rb._cursors()
        assert size == n * T
        b = rb._gather(np.arange(size))
        a = b["actions"][:, 0]
        if eps == 0.0:
            assert np.array_equal(a.astype(np.int64), qf(b["observations"]).argmax(1))
        else:
            assert set(a.tolist()) == {0.0, 1.0, 2.0}
        env.close()


def test_run_script_writes_reference_columns(tmp_path):
    import yaml
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "dqn", "dqn_cartpole_hip.yaml")))
    ra = spec["constants"]["rl_alg_params"]
    ra.update(num_epochs=2, num_steps_per_epoch=400, min_steps_before_training=100, num_steps_per_eval=400, freq_saving=1)
    (tmp_path / "spec.yaml").write_text(yaml.safe_dump(spec))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_scripts", "dqn_exp_script.py"), "-e", str(tmp_path / "spec.yaml")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    found = [os.path.join(d, "progress.csv") for d, _, fs in os.walk(tmp_path / "logs") if "progress.csv" in fs]
    assert len(found) == 1
    rows = list(csv.DictReader(open(found[0])))
    assert len(rows) >= 2
    cols = ("QF Loss", "Y Predictions Mean", "Y Predictions Std", "Y Predictions Max", "Y Predictions Min", "AverageReturn", "Epoch",
            "Number of env steps total")
    for col in cols:
        assert col in rows[0], col
    assert all(np.isfinite(float(r_[col])) for r_ in rows for col in cols)
