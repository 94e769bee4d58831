"""GPU suite for GCSL: the device horizon gather, the BatchNorm categorical step (ilsx_bncat) and the MSE step against the reference's own
vectors (tests/golden/g29_gcsl.npz), determinism, eval-mode probabilities, the stochastic draw, snapshots, short runs of
run_scripts/gcsl_exp_script.py and the refusals."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import gcsl_restatement as GR  # noqa: E402
from test_gcsl_cpu import CAP, D, G, GD, LR, O, T, _Env, _case, _check_final, fill  # noqa: E402

pytestmark = pytest.mark.gpu


def _cat(ctx, c, max_batch=None):
    from ilswiss_amd.gcsl import GCSL, CatagorialConditionPolicy
    Hw, B, n, seed, steps = _case(c)
    pol = CatagorialConditionPolicy([Hw, Hw], O, GD + T, n, max_rows=max(B, 64), ctx=ctx)
    pol.set_flat_params(GR.cat_init(seed, D, Hw, 2, n))
    tr = GCSL(pol, mode="CLASS", use_horizons=True, goal_dim=GD, policy_lr=LR, max_batch=max_batch or B)
    return pol, tr


def _run_cat(ctx, c):
    pol, tr = _cat(ctx, c)
    Hw, B, n, seed, steps = _case(c)
    stats = []
    for X, y in GR.cat_batches(seed + 100, B, steps, O, GD, T, n):
        tr.end_epoch()
        tr.train_step(dict(observations=X[:, :O], desired_goals=X[:, O:O + GD], horizons=X[:, O + GD:], actions=y.reshape(B, 1)))
        stats.append((tr.get_eval_statistics()["CE Loss"], tr.get_eval_statistics()["Accuracy"]))
    return pol, tr, stats


def test_device_gather_matches_reference_and_host_buffer(ctx):
    from ilswiss_amd.gcsl import DeviceHindsightHorizonReplayBuffer, HindsightHorizonReplayBuffer
    dev = DeviceHindsightHorizonReplayBuffer(T, CAP, _Env(), random_seed=29, relabel_type="future", ctx=ctx)
    host = HindsightHorizonReplayBuffer(T, CAP, _Env(), random_seed=29, relabel_type="future")
    fill(dev), fill(host)
    np.random.seed(2930)
    b = dev.random_batch(64)
    np.random.seed(2930)
    hb = host.random_batch(64)
    assert np.array_equal(dev.last_indices[0], G["buf_idx"]) and np.array_equal(dev.last_indices[1], G["buf_idx_relabel"])
    X, lab = dev.gather(b, 1)
    X, lab = X.numpy(), lab.numpy()
    want = np.concatenate([G["buf_obs"], G["buf_desired_goals"], G["buf_horizons"]], 1).astype(np.float32)
    assert np.array_equal(X, want)
    assert np.array_equal(lab, G["buf_actions"][:, 0].astype(np.int32))
    assert np.array_equal(X, np.concatenate([hb["observations"], hb["desired_goals"], hb["horizons"]], 1).astype(np.float32))
    Xf, act = dev.gather(b, 0)
    assert np.array_equal(Xf.numpy(), X) and np.array_equal(act.numpy()[:, 0], hb["actions"][:, 0].astype(np.float32))


@pytest.mark.parametrize("c", [0, 1])
def test_device_class_step_matches_reference(ctx, c):
    pol, tr, stats = _run_cat(ctx, c)
    for s, (ce, acc) in enumerate(stats):
        np.testing.assert_allclose(ce, G[f"c{c}_ce"][s], rtol=1e-5)
        assert np.float32(acc) == G[f"c{c}_acc"][s]
    rm, rv = pol.get_running_stats()
    _check_final(c, pol.get_flat_params(), rm, rv, pol.probs)


def test_device_class_step_is_deterministic(ctx):
    p1, _, s1 = _run_cat(ctx, 0)
    p2, _, s2 = _run_cat(ctx, 0)
    assert s1 == s2
    assert p1.get_flat_params().tobytes() == p2.get_flat_params().tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(p1.get_running_stats(), p2.get_running_stats()))


def test_eval_probs_from_reference_state(ctx):
    """Eval-mode softmax from the reference's own final state (the small case stores every parameter and the running statistics)."""
    pol, _ = _cat(ctx, 1)
    Hw, B, n, seed, steps = _case(1)
    pol.set_flat_params(G["c1_final"])
    pol.set_running_stats(G["c1_running_mean"], G["c1_running_var"])
    pr = GR.probe(seed + 200, 64, O, GD, T)
    probs = pol.probs(pr)
    np.testing.assert_allclose(probs, G["c1_probe_probs"], rtol=0, atol=1e-5)
    ref = G["c1_probe_probs"]
    top2 = np.sort(ref, 1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-5
    am = pol.get_actions(pr, deterministic=True)[:, 0]
    assert np.array_equal(am[clear], ref.argmax(1)[clear])


def test_stochastic_draws_follow_the_probabilities(ctx):
    pol, _ = _cat(ctx, 1)
    pol.set_flat_params(G["c1_final"])
    pol.set_running_stats(G["c1_running_mean"], G["c1_running_var"])
    x = np.repeat(GR.probe(7, 1, O, GD, T), 64, 0)
    p = pol.probs(x[:1])[0].astype(np.float64)
    N, counts = 0, np.zeros(p.size)
    while N < 100000:
        a = pol.get_actions(x)[:, 0]
        counts += np.bincount(a, minlength=p.size)
        N += a.size
    sig = np.sqrt(N * p * (1 - p)) + 1e-9
    assert (np.abs(counts - N * p) <= 5 * sig + 1).all(), (counts / N, p)


def test_device_mse_step_matches_reference(ctx):
    from ilswiss_amd.gcsl import GCSL, MlpGaussianAndEpsilonConditionPolicy
    from ilswiss_amd.her import Box
    Hw, B, a, seed, steps = [int(v) for v in G["m0_shape"]]
    pol = MlpGaussianAndEpsilonConditionPolicy([Hw, Hw], O, GD + T, a, action_space=Box(-np.ones(a), np.ones(a)), ctx=ctx)
    pol.set_flat_params(GR.mse_init(seed, D, Hw, 2, a))
    tr = GCSL(pol, mode="MSE", use_horizons=True, goal_dim=GD, policy_lr=LR, max_batch=B)
    for s, (X, act) in enumerate(GR.mse_batches(seed + 100, B, steps, O, GD, T, a)):
        tr.end_epoch()
        tr.train_step(dict(observations=X[:, :O], desired_goals=X[:, O:O + GD], horizons=X[:, O + GD:], actions=act))
        np.testing.assert_allclose(tr.get_eval_statistics()["MSE"], G["m0_mse"][s], rtol=1e-5)
    assert np.abs(pol.get_flat_params()[G["m0_idx"]] - G["m0_final"]).max() < 5e-5
    X = GR.mse_batches(seed + 100, 8, 1, O, GD, T, a)[0][0]
    np.testing.assert_allclose(pol.get_actions(X, deterministic=True), GR.MseRestatement(pol.get_flat_params(), D, Hw, 2, a).net(
        __import__("torch").from_numpy(X)).tanh().detach().numpy(), atol=1e-5)


def test_snapshot_round_trip_restores_training(ctx):
    Hw, B, n, seed, steps = _case(1)
    batches = GR.cat_batches(seed + 100, B, 6, O, GD, T, n)

    def step(tr, X, y):
        tr.train_step(dict(observations=X[:, :O], desired_goals=X[:, O:O + GD], horizons=X[:, O + GD:], actions=y.reshape(B, 1)))
    pol, tr = _cat(ctx, 1)
    for X, y in batches[:3]:
        step(tr, X, y)
    snap = tr.get_snapshot()
    for X, y in batches[3:]:
        step(tr, X, y)
    want = pol.get_flat_params()
    pol2, tr2 = _cat(ctx, 1)
    tr2.load_snapshot(snap)
    for X, y in batches[3:]:
        step(tr2, X, y)
    assert pol2.get_flat_params().tobytes() == want.tobytes()


def test_mse_snapshot_round_trip_restores_training(ctx):
    """MSE mode: the snapshot holds the device trainer's whole 2-head vector and its Adam state; loading it into a fresh trainer and
    training on reproduces the original bit for bit."""
    from ilswiss_amd.gcsl import GCSL, MlpGaussianAndEpsilonConditionPolicy
    from ilswiss_amd.her import Box
    Hw, B, a, seed, steps = [int(v) for v in G["m0_shape"]]
    batches = GR.mse_batches(seed + 100, B, 6, O, GD, T, a)

    def make():
        pol = MlpGaussianAndEpsilonConditionPolicy([Hw, Hw], O, GD + T, a, action_space=Box(-np.ones(a), np.ones(a)), ctx=ctx)
        pol.set_flat_params(GR.mse_init(seed, D, Hw, 2, a))
        return pol, GCSL(pol, mode="MSE", use_horizons=True, goal_dim=GD, policy_lr=LR, max_batch=B)

    def step(tr, X, act):
        tr.train_step(dict(observations=X[:, :O], desired_goals=X[:, O:O + GD], horizons=X[:, O + GD:], actions=act))
    pol, tr = make()
    for X, act in batches[:3]:
        step(tr, X, act)
    snap = tr.get_snapshot()
    assert snap["policy"]["params"].size == pol.get_device_flat_params().size
    for X, act in batches[3:]:
        step(tr, X, act)
    want = pol.get_device_flat_params()
    pol2, tr2 = make()
    tr2.load_snapshot(snap)
    for X, act in batches[3:]:
        step(tr2, X, act)
    assert pol2.get_device_flat_params().tobytes() == want.tobytes()


@pytest.mark.parametrize("c", [0, 1])
def test_device_running_statistics_at_zero_lr(ctx, c):
    """The running-statistics update at rtol 1e-4 / atol 1e-5: with lr = 0 no parameter moves (so no BN-dead bias drifts into the batch
    means), and the device's running statistics must equal the restatement's (pinned to the reference by the CPU suite)."""
    from ilswiss_amd.gcsl import GCSL, CatagorialConditionPolicy
    Hw, B, n, seed, steps = _case(c)
    p0 = GR.cat_init(seed, D, Hw, 2, n)
    pol = CatagorialConditionPolicy([Hw, Hw], O, GD + T, n, max_rows=max(B, 64), ctx=ctx)
    pol.set_flat_params(p0)
    rm0, rv0 = pol.get_running_stats()
    assert (rm0 == 0).all() and (rv0 == 1).all()          # BatchNorm1d's initial running statistics
    tr = GCSL(pol, mode="CLASS", use_horizons=True, goal_dim=GD, policy_lr=0.0, max_batch=B)
    rst = GR.CatRestatement(p0, D, Hw, 2, n, lr=0.0)
    for X, y in GR.cat_batches(seed + 100, B, steps, O, GD, T, n):
        tr.train_step(dict(observations=X[:, :O], desired_goals=X[:, O:O + GD], horizons=X[:, O + GD:], actions=y.reshape(B, 1)))
        rst.train_step(X, y)
    assert np.array_equal(pol.get_flat_params(), p0)
    rm, rv = pol.get_running_stats()
    want_m, want_v = rst.running()
    np.testing.assert_allclose(rm, want_m, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rv, want_v, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("spec", ["gcsl_reach_hip.yaml", "gcsl_reach_dis_hip.yaml"])
def test_run_script_writes_progress(tmp_path, spec):
    import yaml
    s = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "gcsl", spec)))
    s["constants"]["rl_alg_params"].update(num_epochs=2, num_steps_per_epoch=300, min_steps_before_training=150, num_steps_per_eval=100)
    (tmp_path / "spec.yaml").write_text(yaml.safe_dump(s))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_scripts", "gcsl_exp_script.py"), "-e", str(tmp_path / "spec.yaml")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    found = [os.path.join(d, "progress.csv") for d, _, fs in os.walk(tmp_path / "logs") if "progress.csv" in fs]
    assert len(found) == 1
    rows = list(csv.DictReader(open(found[0])))
    assert len(rows) == 2
    cols = ("CE Loss", "Accuracy") if "dis" in spec else ("MSE",)
    for col in ("Epoch", "Success Rate", "AverageReturn", "Number of env steps total") + cols:
        assert col in rows[0], col
    assert all(np.isfinite(float(r_[cols[0]])) for r_ in rows)


def test_refusals(ctx, tmp_path):
    import yaml
    for spec, patch in (("gcsl_reach_hip.yaml", dict(env_name="fetch-reach")), ("gcsl_reach_dis_hip.yaml", dict(discretize=False))):
        s = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "gcsl", spec)))
        s["constants"]["env_specs"].update(patch)
        (tmp_path / "spec.yaml").write_text(yaml.safe_dump(s))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "run_scripts", "gcsl_exp_script.py"), "-e", str(tmp_path / "spec.yaml")],
                           cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and ("NotImplementedError" in r.stderr or "ValueError" in r.stderr), r.stderr[-2000:]
    from ilswiss_amd.gcsl import GCSL, CatagorialConditionPolicy
    pol = CatagorialConditionPolicy([64, 64], O, GD + T, 25, max_rows=64, ctx=ctx)
    with pytest.raises(NotImplementedError):
        GCSL(pol, mode="MLE", use_horizons=True, goal_dim=GD)
    with pytest.raises(ValueError):
        GCSL(pol, mode="CLASS", use_horizons=True)             # goal | horizon cannot be split without goal_dim
    with pytest.raises(RuntimeError, match="n_classes=65"):
        CatagorialConditionPolicy([64, 64], O, GD + T, 65, ctx=ctx)   # more classes than lanes
