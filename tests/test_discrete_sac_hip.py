"""GPU suite for discrete SAC: the device trainer (ilsx_dsac_*, csrc/dsac.h) against the reference's own DiscreteSoftActorCritic
(tests/golden/g28_discrete_sac.npz), the categorical head of ilsx_policy_act, train_from_replay, snapshots, the refusals, and a short
run of run_scripts/discrete_sac_exp_script.py."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from dsac_restatement import golden_cases  # noqa: E402

G28 = os.path.join(HERE, "golden", "g28_discrete_sac.npz")
pytestmark = pytest.mark.gpu


def _build(ctx, c, max_batch=None):
    import ilswiss_amd as ia
    from ilswiss_amd.discrete_sac import DiscreteSoftActorCritic
    hid = [c["H"], c["H"]]
    pol = ia.DiscretePolicy(hidden_sizes=hid, obs_dim=c["o"], action_dim=c["n"], ctx=ctx)
    q1 = ia.FlattenMlp(hidden_sizes=hid, input_size=c["o"], output_size=c["n"], ctx=ctx)
    q2 = ia.FlattenMlp(hidden_sizes=hid, input_size=c["o"], output_size=c["n"], ctx=ctx)
    pol.set_flat_params(c["pi0"]), q1.set_flat_params(c["q10"]), q2.set_flat_params(c["q20"])
    tr = DiscreteSoftActorCritic(pol, q1, q2, max_batch=max_batch or c["B"], **c["kw"])
    return pol, tr


@pytest.mark.parametrize("case", [0, 1])
def test_device_trainer_matches_reference(ctx, case):
    c = golden_cases(G28)[case]
    pol, tr = _build(ctx, c)
    idx = c["idx"]
    for s, b in enumerate(c["batches"]):
        tr.end_epoch()
        tr.train_step(b)
        st = tr.get_eval_statistics()
        assert st["Reward Scale"] == c["kw"]["reward_scale"]
        for k, ref in (("QF1 Loss", "qf1_loss"), ("QF2 Loss", "qf2_loss"), ("Policy Loss", "policy_loss")):
            want = float(c[f"s{s}_{ref}"])
            assert abs(st[k] - want) <= 1e-4 * max(1.0, abs(want)), (s, k, st[k], want)
        for q in ("Q1", "Q2"):
            got = [st[f"{q} Predictions {k}"] for k in ("Mean", "Std", "Max", "Min")]
            assert np.allclose(got, c[f"s{s}_{q.lower()}_pred"], atol=1e-4), (s, q, got)
        if s == 0:   # the first Adam step: exp_avg = (1 - beta_1) * grad
            snap = tr.get_snapshot()
            for k, name in (("q1", "qf1"), ("q2", "qf2"), ("pi", "policy")):
                g = snap[name + "_optimizer"]["exp_avg"][idx] / (1.0 - c["kw"]["beta_1"])
                ref = c["grad_" + k]
                assert np.abs(g - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), (k, np.abs(g - ref).max())
    for k, name in (("pi", "policy"), ("q1", "qf1"), ("q2", "qf2"), ("tq1", "target_qf1"), ("tq2", "target_qf2")):
        err = np.abs(tr.get_flat_params(name)[idx] - c[k]).max()
        assert err < 5e-5, (k, err)


def test_policy_act_deterministic_and_log_prob(ctx):
    import ilswiss_amd as ia
    for c in golden_cases(G28):
        pol = ia.DiscretePolicy(hidden_sizes=[c["H"]] * 2, obs_dim=c["o"], action_dim=c["n"], ctx=ctx)
        pol.set_flat_params(c["pi0"])
        det = ia.MakeDeterministic(pol).get_actions(c["lp_obs"])
        assert det.shape == (64, 1) and np.array_equal(det[:, 0].astype(np.int64), c["log_pis"].argmax(1))
        assert np.allclose(pol.get_log_pis(c["lp_obs"]), c["log_pis"], atol=1e-5)
        idx, lp = pol(c["lp_obs"])
        assert np.allclose(lp[:, 0], c["log_pis"][np.arange(64), idx[:, 0]], atol=1e-5)


def test_stochastic_draws_follow_softmax(ctx):
    import ilswiss_amd as ia
    c = golden_cases(G28)[1]
    pol = ia.DiscretePolicy(hidden_sizes=[c["H"]] * 2, obs_dim=c["o"], action_dim=c["n"], ctx=ctx)
    pol.set_flat_params(c["pi0"])
    obs = np.repeat(c["lp_obs"][:1], 1 << 20, axis=0)
    a = pol.get_actions(obs)[:, 0].astype(np.int64)
    p = np.exp(c["log_pis"][0].astype(np.float64))
    N = a.size
    cnt = np.bincount(a, minlength=c["n"])
    assert cnt.size == c["n"]
    sig = np.sqrt(N * p * (1 - p))
    assert np.all(np.abs(cnt - N * p) <= 5 * sig), (cnt / N, p)


def test_train_from_replay_equals_train_step(ctx):
    c = golden_cases(G28)[0]
    b = c["batches"][0]
    row = {k: v[:1] for k, v in b.items()}
    B = 64
    rep = {k: np.repeat(v, B, axis=0) for k, v in row.items()}
    _, t1 = _build(ctx, c, max_batch=B)
    _, t2 = _build(ctx, c, max_batch=B)
    import ilswiss_amd as ia
    rb = ia.SimpleReplayBuffer(256, c["o"], 1, ctx=ctx)
    rb.add_rows(rep["observations"], rep["actions"], rep["rewards"], rep["terminals"], rep["next_observations"])
    for _ in range(3):   # every row of the ring is the same transition, so every sampled batch is `rep`
        t1.train_step(rep)
    t2.train_from_replay(rb, 3, B)
    for k in ("policy", "qf1", "qf2", "target_qf1", "target_qf2"):
        assert np.array_equal(t1.get_flat_params(k), t2.get_flat_params(k)), k


def test_snapshot_round_trip(ctx):
    c = golden_cases(G28)[0]
    _, tr = _build(ctx, c)
    tr.train_step(c["batches"][0])
    snap = tr.get_snapshot()
    for b in c["batches"][1:]:
        tr.train_step(b)
    after = {k: tr.get_flat_params(k) for k in ("policy", "qf1", "qf2", "target_qf1", "target_qf2")}
    tr.load_snapshot(snap)
    for b in c["batches"][1:]:
        tr.train_step(b)
    for k, v in after.items():
        assert np.array_equal(tr.get_flat_params(k), v), k


def test_refusals(ctx):
    import ilswiss_amd as ia
    from ilswiss_amd.discrete_sac import DiscreteSoftActorCritic
    c = golden_cases(G28)[0]
    pol, tr = _build(ctx, c)
    bad = dict(c["batches"][0], actions=np.full((c["B"], 1), 2.0, np.float32))
    with pytest.raises(RuntimeError, match="not an index"):
        tr.train_step(bad)
    dp = ia.DiscretePolicy(hidden_sizes=[64, 64], obs_dim=4, action_dim=2, ctx=ctx)
    q = [ia.FlattenMlp(hidden_sizes=[64, 64], input_size=6, output_size=1, ctx=ctx) for _ in range(2)]
    with pytest.raises(RuntimeError, match="categorical"):
        _td3_with(ctx, dp, q)
    gp = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[64, 64], obs_dim=4, action_dim=2, ctx=ctx)
    q2 = [ia.FlattenMlp(hidden_sizes=[64, 64], input_size=4, output_size=2, ctx=ctx) for _ in range(2)]
    with pytest.raises(RuntimeError, match="categorical"):
        DiscreteSoftActorCritic(gp, q2[0], q2[1])


def _td3_with(ctx, pol, q):
    import ctypes as C

    from ilswiss_amd import _lib
    cfg = _lib.Td3Cfg(1.0, 0.99, 1e-3, 1e-3, 2, 0.005, 0.1, 0.5, 1.0, 64, 0, 0.0, 0.0)
    h = C.c_void_p()
    _lib.check(ctx.lib.ilsx_td3_create(ctx.h, C.byref(cfg), pol.h, q[0].h, q[1].h, C.byref(h)))


def test_run_script_writes_reference_columns(tmp_path):
    import yaml
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "sac", "sac_cartpole_d_hip.yaml")))
    ra = spec["constants"]["rl_alg_params"]
    ra.update(num_epochs=2, num_steps_per_epoch=400, min_steps_before_training=100, num_steps_per_eval=400, freq_saving=1)
    (tmp_path / "spec.yaml").write_text(yaml.safe_dump(spec))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_scripts", "discrete_sac_exp_script.py"), "-e", str(tmp_path / "spec.yaml")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    found = [os.path.join(d, "progress.csv") for d, _, fs in os.walk(tmp_path / "logs") if "progress.csv" in fs]
    assert len(found) == 1
    rows = list(csv.DictReader(open(found[0])))
    assert len(rows) >= 2
    for col in ("Reward Scale", "QF1 Loss", "QF2 Loss", "Policy Loss", "Q1 Predictions Mean", "Q1 Predictions Std", "Q1 Predictions Max",
                "Q1 Predictions Min", "Q2 Predictions Mean", "AverageReturn", "Epoch", "Number of env steps total"):
        assert col in rows[0], col
    assert all(np.isfinite(float(r_["QF1 Loss"])) and float(r_["AverageReturn"]) >= 1.0 for r_ in rows)
