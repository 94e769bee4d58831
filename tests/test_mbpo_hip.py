"""GPU suite of the MBPO ensemble (ilsx_bnn_* / ilsx_mbpo_model_step, ilswiss_amd/mbpo.py) against the torch-CPU restatement in
tests/mbpo_restatement.py."""
import csv
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mbpo_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bnn(ctx, E=3, o=11, a=3, H=200, nh=4, lr=1e-3, B=64, seed=0):
    from ilswiss_amd.mbpo import BNN, BNNTrainer
    bnn = BNN(hidden_sizes=nh * [H], output_size=o + 1, input_size=o + a, num_nets=E, ctx=ctx, seed=seed)
    tr = BNNTrainer(bnn, lr=lr, batch_size=B, num_elites=min(2, E), holdout_ratio=0.2)
    return bnn, tr


def _data(rng, n, o=11, a=3):
    obs = rng.normal(0, 1, (n, o)).astype(np.float32)
    act = rng.uniform(-1, 1, (n, a)).astype(np.float32)
    rew = rng.normal(0, 1, n).astype(np.float32)
    nobs = (obs + 0.1 * rng.normal(0, 1, (n, o))).astype(np.float32)
    return obs, act, rew, nobs


def _ring(ctx, obs, act, rew, nobs):
    from ilswiss_amd.replay import SimpleReplayBuffer
    n = len(rew)
    rb = SimpleReplayBuffer(n, obs.shape[1], act.shape[1], ctx=ctx)
    rb.add_rows(obs, act, rew, np.zeros(n, np.uint8), nobs)
    return rb


def _padding(bnn):
    import ctypes as C
    from ilswiss_amd import _lib
    mx = C.c_double()
    _lib.check(bnn.ctx.lib.ilsx_bnn_debug_padding(bnn.h, C.byref(mx)))
    return mx.value


def _rel(a, b):
    """largest error relative to the array's scale"""
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-12))


def test_forward_and_predict_match_the_restatement(ctx):
    rng = np.random.default_rng(1)
    bnn, _ = _bnn(ctx, E=3)
    params = R.init_params(rng, 3, 14, [200] * 4, 12, init_w=0.3)
    bnn.set_params(params)
    got = bnn.get_params()
    assert all(np.array_equal(g, p) for g, p in zip(got, params))   # named_parameters() layout, padding invisible
    mean, std = rng.normal(0, 1, 14).astype(np.float32), rng.uniform(0.5, 2, 14).astype(np.float32)
    bnn.normalizer._set(mean, std)
    x = rng.normal(0, 1, (37, 14)).astype(np.float32)
    mu, lv = bnn.forward(x, ret_log_var=True)
    rmu, rlv = R.forward(params, mean, std, x)
    assert _rel(mu, rmu.detach().numpy()) < 1e-5 and _rel(lv, rlv.detach().numpy()) < 1e-5
    m2, v2 = bnn.predict(x)                     # factored=False: the ensemble mean / total variance
    rv = np.exp(rlv.detach().numpy())
    assert _rel(m2, rmu.detach().numpy().mean(0)) < 1e-5
    assert _rel(v2, rv.mean(0) + ((rmu.detach().numpy() - rmu.detach().numpy().mean(0)) ** 2).mean(0)) < 1e-5
    bnn.close()


def test_init_rule_bounds(ctx):
    bnn, _ = _bnn(ctx, E=7)
    ps = bnn.get_params()
    for li in range(len(ps) // 2):
        W, b = ps[2 * li], ps[2 * li + 1]
        if li < len(ps) // 2 - 1:
            bound = 1.0 / np.sqrt(W.shape[1] * W.shape[2])      # fanin_init on [E, in, out]: fan-in = in * out
            assert np.abs(W).max() <= bound and np.abs(W).max() > 0.9 * bound and np.all(b == np.float32(0.1))
        else:
            assert np.abs(W).max() <= 3e-3 and np.abs(b).max() <= 3e-3
    bnn.close()


def _train_vs_torch(ctx, E, H, B, steps, n_rows, last_short, tol):
    rng = np.random.default_rng(7)
    o, a = 11, 3
    obs, act, rew, nobs = _data(rng, n_rows, o, a)
    rb = _ring(ctx, obs, act, rew, nobs)
    bnn, tr = _bnn(ctx, E=E, H=H, B=B)
    params = R.init_params(rng, E, o + a, [H] * 4, o + 1, init_w=0.1)
    bnn.set_params(params)
    x, t = R.data_from_rows(obs, act, rew, nobs)
    mean, std = R.normalizer_stats(x)
    bnn.normalizer._set(mean, std)
    ref = R.AdamTrainer(params, 1e-3, tr.fc_weight_decays)
    table_h = rng.integers(0, n_rows, (E, B * steps)).astype(np.int32)
    table = ctx.from_numpy(table_h, np.int32)
    for s in range(steps):
        Bs = B - 17 if (last_short and s == steps - 1) else B
        loss = tr._train_batch(rb, table, s * B, B * steps, Bs, want_loss=True)
        idx = table_h[:, s * B:s * B + Bs]
        rl = ref.step(mean, std, x[idx], t[idx])
        assert abs(float(np.mean(loss)) + 0.105 - rl) < 1e-4 * max(1.0, abs(rl)), (s, loss, rl)
    err = max(float(np.max(np.abs(g - r))) for g, r in zip(bnn.get_params(), ref.params()))
    assert err < tol, err
    bnn.close()


def test_three_adam_steps_with_short_last_batch(ctx):
    _train_vs_torch(ctx, E=3, H=200, B=64, steps=3, n_rows=300, last_short=True, tol=5e-5)


def test_train_batch_e7_h200_b256_fifty_steps(ctx):
    _train_vs_torch(ctx, E=7, H=200, B=256, steps=50, n_rows=4000, last_short=False, tol=5e-4)


def test_padded_units_stay_zero_and_same_seed_is_bit_identical(ctx):
    """H = 200 is padded to 208 inside the library: 100 steps later the visible parameters of two identically seeded ensembles are
    bit-identical, every padded entry of the internal blocks (W, Wt, b, Adam's m and v) is exactly zero, and a width-208 ensemble given the
    same parameters padded with zeros computes the same forward."""
    rng = np.random.default_rng(3)
    obs, act, rew, nobs = _data(rng, 500)
    rb = _ring(ctx, obs, act, rew, nobs)
    runs = []
    for _ in range(2):
        bnn, tr = _bnn(ctx, E=2, B=64, seed=11)
        table = ctx.from_numpy(np.random.default_rng(5).integers(0, 500, (2, 6400)).astype(np.int32), np.int32)
        for s in range(100):
            tr._train_batch(rb, table, s * 64, 6400, 64)
        runs.append((bnn, bnn.get_flat_params()))
    assert np.array_equal(runs[0][1], runs[1][1])
    assert _padding(runs[0][0]) == 0.0 and _padding(runs[1][0]) == 0.0   # W, Wt, b, m and v of every padded unit: exactly zero
    bnn = runs[0][0]
    p200 = bnn.get_params()
    wide, _ = _bnn(ctx, E=2, H=208, B=64)
    p208 = []
    for li in range(len(p200) // 2):
        W, b = p200[2 * li], p200[2 * li + 1]
        Wp = np.zeros((2, 14 if li == 0 else 208, 24 if li == 4 else 208), np.float32)
        Wp[:, :W.shape[1], :W.shape[2]] = W
        bp = np.zeros((2, 1, Wp.shape[2]), np.float32)
        bp[:, :, :b.shape[2]] = b
        p208 += [Wp, bp]
    wide.set_params(p208)
    x = np.concatenate([obs, act], -1)[:50]
    a1, b1 = bnn.forward(x, ret_log_var=True)
    a2, b2 = wide.forward(x, ret_log_var=True)
    assert np.allclose(a1, a2, rtol=1e-5, atol=1e-6) and np.allclose(b1, b2, rtol=1e-5, atol=1e-6)
    for b_, _ in runs:
        b_.close()
    wide.close()


def test_normalizer_stats_and_holdout_mse(ctx):
    rng = np.random.default_rng(4)
    obs, act, rew, nobs = _data(rng, 700)
    obs[:, 3] = 2.5   # a constant column: std < 1e-12 -> 1
    rb = _ring(ctx, obs, act, rew, nobs)
    bnn, tr = _bnn(ctx, E=3)
    rows = rng.permutation(700).astype(np.int32)
    d = ctx.from_numpy(rows[:500], np.int32)
    from ilswiss_amd import _lib
    _lib.check(ctx.lib.ilsx_bnn_fit_stats(bnn.h, rb.h, d.ptr, 500))
    x, t = R.data_from_rows(obs, act, rew, nobs)
    m, s = R.normalizer_stats(x[rows[:500]])
    gm, gs = bnn.normalizer._get()
    assert np.allclose(gm, m, rtol=1e-5, atol=1e-6) and np.allclose(gs, s, rtol=1e-5) and gs[3] == np.float32(1.0 + 1e-8)
    ho = ctx.from_numpy(rows[500:], np.int32)
    mse = tr._mse(rb, ho, 0, 200)
    loss = tr._mse(rb, ho, 0, 200, add_var=True)
    params = bnn.get_params()
    with torch.no_grad():
        rm = R.compute_loss(params, gm, gs, x[rows[500:]], t[rows[500:]], add_var_loss=False).numpy()
        rv = R.compute_loss(params, gm, gs, x[rows[500:]], t[rows[500:]], add_var_loss=True).numpy()
    assert _rel(mse, rm) < 1e-5 and _rel(loss, rv) < 1e-5
    assert np.array_equal(mse, tr._mse(rb, ho, 0, 200))   # fixed reduction order
    bnn.close()


def test_model_step_with_explicit_eps(ctx):
    """FakeEnv.step + one rollout step on Hopper shapes: explicit members and noise, rows into the model ring, survivors compacted"""
    from ilswiss_amd import _lib
    from ilswiss_amd.envs.terminals import get_terminal_func
    from ilswiss_amd.mbpo import terminal_kind
    from ilswiss_amd.replay import SimpleReplayBuffer
    import ctypes as C
    rng = np.random.default_rng(9)
    E, o, a, n = 4, 11, 3, 300
    bnn, _ = _bnn(ctx, E=E)
    params = R.init_params(rng, E, o + a, [200] * 4, o + 1, init_w=0.05)
    bnn.set_params(params)
    mean, std = np.zeros(o + a, np.float32), np.ones(o + a, np.float32)
    obs = np.zeros((n, o), np.float32)
    obs[:, 0] = rng.uniform(0.6, 1.6, n)       # heights around Hopper's 0.7 bound: some rows end
    obs[:, 1:] = rng.normal(0, 0.05, (n, o - 1))
    act = rng.uniform(-1, 1, (n, a)).astype(np.float32)
    midx = rng.integers(0, E, n).astype(np.int32)
    eps = rng.normal(0, 1, (n, o + 1)).astype(np.float32)
    ring = SimpleReplayBuffer(1000, o, a, ctx=ctx)
    kind = terminal_kind(get_terminal_func("hopper"))
    d_obs, d_act, d_mid, d_eps = ctx.from_numpy(obs), ctx.from_numpy(act), ctx.from_numpy(midx, np.int32), ctx.from_numpy(eps)
    nxt, ns, mo = ctx.empty((n, o)), C.c_int(), ctx.empty((n,), np.int32)
    _lib.check(ctx.lib.ilsx_mbpo_model_step(bnn.h, None, ring.h, kind, d_obs.ptr, d_act.ptr, n, None, 0, 0, d_eps.ptr, d_mid.ptr, None,
                                            mo.ptr, nxt.ptr, C.byref(ns)))
    ref_next, ref_rew = R.fake_env_step(params, mean, std, obs, act, midx, eps)
    rows = ring.get_all()
    assert rows["observations"].shape == (n, o) and np.array_equal(rows["observations"], obs) and np.array_equal(rows["actions"], act)
    assert np.allclose(rows["next_observations"], ref_next, rtol=1e-5, atol=1e-5)
    assert np.allclose(rows["rewards"], ref_rew, rtol=1e-5, atol=1e-5)
    term = get_terminal_func("hopper")(obs, act, rows["next_observations"], ctx=ctx)
    assert np.array_equal(rows["terminals"].astype(bool), term) and 0 < term.sum() < n
    assert ns.value == int((~term[:, 0]).sum())
    assert np.array_equal(nxt.numpy()[:ns.value], rows["next_observations"][~term[:, 0]])   # obs = next_obs[~terminal], in order
    assert max(ring._traj_endpoints.values()) == n   # add_path ends with terminate_episode: the step's block closes a trajectory
    assert np.array_equal(mo.numpy(), midx)
    # Philox members: only elites, and the same draws from the same counter
    el = np.array([1, 3], np.int32)
    m1, m2 = ctx.empty((n,), np.int32), ctx.empty((n,), np.int32)
    from ilswiss_amd.mbpo import BNN  # noqa: F401
    p0 = bnn.get_opt()[2]
    _lib.check(ctx.lib.ilsx_mbpo_model_step(bnn.h, None, None, kind, d_obs.ptr, d_act.ptr, n, el.ctypes.data_as(C.c_void_p), 2, 0, None,
                                            None, None, m1.ptr, nxt.ptr, C.byref(ns)))
    a1 = nxt.numpy()
    bnn.set_opt(*bnn.get_opt()[:2], p0)
    _lib.check(ctx.lib.ilsx_mbpo_model_step(bnn.h, None, None, kind, d_obs.ptr, d_act.ptr, n, el.ctypes.data_as(C.c_void_p), 2, 0, None,
                                            None, None, m2.ptr, nxt.ptr, C.byref(ns)))
    assert set(np.unique(m1.numpy())) == {1, 3} and np.array_equal(m1.numpy(), m2.numpy()) and np.array_equal(a1, nxt.numpy())
    bnn.close()


def test_trainer_train_step_elites_and_snapshot(ctx):
    rng = np.random.default_rng(12)
    obs, act, rew, nobs = _data(rng, 600)
    rb = _ring(ctx, obs, act, rew, nobs)
    bnn, tr = _bnn(ctx, E=4, B=128)
    tr.max_epochs = 3
    np.random.seed(0)
    out = tr.train_step(rb)
    assert out["epochs"] == 3 and len(tr._model_idx) == 2 and "BNN Loss" in tr.get_eval_statistics()
    ho = np.sort(out["holdout_mse"])
    assert np.isclose(tr.get_eval_statistics()["BNN Loss"], ho[:2].mean())
    snap = tr.get_snapshot()
    bnn2, tr2 = _bnn(ctx, E=4, B=128, seed=99)
    tr2.load_snapshot(snap)
    assert np.array_equal(bnn2.get_flat_params(), bnn.get_flat_params()) and tr2._model_idx == tr._model_idx
    assert np.array_equal(bnn2.normalizer.std, bnn.normalizer.std)
    bnn.close(), bnn2.close()


def test_mbpo_exp_script_hopper_end_to_end(tmp_path):
    import yaml
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "mbpo", "mbpo_hopper_hip.yaml")))
    c = spec["constants"]
    c["mbpo_params"].update(num_epochs=2, num_steps_per_epoch=300, min_steps_before_training=400, rollout_batch_size=2000,
                            num_steps_per_eval=1000, max_path_length=200, replay_buffer_size=20000, model_replay_buffer_size=5000,
                            model_train_freq=150, num_train_steps_per_train_call=2, freq_saving=1, rollout_schedule=[0, 2, 1, 3])
    c["bnn_params"].update(max_epochs=2, log_freq=1)
    spec_path = tmp_path / "mbpo_small.yaml"
    spec_path.write_text(yaml.safe_dump(spec))
    env = dict(os.environ)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "run_scripts", "mbpo_exp_script.py"), "-e",
                        str(spec_path)], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    prog = glob.glob(str(tmp_path / "logs" / "*" / "*" / "progress.csv"))
    assert len(prog) == 1
    rows = list(csv.DictReader(open(prog[0])))
    assert len(rows) == 2
    for k in ("BNN Loss", "mean_rollout_length", "QF1 Loss", "Policy Loss", "AverageReturn", "Epoch"):
        assert k in rows[-1] and rows[-1][k] != "", k
    assert 1.0 <= float(rows[-1]["mean_rollout_length"]) <= 3.0


# ---- against tests/golden/g27_mbpo.npz (the reference's own BNN / BNNTrainer / FakeEnv, tools/make_golden.py)
def _golden():
    from conftest import load_golden
    return load_golden("g27_mbpo")


def _golden_bnn(ctx, g, tag):
    from ilswiss_amd.mbpo import BNN, BNNTrainer
    bnn = BNN(hidden_sizes=[40] * 4, output_size=12, input_size=14, num_nets=3, ctx=ctx, seed=0)
    tr = BNNTrainer(bnn, lr=1e-3, num_elites=2, reward_scale=2.0, batch_size=48, max_epochs=1, holdout_ratio=0.2, max_holdout=5000,
                    log_freq=1)
    bnn.set_params([g[f"{tag}_{i}"] for i in range(10)])
    return bnn, tr


def test_golden_forward(ctx):
    g = _golden()
    bnn, _ = _golden_bnn(ctx, g, "p0")
    bnn.normalizer._set(g["fwd_norm_mean"], g["fwd_norm_std"])
    mu, lv = bnn.forward(g["fwd_x"], ret_log_var=True)
    m2, var = bnn.predict(g["fwd_x"], factored=True)
    assert _rel(mu, g["fwd_mean"]) < 1e-5 and _rel(lv, g["fwd_logvar"]) < 1e-5 and _rel(var, g["fwd_var"]) < 1e-5
    assert np.array_equal(m2, mu)
    bnn.close()


def test_golden_train_step_one_epoch(ctx):
    """BNNTrainer.train_step on the fixture's rows with the reference's np.random seed: holdout split, normaliser, three Adam steps
    (48, 48, 24 rows), holdout MSE, elites and BNN Loss as the reference's own train_step left them"""
    g = _golden()
    bnn, tr = _golden_bnn(ctx, g, "p0")
    np.random.seed(int(g["train_seed"]))
    out = tr.train_step(dict(observations=g["obs"], actions=g["act"], rewards=g["rew"], next_observations=g["nobs"]))
    assert out["epochs"] == 1 and out["grad_updates"] == 3
    m, s = bnn.normalizer._get()
    assert np.allclose(m, g["train_norm_mean"], rtol=1e-5, atol=1e-6) and np.allclose(s, g["train_norm_std"], rtol=1e-5)
    err = max(float(np.max(np.abs(a - g[f"p3_{i}"]))) for i, a in enumerate(bnn.get_params()))
    assert err < 5e-5, err
    assert np.allclose(np.sort(g["train_holdout_mse"]), out["holdout_mse"], rtol=1e-4)
    assert tr._model_idx == list(g["train_elites"])
    assert np.isclose(tr.get_eval_statistics()["BNN Loss"], g["train_bnn_loss"], rtol=1e-4)
    assert _padding(bnn) == 0.0
    bnn.close()


def test_golden_fake_env_step(ctx, monkeypatch):
    """FakeEnv.step on Hopper with the reference's injected np.random.normal draw [E, n, D] and its members"""
    from ilswiss_amd.envs.terminals import get_terminal_func
    from ilswiss_amd.mbpo import FakeEnv
    g = _golden()
    bnn, tr = _golden_bnn(ctx, g, "p3")
    bnn.normalizer._set(g["train_norm_mean"], g["train_norm_std"])
    midx = g["fe_midx"]
    monkeypatch.setattr(np.random, "normal", lambda size=None, **kw: g["fe_noise"].reshape(size))
    env = FakeEnv(tr, get_terminal_func("hopper"), lambda k: midx[:k])
    nob, rew, term, _ = env.step(g["fe_obs"], g["fe_act"])
    assert np.allclose(nob, g["fe_next_obs"], rtol=1e-5, atol=1e-5) and np.allclose(rew, g["fe_rew"], rtol=1e-5, atol=1e-5)
    assert np.array_equal(term, g["fe_term"])
    bnn.close()
