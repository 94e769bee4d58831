"""CPU suite: the MBPO restatement (tests/mbpo_restatement.py) and the shipped schedule / split arithmetic (ilswiss_amd/mbpo.py) against
tests/golden/g27_mbpo.npz, which tools/make_golden.py writes by running the reference's own BNN, BNNTrainer, FakeEnv and MBPO."""
import numpy as np
import torch
from conftest import load_golden

import mbpo_restatement as R


def G():
    return load_golden("g27_mbpo")


def _params(g, tag):
    return [g[f"{tag}_{i}"] for i in range(10)]


def _data(g, reward_scale=2.0):
    return R.data_from_rows(g["obs"], g["act"], g["rew"], g["nobs"], reward_scale)


def test_fixture_init_rule_and_layout():
    g = G()
    p0 = _params(g, "p0")
    assert [p.shape for p in p0] == R.shapes(3, 14, [40] * 4, 12)
    for li in range(4):
        W, b = p0[2 * li], p0[2 * li + 1]
        bound = 1 / np.sqrt(W.shape[1] * W.shape[2])
        assert np.abs(W).max() <= bound and np.abs(W).max() > 0.9 * bound and np.all(b == np.float32(0.1))
    assert np.abs(p0[8]).max() <= 3e-3 and np.abs(p0[9]).max() <= 3e-3


def test_restatement_forward_and_losses():
    g = G()
    p0 = _params(g, "p0")
    x, t = _data(g)
    m, s = R.normalizer_stats(x)
    assert np.allclose(m, g["fwd_norm_mean"], rtol=1e-6, atol=1e-7) and np.allclose(s, g["fwd_norm_std"], rtol=1e-6)
    with torch.no_grad():
        mu, lv = R.forward(p0, g["fwd_norm_mean"], g["fwd_norm_std"], g["fwd_x"])
        assert np.allclose(mu.numpy(), g["fwd_mean"], rtol=1e-5, atol=1e-7) and np.allclose(lv.numpy(), g["fwd_logvar"], rtol=1e-5, atol=1e-6)
        assert np.allclose(np.exp(lv.numpy()), g["fwd_var"], rtol=1e-5)
        idx = g["loss_idx"]
        l1 = R.compute_loss(p0, g["fwd_norm_mean"], g["fwd_norm_std"], x[idx], t[idx], add_var_loss=True).numpy()
        l0 = R.compute_loss(p0, g["fwd_norm_mean"], g["fwd_norm_std"], x[idx], t[idx], add_var_loss=False).numpy()
    assert np.allclose(l1, g["loss_var"], rtol=1e-5) and np.allclose(l0, g["loss_novar"], rtol=1e-5)


def test_restatement_one_epoch_of_train_step():
    """three Adam steps (48, 48 and a short 24-row batch) on the reference's own index draws, then holdout MSE, elites and BNN Loss"""
    g = G()
    x, t = _data(g)
    perm, idxs = g["train_perm"], g["train_idxs"]
    tr_rows, ho = perm[30:], perm[:30]
    m, s = R.normalizer_stats(x[tr_rows])
    assert np.allclose(m, g["train_norm_mean"], rtol=1e-6, atol=1e-7) and np.allclose(s, g["train_norm_std"], rtol=1e-6)
    from ilswiss_amd.mbpo import default_weight_decays
    ref = R.AdamTrainer(_params(g, "p0"), 1e-3, default_weight_decays(4))
    for lo in (0, 48, 96):
        rows = tr_rows[idxs[:, lo:lo + 48]]
        ref.step(g["train_norm_mean"], g["train_norm_std"], x[rows], t[rows])
    err = max(float(np.max(np.abs(a - b))) for a, b in zip(ref.params(), _params(g, "p3")))
    assert err < 1e-6, err
    with torch.no_grad():
        ho_mse = R.compute_loss(_params(g, "p3"), g["train_norm_mean"], g["train_norm_std"], x[ho], t[ho], add_var_loss=False).numpy()
    assert np.allclose(ho_mse, g["train_holdout_mse"], rtol=1e-6)
    assert list(np.argsort(ho_mse)[:2]) == list(g["train_elites"])
    assert np.isclose(np.sort(ho_mse)[:2].mean(), g["train_bnn_loss"], rtol=1e-6)


def test_restatement_fake_env_step():
    g = G()
    midx = g["fe_midx"]
    noise = g["fe_noise"][midx, np.arange(len(midx))]
    nob, rew = R.fake_env_step(_params(g, "p3"), g["train_norm_mean"], g["train_norm_std"], g["fe_obs"], g["fe_act"], midx, noise)
    assert np.allclose(nob, g["fe_next_obs"], rtol=1e-5, atol=1e-5) and np.allclose(rew, g["fe_rew"], rtol=1e-5, atol=1e-5)
    assert 0 < g["fe_term"].sum() < len(midx)


def test_schedule_and_batch_split_match_the_reference():
    from ilswiss_amd.mbpo import batch_split, rollout_length_at
    g = G()
    for row in g["sched"]:
        assert rollout_length_at(list(row[:4]), int(row[4])) == int(row[5]), row
    for bs, rr, msize, real, model in g["split"]:
        assert batch_split(int(bs), rr, int(msize)) == (int(real), int(model))
