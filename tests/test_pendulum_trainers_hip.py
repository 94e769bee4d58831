"""GPU suite: the continuous trainers at Pendulum's shapes (o = 3, a = 1: one action column) against their oracles — SAC-alpha
(oracle/sac_alpha.py), SAC-V (oracle/sac_v.py), TD3 (oracle/td3.py) and PPO (oracle/ppo.py) — and a 2-epoch run of each new Pendulum spec
through its run script, finishing with finite statistics."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

SAC_KW = dict(reward_scale=2.0, discount=0.99, policy_lr=3e-4, qf_lr=1e-3, alpha_lr=3e-4, soft_target_tau=0.005,
              alpha=0.2, train_alpha=True, policy_mean_reg_weight=1e-3, policy_std_reg_weight=1e-3, beta_1=0.9)
SACV_KW = dict(reward_scale=1.0, discount=0.99, alpha=0.2, policy_lr=3e-4, qf_lr=3e-4, vf_lr=3e-4, soft_target_tau=0.005,
               policy_mean_reg_weight=1e-3, policy_std_reg_weight=1e-3, beta_1=0.9)
TD3_KW = dict(reward_scale=1.0, discount=0.99, policy_lr=3e-4, qf_lr=3e-4, policy_and_target_update_period=2, soft_target_tau=0.005)
PPO_KW = dict(reward_scale=1.0, discount=0.99, clip_eps=0.2, policy_lr=3e-4, value_lr=3e-4, gae_tau=0.95, value_l2_reg=1e-3,
              mini_batch_size=48, update_epoch=3)


def _batch(rng, B, o, a):
    return dict(observations=rng.normal(0, 1, (B, o)).astype(np.float32),
                actions=np.tanh(rng.normal(0, 1, (B, a))).astype(np.float32),
                rewards=rng.normal(-3, 2, (B, 1)).astype(np.float32),
                terminals=np.zeros((B, 1), np.float32),
                next_observations=rng.normal(0, 1, (B, o)).astype(np.float32))


@pytest.mark.parametrize("o,a,H,B", [(3, 1, 256, 256), (3, 1, 64, 32)])
def test_sac_alpha_steps_vs_oracle(ctx, o, a, H, B):
    """5 chained SoftActorCritic.train_step calls at one action column: losses, statistics, gradients, alpha and every parameter."""
    import ilswiss_amd as ia
    from oracle import mlp as omlp
    from oracle.sac_alpha import SacAlphaOracle
    rng = np.random.default_rng(H + B)
    hidden = [H, H]
    pi0 = omlp.init_mlp(rng, o, hidden, a, init_w=1e-3, n_heads=2)
    q10, q20 = omlp.init_mlp(rng, o + a, hidden, 1), omlp.init_mlp(rng, o + a, hidden, 1)
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden, o, a, ctx=ctx)
    q1, q2 = ia.FlattenMlp(hidden, 1, o + a, ctx=ctx), ia.FlattenMlp(hidden, 1, o + a, ctx=ctx)
    pol.set_flat_params(pi0), q1.set_flat_params(q10), q2.set_flat_params(q20)
    tr = ia.SoftActorCritic(pol, q1, q2, max_batch=B, **SAC_KW)
    orc = SacAlphaOracle(o, a, hidden, pi0, q10, q20, **SAC_KW)
    for s in range(5):
        batch = _batch(rng, B, o, a)
        e1, e2 = rng.normal(0, 1, (B, a)).astype(np.float32), rng.normal(0, 1, (B, a)).astype(np.float32)
        tr.end_epoch()
        tr.train_step(batch, e1, e2)
        res = orc.train_step(batch, e1, e2)
        st = tr.get_eval_statistics()
        for k_ref, k_or in (("QF1 Loss", "qf1_loss"), ("QF2 Loss", "qf2_loss"), ("Policy Loss", "policy_loss"), ("Alpha Loss", "alpha_loss")):
            np.testing.assert_allclose(st[k_ref], res[k_or], rtol=2e-4, atol=2e-6, err_msg=f"{k_ref} step {s}")
        np.testing.assert_allclose(st["Log Pis Mean"], res["log_pi"].mean(), rtol=1e-4, atol=1e-5)
        for name, arr in (("Q1 Predictions", res["q1_pred"]), ("Log Pis", res["log_pi"]), ("Policy mu", res["policy_mean"]),
                          ("Policy log std", res["policy_log_std"])):
            np.testing.assert_allclose(st[name + " Std"], arr.std(), rtol=1e-4, atol=1e-6, err_msg=name)
            np.testing.assert_allclose(st[name + " Max"], arr.max(), rtol=1e-4, atol=1e-5, err_msg=name)
            np.testing.assert_allclose(st[name + " Min"], arr.min(), rtol=1e-4, atol=1e-5, err_msg=name)
        for nm, key in (("qf1", "q1_grad"), ("qf2", "q2_grad"), ("policy", "pi_grad")):
            got, ref = tr.get_grads(nm), res[key]
            assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), (s, nm, np.abs(got - ref).max(), np.abs(ref).max())
        np.testing.assert_allclose(tr.log_alpha, orc.log_alpha[0], rtol=0, atol=1e-6)
        for nm, ov in (("policy", orc.pi), ("qf1", orc.q1), ("qf2", orc.q2), ("target_qf1", orc.tq1), ("target_qf2", orc.tq2)):
            np.testing.assert_allclose(tr.get_params(nm), ov, rtol=0, atol=5e-5, err_msg=f"{nm} step {s}")


def test_sac_v_steps_vs_oracle(ctx):
    from ilswiss_amd.networks import FlattenMlp, ReparamTanhMultivariateGaussianPolicy
    from ilswiss_amd.sac_v import SoftActorCriticV
    from oracle import mlp as omlp
    from oracle.sac_v import SacVOracle
    rng = np.random.default_rng(7)
    o, a, hid, B = 3, 1, [256, 256], 256
    pi0 = omlp.init_mlp(rng, o, hid, a, init_w=1e-3, n_heads=2)
    pi0[-(2 * (hid[-1] * a + a)):] *= 100.0
    q10, q20, vf0 = omlp.init_mlp(rng, o + a, hid, 1), omlp.init_mlp(rng, o + a, hid, 1), omlp.init_mlp(rng, o, hid, 1)
    orc = SacVOracle(o, a, hid, pi0, q10, q20, vf0, **SACV_KW)
    pol = ReparamTanhMultivariateGaussianPolicy(hid, o, a, ctx=ctx, seed=1)
    q1, q2, vf = FlattenMlp(hid, 1, o + a, ctx=ctx, seed=2), FlattenMlp(hid, 1, o + a, ctx=ctx, seed=3), FlattenMlp(hid, 1, o, ctx=ctx, seed=4)
    for net, p0 in ((pol, pi0), (q1, q10), (q2, q20), (vf, vf0)):
        net.set_flat_params(p0)
    tr = SoftActorCriticV(pol, q1, q2, vf, max_batch=B, **SACV_KW)
    for s in range(4):
        batch = _batch(rng, B, o, a)
        eps = rng.normal(0, 1, (B, a)).astype(np.float32)
        res = orc.train_step(batch, eps)
        tr.eval_statistics = None
        tr.train_step(batch, eps=eps)
        st = tr.get_eval_statistics()
        for ref, k in (("QF1 Loss", "qf1_loss"), ("VF Loss", "vf_loss"), ("Policy Loss", "policy_loss")):
            np.testing.assert_allclose(st[ref], res[k], rtol=3e-4, atol=2e-6, err_msg=f"step {s} {ref}")
        np.testing.assert_allclose(st["Log Pis Mean"], res["log_pi"].mean(), rtol=1e-4, atol=1e-5)
    for k in ("pi", "q1", "q2", "vf", "tvf"):
        np.testing.assert_allclose(tr.get_flat_params(k), getattr(orc, k), rtol=0, atol=1e-4, err_msg=k)


def test_td3_steps_vs_oracle(ctx):
    from ilswiss_amd.networks import FlattenMlp
    from ilswiss_amd.td3 import TD3, MlpGaussianNoisePolicy
    from oracle import mlp as omlp
    from oracle.td3 import TD3Oracle
    rng = np.random.default_rng(61)
    o, a, hid, B = 3, 1, [256, 256], 256
    pi0, q10, q20 = omlp.init_mlp(rng, o, hid, a, init_w=1e-3), omlp.init_mlp(rng, o + a, hid, 1), omlp.init_mlp(rng, o + a, hid, 1)
    pi0[-(256 * a + a):] *= 100.0
    orc = TD3Oracle(o, a, hid, pi0, q10, q20, policy_noise=0.2, policy_noise_clip=0.5, output_activation="tanh", **TD3_KW)
    pol = MlpGaussianNoisePolicy(hid, o, a, policy_noise=0.2, policy_noise_clip=0.5, output_activation="tanh", ctx=ctx, seed=1)
    q1, q2 = FlattenMlp(hid, 1, o + a, ctx=ctx, seed=2), FlattenMlp(hid, 1, o + a, ctx=ctx, seed=3)
    pol.set_flat_params(pi0); q1.set_flat_params(q10); q2.set_flat_params(q20)
    tr = TD3(pol, q1, q2, max_batch=B, **TD3_KW)
    for s in range(6):
        batch = _batch(rng, B, o, a)
        eps = rng.normal(0, 1, (B, a)).astype(np.float32)
        orc.train_step(batch, eps)
        tr.train_step(batch, eps_target=eps)
    for k in ("pi", "q1", "q2", "tpi", "tq1", "tq2"):
        np.testing.assert_allclose(tr.get_flat_params(k), getattr(orc, k), rtol=0, atol=1e-4, err_msg=k)
    obs = rng.normal(0, 1, (64, o)).astype(np.float32)
    det = pol.get_actions(obs, deterministic=True)
    np.testing.assert_allclose(det, orc.policy(orc.pi, obs)[0], rtol=1e-4, atol=2e-5)


def test_ppo_update_vs_oracle(ctx):
    """GAE and one PPO update (3 epochs of minibatches, ragged last one) at one action column, action_log_std of width 1."""
    from ilswiss_amd.networks import FlattenMlp
    from ilswiss_amd.ppo import PPO, ReparamMultivariateGaussianPolicy
    from oracle import mlp as omlp
    from oracle.ppo import PPOOracle
    rng = np.random.default_rng(98)
    o, a, hid = 3, 1, [256, 256]
    vf0 = omlp.init_mlp(rng, o, hid, 1)
    pi0 = np.concatenate([omlp.init_mlp(rng, o, hid, a, init_w=1e-3, last_scale=(0.1, 0.0)), rng.normal(-0.5, 0.2, a).astype(np.float32)])
    trajs = [dict(observations=rng.normal(0, 1, (L, o)).astype(np.float32), actions=rng.normal(0, 0.7, (L, a)).astype(np.float32),
                  rewards=rng.normal(-5, 2.0, (L, 1)).astype(np.float32)) for L in (200, 200, 37, 2)]
    N = sum(t["rewards"].shape[0] for t in trajs)
    perms = np.stack([rng.permutation(N) for _ in range(3)])
    orc = PPOOracle(o, a, hid, pi0, vf0, **PPO_KW)
    pol = ReparamMultivariateGaussianPolicy(hid, o, a, conditioned_std=False, hidden_activation="tanh", ctx=ctx, seed=3)
    vf = FlattenMlp(hid, 1, o, hidden_activation="tanh", ctx=ctx, seed=4)
    tr = PPO(pol, vf, max_samples=4096, **PPO_KW)
    tr.set_flat_params(pi0, vf0)
    R, A, V, lp = tr.calc_adv(trajs)
    _, _, R0, A0, V0 = orc.calc_adv(trajs)
    np.testing.assert_allclose(V, V0, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(A, A0, rtol=2e-4, atol=2e-5)
    orc.train_step(trajs, list(perms))
    tr.train_step(trajs, perms)
    np.testing.assert_allclose(tr.get_flat_params(1), orc.vf, rtol=0, atol=5e-5)
    np.testing.assert_allclose(tr.get_flat_params(0), orc.pi, rtol=0, atol=5e-5)


@pytest.mark.parametrize("spec,script,over", [
    ("sac/sac_pendulum_hip.yaml", "sac_alpha_exp_script.py",
     dict(num_epochs=2, num_steps_per_epoch=400, num_steps_between_train_calls=400, num_train_steps_per_train_call=100,
          min_steps_before_training=200, num_steps_per_eval=400, max_path_length=200, freq_saving=1)),
    ("ppo/ppo_pendulum_hip.yaml", "ppo_exp_script.py",
     dict(num_epochs=2, num_steps_per_epoch=1024, num_steps_between_train_calls=512, min_steps_before_training=512,
          num_steps_per_eval=400, freq_saving=1))])
def test_spec_runs_two_epochs(tmp_path, spec, script, over):
    import yaml
    s = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", spec)))
    s["constants"]["rl_alg_params"].update(over)
    s["variables"]["seed"] = s["variables"]["seed"][:1]
    (tmp_path / "spec.yaml").write_text(yaml.safe_dump(s))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_scripts", script), "-e", str(tmp_path / "spec.yaml")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    found = [os.path.join(d, "progress.csv") for d, _, fs in os.walk(tmp_path / "logs") if "progress.csv" in fs]
    assert len(found) == 1
    rows = list(csv.DictReader(open(found[0])))
    assert len(rows) >= 2
    for col in ("AverageReturn", "Epoch", "Number of env steps total"):
        assert col in rows[0], col
    def num(v):
        try:
            return float(v)
        except (TypeError, ValueError):
            return None
    for row in rows:
        vals = [num(v) for v in row.values()]
        assert all(np.isfinite(v) for v in vals if v is not None), row
        assert float(row["AverageReturn"]) < 0.0           # every Pendulum reward is <= 0
