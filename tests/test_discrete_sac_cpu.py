"""CPU suite for discrete SAC: the torch restatement of one step (tests/dsac_restatement.py) against the reference's own trainer
(tests/golden/g28_discrete_sac.npz), the float64 CartPole restatement against hand-computed properties of gym 0.22's CartPoleEnv, and the
Python surface that needs no GPU (Discrete space, registry, refusals of the run script)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from dsac_restatement import DsacRestatement, cartpole_step, golden_cases  # noqa: E402

G28 = os.path.join(HERE, "golden", "g28_discrete_sac.npz")


@pytest.mark.parametrize("case", [0, 1])
def test_restatement_matches_reference_trainer(case):
    c = golden_cases(G28)[case]
    r = DsacRestatement(c["o"], [c["H"]] * 2, c["n"], c["pi0"], c["q10"], c["q20"], **c["kw"])
    idx = c["idx"]
    for s, b in enumerate(c["batches"]):
        out = r.train_step(b)
        for k, ref in (("q1_loss", "qf1_loss"), ("q2_loss", "qf2_loss"), ("policy_loss", "policy_loss")):
            assert abs(out[k] - float(c[f"s{s}_{ref}"])) <= 1e-5 * max(1.0, abs(float(c[f"s{s}_{ref}"]))), (s, k)
        for q in ("q1", "q2"):
            p = out[q + "_pred"]
            assert np.allclose([p.mean(), p.std(), p.max(), p.min()], c[f"s{s}_{q}_pred"], atol=1e-5), (s, q)
        if s == 0:
            for k in ("q1", "q2", "pi"):
                assert np.abs(out["grad_" + k][idx] - c["grad_" + k]).max() <= 1e-6, k
    for k in ("pi", "q1", "q2", "tq1", "tq2"):
        assert np.abs(r.params(k)[idx] - c[k]).max() <= 1e-6, k


def test_golden_log_pis_and_deterministic_actions_are_consistent():
    for c in golden_cases(G28):
        lp = c["log_pis"].astype(np.float64)
        assert np.allclose(np.exp(lp).sum(1), 1.0, atol=1e-5)
        assert np.array_equal(c["det_act"], lp.argmax(1))   # torch.max(log_probs, 1): the first maximal entry


def test_cartpole_constants_and_one_step_by_hand():
    # theta = 0, theta_dot = 0, push right: temp = 10 / 1.1, thetaacc = -temp / (0.5 * (4/3 - 0.1/1.1)), xacc = temp - 0.05 thetaacc / 1.1
    s = np.array([[0.1, 0.2, 0.0, 0.0]])
    nxt, rew, done = cartpole_step(s, np.array([1]))
    temp = 10.0 / 1.1
    thacc = -temp / (0.5 * (4.0 / 3.0 - 0.1 / 1.1))
    xacc = temp - 0.05 * thacc / 1.1
    assert np.allclose(nxt[0], [0.1 + 0.02 * 0.2, 0.2 + 0.02 * xacc, 0.0, 0.02 * thacc], rtol=0, atol=1e-15)
    assert rew[0] == 1.0 and not done[0]
    left, _, _ = cartpole_step(s, np.array([0]))
    assert left[0, 1] < s[0, 1] < nxt[0, 1]          # action 0 pushes left, 1 right


def test_cartpole_thresholds_are_strict_and_terminal_step_is_rewarded():
    th = 12 * 2 * math.pi / 360
    # positions that land exactly on / just past the bounds after x += 0.02 * x_dot with x_dot = 0
    for x, want in ((2.4, False), (-2.4, False), (np.nextafter(2.4, 3.0), True), (np.nextafter(-2.4, -3.0), True)):
        _, rew, done = cartpole_step(np.array([[x, 0.0, 0.0, 0.0]]), np.array([0]))
        assert bool(done[0]) == want and rew[0] == 1.0, x
    for t, want in ((th, False), (-th, False), (np.nextafter(th, 1.0), True), (np.nextafter(-th, -1.0), True)):
        _, rew, done = cartpole_step(np.array([[0.0, 0.0, t, 0.0]]), np.array([1]))
        assert bool(done[0]) == want and rew[0] == 1.0, t


def test_cartpole_random_episodes_end_and_stay_finite():
    rng = np.random.default_rng(0)
    s = rng.uniform(-0.05, 0.05, (256, 4))
    lens = np.zeros(256, int)
    alive = np.ones(256, bool)
    for t in range(200):
        s2, _, done = cartpole_step(s, rng.integers(0, 2, 256))
        lens += alive
        alive &= ~done
        s = np.where(alive[:, None], s2, s)
    assert np.isfinite(s).all() and (~alive).mean() > 0.9 and 8 <= np.median(lens) <= 60   # random play fails in ~20 steps


def test_discrete_space_and_registry():
    from ilswiss_amd.envs import CLASSIC, Discrete
    d = Discrete(5)
    assert d.n == 5 and int(np.prod(d.shape)) == 1 and all(0 <= d.sample() < 5 for _ in range(50))
    assert d.contains(4) and not d.contains(5) and "cartpole" in CLASSIC


def test_run_script_refuses_grouped_and_split_runs(tmp_path):
    import yaml
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "sac", "sac_cartpole_d_hip.yaml")))
    spec["constants"]["rl_alg_params"]["split_ranks"] = 2
    (tmp_path / "split.yaml").write_text(yaml.safe_dump(spec))
    script = os.path.join(ROOT, "run_scripts", "discrete_sac_exp_script.py")
    for extra, why in ((["-e", "a.yaml", "b.yaml"], "--group"), (["-e", "split.yaml"], "split_ranks")):
        r = subprocess.run([sys.executable, script] + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and why in (r.stdout + r.stderr), r.stdout + r.stderr
