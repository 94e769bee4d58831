"""Gradient-level parity of the behaviour-cloning step (ilsx_bc_*: BC, DAgger, GCSL's MSE mode) against the float64 autograd restatement of
tests/bc_restatement.py, over the shapes at which the device step changes path, and the tanh-Gaussian head calls on real trunks.

Parameters after Adam say little about a gradient: the update is lr * m / (sqrt(v) + 1e-8), so a gradient that is wrong by a constant factor
(1/max_batch for 1/B, a lost 2 in the MSE branch) moves the parameters exactly as the right one does.  The gradient itself is read here: a
trainer built with momentum = 0 has beta_1 = 0, its first Adam moment IS the gradient of the last step, and get_snapshot() returns it in the
flat ABI layout (exp_avg), with exp_avg_sq = 0.001 * g^2 after the first step.

Bounds (each one the project's existing figure for that quantity): gradient <= 1e-4 of the largest reference entry, here PER parameter block
so that a small block cannot hide behind a large one; statistic rtol 2e-4 / atol 2e-5; parameters after chained steps atol 1e-4 at these
widths; log-prob of given actions rtol 2e-4 / atol 2e-3; actions rtol 1e-5 / atol 2e-6; sampled log-prob the Jacobian-aware bound of
oracle.tanh_gaussian.logp_fp32_tolerance(ulps=8).  What keeps them honest is checked without a GPU (the first two tests): the numpy fp32
oracle sits within 1e-5 per block of the float64 restatement on every case (a tenth of the device bound), and its fp32 trunk meets the head
bounds on the head cases."""
import functools

import numpy as np
import pytest

import bc_restatement as R
from oracle import mlp as omlp
from oracle import tanh_gaussian as otg
from oracle.bc import BCOracle

gpu = pytest.mark.gpu
CASE_MODE = [(c, m) for c in R.CASES for m in R.MODES]
STAT_KEY = dict(MLE="Log-Likelihood", MSE="MSE")
HEAD_CASES, HEAD_ROWS = ("ragged", "spec", "humanoid"), (1, 17, 1000)


@functools.lru_cache(maxsize=None)
def _case(case, mode):
    """(pi0, obs, acts, eps, float64 reference) of one cell of the matrix, computed once and never written to."""
    o, a, hidden, _, _ = R.CASES[case]
    pi0, obs, acts, eps, _ = R.make_case(case, mode)
    ref = R.bc_reference(pi0, obs, acts, eps, o, hidden, a, mode)
    for x in (pi0, obs, acts, eps, ref["grad"], ref["lsr"]):
        x.setflags(write=False)
    return pi0, obs, acts, eps, ref


def _assert_regimes(case, mode, lsr):
    """The raw log-std really sits on the sides of the clamp the case is about."""
    above, below = float(np.mean(lsr > otg.LOG_SIG_MAX)), float(np.mean(lsr < otg.LOG_SIG_MIN))
    print(f"{case} {mode}: raw log-std above +2: {above:.3f}, below -20: {below:.3f}")
    if case == "one_row":          # a = 3, one row: one dimension per side is all there is
        assert above > 0 and (below > 0 if mode == "MSE" else below == 0)
    elif mode == "MSE":
        assert above >= 0.05 and below >= 0.05
    else:
        assert above >= 0.02 and below == 0


def _assert_blocks(got, ref, dims, rel, what):
    """max|got - ref| <= rel * max|ref| on every W and b block (an all-zero reference block therefore demands exact zeros)."""
    errs = R.block_errors(np.asarray(got, np.float64), ref, *dims)
    print(what, " ".join(f"{nm}:{e:.2e}/{m:.2e}" for nm, e, m in errs))
    bad = [(nm, e, m) for nm, e, m in errs if not e <= rel * m]
    assert not bad, (what, rel, bad)


# ------------------------------------------------------------------------------------------- without a GPU: the references agree
@pytest.mark.parametrize("case,mode", CASE_MODE)
def test_restatement_agrees_with_the_oracle(case, mode):
    """Autograd in float64 and the oracle's hand-derived fp32 backward: gradient within 1e-5 per block, the statistic, the clamp regimes.
    In MSE mode the clamp's gate is visible by far: without it the log-std head's gradient moves by more than 1e-2 of its largest entry,
    a hundred times the device bound (in MLE mode the +-1 actions' entries dominate the blocks and the gate shows less)."""
    o, a, hidden, _, B = R.CASES[case]
    pi0, obs, acts, eps, ref = _case(case, mode)
    _assert_regimes(case, mode, ref["lsr"])
    assert acts[0, 0] == 1.0 and acts[-1, -1] == -1.0 and obs.shape == (B, o)
    res = BCOracle(o, a, hidden, pi0, mode=mode, lr=1e-3, momentum=0.0).update(obs, acts, eps)
    _assert_blocks(res["grad"], ref["grad"], (o, hidden, a), 1e-5, f"{case} {mode} oracle")
    np.testing.assert_allclose(res["stat"], ref["stat"], rtol=2e-5, atol=2e-6)
    mu, lsr = R.trunk_f64(pi0, obs, o, hidden, a)
    if mode == "MLE":
        np.testing.assert_allclose(ref["stat"], otg.log_prob_of_action(mu, lsr, acts, dtype=np.float64).mean(), rtol=1e-12)
    else:
        pred = otg.head_forward(mu, lsr, eps, dtype=np.float64)["action"]
        np.testing.assert_allclose(ref["stat"], np.sum((pred - acts.astype(np.float64)) ** 2, 1).mean(), rtol=1e-12)
        ungated = R.bc_reference(pi0, obs, acts, eps, o, hidden, a, mode, gate=False)["grad"]
        moved = {nm: e / m for nm, e, m in R.block_errors(ungated, ref["grad"], o, hidden, a) if m > 0}
        n = len(hidden) + 1
        print(f"{case} {mode}: without the gate the log-std head moves by {moved[f'W{n}']:.2e} (W), {moved[f'b{n}']:.2e} (b) of its largest entry")
        assert moved[f"W{n}"] > 1e-2 and moved[f"b{n}"] > 1e-2


@functools.lru_cache(maxsize=None)
def _head_case(case, rows):
    """A case's policy with the scaled heads (the MLE bias pattern: at log_std = -20 a log-prob of given actions is fp32-meaningless),
    `rows` inputs and the float64 values of everything the head calls return."""
    o, a, hidden, _, _ = R.CASES[case]
    rng = np.random.default_rng(9000 + 10 * HEAD_CASES.index(case) + rows)
    pi = R.make_policy(rng, o, a, hidden, "MLE")
    obs, acts, eps = R.make_batch(rng, rows, o, a)
    mu, lsr = R.trunk_f64(pi, obs, o, hidden, a)
    fw = otg.head_forward(mu, lsr, eps, dtype=np.float64)
    out = dict(pi=pi, obs=obs, acts=acts, eps=eps, mu=mu, lsr=lsr, det=np.tanh(mu), action=fw["action"], logp=fw["log_prob"],
               logp_of_acts=otg.log_prob_of_action(mu, lsr, acts, dtype=np.float64))
    for x in out.values():
        x.setflags(write=False)
    return out


def _assert_head(h, lp_of_acts, det, action, logp, mean, log_std):
    np.testing.assert_allclose(lp_of_acts, h["logp_of_acts"], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(det, h["det"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(action, h["action"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(mean, h["mu"], rtol=2e-5, atol=2e-5)          # the MLP forward bound of test_mlp_forward_vs_oracle
    np.testing.assert_allclose(log_std, np.clip(h["lsr"], otg.LOG_SIG_MIN, otg.LOG_SIG_MAX), rtol=2e-5, atol=2e-5)
    err, tol = np.abs(logp - h["logp"]), otg.logp_fp32_tolerance(h["action"], ulps=8.0)
    print(f"sampled log-prob: worst error / bound {np.max(err / tol):.3f}")
    assert np.all(err <= tol), (err.max(), np.max(err / tol))


@pytest.mark.parametrize("rows", HEAD_ROWS)
@pytest.mark.parametrize("case", HEAD_CASES)
def test_head_bounds_hold_for_the_fp32_oracle(case, rows):
    """The head bounds are meant for fp32: the numpy fp32 trunk and head formulas meet them against float64 on these inputs."""
    o, a, hidden, _, _ = R.CASES[case]
    h = _head_case(case, rows)
    (mu, lsr), _ = omlp.forward(h["pi"], h["obs"], o, hidden, a, n_heads=2)
    fw = otg.head_forward(mu, lsr, h["eps"])
    assert np.mean(h["lsr"] > otg.LOG_SIG_MAX) > 0 or rows == 1
    assert h["lsr"].min() > -10.0
    _assert_head(h, otg.log_prob_of_action(mu, lsr, h["acts"]), np.tanh(mu), fw["action"], fw["log_prob"], mu, fw["log_std"])


# ------------------------------------------------------------------------------------------- the device step
def _trainer(ctx, case, mode, pi0, momentum=0.0, lr=1e-3):
    import ilswiss_amd as ia
    from ilswiss_amd.bc import BC
    o, a, hidden, max_batch, _ = R.CASES[case]
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden, o, a, ctx=ctx, seed=1)
    assert pol.num_params == pi0.size
    pol.set_flat_params(pi0)
    return BC(mode, pol, batch_size=max_batch, lr=lr, momentum=momentum), pol


def _step(tr, mode, obs, acts, eps):
    """One train_step that reports its statistic; returns (gradient = exp_avg at beta_1 = 0, optimiser state, statistic)."""
    tr.end_epoch()
    tr.train_step(dict(observations=obs, actions=acts), eps=eps if mode == "MSE" else None)
    opt = tr.get_snapshot()["optimizer"]
    return opt["exp_avg"], opt, tr.get_eval_statistics()[STAT_KEY[mode]]


@gpu
@pytest.mark.parametrize("case,mode", CASE_MODE)
def test_hip_bc_gradient_vs_float64(ctx, case, mode):
    """The device gradient of one step (exp_avg at beta_1 = 0), its square in exp_avg_sq and the statistic, per parameter block.  The
    `unequal` case goes on for three steps: the padded units never show in the ABI vectors, and an element whose gradient is exactly zero
    in every step (a unit no row switches on, a log-std column every row clamps) keeps its initial value."""
    o, a, hidden, _, B = R.CASES[case]
    dims = (o, hidden, a)
    pi0, obs, acts, eps, ref = _case(case, mode)
    _assert_regimes(case, mode, ref["lsr"])
    tr, pol = _trainer(ctx, case, mode, pi0)
    g, opt, stat = _step(tr, mode, obs, acts, eps)
    assert opt["step"] == 1 and g.size == pi0.size
    _assert_blocks(g, ref["grad"], dims, 1e-4, f"{case} {mode} grad")
    _assert_blocks(opt["exp_avg_sq"], 0.001 * ref["grad"] ** 2, dims, 2e-4, f"{case} {mode} exp_avg_sq")
    print(f"{case} {mode} statistic {stat!r} vs {ref['stat']!r}")
    np.testing.assert_allclose(stat, ref["stat"], rtol=2e-4, atol=2e-5)
    if case != "unequal":
        return
    rng = R.make_case(case, mode)[-1]
    zero = ref["grad"] == 0
    for s in range(1, 4):
        p = pol.get_flat_params()
        assert p.size == pi0.size
        obs, acts, eps = R.make_batch(rng, B, o, a)
        ref_s = R.bc_reference(p, obs, acts, eps, o, hidden, a, mode)
        g, opt, stat = _step(tr, mode, obs, acts, eps)
        assert opt["step"] == s + 1 and g.size == pi0.size and opt["exp_avg_sq"].size == pi0.size
        _assert_blocks(g, ref_s["grad"], dims, 1e-4, f"{case} {mode} grad step {s}")
        np.testing.assert_allclose(stat, ref_s["stat"], rtol=2e-4, atol=2e-5)
        zero &= ref_s["grad"] == 0
    p = pol.get_flat_params()
    print(f"{case} {mode}: {int(zero.sum())} of {zero.size} elements have a zero gradient in all four steps")
    assert zero.sum() > 0 and p.size == pi0.size
    np.testing.assert_array_equal(p[zero], pi0[zero])
    assert np.abs(p - pi0).max() > 1e-4          # the rest did move


@gpu
@pytest.mark.parametrize("mode", R.MODES)
def test_hip_bc_small_batch_after_a_full_one_reads_no_stale_rows(ctx, mode):
    """max_batch = 256 at [256, 256]: a step at B = 256, the initial parameters again, then a step at B = 17 on other data.  The second
    gradient is that of the 17 rows alone; a contraction or a head that reads rows 17..255 of the workspaces shows here only."""
    o, a, hidden, _, _ = R.CASES["spec"]
    rng = np.random.default_rng(7700 + R.MODES.index(mode))
    pi0 = R.make_policy(rng, o, a, hidden, mode)
    full, few = R.make_batch(rng, 256, o, a), R.make_batch(rng, 17, o, a)
    ref = R.bc_reference(pi0, *few, o, hidden, a, mode)
    tr, pol = _trainer(ctx, "spec", mode, pi0)
    _step(tr, mode, *full)
    assert np.abs(pol.get_flat_params() - pi0).max() > 1e-4
    pol.set_flat_params(pi0)
    g, opt, stat = _step(tr, mode, *few)
    assert opt["step"] == 2
    _assert_blocks(g, ref["grad"], (o, hidden, a), 1e-4, f"stale rows {mode} grad")
    np.testing.assert_allclose(stat, ref["stat"], rtol=2e-4, atol=2e-5)


@gpu
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", ["spec", "row_split"])
def test_hip_bc_five_steps_with_momentum_vs_oracle(ctx, case, mode):
    """Five chained steps at betas = (0.9, 0.999), lr 3e-4, fresh batches, against the fp32 oracle: parameters and every step's statistic."""
    o, a, hidden, _, B = R.CASES[case]
    rng = np.random.default_rng(7800 + 10 * list(R.CASES).index(case) + R.MODES.index(mode))
    pi0 = R.make_policy(rng, o, a, hidden, mode)
    tr, pol = _trainer(ctx, case, mode, pi0, momentum=0.9, lr=3e-4)
    orc = BCOracle(o, a, hidden, pi0, mode=mode, lr=3e-4, momentum=0.9)
    for s in range(5):
        obs, acts, eps = R.make_batch(rng, B, o, a)
        res = orc.update(obs, acts, eps)
        _, opt, stat = _step(tr, mode, obs, acts, eps)
        print(f"{case} {mode} step {s}: statistic {stat!r} vs {res['stat']!r}, parameters off by {np.abs(pol.get_flat_params() - orc.pi).max():.2e}")
        np.testing.assert_allclose(stat, res["stat"], rtol=2e-4, atol=2e-5, err_msg=f"step {s}")
        np.testing.assert_allclose(pol.get_flat_params(), orc.pi, rtol=0, atol=1e-4, err_msg=f"step {s}")
    assert opt["step"] == 5
    assert np.abs(orc.pi - pi0).max() > 1e-3


@gpu
@pytest.mark.parametrize("rows", HEAD_ROWS)
@pytest.mark.parametrize("case", HEAD_CASES)
def test_hip_policy_head_calls_on_real_trunks(ctx, case, rows):
    """get_log_prob, deterministic get_actions and the sampling forward on two-layer trunks at H = 128 / 256 with heads that spread."""
    import ilswiss_amd as ia
    o, a, hidden, _, _ = R.CASES[case]
    h = _head_case(case, rows)
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden, o, a, ctx=ctx, seed=1)
    pol.set_flat_params(h["pi"])
    action, mean, log_std, logp, *_ = pol.forward(h["obs"], return_log_prob=True, eps=h["eps"])
    _assert_head(h, pol.get_log_prob(h["obs"], h["acts"]), pol.get_actions(h["obs"], deterministic=True), action, logp, mean, log_std)
