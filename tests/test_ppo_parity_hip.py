"""Gradient-level parity of the device PPO step (csrc/ilsx_ppo.hip, the LOSS_MSE / LOSS_PPO_POLICY heads, the three weight-gradient paths behind
launch_bwd_dw, k_ppo_norm, k_ppo_update) against the float64 autograd restatement of tests/ppo_restatement.py.

Parameters after Adam say little about a gradient: the update is lr * m / (sqrt(v) + 1e-8), so a gradient that is wrong by a constant factor
(1/mini_batch_size for 1/rows on the ragged last minibatch, a lost 2 in the value loss) moves the parameters exactly as the right one does.  The
gradient is read from the Adam moments that get_snapshot() returns in the flat ABI layout (PPO's betas are fixed at 0.9 / 0.999):

  T1, frozen parameters: a trainer with both learning rates 0 never moves; after k minibatches exp_avg = sum_i 0.9^(k-i) * 0.1 * c_i * g_i and
      exp_avg_sq = sum_i 0.999^(k-i) * 0.001 * (c_i * g_i)^2 with g_i the gradient of minibatch i at the initial parameters; policy:
      c_i = min(1, 20 / (|g_i| + 1e-6)); value: c_i = 1 and g_i includes 2 * value_l2_reg * p.  The last (ragged) minibatch weighs most.
  T2, moved parameters: run A is one real step (one epoch, one minibatch), run B the same step and a second one; (m_B - 0.9 * m_A) / 0.1 is the
      device's gradient of the second step, whose ratios and values have left the clip windows.  The reference evaluates it at run A's parameters.

Bounds: exp_avg within 1e-4 of the largest reference entry (the figure of test_sac_steps_vs_oracle and test_bc_parity_hip.py), exp_avg_sq within
2e-4, both PER parameter block so that a small block cannot hide behind a large one; the norm clip_grad_norm_ saw within 10 x NORM_ORACLE_DEV.
What keeps them honest runs without a GPU: on every case the numpy fp32 oracle sits within 1e-5 (2e-5) per block of the restatement, its norm
within NORM_ORACLE_DEV; the T2 inputs keep every row away from the points where the two sides of a min / max / clamp differ; and the same checks
fail by far against deliberately wrong references."""
import ctypes as C
import functools

import numpy as np
import pytest

import ppo_restatement as R
from oracle import tanh_gaussian as otg
from oracle.ppo import PPOOracle

gpu = pytest.mark.gpu
GRAD_REL, SQ_REL = 1e-4, 2e-4
# the largest relative deviation of the fp32 oracle's policy-gradient norm from the float64 one, over every minibatch of every case: 2.18e-7
# measured (dw_big, first minibatch); test_restatement_agrees_with_the_oracle / test_clip_* assert that it holds.  The device gets ten times that,
# the ratio of the gradient's 1e-5 -> 1e-4.
NORM_ORACLE_DEV = 2.2e-7
NORM_REL = 10 * NORM_ORACLE_DEV


def _freeze(*arrays):
    for x in arrays:
        x.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = R.make_case(name)
    _freeze(case["pi0"], case["vf0"], case["perms"], *[v for t in case["trajs"] for v in t.values()])
    return R.ALL[name], case


@functools.lru_cache(maxsize=None)
def _frozen(name):
    """(case settings, inputs, fixed quantities, per-minibatch reference, expected state) of a T1 case, computed once and never written to"""
    c, case = _inputs(name)
    fx, ref = R.frozen_run_f64(c, case)
    return c, case, fx, ref, _expected(ref)


def _expected(ref):
    """the state a run over the minibatches `ref` (at unmoved parameters) leaves: Adam moments of both nets, last norm, step count"""
    pi_m, pi_v = R.adam_moments([r["coef"] * r["pi_grad"] for r in ref])
    vf_m, vf_v = R.adam_moments([r["vf_grad"] for r in ref])
    return dict(pi_m=pi_m, pi_v=pi_v, vf_m=vf_m, vf_v=vf_v, norm=ref[-1]["norm"], steps=len(ref))


def _block_check(what, got, ref, c, value, rel):
    """max|got - ref| <= rel * max|ref| on every block (an all-zero reference block therefore demands exact zeros)"""
    errs = R.block_errors(got, ref, c, value)
    print(what, " ".join(f"{nm}:{e:.2e}/{m:.2e}" for nm, e, m in errs))
    bad = [(nm, e, m) for nm, e, m in errs if not e <= rel * m]
    assert not bad, (what, rel, bad)


def _check_state(what, c, got, want, grad_rel, sq_rel, norm_rel):
    assert got["steps"] == (want["steps"], want["steps"]), (what, got["steps"], want["steps"])
    for k, value, rel in (("vf_m", True, grad_rel), ("pi_m", False, grad_rel), ("vf_v", True, sq_rel), ("pi_v", False, sq_rel)):
        _block_check(f"{what} {k}", got[k], want[k], c, value, rel)
    dev = abs(got["norm"] / want["norm"] - 1)
    print(f"{what} norm {got['norm']!r} vs {want['norm']!r}: off by {dev:.2e} (allowed {norm_rel:.1e})")
    assert dev <= norm_rel, (what, got["norm"], want["norm"])


# ------------------------------------------------------------------------------------------------ the two runners: fp32 oracle, device
def _oracle_run(c, case, epochs=None):
    kw = dict(R.hyper(c), update_epoch=epochs or c["epochs"])
    orc = PPOOracle(c["o"], c["a"], c["hidden"], case["pi0"], case["vf0"], **kw)
    res = orc.train_step(case["trajs"], list(case["perms"][:kw["update_epoch"]]))
    return dict(pi=orc.pi, vf=orc.vf, pi_m=orc.opt_pi.m, pi_v=orc.opt_pi.v, vf_m=orc.opt_vf.m, vf_v=orc.opt_vf.v, norm=float(res["pi_grad_norm"]),
                steps=(orc.opt_pi.t, orc.opt_vf.t), res=res)


def _trainer(ctx, c, case, epochs=None):
    from ilswiss_amd.networks import FlattenMlp
    from ilswiss_amd.ppo import PPO, ReparamMultivariateGaussianPolicy
    kw = dict(R.hyper(c), update_epoch=epochs or c["epochs"])
    pol = ReparamMultivariateGaussianPolicy(c["hidden"], c["o"], c["a"], conditioned_std=kw.pop("conditioned_std"), hidden_activation="tanh", ctx=ctx, seed=3)
    vf = FlattenMlp(c["hidden"], 1, c["o"], hidden_activation="tanh", ctx=ctx, seed=4)
    tr = PPO(pol, vf, max_samples=case["N"], **kw)
    tr.set_flat_params(case["pi0"], case["vf0"])
    return tr


def _device_run(ctx, c, case, epochs=None):
    from ilswiss_amd import _lib
    tr = _trainer(ctx, c, case, epochs)
    tr.train_step(case["trajs"], case["perms"][:tr.update_epoch])
    s, gn = tr.get_snapshot(), C.c_float()
    _lib.check(ctx.lib.ilsx_ppo_debug_grad_norm(tr.h, C.byref(gn)))
    po, vo = s["policy_optimizer"], s["vf_optimizer"]
    assert po["exp_avg"].size == case["pi0"].size and vo["exp_avg"].size == case["vf0"].size
    return dict(pi=s["policy"], vf=s["vf"], pi_m=po["exp_avg"], pi_v=po["exp_avg_sq"], vf_m=vo["exp_avg"], vf_v=vo["exp_avg_sq"], norm=float(gn.value),
                steps=(po["step"], vo["step"]))


# ------------------------------------------------------------------------------------------------ T1 without a GPU
def _assert_case_reaches_its_path(name, c, case, ref):
    lens, mbs = c["lens"], R.minibatches(c, case["perms"])
    assert min(lens) == 2 and sum(lens) == case["N"]
    assert all((np.sort(p) == np.arange(case["N"])).all() and (p != np.arange(case["N"])).any() for p in case["perms"])     # real shuffles
    if name not in ("one_hidden", "three_hidden"):
        assert 0 < len(mbs[-1]) < c["mb"] and len(mbs[-2]) == c["mb"]                      # a ragged minibatch after a full one
    if name == "one_row_tail":
        assert len(mbs[-1]) == 1
    if name in ("one_hidden", "three_hidden"):
        print(f"{name}: norm {ref[-1]['norm']:.1f}, clip coefficient {ref[-1]['coef']:.3f}")
        assert ref[-1]["norm"] >= 2 * R.MAX_NORM and ref[-1]["coef"] <= 0.5 and len(c["hidden"]) == (1 if name == "one_hidden" else 3)
    elif name != "wide":                                                                 # elsewhere the clip stays out of the way (wide: it happens to act)
        assert all(r["coef"] == 1.0 for r in ref)
    if name == "cond_std":
        lsr = np.concatenate([r["lsr"].ravel() for r in ref])
        above, below = float(np.mean(lsr > otg.LOG_SIG_MAX)), float(np.mean(lsr < otg.LOG_SIG_MIN))
        print(f"cond_std: raw log-std above +2: {above:.3f}, inside: {1 - above - below:.3f}, below -20: {below:.3f}")
        assert above >= 0.05 and 1 - above >= 0.05 and below == 0 and np.abs(lsr - otg.LOG_SIG_MAX).min() > 1e-4
    if name in ("row_split", "dw_big"):
        from ilswiss_amd import _lib
        big = name == "dw_big"
        lo, hi = (R.DW_BIG_MIN_ROWS, 1 << 30) if big else (R.DW_SPLIT_MIN_ROWS, R.DW_BIG_MIN_ROWS)
        assert lo <= len(mbs[0]) < min(hi, lo + 64) and len(mbs[1]) < R.DW_SPLIT_MIN_ROWS and max(c["hidden"]) <= 128
        s, rps = C.c_int(), C.c_int()
        assert _lib.load().ilsx_debug_dw_split(len(mbs[0]), int(big), C.byref(s), C.byref(rps)) == 0
        assert s.value > 1 and (len(mbs[0]) - (s.value - 1) * rps.value) % (32 if big else 128) != 0      # the last row range ends inside a row step


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_agrees_with_the_oracle(name):
    """Autograd in float64 and the oracle's hand-derived fp32 backward at unmoved parameters: every minibatch's value and policy gradient within 1e-5
    per block, the Adam moments the device test reads within 1e-5 / 2e-5, the norm within NORM_ORACLE_DEV; the case reaches the path it is named
    for; a zero learning rate leaves the oracle's parameters bitwise alone."""
    c, case, fx, ref, want = _frozen(name)
    _assert_case_reaches_its_path(name, c, case, ref)
    got = _oracle_run(c, case)
    res = got["res"]
    np.testing.assert_array_equal(got["pi"], case["pi0"])
    np.testing.assert_array_equal(got["vf"], case["vf0"])
    np.testing.assert_allclose(res["values"].ravel(), fx["values"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(res["advantages"].ravel(), fx["adv"], rtol=2e-4, atol=2e-5)
    worst = 0.0
    for i, r in enumerate(ref):
        _block_check(f"{name} minibatch {i} value", res["vf_grads"][i], r["vf_grad"], c, True, 1e-5)
        _block_check(f"{name} minibatch {i} policy", res["pi_grads"][i], r["pi_grad"], c, False, 1e-5)
        worst = max(worst, abs(res["pi_grad_norms"][i] / r["norm"] - 1))
    print(f"{name}: the oracle's norm deviates by at most {worst:.2e}")
    assert worst <= NORM_ORACLE_DEV
    _check_state(f"{name} oracle", c, got, want, GRAD_REL / 10, SQ_REL / 10, NORM_ORACLE_DEV)


# ------------------------------------------------------------------------------------------------ T2 without a GPU
def _second_step(c, case, pi1, vf1):
    """The reference of the second step at (pi1, vf1), after the branch conditions have been checked ON THE REFERENCE: every live branch holds at
    least 5% of the rows, and no row lies within the margin of a point where the two sides give different gradients — ratio at 1 +- clip_eps,
    v - v_old at +- clip_eps, l1 = l2 outside the value window.  Margin: 100 x the largest difference between the fp32 oracle's and the float64 value
    of that quantity at these parameters, at least 1e-4."""
    eps = float(np.float32(c["clip_eps"]))
    idx = case["perms"][1]
    assert c["mb"] >= case["N"] and c["epochs"] == 2
    fx = R.fixed_f64(c, case, case["pi0"], case["vf0"])
    r = R.minibatch_f64(c, fx, idx, pi1, vf1)
    # the same quantities as the fp32 oracle has them
    o0 = PPOOracle(c["o"], c["a"], c["hidden"], case["pi0"], case["vf0"], **R.hyper(c))
    obs, act, R0, _, V0 = o0.calc_adv(case["trajs"])
    lp0 = o0.log_prob(obs, act)[0]
    o1 = PPOOracle(c["o"], c["a"], c["hidden"], np.asarray(pi1, np.float32), np.asarray(vf1, np.float32), **R.hyper(c))
    ratio32 = np.exp(o1.log_prob(obs, act)[0] - lp0).ravel()[idx]
    v32 = o1.v(obs)[0]
    dv32 = (v32 - V0).ravel()[idx]
    vc32 = V0 + np.clip(v32 - V0, np.float32(-eps), np.float32(eps))
    dl32 = ((v32 - R0) ** 2 - (vc32 - R0) ** 2).ravel()[idx]
    A = fx["adv"][idx]
    ratio, dv, dl = r["ratio"], r["dv"], r["l1"] - r["l2"]
    frac = lambda m: float(np.mean(m))   # noqa: E731
    # policy
    m_ratio = max(1e-4, 100 * float(np.abs(ratio32 - ratio).max()))
    d_ratio = float(np.minimum(np.abs(ratio - (1 - eps)), np.abs(ratio - (1 + eps))).min())
    above, below = ratio > 1 + eps, ratio < 1 - eps
    shares = dict(inside=frac(~above & ~below), above=frac(above), below=frac(below), outside_pos=frac((above | below) & (A > 0)), outside_neg=frac((above | below) & (A < 0)),
                  live_above=frac(above & (A < 0)), live_below=frac(below & (A > 0)))
    print(f"policy: margin {m_ratio:.2e}, nearest row {d_ratio:.2e}; shares {shares}")
    assert d_ratio > m_ratio
    assert min(shares.values()) >= 0.05, shares      # live_*: outside the window on the side where min() keeps the unclipped term
    # value net
    m_dv = max(1e-4, 100 * float(np.abs(dv32 - dv).max()))
    d_dv = float(np.abs(np.abs(dv) - eps).min())
    out = np.abs(dv) > eps
    m_dl = max(1e-4, 100 * float(np.abs(dl32 - dl)[out].max()))
    d_dl = float(np.abs(dl[out]).min())
    vshares = dict(inside=frac(~out), clipped_unclipped_larger=frac(out & (dl > 0)), clipped_clipped_larger=frac(out & (dl < 0)))
    print(f"value: window margin {m_dv:.2e}, nearest row {d_dv:.2e}; l1 = l2 margin {m_dl:.2e}, nearest row {d_dl:.2e}; shares {vshares}")
    if c["vclip"]:
        assert d_dv > m_dv and d_dl > m_dl
        assert min(vshares.values()) >= 0.05, vshares
    return r


def _second_step_checks(what, c, a, b, r, grad_rel, sq_rel, norm_rel):
    """run A (one step) and run B (the same step, then a second one): the second step's gradient and its square by subtraction, per block"""
    assert a["steps"] == (1, 1) and b["steps"] == (2, 2)
    f64 = lambda x: np.asarray(x, np.float64)   # noqa: E731
    for net, value, g in (("vf", True, r["vf_grad"]), ("pi", False, r["coef"] * r["pi_grad"])):
        _block_check(f"{what} {net} gradient", (f64(b[net + "_m"]) - R.B1 * f64(a[net + "_m"])) / (1 - R.B1), g, c, value, grad_rel)
        _block_check(f"{what} {net} squared", (f64(b[net + "_v"]) - R.B2 * f64(a[net + "_v"])) / (1 - R.B2), g * g, c, value, sq_rel)
    dev = abs(b["norm"] / r["norm"] - 1)
    print(f"{what} norm {b['norm']!r} vs {r['norm']!r}: off by {dev:.2e} (allowed {norm_rel:.1e})")
    assert dev <= norm_rel


@pytest.mark.parametrize("name", list(R.CLIP_CASES))
def test_clip_inputs_are_sound_and_the_oracle_agrees(name):
    """T2 on the fp32 oracle: the reference alone satisfies the branch conditions with no row excluded (shares and margins printed), the first step
    moved both networks, the oracle's second gradient sits within 1e-5 per block of the restatement at the oracle's own moved parameters — read
    directly and by the subtraction the device test uses — and its norm within NORM_ORACLE_DEV."""
    c, case = _inputs(name)
    a, a2, b = _oracle_run(c, case, epochs=1), _oracle_run(c, case, epochs=1), _oracle_run(c, case, epochs=2)
    for k in ("pi", "vf", "pi_m", "pi_v", "vf_m", "vf_v"):
        np.testing.assert_array_equal(a[k], a2[k])
    assert np.abs(a["pi"] - case["pi0"]).max() > 1e-3 and np.abs(a["vf"] - case["vf0"]).max() > 1e-3
    r = _second_step(c, case, a["pi"], a["vf"])
    _block_check(f"{name} oracle value", b["res"]["vf_grads"][1], r["vf_grad"], c, True, 1e-5)
    _block_check(f"{name} oracle policy", b["res"]["pi_grads"][1], r["pi_grad"], c, False, 1e-5)
    _second_step_checks(f"{name} oracle", c, a, b, r, GRAD_REL / 10, SQ_REL / 10, NORM_ORACLE_DEV)
    # the windows matter: the same step without them is another gradient
    free = R.minibatch_f64(dict(c, clip_eps=10.0), R.fixed_f64(c, case, case["pi0"], case["vf0"]), case["perms"][1], a["pi"], a["vf"])
    assert max(e / m for _, e, m in R.block_errors(free["pi_grad"], r["pi_grad"], c)) > 0.05
    if c["vclip"]:
        assert max(e / m for _, e, m in R.block_errors(free["vf_grad"], r["vf_grad"], c, True)) > 0.05


# ------------------------------------------------------------------------------------------------ wrong references
def _worst(got, ref, c, value=False):
    return max(e / m for _, e, m in R.block_errors(got, ref, c, value) if m > 0)


@pytest.mark.parametrize("wrong,name", [("last_scale", "ragged"), ("last_scale", "row_split"), ("last_scale", "dw_big"), ("tie", "one_row_tail"), ("tie", "spec"),
                                        ("norm1", "three_hidden"), ("norm2", "three_hidden"), ("gate", "cond_std"), ("gate", "clip"), ("gate", "clip_vclip")])
def test_wrong_references_are_caught(wrong, name):
    """The fp32 oracle stands in for the device; against a deliberately wrong reference the device checks fail by far (worst per-block error of
    exp_avg, as a multiple of the largest reference entry; bound 1e-4):
      last_scale — the last minibatch's gradient scaled by rows / mini_batch_size;
      tie        — ties of min / max without torch's weight of 1/2 (at unmoved parameters every ratio is exactly 1 and, with the value clip, every
                   v = v_old: all rows tie);
      norm1 / 2  — the first / second hidden -> hidden matrix counted twice in the norm (shows in the norm and, the clip being active, in the clipped gradient);
      gate       — the clamps' derivative taken as 1 outside their windows."""
    c, case = _inputs(name)
    if name in R.CASES:
        got = _oracle_run(c, case)
        want = _expected(R.frozen_run_f64(c, case, wrong=wrong)[1])
        pi_err, vf_err = _worst(got["pi_m"], want["pi_m"], c), _worst(got["vf_m"], want["vf_m"], c, True)
        norm_err = abs(got["norm"] / want["norm"] - 1)
    else:
        a, b = _oracle_run(c, case, epochs=1), _oracle_run(c, case, epochs=2)
        r = R.minibatch_f64(c, R.fixed_f64(c, case, case["pi0"], case["vf0"]), case["perms"][1], a["pi"], a["vf"], wrong=wrong)
        pi_err = _worst((b["pi_m"].astype(np.float64) - R.B1 * a["pi_m"]) / (1 - R.B1), r["coef"] * r["pi_grad"], c)
        vf_err = _worst((b["vf_m"].astype(np.float64) - R.B1 * a["vf_m"]) / (1 - R.B1), r["vf_grad"], c, True)
        norm_err = abs(b["norm"] / r["norm"] - 1)
    print(f"wrong reference {wrong} on {name}: policy exp_avg off by {pi_err:.2e}, value exp_avg by {vf_err:.2e}, norm by {norm_err:.2e}")
    assert pi_err > 100 * GRAD_REL
    if wrong == "last_scale" or (wrong in ("tie", "gate") and c["vclip"]):
        assert vf_err > 100 * GRAD_REL
    if wrong in ("last_scale", "norm1", "norm2", "tie"):
        assert norm_err > 100 * NORM_REL


# ------------------------------------------------------------------------------------------------ the device step
@gpu
@pytest.mark.parametrize("name", list(R.CASES))
def test_hip_ppo_frozen_gradients_vs_float64(ctx, name):
    """T1 on the device: both Adam moments of both networks per parameter block, the step counts, the norm of the last minibatch, and both
    parameter vectors bitwise unchanged (ilsx_ppo_create accepts a zero learning rate).  Norm: the fp32 oracle deviates from float64 by at most
    2.18e-7 on these cases (measured without a GPU, NORM_ORACLE_DEV), the device is allowed ten times that, 2.2e-6."""
    c, case, _, ref, want = _frozen(name)
    _assert_case_reaches_its_path(name, c, case, ref)
    got = _device_run(ctx, c, case)
    np.testing.assert_array_equal(got["pi"], case["pi0"])
    np.testing.assert_array_equal(got["vf"], case["vf0"])
    _check_state(name, c, got, want, GRAD_REL, SQ_REL, NORM_REL)


@gpu
@pytest.mark.parametrize("name", list(R.CLIP_CASES))
def test_hip_ppo_second_step_vs_float64(ctx, name):
    """T2 on the device: one real step is reproducible bit for bit, and the gradient of the step after it — clipped-surrogate derivative and value
    clip with their live branches — by subtraction, against float64 at the device's own moved parameters, where the branch conditions are
    asserted again.  Norm bound as in the frozen test: 10 x the oracle's measured 2.18e-7."""
    c, case = _inputs(name)
    a, a2, b = _device_run(ctx, c, case, epochs=1), _device_run(ctx, c, case, epochs=1), _device_run(ctx, c, case, epochs=2)
    for k in ("pi", "vf", "pi_m", "pi_v", "vf_m", "vf_v"):
        np.testing.assert_array_equal(a[k], a2[k], err_msg=k)
    assert np.abs(a["pi"] - case["pi0"]).max() > 1e-3 and np.abs(a["vf"] - case["vf0"]).max() > 1e-3
    r = _second_step(c, case, a["pi"], a["vf"])
    _second_step_checks(name, c, a, b, r, GRAD_REL, SQ_REL, NORM_REL)


@gpu
@pytest.mark.parametrize("name", ["cond_std", "wide"])
def test_hip_calc_adv_vs_float64(ctx, name):
    """values, returns, standardised advantages and fixed log-probs against float64, at the figures of test_hip_gae_and_fixed_log_probs_golden"""
    c, case, fx, _, _ = _frozen(name)
    R_, A, V, lp = _trainer(ctx, c, case).calc_adv(case["trajs"])
    np.testing.assert_allclose(V.ravel(), fx["values"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(R_.ravel(), fx["returns"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(A.ravel(), fx["adv"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(lp.ravel(), fx["lp_old"], rtol=1e-5, atol=1e-5)
