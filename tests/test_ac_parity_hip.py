"""Gradient-level parity of the TD3, HER-TD3 and SAC-V steps (csrc/ilsx_ac.hip on the AcAgent frame: ac_fwd / ac_bwd / ac_dw_adam, the
LOSS_TD_CRITIC / LOSS_TD3_POLICY / LOSS_SACV_VALUE / LOSS_SAC_ACTORQ / LOSS_SAC_POLICY heads, the HER side kernels, the three weight-gradient
paths behind launch_bwd_dw with Adam and the Polyak write in their epilogues) against the float64 autograd restatement of
tests/ac_restatement.py.

Parameters after Adam say little about a gradient: the update is lr * m / (sqrt(v) + 1e-8), so a gradient that is wrong by a constant factor
(1/max_batch for 1/B, a lost 2 in TD3's critic, max_act, HER's 1/(B A)) moves the parameters exactly as the right one does, and one that is
wrong in a few entries moves them by about lr.  The gradient is read from the Adam moments that get_snapshot() returns in the flat ABI layout:

  T1, first step from zero moments: a fresh trainer, EVERY block set with set_flat_params — the target blocks to independent draws, so that a
      task that reads the online net for a target is as wrong as a wrong net — one train_step with explicit noise at real learning rates.
      Then exp_avg = (1 - beta_1) g and exp_avg_sq = 0.001 g^2 (beta_1 = 0.9; SAC-V also at beta_1 = 0, where exp_avg is g).
  T3, the actor sees the updated critics: in T1 the reference's policy loss is evaluated with the critics the RUN reports after its step
      (get_flat_params), on every case; that this discriminates is asserted without a GPU: with the critics before the step the policy
      gradient is off by at least ten times the bound.  After the step the targets are tau * new + (1 - tau) * old.
  T2, frozen: all learning rates and tau 0, three steps at B = 96, 37, 64 under max_batch = 128.  Parameters and targets stay bitwise, the
      moments are the geometric sums of the three reference gradients (the last step weighs most), the step counts are 3: nothing of step i
      reaches step i + 1 through the reused workspaces and partial slabs.
  T4, TD3's delay (period 2, three steps): a step without a policy update leaves the policy's moments, its step count, the policy and all
      three targets bitwise alone, the critics' optimiser counts 2 — with and without a statistics request on that step (which makes the actor
      forward run anyway); on an update step the whole state is bitwise the same with and without the request.

Bounds: exp_avg within 1e-4 of the largest reference entry (the figure of test_sac_steps_vs_oracle, test_bc_parity_hip.py and
test_ppo_parity_hip.py), exp_avg_sq within 2e-4, both PER parameter block, so that a small block cannot hide behind a large one; an all-zero
reference block demands exact zeros.  What keeps them honest runs without a GPU: on every case the numpy fp32 oracles (oracle/td3.py with her=
for HER-TD3, oracle/sac_v.py) sit within 1e-5 / 2e-5 per block of the restatement — measured worst over all cases: 2.7e-6 (her/wide q1) — so no
case needed a bound of its own; the inputs keep every row away from the points where an fp32 evaluation could take another branch than the
float64 one (ac_restatement.violations); and the same `_check` fails by at least ten times the bound against ten deliberately wrong references."""
import ctypes as C

import numpy as np
import pytest

import ac_restatement as R
from oracle import tanh_gaussian as otg

gpu = pytest.mark.gpu
GRAD_REL, SQ_REL = 1e-4, 2e-4
OPT_KEY = dict(q1="qf1_optimizer", q2="qf2_optimizer", vf="vf_optimizer", pi="policy_optimizer")
ONE_STEP, THREE_STEPS, DELAYED = list(R.CASES), list(R.FROZEN), list(R.DELAY)


def _block_check(what, got, ref, c, net, rel):
    """max|got - ref| <= rel * max|ref| on every block (an all-zero reference block therefore demands exact zeros)"""
    errs = R.block_errors(got, ref, c, net)
    print(what, " ".join(f"{nm}:{e:.2e}/{m:.2e}" for nm, e, m in errs))
    bad = [(nm, e, m) for nm, e, m in errs if not e <= rel * m]
    assert not bad, (what, rel, bad)


def _references(c, case, got, wrong=None):
    """the float64 step of every batch of a run; a one-step run's actor phase sees the critics the run itself reports after the step (T3)"""
    one = len(case["batches"]) == 1
    actor = {k: got["P"][k] for k in R.CRITICS[c["algo"]]} if one else None
    assert one or c["lr"] == 0.0
    return [R.step_f64(c, case["P"], b, actor=actor, wrong=wrong) for b in case["batches"]]


def _check(what, c, case, got, grad_rel, sq_rel, wrong=None):
    """A run's Adam state against the float64 reference: both moments of every trainable net per parameter block, the step counts.  `got`:
    dict(P = every block after the run, m / v / steps per trainable net).  Returns the references (one per step)."""
    refs = _references(c, case, got, wrong)
    for net in R.NETS[c["algo"]]:
        assert got["steps"][net] == len(refs), (what, net, got["steps"][net])
        m, v = R.adam_moments([r["grads"][net] for r in refs], c["beta_1"])
        _block_check(f"{what} {net} exp_avg", got["m"][net], m, c, net, grad_rel)
        _block_check(f"{what} {net} exp_avg_sq", got["v"][net], v, c, net, sq_rel)
    return refs


def _assert_inputs(name, c, case, refs):
    """Conditions on the INPUTS, evaluated on the float64 reference: no row breaks a kink condition (ac_restatement.violations: |Q1 - Q2|
    at the pre- and post-update critics, the clip_return and noise bounds, the log-std clamp), and the regimes a case is about are populated."""
    shape, a = c["shape"], c["a"]
    for batch, ref in zip(case["batches"], refs):
        rows, B = ref["rows"], batch["observations"].shape[0]
        assert not R.violations(c, ref).any(), (name, np.nonzero(R.violations(c, ref))[0])
        frac = lambda m: float(np.mean(m))   # noqa: E731
        if B > 1:
            assert 0.05 <= frac(batch["terminals"]) <= 0.5                                   # terminals mixed
        if c["algo"] == "sacv":
            above, below = frac(rows["lsr"] > otg.LOG_SIG_MAX), frac(rows["lsr"] < otg.LOG_SIG_MIN)
            print(f"{name}: raw log-std above +2: {above:.3f}, inside: {1 - above - below:.3f}, below -20: {below:.3f}; max |Q| {ref['max_q']:.2f}")
            assert below == 0 and (above >= 0.05 and 1 - above >= 0.05 if B > 1 else 0 < above < 1)
            assert c["alpha"] == 0.2 and c["reward_scale"] == 5.0 and c["w_mu"] != c["w_std"] and min(c["w_mu"], c["w_std"]) > 0
            continue
        assert c["reward_scale"] == 5.0 and c["max_act"] != 1.0
        bound = R.f32(c["max_act"] if c["algo"] == "her" else c["noise_clip"])
        hi, lo = (rows["noise"] > bound).any(1), (rows["noise"] < -bound).any(1)
        shares = dict(high=frac(hi), low=frac(lo), none=frac(~hi & ~lo))
        if c["algo"] == "her":
            cl, cr = rows["tq_raw"] < R.f32(c["clip_l"]), rows["tq_raw"] > R.f32(c["clip_r"])
            clip = dict(left=frac(cl), right=frac(cr), neither=frac(~cl & ~cr))
            print(f"{name}: sigma * eps past max_act: {shares}; clip_return [{c['clip_l']:.4f}, {c['clip_r']:.4f}]: {clip}; max |Q| {ref['max_q']:.2f}")
            assert shares["none"] < 1 and (a > 1 or shape == "pendulum")
            assert min(clip.values()) >= 0.1 if B > 1 else clip["left"] == 1
        else:
            print(f"{name}: rows whose noise the clip binds: {shares}; max |Q| {ref['max_q']:.2f}")
            if B > 1:                      # a = 17: a row with no bound entry is rare (0.79^17), one of them is what there is
                assert min(shares.values()) >= (0.05 if a <= 6 else 1.0 / B), shares


# ------------------------------------------------------------------------------------------------ the two runners: fp32 oracle, device
def _oracle_run(c, case):
    orc = R.make_oracle(c, case["P"])
    res = [R.oracle_step(orc, b) for b in case["batches"]]
    opt = dict(q1=orc.opt_q1, q2=orc.opt_q2, pi=orc.opt_pi) if c["algo"] != "sacv" else orc.opt
    nets = R.NETS[c["algo"]]
    return dict(P={k: getattr(orc, k).copy() for k in nets + R.TARGETS[c["algo"]]}, m={k: opt[k].m for k in nets}, v={k: opt[k].v for k in nets},
                steps={k: opt[k].t for k in nets}, res=res)


def _trainer(ctx, c, case):
    """a fresh device trainer of the case with EVERY block, targets included, set from the case; no statistics are requested until a test asks"""
    from ilswiss_amd import her
    from ilswiss_amd.networks import FlattenMlp, ReparamTanhMultivariateGaussianPolicy
    from ilswiss_amd.sac_v import SoftActorCriticV
    from ilswiss_amd.td3 import TD3, MlpGaussianNoisePolicy
    o, a, hid, algo = c["o"], c["a"], c["hidden"], c["algo"]
    net = dict(hidden_activation=c["act"], ctx=ctx)
    q1, q2 = FlattenMlp(hid, 1, o + a, seed=2, **net), FlattenMlp(hid, 1, o + a, seed=3, **net)
    kw = R.hyper(c)
    kw.pop("hidden_activation")
    if algo == "sacv":
        pol, vf = ReparamTanhMultivariateGaussianPolicy(hid, o, a, seed=1, **net), FlattenMlp(hid, 1, o, seed=4, **net)
        tr = SoftActorCriticV(pol, q1, q2, vf, max_batch=c["max_batch"], **kw)
    else:
        for k in ("policy_noise", "policy_noise_clip", "max_act", "output_activation", "her"):
            kw.pop(k, None)
        if algo == "td3":
            pol = MlpGaussianNoisePolicy(hid, o, a, policy_noise=c["sigma"], policy_noise_clip=c["noise_clip"], max_act=c["max_act"],
                                         output_activation=c["out_act"], seed=1, **net)
            tr = TD3(pol, q1, q2, max_batch=c["max_batch"], **kw)
        else:
            pol = her.MlpGaussianAndEpsilonPolicy(hid, o - c["gd"], a, condition_dim=c["gd"], max_sigma=c["sigma"], min_sigma=c["sigma"],
                                                  max_act=c["max_act"], min_act=-c["max_act"], output_activation=c["out_act"], seed=1, **net)
            tr = her.TD3(pol, q1, q2, max_batch=c["max_batch"], **kw)
    for k in R.NETS[algo] + R.TARGETS[algo]:
        tr.set_flat_params(k, case["P"][k])
        np.testing.assert_array_equal(tr.get_flat_params(k), case["P"][k])
    tr.eval_statistics = {}
    return tr


def _device_step(tr, c, batch, stats=False):
    b = {k: v for k, v in batch.items() if k != "eps"}
    if c["algo"] == "her":          # her.TD3 concatenates observation | desired_goal itself
        n = c["o"] - c["gd"]
        b.update(observations=batch["observations"][:, :n], desired_goals=batch["observations"][:, n:],
                 next_observations=batch["next_observations"][:, :n], next_desired_goals=batch["next_observations"][:, n:])
    tr.eval_statistics = None if stats else {}
    tr.train_step(b, batch["eps"])
    if stats:
        assert np.isfinite(tr.get_eval_statistics()["Policy Loss"])


def _device_state(tr, c):
    nets, snap = R.NETS[c["algo"]], tr.get_snapshot()
    opt = {k: snap[OPT_KEY[k]] for k in nets}
    return dict(P={k: tr.get_flat_params(k) for k in nets + R.TARGETS[c["algo"]]}, m={k: opt[k]["exp_avg"] for k in nets},
                v={k: opt[k]["exp_avg_sq"] for k in nets}, steps={k: opt[k]["step"] for k in nets})


def _device_run(ctx, c, case):
    tr = _trainer(ctx, c, case)
    for b in case["batches"]:
        _device_step(tr, c, b)
    return _device_state(tr, c)


def _assert_targets(what, c, case, got):
    """after one step every target the step updates is tau * new + (1 - tau) * old, with `new` read from the run itself"""
    tau = R.f32(c["tau"])
    for t in R.TARGETS[c["algo"]]:
        new, old = got["P"][R.ONLINE_OF[t]].astype(np.float64), case["P"][t].astype(np.float64)
        err = np.abs(got["P"][t] - (tau * new + (1 - tau) * old)).max()
        print(f"{what} {t}: Polyak off by {err:.2e}")
        assert err <= 2e-7 * max(1.0, np.abs(old).max()), (what, t, err)
        assert np.abs(new - case["P"][R.ONLINE_OF[t]]).max() > 1e-4          # ... and the online net did move


def _assert_unmoved(what, c, case, got):
    for k in R.NETS[c["algo"]] + R.TARGETS[c["algo"]]:
        np.testing.assert_array_equal(got["P"][k], case["P"][k], err_msg=f"{what} {k}")


# ------------------------------------------------------------------------------------------------ without a GPU
@pytest.mark.parametrize("name", ONE_STEP)
def test_restatement_agrees_with_the_oracle(name):
    """T1 / T3 on the fp32 oracle: every gradient the oracle reports within 1e-5 per block of autograd in float64, the Adam moments the
    device test reads within 1e-5 / 2e-5, the targets' Polyak step, the kink conditions and regime shares of the inputs — and the case
    discriminates: with the critics BEFORE their update the policy gradient misses by at least ten times the device's bound."""
    c, case = R.make_case(name)
    got = _oracle_run(c, case)
    refs = _check(f"{name} oracle", c, case, got, GRAD_REL / 10, SQ_REL / 10)
    _assert_inputs(name, c, case, refs)
    for net in R.NETS[c["algo"]]:
        _block_check(f"{name} oracle {net} gradient", got["res"][0][net + "_grad"], refs[0]["grads"][net], c, net, 1e-5)
    _assert_targets(f"{name} oracle", c, case, got)
    pre = R.step_f64(c, case["P"], case["batches"][0], actor=None)["grads"]["pi"]
    off = max(e / m for _, e, m in R.block_errors(got["res"][0]["pi_grad"], pre, c, "pi") if m > 0)
    print(f"{name}: against the pre-update critics the policy gradient is off by {off:.2e} of a block's largest entry")
    assert off > 10 * GRAD_REL


@pytest.mark.parametrize("name", THREE_STEPS)
def test_frozen_run_agrees_with_the_oracle(name):
    """T2 on the fp32 oracle: zero learning rates and tau leave every block bitwise alone, and the moments after B = 96, 37, 64 are the
    geometric sums of the three float64 gradients within 1e-5 / 2e-5 per block."""
    c, case = R.make_case(name)
    assert [b["observations"].shape[0] for b in case["batches"]] == [96, 37, 64] and c["max_batch"] == 128 and c["lr"] == 0 and c["tau"] == 0
    got = _oracle_run(c, case)
    _assert_unmoved(f"{name} oracle", c, case, got)
    _assert_inputs(name, c, case, _check(f"{name} oracle", c, case, got, GRAD_REL / 10, SQ_REL / 10))
    m_last = R.adam_moments([R.step_f64(c, case["P"], case["batches"][-1])["grads"]["q1"]], c["beta_1"])[0]
    assert max(e / m for _, e, m in R.block_errors(got["m"]["q1"], m_last, c, "q1")) > 100 * GRAD_REL       # the earlier steps do weigh


@pytest.mark.parametrize("name", DELAYED)
def test_delay_inputs_are_sound(name):
    c, case = R.make_case(name)
    assert c["period"] == 2 and len(case["batches"]) == 3
    _assert_inputs(name, c, case, [R.step_f64(c, case["P"], b) for b in case["batches"]])


def test_large_batches_land_on_the_intended_weight_gradient_plans():
    """launch_bwd_dw changes kernel at DW_SPLIT_MIN_ROWS and DW_BIG_MIN_ROWS rows (read from kernels.h): dw_1024 and dw_4096 sit exactly on
    the two thresholds, dw_1100 between them with a last row range that ends inside a 128-row step; every other case stays below."""
    from ilswiss_amd import _lib
    lib, plans = _lib.load(), {}
    for shape, big in (("dw_1024", 0), ("dw_1100", 0), ("dw_4096", 1)):
        rows = R.SHAPES[shape][5][0]
        assert rows == R.SHAPES[shape][4] and (rows >= R.DW_BIG_MIN_ROWS) == bool(big) and rows >= R.DW_SPLIT_MIN_ROWS
        s, rps = C.c_int(), C.c_int()
        assert lib.ilsx_debug_dw_split(rows, big, C.byref(s), C.byref(rps)) == 0
        plans[shape] = (s.value, rps.value)
        assert s.value > 1 and (s.value - 1) * rps.value < rows <= s.value * rps.value
    print("row-split plans (ranges, rows per range):", plans)
    assert R.SHAPES["dw_1024"][5][0] == R.DW_SPLIT_MIN_ROWS and R.SHAPES["dw_4096"][5][0] == R.DW_BIG_MIN_ROWS
    assert (1100 - (plans["dw_1100"][0] - 1) * plans["dw_1100"][1]) % 128 != 0
    assert all(max(v[5]) < R.DW_SPLIT_MIN_ROWS for k, v in {**R.SHAPES, **R.FROZEN_SHAPES, **R.DELAY_SHAPES}.items() if not k.startswith("dw_"))


WRONG_CASES = [("inv_b", "td3/h128_part"), ("inv_b", "her/h256_part"), ("inv_b", "sacv/h128_part"), ("td3_half", "td3/h64"), ("td3_half", "her/h64"),
               ("sacv_double", "sacv/h64"), ("no_max_act", "td3/h64"), ("no_max_act", "td3/one_hidden"), ("online_targets", "td3/h64"),
               ("online_targets", "her/h128_full"), ("online_targets", "sacv/h256_full"), ("l2_over_b", "her/h64"), ("l2_over_b", "her/wide"),
               ("unclipped", "her/h64"), ("unclipped", "her/one_row"), ("v_post", "sacv/h64"), ("pi_pre", "td3/dw_1024"), ("pi_pre", "her/pendulum"),
               ("pi_pre", "sacv/dw_4096"), ("swap_reg", "sacv/h64"), ("swap_reg", "sacv/wide")]


@pytest.mark.parametrize("wrong,name", WRONG_CASES)
def test_wrong_references_are_caught(wrong, name):
    """The fp32 oracle stands in for the device.  The same `_check` the GPU tests use, at TEN times their bounds, rejects each of:
      inv_b          — 1/max_batch for 1/B;
      td3_half       — TD3's critic loss with a 1/2 (the factor 2 lost);   sacv_double — SAC-V's critic loss without its 1/2;
      no_max_act     — max_act dropped from the derivative of TD3's policy loss;
      online_targets — the online nets read where the targets belong;
      l2_over_b      — HER's mean(pi(s)^2) taken over B instead of B * A;   unclipped — HER's target left unclipped;
      v_post         — V trained against the critics after their update;    pi_pre — the policy against the critics before it;
      swap_reg       — the mean and the std regulariser weights swapped."""
    c, case = R.make_case(name)
    got = _oracle_run(c, case)
    _check(f"{name} oracle", c, case, got, GRAD_REL / 10, SQ_REL / 10)
    with pytest.raises(AssertionError) as failure:
        _check(f"{name} against {wrong}", c, case, got, 10 * GRAD_REL, 10 * SQ_REL, wrong=wrong)
    print("rejected:", str(failure.value)[:300])


# ------------------------------------------------------------------------------------------------ the device step
@gpu
@pytest.mark.parametrize("name", ONE_STEP)
def test_hip_first_step_gradients_vs_float64(ctx, name):
    """T1 and T3 on the device: one step from zero moments with every block set, the actor phase of the reference evaluated with the critics
    the device reports after the step (the kink conditions are asserted again on that reference); the targets' Polyak step, for SAC-V the one
    that rides in the weight-gradient launch's epilogue (k_dw_reduce on the row-split plans)."""
    c, case = R.make_case(name)
    got = _device_run(ctx, c, case)
    _assert_inputs(name, c, case, _check(name, c, case, got, GRAD_REL, SQ_REL))
    _assert_targets(name, c, case, got)


@gpu
@pytest.mark.parametrize("name", THREE_STEPS)
def test_hip_frozen_three_steps_vs_float64(ctx, name):
    """T2 on the device: B = 96, then 37, then 64 under max_batch = 128 with nothing moving."""
    c, case = R.make_case(name)
    got = _device_run(ctx, c, case)
    _assert_unmoved(name, c, case, got)
    _check(name, c, case, got, GRAD_REL, SQ_REL)


def _same(what, x, y):
    for k in x["P"]:
        np.testing.assert_array_equal(x["P"][k], y["P"][k], err_msg=f"{what} {k}")
    for k in x["m"]:
        np.testing.assert_array_equal(x["m"][k], y["m"][k], err_msg=f"{what} exp_avg {k}")
        np.testing.assert_array_equal(x["v"][k], y["v"][k], err_msg=f"{what} exp_avg_sq {k}")
    assert x["steps"] == y["steps"], (what, x["steps"], y["steps"])


@gpu
@pytest.mark.parametrize("name", DELAYED)
def test_hip_td3_delay_leaves_policy_and_targets_alone(ctx, name):
    """T4: three runs of three steps that differ only in the steps on which statistics are requested (none; step 1, which has no policy
    update; steps 0 and 2, which have one)."""
    c, case = R.make_case(name)
    runs = []
    for stats_on in ((), (1,), (0, 2)):
        tr, states = _trainer(ctx, c, case), []
        for i, b in enumerate(case["batches"]):
            _device_step(tr, c, b, stats=i in stats_on)
            states.append(_device_state(tr, c))
        s0, s1, s2 = states
        for k in ("pi",) + R.TARGETS[c["algo"]]:
            np.testing.assert_array_equal(s1["P"][k], s0["P"][k], err_msg=f"{name} {stats_on} {k}")
            assert np.abs(s0["P"][k] - case["P"][k]).max() > 0 and np.abs(s2["P"][k] - s1["P"][k]).max() > 0
        np.testing.assert_array_equal(s1["m"]["pi"], s0["m"]["pi"])
        np.testing.assert_array_equal(s1["v"]["pi"], s0["v"]["pi"])
        assert np.abs(s2["m"]["pi"] - s1["m"]["pi"]).max() > 0
        assert [s["steps"] for s in states] == [dict(q1=i, q2=i, pi=p) for i, p in ((1, 1), (2, 1), (3, 2))], (name, stats_on, [s["steps"] for s in states])
        runs.append(states)
    for other, what in ((runs[1], "statistics on the step without an update"), (runs[2], "statistics on the update steps")):
        for i in range(3):
            _same(f"{name} step {i}: {what}", runs[0][i], other[i])
