"""Gradient-level parity of the three discrete-action steps — discrete SAC (csrc/dsac.h: k_dsac_critic_grad, k_dsac_policy_grad; dsac_step in
ilsx_ac.hip), DQN / Double DQN (csrc/dqn.h: k_dqn_grad; dqn_step) and GCSL's BatchNorm categorical CLASS step (csrc/gcsl.h, ilsx_gcsl.hip) —
against the float64 autograd restatements of tests/discrete_restatement.py and gcsl_restatement.CatRestatement.

Parameters after Adam say little about a gradient: the update is lr * m / (sqrt(v) + 1e-8), so a gradient that is wrong by a constant factor moves
the parameters exactly as the right one does.  The gradient is read from the Adam moments (get_snapshot(); bncat: policy.get_snapshot()):

  T1, first step from zero moments: a fresh trainer, EVERY block set with set_flat_params — the targets to independent draws, reward_scale 5,
      alpha 0.2, discount 0.97, tau 0.01 — one train_step at real learning rates.  Then exp_avg = (1 - beta_1) g and exp_avg_sq = 0.001 g^2.
      The head rows of classes no row took hold exact zeros.  The step's statistics (losses at rtol 1e-4, Accuracy exactly) ride along.
  T3, dsac's policy sees the updated critics: the reference's policy loss is evaluated with the critics the RUN reports after its step; after
      the step every target is tau * new + (1 - tau) * old.
  T2, frozen: all learning rates and tau 0, three steps at B = 96, 37, 64 under max_batch = 128: parameters and targets stay bitwise, the
      moments are the geometric sums of the three reference gradients, the step counts are 3.
  GCSL: the live entries per block (the nblk * H Linear biases under a BatchNorm are left out: the mask is dead_bias_mask() exactly), the
      running mean and variance after the one step at rtol 1e-4 / atol 1e-5.

Bounds: exp_avg within 1e-4 of the largest reference entry, exp_avg_sq within 2e-4, both PER parameter block.  What keeps them honest runs
without a GPU: on every case the fp32 witness (dsac_restatement.DsacRestatement; dqn_restatement in float32; for GCSL the device text compiled
for the host, tests/harness/gcsl_bn_host.cpp) sits within a tenth of those bounds of the float64 restatement; DQN's inputs keep every row's
arg-max 1e-3 * max|Q| clear of the runner-up and GCSL's every row's top two probabilities 1e-5 apart (no row is dropped); dsac needs no such
condition: min(Q1, Q2) is continuous and carries no gradient in either loss.  The same `_check` fails by at least ten times the bound against
every wrong reference of WRONG_CASES / GCSL_WRONG_CASES.

Measured on the CPU, worst over all cases, as a share of the block's largest reference entry (the bounds asserted there are 1e-5 / 2e-5):
  dsac  DsacRestatement in fp32 vs float64:    exp_avg 1.4e-6, exp_avg_sq 1.7e-6 (both dsac/wide_ragged)
  DQN   dqn_restatement in float32 vs float64: exp_avg 1.8e-6, exp_avg_sq 1.5e-5 (both dqn/wide_ragged)
  GCSL  host emulation vs float64:             exp_avg 1.3e-6, exp_avg_sq 1.4e-5 (both two_column_batches)
so no case needed a bound of its own; 1.3e-5 of the two larger exp_avg_sq figures is the fp32 rounding of 1 - 0.999.  Every wrong reference
runs on EVERY one-step case of its algorithm (5 dsac, 7 DQN, 4 GCSL) but for the identities `_identity` names and asserts.  Smallest miss
factor per wrong reference over those cases (the worst block's error of exp_avg over the GPU bound of 1e-4; the tests assert at least 10):
  dsac  online_targets 8.1e2 (max_heads), target_pi_s 5.5e2 (max_heads), no_target_entropy 1.0e3 (generic), no_reward_scale 8.1e3 (one_row),
        no_done 1.6e3 (generic), inv_b 7.3e3 (wide_ragged), no_half 5.0e3, shift_action 1.7e4 (wide_ragged), pi_pre 8.6e3 (max_heads),
        pi_q1 8.2e2 (spec), no_policy_entropy 1.9e2 (one_row)
  DQN   online_targets 2.9e3 (max_heads), swap_double 2.8e3 (spec), half 1.0e4, inv_b 7.3e3 (wide_ragged), no_done 5.6e3 (generic_plain),
        no_discount 2.2e2 (max_heads_double)
  GCSL  bn_const 4.4e3 (one_block), running_fwd 1.9e4 (one_block), no_inv_b 9.7e3 (one_block), label_shift 1.5e4 (two_column_batches),
        bo_mean 3.6e5 (one_block)"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import discrete_restatement as R  # noqa: E402
import gcsl_restatement as GR  # noqa: E402
from test_gcsl_cpu import hostlib  # noqa: E402,F401  (the fixture that builds the host emulation of csrc/gcsl.h)

gpu = pytest.mark.gpu
GRAD_REL, SQ_REL, STAT_RTOL = 1e-4, 2e-4, 1e-4
ONE_STEP, THREE_STEPS, GCSL = list(R.CASES), list(R.FROZEN), list(R.GCSL_CASES)
STAT_KEYS = dict(dsac=(("QF1 Loss", "QF2 Loss", "Policy Loss"), ("Q1 Predictions", "Q2 Predictions")), dqn=(("QF Loss",), ("Y Predictions",)))


# ------------------------------------------------------------------------------------------------ dsac and DQN: the shared checks
def _block_check(what, errs, rel, report=None):
    """max|got - ref| <= rel * max|ref| on every block (an all-zero reference block therefore demands exact zeros)"""
    print(what, " ".join(f"{nm}:{e:.2e}/{m:.2e}" for nm, e, m in errs))
    if report is not None:      # the worst block's error as a share of its largest reference entry
        report.append(max(e / m if m > 0 else (0.0 if e == 0 else np.inf) for _, e, m in errs))
    bad = [(nm, e, m) for nm, e, m in errs if not e <= rel * m]
    assert not bad, (what, rel, bad)


def _references(c, case, got, wrong=None):
    """the float64 step of every batch of a run; a one-step dsac run's policy loss sees the critics the run itself reports after the step (T3)"""
    one = len(case["batches"]) == 1
    actor = {k: got["P"][k] for k in ("q1", "q2")} if one and c["algo"] == "dsac" else None
    assert one or c["lr"] == 0.0
    return [R.step_f64(c, case["P"], b, actor=actor, wrong=wrong) for b in case["batches"]]


def _check(what, c, case, got, grad_rel, sq_rel, wrong=None, report=None):
    """A run's Adam state against the float64 reference: both moments of every trainable net per parameter block, the step counts.  `got`:
    dict(P = every block after the run, m / v / steps per trainable net).  Returns the references (one per step)."""
    refs = _references(c, case, got, wrong)
    for net in R.NETS[c["algo"]]:
        assert got["steps"][net] == len(refs), (what, net, got["steps"][net])
        m, v = R.adam_moments([r["grads"][net] for r in refs], c["beta_1"])
        _block_check(f"{what} {net} exp_avg", R.block_errors(got["m"][net], m, c), grad_rel, None if report is None else report[0])
        _block_check(f"{what} {net} exp_avg_sq", R.block_errors(got["v"][net], v, c), sq_rel, None if report is None else report[1])
    return refs


def _worst(c, case, got, wrong=None):
    """the largest error of (exp_avg, exp_avg_sq) over all nets and blocks, as a share of the block's largest reference entry"""
    report = ([], [])
    _check("measure", c, case, got, np.inf, np.inf, wrong=wrong, report=report)
    return max(report[0]), max(report[1])


def _assert_untaken_zero(what, c, case, got, refs):
    """the head rows of the classes no row took: the reference's gradient there is exactly zero, and so are both moments of the run"""
    mask = np.logical_and.reduce([R.untaken_head_mask(c, b) for b in case["batches"]])
    taken = len(np.unique(np.concatenate([b["actions"].ravel() for b in case["batches"]])))
    assert mask.sum() == (c["n"] - taken) * (c["hidden"][-1] + 1)
    for net in R.NETS[c["algo"]]:
        if net != "pi":
            assert all((r["grads"][net][mask] == 0).all() for r in refs)
            assert (got["m"][net][mask] == 0).all() and (got["v"][net][mask] == 0).all(), (what, net)
    return int(mask.sum())


def _assert_stats(what, c, got, ref):
    losses, preds = STAT_KEYS[c["algo"]]
    for k in losses:
        print(f"{what} {k}: {got['stats'][k]:.7g} vs {ref['stats'][k]:.7g}")
        np.testing.assert_allclose(got["stats"][k], ref["stats"][k], rtol=STAT_RTOL, atol=0, err_msg=f"{what} {k}")
    for k in preds:     # Mean, Std, Max, Min of Q(s)[a]: within the losses' 1e-4 of the largest prediction
        err = np.abs(np.asarray(got["stats"][k], np.float64) - ref["stats"][k]).max()
        print(f"{what} {k}: off by {err:.2e}")
        assert err <= STAT_RTOL * np.abs(ref["stats"][k]).max(), (what, k, got["stats"][k], ref["stats"][k])


def _assert_targets(what, c, case, got):
    """after one step every target is tau * new + (1 - tau) * old, with `new` read from the run itself"""
    tau = R.f32(c["tau"])
    for t in R.TARGETS[c["algo"]]:
        on = R.ONLINE_OF[t]
        new, old = got["P"][on].astype(np.float64), case["P"][t].astype(np.float64)
        err = np.abs(got["P"][t] - (tau * new + (1 - tau) * old)).max()
        print(f"{what} {t}: Polyak off by {err:.2e}")
        assert err <= 2e-7 * max(1.0, np.abs(old).max()), (what, t, err)
        assert np.abs(new - case["P"][on]).max() > 1e-4          # ... and the online net did move
    if c["algo"] == "dsac":
        assert np.abs(got["P"]["pi"].astype(np.float64) - case["P"]["pi"]).max() > 1e-4


def _assert_unmoved(what, c, case, got):
    for k in R.NETS[c["algo"]] + R.TARGETS[c["algo"]]:
        np.testing.assert_array_equal(got["P"][k], case["P"][k], err_msg=f"{what} {k}")


def _assert_inputs(name, c, case, refs):
    """Conditions on the INPUTS, evaluated on the float64 reference: the settings the case is about, mixed terminals, the class cover of the
    actions, max|Q| of order one, a visibly non-uniform policy, and no row (the allowed share is zero) inside DQN's arg-max margin."""
    n = c["n"]
    assert c["discount"] == 0.97 and (c["lr"], c["tau"]) in ((1e-3, 0.01), (0.0, 0.0))
    if c["algo"] == "dsac":
        assert c["reward_scale"] == 5.0 and c["alpha"] == 0.2
    for batch, ref in zip(case["batches"], refs):
        B = batch["observations"].shape[0]
        assert not R.violations(c, ref).any(), (name, np.nonzero(R.violations(c, ref))[0])
        if B > 1:
            assert 0.05 <= float(batch["terminals"].mean()) <= 0.5
        assert len(np.unique(batch["actions"])) >= min(n, 8, B)
        assert 0.5 <= ref["max_q"] <= 20.0, ref["max_q"]
        if c["algo"] == "dsac":
            ent = ref["rows"]["ent"]
            print(f"{name}: B {B}, entropy of pi(s) in [{ent.min():.3f}, {ent.max():.3f}] of log n = {np.log(n):.3f}; max |Q| {ref['max_q']:.2f}")
            assert ent.mean() < 0.95 * np.log(n)
        else:
            print(f"{name}: B {B}, {'double' if c['double_q'] else 'plain'}; smallest arg-max margin {ref['rows']['gap'].min():.2e}, max |Q| {ref['max_q']:.2f}")


@functools.lru_cache(maxsize=None)
def _witness(name):
    c, case = R.make_case(name)
    return R.witness_run(c, case)


# ------------------------------------------------------------------------------------------------ dsac and DQN without a GPU
def test_case_tables_reach_the_intended_paths():
    """Every column-split factor under both losses, a slab stride that is not B, n = ILSX_MAX_NO under dsac, plain and Double DQN, one row."""
    cs = {64: 1, 128: 2, 256: 4}
    for algo in ("dsac", "dqn"):
        cases = [c for k, c in R.CASES.items() if c["algo"] == algo]
        assert {cs[c["hidden"][0]] for c in cases} == {1, 2, 4}
        assert any(c["Bs"][0] < c["max_batch"] and cs[c["hidden"][0]] > 1 for c in cases) and any(c["Bs"] == (1,) for c in cases)
        assert any(c["n"] == 64 for c in cases)
    dq = [c for c in R.CASES.values() if c["algo"] == "dqn"]
    for double in (False, True):
        assert {cs[c["hidden"][0]] for c in dq if c["double_q"] == double} == {1, 2, 4}
        assert any(c["n"] == 64 for c in dq if c["double_q"] == double)
    assert not R.CASES["dqn/max_heads"]["double_q"]
    for c in R.FROZEN.values():
        assert c["Bs"] == (96, 37, 64) and c["max_batch"] == 128 and c["hidden"] == [256, 256] and c["n"] == 5 and c["lr"] == 0 and c["tau"] == 0


@pytest.mark.parametrize("name", ONE_STEP)
def test_restatement_agrees_with_the_witness(name):
    """T1 / T3 on the fp32 witness: the Adam moments the device test reads within 1e-5 / 2e-5 per block of autograd in float64, exact zeros on
    the untaken head rows, the statistics, the targets' Polyak step, the conditions on the inputs."""
    c, case = R.make_case(name)
    got = _witness(name)
    refs = _check(f"{name} witness", c, case, got, GRAD_REL / 10, SQ_REL / 10)
    print("WITNESS {} {}: exp_avg {:.2e}, exp_avg_sq {:.2e} of a block's largest entry".format(c["algo"], name, *_worst(c, case, got)))
    _assert_inputs(name, c, case, refs)
    zeros = _assert_untaken_zero(f"{name} witness", c, case, got, refs)
    assert zeros > 0 or c["shape"] not in ("max_heads", "max_heads_double", "one_row")
    _assert_stats(f"{name} witness", c, got, refs[0])
    _assert_targets(f"{name} witness", c, case, got)
    if c["algo"] == "dqn":      # two float64 statements of the step, one by hand and one by autograd, agree to rounding
        from dqn_restatement import DqnRestatement
        w = DqnRestatement(c["o"], c["hidden"], c["n"], case["P"]["q"], case["P"]["tq"], c["double_q"], False, R.f32(c["discount"]), c["lr"], c["tau"], 1)
        g = w.train_step(case["batches"][0])["grad"]
        assert all(e <= 1e-10 * m for _, e, m in R.block_errors(g, refs[0]["grads"]["q"], c))


@pytest.mark.parametrize("name", THREE_STEPS)
def test_frozen_run_agrees_with_the_witness(name):
    """T2 on the fp32 witness: zero learning rates and tau leave every block bitwise alone, and the moments after B = 96, 37, 64 are the
    geometric sums of the three float64 gradients within 1e-5 / 2e-5 per block — and every one of the three steps weighs."""
    c, case = R.make_case(name)
    got = _witness(name)
    _assert_unmoved(f"{name} witness", c, case, got)
    refs = _check(f"{name} witness", c, case, got, GRAD_REL / 10, SQ_REL / 10)
    print("WITNESS {} {}: exp_avg {:.2e}, exp_avg_sq {:.2e} of a block's largest entry".format(c["algo"], name, *_worst(c, case, got)))
    _assert_inputs(name, c, case, refs)
    net = R.NETS[c["algo"]][0]
    for drop in range(3):
        m = R.adam_moments([r["grads"][net] * (i != drop) for i, r in enumerate(refs)], c["beta_1"])[0]
        assert max(e / m_ for _, e, m_ in R.block_errors(got["m"][net], m, c)) > 100 * GRAD_REL, drop


def _identity(wrong, c):
    """The two pairs in which the wrong reference IS the right one, by the structure of the case, not by its draw:
      inv_b   where B == max_batch (spec, generic): 1/max_batch is 1/B;
      no_done on one_row: its single row is not terminal — a terminal one would turn the five mutations of the bootstrap term (online_targets,
              target_pi_s, no_target_entropy, swap_double, no_discount) into identities instead — so (1 - d) is 1.
    Every other pair of a mutation and a one-step case is in WRONG_CASES; test_excluded_pairs_are_identities asserts these are identities."""
    return (wrong == "inv_b" and c["Bs"][0] == c["max_batch"]) or (wrong == "no_done" and c["Bs"] == (1,))


_PAIRS = [(w, k) for k, c in R.CASES.items() for w in (R.DSAC_WRONG if c["algo"] == "dsac" else R.DQN_WRONG)]
WRONG_CASES = [(w, k) for w, k in _PAIRS if not _identity(w, R.CASES[k])]
IDENTITIES = [(w, k) for w, k in _PAIRS if _identity(w, R.CASES[k])]


@pytest.mark.parametrize("wrong,name", IDENTITIES)
def test_excluded_pairs_are_identities(wrong, name):
    """what WRONG_CASES leaves out computes the right step: the same gradients to the last bit or, where a product with 1.0 was saved, to rounding"""
    c, case = R.make_case(name)
    assert (c["Bs"][0] == c["max_batch"]) if wrong == "inv_b" else not case["batches"][0]["terminals"].any()
    right, other = (R.step_f64(c, case["P"], case["batches"][0], wrong=w)["grads"] for w in (None, wrong))
    for net in R.NETS[c["algo"]]:
        assert all(e <= 1e-14 * m for _, e, m in R.block_errors(other[net], right[net], c)), (wrong, name, net)


@pytest.mark.parametrize("wrong,name", WRONG_CASES)
def test_wrong_references_are_caught(wrong, name):
    """The fp32 witness stands in for the device.  The same `_check` the GPU tests use, at TEN times their bounds, rejects each of — dsac:
      online_targets    — the target from the online critics;           target_pi_s       — the target from pi(s) instead of pi(s');
      no_target_entropy — the entropy term dropped from the target;     no_reward_scale   — reward_scale lost;
      no_done           — (1 - d) lost;                                  inv_b             — 1/max_batch for 1/B;
      no_half           — the critic loss without its 0.5;               shift_action      — the gradient into column a + 1 mod n;
      pi_pre            — the policy loss on the pre-update critics;     pi_q1             — the policy loss on Q1 alone;
      no_policy_entropy — the policy's entropy term dropped;
    DQN:
      online_targets — the target from the online net;   swap_double — Double DQN computed as plain, and plain as double;
      half — the MSE with a 0.5;   inv_b — 1/max_batch;   no_done — (1 - d) lost;   no_discount — the discount lost.
    on EVERY one-step case of its algorithm, but for the pairs `_identity` names.  For swap_double every DQN case has a non-terminal row
    whose two arg-maxes differ (discrete_restatement.swap_sensitive; one_row is drawn until its row is one)."""
    c, case = R.make_case(name)
    got = _witness(name)
    _check(f"{name} witness", c, case, got, GRAD_REL / 10, SQ_REL / 10)
    with pytest.raises(AssertionError) as failure:
        _check(f"{name} against {wrong}", c, case, got, 10 * GRAD_REL, 10 * SQ_REL, wrong=wrong)
    print("rejected:", str(failure.value)[:300])
    print(f"MISS {c['algo']} {wrong} {name}: {_worst(c, case, got, wrong=wrong)[0] / GRAD_REL:.3g} times the bound")


# ------------------------------------------------------------------------------------------------ GCSL CLASS: checks and the host witness
class _NetHead(C.Structure):
    """The harness has no getter for the Adam moments, so they are read through the handle: gch_create returns a HostCat*
    (tests/harness/gcsl_bn_host.cpp), whose first member is `GcslNet N` (csrc/gcsl.h, `struct GcslNet`: int D, H, nblk, n; float *P, *G,
    *M, *V; float *rmean, *rvar).  This mirrors those leading members; _host_run checks the mirror against what the harness's own getters
    return — the dimensions, P and both running statistics before the step, P after it (P - lr * M / (sqrt(V) + eps) of THESE M, V)."""
    _fields_ = [(k, C.c_int) for k in ("D", "H", "nblk", "n")] + [(k, C.POINTER(C.c_float)) for k in ("P", "G", "M", "V", "rmean", "rvar")]


def _gcsl_check(what, c, ref, got, grad_rel, sq_rel, report=None):
    """exp_avg = 0.1 g and exp_avg_sq = 0.001 g^2 of the first step on the live entries of every block; the step count"""
    dead = ref["dead"]
    biases = np.concatenate([np.full(int(np.prod(s)), nm in [f"b{l}" for l in range(c["nblk"])]) for nm, s in GR.layout(c["D"], c["H"], c["nblk"], c["n"])])
    assert dead.sum() == c["nblk"] * c["H"] and np.array_equal(dead, biases)      # dead_bias_mask(): the Linear biases under a BatchNorm, no more
    assert got["step"] == 1, got["step"]
    m, v = R.adam_moments([ref["grad"]], 0.9)
    _block_check(f"{what} exp_avg", R.gcsl_block_errors(got["m"], m, c, ~dead), grad_rel, None if report is None else report[0])
    _block_check(f"{what} exp_avg_sq", R.gcsl_block_errors(got["v"], v, c, ~dead), sq_rel, None if report is None else report[1])


def _gcsl_rest(what, c, ref, got):
    """the statistics (CE at rtol 1e-4, Accuracy exactly) and the running statistics after the one step"""
    print(f"{what}: CE {got['ce']:.7g} vs {ref['ce']:.7g}, accuracy {got['acc']:.6f} vs {ref['acc']:.6f}")
    np.testing.assert_allclose(got["ce"], ref["ce"], rtol=STAT_RTOL, atol=0)
    assert np.float32(got["acc"]) == np.float32(ref["acc"])
    np.testing.assert_allclose(got["rm"], ref["running_mean"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(got["rv"], ref["running_var"], rtol=1e-4, atol=1e-5)


def _gcsl_inputs(name, c, X, y, ref):
    """Conditions on the INPUTS, on the float64 reference: no column is constant over the batch, so every live parameter has a gradient and
    the dead biases none; every row's top two probabilities are 1e-5 apart (no row left out), so Accuracy cannot flip, and it is neither 0 nor 1."""
    assert (X.min(0) < X.max(0)).all() and len(np.unique(y)) >= min(c["n"], 8)
    scale = np.abs(ref["grad"]).max()
    assert (np.abs(ref["grad"][ref["dead"]]) <= 1e-12 * scale).all() and (ref["grad"][~ref["dead"]] != 0).all()
    top = np.sort(ref["probs"], 1)
    print(f"{name}: smallest top-two probability margin {np.min(top[:, -1] - top[:, -2]):.2e}, largest probability {top[:, -1].max():.3f}, accuracy {ref['acc']:.3f}")
    assert (top[:, -1] - top[:, -2] > 1e-5).all() and top[:, -1].max() > 1.5 / c["n"] and 0.25 <= ref["acc"] < 1


def _host_run(lib, c, p0, X, y):
    """one CLASS step of the device text on the host from zero moments"""
    h = lib.gch_create(c["D"], c["H"], c["nblk"], c["n"], c["max_rows"])
    assert h and lib.gch_num_params(h) == p0.size
    head = C.cast(C.c_void_p(h), C.POINTER(_NetHead)).contents
    assert (head.D, head.H, head.nblk, head.n) == (c["D"], c["H"], c["nblk"], c["n"])
    lib.gch_set_params(h, np.ascontiguousarray(p0).ctypes.data_as(C.c_void_p))
    st, y32, Xc = np.zeros(2, np.float32), np.ascontiguousarray(y, np.int32), np.ascontiguousarray(X)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    peek = lambda k, n=p0.size: np.ctypeslib.as_array(getattr(head, k), shape=(n,)).copy()   # noqa: E731
    nbh = c["nblk"] * c["H"]
    assert np.array_equal(peek("P"), p0) and (peek("M") == 0).all() and (peek("V") == 0).all()
    assert (peek("rmean", nbh) == 0).all() and (peek("rvar", nbh) == 1).all()
    assert lib.gch_train_step(h, p(Xc), p(y32), c["B"], c["lr"], p(st)) == 0
    m, v = peek("M"), peek("V")
    params, rm, rv = np.empty(p0.size, np.float32), np.empty((c["nblk"], c["H"]), np.float32), np.empty((c["nblk"], c["H"]), np.float32)
    lib.gch_get(h, p(params), p(rm), p(rv))
    assert np.array_equal(peek("P"), params) and np.array_equal(peek("rmean", nbh), rm.ravel()) and np.array_equal(peek("rvar", nbh), rv.ravel())
    # M and V are the buffers Adam stepped with (a swapped or shifted mirror fails here, not in a bound): first step, bias corrections 0.1 / 0.001
    step = c["lr"] * (m.astype(np.float64) / 0.1) / (np.sqrt(v.astype(np.float64) / 0.001) + 1e-8)
    assert np.abs(params - (p0.astype(np.float64) - step)).max() <= 1e-6 * max(1.0, np.abs(p0).max()) and np.abs(step).max() > 0.5 * c["lr"]
    lib.gch_destroy(h)
    return dict(m=m, v=v, step=1, rm=rm, rv=rv, ce=float(st[0]), acc=float(st[1]))


_HOST = {}


def _gcsl_witness(lib, name):
    if name not in _HOST:
        _HOST[name] = _host_run(lib, *R.gcsl_case(name))
    return _HOST[name]


@pytest.mark.parametrize("name", GCSL)
def test_gcsl_restatement_agrees_with_the_host_emulation(hostlib, name):  # noqa: F811
    """The device text of the CLASS step, compiled for the host, within 1e-5 / 2e-5 per block of autograd in float64; the conditions on the
    inputs: no constant column, every live parameter has a gradient and the dead biases none, every row's top two probabilities 1e-5 apart."""
    c, p0, X, y = R.gcsl_case(name)
    assert (c["H"], c["nblk"], c["n"], c["B"], c["max_rows"]) == R.GCSL_CASES[name] and c["D"] == c["O"] + c["GD"] + c["T"]
    ref = R.gcsl_f64(c, p0, X, y)
    _gcsl_inputs(name, c, X, y, ref)
    got, report = _gcsl_witness(hostlib, name), ([], [])
    _gcsl_check(f"gcsl/{name} host", c, ref, got, GRAD_REL / 10, SQ_REL / 10, report)
    print(f"WITNESS gcsl {name}: exp_avg {report[0][0]:.2e}, exp_avg_sq {report[1][0]:.2e} of a block's largest entry")
    _gcsl_rest(f"gcsl/{name} host", c, ref, got)


GCSL_WRONG_CASES = [(w, k) for w in GR.CatRestatement.WRONG for k in GCSL]


@pytest.mark.parametrize("wrong,name", GCSL_WRONG_CASES)
def test_gcsl_wrong_references_are_caught(hostlib, wrong, name):  # noqa: F811
    """The host emulation stands in for the device; `_gcsl_check` at TEN times the GPU bounds rejects each of CatRestatement.WRONG: BatchNorm's
    backward with the batch statistics held constant, the running statistics in the training forward, dlogit without its 1/B, the one-hot at
    y + 1 mod n, the output bias's gradient as a mean."""
    c, p0, X, y = R.gcsl_case(name)
    got, ref, report = _gcsl_witness(hostlib, name), R.gcsl_f64(c, p0, X, y, wrong=wrong), ([], [])
    with pytest.raises(AssertionError) as failure:
        _gcsl_check(f"gcsl/{name} against {wrong}", c, ref, got, 10 * GRAD_REL, 10 * SQ_REL)
    print("rejected:", str(failure.value)[:300])
    _gcsl_check("measure", c, ref, got, np.inf, np.inf, report)
    print(f"MISS gcsl {wrong} {name}: {report[0][0] / GRAD_REL:.3g} times the bound")


# ------------------------------------------------------------------------------------------------ the device steps
def _trainer(ctx, c, case):
    """a fresh device trainer of the case with EVERY block, targets included, set from the case"""
    import ilswiss_amd as ia
    from ilswiss_amd.discrete_sac import DiscreteSoftActorCritic
    o, hid, n = c["o"], c["hidden"], c["n"]
    qs = [ia.FlattenMlp(hidden_sizes=hid, input_size=o, output_size=n, ctx=ctx) for _ in range(2)]
    if c["algo"] == "dsac":
        pol = ia.DiscretePolicy(hidden_sizes=hid, obs_dim=o, action_dim=n, ctx=ctx)
        tr = DiscreteSoftActorCritic(pol, qs[0], qs[1], reward_scale=c["reward_scale"], discount=c["discount"], alpha=c["alpha"], policy_lr=c["lr"],
                                     qf_lr=c["lr"], soft_target_tau=c["tau"], beta_1=c["beta_1"], max_batch=c["max_batch"])
    else:
        tr = (ia.DoubleDQN if c["double_q"] else ia.DQN)(qs[0], learning_rate=c["lr"], use_hard_updates=False, tau=c["tau"], discount=c["discount"],
                                                         max_batch=c["max_batch"])
    for k in R.NETS[c["algo"]] + R.TARGETS[c["algo"]]:
        tr.set_flat_params(R.DEVICE_NAME[k], case["P"][k])
        np.testing.assert_array_equal(tr.get_flat_params(R.DEVICE_NAME[k]), case["P"][k])
    return tr


def _device_run(ctx, c, case):
    """the statistics are those of the first step; the moments and blocks those after the last"""
    tr = _trainer(ctx, c, case)
    assert tr.get_eval_statistics() is None
    for b in case["batches"]:
        tr.train_step(b)
    st, snap, nets = tr.get_eval_statistics(), tr.get_snapshot(), R.NETS[c["algo"]]
    opt = {k: snap[R.DEVICE_NAME[k] + "_optimizer"] for k in nets}
    stats = {k: st[k] for k in STAT_KEYS[c["algo"]][0]}
    stats.update({k: [st[f"{k} {s}"] for s in ("Mean", "Std", "Max", "Min")] for k in STAT_KEYS[c["algo"]][1]})
    got = dict(P={k: tr.get_flat_params(R.DEVICE_NAME[k]) for k in nets + R.TARGETS[c["algo"]]}, m={k: opt[k]["exp_avg"] for k in nets},
               v={k: opt[k]["exp_avg_sq"] for k in nets}, steps={k: opt[k]["step"] for k in nets}, stats=stats)
    return got


@gpu
@pytest.mark.parametrize("name", ONE_STEP)
def test_hip_first_step_gradients_vs_float64(ctx, name):
    """T1 and T3 on the device: one step from zero moments with every block set, dsac's policy loss of the reference evaluated with the critics
    the device reports after the step; exact zeros on the untaken head rows; the step's statistics; the targets' Polyak step."""
    c, case = R.make_case(name)
    got = _device_run(ctx, c, case)
    refs = _check(name, c, case, got, GRAD_REL, SQ_REL)
    _assert_inputs(name, c, case, refs)
    _assert_untaken_zero(name, c, case, got, refs)
    _assert_stats(name, c, got, refs[0])
    _assert_targets(name, c, case, got)


@gpu
@pytest.mark.parametrize("name", THREE_STEPS)
def test_hip_frozen_three_steps_vs_float64(ctx, name):
    """T2 on the device: B = 96, then 37, then 64 under max_batch = 128 with nothing moving — nothing of the 96-row step survives into the
    37-row one through the reused partial slabs and workspaces."""
    c, case = R.make_case(name)
    got = _device_run(ctx, c, case)
    _assert_unmoved(name, c, case, got)
    refs = _check(name, c, case, got, GRAD_REL, SQ_REL)
    _assert_stats(name, c, got, refs[0])


@gpu
@pytest.mark.parametrize("name", GCSL)
def test_hip_gcsl_class_first_step_vs_float64(ctx, name):
    """The CLASS step on the device: both Adam moments of the first step per block on the live entries, CE and Accuracy, the running
    statistics after the step."""
    from ilswiss_amd.gcsl import GCSL as Trainer
    from ilswiss_amd.gcsl import CatagorialConditionPolicy
    c, p0, X, y = R.gcsl_case(name)
    O, GD, B = c["O"], c["GD"], c["B"]
    pol = CatagorialConditionPolicy([c["H"]] * c["nblk"], O, GD + c["T"], c["n"], max_rows=c["max_rows"], ctx=ctx)
    pol.set_flat_params(p0)
    np.testing.assert_array_equal(pol.get_flat_params(), p0)
    tr = Trainer(pol, mode="CLASS", use_horizons=True, goal_dim=GD, policy_lr=c["lr"], max_batch=c["max_rows"])
    tr.train_step(dict(observations=X[:, :O], desired_goals=X[:, O:O + GD], horizons=X[:, O + GD:], actions=y.reshape(B, 1)))
    st, snap = tr.get_eval_statistics(), pol.get_snapshot()
    got = dict(m=snap["adam_m"], v=snap["adam_v"], step=int(snap["meta"][0]), rm=snap["running_mean"], rv=snap["running_var"],
               ce=st["CE Loss"], acc=st["Accuracy"])
    ref = R.gcsl_f64(c, p0, X, y)
    _gcsl_inputs(name, c, X, y, ref)
    _gcsl_check(f"gcsl/{name}", c, ref, got, GRAD_REL, SQ_REL)
    _gcsl_rest(f"gcsl/{name}", c, ref, got)
