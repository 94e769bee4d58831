"""Gradient-level parity of the MBPO ensemble's train step (csrc/bnn.h k_bnn_fwd<BNN_TRAIN> / k_bnn_wide<BNN_TRAIN> / k_bnn_dw_adam behind
ilsx_bnn_train_batch) against the float64 autograd restatement `step_f64` of tests/mbpo_restatement.py.

Parameters after Adam say little about a gradient (the header of tests/test_ac_parity_hip.py): the update is lr * m / (sqrt(v) + 1e-8), so a
gradient wrong by a constant factor (a lost 1/E, 1/max_batch for 1/B, the 2 of d/dmu) moves the parameters as the right one does, and one
wrong in a few entries moves them by about lr.  The gradient is read from the Adam moments that BNN.get_opt() returns in the parameters'
layout; with weight decay the optimiser sees g + wd_l * p:

  T1, first step from zero moments: a fresh BNN + BNNTrainer at lr 1e-3, set_params, one _train_batch.  Then exp_avg = 0.1 (g + wd p),
      exp_avg_sq = 0.001 (g + wd p)^2, t = 1; the returned loss PER MEMBER against the float64 loss; the padded entries exactly zero.
  T2, frozen: lr 0, batch_size 128, three steps at B = 96, 37, 64.  The parameters stay bitwise, the moments are the geometric sums of the
      three float64 gradients, t = 3: nothing of step i reaches step i + 1 through the workspace rows that only `gr < rows` writes.
  T3, the transposed copy follows the optimiser: after T1's step a second one on new rows; its reference is evaluated at the parameters the
      device reports after step one.  The backward reads Wt, which the dW kernel rewrites next to W; a Wt left behind shows here alone.

Inputs: rows as in tests/test_mbpo_hip.py, parameters from init_params(init_w = 0.1) with the head bias of the raw log-variance columns
redrawn from U(-13.5, 2.5) per member and column, so that every case with B > 1 has at least 5 % of its raw log-variances above max_lv = 0.5,
5 % below min_lv = -10 and 5 % between (both sigmoids of the soft clamp's derivative then matter); reward_scale 2; max_batch = B + 11, so
1/max_batch is not 1/B; one weight decay per layer, all distinct, passed as an explicit list.  The decays are not 0.05, 0.10, ...: the
gradient grows by about sqrt(in * out) per layer towards the head (a column clamped at -10 multiplies d/dmu by e^10 on top), so a fixed
list leaves wd_l * p at 8e-5 .. 1 of a block's largest entry; make_case sets wd_l * max|W_l| to 1 % of the largest float64 gradient entry of
that layer's weight instead, which puts the decay term at 1 % .. 85 % in every weight block — at least ten times the bound.  All of that
is asserted on the float64 reference.  No row sits past softplus's threshold of 20, so an fp32 evaluation takes the float64 one's branch.

Bounds: exp_avg within 1e-4 of the largest reference entry, exp_avg_sq within 2e-4 (the figures of test_ac_parity_hip.py,
test_bc_parity_hip.py and test_ppo_parity_hip.py), PER BLOCK — one member's weight or bias of one layer — so that a small block cannot hide
behind a large one nor one member behind another.  None is tuned to what the device returns.  What keeps them honest runs without a GPU:
  - the float32 torch restatement (AdamTrainer, the one the value-level suites compare with) sits within a TENTH of them on every case.
    Measured worst over all cases and blocks, as a share of the block's largest entry: gradient and exp_avg 1.5e-6, exp_avg_sq 2.2e-6
    (both max_waves, fc2.weight[1]); the other cases 4e-7 .. 1.2e-6.  So no case needed a bound of its own; had one, that measured
    distance would have set it.
  - the same `_check` at TEN times the bounds rejects thirteen deliberately wrong references (test_wrong_references_are_caught: eleven of
    them on all nine cases; the upper clamp's sigmoid and the + mean(lv) term on four, and on the other five at the bounds themselves,
    see BELOW_TEN_BOUNDS) and a backward chain through a
    transposed copy that the optimiser left behind (T3).
Measured on an MI355X, worst over the thirteen device tests: exp_avg 1.7e-6 (max_waves, fc2.weight[1]), exp_avg_sq 1.5e-5 — of which 1.3e-5
is the same in every block: k_bnn_dw_adam forms 1 - beta_2 as 1.0f - 0.999f = 0.99998713e-3 where torch rounds 1 - 0.999 to float32."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mbpo_restatement as R

gpu = pytest.mark.gpu
GRAD_REL, SQ_REL = 1e-4, 2e-4
N_ROWS, REWARD_SCALE, LR, DECAY_SHARE = 300, 2.0, 1e-3, 0.01
# name -> (E, o, a, H, n_hidden, B)
CASES = dict(ref_pad=(3, 11, 3, 200, 4, 37),            # 200 -> 208 padding, 13 waves, partial last tile
             one_hidden=(2, 11, 3, 40, 1, 16),          # one backward iteration, padded H, exact tile
             one_row=(2, 3, 1, 16, 2, 1),               # one wave, one row
             in_head_wider=(2, 62, 8, 32, 2, 33),       # KP0 = 80 and NOP = 128 above HP = 32: waves that idle behind w < np / 16
             max_waves=(2, 11, 3, 256, 2, 32),          # 16 waves: the narrow kernel's limit and the size of sred
             deep=(2, 11, 3, 24, 8, 20),                # ILSX_BNN_MAX_LAYERS
             seven=(7, 11, 3, 48, 2, 64),               # the reference's member count
             wide_odd=(2, 11, 3, 260, 4, 31),           # k_bnn_wide, 17 slices, the last wave has one
             wide_humanoid=(2, 45, 17, 400, 4, 48))     # k_bnn_wide, 25 slices, in 62 -> 64, head 92 -> 96
SEEDS = dict(max_waves=200)      # a case's draw where 100 + its position leaves one of the clamp's regimes under 5 % (_assert_inputs)
FROZEN, FROZEN_BATCHES, FROZEN_MAX = ["ref_pad", "wide_odd"], (96, 37, 64), 128
SECOND = ["ref_pad", "wide_humanoid"]


def _rows(rng, n, o, a):
    """tests/test_mbpo_hip.py's _data"""
    obs = rng.normal(0, 1, (n, o)).astype(np.float32)
    act = rng.uniform(-1, 1, (n, a)).astype(np.float32)
    rew = rng.normal(0, 1, n).astype(np.float32)
    nobs = (obs + 0.1 * rng.normal(0, 1, (n, o))).astype(np.float32)
    return obs, act, rew, nobs


@functools.lru_cache(maxsize=None)
def make_case(name, batches=None, max_batch=None):
    """The inputs of a run: rows, normaliser, parameters, per-layer decays and the [E, sum(batches)] index table, each member on its own
    rows.  Built once per (case, batches) and shared; nothing in it is written afterwards."""
    E, o, a, H, nh, B = CASES[name]
    batches = (B,) if batches is None else batches
    rng = np.random.default_rng(SEEDS.get(name, 100 + list(CASES).index(name)))
    obs, act, rew, nobs = _rows(rng, N_ROWS, o, a)
    D = o + 1
    params = R.init_params(rng, E, o + a, [H] * nh, D, init_w=0.1)
    params[-1][:, :, D:] = rng.uniform(-13.5, 2.5, (E, 1, D)).astype(np.float32)
    x, t = R.data_from_rows(obs, act, rew, nobs, reward_scale=REWARD_SCALE)
    mean, std = R.normalizer_stats(x)
    table = rng.integers(0, N_ROWS, (E, sum(batches))).astype(np.int32)
    cols = [int(c) for c in np.cumsum((0,) + tuple(batches[:-1]))]
    # The decays.  Between the first layer and the head the gradient grows by about 1 / max|W| = sqrt(in * out) per layer (five to eight
    # orders of magnitude over a case) and by up to ten between members, so no fixed list keeps wd_l * p above the bound in one layer
    # without burying the gradient under it in another.  Per layer: wd_l * max|W_l| is DECAY_SHARE of the largest entry of the float64
    # gradient of that layer's weight in the member where it is largest (three digits kept) — a hundred times the bound's 1e-4 there, more in
    # the other members — which _assert_inputs holds to at least ten times the bound in every weight block.
    shp = R.shapes(E, o + a, [H] * nh, D)
    idx0 = table[:, :batches[0]]
    g0 = R.step_f64(params, mean, std, x[idx0], t[idx0], [0.0] * (nh + 1))["grads"]
    g_max = [max(np.abs(g0[sl]).max() for nm, sl in R.blocks(shp) if nm.startswith(f"fc{l}.weight")) for l in range(nh + 1)]
    wd = [float(f"{DECAY_SHARE * g_max[l] / np.abs(params[2 * l]).max():.2e}") for l in range(nh + 1)]
    return dict(name=name, E=E, o=o, a=a, H=H, nh=nh, D=D, batches=batches, max_batch=max(batches) + 11 if max_batch is None else max_batch,
                rows=(obs, act, rew, nobs), x=x, t=t, mean=mean, std=std, params=params, shp=shp, wd=wd, table=table, cols=cols,
                idx=[table[:, c:c + b] for c, b in zip(cols, batches)])


def _step_f64(case, s, params=None, wrong=None, stale=None):
    idx = case["idx"][s]
    return R.step_f64(case["params"] if params is None else params, case["mean"], case["std"], case["x"][idx], case["t"][idx], case["wd"],
                      wrong=wrong, max_batch=case["max_batch"], reward_scale=REWARD_SCALE, stale=stale)


@functools.lru_cache(maxsize=None)
def _initial_refs(name, batches=None, max_batch=None):
    """the float64 step of every batch of a run at the case's own parameters: computed once, shared by the tests, never written"""
    case = make_case(name, batches, max_batch)
    return [_step_f64(case, s) for s in range(len(case["batches"]))]


def _block_check(what, got, ref, shp, rel):
    """max|got - ref| <= rel * max|ref| on every block (an all-zero reference block therefore demands exact zeros); every figure is printed
    before it is asserted.  Returns the worst error as a share of its block's largest entry."""
    errs = R.block_errors(got, ref, shp)
    print(what, " ".join(f"{nm}:{e:.2e}/{m:.2e}" for nm, e, m in errs))
    bad = [(nm, e, m) for nm, e, m in errs if not e <= rel * m]
    assert not bad, (what, rel, bad)
    return max((e / m, nm) for nm, e, m in errs if m > 0)


def _check(what, case, got, grad_rel, sq_rel, wrong=None, params=None, stale=None):
    """A run's Adam state against the float64 reference: the step count and both moments per block.  `got`: dict(m, v, t).  `params`: per
    step, the parameters that step's reference is evaluated at (None: the case's own).  Returns the references and, as text, the worst error of either moment as a share
    of its block's largest entry."""
    n = len(case["batches"])
    params = [None] * n if params is None else params
    if wrong is None and stale is None and all(p is None for p in params):
        refs = _initial_refs(case["name"], case["batches"] if n > 1 else None, case["max_batch"] if n > 1 else None)
    else:
        refs = [_step_f64(case, s, params[s], wrong, stale if s == n - 1 else None) for s in range(n)]
    assert got["t"] == n, (what, got["t"])
    m, v = R.adam_moments([r["grads"] for r in refs])
    worst_m = _block_check(f"{what} exp_avg", got["m"], m, case["shp"], grad_rel)
    worst_v = _block_check(f"{what} exp_avg_sq", got["v"], v, case["shp"], sq_rel)
    return refs, f"exp_avg {worst_m[0]:.2e} ({worst_m[1]}), exp_avg_sq {worst_v[0]:.2e} ({worst_v[1]})"


def _assert_inputs(case, refs):
    """Conditions on the INPUTS, on the float64 reference: the three regimes of the soft clamp are populated, no row is past softplus's
    threshold, and the decay term of every weight block is at least ten times the bound."""
    name = case["name"]
    for s, ref in enumerate(refs):
        raw, B = ref["raw"], case["batches"][s]
        lv1 = R.MAX_LV - np.logaddexp(0.0, R.MAX_LV - raw)
        assert (R.MAX_LV - raw).max() < 20 and (lv1 - R.MIN_LV).max() < 20, name
        shares = dict(above=float(np.mean(raw > R.MAX_LV)), below=float(np.mean(raw < R.MIN_LV)))
        shares["between"] = 1 - shares["above"] - shares["below"]
        print(f"{name} step {s}: raw log-variance above {R.MAX_LV}: {shares['above']:.3f}, below {R.MIN_LV}: {shares['below']:.3f}, "
              f"between: {shares['between']:.3f}; raw in [{raw.min():.2f}, {raw.max():.2f}]")
        assert min(shares.values()) >= 0.05 if B > 1 else max(shares.values()) < 1, (name, shares)
    assert len(case["wd"]) == case["nh"] + 1 and len(set(case["wd"])) == len(case["wd"])
    flat = np.concatenate([p.reshape(-1) for p in case["params"]]).astype(np.float64)
    decay = np.concatenate([np.full(p.size, case["wd"][i // 2]) for i, p in enumerate(case["params"])]) * flat
    share = [(nm, float(np.abs(decay[sl]).max() / np.abs(refs[0]["grads"][sl]).max())) for nm, sl in R.blocks(case["shp"]) if ".weight" in nm]
    print(f"{name}: largest decay term of a weight block as a share of the block's largest entry: "
          f"{min(r for _, r in share):.2e} .. {max(r for _, r in share):.2e}")
    assert min(r for _, r in share) >= 10 * GRAD_REL, (name, [x for x in share if x[1] < 10 * GRAD_REL])


# ------------------------------------------------------------------------------------------------ the float32 restatement as a run
@functools.lru_cache(maxsize=None)
def _torch_run(name, lr, batches=None, max_batch=None):
    """tests/mbpo_restatement.py's AdamTrainer (float32 torch, the value-level suites' reference) over the case's batches: the optimiser's
    own exp_avg / exp_avg_sq / step, the gradient read from .grad with wd * p added, the loss per member, the parameters per step."""
    case = make_case(name, batches, max_batch)
    tr = R.AdamTrainer(case["params"], lr, case["wd"])
    wd = [case["wd"][i // 2] for i in range(len(tr.P))]
    grads, losses, after = [], [], []
    for idx in case["idx"]:
        p0 = tr.params()
        with torch.no_grad():
            losses.append(R.compute_loss(tr.P, case["mean"], case["std"], case["x"][idx], case["t"][idx]).numpy())
        tr.step(case["mean"], case["std"], case["x"][idx], case["t"][idx])
        grads.append(np.concatenate([(p.grad.numpy().astype(np.float64) + w * q).reshape(-1) for p, q, w in zip(tr.P, p0, wd)]))
        after.append(tr.params())
    st = [tr.opt.state[p] for p in tr.P]
    steps = {int(s["step"]) for s in st}
    assert len(steps) == 1
    return dict(m=np.concatenate([s["exp_avg"].numpy().reshape(-1) for s in st]), v=np.concatenate([s["exp_avg_sq"].numpy().reshape(-1) for s in st]),
                t=steps.pop(), loss=losses, grads=grads, P=after)


def _loss_check(what, got, ref):
    """the loss PER MEMBER at the project's 1e-4 * max(1, |loss|)"""
    print(f"{what} loss per member: got {np.asarray(got).tolist()}, float64 {np.asarray(ref).tolist()}")
    for e, (g, r) in enumerate(zip(got, ref)):
        assert abs(float(g) - float(r)) < 1e-4 * max(1.0, abs(float(r))), (what, e, g, r)


# ------------------------------------------------------------------------------------------------ without a GPU
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_is_sound(name):
    """T1 on the float32 restatement: its gradient (.grad + wd p) within 1e-5 per block of float64 autograd, the optimiser's moments within
    a tenth of the device's bounds, the loss per member; the inputs' conditions."""
    case, got = make_case(name), _torch_run(name, LR)
    refs, worst = _check(f"{name} fp32", case, got, GRAD_REL / 10, SQ_REL / 10)
    _assert_inputs(case, refs)
    w2 = _block_check(f"{name} fp32 gradient", got["grads"][0], refs[0]["grads"], case["shp"], GRAD_REL / 10)
    print(f"{name}: worst fp32 figures, of the block's largest entry: {worst}, gradient {w2[0]:.2e} ({w2[1]})")
    _loss_check(f"{name} fp32", got["loss"][0], refs[0]["loss"])
    assert case["max_batch"] != case["batches"][0] and case["E"] > 1


@pytest.mark.parametrize("name", FROZEN)
def test_frozen_restatement_is_sound(name):
    """T2 on the float32 restatement: lr 0 leaves the parameters bitwise alone, the moments after B = 96, 37, 64 are the geometric sums of the
    three float64 gradients within a tenth of the bounds — and the earlier steps do weigh: against the last step's alone the moments are
    off by more than 100 times the bound."""
    case, got = make_case(name, FROZEN_BATCHES, FROZEN_MAX), _torch_run(name, 0.0, FROZEN_BATCHES, FROZEN_MAX)
    for p, q in zip(got["P"][-1], case["params"]):
        np.testing.assert_array_equal(p, q)
    refs, worst = _check(f"{name} frozen fp32", case, got, GRAD_REL / 10, SQ_REL / 10)
    _assert_inputs(case, refs)
    print(f"{name} frozen: worst fp32 figures: {worst}")
    m_last = R.adam_moments([refs[-1]["grads"]])[0]
    off = min(e / m for _, e, m in R.block_errors(got["m"], m_last, case["shp"]) if m > 0)
    print(f"{name} frozen: against the last step alone exp_avg is off by at least {off:.2e} of a block's largest entry")
    assert off > 100 * GRAD_REL


@pytest.mark.parametrize("name", SECOND)
def test_second_step_restatement_is_sound(name):
    """T3 on the float32 restatement: the second step's moments against a reference evaluated at the parameters the run reports after step
    one — and the case discriminates: a backward chain through the weights of BEFORE step one (a transposed copy the optimiser left behind)
    misses by at least ten times the bound."""
    B = CASES[name][5]
    case, got = make_case(name, (B, B)), _torch_run(name, LR, (B, B))
    _, worst = _check(f"{name} second fp32", case, got, GRAD_REL / 10, SQ_REL / 10, params=[None, got["P"][0]])
    print(f"{name} second step: worst fp32 figures: {worst}")
    with pytest.raises(AssertionError) as failure:
        _check(f"{name} second against a stale Wt", case, got, 10 * GRAD_REL, 10 * SQ_REL, params=[None, got["P"][0]], stale=case["params"])
    print("rejected:", str(failure.value)[:300])


# Two of the mistakes change the gradient of the raw log-variance by O(1) * gscale per entry (the upper sigmoid only where raw > 0.5, the
# + mean(lv) term everywhere), while a block's largest entry comes from the columns clamped at -10, whose d/dmu carries e^10: in a member
# that has such columns in every block the miss is 2e-4 .. 1e-3 of the block's largest entry (float64 against float64) — two to ten times
# the bound, under ten times it.  On these five cases they are held to the bounds themselves (test_faint_mistakes_still_fail_the_bounds);
# at ten times the bounds they are caught on the four other cases, and the eleven other mistakes on all nine.
BELOW_TEN_BOUNDS = {(w, n) for w in ("no_upper", "no_mean_lv") for n in ("in_head_wider", "max_waves", "seven", "wide_odd", "wide_humanoid")}
WRONG_CASES = [(w, n) for w in R.WRONG for n in CASES if (w, n) not in BELOW_TEN_BOUNDS]


def test_every_mistake_is_shown_on_at_least_two_cases():
    assert all(sum(1 for w, _ in WRONG_CASES if w == wrong) >= 2 for wrong in R.WRONG) and len(R.WRONG) == 13


@pytest.mark.parametrize("wrong,name", WRONG_CASES)
def test_wrong_references_are_caught(wrong, name):
    """The float32 restatement stands in for the device.  The same `_check` the GPU tests use, at TEN times their bounds, rejects each of:
      no_inv_e        — 1/E dropped from the scale;            inv_max_batch   — 1/max_batch for 1/B;
      half_dmu        — the factor 2 of d/dmu lost;            no_mean_lv      — the + mean(lv) term dropped;
      no_lower        — the lower clamp's sigmoid dropped;     no_upper        — the upper clamp's sigmoid dropped;
      silu_sigmoid    — silu' replaced by sigmoid;             no_reward_scale — reward_scale dropped from the target;
      next_obs_target — next_obs as the target instead of next_obs - obs;
      no_wd           — weight decay dropped;                  wd_weights_only — decay on the weights only;
      wd_shifted      — the decays shifted by one layer;       members_swapped — member 0 given member 1's index row."""
    case, got = make_case(name), _torch_run(name, LR)
    with pytest.raises(AssertionError) as failure:
        _check(f"{name} against {wrong}", case, got, 10 * GRAD_REL, 10 * SQ_REL, wrong=wrong)
    print("rejected:", str(failure.value)[:300])


@pytest.mark.parametrize("wrong,name", sorted(BELOW_TEN_BOUNDS))
def test_faint_mistakes_still_fail_the_bounds(wrong, name):
    """the pairs left out above, at the device tests' own bounds: the float32 restatement, which holds a tenth of them, is rejected"""
    case, got = make_case(name), _torch_run(name, LR)
    with pytest.raises(AssertionError) as failure:
        _check(f"{name} against {wrong}", case, got, GRAD_REL, SQ_REL, wrong=wrong)
    print("rejected:", str(failure.value)[:300])


# ------------------------------------------------------------------------------------------------ the device step
def _ring(ctx, obs, act, rew, nobs):
    from ilswiss_amd.replay import SimpleReplayBuffer
    n = len(rew)
    rb = SimpleReplayBuffer(n, obs.shape[1], act.shape[1], ctx=ctx)
    rb.add_rows(obs, act, rew, np.zeros(n, np.uint8), nobs)
    return rb


def _padding(bnn):
    from ilswiss_amd import _lib
    mx = C.c_double()
    _lib.check(bnn.ctx.lib.ilsx_bnn_debug_padding(bnn.h, C.byref(mx)))
    return mx.value


class _Device:
    """a fresh BNN + BNNTrainer of the case with its parameters and normaliser set, the rows in a replay ring, the index table uploaded"""

    def __init__(self, ctx, case, lr):
        from ilswiss_amd.mbpo import BNN, BNNTrainer
        self.case = case
        self.bnn = BNN(hidden_sizes=case["nh"] * [case["H"]], output_size=case["D"], input_size=case["o"] + case["a"], num_nets=case["E"],
                       ctx=ctx, seed=0)
        self.tr = BNNTrainer(self.bnn, lr=lr, fc_weight_decays=list(case["wd"]), num_elites=min(2, case["E"]), reward_scale=REWARD_SCALE,
                             batch_size=case["max_batch"], holdout_ratio=0.2)
        self.bnn.set_params(case["params"])
        assert all(np.array_equal(g, p) for g, p in zip(self.bnn.get_params(), case["params"]))
        self.bnn.normalizer._set(case["mean"], case["std"])
        self.rb = _ring(ctx, *case["rows"])
        self.table = ctx.from_numpy(case["table"], np.int32)

    def step(self, s):
        """batch s of the case; the loss per member"""
        return self.tr._train_batch(self.rb, self.table, self.case["cols"][s], self.case["table"].shape[1], self.case["batches"][s], want_loss=True)

    def state(self):
        m, v, meta = self.bnn.get_opt()
        return dict(m=m, v=v, t=meta["t"])


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_first_step_gradients_vs_float64(ctx, name):
    """T1 on the device."""
    case = make_case(name)
    dev = _Device(ctx, case, LR)
    loss = dev.step(0)
    refs, worst = _check(name, case, dev.state(), GRAD_REL, SQ_REL)
    print(f"{name}: worst device figures, of the block's largest entry: {worst}")
    _loss_check(name, loss, refs[0]["loss"])
    assert _padding(dev.bnn) == 0.0
    assert max(float(np.abs(g - p).max()) for g, p in zip(dev.bnn.get_params(), case["params"])) > 0.5 * LR      # and the step was taken
    dev.bnn.close()


@gpu
@pytest.mark.parametrize("name", FROZEN)
def test_hip_frozen_three_steps_vs_float64(ctx, name):
    """T2 on the device: B = 96, then 37, then 64 under batch_size = 128 with nothing moving."""
    case = make_case(name, FROZEN_BATCHES, FROZEN_MAX)
    dev = _Device(ctx, case, 0.0)
    losses = [dev.step(s) for s in range(3)]
    for g, p in zip(dev.bnn.get_params(), case["params"]):
        np.testing.assert_array_equal(g, p, err_msg=name)
    refs, worst = _check(f"{name} frozen", case, dev.state(), GRAD_REL, SQ_REL)
    print(f"{name} frozen: worst device figures: {worst}")
    for s in range(3):
        _loss_check(f"{name} frozen step {s}", losses[s], refs[s]["loss"])
    assert _padding(dev.bnn) == 0.0
    dev.bnn.close()


@gpu
@pytest.mark.parametrize("name", SECOND)
def test_hip_second_step_reads_the_updated_transposed_copy(ctx, name):
    """T3 on the device: a second step on new rows against a reference evaluated at the parameters the device reports after step one."""
    B = CASES[name][5]
    case = make_case(name, (B, B))
    dev = _Device(ctx, case, LR)
    dev.step(0)
    after_one = dev.bnn.get_params()
    assert max(float(np.abs(g - p).max()) for g, p in zip(after_one, case["params"])) > 0.5 * LR
    loss = dev.step(1)
    refs, worst = _check(f"{name} second", case, dev.state(), GRAD_REL, SQ_REL, params=[None, after_one])
    print(f"{name} second step: worst device figures: {worst}")
    _loss_check(f"{name} second", loss, refs[1]["loss"])
    assert _padding(dev.bnn) == 0.0
    dev.bnn.close()
