"""A float64 restatement of PPO's minibatch updates (rlkit/torch/algorithms/ppo/ppo.py:57-170) with torch autograd on the CPU, shared by the CPU
and the GPU tests of tests/test_ppo_parity_hip.py:

  * `CASES`: the case matrix, the smallest shapes that still reach each code path of the device step (the two row thresholds of the
    weight-gradient launch are read from csrc/kernels.h);
  * `make_case`: the inputs of a case drawn from its seed — networks whose heads have real spread, trajectories (one of length exactly 2), shuffles;
  * `fixed_f64`: values, GAE returns, per-trajectory standardised advantages (unbiased std) and fixed log-probs in float64;
  * `minibatch_f64`: one minibatch's losses written FORWARDS only — tanh trunk, diagonal-Gaussian log-prob (state-independent log-std parameter, or a
    second head clamped to [LOG_SIG_MIN, LOG_SIG_MAX]), exp(lp - lp_old), min / clamp surrogate, value loss with and without the clip, + l2 * sum p^2 —
    and differentiated by autograd: no backward formula is shared with oracle/ppo.py or kernels.h, tie rules and clamp gates are torch's own;
  * `adam_moments`: what exp_avg / exp_avg_sq hold after the minibatches of a run whose parameters do not move;
  * `blocks` / `block_errors`: per parameter block (each W, each b, the action_log_std block) of the flat ABI vectors.
`wrong=` swaps in a deliberately wrong reference (tests: the bounds tell it from the right one).  Hyper-parameters enter as the fp32 numbers the ABI
carries.  Flat vectors are in the ABI layout: oracle.mlp.unpack, the policy's action_log_std behind its mean net."""
import os
import re

import numpy as np
import torch

from oracle import mlp as omlp
from oracle import tanh_gaussian as otg

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _threshold(name):
    with open(os.path.join(ROOT, "ilswiss_amd", "csrc", "kernels.h")) as f:
        return int(re.search(rf"#define\s+{name}\s+(\d+)", f.read()).group(1))


DW_SPLIT_MIN_ROWS, DW_BIG_MIN_ROWS = _threshold("DW_SPLIT_MIN_ROWS"), _threshold("DW_BIG_MIN_ROWS")
MAX_NORM, B1, B2 = 20.0, 0.9, 0.999          # clip_grad_norm_(20) ; PPO's Adam betas

BASE = dict(epochs=1, cond=False, l2=1e-3, vclip=False, log_std=(-0.5, 0.2), clip_eps=0.2, policy_lr=0.0, value_lr=0.0, rew_mean=0.5, seed=None)


def _case(o, a, hidden, mb, lens, **kw):
    assert min(lens) == 2 and set(kw) <= set(BASE)
    return dict(BASE, o=o, a=a, hidden=hidden, mb=mb, lens=lens, **kw)


_S, _B = DW_SPLIT_MIN_ROWS + 13, DW_BIG_MIN_ROWS + 7
# T1 (frozen parameters: both learning rates 0).  log_std = (mean, std) of the action_log_std entries.
CASES = dict(
    one_row_tail=_case(11, 3, [64, 64], 32, (2, 20, 11), vclip=True),                 # N = 33: one row after a full minibatch
    ragged=_case(17, 6, [128, 128], 48, (2, 31, 50, 30), epochs=2, vclip=True),       # N = 48 * 2 + 17, two epochs
    spec=_case(11, 3, [256, 256], 64, (2, 90, 60, 48)),                               # exp_specs/ppo/ppo_hopper_hip.yaml's minibatch, N = 200
    wide=_case(376, 17, [256, 256], 50, (2, 40, 28)),                                 # input in several slabs, heads past one 16-column group
    one_hidden=_case(11, 3, [64], 64, (2, 30, 28), log_std=(-3.0, 0.1)),              # norm clip active
    three_hidden=_case(11, 3, [64, 64, 64], 64, (2, 30, 28), log_std=(-3.0, 0.1)),    # ... and both skip ranges of k_ppo_norm
    unequal=_case(11, 3, [200, 100], 32, (2, 40, 28)),                                # padded units never show in the ABI vectors
    cond_std=_case(11, 3, [64, 64], 48, (2, 31, 50, 30), cond=True),                  # log-std head, rows on both sides of the clamp's upper end
    l2=_case(11, 3, [64, 64], 48, (2, 40, 28), l2=0.05),
    row_split=_case(17, 6, [128, 128], _S, (2, 500, 300, _S + 37 - 802)),             # one minibatch just above the threshold, ragged last row
    dw_big=_case(11, 3, [64, 64], _B, (2, 1500, 1100, 900, _B + 37 - 3502)),          #   range, then 37 rows
)
# T2 (the second of two real steps, by subtraction): the g7c settings — rows cross the ratio and the value windows
CLIP_CASES = dict(
    clip=_case(11, 3, [64, 64], 256, (2, 90, 60, 48), epochs=2, clip_eps=0.1, policy_lr=3e-3, value_lr=2e-3, rew_mean=0.0, seed=8127),
    clip_vclip=_case(11, 3, [64, 64], 256, (2, 90, 60, 48), epochs=2, clip_eps=0.1, policy_lr=3e-3, value_lr=2e-3, rew_mean=0.0, vclip=True, seed=8127),
)
ALL = dict(CASES, **CLIP_CASES)
LS_SCALE, LS_BIAS = 400.0, (2.0, 0.5, 1.5)      # cond_std: the log-std head's scale and the bias pattern cycled over the action dimensions


def hyper(c):
    """PPOOracle / PPO keyword arguments of a case."""
    return dict(reward_scale=1.0, discount=0.99, clip_eps=c["clip_eps"], policy_lr=c["policy_lr"], value_lr=c["value_lr"], gae_tau=0.95,
                value_l2_reg=c["l2"], mini_batch_size=c["mb"], update_epoch=c["epochs"], use_value_clip=c["vclip"], conditioned_std=c["cond"])


def make_case(name):
    """dict(pi0, vf0, trajs, perms [epochs, N], N) of a case.  Heads U(+-0.2) / U(+-0.3) instead of the 1e-4 / 3e-3 of a fresh network: means and
    values with real spread.  conditioned_std: the log-std head (U(+-1e-3)) scaled by 400 with LS_BIAS cycled onto its bias — raw log-stds spread over
    a few units around LOG_SIG_MAX = 2.  The lower end is left alone: at log_std = -20 a log-prob is (a - mu)^2 * e^40 / 2, the ratio the exponential
    of a difference of such numbers, and no fp32 evaluation holds either."""
    c = ALL[name]
    o, a, hidden = c["o"], c["a"], c["hidden"]
    rng = np.random.default_rng(c["seed"] if c["seed"] is not None else 8000 + list(ALL).index(name))
    vf0 = omlp.init_mlp(rng, o, hidden, 1, init_w=0.3)
    if c["cond"]:
        pi0 = omlp.init_mlp(rng, o, hidden, a, init_w=1e-3, n_heads=2)
        lay = omlp.unpack(pi0, o, hidden, a, n_heads=2)          # views into pi0
        for x in lay[-2]:
            x *= F32(200.0)
        for x in lay[-1]:
            x *= F32(LS_SCALE)
        lay[-1][1][:] += np.asarray([LS_BIAS[j % len(LS_BIAS)] for j in range(a)], F32)
    else:
        pi0 = np.concatenate([omlp.init_mlp(rng, o, hidden, a, init_w=0.2), rng.normal(*c["log_std"], a).astype(F32)])
    trajs = [dict(observations=rng.normal(0, 1, (L, o)).astype(F32), actions=rng.normal(0, 0.7, (L, a)).astype(F32),
                  rewards=rng.normal(c["rew_mean"], 1.0, (L, 1)).astype(F32)) for L in c["lens"]]
    N = sum(c["lens"])
    perms = np.stack([rng.permutation(N) for _ in range(c["epochs"])]).astype(np.int32)
    return dict(pi0=pi0, vf0=vf0, trajs=trajs, perms=perms, N=N)


def minibatches(c, perms):
    """index lists of every minibatch of a run, in order"""
    return [perm[s:s + c["mb"]] for perm in perms for s in range(0, len(perm), c["mb"])]


# ------------------------------------------------------------------------------------------------ networks
def _t64(x):
    return torch.tensor(np.asarray(x, F32).astype(np.float64))


def _layers64(flat, o, hidden, out, n_heads=1, requires_grad=False):
    return [(_t64(W).requires_grad_(requires_grad), _t64(b).requires_grad_(requires_grad)) for W, b in omlp.unpack(np.asarray(flat, F32), o, hidden, out, n_heads)]


def _heads(layers, x, n_hidden):
    h = x
    for W, b in layers[:n_hidden]:
        h = torch.tanh(h @ W.T + b)
    return [h @ W.T + b for W, b in layers[n_hidden:]]


def _policy_params(c, pi, requires_grad=False):
    """(layers, action_log_std or None) of the flat policy vector"""
    n_ls = 0 if c["cond"] else c["a"]
    pi = np.asarray(pi, F32)
    layers = _layers64(pi[:pi.size - n_ls], c["o"], c["hidden"], c["a"], 2 if c["cond"] else 1, requires_grad)
    return layers, (_t64(pi[pi.size - n_ls:]).requires_grad_(requires_grad) if n_ls else None)


def _log_prob(c, layers, ls_param, x, act, gate=True):
    """diagonal Gaussian, un-squashed (distributions.py:43-50): 0.5 * log(2 pi) enters once per row.  Returns (lp [rows], raw log-std or None)."""
    outs = _heads(layers, x, len(c["hidden"]))
    mu, lsr = outs[0], None
    if c["cond"]:
        lsr = outs[1]
        ls = torch.clamp(lsr, otg.LOG_SIG_MIN, otg.LOG_SIG_MAX)
        if not gate:
            ls = lsr + (ls - lsr).detach()
    else:
        ls = ls_param.expand_as(mu)
    return -0.5 * torch.sum((act - mu) ** 2 / torch.exp(2 * ls), 1) - (torch.sum(ls, 1) + otg.HALF_LOG_2PI), lsr


def _flat(grads):
    return np.concatenate([g.numpy().ravel() for g in grads])


# ------------------------------------------------------------------------------------------------ calc_adv
def gae_f64(values, rewards, lens, discount, tau, reward_scale=1.0):
    """ppo.py:73-86 in float64: per trajectory, zero bootstrap, returns = V + A, advantages standardised with the unbiased std."""
    g, lam, rs = (float(F32(x)) for x in (discount, tau, reward_scale))
    R, A, off = np.empty_like(values), np.empty_like(values), 0
    for L in lens:
        v, r = values[off:off + L], rs * rewards[off:off + L]
        adv, nv, na = np.empty(L), 0.0, 0.0
        for i in reversed(range(L)):
            adv[i] = r[i] + g * nv - v[i] + g * lam * na
            nv, na = v[i], adv[i]
        R[off:off + L] = v + adv
        A[off:off + L] = (adv - adv.mean()) / adv.std(ddof=1)
        off += L
    return R, A


def fixed_f64(c, case, pi, vf):
    """What one train_step fixes before its minibatches, at the parameters (pi, vf): dict(obs, act [N, .], values, returns, adv, lp_old [N]), float64."""
    kw = hyper(c)
    obs = np.concatenate([t["observations"] for t in case["trajs"]]).astype(np.float64)
    act = np.concatenate([t["actions"] for t in case["trajs"]]).astype(np.float64)
    rew = np.concatenate([t["rewards"] for t in case["trajs"]]).astype(np.float64).ravel()
    with torch.no_grad():
        values = _heads(_layers64(vf, c["o"], c["hidden"], 1), torch.tensor(obs), len(c["hidden"]))[0][:, 0].numpy()
        lp_old = _log_prob(c, *_policy_params(c, pi), torch.tensor(obs), torch.tensor(act))[0].numpy()
    R, A = gae_f64(values, rew, c["lens"], kw["discount"], kw["gae_tau"], kw["reward_scale"])
    return dict(obs=obs, act=act, values=values, returns=R, adv=A, lp_old=lp_old)


# ------------------------------------------------------------------------------------------------ one minibatch
def _both_on_ties(pick, x, y):
    """min / max with the value of `pick` whose tie sends the WHOLE gradient down both arguments (the wrong reference 'tie')"""
    return torch.where(x == y, x + y - y.detach(), pick(x, y))


def minibatch_f64(c, fx, idx, pi, vf, wrong=None):
    """Gradients of one minibatch (rows `idx` of the fixed quantities `fx`) at the parameters (pi, vf), float64, flat ABI layout.
    Returns dict(vf_grad (with the L2 term), pi_grad (before the norm clip), norm, coef = min(1, 20 / (norm + 1e-6)), and per row: ratio, dv = v - v_old,
    l1, l2 (the two value-loss terms), lsr (raw log-std, conditioned_std)).
    wrong: 'tie' (ties of min / max pass the whole gradient twice, i.e. without torch's weight of 1/2) | 'gate' (every clamp's derivative is 1) |
    'norm1' / 'norm2' (the first / second hidden -> hidden matrix counted twice in the norm)."""
    assert wrong in (None, "tie", "gate", "norm1", "norm2")
    eps, l2 = float(F32(c["clip_eps"])), float(F32(c["l2"]))
    idx = np.asarray(idx)
    x, act = torch.tensor(fx["obs"][idx]), torch.tensor(fx["act"][idx])
    R, A, v_old, lp_old = (torch.tensor(fx[k][idx]) for k in ("returns", "adv", "values", "lp_old"))
    tmin = (lambda p, q: _both_on_ties(torch.min, p, q)) if wrong == "tie" else torch.min
    tmax = (lambda p, q: _both_on_ties(torch.max, p, q)) if wrong == "tie" else torch.max

    def clamp(t, lo, hi):
        y = torch.clamp(t, lo, hi)
        return t + (y - t).detach() if wrong == "gate" else y

    # value net (ppo.py:136-153)
    vl = _layers64(vf, c["o"], c["hidden"], 1, requires_grad=True)
    vp = [p for Wb in vl for p in Wb]
    v = _heads(vl, x, len(c["hidden"]))[0][:, 0]
    l1 = (v - R) ** 2
    v_clip = v_old + clamp(v - v_old, -eps, eps)
    l2t = (v_clip - R) ** 2
    vloss = (tmax(l1, l2t) if c["vclip"] else l1).mean() + l2 * sum((p ** 2).sum() for p in vp)
    vf_grad = _flat(torch.autograd.grad(vloss, vp))
    # policy (ppo.py:155-170)
    layers, ls_param = _policy_params(c, pi, requires_grad=True)
    pp = [p for Wb in layers for p in Wb] + ([ls_param] if ls_param is not None else [])
    lp, lsr = _log_prob(c, layers, ls_param, x, act, gate=wrong != "gate")
    ratio = torch.exp(lp - lp_old)
    ploss = -tmin(ratio * A, clamp(ratio, 1.0 - eps, 1.0 + eps) * A).mean()
    pi_grad = _flat(torch.autograd.grad(ploss, pp))
    sq = float(np.sum(pi_grad ** 2))
    if wrong in ("norm1", "norm2"):
        sq += float(np.sum(pi_grad[dict(blocks(c))["W" + wrong[-1]]] ** 2))
    norm = float(np.sqrt(sq))
    return dict(vf_grad=vf_grad, pi_grad=pi_grad, norm=norm, coef=min(1.0, MAX_NORM / (norm + 1e-6)), ratio=ratio.detach().numpy(),
                dv=(v - v_old).detach().numpy(), l1=l1.detach().numpy(), l2=l2t.detach().numpy(), lsr=None if lsr is None else lsr.detach().numpy())


def adam_moments(grads):
    """(exp_avg, exp_avg_sq) after Adam (betas 0.9 / 0.999, zero start) has seen `grads` in order"""
    m, v = np.zeros_like(grads[0]), np.zeros_like(grads[0])
    for g in grads:
        m, v = B1 * m + (1 - B1) * g, B2 * v + (1 - B2) * g * g
    return m, v


def frozen_run_f64(c, case, wrong=None):
    """T1: every minibatch of a run at the initial parameters.  Returns (fixed quantities, [minibatch_f64 ...]).  wrong = 'last_scale': the last
    minibatch's loss gradients scaled by rows / mini_batch_size, what a mean taken over mini_batch_size rows gives on a ragged minibatch."""
    fx = fixed_f64(c, case, case["pi0"], case["vf0"])
    mbs = minibatches(c, case["perms"])
    out = [minibatch_f64(c, fx, idx, case["pi0"], case["vf0"], wrong=None if wrong == "last_scale" else wrong) for idx in mbs]
    if wrong == "last_scale":
        s, last = len(mbs[-1]) / c["mb"], out[-1]
        reg = 2 * float(F32(c["l2"])) * case["vf0"].astype(np.float64)
        last["vf_grad"] = (last["vf_grad"] - reg) * s + reg
        last["pi_grad"], last["norm"] = last["pi_grad"] * s, last["norm"] * s
        last["coef"] = min(1.0, MAX_NORM / (last["norm"] + 1e-6))
    return fx, out


# ------------------------------------------------------------------------------------------------ per block
def blocks(c, value=False):
    """[(name, slice)] of a flat ABI vector: each W and each b, and the policy's action_log_std block"""
    heads = 1 if value or not c["cond"] else 2
    out, off = [], 0
    for li, (r, k) in enumerate(omlp.layer_shapes(c["o"], c["hidden"], 1 if value else c["a"], heads)):
        out.append((f"W{li}", slice(off, off + r * k)))
        off += r * k
        out.append((f"b{li}", slice(off, off + r)))
        off += r
    if not value and not c["cond"]:
        out.append(("log_std", slice(off, off + c["a"])))
    return out


def block_errors(got, ref, c, value=False):
    """[(name, max|got - ref|, max|ref|)] per parameter block"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape == (blocks(c, value)[-1][1].stop,)
    return [(nm, float(np.abs(got[s] - ref[s]).max()), float(np.abs(ref[s]).max())) for nm, s in blocks(c, value)]
