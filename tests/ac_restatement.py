"""A float64 restatement of the three steps that share AcAgent in csrc/ilsx_ac.hip and run in shipped specs — TD3 (td3.py:72-124), HER-TD3
(her/td3.py:100-170, as the comment block above k_her_target_action states it) and SAC with a V function (sac/sac.py:70-179) — with torch
autograd on the CPU, shared by the CPU and the GPU tests of tests/test_ac_parity_hip.py:

  * `CASES` (one step), `FROZEN` (three steps at zero learning rates, B = 96, 37, 64 under max_batch = 128) and `DELAY` (TD3's delayed update):
    the smallest shapes at which the device step changes path; the two row thresholds of the weight-gradient launch are read from csrc/kernels.h;
  * `make_case`: the inputs of a case drawn from its seed — online nets whose heads have real spread, TARGET nets that are independent draws
    (they differ from the online nets by as much as the weights themselves), batches with mixed terminals, explicit noise — with every row
    that breaks a kink condition (`violations`) drawn again until none is left; HER's clip_return bounds are quantiles of the float64 targets;
  * `step_f64`: one step's losses written FORWARDS only and differentiated by autograd, so that no backward formula is shared with
    oracle/td3.py, oracle/sac_v.py or kernels.h.  Target blocks are given separately from the online ones, and so are the critics of the
    actor phase (`actor=`: the policy loss of all three algorithms is evaluated with the critics AFTER their Adam step).  Returns the
    gradient of every trainable net in the flat ABI layout and every per-row quantity a kink depends on;
  * `adam_moments`: what exp_avg / exp_avg_sq hold after Adam has seen a list of gradients from zero moments;
  * `blocks` / `block_errors`: per parameter block (each W, each b) of a flat ABI vector.
`wrong=` swaps in a deliberately wrong reference (tests: the bounds tell it from the right one).  Hyper-parameters enter as the fp32 numbers the
ABI carries.  Flat vectors are in the ABI layout of oracle.mlp.unpack."""
import functools
import os
import re

import numpy as np
import torch

from oracle import mlp as omlp
from oracle import tanh_gaussian as otg
from oracle.sac_v import SacVOracle
from oracle.td3 import TD3Oracle

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B2 = 0.999


def _threshold(name):
    with open(os.path.join(ROOT, "ilswiss_amd", "csrc", "kernels.h")) as f:
        return int(re.search(rf"#define\s+{name}\s+(\d+)", f.read()).group(1))


DW_SPLIT_MIN_ROWS, DW_BIG_MIN_ROWS = _threshold("DW_SPLIT_MIN_ROWS"), _threshold("DW_BIG_MIN_ROWS")
assert (DW_SPLIT_MIN_ROWS, DW_BIG_MIN_ROWS) == (1024, 4096)      # the case table below is written for these

ALGOS = ("td3", "her", "sacv")
NETS = dict(td3=("q1", "q2", "pi"), her=("q1", "q2", "pi"), sacv=("q1", "q2", "vf", "pi"))            # trainable blocks, arena order
TARGETS = dict(td3=("tq1", "tq2", "tpi"), her=("tq1", "tq2", "tpi"), sacv=("tvf",))
ONLINE_OF = dict(tq1="q1", tq2="q2", tpi="pi", tvf="vf")
CRITICS = dict(td3=("q1",), her=("q1",), sacv=("q1", "q2"))                                          # what the actor phase reads after its update
WRONG = ("inv_b", "td3_half", "sacv_double", "no_max_act", "online_targets", "l2_over_b", "unclipped", "v_post", "pi_pre", "swap_reg")
KINK_REL, LS_MARGIN = 1e-3, 1e-3

# per algorithm: the settings every case of it runs with unless the case says otherwise
HYPER = dict(
    td3=dict(reward_scale=5.0, discount=0.99, sigma=0.4, noise_clip=0.5, max_act=2.0, tau=0.005, period=2, beta_1=0.9, lr=1e-3, out_act="tanh"),
    her=dict(reward_scale=5.0, discount=0.98, sigma=1.2, noise_clip=0.0, max_act=1.5, tau=0.005, period=2, beta_1=0.9, lr=1e-3, out_act="tanh", gd=3),
    sacv=dict(reward_scale=5.0, discount=0.99, alpha=0.2, w_mu=0.03, w_std=0.1, tau=0.01, beta_1=0.9, lr=1e-3),
)
# shape -> (o, a, hidden, hidden activation, max_batch, (B per step ...)); every algorithm runs every shape
SHAPES = dict(
    h64=(11, 3, [64, 64], "relu", 64, (37,)),                  # generic kernels (cs = 1), ragged B
    one_row=(11, 3, [64, 64], "relu", 32, (1,)),
    h128_full=(17, 6, [128, 128], "relu", 256, (256,)),        # column split cs = 2
    h128_part=(17, 6, [128, 128], "relu", 256, (100,)),        #   every slab stride differs from B
    h256_full=(17, 6, [256, 256], "relu", 256, (256,)),        # column split cs = 4
    h256_part=(17, 6, [256, 256], "relu", 256, (100,)),
    one_hidden=(11, 3, [64], "relu", 64, (37,)),
    three_hidden=(11, 3, [64, 64, 64], "relu", 64, (37,)),
    tanh_hidden=(11, 3, [64, 64], "tanh", 64, (37,)),
    pendulum=(3, 1, [64, 64], "relu", 64, (37,)),              # a single action column for dx_cols
    wide=(376, 17, [256, 256], "relu", 64, (64,)),             # input in several slabs, a past one 16-column group
    dw_1024=(11, 3, [64, 64], "relu", 1024, (1024,)),          # k_mlp_bwd_dw<false,2,4> + k_dw_reduce at its first row count
    dw_1100=(11, 3, [64, 64], "relu", 1100, (1100,)),          #   ragged last row range
    dw_4096=(11, 3, [64, 64], "relu", 4096, (4096,)),          # k_dw_big at its first row count
)
IDENTITY_OUT = ("h128_part", "one_hidden", "pendulum", "dw_1100", "h256_full")     # TD3 / HER cases with the identity output activation
FROZEN_SHAPES = dict(frozen64=(11, 3, [64, 64], "relu", 128, (96, 37, 64)), frozen128=(17, 6, [128, 128], "relu", 128, (96, 37, 64)),
                     frozen256=(17, 6, [256, 256], "relu", 128, (96, 37, 64)))
DELAY_SHAPES = dict(delay64=(11, 3, [64, 64], "relu", 64, (37, 37, 37)), delay128=(17, 6, [128, 128], "relu", 128, (100, 100, 100)))


def _table(shapes, algos, first_seed, **over):
    out = {}
    for algo in algos:
        for shape, (o, a, hidden, act, mb, Bs) in shapes.items():
            c = dict(HYPER[algo], algo=algo, shape=shape, o=o, a=a, hidden=hidden, act=act, max_batch=mb, Bs=Bs, **over)
            if algo != "sacv" and shape in IDENTITY_OUT:
                c["out_act"] = "identity"
            if algo == "her":
                c["gd"] = min(c["gd"], o - 2)              # pendulum: observation 2 | goal 1
            c["seed"] = first_seed + len(out)
            out[f"{algo}/{shape}"] = c
    return out


CASES = _table(SHAPES, ALGOS, 9100)
# SAC-V with beta_1 = 0: exp_avg is the gradient itself
CASES.update({k + "/b0": dict(CASES[k], beta_1=0.0, seed=CASES[k]["seed"] + 500) for k in ("sacv/h64", "sacv/h128_part", "sacv/dw_1100")})
FROZEN = _table(FROZEN_SHAPES, ALGOS, 9300, lr=0.0, tau=0.0, period=1)      # nothing moves: tau = 0 keeps the targets where they were set
DELAY = _table(DELAY_SHAPES, ("td3", "her"), 9400)
ALL = dict(CASES, **FROZEN, **DELAY)
# one row is all a one_row case has: seeds whose row has sigma * eps past max_act in one entry and inside in another (HER), a raw log-std
# above the clamp in one entry and inside in another (SAC-V)
SEEDS = {"her/one_row": 9604, "sacv/one_row": 9603}
for _k, _s in SEEDS.items():
    ALL[_k]["seed"] = _s


def f32(x):
    return float(F32(x))


def net_dims(c, net):
    """(input, output, heads) of a block"""
    net = ONLINE_OF.get(net, net)
    if net in ("q1", "q2"):
        return c["o"] + c["a"], 1, 1
    if net == "vf":
        return c["o"], 1, 1
    return c["o"], c["a"], 2 if c["algo"] == "sacv" else 1


# ------------------------------------------------------------------------------------------------ networks in float64
def _t64(x):
    return torch.tensor(np.asarray(x, F32).astype(np.float64))


def _layers(c, net, flat, requires_grad=False):
    i, out, heads = net_dims(c, net)
    return [(_t64(W).requires_grad_(requires_grad), _t64(b).requires_grad_(requires_grad))
            for W, b in omlp.unpack(np.asarray(flat, F32), i, c["hidden"], out, heads)]


def _fwd(c, layers, *xs):
    h = torch.cat(xs, 1) if len(xs) > 1 else xs[0]
    act = torch.tanh if c["act"] == "tanh" else torch.relu
    n = len(c["hidden"])
    for W, b in layers[:n]:
        h = act(h @ W.T + b)
    outs = [h @ W.T + b for W, b in layers[n:]]
    return outs if len(outs) > 1 else outs[0]


def _grad(loss, layers):
    return np.concatenate([g.numpy().ravel() for g in torch.autograd.grad(loss, [p for Wb in layers for p in Wb], retain_graph=True)])


def _np(**rows):
    return {k: v.detach().numpy().copy() for k, v in rows.items()}


def _batch64(batch):
    B = batch["observations"].shape[0]
    s, a, s2 = (_t64(batch[k]) for k in ("observations", "actions", "next_observations"))
    return s, a, _t64(batch["rewards"]).reshape(B), _t64(batch["terminals"]).reshape(B), s2, _t64(batch["eps"])


# ------------------------------------------------------------------------------------------------ TD3 and HER-TD3
def _td3_f64(c, P, batch, actor, wrong):
    her = c["algo"] == "her"
    s, a, r, d, s2, eps = _batch64(batch)
    B = s.shape[0]
    rs, gamma, sigma, clip, max_act = (f32(c[k]) for k in ("reward_scale", "discount", "sigma", "noise_clip", "max_act"))
    out_act = torch.tanh if c["out_act"] == "tanh" else (lambda z: z)
    T = {k: P[ONLINE_OF[k]] if wrong == "online_targets" else P[k] for k in TARGETS[c["algo"]]}
    with torch.no_grad():
        noise = sigma * eps
        if her:      # the clamped noise alone is the target action; the target policy's output has no effect
            a2 = torch.clamp(noise, -max_act, max_act)
        else:        # td3.py:84-85 with the noisy target module: max_act * out(pi_T(s')) + clip(sigma * eps), not clipped again
            a2 = max_act * out_act(_fwd(c, _layers(c, "tpi", T["tpi"]), s2)) + torch.clamp(noise, -clip, clip)
        tq1, tq2 = (_fwd(c, _layers(c, k, T[k]), s2, a2)[:, 0] for k in ("tq1", "tq2"))
        tq_raw = torch.min(tq1, tq2)
        tq = torch.clamp(tq_raw, f32(c["clip_l"]), f32(c["clip_r"])) if her and wrong != "unclipped" else tq_raw
        y = rs * r + (1.0 - d) * gamma * tq
    grads, rows = {}, dict(noise=noise, tq_raw=tq_raw, tq1=tq1, tq2=tq2, y=y)
    for k in ("q1", "q2"):      # nn.MSELoss: the mean square, no 1/2
        lay = _layers(c, k, P[k], True)
        q = _fwd(c, lay, s, a)[:, 0]
        grads[k] = _grad((0.5 if wrong == "td3_half" else 1.0) * ((q - y) ** 2).mean(), lay)
        rows[k] = q
    # actor phase: -mean Q1(s, pi(s)) with the critic the actor phase sees
    q1a = _layers(c, "q1", P["q1"] if actor is None or wrong == "pi_pre" else actor["q1"])
    lay = _layers(c, "pi", P["pi"], True)
    t = out_act(_fwd(c, lay, s))
    pa = t + ((max_act - 1.0) * t).detach() if wrong == "no_max_act" else max_act * t
    qn = _fwd(c, q1a, s, pa)[:, 0]
    loss = -qn.mean()
    if her:
        loss = loss + ((pa ** 2).sum() / B if wrong == "l2_over_b" else (pa ** 2).mean())
    grads["pi"] = _grad(loss, lay)
    rows.update(qn=qn, pa=pa)
    return grads, rows, ("q1", "q2", "tq1", "tq2", "qn")


# ------------------------------------------------------------------------------------------------ SAC with a V function
def _sacv_f64(c, P, batch, actor, wrong):
    s, a, r, d, s2, eps = _batch64(batch)
    rs, gamma, alpha, w_mu, w_std = (f32(c[k]) for k in ("reward_scale", "discount", "alpha", "w_mu", "w_std"))
    if wrong == "swap_reg":
        w_mu, w_std = w_std, w_mu
    with torch.no_grad():
        tv = _fwd(c, _layers(c, "tvf", P["vf"] if wrong == "online_targets" else P["tvf"]), s2)[:, 0]
        y = rs * r + (1.0 - d) * gamma * tv
    grads, rows = {}, dict(tv=tv, y=y)
    for k in ("q1", "q2"):      # 0.5 * mean(.)^2
        lay = _layers(c, k, P[k], True)
        q = _fwd(c, lay, s, a)[:, 0]
        grads[k] = _grad((1.0 if wrong == "sacv_double" else 0.5) * ((q - y) ** 2).mean(), lay)
        rows[k] = q
    # the one policy sample of the step: tanh-Gaussian, log-std clamped as in oracle.tanh_gaussian; 0.5 * log(2 pi) enters once per row
    pl = _layers(c, "pi", P["pi"], True)
    mu, lsr = _fwd(c, pl, s)
    ls = torch.clamp(lsr, otg.LOG_SIG_MIN, otg.LOG_SIG_MAX)
    z = mu + torch.exp(ls) * eps
    an = torch.tanh(z)
    logp = -0.5 * torch.sum((z - mu) ** 2 / torch.exp(2 * ls), 1) - (torch.sum(ls, 1) + otg.HALF_LOG_2PI) - torch.sum(torch.log(1 - an * an + otg.EPS), 1)
    pre = {k: _layers(c, k, P[k]) for k in ("q1", "q2")}
    post = pre if actor is None else {k: _layers(c, k, actor[k]) for k in ("q1", "q2")}
    q1n0, q2n0 = (_fwd(c, pre[k], s, an)[:, 0] for k in ("q1", "q2"))
    q1n, q2n = (_fwd(c, post[k], s, an)[:, 0] for k in ("q1", "q2"))
    # V against min(Q1, Q2)(s, a~) - alpha * logp with the critics BEFORE their update
    vt = ((torch.min(q1n, q2n) if wrong == "v_post" else torch.min(q1n0, q2n0)) - alpha * logp).detach()
    vl = _layers(c, "vf", P["vf"], True)
    v = _fwd(c, vl, s)[:, 0]
    grads["vf"] = _grad(0.5 * ((v - vt) ** 2).mean(), vl)
    # the policy against the critics AFTER their update, same sample; regularisers as means over all B * A entries
    qmin = torch.min(q1n0, q2n0) if wrong == "pi_pre" else torch.min(q1n, q2n)
    grads["pi"] = _grad((alpha * logp - qmin).mean() + w_mu * (mu ** 2).mean() + w_std * (ls ** 2).mean(), pl)
    rows.update(v=v, q1n0=q1n0, q2n0=q2n0, q1n=q1n, q2n=q2n, logp=logp, lsr=lsr, an=an)
    return grads, rows, ("q1", "q2", "tv", "v", "q1n0", "q2n0", "q1n", "q2n")


def step_f64(c, P, batch, actor=None, wrong=None):
    """One step at the blocks `P` (online and target blocks by name) on `batch` (the five transition arrays and `eps`).  actor: the critics the
    actor phase evaluates ({"q1": flat} for TD3 / HER, q1 and q2 for SAC-V), None = the ones in `P`.  Returns dict(grads {net: flat gradient},
    rows {name: per-row float64 array}, max_q = the largest |Q| or |V| of the batch)."""
    assert wrong is None or wrong in WRONG
    grads, rows, qs = (_sacv_f64 if c["algo"] == "sacv" else _td3_f64)(c, P, batch, actor, wrong)
    if wrong == "inv_b":
        grads = {k: g * (batch["observations"].shape[0] / c["max_batch"]) for k, g in grads.items()}
    rows = _np(**rows)
    return dict(grads=grads, rows=rows, max_q=max(float(np.abs(rows[k]).max()) for k in qs))


def adam_moments(grads, b1):
    """(exp_avg, exp_avg_sq) after Adam (betas b1 / 0.999, zero start) has seen `grads` in order"""
    b1 = f32(b1)
    m, v = np.zeros_like(grads[0]), np.zeros_like(grads[0])
    for g in grads:
        m, v = b1 * m + (1 - b1) * g, B2 * v + (1 - B2) * g * g
    return m, v


# ------------------------------------------------------------------------------------------------ kink conditions
def violations(c, ref, factor=1.0):
    """Per row: does it break a kink condition of the float64 step `ref`?  Margin: factor * 1e-3 of the largest |Q| of the batch —
    |Q1 - Q2|(s, a~) at the pre- and the post-update critics (SAC-V), distance to a clip_return bound (HER), distance of |sigma * eps| to the
    noise bound (TD3: noise_clip, HER: max_act); raw log-std: factor * 1e-3 from a clamp bound."""
    rows, m = ref["rows"], factor * KINK_REL * ref["max_q"]
    if c["algo"] == "sacv":
        bad = (np.abs(rows["q1n0"] - rows["q2n0"]) < m) | (np.abs(rows["q1n"] - rows["q2n"]) < m)
        near = np.minimum(np.abs(rows["lsr"] - otg.LOG_SIG_MAX), np.abs(rows["lsr"] - otg.LOG_SIG_MIN)) < factor * LS_MARGIN
        return bad | near.any(1)
    bound = f32(c["max_act"] if c["algo"] == "her" else c["noise_clip"])
    bad = (np.abs(np.abs(rows["noise"]) - bound) < m).any(1)
    if c["algo"] == "her":
        bad |= (np.abs(rows["tq_raw"] - f32(c["clip_l"])) < m) | (np.abs(rows["tq_raw"] - f32(c["clip_r"])) < m)
    return bad


# ------------------------------------------------------------------------------------------------ inputs
LS_BIAS, LS_STD, MEAN_STD = (2.2, 0.8, 1.6), 0.7, 0.5      # SAC-V heads: raw log-std = LS_BIAS (cycled over the action dimensions) + a spread of 0.7


def _init_block(c, net, rng):
    i, out, heads = net_dims(c, net)
    if ONLINE_OF.get(net, net) != "pi":
        p = omlp.init_mlp(rng, i, c["hidden"], out, init_w=0.3)
        if net == "vf":      # V starts a unit below its target: the head bias's gradient, mean(v - v_target), is then no residue of cancellation
            p[-1] -= F32(1.0)
        return p
    if heads == 1:
        return omlp.init_mlp(rng, i, c["hidden"], out, init_w=0.2)
    # tanh-Gaussian policy: each head row rescaled so that over N(0, 1) observations the mean has a standard deviation of MEAN_STD around 0
    # and the raw log-std one of LS_STD around LS_BIAS: rows on both sides of LOG_SIG_MAX = 2 at every width and input size.  The lower
    # end is left alone: at sigma = e^-20 the fp32 (mu - z)^2 / sigma^2 of the reference's log-prob is a rounding residue.
    p = omlp.init_mlp(rng, i, c["hidden"], out, init_w=1e-3, n_heads=2)
    lay = omlp.unpack(p, i, c["hidden"], out, n_heads=2)          # views into p
    outs, _ = omlp.forward(p, rng.normal(0, 1, (256, i)).astype(F32), i, c["hidden"], out, n_heads=2, act=omlp.TANH if c["act"] == "tanh" else omlp.RELU)
    for (W, b), y, std, centre in ((lay[-2], outs[0], MEAN_STD, np.zeros(out)), (lay[-1], outs[1], LS_STD, np.asarray([LS_BIAS[j % len(LS_BIAS)] for j in range(out)]))):
        k = std / (y - b).std(0)
        W *= k[:, None].astype(F32)
        b[:] = (centre - k * (y - b).mean(0)).astype(F32)
    return p


def _draw_rows(c, rng, n):
    """n transitions with their noise.  SAC-V's noise is U(+-0.3): at the clamped sigma = e^2 a N(0, 1) draw saturates tanh, where
    log(1 - a^2 + 1e-6) magnifies one ulp of tanh by up to 1e5 and no fp32 evaluation of log pi holds the bounds."""
    o, a = c["o"], c["a"]
    eps = rng.uniform(-0.3, 0.3, (n, a)) if c["algo"] == "sacv" else rng.normal(0, 1, (n, a))
    return dict(observations=rng.normal(0, 1, (n, o)).astype(F32), actions=np.tanh(rng.normal(0, 1, (n, a))).astype(F32),
                rewards=rng.normal(0, 1, (n, 1)).astype(F32), terminals=(rng.random((n, 1)) < 0.25).astype(F32),
                next_observations=rng.normal(0, 1, (n, o)).astype(F32), eps=eps.astype(F32))


def hyper(c):
    """keyword arguments of the oracle of a case (the device trainers take the same numbers under their own names)"""
    if c["algo"] == "sacv":
        return dict(reward_scale=c["reward_scale"], discount=c["discount"], alpha=c["alpha"], policy_lr=c["lr"], qf_lr=c["lr"], vf_lr=c["lr"],
                    soft_target_tau=c["tau"], policy_mean_reg_weight=c["w_mu"], policy_std_reg_weight=c["w_std"], beta_1=c["beta_1"],
                    hidden_activation=c["act"])
    kw = dict(reward_scale=c["reward_scale"], discount=c["discount"], policy_lr=c["lr"], qf_lr=c["lr"], policy_and_target_update_period=c["period"],
              soft_target_tau=c["tau"], policy_noise=c["sigma"], policy_noise_clip=c["noise_clip"], max_act=c["max_act"],
              output_activation=c["out_act"], hidden_activation=c["act"])
    if c["algo"] == "her":
        kw.update(her=True, clip_return_l=c["clip_l"], clip_return_r=c["clip_r"])
    return kw


def make_oracle(c, P):
    """the numpy fp32 oracle of a case at the blocks P, targets included"""
    if c["algo"] == "sacv":
        return SacVOracle(c["o"], c["a"], c["hidden"], P["pi"], P["q1"], P["q2"], P["vf"], target_vf=P["tvf"], **hyper(c))
    return TD3Oracle(c["o"], c["a"], c["hidden"], P["pi"], P["q1"], P["q2"], target_pi=P["tpi"], target_q1=P["tq1"], target_q2=P["tq2"], **hyper(c))


def oracle_step(orc, batch):
    return orc.train_step({k: v for k, v in batch.items() if k != "eps"}, batch["eps"])


def _post_critics(c, P, batch):
    """the critics after the fp32 oracle's first step on `batch` (what the actor phase of that step evaluates)"""
    if c["lr"] == 0.0:
        return None
    orc = make_oracle(c, P)
    oracle_step(orc, batch)
    return {k: getattr(orc, k).copy() for k in CRITICS[c["algo"]]}


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(settings, dict(P = every block by name, batches = one dict per step)).  HER: the settings gain clip_l / clip_r, the 30 % and 70 %
    quantiles of the float64 min(TQ1, TQ2) over all steps' rows (one row: a bound above it, so that the row clips).  Rows that break a kink
    condition at twice its margin are drawn again (all their arrays), at most 50 times over."""
    c = dict(ALL[name])
    rng = np.random.default_rng(c["seed"])
    P = {k: _init_block(c, k, rng) for k in NETS[c["algo"]] + TARGETS[c["algo"]]}
    batches = [_draw_rows(c, rng, B) for B in c["Bs"]]
    if c["algo"] == "her":
        free = dict(c, clip_l=-1e30, clip_r=1e30)
        tq = np.concatenate([step_f64(free, P, b)["rows"]["tq_raw"] for b in batches])
        if tq.size == 1:
            c["clip_l"], c["clip_r"] = f32(tq[0] + 0.5), f32(tq[0] + 1.5)
        else:
            c["clip_l"], c["clip_r"] = f32(np.quantile(tq, 0.3)), f32(np.quantile(tq, 0.7))
    for batch in batches:
        for _ in range(50):
            bad = violations(c, step_f64(c, P, batch, actor=_post_critics(c, P, batch)), factor=2.0)
            if not bad.any():
                break
            fresh = _draw_rows(c, rng, int(bad.sum()))
            for k in batch:
                batch[k][bad] = fresh[k]
        else:
            raise AssertionError(f"{name}: rows keep breaking the kink conditions; change the seed or the scales")
    for x in list(P.values()) + [v for b in batches for v in b.values()]:
        x.setflags(write=False)
    return c, dict(P=P, batches=batches)


# ------------------------------------------------------------------------------------------------ per block
def blocks(c, net):
    """[(name, slice)] of a block's flat ABI vector: each W and each b"""
    i, o_, heads = net_dims(c, net)
    out, off = [], 0
    for li, (r, k) in enumerate(omlp.layer_shapes(i, c["hidden"], o_, heads)):
        out.append((f"W{li}", slice(off, off + r * k)))
        off += r * k
        out.append((f"b{li}", slice(off, off + r)))
        off += r
    return out


def block_errors(got, ref, c, net):
    """[(name, max|got - ref|, max|ref|)] per parameter block"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape == (blocks(c, net)[-1][1].stop,), (got.shape, ref.shape)
    return [(nm, float(np.abs(got[s] - ref[s]).max()), float(np.abs(ref[s]).max())) for nm, s in blocks(c, net)]
