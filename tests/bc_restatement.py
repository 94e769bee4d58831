"""A float64 restatement of one behaviour-cloning update (rlkit/torch/algorithms/bc/bc.py:81-106) with torch autograd on the CPU, shared by
the CPU and the GPU tests of tests/test_bc_parity_hip.py:

  * `CASES`: the shape matrix (o, a, hidden, max_batch, B), the smallest shapes that still reach each code path of the device step;
  * `make_policy` / `make_batch`: the inputs of a case, drawn from a seed — heads scaled so that the mean and the raw log-std have real spread,
    a per-dimension log-std bias that puts rows on both sides of the [LOG_SIG_MIN, LOG_SIG_MAX] clamp (MSE) or on its upper side (MLE; at
    log_std = -20 the MLE gradient is (mu - z) * e^40, which no fp32 evaluation holds), expert actions with exact +-1 entries;
  * `bc_reference`: the loss written forwards only — ReLU trunk, mean | log_std_raw heads, clamp, tanh-Gaussian log-prob of the expert action
    or squared error of the sampled action — differentiated by autograd, so that it shares no backward formula with oracle/bc.py or kernels.h;
  * `trunk_f64`: the float64 head outputs (mean, raw log-std) of a policy, for the log-prob / action checks.
Flat vectors are in the ABI layout (oracle.mlp.unpack with n_heads=2)."""
import numpy as np
import torch

from oracle import mlp as omlp
from oracle import tanh_gaussian as otg

F32 = np.float32

# name -> (o, a, hidden, max_batch, B)
CASES = dict(
    one_row=(11, 3, [64, 64], 32, 1),             # a single row in a 16-row tile
    ragged=(17, 6, [128, 128], 256, 17),          # B no multiple of 16, B < max_batch, the 128-wide kernels
    spec=(17, 6, [256, 256], 256, 256),           # exp_specs/bc/bc_hopper_hip.yaml: the 1024-thread kernels
    wide_in=(111, 8, [256, 256], 256, 100),       # input staged in more than one 64-column slab
    humanoid=(376, 17, [256, 256], 64, 50),       # a = 17: heads past one 16-column group
    unequal=(11, 3, [200, 100], 64, 33),          # padded widths: structural zeros
    row_split=(17, 6, [128, 128], 1100, 1100),    # row-split dW with a ragged last range, Adam in the reduction, no Polyak target
    dw_big=(11, 3, [64, 64], 4100, 4100),         # the big-batch dW kernel
)
MODES = ("MLE", "MSE")
LS_PATTERN = dict(MSE=(3.0, -23.0, 0.0), MLE=(2.0, -2.0, 0.0))
MEAN_SCALE, LS_SCALE = 300.0, 400.0


# one_row in MSE mode has ONE entry above the clamp, and at sigma = e^2 most draws of its noise saturate tanh: dz ~ 0 and the gate multiplies
# nothing.  This seed draws |eps| = 0.23 there, and removing the gate moves the log-std head's gradient by 3x its largest entry.
SEEDS = {("one_row", "MSE"): 7009}


def case_seed(case, mode):
    return SEEDS.get((case, mode), 7000 + 10 * list(CASES).index(case) + MODES.index(mode))


def make_policy(rng, o, a, hidden, mode):
    """init_mlp(init_w=1e-3) with the mean head scaled by 300, the log-std head by 400 and LS_PATTERN[mode] cycled onto the log-std bias."""
    pi0 = omlp.init_mlp(rng, o, hidden, a, init_w=1e-3, n_heads=2)
    lay = omlp.unpack(pi0, o, hidden, a, n_heads=2)          # views into pi0
    for x in lay[-2]:
        x *= F32(MEAN_SCALE)
    for x in lay[-1]:
        x *= F32(LS_SCALE)
    pat = LS_PATTERN[mode]
    lay[-1][1][:] += np.asarray([pat[j % len(pat)] for j in range(a)], F32)
    return pi0


def make_batch(rng, B, o, a):
    """(obs, acts, eps): N(0,1) observations, tanh(N(0,1)) expert actions with one entry at exactly +1 and one at exactly -1, N(0,1) noise."""
    obs = rng.normal(0, 1, (B, o)).astype(F32)
    acts = np.tanh(rng.normal(0, 1, (B, a))).astype(F32)
    acts[0, 0], acts[-1, -1] = 1.0, -1.0
    eps = rng.normal(0, 1, (B, a)).astype(F32)
    return obs, acts, eps


def make_case(case, mode):
    """(pi0, obs, acts, eps, rng) of one cell of the matrix; `rng` goes on to draw the batches of further steps."""
    o, a, hidden, _, B = CASES[case]
    rng = np.random.default_rng(case_seed(case, mode))
    pi0 = make_policy(rng, o, a, hidden, mode)
    return (pi0,) + make_batch(rng, B, o, a) + (rng,)


def _heads(layers, x, n_hidden):
    h = x
    for W, b in layers[:n_hidden]:
        h = torch.relu(h @ W.T + b)
    (Wm, bm), (Ws, bs) = layers[n_hidden:]
    return h @ Wm.T + bm, h @ Ws.T + bs


def _layers64(flat, o, hidden, a, requires_grad=False):
    return [(torch.tensor(W.astype(np.float64), requires_grad=requires_grad), torch.tensor(b.astype(np.float64), requires_grad=requires_grad))
            for W, b in omlp.unpack(np.asarray(flat, F32), o, hidden, a, n_heads=2)]


def trunk_f64(flat, obs, o, hidden, a):
    """float64 (mean, log_std_raw) of the policy `flat` on `obs`."""
    with torch.no_grad():
        mu, lsr = _heads(_layers64(flat, o, hidden, a), torch.tensor(np.asarray(obs, F32).astype(np.float64)), len(hidden))
    return mu.numpy(), lsr.numpy()


def bc_reference(flat, obs, acts, eps, o, hidden, a, mode, gate=True):
    """One BC loss and its gradient in float64.  Returns dict(grad [flat, ABI layout], stat, lsr [B, a]).  gate=False: the same values with
    the clamp's derivative taken as 1 everywhere — what a backward pass without the gate computes (the tests show that it is far from `grad`)."""
    layers = _layers64(flat, o, hidden, a, requires_grad=True)
    x, act = (torch.tensor(np.asarray(v, F32).astype(np.float64)) for v in (obs, acts))
    mu, lsr = _heads(layers, x, len(hidden))
    ls = torch.clamp(lsr, otg.LOG_SIG_MIN, otg.LOG_SIG_MAX)
    if not gate:
        ls = lsr + (ls - lsr).detach()
    if mode == "MLE":
        # policies.py:329-345 -> distributions.py:74-97 with pre_tanh_value=None; 0.5*log(2 pi) enters once per row (distributions.py:45-49)
        z = 0.5 * (torch.log(1 + act + otg.EPS) - torch.log(1 - act + otg.EPS))
        lp = -0.5 * torch.sum((mu - z) ** 2 / torch.exp(2 * ls), 1) - (torch.sum(ls, 1) + otg.HALF_LOG_2PI)
        lp = lp - torch.sum(torch.log(1 - act * act + otg.EPS), 1)
        stat = lp.mean()
        loss = -stat
    else:
        e = torch.tensor(np.asarray(eps, F32).astype(np.float64))
        pred = torch.tanh(mu + torch.exp(ls) * e)
        loss = stat = torch.sum((pred - act) ** 2, 1).mean()
    grads = torch.autograd.grad(loss, [p for Wb in layers for p in Wb])
    return dict(grad=np.concatenate([g.numpy().ravel() for g in grads]), stat=stat.item(), lsr=lsr.detach().numpy())


def blocks(o, hidden, a):
    """[(name, slice)] of the flat ABI vector: each W and each b of layer_shapes."""
    out, off = [], 0
    for li, (r, c) in enumerate(omlp.layer_shapes(o, hidden, a, n_heads=2)):
        out.append((f"W{li}", slice(off, off + r * c)))
        off += r * c
        out.append((f"b{li}", slice(off, off + r)))
        off += r
    return out


def block_errors(got, ref, o, hidden, a):
    """[(name, max|got - ref|, max|ref|)] per parameter block."""
    return [(nm, float(np.abs(got[s] - ref[s]).max()), float(np.abs(ref[s]).max())) for nm, s in blocks(o, hidden, a)]
