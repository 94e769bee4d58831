"""A torch-CPU restatement of the MBPO ensemble arithmetic (rlkit/torch/common/networks.py:149-279 BNN.forward / predict,
rlkit/torch/algorithms/mbpo/bnn_trainer.py:71-87,141-154 compute_loss + one Adam step, fake_env.py:30-75 FakeEnv.step with given
members and noise), written for this project's tests: parameters in the reference's named_parameters() layout, per layer
weight [E, in, out] then bias [E, 1, out]."""
import numpy as np
import torch
import torch.nn.functional as F

MAX_LV, MIN_LV = 0.5, -10.0


def shapes(E, in_dim, hidden_sizes, out_dim):
    sizes = [in_dim] + list(hidden_sizes) + [2 * out_dim]
    out = []
    for i in range(len(sizes) - 1):
        out += [(E, sizes[i], sizes[i + 1]), (E, 1, sizes[i + 1])]
    return out


def unflatten(flat, shp):
    out, f = [], 0
    for s in shp:
        n = int(np.prod(s))
        out.append(np.asarray(flat[f:f + n], np.float32).reshape(s))
        f += n
    return out


def init_params(rng, E, in_dim, hidden_sizes, out_dim, init_w=3e-3):
    """the reference's init rule with a numpy generator: hidden U(+-1/sqrt(in*out)), hidden bias 0.1, head U(+-init_w)"""
    shp = shapes(E, in_dim, hidden_sizes, out_dim)
    out = []
    for li in range(len(shp) // 2):
        w, b = shp[2 * li], shp[2 * li + 1]
        last = li == len(shp) // 2 - 1
        bound = init_w if last else 1.0 / np.sqrt(w[1] * w[2])
        out.append(rng.uniform(-bound, bound, w).astype(np.float32))
        out.append(rng.uniform(-init_w, init_w, b).astype(np.float32) if last else np.full(b, 0.1, np.float32))
    return out


def forward(params, mean, std, x):
    """x [n, in] or [E, n, in] -> (mean, log-var) [E, n, D]"""
    h = (torch.as_tensor(x, dtype=torch.float32) - torch.as_tensor(mean)) / torch.as_tensor(std)
    P = [p if isinstance(p, torch.Tensor) else torch.as_tensor(p) for p in params]
    L = len(P) // 2
    for li in range(L):
        W, b = P[2 * li], P[2 * li + 1]
        h = (torch.einsum("ij,ljk->lik", h, W) if h.dim() == 2 else torch.matmul(h, W)) + b
        if li < L - 1:
            h = F.silu(h)
    D = h.shape[-1] // 2
    mu, raw = h[:, :, :D], h[:, :, D:]
    max_lv = torch.full((1, D), MAX_LV, device=h.device)
    min_lv = torch.full((1, D), MIN_LV, device=h.device)
    lv = max_lv - F.softplus(max_lv - raw)
    lv = min_lv + F.softplus(lv - min_lv)
    return mu, lv


def compute_loss(params, mean, std, x, t, add_var_loss=True):
    mu, lv = forward(params, mean, std, x)
    t = torch.as_tensor(t, dtype=torch.float32, device=mu.device)
    if add_var_loss:
        return torch.mean((mu - t) ** 2 * torch.exp(-lv), dim=[-2, -1]) + torch.mean(lv, dim=[-2, -1])
    return torch.mean((mu - t) ** 2, dim=[-2, -1])


class AdamTrainer:
    """torch.optim.Adam over the layers with per-layer weight decay, the loss of BNNTrainer.train_step"""

    def __init__(self, params, lr, weight_decays):
        self.P = [torch.nn.Parameter(torch.as_tensor(np.array(p, np.float32))) for p in params]
        groups = [{"params": [self.P[2 * i], self.P[2 * i + 1]], "weight_decay": wd} for i, wd in enumerate(weight_decays)]
        self.opt = torch.optim.Adam(groups, lr=lr)

    def step(self, mean, std, x, t):
        loss = torch.mean(compute_loss(self.P, mean, std, x, t)) + 0.01 * MAX_LV - 0.01 * MIN_LV
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return float(loss.detach())

    def params(self):
        return [p.detach().numpy().copy() for p in self.P]


# ------------------------------------------------------------------------------------------------ float64: the gradient of one train step
B2 = 0.999
WRONG = ("no_inv_e", "inv_max_batch", "half_dmu", "no_lower", "no_upper", "no_mean_lv", "silu_sigmoid", "no_reward_scale", "next_obs_target",
         "no_wd", "wd_weights_only", "wd_shifted", "members_swapped")


def step_f64(params, mean, std, x, t, weight_decays, wrong=None, max_batch=None, reward_scale=1.0, stale=None):
    """One train step in float64 autograd: x [E, B, in], t [E, B, D] the members' own rows (x[idx], t[idx]), one weight decay per layer.
    Returns dict(loss = compute_loss per member [E], grads = g + wd_l * p of every parameter, flat in the parameters' layout, with g the
    gradient of mean_e[ mean((mu - t)^2 e^-lv) + mean(lv) ] (bnn_trainer.py:71-87,141-154), raw = the head's raw log-variance [E, B, D]).
    `wrong` names one deliberate mistake (WRONG), for the tests that show a check discriminates; every mistake leaves the loss VALUE's
    formula alone where it can and changes the gradient.  `stale` (parameters of an earlier step) is one more: the backward chain takes
    dh = dz @ W^T with THOSE weights, the forward and the weight gradient h^T dz with the current ones — a transposed copy that the
    optimiser left behind."""
    assert wrong is None or wrong in WRONG, wrong
    f64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))   # noqa: E731
    P = [f64(p).requires_grad_(True) for p in params]
    L, wd = len(P) // 2, [float(w) for w in weight_decays]
    assert len(wd) == L
    x, t = f64(x).clone(), f64(t).clone()
    E, B, D = t.shape
    if wrong == "members_swapped":          # member 0 reads member 1's index row
        x[0], t[0] = x[1], t[1]
    if wrong == "no_reward_scale":
        t[:, :, 0] /= reward_scale
    if wrong == "next_obs_target":          # next_obs where next_obs - obs belongs
        t[:, :, 1:] += x[:, :, :D - 1]
    h = (x - f64(mean)) / f64(std)
    for li in range(L):
        if stale is None or li == 0:
            z = torch.matmul(h, P[2 * li]) + P[2 * li + 1]
        else:                               # value h @ W + b; d/dW = h^T dz; d/dh = dz @ W_stale^T
            via_stale = torch.matmul(h, f64(stale[2 * li]))
            z = torch.matmul(h.detach(), P[2 * li]) + (via_stale - via_stale.detach()) + P[2 * li + 1]
        if li == L - 1:
            break
        sg = torch.sigmoid(z)
        h = z * (sg.detach() if wrong == "silu_sigmoid" else sg)        # detached: the derivative is sigmoid(z) alone
    mu, raw = z[:, :, :D], z[:, :, D:]
    lv1 = MAX_LV - F.softplus(MAX_LV - raw)
    if wrong == "no_upper":                 # the value of lv1, the derivative 1
        lv1 = raw + (lv1 - raw).detach()
    lv = MIN_LV + F.softplus(lv1 - MIN_LV)
    if wrong == "no_lower":
        lv = lv1 + (lv - lv1).detach()
    if wrong == "half_dmu":                 # the value of mu, half its derivative
        mu = 0.5 * mu + 0.5 * mu.detach()
    per = torch.mean((mu - t) ** 2 * torch.exp(-lv), dim=[-2, -1])
    if wrong != "no_mean_lv":
        per = per + torch.mean(lv, dim=[-2, -1])
    total = torch.sum(per) if wrong == "no_inv_e" else torch.mean(per)
    if wrong == "inv_max_batch":
        total = total * (B / float(max_batch))
    g = torch.autograd.grad(total, P)
    if wrong == "no_wd":
        wd = [0.0] * L
    if wrong == "wd_shifted":
        wd = wd[-1:] + wd[:-1]
    out = []
    for i, (p, gi) in enumerate(zip(P, g)):
        w = 0.0 if (wrong == "wd_weights_only" and i % 2 == 1) else wd[i // 2]
        out.append((gi + w * p.detach()).numpy().reshape(-1))
    return dict(loss=per.detach().numpy(), grads=np.concatenate(out), raw=raw.detach().numpy())


def blocks(shp):
    """[(name, slice)] of a flat vector in the parameters' layout: one block is ONE member's weight or bias of one layer"""
    out, f = [], 0
    for i, s in enumerate(shp):
        n = int(np.prod(s[1:]))
        for e in range(s[0]):
            out.append((f"fc{i // 2}.{'bias' if i % 2 else 'weight'}[{e}]", slice(f, f + n)))
            f += n
    return out


def block_errors(got, ref, shp):
    """[(name, max|got - ref|, max|ref|)] per block"""
    got, ref, bl = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1), blocks(shp)
    assert got.shape == ref.shape == (bl[-1][1].stop,), (got.shape, ref.shape)
    return [(nm, float(np.abs(got[s] - ref[s]).max()), float(np.abs(ref[s]).max())) for nm, s in bl]


def adam_moments(grads, beta_1=0.9):
    """(exp_avg, exp_avg_sq) after Adam (betas beta_1 / 0.999, zero start) has seen `grads` in order"""
    m, v = np.zeros_like(grads[0]), np.zeros_like(grads[0])
    for g in grads:
        m, v = beta_1 * m + (1 - beta_1) * g, B2 * v + (1 - B2) * g * g
    return m, v


def data_from_rows(obs, act, rew, nobs, reward_scale=1.0):
    """inputs [obs | act], targets [reward_scale * rew | next_obs - obs] (bnn_trainer.py:92-97), float32"""
    obs, act, nobs = (np.asarray(a, np.float32) for a in (obs, act, nobs))
    rew = np.asarray(rew, np.float32).reshape(-1, 1)
    x = np.concatenate([obs, act], -1)
    t = np.concatenate([np.float32(reward_scale) * rew, nobs - obs], -1)
    return x, t


def normalizer_stats(x):
    """bnn_trainer.py:113-118 + normalizer.py:101-103"""
    xt = torch.as_tensor(x)
    m = torch.mean(xt, dim=0, keepdim=True)
    s = torch.std(xt, dim=0, keepdim=True)
    s[s < 1e-12] = 1.0
    return m.numpy().reshape(-1), (s.numpy().reshape(-1) + np.float32(1e-8)).astype(np.float32)


def fake_env_step(params, mean, std, obs, act, model_idx, noise_rows=None):
    """FakeEnv.step with the member of each row given and its noise row [n, D] (None = deterministic): next_obs, rew [n, 1]"""
    x = np.concatenate([obs, act], -1).astype(np.float32)
    with torch.no_grad():
        mu, lv = forward(params, mean, std, x)
    mu, var = mu.numpy(), torch.exp(lv).numpy()
    mu[:, :, 1:] += obs
    n = obs.shape[0]
    m_mu, m_std = mu[model_idx, np.arange(n)], np.sqrt(var)[model_idx, np.arange(n)]
    s = m_mu if noise_rows is None else m_mu + noise_rows * m_std
    return s[:, 1:], s[:, :1]

