"""Restatements written here for the discrete-SAC tests (not imported by the package):
  * CartPole — gym 0.22's CartPoleEnv.step (gym/envs/classic_control/cartpole.py) in float64 numpy, Python's math.sin / math.cos per
    element, the products and sums in gym's order (the HIP stepper in csrc/classic_env.h runs the same expression tree with FMA
    contraction off);
  * one discrete SAC step (discrete_sac.py:60-181) in torch on the CPU from flat parameter vectors in the ABI layout
    (fc0.W | fc0.b | fc1.W | fc1.b | last_fc.W | last_fc.b), checked against tests/golden/g28_discrete_sac.npz."""
import math

import numpy as np
import torch

GRAVITY, MASSCART, MASSPOLE, LENGTH, FORCE_MAG, TAU = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
TOTAL_MASS = MASSPOLE + MASSCART
POLEMASS_LENGTH = MASSPOLE * LENGTH
THETA_THRESHOLD = 12 * 2 * math.pi / 360
X_THRESHOLD = 2.4
_sin, _cos = np.frompyfunc(math.sin, 1, 1), np.frompyfunc(math.cos, 1, 1)


def cartpole_step(state, action):
    """state [N, 4] float64 (x, x_dot, theta, theta_dot), action [N] indices -> (next state [N, 4], reward [N], done [N])."""
    x, x_dot, theta, theta_dot = (np.asarray(state[:, i], np.float64) for i in range(4))
    force = np.where(np.asarray(action) == 1, FORCE_MAG, -FORCE_MAG)
    costheta, sintheta = _cos(theta).astype(np.float64), _sin(theta).astype(np.float64)
    temp = (force + POLEMASS_LENGTH * (theta_dot * theta_dot) * sintheta) / TOTAL_MASS
    thetaacc = (GRAVITY * sintheta - costheta * temp) / (LENGTH * (4.0 / 3.0 - MASSPOLE * (costheta * costheta) / TOTAL_MASS))
    xacc = temp - POLEMASS_LENGTH * thetaacc * costheta / TOTAL_MASS
    x = x + TAU * x_dot
    x_dot = x_dot + TAU * xacc
    theta = theta + TAU * theta_dot
    theta_dot = theta_dot + TAU * thetaacc
    done = (x < -X_THRESHOLD) | (x > X_THRESHOLD) | (theta < -THETA_THRESHOLD) | (theta > THETA_THRESHOLD)
    return np.stack([x, x_dot, theta, theta_dot], 1), np.ones(len(x)), done


# ---------------------------------------------------------------------------------------------------- discrete SAC
def unflatten(flat, in_dim, hidden, out_dim):
    flat = torch.as_tensor(np.asarray(flat, np.float32))
    dims, off, layers = [in_dim] + list(hidden) + [out_dim], 0, []
    for i in range(len(dims) - 1):
        w = flat[off:off + dims[i + 1] * dims[i]].view(dims[i + 1], dims[i]).clone().requires_grad_(True)
        off += dims[i + 1] * dims[i]
        b = flat[off:off + dims[i + 1]].clone().requires_grad_(True)
        off += dims[i + 1]
        layers += [w, b]
    assert off == flat.numel()
    return layers


def mlp(params, x):
    h = x
    for i in range(0, len(params) - 2, 2):
        h = torch.relu(h @ params[i].T + params[i + 1])
    return h @ params[-2].T + params[-1]


def flat(params, grad=False):
    return torch.cat([(p.grad if grad else p).detach().reshape(-1) for p in params]).numpy().astype(np.float32)


class DsacRestatement:
    """Policy, qf1, qf2 and their targets as flat-vector MLPs; Adam with betas (beta_1, 0.999); fixed alpha."""

    def __init__(self, o, hidden, n, pi0, q10, q20, discount, reward_scale, alpha, soft_target_tau, policy_lr, qf_lr, beta_1=0.9, **_):
        self.pi, self.q1, self.q2 = (unflatten(p, o, hidden, n) for p in (pi0, q10, q20))
        self.tq1 = [p.detach().clone() for p in self.q1]
        self.tq2 = [p.detach().clone() for p in self.q2]
        self.gamma, self.rs, self.alpha, self.tau = discount, reward_scale, alpha, soft_target_tau
        betas = (beta_1, 0.999)
        self.opt_pi = torch.optim.Adam(self.pi, lr=policy_lr, betas=betas)
        self.opt_q1 = torch.optim.Adam(self.q1, lr=qf_lr, betas=betas)
        self.opt_q2 = torch.optim.Adam(self.q2, lr=qf_lr, betas=betas)

    def train_step(self, batch):
        T = {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in batch.items()}
        s, s2, r, d = T["observations"], T["next_observations"], T["rewards"].reshape(-1), T["terminals"].reshape(-1)
        a = T["actions"].reshape(-1).long()
        out = {}
        # critic: y = rs r + (1 - d) gamma (sum_j p'_j min(TQ1, TQ2)_j + alpha H(p')), L_i = 0.5 mean((Q_i(s)[a] - y)^2)
        with torch.no_grad():
            lp2 = torch.log_softmax(mlp(self.pi, s2), 1)
            p2 = lp2.exp()
            v2 = (p2 * torch.min(mlp(self.tq1, s2), mlp(self.tq2, s2))).sum(1) - self.alpha * (p2 * lp2).sum(1)
            y = self.rs * r + (1.0 - d) * self.gamma * v2
        for q, opt, k in ((self.q1, self.opt_q1, "q1"), (self.q2, self.opt_q2, "q2")):
            opt.zero_grad()
            qa = mlp(q, s).gather(1, a[:, None])[:, 0]
            loss = 0.5 * ((qa - y) ** 2).mean()
            loss.backward()
            out[k + "_loss"], out[k + "_pred"], out["grad_" + k] = float(loss.detach()), qa.detach().numpy(), flat(q, True)
            opt.step()
        # policy on the updated critics: L = -mean(alpha H(p) + sum_j p_j min(Q1, Q2)_j)
        with torch.no_grad():
            qmin = torch.min(mlp(self.q1, s), mlp(self.q2, s))
        self.opt_pi.zero_grad()
        lp = torch.log_softmax(mlp(self.pi, s), 1)
        p = lp.exp()
        ploss = -((p * (qmin - self.alpha * lp)).sum(1)).mean()
        ploss.backward()
        out["policy_loss"], out["grad_pi"] = float(ploss.detach()), flat(self.pi, True)
        self.opt_pi.step()
        with torch.no_grad():
            for q, tq in ((self.q1, self.tq1), (self.q2, self.tq2)):
                for pp, tp in zip(q, tq):
                    tp.mul_(1.0 - self.tau).add_(pp.detach() * self.tau)
        return out

    def params(self, which):
        return flat(dict(pi=self.pi, q1=self.q1, q2=self.q2, tq1=self.tq1, tq2=self.tq2)[which])


def golden_cases(path):
    """(case dict, DsacRestatement kwargs) of every case of g28: initial parameters rebuilt from the stored seed (tools/make_golden.py
    dsac_init, oracle/mlp.py init_mlp)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import mlp as omlp
    g = np.load(path)
    kw = dict(zip([str(k) for k in g["kw_keys"]], g["kw_vals"].tolist()))
    o, steps = (int(v) for v in g["dims"])
    out = []
    for c in range(2):
        Hw, B, n, seed = (int(v) for v in g[f"c{c}_shape"])
        rng = np.random.default_rng(seed)
        pi0 = omlp.init_mlp(rng, o, [Hw, Hw], n, init_w=1e-3)
        pi0[-(Hw * n + n):] *= 100.0
        q10, q20 = omlp.init_mlp(rng, o, [Hw, Hw], n), omlp.init_mlp(rng, o, [Hw, Hw], n)
        pre = f"c{c}_"
        batches = [{k: g[f"{pre}s{s}_{k}"] for k in ("observations", "actions", "rewards", "terminals", "next_observations")} for s in range(steps)]
        out.append(dict(o=o, H=Hw, B=B, n=n, pi0=pi0, q10=q10, q20=q20, batches=batches, kw=kw,
                        **{k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}))
    return out
