"""Restatements written here for the DDPG tests (not imported by the package), checked against tests/golden/g31_ddpg.npz:
  * one DDPG step (rlkit/torch/algorithms/ddpg/ddpg.py:102-235) in torch on the CPU from flat parameter vectors in the ABI layout
    (fc0.W | fc0.b | ... | last_fc.W | last_fc.b);
  * OUStrategy / GaussianStrategy (rlkit/exploration_strategies/) in float64 numpy, the single-env forms, draws passed in."""
import os
import sys

import numpy as np
import torch

from dsac_restatement import flat, mlp, unflatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g31_ddpg.npz")
# tools/make_golden.py DDPG_CASES: (o, a, hidden, B, seed, tanh output, trainer keywords)
CASES = (
    (3, 1, [64, 64], 37, 3100, False, dict(target_update_period=2, policy_lr=1e-3, qf_lr=3e-3)),
    (11, 3, [128, 128], 256, 3101, True, dict(use_soft_update=True, policy_pre_activation_weight=0.01, qf_weight_decay=1e-3)),
    (11, 3, [256, 256, 256], 128, 3102, False, dict(min_q_value=-0.5, max_q_value=0.8)),
    (111, 8, [256, 256], 64, 3103, True, dict(use_soft_update=True)),
)
LOSS_KEYS = ("qf_loss", "policy_loss", "raw_policy_loss", "preactivation_policy_loss")
STAT_KEYS = ("q_predictions", "q_targets", "bellman_errors", "policy_action")


def msmm(x):
    x = np.asarray(x, np.float64)
    return np.array([x.mean(), x.std(), x.max(), x.min()])


class DdpgRestatement:
    def __init__(self, o, a, hidden, pi0, q0, tanh_out, discount=0.99, policy_lr=1e-4, qf_lr=1e-3, qf_weight_decay=0.0,
                 target_update_period=1000, soft_target_tau=1e-2, use_soft_update=False, policy_pre_activation_weight=0.0,
                 min_q_value=-np.inf, max_q_value=np.inf):
        self.pi, self.q = unflatten(pi0, o, hidden, a), unflatten(q0, o + a, hidden, 1)
        self.tpi, self.tq = [p.detach().clone() for p in self.pi], [p.detach().clone() for p in self.q]
        self.tanh_out, self.gamma, self.wd, self.period, self.tau = tanh_out, discount, qf_weight_decay, target_update_period, soft_target_tau
        self.soft, self.pw, self.lo, self.hi = use_soft_update, policy_pre_activation_weight, min_q_value, max_q_value
        self.opt_pi, self.opt_q = torch.optim.Adam(self.pi, lr=policy_lr), torch.optim.Adam(self.q, lr=qf_lr)
        self.counter, self.copied = 0, []

    def act(self, params, s):
        pre = mlp(params, s)
        return (torch.tanh(pre) if self.tanh_out else pre), pre

    def train_step(self, batch):
        T = {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in batch.items()}
        s, s2, ac = T["observations"], T["next_observations"], T["actions"]
        r, d = T["rewards"].reshape(-1, 1), T["terminals"].reshape(-1, 1)
        out = {}
        pa, pre = self.act(self.pi, s)
        raw = -mlp(self.q, torch.cat([s, pa], 1)).mean()
        ploss = raw + self.pw * (pre ** 2).sum(1).mean() if self.pw > 0 else raw
        with torch.no_grad():
            y = r + (1.0 - d) * self.gamma * mlp(self.tq, torch.cat([s2, self.act(self.tpi, s2)[0]], 1))
            y = torch.clamp(y, self.lo, self.hi)
        qp = mlp(self.q, torch.cat([s, ac], 1))
        qloss = ((qp - y) ** 2).mean()
        if self.wd > 0:
            qloss = qloss + self.wd * sum((p ** 2).sum() for p in self.q if p.dim() > 1)
        self.opt_pi.zero_grad()
        ploss.backward()
        out["grad_pi"] = flat(self.pi, True)
        self.opt_pi.step()
        self.opt_q.zero_grad()
        qloss.backward()
        out["grad_q"] = flat(self.q, True)
        self.opt_q.step()
        with torch.no_grad():
            if self.soft:
                for src, dst in ((self.pi, self.tpi), (self.q, self.tq)):
                    for p, tp in zip(src, dst):
                        tp.copy_(tp * (1.0 - self.tau) + p * self.tau)
            elif self.counter % self.period == 0:   # tested before the increment: the first step copies
                for src, dst in ((self.pi, self.tpi), (self.q, self.tq)):
                    for p, tp in zip(src, dst):
                        tp.copy_(p)
                self.copied.append(self.counter)
        self.counter += 1
        ql, pl, rw = float(qloss.detach()), float(ploss.detach()), float(raw.detach())
        out["losses"] = np.array([ql, pl, rw, pl - rw])
        out["q_predictions"], out["q_targets"] = msmm(qp.detach().numpy()), msmm(y.numpy())
        out["bellman_errors"], out["policy_action"] = msmm(((qp - y) ** 2).detach().numpy()), msmm(pa.detach().numpy())
        return out

    def params(self, which):
        return flat(dict(pi=self.pi, q=self.q, tpi=self.tpi, tq=self.tq)[which])


def golden_cases():
    """Every case of g31 as a dict: shapes, initial parameters rebuilt from the seed (tools/make_golden.py ddpg_init, oracle/mlp.py
    init_mlp), the batches, and the case's golden arrays with the `c<i>_` prefix removed."""
    sys.path.insert(0, ROOT)
    from oracle import mlp as omlp
    g = np.load(GOLDEN)
    steps = int(g["steps"])
    out = []
    for c, (o, a, Hh, B, seed, tanh_out, kw) in enumerate(CASES):
        rng = np.random.default_rng(seed)
        pi0 = omlp.init_mlp(rng, o, Hh, a, init_w=1e-3)
        pi0[-(Hh[-1] * a + a):] *= 300.0
        q0 = omlp.init_mlp(rng, o + a, Hh, 1)
        pre = f"c{c}_"
        batches = [{k: g[f"{pre}s{s}_{k}"] for k in ("observations", "actions", "rewards", "terminals", "next_observations")} for s in range(steps)]
        out.append(dict(c=c, o=o, a=a, hidden=Hh, B=B, tanh_out=tanh_out, kw=dict(kw, discount=float(g["discount"])), pi0=pi0, q0=q0,
                        batches=batches, steps=steps, **{k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}))
    return out


# ---------------------------------------------------------------------------------------------- exploration strategies
def sigma_at(t, max_sigma, min_sigma, decay_period):
    return max_sigma - (max_sigma - min_sigma) * min(1.0, t * 1.0 / decay_period)


def ou_trace(raw, eps, ts, resets, mu, theta, max_sigma, min_sigma, decay_period, low=-1.0, high=1.0):
    """ou_strategy.py:46-60 per call: evolve with the previous call's sigma, then anneal; reset() puts the state back to mu."""
    state, sigma, out = np.ones(raw.shape[1]) * mu, max_sigma, []
    for k in range(len(raw)):
        if k in resets:
            state = np.ones(raw.shape[1]) * mu
        state = state + (theta * (mu - state) + sigma * eps[k])
        sigma = sigma_at(ts[k], max_sigma, min_sigma, decay_period)
        out.append(np.clip(raw[k] + state, low, high))
    return np.stack(out)


def gaussian_trace(raw, eps, ts, max_sigma, min_sigma, decay_period, low=-1.0, high=1.0):
    return np.stack([np.clip(raw[k] + eps[k] * sigma_at(ts[k], max_sigma, min_sigma, decay_period), low, high) for k in range(len(raw))])
