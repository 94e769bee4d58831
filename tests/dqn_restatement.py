"""Restatement written here for the DQN tests (not imported by the package): one DQN / Double DQN step (dqn.py:67-112, double_dqn.py:12-38)
in plain numpy from flat parameter vectors in the ABI layout (fc0.W | fc0.b | fc1.W | fc1.b | last_fc.W | last_fc.b) — forward, the MSE
gradient by hand, torch's Adam, the soft or hard target update — checked against tests/golden/g32_dqn.npz.  `dtype` selects the precision
of the whole step: float64 is the restatement, float32 measures what a second fp32 summation order costs (the DQN section)."""
import numpy as np


def unflatten(flat, dims, dtype):
    flat, off, layers = np.asarray(flat, dtype), 0, []
    for i in range(len(dims) - 1):
        w = flat[off:off + dims[i + 1] * dims[i]].reshape(dims[i + 1], dims[i]).copy()
        off += w.size
        layers.append((w, flat[off:off + dims[i + 1]].copy()))
        off += dims[i + 1]
    assert off == flat.size
    return layers


def flatten(layers):
    return np.concatenate([a.ravel() for wb in layers for a in wb])


def forward(layers, x):
    """-> (head output, the input of every layer)"""
    xs, h = [], x
    for i, (w, b) in enumerate(layers):
        xs.append(h)
        h = h @ w.T + b
        if i < len(layers) - 1:
            h = np.maximum(h, 0)
    return h, xs


def backward(layers, xs, g):
    """dL/d(head output) [B, n] -> the flat gradient"""
    grads = [None] * len(layers)
    for i in range(len(layers) - 1, -1, -1):
        grads[i] = (g.T @ xs[i], g.sum(0))
        if i:
            g = (g @ layers[i][0]) * (xs[i] > 0)   # xs[i] = relu(pre_{i-1})
    return flatten(grads)


class DqnRestatement:
    def __init__(self, o, hidden, n, q0, tq0, double_q, use_hard_updates, discount, learning_rate, tau, hard_update_period, dtype=np.float64):
        self.dims, self.dt = [o] + list(hidden) + [n], dtype
        self.q, self.tq = unflatten(q0, self.dims, dtype), unflatten(tq0, self.dims, dtype)
        self.double_q, self.hard, self.period = bool(double_q), bool(use_hard_updates), int(hard_update_period)
        self.gamma, self.lr, self.tau = dtype(discount), dtype(learning_rate), dtype(tau)
        self.m, self.v = np.zeros(flatten(self.q).size, dtype), np.zeros(flatten(self.q).size, dtype)
        self.t = self.n_train_steps = 0
        self.copied = []

    def train_step(self, batch):
        dt = self.dt
        s, s2 = np.asarray(batch["observations"], dt), np.asarray(batch["next_observations"], dt)
        r, d = np.asarray(batch["rewards"], dt).reshape(-1), np.asarray(batch["terminals"], dt).reshape(-1)
        a = np.asarray(batch["actions"]).reshape(-1).astype(np.int64)
        B, rows = len(a), np.arange(len(a))
        tq = forward(self.tq, s2)[0]
        if self.double_q:   # double_dqn.py:24-25: the target net at the online net's first maximal action
            v = tq[rows, forward(self.q, s2)[0].argmax(1)]
        else:               # dqn.py:79
            v = tq.max(1)
        y = r + (dt(1) - d) * self.gamma * v
        qs, xs = forward(self.q, s)
        qa = qs[rows, a]
        g = np.zeros_like(qs)
        g[rows, a] = dt(2) * (qa - y) / dt(B)   # nn.MSELoss(): mean((Q_a - y)^2)
        grad = backward(self.q, xs, g)
        # torch.optim.Adam, betas (0.9, 0.999), eps 1e-8
        self.t += 1
        b1, b2 = dt(0.9), dt(0.999)
        self.m = b1 * self.m + (dt(1) - b1) * grad
        self.v = b2 * self.v + (dt(1) - b2) * grad * grad
        step = self.lr / (dt(1) - b1 ** self.t)
        denom = np.sqrt(self.v) / np.sqrt(dt(1) - b2 ** self.t) + dt(1e-8)
        self.q = unflatten(flatten(self.q) - step * (self.m / denom), self.dims, dt)
        if self.hard:       # dqn.py:108-110: the counter is tested before the loop increments it
            if self.n_train_steps % self.period == 0:
                self.tq = [(w.copy(), b.copy()) for w, b in self.q]
                self.copied.append(self.n_train_steps)
        else:               # :112
            self.tq = [(tw * (dt(1) - self.tau) + w * self.tau, tb * (dt(1) - self.tau) + b * self.tau) for (tw, tb), (w, b) in zip(self.tq, self.q)]
        self.n_train_steps += 1
        return dict(qf_loss=float(np.mean((qa - y) ** 2)), y_pred=qa, grad=grad)

    def params(self, which):
        return flatten(dict(q=self.q, tq=self.tq)[which])


def golden_cases(path):
    """The cases of g32 as dicts: initial parameters rebuilt from the stored seed (tools/make_golden.py dqn_init, oracle/mlp.py init_mlp),
    `kw` = DqnRestatement's / the trainers' keywords."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import mlp as omlp
    g = np.load(path)
    kw = dict(zip([str(k) for k in g["kw_keys"]], g["kw_vals"].tolist()))
    kw["hard_update_period"] = int(kw["hard_update_period"])
    steps, out = int(g["steps"]), []
    for c in range(4):
        double_q, hard, Hw, B, n, o, seed = (int(v) for v in g[f"c{c}_shape"])
        rng = np.random.default_rng(seed)
        q0, tq0 = omlp.init_mlp(rng, o, [Hw, Hw], n), omlp.init_mlp(rng, o, [Hw, Hw], n)
        for p in (q0, tq0):
            p[-(Hw * n + n):] *= 100.0
        pre = f"c{c}_"
        batches = [{k: g[f"{pre}s{s}_{k}"] for k in ("observations", "actions", "rewards", "terminals", "next_observations")} for s in range(steps)]
        out.append(dict(o=o, H=Hw, B=B, n=n, double_q=bool(double_q), hard=bool(hard), q0=q0, tq0=tq0, batches=batches,
                        kw=dict(kw, use_hard_updates=bool(hard)), **{k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}))
    return out
