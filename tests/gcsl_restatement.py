"""A torch / numpy restatement of GCSL's update (rlkit/torch/algorithms/gcsl/gcsl.py:58-103), shared by the fixture generator and the tests:

  * `cat_init` / `mse_init`: the initial parameters of g29's cases, drawn from a seed (the fixture stores the seed, not the vectors);
  * `cat_batches` / `mse_batches`: the goal-conditioned inputs obs | goal | horizon of every step, drawn from a seed the same way;
  * `CatRestatement`: CatagorialMlp(batch_norm=True) in train mode — Linear -> BatchNorm1d -> ReLU blocks, last_fc, CrossEntropyLoss,
    accuracy of the first argmax, Adam over every parameter (gamma and beta included) — and its eval-mode probabilities;
  * `MseRestatement`: the plain ReLU MLP with max_act * tanh output (MlpGaussianAndEpsilonPolicy.forward never applies its BN modules,
    policies.py:533-540) under sum((pred - a)^2, -1).mean().
Flat parameter layout: torch's parameters() order of the network (per block W | b | gamma | beta, then last_fc W | b); the MSE net has no
gamma / beta (the reference's unused BN parameters are left out)."""
import numpy as np
import torch
from torch import nn

F32 = np.float32


def layout(D, H, nblk, n, bn=True):
    """[(name, shape)] in parameters() order."""
    out, k = [], D
    for l in range(nblk):
        out += [(f"W{l}", (H, k)), (f"b{l}", (H,))]
        if bn:
            out += [(f"g{l}", (H,)), (f"be{l}", (H,))]
        k = H
    return out + [("Wo", (n, H)), ("bo", (n,))]


def n_params(D, H, nblk, n, bn=True):
    return sum(int(np.prod(s)) for _, s in layout(D, H, nblk, n, bn))


def _init(seed, D, H, nblk, n, bn, head_scale):
    rng = np.random.default_rng(seed)
    parts = []
    for nm, s in layout(D, H, nblk, n, bn):
        if nm.startswith("W") and nm != "Wo":
            v = rng.uniform(-1.0 / np.sqrt(s[0]), 1.0 / np.sqrt(s[0]), s)     # fanin_init reads size[0] (pytorch_util.py:21-24)
        elif nm.startswith("b") and nm != "bo":
            v = np.full(s, 0.1)
        elif nm.startswith("g"):
            v = rng.uniform(0.8, 1.2, s)        # off the default 1 / 0 so that gamma and beta matter from the first step
        elif nm.startswith("be"):
            v = rng.uniform(-0.1, 0.1, s)
        else:
            v = rng.uniform(-head_scale, head_scale, s)
        parts.append(np.asarray(v, F32).ravel())
    return np.concatenate(parts).astype(F32)


def cat_init(seed, D, H, nblk, n):
    return _init(seed, D, H, nblk, n, True, 0.05)


def mse_init(seed, D, H, nblk, a):
    return _init(seed, D, H, nblk, a, False, 0.05)


def _horizons(rng, B, T):
    lens = rng.integers(-3, T, B)             # negative lengths: the all-ones rows of a wrapped trajectory
    return (np.arange(T)[None, :] >= lens[:, None]).astype(F32)


def cat_batches(seed, B, steps, d_obs, d_goal, T, n):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        x = np.concatenate([rng.normal(0, 1, (B, d_obs)), rng.uniform(-1, 1, (B, d_goal))], 1).astype(F32)
        X = np.concatenate([x, _horizons(rng, B, T)], 1).astype(F32)
        # labels that depend on the input, so that the accuracy moves
        y = (np.floor((np.clip(x[:, d_obs] , -0.999, 0.999) + 1) * 2.5).astype(np.int64) * 5
             + np.floor((np.clip(x[:, d_obs + 1], -0.999, 0.999) + 1) * 2.5).astype(np.int64)) % n
        out.append((X, y.astype(np.int64)))
    return out


def mse_batches(seed, B, steps, d_obs, d_goal, T, a):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        x = np.concatenate([rng.normal(0, 1, (B, d_obs)), rng.uniform(-1, 1, (B, d_goal))], 1).astype(F32)
        X = np.concatenate([x, _horizons(rng, B, T)], 1).astype(F32)
        out.append((X, rng.uniform(-1, 1, (B, a)).astype(F32)))
    return out


def probe(seed, rows, d_obs, d_goal, T):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.normal(0, 1, (rows, d_obs)), rng.uniform(-1, 1, (rows, d_goal))], 1).astype(F32)
    return np.concatenate([x, _horizons(rng, rows, T)], 1).astype(F32)


class _Net(nn.Module):
    def __init__(self, D, H, nblk, n, bn):
        super().__init__()
        self.fcs, self.bns = nn.ModuleList(), nn.ModuleList()
        k = D
        for _ in range(nblk):
            self.fcs.append(nn.Linear(k, H))
            if bn:
                self.bns.append(nn.BatchNorm1d(H))
            k = H
        self.last = nn.Linear(H, n)
        self.bn = bn

    def params_in_order(self):
        out = []
        for l, fc in enumerate(self.fcs):
            out += [fc.weight, fc.bias]
            if self.bn:
                out += [self.bns[l].weight, self.bns[l].bias]
        return out + [self.last.weight, self.last.bias]

    def forward(self, x):
        h = x
        for l, fc in enumerate(self.fcs):
            h = fc(h)
            if self.bn:
                h = self.bns[l](h)
            h = torch.relu(h)
        return self.last(h)


class _Restatement:
    bn = True

    def __init__(self, flat, D, H, nblk, n, lr=3e-4, dtype=torch.float32):
        torch.manual_seed(0)
        self.net = _Net(D, H, nblk, n, self.bn).to(dtype)
        self.dtype = dtype
        self.set_flat(flat)
        self.opt = torch.optim.Adam(self.net.params_in_order(), lr=lr)

    def _x(self, a):
        """a float32 input array in the precision of the net"""
        return torch.from_numpy(np.asarray(a, F32)).to(self.dtype)

    def set_flat(self, flat):
        off = 0
        with torch.no_grad():
            for p in self.net.params_in_order():
                k = p.numel()
                p.copy_(torch.from_numpy(np.ascontiguousarray(flat[off:off + k], F32)).view_as(p))
                off += k
        assert off == flat.size

    def flat(self):
        return np.concatenate([p.detach().numpy().ravel() for p in self.net.params_in_order()]).astype(F32)

    def running(self):
        return (np.stack([b.running_mean.numpy() for b in self.net.bns]).astype(F32),
                np.stack([b.running_var.numpy() for b in self.net.bns]).astype(F32))

    def dead_bias_mask(self):
        """The Linear biases under a BatchNorm: gradient exactly 0 (what any implementation holds there is rounding noise)."""
        m, off = np.zeros(self.flat().size, bool), 0
        for l, p in enumerate(self.net.params_in_order()):
            if self.bn and l % 4 == 1 and l < 4 * len(self.net.fcs):
                m[off:off + p.numel()] = True
            off += p.numel()
        return m


class CatRestatement(_Restatement):
    def train_step(self, X, y):
        self.net.train()
        logits = self.net(self._x(X))
        yt = torch.from_numpy(np.asarray(y, np.int64))
        loss = nn.CrossEntropyLoss()(logits, yt)
        acc = (torch.argmax(torch.softmax(logits, -1), -1) == yt).float().mean()
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss.item(), acc.item()

    WRONG = ("bn_const", "running_fwd", "no_inv_b", "label_shift", "bo_mean")

    def gradients(self, X, y, wrong=None):
        """One train-mode batch WITHOUT an optimiser step, in the precision the restatement was built with: dict(grad = the gradient of every
        parameter in the flat layout, ce, acc, probs [B, n] = the train-mode softmax, running_mean / running_var [nblk, H] after this one
        batch, dead = dead_bias_mask()).  The right step runs the modules themselves (nn.BatchNorm1d in train mode); `wrong` computes a
        deliberately wrong one from a forward written out here (tests: the bounds tell it from the right one):
          bn_const    — BatchNorm's backward with the batch mean and variance held constant;
          running_fwd — the running statistics (0 / 1 at the start) normalise the training forward;
          no_inv_b    — the cross-entropy summed, not averaged (dlogit without its 1/B);
          label_shift — the one-hot at y + 1 mod n;
          bo_mean     — the output bias's gradient as a mean over the rows instead of a sum."""
        assert wrong is None or wrong in self.WRONG, wrong
        net, n = self.net, self.net.last.out_features
        x, yt = self._x(X), torch.from_numpy(np.asarray(y, np.int64))
        B = x.shape[0]
        net.train()
        for p in net.parameters():
            p.grad = None
        if wrong in ("bn_const", "running_fwd"):
            h = x
            for fc, bn in zip(net.fcs, net.bns):
                z = fc(h)
                if wrong == "bn_const":
                    mean, var = z.mean(0).detach(), z.var(0, unbiased=False).detach()
                else:
                    mean, var = bn.running_mean, bn.running_var
                h = torch.relu(bn.weight * (z - mean) / torch.sqrt(var + bn.eps) + bn.bias)
            logits = net.last(h)
        else:
            logits = net(x)
        if wrong == "label_shift":
            yt = (yt + 1) % n
        loss = nn.CrossEntropyLoss(reduction="sum" if wrong == "no_inv_b" else "mean")(logits, yt)
        loss.backward()
        if wrong == "bo_mean":
            net.last.bias.grad /= B
        probs = torch.softmax(logits, -1).detach()
        ce = nn.CrossEntropyLoss()(logits, yt).item()
        acc = (torch.argmax(probs, -1) == yt).double().mean().item()
        grad = np.concatenate([(torch.zeros_like(p) if p.grad is None else p.grad).numpy().ravel() for p in net.params_in_order()])
        rm, rv = (np.stack([getattr(b, k).numpy().copy() for b in net.bns]) for k in ("running_mean", "running_var"))
        return dict(grad=grad, ce=ce, acc=acc, probs=probs.numpy(), running_mean=rm, running_var=rv, dead=self.dead_bias_mask())

    def probs(self, X):
        self.net.eval()
        with torch.no_grad():
            return torch.softmax(self.net(self._x(X)), -1).numpy()


class MseRestatement(_Restatement):
    bn = False

    def train_step(self, X, a, max_act=1.0):
        pred = max_act * torch.tanh(self.net(self._x(X)))
        loss = torch.sum((pred - self._x(a)) ** 2, -1).mean()
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss.item()
