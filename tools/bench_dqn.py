#!/usr/bin/env python
"""DQN / Double DQN measurements on one MI355X (prints one JSON line, writes under --out-dir, default profiles/):

  step    microseconds per gradient step of DQN.train_from_replay and DoubleDQN.train_from_replay at the CartPole spec's shape (2 x 128,
          B = 128, n = 2, o = 4), soft targets, over a window of --steps steps that ends in a synchronise; the same two steps as an eager
          torch-ROCm restatement (tests/dqn_restatement.py's arithmetic with autograd and torch.optim.Adam) timed beside them in the same
          run; launches per step AS DESIGNED (replay gather, forward, loss kernel, backward, dW + Adam + Polyak, tick) — a count, not a
          measurement; `--train-only N` runs nothing but N DQN steps so that a `rocprofv3 --kernel-trace --stats` table gives the
          measured count -> dqn_bench.json
  learn   a spec of exp_specs/dqn/ through run_scripts/dqn_exp_script.py, one process per seed, cut to --epochs epochs
          -> dqn_<task>_summary.json: every epoch's evaluation return per seed (the runs' progress logs are not kept)

Wall-clock timing after warm-up, the stream synchronised before and after every timed stretch; process handling of `learn` is
tools/bench_pendulum.py's."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

LAUNCHES_PER_STEP_DESIGN = 6   # replay gather + fwd + k_dqn_grad + bwd + dW/Adam/Polyak + tick (hard updates: + the copy on its steps)
SPECS = {"cartpole": "dqn/dqn_cartpole_hip.yaml", "mountaincar": "dqn/dqn_mountaincar_hip.yaml", "acrobot": "dqn/ddqn_acrobot_hip.yaml"}
H, B, N_ACT, OBS = 128, 128, 2, 4


def dqn_rate(ctx, double_q, steps, warm=200):
    import ilswiss_amd as ia
    qf = ia.FlattenMlp(hidden_sizes=[H, H], input_size=OBS, output_size=N_ACT, ctx=ctx)
    tr = (ia.DoubleDQN if double_q else ia.DQN)(qf, max_batch=B)
    rng = np.random.default_rng(0)
    N = 20000
    rb = ia.SimpleReplayBuffer(N, OBS, 1, ctx=ctx)
    rb.add_rows(rng.normal(0, 1, (N, OBS)), rng.integers(0, N_ACT, (N, 1)), np.ones(N), rng.random(N) < 0.05, rng.normal(0, 1, (N, OBS)))
    if warm:
        tr.train_from_replay(rb, warm, B)
    ctx.sync()
    t0 = time.perf_counter()
    tr.train_from_replay(rb, steps, B)
    ctx.sync()
    return steps / (time.perf_counter() - t0)


def torch_rate(double_q, steps):
    import torch
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(0)

    def mlp(ps, x):
        h = x
        for i in range(0, len(ps) - 2, 2):
            h = torch.relu(h @ ps[i].T + ps[i + 1])
        return h @ ps[-2].T + ps[-1]
    dims, q = [OBS, H, H, N_ACT], []
    for i in range(3):
        q += [(torch.randn(dims[i + 1], dims[i], generator=g) * 0.1).to(dev).requires_grad_(True), torch.zeros(dims[i + 1], device=dev, requires_grad=True)]
    tq = [p.detach().clone() for p in q]
    opt = torch.optim.Adam(q, lr=1e-3)
    s, s2 = torch.randn(B, OBS, device=dev), torch.randn(B, OBS, device=dev)
    a, r, d = torch.randint(0, N_ACT, (B, 1), device=dev), torch.ones(B, device=dev), torch.zeros(B, device=dev)

    def step():
        with torch.no_grad():
            t2 = mlp(tq, s2)
            v = t2.gather(1, mlp(q, s2).max(1, keepdim=True)[1])[:, 0] if double_q else t2.max(1)[0]
            y = r + (1 - d) * 0.99 * v
        opt.zero_grad()
        ((mlp(q, s).gather(1, a)[:, 0] - y) ** 2).mean().backward()
        opt.step()
        with torch.no_grad():
            for pp, tp in zip(q, tq):
                tp.mul_(0.999).add_(pp * 0.001)
    for _ in range(50):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def cmd_step(args):
    if args.train_only:
        import ilswiss_amd as ia
        ctx = ia.Context(0, seed=5)
        res = dict(train_only_steps=args.train_only, steps_per_s=dqn_rate(ctx, False, args.train_only, warm=0))
        ctx.close()
        return res, None
    import torch   # before the library's context, as tools/bench_dsac.py does: torch then sees the GPU

    import ilswiss_amd as ia
    assert torch.cuda.is_available()
    ctx = ia.Context(0, seed=5)
    res = dict(metric="dqn_us_per_grad_step", unit="us/step", shape=dict(hidden=[H, H], batch=B, actions=N_ACT, obs=OBS), steps=args.steps,
               launches_per_step_design=LAUNCHES_PER_STEP_DESIGN)
    for rep in range(2):   # both legs twice, alternating: the second pass shows the run's own spread
        for name, dq in (("dqn", False), ("double_dqn", True)):
            res[f"{name}_us_per_step_pass{rep}"] = 1e6 / dqn_rate(ctx, dq, args.steps)
            res[f"torch_{name}_us_per_step_pass{rep}"] = 1e6 / torch_rate(dq, args.steps // 8)
    for name in ("dqn", "double_dqn"):
        res[f"{name}_us_per_step"] = min(res[f"{name}_us_per_step_pass{r}"] for r in range(2))
        res[f"torch_{name}_us_per_step"] = min(res[f"torch_{name}_us_per_step_pass{r}"] for r in range(2))
        res[f"{name}_torch_over_device"] = res[f"torch_{name}_us_per_step"] / res[f"{name}_us_per_step"]
    res["value"] = res["dqn_us_per_step"]
    ctx.close()
    return res, "dqn_bench.json"


def _fields(rets):
    return dict(mean_last_5=sum(rets[-5:]) / len(rets[-5:]), returns=rets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "learn"], nargs="?", default="step")
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--train-only", type=int, default=0, metavar="N", help="step: only N DQN steps, no warm-up, no other leg (for a kernel trace)")
    ap.add_argument("--task", choices=sorted(SPECS), default="cartpole")
    ap.add_argument("--seeds", type=int, nargs="*", default=[723894, 1, 2])
    ap.add_argument("--epochs", type=int, default=0, help="learn: cut the spec to this many epochs (0: the spec's)")
    ap.add_argument("--serial", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.what == "learn":
        import tempfile

        import bench_pendulum as bp
        with tempfile.TemporaryDirectory() as logs:   # the copies of progress.csv: the summary keeps their return column
            res = bp._run_spec(SPECS[args.task], "dqn_exp_script.py", args.seeds, args.epochs, logs, args.task, args.serial, prefix="dqn",
                               fields=_fields)
        name = f"dqn_{args.task}_summary.json"
    else:
        res, name = cmd_step(args)
    line = json.dumps(res)
    print(line)
    if name:
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
