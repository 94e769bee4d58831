#!/usr/bin/env python
"""Discrete SAC measurements on one MI355X (prints one JSON line; --out writes it too):
  - gradient steps/s of DiscreteSoftActorCritic.train_from_replay at the spec's shape (2 x 128, B = 128, n = 2) and at 2 x 256, B = 256;
  - launches per gradient step AS DESIGNED (DESIGN.md §16's launch list: replay gather, 3 forwards, 2 loss kernels, 2 backwards, 2 dW +
    Adam, 1 tick) — a count, not a measurement; `--train-only N` runs nothing but N gradient steps (after setup) so that a
    `rocprofv3 --kernel-trace --stats` table of it gives the measured count (profiles/dsac_train_kernel_stats.csv);
  - the same step as a torch-ROCm restatement on the same GPU (tests/dsac_restatement.py's arithmetic, torch.optim.Adam);
  - CartPole env-steps/s of the fused rollout (random actions, replay insert) at 4096 and 65536 envs.
Wall-clock timing after warm-up, the stream synchronised before and after every timed stretch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAUNCHES_PER_STEP_DESIGN = 11   # replay gather + fwd x 3 + critic loss + bwd + dW/Adam/Polyak + policy loss + bwd + dW/Adam + tick


def dsac_rate(ctx, H, B, n, steps, o=4, warm=50):
    import ilswiss_amd as ia
    from ilswiss_amd.discrete_sac import DiscreteSoftActorCritic
    hid = [H, H]
    pol = ia.DiscretePolicy(hidden_sizes=hid, obs_dim=o, action_dim=n, ctx=ctx)
    q1 = ia.FlattenMlp(hidden_sizes=hid, input_size=o, output_size=n, ctx=ctx)
    q2 = ia.FlattenMlp(hidden_sizes=hid, input_size=o, output_size=n, ctx=ctx)
    tr = DiscreteSoftActorCritic(pol, q1, q2, max_batch=B, alpha=0.05, discount=0.95, policy_lr=1e-4, qf_lr=1e-3, soft_target_tau=0.005)
    rng = np.random.default_rng(0)
    N = 20000
    rb = ia.SimpleReplayBuffer(N, o, 1, ctx=ctx)
    rb.add_rows(rng.normal(0, 1, (N, o)), rng.integers(0, n, (N, 1)), np.ones(N), rng.random(N) < 0.05, rng.normal(0, 1, (N, o)))
    if warm:
        tr.train_from_replay(rb, warm, B)
    ctx.sync()
    t0 = time.perf_counter()
    tr.train_from_replay(rb, steps, B)
    ctx.sync()
    return steps / (time.perf_counter() - t0)


def torch_rate(H, B, n, steps, o=4):
    import torch
    from dsac_restatement import mlp
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(0)

    def net():
        dims, ps = [o, H, H, n], []
        for i in range(3):
            ps += [(torch.randn(dims[i + 1], dims[i], generator=g) * 0.1).to(dev).requires_grad_(True),
                   torch.zeros(dims[i + 1], device=dev, requires_grad=True)]
        return ps
    pi, q1, q2 = net(), net(), net()
    tq1, tq2 = [p.detach().clone() for p in q1], [p.detach().clone() for p in q2]
    opts = [torch.optim.Adam(p, lr=1e-3) for p in (pi, q1, q2)]
    s, s2 = torch.randn(B, o, device=dev), torch.randn(B, o, device=dev)
    a, r, d = torch.randint(0, n, (B,), device=dev), torch.ones(B, device=dev), torch.zeros(B, device=dev)

    def step():
        with torch.no_grad():
            lp2 = torch.log_softmax(mlp(pi, s2), 1)
            p2 = lp2.exp()
            y = r + (1 - d) * 0.95 * ((p2 * torch.min(mlp(tq1, s2), mlp(tq2, s2))).sum(1) - 0.05 * (p2 * lp2).sum(1))
        for q, opt in ((q1, opts[1]), (q2, opts[2])):
            opt.zero_grad()
            (0.5 * ((mlp(q, s).gather(1, a[:, None])[:, 0] - y) ** 2).mean()).backward()
            opt.step()
        with torch.no_grad():
            qm = torch.min(mlp(q1, s), mlp(q2, s))
        opts[0].zero_grad()
        lp = torch.log_softmax(mlp(pi, s), 1)
        (-((lp.exp() * (qm - 0.05 * lp)).sum(1)).mean()).backward()
        opts[0].step()
        with torch.no_grad():
            for q, tq in ((q1, tq1), (q2, tq2)):
                for pp, tp in zip(q, tq):
                    tp.mul_(0.995).add_(pp * 0.005)
    for _ in range(30):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def env_rate(ctx, n, steps):
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    env = HipVectorEnv("cartpole", n, seed=1, ctx=ctx)
    rb = ia.SimpleReplayBuffer(4 * n, 4, 1, ctx=ctx)
    for _ in range(20):
        env.rollout_step(replay=rb, max_path_length=200, random_actions=True)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.rollout_step(replay=rb, max_path_length=200, random_actions=True)
    ctx.sync()
    dt = time.perf_counter() - t0
    env.close()
    return n * steps / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--train-only", type=int, default=0, metavar="N",
                    help="only N gradient steps at the spec's shape, no warm-up, no other leg (for a kernel trace)")
    args = ap.parse_args()
    if args.train_only:
        import ilswiss_amd as ia
        ctx = ia.Context(0, seed=5)
        print(json.dumps(dict(train_only_steps=args.train_only, steps_per_s=dsac_rate(ctx, 128, 128, 2, args.train_only, warm=0))))
        ctx.close()
        return
    import torch   # before the library's context, as tools/bench_mbpo.py does: torch then sees the GPU

    import ilswiss_amd as ia
    assert torch.cuda.is_available()
    ctx = ia.Context(0, seed=5)
    res = dict(metric="dsac_grad_steps_per_s", unit="steps/s", launches_per_step_design=LAUNCHES_PER_STEP_DESIGN)
    res["steps_per_s_h128_b128_n2"] = dsac_rate(ctx, 128, 128, 2, args.steps)
    res["steps_per_s_h256_b256_n2"] = dsac_rate(ctx, 256, 256, 2, args.steps)
    res["us_per_step_h128_b128_n2"] = 1e6 / res["steps_per_s_h128_b128_n2"]
    try:
        res["torch_steps_per_s_h128_b128_n2"] = torch_rate(128, 128, 2, args.steps // 4)
        res["torch_steps_per_s_h256_b256_n2"] = torch_rate(256, 256, 2, args.steps // 4)
    except Exception as e:   # noqa: BLE001 — the baseline is informative; its absence is reported, not hidden
        res["torch_error"] = repr(e)
    res["cartpole_env_steps_per_s_4096"] = env_rate(ctx, 4096, 500)
    res["cartpole_env_steps_per_s_65536"] = env_rate(ctx, 65536, 200)
    res["value"] = res["steps_per_s_h128_b128_n2"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
