#!/usr/bin/env python
"""DDPG measurements on one MI355X at the Hopper spec's shape (o 11, a 3, 2 x 256, B 256); prints one JSON line and writes it to
--out (default profiles/ddpg_bench.json).  Records, never asserts:
  - us per DDPG gradient step (DDPG.train_from_replay, soft target updates as in the spec), the MEDIAN of `--windows` timed windows of
    `--steps` steps each, every window bracketed by stream synchronisations, after a warm-up of the same shape;
  - the TD3 step of this library, timed the same way in the same process, windows of the two alternating;
  - an eager torch-ROCm restatement of the DDPG step (tests/ddpg_restatement.py's arithmetic on the GPU, torch.optim.Adam);
  - the fused rollout step at 4096 Hopper envs, policy-driven, without and with OU exploration (us per vec step, env-steps/s).
LAUNCHES_PER_STEP_DESIGN is a count read off DESIGN.md section 21's launch list, not a measurement.
`--curves DIR`: instead of the timings, the shipped Pendulum spec for seeds 0-2 (profiles/ddpg_pendulum_*)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

O, A, H, B = 11, 3, 256, 256
# replay gather, fwd{pi_tgt, pi}, fwd{Q_tgt, Q}, fwd{Q(s, pi(s))} (column-split path), critic head, bwd{Q x 2}, policy head, bwd{pi},
# dW+Adam{pi}, dW+Adam{Q}, polyak, tick
LAUNCHES_PER_STEP_DESIGN = 12


def _ring(ia, ctx):
    rng = np.random.default_rng(0)
    N = 20000
    rb = ia.SimpleReplayBuffer(N, O, A, ctx=ctx)
    rb.add_rows(rng.normal(0, 1, (N, O)), np.tanh(rng.normal(0, 1, (N, A))), rng.normal(0, 1, N), rng.random(N) < 0.05, rng.normal(0, 1, (N, O)))
    return rb


def window_us(ctx, tr, rb, steps):
    ctx.sync()
    t0 = time.perf_counter()
    tr.train_from_replay(rb, steps, B)
    ctx.sync()
    return (time.perf_counter() - t0) / steps * 1e6


def step_times(ctx, steps, windows):
    import ilswiss_amd as ia
    from ilswiss_amd.ddpg import DDPG, MlpPolicy
    from ilswiss_amd.td3 import TD3, MlpGaussianNoisePolicy
    hid = [H, H]
    rb = _ring(ia, ctx)
    pol = MlpPolicy(hidden_sizes=hid, obs_dim=O, action_dim=A, output_activation="tanh", ctx=ctx)
    qf = ia.FlattenMlp(hidden_sizes=hid, input_size=O + A, output_size=1, ctx=ctx)
    ddpg = DDPG(pol, qf, max_batch=B, use_soft_update=True)
    tpol = MlpGaussianNoisePolicy(hidden_sizes=hid, obs_dim=O, action_dim=A, output_activation="tanh", policy_noise=0.2, policy_noise_clip=0.5, ctx=ctx)
    q1, q2 = (ia.FlattenMlp(hidden_sizes=hid, input_size=O + A, output_size=1, ctx=ctx) for _ in range(2))
    td3 = TD3(tpol, q1, q2, max_batch=B, policy_lr=3e-4, qf_lr=3e-4)
    for tr in (ddpg, td3):
        tr.train_from_replay(rb, 200, B)
        tr.end_epoch()
        tr.train_from_replay(rb, 10, B)   # takes the epoch's statistics, so that the timed windows ask for none
    d, t = [], []
    for _ in range(windows):   # alternating, so that both see the same machine
        d.append(window_us(ctx, ddpg, rb, steps))
        t.append(window_us(ctx, td3, rb, steps))
    return d, t


def torch_ddpg_us(steps, windows):
    import torch
    from dsac_restatement import mlp
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(0)

    def net(i, o):
        dims, ps = [i, H, H, o], []
        for k in range(3):
            ps += [(torch.randn(dims[k + 1], dims[k], generator=g) * 0.05).to(dev).requires_grad_(True),
                   torch.zeros(dims[k + 1], device=dev, requires_grad=True)]
        return ps
    pi, q = net(O, A), net(O + A, 1)
    tpi, tq = [p.detach().clone() for p in pi], [p.detach().clone() for p in q]
    opt_pi, opt_q = torch.optim.Adam(pi, lr=1e-4), torch.optim.Adam(q, lr=1e-3)
    s, s2, a = torch.randn(B, O, device=dev), torch.randn(B, O, device=dev), torch.rand(B, A, device=dev) * 2 - 1
    r, d = torch.randn(B, 1, device=dev), torch.zeros(B, 1, device=dev)

    def step():   # ddpg.py:102-235 with use_soft_update
        ploss = -mlp(q, torch.cat([s, torch.tanh(mlp(pi, s))], 1)).mean()
        with torch.no_grad():
            y = r + (1.0 - d) * 0.99 * mlp(tq, torch.cat([s2, torch.tanh(mlp(tpi, s2))], 1))
        qloss = ((mlp(q, torch.cat([s, a], 1)) - y) ** 2).mean()
        opt_pi.zero_grad()
        ploss.backward()
        opt_pi.step()
        opt_q.zero_grad()
        qloss.backward()
        opt_q.step()
        with torch.no_grad():
            for src, dst in ((pi, tpi), (q, tq)):
                for p, tp in zip(src, dst):
                    tp.mul_(0.99).add_(p * 0.01)
    for _ in range(50):
        step()
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e6)
    return out


def rollout_us(ctx, n_env, steps, windows):
    """us per fused vec step (policy inference -> [k_explore] -> physics -> replay record), the two variants' windows alternating."""
    import ilswiss_amd as ia
    from ilswiss_amd.ddpg import MlpPolicy, OUStrategy, PolicyWrappedWithExplorationStrategy
    from ilswiss_amd.envs import HipVectorEnv
    pol = MlpPolicy(hidden_sizes=[H, H], obs_dim=O, action_dim=A, output_activation="tanh", ctx=ctx)
    runs = {}
    for name in ("plain", "ou"):
        env = HipVectorEnv("hopper", n_env, seed=1, ctx=ctx)
        env.reset()
        p = pol if name == "plain" else PolicyWrappedWithExplorationStrategy(OUStrategy(env.single_action_space, max_sigma=0.3, min_sigma=0.1), pol)
        runs[name] = (env, p, ia.SimpleReplayBuffer(8 * n_env, O, A, ctx=ctx), [])
        for _ in range(50):
            env.rollout_step(p, runs[name][2], max_path_length=1000)
    for _ in range(windows):
        for name, (env, p, rb, out) in runs.items():
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                env.rollout_step(p, rb, max_path_length=1000)
            ctx.sync()
            out.append((time.perf_counter() - t0) / steps * 1e6)
    res = {name: out for name, (_, _, _, out) in runs.items()}
    for env, _, _, _ in runs.values():
        env.close()
    return res


def curves(out_dir, seeds=(0, 1, 2)):
    """The shipped Pendulum spec as it is, one run per seed through run_scripts/ddpg_exp_script.experiment: progress.csv of each run as
    <out_dir>/ddpg_pendulum_seed<k>.csv and the evaluation returns (deterministic policy) of first / best / last epoch as a summary."""
    import csv
    import shutil
    import tempfile

    import yaml
    sys.path.insert(0, os.path.join(ROOT, "run_scripts"))
    import ddpg_exp_script as script
    from _common import flatten_spec
    os.makedirs(out_dir, exist_ok=True)
    summary = {}
    for seed in seeds:
        v = flatten_spec(yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "ddpg", "ddpg_pendulum_hip.yaml"))))
        v["seed"] = seed
        log = tempfile.mkdtemp(prefix="ddpg_curve_")
        t0 = time.perf_counter()
        script.experiment(v, 0, log)
        wall = time.perf_counter() - t0
        dst = os.path.join(out_dir, f"ddpg_pendulum_seed{seed}.csv")
        shutil.copy(os.path.join(log, "progress.csv"), dst)
        shutil.rmtree(log, ignore_errors=True)
        ret = [float(r["AverageReturn"]) for r in csv.DictReader(open(dst))]
        summary[f"seed{seed}"] = dict(epochs=len(ret), first=ret[0], best=max(ret), last=ret[-1], last5_mean=float(np.mean(ret[-5:])), wall_s=wall)
    line = json.dumps(dict(spec="exp_specs/ddpg/ddpg_pendulum_hip.yaml", metric="AverageReturn (deterministic evaluation, 200-step episodes)", **summary))
    print(line)
    with open(os.path.join(out_dir, "ddpg_pendulum_summary.json"), "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10000, help="gradient steps per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rollout-steps", type=int, default=3000, help="vec steps per timed rollout window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddpg_bench.json"))
    ap.add_argument("--curves", default=None, metavar="DIR", help="instead: run the shipped Pendulum spec for seeds 0-2, write the progress files to DIR")
    args = ap.parse_args()
    if args.curves:
        return curves(args.curves)
    import torch   # before the library's context, as tools/bench_dsac.py does: torch then sees the GPU

    import ilswiss_amd as ia
    assert torch.cuda.is_available(), "tools/bench_ddpg.py measures on the GPU; there is none"
    ctx = ia.Context(0, seed=5)
    med = statistics.median
    res = dict(metric="ddpg_us_per_step", unit="us", shape=dict(obs=O, act=A, hidden=[H, H], batch=B), steps_per_window=args.steps,
               windows=args.windows, launches_per_step_design=LAUNCHES_PER_STEP_DESIGN)
    d, t = step_times(ctx, args.steps, args.windows)
    res.update(ddpg_us_per_step=med(d), ddpg_us_windows=d, td3_us_per_step=med(t), td3_us_windows=t)
    try:
        tw = torch_ddpg_us(max(args.steps // 4, 1), args.windows)
        res.update(torch_ddpg_us_per_step=med(tw), torch_ddpg_us_windows=tw)
    except Exception as e:   # noqa: BLE001 — the baseline is informative; its absence is reported, not hidden
        res["torch_error"] = repr(e)
    ro = rollout_us(ctx, 4096, args.rollout_steps, args.windows)
    res.update(rollout_us_per_vec_step_4096=med(ro["plain"]), rollout_ou_us_per_vec_step_4096=med(ro["ou"]),
               rollout_us_windows=ro["plain"], rollout_ou_us_windows=ro["ou"],
               rollout_env_steps_per_s_4096=4096 / med(ro["plain"]) * 1e6, rollout_ou_env_steps_per_s_4096=4096 / med(ro["ou"]) * 1e6)
    res["value"] = res["ddpg_us_per_step"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
