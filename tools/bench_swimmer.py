#!/usr/bin/env python
"""Swimmer measurements on one MI355X (prints one JSON line, writes under --out-dir, default profiles/):

  rate    fused-rollout env-steps/s (random actions, replay insert) at 4096 and 65536 envs -> swimmer_rate.json
  random  the random-policy return over whole 1000-step episodes of 1024 envs -> swimmer_random.json
  sac     exp_specs/sac/sac_swimmer_hip.yaml through its run script, one process per seed, cut to --epochs epochs
          -> swimmer_sac_seed<S>.csv (progress.csv) and swimmer_summary.json

`rate` under `rocprofv3 --kernel-trace --stats` gives the kernel table.  Timing and process handling are tools/bench_pendulum.py's."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bench_pendulum as bp  # noqa: E402


def env_rate(ctx, n, steps):
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    env = HipVectorEnv("swimmer", n, seed=1, ctx=ctx)
    rb = ia.SimpleReplayBuffer(4 * n, 8, 2, ctx=ctx)
    for _ in range(20):
        env.rollout_step(replay=rb, max_path_length=1000, random_actions=True)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.rollout_step(replay=rb, max_path_length=1000, random_actions=True)
    ctx.sync()
    dt = time.perf_counter() - t0
    env.close()
    return n * steps / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rate", "random", "sac"])
    ap.add_argument("--out-dir", default=os.path.join(bp.ROOT, "profiles"))
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--epochs", type=int, default=0, help="cut the spec to this many epochs (0: the spec's)")
    ap.add_argument("--serial", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.what == "sac":
        res = bp._run_spec("sac/sac_swimmer_hip.yaml", "sac_alpha_exp_script.py", args.seeds, args.epochs, args.out_dir, "sac", args.serial,
                           prefix="swimmer", fields=lambda rets: dict(mean_last_10=sum(rets[-10:]) / len(rets[-10:])))
        name = "swimmer_summary.json"
    else:
        import ilswiss_amd as ia
        ctx = ia.Context(0, seed=5)
        if args.what == "rate":
            res = dict(metric="swimmer_env_steps_per_s", unit="env-steps/s")
            for n, steps in ((4096, 200), (65536, 100)):
                res[f"swimmer_env_steps_per_s_{n}"] = env_rate(ctx, n, steps)
            res["value"] = res["swimmer_env_steps_per_s_65536"]
            name = "swimmer_rate.json"
        else:
            from ilswiss_amd.envs import HipVectorEnv
            n = 1024
            env = HipVectorEnv("swimmer", n, seed=1, ctx=ctx)
            env.rollout_stats(reset=True)
            for _ in range(1000):
                env.rollout_step(max_path_length=1000, random_actions=True)
            e, r = env.rollout_stats(reset=True)
            env.close()
            res = dict(metric="swimmer_random_policy_return", episodes=e, value=r / max(e, 1.0))
            name = "swimmer_random.json"
        ctx.close()
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, name), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
