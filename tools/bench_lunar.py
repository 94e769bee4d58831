#!/usr/bin/env python
"""LunarLanderContinuous measurements on one MI355X (prints one JSON line, writes under --out-dir, default profiles/):

  rate    fused-rollout env-steps/s (random actions, replay insert) at 4096 and 65536 envs -> lunar_rate.json
  random  mean return and mean episode length of the device's uniform policy over 1024 whole episodes -> lunar_random.json
  parity  the parity protocol of tests/test_lunar_hip.py (70 envs, 120 auto-resetting steps) held to the 1e-9 cap: the largest
          relative state difference per step and the share of lane-steps near a switch -> lunar_parity.json, which the tests read
  sac     exp_specs/sac/sac_lunar_hip.yaml through its run script, one process per seed, cut to --epochs epochs
          -> lunar_sac_seed<S>.csv (progress.csv) and lunar_summary.json

`rate` under `rocprofv3 --kernel-trace --stats` gives the kernel table.  Timing and process handling are tools/bench_pendulum.py's."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bench_pendulum as bp  # noqa: E402

NAME = "lunarlandercont"


def env_rate(ctx, n, steps):
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    env = HipVectorEnv(NAME, n, seed=1, ctx=ctx)
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


def random_policy(ctx, n=1024, most=1000):
    """Every env plays its first episode to the end (a terminal, or `most` steps): n whole episodes, none cut short by the sample.  The
    rewards and terminals are read from the fused record of every step (a ring of capacity n: env i's record sits at slot i)."""
    import numpy as np
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    env = HipVectorEnv(NAME, n, seed=1, ctx=ctx)
    rb = ia.SimpleReplayBuffer(n, 8, 2, ctx=ctx)
    ret, length, done = np.zeros(n), np.zeros(n, int), np.zeros(n, bool)
    plus = 0
    for _ in range(most):
        env.rollout_step(replay=rb, max_path_length=most, random_actions=True)
        rec = rb._gather(np.arange(n))
        live = ~done
        ret[live] += rec["rewards"][live, 0]
        length[live] += 1
        ended = live & (rec["terminals"][:, 0] != 0)
        plus += int((rec["rewards"][ended, 0] == 100.0).sum())
        done |= ended
        if done.all():
            break
    env.close()
    return dict(metric="lunar_random_policy_return", episodes=n, value=float(ret.mean()), return_std=float(ret.std()),
                mean_episode_length=float(length.mean()), min_episode_length=int(length.min()), max_episode_length=int(length.max()),
                ended_by_terminal=int(done.sum()), ended_asleep=plus)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rate", "random", "parity", "sac"])
    ap.add_argument("--out-dir", default=os.path.join(bp.ROOT, "profiles"))
    ap.add_argument("--seeds", type=int, nargs="*", default=[723894, 1, 2])
    ap.add_argument("--epochs", type=int, default=0, help="cut the spec to this many epochs (0: the spec's)")
    ap.add_argument("--serial", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.what == "sac":
        res = bp._run_spec("sac/sac_lunar_hip.yaml", "sac_exp_script.py", args.seeds, args.epochs, args.out_dir, "sac", args.serial,
                           prefix="lunar", fields=lambda rets: dict(mean_last_5=sum(rets[-5:]) / len(rets[-5:])))
        name = "lunar_summary.json"
    else:
        import ilswiss_amd as ia
        ctx = ia.Context(0, seed=5)
        if args.what == "rate":
            res = dict(metric="lunar_env_steps_per_s", unit="env-steps/s")
            for n, steps in ((4096, 200), (65536, 100)):
                res[f"lunar_env_steps_per_s_{n}"] = env_rate(ctx, n, steps)
            res["value"] = res["lunar_env_steps_per_s_65536"]
            name = "lunar_rate.json"
        elif args.what == "random":
            res = random_policy(ctx)
            name = "lunar_random.json"
        else:
            sys.path.insert(0, os.path.join(bp.ROOT, "tests"))
            import test_lunar_hip as tl
            worst, near, total = tl.run_parity(ctx, tl.CAP)
            res = dict(metric="lunar_max_rel_state_diff_per_step", envs=70, steps=120, max_rel_state_diff=worst,
                       lane_steps=total, lane_steps_near_a_switch=near)
            name = "lunar_parity.json"
        ctx.close()
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, name), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
