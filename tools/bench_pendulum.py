#!/usr/bin/env python
"""Pendulum measurements on one MI355X (each subcommand prints one JSON line and writes its files under --out-dir, default profiles/):

  rate   fused-rollout env-steps/s (random actions, replay insert) at 4096 and 65536 envs, Pendulum and CartPole in the same process
         -> pendulum_rate.json
  sac    the shipped SAC-alpha spec (exp_specs/sac/sac_pendulum_hip.yaml) through its run script, one process per seed, all seeds at once
         (--serial: one after another, for an uncontended wall time per epoch) -> pendulum_sac_seed<S>.csv (progress.csv) and
         pendulum_sac_summary.json (wall time per run and per epoch, the best and last evaluation returns)
  ppo    the PPO spec cut to --epochs epochs -> pendulum_ppo_seed<S>.csv, pendulum_ppo_summary.json

`sac --epochs 2 --seeds 723894 --serial` under `rocprofv3 --kernel-trace --stats` gives the kernel table of the spec's first epochs.
Wall-clock timing after warm-up; the stream synchronised before and after every timed stretch."""
import argparse
import csv
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def env_rate(ctx, name, n, steps, o):
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    env = HipVectorEnv(name, n, seed=1, ctx=ctx)
    rb = ia.SimpleReplayBuffer(4 * n, o, 1, ctx=ctx)
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


def cmd_rate(args):
    import ilswiss_amd as ia
    ctx = ia.Context(0, seed=5)
    res = dict(metric="pendulum_env_steps_per_s", unit="env-steps/s")
    for n, steps in ((4096, 500), (65536, 200)):
        res[f"pendulum_env_steps_per_s_{n}"] = env_rate(ctx, "pendulum", n, steps, 3)
        res[f"cartpole_env_steps_per_s_{n}"] = env_rate(ctx, "cartpole", n, steps, 4)
    res["value"] = res["pendulum_env_steps_per_s_65536"]
    ctx.close()
    return res, "pendulum_rate.json"


def _pendulum_fields(rets):
    return dict(first_epoch_above_minus_1000=next((i for i, r in enumerate(rets) if r > -1000), None))


def _run_spec(spec_rel, script, seeds, epochs, out_dir, tag, serial, over=None, prefix="pendulum", fields=_pendulum_fields):
    """prefix: the copies of progress.csv are <prefix>_<tag>_seed<S>.csv; fields(returns) -> the task's own entries of a run's summary."""
    import yaml
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", spec_rel)))
    if epochs:
        spec["constants"]["rl_alg_params"]["num_epochs"] = epochs
    spec["constants"]["rl_alg_params"].update(over or {})
    tmp = tempfile.mkdtemp(prefix=f"pend_{tag}_")
    procs, res = [], dict(spec=spec_rel, epochs=spec["constants"]["rl_alg_params"]["num_epochs"], serial=bool(serial), runs={})
    try:
        def start(seed):
            d = os.path.join(tmp, f"s{seed}")
            os.makedirs(d)
            s = json.loads(json.dumps(spec))
            s["variables"]["seed"] = [seed]
            with open(os.path.join(d, "spec.yaml"), "w") as f:
                yaml.safe_dump(s, f)
            log = open(os.path.join(d, "stdout.txt"), "w")
            p = subprocess.Popen([sys.executable, os.path.join(ROOT, "run_scripts", script), "-e", os.path.join(d, "spec.yaml")], cwd=d,
                                 stdout=log, stderr=subprocess.STDOUT)
            return seed, d, p, time.perf_counter()

        def finish(seed, d, p, t0):
            rc = p.wait()
            wall = time.perf_counter() - t0
            found = [os.path.join(r, "progress.csv") for r, _, fs in os.walk(os.path.join(d, "logs")) if "progress.csv" in fs]
            run = dict(rc=rc, wall_s=wall)
            if rc != 0 or not found:
                run["tail"] = open(os.path.join(d, "stdout.txt")).read()[-2000:]
            else:
                shutil.copy(found[0], os.path.join(out_dir, f"{prefix}_{tag}_seed{seed}.csv"))
                rows = list(csv.DictReader(open(found[0])))
                rets = [float(r["AverageReturn"]) for r in rows]
                run.update(n_epochs=len(rows), wall_s_per_epoch=wall / max(1, len(rows)), last_return=rets[-1], best_return=max(rets),
                           best_epoch=int(max(range(len(rets)), key=rets.__getitem__)), first_return=rets[0], **fields(rets))
            res["runs"][str(seed)] = run

        if serial:
            for seed in seeds:
                finish(*start(seed))
        else:
            procs = [start(seed) for seed in seeds]
            for p in procs:
                finish(*p)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rate", "sac", "ppo"])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--seeds", type=int, nargs="*", default=None)
    ap.add_argument("--epochs", type=int, default=0, help="cut the spec to this many epochs (0: the spec's)")
    ap.add_argument("--serial", action="store_true", help="one seed after another")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.what == "rate":
        res, name = cmd_rate(args)
    elif args.what == "sac":
        res = _run_spec("sac/sac_pendulum_hip.yaml", "sac_alpha_exp_script.py", args.seeds or [723894, 1, 2], args.epochs, args.out_dir,
                        "sac", args.serial)
        name = "pendulum_sac_summary.json"
    else:
        res = _run_spec("ppo/ppo_pendulum_hip.yaml", "ppo_exp_script.py", args.seeds or [0], args.epochs or 40, args.out_dir, "ppo",
                        args.serial)
        name = "pendulum_ppo_summary.json"
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, name), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
