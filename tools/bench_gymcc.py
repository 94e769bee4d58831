#!/usr/bin/env python
"""MountainCarContinuous / MountainCar / Acrobot measurements on one MI355X (prints one JSON line, writes under --out-dir, default
profiles/):

  rate    fused-rollout env-steps/s (random actions, replay insert) at 4096 and 65536 envs, every task and Pendulum in the same process
          -> gymcc_rate.json
  sac     a task's spec through its run script, one process per seed, cut to --epochs epochs: --task acrobot
          (exp_specs/sac/sac_acrobot_d_hip.yaml), mountaincar (sac_mountaincar_d_hip.yaml) or mountaincarcont (sac_mountain_hip.yaml)
          -> gymcc_<task>_sac_seed<S>.csv (progress.csv) and gymcc_<task>_summary.json

`rate` under `rocprofv3 --kernel-trace --stats` gives the kernel table.  Timing and process handling are tools/bench_pendulum.py's."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bench_pendulum as bp  # noqa: E402

TASKS = {"mountaincarcont": (2, "sac/sac_mountain_hip.yaml", "sac_exp_script.py"),
         "mountaincar": (2, "sac/sac_mountaincar_d_hip.yaml", "discrete_sac_exp_script.py"),
         "acrobot": (6, "sac/sac_acrobot_d_hip.yaml", "discrete_sac_exp_script.py")}


def _fields(rets):
    return dict(mean_last_5=sum(rets[-5:]) / len(rets[-5:]), returns=rets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rate", "sac"])
    ap.add_argument("--task", choices=sorted(TASKS), default="acrobot")
    ap.add_argument("--out-dir", default=os.path.join(bp.ROOT, "profiles"))
    ap.add_argument("--seeds", type=int, nargs="*", default=[723894, 1, 2])
    ap.add_argument("--epochs", type=int, default=0, help="cut the spec to this many epochs (0: the spec's)")
    ap.add_argument("--serial", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.what == "sac":
        _, spec, script = TASKS[args.task]
        res = bp._run_spec(spec, script, args.seeds, args.epochs, args.out_dir, "sac", args.serial, prefix=f"gymcc_{args.task}", fields=_fields)
        name = f"gymcc_{args.task}_summary.json"
    else:
        import ilswiss_amd as ia
        ctx = ia.Context(0, seed=5)
        res = dict(metric="gymcc_env_steps_per_s", unit="env-steps/s")
        for n, steps in ((4096, 500), (65536, 200)):
            for task, o in [("pendulum", 3)] + [(t, v[0]) for t, v in TASKS.items()] + [("pendulum_again", 3)]:   # Pendulum twice: the run's own spread
                res[f"{task}_env_steps_per_s_{n}"] = bp.env_rate(ctx, task.split("_")[0], n, steps, o)
        res["value"] = res["acrobot_env_steps_per_s_65536"]
        ctx.close()
        name = "gymcc_rate.json"
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, name), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
