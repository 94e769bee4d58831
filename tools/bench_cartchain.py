#!/usr/bin/env python
"""InvertedPendulum / InvertedDoublePendulum measurements on one MI355X (prints one JSON line, writes under --out-dir, default profiles/):

  rate   fused-rollout env-steps/s (random actions, replay insert) at 4096 and 65536 envs, both tasks and Pendulum in the same process
         -> cartchain_rate.json
  sac    a shipped spec (--task single|double) through its run script, one process per seed, cut to --epochs epochs
         -> cartchain_<task>_seed<S>.csv (progress.csv) and cartchain_<task>_summary.json (per seed: wall time, first / best / last
         evaluation return, the first epoch at the target return -- 1000.0 for single, 9300 for double -- and the later epochs below it)

`rate` under `rocprofv3 --kernel-trace --stats` gives the kernel table.  Timing and process handling are tools/bench_pendulum.py's."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bench_pendulum as bp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rate", "sac"])
    ap.add_argument("--task", choices=["single", "double"], default="double")
    ap.add_argument("--out-dir", default=os.path.join(bp.ROOT, "profiles"))
    ap.add_argument("--seeds", type=int, nargs="*", default=[723894, 1, 2])
    ap.add_argument("--epochs", type=int, default=0, help="cut the spec to this many epochs (0: the spec's)")
    ap.add_argument("--serial", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.what == "rate":
        import ilswiss_amd as ia
        ctx = ia.Context(0, seed=5)
        res = dict(metric="cartchain_env_steps_per_s", unit="env-steps/s")
        for n, steps in ((4096, 500), (65536, 200)):
            for name, o in (("invertedpendulum", 4), ("inverteddoublependulum", 11), ("pendulum", 3)):
                res[f"{name}_env_steps_per_s_{n}"] = bp.env_rate(ctx, name, n, steps, o)
        res["value"] = res["inverteddoublependulum_env_steps_per_s_65536"]
        ctx.close()
        name = "cartchain_rate.json"
    else:
        spec = "sac/sac_inverted_pendulum_hip.yaml" if args.task == "single" else "sac/sac_inverted_double_hip.yaml"
        target = 1000.0 if args.task == "single" else 9300.0    # the saturation score / a return only a balancing policy reaches

        def fields(rets):
            first = next((i for i, r in enumerate(rets) if r >= target), None)
            below = [i for i, r in enumerate(rets) if first is not None and i > first and r < target]
            return dict(target=target, first_epoch_at_target=first, later_epochs_below_target=below,
                        mean_last_10=sum(rets[-10:]) / len(rets[-10:]))

        res = bp._run_spec(spec, "sac_exp_script.py", args.seeds, args.epochs, args.out_dir, args.task, args.serial, prefix="cartchain",
                           fields=fields)
        name = f"cartchain_{args.task}_summary.json"
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, name), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
