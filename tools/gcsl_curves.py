#!/usr/bin/env python
"""Learning curves of GCSL on the point-reach stand-in: both specs (exp_specs/gcsl/gcsl_reach_hip.yaml, MSE; gcsl_reach_dis_hip.yaml,
CLASS) x seeds 0, 1, 2, `--epochs` epochs of the spec's schedule each (1000 env steps, one train step per env step after 1000, a 1000-step
deterministic evaluation), run through run_scripts/gcsl_exp_script.py in child processes.  One CSV row per (spec, seed, epoch).

    python tools/gcsl_curves.py [--epochs 6] [--out profiles/gcsl_learning_curves.csv]"""
import argparse
import csv
import os
import subprocess
import sys
import tempfile

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcsl_learning_curves.csv"))
    args = ap.parse_args()
    rows = []
    for spec in ("gcsl_reach_hip.yaml", "gcsl_reach_dis_hip.yaml"):
        for seed in (0, 1, 2):
            d = tempfile.mkdtemp(prefix="gcsl_curve_")
            s = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "gcsl", spec)))
            s["constants"]["rl_alg_params"]["num_epochs"] = args.epochs
            s["variables"]["seed"] = [seed]
            p = os.path.join(d, "spec.yaml")
            with open(p, "w") as f:
                yaml.safe_dump(s, f)
            subprocess.run([sys.executable, os.path.join(ROOT, "run_scripts", "gcsl_exp_script.py"), "-e", p], cwd=d, check=True,
                           capture_output=True)
            found = [os.path.join(r, "progress.csv") for r, _, fs in os.walk(os.path.join(d, "logs")) if "progress.csv" in fs]
            for r in csv.DictReader(open(found[0])):
                rows.append(dict(spec=spec, seed=seed, epoch=r["Epoch"], success_rate=r["Success Rate"], average_return=r["AverageReturn"],
                                 loss=r.get("CE Loss") or r.get("MSE"), accuracy=r.get("Accuracy", "")))
            print(spec, seed, rows[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)


if __name__ == "__main__":
    main()
