#!/usr/bin/env python
"""The fused rollout step with a replay ring, with and without norm_obs ("Off-policy rollouts with norm_obs").

    python tools/bench_norm_rollout.py                 -> profiles/norm_rollout_bench.json
    python tools/bench_norm_rollout.py --kernels DIR   -> the kernel list of norm-off steps per library (to be run under
                                                          `rocprofv3 --kernel-trace --stats` by --kernel-list, a run of its own)
    python tools/bench_norm_rollout.py --kernel-list   -> profiles/norm_rollout_kernels.json
    python tools/bench_norm_rollout.py --learn         -> profiles/norm_pendulum_summary.json (learn())

Shapes: Hopper 4096 envs and Humanoid 1024 envs, a 256x256 tanh-Gaussian policy, ring of 2^18 rows.  Every window is a fresh process (the
library is chosen per process through ILSX_LIB), warmed up, then steps for at least a second and ends on a stream synchronise; the
libraries alternate window by window.
  norm-off: ilswiss_amd/libilsx_prev.so (the parent commit's build, see tools/README.md) against ilswiss_amd/libilsx.so.  Condition: the
            median of this build is no slower than the slowest window of the parent's own repeats.
  norm-on:  libilsx.so (one launch after the stepper) against ilswiss_amd/libilsx_chain.so (make -C ilswiss_amd/csrc VAR=chain
            VARFLAGS=-DILSX_NORM_RECORD_CHAIN: four launches after the stepper), beside the norm-off time.  Reports, not gates.
A library that is not there is reported as "not measured"."""
import argparse
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = (("hopper", 4096), ("humanoid", 1024))
LIBS = dict(parent="libilsx_prev.so", this="libilsx.so", chain="libilsx_chain.so")
WINDOWS = 5


def child(task, n_env, norm, seconds, fixed_steps):
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    ctx = ia.Context(0, seed=1)
    env = HipVectorEnv(task, n_env, seed=0, ctx=ctx, norm_obs=bool(norm))
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=[256, 256], obs_dim=env.obs_dim, action_dim=env.act_dim, ctx=ctx)
    rb = ia.SimpleReplayBuffer(1 << 18, env.obs_dim, env.act_dim, ctx=ctx)
    for _ in range(fixed_steps or 200):
        env.rollout_step(policy=pol, replay=rb, max_path_length=1000)
    ctx.sync()
    if fixed_steps:
        env.close()
        ctx.close()
        return
    steps, t0 = 0, time.perf_counter()
    while True:
        for _ in range(100):
            env.rollout_step(policy=pol, replay=rb, max_path_length=1000)
        steps += 100
        ctx.sync()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            break
    print(json.dumps(dict(us_per_step=1e6 * dt / steps, steps=steps, seconds=dt)))
    env.close()
    ctx.close()


def _lib(which):
    p = os.path.join(ROOT, "ilswiss_amd", LIBS[which])
    return p if os.path.exists(p) else None


def _window(which, task, n_env, norm, extra=()):
    env = dict(os.environ, ILSX_LIB=_lib(which))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", task, str(n_env), str(int(norm))] + list(extra)
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise SystemExit(f"{which} {task} {n_env} norm={norm}: exit {out.returncode}\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def _dist(xs):
    return dict(windows_us_per_step=[round(x, 3) for x in xs], median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def _alternate(pairs, task, n_env):
    """pairs: (label, library, norm) measured in turn, WINDOWS rounds."""
    got = {label: [] for label, _, _ in pairs}
    for _ in range(WINDOWS):
        for label, which, norm in pairs:
            got[label].append(_window(which, task, n_env, norm)["us_per_step"])
    return {k: _dist(v) for k, v in got.items()}


def measure():
    import torch
    if not torch.cuda.is_available():
        return dict(status="not measured (no GPU)")
    res = dict(device=torch.cuda.get_device_name(0), windows=WINDOWS, window_seconds=1.0, shapes={})
    for task, n_env in SHAPES:
        r = {}
        if _lib("parent"):
            off = _alternate((("parent", "parent", 0), ("this", "this", 0)), task, n_env)
            off["no_slowdown_beyond_parent_spread"] = off["this"]["median"] <= off["parent"]["max"]
            r["norm_off"] = off
        else:
            r["norm_off"] = dict(status="parent build not measured (ilswiss_amd/libilsx_prev.so is not there)")
        pairs = [("norm_off", "this", 0), ("single_launch", "this", 1)] + ([("four_launch_chain", "chain", 1)] if _lib("chain") else [])
        on = _alternate(pairs, task, n_env)
        on["launches_added"] = dict(single_launch=1, four_launch_chain=4)
        on["added_us_per_step"] = {k: round(on[k]["median"] - on["norm_off"]["median"], 3) for k in on if k in ("single_launch", "four_launch_chain")}
        if not _lib("chain"):
            on["four_launch_chain"] = "not measured (ilswiss_amd/libilsx_chain.so is not there)"
        r["norm_on"] = on
        res["shapes"][f"{task}_{n_env}"] = r
        print(json.dumps({f"{task}_{n_env}": r}), flush=True)
    return res


def kernels(out_dir):
    """20 norm-off steps (after 0 warm-up) of every shape on the library ILSX_LIB names: the workload of the kernel trace."""
    for task, n_env in SHAPES:
        child(task, n_env, 0, 0.0, 20)


def kernel_list():
    res = {}
    for which in ("parent", "this"):
        if not _lib(which):
            res[which] = "not measured"
            continue
        d = tempfile.mkdtemp(prefix=f"norm_kernels_{which}_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", which, "--", sys.executable, os.path.abspath(__file__), "--kernels", d]
        out = subprocess.run(cmd, env=dict(os.environ, ILSX_LIB=_lib(which)), capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise SystemExit(f"rocprofv3 ({which}): exit {out.returncode}\n{out.stderr[-2000:]}")
        dbs = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith(".db")]
        db = sqlite3.connect(sorted(dbs)[-1])
        res[which] = {name.split("(")[0].replace("void ", ""): int(calls) for name, calls in db.execute("select name,total_calls from top_kernels")}
        db.close()
        shutil.rmtree(d, ignore_errors=True)
    if isinstance(res.get("parent"), dict) and isinstance(res.get("this"), dict):
        res["equal"] = res["parent"] == res["this"]
    return res


def _progress(path):
    """The rows of a run's progress.csv copy, which is not kept: the summary carries what is reported."""
    import csv
    rows = list(csv.DictReader(open(path)))
    os.remove(path)
    return rows


def learn():
    """The Pendulum spec with and without the knob, three seeds each at full length (a spec's three processes at once): every epoch's
    evaluation return per run.  The first three epochs of the HalfCheetah pair, one run after the other: epoch times only."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_pendulum import _run_spec
    out = os.path.join(ROOT, "profiles")
    res = dict(pendulum={}, halfcheetah_first_epochs={})
    for tag, spec in (("plain", "sac/sac_pendulum_hip.yaml"), ("norm", "sac/sac_pendulum_norm_hip.yaml")):
        r = _run_spec(spec, "sac_alpha_exp_script.py", [723894, 1, 2], 0, out, tag, False, prefix="norm_pendulum")
        for seed, run in r["runs"].items():
            if run["rc"] == 0:
                rets = [float(x["AverageReturn"]) for x in _progress(os.path.join(out, f"norm_pendulum_{tag}_seed{seed}.csv"))]
                run["returns"], run["last_ten_epoch_mean"] = [round(r, 2) for r in rets], sum(rets[-10:]) / len(rets[-10:])
        res["pendulum"][tag] = r
    for tag, spec in (("plain", "sac/sac_halfcheetah_hip.yaml"), ("norm", "sac/sac_halfcheetah_norm_hip.yaml")):
        r = _run_spec(spec, "sac_alpha_exp_script.py", [0], 3, out, tag, True, prefix="norm_halfcheetah", fields=lambda rets: {})
        for seed, run in r["runs"].items():
            if run["rc"] == 0:
                rows = _progress(os.path.join(out, f"norm_halfcheetah_{tag}_seed{seed}.csv"))
                run["epoch_time_s"] = [float(x["Epoch Time (s)"]) for x in rows if "Epoch Time (s)" in x]
        res["halfcheetah_first_epochs"][tag] = r
    res["note"] = "no HalfCheetah learning curve has been measured: three epochs only, for the epoch time"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3)
    ap.add_argument("--kernels")
    ap.add_argument("--kernel-list", action="store_true")
    ap.add_argument("--learn", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), int(a.child[2]), 1.0, 0)
    if a.kernels:
        return kernels(a.kernels)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    if a.learn:
        name, res = "norm_pendulum_summary.json", learn()
    else:
        name, res = ("norm_rollout_kernels.json", kernel_list()) if a.kernel_list else ("norm_rollout_bench.json", measure())
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
