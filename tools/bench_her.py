#!/usr/bin/env python
"""Vectorised-HER measurements on one MI355X (prints one JSON line per part, writes under --out-dir, default profiles/):

  bench   -> her_bench.json, three parts in one process, every figure as [min, mean, max] over --reps repetitions of a timed window that
          ends in a device synchronise, after a warm-up of the same shape; the two sides of a comparison alternate:
            stepper   fused-rollout env-steps/s (random actions, replay insert) of `point-reach` at 4096 and 65536 envs, beside Pendulum and
                      the lander in the same process (tools/bench_gymcc.py's measurement)
            sampler   us per hindsight batch at B = 128 and 256 on ONE ring: ilsx_her_sample (draws in the kernel) against
                      DeviceHindsightReplayBuffer.random_batch (host draws + index upload + ilsx_her_gather)
            loop      env-steps/s and gradient-steps/s of her.VecHER at env_num 1, 64 and 4096, one gradient step per env step (the specs'
                      schedule), against her.HER on the host env: this tree's, and — with --parent-tree DIR, a built checkout of the commit
                      before the vectorised loop — that tree's, in a process of its own, alternated with the device loop's runs
  curves  three seeds of each vectorised spec at full length through its run script -> her_vec_<td3|sac>_seed<S>.csv (progress.csv) and
          her_vec_summary.json (the success rate per epoch)
  host-loop   (used by `bench`) her.HER's env-steps/s in this process, from the tree given by --tree

Timing a launch-bound loop measures the host as much as the device: the figures are end-to-end rates of the loops as a user runs them."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _mmm(xs):
    return [min(xs), sum(xs) / len(xs), max(xs)]


# ---------------------------------------------------------------------------------------------- stepper
def _stepper(ctx, reps):
    import ilswiss_amd as ia
    from ilswiss_amd.envs import HipVectorEnv
    out = {}
    for n, steps in ((4096, 500), (65536, 200)):
        for name in ("point-reach", "pendulum", "lunarlandercont"):
            env = HipVectorEnv(name, n, seed=1, ctx=ctx)
            rb = ia.SimpleReplayBuffer(4 * n, env.obs_dim, env.act_dim, ctx=ctx)
            rates = []
            for rep in range(reps + 1):       # the first window is the warm-up
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(steps):
                    env.rollout_step(replay=rb, max_path_length=200, random_actions=True)
                ctx.sync()
                rates.append(n * steps / (time.perf_counter() - t0))
            out[f"{name}_env_steps_per_s_{n}"] = _mmm(rates[1:])
            env.close()
    return out


# ---------------------------------------------------------------------------------------------- sampler
def _sampler(ctx, reps, calls=2000):
    import ctypes as C

    import numpy as np
    from ilswiss_amd import _lib, her
    env = her.PointReachEnv(seed=0)
    rb = her.DeviceHindsightReplayBuffer(100000, env, random_seed=3, ctx=ctx)
    obs = env.reset()
    rng = np.random.default_rng(0)
    for k in range(200 * 50):                                  # 200 episodes of 50 steps, through the reference's cursor logic
        a = rng.uniform(-1, 1, 2).astype(np.float32)
        nobs, r, d, _ = env.step(a)
        rb.add_sample(obs, a, r, d, nobs)
        obs = nobs
        if (k + 1) % 50 == 0:
            rb.terminate_episode()
            _lib.check(ctx.lib.ilsx_replay_terminate_episode(rb.h))   # the ring's own trajectory table (the class keeps the reference's on the host)
            obs = env.reset()
    lib, out = ctx.lib, {}
    for B in (128, 256):
        o5 = [ctx.empty((B, 6)), ctx.empty((B, 2)), ctx.empty((B,)), ctx.empty((B,)), ctx.empty((B, 6))]
        di, dr = ctx.empty((B,), np.int64), ctx.empty((B,), np.int64)
        p5, thr = [x.ptr for x in o5], C.c_float(env.tol)

        def device():
            for _ in range(calls):
                _lib.check(lib.ilsx_her_sample(rb.h, B, int(0.8 * B), 1, 4, 2, 0, thr, None, *p5, di.ptr, dr.ptr))

        def host():
            for _ in range(calls):
                rb.random_batch(B)
        t = {"her_sample": [], "host_draws_gather": []}
        for rep in range(reps + 1):
            for name, fn in (("her_sample", device), ("host_draws_gather", host)):
                ctx.sync()
                t0 = time.perf_counter()
                fn()
                ctx.sync()
                t[name].append((time.perf_counter() - t0) / calls * 1e6)
        for name in t:
            out[f"{name}_us_B{B}"] = _mmm(t[name][1:])
    return out


# ---------------------------------------------------------------------------------------------- loops
def _vec_loop(ctx, env_num, grad_steps=6400):
    """-> a function timing one window of her.VecHER at env_num envs, one gradient step per env step: (env-steps/s, gradient-steps/s)"""
    import numpy as np
    import ilswiss_amd as ia
    from ilswiss_amd import her
    from ilswiss_amd.envs import HipVectorEnv
    np.random.seed(0)
    env, ev = HipVectorEnv("point-reach", env_num, seed=1, ctx=ctx), HipVectorEnv("point-reach", 16, seed=2, ctx=ctx)
    q1, q2 = ia.FlattenMlp([256, 256], 1, 8, ctx=ctx), ia.FlattenMlp([256, 256], 1, 8, ctx=ctx)
    pol = her.MlpGaussianAndEpsilonPolicy([256, 256], 4, 2, action_space=env.single_action_space, condition_dim=2, output_activation="tanh", ctx=ctx)
    tr = her.TD3(pol, q1, q2, discount=0.99, policy_lr=3e-4, qf_lr=3e-4, max_batch=128)
    tr.eval_statistics = {}                                    # no statistics read-back inside the timed windows
    alg = her.VecHER(tr, env, env, ev, pol, batch_size=128, max_path_length=50, replay_buffer_size=max(100000, 60 * env_num),
                     num_steps_between_train_calls=env_num, num_train_steps_per_train_call=env_num, min_steps_before_training=50 * env_num)
    vec_steps = max(2, grad_steps // env_num)

    def window(k=vec_steps):
        ctx.sync()
        t0 = time.perf_counter()
        g0 = alg._n_grad_steps_total
        for _ in range(k):
            alg._vec_step()
            if alg._train_due() and alg._can_train():
                alg._count_train_call()
                tr.train_from_replay(alg.replay_buffer, alg.num_train_steps_per_train_call, alg.batch_size)
        ctx.sync()
        dt = time.perf_counter() - t0
        return k * env_num / dt, (alg._n_grad_steps_total - g0) / dt
    window(51)                                                 # fills the ring past min_steps_before_training, warms every shape
    return window


def _host_loop(steps):
    """her.HER on the host env with the host spec's schedule (one gradient step per env step) -> a function timing one window"""
    import numpy as np
    import ilswiss_amd as ia
    from ilswiss_amd import her
    ctx = ia.Context(0, seed=5)
    np.random.seed(0)
    env = her.PointReachEnv(seed=1)
    q1, q2 = ia.FlattenMlp([256, 256], 1, 8, ctx=ctx), ia.FlattenMlp([256, 256], 1, 8, ctx=ctx)
    pol = her.MlpGaussianAndEpsilonPolicy([256, 256], 4, 2, action_space=env.action_space, condition_dim=2, output_activation="tanh", ctx=ctx)
    tr = her.TD3(pol, q1, q2, discount=0.99, policy_lr=3e-4, qf_lr=3e-4, max_batch=128)
    alg = her.HER(tr, env, pol, num_epochs=1, num_steps_per_epoch=steps, min_steps_before_training=200, max_path_length=50, batch_size=128,
                  replay_buffer_size=100000, num_steps_per_eval=1)

    def window():
        tr.eval_statistics = {}
        g0 = alg._n_train_steps_total
        ctx.sync()
        t0 = time.perf_counter()
        alg.train()
        ctx.sync()
        dt = time.perf_counter() - t0
        return steps / dt, (alg._n_train_steps_total - g0) / dt
    window()                                                   # fills the buffer, warms every shape
    return window


def cmd_host_loop(args):
    sys.path.insert(0, args.tree)
    w = _host_loop(args.steps)
    print(json.dumps([w() for _ in range(args.reps)]))


def _host_loop_proc(tree, steps, reps):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "host-loop", "--tree", tree, "--steps", str(steps), "--reps", str(reps)],
                       capture_output=True, text=True, cwd=tree)
    if r.returncode != 0:
        raise RuntimeError(f"host loop in {tree} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def cmd_bench(args):
    sys.path.insert(0, ROOT)
    import ilswiss_amd as ia
    ctx = ia.Context(0, seed=5)
    res = dict(metric="her_vec", reps=args.reps, stepper=_stepper(ctx, args.reps), sampler=_sampler(ctx, args.reps))
    loops = {n: _vec_loop(ctx, n) for n in (1, 64, 4096)}
    runs = {f"vec_her_{n}": [] for n in loops}
    runs["host_her_this_tree"], runs["host_her_parent_tree"] = [], []
    for rep in range(args.reps):                               # alternated: device loops, this tree's host loop, the parent's host loop
        for n, w in loops.items():
            runs[f"vec_her_{n}"].append(w())
        runs["host_her_this_tree"] += _host_loop_proc(ROOT, args.host_steps, 1)
        if args.parent_tree:
            runs["host_her_parent_tree"] += _host_loop_proc(os.path.abspath(args.parent_tree), args.host_steps, 1)
    res["loop"] = {k: dict(env_steps_per_s=_mmm([x[0] for x in v]), grad_steps_per_s=_mmm([x[1] for x in v])) for k, v in runs.items() if v}
    if not args.parent_tree:
        res["loop"]["host_her_parent_tree"] = "not measured (no --parent-tree)"
    ctx.close()
    return res, "her_bench.json"


# ---------------------------------------------------------------------------------------------- learning curves
def cmd_curves(args):
    sys.path.insert(0, HERE)
    import bench_pendulum as bp
    res = dict(metric="her_vec_success_rate", seeds=args.seeds)
    for tag, spec, script in (("td3", "her/her_reach_td3_vec_hip.yaml", "her_td3_exp_script.py"),
                              ("sac", "her/her_reach_sac_vec_hip.yaml", "her_sac_exp_script.py")):
        r = bp._run_spec(spec, script, args.seeds, args.epochs, args.out_dir, tag, args.serial, prefix="her_vec", fields=lambda rets: {})
        for seed, run in r["runs"].items():
            path = os.path.join(args.out_dir, f"her_vec_{tag}_seed{seed}.csv")
            if os.path.exists(path):
                run["success_rate"] = [float(x["Success Rate"]) for x in csv.DictReader(open(path))]
        res[tag] = r
    return res, "her_vec_summary.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["bench", "curves", "host-loop"])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the commit before the vectorised loop (bench: the host loop there)")
    ap.add_argument("--host-steps", type=int, default=3000)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--epochs", type=int, default=0, help="cut the specs to this many epochs (0: the specs')")
    ap.add_argument("--serial", action="store_true")
    args = ap.parse_args()
    if args.what == "host-loop":
        return cmd_host_loop(args)
    os.makedirs(args.out_dir, exist_ok=True)
    res, name = cmd_bench(args) if args.what == "bench" else cmd_curves(args)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, name), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
