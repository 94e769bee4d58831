#!/usr/bin/env python
"""GCSL step times at the spec's shape (CLASS: H 300, B 128, 25 classes, input 56; MSE: H 256, B 128, 2 actions) on the device, against
an eager torch-ROCm restatement of the same step (tests/gcsl_restatement.py) on the same GPU, plus the GoalHorizonRL loop's iterations / s.
Step time = the HIP-event time of a window of `--steps` steps, divided by the steps; the median of 5 windows after warm-up.  The device
trainer runs on torch's current stream (the libilsx context is created on it), so one pair of events brackets either implementation's
window.  Writes profiles/gcsl_bench.json (or --out).

    python tools/bench_gcsl.py [--steps 200] [--out profiles/gcsl_bench.json] [--kernel-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gcsl_restatement as GR  # noqa: E402

O, GD, T = 4, 2, 50
D = O + GD + T


def windows(fn, steps, n=5, warm=50):
    """Median over n windows of the per-step time (us) between two HIP events recorded on torch's current stream around `steps` calls."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps * 1e3)
    return float(np.median(out)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcsl_bench.json"))
    ap.add_argument("--kernel-only", action="store_true", help="only the device CLASS steps (for a kernel trace)")
    args = ap.parse_args()
    import ilswiss_amd as ia
    from ilswiss_amd.gcsl import GCSL, CatagorialConditionPolicy, MlpGaussianAndEpsilonConditionPolicy
    from ilswiss_amd.her import Box
    import torch
    torch.cuda.init()
    ctx = ia.Context(0, seed=5, stream=torch.cuda.current_stream().cuda_stream)
    res = {}
    # ---- CLASS on the device: the input buffer is filled once, the step re-reads it (what train_from_replay's gather writes)
    H, B, n = 300, 128, 25
    pol = CatagorialConditionPolicy([H, H], O, GD + T, n, max_rows=B, ctx=ctx, seed=1)
    tr = GCSL(pol, mode="CLASS", use_horizons=True, goal_dim=GD, policy_lr=3e-4, max_batch=B)
    X, y = GR.cat_batches(3, B, 1, O, GD, T, n)[0]
    Xd, yd = ctx.from_numpy(X), ctx.from_numpy(y.astype(np.int32), np.int32)
    lib = ctx.lib
    lib.ilsx_gcsl_train_step(tr.h, Xd.ptr, yd.ptr, B, None)
    med, w = windows(lambda: lib.ilsx_bncat_train_step(pol.h, B, 3e-4, None), args.steps)
    res["class_step_us"], res["class_windows_us"] = med, w
    if args.kernel_only:
        print(json.dumps(res))
        return
    # ---- MSE on the device
    Hm, a = 256, 2
    mp = MlpGaussianAndEpsilonConditionPolicy([Hm, Hm], O, GD + T, a, action_space=Box(-np.ones(a), np.ones(a)), ctx=ctx)
    mt = GCSL(mp, mode="MSE", use_horizons=True, goal_dim=GD, policy_lr=3e-4, max_batch=B)
    Xm, am = GR.mse_batches(4, B, 1, O, GD, T, a)[0]
    Xmd, amd = ctx.from_numpy(Xm), ctx.from_numpy(am)
    med, w = windows(lambda: lib.ilsx_gcsl_train_step(mt.h, Xmd.ptr, amd.ptr, B, None), args.steps)
    res["mse_step_us"], res["mse_windows_us"] = med, w
    # ---- eager torch-ROCm restatements of the same steps on the same GPU
    dev = torch.device("cuda:0")
    rc = GR.CatRestatement(GR.cat_init(1, D, H, 2, n), D, H, 2, n)
    rc.net.to(dev)
    rc.opt = torch.optim.Adam(rc.net.params_in_order(), lr=3e-4)
    Xt, yt = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)

    def eager_cat():
        logits = rc.net(Xt)
        loss = torch.nn.functional.cross_entropy(logits, yt)
        acc = (torch.argmax(torch.softmax(logits, -1), -1) == yt).float().mean()
        rc.opt.zero_grad()
        loss.backward()
        rc.opt.step()
        return acc
    med, w = windows(eager_cat, args.steps)
    res["torch_class_step_us"], res["torch_class_windows_us"] = med, w
    rm = GR.MseRestatement(GR.mse_init(1, D, Hm, 2, a), D, Hm, 2, a)
    rm.net.to(dev)
    rm.opt = torch.optim.Adam(rm.net.params_in_order(), lr=3e-4)
    Xmt, amt = torch.from_numpy(Xm).to(dev), torch.from_numpy(am).to(dev)

    def eager_mse():
        loss = torch.sum((torch.tanh(rm.net(Xmt)) - amt) ** 2, -1).mean()
        rm.opt.zero_grad()
        loss.backward()
        rm.opt.step()
    med, w = windows(eager_mse, args.steps)
    res["torch_mse_step_us"], res["torch_mse_windows_us"] = med, w
    res["class_speedup"] = res["torch_class_step_us"] / res["class_step_us"]
    res["mse_speedup"] = res["torch_mse_step_us"] / res["mse_step_us"]
    # ---- the loop: env steps (one act call each) + one train step per env step after min_steps, CLASS spec
    from ilswiss_amd.envs import DiscretEnv
    from ilswiss_amd.gcsl import GoalHorizonRL
    from ilswiss_amd.her import PointReachEnv
    np.random.seed(0)
    env = DiscretEnv(PointReachEnv(seed=0), granularity=5)
    lp = CatagorialConditionPolicy([H, H], O, GD + T, n, max_rows=B, ctx=ctx, seed=2)
    lt = GCSL(lp, mode="CLASS", use_horizons=True, goal_dim=GD, policy_lr=3e-4, max_batch=B)
    loop = GoalHorizonRL(lt, env, lp, use_horizons=True, num_epochs=1, num_steps_per_epoch=3000, min_steps_before_training=1000,
                         num_steps_per_eval=50, batch_size=B, max_path_length=T)
    t0 = time.perf_counter()
    loop.train()
    res["loop_iters_per_s"] = 3000 / (time.perf_counter() - t0)
    res["timing"] = "HIP events on torch's current stream, shared by the libilsx context; median of 5 windows"
    res["shape"] = dict(class_=dict(H=H, B=B, n=n, D=D), mse=dict(H=Hm, B=B, a=a, D=D))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("windows_us")}))
    ctx.close()


if __name__ == "__main__":
    main()
