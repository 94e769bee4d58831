#!/usr/bin/env python
"""MBPO ensemble measurements on one MI355X (prints one JSON line; --out writes it too):
  - us per ilsx_bnn_train_batch at the reference shape (E = 7, 4 x 200 SiLU, B = 256, Hopper dims) and its share of the fp32 MFMA peak
    (FLOPs from shapes: forward 2*B*sum(in*out) per member, backward ~2x that for dX + dW; the first layer's dX is not computed);
  - model-step rows/s at 1e5 rows (policy act + 7-member forward + sample + terminals + model-ring insert + compaction);
  - seconds per MBPO Hopper epoch at the reference schedule: 4 model trainings (model_train_freq 250) on a ring of `--real-rows` rows to
    early stopping, 4 rollouts of 1e5 rows at length `--rollout-length`, and 1000 SAC steps of B = 256 (20 per env step x 1000 env steps
    in the reference; this leg times one model training + one rollout and adds the SAC steps from bench.py's rate, see --sac-us);
  - baseline: the same train step as a torch-ROCm restatement on the same GPU (tests/mbpo_restatement.py's arithmetic).
Device-event timing after warm-up; the train-batch windows are taken --repeats times, library and restatement alternating, and the
JSON carries every window, the median and the spread (max - min) / median.  --hidden / --obs / --act / --terminal choose another shape
(the Humanoid spec: --hidden 400 --obs 45 --act 17 --terminal humanoid); --spec chooses the shipped spec --epoch runs."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP32_MFMA_PEAK = 157.3e12   # MI355X dense fp32 matrix peak (v_mfma_f32_16x16x4_f32), FLOP/s


def flops_per_step(E, in_dim, H, nh, D, B):
    sizes = [in_dim] + [H] * nh + [2 * D]
    fwd = sum(2 * B * sizes[i] * sizes[i + 1] for i in range(len(sizes) - 1))
    bwd_dx = sum(2 * B * sizes[i] * sizes[i + 1] for i in range(1, len(sizes) - 1))
    return E * (2 * fwd + bwd_dx)   # forward + dW (same as forward) + dX above the first layer


def timed_epochs(args):
    """run_scripts/mbpo_exp_script.py on exp_specs/mbpo/mbpo_hopper_hip.yaml as shipped (the reference's schedule: 5000 presampled steps,
    1000 env steps per epoch, the model trained every 250 steps on the whole real buffer to early stopping, 10^5-row rollouts, 20 SAC
    steps per env step on mixed batches), num_epochs cut to --epochs; progress.csv's "Epoch Time (s)" of the epochs after the first
    (which also holds the presampling)."""
    import csv
    import glob
    import subprocess
    import tempfile

    import yaml
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "mbpo", args.spec)))
    spec["constants"]["mbpo_params"]["num_epochs"] = args.epochs
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "spec.yaml")
        with open(path, "w") as f:
            yaml.safe_dump(spec, f)
        subprocess.run([sys.executable, os.path.join(ROOT, "run_scripts", "mbpo_exp_script.py"), "-e", path], cwd=d, check=True,
                       stdout=subprocess.DEVNULL)
        rows = list(csv.DictReader(open(glob.glob(os.path.join(d, "logs", "*", "*", "progress.csv"))[0])))
    t = [float(r["Epoch Time (s)"]) for r in rows]
    res = dict(metric=args.spec.replace("_hip.yaml", "") + "_epoch_s", spec=args.spec, epoch_s=t, epoch_s_after_first=round(float(np.mean(t[1:])), 3) if len(t) > 1 else None,
               train_time_s=[float(r["Train Time (s)"]) for r in rows], sample_time_s=[float(r["Sample Time (s)"]) for r in rows],
               mean_rollout_length=[float(r["mean_rollout_length"]) for r in rows], bnn_loss=[float(r["BNN Loss"]) for r in rows])
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--real-rows", type=int, default=20000)
    ap.add_argument("--rollout-length", type=int, default=1)
    ap.add_argument("--sac-us", type=float, default=57.0, help="us per SAC step (bench.py's headline) for the epoch estimate")
    ap.add_argument("--out", default=None)
    ap.add_argument("--epoch", action="store_true", help="instead: time MBPO Hopper epochs at the reference schedule through the run script")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--spec", default="mbpo_hopper_hip.yaml", help="with --epoch: the spec under exp_specs/mbpo/ to run")
    ap.add_argument("--hidden", type=int, default=200, help="ensemble hidden width")
    ap.add_argument("--obs", type=int, default=11, help="observation width (Hopper 11, ant_trunc_obs 27, humanoid_trunc_obs 45)")
    ap.add_argument("--act", type=int, default=3, help="action width (Hopper 3, Ant 8, Humanoid 17)")
    ap.add_argument("--terminal", default="hopper", help="terminal predicate of the model step")
    ap.add_argument("--repeats", type=int, default=3, help="timed train-batch windows per implementation, alternating")
    args = ap.parse_args()
    if args.epoch:
        return timed_epochs(args)
    import torch

    import ilswiss_amd as ia
    import mbpo_restatement as R
    from ilswiss_amd import _lib
    from ilswiss_amd.envs.terminals import get_terminal_func
    from ilswiss_amd.mbpo import BNN, BNNTrainer, terminal_kind
    from ilswiss_amd.replay import SimpleReplayBuffer

    ctx = ia.Context(0, seed=3)
    E, o, a, H, nh, B = 7, args.obs, args.act, args.hidden, 4, 256
    rng = np.random.default_rng(0)
    N = args.real_rows
    obs = rng.normal(0, 1, (N, o)).astype(np.float32)
    act = rng.uniform(-1, 1, (N, a)).astype(np.float32)
    rew = rng.normal(0, 1, N).astype(np.float32)
    nobs = (obs + 0.1 * rng.normal(0, 1, (N, o))).astype(np.float32)
    rb = SimpleReplayBuffer(N, o, a, ctx=ctx)
    rb.add_rows(obs, act, rew, np.zeros(N, np.uint8), nobs)
    bnn = BNN(hidden_sizes=[H] * nh, output_size=o + 1, input_size=o + a, num_nets=E, ctx=ctx, seed=1)
    tr = BNNTrainer(bnn, lr=1e-3, batch_size=B, num_elites=5, holdout_ratio=0.2, max_holdout=5000, log_freq=10**9,
                    logger=type("Q", (), {"log": staticmethod(lambda s: None)})())
    n_tab = B * (args.steps + args.warmup)
    table = ctx.from_numpy(rng.integers(0, N, (E, n_tab)).astype(np.int32), np.int32)
    import torch.cuda as tc
    stream = tc.ExternalStream(ctx.stream)

    def lib_window(first, count, timed):
        ev0, ev1 = tc.Event(enable_timing=True), tc.Event(enable_timing=True)
        ev0.record(stream)
        for s in range(first, first + count):
            tr._train_batch(rb, table, s * B, n_tab, B)
        ev1.record(stream)
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e3 / count if timed else None
    fl = flops_per_step(E, o + a, H, nh, o + 1, B)

    # torch-ROCm restatement of the same step on the same GPU
    dev = torch.device("cuda", 0)
    params = [torch.nn.Parameter(torch.as_tensor(p, device=dev)) for p in bnn.get_params()]
    opt = torch.optim.Adam([{"params": [params[2 * i], params[2 * i + 1]], "weight_decay": wd} for i, wd in enumerate(tr.fc_weight_decays)],
                           lr=1e-3)
    xt = torch.as_tensor(np.concatenate([obs, act], -1), device=dev)
    tt = torch.as_tensor(np.concatenate([rew[:, None], nobs - obs], -1), device=dev)
    mean, std = torch.zeros(o + a, device=dev), torch.ones(o + a, device=dev)
    idx_t = torch.as_tensor(rng.integers(0, N, (E, n_tab)), device=dev)

    def torch_step(s):
        ib = idx_t[:, s * B:(s + 1) * B]
        loss = torch.mean(R.compute_loss(params, mean, std, xt[ib], tt[ib])) + 0.105
        opt.zero_grad()
        loss.backward()
        opt.step()

    def torch_window(first, count, timed):
        e0, e1 = tc.Event(enable_timing=True), tc.Event(enable_timing=True)
        e0.record()
        for s in range(first, first + count):
            torch_step(s)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / count if timed else None
    lib_window(0, args.warmup, False)
    torch_window(0, args.warmup, False)
    lib_us, torch_us = [], []
    for _ in range(max(1, args.repeats)):      # the same index windows every time: the rows differ, the work does not
        lib_us.append(lib_window(args.warmup, args.steps, True))
        torch_us.append(torch_window(args.warmup, args.steps, True))
    us_train, us_torch = float(np.median(lib_us)), float(np.median(torch_us))

    def spread(v):
        return round((max(v) - min(v)) / float(np.median(v)), 4)

    # model step at 1e5 rows
    n = args.rows
    pol = ia.ReparamTanhMultivariateGaussianPolicy([256, 256], o, a, ctx=ctx)
    mring = SimpleReplayBuffer(10 * n, o, a, ctx=ctx)
    kind = terminal_kind(get_terminal_func(args.terminal))
    o0 = np.zeros((n, o), np.float32)
    o0[:, 0] = dict(ant=0.6).get(args.terminal, 1.25)      # a height inside every task's healthy range
    cur, nxt = ctx.from_numpy(o0), ctx.empty((n, o))
    el = np.arange(5, dtype=np.int32)
    ns = C.c_int()

    def step():
        _lib.check(ctx.lib.ilsx_mbpo_model_step(bnn.h, pol.h, mring.h, kind, cur.ptr, None, n, el.ctypes.data_as(C.c_void_p), 5, 0, None,
                                                None, None, None, nxt.ptr, C.byref(ns)))
    for _ in range(3):
        mring.clear()
        step()
    reps = 10
    mring.clear()
    t0 = time.perf_counter()
    for _ in range(reps):
        step()
    dt_step = (time.perf_counter() - t0) / reps

    # one model training of the reference schedule (early stopping) and one rollout at the given length
    np.random.seed(0)
    t0 = time.perf_counter()
    out = tr.train_step(rb)
    ctx.sync()
    t_model = time.perf_counter() - t0
    t_rollout = args.rollout_length * dt_step
    epoch_s = 4 * (t_model + t_rollout) + 1000 * 20 * args.sac_us * 1e-6
    res = dict(metric="mbpo_bnn_train_batch_us", shape=dict(E=E, obs=o, act=a, hidden=H, n_hidden=nh, B=B, terminal=args.terminal),
               bnn_train_batch_us=round(us_train, 2), bnn_train_batch_us_windows=[round(v, 2) for v in lib_us],
               bnn_train_batch_spread=spread(lib_us), torch_rocm_train_batch_us_windows=[round(v, 2) for v in torch_us],
               torch_rocm_train_batch_spread=spread(torch_us), gflop_per_step=round(fl / 1e9, 3),
               mfma_fp32_peak_share=round(fl / (us_train * 1e-6) / FP32_MFMA_PEAK, 4), torch_rocm_train_batch_us=round(us_torch, 2),
               speedup_vs_torch=round(us_torch / us_train, 2), model_step_rows_per_s=round(n / dt_step, 1), model_step_ms=round(dt_step * 1e3, 3),
               model_train_s=round(t_model, 3), model_train_epochs=out["epochs"], model_train_grad_steps=out["grad_updates"],
               real_rows=N, rollout_length=args.rollout_length, hopper_epoch_s_estimate=round(epoch_s, 2) if args.terminal == "hopper" else None)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
