#!/usr/bin/env python
"""Do two builds of the library step the SAME states to the SAME bits?  (The acceptance check of a stepper rewrite that claims unchanged arithmetic.)

    ILSX_LIB=ilswiss_amd/libilsx_<old>.so python tools/stepper_bits.py dump /tmp/old.npz [steps]
    python tools/stepper_bits.py dump /tmp/new.npz
    python tools/stepper_bits.py compare /tmp/old.npz /tmp/new.npz

dump: every model, 256 envs (Ant / Humanoid: 64), 300 auto-reset rollout steps with random actions from the seeded device stream — contacts,
joint limits, terminations and resets on the way.  The classic-control tasks and Swimmer run with a path limit of 23 steps, so that every
env is reset a dozen times.  Kept per task: qpos / qvel of every env, the rows of the replay ring (every column of the fused record,
the absorbing pair included) and the rollout statistics; then, from a fresh env, a second pass in path mode (whole episodes staged and
flushed) with its state, rows, episode boundaries and statistics.  compare: exact equality, or the largest difference.  One number cannot
be held to exact equality: the sum of the finished episodes' returns is built by float64 atomic additions whose order changes from run to
run of the SAME build, so it is held to the rounding of a reordered sum, 2 n u sum|x| with n the number of episodes and sum|x| bounded by the
sum of the |rewards| in the ring; the episode count beside it is exact."""
import sys

import numpy as np

sys.path.insert(0, ".")

TASKS = (("hopper", 256, 1000), ("walker", 256, 1000), ("halfcheetah", 256, 1000), ("ant", 64, 1000), ("humanoid", 64, 1000),
         ("cartpole", 256, 23), ("pendulum", 256, 23), ("invertedpendulum", 256, 23), ("inverteddoublependulum", 256, 23), ("swimmer", 256, 23))


def _rollout(ia, ctx, name, n, steps, max_path_length, path_mode, out, tag):
    from ilswiss_amd.envs.vecenv import HipVectorEnv
    env = HipVectorEnv(name, n, seed=3, ctx=ctx)
    rb = ia.SimpleReplayBuffer(400 * n, env.obs_dim, env.act_dim, ctx=ctx)
    env.set_path_mode(path_mode)
    env.reset()
    env.rollout_stats(reset=True)
    for _ in range(steps):
        env.rollout_step(replay=rb, random_actions=True, max_path_length=max_path_length)
    ctx.sync()
    q, v = env.get_state()
    out[f"{name}{tag}_q"], out[f"{name}{tag}_v"] = q, v
    size, top = rb._cursors()
    for k, a in rb._gather(np.arange(size)).items():
        out[f"{name}{tag}_ring_{k}"] = a
    out[f"{name}{tag}_ring_cursors"] = np.array([size, top], np.int64)
    episodes, return_sum = env.rollout_stats(reset=False)
    out[f"{name}{tag}_stats_episodes"] = np.array([episodes], np.float64)
    out[f"{name}{tag}_stats_return_sum"] = np.array([return_sum], np.float64)
    if path_mode:
        out[f"{name}{tag}_traj_endpoints"] = np.array(sorted(rb._traj_endpoints.items()), np.int64).reshape(-1, 2)
    env.close()


def dump(path, steps=300):
    import ilswiss_amd as ia
    ctx = ia.Context(0, seed=11)
    out = {}
    for name, n, max_path_length in TASKS:
        _rollout(ia, ctx, name, n, steps, max_path_length, False, out, "")
        _rollout(ia, ctx, name, n, steps, max_path_length, True, out, "_paths")
    np.savez(path, **out)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = len(set(A.files) ^ set(B.files))
    if bad:
        print("arrays in one file only:", sorted(set(A.files) ^ set(B.files)))
    for k in A.files:
        if k not in B.files:
            continue
        same = A[k].shape == B[k].shape and A[k].tobytes() == B[k].tobytes()
        x, y = A[k].astype(np.float64), B[k].astype(np.float64)
        d = float(np.max(np.abs(x - y), initial=0.0)) if x.shape == y.shape else float("nan")
        word = "identical" if same else "DIFFERENT"
        if not same and k.endswith("_stats_return_sum"):   # a sum of atomic additions: equal up to their order
            base = k[:-len("_stats_return_sum")]
            bound = 2.0 * float(A[base + "_stats_episodes"][0]) * 2.0 ** -53 * float(np.abs(A[base + "_ring_rewards"].astype(np.float64)).sum()) * 1.000001
            if d <= bound:
                word, same = f"order-only (bound {bound:.3e})", True
        print(f"{k:48s} {word}  max |diff| {d:.3e}  shape {A[k].shape}  finite {bool(np.isfinite(x).all() and np.isfinite(y).all())}")
        bad += not same
    print(f"{len(A.files)} arrays, {bad} different")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 300)
    else:
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
