"""numpy restatements for the vectorised HER tests (no GPU, no library):

* the draw rule of ilsx_her_sample (include/ilsx.h) — trajectory, step and relabel step from three uniforms per row,
* the epsilon-uniform / Gaussian exploration step of k_explore (csrc/ilsx_env.hip),
* the goal env's step as the host class her.PointReachEnv takes it, and the generator of the GPU suite's step inputs.
"""
import numpy as np

RELABEL = {None: 0, "none": 0, "future": 1, "final": 2}


# ---------------------------------------------------------------------------------------------- sampler
def traj_table(endpoints, cap):
    """{start: end} in insertion order -> (starts, lengths), length = (end - start) mod cap; an entry of length 0 is left out."""
    rows = [(int(s), int((e - s) % cap)) for s, e in endpoints.items()]
    rows = [r for r in rows if r[1] >= 1]
    return np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64)


def pick(u, n):
    """floor(u n) in float64, clamped to [0, n - 1]."""
    x = np.floor(np.asarray(u, np.float64) * np.asarray(n, np.float64))
    return np.minimum(np.maximum(x, 0.0), np.asarray(n, np.float64) - 1.0).astype(np.int64)


def sample_indices(starts, lens, cap, u, relabel_type):
    """u: [B, 3] in [0, 1) -> (idx, idx_relabel), int64 [B]."""
    u = np.asarray(u, np.float64)
    kind = RELABEL[relabel_type] if not isinstance(relabel_type, (int, np.integer)) else int(relabel_type)
    t = pick(u[:, 0], len(starts))
    s, L = starts[t], lens[t]
    k = pick(u[:, 1], L)
    kf = k + pick(u[:, 2], L - k) if kind == 1 else (L - 1 if kind == 2 else k)
    return (s + k) % cap, (s + kf) % cap


def uniforms_from_reference_draws(rb, batch_size, global_seed):
    """The uniforms u = (draw + 0.5) / n that make the draw rule repeat the integer draws HindsightReplayBuffer.random_batch is about to
    make (relabel_replay_buffer.py:66-94): its RandomState's permutation of the trajectory keys, its trajectory and step draws, and the
    `future` draw from the global numpy stream seeded `global_seed`.  Leaves `rb` and the global stream as they were.  For trajectories
    that do not wrap the ring."""
    state = rb._np_rand_state.get_state()
    gstate = np.random.get_state()
    try:
        np.random.seed(global_seed)
        keys = list(rb._traj_endpoints.keys())
        starts = rb._np_rand_state.choice(keys, size=len(keys), replace=False)
        ends = [rb._traj_endpoints[k] for k in starts]
        u = np.zeros((batch_size, 3))
        for b, i in enumerate(rb._np_rand_state.randint(0, len(starts), batch_size)):
            L = (ends[i] - starts[i]) % rb._size
            k = rb._np_rand_state.randint(0, L, 1)[0]
            fut = np.random.randint(starts[i] + k, L + starts[i])
            u[b] = ((keys.index(starts[i]) + 0.5) / len(keys), (k + 0.5) / L, (fut - starts[i] - k + 0.5) / (L - k))
        return u
    finally:
        rb._np_rand_state.set_state(state)
        np.random.set_state(gstate)


# ---------------------------------------------------------------------------------------------- exploration
def explore_step(act, eps, u, epsilon, max_sigma, min_sigma, decay_period, low, high, t):
    """act float32 [n, a]; eps float64 [n, a] N(0,1) draws; u float64 [n, 1 + a] uniforms.  Per env: u[0] < epsilon gives the uniform action
    (float32)(low + (high - low) u[1 + j]), else (float32)clip(act + eps * sigma(t), low, high) in float64 (gaussian_strategy.py:25-33)."""
    act = np.asarray(act, np.float32)
    sigma = max_sigma - (max_sigma - min_sigma) * min(1.0, t * 1.0 / decay_period)
    gauss = np.minimum(np.maximum(act.astype(np.float64) + np.asarray(eps, np.float64) * sigma, low), high).astype(np.float32)
    if not epsilon > 0.0:
        return gauss
    u = np.asarray(u, np.float64)
    unif = (low + (high - low) * u[:, 1:]).astype(np.float32)
    return np.where(u[:, :1] < epsilon, unif, gauss)


# ---------------------------------------------------------------------------------------------- goal env
STEP_SEED, STEP_N, TOL = 20240611, 300, 0.1


def step_inputs(n=STEP_N, seed=STEP_SEED, tol=TOL):
    """(p, g, v, actions) of the GPU suite's one-step parity test: float64 positions and goals, float32 actions.  Rows cycle through five
    kinds: plain; |a| > 1 (the clip); p on or next to a wall, pushed outwards (the position clip); p a fraction of tol away from g (a
    success after the step or not, as it falls); g next to where the step lands."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.9, 0.9, (n, 2))
    g = rng.uniform(-0.8, 0.8, (n, 2))
    a = rng.uniform(-1.0, 1.0, (n, 2))
    kind = np.arange(n) % 5
    a[kind == 1] *= rng.uniform(1.0, 4.0, (int((kind == 1).sum()), 1))
    w = kind == 2
    side = rng.choice([-1.0, 1.0], (int(w.sum()), 2))
    p[w] = side * (1.0 - rng.choice([0.0, 0.03, 0.2], (int(w.sum()), 2)))
    a[w] = side * rng.uniform(0.5, 1.5, (int(w.sum()), 2))
    c = kind == 3
    g[c] = p[c] + tol * rng.uniform(-1.5, 1.5, (int(c.sum()), 2))
    d = kind == 4
    land = np.clip(p[d] + 0.1 * np.clip(a[d], -1, 1), -1, 1)
    g[d] = land + tol * rng.uniform(-0.9, 0.9, (int(d.sum()), 2))
    v = rng.uniform(-0.1, 0.1, (n, 2))
    return p, g, v, a.astype(np.float32)


def host_step(p, g, actions, tol=TOL, dense=False):
    """One her.PointReachEnv.step per row -> (p', v', float32 observation rows [n, 8], rewards float64, goal distance after the step).
    dense: the reward is -|p' - g| in float64 instead of the class's sparse rule."""
    from ilswiss_amd.her import PointReachEnv
    env = PointReachEnv(tol=tol)
    n = len(p)
    p2, v2, rows, rew, dist = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 8), np.float32), np.zeros(n), np.zeros(n)
    for i in range(n):
        env.p, env.g, env.v, env.k = p[i].copy(), g[i].copy(), np.zeros(2), 0
        o, r, done, _ = env.step(actions[i])
        assert done is False
        p2[i], v2[i] = env.p, env.v
        rows[i] = np.concatenate([o["observation"], o["desired_goal"], o["achieved_goal"]]).astype(np.float32)
        dist[i] = np.linalg.norm(env.p - env.g, axis=-1)
        rew[i] = -dist[i] if dense else r
    return p2, v2, rows, rew, dist
