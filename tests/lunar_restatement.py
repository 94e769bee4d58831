"""numpy float64 statement of the LunarLanderContinuous stepper (the thing k_lunar_step of csrc/lunar_env.h must reproduce), batched over
envs.  Written from the definition in DESIGN.md section 23 with generic tools (rotation matrices, cross products, a terrain lookup by
array indexing, projected Gauss-Seidel as a loop over a row list), not from the kernel's closed forms.  Test infrastructure; the
constants come from ilswiss_amd/envs/models_lunar.py, the Philox draws from oracle/philox.py (`draws`).

State: q = (x, y, theta of the hull origin | smooth_y[0..10]), v = (vx, vy of the hull origin, omega | sleep_time).
    engines   impulses on the composite body about its centre of mass, once per step, before the substeps
    substep   h = 1 / FPS / frame_skip: a = (0, g, 0) + M^-1 J^T f, v += h a, q += h v  (on the centre of mass, M = diag(m, m, I))
    contact   foot point at or below the line of the terrain segment under its x (clamped to [0, W]): rows (normal, tangent),
              (A + R) f = aref - J a0,  A = J M^-1 J^T,  R_i = (1 - d_i) / d_i A_ii,  aref_n = -b J v - k d r,  aref_t = -b J v,
              b = 2 / (dmax tc),  k = 1 / (dmax^2 tc^2 dr^2),  d = impedance(|r|);  f_n >= 0, |f_t| <= mu f_n; rows (n0, t0, n1, t1)
Every step also reports `switch_margin`: the smallest distance to a switch met in any substep (foot gap, hull-vertex gap after the
step, 1 - |s0|, and the distance of the linear and angular speed from their sleep tolerances)."""
import numpy as np


def rot(phi):
    c, s = np.cos(phi), np.sin(phi)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


def cross2(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def impedance(r_abs, solimp):
    d0, dmax, width = solimp
    x = np.minimum(r_abs / width, 1.0) if width > 0 else np.ones_like(r_abs)
    y = np.where(x < 0.5, 2.0 * x * x, 1.0 - 2.0 * (1.0 - x) ** 2)
    return d0 + y * (dmax - d0)


def draws(seed, stream, step, envs, counters):
    """[len(envs), len(counters)] uniforms in (0, 1) of the envs' Philox streams at `step`: word k & 3 of the block with counter
    (env, k >> 2), (word + 0.5) / 2^32."""
    from oracle import philox
    envs = np.asarray(envs, np.uint32)
    out = np.empty((len(envs), len(counters)))
    for j, k in enumerate(counters):
        c = philox.philox4x32_10(*philox._ctr_key(int(seed), int(step), int(stream), envs, k >> 2))
        out[:, j] = (c[:, k & 3].astype(np.float64) + 0.5) / 4294967296.0
    return out


class Lunar:
    def __init__(self, model):
        m = self.m = model
        self.W, self.H, self.fps, self.scale = m["w"], m["h"], m["fps"], m["scale"]
        self.com = np.array(m["com"], np.float64)
        self.foot = np.array(m["foot"], np.float64)
        self.hull = np.array(m["hull_poly"], np.float64)
        self.chunk_dx = self.W / (m["chunks"] - 1)
        tc, dr = m["contact_solref"]
        dmax = m["contact_solimp"][1]
        self.b, self.k = 2.0 / (dmax * tc), 1.0 / (dmax * dmax * tc * tc * dr * dr)

    # ---------------------------------------------------------------- terrain
    def terrain_from_heights(self, height):
        """height [B, 12] -> smooth_y [B, 11]; the five entries 3..7 become the helipad's height first."""
        h = np.array(height, np.float64)
        h[:, 3:8] = self.m["helipad_y"]
        return np.stack([0.33 * (h[:, i - 1] + h[:, i] + h[:, i + 1]) for i in range(11)], 1)

    def gap(self, sy, p):
        """Signed distance of the points p [B, 2] from the line of the terrain segment under their (clamped) x, and the unit tangents."""
        B = np.arange(len(p))
        xc = np.clip(p[:, 0], 0.0, self.W)
        j = np.minimum((xc / self.chunk_dx).astype(int), 9)
        p0 = np.stack([j * self.chunk_dx, sy[B, j]], 1)
        seg = np.stack([np.full(len(p), self.chunk_dx), sy[B, j + 1] - sy[B, j]], 1)
        t = seg / np.sqrt(np.sum(seg * seg, 1))[:, None]
        return cross2(t, p - p0), t

    def points(self, q, local):
        """World positions [B, K, 2] of hull-frame points local [K, 2]."""
        return q[:, None, :2] + np.einsum("bij,kj->bki", rot(q[:, 2]), local)

    # ---------------------------------------------------------------- task rules
    def observe64(self, q, v):
        W, H, m = self.W, self.H, self.m
        feet = self.points(q, self.foot)
        c = [(self.gap(q[:, 3:], feet[:, i])[0] <= 0.0).astype(np.float64) for i in (0, 1)]
        return np.stack([(q[:, 0] - W / 2.0) / (W / 2.0), (q[:, 1] - (m["helipad_y"] + m["leg_down"] / self.scale)) / (H / 2.0),
                         v[:, 0] * (W / 2.0) / self.fps, v[:, 1] * (H / 2.0) / self.fps, q[:, 2], 20.0 * v[:, 2] / self.fps, c[0], c[1]], 1)

    def observe(self, q, v):
        return self.observe64(q, v).astype(np.float32)

    @staticmethod
    def shaping(s):
        return (-100.0 * np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) - 100.0 * np.sqrt(s[:, 2] * s[:, 2] + s[:, 3] * s[:, 3])
                - 100.0 * np.abs(s[:, 4]) + 10.0 * s[:, 6] + 10.0 * s[:, 7])

    def engines(self, q, a, disp):
        """Impulse [B, 2], its moment about the centre of mass [B], m_power, s_power for float32 actions a [B, 2] and the dispersion
        uniforms disp [B, 2] in (0, 1) (U(-1, 1) = 2 u - 1)."""
        m, S = self.m, self.scale
        a = np.clip(np.asarray(a, np.float32), np.float32(-1), np.float32(1)).astype(np.float64)
        th = q[:, 2]
        tip = np.stack([np.sin(th), np.cos(th)], 1)
        side = np.stack([-tip[:, 1], tip[:, 0]], 1)
        d = (2.0 * np.asarray(disp, np.float64) - 1.0) / S
        rcom = np.einsum("bij,j->bi", rot(th), self.com)
        imp, mom = np.zeros((len(q), 2)), np.zeros(len(q))
        fire = a[:, 0] > 0.0
        m_power = np.where(fire, (np.clip(a[:, 0], 0.0, 1.0) + 1.0) * 0.5, 0.0)
        o = np.stack([tip[:, 0] * (4.0 / S + 2.0 * d[:, 0]) + side[:, 0] * d[:, 1], -tip[:, 1] * (4.0 / S + 2.0 * d[:, 0]) - side[:, 1] * d[:, 1]], 1)
        i1 = -o * m["main_engine_power"] * m_power[:, None]
        imp += np.where(fire[:, None], i1, 0.0)
        mom += np.where(fire, cross2(o - rcom, i1), 0.0)
        fire = np.abs(a[:, 1]) > 0.5
        dirn = np.sign(a[:, 1])
        s_power = np.where(fire, np.clip(np.abs(a[:, 1]), 0.5, 1.0), 0.0)
        lat = 3.0 * d[:, 1] + dirn * m["side_engine_away"] / S
        o = np.stack([tip[:, 0] * d[:, 0] + side[:, 0] * lat, -tip[:, 1] * d[:, 0] - side[:, 1] * lat], 1)
        i2 = -o * m["side_engine_power"] * s_power[:, None]
        at = np.stack([o[:, 0] - tip[:, 0] * 17.0 / S, o[:, 1] + tip[:, 1] * m["side_engine_height"] / S], 1)
        imp += np.where(fire[:, None], i2, 0.0)
        mom += np.where(fire, cross2(at - rcom, i2), 0.0)
        return imp, mom, m_power, s_power

    # ---------------------------------------------------------------- dynamics
    def contact_forces(self, sy, c, th, u, w):
        """Constraint acceleration (ax, ay, aw) [B, 3] of the foot contacts at centre of mass c, angle th, velocity (u, w); the feet's gaps."""
        m = self.m
        B = len(c)
        im, ii, mu = 1.0 / m["mass"], 1.0 / m["inertia"], m["friction"]
        lever = np.einsum("bij,kj->bki", rot(th), self.foot - self.com)      # [B, 2, 2]
        a0 = np.array([0.0, m["gravity"], 0.0])
        vel = np.concatenate([u, w[:, None]], 1)
        J, rc, den, on, gaps = np.zeros((B, 4, 3)), np.zeros((B, 4)), np.ones((B, 4)), np.zeros((B, 4), bool), np.zeros((B, 2))
        Minv = np.array([im, im, ii])
        for i in (0, 1):
            r, t = self.gap(sy, c + lever[:, i])
            n = np.stack([-t[:, 1], t[:, 0]], 1)
            gaps[:, i] = r
            d = impedance(np.abs(r), m["contact_solimp"])
            for row, direction in ((2 * i, n), (2 * i + 1, t)):
                J[:, row] = np.concatenate([direction, cross2(lever[:, i], direction)[:, None]], 1)
                att = np.sum(J[:, row] * J[:, row] * Minv, 1)
                aref = -self.b * np.sum(J[:, row] * vel, 1) - (self.k * d * r if row == 2 * i else 0.0)
                den[:, row] = att + (1.0 - d) / d * att
                rc[:, row] = aref - J[:, row] @ a0
                on[:, row] = r <= 0.0
        A = np.einsum("bti,i,bui->btu", J, Minv, J)
        f = np.zeros((B, 4))
        for _ in range(m["pgs_iters"]):
            for t in range(4):
                res = rc[:, t] - (np.sum(A[:, t] * f, 1) - A[:, t, t] * f[:, t])
                fi = res / den[:, t]
                if t % 2 == 0:
                    fi = np.maximum(fi, 0.0)
                else:
                    lim = mu * f[:, t - 1]
                    fi = np.minimum(np.maximum(fi, -lim), lim)
                f[:, t] = np.where(on[:, t], fi, 0.0)
        return np.einsum("bti,bt->bi", J, f) * Minv, gaps

    def move(self, q, v, imp, mom):
        """One env step after the engines.  Returns q', v' (sleep clock included), game_over and the step's switch margin apart from
        the |s0| term."""
        m = self.m
        q, v = np.array(q, np.float64), np.array(v, np.float64)
        sy = q[:, 3:]
        th, w = q[:, 2].copy(), v[:, 2] + mom / m["inertia"]
        rcom = np.einsum("bij,j->bi", rot(th), self.com)
        c = q[:, :2] + rcom
        u = v[:, :2] + v[:, 2:3] * np.stack([-rcom[:, 1], rcom[:, 0]], 1) + imp / m["mass"]
        h = 1.0 / self.fps / m["frame_skip"]
        margin = np.full(len(q), np.inf)
        g = np.array([0.0, m["gravity"]])
        for _ in range(m["frame_skip"]):
            acc, gaps = self.contact_forces(sy, c, th, u, w)
            margin = np.minimum(margin, np.abs(gaps).min(1))
            u = u + h * (g + acc[:, :2])
            w = w + h * acc[:, 2]
            c = c + h * u
            th = th + h * w
        rcom = np.einsum("bij,j->bi", rot(th), self.com)
        q[:, :2], q[:, 2] = c - rcom, th
        v[:, :2] = u - w[:, None] * np.stack([-rcom[:, 1], rcom[:, 0]], 1)
        v[:, 2] = w
        hull = self.points(q, self.hull)
        hg = np.stack([self.gap(sy, hull[:, k])[0] for k in range(len(self.hull))], 1)
        game_over = (hg <= 0.0).any(1)
        margin = np.minimum(margin, np.abs(hg).min(1))
        speed2, ang2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1], v[:, 2] * v[:, 2]
        still = (speed2 <= m["sleep_lin_tol"] * m["sleep_lin_tol"]) & (ang2 <= m["sleep_ang_tol"] * m["sleep_ang_tol"])
        v[:, 3] = np.where(still, v[:, 3] + 1.0 / self.fps, 0.0)
        margin = np.minimum(margin, np.minimum(np.abs(np.sqrt(speed2) - m["sleep_lin_tol"]), np.abs(np.abs(v[:, 2]) - m["sleep_ang_tol"])))
        return q, v, game_over, margin

    def step(self, q, v, a, disp=None):
        """-> q', v', obs (float32), reward (float64, before the float32 store), done, switch_margin, game_over"""
        q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
        disp = np.full((len(q), 2), 0.5) if disp is None else disp          # 0.5 is no dispersion
        before = self.shaping(self.observe64(q, v))
        imp, mom, m_power, s_power = self.engines(q, a, disp)
        q2, v2, game_over, margin = self.move(q, v, imp, mom)
        s = self.observe64(q2, v2)
        rew = (self.shaping(s) - before) - 0.30 * m_power - 0.03 * s_power
        lost = game_over | (np.abs(s[:, 0]) >= 1.0)
        asleep = v2[:, 3] >= self.m["sleep_time"]
        rew = np.where(asleep, 100.0, np.where(lost, -100.0, rew))
        margin = np.minimum(margin, np.abs(1.0 - np.abs(s[:, 0])))
        return q2, v2, s.astype(np.float32), rew, lost | asleep, margin, game_over

    def reset_from_draws(self, u):
        """u [B, 14]: counters 0..11 the terrain heights, 12 and 13 the initial force -> (q, v) that reset returns."""
        u = np.asarray(u, np.float64)
        B = len(u)
        sy = self.terrain_from_heights((self.H / 2.0) * u[:, :12])
        force = -self.m["initial_random"] + 2.0 * self.m["initial_random"] * u[:, 12:14]
        q = np.concatenate([np.tile([self.W / 2.0, self.H, 0.0], (B, 1)), sy], 1)
        q2, v2, _, _ = self.move(q, np.zeros((B, 4)), force / self.fps, np.zeros(B))
        return q2, v2
