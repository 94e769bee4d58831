"""Restatements written for the MountainCarContinuous / MountainCar / Acrobot tests (not imported by the package): gym 0.22's
Continuous_MountainCarEnv (behind the reference's NormalizedBoxEnv), MountainCarEnv and AcrobotEnv ("book" dynamics, no torque noise), in
numpy float64, vectorised over envs, every operation in the order of the kernels in csrc/classic_env.h (which is Python's order of
evaluation of gym's expressions; FMA contraction is off there).  gym is not installed where this was written: the formulas are from
knowledge of gym 0.22 and the points of doubt are listed in DESIGN.md section 24.  This file is the specification the kernels are held to.

Every task is a class with `step(state, action) -> (next_state, reward, done)`, `observe(state) -> float32` and `reset_from_uniforms(u)`.
States are [N, 2] (x, v) for the cars and [N, 4] (theta1, theta2, dtheta1, dtheta2) for Acrobot, float64.  The libm calls go through a
`Libm` object, Python's math.cos / math.sin per element by default; `UlpLibm` moves every result by -1, 0 or +1 ulp at random, which is how
the CPU tests measure what a libm that differs from glibc's by an ulp can do to a step."""
import math

import numpy as np

_sin, _cos = np.frompyfunc(math.sin, 1, 1), np.frompyfunc(math.cos, 1, 1)


class Libm:
    calls = 0

    def cos(self, x):
        self.calls += 1
        return _cos(np.asarray(x, np.float64)).astype(np.float64)

    def sin(self, x):
        self.calls += 1
        return _sin(np.asarray(x, np.float64)).astype(np.float64)


class UlpLibm(Libm):
    """Every result moved by -1, 0 or +1 ulp (np.nextafter), drawn per element."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def _move(self, y):
        k = self.rng.integers(-1, 2, y.shape)
        return np.where(k == 0, y, np.nextafter(y, np.where(k > 0, np.inf, -np.inf)))

    def cos(self, x):
        return self._move(super().cos(x))

    def sin(self, x):
        return self._move(super().sin(x))


LIBM = Libm()
F32 = np.float32


def _clip_keep_nan(x, lo, hi):
    """x < lo ? lo : (x > hi ? hi : x): np.clip's values, a NaN stays a NaN."""
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _move(x, v):
    """What both cars share: the velocity clamp, the move, the position clamp and the inelastic left wall."""
    v = _clip_keep_nan(v, -0.07, 0.07)
    x = x + v
    x = _clip_keep_nan(x, -1.2, 0.6)
    v = np.where((x == -1.2) & (v < 0.0), 0.0, v)
    return x, v


class MountainCarCont:
    """Continuous_MountainCarEnv behind NormalizedBoxEnv over Box(-1, 1)."""
    name, kind, obs_dim, nq, discrete_n = "mountaincarcont", 4, 2, 1, 0
    GOAL = 0.45

    @staticmethod
    def force(action):
        """The policy's float32 action -> the float32 force: lb + (a + 1.0) * 0.5 * (ub - lb) on float32 arrays, np.clip to [lb, ub]."""
        a = np.asarray(action, F32).reshape(-1)
        lb, ub = F32(-1.0), F32(1.0)
        s = lb + (a + F32(1.0)) * F32(0.5) * (ub - lb)
        assert s.dtype == F32
        return _clip_keep_nan(s, lb, ub).astype(F32)

    @classmethod
    def step(cls, state, action, libm=LIBM, rounded=True):
        """rounded=False: the float64 (position, velocity) the step computes, before the env stores them as float32."""
        x, v = np.asarray(state[:, 0], np.float64), np.asarray(state[:, 1], np.float64)
        force = cls.force(action).astype(np.float64)
        v = v + (force * 0.0015 - 0.0025 * libm.cos(3.0 * x))
        x, v = _move(x, v)
        done = (x >= cls.GOAL) & (v >= 0.0)
        reward = np.where(done, 100.0, 0.0) - (force * force) * 0.1
        nxt = np.stack([x, v], 1)
        if rounded:
            nxt = nxt.astype(F32).astype(np.float64)     # self.state = np.array([position, velocity], dtype=np.float32)
        return nxt, reward, done

    @staticmethod
    def observe(state):
        return np.asarray(state, np.float64).astype(F32)

    @staticmethod
    def reset_from_uniforms(u):
        u = np.asarray(u, np.float64).reshape(-1, 1)
        return np.stack([(-0.6 + 0.2 * u[:, 0]).astype(F32).astype(np.float64), np.zeros(len(u))], 1)


class MountainCar:
    """MountainCarEnv: Discrete(3), the index held as a float and used as it is ((a - 1) * 0.001 for any value)."""
    name, kind, obs_dim, nq, discrete_n = "mountaincar", 5, 2, 1, 3
    GOAL = 0.5

    @classmethod
    def step(cls, state, action, libm=LIBM):
        x, v = np.asarray(state[:, 0], np.float64), np.asarray(state[:, 1], np.float64)
        a = np.asarray(action, F32).reshape(-1).astype(np.float64)
        v = v + ((a - 1.0) * 0.001 + libm.cos(3.0 * x) * (-0.0025))
        x, v = _move(x, v)
        done = (x >= cls.GOAL) & (v >= 0.0)
        return np.stack([x, v], 1), np.full(len(x), -1.0), done

    @staticmethod
    def observe(state):
        return np.asarray(state, np.float64).astype(F32)

    @staticmethod
    def reset_from_uniforms(u):
        u = np.asarray(u, np.float64).reshape(-1, 1)
        return np.stack([-0.6 + 0.2 * u[:, 0], np.zeros(len(u))], 1)


class Acrobot:
    """AcrobotEnv, book_or_nips = "book", torque_noise_max = 0."""
    name, kind, obs_dim, nq, discrete_n = "acrobot", 6, 6, 2, 3
    M1 = M2 = L1 = 1.0
    LC1 = LC2 = 0.5
    I1 = I2 = 1.0
    G, DT = 9.8, 0.2
    PI = math.pi
    MAX_VEL_1, MAX_VEL_2 = 4 * math.pi, 9 * math.pi
    WRAP_TRIPS = 16     # wrap()'s loops end after this many turns (gym's own would not end on an infinite angle)

    @classmethod
    def dsdt(cls, th1, th2, dth1, dth2, a, libm=LIBM):
        """_dsdt of the "book" branch, Python's order of evaluation, x ** 2 as x * x -> (ddtheta1, ddtheta2)."""
        m1, m2, l1, lc1, lc2, I1, I2, g, pi = cls.M1, cls.M2, cls.L1, cls.LC1, cls.LC2, cls.I1, cls.I2, cls.G, cls.PI
        c2, s2 = libm.cos(th2), libm.sin(th2)
        d1 = m1 * (lc1 * lc1) + m2 * (((l1 * l1) + (lc2 * lc2)) + ((2 * l1) * lc2) * c2) + I1 + I2
        d2 = m2 * ((lc2 * lc2) + (l1 * lc2) * c2) + I2
        phi2 = ((m2 * lc2) * g) * libm.cos((th1 + th2) - pi / 2.0)
        phi1 = ((((-m2 * l1) * lc2) * (dth2 * dth2)) * s2 - (((((2 * m2) * l1) * lc2) * dth2) * dth1) * s2
                + ((m1 * lc1 + m2 * l1) * g) * libm.cos(th1 - pi / 2)) + phi2
        dd2 = (((a + (d2 / d1) * phi1) - (((m2 * l1) * lc2) * (dth1 * dth1)) * s2) - phi2) / ((m2 * (lc2 * lc2) + I2) - (d2 * d2) / d1)
        dd1 = -(d2 * dd2 + phi1) / d1
        return dd1, dd2

    @classmethod
    def rk4(cls, state, torque, dt, libm=LIBM):
        """One classic RK4 step of (theta, dtheta) with the torque held: y0 + dt / 6 * (k1 + 2 k2 + 2 k3 + k4), the stages at dt / 2, dt / 2
        and dt.  No wrap, no bound."""
        y0 = [np.asarray(state[:, i], np.float64) for i in range(4)]
        ys, total = list(y0), None
        for stage in range(4):
            dd1, dd2 = cls.dsdt(ys[0], ys[1], ys[2], ys[3], torque, libm)
            k = [ys[2], ys[3], dd1, dd2]
            w = 2.0 if stage in (1, 2) else 1.0
            ch = dt if stage == 2 else dt / 2.0
            total = k if stage == 0 else [t + w * ki for t, ki in zip(total, k)]
            ys = [y + ch * ki for y, ki in zip(y0, k)]
        return [y + dt / 6.0 * t for y, t in zip(y0, total)]

    @classmethod
    def wrap(cls, x):
        x = np.array(x, np.float64)
        diff = cls.PI - (-cls.PI)
        for _ in range(cls.WRAP_TRIPS):
            x = np.where(x > cls.PI, x - diff, x)
        for _ in range(cls.WRAP_TRIPS):
            x = np.where(x < -cls.PI, x + diff, x)
        return x

    @classmethod
    def step(cls, state, action, libm=LIBM):
        torque = np.asarray(action, F32).reshape(-1).astype(np.float64) - 1.0
        th1, th2, w1, w2 = cls.rk4(np.asarray(state, np.float64), torque, cls.DT, libm)
        th1, th2 = cls.wrap(th1), cls.wrap(th2)
        w1 = _clip_keep_nan(w1, -cls.MAX_VEL_1, cls.MAX_VEL_1)
        w2 = _clip_keep_nan(w2, -cls.MAX_VEL_2, cls.MAX_VEL_2)
        done = cls.height(th1, th2, libm) > 1.0
        return np.stack([th1, th2, w1, w2], 1), np.where(done, 0.0, -1.0), done

    @classmethod
    def height(cls, th1, th2, libm=LIBM):
        """What _terminal compares with 1: -cos(theta1) - cos(theta2 + theta1)."""
        return -libm.cos(th1) - libm.cos(th2 + th1)

    @staticmethod
    def observe(state, libm=LIBM):
        s = np.asarray(state, np.float64)
        return np.stack([libm.cos(s[:, 0]), libm.sin(s[:, 0]), libm.cos(s[:, 1]), libm.sin(s[:, 1]), s[:, 2], s[:, 3]], 1).astype(F32)

    @staticmethod
    def reset_from_uniforms(u):
        """u [N, 4] -> (theta1, theta2, dtheta1, dtheta2) = -0.1 + 0.2 u, rounded to float32 (reset()'s .astype(np.float32))."""
        return (-0.1 + 0.2 * np.asarray(u, np.float64).reshape(-1, 4)).astype(F32).astype(np.float64)

    @classmethod
    def energy(cls, state):
        """Total mechanical energy of the two links (point of reference: the pivot), for the torque-free conservation test."""
        th1, th2, w1, w2 = (np.asarray(state[:, i], np.float64) for i in range(4))
        m1, m2, l1, lc1, lc2, I1, I2, g = cls.M1, cls.M2, cls.L1, cls.LC1, cls.LC2, cls.I1, cls.I2, cls.G
        d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * np.cos(th2)) + I1 + I2
        d2 = m2 * (lc2 ** 2 + l1 * lc2 * np.cos(th2)) + I2
        d22 = m2 * lc2 ** 2 + I2
        kin = 0.5 * d1 * w1 ** 2 + d2 * w1 * w2 + 0.5 * d22 * w2 ** 2
        pot = -(m1 * lc1 + m2 * l1) * g * np.cos(th1) - m2 * lc2 * g * np.cos(th1 + th2)
        return kin + pot


TASKS = {t.name: t for t in (MountainCarCont, MountainCar, Acrobot)}

# The largest absolute deviation of a next-state component when every libm result of a step is moved by -1, 0 or +1 ulp at random, over
# parity_inputs(task, 1000, seed) for seeds 0..19 (tests/test_gymcc_cpu.py measures it and holds these figures to it).  The GPU tests allow
# 8 times this between the device and the restatement: ROCm's and glibc's double cos / sin differ by at most an ulp where they differ,
# and the factor covers several of a step's calls (at most 16, Acrobot's) disagreeing at once.
ULP_DEV = {"mountaincarcont": 0.0, "mountaincar": 2.220446049250313e-16, "acrobot": 1.0658141036401503e-14}
ULP_FACTOR = 8.0


def parity_inputs(task, n, seed):
    """The states and actions of the single-step parity tests, CPU and GPU alike: -> (state [n, 2 or 4] float64, action [n, 1] float32).
    The cars: x over the whole track, v over +-0.07, every 8th row placed around the goal so that some steps end there; the continuous car's
    states are float32 values and its actions reach past the Box.  Acrobot: angles over the circle, velocities over half their bounds; the
    tip is above the line on about a quarter of the rows."""
    rng = np.random.default_rng([seed, task.kind])
    if task is Acrobot:
        s = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-2 * np.pi, 2 * np.pi, n),
                      rng.uniform(-4.5 * np.pi, 4.5 * np.pi, n)], 1)
        return s, rng.integers(0, 3, (n, 1)).astype(F32)
    x, v = rng.uniform(-1.2, 0.6, n), rng.uniform(-0.07, 0.07, n)
    near = np.arange(n) % 8 == 0
    x[near] = task.GOAL + rng.uniform(-0.06, 0.01, int(near.sum()))
    v[near] = rng.uniform(-0.01, 0.07, int(near.sum()))
    s = np.stack([x, v], 1)
    if task is MountainCarCont:
        return s.astype(F32).astype(np.float64), rng.uniform(-1.2, 1.2, (n, 1)).astype(F32)
    return s, rng.integers(0, 3, (n, 1)).astype(F32)


def done_margin(task, state, action, nxt=None):
    """How far the step's result is from the threshold its done flag compares with: x from the goal (the continuous car's before it is
    rounded to float32), or the tip's height from 1.  nxt: the step's result where the caller has it already."""
    if task is MountainCarCont:
        return np.abs(task.step(state, action, rounded=False)[0][:, 0] - task.GOAL)
    if nxt is None:
        nxt = task.step(state, action)[0]
    if task is Acrobot:
        return np.abs(Acrobot.height(nxt[:, 0], nxt[:, 1]) - 1.0)
    return np.abs(nxt[:, 0] - task.GOAL)


def state_of(task, q, v):
    """get_state()'s (qpos, qvel) -> the restatement's state array."""
    return np.concatenate([q, v], 1)


def split(task, s):
    return s[:, :task.nq].copy(), s[:, task.nq:].copy()
