"""Restatement written for the Pendulum tests (not imported by the package): gym 0.22's PendulumEnv (gym/envs/classic_control/pendulum.py)
behind the reference's NormalizedBoxEnv (rlkit/envs/wrappers.py:342-346), in numpy, the way numpy evaluates the reference's code:

  * the action map on float32 arrays: lb + (a + 1.0) * 0.5 * (ub - lb), np.clip to [lb, ub], then PendulumEnv's own clip to +-2;
  * the cost in float64 with the float32 torque promoted exactly: angle_normalize(th)**2 + 0.1 * thdot**2 + 0.001 * u**2;
  * the dynamics in float64, Python's math.sin per element (the HIP stepper in csrc/classic_env.h runs the same expression tree with FMA
    contraction off): thdot' = clip(thdot + (15 sin th + 3 u) * 0.05, +-8), th' = th + thdot' * 0.05 — gym 0.22's order, the velocity
    clipped before the position update;
  * the observation float32 (cos th', sin th', thdot');
  * reset: th = -pi + 2 pi u0, thdot = -1 + 2 u1 (np_random.uniform(low=-[pi, 1], high=[pi, 1]) with the two uniforms given)."""
import math

import numpy as np

MAX_SPEED, MAX_TORQUE, DT, G, M, L = 8.0, 2.0, 0.05, 10.0, 1.0, 1.0
_sin, _cos = np.frompyfunc(math.sin, 1, 1), np.frompyfunc(math.cos, 1, 1)
LB, UB = np.array([-MAX_TORQUE], np.float32), np.array([MAX_TORQUE], np.float32)   # PendulumEnv.action_space bounds (float32)


def torque(action):
    """action [N] or [N, 1] (float32, the policy's Box(-1, 1) action) -> the float32 torque PendulumEnv applies, shape [N]."""
    a = np.asarray(action, np.float32).reshape(-1, 1)
    scaled = LB + (a + 1.0) * 0.5 * (UB - LB)            # wrappers.py:344, float32 throughout
    scaled = np.clip(scaled, LB, UB)                      # wrappers.py:345
    u = np.clip(scaled, -MAX_TORQUE, MAX_TORQUE)[:, 0]    # pendulum.py step(): np.clip(u, -max_torque, max_torque)[0]
    assert u.dtype == np.float32
    return u


def angle_normalize(x):
    return ((np.asarray(x, np.float64) + np.pi) % (2 * np.pi)) - np.pi


def angle_normalize_fmod(x):
    """The same map as the device computes it: r = fmod(x + pi, 2 pi); r += 2 pi if r < 0; +0.0 if r == 0; r - pi."""
    r = np.fmod(np.asarray(x, np.float64) + np.pi, 2 * np.pi)
    r = np.where(r < 0, r + 2 * np.pi, r)
    r = np.where(r == 0, 0.0, r)
    return r - np.pi


def pendulum_step(state, action):
    """state [N, 2] float64 (theta, theta_dot), action [N] or [N, 1] float32 in the wrapper's space -> (next state [N, 2], reward [N] float64,
    observation [N, 3] float32).  Never done."""
    th, thdot = np.asarray(state[:, 0], np.float64), np.asarray(state[:, 1], np.float64)
    u = torque(action).astype(np.float64)
    an = angle_normalize(th)
    costs = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u)
    newthdot = thdot + (3 * G / (2 * L) * _sin(th).astype(np.float64) + 3.0 / (M * L ** 2) * u) * DT
    newthdot = np.clip(newthdot, -MAX_SPEED, MAX_SPEED)   # gym 0.22: before the position update
    newth = th + newthdot * DT
    nxt = np.stack([newth, newthdot], 1)
    return nxt, -costs, observe(nxt)


def observe(state):
    th, thdot = np.asarray(state[:, 0], np.float64), np.asarray(state[:, 1], np.float64)
    return np.stack([_cos(th).astype(np.float64), _sin(th).astype(np.float64), thdot], 1).astype(np.float32)


def reset_state(u0, u1):
    high = np.array([np.pi, 1.0])
    return np.stack([-high[0] + (high[0] - -high[0]) * np.asarray(u0, np.float64), -high[1] + (high[1] - -high[1]) * np.asarray(u1, np.float64)], 1)
