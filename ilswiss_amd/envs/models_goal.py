"""Goal-env constants for k_goal_step (csrc/goal_env.h): plain data, the one Python source of them.

`point-reach` is ilswiss_amd/her.py's PointReachEnv — a STAND-IN for the reference's goal envs (gym's Fetch robots, MuJoCo), not one of
them: a 2-D point under velocity control, v = step_scale * clip(a, -1, 1), p = clip(p + v, -1, 1), must come within `tol` of a goal;
reset draws p = U(+-p_range)^2 and g = U(+-g_range)^2.  The numbers are the host class's literals.
"""
import math

REWARD_KINDS = {"sparse": 0, "dense": 1}      # gym's GoalEnv rule on the goal distance d: -(d > tol) / -d


def point_reach(tol=0.1, reward_type="sparse"):
    if reward_type not in REWARD_KINDS:
        raise ValueError(f"point-reach: reward_type={reward_type!r}; the stepper knows {sorted(REWARD_KINDS)}")
    tol = float(tol)
    if not (math.isfinite(tol) and tol > 0.0):
        raise ValueError(f"point-reach: tol={tol!r} must be finite and positive")
    return dict(tol=tol, step_scale=0.1, p_range=0.5, g_range=0.8, reward_type=reward_type, reward_kind=REWARD_KINDS[reward_type],
                d_obs=4, d_goal=2, act_dim=2)


MODELS_GOAL = {"point-reach": point_reach}
