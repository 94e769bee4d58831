"""What a fused rollout step of a normalising env leaves in its replay ring, restated in numpy on recorded RAW rows (test infrastructure).

One sampling iteration of the reference (base_algorithm.py:183-277 over vecenvs.py:158-257,299-327) with norm_obs on:
  step():      obs_rms.update(next observations of all envs), then next_n = normalize_obs(next observations)   [updated statistics]
  the record:  observations (what the policy read) | action | reward | terminal | next_n | absorbing
  reset(ids):  obs_rms.update(reset observations of the ended envs), obs_n[ids] = normalize_obs(reset observations)   [newest statistics]
  every other env keeps next_n as its next policy input: the same numbers, not normalised again.
Built on oracle.envnorm.RunningMeanStd / normalize_obs (float64, pinned to the reference by tests/golden g11_g12)."""
import numpy as np

from oracle.envnorm import RunningMeanStd, normalize_obs


def make_rms(mean, var, count):
    rms = RunningMeanStd()
    rms.mean, rms.var, rms.count = np.array(mean, np.float64), np.array(var, np.float64), count
    return rms


def replay_norm_rollout(rms, obs_n, steps, update=True):
    """rms: the statistics before the first step (updated in place).  obs_n [n, o]: the policy input before the first step.
    steps: one dict per step with `nobs` [n, o] (raw next observations), `reset_ids` (envs whose episode ended in the step) and `reset_obs`
    [len(reset_ids), o] (their raw reset observations).  update=False: an env built on shared statistics that it does not feed.
    Returns one dict per step: `obs` and `next` (the record's two observation segments, float64), `obs_n` (the policy input after the step)
    and `mean` / `var` / `count` after the step."""
    obs_n = np.array(obs_n, np.float64)
    out = []
    for st in steps:
        nobs = np.asarray(st["nobs"], np.float64)
        ids = np.asarray(st["reset_ids"], np.int64).reshape(-1)
        if update:
            rms.update(nobs)
        next_n = normalize_obs(nobs, rms)
        rec_obs, rec_next = obs_n.copy(), next_n.copy()
        obs_n = next_n.copy()
        if ids.size:
            r = np.asarray(st["reset_obs"], np.float64).reshape(ids.size, -1)
            if update:
                rms.update(r)
            obs_n[ids] = normalize_obs(r, rms)
        out.append(dict(obs=rec_obs, next=rec_next, obs_n=obs_n.copy(), mean=np.array(rms.mean, np.float64) + np.zeros(nobs.shape[1]),
                        var=np.array(rms.var, np.float64) + np.zeros(nobs.shape[1]), count=rms.count))
    return out
