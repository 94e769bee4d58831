"""CPU suite for off-policy rollouts with norm_obs: the restatement the GPU suite measures the ring against (tests/norm_rollout_restatement.py),
the two specs that turn the knob on, and what the run scripts refuse before they open a device.

The restatement is checked against a transcription of the reference's protocol: a vec env whose workers replay a recorded raw stream, with
BaseVectorEnv's reset(id) / step(action, id) / normalize_obs (vecenvs.py:158-257,299-327), driven in the order of BaseAlgorithm.start_training's
sampling loop (base_algorithm.py:183-277): act on `observations`, step, store (observations, next_obs), reset the ended envs and patch their
rows of next_obs, observations = next_obs."""
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from norm_rollout_restatement import make_rms, replay_norm_rollout  # noqa: E402

from oracle.envnorm import EPS, RunningMeanStd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, O, T = 3, 4, 6
# which envs' episodes end in which step: one of three (steps 1 and 5), two of three, all, none
RESETS = {0: [], 1: [1], 2: [0, 2], 3: [], 4: [0, 1, 2], 5: [2]}


def _stream():
    rng = np.random.default_rng(42)
    scale = np.array([1.0, 30.0, 0.01, 5.0])
    first = rng.normal(0, 1, (N, O)) * scale + 2.0
    steps = []
    for t in range(T):
        ids = RESETS[t]
        steps.append(dict(nobs=rng.normal(0, 1, (N, O)) * scale + 2.0 + t, reset_ids=ids, reset_obs=rng.normal(0, 1, (len(ids), O)) * scale))
    return first, steps


class _TapeVecEnv:
    """BaseVectorEnv with norm_obs on, its workers replaced by the recorded stream."""

    def __init__(self, first, steps, update_obs_rms=True):
        self.first, self.steps, self.t = first, steps, -1
        self.obs_rms, self.update_obs_rms, self.clip_max, self.eps = RunningMeanStd(), update_obs_rms, 10.0, EPS

    def normalize_obs(self, obs):
        return np.clip((obs - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.eps), -self.clip_max, self.clip_max)

    def reset(self, id=None):
        if id is None:
            obs = np.stack(list(self.first))
        else:
            st = self.steps[self.t]
            assert list(id) == list(st["reset_ids"])
            obs = np.stack([st["reset_obs"][k] for k in range(len(id))])
        if self.obs_rms and self.update_obs_rms:
            self.obs_rms.update(obs)
        return self.normalize_obs(obs)

    def step(self, action, id=None):
        self.t += 1
        obs_stack = np.stack(list(self.steps[self.t]["nobs"]))
        if self.obs_rms and self.update_obs_rms:
            self.obs_rms.update(obs_stack)
        return self.normalize_obs(obs_stack)


def _start_training(env, steps):
    records, stats = [], []
    observations = env.reset()
    for t in range(len(steps)):
        next_obs = env.step(None)
        records.append((observations.copy(), next_obs.copy()))           # _handle_vec_step(observations, ..., next_obs, ...)
        ended = list(steps[t]["reset_ids"])
        if ended:
            next_obs[ended] = env.reset(ended)                          # _start_new_rollout(env_ind_local)
        observations = next_obs
        stats.append((np.array(env.obs_rms.mean), np.array(env.obs_rms.var), env.obs_rms.count))
    return records, stats, observations


@pytest.mark.parametrize("update", (True, False))
def test_restatement_reproduces_the_reference_protocol(update):
    first, steps = _stream()
    assert any(len(s["reset_ids"]) == 1 for s in steps)                  # a step in which one env resets and two do not
    env = _TapeVecEnv(first, steps, update_obs_rms=True)
    obs0 = env.reset()
    if not update:                                                       # an eval env: the statistics it was given, never fed
        env.update_obs_rms = False
    env.reset = (lambda orig: (lambda id=None: obs0 if id is None else orig(id)))(env.reset)
    want, stats, last = _start_training(env, steps)
    rms = RunningMeanStd()
    rms.update(first)
    got = replay_norm_rollout(rms, obs0, steps, update=update)
    for t in range(T):
        np.testing.assert_array_equal(got[t]["obs"], want[t][0])
        np.testing.assert_array_equal(got[t]["next"], want[t][1])
        np.testing.assert_array_equal(got[t]["mean"], stats[t][0])
        np.testing.assert_array_equal(got[t]["var"], stats[t][1])
        assert got[t]["count"] == stats[t][2]
    np.testing.assert_array_equal(got[-1]["obs_n"], last)
    assert got[-1]["count"] == (N + sum(N + len(s["reset_ids"]) for s in steps) if update else N)
    # the chain: within an episode record t+1's observation IS record t's next observation; after a reset it is not
    for t in range(T - 1):
        for e in range(N):
            same = np.array_equal(got[t + 1]["obs"][e], got[t]["next"][e])
            assert same == (e not in RESETS[t]), (t, e)
    # old rows are not re-normalised: the statistics moved between two steps, the earlier record did not follow them
    if update:
        assert not np.allclose(got[0]["mean"], got[-1]["mean"])
    assert np.abs(np.concatenate([g["next"] for g in got])).max() <= 10.0


def test_restatement_clips_and_starts_from_given_statistics():
    first, steps = _stream()
    rms = make_rms(np.zeros(O), np.full(O, 1e-4), 1)
    got = replay_norm_rollout(rms, np.zeros((N, O)), steps[:1], update=False)
    assert (np.abs(got[0]["next"]) == 10.0).any() and got[0]["count"] == 1 and np.all(got[0]["var"] == 1e-4)
    got = replay_norm_rollout(rms, np.zeros((N, O)), steps[:1])
    assert got[0]["count"] == 1 + N and np.abs(got[0]["next"]).max() < 10.0   # one real batch swamps a count of 1


@pytest.mark.parametrize("name,base", (("sac_halfcheetah_norm_hip.yaml", "sac_halfcheetah_hip.yaml"), ("sac_pendulum_norm_hip.yaml", "sac_pendulum_hip.yaml")))
def test_the_norm_specs(name, base):
    from ilswiss_amd.launcher import variants
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "sac", name)))
    plain = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "sac", base)))
    v = next(variants(spec))
    assert v["env_specs"]["vec_env_kwargs"] == {"norm_obs": True}
    assert os.path.isfile(os.path.join(ROOT, spec["meta_data"]["script_path"])) and spec["meta_data"]["script_path"] == plain["meta_data"]["script_path"]
    env_specs = dict(spec["constants"]["env_specs"])
    env_specs.pop("vec_env_kwargs")
    assert env_specs == plain["constants"]["env_specs"]                  # the shipped spec plus the knob, nothing else
    for k in ("net_size", "num_hidden_layers", "rl_alg_params", "sac_params"):
        assert spec["constants"][k] == plain["constants"][k], k
    assert spec["variables"] == plain["variables"] and spec["meta_data"]["exp_name"] != plain["meta_data"]["exp_name"]


def _variant(path):
    sys.path.insert(0, os.path.join(ROOT, "run_scripts"))
    from _common import flatten_spec
    return flatten_spec(yaml.safe_load(open(os.path.join(ROOT, "exp_specs", path))))


def _no_device(script, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the refusal must come before the device is opened")
    monkeypatch.setattr(script, "start", boom)
    monkeypatch.setattr(script, "make_envs", boom)


def test_mbpo_refuses_norm_obs_before_the_device(monkeypatch):
    v = _variant("mbpo/mbpo_hopper_hip.yaml")
    import mbpo_exp_script as script
    _no_device(script, monkeypatch)
    v["env_specs"]["vec_env_kwargs"] = {"norm_obs": True}
    with pytest.raises(SystemExit, match="MBPO.*norm_obs.*raw quantities"):
        script.experiment(v)


@pytest.mark.parametrize("name,spec", (("sac_alpha", "sac/sac_pendulum_norm_hip.yaml"), ("td3", "td3/td3_hopper_hip.yaml"), ("ddpg", "ddpg/ddpg_hopper_hip.yaml")))
def test_split_runs_refuse_norm_obs_before_the_device(monkeypatch, name, spec):
    import importlib
    v = _variant(spec)
    script = importlib.import_module(f"{name}_exp_script")
    _no_device(script, monkeypatch)
    v["env_specs"]["vec_env_kwargs"] = {"norm_obs": True}
    v["rl_alg_params"]["split_ranks"] = 2
    with pytest.raises(SystemExit, match="norm_obs.*split_ranks.*own shard"):
        script.experiment(v)
    v["env_specs"]["vec_env_kwargs"] = {"norm_obs": False}               # the knob off: nothing to refuse, the script goes on to the device
    with pytest.raises(AssertionError, match="before the device"):
        script.experiment(v)


def test_scripts_hand_the_knob_to_make_envs(monkeypatch):
    """Every off-policy run script passes env_specs.vec_env_kwargs on, and passes nothing when the spec has none."""
    import importlib
    seen = []

    class Stop(Exception):
        pass

    def make_envs(variant, ctx, **kw):
        seen.append(kw)
        raise Stop
    for name, spec in (("sac_alpha", "sac/sac_pendulum_hip.yaml"), ("sac", "sac/sac_v_hopper_hip.yaml"), ("td3", "td3/td3_hopper_hip.yaml"),
                       ("ddpg", "ddpg/ddpg_hopper_hip.yaml"), ("dqn", "dqn/dqn_cartpole_hip.yaml"), ("discrete_sac", "sac/sac_cartpole_d_hip.yaml")):
        script = importlib.import_module(f"{name}_exp_script")
        monkeypatch.setattr(script, "start", lambda variant, gpu: None)
        monkeypatch.setattr(script, "make_envs", make_envs)
        v = _variant(spec)
        for kw in ({}, {"norm_obs": True}, {"norm_obs": True, "update_obs_rms": False}):
            if kw:
                v["env_specs"]["vec_env_kwargs"] = dict(kw)
            with pytest.raises(Stop):
                script.experiment(v)
            assert seen[-1] == kw, (name, seen[-1])
