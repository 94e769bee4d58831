"""CPU suite of the vectorised HER path (no GPU, no library call): (1) the numpy restatement of ilsx_her_sample's draw rule
(tests/her_sample_restatement.py) returns the reference buffer's own indices when fed uniforms built from its integer draws, and stays
inside a trajectory that wraps the ring; (2) the restatement of the epsilon-uniform / Gaussian exploration step; (3) the GPU suite's
step inputs keep clear of the reward rule's threshold; (4) names, specs, the ctypes table and the refusals that come before the library
is entered."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import her_sample_restatement as R  # noqa: E402

G22 = np.load(os.path.join(HERE, "golden", "g22_her_buffer.npz"))


def _filled_reference_buffer(cap, rtype, ratio=0.8):
    """HindsightReplayBuffer (the reference's buffer, pinned by g22) holding the six g22 paths."""
    from ilswiss_amd.her import Box, DictSpace, HindsightReplayBuffer
    o, gd, a, _ = (int(v) for v in G22["dims"])

    class Env:
        observation_space = DictSpace(observation=Box(-np.ones(o), np.ones(o)), desired_goal=Box(-np.ones(gd), np.ones(gd)),
                                      achieved_goal=Box(-np.ones(gd), np.ones(gd)))
        action_space = Box(-np.ones(a), np.ones(a))

        @staticmethod
        def compute_reward(ag, dg, info=None):
            return -(np.linalg.norm(ag - dg, axis=-1) > 0.5).astype(np.float32)
    rb = HindsightReplayBuffer(cap, Env, random_seed=77, relabel_type=rtype, her_ratio=ratio)
    for p in range(6):
        obs, dg, ag = G22[f"p{p}_obs"], G22[f"p{p}_dg"], G22[f"p{p}_ag"]
        d = lambda i: dict(observation=obs[i], desired_goal=dg[i], achieved_goal=ag[i])   # noqa: E731
        for i in range(len(G22[f"p{p}_act"])):
            rb.add_sample(d(i), G22[f"p{p}_act"][i], G22[f"p{p}_rew"][i], bool(G22[f"p{p}_term"][i]), d(i + 1))
        rb.terminate_episode()
    return rb


@pytest.mark.parametrize("rtype", ("future", "final"))
def test_draw_rule_returns_the_reference_buffers_indices(rtype):
    """The g22 paths in a ring large enough that no trajectory wraps; B = 64 rows, all relabelled in the reference's index lists."""
    cap, B = 128, 64
    rb = _filled_reference_buffer(cap, rtype)
    assert len(rb._traj_endpoints) == 6 and all(e > s for s, e in rb._traj_endpoints.items())      # none wraps
    u = R.uniforms_from_reference_draws(rb, B, global_seed=901)
    assert u.shape == (B, 3) and (u >= 0).all() and (u < 1).all()
    seen = []
    gather = rb._gather
    rb._gather = lambda indices, with_all=True: (seen.append(np.array(indices, np.int64)), gather(indices, with_all))[1]
    np.random.seed(901)
    rb.random_batch(B)
    indices, indices_relabel = seen
    starts, lens = R.traj_table(rb._traj_endpoints, cap)
    idx, rel = R.sample_indices(starts, lens, cap, u, rtype)
    np.testing.assert_array_equal(idx, indices)
    np.testing.assert_array_equal(rel, indices_relabel)
    assert len(set(idx.tolist())) > 10 and (rel != idx).any()


def test_draw_rule_stays_inside_a_wrapped_trajectory():
    cap = 40
    starts, lens = R.traj_table({6: 13, 13: 14, 14: 35, 35: 6}, cap)      # lengths 7, 1, 21, 11 (the last wraps: 35..39, 0..5)
    assert lens.tolist() == [7, 1, 21, 11]
    rng = np.random.default_rng(5)
    u = rng.random((4000, 3))
    u[:8] = [[0.8, 0.0, 0.0], [0.8, 0.999999, 0.999999], [0.8, 0.5, 0.0], [0.8, 0.5, 0.999999], [0.3, 0.7, 0.7], [0.0, 0.0, 0.999999],
             [0.999999, 0.999999, 0.0], [0.8, 0.45, 0.5]]
    for rtype in ("future", "final", None):
        idx, rel = R.sample_indices(starts, lens, cap, u, rtype)
        t = R.pick(u[:, 0], 4)
        off, off_rel = (idx - starts[t]) % cap, (rel - starts[t]) % cap
        assert (idx >= 0).all() and (idx < cap).all() and (rel >= 0).all() and (rel < cap).all()
        assert (off < lens[t]).all() and (off_rel < lens[t]).all()          # both steps lie in the sampled trajectory ...
        assert (off_rel >= off).all()                                        # ... the relabel step at or after the sampled one
        w = t == 3
        assert w.sum() > 500 and (idx[w] < 6).any() and (idx[w] >= 35).any()   # the wrapped one is hit on both sides of the seam
        if rtype == "final":
            assert (off_rel == lens[t] - 1).all()
        if rtype is None:
            assert (rel == idx).all()
        if rtype == "future":                                                 # uniform over the steps from the sampled one on
            last = off_rel[w] == 10
            assert 0.1 < last.mean() < 0.5
    # the clamp: u = 1 - 2^-53 and products that round up to n still give n - 1
    assert R.pick(np.array([np.nextafter(1.0, 0.0)]), np.array([3]))[0] == 2 and R.pick(np.array([0.0]), np.array([3]))[0] == 0


def test_exploration_restatement():
    rng = np.random.default_rng(11)
    n, a = 300, 2
    act = np.tanh(rng.normal(0, 1, (n, a))).astype(np.float32)
    eps, u = rng.normal(0, 1, (n, a)), rng.random((n, 1 + a))
    kw = dict(max_sigma=0.4, min_sigma=0.1, decay_period=1000.0, low=-1.0, high=1.0)
    g0 = R.explore_step(act, eps, u, 0.0, t=250, **kw)
    sigma = 0.4 - 0.3 * 0.25
    np.testing.assert_array_equal(g0, np.clip(act.astype(np.float64) + eps * sigma, -1.0, 1.0).astype(np.float32))
    assert (np.abs(g0) == 1.0).any()                                           # the clip is reached
    g1 = R.explore_step(act, eps, u, 1.0, t=250, **kw)
    np.testing.assert_array_equal(g1, (-1.0 + 2.0 * u[:, 1:]).astype(np.float32))
    assert (g1 >= -1).all() and (g1 <= 1).all() and len({tuple(r) for r in g1.tolist()}) == n
    gm = R.explore_step(act, eps, u, 0.3, t=250, **kw)
    pick = u[:, 0] < 0.3
    assert 50 < pick.sum() < 130
    np.testing.assert_array_equal(gm[pick], g1[pick])
    np.testing.assert_array_equal(gm[~pick], g0[~pick])
    # sigma stops annealing at decay_period
    np.testing.assert_array_equal(R.explore_step(act, eps, u, 0.0, t=5000, **kw), R.explore_step(act, eps, u, 0.0, t=1000, **kw))


def test_step_inputs_keep_clear_of_the_threshold():
    """The GPU suite compares sparse rewards exactly on every row not within 1e-12 of tol in goal distance: for the seed it uses that is
    every row (zero rows excluded), and the inputs exercise what they claim to."""
    p, g, v, a = R.step_inputs()
    assert p.shape == (R.STEP_N, 2) and a.dtype == np.float32
    p2, v2, rows, rew, dist = R.host_step(p, g, a)
    near = np.abs(dist - R.TOL) <= 1e-12
    assert near.mean() <= 0.001
    assert near.sum() == 0
    assert (rew == 0).sum() >= 20 and (rew == -1).sum() >= 20                 # some succeed, some do not
    assert (np.abs(a) > 1).any() and (np.abs(p2) == 1.0).sum() >= 20           # the action clip and the wall clip are reached
    assert (np.linalg.norm(p - g, axis=1) < R.TOL).any()                       # some start within tol of the goal
    np.testing.assert_array_equal(v2, (np.float32(0.1) * np.clip(a, -1, 1)).astype(np.float64))   # float32 product, widened
    assert rows.dtype == np.float32 and np.array_equal(rows[:, 6:], rows[:, :2]) and np.array_equal(rows[:, 4:6], g.astype(np.float32))


def test_names_specs_and_ctypes_table():
    from ilswiss_amd import _lib, her
    from ilswiss_amd.envs import GOAL, MODELS_GOAL
    from ilswiss_amd.launcher import variants
    assert GOAL == {"point-reach": 18}
    m = MODELS_GOAL["point-reach"]()
    assert (m["tol"], m["step_scale"], m["p_range"], m["g_range"], m["reward_kind"]) == (0.1, 0.1, 0.5, 0.8, 0)
    assert MODELS_GOAL["point-reach"](tol=0.05, reward_type="dense")["reward_kind"] == 1
    h = open(os.path.join(ROOT, "include", "ilsx.h")).read()
    for sym in ("ilsx_her_sample", "ilsx_vecenv_create_goal", "ilsx_vecenv_goal_dims", "ilsx_vecenv_set_exploration_epsilon",
                "ilsx_vecenv_explore_u"):
        assert sym in _lib.PROTOTYPES, sym
        assert re.search(r"\bint %s\(" % sym, h), sym
    assert re.search(r"ILSX_GOAL_TASK = 18\b", h) and "ILSX_ABI_VERSION 1" in h.replace("  ", " ")
    assert len(_lib.PROTOTYPES["ilsx_her_sample"][1]) == 16 and ctypes.sizeof(_lib.ExploreCfg) == 64   # the exploration struct is untouched
    for name, script, key in (("her_reach_td3_vec_hip", "her_td3_exp_script.py", "td3_params"),
                              ("her_reach_sac_vec_hip", "her_sac_exp_script.py", "sac_params")):
        path = os.path.join(ROOT, "exp_specs", "her", name + ".yaml")
        spec = yaml.safe_load(open(path))
        assert spec["meta_data"]["script_path"] == "run_scripts/" + script and os.path.exists(os.path.join(ROOT, "run_scripts", script))
        v = next(variants(spec))
        assert v["env_specs"]["env_name"] == "point-reach" and v["env_specs"]["env_num"] == 64 and key in v
        assert v["vec_env_kwargs"] == {"norm_obs": False} and "norm_obs" in open(path).read().split("constants:")[0]
        MODELS_GOAL["point-reach"](**v["env_specs"]["env_kwargs"])
    old = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "her", "her_reach_td3_hip.yaml")))
    assert "env_num" not in old["constants"]["env_specs"]                     # the host loop's spec stays the host loop's
    assert issubclass(her.VecHER, __import__("ilswiss_amd.algorithm", fromlist=["x"]).DeviceRLAlgorithm)
    assert hasattr(her.TD3, "train_from_replay") and hasattr(her.SAC, "train_from_replay")
    assert hasattr(her.MlpGaussianAndEpsilonPolicy, "install") and hasattr(her.MlpGaussianAndEpsilonPolicy, "before_rollout_step")


def test_goal_model_struct_mirrors_the_header(tmp_path):
    from ilswiss_amd import _lib
    from ilswiss_amd.envs.vecenv import goal_struct
    from ilswiss_amd.envs import MODELS_GOAL
    S = _lib.GoalModel
    names = [f[0] for f in S._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ilsx.h"\nint main(void) { printf("%zu", sizeof(ilsx_goal_model));\n'
                   + "".join(f'printf(" %zu", offsetof(ilsx_goal_model, {n}));\n' for n in names) + "return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
    s = goal_struct(MODELS_GOAL["point-reach"](tol=0.07, reward_type="dense"))
    assert (s.tol, s.step_scale, s.p_range, s.g_range, s.reward_kind) == (0.07, 0.1, 0.5, 0.8, 1)


def test_refusals_before_the_library_is_entered():
    """None of these reaches get_context() or libilsx: they raise on a machine without a GPU."""
    from ilswiss_amd import her
    from ilswiss_amd.envs import HipVectorEnv
    with pytest.raises(NotImplementedError, match="norm_obs"):
        HipVectorEnv("point-reach", 4, norm_obs=True)
    with pytest.raises(NotImplementedError, match="ScaledEnv"):
        HipVectorEnv("point-reach", 4, obs_shift=np.zeros(8), obs_scale=np.ones(8))
    with pytest.raises(ValueError, match="unknown env_kwargs"):
        HipVectorEnv("point-reach", 4, env_kwargs=dict(max_steps=50))
    with pytest.raises(ValueError, match="reward_type"):
        HipVectorEnv("point-reach", 4, env_kwargs=dict(reward_type="shaped"))
    for tol in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            HipVectorEnv("point-reach", 4, env_kwargs=dict(tol=tol))
    with pytest.raises(ValueError, match="goal env"):
        HipVectorEnv("hopper", 4, env_kwargs=dict(tol=0.1))
    with pytest.raises(ValueError, match="relabel_type"):
        her.DeviceGoalReplayBuffer(100, her.PointReachEnv(), relabel_type="episode")
    with pytest.raises(TypeError, match="device goal env"):
        her.VecHER(None, None, her.PointReachEnv(), None, None, max_path_length=5, replay_buffer_size=10)
    assert glob.glob(os.path.join(ROOT, "ilswiss_amd", "csrc", "goal_env.h"))
