"""CPU suite for the MountainCarContinuous / MountainCar / Acrobot steppers (csrc/classic_env.h, ILSX_CLASSIC_MOUNTAINCAR_CONT /
_MOUNTAINCAR / _ACROBOT), no GPU needed:

  * known answers of the restatements in tests/gymcc_restatement.py: the goal and the wall of the cars, the float32 action map, Acrobot's
    rotation by 2 pi, wrap and bound, and the energy of the torque-free Acrobot over one RK4 step, whose ORDER is asserted by halving dt
    (measured: the energy error falls by 2^5.1, 2^5.2 and 2^5.15 over dt = 0.2 -> 0.1 -> 0.05 -> 0.025, the local order of RK4);
  * what a libm that is an ulp off glibc's can do to one step: every cos / sin result of the restatement moved by -1, 0 or +1 ulp at
    random over the GPU suite's own input states (gymcc_restatement.parity_inputs, 20 draws of 1000 states).  Measured largest absolute
    deviation of a next-state component: MountainCarContinuous 0 (the float32 store absorbs it), MountainCar 2.22e-16, Acrobot 1.07e-14.
    tests/test_gymcc_hip.py allows 8 x that between the device and the restatement: 0, 1.78e-15, 8.53e-14;
  * the share of those inputs whose result lies within that bound of the threshold `done` compares with (measured 0; at most 0.1 % may be
    left out of the GPU comparison) and that some of them end the episode;
  * names, dicts, envpool names, the three specs, the refusals that come before the library is entered;
  * the compiled step kernels keep no private segment, no scalar spills and no indexed registers."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import gymcc_restatement as gr  # noqa: E402
from gymcc_restatement import Acrobot, MountainCar, MountainCarCont  # noqa: E402

F32 = np.float32
TASKS = list(gr.TASKS.values())


# ---------------------------------------------------------------------------------------------------- the cars
def test_continuous_car_reaches_the_goal_and_is_paid_100_minus_the_push():
    s = np.array([[0.44, 0.069]]).astype(F32).astype(np.float64)
    nxt, rew, done = MountainCarCont.step(s, np.array([1.0], F32))
    assert done[0] and rew[0] == 100.0 - 0.1
    assert nxt[0, 0] >= 0.45 and 0.069 < nxt[0, 1] < 0.07                        # 0.069 + 0.0015 - 0.0025 cos(1.32), under the clamp
    assert np.array_equal(nxt, nxt.astype(F32).astype(np.float64))
    # one step short of the goal: nothing but the push's price
    _, rew, done = MountainCarCont.step(np.array([[0.30, 0.01]]), np.array([0.5], F32))
    assert not done[0] and rew[0] == 0.0 - (0.5 * 0.5) * 0.1
    # at the goal but rolling back: not done
    _, _, done = MountainCarCont.step(np.array([[0.46, -0.005]]), np.array([-1.0], F32))
    assert not done[0]


def test_discrete_car_goal_reward_and_push():
    s = np.array([[0.495, 0.03], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
    nxt, rew, done = MountainCar.step(s, np.array([2, 0, 1, 2], F32))
    assert list(done) == [True, False, False, False] and np.all(rew == -1.0)
    grav = np.cos(0.0) * (-0.0025)
    assert nxt[1, 1] == (0.0 - 1.0) * 0.001 + grav and nxt[2, 1] == 0.0 * 0.001 + grav and nxt[3, 1] == 1.0 * 0.001 + grav
    assert np.array_equal(nxt[1:, 0], nxt[1:, 1])                                 # x' = 0 + v'
    # a value that is no index is used as it is
    odd, _, _ = MountainCar.step(s[1:2], np.array([3.5], F32))
    assert odd[0, 1] == 2.5 * 0.001 + grav
    assert np.isnan(MountainCar.step(s[1:2], np.array([np.nan], F32))[0]).all()


@pytest.mark.parametrize("task", [MountainCarCont, MountainCar], ids=lambda t: t.name)
def test_left_wall_zeroes_a_negative_velocity(task):
    s = np.array([[-1.19, -0.05], [-1.2, -0.01], [0.59, 0.07]]).astype(F32).astype(np.float64)
    nxt, _, done = task.step(s, np.array([0 if task is MountainCar else -1.0] * 3, F32))
    x_min = -1.2 if task is MountainCar else np.float64(F32(-1.2))
    assert nxt[0, 0] == x_min and nxt[0, 1] == 0.0
    assert nxt[1, 0] == x_min and nxt[1, 1] == 0.0                               # still moving left at the wall: stopped again
    assert nxt[2, 0] == (0.6 if task is MountainCar else np.float64(F32(0.6))) and nxt[2, 1] > 0 and done[2]   # the right end only clamps x


def test_float32_action_map_matches_scalar_float32_arithmetic():
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.uniform(-1.3, 1.3, 50000), rng.normal(0, 1e-3, 5000), [-1, 1, 0, -0.5, 0.5, 3, -7.5]]).astype(F32)
    want = np.empty_like(a)
    for i, ai in enumerate(a):
        s = F32(-1) + F32(F32(F32(ai + F32(1)) * F32(0.5)) * F32(2))
        want[i] = min(max(s, F32(-1)), F32(1))
    got = MountainCarCont.force(a)
    assert got.dtype == F32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert got.min() == -1 and got.max() == 1
    assert np.any(got != np.clip(a, -1, 1))                                        # the map is not the identity in float32
    assert np.isnan(MountainCarCont.force(np.array([np.nan], F32))[0])


def test_resets():
    u = np.array([2.0 ** -33, 0.25, 0.5, 1 - 2.0 ** -33])
    for task in (MountainCarCont, MountainCar):
        s = task.reset_from_uniforms(u)
        assert np.all(s[:, 1] == 0) and np.all(s[:, 0] >= -0.6 - 1e-7) and np.all(s[:, 0] <= -0.4 + 1e-7)
    c, d = MountainCarCont.reset_from_uniforms(u), MountainCar.reset_from_uniforms(u)
    assert np.array_equal(c, c.astype(F32).astype(np.float64)) and np.array_equal(c, d.astype(F32).astype(np.float64))
    assert not np.array_equal(d, d.astype(F32).astype(np.float64)) and d[2, 0] == -0.6 + 0.2 * 0.5
    a = Acrobot.reset_from_uniforms(np.tile(u, (3, 1)))
    assert a.shape == (3, 4) and np.all(np.abs(a) <= np.float64(F32(0.1))) and np.array_equal(a, a.astype(F32).astype(np.float64))
    assert a[0, 2] == np.float64(F32(-0.1 + 0.2 * 0.5))


# ---------------------------------------------------------------------------------------------------- Acrobot
def _acro_states(n, seed, vel=1.0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-2, 2, n) * vel, rng.uniform(-2, 2, n) * vel], 1)


def test_acrobot_rotated_by_two_pi_steps_the_same():
    s = _acro_states(500, 0)
    a = np.random.default_rng(1).integers(0, 3, 500).astype(F32)
    want, rew, done = Acrobot.step(s, a)
    for k1, k2 in ((1, 0), (0, 1), (-1, 1), (2, -1)):
        r = s + np.array([k1 * 2 * np.pi, k2 * 2 * np.pi, 0, 0])
        got, rew2, done2 = Acrobot.step(r, a)
        # the same step up to the rounding of theta + 2 k pi and of its cos / sin: wrap() brings the angles back
        far = np.abs(Acrobot.height(want[:, 0], want[:, 1]) - 1) > 1e-9
        edge = (np.abs(np.abs(want[:, :2]) - np.pi) < 1e-9).any(1)                 # a wrapped angle at +-pi may land on either side
        np.testing.assert_allclose(got[~edge], want[~edge], rtol=0, atol=1e-11)
        assert np.array_equal(done2[far], done[far]) and np.array_equal(rew2[far], rew[far])


def test_acrobot_wrap_and_bound_hit_their_limits():
    pi = np.pi
    assert np.array_equal(Acrobot.wrap(np.array([pi, -pi, 0.0, 3.0])), [pi, -pi, 0.0, 3.0])          # the limits themselves stay
    w = Acrobot.wrap(np.array([pi + 1e-9, -pi - 1e-9, 7.0, -7.0, 40.0]))
    assert np.all(np.abs(w) <= pi) and w[0] == (pi + 1e-9) - 2 * pi and w[2] == 7.0 - 2 * pi and w[3] == -7.0 + 2 * pi
    far = Acrobot.wrap(np.array([1e6, np.inf, -np.inf, np.nan]))                                         # the capped loops give up
    assert abs(far[0] - (1e6 - 16 * (2 * pi))) < 1e-6 and np.isinf(far[1]) and np.isinf(far[2]) and np.isnan(far[3])
    # velocities past the bounds after the step: a fast state under full torque
    s = np.array([[0.3, -0.2, 4 * pi, 9 * pi], [0.3, -0.2, -4 * pi, -9 * pi]])
    nxt, rew, done = Acrobot.step(s, np.array([2, 0], F32))
    raw = np.stack(Acrobot.rk4(s, np.array([1.0, -1.0]), 0.2), 1)
    assert np.all(np.abs(raw[:, 2]) > 4 * pi) or np.all(np.abs(raw[:, 3]) > 9 * pi)
    hit1, hit2 = np.abs(raw[:, 2]) > 4 * pi, np.abs(raw[:, 3]) > 9 * pi
    assert np.array_equal(nxt[hit1, 2], np.sign(raw[hit1, 2]) * (4 * pi)) and np.array_equal(nxt[hit2, 3], np.sign(raw[hit2, 3]) * (9 * pi))
    assert np.all(np.abs(nxt[:, 0]) <= pi) and np.all(np.abs(nxt[:, 1]) <= pi)
    # hanging at rest with no torque stays (cos(-pi / 2) is 6e-17, not 0: to rounding), is not terminal and pays -1
    nxt, rew, done = Acrobot.step(np.zeros((1, 4)), np.array([1], F32))
    assert np.all(np.abs(nxt) < 1e-15) and rew[0] == -1.0 and not done[0]
    # the tip above the line: terminal, reward 0
    nxt, rew, done = Acrobot.step(np.array([[pi - 0.1, 0.0, 0.0, 0.0]]), np.array([1], F32))
    assert done[0] and rew[0] == 0.0


def test_acrobot_observation():
    s = _acro_states(50, 2)
    o = Acrobot.observe(s)
    assert o.dtype == F32 and o.shape == (50, 6)
    np.testing.assert_allclose(o, np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]), s[:, 2], s[:, 3]], 1), atol=1e-6)


def test_torque_free_acrobot_conserves_energy_to_the_integrators_order():
    """The energy error of ONE RK4 step is the method's local error, O(dt^5): halving dt divides it by 2^5.  The order is asserted, no
    tolerance on the energy itself (at gym's dt = 0.2 the step moves it by up to 1e-2)."""
    s = _acro_states(200, 0)
    e0 = Acrobot.energy(s)
    errs = []
    for dt in (0.2, 0.1, 0.05, 0.025):
        n = np.stack(Acrobot.rk4(s, np.zeros(200), dt), 1)
        errs.append(np.abs(Acrobot.energy(n) - e0).max())
    orders = [np.log2(errs[i] / errs[i + 1]) for i in range(3)]
    print("energy errors", errs, "orders", orders)
    assert all(4.5 < o < 5.5 for o in orders), orders
    # a torque does work: the same measure no longer falls with dt^5
    n1 = np.stack(Acrobot.rk4(s, np.ones(200), 0.05), 1)
    n2 = np.stack(Acrobot.rk4(s, np.ones(200), 0.025), 1)
    assert np.log2(np.abs(Acrobot.energy(n1) - e0).max() / np.abs(Acrobot.energy(n2) - e0).max()) < 2.0


# ---------------------------------------------------------------------------------------------------- what an ulp of libm can do
@pytest.mark.parametrize("task", TASKS, ids=lambda t: t.name)
def test_ulp_perturbed_libm_deviation_is_what_the_gpu_bound_is_built_on(task):
    worst, ended, left_out, total = 0.0, 0, 0, 0
    for seed in range(20):
        s, a = gr.parity_inputs(task, 1000, seed)
        want, _, done = task.step(s, a)
        got, _, _ = task.step(s, a, gr.UlpLibm(seed))
        worst = max(worst, float(np.abs(got - want).max()))
        ended += int(done.sum())
        left_out += int((gr.done_margin(task, s, a) <= gr.ULP_FACTOR * gr.ULP_DEV[task.name]).sum())
        total += len(s)
    print(f"{task.name}: largest deviation {worst!r}, {ended} of {total} end the episode, {left_out} within the bound of the threshold")
    assert worst <= gr.ULP_DEV[task.name] and worst >= 0.5 * gr.ULP_DEV[task.name]     # the figure in use is the measured one
    assert left_out <= 1e-3 * total
    assert ended >= 0.05 * total                                                            # the inputs are seeded near the goal


def test_parity_inputs_are_what_the_tasks_take():
    s, a = gr.parity_inputs(MountainCarCont, 1000, 0)
    assert np.array_equal(s, s.astype(F32).astype(np.float64)) and a.dtype == F32 and a.min() < -1 and a.max() > 1
    for task in (MountainCar, Acrobot):
        s, a = gr.parity_inputs(task, 1000, 0)
        assert sorted(set(a[:, 0])) == [0.0, 1.0, 2.0] and s.shape == (1000, 2 * task.nq)
    assert np.array_equal(gr.parity_inputs(Acrobot, 10, 3)[0], gr.parity_inputs(Acrobot, 10, 3)[0])


# ---------------------------------------------------------------------------------------------------- names, specs, refusals
def test_names_resolve_and_existing_dicts_are_unchanged():
    from ilswiss_amd import envs
    from ilswiss_amd.envs import CARTCHAIN, CLASSIC, CLASSIC_KINDS, GYM_CLASSIC, LUNAR, SWIMMER
    from ilswiss_amd.envs.envpool import _model_name
    assert GYM_CLASSIC == {"mountaincarcont": 4, "mountaincar": 5, "acrobot": 6} and envs.vecenv.GYM_CLASSIC is GYM_CLASSIC
    assert {t.name: t.kind for t in TASKS} == GYM_CLASSIC
    assert CLASSIC == {"cartpole": 0, "pendulum": 1} and CARTCHAIN == {"invertedpendulum": 2, "inverteddoublependulum": 3}
    assert CLASSIC_KINDS == {**CLASSIC, **CARTCHAIN} and SWIMMER == {"swimmer": 16} and LUNAR == {"lunarlandercont": 17}
    assert not set(GYM_CLASSIC) & (set(CLASSIC_KINDS) | set(SWIMMER) | set(LUNAR))
    assert _model_name("MountainCarContinuous-v0") == "mountaincarcont" and _model_name("MountainCar-v0") == "mountaincar"
    assert _model_name("Acrobot-v1") == "acrobot"
    h = open(os.path.join(ROOT, "include", "ilsx.h")).read()
    assert re.search(r"ILSX_CLASSIC_MOUNTAINCAR_CONT = 4, ILSX_CLASSIC_MOUNTAINCAR = 5, ILSX_CLASSIC_ACROBOT = 6\b", h)


def test_wrappers_and_models_are_refused_before_the_library_is_entered():
    from ilswiss_amd.envs import HipVectorEnv
    nothing = object()                                                 # a context that must not be touched
    for t in TASKS:
        with pytest.raises(NotImplementedError, match="classic-control"):
            HipVectorEnv(t.name, 4, ctx=nothing, obs_shift=np.zeros(t.obs_dim), obs_scale=np.ones(t.obs_dim))
        with pytest.raises(ValueError, match="no model description"):
            HipVectorEnv(t.name, 4, ctx=nothing, model={})


def test_gen_expert_demos_builds_its_env_from_the_name():
    """run_scripts/gen_expert_demos.py (the shape of the reference's gen_expert/mountain.yaml: env_name mountaincarcont) hands --env to
    HipVectorEnv, which resolves every name of GYM_CLASSIC."""
    src = open(os.path.join(ROOT, "run_scripts", "gen_expert_demos.py")).read()
    assert re.search(r"HipVectorEnv\(a\.env,", src) and 'add_argument("--env"' in src and "choices" not in src
    from ilswiss_amd.envs.vecenv import GYM_CLASSIC
    assert "mountaincarcont" in GYM_CLASSIC


def _spec(name):
    import yaml
    return yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "sac", name)))


def test_sac_mountain_spec_carries_the_references_values():
    s = _spec("sac_mountain_hip.yaml")
    c = s["constants"]
    assert s["meta_data"] == dict(script_path="run_scripts/sac_exp_script.py", exp_name="test_sac_mountain",
                                  description="Train an agent using Soft-Actor-Critic", num_workers=1, using_gpus=True)
    assert s["variables"] == {"seed": [723894]} and c["net_size"] == 256 and c["num_hidden_layers"] == 2
    assert c["env_specs"] == dict(env_name="mountaincarcont", env_kwargs={}, env_num=10, training_env_seed=723894, eval_env_seed=723894)
    assert c["rl_alg_params"] == dict(num_epochs=101, num_steps_per_epoch=10000, num_steps_between_train_calls=1000,
                                      num_train_steps_per_train_call=1000, num_steps_per_eval=10000, max_path_length=100,
                                      min_steps_before_training=1000, eval_deterministic=True, batch_size=256, replay_buffer_size=100000,
                                      no_terminal=False, wrap_absorbing=False, save_best=True, freq_saving=10, save_replay_buffer=False)
    assert c["sac_params"] == dict(alpha=0.2, reward_scale=1.0, discount=0.99, soft_target_tau=0.005, policy_lr=1e-4, qf_lr=3e-4,
                                   vf_lr=3e-4, policy_mean_reg_weight=1e-3, policy_std_reg_weight=1e-3)
    assert set(c) == {"net_size", "num_hidden_layers", "rl_alg_params", "sac_params", "env_specs"}
    assert 1000 % c["env_specs"]["env_num"] == 0


@pytest.mark.parametrize("name,env,maxlen", [("sac_mountaincar_d_hip.yaml", "mountaincar", 200), ("sac_acrobot_d_hip.yaml", "acrobot", 500)])
def test_discrete_specs_are_the_cartpole_spec_with_the_tasks_name_and_length(name, env, maxlen):
    s, base = _spec(name), _spec("sac_cartpole_d_hip.yaml")
    assert s["meta_data"]["script_path"] == "run_scripts/discrete_sac_exp_script.py" and s["variables"] == base["variables"]
    c, b = s["constants"], base["constants"]
    assert c["env_specs"] == dict(b["env_specs"], env_name=env)
    assert c["rl_alg_params"] == dict(b["rl_alg_params"], max_path_length=maxlen)
    assert c["sac_params"] == b["sac_params"] and c["net_size"] == b["net_size"] and c["num_hidden_layers"] == b["num_hidden_layers"]
    assert set(s) == set(base) and set(c) == set(b) and set(s["meta_data"]) == set(base["meta_data"])


# ---------------------------------------------------------------------------------------------------- compiled kernels
def test_new_kernels_compile_without_scratch_spills_or_indexed_registers():
    import test_pendulum_cpu as tp
    if not os.path.exists(tp.HIPCC):
        pytest.skip("no hipcc")
    ks = tp._kernels(os.path.join(tp.CSRC, "ilsx_env.hip"))
    names = [f"k_{t}_{w}" for t in ("mountaincar_cont", "mountaincar", "acrobot") for w in ("step", "reset")]
    found = {}
    for sym, (ops, priv) in ks.items():
        dn = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        for k in names:
            if dn.startswith(k + "("):
                found[k] = (ops, priv)
    assert sorted(found) == sorted(names), sorted(found)
    for name, (ops, priv) in found.items():
        assert priv == 0 and not any(o.startswith("scratch_") for o in ops), (name, priv)      # no private segment: no VGPR spills
        assert not any(o.startswith("v_writelane") for o in ops), name                           # no scalar registers spilled to lanes
        assert not any(o.startswith("s_set_gpr_idx") or "movrel" in o for o in ops), name
        assert any(o.startswith("global_store") for o in ops), name
