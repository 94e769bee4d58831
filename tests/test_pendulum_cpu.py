"""CPU suite for the Pendulum engine (csrc/classic_env.h, ILSX_CLASSIC_PENDULUM), no GPU needed:

  * known answers of the restatement in tests/pendulum_restatement.py (gym 0.22's PendulumEnv behind NormalizedBoxEnv);
  * the two new specs load and carry the reference's values;
  * guards on the COMPILED stepper (hipcc -S, in the style of test_gcsl_isa.py / test_dsac_isa.py): every kernel and device function of
    every csrc/*.hip compiles to the same instructions as before the Pendulum engine existed (the sources at the parent of the commit that
    added tests/pendulum_restatement.py, or at HEAD while that file is not committed yet), up to the numbering of block labels; the new
    kernels keep no scratch (private segment 0, no scratch_* instructions) and no indexed registers (s_set_gpr_idx / movrel)."""
import io
import os
import re
import shutil
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pendulum_restatement as pr  # noqa: E402

ROOT = os.path.dirname(HERE)


# ---------------------------------------------------------------------------------------------------- restatement known answers
def test_rest_state_pays_nothing_and_stays():
    nxt, rew, obs = pr.pendulum_step(np.zeros((1, 2)), np.zeros(1, np.float32))
    assert rew[0] == 0.0 and np.array_equal(nxt, np.zeros((1, 2)))
    assert np.array_equal(obs, np.array([[1.0, 0.0, 0.0]], np.float32))


def test_hanging_down_costs_pi_squared():
    _, rew, _ = pr.pendulum_step(np.array([[np.pi, 0.0]]), np.zeros(1, np.float32))
    # angle_normalize(pi) = ((2 pi) % (2 pi)) - pi = -pi
    assert rew[0] == -(np.pi * np.pi)


def test_action_map_endpoints_and_clip():
    assert pr.torque(np.array([1.0], np.float32))[0] == 2.0
    assert pr.torque(np.array([-1.0], np.float32))[0] == -2.0
    assert pr.torque(np.array([0.0], np.float32))[0] == 0.0
    assert pr.torque(np.array([3.0], np.float32))[0] == 2.0
    assert pr.torque(np.array([-7.5], np.float32))[0] == -2.0
    # the torque enters the dynamics: from rest, a = 1 gives theta_dot' = 3 * 2 * 0.05 and costs 0.001 * 4
    nxt, rew, _ = pr.pendulum_step(np.zeros((1, 2)), np.array([1.0], np.float32))
    assert nxt[0, 1] == (0.0 + (15.0 * 0.0 + 3.0 * 2.0) * 0.05) and rew[0] == -0.004
    assert nxt[0, 0] == nxt[0, 1] * 0.05


def test_velocity_clip_comes_before_the_position_update():
    s = np.array([[np.pi / 2, 7.9], [-np.pi / 2, -7.9]])
    nxt, _, obs = pr.pendulum_step(s, np.array([1.0, -1.0], np.float32))
    assert np.array_equal(nxt[:, 1], [8.0, -8.0])
    assert np.array_equal(nxt[:, 0], s[:, 0] + np.array([8.0, -8.0]) * 0.05)   # gym 0.22: the clipped velocity moves theta
    assert np.array_equal(obs[:, 2], np.float32([8.0, -8.0]))


def test_angle_normalize():
    x = np.array([-0.5, -3.0, -7.0, -100.0, 4.0, 10.0, 1e3, 123456.789, 0.0])
    got = pr.angle_normalize(x)
    assert np.all(got >= -np.pi) and np.all(got < np.pi)
    np.testing.assert_allclose(np.cos(got), np.cos(x), atol=1e-9)
    np.testing.assert_allclose(np.sin(got), np.sin(x), atol=1e-9)
    assert pr.angle_normalize(np.array([-0.5]))[0] == -0.5
    # exact multiples of 2 pi (as float64 values): x + pi lands on a representable odd multiple of pi, the remainder is a multiple of the
    # float64 2 pi or nearly so; both forms agree bit for bit, and the result is -pi or within rounding of it / of 0
    k = np.arange(-5, 6, dtype=np.float64)
    m = k * (2 * np.pi)
    assert np.array_equal(pr.angle_normalize(m), pr.angle_normalize_fmod(m))
    assert np.all(np.abs(pr.angle_normalize(m)) < 1e-12)
    odd = (2 * k + 1) * np.pi
    assert np.array_equal(pr.angle_normalize(odd), pr.angle_normalize_fmod(odd))
    assert np.all(np.abs(np.abs(pr.angle_normalize(odd)) - np.pi) < 1e-12)
    assert pr.angle_normalize(np.array([np.pi]))[0] == -np.pi    # (2 pi) % (2 pi) = +0.0


def test_angle_normalize_fmod_form_is_numpys_mod_bit_for_bit():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-50, 50, 200000), rng.uniform(-1e6, 1e6, 20000), np.arange(-64, 65) * np.pi,
                        np.arange(-64, 65) * (np.pi / 2), [-np.pi, np.pi, -0.0, 0.0, 5e-324, -5e-324]])
    a, b = pr.angle_normalize(x), pr.angle_normalize_fmod(x)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_float32_action_map_matches_numpy_float32_arithmetic():
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.uniform(-1.2, 1.2, 100000), rng.normal(0, 1e-3, 10000), [-1, 1, 0, -0.5, 0.5]]).astype(np.float32)
    want = np.empty_like(a)
    f = np.float32
    for i, ai in enumerate(a):   # scalar float32 arithmetic, one rounding per operation
        s = f(-2) + f(f(f(ai + f(1)) * f(0.5)) * f(4))
        want[i] = min(max(s, f(-2)), f(2))
    got = pr.torque(a)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    # float32 matters: the same map in float64 rounds differently on some actions
    exact = np.clip(-2.0 + (a.astype(np.float64) + 1.0) * 0.5 * 4.0, -2, 2).astype(np.float32)
    assert np.any(exact != got)


def test_cost_with_float32_rounded_square_moves_less_than_float32_reward_resolution():
    rng = np.random.default_rng(2)
    u = pr.torque(rng.uniform(-1, 1, 100000).astype(np.float32))
    d = np.abs(0.001 * (u.astype(np.float64) ** 2) - 0.001 * np.float64(u * u))
    assert d.max() < 3e-10


def test_reset_range():
    u = np.array([0.0, 0.5, 1.0 - 2 ** -33, 2 ** -33])
    s = pr.reset_state(u, u)
    assert s[0, 0] == -np.pi and s[0, 1] == -1.0 and s[1, 0] == 0.0 and s[1, 1] == 0.0
    assert np.all(s[:, 0] >= -np.pi) and np.all(s[:, 0] < np.pi) and np.all(s[:, 1] >= -1) and np.all(s[:, 1] < 1)


# ---------------------------------------------------------------------------------------------------- specs
def _spec(rel):
    import yaml
    return yaml.safe_load(open(os.path.join(ROOT, "exp_specs", rel)))


def test_sac_spec_carries_the_references_values():
    s = _spec("sac/sac_pendulum_hip.yaml")
    c = s["constants"]
    assert s["meta_data"]["script_path"] == "run_scripts/sac_alpha_exp_script.py" and s["variables"]["seed"] == [723894]
    assert c["net_size"] == 256 and c["num_hidden_layers"] == 2
    assert c["env_specs"]["env_name"] == "pendulum" and c["env_specs"]["env_kwargs"] == {}
    assert "env_num" not in c["env_specs"]   # one env, as the reference
    assert c["rl_alg_params"] == dict(num_epochs=51, num_steps_per_epoch=1000, num_steps_between_train_calls=1000,
                                      num_train_steps_per_train_call=1000, num_steps_per_eval=10000, max_path_length=1000,
                                      min_steps_before_training=1000, eval_deterministic=True, batch_size=256, replay_buffer_size=10000,
                                      no_terminal=False, wrap_absorbing=False, save_best=True, freq_saving=10, save_replay_buffer=False)
    assert c["sac_params"] == dict(alpha=0.2, reward_scale=2.0, discount=0.99, soft_target_tau=0.005, policy_lr=3e-4, qf_lr=1e-3,
                                   vf_lr=3e-4, policy_mean_reg_weight=1e-3, policy_std_reg_weight=1e-3)


def test_ppo_spec_carries_the_references_values():
    s = _spec("ppo/ppo_pendulum_hip.yaml")
    c = s["constants"]
    assert s["meta_data"]["script_path"] == "run_scripts/ppo_exp_script.py" and s["variables"]["seed"] == [0, 1, 2, 3, 4]
    assert c["net_size"] == 256 and c["num_hidden_layers"] == 2
    assert c["env_specs"] == dict(env_name="pendulum", env_kwargs={}, training_env_num=1, eval_env_num=1)
    assert c["rl_alg_params"] == dict(num_epochs=300, num_steps_per_epoch=10000, num_steps_between_train_calls=2048,
                                      num_train_steps_per_train_call=1, num_steps_per_eval=10000, max_path_length=200,
                                      min_steps_before_training=2048, eval_deterministic=True, batch_size=256, replay_buffer_size=1000000,
                                      no_terminal=False, wrap_absorbing=False, save_best=False, freq_saving=10, save_replay_buffer=False)
    assert c["ppo_params"] == dict(clip_eps=0.2, reward_scale=1.0, discount=0.99, policy_lr=3e-4, value_lr=3e-4, lambda_entropy_policy=0.0,
                                   gae_tau=0.95, value_l2_reg=1e-3, mini_batch_size=128, update_epoch=10)


def test_pendulum_is_a_classic_task():
    from ilswiss_amd.envs import CLASSIC
    assert CLASSIC == {"cartpole": 0, "pendulum": 1}
    h = open(os.path.join(ROOT, "include", "ilsx.h")).read()
    assert re.search(r"ILSX_CLASSIC_PENDULUM = 1\b", h)


# ---------------------------------------------------------------------------------------------------- compiled kernels
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "ilswiss_amd", "csrc")
NEW = ("k_pendulum_step", "k_pendulum_reset")


def _kernels(path):
    d = tempfile.mkdtemp(prefix="isa_")
    out = os.path.join(d, "k.s")
    try:
        r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                            "-I", os.path.dirname(path), path, "-o", out], capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out).read().split("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    ks = {}
    for i, l in enumerate(text):
        m = re.match(r"^(_Z\w+):\s", l)
        if not m:
            continue
        end = next(j for j in range(i, len(text)) if text[j].startswith(".Lfunc_end"))
        ops = [re.sub(r"\.LBB\d+_", ".LBB_", x.split(";")[0].strip()) for x in text[i + 1:end]
               if x.strip() and not x.lstrip().startswith((";", "."))]   # block labels carry the function's ordinal: normalised
        meta = "\n".join(text[end:end + 150])
        priv = re.search(r"\.private_seg_size, (\d+)", meta)
        ks[m.group(1)] = (ops, int(priv.group(1)) if priv else None)
    return ks


def _compile_tree(csrc):
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(srcs, ex.map(lambda f: _kernels(os.path.join(csrc, f)), srcs)))


def _git(*a):
    r = subprocess.run(["git", "-C", ROOT, *a], capture_output=True)
    return r.stdout if r.returncode == 0 else None


@pytest.fixture(scope="module")
def now():
    return _compile_tree(CSRC)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_new_kernels_have_no_scratch_and_no_indexed_registers(now):
    env = now["ilsx_env.hip"]
    found = {}
    for sym, (ops, priv) in env.items():
        dn = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        name = next((k for k in NEW if dn.startswith(k + "(")), None)
        if name:
            found[name] = (ops, priv)
    assert sorted(found) == sorted(NEW), sorted(found)
    for name, (ops, priv) in found.items():
        assert priv == 0 and not any(o.startswith("scratch_") for o in ops), (name, priv)
        assert not any(o.startswith("s_set_gpr_idx") or "movrel" in o for o in ops), name
        assert any(o.startswith("global_store") for o in ops), name


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("git") is None, reason="no hipcc / git")
def test_existing_kernels_compile_to_the_same_instructions(now):
    if _git("rev-parse", "--git-dir") is None:
        pytest.skip("no git history in this checkout")
    added = (_git("log", "--diff-filter=A", "--format=%H", "--", "tests/pendulum_restatement.py") or b"").decode().split()
    rev = added[-1] + "^" if added else "HEAD"
    tar = _git("archive", "--format=tar", rev, "ilswiss_amd/csrc", "include")
    assert tar, f"git archive {rev} failed"
    d = tempfile.mkdtemp(prefix="isa_parent_")
    try:
        with tarfile.open(fileobj=io.BytesIO(tar)) as tf:
            tf.extractall(d)
        before = _compile_tree(os.path.join(d, "ilswiss_amd", "csrc"))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    assert sorted(before) == sorted(now), "the set of HIP sources changed"
    n = 0
    for src, ks in before.items():
        missing = sorted(set(ks) - set(now[src]))
        assert not missing, (src, missing[:5])
        changed = [k for k in ks if now[src][k] != ks[k]]
        assert not changed, (src, changed[:5])
        n += len(ks)
    assert n > 100   # every kernel and out-of-line device function of the library
