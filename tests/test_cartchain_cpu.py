"""CPU suite for the cart-and-poles tasks of the classic-control engine (InvertedPendulum / InvertedDoublePendulum, k_cartchain_step of
csrc/classic_env.h), no GPU needed: physical known answers of the restatement in tests/cartchain_restatement.py, its task rules against
oracle/terminals.py, the share of near-threshold steps the GPU parity test may excuse, the names, the ctypes mirror of the model struct
and the two specs."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import cartchain_restatement as cr  # noqa: E402
from ilswiss_amd.envs.models_cartchain import MODELS_CARTCHAIN, inverted_double_pendulum, inverted_pendulum  # noqa: E402
from oracle import terminals as oterm  # noqa: E402

STATE_TOL_CAP = 1e-9    # the GPU parity test's cap on the relative state tolerance


def _free(model):
    """No actuator, no damping, no limits: a conservative system."""
    m = dict(model)
    m.update(gear=0.0, damping=[0.0] * len(model["damping"]), limited=[0] * len(model["limited"]))
    return m


# measured relative drift over 200 steps from a pole at 0.1 rad (relative to the upright pose's energy): InvertedPendulum 4.50e-05 (8 s of
# the pole swinging through the bottom, RK4 at h = 0.02), InvertedDoublePendulum 8.40e-03 (10 s of the free double pendulum at h = 0.01);
# at half the time step the drifts are 1.60e-06 and 1.41e-04 (28x and 59x smaller: the integrator's order, not a modelling error).
# Asserted at 10x the measured value.
@pytest.mark.parametrize("make,bound", [(inverted_pendulum, 4.5e-4), (inverted_double_pendulum, 8.4e-2)])
def test_energy_is_conserved_without_actuator_and_damping(make, bound):
    c = cr.CartChain(_free(make()))
    q = np.zeros((1, c.n)); v = np.zeros((1, c.n))
    q[0, 1] = 0.1
    e0 = c.energy(q, v)[0]
    scale = max(abs(e0), abs(c.energy(np.zeros((1, c.n)), v)[0]))
    drift = 0.0
    for _ in range(200):
        q, v, _, _, _, _ = c.step(q, v, np.zeros(1, np.float32))
        drift = max(drift, abs(c.energy(q, v)[0] - e0) / scale)
    print(f"{make.__name__}: relative energy drift over 200 steps {drift:.3e}")
    assert np.abs(q[0, 1:]).max() > 1.0        # the pole did fall
    assert drift < bound


@pytest.mark.parametrize("make", [inverted_pendulum, inverted_double_pendulum])
def test_a_pole_hanging_down_stays_at_rest(make):
    m = make()
    m["limited"] = [0] * len(m["limited"])      # the InvertedPendulum hinge range would not let the pole hang
    c = cr.CartChain(m)
    q = np.zeros((1, c.n)); v = np.zeros((1, c.n))
    q[0, 1] = np.pi
    # the InvertedPendulum pole leans by atan(0.001 / 0.6): its rest angle is where the COM is under the hinge
    q[0, 1] += m["jsign"] * np.arctan2(m["com"][1][0], m["com"][1][1])
    q0 = q.copy()
    for _ in range(50):
        q, v, _, _, _, _ = c.step(q, v, np.zeros(1, np.float32))
    assert np.abs(q - q0).max() < 1e-9 and np.abs(v).max() < 1e-9


def test_terminal_rules_agree_with_the_oracle_predicates():
    rng = np.random.default_rng(0)
    for make, name in ((inverted_pendulum, "inverted_pendulum"), (inverted_double_pendulum, "inverted_double_pendulum")):
        c = cr.CartChain(make())
        n = 512
        q = np.zeros((n, c.n)); v = rng.normal(0, 1, (n, c.n))
        q[:, 0] = rng.uniform(-0.5, 0.5, n)
        # both sides of either threshold: |theta| around 0.2; the double pendulum's tip around y = 1 (0.6 (cos t1 + cos(t1 + t2)) = 1)
        q[:, 1:] = rng.uniform(-0.4, 0.4, (n, c.n - 1)) if c.n == 2 else rng.uniform(-0.9, 0.9, (n, c.n - 1))
        q2, v2, qfrc, obs, rew, done = c.step(q, v, rng.uniform(-1, 1, n).astype(np.float32))
        want = oterm.is_terminal(name, obs)[:, 0]
        # float32 observations against the float64 rule: only a state within float32 rounding of the threshold may differ
        near = np.abs(c.margin(q2)) < 1e-6
        assert 0.2 < done.mean() < 0.8
        assert np.array_equal(done[~near], want[~near]) and near.sum() <= 2
        if c.n == 3:
            assert np.allclose(c.tip(q2)[:, 1], 0.6 * (np.cos(q2[:, 1]) + np.cos(q2[:, 1] + q2[:, 2])), rtol=0, atol=1e-12)
            assert np.all(rew < 10.0) and np.all(obs[:, 8:] == 0.0)
        else:
            assert np.all(rew == 1.0)


@pytest.mark.parametrize("make", [inverted_pendulum, inverted_double_pendulum])
def test_full_push_comes_to_rest_at_the_soft_slide_limit(make):
    """A constant full action (300 N / 500 N on ~14 kg / ~18 kg) drives the cart into the slide's upper limit, where the soft row stops
    it: it comes to rest near x = 1 inside the limit's softness (|x| < 1.05; measured rest 1.0006 / 1.0008, the row holding the whole
    thrust) and its velocity goes to zero.  The bound is asserted on the rest position (the last 50 steps).  The cart ARRIVES at several
    m/s, so the transient overshoots the rest position (measured peak 1.0506 / 1.0590): it is printed, not bounded.  The double pendulum's poles, on hinges with damping 0.05, still swing after 400 steps and shake the cart a little,
    hence a bound on the cart's speed of 1e-2 m/s (a thousandth of its arrival speed) rather than an exact zero."""
    c = cr.CartChain(make())
    q = np.zeros((1, c.n)); v = np.zeros((1, c.n))
    xs, fs, vmax = [], [], 0.0
    for _ in range(400):
        q, v, qfrc, _, _, _ = c.step(q, v, np.ones(1, np.float32))
        xs.append(q[0, 0]); fs.append(qfrc[0, 0]); vmax = max(vmax, abs(v[0, 0]))
    print(f"{make.__name__}: peak x {max(xs):.4f}, rest x {xs[-1]:.4f}, cart speed {abs(v[0, 0]):.2e} (peak {vmax:.2f}), row force {fs[-1]:.1f}")
    rest = np.array(xs[-50:])
    assert np.all(rest > 1.0) and np.all(np.abs(rest) < 1.05)
    assert abs(v[0, 0]) < 1e-2 and vmax > 1.0
    assert fs[-1] < 0.0 and np.ptp(rest) < 1e-3          # held by the row, which pushes back (J = -e_0 at the upper limit)


def test_reset_ranges():
    rng = np.random.default_rng(1)
    q, v = cr.CartChain(inverted_pendulum()).reset(rng, 4096)
    assert q.shape == v.shape == (4096, 2) and np.abs(q).max() <= 0.01 and np.abs(v).max() <= 0.01 and q.std() > 0.005
    q, v = cr.CartChain(inverted_double_pendulum()).reset(rng, 4096)
    assert q.shape == v.shape == (4096, 3) and np.abs(q).max() <= 0.1 and q.std() > 0.05
    assert 0.09 < v.std() < 0.11 and np.abs(v).max() > 0.25


def test_action_map_is_float32_and_clipped():
    c = cr.CartChain(inverted_pendulum())
    a = np.array([-1.0, 1.0, 0.0, 0.3, 5.0, -7.0], np.float32)
    assert np.array_equal(c.ctrl(a), np.array([-3.0, 3.0, 0.0, np.float32(-3.0) + np.float32(1.3) * np.float32(0.5) * np.float32(6.0), 3.0, -3.0],
                                              np.float32))
    d = cr.CartChain(inverted_double_pendulum()).ctrl(a)      # lb = -1, ub = 1: the identity up to float32 rounding of (a + 1) - 1, then the clip
    assert d.dtype == np.float32 and np.array_equal(d[[0, 1, 2, 4, 5]], [-1, 1, 0, 1, -1]) and abs(d[3] - np.float32(0.3)) < 1e-7


def test_near_threshold_share_of_the_parity_protocol_stays_under_the_excuse():
    """The GPU parity test (test_cartchain_hip.py) excuses a done flag that differs where |theta| - 0.2 or y_tip - 1 lies within 4x the
    state tolerance of zero, for at most 0.5 % of the steps.  This replays its PROTOCOL on the restatement alone: 64 envs, 200
    auto-resetting steps, uniform random actions.  It is a statistical check of the protocol, not of the device's draws: the actions and
    resets here come from numpy's default_rng(11), the device's from its Philox stream with key 11, which numpy cannot reproduce (the GPU
    run itself recorded 0 excused steps of 12800 on both tasks, profiles/cartchain_parity.json).  Two counts per task, both under 0.5 %:
      * the steps whose done flag FLIPS when the state is perturbed by the tolerance's cap, q -> q + s * 1e-9 * max(1, |q|) for every sign
        pattern s of the pole angles (the cart's position enters neither rule);
      * the steps whose margin lies inside the window the GPU test excuses, 4 * 1e-9: a state moved by 1e-9 relative moves theta by at most
        1e-9 * max(1, |theta|) and y_tip by at most 2 * 1.2e-9 (two levers of 0.6, two angles), so the window covers every such flip."""
    for make in (inverted_pendulum, inverted_double_pendulum):
        c = cr.CartChain(make())
        rng = np.random.default_rng(11)
        q, v = c.reset(rng, 64)
        ep = np.zeros(64, int)
        near = flips = steps = 0
        signs = [s for s in np.ndindex(*([2] * (c.n - 1)))]
        for _ in range(200):
            q, v, _, _, _, done = c.step(q, v, rng.uniform(-1, 1, 64).astype(np.float32))
            inside = np.abs(c.margin(q)) <= 4 * STATE_TOL_CAP
            near += int(inside.sum())
            flipped = np.zeros(64, bool)
            base = c.margin(q) > 0.0 if c.n == 2 else c.margin(q) <= 0.0
            for sg in signs:
                qp = q.copy()
                qp[:, 1:] += (2.0 * np.array(sg) - 1.0) * STATE_TOL_CAP * np.maximum(1.0, np.abs(q[:, 1:]))
                flipped |= (c.margin(qp) > 0.0 if c.n == 2 else c.margin(qp) <= 0.0) != base
            assert not np.any(flipped & ~inside)         # the excused window covers every flip
            flips += int(flipped.sum())
            steps += 64
            ep += 1
            end = done | (ep >= 1000)
            q0, v0 = c.reset(rng, 64)
            q[end], v[end], ep[end] = q0[end], v0[end], 0
        print(f"{make.__name__}: {flips} flips, {near} margins inside the window, of {steps} steps")
        assert flips <= 0.005 * steps and near <= 0.005 * steps, (make.__name__, flips, near, steps)


def test_names_resolve():
    from ilswiss_amd.envs import CARTCHAIN, CLASSIC, CLASSIC_KINDS
    from ilswiss_amd.envs.envpool import _model_name
    from ilswiss_amd.envs.terminals import KINDS
    assert CARTCHAIN == {"invertedpendulum": 2, "inverteddoublependulum": 3} and sorted(MODELS_CARTCHAIN) == sorted(CARTCHAIN)
    assert CLASSIC_KINDS == {**CLASSIC, **CARTCHAIN} and len(set(CLASSIC_KINDS.values())) == 4
    assert _model_name("InvertedPendulum-v2") == "invertedpendulum" and _model_name("InvertedDoublePendulum-v2") == "inverteddoublependulum"
    assert KINDS["InvertedPendulum"] == 0 and KINDS["InvertedDoublePendulum"] == 1
    h = open(os.path.join(ROOT, "include", "ilsx.h")).read()
    assert "ILSX_CLASSIC_INVERTED_PENDULUM = 2," in h and "ILSX_CLASSIC_INVERTED_DOUBLE_PENDULUM = 3 }" in h
    for make in MODELS_CARTCHAIN.values():
        m = make()
        n = m["n_pole"] + 1
        assert all(len(m[k]) == n for k in ("mass", "inertia", "com", "anchor", "armature", "damping", "limited", "range"))


def test_model_struct_mirror_matches_the_header(tmp_path):
    from ilswiss_amd import _lib
    from ilswiss_amd.envs.vecenv import cartchain_struct
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ilsx.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   "sizeof(ilsx_cartchain_model), offsetof(ilsx_cartchain_model, tip), offsetof(ilsx_cartchain_model, limit_solimp)); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off_tip, off_imp = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    M = _lib.CartChainModel
    assert (ctypes.sizeof(M), M.tip.offset, M.limit_solimp.offset) == (size, off_tip, off_imp)
    s = cartchain_struct(inverted_double_pendulum())
    assert s.n_pole == 2 and s.frame_skip == 5 and s.gear == 500.0 and list(s.anchor[2]) == [0.0, 0.6] and list(s.limited) == [1, 0, 0]
    assert abs(s.mass[1] - 1000 * np.pi * 0.045 ** 2 * 0.645) < 1e-12


def _spec(rel):
    import yaml
    return yaml.safe_load(open(os.path.join(ROOT, rel)))


def test_specs_carry_the_references_values():
    ref = _spec("tests/golden/g30_inverted_double_spec.yaml")      # the settings of the reference's exp_specs/sac/sac_inverted_double.yaml
    assert ref["constants"]["rl_alg_params"]["batch_size"] == 512 and ref["meta_data"]["script_path"] == "run_scripts/sac_exp_script.py"
    double = _spec("exp_specs/sac/sac_inverted_double_hip.yaml")
    assert double == ref
    single = _spec("exp_specs/sac/sac_inverted_pendulum_hip.yaml")
    assert single["constants"]["env_specs"] == dict(env_name="invertedpendulum", env_kwargs={})
    single["constants"]["env_specs"]["env_name"] = "inverteddoublependulum"
    single["meta_data"]["exp_name"] = ref["meta_data"]["exp_name"]
    assert single == ref
    assert os.path.exists(os.path.join(ROOT, double["meta_data"]["script_path"]))
