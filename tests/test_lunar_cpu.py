"""CPU suite for the LunarLanderContinuous model (ilswiss_amd/envs/models_lunar.py) and its numpy restatement (tests/lunar_restatement.py),
no GPU needed: the host-side mass properties against an independent quadrature, the terrain rule, known answers of the one-body dynamics
and of the engines, the three ways an episode ends, the telescoping reward, the reset.  The device stepper (csrc/lunar_env.h) is pinned
to this restatement by tests/test_lunar_hip.py; here also the ctypes mirror of the model struct, the spec file, the Python surface that
needs no library call, and the compiled kernels' resource use."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import lunar_restatement as lr  # noqa: E402
from ilswiss_amd.envs.models_lunar import MODELS_LUNAR, foot_point, leg_polygon, lunar  # noqa: E402

M = lunar()
L = lr.Lunar(M)
W, H, FPS, SCALE = M["w"], M["h"], M["fps"], M["scale"]
ZERO = np.zeros((1, 2), np.float32)


def flat_terrain(n=1, height=None):
    """smooth_y of a terrain whose 12 heights are all `height` (default: the helipad's, H / 4)."""
    return L.terrain_from_heights(np.full((n, 12), M["helipad_y"] if height is None else height))


def state(x, y, th, sy, vx=0.0, vy=0.0, om=0.0):
    return np.concatenate([[[x, y, th]], sy[:1]], 1), np.array([[vx, vy, om, 0.0]])


def com_velocity(q, v):
    """Velocity of the centre of mass, which carries the momentum: v + omega x r_com."""
    c, s = np.cos(q[0, 2]), np.sin(q[0, 2])
    r = np.array([c * M["com"][0] - s * M["com"][1], s * M["com"][0] + c * M["com"][1]])
    return v[0, :2] + v[0, 2] * np.array([-r[1], r[0]])


def on_the_pad(th=0.0, x=W / 2):
    """Upright (or turned by th) with the hull origin where both feet of the upright lander sit exactly at the pad's surface."""
    sy = flat_terrain()
    return state(x, sy[0, 5] - M["foot"][0][1], th, sy)


# ---------------------------------------------------------------------------------------------------- model
def _quadrature(poly, density, n=200000):
    """mass, centroid and inertia about the centroid of a CONVEX polygon by slicing along x: exact in y, midpoint rule in x."""
    p = np.asarray(poly, np.float64)
    x0, x1 = p[:, 0].min(), p[:, 0].max()
    xs = x0 + (np.arange(n) + 0.5) * (x1 - x0) / n
    lo, hi = np.full(n, np.inf), np.full(n, -np.inf)
    for k in range(len(p)):
        (ax, ay), (bx, by) = p[k], p[(k + 1) % len(p)]
        if ax == bx:
            continue
        inside = (xs >= min(ax, bx)) & (xs <= max(ax, bx))
        y = ay + (by - ay) * (xs - ax) / (bx - ax)
        lo, hi = np.where(inside, np.minimum(lo, y), lo), np.where(inside, np.maximum(hi, y), hi)
    dx = (x1 - x0) / n
    area = np.sum(hi - lo) * dx
    cx = np.sum(xs * (hi - lo)) * dx / area
    cy = np.sum((hi * hi - lo * lo) / 2.0) * dx / area
    j = np.sum(xs * xs * (hi - lo) + (hi ** 3 - lo ** 3) / 3.0) * dx           # about the origin
    return density * area, np.array([cx, cy]), density * (j - area * (cx * cx + cy * cy))


def test_composite_mass_properties_match_a_quadrature_of_the_three_polygons():
    parts = [_quadrature(M["hull_poly"], M["hull_density"])] + [_quadrature(leg_polygon(i), M["leg_density"]) for i in (1, -1)]
    mass = sum(p[0] for p in parts)
    com = sum(p[0] * p[1] for p in parts) / mass
    inertia = sum(p[2] + p[0] * np.sum((p[1] - com) ** 2) for p in parts)
    # the midpoint rule over 2e5 slices of piecewise-linear bounds: relative error below 1e-8; asserted at 1e-6
    np.testing.assert_allclose(M["mass"], mass, rtol=1e-6)
    np.testing.assert_allclose(M["com"], com, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(M["inertia"], inertia, rtol=1e-6)
    assert M["com"][0] == 0.0 and 0.0 < M["com"][1] < 17.0 / SCALE
    # the hull alone: area of the hexagon by hand, (28 + 34) / 2 * 17 + 34 * 10 pixels^2
    np.testing.assert_allclose(parts[0][0], 5.0 * (31.0 * 17.0 + 340.0) / SCALE ** 2, rtol=1e-9)
    np.testing.assert_allclose(parts[1][0], 1.0 * (4.0 * 16.0) / SCALE ** 2, rtol=1e-6)


def test_feet_are_mirror_images_below_and_outside_the_hull():
    (lx, ly), (rx, ry) = M["foot"]
    assert lx == -rx and ly == ry and lx < 0.0
    assert ly < min(p[1] for p in M["hull_poly"]) and abs(lx) > max(abs(p[0]) for p in M["hull_poly"])
    np.testing.assert_allclose([lx, ly], [-0.95, -0.54], atol=5e-3)
    c, s = np.cos(-0.4), np.sin(-0.4)
    np.testing.assert_allclose(foot_point(1), [c * (-20 / 30) - s * (-26 / 30), s * (-20 / 30) + c * (-26 / 30)], rtol=1e-15)
    assert sorted(MODELS_LUNAR) == ["lunarlandercont"]
    from ilswiss_amd.envs import LUNAR, MODELS_LUNAR as exported
    assert exported is MODELS_LUNAR and LUNAR == {"lunarlandercont": 17}
    assert (M["fps"], M["scale"], M["gravity"], M["main_engine_power"], M["side_engine_power"], M["initial_random"]) == (50, 30, -10, 13, 0.6, 1000)
    assert (W, H, M["helipad_y"], M["chunks"]) == (20.0, 400.0 / 30.0, 400.0 / 30.0 / 4.0, 11)
    assert (M["sleep_lin_tol"], M["sleep_ang_tol"], M["sleep_time"]) == (0.01, np.radians(2.0), 0.5)


def test_model_struct_round_trips_every_field_and_mirrors_the_header(tmp_path):
    from ilswiss_amd import _lib
    from ilswiss_amd.envs.vecenv import lunar_struct
    S = _lib.LunarModel
    names = [f[0] for f in S._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ilsx.h"\nint main(void) { printf("%zu", sizeof(ilsx_lunar_model));\n'
                   + "".join(f'printf(" %zu", offsetof(ilsx_lunar_model, {n}));\n' for n in names) + "return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
    h = open(os.path.join(ROOT, "include", "ilsx.h")).read()
    body = h[h.index("typedef struct {\n  int frame_skip, pgs_iters;\n  double fps"):h.index("} ilsx_lunar_model;")]
    assert re.findall(r"[ ,]([a-z_]+)(?:\[\d\])*[,;]", body) == names            # every field of the header, in its order
    assert re.search(r"ILSX_LUNAR_TASK = 17\b", h) and "ILSX_ABI_VERSION 1" in h.replace("  ", " ")
    s = lunar_struct(M)
    for n in names:
        got = getattr(s, n)
        want = {"hull": M["hull_poly"]}.get(n, M.get(n))
        if isinstance(got, (int, float)):
            assert got == want, n
        else:
            assert np.array_equal(np.array([list(r) if hasattr(r, "__len__") else r for r in got]), np.asarray(want, np.float64)), n


# ---------------------------------------------------------------------------------------------------- terrain
def test_terrain_rule():
    rng = np.random.default_rng(0)
    hgt = rng.uniform(0.0, H / 2.0, (5, 12))
    sy = L.terrain_from_heights(hgt)
    assert sy.shape == (5, 11)
    hp = H / 4.0
    assert np.all(sy[:, 4:7] == 0.33 * (hp + hp + hp))                        # the pad: 0.99 H / 4 as the formula gives it
    assert np.all(sy[:, 0] == 0.33 * (hgt[:, 11] + hgt[:, 0] + hgt[:, 1]))    # the first point wraps to the last height
    assert np.all(sy[:, 10] == 0.33 * (hgt[:, 9] + hgt[:, 10] + hgt[:, 11]))
    assert np.all(sy[:, 3] == 0.33 * (hgt[:, 2] + hp + hp)) and np.all(sy[:, 2] == 0.33 * (hgt[:, 1] + hgt[:, 2] + hp))
    # the lookup: a point on the polyline has gap 0, one above it a positive gap, x outside [0, W] uses the end segments
    x = np.array([0.0, 1.0, 3.9, 10.0, 19.99])
    j = np.minimum((x / 2.0).astype(int), 9)
    y = sy[np.arange(5), j] + (sy[np.arange(5), j + 1] - sy[np.arange(5), j]) * (x - 2.0 * j) / 2.0
    g, t = L.gap(sy, np.stack([x, y], 1))
    assert np.abs(g).max() < 1e-14 and np.allclose(np.sum(t * t, 1), 1.0)
    assert np.all(L.gap(sy, np.stack([x, y + 0.5], 1))[0] > 0.0) and np.all(L.gap(sy, np.stack([x, y - 0.5], 1))[0] < 0.0)
    far = L.gap(sy, np.array([[-3.0, 20.0]] * 5))[0]
    assert np.all(far > 0.0)


# ---------------------------------------------------------------------------------------------------- dynamics known answers
def test_free_flight_is_a_parabola():
    q, v = state(7.0, H, 0.3, flat_terrain())
    for k in range(1, 31):
        q, v, obs, rew, done, margin, _ = L.step(q, v, ZERO)
        assert abs(v[0, 1] - (-10.0 * k / FPS)) < 1e-13 and v[0, 0] == 0.0 and v[0, 2] == 0.0
        assert q[0, 0] == 7.0 and q[0, 2] == 0.3 and not done[0] and obs[0, 6] == obs[0, 7] == 0.0
    # semi-implicit Euler with frame_skip substeps of h: y = y0 - g h^2 n (n + 1) / 2, n = 30 * frame_skip
    h, n = 1.0 / FPS / M["frame_skip"], 30 * M["frame_skip"]
    assert abs(q[0, 1] - (H - 10.0 * h * h * n * (n + 1) / 2.0)) < 1e-11


def test_main_engine():
    q0, v0 = state(10.0, 10.0, 0.0, flat_terrain())
    ref = L.step(q0, v0, ZERO)
    for a0, fires in ((1.0, True), (0.0, False), (-1.0, False), (0.5, True), (3.0, True)):
        q, v, _, rew, _, _, _ = L.step(q0, v0, np.array([[a0, 0.0]], np.float32))        # no dispersion
        power = (min(max(a0, 0.0), 1.0) + 1.0) / 2.0 if fires else 0.0
        dp = M["mass"] * (v[0, :2] - ref[1][0, :2])
        assert dp[0] == 0.0 and abs(dp[1] - 13.0 * (4.0 / 30.0) * power) < 1e-13, (a0, dp)
        assert v[0, 2] == 0.0                                                              # fired along the axis: no torque
        if not fires:
            assert np.array_equal(q, ref[0]) and rew[0] == ref[3][0]                       # m_power = 0 in the reward
        else:
            s0, s1 = L.observe64(q0, v0), L.observe64(q, v)
            assert abs(rew[0] - (L.shaping(s1)[0] - L.shaping(s0)[0] - 0.30 * power)) < 1e-12
    # the impulse turns with the hull: at theta it points along (-sin, cos)
    q1, v1 = state(10.0, 10.0, 0.7, flat_terrain())
    base = L.step(q1, v1, ZERO)[1]
    v = L.step(q1, v1, np.array([[1.0, 0.0]], np.float32))[1]
    np.testing.assert_allclose(M["mass"] * (v[0, :2] - base[0, :2]), 13.0 * (4.0 / 30.0) * np.array([-np.sin(0.7), np.cos(0.7)]), atol=1e-13)


def test_side_engines():
    q0, v0 = state(10.0, 10.0, 0.0, flat_terrain())
    ref = L.step(q0, v0, ZERO)
    for a1 in (0.5, -0.5, 0.3, 0.0):                               # the dead zone: |a1| = 0.5 fires nothing
        out = L.step(q0, v0, np.array([[0.0, a1]], np.float32))
        assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1]) and out[3][0] == ref[3][0]
    edge = np.float32(0.5000001)
    assert edge > np.float32(0.5)
    for a1, dirn, power in ((edge, 1.0, float(edge)), (-edge, -1.0, float(edge)), (1.0, 1.0, 1.0), (-7.0, -1.0, 1.0)):
        q, v, _, rew, _, _, _ = L.step(q0, v0, np.array([[0.0, a1]], np.float32))
        # o = side * dir * 12 / SCALE = (-dir 12 / 30, 0) at theta = 0: impulse (+dir 0.6 * 12 / 30 * power, 0)
        dp = M["mass"] * (com_velocity(q, v) - ref[1][0, :2])
        assert abs(dp[0] - dirn * 0.6 * (12.0 / 30.0) * power) < 1e-13 and abs(dp[1]) < 1e-13
        # applied at (-dir 12 / 30, 14 / 30) from the hull origin, above the centre of mass: the torque has the sign of -dir
        lever_y = 14.0 / 30.0 - M["com"][1]
        assert lever_y > 0.0 and np.sign(v[0, 2]) == -dirn
        assert abs(M["inertia"] * v[0, 2] - (-lever_y * dirn * 0.6 * (12.0 / 30.0) * power)) < 1e-14
        s0, s1 = L.observe64(q0, v0), L.observe64(q, v)
        assert abs(rew[0] - (L.shaping(s1)[0] - L.shaping(s0)[0] - 0.03 * power)) < 1e-12


def test_dispersion_moves_the_nozzle():
    q0, v0 = state(10.0, 10.0, 0.0, flat_terrain())
    a = np.array([[1.0, 0.0]], np.float32)
    u_mid = com_velocity(*L.step(q0, v0, a, np.array([[0.5, 0.5]]))[:2])
    u_hi = com_velocity(*L.step(q0, v0, a, np.array([[1.0, 0.5]]))[:2])            # d0 = +1 / SCALE: o grows by 2 d0 along the axis
    q, v = L.step(q0, v0, a, np.array([[0.5, 1.0]]))[:2]                           # d1 = +1 / SCALE: o moves sideways, the impulse with it
    assert abs(M["mass"] * (u_hi[1] - u_mid[1]) - 13.0 * 2.0 / SCALE) < 1e-13 and u_hi[0] == 0.0
    assert abs(M["mass"] * (com_velocity(q, v)[0] - u_mid[0]) - 13.0 * 1.0 / SCALE) < 1e-13 and v[0, 2] != 0.0


# ---------------------------------------------------------------------------------------------------- outcomes
def test_landing_on_the_pad_ends_asleep_with_plus_100():
    q, v = on_the_pad()
    obs0 = L.observe(q, v)
    assert obs0[0, 6] == 1.0 and obs0[0, 7] == 1.0 and obs0[0, 0] == 0.0
    rewards, clock = [], []
    for t in range(60):
        q, v, obs, rew, done, _, over = L.step(q, v, ZERO)
        assert obs[0, 6] == 1.0 and obs[0, 7] == 1.0 and not over[0]
        rewards.append(rew[0]); clock.append(v[0, 3])
        if done[0]:
            break
    assert done[0] and rewards[-1] == 100.0 and all(abs(r) < 1.0 for r in rewards[:-1])
    assert clock[-1] >= 0.5 and clock[-2] < 0.5 and t < 60            # the sleep time and the few tenths of a second the soft rows take to settle
    assert np.hypot(v[0, 0], v[0, 1]) < 0.1 * M["sleep_lin_tol"] and abs(v[0, 2]) < 0.1 * M["sleep_ang_tol"] and abs(q[0, 2]) < 1e-4
    # at rest the feet sit g (dmax tc)^2 = 0.015 inside the surface, where the soft rows carry the weight
    sink = (flat_terrain()[0, 5] - M["foot"][0][1]) - q[0, 1]
    assert 0.01 < sink < 0.02


def test_crash_ends_with_minus_100_by_game_over():
    q, v = on_the_pad(th=np.pi / 2)
    for t in range(200):
        q, v, obs, rew, done, _, over = L.step(q, v, ZERO)
        if done[0]:
            break
    assert done[0] and over[0] and rew[0] == -100.0 and abs(obs[0, 0]) < 1.0 and v[0, 3] < 0.5


def test_out_of_bounds_ends_with_minus_100():
    for x, vx in ((W + 0.01, 0.0), (-0.01, 0.0), (W - 0.01, 2.0), (0.01, -2.0)):
        q, v = state(x, 10.0, 0.0, flat_terrain(), vx=vx)
        _, _, obs, rew, done, _, over = L.step(q, v, ZERO)
        assert done[0] and rew[0] == -100.0 and not over[0] and abs(obs[0, 0]) >= 1.0
    q, v = state(W - 0.5, 10.0, 0.0, flat_terrain())
    assert not L.step(q, v, ZERO)[4][0]


def test_one_foot_on_a_slope_is_pushed_along_the_normal():
    sy = L.terrain_from_heights(np.linspace(6.0, 0.5, 12)[None])            # falling to the right: the right foot hangs free
    seg = 1                                                            # x in [2, 4]
    t = np.array([2.0, sy[0, seg + 1] - sy[0, seg]]); t /= np.hypot(*t)
    n = np.array([-t[1], t[0]])
    x = 3.5
    # the left foot 1 mm inside the segment's line, the right one well above it
    foot = np.array(M["foot"][0])
    on_line = np.array([x, sy[0, seg] + (sy[0, seg + 1] - sy[0, seg]) * (x - 2.0) / 2.0])
    origin = on_line - 1e-3 * n - foot
    q, v = state(origin[0], origin[1], 0.0, sy)
    obs = L.observe(q, v)
    assert obs[0, 6] == 1.0 and obs[0, 7] == 0.0
    acc, gaps = L.contact_forces(q[:, 3:], q[:, :2] + np.array(M["com"]), q[:, 2], v[:, :2], v[:, 2])
    assert abs(gaps[0, 0] + 1e-3) < 1e-12 and gaps[0, 1] > 0.1
    f = acc[0, :2] * M["mass"]
    assert f @ n > 0.0 and abs(f @ t) <= M["friction"] * (f @ n) * (1 + 1e-12)       # inside the friction cone, pushing out


# ---------------------------------------------------------------------------------------------------- reward and reset
def test_shaping_telescopes_with_the_engines_off():
    rng = np.random.default_rng(3)
    n = 6
    sy = L.terrain_from_heights(rng.uniform(0, H / 2, (n, 12)))
    q = np.concatenate([np.stack([rng.uniform(6, 14, n), np.full(n, 11.0), rng.uniform(-0.3, 0.3, n)], 1), sy], 1)
    v = np.concatenate([rng.uniform(-1, 1, (n, 3)), np.zeros((n, 1))], 1)
    first = L.shaping(L.observe64(q, v))
    total = np.zeros(n)
    a = np.zeros((n, 2), np.float32); a[:, 1] = 0.4                    # inside the dead zone
    for _ in range(25):
        q, v, _, rew, done, _, _ = L.step(q, v, a)
        assert not done.any()
        total += rew
    np.testing.assert_allclose(total, L.shaping(L.observe64(q, v)) - first, rtol=0, atol=1e-10)


def test_reset_is_one_zero_action_step_from_the_stated_start():
    rng = np.random.default_rng(4)
    u = rng.random((5, 14))
    q, v = L.reset_from_draws(u)
    sy = L.terrain_from_heights((H / 2.0) * u[:, :12])
    assert np.array_equal(q[:, 3:], sy) and np.all(v[:, 3] == 0.0)
    q0 = np.concatenate([np.tile([W / 2.0, H, 0.0], (5, 1)), sy], 1)
    kick = (-1000.0 + 2000.0 * u[:, 12:14]) / FPS / M["mass"]         # the force over the first 1 / FPS
    v0 = np.concatenate([kick, np.zeros((5, 2))], 1)
    wq, wv = L.step(q0, v0, np.zeros((5, 2), np.float32))[:2]
    np.testing.assert_allclose(q, wq, rtol=0, atol=1e-13)
    np.testing.assert_allclose(v, wv, rtol=0, atol=1e-13)
    assert np.all(np.abs(q[:, 2]) == 0.0) and np.all(np.abs(v[:, 0]) <= 1000.0 / FPS / M["mass"])
    # the draws are the env's Philox stream: counter k is word k & 3 of block k >> 2
    d = lr.draws(5, 2, 7, np.arange(4), list(range(16)))
    assert d.shape == (4, 16) and np.all((d > 0.0) & (d < 1.0)) and len(np.unique(d)) == 64
    assert np.array_equal(lr.draws(5, 2, 7, [3], [14, 15]), d[3:4, 14:16])


def test_the_restatements_own_rollout_rarely_sits_on_a_switch():
    """The share of lane-steps within 1e-9 of a switch, on the restatement alone at the parity run's size and action distribution
    (70 envs, 120 steps, path limit 50, uniform actions and dispersion): measured 0 of 8400.  The GPU suite allows 0.5 %."""
    rng = np.random.default_rng(11)
    n = 70
    q, v = L.reset_from_draws(rng.random((n, 14)))
    length, close, total = np.zeros(n, int), 0, 0
    for _ in range(120):
        q, v, _, _, done, margin, _ = L.step(q, v, rng.uniform(-1, 1, (n, 2)).astype(np.float32), rng.random((n, 2)))
        close += int((margin <= 1e-9).sum()); total += n
        length += 1
        end = done | (length >= 50)
        if end.any():
            q[end], v[end] = L.reset_from_draws(rng.random((int(end.sum()), 14)))
            length[end] = 0
    print(f"{close} of {total} lane-steps within 1e-9 of a switch")
    assert close <= 0.005 * total


# ---------------------------------------------------------------------------------------------------- Python surface and spec
def test_envpool_name_and_spec():
    import yaml
    from ilswiss_amd.envs.envpool import _model_name
    assert _model_name("LunarLanderContinuous-v2") == "lunarlandercont"
    with pytest.raises(KeyError):
        _model_name("LunarLander-v2")                                  # the discrete task is not provided
    s = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "sac", "sac_lunar_hip.yaml")))
    c = s["constants"]
    assert s["meta_data"]["script_path"] == "run_scripts/sac_exp_script.py" and s["variables"]["seed"] == [723894]
    assert s["meta_data"]["exp_name"] == "test_sac_lunarlander" and c["net_size"] == 256 and c["num_hidden_layers"] == 2
    assert c["env_specs"] == dict(env_name="lunarlandercont", env_kwargs={}, env_num=8, training_env_seed=0, eval_env_seed=0)
    assert c["rl_alg_params"] == dict(num_epochs=101, num_steps_per_epoch=10000, num_steps_between_train_calls=1000,
                                      num_train_steps_per_train_call=1000, num_steps_per_eval=10000, max_path_length=1000,
                                      min_steps_before_training=0, eval_deterministic=True, batch_size=512, replay_buffer_size=1000000,
                                      no_terminal=False, wrap_absorbing=False, save_best=True, freq_saving=10, save_replay_buffer=False)
    assert c["sac_params"] == dict(alpha=0.2, reward_scale=1.0, discount=0.99, soft_target_tau=0.005, policy_lr=3e-4, qf_lr=3e-4,
                                   vf_lr=3e-4, policy_mean_reg_weight=1e-3, policy_std_reg_weight=1e-3)
    assert 1000 % c["env_specs"]["env_num"] == 0


def test_wrappers_and_bad_models_are_refused_before_the_library_is_entered():
    from ilswiss_amd.envs import HipVectorEnv
    from ilswiss_amd.envs.vecenv import lunar_struct
    nothing = object()                                                 # a context that must not be touched
    with pytest.raises(NotImplementedError):
        HipVectorEnv("lunarlandercont", 4, ctx=nothing, obs_shift=np.zeros(8), obs_scale=np.ones(8))
    bad = dict(M, hull_poly=M["hull_poly"][:5])
    with pytest.raises(ValueError, match="vertices"):
        HipVectorEnv("lunarlandercont", 4, ctx=nothing, model=bad)
    bad = dict(M, foot=[(-0.95, -0.2), (0.95, -0.2)])                  # above the hull's bottom at -1/3
    with pytest.raises(ValueError, match="foot"):
        HipVectorEnv("lunarlandercont", 4, ctx=nothing, model=bad)
    with pytest.raises(ValueError, match="foot"):
        lunar_struct(dict(M, foot=[(-0.95, -0.54)]))


# ---------------------------------------------------------------------------------------------------- compiled kernels
def test_new_kernels_compile_without_scratch_or_indexed_registers():
    import test_pendulum_cpu as tp
    if not os.path.exists(tp.HIPCC):
        pytest.skip("no hipcc")
    ks = tp._kernels(os.path.join(tp.CSRC, "ilsx_env.hip"))
    found = {}
    for sym, (ops, priv) in ks.items():
        dn = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        for k in ("k_lunar_step", "k_lunar_reset"):
            if dn.startswith(k + "("):
                found[k] = (ops, priv)
    assert sorted(found) == ["k_lunar_reset", "k_lunar_step"], sorted(found)
    for name, (ops, priv) in found.items():
        assert priv == 0 and not any(o.startswith("scratch_") for o in ops), (name, priv)      # no private segment: no VGPR spills
        assert not any(o.startswith("s_set_gpr_idx") or "movrel" in o for o in ops), name
        assert any(o.startswith("global_store") for o in ops), name
