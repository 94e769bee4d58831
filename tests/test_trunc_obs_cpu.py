"""CPU suite of the truncated-observation 3-D tasks (ant_trunc_obs, humanoid_trunc_obs: the MBPO tasks whose observation is
qpos[2:] | qvel): the model table, the C struct's flag, the DEVICE observation code of env3d.h / env3d_wave.h compiled for the host by
tests/harness/env3d_host.cpp (the truncated model against the full one, bit for bit), the terminal predicates and the two MBPO specs."""
import ast
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import yaml

from ilswiss_amd.envs.models3d import MODELS3D
from ilswiss_amd.envs.vecenv import spatial_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE_FLAGS = {"wave-ascending": 0, "wave-descending": 1, "wave-static-ascending": 2, "wave-static-descending": 3}
FORMS = ["lane"] + list(WAVE_FLAGS)
PAIRS = {"ant": ("ant_trunc_obs", 27), "humanoid": ("humanoid_trunc_obs", 45)}
FULL_MAX = 376   # the widest full observation (Humanoid)


def test_models3d_has_the_truncated_tasks():
    for full, (name, dim) in PAIRS.items():
        assert name in MODELS3D
        m, f = MODELS3D[name](), MODELS3D[full]()
        assert m["obs_dim"] == dim == (m["nq"] - 2) + m["nv"] and m["obs_trunc"] == 1
        assert not f.get("obs_trunc", 0) and f["obs_dim"] > dim
        for k in f:   # the same model otherwise
            if k not in ("obs_dim", "obs_trunc"):
                assert np.array_equal(np.asarray(m[k], dtype=object), np.asarray(f[k], dtype=object)), k


def test_spatial_struct_carries_the_flag():
    for full, (name, _) in PAIRS.items():
        assert spatial_struct(MODELS3D[name]()).obs_trunc == 1
        assert spatial_struct(MODELS3D[full]()).obs_trunc == 0
    assert C.sizeof(spatial_struct(MODELS3D["ant"]())) % 8 == 0


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(tempfile.mkdtemp(prefix="e3h_trunc_"), "libe3h.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "harness", "env3d_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.e3h_step.restype = C.c_int
    lib.e3hw_step.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _step(harness, form, sm, q, v, act):
    """one step from (q, v) into a NaN-prefilled FULL_MAX-wide buffer: (obs buffer, reward, done, q', v')"""
    q, v = q.copy(), v.copy()
    obs, r, d = np.full(FULL_MAX, np.nan), C.c_double(), C.c_int()
    if form == "lane":
        rc = harness.e3h_step(C.byref(sm), _p(q), _p(v), _p(act), _p(obs), C.byref(r), C.byref(d))
    else:
        rc = harness.e3hw_step(C.byref(sm), WAVE_FLAGS[form], _p(q), _p(v), _p(act), _p(obs), C.byref(r), C.byref(d))
    assert rc == 0
    return obs, r.value, d.value, q, v


def _states(m, rng):
    """standing (near init_qpos), low (limbs spread, in or near contact) and one terminal (root far above z_max)"""
    out = []
    for kind in ("standing", "low", "terminal"):
        q = np.asarray(m["init_qpos"], float).copy()
        if kind == "standing":
            q[7:] += rng.uniform(-0.05, 0.05, m["nq"] - 7)
            v = rng.normal(0, 0.1, m["nv"])
        else:
            q[2] += rng.uniform(-0.3, -0.1) if kind == "low" else 3.0
            q[3:7] += rng.normal(0, 0.3, 4)
            q[3:7] /= np.linalg.norm(q[3:7])
            q[7:] += rng.uniform(-0.8, 0.8, m["nq"] - 7)
            v = rng.normal(0, 1.5, m["nv"])
        out.append((kind, q, v))
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("full", list(PAIRS))
def test_truncated_step_is_the_prefix_of_the_full_step(harness, full, form):
    name, dim = PAIRS[full]
    mt, mf = MODELS3D[name](), MODELS3D[full]()
    st, sf = spatial_struct(mt), spatial_struct(mf)
    assert harness.e3h_obs_dim(C.byref(st)) == dim
    assert harness.e3h_obs_dim(C.byref(sf)) == mf["obs_dim"]
    rng = np.random.default_rng(17)
    for kind, q, v in _states(mf, rng):
        act = rng.uniform(-1.3, 1.3, mf["act_dim"]).astype(np.float32)
        ot, rt, dt, qt, vt = _step(harness, form, st, q, v, act)
        of, rf, df, qf, vf = _step(harness, form, sf, q, v, act)
        assert np.array_equal(qt, qf) and np.array_equal(vt, vf), kind
        assert not np.isnan(of[:mf["obs_dim"]]).any()
        assert np.array_equal(ot[:dim], of[:dim]), kind                       # bit-equal prefix
        assert np.array_equal(ot[:dim], np.r_[qt[2:], vt]), kind              # and it is qpos[2:] | qvel
        assert np.isnan(ot[dim:]).all(), kind                                 # nothing written past the truncated width
        assert rt == rf and dt == df, kind
        assert bool(dt) == (kind == "terminal"), (kind, dt)


def test_terminal_funcs_resolve():
    from ilswiss_amd.envs.terminals import get_terminal_func
    for n in ("ant", "humanoid"):
        assert callable(get_terminal_func(n))


def _script_terminals():
    """the TERMINALS table of run_scripts/mbpo_exp_script.py, read from its source (importing the script loads the device library)"""
    src = open(os.path.join(ROOT, "run_scripts", "mbpo_exp_script.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "TERMINALS" for t in node.targets):
            assert isinstance(node.value, ast.Call) and node.value.func.id == "dict"
            return {k.arg: ast.literal_eval(k.value) for k in node.value.keywords}
    raise AssertionError("no TERMINALS table")


@pytest.mark.parametrize("task,width", [("ant", 200), ("humanoid", 400)])
def test_specs_parse_and_name_an_accepted_env(task, width):
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "mbpo", f"mbpo_{task}_hip.yaml")))
    c = spec["constants"]
    name = c["env_specs"]["env_name"]
    table = _script_terminals()
    assert name == f"{task}_trunc_obs" and table[name] == task and name in MODELS3D
    assert "ant" not in table and "humanoid" not in table        # the full-observation tasks stay refused
    assert c["bnn_params"]["net_size"] == width and c["bnn_params"]["num_nets"] == 7
    assert spec["meta_data"]["script_path"] == "run_scripts/mbpo_exp_script.py"
