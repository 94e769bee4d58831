"""CPU suite for DQN / Double DQN: the numpy restatement of both steps (tests/dqn_restatement.py) against the reference's own
_do_training methods (tests/golden/g32_dqn.npz), what the fixture promises about its own inputs, and the surface that needs no GPU (ctypes
structs and prototypes, constructor defaults, the three specs, the run script's refusals)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from dqn_restatement import DqnRestatement, forward, golden_cases, unflatten  # noqa: E402

G32 = os.path.join(HERE, "golden", "g32_dqn.npz")
SPECS = ("dqn_cartpole_hip.yaml", "dqn_mountaincar_hip.yaml", "ddqn_acrobot_hip.yaml")


@pytest.fixture(scope="module")
def cases():
    return golden_cases(G32)


def _restate(c, **kw):
    return DqnRestatement(c["o"], [c["H"]] * 2, c["n"], c["q0"], c["tq0"], c["double_q"], **dict(c["kw"], **kw))


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_restatement_matches_reference_step(cases, case):
    c = cases[case]
    r = _restate(c)
    idx = c["idx"]
    for s, b in enumerate(c["batches"]):
        out = r.train_step(b)
        want = float(c[f"s{s}_qf_loss"])
        assert abs(out["qf_loss"] - want) <= 1e-5 * max(1.0, abs(want)), s
        p = out["y_pred"]
        assert np.allclose([p.mean(), p.std(), p.max(), p.min()], c[f"s{s}_y_pred"], atol=1e-5), s
        if s == 0:
            assert np.abs(out["grad"][idx] - c["grad_q"]).max() <= 1e-6
    for k in ("q", "tq"):
        assert np.abs(r.params(k)[idx] - c[k]).max() <= 1e-6, k
    assert r.copied == ([0, 2] if c["hard"] else [])


@pytest.mark.parametrize("case", [1, 3])
def test_wrong_target_rule_misses_the_golden(cases, case):
    """A DQN target on a Double DQN case is off by far more than any tolerance used on it: the fixture tells the two rules apart."""
    c = cases[case]
    r = DqnRestatement(c["o"], [c["H"]] * 2, c["n"], c["q0"], c["tq0"], False, **c["kw"])
    out = r.train_step(c["batches"][0])
    assert abs(out["qf_loss"] - float(c["s0_qf_loss"])) > 1e-2
    assert np.abs(out["grad"][c["idx"]] - c["grad_q"]).max() > 1e-3 * np.abs(c["grad_q"]).max()


def test_hard_update_schedule_shows_in_the_golden(cases):
    """c2 with the copy one step late (counter tested after its increment) or with soft updates ends on another target net."""
    c = cases[2]
    for kw in (dict(use_hard_updates=False), dict(hard_update_period=3)):
        r = _restate(c, **kw)
        for b in c["batches"]:
            r.train_step(b)
        assert np.abs(r.params("tq")[c["idx"]] - c["tq"]).max() > 1e-4, kw


def test_fixture_inputs_keep_their_promises(cases):
    for c in cases:
        assert not np.array_equal(c["q0"], c["tq0"])                         # the target net has a vector of its own
        dims = [c["o"], c["H"], c["H"], c["n"]]
        q, tq = unflatten(c["q0"], dims, np.float64), unflatten(c["tq0"], dims, np.float64)
        z = forward(q, c["am_obs"].astype(np.float64))[0]
        top = np.sort(z, 1)
        assert (top[:, -1] - top[:, -2]).min() > 1e-3 and np.array_equal(z.argmax(1), c["argmax"])
        b0 = c["batches"][0]
        for net in (q, tq):                                                   # step 0's max / argmax inputs, from the initial vectors
            top = np.sort(forward(net, b0["next_observations"].astype(np.float64))[0], 1)
            assert (top[:, -1] - top[:, -2]).min() > 1e-3
        for b in c["batches"]:
            assert set(np.unique(b["terminals"])) == {0.0, 1.0}
            a = b["actions"]
            assert a.shape == (c["B"], 1) and np.array_equal(a, np.floor(a)) and a.min() >= 0 and a.max() < c["n"]
        if c["double_q"]:   # soft targets: every batch; hard targets: the batch before the first copy (after it the nets coincide)
            d = c["argmax_differ"]
            assert (d[:1] if c["hard"] else d).min() >= 0.25


def test_ctypes_surface():
    import ctypes as C

    from ilswiss_amd import _lib
    assert [f[0] for f in _lib.DqnCfg._fields_] == ["discount", "learning_rate", "tau", "use_hard_updates", "hard_update_period", "double_q",
                                                    "max_batch"]
    assert C.sizeof(_lib.DqnCfg) == 28 and C.sizeof(_lib.DqnStats) == 20
    for name in ("ilsx_net_set_epsilon_greedy", "ilsx_dqn_create", "ilsx_dqn_destroy", "ilsx_dqn_train_step", "ilsx_dqn_train_from_replay",
                 "ilsx_dqn_get_params", "ilsx_dqn_set_params", "ilsx_dqn_get_opt", "ilsx_dqn_set_opt"):
        assert name in _lib.PROTOTYPES, name
    assert _lib.PROTOTYPES["ilsx_net_set_epsilon_greedy"][1][2] is C.c_float


def test_struct_sizes_match_header(tmp_path):
    import ctypes

    from ilswiss_amd import _lib
    pairs = dict(ilsx_dqn_cfg="DqnCfg", ilsx_dqn_stats="DqnStats")
    src = tmp_path / "sizes.c"
    body = "".join(f'  printf("{c} %zu\\n", sizeof({c}));\n' for c in pairs)
    src.write_text('#include <stdio.h>\n#include "ilsx.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    sizes = dict(zip(out[::2], map(int, out[1::2])))
    for c, py in pairs.items():
        assert ctypes.sizeof(getattr(_lib, py)) == sizes[c], c


def test_constructor_is_the_references():
    import inspect

    import ilswiss_amd as ia
    d = {k: v.default for k, v in inspect.signature(ia.DQN.__init__).parameters.items() if v.default is not inspect.Parameter.empty}
    assert (d["learning_rate"], d["use_hard_updates"], d["hard_update_period"], d["tau"], d["epsilon"]) == (1e-3, False, 1000, 0.001, 0.1)
    assert d["discount"] == 0.99 and d["qf_criterion"] is None
    assert issubclass(ia.DoubleDQN, ia.DQN) and ia.DoubleDQN.DOUBLE_Q and not ia.DQN.DOUBLE_Q
    assert ia.DQN.SNAPSHOT_KEYS == ("qf", "target_qf") and ia.DQN.OPT == (("qf", 0),)

    class Net:
        ctx = h = None
    for kw in (dict(qf_criterion="huber"), dict(optimizer_class="SGD")):
        with pytest.raises(NotImplementedError):
            ia.DQN(Net(), policy=object(), **kw)


@pytest.mark.parametrize("name", SPECS)
def test_spec_files(name):
    import yaml
    path = os.path.join(ROOT, "exp_specs", "dqn", name)
    spec = yaml.safe_load(open(path))
    cst = spec["constants"]
    assert spec["meta_data"]["script_path"] == "run_scripts/dqn_exp_script.py" and os.path.isfile(os.path.join(ROOT, spec["meta_data"]["script_path"]))
    assert cst["double_dqn"] is name.startswith("ddqn")
    assert cst["dqn_params"] == dict(learning_rate=1e-3, use_hard_updates=False, hard_update_period=1000, tau=0.001, epsilon=0.1)
    task = cst["env_specs"]["env_name"]
    sac = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "sac", f"sac_{task}_d_hip.yaml")))
    assert cst["rl_alg_params"] == sac["constants"]["rl_alg_params"]          # the loop is the discrete-SAC spec's of the same task
    assert "no DQN spec" in open(path).read()


def test_run_script_refusals(tmp_path):
    import yaml
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "dqn", "dqn_cartpole_hip.yaml")))
    split = yaml.safe_load(yaml.safe_dump(spec))
    split["constants"]["rl_alg_params"]["split_ranks"] = 2
    (tmp_path / "split.yaml").write_text(yaml.safe_dump(split))
    script = os.path.join(ROOT, "run_scripts", "dqn_exp_script.py")
    for extra, why in ((["-e", "a.yaml", "b.yaml"], "--group"), (["-e", "split.yaml"], "split_ranks")):
        r = subprocess.run([sys.executable, script] + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and why in (r.stdout + r.stderr), r.stdout + r.stderr


def test_run_script_refuses_a_box_action_space(monkeypatch):
    """The action space is the library's to tell (it needs a device), so experiment() is called on stand-ins for the context and the envs."""
    import yaml
    sys.path.insert(0, os.path.join(ROOT, "run_scripts"))
    import dqn_exp_script as script
    from ilswiss_amd.envs.vecenv import Box

    class Env:
        obs_dim, action_space = 3, Box(-np.ones(1), np.ones(1))
    monkeypatch.setattr(script, "start", lambda variant, gpu: None)
    monkeypatch.setattr(script, "make_envs", lambda variant, ctx: (Env(), Env(), Env()))
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "dqn", "dqn_cartpole_hip.yaml")))
    variant = script.flatten_spec(spec)
    with pytest.raises(SystemExit, match="Discrete action space"):
        script.experiment(variant)
