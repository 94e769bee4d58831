"""CPU suite for DDPG: the torch restatement of one step and the numpy restatements of both exploration strategies
(tests/ddpg_restatement.py) against the reference's own vectors (tests/golden/g31_ddpg.npz, tools/make_golden.py `ddpg`), the
NotImplementedError surface of the trainer, the spec files, and the hard-update schedule.

Tolerances are those tests/test_hip_parity.py states for these quantities: losses and statistics rtol 2e-4 / atol 2e-6, parameters after
the chained steps 5e-5 absolute; every gradient vector within 1e-4 of ITS largest entry, no absolute floor (the project's gradient bound).  Strategy traces
are float64 in the reference's order: exact."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from ddpg_restatement import (CASES, GOLDEN, LOSS_KEYS, STAT_KEYS, DdpgRestatement, gaussian_trace, golden_cases,  # noqa: E402
                              ou_trace)

RTOL, ATOL, PTOL = 2e-4, 2e-6, 5e-5


@pytest.fixture(scope="module")
def cases():
    return golden_cases()


def _restatement(c):
    return DdpgRestatement(c["o"], c["a"], c["hidden"], c["pi0"], c["q0"], c["tanh_out"], **c["kw"])


@pytest.mark.parametrize("case", range(len(CASES)))
def test_restatement_matches_reference(cases, case):
    c = cases[case]
    r = _restatement(c)
    for s, b in enumerate(c["batches"]):
        out = r.train_step(b)
        assert np.allclose(out["losses"], c[f"s{s}_losses"], rtol=RTOL, atol=ATOL), (s, out["losses"], c[f"s{s}_losses"])
        for k in STAT_KEYS:
            assert np.allclose(out[k], c[f"s{s}_{k}"], rtol=RTOL, atol=ATOL), (s, k, out[k], c[f"s{s}_{k}"])
        if s == 0:
            for k, idx in (("grad_q", c["idx_q"]), ("grad_pi", c["idx_pi"])):
                ref = c[k]
                assert np.abs(out[k][idx] - ref).max() <= 1e-4 * np.abs(ref).max(), (k, np.abs(out[k][idx] - ref).max(), np.abs(ref).max())
        if case == 0:
            for k in ("pi", "q", "tpi", "tq"):
                assert np.abs(r.params(k) - c[f"s{s}_{k}"]).max() < PTOL, (s, k)
    for k, idx in (("pi", c["idx_pi"]), ("q", c["idx_q"]), ("tpi", c["idx_pi"]), ("tq", c["idx_q"])):
        assert np.abs(r.params(k)[idx] - c[k]).max() < PTOL, k


def test_golden_cases_reach_their_paths(cases):
    """What each case is there for, read off the reference's own numbers."""
    c0, c1, c2, _ = cases
    assert np.array_equal(c0["s0_tq"], c0["s0_q"]) and np.array_equal(c0["s2_tpi"], c0["s2_pi"])        # steps 0 and 2 hard-copy
    assert np.array_equal(c0["s1_tq"], c0["s0_q"]) and np.abs(c0["s1_tq"] - c0["s1_q"]).max() > 1e-3    # step 1 does not
    assert all(c1[f"s{s}_losses"][3] > 0 for s in range(3))                                              # the pre-activation penalty is on
    assert all(0.1 < float(c2[f"s{s}_clamp_frac"]) < 0.9 for s in range(3))                              # the clamp bites on some rows
    assert all(c2[f"s{s}_q_targets"][2] == np.float32(0.8) and c2[f"s{s}_q_targets"][3] == np.float32(-0.5) for s in range(3))


def test_hard_update_schedule():
    c = golden_cases()[0]
    r = DdpgRestatement(c["o"], c["a"], c["hidden"], c["pi0"], c["q0"], c["tanh_out"], **dict(c["kw"], target_update_period=2))
    for i in range(5):
        r.train_step(c["batches"][i % 3])
        same = np.array_equal(r.params("tq"), r.params("q")) and np.array_equal(r.params("tpi"), r.params("pi"))
        assert same == (i % 2 == 0), i
    assert r.copied == [0, 2, 4]


def test_strategy_traces_exact():
    g = np.load(GOLDEN)
    ts = [7 * k for k in range(40)]
    mu, theta, mx, mn, dp = g["ou_kw"]
    ou = ou_trace(g["ou_raw"], g["ou_eps"], ts, (13, 29), mu, theta, mx, mn, dp)
    assert ou.dtype == np.float64 and np.array_equal(ou, g["ou_out"])
    ga = gaussian_trace(g["ga_raw"], g["ga_eps"], ts, *g["ga_kw"])
    assert np.array_equal(ga, g["ga_out"])
    # without the resets the OU trace departs at call 13 and never before
    free = ou_trace(g["ou_raw"], g["ou_eps"], ts, (), mu, theta, mx, mn, dp)
    assert np.array_equal(free[:13], ou[:13]) and not np.array_equal(free[13], ou[13])
    for out in (g["ou_out"], g["ga_out"]):   # the clip fires on some entries, not on all
        assert 0 < (np.abs(out) == 1.0).sum() < out.size


class _Net:   # what DDPG.__init__ touches before it reaches the library
    ctx, h, max_act = None, None, 1.0


@pytest.mark.parametrize("kw", [dict(residual_gradient_weight=0.5), dict(obs_normalizer=object()), dict(action_normalizer=object()),
                                dict(num_paths_for_normalization=3), dict(epoch_discount_schedule=object()),
                                dict(eval_with_target_policy=True), dict(optimizer_class="SGD"), dict(qf_criterion="huber")])
def test_not_implemented_surface(kw):
    from ilswiss_amd.ddpg import DDPG
    with pytest.raises(NotImplementedError):
        DDPG(_Net(), _Net(), **kw)


def test_strategy_constructors_are_the_references():
    import inspect

    from ilswiss_amd.ddpg import DDPG, GaussianStrategy, OUStrategy
    from ilswiss_amd.envs.vecenv import Box
    d = {k: v.default for k, v in inspect.signature(OUStrategy.__init__).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(mu=0, theta=0.15, max_sigma=0.3, min_sigma=0.3, decay_period=100000)
    d = {k: v.default for k, v in inspect.signature(GaussianStrategy.__init__).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(max_sigma=1.0, min_sigma=None, decay_period=1000000)
    d = {k: v.default for k, v in inspect.signature(DDPG.__init__).parameters.items() if v.default is not inspect.Parameter.empty}
    assert (d["policy_lr"], d["qf_lr"], d["soft_target_tau"], d["use_soft_update"], d["target_update_period"]) == (1e-4, 1e-3, 1e-2, False, 1000)
    assert d["discount"] == 0.99 and d["min_q_value"] == -np.inf and d["max_q_value"] == np.inf
    cfg = GaussianStrategy(Box(-np.ones(3), np.ones(3)), max_sigma=0.4).cfg()
    assert (cfg.kind, cfg.max_sigma, cfg.min_sigma, cfg.low, cfg.high) == (1, 0.4, 0.4, -1.0, 1.0)
    with pytest.raises(NotImplementedError):
        OUStrategy(Box([-1.0, -2.0], [1.0, 2.0]))


@pytest.mark.parametrize("name", ["ddpg_hopper_hip.yaml", "ddpg_pendulum_hip.yaml"])
def test_spec_files(name):
    import yaml
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "ddpg", name)))
    cst = spec["constants"]
    assert os.path.isfile(os.path.join(ROOT, spec["meta_data"]["script_path"]))
    assert spec["meta_data"]["script_path"] == "run_scripts/ddpg_exp_script.py"
    from ilswiss_amd.envs import vecenv
    known = set(vecenv.CLASSIC) | {"hopper", "walker", "halfcheetah", "ant", "humanoid"}
    assert cst["env_specs"]["env_name"] in known
    assert cst["ddpg_params"]["use_soft_update"] is True
    assert cst["exploration"]["type"] in ("ou", "gaussian")
    for k in ("batch_size", "num_epochs", "max_path_length", "min_steps_before_training", "num_train_steps_per_train_call"):
        assert k in cst["rl_alg_params"], k


def test_struct_sizes_match_header(tmp_path):
    """The three structs this feature adds to the ABI: sizeof() as gcc lays include/ilsx.h out == the ctypes mirrors in _lib.py."""
    import ctypes
    import subprocess

    from ilswiss_amd import _lib
    pairs = dict(ilsx_ddpg_cfg="DdpgCfg", ilsx_ddpg_stats="DdpgStats", ilsx_explore_cfg="ExploreCfg")
    src = tmp_path / "sizes.c"
    body = "".join(f'  printf("{c} %zu\\n", sizeof({c}));\n' for c in pairs)
    src.write_text('#include <stdio.h>\n#include "ilsx.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    sizes = dict(zip(out[::2], map(int, out[1::2])))
    for c, py in pairs.items():
        assert ctypes.sizeof(getattr(_lib, py)) == sizes[c], (c, ctypes.sizeof(getattr(_lib, py)), sizes[c])
