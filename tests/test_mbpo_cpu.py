"""CPU suite of MBPO (ilswiss_amd/mbpo.py, ilswiss_amd/csrc/bnn.h): schedule and buffer arithmetic of mbpo.py:170-232, the
reference's _save_state / _set_state alias behaviour, the restatement's init rule, the three specs, and the new kernels' resource
usage (gfx950 cross-compile: no scratch)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import yaml

import mbpo_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollout_length_schedule():
    from ilswiss_amd.mbpo import rollout_length_at
    s = [20, 150, 1, 15]
    assert [rollout_length_at(s, e) for e in (0, 19, 20, 21, 85, 149, 150, 300)] == [1, 1, 1, 1, 8, 14, 15, 15]
    assert all(rollout_length_at([20, 150, 1, 1], e) == 1 for e in range(0, 301, 7))


def test_model_pool_growth_and_batch_split():
    from ilswiss_amd.mbpo import batch_split, model_pool_size
    # model_retrain_epochs * int(rollout_length * rollout_batch_size * max_path_length / model_train_freq)
    assert model_pool_size(1, 1, 100000, 1000, 250) == 400000
    assert model_pool_size(1, 15, 100000, 1000, 250) == 6000000
    assert model_pool_size(2, 3, 2000, 200, 150) == 2 * int(3 * 2000 * 200 / 150)
    assert batch_split(256, 0.05, 0) == (256, 0)          # model ring empty: all real rows
    assert batch_split(256, 0.05, 1) == (12, 244)         # int(256 * 0.05) real rows, the rest from the model ring
    assert batch_split(256, 1.0, 10) == (256, 0)


def test_default_weight_decays():
    from ilswiss_amd.mbpo import default_weight_decays
    assert default_weight_decays(4) == [2.5e-5, 5e-5, 7.5e-5, 7.5e-5, 1e-4]
    assert default_weight_decays(2) == [2.5e-5, 1e-4]


def test_reference_save_state_stores_aliases():
    """bnn_trainer.py:243-253 stores `fc.weight.data`, which shares storage with the parameter: after further optimiser steps the
    "saved" state IS the live state, so _set_state restores nothing.  Shown on a torch layer with the reference's statements."""
    w = torch.nn.Parameter(torch.ones(2, 3, 4))
    opt = torch.optim.Adam([w], lr=0.1)
    saved = {"weight": w.data}                 # _save_state
    (w ** 2).sum().backward()
    opt.step()
    assert torch.equal(saved["weight"], w.data) and not torch.equal(saved["weight"], torch.ones(2, 3, 4))
    before = w.data.clone()
    w.data.copy_(saved["weight"])              # load_state_dict of the aliases in _set_state
    assert torch.equal(w.data, before)


def test_trainer_set_state_is_a_no_op_and_needs_every_member():
    from ilswiss_amd.mbpo import BNNTrainer
    tr = BNNTrainer.__new__(BNNTrainer)
    tr.bnn = type("B", (), {"num_nets": 3})()
    tr._state, tr._snapshots, tr._epochs_since_update, tr.max_epochs_since_update = {}, {i: (None, 1e10) for i in range(3)}, 0, 5
    assert tr._save_best(0, np.array([1.0, 2.0, 3.0])) is False and sorted(tr._state) == [0, 1, 2]
    tr._set_state()
    assert tr._save_best(1, np.array([0.995, 1.0, 3.0])) is False   # 0.5 % is no improvement, 50 % is
    assert tr._snapshots[0] == (0, 1.0) and tr._snapshots[1] == (1, 1.0) and tr._epochs_since_update == 0
    for e in range(2, 8):
        stop = tr._save_best(e, np.array([1.0, 1.0, 3.0]))
    assert stop and tr._epochs_since_update == 6
    tr._state.pop(2)
    with pytest.raises(KeyError):
        tr._set_state()


def test_restatement_init_rule_bounds():
    ps = R.init_params(np.random.default_rng(0), 7, 14, [200] * 4, 12)
    assert [p.shape for p in ps] == R.shapes(7, 14, [200] * 4, 12)
    assert np.abs(ps[0]).max() <= 1 / np.sqrt(14 * 200) and np.abs(ps[2]).max() <= 1 / np.sqrt(200 * 200)
    assert np.all(ps[1] == np.float32(0.1)) and np.abs(ps[-2]).max() <= 3e-3


def test_restatement_loss_gradient_matches_autograd_head_formula():
    """the kernel's head gradient: d/dmu = 2 (mu - t) e^-lv / (E B D), d/dlv = (1 - (mu - t)^2 e^-lv) / (E B D), through both softplus"""
    torch.manual_seed(0)
    E, B, D = 2, 5, 3
    mu = torch.randn(E, B, D, requires_grad=True)
    raw = torch.randn(E, B, D, requires_grad=True) * 3
    raw.retain_grad()
    t = torch.randn(E, B, D)
    F = torch.nn.functional
    lv1 = 0.5 - F.softplus(0.5 - raw)
    lv = -10.0 + F.softplus(lv1 + 10.0)
    loss = torch.mean(torch.mean((mu - t) ** 2 * torch.exp(-lv), dim=[-2, -1]) + torch.mean(lv, dim=[-2, -1]))
    loss.backward()
    s = 1.0 / (E * B * D)
    with torch.no_grad():
        inv = torch.exp(-lv)
        gmu = s * 2 * (mu - t) * inv
        graw = s * (1 - (mu - t) ** 2 * inv) * torch.sigmoid(lv1 + 10.0) * torch.sigmoid(0.5 - raw)
    assert torch.allclose(mu.grad, gmu, atol=1e-7) and torch.allclose(raw.grad, graw, atol=1e-7)


@pytest.mark.parametrize("task", ["hopper", "walker", "halfcheetah"])
def test_specs_parse_through_the_run_script(task):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "run_scripts"))
    import mbpo_exp_script as ms
    from _common import flatten_spec
    spec = yaml.safe_load(open(os.path.join(ROOT, "exp_specs", "mbpo", f"mbpo_{task}_hip.yaml")))
    v = flatten_spec(spec)
    assert v["env_specs"]["env_name"] in ms.TERMINALS and spec["meta_data"]["script_path"] == "run_scripts/mbpo_exp_script.py"
    assert v["bnn_params"]["num_nets"] == 7 and v["bnn_params"]["net_size"] == 200 and v["bnn_params"]["num_hidden_layers"] == 4
    assert v["mbpo_params"]["model_train_freq"] == 250 and v["mbpo_params"]["rollout_batch_size"] == 100000
    from ilswiss_amd.envs.terminals import get_terminal_func
    assert get_terminal_func(ms.TERMINALS[v["env_specs"]["env_name"]]) is not None


def test_bnn_kernels_use_no_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage on ilsx_bnn.hip (gfx950): every new kernel reports ScratchSize 0, and the H = 208 forward
    keeps 8 waves per SIMD."""
    src = os.path.join(ROOT, "ilswiss_amd", "csrc", "ilsx_bnn.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "bnn.o")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(occ) >= 7, names
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
    for n_, o_ in zip(names, occ):
        if "k_bnn_fwd" in n_:
            assert o_ >= 8, (n_, o_)
    assert any("k_bnn_dw_adam" in n_ for n_ in names) and any("k_mbpo_sample" in n_ for n_ in names)
