"""Phase A of the single-run SAC step with the target critics on grid rows of their own (kernels.h PhaseAArgs::own_rows: rows y = 5 / 6
request their weights at entry, wait for the tile's policy slices, run the one stage; the policy rows return after their arrival).
The mapping moves a stage to other workgroups and nothing else — same stage text, same operands, same summation order — so every result must
equal, bit for bit, the one-launch-per-stage path (ILSX_NO_PHASE=1) and the mapping it replaces (ILSX_PHASE_OWN_ROWS=0), at the shapes where
a mapping can go wrong: a second tile with one row, padding tiles in the first and in the second round of eight, one full tile of the
2-slice instance.  The no-GPU test holds the register budget that two workgroups per CU (what the extra rows' residency rests on) need."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SAC_KW = dict(reward_scale=1.0, discount=0.99, policy_lr=3e-4, qf_lr=3e-4, alpha_lr=3e-4, soft_target_tau=0.005,
              alpha=0.2, train_alpha=True, policy_mean_reg_weight=1e-3, policy_std_reg_weight=1e-3, beta_1=0.9)
_SWITCHES = ("ILSX_NO_PHASE", "ILSX_PHASE_OWN_ROWS")


@functools.lru_cache(maxsize=None)
def _run(o, a, H, B, n_steps, mode):
    """One agent through three train calls (a window, a call boundary, a window that ends with statistics) under `mode`:
    'own' (default), 'old' (ILSX_PHASE_OWN_ROWS=0) or 'stages' (ILSX_NO_PHASE=1).  Computed once per shape and mode, shared by the tests."""
    import ilswiss_amd as ia
    from oracle import mlp as omlp
    hidden, N = [H, H], 6000
    rng = np.random.default_rng(o + H + B)
    params = (omlp.init_mlp(rng, o, hidden, a, init_w=1e-3, n_heads=2), omlp.init_mlp(rng, o + a, hidden, 1), omlp.init_mlp(rng, o + a, hidden, 1))
    data = (rng.normal(0, 1, (N, o)).astype(np.float32), np.tanh(rng.normal(0, 1, (N, a))).astype(np.float32),
            rng.normal(0, 1, N).astype(np.float32), (rng.random(N) < 0.05).astype(np.uint8), rng.normal(0, 1, (N, o)).astype(np.float32))
    saved = {k: os.environ.pop(k, None) for k in _SWITCHES}
    if mode == "stages":
        os.environ["ILSX_NO_PHASE"] = "1"
    elif mode == "old":
        os.environ["ILSX_PHASE_OWN_ROWS"] = "0"
    try:
        ctx = ia.Context(0, seed=2024)
        rb = ia.SimpleReplayBuffer(8192, o, a, random_seed=5, ctx=ctx)
        rb.add_rows(*data)
        pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden, o, a, ctx=ctx)
        q1, q2 = ia.FlattenMlp(hidden, 1, o + a, ctx=ctx), ia.FlattenMlp(hidden, 1, o + a, ctx=ctx)
        pol.set_flat_params(params[0]), q1.set_flat_params(params[1]), q2.set_flat_params(params[2])
        tr = ia.SoftActorCritic(pol, q1, q2, max_batch=B, **SAC_KW)
        tr.eval_statistics = {}
        tr.train_from_replay(rb, n_steps, B)
        tr.train_from_replay(rb, 1, B)             # call boundary: pending tail flushed and re-armed
        tr.eval_statistics = None
        tr.train_from_replay(rb, 2, B)             # statistics of the last step
        out = (tr.get_snapshot(), dict(tr.get_eval_statistics()), tr.rng_step, tr.phase_state())
        ctx.close()
        return out
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _assert_same(r0, r1, n_steps):
    (s0, st0, c0, _), (s1, st1, c1, _) = r0, r1
    assert c0 == c1 == n_steps + 3
    for k in ("policy", "qf1", "qf2", "target_qf1", "target_qf2"):
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=k)
    assert s0["log_alpha"] == s1["log_alpha"]
    for k in ("policy_optimizer", "qf1_optimizer", "qf2_optimizer"):
        np.testing.assert_array_equal(s0[k]["exp_avg"], s1[k]["exp_avg"], err_msg=k)
        np.testing.assert_array_equal(s0[k]["exp_avg_sq"], s1[k]["exp_avg_sq"], err_msg=k)
    assert set(st0) == set(st1)
    for k, v in st0.items():
        assert v == st1[k] or (np.isnan(v) and np.isnan(st1[k])), (k, v, st1[k])


@pytest.mark.gpu
@pytest.mark.parametrize("o,a,H,B,n_steps", [(11, 3, 256, 17, 3),     # two tiles, the second with one row, six padding tiles
                                             (17, 6, 128, 16, 3),     # one full tile, the 2-slice instance
                                             (11, 3, 256, 129, 2)])   # nine tiles, padding in the second round of eight
def test_own_rows_are_bitwise_the_one_launch_per_stage_path(o, a, H, B, n_steps):
    own, stages = _run(o, a, H, B, n_steps, "own"), _run(o, a, H, B, n_steps, "stages")
    assert own[3]["last_window_on_phase"] and own[3]["fallbacks"] == 0 and not stages[3]["last_window_on_phase"], (own[3], stages[3])
    _assert_same(own, stages, n_steps)


@pytest.mark.gpu
@pytest.mark.parametrize("o,a,H,B,n_steps", [(11, 3, 256, 256, 3), (17, 6, 128, 37, 3)])
def test_own_rows_are_bitwise_the_mapping_they_replace(o, a, H, B, n_steps):
    own, old = _run(o, a, H, B, n_steps, "own"), _run(o, a, H, B, n_steps, "old")
    for r in (own, old):
        assert r[3]["last_window_on_phase"] and r[3]["fallbacks"] == 0, r[3]
    _assert_same(own, old, n_steps)


@pytest.mark.gpu
def test_default_batch_stays_on_the_phase_path_with_two_workgroups_per_cu():
    """B = 256 / H = 256 with the extra rows: 16 tiles x 6 working rows x 4 slices + the tail workgroup = 385 workgroups that wait for each
    other, resident only at two per CU."""
    ps = _run(11, 3, 256, 256, 3, "own")[3]
    assert ps["last_window_on_phase"] and not ps["disabled"] and ps["fallbacks"] == 0, ps
    assert ps["wgs_per_cu_a"] >= 2, ps


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_phase_a_constant_table_instances_fit_two_workgroups_per_cu():
    """No GPU: the translation unit compiled device-only to assembly (as tools/kernel_static.py does).  Two 16-wave workgroups per CU are two
    waves per SIMD: 512 registers / 2 = 256 per wave, vector registers allocated in blocks of 8, accumulation registers on top, and no
    private segment (scratch is not what the occupancy figure counts, but it is what a kernel pushed over the budget gets)."""
    out = os.path.join(tempfile.mkdtemp(prefix="isa_phase_"), "core.s")
    try:
        r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "ilswiss_amd", "csrc", "ilsx_core.hip"), "-o", out], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out).read().split("\n")
        starts = [(i, m.group(1)) for i, l in enumerate(text) for m in [re.match(r"^(_Z\w+):\s", l)] if m]
        seen = set()
        for i, name in starts:
            dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            m = re.match(r"void k_sac_phase_a<(\d+), [^,]+, (\d+), true>", dn)
            if not m:
                continue
            end = next(j for j in range(i, len(text)) if text[j].startswith(".Lfunc_end"))
            meta = "\n".join(text[end:end + 150])
            priv = int(re.search(r"\.private_seg_size, (\d+)", meta).group(1))
            vgpr, agpr = int(re.search(r"\.num_vgpr, (\d+)", meta).group(1)), int(re.search(r"\.num_agpr, (\d+)", meta).group(1))
            print(dn, "vgpr", vgpr, "agpr", agpr, "private", priv)
            assert priv == 0, (dn, priv)
            assert (vgpr + 7) // 8 * 8 + agpr <= 256, (dn, vgpr, agpr)
            seen.add((int(m.group(1)), int(m.group(2))))
        assert {(256, 4), (128, 2)} <= seen, seen   # ReLU and tanh instances of both widths are all checked; both widths must be there
    finally:
        shutil.rmtree(os.path.dirname(out), ignore_errors=True)
