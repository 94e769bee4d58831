"""The static heads of the merged phase kernels (bwd_split_tile.inc / fwd_split_tile.inc): each backward stage's loss kind is a compile-time
constant of the stage, the descriptor fields a head needs are read ahead of the stage's wait and held in scalar registers, and every operand
and sub-expression that does not depend on the awaited stage is loaded / evaluated before the wait (the noise of pi(s') and the staging
indices of the target critics; reward, done, own q and alpha of the critics' backward, which now waits for the deferred tail BEFORE the
target critics' hand-off; everything of the policy's loss head but the critics' dQ/da).  The library is built with -ffp-contract=off and
every expression keeps its association, so the phase path must still equal the one-launch-per-stage path bit for bit — with a trained
alpha, so that an alpha read too early would show.

The no-GPU test compiles the phase kernels to assembly and holds, per post-wait window (tools/kernel_static.py head_windows: from a
stage's last poll loop to the next v_mfma), the scalar loads and `s_waitcnt lgkmcnt` against a quarter of what the commit before this
change had there (tests/golden/phase_head_counts_parent.json, the same scan on that commit).

Measured on this tree, H = 256 constant-table instances (parent -> now), s_load / lgkmcnt waits per window:
    phase A critics' backward 112 / 117 -> 2 / 20      phase A target critics 44 / 46 -> 6 / 10
    phase C critics' backward 113 / 120 -> 0 / 16      phase C policy backward 112 / 121 -> 2 / 13"""
import functools
import importlib.util
import json
import os
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
LOSS_SAC_CRITIC, LOSS_SAC_ACTORQ, LOSS_SAC_POLICY, LOSS_MSE = 1, 2, 3, 4   # kernels.h
HEAD_TANH_SAMPLE, HEAD_TANH_DET = 1, 2


def _setup(ia, o, a, H, B):
    from oracle import mlp as omlp
    hidden, N = [H, H], 6000
    rng = np.random.default_rng(o + H + B)
    params = (omlp.init_mlp(rng, o, hidden, a, init_w=1e-3, n_heads=2), omlp.init_mlp(rng, o + a, hidden, 1), omlp.init_mlp(rng, o + a, hidden, 1))
    data = (rng.normal(0, 1, (N, o)).astype(np.float32), np.tanh(rng.normal(0, 1, (N, a))).astype(np.float32),
            rng.normal(0, 1, N).astype(np.float32), (rng.random(N) < 0.05).astype(np.uint8), rng.normal(0, 1, (N, o)).astype(np.float32))
    ctx = ia.Context(0, seed=2024)
    rb = ia.SimpleReplayBuffer(8192, o, a, random_seed=5, ctx=ctx)
    rb.add_rows(*data)
    pol = ia.ReparamTanhMultivariateGaussianPolicy(hidden, o, a, ctx=ctx)
    q1, q2 = ia.FlattenMlp(hidden, 1, o + a, ctx=ctx), ia.FlattenMlp(hidden, 1, o + a, ctx=ctx)
    pol.set_flat_params(params[0]), q1.set_flat_params(params[1]), q2.set_flat_params(params[2])
    tr = ia.SoftActorCritic(pol, q1, q2, max_batch=B, **SAC_KW)
    return ctx, rb, tr, data


@functools.lru_cache(maxsize=None)
def _run(o, a, H, B, n_steps, mode, explicit=False):
    """One agent through three train calls (a window, a call boundary, a window that ends with statistics) under `mode`: 'phase' (default
    path), 'old' (ILSX_PHASE_OWN_ROWS=0) or 'stages' (ILSX_NO_PHASE=1).  explicit: two steps on a host batch with explicit noise instead.
    Computed once per case, shared by the tests."""
    import ilswiss_amd as ia
    saved = {k: os.environ.pop(k, None) for k in _SWITCHES}
    if mode == "stages":
        os.environ["ILSX_NO_PHASE"] = "1"
    elif mode == "old":
        os.environ["ILSX_PHASE_OWN_ROWS"] = "0"
    try:
        ctx, rb, tr, data = _setup(ia, o, a, H, B)
        tr.eval_statistics = {}
        if explicit:
            rng = np.random.default_rng(7)
            for k in range(2):
                idx = rng.integers(0, data[0].shape[0], B)
                batch = dict(observations=data[0][idx], actions=data[1][idx], rewards=data[2][idx][:, None],
                             terminals=data[3][idx].astype(np.float32)[:, None], next_observations=data[4][idx])
                tr.train_step(batch, rng.normal(0, 1, (B, a)).astype(np.float32), rng.normal(0, 1, (B, a)).astype(np.float32))
            n_done = 2
        else:
            tr.train_from_replay(rb, n_steps, B)
            tr.train_from_replay(rb, 1, B)             # call boundary: pending tail flushed and re-armed
            tr.eval_statistics = None
            tr.train_from_replay(rb, 2, B)             # statistics of the last step
            n_done = n_steps + 3
        stats = dict(tr.get_eval_statistics()) if not explicit else {}
        out = (tr.get_snapshot(), stats, tr.rng_step, tr.phase_state(), n_done)
        ctx.close()
        return out
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _assert_same(r0, r1):
    (s0, st0, c0, _, n0), (s1, st1, c1, _, n1) = r0, r1
    assert c0 == c1 == n0 == n1
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
@pytest.mark.parametrize("o,a,H,B,n_steps", [(11, 3, 256, 17, 3),     # ragged second tile, padding tiles
                                             (17, 6, 128, 16, 3),     # the 2-slice instance, a = 6 head
                                             (11, 3, 256, 129, 2),    # second round of eight tiles
                                             (27, 8, 256, 17, 2),     # 16 head outputs: the last lane of the broadcast; three staging trips
                                             (11, 9, 256, 17, 2)])    # 18 head outputs: a second head trip, delta_1 output by output
def test_static_heads_are_bitwise_the_one_launch_per_stage_path(o, a, H, B, n_steps):
    phase, stages = _run(o, a, H, B, n_steps, "phase"), _run(o, a, H, B, n_steps, "stages")
    assert phase[3]["last_window_on_phase"] and phase[3]["fallbacks"] == 0 and not stages[3]["last_window_on_phase"], (phase[3], stages[3])
    assert phase[0]["log_alpha"] != float(np.log(SAC_KW["alpha"]))   # alpha moved: a stale one would differ
    _assert_same(phase, stages)


@pytest.mark.gpu
def test_target_critics_on_the_policy_rows_take_the_same_text():
    own, old = _run(11, 3, 256, 37, 3, "phase"), _run(11, 3, 256, 37, 3, "old")
    for r in (own, old):
        assert r[3]["last_window_on_phase"] and r[3]["fallbacks"] == 0, r[3]
    _assert_same(own, old)


@pytest.mark.gpu
def test_explicit_noise_steps_take_one_launch_per_stage_whatever_the_switch():
    """Explicit noise reaches the library only through train_step, which never runs on the phase kernels (and launch_phase_a refuses a
    descriptor that carries it, below): such steps are one launch per stage with and without ILSX_NO_PHASE, and give the same bits — the
    wrappers' code, which this change leaves as it was."""
    a, b = _run(11, 3, 256, 17, 0, "phase", explicit=True), _run(11, 3, 256, 17, 0, "stages", explicit=True)
    assert not a[3]["last_window_on_phase"] and not b[3]["last_window_on_phase"] and a[3]["fallbacks"] == b[3]["fallbacks"] == 0, (a[3], b[3])
    _assert_same(a, b)


def test_phase_launches_refuse_descriptors_they_are_not_compiled_for():
    """Host only: the checks launch_phase_a / _c run on their descriptor blocks (ilsx_core.hip phase_a_static_ok / phase_c_static_ok)."""
    from ilswiss_amd import _lib
    lib = _lib.load()
    ok = lambda *v, flags=0: lib.ilsx_debug_phase_static_ok(*v, flags)   # noqa: E731   (stage, loss_critic, loss_policy, no_critic, slabs, fin_head, a, H, cs)
    assert ok(0, LOSS_SAC_CRITIC, 0, 1, 4, HEAD_TANH_SAMPLE, 3, 256, 4) == 1
    assert ok(0, LOSS_SAC_CRITIC, 0, 1, 2, HEAD_TANH_SAMPLE, 6, 128, 2) == 1
    assert ok(0, LOSS_MSE, 0, 1, 4, HEAD_TANH_SAMPLE, 3, 256, 4) == 0          # foreign loss kind
    assert ok(0, LOSS_SAC_CRITIC, 0, 2, 4, HEAD_TANH_SAMPLE, 3, 256, 4) == 0   # two head outputs
    assert ok(0, LOSS_SAC_CRITIC, 0, 1, 2, HEAD_TANH_SAMPLE, 3, 256, 4) == 0   # slab count != the kernel's
    assert ok(0, LOSS_SAC_CRITIC, 0, 1, 4, HEAD_TANH_DET, 3, 256, 4) == 0      # another head kind
    assert ok(0, LOSS_SAC_CRITIC, 0, 1, 4, HEAD_TANH_SAMPLE, 17, 256, 4) == 0  # more epilogue elements than threads
    assert ok(1, LOSS_SAC_ACTORQ, LOSS_SAC_POLICY, 1, 4, 0, 3, 256, 4) == 1
    assert ok(1, LOSS_MSE, LOSS_SAC_POLICY, 1, 4, 0, 3, 256, 4) == 0
    assert ok(1, LOSS_SAC_ACTORQ, LOSS_MSE, 1, 4, 0, 3, 256, 4) == 0
    assert ok(1, LOSS_SAC_ACTORQ, LOSS_SAC_POLICY, 1, 2, 0, 3, 256, 4) == 0
    assert ok(0, LOSS_SAC_CRITIC, 0, 1, 4, HEAD_TANH_SAMPLE, 3, 256, 4, flags=1) == 0   # explicit noise for the epilogue
    assert ok(1, LOSS_SAC_ACTORQ, LOSS_SAC_POLICY, 1, 4, 0, 3, 256, 4, flags=2) == 0    # phase C's stage 1 would finish a policy


@functools.lru_cache(maxsize=None)
def _static_counts():
    spec = importlib.util.spec_from_file_location("kernel_static", os.path.join(ROOT, "tools", "kernel_static.py"))
    ks = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks)
    out = os.path.join(tempfile.mkdtemp(prefix="isa_heads_"), "core.s")
    try:
        r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "ilswiss_amd", "csrc", "ilsx_core.hip"), "-o", out], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out).read().split("\n")
        return {dn: dict(total=len(body), windows=ks.head_windows(body)) for dn, body, _ in ks.kernel_bodies(text) if dn.startswith("void k_sac_phase_")}
    finally:
        shutil.rmtree(os.path.dirname(out), ignore_errors=True)


def _window_pairs(dn, p, n):
    """(parent's counts, this tree's window) per post-wait window of one kernel.  Phase A: the window behind more poll loops is the critics'
    backward (f1, tail flag, f2 in series), the other the target critics.  Phase C's two windows (critics' backward, policy backward) are
    each held against the SMALLER of the parent's two counts, which needs no telling them apart."""
    assert len(n["windows"]) == len(p["windows"]) == 2, (dn, n["windows"])
    if "phase_a" in dn:
        return list(zip(sorted(p["windows"], key=lambda w: w["polls"]), sorted(n["windows"], key=lambda w: w["polls"])))
    least = dict(s_load=min(w["s_load"] for w in p["windows"]), lgkm=min(w["lgkm"] for w in p["windows"]))
    return [(least, w) for w in n["windows"]]


def _parent_and_now(family):
    parent = json.load(open(os.path.join(ROOT, "tests", "golden", "phase_head_counts_parent.json")))
    assert len(parent) == 4   # ReLU and tanh instances of both 256-wide constant-table kernels
    now = _static_counts()
    for dn, p in sorted(parent.items()):
        if family in dn:
            print(dn, "total", p["total"], "->", now[dn]["total"], now[dn]["windows"])
            yield dn, p, now[dn]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("family", ["k_sac_phase_a", "k_sac_phase_c"])
def test_post_wait_windows_hold_a_quarter_of_the_parents_scalar_loads(family):
    """No GPU.  Also: neither kernel's instruction count grew."""
    for dn, p, n in _parent_and_now(family):
        assert n["total"] <= p["total"], (dn, n["total"], p["total"])
        for pw, nw in _window_pairs(dn, p, n):
            assert 4 * nw["s_load"] <= pw["s_load"], (dn, nw, pw)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("family", ["k_sac_phase_a", "k_sac_phase_c"])
def test_post_wait_windows_hold_a_quarter_of_the_parents_lgkmcnt_waits(family):
    """No GPU.  (The policy backward's delta_1 phase reads the tile's head gradients from LDS once per wave and broadcasts them from lanes:
    with one LDS read per (row, output) and thread that window alone held 53 of these waits.)"""
    for dn, p, n in _parent_and_now(family):
        for pw, nw in _window_pairs(dn, p, n):
            assert 4 * nw["lgkm"] <= pw["lgkm"], (dn, nw, pw)
