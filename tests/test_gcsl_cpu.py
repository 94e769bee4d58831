"""CPU suite for GCSL against the reference's own vectors (tests/golden/g29_gcsl.npz, written by tools/make_golden.py's `gcsl` group):
(1) the torch restatement (tests/gcsl_restatement.py) reproduces the reference's CLASS and MSE steps; (2) the host horizon buffer draws
the reference's indices and builds its horizons (a wrapped trajectory's all-ones rows included); (3) DiscretEnv's action grid; (4) the DEVICE
text of the BatchNorm categorical step and of the horizon gather (ilswiss_amd/csrc/gcsl.h over disc_bn.h) compiled for the host
(tests/harness/gcsl_bn_host.cpp, every phase a serial loop) reproduces the reference."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import gcsl_restatement as GR  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "g29_gcsl.npz"))
O, GD, A, T, CAP = [int(v) for v in G["dims"]]
D = O + GD + T
LR = 3e-4


def _case(c):
    Hw, B, n, seed, steps = [int(v) for v in G[f"c{c}_shape"]]
    return Hw, B, n, seed, steps


def _live(c, Hw, n, seed, steps, B):
    """Parameters with a gradient: not the Linear biases under a BatchNorm, and not the first layer's weights on an input column that is
    constant over every batch (the last horizon column): BatchNorm removes both exactly, so what they hold is rounding noise."""
    rst = GR.CatRestatement(GR.cat_init(seed, D, Hw, 2, n), D, Hw, 2, n, lr=LR)
    live = ~rst.dead_bias_mask()
    Xs = np.concatenate([X for X, _ in GR.cat_batches(seed + 100, B, steps, O, GD, T, n)])
    const = np.where(Xs.min(0) == Xs.max(0))[0]
    W0 = np.zeros((Hw, D), bool)
    W0[:, const] = True
    live[:Hw * D] &= ~W0.ravel()
    return live


def _check_final(c, params, rm, rv, probs_fn):
    Hw, B, n, seed, steps = _case(c)
    idx = G[f"c{c}_idx"]
    live = _live(c, Hw, n, seed, steps, B)[idx]
    assert np.abs(params[idx] - G[f"c{c}_final"])[live].max() < 5e-5
    np.testing.assert_allclose(rv, G[f"c{c}_running_var"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rm, G[f"c{c}_running_mean"], rtol=0, atol=steps * 2.02 * LR + 1e-5)   # the batch mean carries the dead bias
    pr = GR.probe(seed + 200, 64, O, GD, T)
    np.testing.assert_allclose(probs_fn(pr), G[f"c{c}_probe_probs"], rtol=0, atol=1e-3)


@pytest.mark.parametrize("c", [0, 1])
def test_restatement_matches_reference_class(c):
    Hw, B, n, seed, steps = _case(c)
    rst = GR.CatRestatement(GR.cat_init(seed, D, Hw, 2, n), D, Hw, 2, n, lr=LR)
    for s, (X, y) in enumerate(GR.cat_batches(seed + 100, B, steps, O, GD, T, n)):
        ce, acc = rst.train_step(X, y)
        np.testing.assert_allclose(ce, G[f"c{c}_ce"][s], rtol=1e-5)
        assert np.float32(acc) == G[f"c{c}_acc"][s]
    rm, rv = rst.running()
    _check_final(c, rst.flat(), rm, rv, rst.probs)
    np.testing.assert_allclose(np.stack([b.weight.detach().numpy() for b in rst.net.bns]), G[f"c{c}_gamma"], atol=5e-5)


def test_restatement_matches_reference_mse():
    Hw, B, a, seed, steps = [int(v) for v in G["m0_shape"]]
    rst = GR.MseRestatement(GR.mse_init(seed, D, Hw, 2, a), D, Hw, 2, a, lr=LR)
    for s, (X, act) in enumerate(GR.mse_batches(seed + 100, B, steps, O, GD, T, a)):
        np.testing.assert_allclose(rst.train_step(X, act), G["m0_mse"][s], rtol=1e-5)
    assert np.abs(rst.flat()[G["m0_idx"]] - G["m0_final"]).max() < 5e-5


class _Env:
    tol = 0.1   # the sparse rule's threshold (what DeviceHindsightReplayBuffer reads)

    def __init__(self):
        from ilswiss_amd.her import Box, DictSpace
        self.observation_space = DictSpace(observation=Box(-np.ones(O), np.ones(O)), desired_goal=Box(-np.ones(GD), np.ones(GD)),
                                           achieved_goal=Box(-np.ones(GD), np.ones(GD)))
        self.action_space = Box(-np.ones(1), np.ones(1))

    @staticmethod
    def compute_reward(ag, dg, info=None):
        return -(np.linalg.norm(ag - dg, axis=-1) > 0.1).astype(np.float32)


def fill(buf):
    p = 0
    while f"p{p}_obs" in G.files:
        obs, dg, ag, act = G[f"p{p}_obs"], G[f"p{p}_dg"], G[f"p{p}_ag"], G[f"p{p}_act"]
        for i in range(act.shape[0]):
            buf.add_sample(dict(observation=obs[i], desired_goal=dg[i], achieved_goal=ag[i]), act[i], -1.0, False,
                           dict(observation=obs[i + 1], desired_goal=dg[i + 1], achieved_goal=ag[i + 1]))
        buf.terminate_episode()
        p += 1


def test_host_buffer_indices_and_horizons_match_reference():
    from ilswiss_amd.gcsl import HindsightHorizonReplayBuffer
    buf = HindsightHorizonReplayBuffer(T, CAP, _Env(), random_seed=29, relabel_type="future")
    assert buf.her_ratio == 1.0
    fill(buf)
    assert np.array_equal(np.array(sorted(buf._traj_endpoints.items())), G["buf_endpoints"])
    np.random.seed(2930)
    b = buf.random_batch(64)
    idx, idx_rel = buf.last_indices
    assert np.array_equal(idx, G["buf_idx"]) and np.array_equal(idx_rel, G["buf_idx_relabel"])
    assert np.array_equal(b["horizons"], G["buf_horizons"].astype(np.float32))
    wrapped = idx_rel < idx
    assert wrapped.any() and b["horizons"][wrapped].all()          # the reference's all-ones rows of a wrapped trajectory
    assert np.array_equal(b["observations"], G["buf_obs"]) and np.array_equal(b["desired_goals"], G["buf_desired_goals"])
    # the reference's env had a 2-wide action box: its ring held each class index in both columns
    assert np.array_equal(b["actions"][:, 0], G["buf_actions"][:, 0]) and np.array_equal(b["rewards"], G["buf_rewards"])


def test_discret_env_base_actions_match_reference():
    from ilswiss_amd.envs import DiscretEnv
    from ilswiss_amd.her import PointReachEnv
    env = DiscretEnv(PointReachEnv(seed=0), granularity=5)
    assert env.action_space.n == 25 and env.action_space.n_dims == 2 and env.action_space.granularity == 5
    assert np.array_equal(env.base_actions, G["base_actions"])
    env.reset()
    env.step(np.array([24]))
    np.testing.assert_allclose(env.wrapped_env.v, 0.1 * G["base_actions"][24])


@pytest.fixture(scope="module")
def hostlib():
    d = tempfile.mkdtemp(prefix="gch_")
    so = os.path.join(d, "libgch.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "harness", "gcsl_bn_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.gch_create.restype = C.c_void_p
    lib.gch_create.argtypes = [C.c_int] * 5
    lib.gch_destroy.argtypes = [C.c_void_p]
    lib.gch_num_params.argtypes = [C.c_void_p]
    lib.gch_set_params.argtypes = [C.c_void_p, C.c_void_p]
    lib.gch_get.argtypes = [C.c_void_p] * 4
    lib.gch_train_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    lib.gch_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.gch_gather.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("c", [0, 1])
def test_device_phases_on_the_host_match_the_reference(hostlib, c):
    lib = hostlib
    Hw, B, n, seed, steps = _case(c)
    h = lib.gch_create(D, Hw, 2, n, max(B, 64))
    p0 = GR.cat_init(seed, D, Hw, 2, n)
    assert lib.gch_num_params(h) == p0.size
    lib.gch_set_params(h, _p(p0))
    for s, (X, y) in enumerate(GR.cat_batches(seed + 100, B, steps, O, GD, T, n)):
        st, y32 = np.zeros(2, np.float32), np.ascontiguousarray(y, np.int32)
        assert lib.gch_train_step(h, _p(X), _p(y32), B, LR, _p(st)) == 0
        np.testing.assert_allclose(st[0], G[f"c{c}_ce"][s], rtol=1e-5)
        assert st[1] == G[f"c{c}_acc"][s]
    params, rm, rv = np.empty(p0.size, np.float32), np.empty((2, Hw), np.float32), np.empty((2, Hw), np.float32)
    lib.gch_get(h, _p(params), _p(rm), _p(rv))

    def probs(x):
        out, am = np.empty((x.shape[0], n), np.float32), np.empty(x.shape[0], np.float32)
        assert lib.gch_eval(h, _p(x), x.shape[0], _p(out), _p(am)) == 0
        assert np.array_equal(am, out.argmax(1))
        return out
    _check_final(c, params, rm, rv, probs)
    lib.gch_destroy(h)


def test_host_gather_matches_reference_batch(hostlib):
    """The horizon gather of gcsl.h over a host copy of the ring's records (the layout of ilsx_replay) equals the reference's batch."""
    from ilswiss_amd.gcsl import HindsightHorizonReplayBuffer
    buf = HindsightHorizonReplayBuffer(T, CAP, _Env(), random_seed=29, relabel_type="future")
    fill(buf)
    o = O + 2 * GD
    rec = o + 1 + 2 + o
    data = np.zeros((CAP, rec), np.float32)
    for k, key in enumerate(("observation", "desired_goal", "achieved_goal")):
        lo = [0, O, O + GD][k]
        w = O if k == 0 else GD
        data[:, lo:lo + w] = buf._observations[key]
        data[:, o + 3 + lo:o + 3 + lo + w] = buf._next_obs[key]
    data[:, o] = buf._actions[:, 0]
    idx, idx_rel = np.ascontiguousarray(G["buf_idx"], np.int64), np.ascontiguousarray(G["buf_idx_relabel"], np.int64)
    B = idx.size
    X, lab = np.zeros((B, D), np.float32), np.zeros(B, np.int32)
    lib = hostlib
    lib.gch_gather(_p(data), rec, _p(idx), _p(idx_rel), B, O, GD, 1, T, 1, _p(X), None, _p(lab))
    assert np.array_equal(X[:, :O], G["buf_obs"].astype(np.float32))
    assert np.array_equal(X[:, O:O + GD], G["buf_desired_goals"].astype(np.float32))
    assert np.array_equal(X[:, O + GD:], G["buf_horizons"].astype(np.float32))
    assert np.array_equal(lab, G["buf_actions"][:, 0].astype(np.int32))


@pytest.mark.parametrize("c", [0, 1])
def test_running_statistics_on_the_host_match_at_zero_lr(hostlib, c):
    """The running-statistics update at the issue's tolerance (rtol 1e-4 / atol 1e-5).  With lr = 0 Adam moves no parameter, so the
    BN-dead Linear biases, whose rounding noise otherwise drifts into the batch means, stay put: the device text (host build) and the
    restatement (pinned to the reference above) then see the same batch means step after step."""
    lib = hostlib
    Hw, B, n, seed, steps = _case(c)
    p0 = GR.cat_init(seed, D, Hw, 2, n)
    h = lib.gch_create(D, Hw, 2, n, max(B, 64))
    lib.gch_set_params(h, _p(p0))
    rst = GR.CatRestatement(p0, D, Hw, 2, n, lr=0.0)
    for X, y in GR.cat_batches(seed + 100, B, steps, O, GD, T, n):
        st = np.zeros(2, np.float32)
        assert lib.gch_train_step(h, _p(X), _p(np.ascontiguousarray(y, np.int32)), B, 0.0, _p(st)) == 0
        rst.train_step(X, y)
    params, rm, rv = np.empty(p0.size, np.float32), np.empty((2, Hw), np.float32), np.empty((2, Hw), np.float32)
    lib.gch_get(h, _p(params), _p(rm), _p(rv))
    assert np.array_equal(params, p0)
    want_m, want_v = rst.running()
    np.testing.assert_allclose(rm, want_m, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rv, want_v, rtol=1e-4, atol=1e-5)
    lib.gch_destroy(h)
