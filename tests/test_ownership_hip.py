"""GPU suite: every library object gives its device memory back when it is destroyed (csrc/dev_owner.h: one owner per handle), and the Python
trainers reach that through close().  The two-lives pattern of tests/test_lane_frame_hip.py on the session context: networks, replay rings
and the batches are built once; a life builds the object, runs one step at B = 8 and one at B = 1024 (DW_SPLIT_MIN_ROWS: the first row count
whose weight gradients run split over row ranges and allocate a scratch region), and closes it.  Life 1 warms up what the context itself
keeps (its staging buffer); the context's allocation count after life 2 must equal the count before it.

Shapes: obs 3, act 2 (two actions for the discrete kinds), hidden [32, 32], max_batch 1024 — except where an allocation needs more:
  sac        once more at [256, 256], B = 256 through train_from_replay: the column-split path (cs > 1) allocates the deferred tail's record
             (tail_dev) and the window's checkpoint (snap) there.  `vote` exists only in a run split over ranks with a communicator: not
             reachable on one GPU.
  sac_group  [128, 128]: grouped steps exist only on the column-split kernels, and 128 is their smallest width.
The discriminator's `snap` is allocated by ilsx_advirl_train's windows only and is not reached here."""
import ctypes as C

import numpy as np
import pytest

O, A, HID, MAXB = 3, 2, [32, 32], 1024
BATCHES = (8, 1024)


def _ctx_allocs(ctx):
    n = C.c_size_t()
    assert ctx.lib.ilsx_debug_ctx_allocs(ctx.h, C.byref(n)) == 0
    return n.value


def _batch(B, o=O, a=A, discrete=False, seed=0):
    rng = np.random.default_rng(seed + B)
    act = rng.integers(0, 2, (B, 1)).astype(np.float32) if discrete else np.tanh(rng.normal(0, 1, (B, a))).astype(np.float32)
    return dict(observations=rng.normal(0, 1, (B, o)).astype(np.float32), actions=act, rewards=rng.normal(0, 1, (B, 1)).astype(np.float32),
                terminals=(rng.random((B, 1)) < 0.1).astype(np.float32), next_observations=rng.normal(0, 1, (B, o)).astype(np.float32))


def _ring(ctx, o=O, a=A, n=2048, seed=0):
    import ilswiss_amd as ia
    b = _batch(n, o, a, seed=seed)
    rb = ia.SimpleReplayBuffer(n, o, a, ctx=ctx)
    rb.add_rows(b["observations"], b["actions"], b["rewards"], b["terminals"], b["next_observations"])
    return rb


def _actor_critic(ctx, kind, hid=HID):
    """(build, nets): build() makes the trainer of `kind` around networks made here, once."""
    import ilswiss_amd as ia
    from ilswiss_amd.bc import BC
    from ilswiss_amd.sac_v import SoftActorCriticV
    from ilswiss_amd.td3 import TD3, MlpGaussianNoisePolicy
    q = lambda out=1, inp=O + A: ia.FlattenMlp(hid, out, inp, ctx=ctx)   # noqa: E731
    gauss = lambda: ia.ReparamTanhMultivariateGaussianPolicy(hid, O, A, ctx=ctx)   # noqa: E731
    if kind == "sac":
        nets = (gauss(), q(), q())
        return (lambda: ia.SoftActorCritic(*nets, max_batch=MAXB)), nets
    if kind in ("td3", "her_td3"):
        nets = (MlpGaussianNoisePolicy(hid, O, A, ctx=ctx), q(), q())
        kw = dict(her=True, clip_return_l=-100.0, clip_return_r=0.0) if kind == "her_td3" else {}
        return (lambda: TD3(*nets, max_batch=MAXB, **kw)), nets
    if kind == "ddpg":
        nets = (ia.MlpPolicy(hid, O, A, ctx=ctx), q())
        return (lambda: ia.DDPG(*nets, max_batch=MAXB)), nets
    if kind == "sacv":
        nets = (gauss(), q(), q(), q(1, O))
        return (lambda: SoftActorCriticV(*nets, max_batch=MAXB)), nets
    if kind == "bc":
        nets = (gauss(),)
        return (lambda: BC("MLE", nets[0], batch_size=MAXB)), nets
    if kind == "dsac":
        nets = (ia.DiscretePolicy(hid, O, 2, ctx=ctx), q(2, O), q(2, O))
        return (lambda: ia.DiscreteSoftActorCritic(*nets, max_batch=MAXB)), nets
    assert kind in ("dqn", "double_dqn")
    qf = q(2, O)
    pol = ia.ArgmaxDiscretePolicy(qf, 0.1)
    return (lambda: (ia.DoubleDQN if kind == "double_dqn" else ia.DQN)(qf, policy=pol, max_batch=MAXB)), (qf,)


AC_KINDS = ("sac", "td3", "her_td3", "ddpg", "sacv", "bc", "dsac", "dqn", "double_dqn")


def _life_of(ctx, kind):
    """(life, adopted).  life() -> the context's allocation count after the steps, before the close; everything that outlives a life is
    made here.  adopted: the networks the object takes into its arena, whose own blocks go back to the context while it lives."""
    import ilswiss_amd as ia
    from ilswiss_amd import _lib
    if kind in AC_KINDS:
        build, nets = _actor_critic(ctx, kind)
        batches = [_batch(B, discrete=kind in ("dsac", "dqn", "double_dqn")) for B in BATCHES]

        def life():
            tr = build()
            for b in batches:
                tr.train_step(b)
            ctx.sync()
            n = _ctx_allocs(ctx)
            tr.close()
            return n
        return life, len(nets)
    if kind == "sac_wide":   # the column-split path: deferred tail record + window checkpoint
        build, nets = _actor_critic(ctx, "sac", [256, 256])
        rb = _ring(ctx)

        def life():
            tr = build()
            tr.train_from_replay(rb, 2, 256)
            ctx.sync()
            n = _ctx_allocs(ctx)
            tr.close()
            return n
        return life, len(nets)
    if kind == "sac_group":
        sets = [_actor_critic(ctx, "sac", [128, 128])[0] for _ in range(2)]
        rbs = [_ring(ctx, seed=k) for k in range(2)]

        def life():
            trs = [build() for build in sets]
            grp = ia.SoftActorCriticGroup(trs)
            for B in BATCHES:
                grp.train_from_replay(rbs, 1, B)
            ctx.sync()
            n = _ctx_allocs(ctx)
            grp.close()
            grp.close()
            for t in trs:
                t.close()
            return n
        return life, 6
    if kind == "ppo":
        from ilswiss_amd.ppo import PPO, ReparamMultivariateGaussianPolicy
        pol = ReparamMultivariateGaussianPolicy(HID, O, A, conditioned_std=False, hidden_activation="tanh", ctx=ctx)
        vf = ia.FlattenMlp(HID, 1, O, hidden_activation="tanh", ctx=ctx)

        def trajs(n, T):
            return [{k: v.reshape(T, -1) for k, v in _batch(T, seed=i).items() if k in ("observations", "actions", "rewards")} for i in range(n)]
        small, big = trajs(1, 8), trajs(4, 256)

        def life():
            tr = PPO(pol, vf, mini_batch_size=1024, update_epoch=1, max_samples=1024)
            tr.train_step(small)
            ctx.sync()
            n0 = _ctx_allocs(ctx)
            tr.train_step(big)     # one minibatch of 1024 rows: the split weight-gradient launch allocates its scratch region
            ctx.sync()
            n = _ctx_allocs(ctx)
            assert n > n0, (n0, n)
            tr.close()
            tr.close()
            return n
        return life, 0
    if kind in ("disc", "disc_bn"):
        from ilswiss_amd.adv_irl import MLPDisc
        disc = MLPDisc(O + A, hid_dim=32, hid_act="relu", use_bn=kind == "disc_bn", ctx=ctx, seed=1)
        batches = [(_batch(B, seed=1), _batch(B, seed=2)) for B in BATCHES]

        def life():
            disc.bind(O, max_batch=MAXB)
            for e, p in batches:
                disc.train_step(e["observations"], e["actions"], p["observations"], p["actions"])
            ctx.sync()
            n = _ctx_allocs(ctx)
            disc.close()
            disc.close()
            assert disc.h is None and disc.get_flat_params().size == disc.num_params   # unbound again, parameters kept
            return n
        return life, 0
    if kind == "bnn":
        from ilswiss_amd.envs.terminals import get_terminal_func
        from ilswiss_amd.mbpo import BNN, terminal_kind
        E, n_rows = 2, 1024
        rb = _ring(ctx, n=n_rows)
        rng = np.random.default_rng(3)
        table = ctx.from_numpy(rng.integers(0, n_rows, (E, n_rows)), np.int32)
        b = _batch(8)
        d_obs, d_act = ctx.from_numpy(b["observations"]), ctx.from_numpy(b["actions"])
        nxt, mo, ns = ctx.empty((8, O)), ctx.empty((8,), np.int32), C.c_int()
        elites = np.array([0, 1], np.int32)
        term = terminal_kind(get_terminal_func("hopper"))

        def life():
            bnn = BNN(hidden_sizes=HID, output_size=O + 1, input_size=O + A, num_nets=E, ctx=ctx, seed=0)
            bnn._configure(max_batch=MAXB)
            for B in BATCHES:
                _lib.check(ctx.lib.ilsx_bnn_train_batch(bnn.h, rb.h, table.ptr, n_rows, B, None))
            _lib.check(ctx.lib.ilsx_mbpo_model_step(bnn.h, None, None, term, d_obs.ptr, d_act.ptr, 8, elites.ctypes.data_as(C.c_void_p), 2, 0,
                                                    None, None, None, mo.ptr, nxt.ptr, C.byref(ns)))   # the rollout buffers s_*
            ctx.sync()
            n = _ctx_allocs(ctx)
            bnn.close()
            bnn.close()
            return n
        return life, 0
    assert kind in ("gcsl_class", "gcsl_mse")
    from ilswiss_amd.gcsl import GCSL, CatagorialConditionPolicy, MlpGaussianAndEpsilonConditionPolicy
    batches = []
    for B in BATCHES:
        b = _batch(B, o=2, discrete=kind == "gcsl_class")
        batches.append(dict(observations=b["observations"], desired_goals=b["rewards"], actions=b["actions"]))
    if kind == "gcsl_class":   # ilsx_gcsl holds no device memory of its own in this mode: the object that does is its policy, an ilsx_bncat
        def life():
            pol = CatagorialConditionPolicy(HID, 2, 1, 2, max_rows=MAXB, ctx=ctx, seed=0)
            tr = GCSL(pol, mode="CLASS", max_batch=MAXB)
            for b in batches:
                tr.train_step(b)
            ctx.sync()
            n = _ctx_allocs(ctx)
            tr.close()
            tr.close()
            _lib.check(ctx.lib.ilsx_bncat_destroy(pol.h))
            pol.h = C.c_void_p()   # (what the policy's own finaliser would do)
            return n
        return life, 0
    pol = MlpGaussianAndEpsilonConditionPolicy(HID, 2, 1, A, ctx=ctx, seed=0)

    def life():
        tr = GCSL(pol, mode="MSE", max_batch=MAXB)
        for b in batches:
            tr.train_step(b)
        ctx.sync()
        n = _ctx_allocs(ctx)
        tr.close()
        tr.close()
        return n
    return life, 1   # the behaviour-cloning trainer inside adopts the policy


@pytest.mark.gpu
@pytest.mark.parametrize("kind", AC_KINDS + ("sac_wide", "sac_group", "ppo", "disc", "disc_bn", "bnn", "gcsl_class", "gcsl_mse"))
def test_an_object_gives_back_every_device_allocation(ctx, kind):
    life, adopted = _life_of(ctx, kind)
    life()
    before = _ctx_allocs(ctx)
    inside = life()
    after = _ctx_allocs(ctx)
    print(f"{kind}: context allocations after the first life {before}, inside the second {inside} ({adopted} networks adopted), after it {after}")
    # The life did allocate, so the equality below is not vacuous.  The object's own blocks are those inside the life minus what else is alive
    # then: `before` less the adopted networks' blocks, which went back to the context at adoption (sac at hidden 32: one slab + two scratch
    # regions - three networks = a count that does not move, so `inside > before` alone would not say what it is meant to).
    assert inside - (before - adopted) > 0
    assert after == before


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("td3", "sac"))
def test_close_hands_the_networks_back_and_an_adopted_network_cannot_be_destroyed(ctx, kind):
    build, nets = _actor_critic(ctx, kind)
    policy = nets[0]
    tr = build()
    small = _batch(8)
    tr.train_step(small)
    assert ctx.lib.ilsx_net_destroy(policy.h) != 0              # refused: the trainer writes through the network when it goes
    assert b"agent" in ctx.lib.ilsx_last_error()
    tr.train_step(small)                                        # ... and both are alive
    tr.train_step(small)
    ctx.sync()
    held = tr.get_flat_params("policy")
    assert np.array_equal(held, policy.get_flat_params())       # the network's handle reads the trainer's arena
    tr.close()
    own = policy.get_flat_params()                              # storage of its own again
    assert own.tobytes() == held.tobytes()
    before = _ctx_allocs(ctx)
    tr.close()                                                  # a second close: nothing happens
    assert tr.h is None and _ctx_allocs(ctx) == before
    tr2 = build()                                               # the networks can be adopted again
    tr2.train_step(small)
    ctx.sync()
    tr2.close()
    assert _ctx_allocs(ctx) == before
