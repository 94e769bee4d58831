"""A float64 restatement of the three discrete-action steps — discrete SAC (discrete_sac.py:60-181; csrc/dsac.h, dsac_step in ilsx_ac.hip),
DQN / Double DQN (dqn.py:67-112, double_dqn.py:12-38; csrc/dqn.h, dqn_step) and GCSL's BatchNorm categorical CLASS step (csrc/gcsl.h,
ilsx_gcsl.hip) — shared by the CPU and the GPU tests of tests/test_discrete_parity_hip.py:

  * `CASES` (one step) and `FROZEN` (three steps at zero learning rates and tau, B = 96, 37, 64 under max_batch = 128) for dsac and DQN,
    `GCSL_CASES` for the CLASS step: the smallest shapes at which the device step changes path (column split cs = 1 / 2 / 4, a slab stride
    that is not B, n = ILSX_MAX_NO, one row; one / two / three BatchNorm blocks, more than 512 rows);
  * `make_case`: the inputs of a case drawn from its seed — every block, TARGETS included, an independent draw whose head is rescaled so that
    max|Q| is O(1) and pi(s) is visibly non-uniform; batches with mixed terminals and actions that cover the classes; DQN rows whose
    arg-maxed row has its two largest entries closer than twice the margin are drawn again until none is left;
  * `dsac_f64` / `dqn_f64`: one step's losses written FORWARDS only and differentiated by torch autograd, so that no backward formula is shared
    with dsac_restatement.py, dqn_restatement.py or the kernels.  Target blocks are given separately from the online ones, and so are the
    critics dsac's policy loss sees (`actor=`: the critics AFTER their Adam step);
  * `gcsl_f64`: gcsl_restatement.CatRestatement in float64 (gradient of every parameter of one batch, no step);
  * the fp32 witnesses that stand in for the device without a GPU: dsac_restatement.DsacRestatement, dqn_restatement.DqnRestatement(float32);
  * `block_errors` (ac_restatement's, on the FlattenMlp / DiscretePolicy layout o -> hidden -> n) and `gcsl_block_errors`.
`wrong=` swaps in a deliberately wrong reference (`DSAC_WRONG`, `DQN_WRONG`, CatRestatement.WRONG).  Hyper-parameters enter as the fp32 numbers the
ABI carries.  Flat vectors are in the ABI layout fc0.W | fc0.b | fc1.W | fc1.b | last_fc.W | last_fc.b."""
import functools

import numpy as np
import torch

import ac_restatement as AR
import gcsl_restatement as GR
from ac_restatement import adam_moments, f32  # noqa: F401  (re-exported)
from dqn_restatement import DqnRestatement
from dsac_restatement import DsacRestatement, unflatten
from oracle import mlp as omlp

F32 = np.float32
KINK_REL = 1e-3

NETS = dict(dsac=("q1", "q2", "pi"), dqn=("q",))
TARGETS = dict(dsac=("tq1", "tq2"), dqn=("tq",))
ONLINE_OF = dict(tq1="q1", tq2="q2", tq="q")
DEVICE_NAME = dict(q1="qf1", q2="qf2", pi="policy", tq1="target_qf1", tq2="target_qf2", q="qf", tq="target_qf")
DSAC_WRONG = ("online_targets", "target_pi_s", "no_target_entropy", "no_reward_scale", "no_done", "inv_b", "no_half", "shift_action", "pi_pre",
              "pi_q1", "no_policy_entropy")
DQN_WRONG = ("online_targets", "swap_double", "half", "inv_b", "no_done", "no_discount")

HYPER = dict(dsac=dict(reward_scale=5.0, alpha=0.2, discount=0.97, tau=0.01, lr=1e-3, beta_1=0.9),
             dqn=dict(discount=0.97, tau=0.01, lr=1e-3, beta_1=0.9))      # DQN has no reward scale and no alpha; its Adam is (0.9, 0.999)
# shape -> (o, hidden, n, max_batch, (B per step ...))
SHAPES = dict(
    spec=(4, [128, 128], 2, 128, (128,)),             # the committed spec, column split cs = 2
    wide_ragged=(6, [256, 256], 5, 64, (37,)),        # cs = 4, slab stride != B, ragged tile
    generic=(11, [64, 64], 3, 96, (96,)),             # cs = 1: the generic kernels finish the head themselves
    max_heads=(8, [128, 128], 64, 128, (48,)),        # n = ILSX_MAX_NO, slab stride != B
    one_row=(4, [256, 256], 3, 16, (1,)),             # inv_B = 1, statistics of one row
)
FROZEN_SHAPE = (7, [256, 256], 5, 128, (96, 37, 64))
# DQN: plain and double alternate so that each runs at cs = 1, 2 and 4; max_heads is plain (the maximum over 64 entries), max_heads_double its twin
DQN_DOUBLE = dict(spec=True, wide_ragged=False, generic=True, max_heads=False, one_row=True, max_heads_double=True, generic_plain=False)
DQN_SHAPES = dict(SHAPES, max_heads_double=SHAPES["max_heads"], generic_plain=SHAPES["generic"])


def _case(algo, shape, dims, seed, **over):
    o, hidden, n, mb, Bs = dims
    return dict(HYPER[algo], algo=algo, shape=shape, o=o, hidden=hidden, n=n, max_batch=mb, Bs=Bs, seed=seed, **over)


CASES = {f"dsac/{k}": _case("dsac", k, v, 7100 + i) for i, (k, v) in enumerate(SHAPES.items())}
CASES.update({f"dqn/{k}": _case("dqn", k, v, 7200 + i, double_q=DQN_DOUBLE[k]) for i, (k, v) in enumerate(DQN_SHAPES.items())})
FROZEN = {"dsac/frozen": _case("dsac", "frozen", FROZEN_SHAPE, 7300, lr=0.0, tau=0.0),
          "dqn/frozen": _case("dqn", "frozen", FROZEN_SHAPE, 7301, lr=0.0, tau=0.0, double_q=True)}
ALL = dict(CASES, **FROZEN)

# GCSL CLASS: name -> (H, nblk, n, B, max_rows); the input is observation | goal | horizon of test_gcsl_cpu.py's widths
GCSL_LR = 3e-4
GCSL_CASES = dict(
    spec=(300, 2, 25, 128, 128),                 # the committed spec; H is no multiple of 16 x 4 waves
    one_block=(64, 1, 2, 37, 64),                # the top block is block 0
    three_blocks=(48, 3, 64, 96, 96),            # GCSL_MAX_BLK, every lane a class
    two_column_batches=(32, 2, 5, 520, 520),     # more than 512 rows: the general column path; contraction ranges 160/160/160/40
)


# ------------------------------------------------------------------------------------------------ networks in float64
def _t64(x):
    return torch.tensor(np.asarray(x, F32).astype(np.float64))


def _layers(c, flat, requires_grad=False):
    return [(_t64(W).requires_grad_(requires_grad), _t64(b).requires_grad_(requires_grad))
            for W, b in omlp.unpack(np.asarray(flat, F32), c["o"], c["hidden"], c["n"])]


def _fwd(layers, x):
    h = x
    for W, b in layers[:-1]:
        h = torch.relu(h @ W.T + b)
    W, b = layers[-1]
    return h @ W.T + b


def _grad(loss, layers):
    return np.concatenate([g.numpy().ravel() for g in torch.autograd.grad(loss, [p for Wb in layers for p in Wb])])


def _batch64(batch):
    B = batch["observations"].shape[0]
    return (_t64(batch["observations"]), torch.from_numpy(np.asarray(batch["actions"]).reshape(B).astype(np.int64)),
            _t64(batch["rewards"]).reshape(B), _t64(batch["terminals"]).reshape(B), _t64(batch["next_observations"]))


def _np(rows):
    return {k: v.detach().numpy().copy() for k, v in rows.items()}


def _msmm(x):
    return np.array([x.mean(), x.std(), x.max(), x.min()])


# ------------------------------------------------------------------------------------------------ discrete SAC
def dsac_f64(c, P, batch, actor=None, wrong=None):
    """One step at the blocks P = {pi, q1, q2, tq1, tq2} on `batch`.  actor: {"q1": flat, "q2": flat}, the critics the policy loss sees (None:
    the ones in P).  Returns dict(grads {net: flat}, rows {y, qa1, qa2, ploss, ent: per row}, stats {the device's statistics}, max_q)."""
    assert wrong is None or wrong in DSAC_WRONG, wrong
    s, a, r, d, s2 = _batch64(batch)
    B, n = s.shape[0], c["n"]
    rs, gamma, alpha = (f32(c[k]) for k in ("reward_scale", "discount", "alpha"))
    T = {k: P[ONLINE_OF[k]] if wrong == "online_targets" else P[k] for k in TARGETS["dsac"]}
    if wrong == "shift_action":
        a = (a + 1) % n
    with torch.no_grad():      # y = rs r + (1 - d) gamma (sum_j p'_j min(TQ1, TQ2)(s')_j + alpha H(p')), p' = pi(s')
        lp2 = torch.log_softmax(_fwd(_layers(c, P["pi"]), s if wrong == "target_pi_s" else s2), 1)
        p2 = lp2.exp()
        tq1, tq2 = (_fwd(_layers(c, T[k]), s2) for k in ("tq1", "tq2"))
        ent2 = -(p2 * lp2).sum(1)
        v2 = (p2 * torch.min(tq1, tq2)).sum(1) + (0.0 if wrong == "no_target_entropy" else alpha) * ent2
        y = (1.0 if wrong == "no_reward_scale" else rs) * r + (1.0 if wrong == "no_done" else 1.0 - d) * gamma * v2
    grads, rows = {}, dict(y=y, tq1=tq1, tq2=tq2)
    for k in ("q1", "q2"):     # 0.5 * mean((Q_i(s)[a] - y)^2)
        lay = _layers(c, P[k], True)
        q = _fwd(lay, s)
        qa = q.gather(1, a[:, None])[:, 0]
        grads[k] = _grad((1.0 if wrong == "no_half" else 0.5) * ((qa - y) ** 2).mean(), lay)
        rows["qa" + k[1]], rows[k] = qa, q
    # the policy against the critics AFTER their update: -mean(alpha H(p) + sum_j p_j min(Q1, Q2)_j)
    post = {k: _layers(c, P[k] if actor is None or wrong == "pi_pre" else actor[k]) for k in ("q1", "q2")}
    with torch.no_grad():
        q1n, q2n = _fwd(post["q1"], s), _fwd(post["q2"], s)
        qmin = q1n if wrong == "pi_q1" else torch.min(q1n, q2n)
    lay = _layers(c, P["pi"], True)
    lp = torch.log_softmax(_fwd(lay, s), 1)
    p = lp.exp()
    ploss = -(p * (qmin - (0.0 if wrong == "no_policy_entropy" else alpha) * lp)).sum(1)
    grads["pi"] = _grad(ploss.mean(), lay)
    rows.update(ploss=ploss, ent=-(p * lp).sum(1), q1n=q1n, q2n=q2n)
    if wrong == "inv_b":
        grads = {k: g * (B / c["max_batch"]) for k, g in grads.items()}
    rows = _np(rows)
    stats = {"QF1 Loss": 0.5 * np.mean((rows["qa1"] - rows["y"]) ** 2), "QF2 Loss": 0.5 * np.mean((rows["qa2"] - rows["y"]) ** 2),
             "Policy Loss": rows["ploss"].mean(), "Q1 Predictions": _msmm(rows["qa1"]), "Q2 Predictions": _msmm(rows["qa2"])}
    return dict(grads=grads, rows=rows, stats=stats, max_q=max(float(np.abs(rows[k]).max()) for k in ("q1", "q2", "tq1", "tq2")))


# ------------------------------------------------------------------------------------------------ DQN / Double DQN
def dqn_f64(c, P, batch, actor=None, wrong=None):
    """One step at the blocks P = {q, tq}.  Returns dict(grads {"q": flat}, rows {y, qa, gap: per row}, stats, max_q); gap = the distance of
    the two largest entries of the row that is arg-maxed (TQ(s'); Double DQN: the online Q(s'))."""
    assert wrong is None or wrong in DQN_WRONG, wrong
    s, a, r, d, s2 = _batch64(batch)
    B, gamma = s.shape[0], f32(c["discount"])
    double_q = c["double_q"] != (wrong == "swap_double")
    with torch.no_grad():
        tq = _fwd(_layers(c, P["q"] if wrong == "online_targets" else P["tq"]), s2)
        qn = _fwd(_layers(c, P["q"]), s2)
        v = tq.gather(1, qn.argmax(1)[:, None])[:, 0] if double_q else tq.max(1)[0]
        y = r + (1.0 if wrong == "no_done" else 1.0 - d) * (1.0 if wrong == "no_discount" else gamma) * v
        top = torch.sort(qn if c["double_q"] else tq, 1)[0]
    lay = _layers(c, P["q"], True)
    q = _fwd(lay, s)
    qa = q.gather(1, a[:, None])[:, 0]
    g = _grad((0.5 if wrong == "half" else 1.0) * ((qa - y) ** 2).mean(), lay)      # nn.MSELoss(): the mean square, no 1/2
    if wrong == "inv_b":
        g = g * (B / c["max_batch"])
    rows = _np(dict(y=y, qa=qa, gap=top[:, -1] - top[:, -2], q=q, tq=tq, qn=qn))
    stats = {"QF Loss": np.mean((rows["qa"] - rows["y"]) ** 2), "Y Predictions": _msmm(rows["qa"])}
    return dict(grads=dict(q=g), rows=rows, stats=stats, max_q=max(float(np.abs(rows[k]).max()) for k in ("q", "tq", "qn")))


def step_f64(c, P, batch, actor=None, wrong=None):
    return (dsac_f64 if c["algo"] == "dsac" else dqn_f64)(c, P, batch, actor=actor, wrong=wrong)


def violations(c, ref, factor=1.0):
    """Per row: is the arg-maxed row's top-two distance below factor * 1e-3 * max|Q|?  dsac has no kink: min(Q1, Q2) is continuous and carries
    no gradient in either loss, so an fp32 evaluation that takes the other branch at a near-tie changes the value by the size of the tie."""
    if c["algo"] == "dsac":
        return np.zeros(ref["rows"]["y"].shape[0], bool)
    return ref["rows"]["gap"] < factor * KINK_REL * ref["max_q"]


def swap_sensitive(batch, ref):
    """Per row of a DQN step: does it tell plain from Double DQN?  A non-terminal row on which the online and the target net put their
    maxima at s' in different columns."""
    rows = ref["rows"]
    return (batch["terminals"].ravel() == 0) & (rows["qn"].argmax(1) != rows["tq"].argmax(1))


# ------------------------------------------------------------------------------------------------ inputs
def _init_block(c, net, rng):
    """A FlattenMlp / DiscretePolicy draw whose head rows are rescaled so that over N(0, 1) observations every output has a standard
    deviation of 1 around a centre of its own: critics around 1 + U(+-0.5) (max|Q| a few units at every width), the policy around 0
    (logits of spread 1: entropies well below log n)."""
    o, hidden, n = c["o"], c["hidden"], c["n"]
    p = omlp.init_mlp(rng, o, hidden, n, init_w=1e-2)
    W, b = omlp.unpack(p, o, hidden, n)[-1]                      # views into p
    y = omlp.forward(p, rng.normal(0, 1, (512, o)).astype(F32), o, hidden, n)[0][0].astype(np.float64) - b
    k = 1.0 / y.std(0)
    centre = np.zeros(n) if net == "pi" else 1.0 + rng.uniform(-0.5, 0.5, n)
    W *= k[:, None].astype(F32)
    b[:] = (centre - k * y.mean(0)).astype(F32)
    return p


def _draw_rows(c, rng, B):
    """B transitions: N(0, 1) observations and rewards, a quarter of the rows terminal (B > 1), actions that take min(n, B) distinct
    classes before they repeat"""
    o, n = c["o"], c["n"]
    act = np.concatenate([rng.permutation(n)[:min(n, B)], rng.integers(0, n, max(0, B - n))])
    done = np.zeros(B, F32)
    if B > 1:
        done[rng.permutation(B)[:max(1, round(0.25 * B))]] = 1.0
    return dict(observations=rng.normal(0, 1, (B, o)).astype(F32), actions=rng.permutation(act).astype(F32).reshape(B, 1),
                rewards=rng.normal(0, 1, (B, 1)).astype(F32), terminals=done.reshape(B, 1), next_observations=rng.normal(0, 1, (B, o)).astype(F32))


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(settings, dict(P = every block by name, batches = one dict per step)).  DQN rows that break the arg-max margin at twice its size get
    fresh observations (terminal flag and action stay, so the shares and the class cover do), at most 50 times over; so do the
    non-terminal rows of a DQN batch in which no row tells plain from Double DQN (`swap_sensitive`: what the single row of one_row needs)."""
    c = dict(ALL[name])
    rng = np.random.default_rng(c["seed"])
    P = {k: _init_block(c, k, rng) for k in NETS[c["algo"]] + TARGETS[c["algo"]]}
    batches = [_draw_rows(c, rng, B) for B in c["Bs"]]
    for batch in batches:
        for _ in range(50):
            ref = step_f64(c, P, batch)
            bad = violations(c, ref, factor=2.0)
            if c["algo"] == "dqn" and not swap_sensitive(batch, ref).any():      # one row: its two arg-maxes must differ
                bad |= batch["terminals"].ravel() == 0
            if not bad.any():
                break
            for k in ("observations", "next_observations"):
                batch[k][bad] = rng.normal(0, 1, (int(bad.sum()), c["o"])).astype(F32)
        else:
            raise AssertionError(f"{name}: rows keep breaking the arg-max margin; change the seed or the scales")
    for x in list(P.values()) + [v for b in batches for v in b.values()]:
        x.setflags(write=False)
    return c, dict(P=P, batches=batches)


# ------------------------------------------------------------------------------------------------ the fp32 witnesses
def _torch_adam_state(opt, params):
    st = [opt.state[p] for p in params]
    return (np.concatenate([s["exp_avg"].numpy().ravel() for s in st]), np.concatenate([s["exp_avg_sq"].numpy().ravel() for s in st]),
            {int(s["step"]) for s in st})


def witness_run(c, case):
    """The fp32 restatement of the algorithm run over the case's batches from the blocks P (targets included): dict(P after the run,
    m / v / steps per trainable net, stats of the FIRST step) — what the device tests read from the trainer."""
    P, kw = case["P"], dict(discount=c["discount"], soft_target_tau=c["tau"])
    if c["algo"] == "dsac":
        w = DsacRestatement(c["o"], c["hidden"], c["n"], P["pi"], P["q1"], P["q2"], reward_scale=c["reward_scale"], alpha=c["alpha"],
                            policy_lr=c["lr"], qf_lr=c["lr"], beta_1=c["beta_1"], **kw)
        w.tq1, w.tq2 = ([p.detach() for p in unflatten(P[k], c["o"], c["hidden"], c["n"])] for k in ("tq1", "tq2"))
        outs = [w.train_step(b) for b in case["batches"]]
        m, v, steps = {}, {}, {}
        for k, opt, params in (("q1", w.opt_q1, w.q1), ("q2", w.opt_q2, w.q2), ("pi", w.opt_pi, w.pi)):
            m[k], v[k], t = _torch_adam_state(opt, params)
            assert len(t) == 1
            steps[k] = t.pop()
        o0 = outs[0]
        stats = {"QF1 Loss": o0["q1_loss"], "QF2 Loss": o0["q2_loss"], "Policy Loss": o0["policy_loss"],
                 "Q1 Predictions": _msmm(o0["q1_pred"].astype(np.float64)), "Q2 Predictions": _msmm(o0["q2_pred"].astype(np.float64))}
        return dict(P={k: w.params(k) for k in NETS["dsac"] + TARGETS["dsac"]}, m=m, v=v, steps=steps, stats=stats)
    w = DqnRestatement(c["o"], c["hidden"], c["n"], P["q"], P["tq"], c["double_q"], False, c["discount"], c["lr"], c["tau"], 1, dtype=np.float32)
    outs = [w.train_step(b) for b in case["batches"]]
    stats = {"QF Loss": outs[0]["qf_loss"], "Y Predictions": _msmm(outs[0]["y_pred"].astype(np.float64))}
    return dict(P=dict(q=w.params("q"), tq=w.params("tq")), m=dict(q=w.m), v=dict(q=w.v), steps=dict(q=w.t), stats=stats)


# ------------------------------------------------------------------------------------------------ per block
def block_errors(got, ref, c):
    """[(name, max|got - ref|, max|ref|)] per parameter block (W0 b0 W1 b1 W2 b2) of a net o -> hidden -> n: ac_restatement.block_errors on
    the same flat layout"""
    return AR.block_errors(got, ref, dict(o=c["o"], a=c["n"], hidden=c["hidden"], algo="td3"), "pi")


def untaken_head_mask(c, batch):
    """flat mask of a critic's head rows (weights and bias) of the classes no row of `batch` took: their gradient is exactly zero"""
    o, hidden, n = c["o"], c["hidden"], c["n"]
    free = ~np.isin(np.arange(n), np.asarray(batch["actions"]).reshape(-1).astype(np.int64))
    m = np.zeros(omlp.n_params(o, hidden, n), bool)
    W, b = omlp.unpack(m, o, hidden, n)[-1]
    W[free], b[free] = True, True
    return m


# ------------------------------------------------------------------------------------------------ GCSL CLASS
def gcsl_dims():
    from test_gcsl_cpu import GD, O, T
    return O, GD, T


@functools.lru_cache(maxsize=None)
def gcsl_case(name):
    """(settings, p0, X [B, D], y [B]): parameters from gcsl_restatement.cat_init with the head widened (class probabilities with real spread),
    inputs whose every column varies over the batch — the horizon part is drawn at random, 0 / 1 entries, not built from a horizon — so that
    the only parameters without a gradient are the nblk * H Linear biases under a BatchNorm; labels drawn over all classes, a quarter of
    them then set to the float64 arg-max of their row."""
    H, nblk, n, B, max_rows = GCSL_CASES[name]
    O, GD, T = gcsl_dims()
    D = O + GD + T
    seed = 7400 + list(GCSL_CASES).index(name)
    rng = np.random.default_rng(seed)
    p0 = GR.cat_init(seed, D, H, nblk, n)
    p0[-(n * H + n):] *= F32(8.0 / np.sqrt(H / 64.0))
    X = np.concatenate([rng.normal(0, 1, (B, O)), rng.uniform(-1, 1, (B, GD)), (rng.random((B, T)) < 0.5)], 1).astype(F32)
    y = rng.permutation(np.concatenate([rng.permutation(n)[:min(n, B)], rng.integers(0, n, max(0, B - n))])).astype(np.int64)
    c = dict(name=name, D=D, H=H, nblk=nblk, n=n, B=B, max_rows=max_rows, lr=GCSL_LR, O=O, GD=GD, T=T)
    y[:B // 4] = gcsl_f64(c, p0, X, y)["probs"].argmax(1)[:B // 4]      # a quarter of the rows is classified rightly: Accuracy is no 0 == 0
    for x in (p0, X, y):
        x.setflags(write=False)
    return c, p0, X, y


def gcsl_f64(c, p0, X, y, wrong=None):
    return GR.CatRestatement(p0, c["D"], c["H"], c["nblk"], c["n"], lr=c["lr"], dtype=torch.float64).gradients(X, y, wrong=wrong)


def gcsl_block_errors(got, ref, c, live):
    """[(name, max|got - ref|, max|ref|)] over the live entries of every block of gcsl_restatement.layout that has one"""
    got, ref, out, off = np.asarray(got, np.float64), np.asarray(ref, np.float64), [], 0
    for nm, shape in GR.layout(c["D"], c["H"], c["nblk"], c["n"]):
        s = slice(off, off + int(np.prod(shape)))
        off = s.stop
        if live[s].any():
            out.append((nm, float(np.abs(got[s] - ref[s])[live[s]].max()), float(np.abs(ref[s])[live[s]].max())))
    assert off == got.size == ref.size
    return out
