"""Stage timestamps of the merged phase kernels (k_sac_phase_a / _c) of ONE SAC step at bench.py's sizes, from the measurement build
(make STAMPS=1): per launch and per task row, the median time of every stage boundary after the launch's first workgroup start.

    python tools/phase_gantt.py

Under the rows, per launch, the hand-offs between the stages: for every consuming workgroup the time from the LAST arrival of its tile's
producers to the return of its wait.  Phase A with the target critics on rows of their own (PhaseAArgs::own_rows) has rows 5 / 6; their
hand-off is also split by the row of the workgroup they share a CU with (slot 7 of the measurement build holds XCD / CU, not a time).
ILSX_GANTT_NO_BUILD=1 with ILSX_LIB set traces that library (another commit's measurement build) instead of building this tree's.

The four stages that begin behind a wait also stamp their inner boundaries (the stage text's stamp points 1 / 2 / 3, routed to free slots of
the row, POST_WAIT below); per such row a line "after the wait" gives the median time from the wait's return to each of them.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

os.environ["ILSX_NO_GRAPH"] = "1"
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not os.environ.get("ILSX_GANTT_NO_BUILD"):
    subprocess.check_call(["make", "-C", os.path.join(_ROOT, "ilswiss_amd", "csrc"), "-j8", "STAMPS=1"], stdout=subprocess.DEVNULL)
if not (os.environ.get("ILSX_GANTT_NO_BUILD") and os.environ.get("ILSX_LIB")):
    os.environ["ILSX_LIB"] = os.path.join(_ROOT, "ilswiss_amd", "libilsx_stamps.so")
sys.path.insert(0, _ROOT)
import ilswiss_amd as ia  # noqa: E402
from ilswiss_amd import _lib  # noqa: E402

MAXWG, SLOTS, MAXL = 2048, 8, 14
ROWS_A = {0: "pi(s')", 1: "Q1 fwd, bwd", 2: "Q2 fwd, bwd", 3: "pi(s)", 5: "TQ1, own row", 6: "TQ2, own row"}
ROWS_A_OLD = {0: "pi(s') then TQ1", 1: "Q1 fwd, bwd", 2: "Q2 fwd, bwd", 3: "pi(s) then TQ2"}
ROWS_C = {0: "Q1 fwd, bwd", 1: "Q2 fwd, bwd", 2: "pi bwd"}
# (launch kind, row) -> slot of the wait's return, then (label, slot) of what follows it
POST_WAIT = {("A", 1): (3, (("head barrier", 5), ("delta_1", 6), ("delta_0 = end", 4))), ("A", 2): (3, (("head barrier", 5), ("delta_1", 6), ("delta_0 = end", 4))),
             ("A", 5): (3, (("rows staged", 1), ("layer 0", 2), ("layer 1", 6), ("end", 4))), ("A", 6): (3, (("rows staged", 1), ("layer 0", 2), ("layer 1", 6), ("end", 4))),
             ("C", 0): (2, (("head barrier", 4), ("delta_1", 5), ("delta_0", 6), ("end", 3))), ("C", 1): (2, (("head barrier", 4), ("delta_1", 5), ("delta_0", 6), ("end", 3))),
             ("C", 2): (4, (("head barrier", 1), ("delta_1", 2), ("delta_0", 3), ("end", 5)))}


def post_wait(kind, own, yy, tm):
    """tm: the row's workgroups x slots, us"""
    if (kind, yy) not in POST_WAIT or (kind == "A" and yy >= 5 and not own):
        return
    w, pts = POST_WAIT[(kind, yy)]
    out = []
    for label, sl in pts:
        ok = (tm[:, w] > 0) & (tm[:, sl] > 0)
        if ok.any():
            d = tm[ok, sl] - tm[ok, w]
            out.append(f"{label} +{np.median(d):5.2f} (max {d.max():5.2f})")
    if out:
        print(f"        after the wait (s{w}): " + "  ".join(out))


def handoff(name, tl, bx, prod, pslot, cons, cslot, s0):
    """per consuming workgroup: its wait's return minus the last arrival among its tile's producers"""
    d = []
    for w in np.flatnonzero(cons):
        p = prod & (bx == bx[w]) & (tl[:, pslot] > 0)
        if p.any() and tl[w, cslot] > 0:
            d.append(tl[w, cslot] - tl[p, pslot].max())
    if d:
        d = np.array(d)
        print(f"    hand-off {name}: last arrival -> wait returns  median {np.median(d):5.2f}  max {d.max():5.2f} us  ({d.size} workgroups;"
              f" last arrival of all @ {tl[prod & (tl[:, pslot] > 0), pslot].max() - s0:5.2f}, returns median @ {np.median(tl[cons & (tl[:, cslot] > 0), cslot]) - s0:5.2f})")
    return d
ctx = ia.Context(0, seed=0)
o, a, H, B, CAP = 11, 3, 256, 256, 100_000
rng = np.random.default_rng(0)
rows = (rng.normal(0, 1, (CAP, o)).astype(np.float32), np.tanh(rng.normal(0, 1, (CAP, a))).astype(np.float32),
        rng.normal(0, 1, CAP).astype(np.float32), rng.random(CAP) < 1e-3, rng.normal(0, 1, (CAP, o)).astype(np.float32))
rb = ia.SimpleReplayBuffer(CAP, o, a, random_seed=1, ctx=ctx)
rb.add_rows(*rows)
tr = ia.SoftActorCritic(ia.ReparamTanhMultivariateGaussianPolicy([H, H], o, a, ctx=ctx, seed=1), ia.FlattenMlp([H, H], 1, o + a, ctx=ctx, seed=2),
                        ia.FlattenMlp([H, H], 1, o + a, ctx=ctx, seed=3), policy_lr=3e-4, qf_lr=3e-4, soft_target_tau=0.005, max_batch=B)
tr.eval_statistics = {}
tr.train_from_replay(rb, 20, B)
ctx.sync()
buf = ctx.from_numpy(np.zeros((MAXL, MAXWG, SLOTS), np.int64), np.int64)
for rep in range(2):
    buf.copy_from(np.zeros((MAXL, MAXWG, SLOTS), np.int64))
    _lib.check(ctx.lib.ilsx_debug_set_stamp_buffer(ctx.h, buf.ptr, MAXL, None))
    tr.train_from_replay(rb, 3, B)
    ctx.sync()
    n = C.c_int()
    _lib.check(ctx.lib.ilsx_debug_set_stamp_buffer(ctx.h, None, 0, C.byref(n)))
    buf_raw = buf.numpy()
    t = buf_raw.astype(np.float64) * 0.01   # 100 MHz ticks -> us
    print(f"--- rep {rep}: {n.value} instrumented launches (3 steps of A D1 C D2)")
    base = None
    for L in range(4, min(n.value, 8)):
        live = np.flatnonzero(t[L][:, 0] > 0)
        if not live.size:
            continue
        s0 = t[L][live, 0].min()
        if base is None:
            base = s0
        kind = "ACAC"[L % 4] if False else ("A", "D1", "C", "D2")[L % 4]
        print(f"launch {L} ({kind}): {live.size} workgroups, begins {s0 - base:7.2f} us after the step's first launch")
        if kind in ("A", "C"):
            own = kind == "A" and live.max() >= 16 * 5 * 4   # grid.y = 7: the target critics on rows of their own
            ny = (7 if own else 5) if kind == "A" else 4
            names = (ROWS_A if own else ROWS_A_OLD) if kind == "A" else ROWS_C
            y = (live // 16) % ny
            cu = buf_raw[L][live, 7]
            has_cu = bool(((cu >> 16) == 1).all())   # slot 7 of the measurement build: 0x10000 | XCD << 8 | SE / SH / CU, not a time
            for yy in sorted(names):
                m = live[y == yy]
                row = []
                for sl in range(7 if has_cu else 8):
                    v = t[L][m, sl]
                    ok = v > 0
                    if ok.any():
                        row.append(f"s{sl}@{np.median(v[ok]) - s0:6.2f}(max {v[ok].max() - s0:6.2f})")
                print(f"    task row {yy} ({names[yy]}): " + "  ".join(row))
                post_wait(kind, own, yy, t[L][m])
                if kind == "A" and yy in (1, 2):     # fine build: slots 5 / 6 hold the shader clock at the same two points as stamps 0 / 4
                    raw = buf_raw[L][m]
                    ok = (raw[:, 5] > 0) & (raw[:, 6] > 0) & (raw[:, 4] > 0)
                    if ok.any() and (raw[ok, 6] - raw[ok, 5]).min() > 2 * (raw[ok, 4] - raw[ok, 0]).max():   # (the plain build stamps the head's boundaries there)
                        cyc = (raw[ok, 6] - raw[ok, 5]).astype(np.float64)
                        us = (raw[ok, 4] - raw[ok, 0]).astype(np.float64) * 0.01
                        print(f"        shader clock over the workgroup's life: {np.median(cyc / us):.0f} MHz (s_memtime cycles / 100 MHz stamps)")
            tl, bx = t[L][live], live % 16
            if kind == "A":
                tq = (y >= 5) if own else ((y == 0) | (y == 3))
                handoff("pi(s') -> target critics", tl, bx, y == 0, 2, tq, 3, s0)
                if own and has_cu:
                    for part, label in ((1, "a critic row (1 / 2)"), (0, "a policy row (0 / 3)"), (-1, "no stage-1 workgroup")):
                        sel = np.zeros(live.size, bool)
                        for w in np.flatnonzero(tq):
                            mates = y[(cu == cu[w]) & (y < 5)]
                            kind_w = -1 if not mates.size else (1 if ((mates == 1) | (mates == 2)).any() else 0)
                            sel[w] = kind_w == part
                        if sel.any():
                            handoff(f"    ... sharing a CU with {label}", tl, bx, y == 0, 2, sel, 3, s0)
                handoff("target critics -> critics' backward", tl, bx, tq, 5, (y == 1) | (y == 2), 3, s0)
            else:
                handoff("Q forward -> Q backward", tl, bx, y < 2, 1, y < 2, 2, s0)
                handoff("Q backward -> pi backward", tl, bx, y < 2, 3, y == 2, 4, s0)
        else:
            e = t[L][live, 7]
            p1, p2 = t[L][live, 1], t[L][live, 2]
            print(f"    span {e.max() - s0:6.2f}   workgroup starts: median {np.median(t[L][live, 0]) - s0:5.2f} max {t[L][live, 0].max() - s0:5.2f};  "
                  f"operands + MFMA done @ {np.median(p1) - s0:5.2f} (max {p1.max() - s0:5.2f});  partials in LDS @ {np.median(p2) - s0:5.2f} (max {p2.max() - s0:5.2f});  "
                  f"end median {np.median(e) - s0:5.2f}")
    nxt = np.flatnonzero(t[8][:, 0] > 0)
    if nxt.size and base is not None:
        print(f"    step: {t[8][nxt, 0].min() - base:.2f} us from A to the next A")
