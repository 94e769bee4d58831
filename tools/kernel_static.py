#!/usr/bin/env python
"""Static footprint of the hot kernels, without a GPU: hipcc -S of one translation unit, then per kernel the instruction count, the
scalar-spill traffic (v_writelane / v_readlane), MFMA count, registers and private-segment size.  With one wave per SIMD a kernel's
lifetime is ~4 cycles x the instructions a wave issues, so these counts are the first thing to look at after a
kernel edit; round 2 found three regressions this way (a 68-byte private segment left by a shared lambda, 395 spill instructions caused
by the trace pointer, ~90 branchy instructions per element in a predicated staging loop).

    python tools/kernel_static.py [ilsx_core.hip] [name-filter ...]

Under a kernel that polls (the merged phase kernels) one line per POST-WAIT WINDOW: the text from a stage's last poll loop (s_sleep) to the next
v_mfma — what a wave has to get through between the return of its wait and its first matrix instruction — with the window's instruction
count, scalar loads, `s_waitcnt lgkmcnt` and scalar branches (head_windows; tests/test_phase_static_heads.py holds these against the
counts of the commit before the static heads, tests/golden/phase_head_counts_parent.json).

    python tools/kernel_static.py --asm dev.s --heads-json     # scan an assembly file instead of compiling; the windows as JSON
"""
import os
import re
import subprocess
import sys
import json
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_asm(src):
    out = os.path.join(tempfile.mkdtemp(prefix="kstat_"), "dev.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only",
                           "-S", os.path.join(ROOT, "ilswiss_amd", "csrc", src), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def kernel_bodies(text):
    """(demangled name, instruction lines, metadata text) of every kernel in an assembly listing (list of lines)"""
    demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()   # noqa: E731
    for i, name in [(i, m.group(1)) for i, l in enumerate(text) for m in [re.match(r"^(_Z\w+):\s", l)] if m]:
        end = next(j for j in range(i, len(text)) if text[j].startswith(".Lfunc_end"))
        body = [l for l in text[i + 1:end] if l.strip() and not l.lstrip().startswith((";", "."))]
        yield demangle(name), body, "\n".join(text[end:end + 150])


def head_windows(body):
    """The post-wait windows of a kernel's instruction lines, in textual order: from the LAST s_sleep before a v_mfma to that v_mfma.
    polls = s_sleep lines since the previous window (a poll loop is unrolled, and waits in series add up: the stage behind more waits
    has more)."""
    out, polls, start = [], 0, None
    for n, l in enumerate(body):
        if "s_sleep" in l:
            polls += 1
            start = n
        elif "v_mfma" in l and start is not None:
            w = body[start:n]
            out.append(dict(polls=polls, instr=len(w), s_load=sum("s_load_" in x for x in w),
                            lgkm=sum("s_waitcnt" in x and "lgkmcnt" in x for x in w), branch=sum(bool(re.match(r"\s*s_c?branch", x)) for x in w)))
            polls, start = 0, None
    return out


def main():
    args = sys.argv[1:]
    asm = None
    if "--asm" in args:
        asm = args[args.index("--asm") + 1]
        del args[args.index("--asm"):args.index("--asm") + 2]
    heads_json = "--heads-json" in args
    args = [a for a in args if a != "--heads-json"]
    if heads_json:   # the constant-table instances of the 256-wide phase kernels: what the static-heads test compares
        text = open(asm).read().split("\n") if asm else compile_asm("ilsx_core.hip")
        res = {dn: dict(total=len(body), windows=head_windows(body)) for dn, body, _ in kernel_bodies(text)
               if re.match(r"void k_sac_phase_[ac]<256, [^,]+, 4, true>", dn)}
        print(json.dumps(res, indent=1, sort_keys=True))
        return
    src = args[0] if args and args[0].endswith(".hip") else "ilsx_core.hip"
    filters = [a for a in args if not a.endswith(".hip")] or ["k_mlp2_fwd_split<256, 0, 4", "k_mlp2_bwd_split<256, 0, 4", "k_mlp_bwd_dw", "k_sac_phase_a<256, 0, 4", "k_sac_phase_c<256, 0, 4",
                                                                   "k_sac_phase_a<128, 0, 2", "k_sac_phase_c<128, 0, 2"]
    text = open(asm).read().split("\n") if asm else compile_asm(src)
    print(f"{'kernel':78s} {'instr':>6s} {'mfma':>5s} {'wlane':>6s} {'rlane':>6s} {'vgpr':>5s} {'agpr':>5s} {'priv':>5s}")
    for dn, body, meta in kernel_bodies(text):
        if not any(f in dn for f in filters):
            continue
        g = lambda pat: (re.search(pat, meta) or [None, "?"])[1]   # noqa: E731
        vg, ag, pv = g(r"\.num_vgpr, (\d+)"), g(r"\.num_agpr, (\d+)"), g(r"\.private_seg_size, (\d+)")
        cnt = lambda w: sum(w in l for l in body)   # noqa: E731
        print(f"{dn[:78]:78s} {len(body):6d} {cnt('v_mfma'):5d} {cnt('v_writelane'):6d} {cnt('v_readlane'):6d} {vg:>5s} {ag:>5s} {pv:>5s}")
        for w in head_windows(body):
            print(f"    post-wait window (behind {w['polls']:2d} s_sleep): {w['instr']:5d} instr  {w['s_load']:4d} s_load  {w['lgkm']:4d} lgkmcnt waits  {w['branch']:4d} branches")


if __name__ == "__main__":
    main()
