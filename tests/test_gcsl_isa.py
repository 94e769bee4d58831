"""Guards on the COMPILED GCSL kernels (no GPU needed: hipcc -S), in the style of test_dsac_isa.py: the horizon gather and every
instance of the BN launcher kernels in ilsx_gcsl.hip keep no scratch (private segment 0, no scratch_* instructions) and no indexed
registers.  The BatchNorm discriminator's launcher moved from ilsx_disc.hip into disc_bn_launch.h: every kernel of ilsx_disc.hip compiles to
the same instructions as at the commit before that move (read from git history), and the copy of k_dbn_gemm that ilsx_gcsl.hip
instantiates in its own namespace compiles to the same code as the discriminator's."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


CSRC = os.path.join(ROOT, "ilswiss_amd", "csrc")


def _kernels(src):
    d = tempfile.mkdtemp(prefix="isa_")
    out = os.path.join(d, "k.s")
    try:
        r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                            "-I", CSRC, src if os.path.isabs(src) else os.path.join(CSRC, src), "-o", out], capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out).read().split("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    ks = {}
    for i, l in enumerate(text):
        m = re.match(r"^(_Z\w+):\s", l)
        if not m:
            continue
        dn = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        end = next(j for j in range(i, len(text)) if text[j].startswith(".Lfunc_end"))
        ops = [re.sub(r"\.LBB\d+_", ".LBB_", x.split(";")[0].strip()) for x in text[i + 1:end]
               if x.strip() and not x.lstrip().startswith((";", "."))]   # block labels carry the function's ordinal: normalised
        meta = "\n".join(text[end:end + 150])
        priv = re.search(r"\.private_seg_size, (\d+)", meta)
        ks[dn] = (ops, int(priv.group(1)) if priv else None)
    return ks


@pytest.fixture(scope="module")
def gcsl_k():
    return _kernels("ilsx_gcsl.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_new_kernels_have_no_scratch_and_no_indexed_registers(gcsl_k):
    names = [k for k in gcsl_k if "k_her_horizon_gather" in k or "gcsl_dev::" in k]
    assert any("k_her_horizon_gather" in k for k in names) and any("k_dbn_gemm" in k for k in names)
    assert sum("k_dbn_col" in k for k in names) >= 5
    for k in names:
        ops, priv = gcsl_k[k]
        assert priv == 0 and not any(o.startswith("scratch_") for o in ops), (k, priv)
        assert not any(o.startswith("s_set_gpr_idx") or "movrel" in o for o in ops), k


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_shared_launcher_compiles_to_the_same_code(gcsl_k):
    disc = _kernels("ilsx_disc.hip")
    a = next(v for k, v in disc.items() if k.startswith("k_dbn_gemm("))
    b = next(v for k, v in gcsl_k.items() if "gcsl_dev::k_dbn_gemm(" in k)
    assert a[1] == 0 and a[0] == b[0]


def _disc_before_the_move():
    """ilsx_disc.hip as it was before disc_bn_launch.h existed: at the parent of the commit that added the header, or at HEAD while the
    header is not committed yet.  None without git history."""
    def git(*a):
        r = subprocess.run(["git", "-C", ROOT, *a], capture_output=True, text=True)
        return r.stdout if r.returncode == 0 else None
    if git("rev-parse", "--git-dir") is None:
        return None
    added = (git("log", "--diff-filter=A", "--format=%H", "--", "ilswiss_amd/csrc/disc_bn_launch.h") or "").split()
    rev = added[-1] + "^" if added else "HEAD"
    return git("show", f"{rev}:ilswiss_amd/csrc/ilsx_disc.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("git") is None, reason="no hipcc / git")
def test_discriminator_kernels_unchanged_by_the_launcher_move():
    old = _disc_before_the_move()
    if old is None:
        pytest.skip("no git history in this checkout")
    assert "struct DbnLaunch" in old            # the launcher was still inline there
    # The old text compiles against today's headers.  One HOST signature it calls has changed since: launch_bwd_dw takes the owner of the
    # gradient arena (host_common.h).  The old calls get one; the kernels under comparison are device code and do not see it.
    inc = '#include "host_common.h"\n'
    assert old.count(inc) == 1
    old = old.replace(inc, inc + "static DevOwner owner_of_the_old_text;\n"
                      "#define launch_bwd_dw(ctx, ...) launch_bwd_dw(ctx, owner_of_the_old_text, __VA_ARGS__)\n")
    d = tempfile.mkdtemp(prefix="isa_old_")
    try:
        path = os.path.join(d, "ilsx_disc_before.hip")
        with open(path, "w") as f:
            f.write(old)
        before = _kernels(path)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    now = _kernels("ilsx_disc.hip")
    assert sorted(before) == sorted(now)
    changed = [k for k in now if now[k] != before[k]]
    assert not changed, changed[:5]
