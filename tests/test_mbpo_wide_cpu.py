"""CPU check of the wide ensemble kernel (bnn.h k_bnn_wide, hidden widths 257..400): -Rpass-analysis=kernel-resource-usage on
ilsx_bnn.hip for gfx950.  The three instantiations (PREDICT, TRAIN, MSE) exist, use no scratch (the two accumulators of a wave keep
static register indices) and hold 8 waves per SIMD, the narrow kernel's floor: two 16 x 404 LDS tiles (51.7 KB) leave three
1024-thread workgroups per CU, so the register count decides, and it stays at or below 64."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OCCUPANCY_FLOOR = 8


def test_wide_bnn_kernels_exist_without_scratch_at_the_occupancy_floor(tmp_path):
    src = os.path.join(ROOT, "ilswiss_amd", "csrc", "ilsx_bnn.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "bnn.o")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(occ), names
    wide = [(n, s, o) for n, s, o in zip(names, scratch, occ) if "k_bnn_wide" in n]
    assert len(wide) == 3, names                       # BNN_PREDICT, BNN_TRAIN, BNN_MSE
    assert len({n for n, _, _ in wide}) == 3
    for n, s, o in wide:
        assert s == 0, (n, s)
        assert o >= OCCUPANCY_FLOOR, (n, o)
