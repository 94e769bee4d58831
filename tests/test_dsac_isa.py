"""Guards on the COMPILED discrete-SAC kernels (no GPU needed: hipcc -S), in the style of test_isa_guards.py: the CartPole stepper and reset,
the discrete random-action draw, the categorical head and the two fused loss kernels keep no scratch (private segment 0, no scratch_*
instructions) and no indexed registers (s_set_gpr_idx / movrel)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = {"ilsx_env.hip": ("k_cartpole_step", "k_cartpole_reset", "k_random_discrete_actions"),
           "ilsx_ac.hip": ("k_categorical_act", "k_categorical_log_softmax", "k_dsac_critic_grad", "k_dsac_policy_grad")}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("src", sorted(KERNELS))
def test_new_kernels_have_no_scratch_and_no_indexed_registers(src):
    out = os.path.join(tempfile.mkdtemp(prefix="isa_"), "k.s")
    try:
        r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "ilswiss_amd", "csrc", src), "-o", out], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out).read().split("\n")
        seen = set()
        for i, l in enumerate(text):
            m = re.match(r"^(_Z\w+):\s", l)
            if not m:
                continue
            dn = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            name = next((k for k in KERNELS[src] if dn.startswith(k + "(") or dn.startswith("void " + k + "(")), None)
            if name is None:
                continue
            end = next(j for j in range(i, len(text)) if text[j].startswith(".Lfunc_end"))
            ops = [x.split()[0] for x in text[i + 1:end] if x.strip() and not x.lstrip().startswith((";", "."))]
            meta = "\n".join(text[end:end + 150])
            priv = int(re.search(r"\.private_seg_size, (\d+)", meta).group(1))
            assert priv == 0 and not any(o.startswith("scratch_") for o in ops), (name, priv)
            assert not any(o.startswith("s_set_gpr_idx") or "movrel" in o for o in ops), name
            seen.add(name)
        assert seen == set(KERNELS[src]), seen
    finally:
        shutil.rmtree(os.path.dirname(out), ignore_errors=True)
