"""Register class of the shipped row kernels that run in the derived latency form (pow2_config.h: pow2_row_flags): at most 64 VGPRs, 8 waves per SIMD, no
scratch -- the occupancy the HBM-bound kernel needs.  The instances come from Pow2RowKernel, the alias the launcher uses; only the compiler's
kernel-resource-usage remarks are read.  No GPU needed; skipped where there is no hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndrustfft_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# (type, n, elements per global access) of the instances in the derived latency form, both load policies each
INSTANCES = (("double", 4096, 1), ("float", 4096, 2), ("float", 4096, 1))

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def test_latency_form_instances_keep_their_register_class(tmp_path):
    tu = ['#include "pow2_config.h"', "namespace ndfft {"]
    for t, n, vec in INSTANCES:
        tu.append(f'static_assert((pow2_row_flags<{t}>({n}, false) & 96) == 96, "{t} {n} is not in the derived latency form");')
        for nt in (1, 3):
            tu.append(f"template __global__ void k_pow2<Pow2RowKernel<{t}, {n}, {nt}, {vec}>>(const Pow2Args);")
    tu.append("}")
    src = tmp_path / "row_instances.hip"
    src.write_text("\n".join(tu) + "\n")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only", "-I" + CSRC, "-c", str(src),
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}; kernels.append(cur); continue
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    assert len(kernels) == 2 * len(INSTANCES), kernels
    for k in kernels:
        print(k)
        assert k["vgpr"] <= 64 and k["occ"] == 8 and k["scratch"] == 0, k
