"""What the compiler made of the shipped column instances of the fused filter (kernels_filter.hip: FilterColInst), both load policies each: no scratch, and a
tile of at most 160 KiB of dynamic LDS.  The unit itself is compiled for gfx950, so the instances are the launcher's own; only the compiler's
kernel-resource-usage remarks are read (the LDS size is the kernel struct's constant, asserted at compile time).  No GPU needed; skipped where there is no hipcc."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import filter_col_suite as fcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndrustfft_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CTYPE = {np.dtype(np.float64): "double", np.dtype(np.float32): "float"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def test_column_instances_have_no_scratch_and_fit_the_lds(tmp_path):
    tu = ['#include "kernels_filter.hip"', "namespace ndfft {"]
    for n, rdt in fcs.INSTANCES:
        t = CTYPE[np.dtype(rdt)]
        tu.append(f'static_assert(FilterColCfg<{t}, {n}>::LPB >= 4, "{t} {n} is no shipped column instance");')
        for nt in (1, 3):
            tu.append(f'static_assert(FilterColInst<{t}, {n}, {nt}>::LDS_BYTES <= 160 * 1024, "{t} {n}: the tile does not fit the LDS");')
    tu.append("}")
    src = tmp_path / "col_instances.hip"
    src.write_text("\n".join(tu) + "\n")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only", "-DNDFFT_FILTER_UNIT", "-I" + CSRC, "-c", str(src),
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            if "FilterColKernel" in cur["name"]:
                kernels.append(cur)
            continue
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    assert len(kernels) == 2 * len(fcs.INSTANCES), [k["name"] for k in kernels]
    for k in kernels:
        print(k)
        assert k["scratch"] == 0, k
