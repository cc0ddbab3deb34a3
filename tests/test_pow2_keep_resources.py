"""Register class of the streaming-load row kernels with a kept share (NT = 7), which carry the per-lane choice between the two load policies
(Pow2Args::keep64, pow2_kernel.h: run): every instance has the VGPR count, the waves per SIMD and the zero scratch of the streaming-load instance without
the choice (NT = 3) at the commit before the kept share -- the numbers in PARENT, read from this translation unit with NT = 3 compiled against that commit's
kernel headers -- and today's NT = 3 instances, which carry no choice, still have them too.  Only the compiler's
kernel-resource-usage remarks are read.  No GPU needed; skipped where there is no hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndrustfft_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# (type, n, elements per global access, PSPLIT as shipped) -> (VGPRs, waves per SIMD) of the NT = 3 instance at the parent commit
PARENT = {
    ("double", 512, 1, 1): (62, 8),
    ("double", 4096, 1, 1): (62, 8),
    ("double", 8192, 1, 1): (124, 4),
    ("float", 4096, 2, 1): (60, 8),
    ("float", 4096, 1, 1): (60, 8),
    ("float", 8192, 2, 2): (61, 8),
    ("float", 8192, 1, 2): (60, 8),
}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def resources(csrc, tmp_path, nt=7):
    """{instance: (VGPRs, waves per SIMD, scratch bytes per lane)} of the NT = `nt` instances compiled against the headers in `csrc`."""
    tu = ['#include "pow2_config.h"', "namespace ndfft {"]
    for t, n, vec, ps in PARENT:
        tu.append(f'static_assert(Pow2PSplit<{t}, {n}>::value == {ps}, "{t} {n}: not the shipped PSPLIT");')
        tu.append(f"template __global__ void k_pow2<Pow2RowKernel<{t}, {n}, {nt}, {vec}, false, {ps}>>(const Pow2Args);")
    tu.append("}")
    src = tmp_path / "keep_instances.hip"
    src.write_text("\n".join(tu) + "\n")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only", "-I" + csrc, "-c", str(src),
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {}; kernels.append(cur); continue
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    assert len(kernels) == len(PARENT), kernels          # (the remarks come in the order of the instantiations)
    return {inst: (k["vgpr"], k["occ"], k["scratch"]) for inst, k in zip(PARENT, kernels)}


@pytest.mark.parametrize("nt", (7, 3), ids=("kept-share", "streaming"))
def test_streaming_instances_keep_the_parents_register_class(tmp_path, nt):
    got = resources(CSRC, tmp_path, nt)
    bad = []
    for inst, (vgpr, occ) in PARENT.items():
        print(inst, got[inst], "parent", (vgpr, occ))
        if got[inst] != (vgpr, occ, 0):
            bad.append(f"{inst}: {got[inst][0]} VGPRs, {got[inst][1]} waves per SIMD, {got[inst][2]} B scratch; the parent has {vgpr} VGPRs, {occ} waves, 0 B")
    assert not bad, "\n".join(bad)
