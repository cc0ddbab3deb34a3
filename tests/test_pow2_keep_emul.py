"""The kept share of a streamed input (Pow2Args::keep64) on the CPU build of the kernel sources: every forced share gives the bits of share 0, which meets
the oracle, on dense arrays and on offset views, in all four instances that carry the branch.  The claim about the GPU is tests/test_gpu_pow2_keep.py."""
import os
import subprocess

import pytest

import pow2_keep_suite as pks
import pow2_latency_suite as pls
from ndrustfft_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "emul")


@pytest.fixture(scope="module")
def L():
    if os.environ.get("NDFFT_EMUL_LIB"):
        return _lib.Library(os.path.abspath(os.environ["NDFFT_EMUL_LIB"]))
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "-j4"])
    return _lib.Library(os.path.join(EMUL_DIR, "_build", "libndfft_emul.so"))


@pytest.mark.parametrize("offset", (0, pks.OFFSET), ids=("dense", "offset"))
@pytest.mark.parametrize("rdt,n,rows,env", pks.CASES, ids=pks.IDS)
def test_every_share_gives_the_bits_of_share_zero(L, rdt, n, rows, env, offset):
    pks.identity(L, rdt, n, rows, env, lambda name, x, axis: pls.oracle_ref(name, x, axis, rdt), offset)
