"""The derived latency form of the row kernel (pow2_kernel.h FLAGS bits 5 + 6) on the CPU build of the kernel sources: (3, n) lanes of every length
pow2_config.h runs in this form, against the oracle and under the accuracy bar.  The claim about the GPU is tests/test_gpu_pow2_latency.py."""
import os
import subprocess

import numpy as np
import pytest

import pow2_latency_suite as pls
from ndrustfft_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "emul")
IDS = [f"{np.dtype(dt).name}-{n}" for dt, n in pls.LENGTHS]


@pytest.fixture(scope="module")
def L():
    if os.environ.get("NDFFT_EMUL_LIB"):
        return _lib.Library(os.path.abspath(os.environ["NDFFT_EMUL_LIB"]))
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "-j4"])
    return _lib.Library(os.path.join(EMUL_DIR, "_build", "libndfft_emul.so"))


@pytest.mark.parametrize("rdt,n", pls.LENGTHS, ids=IDS)
def test_forward_and_inverse_against_the_oracle_both_policies(L, rdt, n):
    pls.parity(L, 3, n, rdt, lambda name, x, axis: pls.oracle_ref(name, x, axis, rdt))


@pytest.mark.parametrize("rdt,n", pls.LENGTHS, ids=IDS)
def test_base_one_element_into_the_allocation(L, rdt, n):
    pls.parity(L, 3, n, rdt, lambda name, x, axis: pls.oracle_ref(name, x, axis, rdt), offset=1)


@pytest.mark.parametrize("rdt,n", pls.LENGTHS, ids=IDS)
def test_working_precision_both_policies(L, rdt, n):
    pls.accuracy_bar(L, 3, n, rdt)
