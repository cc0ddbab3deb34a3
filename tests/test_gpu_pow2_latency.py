"""The derived latency form of the row kernel (pow2_kernel.h FLAGS bits 5 + 6) on the MI355X: route, load policy, every lane against numpy, the accuracy
bar, and the plain-load instance against the streaming-load one bit for bit -- on dense arrays and on views whose row pitch exceeds n."""
import numpy as np
import pytest

import pow2_latency_suite as pls
from ndrustfft_amd import _lib

pytestmark = pytest.mark.gpu
IDS = [f"{np.dtype(dt).name}-{n}" for dt, n in pls.LENGTHS]
PITCHED = pytest.mark.parametrize("pitched", (False, True), ids=("dense", "pitched"))


@pytest.fixture(scope="module")
def L():
    lib = _lib.default()                      # in-tree gfx950 build; raises if missing
    assert lib.c.ndfft_device_count() >= 1, "no MI355X visible"
    return lib


@PITCHED
@pytest.mark.parametrize("rdt,n", pls.LENGTHS, ids=IDS)
def test_five_lanes_forward_and_inverse(L, rdt, n, pitched):
    pls.parity(L, 5, n, rdt, pls.numpy_ref, pitched=pitched)


@pytest.mark.parametrize("rdt,n", pls.LENGTHS, ids=IDS)
def test_five_lanes_base_one_element_into_the_allocation(L, rdt, n):
    """f32: lanes aligned to 8 bytes only run the instance with one element per global access."""
    pls.parity(L, 5, n, rdt, pls.numpy_ref, offset=1)


@pytest.mark.parametrize("rdt,n", pls.LENGTHS, ids=IDS)
def test_five_lanes_working_precision(L, rdt, n):
    pls.accuracy_bar(L, 5, n, rdt)


@PITCHED
def test_xcd_lane_map_with_ragged_tail(L, pitched):
    """130 one-lane workgroups: the smallest count at which the XCD lane map engages (>= 128 blocks), two whole groups and a tail of two on the identity map."""
    pls.parity(L, 130, 4096, np.float64, pls.numpy_ref, names=("ndfft",), pitched=pitched)
