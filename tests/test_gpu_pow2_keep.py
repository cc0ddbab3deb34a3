"""The kept share of a streamed input (Pow2Args::keep64) on the MI355X: every forced share gives the bits of share 0, which meets numpy, on dense arrays and
on offset views, in all four instances that carry the branch."""
import pytest

import pow2_keep_suite as pks
import pow2_latency_suite as pls
from ndrustfft_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    lib = _lib.default()                      # in-tree gfx950 build; raises if missing
    assert lib.c.ndfft_device_count() >= 1, "no MI355X visible"
    return lib


@pytest.mark.parametrize("offset", (0, pks.OFFSET), ids=("dense", "offset"))
@pytest.mark.parametrize("rdt,n,rows,env", pks.CASES, ids=pks.IDS)
def test_every_share_gives_the_bits_of_share_zero(L, rdt, n, rows, env, offset):
    pks.identity(L, rdt, n, rows, env, pls.numpy_ref, offset)
