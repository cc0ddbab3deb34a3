"""Every compiled instance of the fused filter kernels on the CPU build of the kernel sources (tests/emul): the cases of tests/filter_instances_suite.py.  The
emulation speaks for the launcher's choice of instance, the staging indices and the tables of every (kind, n, dtype, VEC, NT); the claim about the gfx950 code is
tests/test_filter_instances_gpu.py."""
import os
import subprocess

import pytest

import filter_instances_suite as fis
from ndrustfft_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "emul")
DTYPES = dict(argvalues=fis.BOTH, ids=("f64", "f32"))


@pytest.fixture(scope="module")
def L():
    if os.environ.get("NDFFT_EMUL_LIB"):
        return _lib.Library(os.path.abspath(os.environ["NDFFT_EMUL_LIB"]))
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "-j4"])
    return _lib.Library(os.path.join(EMUL_DIR, "_build", "libndfft_emul.so"))


@pytest.mark.parametrize("rdt", **DTYPES)
@pytest.mark.parametrize("K,n", fis.CENSUS, ids=fis.CENSUS_IDS)
def test_census(L, K, n, rdt): fis.census(L, K, n, rdt)


@pytest.mark.parametrize("rdt", **DTYPES)
@pytest.mark.parametrize("K", fis.KINDS, ids=repr)
def test_in_place_under_input_cold(L, K, rdt): fis.in_place_cold(L, K, rdt)


@pytest.mark.parametrize("which", sorted(fis.FORCED))
def test_forced_streaming_on_pitched_views(L, which): fis.forced_streaming(L, which)


def test_hint_and_switch_are_back_at_their_defaults(L): fis.defaults_in_force(L)


@pytest.mark.parametrize("rdt", **DTYPES)
@pytest.mark.parametrize("K", fis.KINDS, ids=repr)
def test_one_dimensional(L, K, rdt): fis.one_dimensional(L, K, rdt)


@pytest.mark.parametrize("rdt", **DTYPES)
@pytest.mark.parametrize("K", fis.KINDS, ids=repr)
def test_three_d_contiguous_is_fused(L, K, rdt): fis.three_d_contiguous(L, K, rdt)


@pytest.mark.parametrize("rdt", **DTYPES)
@pytest.mark.parametrize("K", fis.KINDS, ids=repr)
def test_three_d_window_is_composed(L, K, rdt): fis.three_d_window(L, K, rdt)


@pytest.mark.parametrize("rdt", **DTYPES)
@pytest.mark.parametrize("K", fis.KINDS, ids=repr)
def test_six_d_stepped_is_peeled_and_composed(L, K, rdt): fis.six_d_stepped(L, K, rdt)


@pytest.mark.parametrize("rdt", **DTYPES)
@pytest.mark.parametrize("K", fis.KINDS, ids=repr)
def test_zero_extent_batch_dim(L, K, rdt): fis.zero_extent(L, K, rdt)


@pytest.mark.parametrize("K,n,rdt", fis.RACES, ids=fis.RACE_IDS)
def test_first_filter_call_of_a_shared_plan_from_many_threads(L, K, n, rdt): fis.first_call_race(L, K, n, rdt)
