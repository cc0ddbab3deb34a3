"""Every compiled instance of the fused filter kernels on the MI355X: the cases of tests/filter_instances_suite.py on the gfx950 library.  Run with -s, the census
prints every measured error and one `CENSUS {...}` summary line per (kind, n, dtype): the figures of docs/accuracy.md's section on the instances."""
import pytest

import filter_instances_suite as fis
from ndrustfft_amd import _lib

pytestmark = pytest.mark.gpu
DTYPES = dict(argvalues=fis.BOTH, ids=("f64", "f32"))


@pytest.fixture(scope="module")
def L():
    lib = _lib.default()                      # in-tree gfx950 build; raises if missing
    assert lib.c.ndfft_device_count() >= 1, "no MI355X visible"
    return lib


@pytest.mark.parametrize("rdt", **DTYPES)
@pytest.mark.parametrize("K,n", fis.CENSUS, ids=fis.CENSUS_IDS)
def test_census(L, K, n, rdt): fis.census(L, K, n, rdt, verbose=True)


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
