"""NORM_NONE / NORM_DEFAULT / NORM_SCALE on the MI355X (tests/norm_suite.py; docs/accuracy.md, "Normalisation modes"): every case of
parity_suite.ACC_GPU_FAMILIES through ndfft_exec_device under the modes -- route, P1 or P2 / P3 / P5, no tolerance anywhere -- the working-precision bar on
(SCALE, 0.37) on the first small case of each (route, op, dtype), and the host-array and sharded entry points."""
import pytest

import norm_suite as ns
import parity_suite as ps
from ndrustfft_amd import _lib

pytestmark = pytest.mark.gpu

_SEEN = {}      # (family, dt) / "extra" -> the records of its cases (test_every_required_route_ran_a_scaling_op)


@pytest.fixture(scope="module")
def L():
    lib = _lib.default()                      # in-tree gfx950 build; raises if missing
    assert lib.c.ndfft_device_count() >= 1, "no MI355X visible"
    return lib


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("family", list(ps.ACC_GPU_FAMILIES))
def test_modes_on_every_case(L, family, dt):
    """Every case of the family: 6 to 8 device calls, byte and element comparisons; P4 where norm_suite.gpu_cases says.  Each P4 figure is printed first."""
    _SEEN[family, dt] = ns.gpu_cases(L, ps.acc_gpu_cases(family, dt), tag=family)


def test_modes_on_the_extra_cases(L):
    """The (route, op, dtype) whose family cases are all too large for a long-double truth, at a small shape."""
    _SEEN["extra"] = ns.gpu_cases(L, ns.GPU_EXTRA, tag="extra")


def test_every_required_route_ran_a_scaling_op(L):
    """From the last_path() values seen: every route of ACC_REQUIRED_ROUTES ran P2 with an inverse or a real op, and every (route, op, dtype) that ran P2 also
    ran P4 (a family that has not run in this session runs here)."""
    for family in ps.ACC_GPU_FAMILIES:
        for dt in ("f64", "f32"):
            if (family, dt) not in _SEEN:
                _SEEN[family, dt] = ns.gpu_cases(L, ps.acc_gpu_cases(family, dt), verbose=False)
    if "extra" not in _SEEN:
        _SEEN["extra"] = ns.gpu_cases(L, ns.GPU_EXTRA, verbose=False)
    missing, no_p4 = ns.coverage([r for recs in _SEEN.values() for r in recs])
    assert not missing, f"routes that never ran P2 with a scaling op: {missing}"
    assert not no_p4, f"(route, op, dtype) that ran P2 but have no case small enough for P4: {no_p4}"


@pytest.mark.parametrize("case", ns.HOST_CASES, ids=[f"{c[0]}-{c[2]}-{'x'.join(map(str, c[3]))}" for c in ns.HOST_CASES])
def test_ndfft_exec_on_host_arrays(L, case):
    ns.host_case(L, case)


def test_ndfft_exec_on_pinned_arrays(L):
    ns.host_case(L, ns.HOST_PINNED_CASE, pinned=True)


@pytest.mark.parametrize("case", ns.SHARDED_CASES, ids=[c[0] for c in ns.SHARDED_CASES])
def test_sharded_entry_points(L, case):
    ns.sharded_case(L, case, [0, 0], 0)
