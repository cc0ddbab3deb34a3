"""ndfft_filter on the CPU build of the kernel sources (tests/emul): the cases of tests/filter_suite.py -- the fused kernel runs there thread for thread -- the
bound symbol, and the C++ mirror.  The claim about the GPU is tests/test_filter_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import filter_suite as fs
from ndrustfft_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL_DIR = os.path.join(HERE, "emul")


@pytest.fixture(scope="module")
def L():
    if os.environ.get("NDFFT_EMUL_LIB"):
        return _lib.Library(os.path.abspath(os.environ["NDFFT_EMUL_LIB"]))
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "-j4"])
    return _lib.Library(os.path.join(EMUL_DIR, "_build", "libndfft_emul.so"))


@pytest.mark.parametrize("rdt", fs.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", fs.FUSED_N)
def test_fused_every_instance(L, n, rdt): fs.fused_instance(L, n, rdt)


@pytest.mark.parametrize("rdt", fs.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", fs.FUSED_N)
def test_fused_against_composed_within_the_bar(L, n, rdt): fs.fused_against_composed(L, n, rdt)


def test_f32_without_16_byte_accesses(L): fs.f32_unaligned(L)
def test_xcd_map_with_a_tail(L): fs.xcd_tail(L)
def test_output_view_inside_a_sentinel_allocation(L): fs.guarded_output(L)
def test_in_place_equals_out_of_place(L): fs.in_place(L)
def test_weight_placement(L): fs.weight_placement(L)
def test_conjugate_symmetric_weights_keep_real_input_real(L): fs.conjugate_symmetric_weights(L)
def test_normalisation(L): fs.normalisation(L)
def test_lane_isolation(L): fs.lane_isolation(L)


@pytest.mark.parametrize("rdt", fs.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", (6, 9, 96, 100, 1000, 8192, 16384))
def test_composed_c2c_rows(L, n, rdt): fs.composed_c2c_rows(L, n, rdt)


def test_composed_c2c_layouts_views_and_peeling(L): fs.composed_c2c_layouts(L)


@pytest.mark.parametrize("rdt", fs.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", (8, 9, 64, 1000, 1001))
def test_composed_r2c(L, n, rdt): fs.composed_r2c(L, n, rdt)


def test_errors(L): fs.errors(L)


def test_filter_symbols_bound(L):
    assert _lib.FILTER_SYMBOLS == ["ndfft_exec_filter_device"]
    for s in _lib.FILTER_SYMBOLS:
        assert hasattr(L.c, s)
    assert L.c.ndfft_abi_minor() >= 5


def test_cpp_mirror_against_the_cpu_build(L, tmp_path):
    """tests/cpp/test_filter.cpp (ndfft_filter on DeviceArrays) linked against the CPU build of the kernel sources."""
    exe = str(tmp_path / "test_filter_cpu")
    libdir = os.path.dirname(L.path)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_filter.cpp"), "-o", exe,
                           "-L" + libdir, "-l" + os.path.basename(L.path)[3:-3], "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "test result: ok." in r.stdout, r.stdout + r.stderr
