"""ndfft_filter on real arrays on the CPU build of the kernel sources (tests/emul): the cases of tests/filter_real_suite.py -- the fused kernel, its barriers and its
mirror exchange run there thread for thread -- and the C++ mirror.  The claim about the GPU is tests/test_filter_real_gpu.py."""
import os
import subprocess

import pytest

import filter_real_suite as frs
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


@pytest.mark.parametrize("rdt", frs.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", frs.FUSED_R_N)
def test_every_instance(L, n, rdt): frs.every_instance(L, n, rdt)


@pytest.mark.parametrize("rdt", frs.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", frs.FUSED_R_N)
def test_fused_and_composed_within_the_bar(L, n, rdt): frs.working_precision(L, n, rdt)


def test_dc_and_nyquist(L): frs.dc_and_nyquist(L)
def test_weight_placement(L): frs.weight_placement(L)
def test_alignment_and_pitch(L): frs.alignment_and_pitch(L)
def test_output_window_inside_a_sentinel_allocation(L): frs.sentinel_bands(L)
def test_in_place_equals_out_of_place(L): frs.in_place(L)
def test_xcd_map_with_a_tail(L): frs.xcd_tail(L)
def test_lane_isolation(L): frs.lane_isolation(L)
def test_normalisation(L): frs.normalisation(L)
def test_layouts_and_composed_lengths(L): frs.layouts(L)


def test_cpp_mirror_against_the_cpu_build(L, tmp_path):
    """tests/cpp/test_filter_real.cpp (ndfft_filter on real DeviceArrays) linked against the CPU build of the kernel sources."""
    exe = str(tmp_path / "test_filter_real_cpu")
    libdir = os.path.dirname(L.path)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_filter_real.cpp"), "-o", exe,
                           "-L" + libdir, "-l" + os.path.basename(L.path)[3:-3], "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "test result: ok." in r.stdout, r.stdout + r.stderr
