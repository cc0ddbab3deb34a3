"""ndfft_filter along a strided axis on the CPU build of the kernel sources (tests/emul): the cases of tests/filter_col_suite.py -- the column form of the fused
kernel runs there thread for thread -- and the C++ mirror.  The claim about the GPU is tests/test_filter_col_gpu.py."""
import os
import subprocess

import pytest

import filter_col_suite as fcs
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


@pytest.mark.parametrize("n,rdt", fcs.INSTANCES, ids=fcs.INSTANCE_IDS)
def test_every_instance(L, n, rdt): fcs.every_instance(L, n, rdt)


@pytest.mark.parametrize("n,rdt", fcs.INSTANCES, ids=fcs.INSTANCE_IDS)
def test_against_composed_within_the_bar(L, n, rdt): fcs.against_composed(L, n, rdt)


@pytest.mark.parametrize("n,rdt", fcs.INSTANCES, ids=fcs.INSTANCE_IDS)
def test_both_load_policies(L, n, rdt): fcs.both_policies(L, n, rdt)


def test_two_batch_dims(L): fcs.two_batch_dims(L)
def test_windows_inside_sentinel_allocations(L): fcs.guarded_windows(L)
def test_in_place_equals_out_of_place(L): fcs.in_place(L)
def test_weight_placement(L): fcs.weight_placement(L)
def test_lane_isolation_inside_a_tile(L): fcs.lane_isolation(L)
def test_xcd_map_with_a_tail(L): fcs.xcd_tail(L)
def test_normalisation(L): fcs.normalisation(L)
def test_declined_still_correct(L): fcs.declined(L)


def test_cpp_mirror_against_the_cpu_build(L, tmp_path):
    """tests/cpp/test_filter_col.cpp (ndfft_filter on DeviceArrays along axis 0) linked against the CPU build of the kernel sources."""
    exe = str(tmp_path / "test_filter_col_cpu")
    libdir = os.path.dirname(L.path)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_filter_col.cpp"), "-o", exe,
                           "-L" + libdir, "-l" + os.path.basename(L.path)[3:-3], "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "test result: ok." in r.stdout, r.stdout + r.stderr
