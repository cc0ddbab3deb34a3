"""nddct_filter on the CPU build of the kernel sources (tests/emul): the cases of tests/filter_dct_suite.py -- the fused kernel, its staging barriers and its mirror
exchange run there thread for thread -- the host path of api.nddct_filter, and the C++ mirror.  The claim about the GPU is tests/test_filter_dct_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import filter_dct_suite as fds
from helpers import TOL, assert_close
from ndrustfft_amd import _lib, api, handlers
from ndrustfft_amd.handlers import Normalization

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL_DIR = os.path.join(HERE, "emul")


@pytest.fixture(scope="module")
def L():
    if os.environ.get("NDFFT_EMUL_LIB"):
        return _lib.Library(os.path.abspath(os.environ["NDFFT_EMUL_LIB"]))
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "-j4"])
    return _lib.Library(os.path.join(EMUL_DIR, "_build", "libndfft_emul.so"))


def test_scipy_factors(): fds.scipy_factors()


@pytest.mark.parametrize("rdt", fds.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", fds.FUSED_D_N)
def test_every_instance(L, n, rdt): fds.every_instance(L, n, rdt)


@pytest.mark.parametrize("rdt", fds.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", fds.FUSED_D_N)
def test_fused_and_composed_within_the_bar(L, n, rdt): fds.working_precision(L, n, rdt)


def test_weight_placement(L): fds.weight_placement(L)
def test_unit_weights(L): fds.unit_weights(L)
def test_base_and_pitch(L): fds.base_and_pitch(L)
def test_output_window_inside_a_sentinel_allocation(L): fds.sentinel_window(L)
def test_in_place_equals_out_of_place(L): fds.in_place(L)
def test_xcd_map_with_a_tail(L): fds.xcd_tail(L)
def test_lane_isolation(L): fds.lane_isolation(L)
def test_normalisation(L): fds.normalisation(L)
def test_layouts_and_composed_lengths(L): fds.layouts(L)
def test_errors(L): fds.errors(L)
def test_abi(L): fds.abi(L, ROOT)


def test_python_api_checks_and_host_path(L):
    """api.nddct_filter: wrong arguments raise before any C call; numpy arrays run the three host calls; ndfft_filter keeps refusing a DctHandler."""
    n = 24
    for rdt in fds.BOTH:
        for norm in ("Default", "None"):
            h = fds.handler(L, n, rdt).normalization(Normalization(norm))
            x = fds.make_x((5, n), rdt, seed=n)
            g = fds.make_g(n, rdt, seed=4)
            y = np.zeros_like(x)
            api.nddct_filter(x, y, h, 1, g)
            assert_close(y, fds.oracle_filter(x, g, n, 1, rdt, _lib.NORM_NONE if norm == "None" else _lib.NORM_DEFAULT), 1, TOL[np.dtype(rdt)], f"host path {norm}")
    h = fds.handler(L, n, np.float64)
    x = fds.make_x((5, n), np.float64); y = np.zeros_like(x); g = fds.make_g(n, np.float64)
    for bad_h in (handlers.FftHandler(n, np.float64, _library=L), handlers.R2cFftHandler(n, np.float64, _library=L)):
        with pytest.raises(TypeError):
            api.nddct_filter(x, y, bad_h, 1, g)
    with pytest.raises(TypeError):
        api.ndfft_filter(x, y, h, 1, g.astype(np.complex128))
    with pytest.raises(TypeError):
        api.nddct_filter(x, y, h, 1, g.astype(np.float32))
    with pytest.raises(TypeError):
        api.nddct_filter(x, y, h, 1, g.astype(np.complex128))
    with pytest.raises(TypeError):
        api.nddct_filter(x.astype(np.float32), y, h, 1, g)
    with pytest.raises(TypeError):
        api.nddct_filter(x, y, h, 1, g.reshape(2, -1))
    with pytest.raises(TypeError):
        api.nddct_filter(x, y, h, -1, g)
    with pytest.raises(ValueError):
        api.nddct_filter(x, y, h, 1, g[:-1])
    with pytest.raises(ValueError):
        api.nddct_filter(x, y, h.normalization(Normalization.custom(lambda lane: None)), 1, g)


def test_cpp_mirror_against_the_cpu_build(L, tmp_path):
    """tests/cpp/test_filter_dct.cpp (nddct_filter on DeviceArrays) linked against the CPU build of the kernel sources."""
    exe = str(tmp_path / "test_filter_dct_cpu")
    libdir = os.path.dirname(L.path)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_filter_dct.cpp"), "-o", exe,
                           "-L" + libdir, "-l" + os.path.basename(L.path)[3:-3], "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "test result: ok." in r.stdout, r.stdout + r.stderr
