"""Normalization::Weights on the CPU build of the kernel sources (tests/emul): the cases of tests/weights_suite.py that need no MI355X, the C99
view of include/ndfft_mi355x_ext.h, and Normalization.weights_from (no library).  The claim about the GPU is tests/test_weights_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import weights_suite as ws
from ndrustfft_amd import _lib
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


def test_rows_every_op(L): ws.rows(L)
def test_columns_c_and_f_layout(L): ws.columns(L)
def test_views_offsets_holes_and_peeling(L): ws.views(L)
def test_exactness_against_norm_none(L): ws.exactness(L)
def test_c2r_end_points_dropped_after_weighting(L): ws.c2r_end_points(L)
def test_working_precision(L): ws.working_precision(L)
def test_multi_pass_routes_beside_the_pass_image(L): ws.multi_pass_routes(L)
def test_errors(L): ws.errors(L)


def test_ext_symbols_bound(L):
    assert _lib.EXT_SYMBOLS == ["ndfft_exec_weighted_device"]
    for s in _lib.EXT_SYMBOLS:
        assert hasattr(L.c, s)
    assert L.c.ndfft_abi_minor() >= 4


def test_weights_from_diagonal_function_round_trips():
    for dt in (np.float32, np.float64, np.complex64, np.complex128):
        d = (np.arange(1, 10) / 4).astype(dt) * (1j if np.dtype(dt).kind == "c" else 1)

        def fn(lane, d=d):
            lane *= d
        nm = Normalization.weights_from(fn, 9, dt)
        assert nm.kind == Normalization.WEIGHTS and np.array_equal(nm.host_weights(dt, 9), d)
        with pytest.raises(ValueError):
            nm.host_weights(dt, 8)


def test_weights_from_refuses_a_permutation():
    def rev(lane):
        lane[:] = lane[::-1].copy()
    with pytest.raises(ValueError, match="not an element-wise function"):
        Normalization.weights_from(rev, 8, np.float64)

    def aliased(lane):          # the issue's own example, written with the aliasing slice
        lane[:] = lane[::-1]
    with pytest.raises(ValueError, match="not an element-wise function"):
        Normalization.weights_from(aliased, 8, np.complex128)


def test_ext_header_is_strict_c99_and_links(tmp_path):
    """include/ndfft_mi355x_ext.h in a C99 translation unit that takes the function's address, linked against the product library."""
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndrustfft_amd", "csrc"), "-s", "-j4"])
    exe = str(tmp_path / "ext_c99")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "c", "ext_c99.c"), "-o", exe,
                           "-L" + libdir, "-lndfft_mi355x", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ext c99 ok" in out.stdout, out.stdout + out.stderr


def test_cpp_mirror_host_logic_against_the_cpu_build(L, tmp_path):
    """tests/cpp/test_weights.cpp (host path and DeviceArray path of Normalization::weights) linked against the CPU build of the kernel sources."""
    exe = str(tmp_path / "test_weights_cpu")
    libdir = os.path.dirname(L.path)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_weights.cpp"), "-o", exe,
                           "-L" + libdir, "-l" + os.path.basename(L.path)[3:-3], "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "test result: ok." in r.stdout, r.stdout + r.stderr
