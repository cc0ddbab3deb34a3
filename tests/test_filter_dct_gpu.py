"""nddct_filter on the MI355X: the cases of tests/filter_dct_suite.py on the gfx950 library, api.nddct_filter on torch tensors (windowed output, in place, numpy
weights, a side stream), a fused call inside a HIP graph after a single warm-up call, numpy arrays through the host path, and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import filter_dct_suite as fds
from helpers import TOL, assert_close
from ndrustfft_amd import _lib, api, handlers
from ndrustfft_amd.handlers import Normalization

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def L():
    lib = _lib.default()                      # in-tree gfx950 build; raises if missing
    assert lib.c.ndfft_device_count() >= 1, "no MI355X visible"
    return lib


@pytest.mark.parametrize("rdt", fds.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", fds.FUSED_D_N)
def test_every_instance(L, n, rdt): fds.every_instance(L, n, rdt)


@pytest.mark.parametrize("rdt", fds.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", fds.FUSED_D_N)
def test_fused_and_composed_within_the_bar(L, n, rdt): fds.working_precision(L, n, rdt, verbose=True)


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


def test_public_api_torch_tensors(L):
    """api.nddct_filter on tensors: dense, a window of a larger tensor at an odd offset (nothing outside it changes), in place, and the composed form on request."""
    import torch
    for rdt in fds.BOTH:
        shape, n = (37, 256), 256
        for norm in ("Default", "None"):
            h = fds.handler(L, n, rdt).normalization(Normalization(norm))
            x = fds.make_x(shape, rdt, seed=n)
            g = fds.make_g(n, rdt, seed=4)
            yo = fds.oracle_filter(x, g, n, 1, rdt, _lib.NORM_NONE if norm == "None" else _lib.NORM_DEFAULT)
            tol, tdt = TOL[np.dtype(rdt)], getattr(torch, np.dtype(rdt).name)
            xd = torch.from_numpy(x).to("cuda"); gd = torch.from_numpy(g).to("cuda")
            yd = torch.full(shape, 7.25, dtype=tdt, device="cuda")
            api.nddct_filter(xd, yd, h, 1, gd)
            assert L.last_path() == fds.FUSED_D, L.last_path()
            assert_close(yd.cpu().numpy(), yo, 1, tol, f"api.nddct_filter {np.dtype(rdt).name} norm={norm}")
            assert np.array_equal(xd.cpu().numpy(), x), "the caller's input was written"
            api.nddct_filter(xd, yd, h, 1, g, fuse=False)
            assert fds.composed(L.last_path()), L.last_path()
            assert_close(yd.cpu().numpy(), yo, 1, tol, "numpy weights, fuse=False")
            big = torch.full((shape[0] + 2, shape[1] + 7), 7.25, dtype=tdt, device="cuda")
            win = big[1:shape[0] + 1, 3:3 + shape[1]]                   # an odd offset and an odd pitch
            api.nddct_filter(xd, win, h, 1, gd)
            assert L.last_path() == fds.FUSED_D, L.last_path()
            got = big.cpu().numpy()
            assert_close(got[1:shape[0] + 1, 3:3 + shape[1]], yo, 1, tol, "windowed output")
            got[1:shape[0] + 1, 3:3 + shape[1]] = 7.25
            assert np.all(got == 7.25), "an element outside the output view was written"
            api.nddct_filter(xd, xd, h, 1, gd)
            assert L.last_path() == fds.FUSED_D, L.last_path()
            assert_close(xd.cpu().numpy(), yo, 1, tol, "in place")


def test_wrong_arguments_and_the_host_path(L):
    """Wrong arguments raise before the C call; numpy arrays run the three host calls; api.ndfft_filter keeps refusing a DctHandler."""
    import torch
    n = 256
    h = fds.handler(L, n, np.float64)
    x = fds.make_x((5, n), np.float64, seed=2); g = fds.make_g(n, np.float64, seed=2)
    y = np.zeros_like(x)
    api.nddct_filter(x, y, h, 1, g)
    assert_close(y, fds.oracle_filter(x, g, n, 1, np.float64), 1, TOL[np.dtype(np.float64)], "numpy arrays through the host path")
    xd = torch.from_numpy(x).to("cuda"); yd = torch.empty_like(xd); gd = torch.from_numpy(g).to("cuda")
    with pytest.raises(TypeError):
        api.ndfft_filter(xd, yd, h, 1, gd.to(torch.complex128))
    for bad_h in (handlers.FftHandler(n, np.float64, _library=L), handlers.R2cFftHandler(n, np.float64, _library=L)):
        with pytest.raises(TypeError):
            api.nddct_filter(xd, yd, bad_h, 1, gd)
    with pytest.raises(TypeError):
        api.nddct_filter(xd, yd, h, 1, gd.to(torch.float32))
    with pytest.raises(TypeError):
        api.nddct_filter(xd, yd, h, 1, gd.to(torch.complex128))
    with pytest.raises(TypeError):
        api.nddct_filter(xd.to(torch.float32), yd, h, 1, gd)
    with pytest.raises(TypeError):
        api.nddct_filter(xd, y, h, 1, gd)                                  # one array on the host
    with pytest.raises(ValueError):
        api.nddct_filter(xd, yd, h, 1, gd[:-1])
    with pytest.raises(ValueError):
        api.nddct_filter(xd, yd, h.normalization(Normalization.custom(lambda lane: None)), 1, gd)
    with pytest.raises(ValueError):
        api.nddct_filter(xd, torch.empty_like(xd)._neg_view(), fds.handler(L, n, np.float64), 1, gd)
    with pytest.raises(_lib.Panic):
        api.nddct_filter(xd, torch.empty((5, n + 1), dtype=torch.float64, device="cuda"), fds.handler(L, n, np.float64), 1, gd)


def test_tensor_on_a_side_stream(L):
    import torch
    n = 1024
    h = fds.handler(L, n, np.float64)
    x = fds.make_x((64, n), np.float64, seed=9)
    g = fds.make_g(n, np.float64, seed=9)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        xd = torch.from_numpy(x).to("cuda", non_blocking=False)
        gd = torch.from_numpy(g).to("cuda")
        xd.mul_(2.0)                                    # queued on s ahead of the call: the call must run behind it
        yd = torch.empty_like(xd)
        api.nddct_filter(xd, yd, h, 1, gd)
        assert L.last_path() == fds.FUSED_D
        yd.mul_(0.5)                                    # ... and this behind the call
    s.synchronize()
    assert_close(yd.cpu().numpy(), fds.oracle_filter(x, g, n, 1, np.float64), 1, TOL[np.dtype(np.float64)], "dct filter on a side stream")


def test_fused_dct_filter_in_a_hip_graph(L):
    """One fused call captured on one stream after a SINGLE warm-up call (which builds and uploads the plan's tables), replayed twice on new data."""
    import torch
    rows, n = 48, 2048
    rng = np.random.default_rng(5)
    g = fds.make_g(n, np.float64, seed=3)
    h = handlers.DctHandler(n, _library=L)
    new = lambda: rng.uniform(-1, 1, (rows, n))
    x0 = new()
    xd = torch.from_numpy(x0).to("cuda"); gd = torch.from_numpy(g).to("cuda")
    out = torch.zeros((rows, n), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        api.nddct_filter(xd, out, h, 1, gd)            # the warm-up, on the capture stream
        assert L.last_path() == fds.FUSED_D
        s.synchronize()
        assert_close(out.cpu().numpy(), fds.oracle_filter(x0, g, n, 1, np.float64), 1, 1e-10, "eager call")
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            api.nddct_filter(xd, out, h, 1, gd)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        x1 = new()
        xd.copy_(torch.from_numpy(x1).to("cuda"))
        out.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert_close(out.cpu().numpy(), fds.oracle_filter(x1, g, n, 1, np.float64), 1, 1e-10, "replayed dct filter on new data")


def test_cpp_mirror_on_gpu(tmp_path):
    """tests/cpp/test_filter_dct.cpp: nddct_filter on DeviceArrays against the three calls it stands for."""
    exe = str(tmp_path / "test_filter_dct")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_filter_dct.cpp"), "-o", exe,
                           "-L" + libdir, "-lndfft_mi355x", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "test result: ok." in r.stdout, r.stdout + r.stderr
