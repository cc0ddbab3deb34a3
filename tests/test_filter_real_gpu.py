"""ndfft_filter on real arrays on the MI355X: the cases of tests/filter_real_suite.py on the gfx950 library, api.ndfft_filter on real torch tensors (windowed
output, in place, a side stream), a fused call inside a HIP graph after a single warm-up call, and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import filter_real_suite as frs
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


@pytest.mark.parametrize("rdt", frs.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", frs.FUSED_R_N)
def test_every_instance(L, n, rdt): frs.every_instance(L, n, rdt)


@pytest.mark.parametrize("rdt", frs.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", frs.FUSED_R_N)
def test_fused_and_composed_within_the_bar(L, n, rdt): frs.working_precision(L, n, rdt, verbose=True)


def test_dc_and_nyquist(L): frs.dc_and_nyquist(L)
def test_weight_placement(L): frs.weight_placement(L)
def test_alignment_and_pitch(L): frs.alignment_and_pitch(L)
def test_output_window_inside_a_sentinel_allocation(L): frs.sentinel_bands(L)
def test_in_place_equals_out_of_place(L): frs.in_place(L)
def test_xcd_map_with_a_tail(L): frs.xcd_tail(L)
def test_lane_isolation(L): frs.lane_isolation(L)
def test_normalisation(L): frs.normalisation(L)
def test_layouts_and_composed_lengths(L): frs.layouts(L)


def test_public_api_real_torch_tensors(L):
    """api.ndfft_filter on real tensors: dense, a window of a larger tensor (nothing outside it changes), in place, and the composed form on request."""
    import torch
    for rdt in frs.BOTH:
        shape, n = (37, 256), 256
        for norm in ("Default", "None"):
            h = frs.handler(L, n, rdt, True).normalization(Normalization(norm))
            x = frs.make_x(shape, rdt, r2c=True, seed=n)
            w = frs.make_weights("ndifft_r2c", n, rdt, seed=4)
            yo = frs.oracle_filter(x, w, n, 1, rdt, True, _lib.NORM_NONE if norm == "None" else _lib.NORM_DEFAULT)
            tol, tdt = TOL[np.dtype(rdt)], getattr(torch, np.dtype(rdt).name)
            xd = torch.from_numpy(x).to("cuda"); wd = torch.from_numpy(w).to("cuda")
            yd = torch.full(shape, 7.25, dtype=tdt, device="cuda")
            api.ndfft_filter(xd, yd, h, 1, wd)
            assert L.last_path() == frs.FUSED_R, L.last_path()
            assert_close(yd.cpu().numpy(), yo, 1, tol, f"api.ndfft_filter real {np.dtype(rdt).name} norm={norm}")
            assert np.array_equal(xd.cpu().numpy(), x), "the caller's input was written"
            api.ndfft_filter(xd, yd, h, 1, w, fuse=False)
            assert frs.composed(L.last_path()), L.last_path()
            assert_close(yd.cpu().numpy(), yo, 1, tol, "numpy weights, fuse=False")
            big = torch.full((shape[0] + 2, shape[1] + 6), 7.25, dtype=tdt, device="cuda")
            win = big[1:shape[0] + 1, 4:4 + shape[1]]                   # an even offset and an even pitch
            api.ndfft_filter(xd, win, h, 1, wd)
            assert L.last_path() == frs.FUSED_R, L.last_path()
            got = big.cpu().numpy()
            assert_close(got[1:shape[0] + 1, 4:4 + shape[1]], yo, 1, tol, "windowed output")
            got[1:shape[0] + 1, 4:4 + shape[1]] = 7.25
            assert np.all(got == 7.25), "an element outside the output view was written"
            api.ndfft_filter(xd, xd, h, 1, wd)
            assert L.last_path() == frs.FUSED_R, L.last_path()
            assert_close(xd.cpu().numpy(), yo, 1, tol, "in place")


def test_real_tensor_on_a_side_stream(L):
    import torch
    n = 1024
    h = frs.handler(L, n, np.float64, True)
    x = frs.make_x((64, n), np.float64, r2c=True, seed=9)
    w = frs.make_weights("ndifft_r2c", n, np.float64, seed=9)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        xd = torch.from_numpy(x).to("cuda", non_blocking=False)
        wd = torch.from_numpy(w).to("cuda")
        xd.mul_(2.0)                                    # queued on s ahead of the call: the call must run behind it
        yd = torch.empty_like(xd)
        api.ndfft_filter(xd, yd, h, 1, wd)
        assert L.last_path() == frs.FUSED_R
        yd.mul_(0.5)                                    # ... and this behind the call
    s.synchronize()
    assert_close(yd.cpu().numpy(), frs.oracle_filter(x, w, n, 1, np.float64, True), 1, TOL[np.dtype(np.float64)], "real filter on a side stream")


def test_fused_real_filter_in_a_hip_graph(L):
    """One fused call captured on one stream after a SINGLE warm-up call (which builds and uploads the plan's tables), replayed twice on new data."""
    import torch
    rows, n = 48, 2048
    rng = np.random.default_rng(5)
    w = frs.make_weights("ndifft_r2c", n, np.float64, seed=3)
    h = handlers.R2cFftHandler(n, _library=L)
    new = lambda: rng.uniform(-1, 1, (rows, n))
    x0 = new()
    xd = torch.from_numpy(x0).to("cuda"); wd = torch.from_numpy(w).to("cuda")
    out = torch.zeros((rows, n), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        api.ndfft_filter(xd, out, h, 1, wd)            # the warm-up, on the capture stream
        assert L.last_path() == frs.FUSED_R
        s.synchronize()
        assert_close(out.cpu().numpy(), frs.oracle_filter(x0, w, n, 1, np.float64, True), 1, 1e-10, "eager call")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            api.ndfft_filter(xd, out, h, 1, wd)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        x1 = new()
        xd.copy_(torch.from_numpy(x1).to("cuda"))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_close(out.cpu().numpy(), frs.oracle_filter(x1, w, n, 1, np.float64, True), 1, 1e-10, "replayed real filter on new data")


def test_cpp_mirror_on_gpu(tmp_path):
    """tests/cpp/test_filter_real.cpp: ndfft_filter on real DeviceArrays against the three calls it stands for."""
    exe = str(tmp_path / "test_filter_real")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_filter_real.cpp"), "-o", exe,
                           "-L" + libdir, "-lndfft_mi355x", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "test result: ok." in r.stdout, r.stdout + r.stderr
