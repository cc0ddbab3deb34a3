"""ndfft_filter along a strided axis on the MI355X: the cases of tests/filter_col_suite.py on the gfx950 library, api.ndfft_filter on torch tensors, a side
stream, a fused column call inside a HIP graph, and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import filter_col_suite as fcs
import filter_suite as fs
from helpers import TOL, assert_close, cdt_of
from ndrustfft_amd import _lib, api, handlers

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def L():
    lib = _lib.default()                      # in-tree gfx950 build; raises if missing
    assert lib.c.ndfft_device_count() >= 1, "no MI355X visible"
    return lib


@pytest.mark.parametrize("n,rdt", fcs.INSTANCES, ids=fcs.INSTANCE_IDS)
def test_every_instance(L, n, rdt): fcs.every_instance(L, n, rdt)


@pytest.mark.parametrize("n,rdt", fcs.INSTANCES, ids=fcs.INSTANCE_IDS)
def test_against_composed_within_the_bar(L, n, rdt): fcs.against_composed(L, n, rdt, verbose=True)


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


def test_public_api_torch_tensors_and_views(L):
    import torch
    for rdt in fs.BOTH:
        cdt = np.dtype(cdt_of(rdt))
        tol = TOL[np.dtype(rdt)]
        for shape, axis in (((256, 40), 0), ((3, 128, 24), 1)):
            n = shape[axis]
            h = fs.handler(L, n, rdt)
            x = fs.make_x(shape, rdt, seed=n)
            w = fs.make_weights("ndifft", n, rdt, seed=4)
            yo = fs.oracle_filter(x, w, n, axis, rdt)
            what = f"api.ndfft_filter {shape} axis={axis} {cdt.name}"
            xd, wd = torch.from_numpy(x).to("cuda"), torch.from_numpy(w).to("cuda")
            yd = torch.full(shape, 7.25, dtype=getattr(torch, cdt.name), device="cuda")
            api.ndfft_filter(xd, yd, h, axis, wd)
            assert L.last_path() == fcs.FUSED_COL, L.last_path()
            assert_close(yd.cpu().numpy(), yo, axis, tol, what)
            assert np.array_equal(xd.cpu().numpy(), x), "the caller's input was written"
            api.ndfft_filter(xd, yd, h, axis, w, fuse=False)                 # numpy weights: uploaded for the call; the composed form on request
            assert "+weights+" in L.last_path()
            assert_close(yd.cpu().numpy(), yo, axis, tol, what + " numpy weights, fuse=False")
            # the output is a window of a larger tensor: nothing outside it changes
            big = torch.full(tuple(s + 2 for s in shape[:-1]) + (shape[-1] + 6,), 7.25, dtype=yd.dtype, device="cuda")
            cut = tuple(slice(1, s + 1) for s in shape[:-1]) + (slice(4, 4 + shape[-1]),)
            api.ndfft_filter(xd, big[cut], h, axis, wd)
            assert L.last_path() == fcs.FUSED_COL, L.last_path()
            got = big.cpu().numpy()
            assert_close(got[cut], yo, axis, tol, what + " window output")
            got[cut] = 7.25
            assert np.all(got == 7.25), "an element outside the output view was written"
            api.ndfft_filter(xd, xd, h, axis, wd)
            assert L.last_path() == fcs.FUSED_COL, L.last_path()
            assert_close(xd.cpu().numpy(), yo, axis, tol, what + " in place")


def test_tensor_on_the_current_stream(L):
    import torch
    n = 1024
    h = fs.handler(L, n, np.float64)
    x = fs.make_x((n, 64), np.float64, seed=9)
    w = fs.make_weights("ndifft", n, np.float64, seed=9)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        xd = torch.from_numpy(x).to("cuda", non_blocking=False)
        wd = torch.from_numpy(w).to("cuda")
        xd.mul_(2.0)                                    # queued on s ahead of the call: the call must run behind it
        yd = torch.empty_like(xd)
        api.ndfft_filter(xd, yd, h, 0, wd)
        assert L.last_path() == fcs.FUSED_COL
        yd.mul_(0.5)                                    # ... and this behind the call
    s.synchronize()
    assert_close(yd.cpu().numpy(), fs.oracle_filter(x, w, n, 0, np.float64), 0, TOL[np.dtype(np.float64)], "column filter on a side stream")


def test_fused_column_filter_in_a_hip_graph(L):
    """A fused column call captured on one stream after one warm-up call, replayed twice on changed input."""
    import torch
    n, cols = 2048, 48                                  # (a radix list that is no palindrome: the warm-up call uploads the second twiddle table)
    rng = np.random.default_rng(5)
    w = fs.make_weights("ndifft", n, np.float64, seed=3)
    h = handlers.FftHandler(n, _library=L)
    new = lambda: rng.uniform(-1, 1, (n, cols)) + 1j * rng.uniform(-1, 1, (n, cols))
    x0 = new()
    xd = torch.from_numpy(x0).to("cuda"); wd = torch.from_numpy(w).to("cuda")
    out = torch.zeros((n, cols), dtype=torch.complex128, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        api.ndfft_filter(xd, out, h, 0, wd)            # warm-up on the capture stream
        assert L.last_path() == fcs.FUSED_COL
        s.synchronize()
        assert_close(out.cpu().numpy(), fs.oracle_filter(x0, w, n, 0, np.float64), 0, 1e-10, "eager call")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            api.ndfft_filter(xd, out, h, 0, wd)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        x1 = new()
        xd.copy_(torch.from_numpy(x1).to("cuda"))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_close(out.cpu().numpy(), fs.oracle_filter(x1, w, n, 0, np.float64), 0, 1e-10, "replayed column filter on new data")


def test_cpp_mirror_on_gpu(tmp_path):
    """tests/cpp/test_filter_col.cpp: ndfft_filter on DeviceArrays along axis 0 against the three calls it stands for."""
    exe = str(tmp_path / "test_filter_col")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_filter_col.cpp"), "-o", exe,
                           "-L" + libdir, "-lndfft_mi355x", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "test result: ok." in r.stdout, r.stdout + r.stderr
