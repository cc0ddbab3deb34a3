"""ndfft_filter on the MI355X: the cases of tests/filter_suite.py on the gfx950 library, api.ndfft_filter on torch tensors and numpy arrays, a fused call
inside a HIP graph, and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import filter_suite as fs
from helpers import TOL, assert_close, cdt_of
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


@pytest.mark.parametrize("rdt", fs.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", fs.FUSED_N)
def test_fused_every_instance(L, n, rdt): fs.fused_instance(L, n, rdt)


@pytest.mark.parametrize("rdt", fs.BOTH, ids=("f64", "f32"))
@pytest.mark.parametrize("n", fs.FUSED_N)
def test_fused_against_composed_within_the_bar(L, n, rdt): fs.fused_against_composed(L, n, rdt, verbose=True)


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


def _host(x, w, n, axis, rdt, r2c, norm):
    return fs.oracle_filter(x, w, n, axis, rdt, r2c, _lib.NORM_NONE if norm == "None" else _lib.NORM_DEFAULT)


@pytest.mark.parametrize("r2c", (False, True), ids=("c2c", "r2c"))
def test_public_api_torch_tensors_and_views(L, r2c):
    import torch
    for rdt in fs.BOTH:
        adt = np.dtype(rdt) if r2c else np.dtype(cdt_of(rdt))
        for shape, axis, fused in (((37, 256), 1, True), ((9, 70), 0, False), ((5, 96), 1, False)):
            n = shape[axis]
            for norm in ("Default", "None"):
                h = fs.handler(L, n, rdt, r2c).normalization(Normalization(norm))
                x = fs.make_x(shape, rdt, r2c, seed=n)
                w = fs.make_weights(fs.wname(r2c), n, rdt, seed=4)
                yo = _host(x, w, n, axis, rdt, r2c, norm)
                xd = torch.from_numpy(x).to("cuda")
                yd = torch.full(shape, 7.25, dtype=getattr(torch, adt.name), device="cuda")
                api.ndfft_filter(xd, yd, h, axis, torch.from_numpy(w).to("cuda"))
                path = L.last_path()
                assert (path == fs.FUSED) == (fused and not r2c), path
                assert_close(yd.cpu().numpy(), yo, axis, TOL[np.dtype(rdt)], f"api.ndfft_filter {shape} axis={axis} {adt.name} r2c={r2c} norm={norm} {path}")
                assert np.array_equal(xd.cpu().numpy(), x), "the caller's input was written"
                api.ndfft_filter(xd, yd, h, axis, w, fuse=False)                 # numpy weights: uploaded for the call; the composed form on request
                assert "+weights+" in L.last_path()
                assert_close(yd.cpu().numpy(), yo, axis, TOL[np.dtype(rdt)], "numpy weights, fuse=False")
                # views: the output is a window of a larger tensor (nothing outside it changes), the input a transposed tensor; then in place
                big = torch.full((shape[0] + 2, shape[1] + 6), 7.25, dtype=yd.dtype, device="cuda")
                win = big[1:shape[0] + 1, 4:4 + shape[1]]
                xt = torch.from_numpy(np.ascontiguousarray(x.T)).to("cuda").T
                api.ndfft_filter(xt, win, h, axis, torch.from_numpy(w).to("cuda"))
                got = big.cpu().numpy()
                assert_close(got[1:shape[0] + 1, 4:4 + shape[1]], yo, axis, TOL[np.dtype(rdt)], f"views {shape} axis={axis} {L.last_path()}")
                got[1:shape[0] + 1, 4:4 + shape[1]] = 7.25
                assert np.all(got == 7.25), "an element outside the output view was written"
                api.ndfft_filter(xd, xd, h, axis, torch.from_numpy(w).to("cuda"))
                assert_close(xd.cpu().numpy(), yo, axis, TOL[np.dtype(rdt)], "in place")
                # numpy arrays: the three host calls
                y = np.zeros(shape, adt)
                api.ndfft_filter(x, y, h, axis, w)
                assert_close(y, yo, axis, TOL[np.dtype(rdt)], "numpy arrays")


def test_tensor_on_the_current_stream(L):
    import torch
    n = 1024
    h = fs.handler(L, n, np.float64)
    x = fs.make_x((64, n), np.float64, seed=9)
    w = fs.make_weights("ndifft", n, np.float64, seed=9)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        xd = torch.from_numpy(x).to("cuda", non_blocking=False)
        wd = torch.from_numpy(w).to("cuda")
        xd.mul_(2.0)                                    # queued on s ahead of the call: the call must run behind it
        yd = torch.empty_like(xd)
        api.ndfft_filter(xd, yd, h, 1, wd)
        assert L.last_path() == fs.FUSED
        yd.mul_(0.5)                                    # ... and this behind the call
    s.synchronize()
    assert_close(yd.cpu().numpy(), fs.oracle_filter(x, w, n, 1, np.float64), 1, TOL[np.dtype(np.float64)], "filter on a side stream")


def test_wrong_arguments_raise_before_the_c_call(L):
    import torch
    x = torch.zeros((3, 8), dtype=torch.complex128, device="cuda")
    with pytest.raises(ValueError, match="got 7 expected 8"):
        api.ndfft_filter(x, x.clone(), handlers.FftHandler(8, _library=L), 1, np.ones(7, np.complex128))
    with pytest.raises(ValueError, match="None or Default"):
        api.ndfft_filter(x, x.clone(), handlers.FftHandler(8, _library=L).normalization(Normalization.weights(np.ones(8, np.complex128))), 1, np.ones(8, np.complex128))
    with pytest.raises(ValueError, match="None or Default"):
        api.ndfft_filter(x, x.clone(), handlers.FftHandler(8, _library=L).normalization(Normalization.custom(lambda lane: None)), 1, np.ones(8, np.complex128))
    with pytest.raises(TypeError):
        api.ndfft_filter(x, x.clone(), handlers.DctHandler(8, _library=L), 1, np.ones(8, np.complex128))


def test_fused_filter_in_a_hip_graph(L):
    """A fused call captured on one stream after one warm-up call, replayed twice on changed input."""
    import torch
    rows, n = 48, 2048                                  # (a radix list that is no palindrome: the warm-up call uploads the second twiddle table)
    rng = np.random.default_rng(5)
    w = fs.make_weights("ndifft", n, np.float64, seed=3)
    h = handlers.FftHandler(n, _library=L)
    new = lambda: rng.uniform(-1, 1, (rows, n)) + 1j * rng.uniform(-1, 1, (rows, n))
    x0 = new()
    xd = torch.from_numpy(x0).to("cuda"); wd = torch.from_numpy(w).to("cuda")
    out = torch.zeros((rows, n), dtype=torch.complex128, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        api.ndfft_filter(xd, out, h, 1, wd)            # warm-up on the capture stream
        assert L.last_path() == fs.FUSED
        s.synchronize()
        assert_close(out.cpu().numpy(), fs.oracle_filter(x0, w, n, 1, np.float64), 1, 1e-10, "eager call")
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
        assert_close(out.cpu().numpy(), fs.oracle_filter(x1, w, n, 1, np.float64), 1, 1e-10, "replayed filter on new data")


def test_cpp_mirror_on_gpu(tmp_path):
    """tests/cpp/test_filter.cpp: ndfft_filter on DeviceArrays against the three calls it stands for."""
    exe = str(tmp_path / "test_filter")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_filter.cpp"), "-o", exe,
                           "-L" + libdir, "-lndfft_mi355x", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "test result: ok." in r.stdout, r.stdout + r.stderr
