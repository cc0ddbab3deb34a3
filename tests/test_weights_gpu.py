"""Normalization::Weights on the MI355X: the cases of tests/weights_suite.py on the gfx950 library, Normalization.weights through the public
functions on torch tensors and numpy arrays, a weighted chain inside a HIP graph, and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import parity_suite as ps
import weights_suite as ws
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


def test_rows_every_op(L): ws.rows(L)
def test_columns_c_and_f_layout(L): ws.columns(L)
def test_views_offsets_holes_and_peeling(L): ws.views(L)
def test_exactness_against_norm_none(L): ws.exactness(L)
def test_c2r_end_points_dropped_after_weighting(L): ws.c2r_end_points(L)
def test_working_precision(L): ws.working_precision(L, verbose=True)
def test_multi_block(L): ws.multi_block(L)
def test_multi_pass_routes_beside_the_pass_image(L): ws.multi_pass_routes(L)
def test_errors(L): ws.errors(L)


def _public_case(L, name, shape, axis, rdt, device):
    import torch
    n = shape[axis]
    sin, sout = ps.shapes_for(name, shape, axis)
    x = ps.make_input(name, sin, rdt, offset=n)
    odt = np.dtype(cdt_of(rdt)) if ps.OPS[name][4] else np.dtype(rdt)
    w = ws.make_weights(name, n, rdt)
    h = getattr(handlers, ps.OPS[name][2])(n, rdt, _library=L).normalization(Normalization.weights(w.astype(np.complex128 if w.dtype.kind == "c" else np.float64)))
    yo = ws.oracle_weighted(name, x, w, n, axis, rdt)
    if device:
        xd = torch.from_numpy(x).to("cuda"); yd = torch.zeros(sout, dtype=getattr(torch, odt.name), device="cuda")
        ps.OPS[name][0](xd, yd, h, axis)
        path = L.last_path()
        y = yd.cpu().numpy()
        assert np.array_equal(xd.cpu().numpy(), x), "the caller's input was written"
        if name in ws.WEIGHTED:
            assert "weights" in path, path
            assert list(h.norm._dev) == [(np.dtype(ws.wdtype(name, rdt)), "cuda:0")], h.norm._dev.keys()
    else:
        y = np.zeros(sout, odt)
        ps.OPS[name][0](x, y, h, axis)
        path = L.last_path()
        assert "weights" not in path, path          # host arrays: multiplied on the host around ndfft_exec
    assert_close(y, yo, axis, TOL[np.dtype(rdt)], f"Normalization.weights {name} {shape} axis={axis} {np.dtype(rdt).name} device={device} path={path}")


@pytest.mark.parametrize("name", list(ps.OPS))
def test_public_api_torch_tensors(L, name):
    for rdt in ws.BOTH:
        _public_case(L, name, (5, 12), 1, rdt, True)
        _public_case(L, name, (9, 70), 0, rdt, True)


@pytest.mark.parametrize("name", list(ps.OPS))
def test_public_api_numpy_arrays(L, name):
    for rdt in ws.BOTH:
        _public_case(L, name, (5, 12), 1, rdt, False)
        _public_case(L, name, (9, 7), 0, rdt, False)


def test_wrong_length_raises_before_the_c_call(L):
    import torch
    h = handlers.DctHandler(8, _library=L).normalization(Normalization.weights(np.ones(7)))
    with pytest.raises(ValueError, match="got 7 expected 8"):
        api.nddct2(np.zeros((3, 8)), np.zeros((3, 8)), h, 1)
    with pytest.raises(ValueError, match="got 7 expected 8"):
        api.nddct2(torch.zeros((3, 8), dtype=torch.float64, device="cuda"), torch.zeros((3, 8), dtype=torch.float64, device="cuda"), h, 1)


def test_weighted_chain_in_a_hip_graph(L):
    """ndifft followed by nddct2, both with weights, captured on one stream after one warm-up call (which allocates the pass's image and uploads the
    vectors), replayed on new data."""
    import torch
    rows, n = 16, 96
    rng = np.random.default_rng(5)
    wc = ws.make_weights("ndifft", n, np.float64, seed=3); wr = ws.make_weights("nddct2", n, np.float64, seed=4)
    hf = handlers.FftHandler(n, _library=L).normalization(Normalization.weights(wc))
    hd = handlers.DctHandler(n, _library=L).normalization(Normalization.weights(wr))

    def host(x):
        mid = ws.oracle_weighted("ndifft", x, wc, n, 1, np.float64)
        re = np.ascontiguousarray(mid.real)
        return ws.oracle_weighted("nddct2", re, wr, n, 1, np.float64)
    x0 = (rng.uniform(-1, 1, (rows, n)) + 1j * rng.uniform(-1, 1, (rows, n)))
    xd = torch.from_numpy(x0).to("cuda")
    mid = torch.zeros((rows, n), dtype=torch.complex128, device="cuda")
    re = torch.zeros((rows, n), dtype=torch.float64, device="cuda")
    out = torch.zeros((rows, n), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        def chain():
            api.ndifft(xd, mid, hf, 1)
            re.copy_(torch.view_as_real(mid)[..., 0])
            api.nddct2(re, out, hd, 1)
        chain()                                   # warm-up on the capture stream
        s.synchronize()
        assert_close(out.cpu().numpy(), host(x0), 1, 1e-10, "eager chain")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            chain()
    torch.cuda.current_stream().wait_stream(s)
    x1 = (rng.uniform(-1, 1, (rows, n)) + 1j * rng.uniform(-1, 1, (rows, n)))
    xd.copy_(torch.from_numpy(x1).to("cuda"))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert_close(out.cpu().numpy(), host(x1), 1, 1e-10, "replayed chain on new data")


def test_cpp_mirror_on_gpu(tmp_path):
    """tests/cpp/test_weights.cpp: host path and DeviceArray path of Normalization::weights for ndifft and nddct1."""
    exe = str(tmp_path / "test_weights")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_weights.cpp"), "-o", exe,
                           "-L" + libdir, "-lndfft_mi355x", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "test result: ok." in r.stdout, r.stdout + r.stderr
