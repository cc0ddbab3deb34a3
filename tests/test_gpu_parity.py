"""THE parity tests: hand-written HIP on a real MI355X, called through the C ABI
(include/ndfft_mi355x.h) via the thin ctypes host layer, compared with the CPU oracle on the same
seeded inputs, with the committed golden vectors, and -- at BASELINE.json's full sizes -- on EVERY lane of the
array (the oracle's OpenMP `_par` form) plus size-independent properties (Parseval, round trips, linearity)."""
import os

import numpy as np
import pytest

import parity_suite as ps
import synth
from helpers import GOLDEN_SIZES, TOL, assert_close, rel_global
from ndrustfft_amd import _lib, api, handlers
from oracle import oracle_ctypes as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    lib = _lib.default()                      # in-tree gfx950 build; raises if missing
    assert lib.c.ndfft_device_count() >= 1, "no MI355X visible"
    return lib


def test_reference_unit_tests(L, refvec): ps.reference_unit_tests(L, refvec)
def test_reference_examples(L, refvec): ps.reference_examples(L, refvec)
def test_layouts(L): ps.layouts(L)
def test_normalization(L): ps.normalization_modes(L)
def test_panics(L): ps.panics(L)
def test_clone(L): ps.handler_clone_shares_plan(L)
def test_wave_short_lanes(L): ps.wave_short_lanes(L)
def test_tiny_lanes(L): ps.tiny_lanes(L)
def test_reg_lanes(L): ps.reg_lanes(L)
def test_regreal_lanes(L): ps.regreal_lanes(L, sizes=(12, 17, 18, 21, 24, 30, 42, 48), sizes_f32=(49, 64, 72))      # (every op x dtype x layout is one hiprtc compile: ~100 s for the default lists)
def test_tinymat_lanes(L): ps.tinymat_lanes(L)
def test_host_pipeline_pageable(L): ps.host_pipeline_pageable(L)
def test_prebuilt_jit_objects_serve_reference_lengths():
    """The code objects shipped beside the library (ndrustfft_amd/csrc/jit_prebuilt, tools/prebuild_jit.py) must serve the reference's own bench lengths
    without hiprtc: a fresh process with the user cache disabled and compilation forbidden still takes the specialised kernels.  Fails when the kernel
    headers have changed since the set was built (regenerate it on an MI355X)."""
    import subprocess
    import sys
    pre = os.path.join(ROOT, "ndrustfft_amd", "csrc", "jit_prebuilt")
    if not os.path.isdir(pre) or not any(f.endswith(".hsaco") for f in os.listdir(pre)):
        pytest.skip("no prebuilt code objects in this tree (tools/prebuild_jit.py writes them on an MI355X)")
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from ndrustfft_amd import DctHandler, FftHandler, _lib, nddct1, ndfft
n = 264
x = torch.zeros((n, n), dtype=torch.complex128, device="cuda:0"); y = torch.empty_like(x)
ndfft(x, y, FftHandler(n), 0); p1 = _lib.default().last_path()
xr = torch.zeros((265, 265), dtype=torch.float64, device="cuda:0"); yr = torch.empty_like(xr)
nddct1(xr, yr, DctHandler(265), 0); p2 = _lib.default().last_path()
xb = torch.zeros((4096, n), dtype=torch.complex128, device="cuda:0"); yb = torch.empty_like(xb)
ndfft(xb, yb, FftHandler(n), 1); p3 = _lib.default().last_path()
torch.cuda.synchronize()
print("PATHS", p1, p2, p3)
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, NDFFT_JIT_CACHE="0", NDFFT_JIT="cached")
    env.pop("NDFFT_JIT_PREBUILT", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("PATHS")][-1].split()
    assert line[1:] == ["jit_col", "jit_col", "jit_reg"], f"prebuilt code objects missing or stale (paths {line[1:]}): run tools/prebuild_jit.py on an MI355X"


def test_four_step_without_hiprtc_kernels_falls_back():
    """Long lanes whose four-step factors are not powers of two run their two passes on hiprtc kernels.  When those cannot be had (here: NDFFT_JIT=cached
    with no cache and no prebuilt objects) the pass declines and the call takes the route it took before round 6 -- the transpose form of the complex
    four-step, the packed route of DCT-IV -- instead of failing (round-6 advisor, medium item)."""
    import subprocess
    import sys
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import parity_suite as ps
from ndrustfft_amd import _lib
L = _lib.default()
print("PATHS", ps.run_case(L, "ndfft", (2, 196608), 1, np.float64), ps.run_case(L, "nddct4", (2, 163840), 1, np.float64))
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, NDFFT_JIT="cached", NDFFT_JIT_CACHE="0", NDFFT_JIT_PREBUILT="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("PATHS")][-1].split()
    assert line[1:] == ["four_step", "four_step"], line[1:]


def test_regreal_tail_workgroup(L):
    """RegReal's tail workgroup clamps its staging addresses (predicated loads into AGPR-spilled registers once lost values on the
    MI355X, n = 40, 48 in f64): the product form on a partial last workgroup.  The predicated form is no longer in the product library
    (round 4: it is compiled only in a developer build, `make DEV=1`; tools/repro_masked_tail.py)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import repro_masked_tail as rp
    for n in (40, 48):
        lanes = 65536 // n * 2 + 37
        path, err = rp.run_case(n, lanes, masked=False)
        assert path == "regreal_row", path
        assert err.max() <= 1e-10, f"product (clamped) form wrong for n={n}: {err.max()}"


def test_host_registration_cache(L):
    """Caller arrays in ordinary malloc memory: the second ndfft_exec on the same arrays registers them, later calls run the pinned pipeline; results
    identical on every path; arrays that change size at the same address, ndfft_host_forget, and a different input through the same output."""
    import ctypes
    n = 1024
    x = synth.complex_array((4096, n)); yo = np.zeros_like(x); orc.ndfft_par(x, yo, orc.FftHandler(n), 1)
    h = handlers.FftHandler(n, _library=L)
    L.check(L.c.ndfft_host_reg_cache(1 << 30))                   # opt-in
    ys = []
    for k in range(4):
        y = np.zeros_like(x) if k == 0 else ys[0]
        if k == 0: ys.append(y)
        y[...] = 0
        api.ndfft(x, y, h, 1)
        assert_close(y, yo, 1, 1e-10, f"host call {k}")
    attr_pinned = lambda a: L.c.ndfft_host_forget(ctypes.c_void_p(a.ctypes.data)) == 0
    x2 = synth.complex_array((4096, n), offset=77); y2o = np.zeros_like(x2); orc.ndfft_par(x2, y2o, orc.FftHandler(n), 1)
    api.ndfft(x2, ys[0], h, 1); assert_close(ys[0], y2o, 1, 1e-10, "new input, registered output")
    assert attr_pinned(x) and attr_pinned(ys[0])
    api.ndfft(x, ys[0], h, 1); assert_close(ys[0], yo, 1, 1e-10, "after forget")
    # a view of the registered array (smaller range inside it) and a larger array over it
    for k in range(3):
        api.ndfft(x[:2048], ys[0][:2048], h, 1)
    assert_close(ys[0][:2048], yo[:2048], 1, 1e-10, "sub-range of a seen array")
    # the contract the cache is opt-in for: forget BEFORE freeing (round 3 measured what happens otherwise on the MI355X: the allocator hands the
    # addresses out again, and the next copy touching the stale registration fails with "invalid argument" or aborts inside the HIP runtime)
    for rep in range(4):
        a = synth.complex_array((4096, n), offset=rep); b = np.zeros_like(a)
        for k in range(3):
            api.ndfft(a, b, h, 1)
        bo = np.zeros_like(a); orc.ndfft_par(a, bo, orc.FftHandler(n), 1)
        assert_close(b, bo, 1, 1e-10, f"arrays allocated, transformed three times, forgotten and freed, round {rep}")
        L.check(L.c.ndfft_host_forget(ctypes.c_void_p(a.ctypes.data))); L.check(L.c.ndfft_host_forget(ctypes.c_void_p(b.ctypes.data)))
        del a, b
    L.check(L.c.ndfft_host_reg_cache(0))


def test_sharded_fft2_pipeline_on_one_gpu(L, monkeypatch):
    """fft2 / rfft2 at bench.py's sharded-fft2 size (1024 x 1024) through ndfft_exec_sharded_device, every block forced through the remote pipeline."""
    monkeypatch.setenv("NDFFT_SHARD_FORCE_REMOTE", "1"); L.reload_switches()
    n = L.c.ndfft_device_count()
    ids = list(range(n)) if n > 1 else [0, 0, 0]
    ps.dev_sharded_fft2(L, (1024, 1024), root=0, ids=ids)
    ps.dev_sharded_fft2(L, (768, 1000), root=0, ids=ids, real=True)


def test_sharded_device_resident_pipeline_on_one_gpu(L, monkeypatch):
    """ndfft_exec_sharded_device's scatter -> transform -> gather pipeline (pack / unpack kernels on the root, per-device streams, events, two buffer
    slots) on real hardware: with one GPU per lease every block lives on the root, so NDFFT_SHARD_FORCE_REMOTE sends them through the pipeline anyway.
    Blocks interleaved in memory (axis 0 of a C-contiguous array), output views with holes (sentinels must survive), many small chunks."""
    monkeypatch.setenv("NDFFT_SHARD_FORCE_REMOTE", "1"); L.reload_switches()     # (conftest reloads again after the test)
    n = L.c.ndfft_device_count()
    ids = list(range(n)) if n > 1 else [0, 0, 0]
    ps.dev_sharded_case(L, "ndfft", (64, 300), 0, root=0, ids=ids, repeats=5)
    ps.dev_sharded_case(L, "ndfft_r2c", (64, 5, 3), 0, root=0, ids=ids, repeats=3)
    ps.dev_sharded_case(L, "ndfft", (9, 16, 6), 1, root=0, ids=ids, out_view=((9, 16, 12), np.s_[:, :, ::2]), repeats=3)
    ps.dev_sharded_case(L, "ndfft", (9, 16, 6), 1, root=0, ids=ids, out_view=((9, 16, 12), np.s_[::-1, :, 1::2]), in_view=((18, 16, 6), np.s_[::2]), repeats=3)
    ps.dev_sharded_case(L, "ndfft", (4096, 512), 1, root=0, ids=ids, repeats=2)                     # contiguous spans, 16 MiB
    ps.dev_sharded_case(L, "ndfft", (512, 4096), 0, root=0, ids=ids, repeats=2)                     # packed images, 16 MiB
    monkeypatch.setenv("NDFFT_SHARD_CHUNK_KB", "256"); L.reload_switches()
    ps.dev_sharded_case(L, "ndfft", (4096, 512), 1, root=0, ids=ids, repeats=2)                     # ~22 chunks per block through two slots
    ps.dev_sharded_case(L, "nddct2", (300, 64, 40), 1, root=0, ids=ids, out_view=((300, 64, 80), np.s_[:, :, ::2]), repeats=2)


def test_sharded_exec_same_device_twice(L):
    n = L.c.ndfft_device_count()
    ps.sharded_exec(L, list(range(n)) if n > 1 else [0, 0, 0], torch_device="cuda:0")
def test_interleaved_mut_views_two_threads(L): ps.interleaved_mut_views_two_threads(L)
def test_shared_handler_across_threads(L): ps.shared_handler_across_threads(L)
def test_long_strided_lanes(L): ps.long_strided_lanes(L)
def test_narrow_xcd_tiles(L): ps.narrow_xcd_tiles(L)
def test_column_four_step(L): ps.column_four_step(L)
def test_huge_prime_factors(L): ps.huge_prime_factors(L)
def test_fuzz(L):
    paths = ps.fuzz(L, seed=7, count=400)
    assert len(paths) >= 8, paths
def test_fuzz_streaming_loads(L):
    """The input hint COLD sends every kernel that has a streaming-load form down it (C2C rows, real-op rows with 16-byte staging, column tiles): same parity bar."""
    L.check(L.c.ndfft_set_input_hint(_lib.INPUT_COLD))
    try:
        paths = ps.fuzz(L, seed=13, count=250)
        assert len(paths) >= 8, paths
        ps.pow2_real_sizes(L, sizes=(64, 512, 4096), dtypes=(np.float64, np.float32))
        ps.rader_kernel(L, sizes=(511, 513), col_max_F=0, dtypes=(np.float64,))       # (round 5: streaming staging loads of the Rader rows, symmetric DCT-I form included)
        ps.baseline_length_fixtures(L, np.load(os.path.join(ROOT, "tests", "golden", "baseline_lengths.npz")), device="cuda:0")
    finally:
        L.check(L.c.ndfft_set_input_hint(_lib.INPUT_AUTO))
def test_fuzz_short_lanes(L):
    """the same fuzz restricted to lanes of <= 100 points with enough lanes to reach the plan-time specialisations: wavefront,
    thread-per-lane (tiny / tinymat / reg / regreal) and their fallbacks, in every layout the fuzz generates"""
    paths = ps.fuzz(L, seed=31, count=300, max_points=1 << 18, lengths=tuple(range(2, 65)) + (66, 70, 72, 80, 90, 96, 100))
    assert {"tiny_col", "tinymat_col"} <= set(paths) and any(p.startswith("reg") for p in paths), paths
def test_partial_round_configs(L): ps.partial_round_configs(L, sizes=(264, 210, 840, 1008, 630, 2520, 3003, 6006, 33, 66))
def test_long_smooth_lanes(L): ps.long_smooth_lanes(L)
def test_rader_kernel(L): ps.rader_kernel(L, sizes=(31, 62, 127, 257, 511, 1009, 3027), col_max_F=600)
def test_rader_two_factor_cofactor_and_wide_radices(L):
    """Cofactors 17..32 as two butterflies in registers (306 = 18 x 17, 513 = 27 x 19, 532 = 28 x 19, 522 = 18 x 29, 2336 = 32 x 73) and p - 1 with a factor 17 / 19
    (103, 137, 191; 206 = 2 x 103, 2466 = 18 x 137)."""
    ps.rader_kernel(L, sizes=(306, 513, 2336, 103, 206), col_max_F=600)
def test_rader_f32_radix_23_29_31(L):
    """p - 1 with one factor 23 / 29 / 31 gets a pass of that radix (139: 138 = 23 x 6, 233: 232 = 29 x 8, 311: 310 = 31 x 10)."""
    ps.rader_kernel(L, sizes=(139, 311), col_max_F=200, dtypes=(np.float32,))
@pytest.mark.gpu
def test_rader_f64_radix_23_29_31(L):
    """The same in f64 (round 6; Bluestein before): rows of every op family; column tiles where the lane count allows, else any correct route."""
    ps.rader_kernel(L, sizes=(139, 233, 311), col_max_F=0, dtypes=(np.float64,))
    for name, shape, axis in (("ndfft", (139, 2048), 0), ("nddct2", (278, 1024), 0), ("ndfft_r2c", (3, 622, 512), 1)):
        ps.run_case(L, name, shape, axis, np.float64, offset=7)
def test_c64_rows_on_half_the_threads(L):
    """Round 6 (jit.hip: jit_c2c_row_vec): f32 C2C rows of the 14 lengths whose default recipe has one butterfly per thread in its first or last pass run the same
    radix list on half the threads with 16-byte accesses -- against the oracle, both directions; and from a base pointer that is only 8-byte aligned (plain recipe)."""
    import torch
    from ndrustfft_amd import FftHandler, ndfft
    for n in (432, 500, 648, 1000, 1296, 2500, 2592, 3888, 5184):
        rows = max(64, (1 << 18) // n)
        for name in ("ndfft", "ndifft"):
            assert ps.run_case(L, name, (rows, n), 1, np.float32, offset=n) == "jit_reg", (name, n)
    n, rows = 1000, 300
    x = synth.complex_array((rows, n), np.complex64)
    ref = np.fft.fft(x.astype(np.complex128), axis=1)
    for shift in (0, 1):
        buf = torch.zeros(rows * n + shift, dtype=torch.complex64, device="cuda:0"); out = torch.zeros(rows * n + shift, dtype=torch.complex64, device="cuda:0")
        xd = buf[shift:].view(rows, n); yd = out[shift:].view(rows, n)
        xd.copy_(torch.from_numpy(x))
        assert xd.data_ptr() % 16 == 8 * shift
        ndfft(xd, yd, FftHandler(n, np.float32), 1)
        torch.cuda.synchronize()
        err = np.abs(yd.cpu().numpy() - ref).max() / np.abs(ref).max()
        assert err < 1e-5 and _lib.default().last_path() == "jit_reg", (shift, err)
def test_odd_real_lengths(L): ps.odd_real_lengths(L, sizes=(63, 125, 1001, 3003), dct4=True)
def test_dct1_power_of_two_lengths(L): ps.dct1_power_of_two_lengths(L)
def test_rader_kernel_beyond_bluestein(L):
    """F > 4096: Bluestein's M = 2^k >= 2F - 1 no longer fits one launch, Rader's F elements of LDS do (7001, 8191 prime; 8402 = 2 x 4201)."""
    ps.rader_kernel(L, sizes=(8191, 8402), col_max_F=0)
def test_bluestein_register_kernel(L):
    ps.bluestein_register_kernel(L, sizes=((17, 64), (31, 64), (97, 256), (127, 256), (511, 1024), (1009, 2048), (2039, 4096), (4093, 8192)), col_max_M=1024)
def test_long_lanes_four_step(L): ps.long_lanes_four_step(L, full=True)
@pytest.mark.gpu
def test_long_lanes_padded_views(L): ps.long_lanes_padded_views(L)
def test_pow2_real_sizes(L): ps.pow2_real_sizes(L)
def test_jit_specialised_sizes(L): ps.jit_specialised_sizes(L)
def test_pow2_col_sizes(L): ps.pow2_col_sizes(L)
def test_reference_bench_shapes(L): ps.reference_bench_shapes(L)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", GOLDEN_SIZES)
def test_golden(L, npvec, dt, n): ps.golden_vectors(L, npvec, dt, n)


def test_baseline_length_fixtures_host(L, blvec):
    """HIP path (host arrays) against numpy / scipy, long-double definitions and mpmath at n = 4096 / 8192 / 16384 / 512: no oracle in the loop."""
    ps.baseline_length_fixtures(L, blvec)


def test_baseline_length_fixtures_device(L, blvec):
    """The same through ndfft_exec_device on torch tensors (the path the roofline numbers are measured on)."""
    ps.baseline_length_fixtures(L, blvec, device="cuda:0")


@pytest.mark.parametrize("n", ps.SIZE_SWEEP)
def test_sizes_f64(L, n): ps.size_sweep(L, n, np.float64)


@pytest.mark.parametrize("n", ps.SIZE_SWEEP)
def test_sizes_f32(L, n): ps.size_sweep(L, n, np.float32)


@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384])
@pytest.mark.parametrize("rdt", [np.float64, np.float32])
def test_pow2_tuned(L, n, rdt):
    for name in ("ndfft", "ndifft"):
        for norm in ("Default", "None"):
            assert ps.run_case(L, name, (37, n), 1, rdt, norm=norm, offset=n) == ("wave_reg" if n == 64 else "pow2_reg")


# ---- BASELINE.json configs at full size: EVERY lane against the oracle ---------------------------
def _all_lanes_vs_oracle(x, y, ofn_par, oh, axis, tol, what):
    """The whole array through the oracle's OpenMP `_par` form (create_transform_par!, src/lib.rs:169-238) and a
    comparison of every lane: per-lane relative L2 and global max, SURVEY 8c's two metrics."""
    yo = np.zeros_like(y)
    ofn_par(x, yo, oh, axis)
    assert_close(y, yo, axis, tol, what)
    return yo


def test_cfg2_fft_4096x4096_f64(L):
    """configs[1]: ndfft axis=1 on 4096x4096 Complex<f64>, both fills, all 4096 lanes."""
    n = 4096
    h = handlers.FftHandler(n, _library=L); oh = orc.FftHandler(n)
    for fill in ("splitmix", "bench"):
        x = synth.complex_array((n, n)) if fill == "splitmix" else synth.bench_fill_complex((n, n))
        y = np.zeros_like(x)
        api.ndfft(x, y, h, 1)
        assert L.last_path() == "pow2_reg"
        _all_lanes_vs_oracle(x, y, orc.ndfft_par, oh, 1, 1e-10, f"cfg2 {fill}")
        # Parseval on every lane: sum|X|^2 = n sum|x|^2
        e_in = (np.abs(x) ** 2).sum(axis=1); e_out = (np.abs(y) ** 2).sum(axis=1)
        assert np.abs(e_out / (n * e_in) - 1).max() < 1e-12
        # round trip through ndifft (Default 1/n) returns the input
        z = np.zeros_like(x); api.ndifft(y, z, h, 1)
        assert rel_global(z, x) < 1e-13
        _all_lanes_vs_oracle(y, z, orc.ndifft_par, oh, 1, 1e-10, f"cfg2' ndifft {fill}")
    # linearity: F(a x + b y) = a F(x) + b F(y) on a slab
    a, b = 0.75 - 0.5j, -1.25 + 2j
    x1 = synth.complex_array((256, n), offset=1); x2 = synth.complex_array((256, n), offset=99991)
    y1, y2, y3 = np.zeros_like(x1), np.zeros_like(x1), np.zeros_like(x1)
    api.ndfft(x1, y1, h, 1); api.ndfft(x2, y2, h, 1); api.ndfft(a * x1 + b * x2, y3, h, 1)
    assert rel_global(y3, a * y1 + b * y2) < 1e-13


def test_cfg3_r2c_then_c2c_8192_f32(L):
    """configs[2]: ndfft_r2c axis=0 then ndfft axis=1 on 8192x8192 f32; every lane of both steps and of the way back."""
    n = 8192; m = n // 2 + 1
    x = synth.real_array((n, n), np.float32)
    work = np.zeros((m, n), np.complex64)
    hr = handlers.R2cFftHandler(n, np.float32, _library=L); hc = handlers.FftHandler(n, np.float32, _library=L)
    ohr = orc.R2cFftHandler(n, np.float32); ohc = orc.FftHandler(n, np.float32)
    api.ndfft_r2c(x, work, hr, 0)
    _all_lanes_vs_oracle(x, work, orc.ndfft_r2c_par, ohr, 0, 1e-4, "cfg3A r2c axis0")
    out = np.zeros_like(work)
    api.ndfft(work, out, hc, 1)
    _all_lanes_vs_oracle(work, out, orc.ndfft_par, ohc, 1, 1e-4, "cfg3B c2c axis1")
    # round trip back to the real array
    w2 = np.zeros_like(work); api.ndifft(out, w2, hc, 1)
    _all_lanes_vs_oracle(out, w2, orc.ndifft_par, ohc, 1, 1e-4, "cfg3B' ndifft axis1")
    x2 = np.zeros_like(x); api.ndifft_r2c(w2, x2, hr, 0)
    _all_lanes_vs_oracle(w2, x2, orc.ndifft_r2c_par, ohr, 0, 1e-4, "cfg3A' c2r axis0")
    assert rel_global(x2, x) < 1e-4


def test_cfg4_dct_256x256x512_f64(L):
    """configs[3]: nddct2 axis=2 on 256x256x512 f64, all 65536 lanes; the other three DCT types on the same array;
    DCT-III undoes DCT-II up to 2n."""
    shape = (256, 256, 512); n = 512
    x = synth.real_array(shape)
    y = np.zeros_like(x); h = handlers.DctHandler(n, _library=L); oh = orc.DctHandler(n)
    api.nddct2(x, y, h, 2)
    _all_lanes_vs_oracle(x, y, orc.nddct2_par, oh, 2, 1e-10, "cfg4 dct2")
    z = np.zeros_like(x); api.nddct3(y, z, h, 2)
    assert rel_global(z / (2.0 * n), x) < 1e-12      # scipy: dct3(dct2(x)) = 2n x under the Default (x2) scaling
    _all_lanes_vs_oracle(y, z, orc.nddct3_par, oh, 2, 1e-10, "cfg4 dct3")
    for fn, ofn, nm in ((api.nddct1, orc.nddct1_par, "dct1"), (api.nddct4, orc.nddct4_par, "dct4")):
        fn(x, z, h, 2)
        _all_lanes_vs_oracle(x, z, ofn, oh, 2, 1e-10, f"cfg4 {nm}")
    # the same array along its strided axes (column tiles)
    h1 = handlers.DctHandler(256, _library=L); oh1 = orc.DctHandler(256)
    for axis in (1, 0):
        api.nddct2(x, y, h1, axis)
        _all_lanes_vs_oracle(x, y, orc.nddct2_par, oh1, axis, 1e-10, f"cfg4 dct2 axis={axis}")


def test_cfg5_shard_shape_8192x4096_f64(L):
    """configs[4] per-GPU shard (65536/8 rows): same kernel, bigger batch; all 8192 lanes."""
    rows, n = 8192, 4096
    x = synth.complex_array((rows, n)); y = np.zeros_like(x)
    h = handlers.FftHandler(n, _library=L)
    api.ndfft(x, y, h, 1)
    _all_lanes_vs_oracle(x, y, orc.ndfft_par, orc.FftHandler(n), 1, 1e-10, "cfg5 shard")


def test_cfg5_full_65536x4096_f64_one_gpu(L):
    """configs[4] WHOLE: ndfft axis=1 on the full 65536x4096 Complex<f64> array (4 GiB in, 4 GiB out) resident on one
    GPU, transformed by ONE call; every one of the 65536 lanes is then compared with the oracle, a block of rows at a
    time (the device result is downloaded per block, the oracle transforms the identical seeded block)."""
    torch = pytest.importorskip("torch")
    rows, n, blk = 65536, 4096, 4096
    dev = torch.device("cuda:0")
    xd = synth.complex_array_torch((rows, n), dev)
    yd = torch.empty_like(xd)
    h = handlers.FftHandler(n, _library=L); oh = orc.FftHandler(n)
    api.ndfft(xd, yd, h, 1)
    torch.cuda.synchronize()
    assert L.last_path() == "pow2_reg"
    worst = 0.0
    for r0 in range(0, rows, blk):
        xb = synth.complex_array((blk, n), offset=r0 * n)
        if r0 in (0, rows - blk):                                   # the device generator is the same stream
            assert np.array_equal(xd[r0:r0 + blk].cpu().numpy(), xb)
        yo = np.zeros_like(xb)
        orc.ndfft_par(xb, yo, oh, 1)
        got = yd[r0:r0 + blk].cpu().numpy()
        assert_close(got, yo, 1, 1e-10, f"cfg5 full rows {r0}..{r0 + blk}")
        worst = max(worst, rel_global(got, yo))
    # a checksum of checksums over the whole output: Parseval per lane, on the device
    e_in = (xd.real ** 2 + xd.imag ** 2).sum(dim=1); e_out = (yd.real ** 2 + yd.imag ** 2).sum(dim=1)
    assert float((e_out / (n * e_in) - 1).abs().max()) < 1e-12
    print(f"cfg5 full: worst global rel err over 16 blocks {worst:.2e}")


def test_device_resident_path_matches_host_path(L):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    n = 1024
    x = synth.complex_array((64, n)); y = np.zeros_like(x)
    h = handlers.FftHandler(n, _library=L)
    api.ndfft(x, y, h, 1)
    xd = torch.from_numpy(x).cuda(); yd = torch.zeros_like(xd)
    api.ndfft(xd, yd, h, 1)
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), y)
    # non-contiguous device views: axis 0 of a transposed tensor
    xt = xd.t()                      # shape (n, 64), strides (1, n)
    yt = torch.zeros((n, 64), dtype=xd.dtype, device="cuda")
    api.ndfft(xt, yt, h, 0)
    torch.cuda.synchronize()
    assert_close(yt.cpu().numpy(), y.T, 0, 1e-10, "transposed device view")


def test_perf_canary_never_fails(L):
    """NOT a pass / fail gate (box-to-box spread is several per cent and a slow lease must not turn the suite red): times the BASELINE row kernels for a
    few milliseconds and WARNS when one is more than 15 % slower than the best value on record (profiles/r07/r07d, r07j), so that a regression shows up
    in the warnings summary of whoever runs the GPU tests.  tools/bench_configs.py --compare is the real guard."""
    import time
    import warnings
    torch = pytest.importorskip("torch")
    from ndrustfft_amd import DctHandler, FftHandler, nddct2, ndfft
    dev = torch.device("cuda:0")
    rows = []
    x = torch.from_numpy(synth.complex_array((4096, 4096))).to(dev); y = torch.empty_like(x); h = FftHandler(4096)
    rows.append(("cfg2 ndfft axis=1 4096x4096 c128 (re-read loop)", lambda: ndfft(x, y, h, 1), 77.9))
    xr = torch.from_numpy(synth.real_array((256, 256, 512))).to(dev); yr = torch.empty_like(xr); hd = DctHandler(512)
    rows.append(("cfg4 nddct2 axis=2 256x256x512 f64 (re-read loop)", lambda: nddct2(xr, yr, hd, 2), 79.0))
    for name, fn, best_us in rows:
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.4:                     # clocks
            for _ in range(50): fn()
            torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50): fn()
            e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / 50)
        us = min(ts)
        print(f"perf canary: {name}: {us:.1f} us (best on record {best_us} us)")
        if us > 1.15 * best_us:
            warnings.warn(f"perf canary: {name} took {us:.1f} us, more than 15 % over its best recorded {best_us} us")


def test_hip_graph_capture_and_replay(L):
    """exec_device issues only kernel launches on the caller's stream (no allocation, no sync) on the row
    kernels, so a multi-axis transform can be captured once into a HIP graph and replayed."""
    torch = pytest.importorskip("torch")
    n = 512
    x = synth.complex_array((n, n)); xd = torch.from_numpy(x).cuda()
    w = torch.zeros_like(xd); y = torch.zeros_like(xd)
    h = handlers.FftHandler(n, _library=L)
    api.ndfft(xd, w, h, 1); api.ndfft(w, y, h, 0)           # warm-up: tables, function attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            api.ndfft(xd, w, h, 1)                           # axis 1: pow2_reg
            api.ndfft(w, y, h, 0)                            # axis 0: pow2_col
    y.zero_()
    g.replay(); torch.cuda.synchronize()
    assert_close(y.cpu().numpy(), np.fft.fft2(x), 1, 1e-10, "graph replay fft2")
    xd.copy_(torch.from_numpy(x * 2)); g.replay(); torch.cuda.synchronize()
    assert_close(y.cpu().numpy(), np.fft.fft2(2 * x), 1, 1e-10, "graph replay on new data")


def test_jit_disk_cache(tmp_path):
    """Specialised kernels are written to $NDFFT_JIT_CACHE and a second process loads them instead of compiling."""
    import subprocess, sys, time
    code = r'''
import sys, os, time, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import synth
from ndrustfft_amd import FftHandler, ndfft, _lib
x = synth.complex_array((200, 1000)); y = np.zeros_like(x)
t0 = time.perf_counter(); ndfft(x, y, FftHandler(1000), 1); dt = time.perf_counter() - t0
assert _lib.default().last_path() == "jit_reg"
assert np.abs(y - np.fft.fft(x, axis=1)).max() / np.abs(y).max() < 1e-12
print("CALL_S", dt)
''' % (ROOT, ROOT)
    env = dict(os.environ, NDFFT_JIT_CACHE=str(tmp_path))
    # second process: compiling is forbidden (NDFFT_JIT=cached), so "jit_reg" can only come from the cached code object
    for extra in ({}, {"NDFFT_JIT": "cached"}):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(env, **extra), timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        files = [f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]
        assert len(files) == 1, files
    # and without a cache the same switch sends the call to the LDS kernel (the assert inside the child fails)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       env=dict(os.environ, NDFFT_JIT_CACHE="0", NDFFT_JIT="cached"), timeout=600)
    assert r.returncode != 0 and "AssertionError" in r.stderr, r.stdout[-500:] + r.stderr[-1500:]


def test_fuzz_without_hiprtc():
    """NDFFT_JIT=0 (= a host without libhiprtc): every length still runs, on the LDS kernel, the four-step or the
    global-memory Bluestein -- same parity bar."""
    import subprocess, sys
    code = r'''
import sys, os
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import parity_suite as ps
from ndrustfft_amd import _lib
paths = ps.fuzz(_lib.default(), seed=23, count=200)
assert not any(p.startswith(("jit_", "blue_reg", "blue_col")) for p in paths), paths
print("NOJIT_OK", sorted(paths))
''' % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, NDFFT_JIT="0"), timeout=1200)
    assert r.returncode == 0 and "NOJIT_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_release_workspace(L):
    """ndfft_release_workspace frees the per-thread scratch; the next call simply allocates it again."""
    x = synth.real_array((4096, 96), np.float32); y = np.zeros((2049, 96), np.complex64)
    h = handlers.R2cFftHandler(4096, np.float32, _library=L)
    api.ndfft_r2c(x, y, h, 0); first = y.copy()
    assert L.c.ndfft_release_workspace() == 0
    y[:] = 0; api.ndfft_r2c(x, y, h, 0)
    assert np.array_equal(y, first)


def test_pinned_host_pipeline(L):
    """Arrays from ndfft_host_alloc: ndfft_exec runs as overlapped row chunks; same results as the plain host path."""
    from ndrustfft_amd import pinned_empty
    for name, shape, axis, rdt in (("ndfft", (512, 4096), 1, np.float64), ("ndfft_r2c", (300, 8, 1000), 2, np.float32),
                                   ("nddct2", (64, 96, 512), 1, np.float64), ("ndifft_r2c", (257, 2049), 1, np.float64)):
        sin, sout = ps.shapes_for(name, shape, axis)
        src = ps.make_input(name, sin, rdt)
        x = pinned_empty(sin, src.dtype, _library=L); x[...] = src
        odt = (np.complex64 if rdt == np.float32 else np.complex128) if ps.OPS[name][4] else np.dtype(rdt)
        y = pinned_empty(sout, odt, _library=L); y[...] = 0
        y2 = np.zeros(sout, odt)
        h, o = ps.handlers_for(name, shape[axis], rdt, L)
        ps.OPS[name][0](x, y, h, axis)
        ps.OPS[name][0](src, y2, h, axis)
        # (same kernels, but a chunk may fall on the other side of a specialisation threshold: compare to rounding)
        assert np.abs(y - y2).max() <= 50 * np.finfo(rdt).eps * np.abs(y2).max(), (name, shape)
        yo = np.zeros(sout, odt); ps.OPS[name][1](src, yo, o, axis)
        assert_close(y, yo, axis, TOL[np.dtype(rdt)], f"pinned {name} {shape}")


def test_jit_column_tiles_of_four_lanes(L):
    """Smooth non-power-of-two C2C lanes too long for an 8-lane column tile (n = 1500, 2000) take 4-lane tiles instead of the transpose route (round 3); real-output ops keep
    the 8-lane rule (their 4-lane rows measured 2-4 x slower) and fall to the transpose route as before."""
    for name, shape, rdt, want in (("ndfft", (1500, 48), np.float64, "jit_col"), ("ndifft", (2000, 40), np.float64, "jit_col"), ("ndfft", (2000, 37), np.float32, "jit_col"),
                                   ("ndfft", (3, 1500, 17), np.float64, "jit_col")):
        axis = len(shape) - 2
        for norm in ("Default", "None"):
            assert ps.run_case(L, name, shape, axis, rdt, norm=norm) == want, (name, shape)
    assert ps.run_case(L, "nddct2", (4000, 40), 0, np.float64) != "jit_col"


# ---- working precision: every kernel route within 3 x the oracle's own error against an 80-bit truth, and lanes independent (docs/accuracy.md) -------------
_ACC_SEEN = {}      # family -> routes its accuracy test saw (test_accuracy_required_routes)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("family", list(ps.ACC_GPU_FAMILIES))
def test_accuracy_routes(L, family, dt):
    """Lane L2 and worst bin, in eps, of every case of the family on uniform, impulse and graded inputs: e(library) <= 3 max(e(oracle), e(oracle on U[-1,1))),
    the oracle measured here at the same dtype against the same truth; every case on the route it names.  Each figure is printed before the assertion."""
    seen, _ = ps.accuracy_routes(L, ps.acc_gpu_cases(family, dt), verbose=True)
    _ACC_SEEN[family, dt] = seen


def _unaligned_device_transform(name, x, y, h, axis):
    """The call on torch tensors whose base pointers are only 8-byte aligned (jit.hip compiles the plain-recipe variant for them)."""
    import torch
    tdt = torch.from_numpy(np.zeros(1, x.dtype)).dtype
    buf = torch.zeros(x.size + 1, dtype=tdt, device="cuda:0"); out = torch.zeros(y.size + 1, dtype=tdt, device="cuda:0")
    xd = buf[1:].view(*x.shape); yd = out[1:].view(*y.shape)
    xd.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert xd.data_ptr() % 16 == 8 and yd.data_ptr() % 16 == 8
    ps.OPS[name][0](xd, yd, h, axis)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def test_accuracy_c64_rows_from_8_byte_aligned_base(L):
    """f32 C2C rows of 1000 points from a base pointer that is only 8-byte aligned: the same bar, and the lanes stay independent."""
    cases = [({}, name, (300, 1000), 1, np.float32, "C", "jit_reg") for name in ("ndfft", "ndifft")]
    ps.accuracy_routes(L, cases, transform=_unaligned_device_transform, verbose=True)
    ps.lane_isolation(L, cases, transform=_unaligned_device_transform)


def test_accuracy_required_routes(L):
    """The accuracy families together ran every kernel route (a family that has not run in this session runs here)."""
    for family in ps.ACC_GPU_FAMILIES:
        for dt in ("f64", "f32"):
            if (family, dt) not in _ACC_SEEN:
                _ACC_SEEN[family, dt] = ps.accuracy_routes(L, ps.acc_gpu_cases(family, dt))[0]
    seen = set().union(*_ACC_SEEN.values())
    assert ps.ACC_REQUIRED_ROUTES <= seen, sorted(ps.ACC_REQUIRED_ROUTES - seen)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("family", list(ps.ACC_GPU_FAMILIES))
def test_lane_isolation(L, family, dt):
    """The kept lanes of every case come out bit-identical whether their neighbours hold U[-1,1), values 1e30 / 1e250 times larger, or NaN: no arithmetic
    crosses lanes (wavefront swaps with the wrong bank mask, two lanes packed into one transform, a clamped tail load landing in a live register)."""
    ps.lane_isolation(L, ps.acc_gpu_cases(family, dt))


# ---- where the kernels touch memory: device-resident views between guard bands (parity_suite.guarded_views, docs/device_views.md) ------------------------
_GUARD_SEEN = {}      # (family, dt) -> routes its G1 calls took (test_guarded_views_required_routes)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("family", list(ps.ACC_GPU_FAMILIES))
def test_guarded_views(L, family, dt):
    """Every case of the family through ndfft_exec_device on allocations  band | image | band : dense (on the route the case names), padded rows with
    pitch_in != pitch_out, and -- first case of each route -- an odd pitch and a base pointer one element in.  Outside the output view every element keeps
    its sentinel, the input allocation comes back byte-identical, the view is finite (nothing skipped, nothing computed from the NaN bands) and correct."""
    seen, records = ps.guarded_views(L, ps.acc_gpu_cases(family, dt), verbose=True)
    _GUARD_SEEN[family, dt] = seen
    print("routes of the padded / offset geometries:", {k: sorted(v) for k, v in sorted(ps.guard_route_table(records).items())})


def test_guarded_views_extra(L):
    """The same checks on views that step backwards along the transform axis (both sides) and on an input whose outermost batch dimension has stride 0."""
    _, records = ps.guarded_views(L, ps.guard_extra_cases(), geometries=("NEG", "BCAST"), verbose=True)
    print("routes of the reversed / broadcast views:", {k: sorted(v) for k, v in sorted(ps.guard_route_table(records).items())})


def _guard_torch_cases():
    """The first row case and the first column case of every family and dtype."""
    out = []
    for family in ps.ACC_GPU_FAMILIES:
        for dt in ("f64", "f32"):
            cases = ps.acc_gpu_cases(family, dt)
            for col in (False, True):
                out += [c for c in cases if c[5] == "C" and (c[3] != len(c[2]) - 1) == col][:1]
    return out


def test_guarded_views_torch(L):
    """The banded construction on torch tensors through the public functions: a flat torch.full buffer per side, torch.as_strided views with the
    geometry's storage offset and strides, the call on the current stream -- api.py's stride and offset plumbing, which the ctypes calls above bypass."""
    import torch

    def tensor_of(a, v):
        t = torch.full((a.size,), ps._nan_of(a.dtype) if np.isnan(a.flat[0]) else float(a.flat[0].real), dtype=getattr(torch, a.dtype.name), device="cuda:0")
        tv = torch.as_strided(t, v.shape, [s // v.itemsize for s in v.strides], (v.__array_interface__["data"][0] - a.__array_interface__["data"][0]) // a.itemsize)
        tv.copy_(torch.from_numpy(np.ascontiguousarray(v)))
        assert t.data_ptr() % 16 == 0                  # (the view's alignment is the geometry's)
        return t, tv

    def run(name, h, xa, xv, ya, yv, axis):
        (xt, xtv), (yt, ytv) = tensor_of(xa, xv), tensor_of(ya, yv)
        ps.OPS[name][0](xtv, ytv, h, axis)
        path = L.last_path()
        torch.cuda.synchronize()
        return yt.cpu().numpy(), xt.cpu().numpy(), path
    ps.guarded_views(L, _guard_torch_cases(), geometries=("G1", "G2"), verbose=True, runner=run)


def test_guarded_views_required_routes(L):
    """The dense (G1) calls of the guard-band families together ran every kernel route (a family that has not run in this session runs here)."""
    for family in ps.ACC_GPU_FAMILIES:
        for dt in ("f64", "f32"):
            if (family, dt) not in _GUARD_SEEN:
                _GUARD_SEEN[family, dt] = ps.guarded_views(L, ps.acc_gpu_cases(family, dt), geometries=("G1",))[0]
    seen = set().union(*_GUARD_SEEN.values())
    assert ps.ACC_REQUIRED_ROUTES <= seen, sorted(ps.ACC_REQUIRED_ROUTES - seen)
