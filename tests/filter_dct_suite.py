"""Cases of nddct_filter on device arrays under a DctHandler: ndfft_exec_dct_filter_device (include/ndfft_mi355x_ext.h) driven through ctypes with devmem's helpers,
so that the same functions run on the CPU build of the kernel sources (tests/test_filter_dct_emul.py) and on the MI355X (tests/test_filter_dct_gpu.py).  The fused
route filter_dct_pow2 (filter_kernel.h: FILTER_DCT; compose.hip: filter_fused) and the calls that must stay on the composed route.

Expected values: the CPU oracle composed, nddct2 -> `*= g` in the working dtype -> nddct3 under the same normalisation; coarse bound helpers.TOL.  Working
precision: the bar of docs/accuracy.md, truth = scipy.fft.dct of type 2 and 3 one precision up, rescaled to the library's lane definitions
    C[k] = sum_j x[j] cos(pi (2j+1) k / (2n)),     y[j] = D[0] / 2 + sum_{k >= 1} D[k] cos(pi (2j+1) k / (2n)):
scipy's unnormalised DCT-II is 2 C, its DCT-III is x[0] + 2 sum_{k >= 1} x[k] cos(..) = 2 y (pinned by test_scipy_factors against the definition)."""
import ctypes

import numpy as np
import scipy.fft as sf

import accuracy as acc
import parity_suite as ps
from devmem import LAST, SENTINEL, DevBuf, _off, in_alloc, out_alloc, strides_of, view_mask
from helpers import TOL, assert_close
from ndrustfft_amd import _lib, api, handlers
from oracle import oracle_ctypes as orc
from weights_suite import make_weights

BOTH = (np.float64, np.float32)
NO_FUSE = _lib.FILTER_NO_FUSE
FUSED_D = "filter_dct_pow2"
FUSED_D_N = (128, 256, 512, 1024, 2048, 4096, 8192)          # kernels_filter.hip: NDFFT_FILTER_LENGTHS, as n = 2 F
SCALE_OF = {_lib.NORM_NONE: 1.0, _lib.NORM_DEFAULT: 4.0}
# (n = 2 F, the kernel is the complex one of length F: the radix lists of F = 128, 1024, 2048 in f64 and F = 2048 in f32 are no palindromes, so n = 256, 2048, 4096
#  in f64 and n = 4096 in f32 run their second pass set on a second twiddle table -- weight_placement's lengths hold both kinds per dtype)


def composed(path):
    return "+weights+" in path and FUSED_D not in path


def handler(L, n, rdt):
    return handlers.DctHandler(n, rdt, _library=L)


def make_x(shape, rdt, seed=1):
    return ps.make_input("nddct2", shape, rdt, offset=seed)


def make_g(n, rdt, seed=1, kind="general"):
    return make_weights("nddct2", n, rdt, seed, kind)          # n reals, moduli in [0.5, 2], any sign


def filt_call(L, h, xa, xv, ya, yv, axis, g, *, norm=_lib.NORM_DEFAULT, scale=0.0, flags=0, inplace=False, n_weights=None, check=True, entry="ndfft_exec_dct_filter_device"):
    """One call on device images of the allocations xa / ya, the views xv / yv into them giving the geometry (inplace: ya / yv are ignored, the output is the input
    view).  g None: a NULL pointer.  Returns (output allocation after the call, input allocation after the call, path, status)."""
    din = DevBuf(L, xa)
    dout = din if inplace else DevBuf(L, ya)
    if inplace:
        ya, yv = xa, xv
    dw = None
    try:
        wp = None
        if g is not None:
            g = np.ascontiguousarray(g)
            dw = DevBuf(L, g)
            wp = dw.p
        st = getattr(L.c, entry)(h._plan, ctypes.c_void_p(din.p.value + _off(xv, xa)), ctypes.c_void_p(dout.p.value + _off(yv, ya)), xv.ndim,
                                 api._i64(xv.shape), api._i64(strides_of(xv)), api._i64(strides_of(yv)), axis, wp,
                                 (len(g) if g is not None else 0) if n_weights is None else n_weights, norm, scale, flags, None)
        LAST["msg"] = L.c.ndfft_last_error().decode()
        if check:
            L.check(st)
        path = L.last_path() if st == _lib.OK else None
        L.check(L.c.ndfft_dev_sync(None))
        return dout.download(ya), din.download(xa), path, st
    finally:
        din.free()
        if not inplace:
            dout.free()
        if dw is not None:
            dw.free()


def oracle_filter(x, g, n, axis, rdt, norm=_lib.NORM_DEFAULT, scale=0.0):
    """The composed oracle on the C-contiguous array x: nddct2, `*= g` in the working dtype, nddct3, both under `norm` (SCALE: unscaled, then one multiply)."""
    x = np.ascontiguousarray(x)
    o = orc.DctHandler(n, rdt).normalization(orc.NORM_DEFAULT if norm == _lib.NORM_DEFAULT else orc.NORM_NONE)
    coef = np.zeros_like(x)
    orc.nddct2(x, coef, o, axis)
    coef *= np.asarray(g, coef.dtype).reshape([-1 if d == axis else 1 for d in range(x.ndim)])
    yo = np.zeros_like(x)
    orc.nddct3(coef, yo, o, axis)
    if norm == _lib.NORM_SCALE:
        yo *= np.dtype(rdt).type(scale)
    return yo


def hi_of(a):
    if a.dtype == np.float64:
        acc.require_long_double()
        return acc.LD
    return np.float64


def truth_dct2(x, axis):
    """C of the lanes of x (the definition above) one precision above x's."""
    return sf.dct(x.astype(hi_of(x)), type=2, axis=axis) / 2


def truth_filter(x, g, n, axis, s=4.0):
    """s DCT3(g (.) DCT2(x)) one precision above the input's."""
    hi = hi_of(x)
    gh = g.astype(hi).reshape([-1 if d == axis else 1 for d in range(x.ndim)])
    return hi(s) * sf.dct(truth_dct2(x, axis) * gh, type=3, axis=axis) / 2


def scipy_factors():
    """scipy's unnormalised DCT-II is 2 C and its DCT-III is 2 y, against the definitions summed in long double at n = 8."""
    acc.require_long_double()
    n, LD = 8, acc.LD
    x64 = np.random.default_rng(8).uniform(-1, 1, (1, n))
    x = x64[0].astype(LD)
    j = np.arange(n, dtype=LD)
    cosm = np.cos(np.arctan(LD(1)) * 4 * (2 * j[None, :] + 1) * j[:, None] / (2 * n))          # [k, j]
    C = cosm @ x
    y = x[0] / 2 + cosm[1:].T @ x[1:]
    tol = 64 * np.finfo(LD).eps * n
    assert np.abs(sf.dct(x, type=2) - 2 * C).max() <= tol, "scipy DCT-II is not 2 C"
    assert np.abs(sf.dct(x, type=3) - 2 * y).max() <= tol, "scipy DCT-III is not 2 y"
    assert np.abs(truth_dct2(x64, 1)[0] - C).max() <= tol
    assert np.abs(truth_filter(x64, np.ones(n), n, 1, 1.0)[0] - (n / 2) * x).max() <= tol * n, "unit weights do not return (n / 2) x"


def filter_case(L, shape, axis, rdt, *, layout="C", x=None, xa=None, xv=None, out_view=None, ya=None, yv=None, g=None, gkind="general",
                norm=_lib.NORM_DEFAULT, scale=0.0, flags=0, inplace=False, seed=1, want_path=None):
    """One call against the composed oracle.  Out of place: no element of the output allocation outside the view changes and the input allocation is
    bit-identical afterwards.  Returns (a copy of the output view, path)."""
    n = shape[axis]
    if xv is None:
        if x is None:
            x = make_x(shape, rdt, seed)
        xa, xv = in_alloc(x, layout)
    assert xv.shape == tuple(shape), (xv.shape, shape)
    if g is None:
        g = make_g(n, rdt, seed, gkind)
    if ya is None and not inplace:
        ya, yv = out_alloc("nddct2", shape, axis, rdt, out_view, layout)
    h = handler(L, n, rdt)
    got, xin, path, _ = filt_call(L, h, xa, xv, ya, yv, axis, g, norm=norm, scale=scale, flags=flags, inplace=inplace)
    if inplace:
        ya, yv = xa, xv
    gv = np.lib.stride_tricks.as_strided(got.reshape(-1)[_off(yv, ya) // ya.itemsize:], yv.shape, yv.strides)
    yo = oracle_filter(np.ascontiguousarray(xv), g, n, axis, rdt, norm, scale)
    what = f"dct filter shape={shape} axis={axis} {np.dtype(rdt).name} layout={layout} norm={norm} flags={flags} inplace={inplace} path={path}"
    assert_close(gv, yo, axis, TOL[np.dtype(rdt)], what)
    if want_path is not None:
        assert path == want_path, (path, want_path, what)
    if flags & NO_FUSE:
        assert composed(path), what
    if not inplace:
        mask = view_mask(ya, yv)
        assert np.array_equal(got[mask], np.full(int(mask.sum()), SENTINEL, got.dtype)), "an element outside the output view was written: " + what
        assert xin.tobytes() == np.ascontiguousarray(xa).tobytes(), "the input allocation was written: " + what
    else:
        mask = view_mask(xa, xv)
        assert got[mask].tobytes() == np.ascontiguousarray(xa)[mask].tobytes(), "an element outside the view was written in place: " + what
    return np.array(gv), path


# ---- 1. every instance ---------------------------------------------------------------------------------------------------------------------------------
def every_instance(L, n, rdt):
    """37 lanes leave a partial last workgroup for every LPB > 1."""
    filter_case(L, (37, n), 1, rdt, want_path=FUSED_D, seed=n)


# ---- 2. working precision: the bar of docs/accuracy.md, fused and composed under the same bar -----------------------------------------------------------------
def working_precision(L, n, rdt, verbose=False):
    """e(library) <= ACC_FACTOR max(e(composed oracle, this input), e(composed oracle, U[-1,1))), both metrics, every input, fused and NO_FUSE.  Nothing measured
    from the library enters the bar."""
    shape, axis = (37, n), 1
    g = make_g(n, rdt, seed=2)
    h = handler(L, n, rdt)
    bad, paths, uni = [], {}, None
    assert acc.INPUTS[0] == "uniform"
    for kind in acc.INPUTS:
        x = acc.make_input(kind, "nddct2", shape, axis, rdt, offset=n)
        t = acc.prepare(truth_filter(x, g, n, axis), axis)
        orac = acc.errors(oracle_filter(x, g, n, axis, rdt), t, axis, rdt)
        if kind == "uniform":
            uni = orac
        den = tuple(max(a, b) for a, b in zip(orac, uni))
        for flags in (0, NO_FUSE):
            ya, yv = out_alloc("nddct2", shape, axis, rdt)
            got, _, path, _ = filt_call(L, h, x, x, ya, yv, axis, g, flags=flags)
            paths[flags] = path
            lib = acc.errors(got, t, axis, rdt)
            line = f"{path} dct filter {shape} {np.dtype(rdt).name} {kind}: e_l2 {lib[0]:.3f} eps (bar's oracle {den[0]:.3f}), e_bin {lib[1]:.3f} eps (bar's oracle {den[1]:.3f})"
            if verbose:
                print(line, flush=True)
            if not all(l <= ps.ACC_FACTOR * d for l, d in zip(lib, den)):
                bad.append(line)
    assert not bad, "\n".join([f"{len(bad)} beyond {ps.ACC_FACTOR} x the oracle's own error"] + bad)
    assert paths[0] == FUSED_D and composed(paths[NO_FUSE]), paths


# ---- 3. the weights' placement ---------------------------------------------------------------------------------------------------------------------------
def weight_placement(L, cases=((np.float64, 128), (np.float64, 256), (np.float64, 2048), (np.float64, 4096), (np.float32, 512), (np.float32, 4096))):
    """g = e_k moves exactly coefficient k: s C[k] cos(pi (2j+1) k / (2n)), halved for k = 0.  k = 0 / n/2 and n/4 / 3n/4 are the bins the kernel's mirror exchange
    pairs with themselves, n/2 +- 1, 3n/4 and n - 1 sit on the mirror side (-Im), 37 is odd and a multiple of no radix."""
    for rdt, n in cases:
        x = make_x((5, n), rdt, seed=n + 1)
        C = truth_dct2(x, 1).astype(np.float64)
        j = np.arange(n)
        h = handler(L, n, rdt)
        for k in (0, 1, 37, n // 4, n // 2 - 1, n // 2, n // 2 + 1, 3 * n // 4, n - 1):
            g = np.zeros(n, rdt); g[k] = 1
            ya, yv = out_alloc("nddct2", (5, n), 1, rdt)
            got, _, path, _ = filt_call(L, h, x, x, ya, yv, 1, g)
            assert path == FUSED_D, path
            want = 4.0 * (0.5 if k == 0 else 1.0) * C[:, k:k + 1] * np.cos(np.pi * (2 * j + 1) * k / (2 * n))[None, :]
            assert_close(got, want, 1, TOL[np.dtype(rdt)], f"dct filter g = e_{k}, n = {n} {np.dtype(rdt).name}")


# ---- 4. unit weights ------------------------------------------------------------------------------------------------------------------------------------
def unit_weights(L, lengths=(128, 8192)):
    for rdt in BOTH:
        for n in lengths:
            x = make_x((5, n), rdt, seed=n)
            for norm, s in SCALE_OF.items():
                c, _ = filter_case(L, (5, n), 1, rdt, x=x, gkind="ones", norm=norm, want_path=FUSED_D)
                assert_close(c, s * (n / 2) * x.astype(np.float64), 1, TOL[np.dtype(rdt)], f"dct filter g = 1 n={n} norm={norm}")


# ---- 5. base and pitch (offsets and pitches in reals): every combination is fused ------------------------------------------------------------------------------
def _pitched(rows, n, pitch, base, dt, fill, x=None):
    a = np.full(base + rows * pitch + 3, fill, dt)
    v = np.lib.stride_tricks.as_strided(a[base:], (rows, n), (pitch * a.itemsize, a.itemsize))
    if x is not None:
        v[...] = x
    return a, v


def base_and_pitch(L, shapes=((37, 1024), (5, 8192))):
    for rdt in BOTH:
        for rows, n in shapes:
            x = make_x((rows, n), rdt, seed=n + 3)
            #                 base in/out, pitch in/out
            for bi, bo, pi, po in ((0, 0, n, n), (0, 0, n + 4, n + 8), (4, 8, n, n + 4),                              # 16-byte bases and pitches on both sides (f32 and f64)
                                   (0, 0, n + 2, n + 6), (2, 2, n, n), (2, 0, n + 4, n), (0, 2, n, n + 4),            # even: 16-byte for f64 only
                                   (0, 0, n + 1, n), (0, 0, n, n + 3), (0, 0, n + 1, n + 5),                           # an odd pitch on either side, on both
                                   (1, 0, n, n), (0, 1, n + 2, n + 2), (3, 1, n, n), (1, 3, n + 1, n + 3)):            # an odd base offset on either side, on both
                xa, xv = _pitched(rows, n, pi, bi, rdt, 0, x)
                ya, yv = _pitched(rows, n, po, bo, rdt, SENTINEL)
                filter_case(L, (rows, n), 1, rdt, xa=xa, xv=xv, ya=ya, yv=yv, seed=n, want_path=FUSED_D)


# ---- 6. sentinel window ---------------------------------------------------------------------------------------------------------------------------------
def sentinel_window(L, shapes=((37, 128), (5, 1024), (3, 8192))):
    """The output is a window of a larger sentinel-filled allocation (filter_case: nothing outside it changes, the input allocation is bit-identical)."""
    for rdt in BOTH:
        for rows, n in shapes:
            for flags in (0, NO_FUSE):
                for col in (4, 3):
                    _, path = filter_case(L, (rows, n), 1, rdt, out_view=((rows + 2, n + 7), np.s_[1:rows + 1, col:col + n]), flags=flags, want_path=None if flags else FUSED_D)
                    assert flags == 0 or composed(path), path


# ---- 7. in place --------------------------------------------------------------------------------------------------------------------------------------------
def in_place(L, shapes=((37, 256), (5, 8192))):
    for rdt in BOTH:
        for shape in shapes:
            x = make_x(shape, rdt, seed=shape[1])
            a, _ = filter_case(L, shape, 1, rdt, x=x, want_path=FUSED_D)
            b, _ = filter_case(L, shape, 1, rdt, x=x.copy(), inplace=True, want_path=FUSED_D)
            assert a.tobytes() == b.tobytes(), f"in place differs from out of place: {shape} {np.dtype(rdt).name}"


# ---- 8. the XCD map with a ragged last group ------------------------------------------------------------------------------------------------------------------
def xcd_tail(L, shapes=((131, 8192), (8197, 128))):
    """Both are past nblk >= 16 chunk (8 blocks of one 64 KiB lane; 16 blocks of 32 lanes of 1 KiB) with blocks left over after the last whole group."""
    for shape in shapes:
        filter_case(L, shape, 1, np.float64, want_path=FUSED_D, seed=7)


# ---- 9. lane isolation (the three-copy scheme of parity_suite.lane_isolation) -----------------------------------------------------------------------------------
def lane_isolation(L, shapes=((37, 128), (37, 1024), (9, 4096))):
    bad = []
    for rdt in BOTH:
        for shape in shapes:
            n = shape[1]
            keep = acc.kept_lanes(shape[0])
            km = keep[:, None]
            x = acc.make_input("uniform", "nddct2", shape, 1, rdt, offset=n)
            big = np.dtype(rdt).type(1e30 if np.dtype(rdt) == np.float32 else 1e250)
            xs = (x, (x * np.where(km, np.dtype(rdt).type(1), big)).astype(x.dtype), np.where(km, x, np.nan).astype(x.dtype))
            g = make_g(n, rdt, seed=3)
            h = handler(L, n, rdt)
            outs = []
            for xi in xs:
                ya, yv = out_alloc("nddct2", shape, 1, rdt)
                got, _, path, _ = filt_call(L, h, xi, xi, ya, yv, 1, g)
                assert path == FUSED_D, path
                outs.append(got[keep])
            what = f"{shape} {np.dtype(rdt).name}"
            if not np.isfinite(outs[0]).all():
                bad.append("non-finite output of a finite lane: " + what)
            for k, label in ((1, "scaled"), (2, "NaN")):
                if outs[0].tobytes() != outs[k].tobytes():
                    bad.append(f"kept lanes differ with {label} neighbours: " + what)
    assert not bad, "\n".join(bad)


# ---- 10. normalisation ------------------------------------------------------------------------------------------------------------------------------------
def normalisation(L, shape=(37, 512)):
    for rdt in BOTH:
        n = shape[1]
        x = make_x(shape, rdt, seed=n)
        for flags in (0, NO_FUSE):
            outs = {}
            for norm in (_lib.NORM_NONE, _lib.NORM_DEFAULT, _lib.NORM_SCALE):
                outs[norm], _ = filter_case(L, shape, 1, rdt, x=x, norm=norm, scale=0.37, flags=flags, want_path=None if flags else FUSED_D)
            what = f"{shape} {np.dtype(rdt).name} flags={flags}"
            assert np.array_equal(outs[_lib.NORM_DEFAULT], 4 * outs[_lib.NORM_NONE]), "DEFAULT is not exactly 4 x NONE: " + what
            if flags:      # composed: nddct3 pre-scales its INPUT by the scalar (lib.rs:736-741), so only the power-of-two factor is a pure one there; SCALE is filter_case's
                continue
            # fused: SCALE is one rounded multiply of the same value by the working-precision scalar: 2 eps covers that rounding and the other side's
            T = np.dtype(rdt).type
            eps = acc.LD(np.finfo(rdt).eps)
            for lo, f in ((_lib.NORM_DEFAULT, acc.LD(T(0.37)) / 4), (_lib.NORM_NONE, acc.LD(T(0.37)))):
                a = outs[_lib.NORM_SCALE].astype(acc.LD); b = outs[lo].astype(acc.LD) * f
                assert np.all(np.abs(a - b) <= 2 * eps * np.abs(a)), f"SCALE is no pure factor of norm {lo}: " + what


# ---- 11. layouts and what stays composed -----------------------------------------------------------------------------------------------------------------------
def layouts(L):
    for rdt in BOTH:
        filter_case(L, (256, 6), 0, rdt, layout="F", want_path=FUSED_D)                  # unit-stride lanes of 256 points at pitch 256
        _, path = filter_case(L, (256, 6), 0, rdt, layout="C")                            # strided lanes
        assert composed(path), path
        x = make_x((6, 256), rdt, seed=256)
        xa = np.ascontiguousarray(x[:, ::-1])
        _, path = filter_case(L, (6, 256), 1, rdt, xa=xa, xv=xa[:, ::-1])                # reversed stride along the axis
        assert composed(path), path
        _, path = filter_case(L, (37, 256), 1, rdt, flags=NO_FUSE)
        assert composed(path), path
        for shape in ((37, 64), (3, 16384), (6, 96)):
            assert shape[1] not in FUSED_D_N
            _, path = filter_case(L, shape, 1, rdt, seed=shape[1])
            assert composed(path), (path, shape)


# ---- 12. errors ------------------------------------------------------------------------------------------------------------------------------------------
def errors(L):
    n, rdt = 6, np.float64

    def refused(h, x, axis, g, want_st, **kw):
        ya = np.full(x.shape, SENTINEL, x.dtype)
        got, xin, _, st = filt_call(L, h, x, x, ya, ya, axis, g, check=False, **kw)
        assert st == want_st, (st, want_st, LAST["msg"])
        assert np.all(got == SENTINEL), "a refused call wrote its output"
        assert xin.tobytes() == x.tobytes()
        return LAST["msg"]
    h = handler(L, n, rdt)
    x = make_x((3, n), rdt)
    g = make_g(n, rdt)
    assert "weights" in refused(h, x, 1, None, _lib.ERR_INVALID_ARG, n_weights=n)
    for off in (1, -1):
        msg = refused(h, x, 1, g, _lib.ERR_INVALID_ARG, n_weights=n + off)
        assert str(n + off) in msg and str(n) in msg, msg
    for flags in (2, 4, 1 << 30, 3):
        refused(h, x, 1, g, _lib.ERR_INVALID_ARG, flags=flags)
    # the reference's panics, with the texts of ndfft_exec_device for NDFFT_OP_DCT2 -- also when the weights are wrong too (the order of the checks)
    x5 = make_x((3, 5), rdt)
    assert refused(h, x5, 1, g, _lib.ERR_SIZE_MISMATCH) == "Size mismatch in dct, got 5 expected 6"
    assert refused(h, x5, 1, None, _lib.ERR_SIZE_MISMATCH, flags=8) == "Size mismatch in dct, got 5 expected 6"
    assert refused(h, x, 2, g, _lib.ERR_AXIS) == "index out of bounds: the len is 2 but the index is 2"
    assert refused(h, x, 2, None, _lib.ERR_AXIS, n_weights=3, flags=8) == "index out of bounds: the len is 2 but the index is 2"
    ya = np.full((3, n), SENTINEL, x.dtype)
    _, _, _, st = filt_call(L, h, x, x, ya, ya, 1, g, norm=7, check=False)
    assert st == _lib.ERR_INVALID_ARG
    # the other two plan kinds are refused here, and the FFT filter's entry point still refuses a DCT plan
    for cls in (handlers.FftHandler, handlers.R2cFftHandler):
        assert "handler kind" in refused(cls(n, rdt, _library=L), x, 1, g, _lib.ERR_INVALID_ARG)
    assert "handler kind" in refused(h, x, 1, np.ones(n, np.complex128), _lib.ERR_INVALID_ARG, entry="ndfft_exec_filter_device")


# ---- 14. ABI ---------------------------------------------------------------------------------------------------------------------------------------------
def abi(L, root):
    import os
    import re
    assert L.c.ndfft_abi_minor() >= 6
    assert _lib.DCT_FILTER_SYMBOLS == ["ndfft_exec_dct_filter_device"]
    text = open(os.path.join(root, "include", "ndfft_mi355x_ext.h")).read()
    declared = sorted(set(re.findall(r"^int\s+(ndfft_\w+)\s*\(", text, re.M)))
    assert declared == sorted(_lib.EXT_SYMBOLS + _lib.FILTER_SYMBOLS + _lib.DCT_FILTER_SYMBOLS), declared
    for s in _lib.DCT_FILTER_SYMBOLS:
        assert hasattr(L.c, s) and getattr(L.c, s).argtypes is not None, s
