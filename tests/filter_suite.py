"""Cases of ndfft_filter on device arrays: ndfft_exec_filter_device (include/ndfft_mi355x_ext.h) driven through ctypes with devmem's helpers, so that the same
functions run on the CPU build of the kernel sources (tests/test_filter_emul.py) and on the MI355X (tests/test_filter_gpu.py).  Expected values: the CPU oracle
composed, forward -> `*= w` in the working dtype -> inverse; coarse bound helpers.TOL.  Working precision: the bar of docs/accuracy.md, truth = scipy.fft one
precision up on ifft(fft(x) * w)."""
import ctypes

import numpy as np
import scipy.fft as sf

import accuracy as acc
import parity_suite as ps
from devmem import LAST, SENTINEL, DevBuf, _off, in_alloc, out_alloc, strides_of, view_mask
from helpers import TOL, assert_close, cdt_of
from ndrustfft_amd import _lib, api, handlers
from oracle import oracle_ctypes as orc
from weights_suite import make_weights

BOTH = (np.float64, np.float32)
NO_FUSE = _lib.FILTER_NO_FUSE
FUSED = "filter_pow2"
FUSED_N = (64, 128, 256, 512, 1024, 2048, 4096)
# (radix lists that are no palindrome, i.e. a second twiddle table for the inverse pass set: f64 128, 1024, 2048 and f32 2048 -- all in FUSED_N)


def handler(L, n, rdt, r2c=False):
    return (handlers.R2cFftHandler if r2c else handlers.FftHandler)(n, rdt, _library=L)


def wname(r2c):
    return "ndifft_r2c" if r2c else "ndifft"           # (weights_suite.make_weights: n // 2 + 1 / n complex weights)


def filt_call(L, h, xa, xv, ya, yv, axis, w, *, norm=_lib.NORM_DEFAULT, scale=0.0, flags=0, inplace=False, n_weights=None, check=True):
    """One filter call on device images of the allocations xa / ya, the views xv / yv into them giving the geometry (inplace: ya / yv are ignored, the output
    is the input view).  w None: a NULL pointer.  Returns (output allocation after the call, input allocation after the call, path, status)."""
    din = DevBuf(L, xa)
    dout = din if inplace else DevBuf(L, ya)
    if inplace:
        ya, yv = xa, xv
    dw = None
    try:
        wp = None
        if w is not None:
            w = np.ascontiguousarray(w)
            dw = DevBuf(L, w)
            wp = dw.p
        st = L.c.ndfft_exec_filter_device(h._plan, ctypes.c_void_p(din.p.value + _off(xv, xa)), ctypes.c_void_p(dout.p.value + _off(yv, ya)), xv.ndim,
                                          api._i64(xv.shape), api._i64(strides_of(xv)), api._i64(strides_of(yv)), axis, wp,
                                          (len(w) if w is not None else 0) if n_weights is None else n_weights, norm, scale, flags, None)
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


def oracle_filter(x, w, n, axis, rdt, r2c=False, norm=_lib.NORM_DEFAULT, scale=0.0):
    """The composed oracle on the C-contiguous array x: forward, `*= w` in the working dtype, inverse under `norm` (SCALE: unscaled, then one multiply)."""
    x = np.ascontiguousarray(x)
    sshape = list(x.shape); sshape[axis] = n // 2 + 1 if r2c else n
    spec = np.zeros(sshape, cdt_of(rdt))
    cls = orc.R2cFftHandler if r2c else orc.FftHandler
    (orc.ndfft_r2c if r2c else orc.ndfft)(x, spec, cls(n, rdt), axis)
    spec *= np.asarray(w, spec.dtype).reshape([-1 if d == axis else 1 for d in range(x.ndim)])
    yo = np.zeros_like(x)
    o = cls(n, rdt).normalization(orc.NORM_DEFAULT if norm == _lib.NORM_DEFAULT else orc.NORM_NONE)
    (orc.ndifft_r2c if r2c else orc.ndifft)(spec, yo, o, axis)
    if norm == _lib.NORM_SCALE:
        yo *= np.dtype(rdt).type(scale)
    return yo


def make_x(shape, rdt, r2c=False, seed=1):
    return ps.make_input("ndfft_r2c" if r2c else "ndfft", shape, rdt, offset=seed)


def filter_case(L, shape, axis, rdt, *, r2c=False, layout="C", x=None, xa=None, xv=None, out_view=None, ya=None, yv=None, w=None, wkind="general",
                norm=_lib.NORM_DEFAULT, scale=0.0, flags=0, inplace=False, seed=1, want_path=None, want_in_path=None):
    """One call against the composed oracle.  Out of place: no element of the output allocation outside the view changes and the input allocation is
    bit-identical afterwards.  Returns (a copy of the output view, path)."""
    n = shape[axis]
    if xv is None:
        if x is None:
            x = make_x(shape, rdt, r2c, seed)
        xa, xv = in_alloc(x, layout)
    assert xv.shape == tuple(shape), (xv.shape, shape)
    if w is None:
        w = make_weights(wname(r2c), n, rdt, seed, wkind)
    if ya is None and not inplace:
        ya, yv = out_alloc("nddct2" if r2c else "ndfft", shape, axis, rdt, out_view, layout)
    h = handler(L, n, rdt, r2c)
    got, xin, path, _ = filt_call(L, h, xa, xv, ya, yv, axis, w, norm=norm, scale=scale, flags=flags, inplace=inplace)
    if inplace:
        ya, yv = xa, xv
    gv = np.lib.stride_tricks.as_strided(got.reshape(-1)[_off(yv, ya) // ya.itemsize:], yv.shape, yv.strides)
    yo = oracle_filter(np.ascontiguousarray(xv), w, n, axis, rdt, r2c, norm, scale)
    what = f"filter shape={shape} axis={axis} {np.dtype(rdt).name} r2c={r2c} layout={layout} norm={norm} flags={flags} inplace={inplace} path={path}"
    assert_close(gv, yo, axis, TOL[np.dtype(rdt)], what)
    if want_path is not None:
        assert path == want_path, (path, want_path, what)
    if want_in_path is not None:
        assert want_in_path in path, (path, want_in_path, what)
    if flags & NO_FUSE:
        assert "+weights+" in path, what
    if not inplace:
        mask = view_mask(ya, yv)
        assert np.array_equal(got[mask], np.full(int(mask.sum()), SENTINEL, got.dtype)), "an element outside the output view was written: " + what
        assert xin.tobytes() == np.ascontiguousarray(xa).tobytes(), "the input allocation was written: " + what
    else:
        mask = view_mask(xa, xv)
        assert got[mask].tobytes() == np.ascontiguousarray(xa)[mask].tobytes(), "an element outside the view was written in place: " + what
    return np.array(gv), path


# ---- 1. fused, every instance -------------------------------------------------------------------------------------------------------------------
def fused_instance(L, n, rdt):
    """37 lanes leave a partial last workgroup for every LPB > 1."""
    filter_case(L, (37, n), 1, rdt, want_path=FUSED, seed=n)


# ---- 2. f32 without 16-byte accesses ------------------------------------------------------------------------------------------------------------
def _pitched(rows, n, pitch, base, dt, fill, x=None):
    a = np.full(base + rows * pitch + 3, fill, dt)
    v = np.lib.stride_tricks.as_strided(a[base:], (rows, n), (pitch * a.itemsize, a.itemsize))
    if x is not None:
        v[...] = x
    return a, v


def f32_unaligned(L, shapes=((37, 1024), (5, 4096))):
    rdt, cdt = np.float32, np.complex64
    for rows, n in shapes:
        x = make_x((rows, n), rdt, seed=n + 3)
        #                 base in/out, pitch in/out
        for bi, bo, pi, po in ((1, 1, n, n), (1, 0, n, n), (0, 1, n, n),      # a base one element (8 bytes) into the allocation: the VEC = 1 instance
                               (0, 0, n + 1, n + 1), (1, 1, n + 1, n + 1),      # odd lane pitch
                               (0, 0, n, n + 3), (0, 0, n + 2, n + 4), (0, 0, n + 1, n + 2)):   # the two pitches differ (odd / even, even / even: 16-byte accesses)
            xa, xv = _pitched(rows, n, pi, bi, cdt, 0, x)
            ya, yv = _pitched(rows, n, po, bo, cdt, SENTINEL)
            filter_case(L, (rows, n), 1, rdt, xa=xa, xv=xv, ya=ya, yv=yv, want_path=FUSED, seed=n)


# ---- 3. the XCD map with a ragged last group ---------------------------------------------------------------------------------------------------------
def xcd_tail(L, shapes=((131, 4096), (8197, 64))):
    """Both are past nblk >= 16 chunk (8 blocks of one 64 KiB lane; 16 blocks of 32 lanes of 1 KiB) with blocks left over after the last whole group."""
    for shape in shapes:
        filter_case(L, shape, 1, np.float64, want_path=FUSED, seed=7)


# ---- 4. where memory is touched -------------------------------------------------------------------------------------------------------------------
def guarded_output(L):
    """The output is a view inside a larger allocation filled with the sentinel, with a padded pitch and an offset base (filter_case checks every element
    outside it, and the input allocation)."""
    for rdt in BOTH:
        for rows, n in ((37, 64), (5, 1024), (3, 4096)):
            for flags in (0, NO_FUSE):
                filter_case(L, (rows, n), 1, rdt, out_view=((rows + 2, n + 6), np.s_[1:rows + 1, 4:4 + n]), flags=flags, want_path=None if flags else FUSED)
        filter_case(L, (40, 96), 1, rdt, out_view=((42, 101), np.s_[1:41, 3:99]), want_in_path="+weights+")
        filter_case(L, (64, 40), 0, rdt, out_view=((66, 45), np.s_[2:66, 3:43]), want_in_path="+weights+")
        filter_case(L, (40, 64), 1, rdt, r2c=True, out_view=((42, 70), np.s_[1:41, 3:67]), want_in_path="+weights+")


# ---- 5. in place ----------------------------------------------------------------------------------------------------------------------------------
def in_place(L):
    for rdt in BOTH:
        for shape, axis, want in (((37, 256), 1, FUSED), ((5, 4096), 1, FUSED), ((40, 96), 1, None), ((64, 40), 0, None)):
            x = make_x(shape, rdt, seed=shape[axis])
            a, p0 = filter_case(L, shape, axis, rdt, x=x, want_path=want)
            b, p1 = filter_case(L, shape, axis, rdt, x=x.copy(), inplace=True, want_path=want)
            assert p0 == p1 and (want or "+weights+" in p0), (p0, p1)
            assert a.tobytes() == b.tobytes(), f"in place differs from out of place: {shape} axis={axis} {np.dtype(rdt).name} {p0}"


# ---- 6. the weights' placement -----------------------------------------------------------------------------------------------------------------------
def weight_placement(L, cases=((np.float64, 1024), (np.float64, 512), (np.float32, 256), (np.float32, 2048), (np.float64, 128))):
    for rdt, n in cases:
        cdt = cdt_of(rdt)
        x = make_x((5, n), rdt, seed=n + 1)
        X = sf.fft(x.astype(np.complex128), axis=1)
        j = np.arange(n)
        for k in (0, 1, n // 2, n - 1, 37):                  # 37: odd, a multiple of no radix
            w = np.zeros(n, cdt); w[k] = 1
            ya, yv = out_alloc("ndfft", (5, n), 1, rdt)
            got, _, path, _ = filt_call(L, handler(L, n, rdt), x, x, ya, yv, 1, w)
            assert path == FUSED, path
            want = X[:, k:k + 1] * np.exp(2j * np.pi * k * j / n)[None, :] / n
            assert_close(got, want, 1, TOL[np.dtype(rdt)], f"w = e_{k}, n = {n} {np.dtype(rdt).name}")
        for norm, s in ((_lib.NORM_NONE, 1.0), (_lib.NORM_DEFAULT, 1.0 / n)):
            ya, yv = out_alloc("ndfft", (5, n), 1, rdt)
            got, _, _, _ = filt_call(L, handler(L, n, rdt), x, x, ya, yv, 1, np.ones(n, cdt), norm=norm)
            assert_close(got, s * n * x.astype(np.complex128), 1, TOL[np.dtype(rdt)], f"w = 1, n = {n} {np.dtype(rdt).name} norm={norm}")


# ---- 7. working precision (docs/accuracy.md); fused against composed -----------------------------------------------------------------------------------
def truth_filter(x, w, n, axis, r2c=False):
    """ifft(fft(x) * w) (1 / n scaling) one precision above the input's."""
    hi_c, hi_r = (acc.CLD, acc.LD) if x.real.dtype == np.float64 else (np.complex128, np.float64)
    if x.real.dtype == np.float64:
        acc.require_long_double()
    wh = w.astype(hi_c).reshape([-1 if d == axis else 1 for d in range(x.ndim)])
    if not r2c:
        return sf.ifft(sf.fft(x.astype(hi_c), axis=axis) * wh, axis=axis)
    v = np.moveaxis(sf.rfft(x.astype(hi_r), axis=axis) * wh, axis, -1).copy()
    v[..., 0] = v[..., 0].real
    if n % 2 == 0:
        v[..., -1] = v[..., -1].real
    return sf.irfft(np.moveaxis(v, -1, axis), n=n, axis=axis)


def within_bar(L, shape, axis, rdt, *, r2c=False, flag_sets=(0,), kinds=acc.INPUTS, w=None, xs=None, verbose=False, want=None):
    """e(library) <= 3 max(e(composed oracle, this input), e(composed oracle, U[-1,1))), both metrics, every input, every flag set.  Nothing measured from the
    library enters the bar.  Returns the paths, one per flag set."""
    n = shape[axis]
    if w is None:
        w = make_weights(wname(r2c), n, rdt, seed=2)
    h = handler(L, n, rdt, r2c)
    bad, paths, uni = [], {}, None
    assert kinds[0] == "uniform"
    for kind in kinds:
        x = xs[kind] if xs else acc.make_input(kind, "ndfft_r2c" if r2c else "ndfft", shape, axis, rdt, offset=n)
        t = acc.prepare(truth_filter(x, w, n, axis, r2c), axis)
        orac = acc.errors(oracle_filter(x, w, n, axis, rdt, r2c), t, axis, rdt)
        if kind == "uniform":
            uni = orac
        den = tuple(max(a, b) for a, b in zip(orac, uni))
        for flags in flag_sets:
            ya, yv = out_alloc("nddct2" if r2c else "ndfft", shape, axis, rdt)
            got, _, path, _ = filt_call(L, h, x, x, ya, yv, axis, w, flags=flags)
            paths[flags] = path
            lib = acc.errors(got, t, axis, rdt)
            line = f"{path} filter {shape} axis={axis} {np.dtype(rdt).name} {kind}: e_l2 {lib[0]:.3f} eps (bar's oracle {den[0]:.3f}), e_bin {lib[1]:.3f} eps (bar's oracle {den[1]:.3f})"
            if verbose:
                print(line, flush=True)
            if not all(l <= ps.ACC_FACTOR * d for l, d in zip(lib, den)):
                bad.append(line)
            if want is not None and flags == 0 and path != want:
                bad.append(f"route {path} instead of {want}: " + line)
    assert not bad, "\n".join([f"{len(bad)} beyond {ps.ACC_FACTOR} x the oracle's own error"] + bad)
    return paths


def fused_against_composed(L, n, rdt, verbose=False):
    paths = within_bar(L, (37, n), 1, rdt, flag_sets=(0, NO_FUSE), verbose=verbose, want=FUSED)
    assert paths[0] == FUSED and "+weights+" in paths[NO_FUSE] and FUSED not in paths[NO_FUSE], paths


def conjugate_symmetric_weights(L, cases=((np.float64, 1024), (np.float32, 256), (np.float64, 96))):
    """A conjugate-symmetric w on real-valued complex input: the truth's imaginary parts are exactly zero, and the bar holds against that truth."""
    for rdt, n in cases:
        cdt = cdt_of(rdt)
        w = make_weights("ndifft", n, rdt, seed=5)
        w[0] = w[0].real; w[n // 2] = w[n // 2].real
        w[n // 2 + 1:] = np.conj(w[1:(n + 1) // 2][::-1])
        xs = {k: acc.make_input(k, "ndfft", (9, n), 1, rdt, offset=n).real.astype(cdt) for k in acc.INPUTS}
        for k in acc.INPUTS:
            assert np.abs(truth_filter(xs[k], w, n, 1).imag).max() <= 64 * np.finfo(np.float64 if rdt == np.float32 else acc.LD).eps * np.abs(xs[k]).max() * 2
        within_bar(L, (9, n), 1, rdt, w=w, xs=xs)


# ---- 8. normalisation ------------------------------------------------------------------------------------------------------------------------------------
def normalisation(L):
    for rdt in BOTH:
        for shape, axis, want in (((37, 512), 1, FUSED), ((40, 96), 1, None)):
            n = shape[axis]
            x = make_x(shape, rdt, seed=n)
            outs = {}
            for norm in (_lib.NORM_NONE, _lib.NORM_DEFAULT, _lib.NORM_SCALE):
                outs[norm], path = filter_case(L, shape, axis, rdt, x=x, norm=norm, scale=0.37, want_path=want)
                assert want or "+weights+" in path
            # SCALE against DEFAULT: a pure factor.  Each is one rounded multiply of the same value by the working-precision scalar: 2 eps covers both roundings
            T = np.dtype(rdt).type
            f = acc.LD(T(0.37)) / acc.LD(T(1.0) / T(n))
            eps = acc.LD(np.finfo(rdt).eps)
            for part in ("real", "imag"):
                a = getattr(outs[_lib.NORM_SCALE], part).astype(acc.LD); b = getattr(outs[_lib.NORM_DEFAULT], part).astype(acc.LD) * f
                assert np.all(np.abs(a - b) <= 2 * eps * np.abs(a)), f"SCALE is no pure factor of DEFAULT: {shape} {np.dtype(rdt).name} {part}"
            g = acc.LD(T(1.0) / T(n))
            for part in ("real", "imag"):
                a = getattr(outs[_lib.NORM_DEFAULT], part).astype(acc.LD); b = getattr(outs[_lib.NORM_NONE], part).astype(acc.LD) * g
                assert np.all(np.abs(a - b) <= 2 * eps * np.abs(a)), f"DEFAULT is no pure factor of NONE: {shape} {np.dtype(rdt).name} {part}"


# ---- 9. lane isolation (the three-copy scheme of parity_suite.lane_isolation) --------------------------------------------------------------------------
def lane_isolation(L, shapes=((37, 64), (37, 512), (9, 2048))):
    bad = []
    for rdt in BOTH:
        for shape in shapes:
            n = shape[1]
            keep = acc.kept_lanes(shape[0])
            km = keep[:, None]
            x = acc.make_input("uniform", "ndfft", shape, 1, rdt, offset=n)
            big = np.dtype(rdt).type(1e30 if np.dtype(rdt) == np.float32 else 1e250)
            xs = (x, (x * np.where(km, np.dtype(rdt).type(1), big)).astype(x.dtype), np.where(km, x, complex(np.nan, np.nan)).astype(x.dtype))
            w = make_weights("ndifft", n, rdt, seed=3)
            h = handler(L, n, rdt)
            outs = []
            for xi in xs:
                ya, yv = out_alloc("ndfft", shape, 1, rdt)
                got, _, path, _ = filt_call(L, h, xi, xi, ya, yv, 1, w)
                assert path == FUSED, path
                outs.append(got[keep])
            what = f"{shape} {np.dtype(rdt).name}"
            if not np.isfinite(outs[0]).all():
                bad.append("non-finite output of a finite lane: " + what)
            for k, label in ((1, "scaled"), (2, "NaN")):
                if outs[0].tobytes() != outs[k].tobytes():
                    bad.append(f"kept lanes differ with {label} neighbours: " + what)
    assert not bad, "\n".join(bad)


# ---- 10. composed, C2C kind ----------------------------------------------------------------------------------------------------------------------------
def composed_c2c_rows(L, n, rdt):
    filter_case(L, (3 if n >= 8192 else 5, n), 1, rdt, want_in_path="+weights+", seed=n)


def composed_c2c_layouts(L):
    for rdt in BOTH:
        for shape in ((64, 40), (96, 33)):
            for layout in ("C", "F"):
                # ((64, 40) in F layout has unit-stride lanes of 64 points: the fused kernel's by its predicate, so the composed route is asked for there)
                fusable = layout == "F" and shape[0] in FUSED_N
                _, path = filter_case(L, shape, 0, rdt, layout=layout, flags=NO_FUSE if fusable else 0, want_in_path="+weights+")
                assert FUSED not in path
                if fusable:
                    filter_case(L, shape, 0, rdt, layout=layout, want_path=FUSED)
        # a 3-D permuted view: the transform axis is the middle dim of the allocation
        x = make_x((4, 12, 6), rdt, seed=4)
        xa = np.ascontiguousarray(x.transpose(2, 1, 0)); xv = xa.transpose(2, 1, 0)
        ya = np.full((6, 12, 4), SENTINEL, cdt_of(rdt)); yv = ya.transpose(2, 1, 0)
        filter_case(L, (4, 12, 6), 1, rdt, xa=xa, xv=xv, ya=ya, yv=yv, want_in_path="+weights+")
        xa = np.ascontiguousarray(x.transpose(1, 2, 0)); xv = xa.transpose(2, 0, 1)
        filter_case(L, (4, 12, 6), 2, rdt, xa=xa, xv=xv, want_in_path="+weights+")
        # reversed strides on the input, along the axis (also at a fused length: no unit stride, so composed) and along the batch dim
        for n in (12, 256):
            x = make_x((6, n), rdt, seed=n)
            xa = np.ascontiguousarray(x[:, ::-1])
            filter_case(L, (6, n), 1, rdt, xa=xa, xv=xa[:, ::-1], want_in_path="+weights+")
            xa = np.ascontiguousarray(x[::-1])
            filter_case(L, (6, n), 1, rdt, xa=xa, xv=xa[::-1])
        # a broadcast batch dim: one lane serves every index, and is materialised in the spectrum image
        for n in (12, 256):
            xa = make_x((1, n), rdt, seed=n + 1)
            filter_case(L, (6, n), 1, rdt, xa=xa, xv=np.broadcast_to(xa, (6, n)))
            xa3 = make_x((1, 6, n), rdt, seed=n + 2)
            filter_case(L, (4, 6, n), 2, rdt, xa=xa3, xv=np.broadcast_to(xa3, (4, 6, n)), flags=NO_FUSE)
        # six dimensions, stepped in every batch dim: five un-mergeable batch dims, the slowest is peeled on the host
        shape = (2, 2, 2, 2, 2, 6)
        x = make_x(shape, rdt, seed=11)
        xa = np.zeros((4, 4, 4, 4, 4, 6), x.dtype); xa[::2, ::2, ::2, ::2, ::2] = x
        filter_case(L, shape, 5, rdt, xa=xa, xv=xa[::2, ::2, ::2, ::2, ::2], out_view=((4, 4, 4, 4, 4, 6), np.s_[1::2, ::2, 1::2, ::2, 1::2]), want_in_path="+weights+")


# ---- 11. composed, R2C kind ----------------------------------------------------------------------------------------------------------------------------
def composed_r2c(L, n, rdt):
    for shape, axis in (((5, n), 1), ((n, 6), 0)):
        x = make_x(shape, rdt, r2c=True, seed=n)
        w = make_weights("ndifft_r2c", n, rdt, seed=n)
        assert w[0].imag != 0 and w[-1].imag != 0
        a, path = filter_case(L, shape, axis, rdt, r2c=True, x=x, w=w, want_in_path="+weights+")
        # Im(DC) and, for even n, Im(Nyquist) of the product are dropped: with real input both products' real parts do not depend on Im(w) there
        w2 = w.copy(); w2[0] = complex(w[0].real, -3 * w[0].imag + 1)
        if n % 2 == 0:
            w2[-1] = complex(w[-1].real, 0.25 - w[-1].imag)
        b, _ = filter_case(L, shape, axis, rdt, r2c=True, x=x, w=w2, want_path=path)
        assert a.tobytes() == b.tobytes(), f"R2C filter n={n} axis={axis} {np.dtype(rdt).name}: the result depends on Im(w[0]) / Im(w[n/2])"
        for norm, s in ((_lib.NORM_NONE, 1.0), (_lib.NORM_DEFAULT, 1.0 / n)):
            c, _ = filter_case(L, shape, axis, rdt, r2c=True, x=x, wkind="ones", norm=norm)
            assert_close(c, s * n * x.astype(np.float64), axis, TOL[np.dtype(rdt)], f"R2C w = 1 n={n} norm={norm}")
    within_bar(L, (5, n), 1, rdt, r2c=True)


# ---- 12. errors ------------------------------------------------------------------------------------------------------------------------------------------
def errors(L):
    n, rdt = 6, np.float64

    def refused(h, x, axis, w, want_st, **kw):
        ya = np.full(x.shape, SENTINEL, x.dtype)
        got, xin, _, st = filt_call(L, h, x, x, ya, ya, axis, w, check=False, **kw)
        assert st == want_st, (st, want_st, LAST["msg"])
        assert np.all(got == SENTINEL), "a refused call wrote its output"
        assert xin.tobytes() == x.tobytes()
        return LAST["msg"]
    for r2c in (False, True):
        h = handler(L, n, rdt, r2c)
        x = make_x((3, n), rdt, r2c)
        w = make_weights(wname(r2c), n, rdt)
        m = len(w)
        assert "weights" in refused(h, x, 1, None, _lib.ERR_INVALID_ARG, n_weights=m)
        for off in (1, -1):
            msg = refused(h, x, 1, w, _lib.ERR_INVALID_ARG, n_weights=m + off)
            assert str(m + off) in msg and str(m) in msg, msg
        for flags in (2, 4, 1 << 30, 3):
            refused(h, x, 1, w, _lib.ERR_INVALID_ARG, flags=flags)
        # the reference's panics, with the texts of ndfft_exec_device for the forward op -- also when the weights are wrong too (the order of the checks)
        x5 = make_x((3, 5), rdt, r2c)
        assert refused(h, x5, 1, w, _lib.ERR_SIZE_MISMATCH) == "Size mismatch in fft, got 5 expected 6"
        assert refused(h, x5, 1, None, _lib.ERR_SIZE_MISMATCH, flags=8) == "Size mismatch in fft, got 5 expected 6"
        assert refused(h, x, 2, w, _lib.ERR_AXIS) == "index out of bounds: the len is 2 but the index is 2"
        ya = np.full((3, n), SENTINEL, x.dtype)
        _, _, _, st = filt_call(L, h, x, x, ya, ya, 1, w, norm=7, check=False)
        assert st == _lib.ERR_INVALID_ARG
    hd = handlers.DctHandler(n, rdt, _library=L)
    refused(hd, make_x((3, n), rdt, True), 1, np.ones(n, np.complex128), _lib.ERR_INVALID_ARG)
