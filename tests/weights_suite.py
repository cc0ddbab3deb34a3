"""Cases of Normalization::Weights on device arrays: ndfft_exec_weighted_device (include/ndfft_mi355x_ext.h) driven through ctypes with
ndfft_dev_alloc / upload / download, so that the same functions run on the CPU build of the kernel sources (tests/test_weights_emul.py) and on
the MI355X (tests/test_weights_gpu.py).  Truth: the CPU oracle under NORM_CUSTOM with `lane *= w`; coarse bound helpers.TOL, as run_case uses."""
import numpy as np
import scipy.fft as sf

import accuracy as acc
import parity_suite as ps
from devmem import LAST, OPC, SENTINEL, DevBuf, _off, dev_call, in_alloc, out_alloc, strides_of, view_mask      # noqa: F401 (the tests reach them as ws.*)
from helpers import TOL, assert_close, cdt_of
from ndrustfft_amd import _lib, api, handlers
from oracle import oracle_ctypes as orc

WEIGHTED = ("ndifft", "ndifft_r2c", "nddct1", "nddct2", "nddct3", "nddct4")
FORWARD = ("ndfft", "ndfft_r2c")
DCTS = ("nddct1", "nddct2", "nddct3", "nddct4")
BOTH = (np.float64, np.float32)


def wlen(name, n):
    """Length of the weighted lane of op `name` for handler length n."""
    return n // 2 + 1 if name == "ndifft_r2c" else n


def wdtype(name, rdt):
    return np.dtype(rdt) if name in DCTS else np.dtype(cdt_of(rdt))


def make_weights(name, n, rdt, seed=1, kind="general"):
    """general: moduli in [0.5, 2], any phase (real ops: any sign); real: complex weights with zero imaginary part; ones."""
    m = wlen(name, n)
    rng = np.random.default_rng(1000 * seed + n)
    mod = rng.uniform(0.5, 2.0, m)
    dt = wdtype(name, rdt)
    if kind == "ones":
        return np.ones(m, dt)
    if dt.kind != "c":
        return (mod * rng.choice([-1.0, 1.0], m)).astype(dt)
    if kind == "real":
        return (mod * rng.choice([-1.0, 1.0], m)).astype(dt)
    return (mod * np.exp(2j * np.pi * rng.uniform(0, 1, m))).astype(dt)


def oracle_weighted(name, x, w, n, axis, rdt):
    """The oracle's result of op `name` on the C-contiguous array x under NORM_CUSTOM with lane *= w."""
    _, sout = ps.shapes_for(name, _full_shape(name, x.shape, n, axis), axis)
    odt = cdt_of(rdt) if ps.OPS[name][4] else np.dtype(rdt)
    yo = np.zeros(sout, odt)

    def fn(lane):
        np.multiply(lane, w, out=lane)
    o = getattr(orc, ps.OPS[name][2])(n, rdt).normalization(orc.NORM_CUSTOM, fn)
    ps.OPS[name][1](np.ascontiguousarray(x), yo, o, axis)
    return yo


def _full_shape(name, in_shape, n, axis):
    s = list(in_shape); s[axis] = n
    return tuple(s)


def weighted_case(L, name, shape, axis, rdt, *, layout="C", x=None, xa=None, xv=None, out_view=None, wkind="general", w=None, w_offset=0, seed=1, want_path=None):
    """One weighted call against the oracle; every element of the output allocation outside the view keeps the sentinel.  Returns (output view, path)."""
    n = shape[axis]
    sin, _ = ps.shapes_for(name, shape, axis)
    if xv is None:
        if x is None:
            x = ps.make_input(name, sin, rdt, offset=seed)
        xa, xv = in_alloc(x, layout)
    assert xv.shape == tuple(sin), (xv.shape, sin)
    if w is None:
        w = make_weights(name, n, rdt, seed, wkind)
    ya, yv = out_alloc(name, shape, axis, rdt, out_view, layout)
    h = getattr(handlers, ps.OPS[name][2])(n, rdt, _library=L)
    got, path, _ = dev_call(L, h, name, xa, xv, ya, yv, axis, w, w_offset=w_offset)
    gv = np.lib.stride_tricks.as_strided(got.reshape(-1)[_off(yv, ya) // ya.itemsize:], yv.shape, yv.strides)
    yo = oracle_weighted(name, np.ascontiguousarray(xv), w, n, axis, rdt)
    what = f"weighted {name} shape={shape} axis={axis} {np.dtype(rdt).name} layout={layout} path={path}"
    assert_close(gv, yo, axis, TOL[np.dtype(rdt)], what)
    if name in FORWARD:
        assert "weights" not in path, path
    elif name == "ndifft":
        assert path.endswith("+weights"), path
    else:
        assert path.startswith("weights+"), path
    if want_path is not None:
        assert path == want_path, (path, want_path)
    mask = view_mask(ya, yv)
    assert np.array_equal(got[mask], np.full(int(mask.sum()), SENTINEL, got.dtype)), "an element outside the output view was written: " + what
    return np.array(gv), path


# ---- 1. every op x dtype on rows ---------------------------------------------------------------------------------------------------------------
def rows(L, sizes=(6, 9, 16)):
    for rdt in BOTH:
        for n in sizes:
            for name in WEIGHTED:
                weighted_case(L, name, (5, n), 1, rdt)
            for name in FORWARD:      # ignored: bitwise the unweighted result, with NULL and with non-NULL weights
                sin, _ = ps.shapes_for(name, (5, n), 1)
                x = ps.make_input(name, sin, rdt)
                ya, yv = out_alloc(name, (5, n), 1, rdt)
                h = getattr(handlers, ps.OPS[name][2])(n, rdt, _library=L)
                plain, p0, _ = dev_call(L, h, name, x, x, ya, yv, 1, weighted=False, norm=_lib.NORM_DEFAULT)
                null, p1, _ = dev_call(L, h, name, x, x, ya, yv, 1, None)
                some, p2, _ = dev_call(L, h, name, x, x, ya, yv, 1, make_weights("ndifft", 3, rdt), n_weights=3)
                assert p0 == p1 == p2, (p0, p1, p2)
                assert plain.tobytes() == null.tobytes() == some.tobytes(), f"{name} n={n}: a forward op looked at the weights"


# ---- 2. columns, C and F layout -----------------------------------------------------------------------------------------------------------------
def columns(L, sizes=(8, 9), names=WEIGHTED, dtypes=BOTH):
    for rdt in dtypes:
        for n in sizes:
            for name in names:
                for layout in ("C", "F"):
                    weighted_case(L, name, (n, 70), 0, rdt, layout=layout)
                    weighted_case(L, name, (3, n, 5), 1, rdt, layout=layout)


# ---- 3. views -----------------------------------------------------------------------------------------------------------------------------------
def views(L):
    for rdt in BOTH:
        for name in ("ndifft", "ndifft_r2c", "nddct2", "nddct1"):
            n = 12
            sin, sout = ps.shapes_for(name, (6, n), 1)
            x = ps.make_input(name, sin, rdt, offset=3)
            # negative axis stride
            xa = np.ascontiguousarray(x[:, ::-1])
            weighted_case(L, name, (6, n), 1, rdt, xa=xa, xv=xa[:, ::-1])
            # stepped batch dim (input), stepped + padded output view: holes between the lanes and inside them
            xa = np.zeros((12, sin[1]), x.dtype); xa[::2] = x
            weighted_case(L, name, (6, n), 1, rdt, xa=xa, xv=xa[::2], out_view=((13, 2 * sout[1] + 3), np.s_[1::2, 2:2 + 2 * sout[1]:2]))
            weighted_case(L, name, (6, n), 1, rdt, xa=xa, xv=xa[::2], out_view=((8, sout[1] + 5), np.s_[1:7, 3:3 + sout[1]]))
            # stride-0 batch dim on the input: one lane serves every index
            xa = np.ascontiguousarray(x[:1])
            weighted_case(L, name, (6, n), 1, rdt, xa=xa, xv=np.broadcast_to(xa, sin))
            xa3 = np.ascontiguousarray(ps.make_input(name, (1,) + tuple(sin), rdt, offset=5))
            weighted_case(L, name, (4, 6, n), 2, rdt, xa=xa3, xv=np.broadcast_to(xa3, (4,) + tuple(sin)))
            # stride-0 TRANSFORM axis: every element of the lane is the same number, the weighted lane is not -- the image materialises the axis
            xc = ps.make_input(name, (6, 1), rdt, offset=13)
            weighted_case(L, name, (6, n), 1, rdt, xa=xc, xv=np.broadcast_to(xc, sin))
            xc = ps.make_input(name, (1, 7), rdt, offset=14)
            weighted_case(L, name, (n, 7), 0, rdt, xa=xc, xv=np.broadcast_to(xc, (sin[1], 7)))
            xc = ps.make_input(name, (1, 1), rdt, offset=15)
            weighted_case(L, name, (1, n), 1, rdt, xa=xc, xv=np.broadcast_to(xc, (1, sin[1])))
            # the transform axis is not the contiguous one and the view is stepped along it
            xs = ps.make_input(name, (sin[1], 7), rdt, offset=9)
            xa = np.zeros((2 * sin[1], 7), xs.dtype); xa[::2] = xs
            weighted_case(L, name, (n, 7), 0, rdt, xa=xa, xv=xa[::2], out_view=((sout[1], 9), np.s_[:, 1:8]))
    # lanes / inner dims whose length is no multiple of the 16-byte vector on pitches that are: the vector path with its element-wide tail, rows and columns
    for rdt in BOTH:
        for name in ("nddct2", "ndifft", "ndifft_r2c"):
            for n in (5, 6, 7, 10):
                sin, sout = ps.shapes_for(name, (5, n), 1)
                x = ps.make_input(name, sin, rdt, offset=n)
                xa = np.zeros((5, 12), x.dtype); xa[:, :sin[1]] = x
                weighted_case(L, name, (5, n), 1, rdt, xa=xa, xv=xa[:, :sin[1]], out_view=((5, 12), np.s_[:, :sout[1]]))
            sin, sout = ps.shapes_for(name, (8, 70), 0)
            x = ps.make_input(name, sin, rdt, offset=70)
            xa = np.zeros((sin[0], 72), x.dtype); xa[:, :70] = x
            weighted_case(L, name, (8, 70), 0, rdt, xa=xa, xv=xa[:, :70], out_view=((sout[0], 72), np.s_[:, :70]))
            sin, sout = ps.shapes_for(name, (3, 8, 5), 1)
            x = ps.make_input(name, sin, rdt, offset=5)
            xa = np.zeros(sin[:2] + (8,), x.dtype); xa[:, :, :5] = x
            weighted_case(L, name, (3, 8, 5), 1, rdt, xa=xa, xv=xa[:, :, :5], out_view=(sout[:2] + (8,), np.s_[:, :, :5]))
    # base pointers one element into the allocation: only element-aligned (f32 real and c64), data and weights
    for name, shape, axis in (("nddct2", (5, 16), 1), ("nddct3", (16, 70), 0), ("ndifft", (5, 16), 1), ("ndifft", (16, 70), 0), ("ndifft_r2c", (5, 30), 1)):
        sin, sout = ps.shapes_for(name, shape, axis)
        x = ps.make_input(name, sin, np.float32, offset=7)
        xa = np.zeros(x.size + 1, x.dtype); xa[1:] = x.reshape(-1)
        tot = int(np.prod(sout))
        for w_offset in (0, 1):
            weighted_case(L, name, shape, axis, np.float32, xa=xa, xv=xa[1:].reshape(sin), w_offset=w_offset)
        # ... and the output (the in-place pass of ndifft works on it)
        ya_shape = (tot + 3,)
        odt = cdt_of(np.float32) if ps.OPS[name][4] else np.dtype(np.float32)
        n = shape[axis]
        w = make_weights(name, n, np.float32)
        ya = np.full(ya_shape, SENTINEL, odt); yv = ya[1:1 + tot].reshape(sout)
        h = getattr(handlers, ps.OPS[name][2])(n, np.float32, _library=L)
        got, path, _ = dev_call(L, h, name, xa, xa[1:].reshape(sin), ya, yv, axis, w)
        assert_close(got[1:1 + tot].reshape(sout), oracle_weighted(name, x, w, n, axis, np.float32), axis, TOL[np.dtype(np.float32)], f"offset output {name} {shape} {path}")
        assert got[0] == SENTINEL and np.all(got[1 + tot:] == SENTINEL)
    # six dimensions, stepped in every batch dim: five un-mergeable batch dims -> the slowest is peeled on the host, every piece is weighted
    for rdt in BOTH:
        for name in ("ndifft", "nddct2", "ndifft_r2c"):
            shape = (2, 2, 2, 2, 2, 6)
            sin, sout = ps.shapes_for(name, shape, 5)
            x = ps.make_input(name, sin, rdt, offset=11)
            xa = np.zeros((4, 4, 4, 4, 4, sin[5]), x.dtype); xa[::2, ::2, ::2, ::2, ::2] = x
            weighted_case(L, name, shape, 5, rdt, xa=xa, xv=xa[::2, ::2, ::2, ::2, ::2], out_view=((4, 4, 4, 4, 4, sout[5]), np.s_[1::2, ::2, 1::2, ::2, 1::2]))


# ---- 4. exactness: a lone IEEE multiply has nothing to contract with ------------------------------------------------------------------------------
def exactness(L, sizes=(6, 9, 16)):
    for rdt in BOTH:
        for shape_of, axis in ((lambda n: (5, n), 1), (lambda n: (n, 70), 0)):
            for n in sizes:
                for name in DCTS + ("ndifft_r2c",):
                    shape = shape_of(n)
                    sin, _ = ps.shapes_for(name, shape, axis)
                    x = ps.make_input(name, sin, rdt, offset=n)
                    w = make_weights(name, n, rdt, kind="real")
                    ya, yv = out_alloc(name, shape, axis, rdt)
                    h = getattr(handlers, ps.OPS[name][2])(n, rdt, _library=L)
                    got, path, _ = dev_call(L, h, name, x, x, ya, yv, axis, w)
                    xw = (x * w.reshape([-1 if d == axis else 1 for d in range(x.ndim)])).astype(x.dtype)   # the same multiply on the host, same dtype
                    ref, path0, _ = dev_call(L, h, name, xw, xw, ya, yv, axis, weighted=False, norm=_lib.NORM_NONE)
                    assert path == "weights+" + path0, f"{name} {shape}: the image took route {path}, the caller's array {path0}"
                    assert np.array_equal(got, ref), f"{name} {shape} {np.dtype(rdt).name}: weighted call differs from NORM_NONE on the weighted input ({path})"
                for name in WEIGHTED:       # all-ones weights: the NORM_NONE result, not the Default one
                    shape = shape_of(n)
                    sin, _ = ps.shapes_for(name, shape, axis)
                    x = ps.make_input(name, sin, rdt, offset=n + 1)
                    ya, yv = out_alloc(name, shape, axis, rdt)
                    h = getattr(handlers, ps.OPS[name][2])(n, rdt, _library=L)
                    got, path, _ = dev_call(L, h, name, x, x, ya, yv, axis, make_weights(name, n, rdt, kind="ones"))
                    ref, path0, _ = dev_call(L, h, name, x, x, ya, yv, axis, weighted=False, norm=_lib.NORM_NONE)
                    dflt, _, _ = dev_call(L, h, name, x, x, ya, yv, axis, weighted=False, norm=_lib.NORM_DEFAULT)
                    assert path.replace("weights+", "").replace("+weights", "") == path0, (path, path0)
                    assert np.array_equal(got, ref), f"{name} {shape} {np.dtype(rdt).name}: all-ones weights differ from NORM_NONE ({path})"
                    assert not np.array_equal(got, dflt), f"{name} {shape}: all-ones weights gave the Default scaling"


# ---- 5. ndifft_r2c: Im(DC) and Im(Nyquist) are dropped AFTER the weighting ------------------------------------------------------------------------
def c2r_end_points(L):
    for rdt in BOTH:
        for n in (8, 9, 16, 15):
            w = make_weights("ndifft_r2c", n, rdt, seed=n)
            assert w[0].imag != 0 and w[-1].imag != 0
            weighted_case(L, "ndifft_r2c", (5, n), 1, rdt, w=w)
            weighted_case(L, "ndifft_r2c", (n, 6), 0, rdt, w=w)


# ---- 6. working precision (docs/accuracy.md) -------------------------------------------------------------------------------------------------------
def _truth_weighted(name, x, w, n, axis):
    """The weighted op without any other scaling, one precision above the input's, from the weighted input (pre ops) / times w (ndifft)."""
    hi_c, hi_r = (acc.CLD, acc.LD) if x.real.dtype == np.float64 else (np.complex128, np.float64)
    if x.real.dtype == np.float64:
        acc.require_long_double()
    xh = x.astype(hi_c if np.iscomplexobj(x) else hi_r)
    wh = w.astype(hi_c if np.iscomplexobj(w) else hi_r).reshape([-1 if d == axis else 1 for d in range(x.ndim)])
    if name == "ndifft":
        return sf.ifft(xh, axis=axis) * n * wh
    xh = xh * wh
    if name == "ndifft_r2c":
        v = np.moveaxis(xh.copy(), axis, -1)
        v[..., 0] = v[..., 0].real
        if n % 2 == 0:
            v[..., -1] = v[..., -1].real
        return sf.irfft(np.moveaxis(v, -1, axis), n=n, axis=axis) * n
    return sf.dct(xh, type=acc.DCT_TYPE[name], axis=axis) / 2


def working_precision(L, cases=(("ndifft", (64, 256)), ("ndifft_r2c", (64, 256)), ("nddct2", (32, 128))), verbose=False):
    bad = []
    for name, rows_shape in cases:
        for rdt in BOTH:
            for shape, axis in ((rows_shape, 1), (rows_shape[::-1], 0)):
                n = shape[axis]
                sin, sout = ps.shapes_for(name, shape, axis)
                x = acc.make_input("uniform", name, sin, axis, rdt, offset=n)
                w = make_weights(name, n, rdt, seed=2)
                ya, yv = out_alloc(name, shape, axis, rdt)
                h = getattr(handlers, ps.OPS[name][2])(n, rdt, _library=L)
                got, path, _ = dev_call(L, h, name, x, x, ya, yv, axis, w)
                yo = oracle_weighted(name, x, w, n, axis, rdt)
                t = acc.prepare(_truth_weighted(name, x, w, n, axis), axis)
                lib = acc.errors(got, t, axis, rdt); orac = acc.errors(yo, t, axis, rdt)
                line = f"{path} {name} {shape} axis={axis} {np.dtype(rdt).name}: e_l2 {lib[0]:.3f} eps (oracle {orac[0]:.3f}), e_bin {lib[1]:.3f} eps (oracle {orac[1]:.3f})"
                if verbose:
                    print(line, flush=True)
                if not all(l <= ps.ACC_FACTOR * o for l, o in zip(lib, orac)):
                    bad.append(line)
    assert not bad, "\n".join([f"{len(bad)} beyond {ps.ACC_FACTOR} x the oracle's own error"] + bad)


# ---- 7. several blocks; the pass's image beside the scratch arrays of a multi-pass route (MI355X only: sizes) --------------------------------------
def first_multi_pass_length(L, kind, rdt):
    """Shortest handler length whose MAIN slot ndfft_explain_plan reports as a multi-pass route (four-step, or Bluestein over global memory).  The scan
    starts at 4000 to stay quick (a plan per length): scanned once from 1024, every length up to 4096 runs in one launch and 4097 is the first that does
    not, for the three kinds and both dtypes."""
    for n in range(4000, 70000):
        main = [l for l in L.explain_plan(kind, _lib.F32 if np.dtype(rdt) == np.float32 else _lib.F64, n).splitlines() if l.startswith("slot=MAIN")]
        if main and ("route=four_step" in main[0] or "blue_global" in main[0]):
            return n
    raise AssertionError("no multi-pass length below 70000")


def multi_pass_routes(L):
    """The pass's image (the ninth scratch slot) beside the scratch arrays of the multi-pass routes: the row four-step, the transpose route (a strided axis)
    and the packed route (an output view stepped along the axis), each twice on the same stream with different data."""
    for name, kind in (("nddct2", _lib.KIND_DCT), ("ndifft_r2c", _lib.KIND_R2C)):
        n = first_multi_pass_length(L, kind, np.float64)
        _, sout = ps.shapes_for(name, (4, n), 1)
        seen = []
        for shape, axis, out_view, prefix in (((4, n), 1, None, "weights+"), ((n, 16), 0, None, "weights+transpose+"),
                                              ((4, n), 1, ((4, 2 * sout[1]), np.s_[:, ::2]), "weights+pack+")):
            paths = set()
            for seed in (1, 2):
                _, path = weighted_case(L, name, shape, axis, np.float64, seed=seed, out_view=out_view)
                paths.add(path)
            assert len(paths) == 1 and path.startswith(prefix), (name, shape, paths, prefix)
            seen.append(path)
        assert not seen[0].startswith("weights+transpose+") and not seen[0].startswith("weights+pack+"), seen


def multi_block(L):
    for seed in (1, 2):       # twice on the same stream with different data
        weighted_case(L, "ndifft", (300, 1030), 1, np.float32, seed=seed)
        weighted_case(L, "ndifft", (1030, 300), 0, np.float32, seed=seed)


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------------------
def errors(L):
    for name, n in (("ndifft", 6), ("ndifft_r2c", 6), ("nddct1", 6), ("nddct4", 5)):
        sin, _ = ps.shapes_for(name, (3, n), 1)
        x = ps.make_input(name, sin, np.float64)
        ya, yv = out_alloc(name, (3, n), 1, np.float64)
        h = getattr(handlers, ps.OPS[name][2])(n, np.float64, _library=L)
        w = make_weights(name, n, np.float64)
        m = wlen(name, n)
        _, _, st = dev_call(L, h, name, x, x, ya, yv, 1, w, n_weights=m + 1, check=False)
        msg = LAST["msg"]
        assert st == _lib.ERR_INVALID_ARG and str(m + 1) in msg and str(m) in msg, (st, msg)
        got, _, st = dev_call(L, h, name, x, x, ya, yv, 1, None, n_weights=m, check=False)
        assert st == _lib.ERR_INVALID_ARG and "weights" in LAST["msg"], LAST["msg"]
        assert np.all(got == SENTINEL), "a refused call wrote its output"
    # the reference's panics: same texts as ndfft_exec_device
    def texts(name, n, sin, sout, axis, rdt=np.float64):
        h = getattr(handlers, ps.OPS[name][2])(n, rdt, _library=L)
        x = np.zeros(sin, cdt_of(rdt) if ps.OPS[name][3] else rdt); y = np.zeros(sout, cdt_of(rdt) if ps.OPS[name][4] else rdt)
        w = np.ones(max(x.shape[axis] if axis < x.ndim else 1, 1), wdtype(name, rdt))
        out = []
        for weighted in (False, True):
            _, _, st = dev_call(L, h, name, x, x, y, y, axis, w, weighted=weighted, check=False)
            out.append((st, LAST["msg"]))
        assert out[0] == out[1] and out[0][0] != _lib.OK, out
        return out[0]
    assert texts("ndifft", 6, (3, 5), (3, 5), 1) == (_lib.ERR_SIZE_MISMATCH, "Size mismatch in fft, got 5 expected 6")
    assert texts("nddct1", 4, (3, 5), (3, 5), 1) == (_lib.ERR_SIZE_MISMATCH, "Size mismatch in dct, got 5 expected 4")
    assert texts("ndifft_r2c", 6, (2, 6), (2, 6), 1) == (_lib.ERR_SIZE_MISMATCH, "Size mismatch in fft, got 6 expected 4")
    assert texts("ndifft", 5, (3, 5), (3, 5), 2)[0] == _lib.ERR_AXIS
    assert texts("ndifft", 5, (3, 5), (4, 5), 1)[0] == _lib.ERR_SHAPE_MISMATCH
    assert texts("nddct2", 5, (3, 5), (4, 5), 1)[0] == _lib.ERR_SHAPE_MISMATCH
