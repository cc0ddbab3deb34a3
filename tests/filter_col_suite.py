"""Cases of ndfft_filter along a STRIDED axis of a C-layout array: the column form of the fused kernel (filter_kernel.h: FilterColKernel, path filter_col_pow2),
one workgroup per tile of adjacent lanes.  Built on filter_suite (filter_case, within_bar, filt_call, make_x) as it is: expected values from the composed CPU
oracle within helpers.TOL, working precision by the bar of docs/accuracy.md.  The functions take the library L, so the same cases run on the CPU build of the
kernel sources (tests/test_filter_col_emul.py) and on the MI355X (tests/test_filter_col_gpu.py)."""
import numpy as np
import scipy.fft as sf

import accuracy as acc
import filter_instances_suite as fis
import filter_suite as fs
from devmem import SENTINEL, _off, out_alloc
from filter_suite import NO_FUSE, filt_call, filter_case, make_x, within_bar
from helpers import TOL, assert_close, cdt_of
from ndrustfft_amd import _lib
from weights_suite import make_weights

BOTH = fs.BOTH
FUSED_COL = "filter_col_pow2"
# mirrors NDFFT_FILTER_COL_LENGTHS_F64 / _F32 of kernels_filter.hip
FUSED_COL_N = {np.float64: (128, 256, 512, 1024, 2048), np.float32: (128, 256, 512, 1024, 2048)}
INSTANCES = [(n, rdt) for rdt in BOTH for n in FUSED_COL_N[rdt]]
INSTANCE_IDS = [f"{np.dtype(rdt).name}-{n}" for n, rdt in INSTANCES]
INNER = 37      # lanes: a ragged last tile for every power-of-two tile width


# ---- 1. every instance ------------------------------------------------------------------------------------------------------------------------------
def every_instance(L, n, rdt):
    filter_case(L, (n, INNER), 0, rdt, want_path=FUSED_COL, seed=n)


# ---- 2. two batch dims: tiles meet an o boundary, or a tile is wider than inner ----------------------------------------------------------------------
def two_batch_dims(L):
    for rdt in BOTH:
        for shape in ((3, 256, 21), (2, 1024, 9)):
            filter_case(L, shape, 1, rdt, want_path=FUSED_COL, seed=shape[1] + 1)


# ---- 3. where memory is touched ----------------------------------------------------------------------------------------------------------------------
def guarded_windows(L):
    """The output is a window of a sentinel allocation, the input a window of a padded allocation at an odd element offset (filter_case checks every element outside
    the output view, and the input's bytes).  Element 47 is where both windows start: for c64 that is 8 bytes off 16-byte alignment already; the dense pair
    behind it has unit lane stride, pitch 37 and both bases one element (8 bytes) into their allocations."""
    for rdt in BOTH:
        cdt = cdt_of(rdt)
        for n in (128, 512):
            x = make_x((n, INNER), rdt, seed=n + 2)
            xa = np.zeros((n + 2, 45), cdt)
            xv = xa[1:n + 1, 2:2 + INNER]
            xv[...] = x
            assert (_off(xv, xa) // xa.itemsize) % 2 == 1
            filter_case(L, (n, INNER), 0, rdt, xa=xa, xv=xv, out_view=((n + 2, 43), np.s_[1:n + 1, 4:4 + INNER]), want_path=FUSED_COL, seed=n)
            filter_case(L, (n, INNER), 0, rdt, xa=xa, xv=xv, out_view=((n + 2, 43), np.s_[1:n + 1, 4:4 + INNER]), flags=NO_FUSE, seed=n)
            if np.dtype(rdt) == np.float32:
                flat = lambda fill: np.full(1 + n * INNER + 3, fill, cdt)
                view = lambda a: np.lib.stride_tricks.as_strided(a[1:], (n, INNER), (INNER * a.itemsize, a.itemsize))
                xa1 = flat(0); xv1 = view(xa1); xv1[...] = x
                ya1 = flat(SENTINEL)
                filter_case(L, (n, INNER), 0, rdt, xa=xa1, xv=xv1, ya=ya1, yv=view(ya1), want_path=FUSED_COL, seed=n)


# ---- 4. in place equals out of place, bit for bit -------------------------------------------------------------------------------------------------------
def in_place(L):
    for rdt in BOTH:
        for shape, axis in (((256, INNER), 0), ((3, 128, 21), 1)):
            x = make_x(shape, rdt, seed=shape[axis])
            a, p0 = filter_case(L, shape, axis, rdt, x=x, want_path=FUSED_COL)
            b, p1 = filter_case(L, shape, axis, rdt, x=x.copy(), inplace=True, want_path=FUSED_COL)
            assert a.tobytes() == b.tobytes(), f"in place differs from out of place: {shape} axis={axis} {np.dtype(rdt).name}"


# ---- 5. weight placement ----------------------------------------------------------------------------------------------------------------------------------
def weight_placement(L, cases=((np.float64, 128), (np.float64, 1024), (np.float32, 2048), (np.float64, 256))):
    """(the first three have reversed radix lists with a twiddle table of their own, f64 256 is a palindrome)"""
    for rdt, n in cases:
        cdt = cdt_of(rdt)
        shape = (n, 9)
        x = make_x(shape, rdt, seed=n + 1)
        X = sf.fft(x.astype(np.complex128), axis=0)
        j = np.arange(n)
        h = fs.handler(L, n, rdt)
        for k in (0, 1, n // 2, n - 1, 37):
            w = np.zeros(n, cdt); w[k] = 1
            ya, yv = out_alloc("ndfft", shape, 0, rdt)
            got, _, path, _ = filt_call(L, h, x, x, ya, yv, 0, w)
            assert path == FUSED_COL, path
            want = X[k:k + 1, :] * np.exp(2j * np.pi * k * j / n)[:, None] / n
            assert_close(got, want, 0, TOL[np.dtype(rdt)], f"w = e_{k}, n = {n} {np.dtype(rdt).name} axis 0")
        for norm, s in ((_lib.NORM_NONE, 1.0), (_lib.NORM_DEFAULT, 1.0 / n)):
            ya, yv = out_alloc("ndfft", shape, 0, rdt)
            got, _, path, _ = filt_call(L, h, x, x, ya, yv, 0, np.ones(n, cdt), norm=norm)
            assert path == FUSED_COL, path
            assert_close(got, s * n * x.astype(np.complex128), 0, TOL[np.dtype(rdt)], f"w = 1, n = {n} {np.dtype(rdt).name} norm={norm} axis 0")


# ---- 6. against composed, within the bar; the same lanes through the row kernel ------------------------------------------------------------------------------
def against_composed(L, n, rdt, verbose=False):
    shape = (n, INNER)
    paths = within_bar(L, shape, 0, rdt, flag_sets=(0, NO_FUSE), verbose=verbose, want=FUSED_COL)
    assert paths[0] == FUSED_COL and "+weights+" in paths[NO_FUSE] and FUSED_COL not in paths[NO_FUSE] and fs.FUSED not in paths[NO_FUSE], paths
    x = make_x(shape, rdt, seed=n + 3)
    a, _ = filter_case(L, shape, 0, rdt, x=x, want_path=FUSED_COL, seed=n)
    b, _ = filter_case(L, shape, 0, rdt, x=x, layout="F", want_path=fs.FUSED, seed=n)
    # an observation, not a requirement: the column and the row kernel are separate compilations
    print(f"filter_col_pow2 against filter_pow2 on the same lanes, n = {n} {np.dtype(rdt).name}: "
          f"{'bit-identical' if a.tobytes() == b.tobytes() else 'not bit-identical'}", flush=True)


# ---- 7. lane isolation inside a tile (filter_suite.lane_isolation, transposed) --------------------------------------------------------------------------------
def lane_isolation(L, lengths=(128, 512, 2048)):
    bad = []
    for rdt in BOTH:
        for n in lengths:
            shape = (n, INNER)
            keep = acc.kept_lanes(INNER)
            km = keep[None, :]
            x = acc.make_input("uniform", "ndfft", shape, 0, rdt, offset=n)
            big = np.dtype(rdt).type(1e30 if np.dtype(rdt) == np.float32 else 1e250)
            xs = (x, (x * np.where(km, np.dtype(rdt).type(1), big)).astype(x.dtype), np.where(km, x, complex(np.nan, np.nan)).astype(x.dtype))
            w = make_weights("ndifft", n, rdt, seed=3)
            h = fs.handler(L, n, rdt)
            outs = []
            for xi in xs:
                ya, yv = out_alloc("ndfft", shape, 0, rdt)
                got, _, path, _ = filt_call(L, h, xi, xi, ya, yv, 0, w)
                assert path == FUSED_COL, path
                outs.append(np.ascontiguousarray(got[:, keep]))
            what = f"{shape} axis 0 {np.dtype(rdt).name}"
            if not np.isfinite(outs[0]).all():
                bad.append("non-finite output of a finite lane: " + what)
            for k, label in ((1, "scaled"), (2, "NaN")):
                if outs[0].tobytes() != outs[k].tobytes():
                    bad.append(f"kept lanes differ with {label} neighbours: " + what)
    assert not bad, "\n".join(bad)


# ---- 8. many tiles with a tail: the XCD map ----------------------------------------------------------------------------------------------------------------
def xcd_tail(L, shape=(128, 4101)):
    """f64 n = 128 has tiles of 32 lanes: 129 tiles, past the 64 from which the launch maps runs of 4 tiles per XCD (groups of 32), one tile past the last whole
    group, and that one ragged (5 lanes)."""
    filter_case(L, shape, 0, np.float64, want_path=FUSED_COL, seed=7)


# ---- 9. normalisation (filter_suite.normalisation on a column shape) --------------------------------------------------------------------------------------------
def normalisation(L, shape=(512, INNER)):
    for rdt in BOTH:
        n = shape[0]
        x = make_x(shape, rdt, seed=n)
        outs = {}
        for norm in (_lib.NORM_NONE, _lib.NORM_DEFAULT, _lib.NORM_SCALE):
            outs[norm], _ = filter_case(L, shape, 0, rdt, x=x, norm=norm, scale=0.37, want_path=FUSED_COL)
        T = np.dtype(rdt).type
        eps = acc.LD(np.finfo(rdt).eps)
        for hi, lo, f, label in ((_lib.NORM_SCALE, _lib.NORM_DEFAULT, acc.LD(T(0.37)) / acc.LD(T(1.0) / T(n)), "SCALE is no pure factor of DEFAULT"),
                                 (_lib.NORM_DEFAULT, _lib.NORM_NONE, acc.LD(T(1.0) / T(n)), "DEFAULT is no pure factor of NONE")):
            for part in ("real", "imag"):
                a = getattr(outs[hi], part).astype(acc.LD); b = getattr(outs[lo], part).astype(acc.LD) * f
                assert np.all(np.abs(a - b) <= 2 * eps * np.abs(a)), f"{label}: {shape} axis 0 {np.dtype(rdt).name} {part}"


# ---- 10. both load policies ----------------------------------------------------------------------------------------------------------------------------------
def both_policies(L, n, rdt):
    """A dense C-layout block honours the input hint; ndfft_last_input_policy() names the instance (NT = 1 / NT = 3)."""
    fis.settle_residency_model(L)
    for value in (fis.AUTO, fis.COLD):
        with fis.hint(L, value):
            filter_case(L, (n, INNER), 0, rdt, want_path=FUSED_COL, seed=n + 4)
            fis.policy_is(L, value, f"filter_col_pow2 n={n} {np.dtype(rdt).name}")


# ---- 11. declined, still correct ----------------------------------------------------------------------------------------------------------------------------
def declined(L):
    for rdt in BOTH:
        cdt = cdt_of(rdt)
        for shape in ((256, 6), (64, 40), (8192, 9), (4096, 9)):      # too few lanes, too short, two lengths without a column instance
            filter_case(L, shape, 0, rdt, want_in_path="+weights+", seed=shape[0])
        # reversed stride along the inner dim
        x = make_x((256, 12), rdt, seed=5)
        xa = np.ascontiguousarray(x[:, ::-1])
        filter_case(L, (256, 12), 0, rdt, xa=xa, xv=xa[:, ::-1], want_in_path="+weights+")
        # a column-layout input with a row-layout output
        x = make_x((256, INNER), rdt, seed=6)
        ya = np.full((INNER, 256), SENTINEL, cdt)
        filter_case(L, (256, INNER), 0, rdt, xa=x, xv=x, ya=ya, yv=ya.T, want_in_path="+weights+")
        # three batch dims that do not merge, the axis not last
        big, win = (3, 4, 128, 11), np.s_[0:2, 0:3, :, 1:10]
        xa = np.zeros(big, cdt)
        xv = xa[win]
        xv[...] = make_x((2, 3, 128, 9), rdt, seed=8)
        filter_case(L, (2, 3, 128, 9), 2, rdt, xa=xa, xv=xv, out_view=(big, win), want_in_path="+weights+")
        filter_case(L, (256, INNER), 0, rdt, flags=NO_FUSE, want_in_path="+weights+")
        filter_case(L, (256, INNER), 0, rdt, layout="F", want_path=fs.FUSED)
