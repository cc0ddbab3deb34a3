"""Cases of ndfft_filter on REAL device arrays under an R2cFftHandler: the fused route filter_r2c_pow2 (filter_kernel.h: REAL; compose.hip: filter_fused) and the calls
that must stay on the composed route.  Built on tests/filter_suite.py's helpers -- filter_case(..., r2c=True) checks every call against the composed CPU oracle
within helpers.TOL, every element of the output allocation outside the view, and the input allocation -- so that the same functions run on the CPU build of the
kernel sources (tests/test_filter_real_emul.py) and on the MI355X (tests/test_filter_real_gpu.py)."""
import numpy as np
import scipy.fft as sf

import accuracy as acc
from devmem import SENTINEL, out_alloc
from filter_suite import BOTH, NO_FUSE, filt_call, filter_case, handler, make_x, oracle_filter, truth_filter, within_bar  # noqa: F401  (oracle / truth: the bar's)
from helpers import TOL, assert_close, cdt_of
from ndrustfft_amd import _lib
from weights_suite import make_weights

FUSED_R = "filter_r2c_pow2"
FUSED_R_N = (128, 256, 512, 1024, 2048, 4096, 8192)          # kernels_filter.hip: NDFFT_FILTER_LENGTHS, as n = 2 F
# (n = 2 F, the kernel is the complex one of length F: the radix lists of F = 128, 1024, 2048 in f64 and F = 2048 in f32 are no palindromes, so n = 256, 2048, 4096
#  in f64 and n = 4096 in f32 run their second pass set on a second twiddle table -- weight_placement's lengths hold all four)


def composed(path):
    return "+weights+" in path and FUSED_R not in path


# ---- 1. every instance ---------------------------------------------------------------------------------------------------------------------------------
def every_instance(L, n, rdt):
    """37 lanes leave a partial last workgroup for every LPB > 1."""
    filter_case(L, (37, n), 1, rdt, r2c=True, want_path=FUSED_R, seed=n)


# ---- 2. working precision: the bar of docs/accuracy.md, fused and composed under the same bar -----------------------------------------------------------------
def working_precision(L, n, rdt, verbose=False):
    paths = within_bar(L, (37, n), 1, rdt, r2c=True, flag_sets=(0, NO_FUSE), verbose=verbose, want=FUSED_R)
    assert paths[0] == FUSED_R and composed(paths[NO_FUSE]), paths


# ---- 3. DC and Nyquist ------------------------------------------------------------------------------------------------------------------------------------
def dc_and_nyquist(L, cases=((np.float64, 128), (np.float64, 2048), (np.float32, 256), (np.float32, 8192))):
    for rdt, n in cases:
        shape = (5, n)
        x = make_x(shape, rdt, r2c=True, seed=n)
        w = make_weights("ndifft_r2c", n, rdt, seed=n)
        assert w[0].imag != 0 and w[-1].imag != 0
        a, _ = filter_case(L, shape, 1, rdt, r2c=True, x=x, w=w, want_path=FUSED_R)
        # Im(DC) and Im(Nyquist) of the product are dropped: with real input both products' real parts do not depend on Im(w) there
        w2 = w.copy(); w2[0] = complex(w[0].real, -3 * w[0].imag + 1); w2[-1] = complex(w[-1].real, 0.25 - w[-1].imag)
        b, _ = filter_case(L, shape, 1, rdt, r2c=True, x=x, w=w2, want_path=FUSED_R)
        assert a.tobytes() == b.tobytes(), f"real filter n={n} {np.dtype(rdt).name}: the result depends on Im(w[0]) / Im(w[n/2])"
        for norm, s in ((_lib.NORM_NONE, 1.0), (_lib.NORM_DEFAULT, 1.0 / n)):
            c, _ = filter_case(L, shape, 1, rdt, r2c=True, x=x, wkind="ones", norm=norm, want_path=FUSED_R)
            assert_close(c, s * n * x.astype(np.float64), 1, TOL[np.dtype(rdt)], f"real filter w = 1 n={n} norm={norm}")


# ---- 4. the weights' placement ---------------------------------------------------------------------------------------------------------------------------
def weight_placement(L, cases=((np.float64, 256), (np.float64, 2048), (np.float64, 4096), (np.float32, 512), (np.float32, 4096))):
    """w = e_k moves exactly bin k: (c_k / n) Re(X[k] e^{2 pi i k j / n}), c_k = 2 for 0 < k < n / 2 (the bin and its mirror), 1 for DC and Nyquist.
    k = n / 4 is the bin that pairs with itself in the kernel's mirror exchange, 37 is odd and a multiple of no radix."""
    for rdt, n in cases:
        cdt = cdt_of(rdt)
        x = make_x((5, n), rdt, r2c=True, seed=n + 1)
        X = sf.rfft(x.astype(np.float64), axis=1)
        j = np.arange(n)
        h = handler(L, n, rdt, True)
        for k in (0, 1, 37, n // 4, n // 2 - 1, n // 2):
            w = np.zeros(n // 2 + 1, cdt); w[k] = 1
            ya, yv = out_alloc("nddct2", (5, n), 1, rdt)
            got, _, path, _ = filt_call(L, h, x, x, ya, yv, 1, w)
            assert path == FUSED_R, path
            ck = 2.0 if 0 < k < n // 2 else 1.0
            want = (ck / n) * (X[:, k:k + 1] * np.exp(2j * np.pi * k * j / n)[None, :]).real
            assert_close(got, want, 1, TOL[np.dtype(rdt)], f"real filter w = e_{k}, n = {n} {np.dtype(rdt).name}")


# ---- 5. alignment and pitch (offsets and pitches in REALS) ---------------------------------------------------------------------------------------------------
def _pitched(rows, n, pitch, base, dt, fill, x=None):
    a = np.full(base + rows * pitch + 3, fill, dt)
    v = np.lib.stride_tricks.as_strided(a[base:], (rows, n), (pitch * a.itemsize, a.itemsize))
    if x is not None:
        v[...] = x
    return a, v


def alignment_and_pitch(L, shapes=((37, 1024), (5, 8192))):
    """A lane base that is a whole complex element (even base offset, even pitch) is fused; one that is not is composed; every result is right (filter_case)."""
    for rdt in BOTH:
        for rows, n in shapes:
            x = make_x((rows, n), rdt, r2c=True, seed=n + 3)
            #                 base in/out, pitch in/out, fused
            for bi, bo, pi, po, fused in ((0, 0, n + 2, n + 6, True), (0, 0, n + 4, n + 8, True), (0, 0, n, n + 2, True),     # padded even pitches that differ (f32: n + 2 is no 16-byte pitch)
                                          (2, 2, n, n, True), (2, 0, n + 4, n, True), (0, 2, n, n + 4, True),                   # f32: a base 8 bytes into the allocation, the VEC = 1 instance
                                          (0, 0, n + 1, n, False), (0, 0, n, n + 3, False),                                      # an odd pitch on either side
                                          (1, 0, n, n, False), (0, 1, n + 2, n + 2, False), (3, 1, n, n, False)):                # an odd base offset on either side
                xa, xv = _pitched(rows, n, pi, bi, rdt, 0, x)
                ya, yv = _pitched(rows, n, po, bo, rdt, SENTINEL)
                _, path = filter_case(L, (rows, n), 1, rdt, r2c=True, xa=xa, xv=xv, ya=ya, yv=yv, seed=n)
                assert (path == FUSED_R) if fused else composed(path), (path, (bi, bo, pi, po), n, np.dtype(rdt).name)


# ---- 6. sentinel bands ------------------------------------------------------------------------------------------------------------------------------------
def sentinel_bands(L, shapes=((37, 128), (5, 1024), (3, 8192))):
    """The output is a window of a larger sentinel-filled allocation at even offsets (filter_case: nothing outside it changes, the input allocation is bit-identical)."""
    for rdt in BOTH:
        for rows, n in shapes:
            for flags in (0, NO_FUSE):
                _, path = filter_case(L, (rows, n), 1, rdt, r2c=True, out_view=((rows + 2, n + 6), np.s_[1:rows + 1, 4:4 + n]), flags=flags, want_path=None if flags else FUSED_R)
                assert flags == 0 or composed(path), path


# ---- 7. in place --------------------------------------------------------------------------------------------------------------------------------------------
def in_place(L, shapes=((37, 256), (5, 8192))):
    for rdt in BOTH:
        for shape in shapes:
            x = make_x(shape, rdt, r2c=True, seed=shape[1])
            a, _ = filter_case(L, shape, 1, rdt, r2c=True, x=x, want_path=FUSED_R)
            b, _ = filter_case(L, shape, 1, rdt, r2c=True, x=x.copy(), inplace=True, want_path=FUSED_R)
            assert a.tobytes() == b.tobytes(), f"in place differs from out of place: {shape} {np.dtype(rdt).name}"


# ---- 8. the XCD map with a ragged last group ------------------------------------------------------------------------------------------------------------------
def xcd_tail(L, shapes=((131, 8192), (8197, 128))):
    """Both are past nblk >= 16 chunk (8 blocks of one 64 KiB lane; 16 blocks of 32 lanes of 1 KiB) with blocks left over after the last whole group."""
    for shape in shapes:
        filter_case(L, shape, 1, np.float64, r2c=True, want_path=FUSED_R, seed=7)


# ---- 9. lane isolation (the three-copy scheme of parity_suite.lane_isolation) -----------------------------------------------------------------------------------
def lane_isolation(L, shapes=((37, 128), (37, 1024), (9, 4096))):
    bad = []
    for rdt in BOTH:
        for shape in shapes:
            n = shape[1]
            keep = acc.kept_lanes(shape[0])
            km = keep[:, None]
            x = acc.make_input("uniform", "ndfft_r2c", shape, 1, rdt, offset=n)
            big = np.dtype(rdt).type(1e30 if np.dtype(rdt) == np.float32 else 1e250)
            xs = (x, (x * np.where(km, np.dtype(rdt).type(1), big)).astype(x.dtype), np.where(km, x, np.nan).astype(x.dtype))
            w = make_weights("ndifft_r2c", n, rdt, seed=3)
            h = handler(L, n, rdt, True)
            outs = []
            for xi in xs:
                ya, yv = out_alloc("nddct2", shape, 1, rdt)
                got, _, path, _ = filt_call(L, h, xi, xi, ya, yv, 1, w)
                assert path == FUSED_R, path
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
        x = make_x(shape, rdt, r2c=True, seed=n)
        outs = {}
        for norm in (_lib.NORM_NONE, _lib.NORM_DEFAULT, _lib.NORM_SCALE):
            outs[norm], _ = filter_case(L, shape, 1, rdt, r2c=True, x=x, norm=norm, scale=0.37, want_path=FUSED_R)
        # each is one rounded multiply of the same value by the working-precision scalar: 2 eps covers both roundings (filter_suite.normalisation)
        T = np.dtype(rdt).type
        eps = acc.LD(np.finfo(rdt).eps)
        for hi, lo, f, what in ((_lib.NORM_SCALE, _lib.NORM_DEFAULT, acc.LD(T(0.37)) / acc.LD(T(1.0) / T(n)), "SCALE is no pure factor of DEFAULT"),
                                (_lib.NORM_DEFAULT, _lib.NORM_NONE, acc.LD(T(1.0) / T(n)), "DEFAULT is no pure factor of NONE")):
            a = outs[hi].astype(acc.LD); b = outs[lo].astype(acc.LD) * f
            assert np.all(np.abs(a - b) <= 2 * eps * np.abs(a)), f"{what}: {shape} {np.dtype(rdt).name}"


# ---- 11. layouts and the lengths that stay composed ---------------------------------------------------------------------------------------------------------
def layouts(L):
    for rdt in BOTH:
        filter_case(L, (256, 6), 0, rdt, r2c=True, layout="F", want_path=FUSED_R)                  # unit-stride lanes of 256 points at pitch 256
        _, path = filter_case(L, (256, 6), 0, rdt, r2c=True, layout="C")                            # strided lanes
        assert composed(path), path
        x = make_x((6, 256), rdt, r2c=True, seed=256)
        xa = np.ascontiguousarray(x[:, ::-1])
        _, path = filter_case(L, (6, 256), 1, rdt, r2c=True, xa=xa, xv=xa[:, ::-1])              # reversed stride along the axis
        assert composed(path), path
        _, path = filter_case(L, (37, 256), 1, rdt, r2c=True, flags=NO_FUSE)
        assert composed(path), path
        for shape in ((37, 64), (3, 16384)):
            assert shape[1] not in FUSED_R_N
            _, path = filter_case(L, shape, 1, rdt, r2c=True, seed=shape[1])
            assert composed(path), (path, shape)
