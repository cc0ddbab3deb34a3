"""Truth and error metrics at WORKING PRECISION (docs/accuracy.md): what helpers.TOL (1e-10 / 1e-4, about 450 000 / 840 machine
epsilons) cannot see.  No GPU needed.

truth(name, x, n, axis)   the exact answer of op `name` under Default normalisation for the input AS STORED: f32 inputs in float64,
                          f64 inputs in np.longdouble, both through scipy.fft (which computes in the precision it is handed).
errors(got, ref, axis, rdt)   (e_l2, e_bin) in units of eps = np.finfo(rdt).eps, computed in long double:
                          e_l2  = max over lanes of ||got - truth||_2 / ||truth||_2
                          e_bin = max over elements of |got - truth| / rms(truth lane)
inputs: U[-1,1) (synth), one unit impulse per lane at (7 lane + 1) mod len, U[-1,1) x 10^(-6 j / len) along the lane."""
import numpy as np
import scipy.fft as sf

import synth
from helpers import cdt_of

LD = np.longdouble
CLD = np.clongdouble
INPUTS = ("uniform", "impulse", "graded")
DCT_TYPE = {"nddct1": 1, "nddct2": 2, "nddct3": 3, "nddct4": 4}
COMPLEX_IN = {"ndfft": True, "ndifft": True, "ndfft_r2c": False, "ndifft_r2c": True,
              "nddct1": False, "nddct2": False, "nddct3": False, "nddct4": False}


def require_long_double():
    """f64 truths need an 80-bit (or wider) long double; where numpy has none the f64 cases FAIL with this message, they do not skip."""
    eps = np.finfo(LD).eps
    assert eps <= 2.0 ** -63, f"f64 accuracy cases need np.finfo(np.longdouble).eps <= 2**-63; this platform has {float(eps):.3e}"


def truth(name, x, n, axis):
    """Op `name` of the array x (lane length n of the REAL side on `axis`), Default normalisation (src/lib.rs: ndifft 1/n, ndifft_r2c 1/n,
    DCT-I..IV = scipy's unnormalised forms), one precision above the input's."""
    x = np.asarray(x)
    if x.real.dtype == np.float64:
        require_long_double()
        w = x.astype(CLD if np.iscomplexobj(x) else LD)
    else:
        w = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    if name == "ndfft":
        return sf.fft(w, axis=axis)
    if name == "ndifft":
        return sf.ifft(w, axis=axis)
    if name == "ndfft_r2c":
        return sf.rfft(w, axis=axis)
    if name == "ndifft_r2c":                       # C2R drops Im(DC) and, n even, Im(Nyquist) first (src/lib.rs:516-521)
        w = np.moveaxis(w.copy(), axis, -1)
        w[..., 0] = w[..., 0].real
        if n % 2 == 0:
            w[..., -1] = w[..., -1].real
        return sf.irfft(np.moveaxis(w, -1, axis), n=n, axis=axis)
    return sf.dct(w, type=DCT_TYPE[name], axis=axis)


def _ld_parts(a):
    a = np.asarray(a)
    return (a.real.astype(LD), a.imag.astype(LD)) if np.iscomplexobj(a) else (a.astype(LD), None)


def prepare(ref, axis):
    """The truth's side of errors(), computed once per truth: long-double parts, sum of squares per lane, lane length."""
    rr, ri = _ld_parts(ref)
    r2 = rr * rr
    if ri is not None:
        r2 += ri * ri
    den2 = r2.sum(axis=axis, keepdims=True)
    return rr, ri, np.where(den2 > 0, den2, LD(1)), np.asarray(ref).shape[axis]


def errors(got, ref, axis, rdt):
    """(e_l2, e_bin) of `got` against `ref` (an array, or prepare(array, axis)) in units of eps(rdt), in long double; nan when got holds a
    non-finite value.  (Real and imaginary parts apart and squares throughout: complex long-double abs is several times slower.)"""
    eps = LD(np.finfo(rdt).eps)
    rr, ri, den2, n = ref if isinstance(ref, tuple) else prepare(ref, axis)
    gr, gi = _ld_parts(got)
    d2 = (gr - rr) ** 2
    if gi is not None or ri is not None:
        di = (gi if gi is not None else 0) - (ri if ri is not None else 0)
        d2 += di * di
    num2 = d2.sum(axis=axis, keepdims=True)
    e_l2 = np.sqrt((num2 / den2).max()) / eps
    e_bin = np.sqrt((d2 / (den2 / LD(n))).max()) / eps
    return float(e_l2), float(e_bin)


def make_input(kind, name, shape, axis, rdt, offset=0):
    """Input array of op `name` (`shape` = the input's shape, lane on `axis`) of one of INPUTS."""
    cplx = COMPLEX_IN[name]
    dt = cdt_of(rdt) if cplx else np.dtype(rdt)
    n = shape[axis]
    if kind == "impulse":
        other = tuple(s for d, s in enumerate(shape) if d != axis)
        xl = np.zeros((int(np.prod(other)), n), dt)        # lanes in C order of the other dimensions
        lanes = np.arange(xl.shape[0])
        xl[lanes, (7 * lanes + 1) % n] = 1
        return np.ascontiguousarray(np.moveaxis(xl.reshape(other + (n,)), -1, axis))
    x = synth.complex_array(shape, dt, offset=offset) if cplx else synth.real_array(shape, rdt, offset=offset)
    if kind == "graded":
        g = 10.0 ** (-6.0 * np.arange(n) / n)
        x = (x * g.reshape([n if d == axis else 1 for d in range(len(shape))])).astype(dt)
    else:
        assert kind == "uniform", kind
    return x


def kept_lanes(nlanes):
    """Lane isolation: the lanes that keep their values ({0, middle, last, every 5th}); every other lane is scaled or poisoned."""
    keep = np.zeros(nlanes, bool)
    keep[::5] = True; keep[[0, nlanes // 2, nlanes - 1]] = True
    return keep
