"""The row kernel in its derived latency form (pow2_kernel.h FLAGS bits 5 + 6; pow2_config.h names the lengths): the cases shared by the CPU build of the
kernel sources (tests/test_pow2_latency_emul.py) and the MI355X (tests/test_gpu_pow2_latency.py).  Every call goes through ndfft_exec_device on device
images, asserts the route (pow2_reg) and, on dense arrays, the load policy (the plain-load and the streaming-load instance are two kernels with one
arithmetic), and is compared on every lane."""
import numpy as np

import accuracy as acc
import devmem
import filter_instances_suite as fis
import parity_suite as ps
from helpers import TOL, assert_close
from ndrustfft_amd import _lib

# (dtype, n) of pow2_config.h's pow2_row_flags(): the instances that run in this form
LENGTHS = ((np.float64, 4096), (np.float32, 4096))
AUTO, COLD = _lib.INPUT_AUTO, _lib.INPUT_COLD
ROUTE = "pow2_reg"
PAD = 24          # elements between the lanes of a pitched view


def numpy_ref(name, x, axis):
    return np.fft.fft(x, axis=axis) if name == "ndfft" else np.fft.ifft(x, axis=axis)


def oracle_ref(name, x, axis, rdt):
    n = x.shape[axis]
    yo = np.zeros_like(x); ps.OPS[name][1](np.ascontiguousarray(x), yo, ps.orc.FftHandler(n, rdt), axis)
    return yo


def call(L, h, name, x, hint, pitched=False, offset=0):
    """One call under `hint` on a dense array, on a dense array that starts `offset` elements into its allocation (one element: f32 lanes are then 8-byte aligned
    only, the instance with one element per access), or on a view whose row pitch exceeds n; returns the output view's values.  The sentinels around the view stay."""
    rows, n = x.shape
    if offset:
        xa = np.full(rows * n + 2 * offset, devmem.SENTINEL, x.dtype); xa[offset:offset + rows * n] = x.reshape(-1)
        ya = np.full(rows * n + 2 * offset, devmem.SENTINEL, x.dtype)
        xv, yv = xa[offset:offset + rows * n].reshape(rows, n), ya[offset:offset + rows * n].reshape(rows, n)
    elif pitched:
        xa = np.full((rows, n + PAD), devmem.SENTINEL, x.dtype); xa[:, :n] = x
        ya = np.full((rows, n + PAD), devmem.SENTINEL, x.dtype)
        xv, yv = xa[:, :n], ya[:, :n]
    else:
        xa = xv = np.ascontiguousarray(x)
        ya = yv = np.full(x.shape, devmem.SENTINEL, x.dtype)
    if pitched:      # the hint and the residency model serve dense arrays; on a view the launcher decides by size, or as NDFFT_STREAM_LOADS says
        with ps.switches(L, NDFFT_STREAM_LOADS="1" if hint == COLD else "0"):
            img, path, _ = devmem.dev_call(L, h, name, xa, xv, ya, yv, 1, weighted=False, norm=_lib.NORM_DEFAULT)
    else:
        with fis.hint(L, hint):
            img, path, _ = devmem.dev_call(L, h, name, xa, xv, ya, yv, 1, weighted=False, norm=_lib.NORM_DEFAULT)
            fis.policy_is(L, hint, f"{name} {x.shape}")
    assert path == ROUTE, f"{name} {x.shape} pitched={pitched} took {path}"
    if offset:
        assert (img[:offset] == devmem.SENTINEL).all() and (img[offset + rows * n:] == devmem.SENTINEL).all(), "the call wrote outside the output view"
        return np.ascontiguousarray(img[offset:offset + rows * n].reshape(rows, n))
    if pitched:
        assert (img[:, n:] == devmem.SENTINEL).all(), "the call wrote between the lanes of the output view"
        return np.ascontiguousarray(img[:, :n])
    return img


def both_policies(L, h, name, x, pitched=False, offset=0):
    """The output under INPUT_AUTO (plain loads) after checking that INPUT_COLD (streaming loads) gives the same bits."""
    fis.settle_residency_model(L)
    a = call(L, h, name, x, AUTO, pitched, offset)
    c = call(L, h, name, x, COLD, pitched, offset)
    assert a.tobytes() == c.tobytes(), f"{name} {x.shape}: the two load-policy instances differ"
    return a


def parity(L, rows, n, rdt, ref, names=("ndfft", "ndifft"), pitched=False, offset=0):
    """Every lane at helpers.TOL against ref(name, x, axis), under both hints."""
    for name in names:
        h, _ = ps.handlers_for(name, n, rdt, L)
        x = ps.make_input(name, (rows, n), rdt, offset=n + rows)
        got = both_policies(L, h, name, x, pitched, offset)
        assert_close(got, ref(name, x, 1), 1, TOL[np.dtype(rdt)], f"{name} ({rows}, {n}) pitched={pitched} offset={offset}")


def accuracy_bar(L, rows, n, rdt, verbose=True):
    """docs/accuracy.md: both metrics within ACC_FACTOR of the oracle's own error (this input's, or the uniform input's if larger), all three inputs."""
    bad = []
    for name in ("ndfft", "ndifft"):
        h, _ = ps.handlers_for(name, n, rdt, L)
        uni = None
        for kind in acc.INPUTS:
            x = acc.make_input(kind, name, (rows, n), 1, rdt, offset=n)
            t = acc.prepare(acc.truth(name, x, n, 1), 1)
            orac = acc.errors(oracle_ref(name, x, 1, rdt), t, 1, rdt)
            if kind == "uniform":
                uni = orac
            den = tuple(max(a, b) for a, b in zip(orac, uni))
            lib = acc.errors(both_policies(L, h, name, x), t, 1, rdt)
            line = f"{name} ({rows}, {n}) {kind}: e_l2 {lib[0]:.3f} eps (oracle {den[0]:.3f}), e_bin {lib[1]:.3f} eps (oracle {den[1]:.3f})"
            if verbose:
                print(line, flush=True)
            if not all(l <= ps.ACC_FACTOR * d for l, d in zip(lib, den)):       # (nan fails)
                bad.append("beyond the bar: " + line)
    assert not bad, "\n".join(bad)
