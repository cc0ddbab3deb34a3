"""Device allocations seen from the host: ndfft_dev_alloc / upload / download through ctypes, host images of an allocation with a view into it, and the
mask of the elements of an allocation that lie outside a view.  Only the C ABI is used, so the same helpers serve the CPU build of the kernel sources
(tests/emul) and the gfx950 library on the MI355X.  Shared by tests/weights_suite.py (the weighted entry point) and parity_suite.guarded_views."""
import ctypes

import numpy as np

from helpers import cdt_of
from ndrustfft_amd import _lib, api

OPC = {"ndfft": _lib.OP_C2C_FWD, "ndifft": _lib.OP_C2C_INV, "ndfft_r2c": _lib.OP_R2C, "ndifft_r2c": _lib.OP_C2R, "nddct1": _lib.OP_DCT1,
       "nddct2": _lib.OP_DCT2, "nddct3": _lib.OP_DCT3, "nddct4": _lib.OP_DCT4}
SENTINEL = 7.25


def _off(v, a):
    return v.__array_interface__["data"][0] - a.__array_interface__["data"][0]


class DevBuf:
    """A device allocation holding the bytes of a host array."""
    def __init__(self, L, host):
        self.L, self.nbytes = L, host.nbytes
        self.p = ctypes.c_void_p()
        L.check(L.c.ndfft_dev_alloc(ctypes.byref(self.p), max(host.nbytes, 16)))
        self.upload(host)

    def upload(self, host):
        host = np.ascontiguousarray(host)
        assert host.nbytes == self.nbytes
        if host.nbytes:
            self.L.check(self.L.c.ndfft_dev_upload(self.p, ctypes.c_void_p(host.ctypes.data), host.nbytes))

    def download(self, like):
        got = np.empty_like(like, order="C")
        if got.nbytes:
            self.L.check(self.L.c.ndfft_dev_download(ctypes.c_void_p(got.ctypes.data), self.p, got.nbytes))
        return got

    def free(self):
        self.L.check(self.L.c.ndfft_dev_free(self.p))


LAST = {"msg": ""}     # message of the last dev_call's exec


def strides_of(v):
    return [s // v.itemsize for s in v.strides]


def dev_call(L, h, name, xa, xv, ya, yv, axis, w=None, *, weighted=True, norm=_lib.NORM_NONE, scale=0.0, n_weights=None, w_offset=0, check=True):
    """One call on device images of the allocations xa / ya (C-contiguous host arrays), the views xv / yv into them giving the geometry.  weighted:
    ndfft_exec_weighted_device with weights w (None: NULL; w_offset: the vector starts that many elements into its allocation), else ndfft_exec_device
    with (`norm`, `scale`).  Returns (image of the output allocation after the call, last path, status)."""
    din, dout = DevBuf(L, xa), DevBuf(L, ya)
    dw = None
    try:
        args = (h._plan, OPC[name], ctypes.c_void_p(din.p.value + _off(xv, xa)), ctypes.c_void_p(dout.p.value + _off(yv, ya)), xv.ndim,
                api._i64(xv.shape), api._i64(strides_of(xv)), api._i64(yv.shape), api._i64(strides_of(yv)), axis)
        if weighted:
            wp = None
            if w is not None:
                w = np.ascontiguousarray(w)
                dw = DevBuf(L, np.concatenate([np.zeros(w_offset, w.dtype), w]))
                wp = ctypes.c_void_p(dw.p.value + w_offset * w.itemsize)
            st = L.c.ndfft_exec_weighted_device(*args, wp, (len(w) if w is not None else 0) if n_weights is None else n_weights, None)
        else:
            st = L.c.ndfft_exec_device(*args, norm, scale, None)
        LAST["msg"] = L.c.ndfft_last_error().decode()      # (the calls below clear it)
        if check:
            L.check(st)
        path = L.last_path() if st == _lib.OK else None
        L.check(L.c.ndfft_dev_sync(None))
        return dout.download(ya), path, st
    finally:
        din.free(); dout.free()
        if dw is not None:
            dw.free()


def out_alloc(name, shape, axis, rdt, out_view=None, layout="C"):
    """(ya, yv): the output allocation, pre-filled with the sentinel, and the output view in it."""
    import parity_suite as ps       # (parity_suite imports this module)
    _, sout = ps.shapes_for(name, shape, axis)
    odt = cdt_of(rdt) if ps.OPS[name][4] else np.dtype(rdt)
    if out_view is None:
        if layout == "F":
            ya = np.full(sout[::-1], SENTINEL, odt)
            return ya, ya.T
        ya = np.full(sout, SENTINEL, odt)
        return ya, ya
    ya = np.full(out_view[0], SENTINEL, odt)
    yv = ya[out_view[1]]
    assert yv.shape == tuple(sout), (yv.shape, sout)
    return ya, yv


def in_alloc(x, layout="C"):
    if layout == "F":
        xa = np.ascontiguousarray(x.T)
        return xa, xa.T
    xa = np.ascontiguousarray(x)
    return xa, xa


def view_index(ya, yv):
    """For every element of the view yv, its flat (C-order) element index in the allocation ya: an int64 array of yv's shape.  Strides of any sign,
    stride 0 included (the indices then repeat)."""
    off = _off(yv, ya)
    assert off % ya.itemsize == 0 and all(st % ya.itemsize == 0 for st in yv.strides)
    idx = np.full((1,) * yv.ndim, off // ya.itemsize, np.int64)
    for d, (n, st) in enumerate(zip(yv.shape, strides_of(yv))):
        idx = idx + (np.arange(n, dtype=np.int64) * st).reshape([n if e == d else 1 for e in range(yv.ndim)])
    idx = np.broadcast_to(idx, yv.shape)
    assert yv.size == 0 or (0 <= idx.min() and idx.max() < ya.size), "the view leaves its allocation"
    return idx


def view_mask(ya, yv):
    """True where an element of the allocation ya lies OUTSIDE the view yv (strides of any sign)."""
    mark = np.zeros(ya.size, bool)
    mark[view_index(ya, yv).reshape(-1)] = True
    return ~mark.reshape(ya.shape)
