"""The sixteen nd* functions of ndrustfft (lib.rs:350-421, 543-611, 753-844) over the C ABI.

Call shape is the reference's: ``ndfft(input, output, handler, axis)``; `output` is written in
place.  Arrays are numpy arrays of ANY layout (host path, ndfft_exec) or torch tensors on an
MI355X (device path, ndfft_exec_device, asynchronous on torch's current stream).  The ``_par``
names exist for drop-in compatibility and dispatch to the same batched device call: on the GPU
every lane is always processed in parallel.
"""
import ctypes

import numpy as np

from . import _lib
from .handlers import DctHandler, FftHandler, Normalization, R2cFftHandler

try:  # torch is optional plumbing for device-resident arrays
    import torch
except Exception:  # pragma: no cover
    torch = None

_SPEC = {
    # op: (handler type, input is complex, output is complex)
    _lib.OP_C2C_FWD: (FftHandler, True, True),
    _lib.OP_C2C_INV: (FftHandler, True, True),
    _lib.OP_R2C: (R2cFftHandler, False, True),
    _lib.OP_C2R: (R2cFftHandler, True, False),
    _lib.OP_DCT1: (DctHandler, False, False),
    _lib.OP_DCT2: (DctHandler, False, False),
    _lib.OP_DCT3: (DctHandler, False, False),
    _lib.OP_DCT4: (DctHandler, False, False),
}


_PAR_DEVICES = None


def set_par_devices(device_ids):
    """Which GPUs the `_par` functions spread one call over (None / one id = the current device only).

    The reference's `_par` twins hand the independent lanes to rayon's worker threads (create_transform_par!,
    lib.rs:169-238); here the workers are GPUs: the array is cut in contiguous blocks along its outermost
    non-transform dimension, one per device, no collective (ndfft_exec_sharded / ndfft_exec_sharded_device)."""
    global _PAR_DEVICES
    ids = None if device_ids is None else [int(d) for d in device_ids]
    _PAR_DEVICES = ids if ids and len(ids) >= 1 else None


def par_devices():
    return None if _PAR_DEVICES is None else list(_PAR_DEVICES)


def _i64(v):
    return (ctypes.c_int64 * max(len(v), 1))(*[int(x) for x in v])


def _is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _np_dtype_of(x):
    if _is_torch(x):
        return np.dtype(str(x.dtype).replace("torch.", ""))
    return x.dtype


def _apply_custom_host(op, inp, handler, axis):
    """Normalization::Custom is a host fn pointer: run it on the host at the reference's
    application point.  C2R and DCT apply it BEFORE the transform, to a copy of each input lane
    (lib.rs:511-515, 692-696); returns the array to feed the device with NORM_NONE."""
    work = np.array(inp, copy=True, order="C")
    lanes = np.moveaxis(work, axis, -1)
    for idx in np.ndindex(lanes.shape[:-1]):
        lane = np.ascontiguousarray(lanes[idx])
        handler.norm.fn(lane)
        lanes[idx] = lane
    return work


def _transform(op, inp, out, handler, axis, par=False):
    htype, in_c, out_c = _SPEC[op]
    if not isinstance(handler, htype):
        raise TypeError(f"handler must be a {htype.__name__}")
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or axis < 0:
        raise TypeError("axis: usize")
    L = handler._L
    dev = _is_torch(inp) or _is_torch(out)
    if dev and not (_is_torch(inp) and _is_torch(out) and inp.is_cuda and out.is_cuda):
        raise TypeError("device path needs both arrays as torch tensors on the GPU")
    want_in = handler.complex_dtype if in_c else handler.real_dtype
    want_out = handler.complex_dtype if out_c else handler.real_dtype
    if _np_dtype_of(inp) != want_in or _np_dtype_of(out) != want_out:
        raise TypeError(f"element types must be {want_in} -> {want_out} for this handler")
    if inp.ndim != out.ndim:
        raise TypeError("input and output must have the same dimensionality D")

    norm = handler.norm
    mode, scale = _lib.NORM_DEFAULT, 0.0
    post_custom = False
    weights = post_weights = None
    if norm.kind == Normalization.NONE:
        mode = _lib.NORM_NONE
    elif norm.kind == Normalization.WEIGHTS:
        # the diagonal form of Custom: applied where Custom would be, replaces the default scaling.  Device tensors: the weighted entry point
        # (no host copy, no synchronisation); numpy arrays: one vectorised multiply on the host around ndfft_exec
        mode = _lib.NORM_NONE
        if op not in (_lib.OP_C2C_FWD, _lib.OP_R2C):
            post = op == _lib.OP_C2C_INV
            side = out if post else inp
            wlen = handler.n // 2 + 1 if op == _lib.OP_C2R else handler.n      # the weighted lane's length under this handler
            wdt = handler.complex_dtype if (post or in_c) else handler.real_dtype
            norm.host_weights(wdt, wlen)               # a vector of the wrong length: ValueError before anything runs
            if axis < side.ndim and int(side.shape[axis]) == wlen:     # (else the C side raises the reference's index / size panic)
                if dev:
                    weights = norm.device_weights(wdt, wlen, out.device)
                else:
                    w = norm.host_weights(wdt, wlen).reshape([wlen if d == axis else 1 for d in range(side.ndim)])
                    if post:
                        post_weights = w
                    else:
                        inp = inp * w                  # a copy of the input, weighted (broadcast along every other dim)
    elif norm.kind == "Custom":
        mode = _lib.NORM_NONE
        if op in (_lib.OP_C2C_FWD, _lib.OP_R2C):
            pass                                      # forward C2C / R2C never look at it (lib.rs:313-318, 497-503)
        elif op == _lib.OP_C2C_INV:
            post_custom = True                        # after, on the output lane (lib.rs:326-330)
        else:
            if dev:
                inp = torch.from_numpy(_apply_custom_host(op, inp.cpu().numpy(), handler, axis)).to(out.device)
            else:
                inp = _apply_custom_host(op, inp, handler, axis)

    if dev:
        if inp.device != out.device:
            raise ValueError(f"input is on {inp.device} but output is on {out.device}: both arrays must live on the same GPU")
        # torch's lazy conj / neg bits are not in the bytes data_ptr() points at: materialise them for the input,
        # refuse them on the output (writing through such a view would store the wrong sign)
        inp = inp.resolve_conj().resolve_neg()
        if out.is_conj() or out.is_neg():
            raise ValueError("output tensor has a lazy conj/neg bit set: pass a plain tensor (out.resolve_conj())")
        shape_in, shape_out = list(inp.shape), list(out.shape)
        sin, sout = list(inp.stride()), list(out.stride())
        # the C side picks twiddle tables, JIT modules and workspaces by the CURRENT device: make it the tensors' one
        with torch.cuda.device(out.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)
            if weights is not None:
                # (the sharded entry points take no weights: a _par call with weights runs on the current device alone)
                st = L.c.ndfft_exec_weighted_device(handler._plan, op, ctypes.c_void_p(inp.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                                    inp.ndim, _i64(shape_in), _i64(sin), _i64(shape_out), _i64(sout), int(axis),
                                                    ctypes.c_void_p(weights.data_ptr()), int(weights.shape[0]), stream)
            elif par and _PAR_DEVICES and len(_PAR_DEVICES) > 1:
                ids = (ctypes.c_int * len(_PAR_DEVICES))(*_PAR_DEVICES)
                st = L.c.ndfft_exec_sharded_device(handler._plan, op, ctypes.c_void_p(inp.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                                   inp.ndim, _i64(shape_in), _i64(sin), _i64(shape_out), _i64(sout), int(axis), mode,
                                                   scale, len(_PAR_DEVICES), ids, stream)
            else:
                st = L.c.ndfft_exec_device(handler._plan, op, ctypes.c_void_p(inp.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                       inp.ndim, _i64(shape_in), _i64(sin), _i64(shape_out), _i64(sout), int(axis), mode,
                                       scale, stream)
    else:
        if not out.flags.writeable:
            raise ValueError("output must be writeable (&mut)")
        sin = [s // inp.itemsize for s in inp.strides]
        sout = [s // out.itemsize for s in out.strides]
        if par and _PAR_DEVICES and len(_PAR_DEVICES) > 1:
            ids = (ctypes.c_int * len(_PAR_DEVICES))(*_PAR_DEVICES)
            st = L.c.ndfft_exec_sharded(handler._plan, op, ctypes.c_void_p(inp.ctypes.data), ctypes.c_void_p(out.ctypes.data), inp.ndim,
                                        _i64(inp.shape), _i64(sin), _i64(out.shape), _i64(sout), int(axis), mode, scale,
                                        len(_PAR_DEVICES), ids)
        else:
            st = L.c.ndfft_exec(handler._plan, op, ctypes.c_void_p(inp.ctypes.data), ctypes.c_void_p(out.ctypes.data), inp.ndim,
                                _i64(inp.shape), _i64(sin), _i64(out.shape), _i64(sout), int(axis), mode, scale)
    L.check(st)
    if post_weights is not None:
        out *= post_weights
    if post_custom:
        host = out.cpu().numpy() if dev else out
        lanes = np.moveaxis(host, axis, -1)
        for idx in np.ndindex(lanes.shape[:-1]):
            lane = np.ascontiguousarray(lanes[idx])
            norm.fn(lane)
            lanes[idx] = lane
        if dev:
            out.copy_(torch.from_numpy(host))


def ndfft(input, output, handler, axis): _transform(_lib.OP_C2C_FWD, input, output, handler, axis)
def ndifft(input, output, handler, axis): _transform(_lib.OP_C2C_INV, input, output, handler, axis)
def ndfft_r2c(input, output, handler, axis): _transform(_lib.OP_R2C, input, output, handler, axis)
def ndifft_r2c(input, output, handler, axis): _transform(_lib.OP_C2R, input, output, handler, axis)
def nddct1(input, output, handler, axis): _transform(_lib.OP_DCT1, input, output, handler, axis)
def nddct2(input, output, handler, axis): _transform(_lib.OP_DCT2, input, output, handler, axis)
def nddct3(input, output, handler, axis): _transform(_lib.OP_DCT3, input, output, handler, axis)
def nddct4(input, output, handler, axis): _transform(_lib.OP_DCT4, input, output, handler, axis)


def _filter_device(name, symbol, abi_minor, handler, input, output, axis, weights, wlen, mode, fuse, resolve):
    """The device half of ndfft_filter / nddct_filter: both arrays are torch tensors on the GPU and the argument types are checked.  `symbol`: the C entry point (ABI
    minor `abi_minor`); `resolve`: the tensor method that clears the lazy bit the weights' dtype can carry (resolve_conj: complex, resolve_neg: real)."""
    L = handler._L
    if not hasattr(L.c, symbol):
        raise _lib.NdfftError(_lib.ERR_UNSUPPORTED, f"this library build is older than ABI minor {abi_minor}: no {symbol}")
    if input.device != output.device:
        raise ValueError(f"input is on {input.device} but output is on {output.device}: both arrays must live on the same GPU")
    if input is not output:
        input = input.resolve_conj().resolve_neg()
    if input.is_conj() or input.is_neg() or output.is_conj() or output.is_neg():
        raise ValueError(f"a tensor written by the call has a lazy conj/neg bit set: pass a plain tensor (t.{resolve}())")
    if list(input.shape) != list(output.shape) and axis < input.ndim:
        raise _lib.Panic(_lib.ERR_SHAPE_MISMATCH, f"{name}: input shape {tuple(input.shape)} differs from output shape {tuple(output.shape)}")
    with torch.cuda.device(output.device):
        if _is_torch(weights):
            if weights.device != output.device:
                raise ValueError("weights must live on the arrays' GPU")
            wd = getattr(weights, resolve)().contiguous()
        else:
            wd = torch.from_numpy(np.ascontiguousarray(weights)).to(output.device)     # (stream-ordered: the caching allocator keeps it alive for the stream's work)
        stream = ctypes.c_void_p(torch.cuda.current_stream(output.device).cuda_stream)
        st = getattr(L.c, symbol)(handler._plan, ctypes.c_void_p(input.data_ptr()), ctypes.c_void_p(output.data_ptr()), input.ndim,
                                  _i64(list(input.shape)), _i64(list(input.stride())), _i64(list(output.stride())), int(axis),
                                  ctypes.c_void_p(wd.data_ptr()), wlen, mode, 0.0, 0 if fuse else _lib.FILTER_NO_FUSE, stream)
    L.check(st)


def ndfft_filter(input, output, handler, axis, weights, *, fuse=True):
    """output = IFFT(weights * FFT(input)) along `axis`, lane by lane: what ndfft -> `lane *= weights` -> ndifft give under the handler's normalisation (None:
    unscaled, Default: 1 / n), in one call.  handler: an FftHandler (complex arrays, n weights) or an R2cFftHandler (real arrays, n // 2 + 1 complex weights;
    meaning ndfft_r2c -> multiply -> ndifft_r2c).  `input is output` is the in-place filter.

    torch tensors on the GPU go to ndfft_exec_filter_device (asynchronous on the current stream): one fused kernel for unit-stride power-of-two lanes -- complex
    lanes of 64 .. 4096 points (path "filter_pow2"), real lanes of 128 .. 8192 points that start on even element offsets ("filter_r2c_pow2") --, one fused
    kernel of column tiles for complex lanes of 128 .. 2048 points along a strided axis whose neighbouring lanes are adjacent in both arrays (axis 0 of a 2-D
    C-layout array, the middle axis of a 3-D one, windows of either; at least 8 adjacent lanes, at most two batch dims; path "filter_col_pow2"), and transform +
    diagonal pass + transform otherwise (fuse=False forces that form).  `weights` is then a device tensor of the handler's complex dtype, or a
    numpy array that is uploaded once per call.  numpy arrays run the three steps through the host calls."""
    if not isinstance(handler, (FftHandler, R2cFftHandler)):
        raise TypeError("handler must be an FftHandler or an R2cFftHandler")
    if handler.norm.kind not in (Normalization.NONE, Normalization.DEFAULT):
        raise ValueError("ndfft_filter: the handler's normalisation must be None or Default")
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or axis < 0:
        raise TypeError("axis: usize")
    r2c = isinstance(handler, R2cFftHandler)
    cdt, adt = np.dtype(handler.complex_dtype), np.dtype(handler.real_dtype if r2c else handler.complex_dtype)
    wlen = handler.n // 2 + 1 if r2c else handler.n
    dev = _is_torch(input) or _is_torch(output)
    if dev and not (_is_torch(input) and _is_torch(output) and input.is_cuda and output.is_cuda):
        raise TypeError("device path needs both arrays as torch tensors on the GPU")
    if _np_dtype_of(input) != adt or _np_dtype_of(output) != adt:
        raise TypeError(f"element types must be {adt} -> {adt} for this handler")
    if input.ndim != output.ndim:
        raise TypeError("input and output must have the same dimensionality D")
    if _np_dtype_of(weights) != cdt or weights.ndim != 1:
        raise TypeError(f"weights: a vector of {cdt}")
    if int(weights.shape[0]) != wlen:
        raise ValueError(f"weights: got {int(weights.shape[0])} expected {wlen}")
    mode = _lib.NORM_NONE if handler.norm.kind == Normalization.NONE else _lib.NORM_DEFAULT
    if not dev:
        if _is_torch(weights):
            raise TypeError("numpy arrays take numpy weights")
        fwd, inv = (ndfft_r2c, ndifft_r2c) if r2c else (ndfft, ndifft)
        sshape = [wlen if d == axis else int(s) for d, s in enumerate(input.shape)]
        spec = np.zeros(sshape, cdt)
        fwd(input, spec, handler, axis)
        spec *= np.asarray(weights).reshape([wlen if d == axis else 1 for d in range(input.ndim)])
        inv(spec, output, handler, axis)
        return
    _filter_device("ndfft_filter", "ndfft_exec_filter_device", 5, handler, input, output, axis, weights, wlen, mode, fuse, "resolve_conj")


def nddct_filter(input, output, handler, axis, weights, *, fuse=True):
    """output = DCT3(weights * DCT2(input)) along `axis`, lane by lane: what nddct2 -> `lane *= weights` -> nddct3 give under the handler's normalisation (None:
    unscaled, Default: each call pre-scales by 2, so 4 in all), in one call; unit weights return (n / 2) * input under None.  handler: a DctHandler; both arrays in
    its real dtype; `weights`: n reals of that dtype.  `input is output` is the in-place filter.

    torch tensors on the GPU go to ndfft_exec_dct_filter_device (asynchronous on the current stream): one fused kernel for unit-stride power-of-two lanes of
    128 .. 8192 points at any offset and pitch (path "filter_dct_pow2"), and nddct2 + diagonal pass + nddct3 otherwise (fuse=False forces that form).  `weights` is
    then a device tensor, or a numpy array that is uploaded once per call.  numpy arrays run the three steps through the host calls."""
    if not isinstance(handler, DctHandler):
        raise TypeError("handler must be a DctHandler")
    if handler.norm.kind not in (Normalization.NONE, Normalization.DEFAULT):
        raise ValueError("nddct_filter: the handler's normalisation must be None or Default")
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or axis < 0:
        raise TypeError("axis: usize")
    rdt = np.dtype(handler.real_dtype)
    n = handler.n
    dev = _is_torch(input) or _is_torch(output)
    if dev and not (_is_torch(input) and _is_torch(output) and input.is_cuda and output.is_cuda):
        raise TypeError("device path needs both arrays as torch tensors on the GPU")
    if _np_dtype_of(input) != rdt or _np_dtype_of(output) != rdt:
        raise TypeError(f"element types must be {rdt} -> {rdt} for this handler")
    if input.ndim != output.ndim:
        raise TypeError("input and output must have the same dimensionality D")
    if _np_dtype_of(weights) != rdt or weights.ndim != 1:
        raise TypeError(f"weights: a vector of {rdt}")
    if int(weights.shape[0]) != n:
        raise ValueError(f"weights: got {int(weights.shape[0])} expected {n}")
    mode = _lib.NORM_NONE if handler.norm.kind == Normalization.NONE else _lib.NORM_DEFAULT
    if not dev:
        if _is_torch(weights):
            raise TypeError("numpy arrays take numpy weights")
        coef = np.zeros([int(s) for s in input.shape], rdt)
        nddct2(input, coef, handler, axis)
        coef *= np.asarray(weights).reshape([n if d == axis else 1 for d in range(input.ndim)])
        nddct3(coef, output, handler, axis)
        return
    _filter_device("nddct_filter", "ndfft_exec_dct_filter_device", 6, handler, input, output, axis, weights, n, mode, fuse, "resolve_neg")


# #[cfg(feature = "parallel")] twins (lib.rs:374-421, 589-611, 777-844).  On one GPU every lane is processed in
# parallel anyway, so they are the same batched call; with set_par_devices([...]) they spread the call over several GPUs.
def ndfft_par(input, output, handler, axis): _transform(_lib.OP_C2C_FWD, input, output, handler, axis, par=True)
def ndifft_par(input, output, handler, axis): _transform(_lib.OP_C2C_INV, input, output, handler, axis, par=True)
def ndfft_r2c_par(input, output, handler, axis): _transform(_lib.OP_R2C, input, output, handler, axis, par=True)
def ndifft_r2c_par(input, output, handler, axis): _transform(_lib.OP_C2R, input, output, handler, axis, par=True)
def nddct1_par(input, output, handler, axis): _transform(_lib.OP_DCT1, input, output, handler, axis, par=True)
def nddct2_par(input, output, handler, axis): _transform(_lib.OP_DCT2, input, output, handler, axis, par=True)
def nddct3_par(input, output, handler, axis): _transform(_lib.OP_DCT3, input, output, handler, axis, par=True)
def nddct4_par(input, output, handler, axis): _transform(_lib.OP_DCT4, input, output, handler, axis, par=True)


def pinned_empty(shape, dtype, _library=None):
    """A C-layout numpy array in page-locked host memory from ndfft_host_alloc: ndfft_exec on such arrays overlaps
    upload, transform and download (include/ndfft_mi355x.h).  The memory is released when the array (and every
    view of it) is garbage-collected."""
    import weakref
    L = _library or _lib.default()
    dt = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    p = ctypes.c_void_p()
    L.check(L.c.ndfft_host_alloc(ctypes.byref(p), max(n * dt.itemsize, 1)))
    buf = (ctypes.c_char * max(n * dt.itemsize, 1)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dt, count=n).reshape(shape)
    weakref.finalize(buf, L.c.ndfft_host_free, p)
    return arr
