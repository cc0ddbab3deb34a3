"""FftHandler / R2cFftHandler / DctHandler / Normalization -- host-side mirror of
/root/reference/src/lib.rs:89-98, 269-311, 451-495, 640-686 over the C ABI."""
import ctypes

import numpy as np

from . import _lib


class Normalization:
    """enum Normalization<T> { None, Default, Custom(fn(&mut [T])) }  (lib.rs:89-98), and Weights(w): the diagonal form of Custom, a vector
    of per-element factors that is applied on the device (include/ndfft_mi355x_ext.h)."""
    NONE = "None"
    DEFAULT = "Default"
    WEIGHTS = "Weights"

    def __init__(self, kind, fn=None, w=None):
        self.kind, self.fn = kind, fn
        self._w = w                # Weights: the vector as given (1-D numpy array)
        self._host = {}            # element dtype -> the vector cast to it
        self._dev = {}             # (element dtype, torch device) -> device copy

    @staticmethod
    def none():
        return Normalization(Normalization.NONE)

    @staticmethod
    def default():
        return Normalization(Normalization.DEFAULT)

    @staticmethod
    def custom(fn):
        """fn(lane) mutates one 1-D numpy lane in place -- a host function, as in the reference."""
        return Normalization("Custom", fn)

    @staticmethod
    def weights(w):
        """A diagonal normalisation: the lane is multiplied element by element by `w` (1-D numpy array or torch tensor) where the reference
        would call a custom function -- after the transform for ndifft (n complex factors), before it for ndifft_r2c (n/2 + 1 complex factors)
        and nddct1..4 (n real factors); ndfft and ndfft_r2c ignore it.  Like Custom it replaces the default scaling.  `w` is cast to the
        handler's element type at first use; for device tensors its device copy is cached here, per device, and the call stays on the GPU."""
        if hasattr(w, "detach"):
            w = w.detach().cpu().numpy()
        w = np.array(w, copy=True)
        if w.ndim != 1:
            raise ValueError("weights must be one-dimensional")
        return Normalization(Normalization.WEIGHTS, w=w)

    @staticmethod
    def weights_from(fn, n, dtype):
        """Normalization.weights for a custom function that is DIAGONAL (element-wise and linear): w = fn(ones).  Checked on a seeded random lane r:
        fn(r) must equal w * r to 4 eps of each element, else ValueError("not an element-wise function")."""
        dtype = np.dtype(dtype)
        w = np.ones(n, dtype)
        fn(w)
        rng = np.random.default_rng(20240607)
        r = rng.uniform(-1.0, 1.0, n)
        if dtype.kind == "c":
            r = r + 1j * rng.uniform(-1.0, 1.0, n)
        r = r.astype(dtype)
        got = r.copy()
        fn(got)
        want = w * r
        eps = np.finfo(dtype).eps
        if got.shape != want.shape or not np.all(np.abs(got - want) <= 4 * eps * np.abs(want)):
            raise ValueError("not an element-wise function")
        return Normalization.weights(w)

    def host_weights(self, dtype, length):
        """The vector in element type `dtype`; ValueError unless it has `length` entries."""
        if self._w.shape[0] != length:
            raise ValueError(f"weights: got {self._w.shape[0]} expected {length} (the length of the weighted lane)")
        dtype = np.dtype(dtype)
        if dtype not in self._host:
            if dtype.kind != "c" and np.iscomplexobj(self._w):
                raise TypeError("complex weights on a real lane")
            self._host[dtype] = np.ascontiguousarray(self._w.astype(dtype))
        return self._host[dtype]

    def device_weights(self, dtype, length, device):
        """The same as a torch tensor on `device` (uploaded once per element type and device)."""
        import torch
        w = self.host_weights(dtype, length)
        key = (np.dtype(dtype), str(device))
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(w).to(device)
        return self._dev[key]


def _dtype_code(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return _lib.F32
    if dtype == np.float64:
        return _lib.F64
    raise TypeError("T must be f32 or f64 (FftNum, lib.rs:111)")


class _Handler:
    KIND = None

    def __init__(self, n, dtype=np.float64, *, _library=None, _share=None):
        self.n = int(n)
        self.dtype = np.dtype(dtype)
        self.norm = Normalization.default()          # lib.rs:302, 486, 677
        self._L = _library or _lib.default()
        if _share is not None:                        # Clone = Arc bump (lib.rs:269, 451, 640)
            self._plan = _share
            self._L.check(self._L.c.ndfft_plan_retain(self._plan))
        else:
            p = ctypes.c_void_p()
            self._L.check(self._L.c.ndfft_plan_create(self.KIND, _dtype_code(dtype), self.n, ctypes.byref(p)))
            self._plan = p

    def normalization(self, norm):
        """Builder: consumes and returns the handler (lib.rs:308-311, 492-495, 683-686)."""
        if norm is None:
            norm = Normalization.none()
        self.norm = norm
        return self

    def clone(self):
        h = type(self)(self.n, self.dtype, _library=self._L, _share=self._plan)
        h.norm = self.norm
        return h

    @property
    def real_dtype(self):
        return self.dtype

    @property
    def complex_dtype(self):
        return np.dtype(np.complex64 if self.dtype == np.float32 else np.complex128)

    def __del__(self):
        try:
            self._L.c.ndfft_plan_destroy(self._plan)
        except Exception:
            pass


class FftHandler(_Handler):
    """FftHandler<T>::new(n)  (lib.rs:294-304)."""
    KIND = _lib.KIND_C2C


class R2cFftHandler(_Handler):
    """R2cFftHandler<T>::new(n), m = n/2 + 1  (lib.rs:477-488)."""
    KIND = _lib.KIND_R2C

    @property
    def m(self):
        return self.n // 2 + 1


class DctHandler(_Handler):
    """DctHandler<T>::new(n): plans DCT-I..IV eagerly  (lib.rs:665-679)."""
    KIND = _lib.KIND_DCT
