"""The kept share of the streaming-load row kernels (Pow2Args::keep64; pow2_kernel.h: run, device_common.h: keep_block): the cases shared by the CPU build of
the kernel sources (tests/test_pow2_keep_emul.py) and the MI355X (tests/test_gpu_pow2_keep.py).  The streaming policy is forced (NDFFT_STREAM_LOADS=1) and
the share is forced to each of SHARES (ndfft_force_input_keep); which lanes load with which policy changes speed only, so every output must equal the share-0 output bit
for bit, and that one the reference at helpers.TOL.  Every call asserts the route, the policy and the share that ran."""
import numpy as np

import devmem
import filter_instances_suite as fis
import parity_suite as ps
from helpers import TOL, assert_close
from ndrustfft_amd import _lib

SHARES = (0, 1, 2, 3, 8, 37, 63)
ROUTE = "pow2_reg"
# (real dtype, n, lanes, route switches)
#   n = 4096 x 130: blocks of one lane, two periods of 64 plus a ragged tail of two; 130 one-lane workgroups engage the XCD lane map (>= 128 blocks);
#       c64 lanes of 32 KiB are blocks of two, in the instance with two elements per access
#   n = 64 x 1000 on the register kernel (NDFFT_WAVE=0): four lanes per workgroup, 64 (c128) / 128 (c64) lanes per block -- at shares 1 .. 3 workgroups
#       straddle the limit between kept and streamed blocks; c64: the instance with 8-byte accesses
CASES = (
    (np.float64, 4096, 130, {}),
    (np.float64, 64, 1000, {"NDFFT_WAVE": "0"}),
    (np.float32, 4096, 130, {}),
    (np.float32, 64, 1000, {"NDFFT_WAVE": "0"}),
)
IDS = [f"{np.dtype(dt).name}-{n}x{rows}" for dt, n, rows, _ in CASES]
OFFSET = 2        # elements between the allocation's base and the offset view (16 bytes in c64: the same instance as the dense call)

_REF = {}         # (name, dtype, rows, n) -> reference output, computed once, never written


def reference(name, x, rdt, ref):
    key = (name, np.dtype(rdt).name, x.shape)
    if key not in _REF:
        _REF[key] = ref(name, x, 1); _REF[key].setflags(write=False)
    return _REF[key]


def call(L, h, name, x, keep, offset, env):
    rows, n = x.shape
    xa = np.full(rows * n + 2 * offset, devmem.SENTINEL, x.dtype); xa[offset:offset + rows * n] = x.reshape(-1)
    ya = np.full(rows * n + 2 * offset, devmem.SENTINEL, x.dtype)
    xv, yv = xa[offset:offset + rows * n].reshape(rows, n), ya[offset:offset + rows * n].reshape(rows, n)
    L.force_input_keep(keep)
    try:
        with ps.switches(L, NDFFT_STREAM_LOADS="1", **env):
            img, path, _ = devmem.dev_call(L, h, name, xa, xv, ya, yv, 1, weighted=False, norm=_lib.NORM_DEFAULT)
            assert path == ROUTE, f"{name} {x.shape} took {path}"
            assert L.last_input_policy() == 1 and L.last_input_keep() == keep, (L.last_input_policy(), L.last_input_keep(), keep)
    finally:
        L.force_input_keep(-1)
    assert (img[:offset] == devmem.SENTINEL).all() and (img[offset + rows * n:] == devmem.SENTINEL).all(), "the call wrote outside the output view"
    return np.ascontiguousarray(img[offset:offset + rows * n].reshape(rows, n))


def identity(L, rdt, n, rows, env, ref, offset):
    """Forward and inverse: every share's output equals the share-0 output bit for bit, which meets `ref(name, x, axis)` at helpers.TOL."""
    for name in ("ndfft", "ndifft"):
        h, _ = ps.handlers_for(name, n, rdt, L)
        x = ps.make_input(name, (rows, n), rdt, offset=n + rows)
        base = call(L, h, name, x, 0, offset, env)
        assert_close(base, reference(name, x, rdt, ref), 1, TOL[np.dtype(rdt)], f"{name} ({rows}, {n}) offset={offset} share 0")
        for keep in SHARES[1:]:
            got = call(L, h, name, x, keep, offset, env)
            assert got.tobytes() == base.tobytes(), f"{name} ({rows}, {n}) offset={offset}: share {keep} differs from share 0"
    fis.settle_residency_model(L)          # the tests after this one see no buffer of it in the residency model
