"""The stream contract of the device entry points (docs/streams.md): ndfft_exec_device, ndfft_exec_weighted_device, ndfft_exec_filter_device and
ndfft_exec_dct_filter_device are asynchronous on the caller's stream and, once a shape has been warmed up on a (host thread, stream), neither allocate nor
wait.  A Spec is one call whose geometry is given by host views, made through ctypes on the base addresses of two device allocations -- so that the same
specs run on the CPU build of the kernel sources with its call log (tests/test_stream_emul.py: deterministic) and on torch tensors on the MI355X
(tests/test_stream_gpu.py: the real runtime, side streams and captured graphs)."""
import ctypes

import numpy as np

import devmem
import filter_dct_suite as fds
import filter_suite as fs
import parity_suite as ps
import weights_suite as ws
from helpers import TOL, assert_close, cdt_of
from ndrustfft_amd import _lib, api, handlers

# Routes that allocate or wait on a warmed-up (host thread, stream) BY DESIGN: route -> reason.  Each entry needs its sentence beside the route's description in
# include/ndfft_mi355x.h / ndfft_mi355x_ext.h.  Empty: no route does.
WARM_EXCEPTIONS = {}


class Spec:
    """One call.  xa / ya: host images of the input and output allocation, xv / yv: the views in them the call works on; w: the weights (None: the entry point
    takes none); expect: the oracle's output, in yv's shape; invoke(din, dout, dw, stream) -> status: the call on device copies of xa, ya and w at those
    base addresses; want: the route -- a name, a tuple of names, None (any) or a predicate of the path."""
    def __init__(self, label, env, rdt, axis, xa, xv, ya, yv, w, expect, invoke, want, remake):
        self.label, self.env, self.rdt, self.axis, self.xa, self.xv, self.ya, self.yv, self.w = label, env, np.dtype(rdt), axis, xa, xv, ya, yv, w
        self.expect, self.invoke, self.want, self.remake = expect, invoke, want, remake

    def route_ok(self, path):
        return self.want(path) if callable(self.want) else ps._route_ok(path, self.want)

    def input_with(self, offset):
        """The input view's contents for another seed (the allocation outside the view is left alone)."""
        return self.remake(offset)


_FIRST_MULTI_PASS = {}


def first_multi_pass_length(L, kind, rdt):
    """weights_suite.first_multi_pass_length, scanned once per library, plan kind and dtype (it makes a plan per length)."""
    key = (L.path, kind, np.dtype(rdt))
    if key not in _FIRST_MULTI_PASS:
        _FIRST_MULTI_PASS[key] = ws.first_multi_pass_length(L, kind, rdt)
    return _FIRST_MULTI_PASS[key]


def _ptr(base, v, a):
    return ctypes.c_void_p(base + devmem._off(v, a))


def _sp(stream):
    return ctypes.c_void_p(stream) if stream else None


# ---- the cases: plain tuples (they name the pytest ids), turned into Specs under the case's switches -------------------------------------------------
def exec_case(row):
    """A ROUTE_TABLE row (switches, op, shape, axis, real dtype, layout, route)."""
    return ("exec",) + tuple(row)


def stepped_case(row):
    """A ROUTE_TABLE_STEPPED row (switches, op, n, real dtype, route): lanes of every second element on padded rows."""
    return ("stepped",) + tuple(row)


def weighted_cases(dtypes=(np.float64,)):
    """weights_suite.multi_pass_routes's calls (f64 there): (op, plan kind, form, dtype) with form 0 rows, 1 a strided axis, 2 an output view stepped along the axis."""
    return [("weighted", name, kind, form, np.dtype(rdt).type) for rdt in dtypes for name, kind in (("nddct2", _lib.KIND_DCT), ("ndifft_r2c", _lib.KIND_R2C))
            for form in (0, 1, 2)]


def no_fuse_filter_cases(dtypes=fs.BOTH):
    """ndfft_filter on a C2C plan and on an R2C plan with NDFFT_FILTER_NO_FUSE, at a length the fused kernels would take."""
    return [("filter", kind, (5, 256), np.dtype(rdt).type, _lib.FILTER_NO_FUSE) for rdt in dtypes for kind in ("c2c", "r2c")]


def composed_filter_cases(dtypes=fs.BOTH):
    """... nddct_filter composed, and one composed filter whose inner route is itself multi-pass: a C2C plan at weights_suite.first_multi_pass_length."""
    out = no_fuse_filter_cases(dtypes)
    out += [("filter", "dct", (5, 256), np.dtype(rdt).type, _lib.FILTER_NO_FUSE) for rdt in dtypes]
    out += [("filter", "c2c", (2, "first_multi_pass_length"), np.dtype(rdt).type, 0) for rdt in dtypes]
    return out


def multi_pass_exec_cases(dtypes=(np.float64, np.float32)):
    """The multi-pass routes of ndfft_exec_device at the smallest shape of each."""
    out = []
    for rdt in dtypes:
        out += [exec_case(({}, "ndfft", (2, 32768), 1, rdt, "C", "four_step")), exec_case(({}, "ndfft_r2c", (2, 65536), 1, rdt, "C", "real_four_step")),
                exec_case(({}, "ndfft", (4096, 16), 0, rdt, "C", "col_split")),
                exec_case(({"NDFFT_COLSPLIT": "0"}, "ndfft", (4096, 24), 0, rdt, "C", "transpose+pow2_reg")),
                exec_case(({}, "ndfft", (3, 4099), 1, rdt, "C", "blue_global"))]
    return out


def case_id(case):
    def one(v):
        if isinstance(v, dict): return ",".join(f"{k}={x}" for k, x in sorted(v.items())) or "-"
        if isinstance(v, type): return np.dtype(v).name
        if isinstance(v, tuple): return "x".join(str(e) for e in v)
        return str(v)
    return "-".join(one(v) for v in case)


def case_env(case):
    return dict(case[1]) if case[0] in ("exec", "stepped") else {}


def make_spec(L, case, offset=0):
    """The Spec of a case; call it, and make every call of the Spec, under ps.switches(L, **case_env(case))."""
    kind = case[0]
    if kind in ("exec", "stepped"):
        if kind == "exec":
            env, name, shape, axis, rdt, layout, want = case[1:]
            sin, sout = ps.shapes_for(name, shape, axis)
            gen = lambda off: ps.make_input(name, sin, rdt, offset=off)
            x = gen(offset)
            xa, xv = devmem.in_alloc(x, layout)
        else:
            env, name, n, rdt, want = case[1:]
            shape, axis, layout = (3, n), 1, "C"
            sin, sout = ps.shapes_for(name, shape, axis)
            assert sin == sout
            gen = lambda off: ps.make_input(name, (3, 2 * n + 3), rdt, offset=off)[:, 1:2 * n + 1:2]
            xa = ps.make_input(name, (3, 2 * n + 3), rdt, offset=offset); xv = xa[:, 1:2 * n + 1:2]
        ya, yv = devmem.out_alloc(name, shape, axis, rdt, None, layout)
        h, o = ps.handlers_for(name, shape[axis], rdt, L)
        yo = np.zeros(sout, yv.dtype); ps.OPS[name][1](np.ascontiguousarray(xv), yo, o, axis)

        def invoke(din, dout, dw, stream):
            return L.c.ndfft_exec_device(h._plan, devmem.OPC[name], _ptr(din, xv, xa), _ptr(dout, yv, ya), xv.ndim, api._i64(xv.shape), api._i64(devmem.strides_of(xv)),
                                         api._i64(yv.shape), api._i64(devmem.strides_of(yv)), axis, _lib.NORM_DEFAULT, 0.0, _sp(stream))
        return Spec(case_id(case), env, rdt, axis, xa, xv, ya, yv, None, yo, invoke, want, gen)
    if kind == "weighted":
        _, name, plan_kind, form, rdt = case
        n = first_multi_pass_length(L, plan_kind, rdt)
        _, so = ps.shapes_for(name, (4, n), 1)
        shape, axis, out_view, prefix = (((4, n), 1, None, "weights+"), ((n, 16), 0, None, "weights+transpose+"),
                                         ((4, n), 1, ((4, 2 * so[1]), np.s_[:, ::2]), "weights+pack+"))[form]
        sin, sout = ps.shapes_for(name, shape, axis)
        gen = lambda off: ps.make_input(name, sin, rdt, offset=off)
        x = gen(offset)
        xa, xv = devmem.in_alloc(x)
        ya, yv = devmem.out_alloc(name, shape, axis, rdt, out_view)
        w = np.ascontiguousarray(ws.make_weights(name, n, rdt))
        h = getattr(handlers, ps.OPS[name][2])(n, rdt, _library=L)
        yo = ws.oracle_weighted(name, x, w, n, axis, rdt)

        def invoke(din, dout, dw, stream):
            return L.c.ndfft_exec_weighted_device(h._plan, devmem.OPC[name], _ptr(din, xv, xa), _ptr(dout, yv, ya), xv.ndim, api._i64(xv.shape), api._i64(devmem.strides_of(xv)),
                                                  api._i64(yv.shape), api._i64(devmem.strides_of(yv)), axis, ctypes.c_void_p(dw), len(w), _sp(stream))
        multi = lambda path: path.startswith(prefix) and (form != 0 or not path.startswith(("weights+transpose+", "weights+pack+")))
        return Spec(case_id(case), {}, rdt, axis, xa, xv, ya, yv, w, yo, invoke, multi, gen)
    if kind == "filter":
        _, plan, shape, rdt, flags = case
        if shape[1] == "first_multi_pass_length":
            shape = (shape[0], first_multi_pass_length(L, _lib.KIND_C2C, rdt))
        n, axis = shape[1], 1
        if plan == "dct":
            gen = lambda off: fds.make_x(shape, rdt, seed=off + 1)
            w = np.ascontiguousarray(fds.make_g(n, rdt, seed=3)); h = fds.handler(L, n, rdt)
            x = gen(offset); yo = fds.oracle_filter(x, w, n, axis, rdt)
            entry = L.c.ndfft_exec_dct_filter_device
        else:
            r2c = plan == "r2c"
            gen = lambda off: fs.make_x(shape, rdt, r2c, seed=off + 1)
            w = np.ascontiguousarray(fs.make_weights(fs.wname(r2c), n, rdt, seed=3)); h = fs.handler(L, n, rdt, r2c)
            x = gen(offset); yo = fs.oracle_filter(x, w, n, axis, rdt, r2c)
            entry = L.c.ndfft_exec_filter_device
        xa, xv = devmem.in_alloc(x)
        ya = np.full(shape, devmem.SENTINEL, x.dtype); yv = ya

        def invoke(din, dout, dw, stream):
            return entry(h._plan, _ptr(din, xv, xa), _ptr(dout, yv, ya), xv.ndim, api._i64(xv.shape), api._i64(devmem.strides_of(xv)), api._i64(devmem.strides_of(yv)),
                         axis, ctypes.c_void_p(dw), len(w), _lib.NORM_DEFAULT, 0.0, flags, _sp(stream))

        def composed(path):
            fwd, _, inv = path.partition("+weights+")
            multi = ("four_step", "blue_global")
            return bool(inv) and "filter_" not in path and (flags or (any(m in fwd for m in multi) and any(m in inv for m in multi)))
        return Spec(case_id(case), {}, rdt, axis, xa, xv, ya, yv, w, yo, invoke, composed, gen)
    raise ValueError(case)


def view_of(spec, got):
    """The output view in a downloaded image of the output allocation."""
    return got.reshape(-1)[devmem.view_index(spec.ya, spec.yv)]


# ---- the CPU emulation: the call log of tests/emul/emul_runtime.cpp -----------------------------------------------------------------------------------
ON = ("launch", "memcpy_async", "memset_async", "event_record", "wait_event")
COUNTERS = ("hipMalloc", "hipFree", "hipHostMalloc", "hipMemcpy", "hipMemset", "hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize")
LOG_CAP = 1 << 16
HANDLE_A, HANDLE_B = 0x5A5A0A00, 0x5B5B0B00          # two stream handles: the emulation never dereferences one


def call_log(L, reset=True):
    """([(kind, stream handle)] of the stream-ordered calls, {counter: count}) of this thread since the last reset."""
    L.c.emul_call_log.restype = ctypes.c_longlong
    streams = (ctypes.c_void_p * LOG_CAP)(); kinds = (ctypes.c_int * LOG_CAP)(); counts = (ctypes.c_longlong * len(COUNTERS))()
    total = L.c.emul_call_log(streams, kinds, LOG_CAP, counts, 1 if reset else 0)
    assert total <= LOG_CAP, f"{total} stream-ordered calls: more than the log holds"
    return [(ON[kinds[i]], streams[i] or 0) for i in range(total)], dict(zip(COUNTERS, counts))


def _logged(L, spec, bufs, stream):
    call_log(L)
    L.check(spec.invoke(*bufs, stream))
    path = L.last_path()
    calls, counts = call_log(L)
    return path, calls, counts


def _off_stream(calls, stream):
    return [f"{kind} #{i} on {'the null stream' if not s else hex(s)}" for i, (kind, s) in enumerate(calls) if s != stream]


def warm_call_contract(L, case):
    """One case on the emulation, under its switches.  (1) A first call on stream A builds the plan's tables; ndfft_release_workspace then frees this thread's
    scratch, and the warm-up call on A allocates it again -- scratch and nothing else, counted.  (2) The same call on A logs at least one launch, every logged
    stream handle is A, nothing was allocated, freed, copied synchronously or waited for, the route is the case's and the result is within helpers.TOL of the
    oracle.  (3) The call on a second stream B stays on B and allocates exactly as often as the warm-up on A did: scratch is per stream, so a slot that B shares
    with A (one keyed without the stream) shows as a missing allocation.  (4) Back on A nothing is allocated and every handle is A: B's call did not evict A's
    scratch.  A route listed in WARM_EXCEPTIONS may allocate and wait in (2) and (4); nothing may leave its stream."""
    with ps.switches(L, **case_env(case)):
        sp = make_spec(L, case)
        din, dout = devmem.DevBuf(L, sp.xa), devmem.DevBuf(L, sp.ya)
        dw = devmem.DevBuf(L, sp.w) if sp.w is not None else None
        bufs = (din.p.value, dout.p.value, dw.p.value if dw else 0)
        bad = []
        try:
            L.check(sp.invoke(*bufs, HANDLE_A))                                   # (1) tables; then the warm-up proper, from no scratch at all
            L.check(L.c.ndfft_release_workspace())
            path, calls, warm = _logged(L, sp, bufs, HANDLE_A)
            bad += [f"{sp.label} [{path}] step 1: warm-up on A: {m}" for m in _off_stream(calls, HANDLE_A)]
            for step, stream in (("2: warm call on A", HANDLE_A), ("3: first call on B", HANDLE_B), ("4: A again after B", HANDLE_A)):
                dout.upload(sp.ya)
                path, calls, counts = _logged(L, sp, bufs, stream)
                got = dout.download(sp.ya)
                what = f"{sp.label} [{path}] step {step}"
                if not any(kind == "launch" for kind, _ in calls):
                    bad.append(f"{what}: no kernel launch was logged")
                bad += [f"{what}: {m}" for m in _off_stream(calls, stream)]
                if stream == HANDLE_A and path not in WARM_EXCEPTIONS:
                    bad += [f"{what}: {v} x {k}" for k, v in counts.items() if v]
                if stream == HANDLE_B and counts["hipMalloc"] != warm["hipMalloc"]:
                    bad.append(f"{what}: {counts['hipMalloc']} allocations, the warm-up on A made {warm['hipMalloc']}: the two streams share scratch")
                if not sp.route_ok(path):
                    bad.append(f"{what}: not the case's route")
                mask = devmem.view_mask(sp.ya, sp.yv)
                if not np.array_equal(got[mask], np.full(int(mask.sum()), devmem.SENTINEL, got.dtype)):
                    bad.append(f"{what}: an element outside the output view was written")
                assert_close(view_of(sp, got), sp.expect, sp.axis, TOL[sp.rdt], what)
        finally:
            din.free(); dout.free()
            if dw: dw.free()
    assert not bad, "\n".join([f"{len(bad)} breaches of the stream contract"] + bad)
    return path
