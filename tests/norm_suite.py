"""NORM_NONE, NORM_DEFAULT and NORM_SCALE on every kernel route (docs/accuracy.md, "Normalisation modes"): the cases shared by the CPU build of the kernel
sources (tests/test_norm_emul.py) and the MI355X (tests/test_norm_gpu.py).  exec.hip's prepare() turns (norm, scale) into one scalar that every launcher hands
to its kernel, and each route applies it somewhere else: on the output lane (inverse C2C), on the complex input lane (C2R), on the input lane or inside the
folds as 0.5 * scale (DCTs), in one of the two passes of a four-step form, inside the Rader gather, in the hiprtc kernels.  Under NORM_DEFAULT that scalar is 2
or 1 / n -- exact scalings that hide a factor dropped on some elements, rounded through the wrong type, or special-cased at 1.

Every call goes through the C ABI (ctypes) on device images of dense arrays.  Per case, one uploaded input and the mode set MODES:

  route   every call reports the same ndfft_last_path(), the one the case names (parity_suite._route_ok)
  P1      ndfft, ndfft_r2c: all outputs byte-identical (forward ops ignore the normalisation)
  P2      out(SCALE, 2^-3) == out(NONE) * T(2^-3), element for element, both finite: a power of two commutes with every rounding (with or without FMA
          contraction, wherever the factor is applied, nothing subnormal on these inputs), so there is no tolerance; uniform and impulse inputs
  P3      out(DEFAULT) == 2 * out(NONE) for the DCTs, == out(NONE) * T(1 / n) for ndifft / ndifft_r2c at power-of-two n
  P4      out(SCALE, 0.37) under the bar of docs/accuracy.md, unchanged: truth = accuracy.truth() * (T(0.37) / Default factor) in long double, the bar's
          oracle = the CPU oracle under Custom(lane *= T(0.37)), e(library) <= ACC_FACTOR * max(e(oracle, this input), e(oracle, uniform)), both metrics
  P5      out(NONE, 123.0) and out(DEFAULT, NaN) byte-identical to out(NONE, 0) and out(DEFAULT, 0): `scale` is read under NORM_SCALE only"""
import ctypes

import numpy as np

import accuracy as acc
import devmem
import parity_suite as ps
from helpers import cdt_of
from ndrustfft_amd import _lib, api
from oracle import oracle_ctypes as orc

LD = acc.LD
P2_SCALE, P4_SCALE = 2.0 ** -3, 0.37
MODES = {"none": (_lib.NORM_NONE, 0.0), "default": (_lib.NORM_DEFAULT, 0.0), "pow2": (_lib.NORM_SCALE, P2_SCALE), "p4": (_lib.NORM_SCALE, P4_SCALE),
         "none_junk": (_lib.NORM_NONE, 123.0), "default_nan": (_lib.NORM_DEFAULT, float("nan"))}
FORWARD = ("ndfft", "ndfft_r2c")
P4_MAX_POINTS = 1 << 18        # the MI355X run measures P4 on cases of at most this many points (the long-double truth is host work)
# MI355X: (route, op, dtype) whose cases in parity_suite.ACC_GPU_FAMILIES all exceed P4_MAX_POINTS get a small case here
GPU_EXTRA = [({}, "ndifft", (2, 32768), 1, np.float32, "C", "four_step"),                 # (the family's f32 four-step lane has 2^22 points)
             ({}, "ndifft_r2c", (8192, 21), 0, np.float64, "C", "col_split")]              # (the family's f64 C2R column four-step is 8192 x 48)


def case_id(case):
    env, name, shape, axis, rdt, layout, want = case
    route = "+".join(want) if isinstance(want, tuple) else str(want)
    return "-".join([route, name, "x".join(map(str, shape)), f"ax{axis}", np.dtype(rdt).name, layout] + [f"{k}={v}" for k, v in env.items()])


def with_inverse_twins(table):
    """[(case, twin_of)]: every row, and behind every ndfft row its ndifft twin (same switches, shape, axis, dtype, layout; twin_of = the forward row).  The
    tables run most C2C routes forward only, and a forward C2C never looks at the scale."""
    out = []
    for row in table:
        out.append((row, None))
        if row[1] == "ndfft":
            out.append(((row[0], "ndifft") + tuple(row[2:]), row))
    return out


class Resident:
    """One input resident on the device and an output allocation that is refilled with the sentinel before every call."""
    def __init__(self, L, h, name, x, shape, axis, rdt, layout):
        self.L, self.h, self.name, self.axis, self.layout = L, h, name, axis, layout
        self.xa, self.xv = devmem.in_alloc(x, layout)
        self.ya, self.yv = devmem.out_alloc(name, shape, axis, rdt, layout=layout)
        self.din, self.dout = devmem.DevBuf(L, self.xa), devmem.DevBuf(L, self.ya)

    def set_input(self, x):
        xa, _ = devmem.in_alloc(x, self.layout)
        assert xa.shape == self.xa.shape and xa.dtype == self.xa.dtype
        self.din.upload(xa)

    def call(self, norm, scale, name=None):
        """(image of the output allocation, last path) of one ndfft_exec_device call on the null stream."""
        L, xv, yv = self.L, self.xv, self.yv
        self.dout.upload(self.ya)
        L.check(L.c.ndfft_exec_device(self.h._plan, devmem.OPC[name or self.name], self.din.p, self.dout.p, xv.ndim, api._i64(xv.shape),
                                      api._i64(devmem.strides_of(xv)), api._i64(yv.shape), api._i64(devmem.strides_of(yv)), self.axis, norm, scale, None))
        path = L.last_path()
        L.check(L.c.ndfft_dev_sync(None))
        return self.dout.download(self.ya), path

    def logical(self, img):
        """The output array of an image of the output allocation."""
        return img.T if self.layout == "F" else img

    def free(self):
        self.din.free(); self.dout.free()


def _parts(a):
    """The real and imaginary parts of a as one real array: a product of them by a real scalar is one rounding per part."""
    a = np.ascontiguousarray(a)
    return a.view(a.real.dtype)


def exactly_scaled(got, base, factor, what):
    """[] if got == base * T(factor) element for element and both are finite, else the failure text."""
    g, b = _parts(got), _parts(base)
    if not (np.isfinite(g).all() and np.isfinite(b).all()):
        return [f"{what}: {np.count_nonzero(~np.isfinite(g))} + {np.count_nonzero(~np.isfinite(b))} non-finite elements"]
    want = b * b.dtype.type(factor)
    if np.array_equal(g, want):
        return []
    diff = np.nonzero((g != want).reshape(-1))[0]
    rel = np.abs((g.reshape(-1)[diff] - want.reshape(-1)[diff]) / np.where(want.reshape(-1)[diff] != 0, want.reshape(-1)[diff], 1)).max()
    return [f"{what}: {diff.size} of {g.size} real parts differ, flat indices {diff[0]} .. {diff[-1]}, largest relative difference {rel:.3e}"]


def same_bytes(got, base, what):
    if got.tobytes() == base.tobytes():
        return []
    diff = np.nonzero((_parts(got).view(np.uint8) != _parts(base).view(np.uint8)).reshape(-1))[0] // got.real.dtype.itemsize
    return [f"{what}: {np.unique(diff).size} of {_parts(got).size} real parts differ, flat indices {diff[0]} .. {diff[-1]}"]


def default_factor(name, n):
    """The Default scaling of a scaling op (src/lib.rs: 1 / n for the inverses, 2 for the DCTs), in long double."""
    return LD(2) if name in acc.DCT_TYPE else LD(1) / LD(n)


def p2_p3_p5(name, n, outs, what):
    """The exact properties on the outputs of one input: outs = {mode: image}, of which "none" and "pow2" are required."""
    bad = []
    if name in FORWARD:                                                                       # P1 (covers P5)
        for m, o in outs.items():
            bad += same_bytes(o, outs["none"], f"P1 {what}: ({m}) against (none)")
        return bad
    bad += exactly_scaled(outs["pow2"], outs["none"], P2_SCALE, f"P2 {what}: (SCALE, 2^-3) against (NONE) * 2^-3")
    if "default" in outs:
        if name in acc.DCT_TYPE:
            bad += exactly_scaled(outs["default"], outs["none"], 2.0, f"P3 {what}: (DEFAULT) against 2 * (NONE)")
        elif n & (n - 1) == 0:
            bad += exactly_scaled(outs["default"], outs["none"], 1.0 / n, f"P3 {what}: (DEFAULT) against (NONE) / n")
    for m, ref in (("none_junk", "none"), ("default_nan", "default")):
        if m in outs:
            bad += same_bytes(outs[m], outs[ref], f"P5 {what}: ({m}) against ({ref})")
    return bad


def _times_p4(lane):
    lane *= lane.real.dtype.type(P4_SCALE)


def p4_errors(name, x, n, axis, rdt, got, sout, odt):
    """(e(library), e(oracle)) of out(SCALE, 0.37) on the input x: both against accuracy.truth() rescaled in long double, the oracle under Custom(lane *=
    T(0.37)) -- the reference's own application point, one extra rounding per element like the library's."""
    T = np.dtype(rdt).type
    t = acc.prepare(acc.truth(name, x, n, axis) * (LD(T(P4_SCALE)) / default_factor(name, n)), axis)
    o = getattr(orc, ps.OPS[name][2])(n, rdt).normalization(orc.NORM_CUSTOM, _times_p4)
    yo = np.zeros(sout, odt); ps.OPS[name][1](np.ascontiguousarray(x), yo, o, axis)
    return acc.errors(got, t, axis, rdt), acc.errors(yo, t, axis, rdt)


def check_case(L, case, p4=(), twin_of=None, verbose=False, tag=""):
    """One case (a ROUTE_TABLE row) through MODES.  p4: the inputs P4 is measured on, or a function (route taken) -> those inputs; "uniform" comes first where
    any is named (its oracle error is the second term of every bar).  The (SCALE, 0.37) call is made where P4 is measured, and on the forward ops (P1).
    twin_of: the forward row this ndifft case is the twin of -- one ndfft call on the same arrays must report the same route.  Every failure is collected
    into one message; the P4 figures are printed first (verbose).  Returns a record: route, op, dtype, shape, scaling (P2 ran), p4 [(input, lib, den, ratio)]."""
    env, name, shape, axis, rdt, layout, want = case
    n = shape[axis]
    sin, sout = ps.shapes_for(name, shape, axis)
    odt = np.dtype(cdt_of(rdt) if ps.OPS[name][4] else rdt)
    what = f"{name} {shape} axis={axis} {np.dtype(rdt).name} {layout} {env or ''}"
    bad, paths, rec_p4 = [], [], []
    with ps.switches(L, **env):
        h, _ = ps.handlers_for(name, n, rdt, L)
        x = acc.make_input("uniform", name, sin, axis, rdt, offset=n)
        dev = Resident(L, h, name, x, shape, axis, rdt, layout)
        try:
            def run(mode):
                img, path = dev.call(*MODES[mode]); paths.append(path)
                return img
            outs = {"none": run("none")}
            route = paths[0]
            kinds = tuple(p4(route) if callable(p4) else p4) if name not in FORWARD else ()
            assert not kinds or kinds[0] == "uniform", kinds
            for m in MODES:
                if m != "none" and (m != "p4" or kinds or name in FORWARD):
                    outs[m] = run(m)
            bad += p2_p3_p5(name, n, outs, f"uniform {what} [{route}]")
            if twin_of is not None:
                assert name == "ndifft" and twin_of[1] == "ndfft" and tuple(twin_of[2:6]) == tuple(case[2:6])
                fwd = dev.call(*MODES["none"], name="ndfft")[1]
                if fwd != route or not ps._route_ok(fwd, twin_of[6]):
                    bad.append(f"route {what}: the inverse twin took {route}, the forward row {fwd} (the table names {twin_of[6]})")
            if name not in FORWARD:
                uni = None
                for kind in ("uniform", "impulse") + tuple(k for k in kinds if k not in ("uniform", "impulse")):
                    if kind != "uniform":
                        x = acc.make_input(kind, name, sin, axis, rdt, offset=n)
                        dev.set_input(x)
                        outs = {}
                        if kind == "impulse":
                            outs = {"none": run("none"), "pow2": run("pow2")}
                            bad += p2_p3_p5(name, n, outs, f"impulse {what} [{route}]")
                        if kind in kinds:
                            outs["p4"] = run("p4")
                    if kind in kinds:
                        lib, orac = p4_errors(name, x, n, axis, rdt, dev.logical(outs["p4"]), sout, odt)
                        uni = orac if kind == "uniform" else uni
                        den = tuple(max(a, b) for a, b in zip(orac, uni))
                        ratio = tuple((l / d if d > 0 else (0.0 if l == 0 else float("inf"))) if l == l else float("nan") for l, d in zip(lib, den))
                        rec_p4.append((kind, lib, den, ratio))
                        line = (f"P4 {tag} {route} {name} {'x'.join(map(str, shape))} axis={axis} {np.dtype(rdt).name} {kind} {env or ''}: e_l2 {lib[0]:.3f} eps (oracle "
                                f"{den[0]:.3f}, ratio {ratio[0]:.2f}), e_bin {lib[1]:.3f} eps (oracle {den[1]:.3f}, ratio {ratio[1]:.2f})")
                        if verbose:
                            print(line, flush=True)
                        if not all(l <= ps.ACC_FACTOR * d for l, d in zip(lib, den)):      # (nan fails)
                            bad.append("beyond the bar: " + line)
        finally:
            dev.free()
    if len(set(paths)) != 1:
        bad.append(f"route {what}: the route moved with the normalisation: {paths}")
    if not ps._route_ok(paths[0], want):
        bad.append(f"route {what}: {paths[0]} instead of {want}")
    assert not bad, "\n".join([f"{len(bad)} normalisation failures"] + bad)
    return {"route": paths[0], "op": name, "dtype": np.dtype(rdt).name, "shape": tuple(shape), "scaling": name not in FORWARD, "p4": rec_p4}


def gpu_cases(L, cases, verbose=True, tag=""):
    """The MI355X form: the exact properties on every case, P4 (uniform input) on the first case, in the order given, of each (route taken, op, dtype) that
    has at most P4_MAX_POINTS points.  Returns the records."""
    first, records = set(), []
    for case in cases:
        key = lambda route: (route, case[1], np.dtype(case[4]).name)
        small = int(np.prod(case[2])) <= P4_MAX_POINTS
        r = check_case(L, case, p4=lambda route: ("uniform",) if small and key(route) not in first else (), verbose=verbose, tag=tag)
        if r["p4"]:
            first.add(key(r["route"]))
        records.append(r)
    return records


def coverage(records, required=None):
    """What the records leave open: required routes that never ran P2 with a scaling op, and (route, op, dtype) that ran P2 but never P4."""
    scaling = [r for r in records if r["scaling"]]
    missing = sorted((required if required is not None else ps.ACC_REQUIRED_ROUTES) - {r["route"] for r in scaling})
    with_p4 = {(r["route"], r["op"], r["dtype"]) for r in scaling if r["p4"]}
    no_p4 = sorted({(r["route"], r["op"], r["dtype"]) for r in scaling} - with_p4)
    return missing, no_p4


# ---- the other entry points: P2 and P5 on the uniform input, against the same call under NORM_NONE ----------------------------------------------------
# ndfft_exec on host arrays, one case per strategy of docs/host_path.md: (strategy, switches, op, shape, axis, real dtype)
HOST_CASES = [("host_small", {}, "ndifft", (64, 128), 1, np.float64),
              ("host_plain", {}, "nddct2", (200, 2048), 1, np.float64),
              ("host_bounce", {"NDFFT_HOST_PIPE": "1"}, "ndifft", (520, 1024), 1, np.float64),      # a chunk that lost the scale shows as a block of rows
              ("host_bounce", {"NDFFT_HOST_PIPE": "1"}, "ndifft_r2c", (520, 2048), 1, np.float32)]
HOST_PINNED_CASE = ("host_pinned", {}, "ndifft", (520, 1024), 1, np.float64)                        # arrays from api.pinned_empty (MI355X)


def _copy_counts(L, reset=False):
    """The CPU build counts its host <-> device copies: (hipMemcpy H2D, D2H, hipMemcpyAsync H2D, D2H, hipMemcpyAsync on a registered range); None elsewhere."""
    if not hasattr(L.c, "emul_copy_counts"):
        return None
    c = (ctypes.c_longlong * 5)(); L.c.emul_copy_counts(c, 1 if reset else 0)
    return tuple(c)


def host_case(L, case, pinned=False):
    """ndfft_exec on host arrays under (NONE, 0), (SCALE, 2^-3), (NONE, 123.0), (DEFAULT, 0), (DEFAULT, NaN): P2, P3 and P5.  On the CPU build the copies of
    the second call tell which strategy ran."""
    strategy, env, name, shape, axis, rdt = case
    n = shape[axis]
    sin, sout = ps.shapes_for(name, shape, axis)
    odt = np.dtype(cdt_of(rdt) if ps.OPS[name][4] else rdt)
    empty = (lambda s, dt: api.pinned_empty(s, dt, _library=L)) if pinned else np.empty
    src = acc.make_input("uniform", name, sin, axis, rdt, offset=n)
    x = empty(sin, src.dtype); x[...] = src
    what = f"ndfft_exec {strategy} {name} {shape} {np.dtype(rdt).name}"
    outs, paths, counts = {}, [], None
    with ps.switches(L, **env):
        h, _ = ps.handlers_for(name, n, rdt, L)
        for m in ("none", "pow2", "none_junk", "default", "default_nan"):
            y = empty(sout, odt); y[...] = devmem.SENTINEL
            _copy_counts(L, reset=True)
            L.check(L.c.ndfft_exec(h._plan, devmem.OPC[name], ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data), x.ndim, api._i64(x.shape),
                                   api._i64(devmem.strides_of(x)), api._i64(y.shape), api._i64(devmem.strides_of(y)), axis, *MODES[m]))
            if m == "pow2":
                counts = _copy_counts(L)
            paths.append(L.last_path()); outs[m] = np.array(y)
    bad = p2_p3_p5(name, n, outs, what)
    if len(set(paths)) != 1:
        bad.append(f"route {what}: the route moved with the normalisation: {paths}")
    if counts is not None:                       # (tests/test_emul_parity.py: HOST_ROUTE_TABLE pins the exact counts per strategy)
        ok = {"host_small": counts == (0, 0, 0, 0, 0), "host_plain": counts == (1, 1, 0, 0, 0),
              "host_bounce": counts[:2] == (0, 0) and counts[2] > 1 and counts[3] > 1 and counts[4] == 0}.get(strategy, True)
        if not ok:
            bad.append(f"{what}: the copies {counts} are not those of {strategy}")
    assert not bad, "\n".join(bad)


SHARDED_CASES = [("ndifft", (12, 7, 3), 0, np.float64), ("nddct1", (3, 9, 5), 1, np.float32), ("ndifft_r2c", (7, 3, 10), 2, np.float64)]


def sharded_case(L, case, ids, root):
    """ndfft_exec_sharded (host arrays) and ndfft_exec_sharded_device (arrays resident on `root`) over the devices `ids`: each output is byte-identical to the
    single-device output of the same mode, for (SCALE, 2^-3), (NONE, 123.0) and (DEFAULT, NaN); and the single-device outputs satisfy P2, P3 and P5."""
    name, shape, axis, rdt = case
    n = shape[axis]
    sin, sout = ps.shapes_for(name, shape, axis)
    x = acc.make_input("uniform", name, sin, axis, rdt, offset=n)
    ya, _ = devmem.out_alloc(name, shape, axis, rdt)
    h, _ = ps.handlers_for(name, n, rdt, L)
    what = f"{name} {shape} axis={axis} {np.dtype(rdt).name} devices {ids}"
    single = {}
    for m in ("none", "pow2", "none_junk", "default", "default_nan"):
        single[m] = devmem.dev_call(L, h, name, x, x, ya, ya, axis, weighted=False, norm=MODES[m][0], scale=MODES[m][1])[0]
    bad = p2_p3_p5(name, n, single, f"single device {what}")
    cids = (ctypes.c_int * len(ids))(*ids)
    geom = (x.ndim, api._i64(x.shape), api._i64(devmem.strides_of(x)), api._i64(ya.shape), api._i64(devmem.strides_of(ya)), axis)
    for m in ("pow2", "none_junk", "default_nan"):
        y = np.array(ya)
        L.check(L.c.ndfft_exec_sharded(h._plan, devmem.OPC[name], ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data), *geom, *MODES[m], len(ids), cids))
        if not L.last_path().startswith("sharded:"):
            bad.append(f"ndfft_exec_sharded {what}: path {L.last_path()}")
        bad += same_bytes(y, single[m], f"ndfft_exec_sharded {what}: ({m}) against the single-device call")
        try:
            assert L.c.ndfft_set_device(root) == 0
            din, dout = devmem.DevBuf(L, x), devmem.DevBuf(L, ya)
            try:
                L.check(L.c.ndfft_exec_sharded_device(h._plan, devmem.OPC[name], din.p, dout.p, *geom, *MODES[m], len(ids), cids, None))
                if not L.last_path().startswith("sharded:"):
                    bad.append(f"ndfft_exec_sharded_device {what}: path {L.last_path()}")
                L.check(L.c.ndfft_dev_sync(None))
                bad += same_bytes(dout.download(ya), single[m], f"ndfft_exec_sharded_device {what}: ({m}) against the single-device call")
            finally:
                din.free(); dout.free()
        finally:
            L.c.ndfft_set_device(0)
    assert not bad, "\n".join(bad)
