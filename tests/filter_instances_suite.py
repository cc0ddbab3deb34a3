"""Every compiled instance of the three fused filter kernels (filter_kernel.h: filter_pow2, filter_r2c_pow2, filter_dct_pow2).  kernels_filter.hip picks one template
instantiation per call from the plan kind, the length, the dtype, the access width VEC (from base alignment and pitch) and the load policy NT (from the input hint, the
residency model or NDFFT_STREAM_LOADS).  The three suites this one is built on (filter_suite, filter_real_suite, filter_dct_suite) run the wide, plain-load instance of
every length and the narrow one at two lengths; here every (kind, length, dtype, VEC, NT) that ships is launched, named by its geometry and by ndfft_last_input_policy().

Expected values: the composed CPU oracle within helpers.TOL with the sentinel and input checks of the suites' filter_case, and the working-precision bar of
docs/accuracy.md.  Instances of different VEC or NT are separate compilations: nothing here asks them to agree bit for bit (census() reports whether they did).
The functions take the library L, so the same cases run on the CPU build of the kernel sources (tests/test_filter_instances_emul.py) and on the MI355X
(tests/test_filter_instances_gpu.py)."""
import ctypes
import json
import threading

import numpy as np

import accuracy as acc
import filter_dct_suite as fds
import filter_real_suite as frs
import filter_suite as fs
import parity_suite as ps
from devmem import SENTINEL, DevBuf, strides_of
from filter_suite import _pitched
from helpers import TOL, assert_close, cdt_of
from ndrustfft_amd import _lib, api
from weights_suite import make_weights

BOTH = fs.BOTH
AUTO, COLD = _lib.INPUT_AUTO, _lib.INPUT_COLD


class Kind:
    """One plan kind: its fused route, shipped lengths, element type, and the helpers of its suite under one set of names (the weights are `w` throughout)."""
    def __init__(self, key, fused, lengths, op, r2c=False, dct=False):
        self.key, self.fused, self.lengths, self.op, self.r2c, self.dct = key, fused, lengths, op, r2c, dct
        self.entry = "ndfft_exec_dct_filter_device" if dct else "ndfft_exec_filter_device"

    def __repr__(self):
        return self.key

    def elem(self, rdt):
        return np.dtype(rdt) if (self.r2c or self.dct) else np.dtype(cdt_of(rdt))

    def handler(self, L, n, rdt):
        return fds.handler(L, n, rdt) if self.dct else fs.handler(L, n, rdt, self.r2c)

    def make_x(self, shape, rdt, seed=1):
        return ps.make_input(self.op, shape, rdt, offset=seed)

    def weights(self, n, rdt, seed=1):
        return fds.make_g(n, rdt, seed) if self.dct else make_weights(fs.wname(self.r2c), n, rdt, seed)

    def oracle(self, x, w, n, axis, rdt):
        return fds.oracle_filter(x, w, n, axis, rdt) if self.dct else fs.oracle_filter(x, w, n, axis, rdt, self.r2c)

    def truth(self, x, w, n, axis):
        return fds.truth_filter(x, w, n, axis) if self.dct else fs.truth_filter(x, w, n, axis, self.r2c)

    def filt_call(self, L, h, xa, xv, ya, yv, axis, w, **kw):
        return fds.filt_call(L, h, xa, xv, ya, yv, axis, w, **kw) if self.dct else fs.filt_call(L, h, xa, xv, ya, yv, axis, w, **kw)

    def filter_case(self, L, shape, axis, rdt, *, w=None, **kw):
        if self.dct:
            return fds.filter_case(L, shape, axis, rdt, g=w, **kw)
        return fs.filter_case(L, shape, axis, rdt, r2c=self.r2c, w=w, **kw)

    def composed(self, path):
        return "+weights+" in path and self.fused not in path

    def narrow(self, rdt):
        """Base offsets, in elements of the array, at which a dense view is still fused but no longer 16-byte aligned: the narrowest instance the dtype has
        (f64 C2C and R2C have one width only; the offset geometry runs anyway).  C2C: one complex element, 8 bytes in f32.  R2C: two reals, a whole complex element
        as the fused route needs.  DCT: one real; f32 also two (8-byte aligned, still no 16-byte access)."""
        if self.dct:
            return (1,) if np.dtype(rdt) == np.float64 else (1, 2)
        return (2,) if self.r2c else (1,)

    def geometries(self, rdt):
        return (("aligned", 0),) + tuple((f"narrow{b}", b) for b in self.narrow(rdt))


C2C = Kind("c2c", fs.FUSED, fs.FUSED_N, "ndfft")
R2C = Kind("r2c", frs.FUSED_R, frs.FUSED_R_N, "ndfft_r2c", r2c=True)
DCT = Kind("dct", fds.FUSED_D, fds.FUSED_D_N, "nddct2", dct=True)
KINDS = (C2C, R2C, DCT)
CENSUS = [(K, n) for K in KINDS for n in K.lengths]
CENSUS_IDS = [f"{K.key}-{n}" for K, n in CENSUS]


def rows_for(n):
    """37 lanes leave a partial last workgroup for every LPB > 1; 5 at the long lengths keep a case to a few seconds."""
    return 37 if n < 4096 else 5


class hint:
    """ndfft_set_input_hint for the duration of a block (the hint is per host thread); INPUT_AUTO afterwards, whatever happened inside."""
    def __init__(self, L, value):
        self.L, self.value = L, value

    def __enter__(self):
        self.L.check(self.L.c.ndfft_set_input_hint(self.value))

    def __exit__(self, *exc):
        self.L.check(self.L.c.ndfft_set_input_hint(AUTO))


def policy_is(L, value, what):
    """ndfft_last_input_policy(): 0 = the plain-load instance (NT = 1) was launched, 1 = the streaming-load one (NT = 3)."""
    pol = L.c.ndfft_last_input_policy()
    assert pol == (1 if value == COLD else 0), f"load policy {pol} under hint {value}: {what}"


def settle_residency_model(L):
    """Under INPUT_AUTO the policy is the residency model's answer (exec_internal.h: MallModel), and the model remembers, by address, the last 32 buffers this thread's
    calls read or wrote: a new allocation that lands on one an earlier test left cold, or read 256 MiB of traffic ago, is streamed.  16 dense calls on 32 distinct
    512-byte ranges of one allocation replace every entry by a small recent one, so that what a case sees under INPUT_AUTO does not depend on the tests before it."""
    n = 64
    h = C2C.handler(L, n, np.float32)
    buf, dw = DevBuf(L, np.zeros(32 * n, np.complex64)), DevBuf(L, np.ones(n, np.complex64))
    try:
        for i in range(16):
            src, dst = (ctypes.c_void_p(buf.p.value + k * n * 8) for k in (2 * i, 2 * i + 1))
            L.check(L.c.ndfft_exec_filter_device(h._plan, src, dst, 1, api._i64((n,)), api._i64((1,)), api._i64((1,)), 0, dw.p, n, _lib.NORM_DEFAULT, 0.0, 0, None))
        L.check(L.c.ndfft_dev_sync(None))
    finally:
        buf.free(); dw.free()


class Bar:
    """The bar of docs/accuracy.md for one (kind, shape, dtype, weights): the three inputs, their truths one precision up and the composed oracle's own errors, computed
    once and shared by every geometry and policy.  filter_suite.within_bar on arrays the caller places: nothing measured from the library enters the bar."""
    def __init__(self, K, shape, axis, rdt, w):
        self.axis, self.rdt, self.x, self.t, self.den = axis, rdt, {}, {}, {}
        n = shape[axis]
        assert acc.INPUTS[0] == "uniform"
        uni = None
        for kind in acc.INPUTS:
            x = acc.make_input(kind, K.op, shape, axis, rdt, offset=n)
            t = acc.prepare(K.truth(x, w, n, axis), axis)
            orac = acc.errors(K.oracle(x, w, n, axis, rdt), t, axis, rdt)
            if kind == "uniform":
                uni = orac
            self.x[kind], self.t[kind], self.den[kind] = x, t, tuple(max(a, b) for a, b in zip(orac, uni))

    def measure(self, kind, got):
        """((e_l2, e_bin) of the library, the bar's oracle figures, within the bar)."""
        lib, den = acc.errors(got, self.t[kind], self.axis, self.rdt), self.den[kind]
        return lib, den, all(l <= ps.ACC_FACTOR * d for l, d in zip(lib, den))


# ---- 1. instance census ------------------------------------------------------------------------------------------------------------------------------------
def census(L, K, n, rdt, verbose=False):
    """Every (geometry, policy) pair of one (kind, n, dtype) on dense lanes (pitch n on both sides, so the hint is honoured), all three inputs of the bar.  Returns
    what was measured: the range of both metrics, the largest ratio to the bar's oracle figure, and how many instance pairs came out bit-identical."""
    rows, edt = rows_for(n), K.elem(rdt)
    shape = (rows, n)
    w = K.weights(n, rdt, seed=2)
    bar = Bar(K, shape, 1, rdt, w)
    settle_residency_model(L)
    bad, outs = [], {}
    stats = {"kind": K.key, "n": n, "dtype": np.dtype(rdt).name, "calls": 0, "e_l2": [np.inf, 0.0], "e_bin": [np.inf, 0.0], "ratio": 0.0}
    for gname, base in K.geometries(rdt):
        for value in (AUTO, COLD):
            with hint(L, value):
                for kind in acc.INPUTS:
                    xa, xv = _pitched(rows, n, n, base, edt, 0, bar.x[kind])
                    ya, yv = _pitched(rows, n, n, base, edt, SENTINEL)
                    what = f"{K.key} n={n} {np.dtype(rdt).name} {gname} hint={value} {kind}"
                    got, _ = K.filter_case(L, shape, 1, rdt, xa=xa, xv=xv, ya=ya, yv=yv, w=w, want_path=K.fused)
                    policy_is(L, value, what)
                    lib, den, ok = bar.measure(kind, got)
                    line = f"{what}: e_l2 {lib[0]:.3f} eps (bar's oracle {den[0]:.3f}), e_bin {lib[1]:.3f} eps (bar's oracle {den[1]:.3f})"
                    if verbose:
                        print(line, flush=True)
                    if not ok:
                        bad.append(line)
                    outs[gname, value, kind] = got.tobytes()
                    stats["calls"] += 1
                    for key, e, d in (("e_l2", lib[0], den[0]), ("e_bin", lib[1], den[1])):
                        stats[key] = [min(stats[key][0], e), max(stats[key][1], e)]
                        stats["ratio"] = max(stats["ratio"], e / d)
    assert not bad, "\n".join([f"{len(bad)} beyond {ps.ACC_FACTOR} x the oracle's own error"] + bad)
    # an observation, not a requirement: which pairs of separately compiled instances gave the same bits
    nt = [outs[g, AUTO, k] == outs[g, COLD, k] for g, _ in K.geometries(rdt) for k in acc.INPUTS]
    vec = [outs["aligned", v, k] == outs[g, v, k] for g, _ in K.geometries(rdt)[1:] for v in (AUTO, COLD) for k in acc.INPUTS]
    stats["nt_pairs_identical"], stats["vec_pairs_identical"] = [sum(nt), len(nt)], [sum(vec), len(vec)]
    if verbose:
        print("CENSUS " + json.dumps(stats), flush=True)
    return stats


def in_place_cold(L, K, rdt):
    """One in-place call per narrow geometry under INPUT_COLD, at n = 256 and at the kind's longest length: bit-identical to the out-of-place call of the same instance."""
    edt = K.elem(rdt)
    for n in (256, K.lengths[-1]):
        rows = rows_for(n)
        x = K.make_x((rows, n), rdt, seed=n + 5)
        for base in K.narrow(rdt):
            what = f"{K.key} n={n} {np.dtype(rdt).name} base offset {base}"
            with hint(L, COLD):
                xa, xv = _pitched(rows, n, n, base, edt, 0, x)
                ya, yv = _pitched(rows, n, n, base, edt, SENTINEL)
                a, _ = K.filter_case(L, (rows, n), 1, rdt, xa=xa, xv=xv, ya=ya, yv=yv, seed=n, want_path=K.fused)
                policy_is(L, COLD, what)
                xa, xv = _pitched(rows, n, n, base, edt, 0, x)
                b, _ = K.filter_case(L, (rows, n), 1, rdt, xa=xa, xv=xv, inplace=True, seed=n, want_path=K.fused)
                policy_is(L, COLD, what + " in place")
            assert a.tobytes() == b.tobytes(), "in place differs from out of place under INPUT_COLD: " + what


# ---- 2. forced streaming loads on pitched views -----------------------------------------------------------------------------------------------------------------
FORCED = {"c2c_f32_unaligned": fs.f32_unaligned, "c2c_guarded_output": fs.guarded_output, "r2c_alignment_and_pitch": frs.alignment_and_pitch,
          "r2c_sentinel_bands": frs.sentinel_bands, "dct_base_and_pitch": fds.base_and_pitch, "dct_sentinel_window": fds.sentinel_window}


def forced_streaming(L, which):
    """The suites' own geometry functions, unchanged, under NDFFT_STREAM_LOADS=1: stream_loads_for() is then true for calls that are not dense too, so every padded
    pitch and odd base they hold runs the streaming-load instances under their own guard-band checks.  The dense call in front shows that the switch is in force."""
    with ps.switches(L, NDFFT_STREAM_LOADS=1):
        C2C.filter_case(L, (5, 128), 1, np.float32, want_path=C2C.fused)
        policy_is(L, COLD, "NDFFT_STREAM_LOADS=1 on a dense call under INPUT_AUTO")
        FORCED[which](L)


def defaults_in_force(L):
    """What every case above leaves behind: INPUT_AUTO and no forced policy, so a small dense input the model has never seen is read with plain loads."""
    settle_residency_model(L)
    C2C.filter_case(L, (5, 128), 1, np.float32, want_path=C2C.fused, seed=9)
    policy_is(L, AUTO, "a small dense call after the cases that set a hint or NDFFT_STREAM_LOADS")


# ---- 3. call shapes with code of their own in compose.hip: filter_fused ------------------------------------------------------------------------------------------
def short_lengths(K):
    return (64, 128) if K is C2C else (128,)


def one_dimensional(L, K, rdt):
    """n points and no batch dim: the pitch falls back to the lane length (R2C: an expression of its own).  Aligned and at the narrow offsets, under both hints: fused,
    dense, so the hint is honoured.  R2C at an odd real offset on either side is no whole complex element: composed, and right."""
    edt = K.elem(rdt)

    def alloc(base, n, fill, x=None):
        a = np.full(base + n + 3, fill, edt)
        v = a[base:base + n]
        if x is not None:
            v[...] = x
        return a, v
    settle_residency_model(L)
    for n in short_lengths(K):
        x = K.make_x((n,), rdt, seed=n)
        for base in (0,) + K.narrow(rdt):
            for value in (AUTO, COLD):
                with hint(L, value):
                    xa, xv = alloc(base, n, 0, x)
                    ya, yv = alloc(base, n, SENTINEL)
                    K.filter_case(L, (n,), 0, rdt, xa=xa, xv=xv, ya=ya, yv=yv, seed=n, want_path=K.fused)
                    policy_is(L, value, f"1-D {K.key} n={n} {np.dtype(rdt).name} base offset {base}")
        if K is R2C:
            for bi, bo in ((1, 1), (1, 0), (0, 3)):
                xa, xv = alloc(bi, n, 0, x)
                ya, yv = alloc(bo, n, SENTINEL)
                _, path = K.filter_case(L, (n,), 0, rdt, xa=xa, xv=xv, ya=ya, yv=yv, seed=n)
                assert K.composed(path), (path, bi, bo)


def three_d_contiguous(L, K, rdt):
    """(3, 5, n) along axis 2, contiguous: the two batch dims merge into one, so the call is fused."""
    for n in short_lengths(K):
        K.filter_case(L, (3, 5, n), 2, rdt, seed=n, want_path=K.fused)


def three_d_window(L, K, rdt):
    """(3, 5, n) as a window of a (5, 7, n + 6) allocation on both sides: two batch dims that do not merge, so the call is composed; nothing outside the window changes
    (the offsets are even: for R2C the window alone, not a half element, is what keeps the call off the fused route)."""
    for n in short_lengths(K):
        big, win = (5, 7, n + 6), np.s_[1:4, 1:6, 4:4 + n]
        xa = np.zeros(big, K.elem(rdt))
        xv = xa[win]
        xv[...] = K.make_x((3, 5, n), rdt, seed=n + 1)
        _, path = K.filter_case(L, (3, 5, n), 2, rdt, xa=xa, xv=xv, out_view=(big, win), seed=n)
        assert K.composed(path), path


def six_d_stepped(L, K, rdt, n=128):
    """(2, 2, 2, 2, 2, n), stepped in every batch dim (the geometry of filter_suite.composed_c2c_layouts' last case at a fused length): five batch dims that do not merge,
    one more than kMaxBatchDims, so the peel of compose.hip (peeled) takes the slowest off on the host and every piece is composed.  filter_case: the skipped elements of the output keep the sentinel."""
    shape, big = (2, 2, 2, 2, 2, n), (4, 4, 4, 4, 4, n)
    xa = np.zeros(big, K.elem(rdt))
    xv = xa[::2, ::2, ::2, ::2, ::2]
    xv[...] = K.make_x(shape, rdt, seed=11)
    _, path = K.filter_case(L, shape, 5, rdt, xa=xa, xv=xv, out_view=(big, np.s_[1::2, ::2, 1::2, ::2, 1::2]), seed=n)
    assert K.composed(path), path


def zero_extent(L, K, rdt, n=128):
    """A batch dim of extent 0: there is no lane, prepare() reports `nothing` and the entry point returns NDFFT_OK before it looks at the array pointers or the weights
    (include/ndfft_mi355x_ext.h lists its checks in that order) -- so a NULL weights pointer is no error here, and nothing is written."""
    edt = K.elem(rdt)
    h = K.handler(L, n, rdt)
    for shape, alloc, cut in (((0, n), (2, n), np.s_[:0]), ((3, 0, n), (3, 1, n), np.s_[:, :0])):
        xa = K.make_x(alloc, rdt, seed=3)
        ya = np.full(alloc, SENTINEL, edt)
        xv, yv = xa[cut], ya[cut]
        assert xv.shape == shape and yv.shape == shape
        for w in (None, K.weights(n, rdt)):
            got, xin, _, st = K.filt_call(L, h, xa, xv, ya, yv, len(shape) - 1, w, check=False)
            assert st == _lib.OK, (st, shape, L.c.ndfft_last_error())
            assert np.all(got == SENTINEL), f"a call on no lane wrote its output allocation: {shape}"
            assert xin.tobytes() == xa.tobytes()


# ---- 4. the first filter call of a shared plan, from many host threads at once ---------------------------------------------------------------------------------------
RACES = ((C2C, 2048, np.float64), (R2C, 256, np.float64), (DCT, 256, np.float64), (C2C, 4096, np.float32), (R2C, 4096, np.float32), (DCT, 4096, np.float32))
RACE_IDS = [f"{K.key}-{n}-{np.dtype(rdt).name}" for K, n, rdt in RACES]
# (C2C 4096 in f32 has a palindromic radix list: its plan's own table serves both pass sets, so that case races the build that finds nothing to upload; every other
#  case uploads the table of the reversed list, R2C and DCT the forward one of the half length as well)


def first_call_race(L, K, n, rdt, nthreads=8, rounds=3):
    """The filter tables are built lazily under the plan's mutex by its first filter call (plan.hip: get_filter_twiddles, get_filter_r2c_tables).  Eight threads,
    released together, make that first call on one fresh plan, each on device buffers and an input of its own, twice; three fresh plans, so the build is raced three
    times.  Every result is the composed oracle's within helpers.TOL."""
    shape, tol = (16, n), TOL[np.dtype(rdt)]
    w = K.weights(n, rdt, seed=4)
    xs = [K.make_x(shape, rdt, seed=1000 * i + n) for i in range(nthreads)]
    yos = [K.oracle(x, w, n, 1, rdt) for x in xs]           # once, before any thread starts
    entry = getattr(L.c, K.entry)
    for rnd in range(rounds):
        h = K.handler(L, n, rdt)                            # no filter call has been made on this plan
        gate, errs = threading.Barrier(nthreads), []

        def work(i):
            bufs = []
            try:
                try:
                    x = xs[i]
                    dx, dw = DevBuf(L, x), DevBuf(L, w)
                    bufs += [dx, dw]
                    douts = [DevBuf(L, np.full(shape, SENTINEL, x.dtype)) for _ in range(2)]
                    bufs += douts
                except BaseException:
                    gate.abort()
                    raise
                gate.wait()
                for dy in douts:
                    L.check(entry(h._plan, dx.p, dy.p, 2, api._i64(shape), api._i64(strides_of(x)), api._i64(strides_of(x)), 1, dw.p, len(w),
                                  _lib.NORM_DEFAULT, 0.0, 0, None))
                    path = L.last_path()
                    assert path == K.fused, path
                L.check(L.c.ndfft_dev_sync(None))
                for rep, dy in enumerate(douts):
                    assert_close(dy.download(x), yos[i], 1, tol, f"{K.key} n={n} {np.dtype(rdt).name} round {rnd} thread {i} call {rep}")
            except Exception as e:
                errs.append(f"round {rnd} thread {i}: {e!r}")
            finally:
                for b in bufs:
                    b.free()

        ts = [threading.Thread(target=work, args=(i,)) for i in range(nthreads)]
        [t.start() for t in ts]; [t.join() for t in ts]
        assert not errs, errs
