"""The stream contract on the MI355X (tests/stream_suite.py, docs/streams.md): every kernel route captured into a HIP graph on a side stream after one warm-up
call and replayed on new data, and the multi-pass and composed routes ordered on a side stream and alternating on two streams of one host thread.  The calls
go through ctypes with the stream's own handle, so ndfft_exec_device and its siblings are under test, not api.py.  tests/test_stream_emul.py is the
deterministic half (the CPU build's call log)."""
import ctypes

import numpy as np
import pytest

import accuracy as acc
import devmem
import parity_suite as ps
import stream_suite as ss
from helpers import TOL, assert_close
from ndrustfft_amd import _lib, api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    lib = _lib.default()                      # in-tree gfx950 build; raises if missing
    assert lib.c.ndfft_device_count() >= 1, "no MI355X visible"
    return lib


def _image(a, v, of=None):
    """(flat device tensor holding the allocation a, bit for bit; the view v of it as a strided tensor).  of: the host allocation v is a view of, where a is
    a copy of that one."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to("cuda:0")
    tv = torch.as_strided(t, v.shape, [s // v.itemsize for s in v.strides], devmem._off(v, a if of is None else of) // a.itemsize)
    return t, tv


def _bits(t):
    """The tensor's elements as integers: NaN patterns and signed zeros compare as what they are."""
    import torch
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same_bits(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


class CaptureFailed(AssertionError):
    pass


def captured_replays(L, call, xt, xtv, yt, ytv, x, decoy, what):
    """The protocol of docs/streams.md on one call, `call(stream handle) -> status`, whose input view xtv (of the allocation xt) holds x and whose output
    allocation yt holds its sentinel pattern.  On a fresh side stream: warm-up and synchronise; refill the output, put `decoy` into the input view and pin the
    load policy; capture one call; the output allocation must still hold its pattern bit for bit (nothing ran eagerly); put x back and replay.  Returns
    (output allocation, input allocation, route) after that replay -- and, in `extra`, what two further replays found: one after an eager call on the same
    stream (bit-identical to it), one on 2 x (bit-identical to twice the first output: every op is linear and a power-of-two scale is exact).  A call that
    fails under capture raises CaptureFailed once the capture has ended."""
    import torch
    extra = []
    s = torch.cuda.Stream()
    hs = s.cuda_stream
    assert hs, "a side stream, not the null stream"
    pattern = yt.clone()
    xd, dd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(decoy)).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        L.check(call(hs)); route = L.last_path()                        # 1. warm-up
        s.synchronize()
        yt.copy_(pattern); xtv.copy_(dd)                                # 2. sentinel everywhere, a decoy in the input
        L.check(L.c.ndfft_set_input_hint(_lib.INPUT_CACHED))
        try:
            g = torch.cuda.CUDAGraph()
            st, msg, err = _lib.OK, "", None
            try:
                with torch.cuda.graph(g, stream=s):                     # 3. one call under capture
                    st = call(hs)
                    msg = L.c.ndfft_last_error().decode()
                    route_captured = L.last_path() if st == _lib.OK else None
            except RuntimeError as e:
                err = e
            if st != _lib.OK or err is not None:
                raise CaptureFailed(f"{what} [{route}]: the call under capture returned status {st} ({msg}); ending the capture: {err}")
            torch.cuda.synchronize()
            if route_captured != route:
                extra.append(f"{what}: route {route_captured} under capture, {route} before")
            if not _same_bits(yt, pattern):                             # 4. nothing ran eagerly
                extra.append(f"{what} [{route}]: the output allocation changed during capture: part of the call is not in the graph")
            xtv.copy_(xd)                                               # 5. the real input, replay
            g.replay(); torch.cuda.synchronize()
            out, inp = yt.cpu().numpy(), xt.cpu().numpy()
            first = ytv.clone()
            # ... a replay after an eager call of the same shape on s: the eager call leaves the graph's scratch and tables as they were
            yt.copy_(pattern)
            L.check(call(hs)); torch.cuda.synchronize()
            eager = yt.clone()
            yt.copy_(pattern)
            g.replay(); torch.cuda.synchronize()
            if not _same_bits(yt, eager):
                extra.append(f"{what} [{route}]: the replay after an eager call differs from the eager call")
            # ... a replay on 2 x
            xtv.mul_(2); yt.copy_(pattern)
            g.replay(); torch.cuda.synchronize()
            twice = (torch.view_as_real(first) if first.is_complex() else first) * 2      # (part by part: a complex product by 2 + 0i turns an imaginary -0 into +0)
            if not torch.equal(_bits(ytv), _bits(twice)):
                extra.append(f"{what} [{route}]: the replay on 2 x is not 2 x the first replay, bit for bit")
            del g
        finally:
            L.check(L.c.ndfft_set_input_hint(_lib.INPUT_AUTO))
    torch.cuda.current_stream().wait_stream(s)
    return out, inp, route, extra


# ---- 2. every route captured on a side stream and replayed on new data ---------------------------------------------------------------------------------
def graph_cases(family, dt):
    """The first case of each (route, dtype, real / complex input) of a family, in table order: the rule of parity_suite.GUARD_SPARSE."""
    first, out = set(), []
    for c in ps.acc_gpu_cases(family, dt):
        key = (c[6], np.dtype(c[4]), ps.OPS[c[1]][3])
        if key not in first:
            first.add(key); out.append(c)
    return out


_GRAPH_SEEN = {}      # (family, dt) -> routes its G1 calls took


def _graph_family(L, family, dt, geometry, verbose=True):
    extra = []

    def runner(name, h, xa, xv, ya, yv, axis):
        (xt, xtv), (yt, ytv) = _image(xa, xv), _image(ya, yv)
        x = np.ascontiguousarray(xv)
        decoy = acc.make_input("uniform", name, xv.shape, axis, xv.real.dtype, offset=xv.shape[axis] + 7919)
        assert decoy.dtype == x.dtype and not np.array_equal(decoy, x)

        def call(hs):
            return L.c.ndfft_exec_device(h._plan, devmem.OPC[name], ctypes.c_void_p(xtv.data_ptr()), ctypes.c_void_p(ytv.data_ptr()), xv.ndim, api._i64(xv.shape),
                                         api._i64(devmem.strides_of(xv)), api._i64(yv.shape), api._i64(devmem.strides_of(yv)), axis, _lib.NORM_DEFAULT, 0.0,
                                         ctypes.c_void_p(hs))
        out, inp, route, more = captured_replays(L, call, xt, xtv, yt, ytv, x, decoy, f"{name} {xv.shape} axis={axis} {xv.dtype.name}")
        extra.extend(more)
        return out.reshape(ya.shape), inp.reshape(xa.shape), route
    seen, _ = ps.guarded_views(L, graph_cases(family, dt), geometries=(geometry,), verbose=verbose, runner=runner)
    assert not extra, "\n".join([f"{len(extra)} failures of the replays"] + extra)
    return seen


@pytest.mark.parametrize("geometry", ["G1", "G2"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("family", list(ps.ACC_GPU_FAMILIES))
def test_every_route_in_a_captured_graph(L, family, dt, geometry):
    """The first case of each (route, dtype, real / complex input) of the family, dense (G1) or with padded rows (G2), through captured_replays; then
    parity_suite.guarded_views's own checks on what the replay left: the guard bands untouched, the input byte-identical, the view finite and within helpers.TOL
    of the oracle, in G1 the route the case names.  The two further replays of each case run before the runner returns -- the graph lives there -- and their
    findings are asserted after the guarded checks."""
    seen = _graph_family(L, family, dt, geometry)
    if geometry == "G1":
        _GRAPH_SEEN[family, dt] = seen


NO_FUSE = ss.no_fuse_filter_cases()


def _spec_tensors(sp, x=None):
    import torch
    xa = sp.xa
    if x is not None:
        xa = np.array(sp.xa); np.lib.stride_tricks.as_strided(xa.reshape(-1)[devmem._off(sp.xv, sp.xa) // xa.itemsize:], sp.xv.shape, sp.xv.strides)[...] = x
    (xt, xtv), (yt, ytv) = _image(xa, sp.xv, of=sp.xa), _image(sp.ya, sp.yv)
    wt = torch.from_numpy(sp.w).to("cuda:0") if sp.w is not None else None
    return xt, xtv, yt, ytv, wt


@pytest.mark.parametrize("case", NO_FUSE, ids=[ss.case_id(c) for c in NO_FUSE])
def test_composed_filter_in_a_captured_graph(L, case):
    """ndfft_filter with NDFFT_FILTER_NO_FUSE on a C2C plan and on an R2C plan -- forward route, weight pass on the spectrum image, inverse route -- through the
    same protocol; the replay against the composed oracle at helpers.TOL."""
    sp = ss.make_spec(L, case)
    xt, xtv, yt, ytv, wt = _spec_tensors(sp)
    call = lambda hs: sp.invoke(xt.data_ptr(), yt.data_ptr(), wt.data_ptr(), hs)
    out, inp, route, extra = captured_replays(L, call, xt, xtv, yt, ytv, np.ascontiguousarray(sp.xv), sp.input_with(4242), sp.label)
    assert sp.route_ok(route), route
    assert inp.tobytes() == np.ascontiguousarray(sp.xa).tobytes(), "the input allocation was written"
    assert_close(ss.view_of(sp, out), sp.expect, sp.axis, TOL[sp.rdt], f"{sp.label} [{route}] replayed")
    assert not extra, "\n".join(extra)


def test_captured_graphs_ran_every_required_route(L):
    """The dense (G1) captures of the families together ran every kernel route (a family that has not run in this session runs here)."""
    for family in ps.ACC_GPU_FAMILIES:
        for dt in ("f64", "f32"):
            if (family, dt) not in _GRAPH_SEEN:
                _GRAPH_SEEN[family, dt] = _graph_family(L, family, dt, "G1", verbose=False)
    seen = set().union(*_GRAPH_SEEN.values())
    assert ps.ACC_REQUIRED_ROUTES <= seen, sorted(ps.ACC_REQUIRED_ROUTES - seen)


# ---- 3. side-stream order and two streams from one thread: the multi-pass and composed routes ------------------------------------------------------------
MULTI = ss.multi_pass_exec_cases() + ss.weighted_cases(dtypes=(np.float64, np.float32)) + ss.composed_filter_cases()
MULTI_IDS = [ss.case_id(c) for c in MULTI]


class _Hint:
    def __init__(self, L): self.L = L
    def __enter__(self): self.L.check(self.L.c.ndfft_set_input_hint(_lib.INPUT_CACHED))
    def __exit__(self, *exc): self.L.check(self.L.c.ndfft_set_input_hint(_lib.INPUT_AUTO))


def _null_stream_result(L, sp, x=None, expect=True):
    """The call on the null stream after a full synchronise: (output allocation as a device tensor, route); against the oracle at helpers.TOL."""
    import torch
    xt, xtv, yt, ytv, wt = _spec_tensors(sp, x)
    torch.cuda.synchronize()
    L.check(sp.invoke(xt.data_ptr(), yt.data_ptr(), wt.data_ptr() if wt is not None else 0, 0))
    route = L.last_path()
    torch.cuda.synchronize()
    assert sp.route_ok(route), f"{sp.label}: route {route}"
    if expect:
        assert_close(ss.view_of(sp, yt.cpu().numpy()), sp.expect, sp.axis, TOL[sp.rdt], f"{sp.label} [{route}] on the null stream")
    return yt, route


@pytest.mark.parametrize("case", MULTI, ids=MULTI_IDS)
def test_call_is_ordered_on_a_side_stream(L, case):
    """On a non-default stream, with no host synchronisation in between: a device copy that produces the input, the call, a device copy that consumes the
    output -- while the default stream fills an unrelated 256 MiB tensor.  Bit-identical to the same call on the null stream after a full synchronise.  A
    launch that dropped its stream argument would run beside the copies instead of between them."""
    import torch
    with ps.switches(L, **ss.case_env(case)), _Hint(L):
        sp = ss.make_spec(L, case)
        ref, route = _null_stream_result(L, sp)
        xt, xtv, yt, ytv, wt = _spec_tensors(sp)
        src = xtv.clone(); pattern = yt.clone(); res = torch.zeros_like(yt)
        dw = wt.data_ptr() if wt is not None else 0
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            L.check(sp.invoke(xt.data_ptr(), yt.data_ptr(), dw, s.cuda_stream))        # warm-up: this stream's scratch
        torch.cuda.synchronize()
        xtv.zero_(); yt.copy_(pattern)
        other = torch.empty(256 << 20, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        other.fill_(1)                                                                 # the default stream is busy ...
        with torch.cuda.stream(s):
            xtv.copy_(src)
            st = sp.invoke(xt.data_ptr(), yt.data_ptr(), dw, s.cuda_stream)
            res.copy_(yt)
        other.fill_(2)
        L.check(st)
        assert L.last_path() == route
        torch.cuda.synchronize()
        assert _same_bits(res, ref), f"{sp.label} [{route}]: the result on a side stream differs from the null-stream result"
        assert int(other[0]) == 2 and int(other[-1]) == 2


@pytest.mark.parametrize("case", MULTI, ids=MULTI_IDS)
def test_two_streams_from_one_thread(L, case):
    """One host thread and one plan make alternating calls on two streams with distinct inputs, four rounds, synchronising only at the end; both outputs are
    bit-identical to their null-stream results.  For a scratch slot shared between the streams this test is probabilistic (the two calls must overlap on the
    device to collide); step 4 of stream_suite.warm_call_contract is the deterministic check of the same property on the CPU build."""
    import torch
    with ps.switches(L, **ss.case_env(case)), _Hint(L):
        sp = ss.make_spec(L, case)
        xs = [np.ascontiguousarray(sp.xv), np.ascontiguousarray(sp.input_with(977))]
        assert not np.array_equal(xs[0], xs[1])
        refs = [_null_stream_result(L, sp, x, expect=(k == 0))[0] for k, x in enumerate(xs)]
        assert not _same_bits(refs[0], refs[1])
        bufs = [_spec_tensors(sp, x) for x in xs]
        pattern = bufs[0][2].clone()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        assert streams[0].cuda_stream != streams[1].cuda_stream
        torch.cuda.synchronize()
        for rnd in range(5):                                                           # round 0 warms both streams up
            for (xt, xtv, yt, ytv, wt), s in zip(bufs, streams):
                L.check(sp.invoke(xt.data_ptr(), yt.data_ptr(), wt.data_ptr() if wt is not None else 0, s.cuda_stream))
            if rnd == 0:
                torch.cuda.synchronize()
                for b in bufs:
                    b[2].copy_(pattern)                                                # (the warm-up's results are gone: the four rounds must produce them)
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        for k in range(2):
            assert _same_bits(bufs[k][2], refs[k]), f"{sp.label}: stream {k + 1}'s output differs from its null-stream result"
