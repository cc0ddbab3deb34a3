"""The stream contract on the CPU build of the kernel sources (tests/stream_suite.py, docs/streams.md): tests/emul ignores every hipStream_t, so a call may be
given any handle, and its runtime logs the handle of every launch, asynchronous copy, fill and event call of the thread, and counts its allocations and waits.
Every route the emulation reaches -- ROUTE_TABLE, ROUTE_TABLE_STEPPED, ACC_EXTRA, the weighted multi-pass calls and the composed filters -- must stay on the
caller's stream and, once warm, allocate and wait for nothing.  Deterministic; tests/test_stream_gpu.py speaks for the real runtime."""
import os
import subprocess

import pytest

import stream_suite as ss
from ndrustfft_amd import _lib
from test_emul_parity import ACC_EXTRA, EMUL_DIR, ROUTE_TABLE, ROUTE_TABLE_STEPPED

CASES = ([ss.exec_case(r) for r in ROUTE_TABLE + ACC_EXTRA] + [ss.stepped_case(r) for r in ROUTE_TABLE_STEPPED] + ss.weighted_cases() + ss.composed_filter_cases())


@pytest.fixture(scope="module")
def L():
    if os.environ.get("NDFFT_EMUL_LIB"):                    # a side build of the emulation (make -C tests/emul SAN=1: UBSan)
        return _lib.Library(os.path.abspath(os.environ["NDFFT_EMUL_LIB"]))
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "-j4"])
    return _lib.Library(os.path.join(EMUL_DIR, "_build", "libndfft_emul.so"))


def test_exception_table_names_routes_with_reasons():
    """An entry of WARM_EXCEPTIONS is a route name with its reason (docs/streams.md lists the same table; empty is the expected state)."""
    assert all(isinstance(k, str) and isinstance(v, str) and v.strip() for k, v in ss.WARM_EXCEPTIONS.items())


@pytest.mark.parametrize("case", CASES, ids=[ss.case_id(c) for c in CASES])
def test_warm_call_stays_on_its_stream_and_allocates_nothing(L, case):
    """stream_suite.warm_call_contract: warm-up on A; the same call on A is all on A, allocates, frees, copies and waits for nothing, takes the case's route and
    matches the oracle; a call on B stays on B; A again allocates nothing -- B did not evict A's scratch (the deterministic form of the two-stream test on the
    MI355X)."""
    ss.warm_call_contract(L, case)


def test_the_log_sees_what_it_claims_to_see(L):
    """The instrument itself: an upload and a download are synchronous copies, ndfft_dev_sync is a wait, the first call of a multi-pass shape on a new stream
    allocates -- so a zero in the contract test is a measured zero."""
    import ctypes

    import numpy as np

    import devmem
    import parity_suite as ps
    ss.call_log(L)
    buf = devmem.DevBuf(L, np.zeros(64))                     # hipMalloc + hipMemcpy
    buf.download(np.zeros(64)); L.check(L.c.ndfft_dev_sync(ctypes.c_void_p(ss.HANDLE_A))); buf.free()
    calls, counts = ss.call_log(L)
    assert not calls and counts == dict(zip(ss.COUNTERS, (1, 1, 0, 2, 0, 1, 0, 0))), (calls, counts)
    case = ss.exec_case(({}, "ndfft", (2, 32768), 1, np.float64, "C", "four_step"))
    sp = ss.make_spec(L, case)
    din, dout = devmem.DevBuf(L, sp.xa), devmem.DevBuf(L, sp.ya)
    try:
        fresh = 0x5C5C0C00                                   # a stream no test has used
        path, calls, counts = ss._logged(L, sp, (din.p.value, dout.p.value, 0), fresh)
        assert path == "four_step" and counts["hipMalloc"] >= 1 and len(calls) >= 2 and {s for _, s in calls} == {fresh}, (path, calls, counts)
    finally:
        din.free(); dout.free()
