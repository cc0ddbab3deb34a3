"""exec_internal.h: MallModel's kept share, through ndfft_last_input_policy and ndfft_last_input_keep (device-resident arrays on the emulation).  A rotation of
inputs larger than the Infinity Cache streams every member, and every member keeps floor(64 budget / D) of every 64 blocks, D its reuse distance in bytes; no share
for a buffer last written past the cache, for INPUT_COLD, with the budget at 0; the size-rule path of a buffer larger than the cache computes one too."""
import ctypes
import os
import subprocess

import pytest

import filter_instances_suite as fis
import parity_suite as ps
from ndrustfft_amd import _lib, api, handlers

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "emul")
MIB = 1 << 20
N = 64
BUDGET = 192          # MiB, set through ndfft_set_keep_budget


@pytest.fixture(scope="module")
def L():
    if os.environ.get("NDFFT_EMUL_LIB"):
        return _lib.Library(os.path.abspath(os.environ["NDFFT_EMUL_LIB"]))
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "-j4"])
    return _lib.Library(os.path.join(EMUL_DIR, "_build", "libndfft_emul.so"))


def test_kept_share_of_a_rotation_larger_than_the_cache(L):
    h = handlers.FftHandler(N, _library=L)
    bufs = []
    def dev_buf(mib):
        p = ctypes.c_void_p(); L.check(L.c.ndfft_dev_alloc(ctypes.byref(p), mib * MIB)); bufs.append(p); return p
    def fft(src, dst, mib):
        """(policy, share) of one forward call on `mib` MiB of 64-point c128 lanes: the register row kernel, the one the model serves"""
        rows = mib * MIB // (N * 16)
        L.check(L.c.ndfft_exec_device(h._plan, _lib.OP_C2C_FWD, src, dst, 2, api._i64((rows, N)), api._i64((N, 1)), api._i64((rows, N)), api._i64((N, 1)), 1, _lib.NORM_DEFAULT, 0.0, None))
        assert L.last_path() == "pow2_reg", L.last_path()
        return L.last_input_policy(), L.last_input_keep()
    big = 72                                        # outputs above the 64 MiB line: written past the cache
    xs = [dev_buf(big) for _ in range(6)]
    o, o2 = dev_buf(big), dev_buf(big)
    h1, ho = dev_buf(260), dev_buf(260)
    fis.settle_residency_model(L)                   # what earlier tests left in the model, by address, is gone
    share = 64 * BUDGET // (6 * big)                # D = 432 MiB: the five other members read since, plus the member itself
    assert share == 28 and 6 * share * big <= 64 * BUDGET, "the kept parts of a whole cycle fit the budget"
    try:
        with ps.switches(L, NDFFT_WAVE="0"):
            L.set_keep_budget(BUDGET)
            for x in xs: assert fft(x, o, big) == (0, 0), "first cycle: never seen, the size rule, plain loads"
            for cycle in (2, 3):
                for x in xs: assert fft(x, o, big) == (1, share), f"cycle {cycle}: streamed, floor(64 * {BUDGET} / 432) kept"
            assert fft(o, o2, big) == (1, 0), "last written as an output of more than 64 MiB: nothing of it is in the cache"
            assert fft(xs[0], o, big)[0] == 1 and fft(xs[0], o, big) == (0, 0), "re-read at once: plain loads, the whole input allocates"
            L.check(L.c.ndfft_set_input_hint(_lib.INPUT_COLD))
            assert fft(xs[1], o, big) == (1, 0), "INPUT_COLD: the caller says the data is not there"
            L.check(L.c.ndfft_set_input_hint(_lib.INPUT_AUTO))
            # larger than the cache, read again at once: the size-rule path.  The share is computed from D = the buffer's size; the policy is the size rule's
            assert fft(h1, ho, 260) == (0, 0), "never seen"
            assert fft(h1, ho, 260) == (0, 64 * BUDGET // 260)
            L.set_keep_budget(0)
            for x in xs: assert fft(x, o, big)[1] == 0, "budget 0: the feature is off"
            assert fft(xs[0], o, big) == (1, 0)
            L.set_keep_budget(100000)
            assert fft(xs[1], o, big) == (1, 63), "the share is clamped to 63"
            L.set_keep_budget(-1)                   # the default budget: on
            pol, k = fft(xs[2], o, big)
            assert pol == 1 and 0 < k <= 63
            with ps.switches(L, NDFFT_STREAM_LOADS="1"):
                assert fft(xs[3], o, big) == (1, 0), "a forced policy keeps nothing"
                L.force_input_keep(37)
                assert fft(xs[4], o, big) == (1, 37), "ndfft_force_input_keep forces the share of whatever streams"
    finally:
        L.c.ndfft_set_input_hint(_lib.INPUT_AUTO); L.set_keep_budget(-1); L.force_input_keep(-1)
        for p in bufs: L.check(L.c.ndfft_dev_free(p))
        fis.settle_residency_model(L)
