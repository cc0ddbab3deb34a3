"""NORM_NONE / NORM_DEFAULT / NORM_SCALE on the CPU build of the kernel sources (tests/norm_suite.py; docs/accuracy.md, "Normalisation modes"): every row of
ROUTE_TABLE and ACC_EXTRA and an ndifft twin of every ndfft row through ndfft_exec_device under the six modes -- the exact properties P1, P2, P3 and P5 and the
working-precision bar on (SCALE, 0.37), all three inputs -- then ndfft_exec on host arrays, one case per strategy, and the two sharded entry points on the
fake devices.  The emulation speaks for the launchers and the order of operations; tests/test_norm_gpu.py for the gfx950 code."""
import os
import subprocess

import pytest

import accuracy as acc
import norm_suite as ns
from ndrustfft_amd import _lib
from test_emul_parity import ACC_EXTRA, EMUL_DIR, ROUTE_TABLE

CASES = ns.with_inverse_twins(ROUTE_TABLE + ACC_EXTRA)


@pytest.fixture(scope="module")
def L():
    if os.environ.get("NDFFT_EMUL_LIB"):                    # a side build of the emulation (make -C tests/emul SAN=1: UBSan)
        return _lib.Library(os.path.abspath(os.environ["NDFFT_EMUL_LIB"]))
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "-j4"])
    return _lib.Library(os.path.join(EMUL_DIR, "_build", "libndfft_emul.so"))


@pytest.mark.parametrize("case,twin_of", CASES, ids=[("twin-" if t else "") + ns.case_id(c) for c, t in CASES])
def test_modes_on_a_table_row(L, case, twin_of):
    """One row: route, P1 or P2 / P3 / P5 on the uniform input, P2 on the impulse input, P4 on uniform, impulse and graded inputs."""
    ns.check_case(L, case, p4=acc.INPUTS, twin_of=twin_of, verbose=True, tag="twin" if twin_of else "row")


def test_every_c2c_route_of_the_tables_has_an_inverse_case():
    fwd = [c for c, t in CASES if c[1] == "ndfft"]
    twins = [t for c, t in CASES if t is not None]
    assert fwd and fwd == twins


@pytest.mark.parametrize("case", ns.HOST_CASES, ids=[f"{c[0]}-{c[2]}-{'x'.join(map(str, c[3]))}" for c in ns.HOST_CASES])
def test_ndfft_exec_on_host_arrays(L, case):
    ns.host_case(L, case)


@pytest.mark.parametrize("ids,root", [([0, 1, 2], 1), ([2, 0], 0)], ids=["012", "20"])
@pytest.mark.parametrize("case", ns.SHARDED_CASES, ids=[c[0] for c in ns.SHARDED_CASES])
def test_sharded_entry_points(L, case, ids, root):
    assert L.c.ndfft_device_count() == 3
    ns.sharded_case(L, case, ids, root)
