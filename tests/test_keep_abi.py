"""include/ndfft_mi355x_keep.h (ABI minor 7): the header declares exactly the binding's KEEP_SYMBOLS, the gfx950 library exports them, the extension header
still reaches them, and the two setters refuse what they document.  CPU test: no GPU call."""
import os
import re
import subprocess

import pytest

from ndrustfft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndrustfft_amd", "csrc"), "-s", "-j4"])
    return _lib.Library()


def test_header_symbols_exported(lib):
    text = open(os.path.join(ROOT, "include", "ndfft_mi355x_keep.h")).read()
    declared = sorted(set(re.findall(r"^int\s+(ndfft_\w+)\s*\(", text, re.M)))
    assert declared == sorted(_lib.KEEP_SYMBOLS), declared
    for s in declared:
        assert hasattr(lib.c, s) and getattr(lib.c, s).argtypes is not None, s
    assert lib.c.ndfft_abi_minor() >= 7
    ext = open(os.path.join(ROOT, "include", "ndfft_mi355x_ext.h")).read()
    assert '#include "ndfft_mi355x_keep.h"' in ext, "a consumer of the extension header gets the declarations too"


def test_setters_check_their_argument(lib):
    assert lib.c.ndfft_last_input_keep() == 0                       # no device exec on this thread yet, or one that kept nothing
    assert lib.c.ndfft_set_keep_budget((1 << 20) + 1) == _lib.ERR_INVALID_ARG and b"budget" in lib.c.ndfft_last_error()
    assert lib.c.ndfft_force_input_keep(65) == _lib.ERR_INVALID_ARG and b"share" in lib.c.ndfft_last_error()
    for v in (0, 192, -1):
        assert lib.c.ndfft_set_keep_budget(v) == _lib.OK
    for v in (0, 64, -1):
        assert lib.c.ndfft_force_input_keep(v) == _lib.OK


def test_header_is_strict_c99(tmp_path):
    src = tmp_path / "keep_c99.c"
    src.write_text('#include "ndfft_mi355x_ext.h"\nint main(void) { int (*f)(void) = ndfft_last_input_keep; int (*g)(int) = ndfft_set_keep_budget; int (*h)(int) = ndfft_force_input_keep;\n'
                   "    return f && g && h ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "keep_c99.o")])
