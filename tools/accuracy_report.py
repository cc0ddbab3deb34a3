#!/usr/bin/env python3
"""Measure every case of the accuracy tables (tests/parity_suite.py: ACC_GPU_FAMILIES on the MI355X; tests/test_emul_parity.py: ROUTE_TABLE + ACC_EXTRA on the
CPU emulation) and write the table of docs/accuracy.md: per case and input the route, op, shape, dtype, the library's and the oracle's error in eps and their
ratio, for lane L2 and worst bin.  Nothing is asserted here; rows beyond the tests' bar are marked.

    python tools/accuracy_report.py --target emul                      # builds tests/emul, rewrites the emulation table of docs/accuracy.md
    python tools/accuracy_report.py --target gpu --table-out FILE      # on an MI355X: the table alone, into FILE
    python tools/accuracy_report.py --target gpu --splice FILE         # put a table measured elsewhere into docs/accuracy.md
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
DOC = os.path.join(ROOT, "docs", "accuracy.md")
TITLE = {"emul": "CPU emulation (x86-64, -O1, no FMA contraction)", "gpu": "MI355X (gfx950, -ffp-contract=fast)"}


def measure(target):
    import numpy as np
    import parity_suite as ps
    from ndrustfft_amd import _lib
    if target == "emul":
        os.environ.setdefault("EMUL_DEVICES", "3")
        import test_emul_parity as te
        subprocess.check_call(["make", "-C", te.EMUL_DIR, "-s", "-j4"])
        L = _lib.Library(os.path.join(te.EMUL_DIR, "_build", "libndfft_emul.so"))
        families = {"route table": te.ROUTE_TABLE, "long rows, DCT-I, Bluestein and odd lengths": te.ACC_EXTRA}
    else:
        L = _lib.default()
        families = {k: f() for k, f in ps.ACC_GPU_FAMILIES.items()}
    lines = []
    for fam, cases in families.items():
        t0 = time.time(); worst = (0.0, 0.0)
        lines += ["", f"#### {fam}", "", "| route | op | shape | axis | dtype | switches | input | lib L2 | oracle L2 | ratio | lib bin | oracle bin | ratio |", "|" + "---|" * 13]
        for case in cases:
            for r in ps.accuracy_records(L, case):
                over = any(not (l <= ps.ACC_FACTOR * d) for l, d in zip(r["lib"], r["den"]))
                sw = " ".join(f"{k}={v}" for k, v in r["switches"].items())
                shape = "x".join(str(s) for s in r["shape"]) + (" F" if case[5] == "F" else "")
                lines.append(f"| {r['route']} | {r['op']} | {shape} | {r['axis']} | {r['dtype']} | {sw} | {r['input']} | {r['lib'][0]:.2f} | {r['den'][0]:.2f} | {r['ratio'][0]:.2f} | "
                             f"{r['lib'][1]:.2f} | {r['den'][1]:.2f} | {r['ratio'][1]:.2f}{' **over**' if over else ''} |")
                worst = tuple(max(w, x) if x == x else float("nan") for w, x in zip(worst, r["ratio"]))
        print(f"{fam}: {len(cases)} cases, worst ratio L2 {worst[0]:.2f} bin {worst[1]:.2f}, {time.time() - t0:.1f} s", flush=True)
    import scipy
    head = [f"### {TITLE[target]}", "", f"`tools/accuracy_report.py --target {target}`; numpy {np.__version__}, scipy {scipy.__version__}, long double eps {float(np.finfo(np.longdouble).eps):.2e}.  "
            "Errors in eps of the real dtype; `oracle` is the bar's denominator max(oracle on this input, oracle on U[-1,1)); ratio = lib / oracle."]
    return "\n".join(head + lines) + "\n"


def splice(target, table):
    begin, end = f"<!-- BEGIN {target} table -->", f"<!-- END {target} table -->"
    doc = open(DOC).read()
    a, b = doc.index(begin) + len(begin), doc.index(end)
    open(DOC, "w").write(doc[:a] + "\n" + table + doc[b:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--target", choices=("emul", "gpu"), required=True)
    ap.add_argument("--table-out", help="write the table to this file instead of docs/accuracy.md")
    ap.add_argument("--splice", help="take the table from this file instead of measuring")
    a = ap.parse_args()
    table = open(a.splice).read() if a.splice else measure(a.target)
    if a.table_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.table_out)), exist_ok=True)
        open(a.table_out, "w").write(table)
    else:
        splice(a.target, table)


if __name__ == "__main__":
    main()
