#!/usr/bin/env python3
"""What ndfft_filter costs on the MI355X (needs the GPU; fails without one).

Device-resident arrays, HBM-sourced over rotating (in, out) pairs whose inputs add up to at least 768 MiB (three times the Infinity Cache), timed with device
events after a warm-up that also ramps the clock.  For c128 and c64 (an FftHandler), f64 and f32 (real arrays under an R2cFftHandler, n // 2 + 1 weights) or d64 and
d32 (real arrays under a DctHandler: nddct_filter, n real weights; two_calls is nddct2 then nddct3) and the shapes 4096 x 4096, 16384 x 1024 and 65536 x 256 (lanes along axis 1;
--axis 0: a shape R x C means lanes of R points along axis 0 of an R x C array, the strided axis), in the same run, in alternating blocks:
  two_calls   ndfft then ndifft (real: ndfft_r2c then ndifft_r2c) through a work array: code the filter does not touch, and a lower bound for any three-call
              form (the multiply is left out)
  composed    the filter with fuse=False: the forward transform into the spectrum image, the diagonal pass in place, the inverse
  fused       the filter's one kernel
Reports the median block time per call in us and 2 x array bytes / time as a fraction of 8 TB/s.  One JSON line per configuration and a final line with all."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24, help="timed calls per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per form")
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--min-input-mib", type=int, default=768)
    ap.add_argument("--shapes", default="4096x4096,16384x1024,65536x256")
    ap.add_argument("--axis", type=int, choices=(0, 1), default=1, help="the axis of the lanes: 1 = rows x n (unit stride), 0 = n x columns (strided)")
    ap.add_argument("--dtypes", default="c128,c64", help="of c128, c64 (complex arrays), f64, f32 (real arrays, R2C) and d64, d32 (real arrays, DCT)")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_filter.py needs an MI355X"
    from ndrustfft_amd import DctHandler, FftHandler, R2cFftHandler, _lib, nddct2, nddct3, nddct_filter, ndfft, ndfft_filter, ndfft_r2c, ndifft, ndifft_r2c
    L = _lib.default()
    rng = np.random.default_rng(7)
    results = []
    for dname in args.dtypes.split(","):
        assert dname in ("c128", "c64", "f64", "f32", "d64", "d32"), dname
        dct = dname[0] == "d"
        real = dname[0] == "f" or dct
        cdt, rdt, rnp = (torch.complex128, torch.float64, np.float64) if dname in ("c128", "f64", "d64") else (torch.complex64, torch.float32, np.float32)
        adt = rdt if real else cdt
        for sh in args.shapes.split(","):
            dims = tuple(int(v) for v in sh.split("x"))
            axis = args.axis
            n = dims[axis]
            rows = dims[1 - axis]
            nbytes = rows * n * torch.empty((), dtype=adt).element_size()
            npairs = max(2, -(-(args.min_input_mib << 20) // nbytes))
            h = DctHandler(n, rnp) if dct else R2cFftHandler(n, rnp) if real else FftHandler(n, rnp)
            m = n if dct else n // 2 + 1 if real else n             # the spectrum lane
            if dct:
                w = torch.from_numpy((rng.uniform(0.5, 2.0, m) * rng.choice([-1.0, 1.0], m)).astype(rnp)).to("cuda")
            else:
                w = torch.from_numpy((rng.uniform(0.5, 2.0, m) * np.exp(2j * np.pi * rng.uniform(0, 1, m))).astype(np.complex128 if rnp is np.float64 else np.complex64)).to("cuda")
            pairs = []
            for _ in range(npairs):
                x = torch.rand(dims, dtype=rdt, device="cuda") - 0.5
                if not real:
                    x = torch.complex(x, torch.rand(dims, dtype=rdt, device="cuda") - 0.5)
                wdims = tuple(m if d == axis else e for d, e in enumerate(dims))
                pairs.append((x, torch.zeros(dims, dtype=adt, device="cuda"), torch.zeros(wdims, dtype=rdt if dct else cdt, device="cuda")))
            k = [0]

            def two_calls(x, y, work):
                if dct:
                    nddct2(x, work, h, axis); nddct3(work, y, h, axis)
                elif real:
                    ndfft_r2c(x, work, h, axis); ndifft_r2c(work, y, h, axis)
                else:
                    ndfft(x, work, h, axis); ndifft(work, y, h, axis)

            def composed(x, y, work):
                (nddct_filter if dct else ndfft_filter)(x, y, h, axis, w, fuse=False)

            def fused(x, y, work):
                (nddct_filter if dct else ndfft_filter)(x, y, h, axis, w)
            forms = {"two_calls": two_calls, "composed": composed, "fused": fused}
            routes = {}

            def block(fn, steps):
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    fn(*pairs[k[0] % npairs]); k[0] += 1
                e1.record(); torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / steps
            for name, fn in forms.items():
                for _ in range(args.warmup):
                    fn(*pairs[k[0] % npairs]); k[0] += 1
                torch.cuda.synchronize()
                routes[name] = L.last_path()
            times = {name: [] for name in forms}
            for _ in range(args.blocks):
                for name, fn in forms.items():
                    times[name].append(block(fn, args.steps))
            rec = {"dtype": dname, "shape": list(dims), "pairs": npairs, "array_bytes": nbytes, "routes": routes}
            if axis != 1:
                rec["axis"] = axis
            for name in forms:
                med = float(np.median(times[name]))
                rec[name + "_us"] = round(med, 2); rec[name + "_us_blocks"] = [round(t, 2) for t in times[name]]
                rec[name + "_frac_of_8TBps"] = round(2 * nbytes / (med * 1e-6) / PEAK, 3)
            rec["fused_over_composed"] = round(rec["fused_us"] / rec["composed_us"], 3)
            rec["fused_over_two_calls"] = round(rec["fused_us"] / rec["two_calls_us"], 3)
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del pairs
            torch.cuda.empty_cache()
    print(json.dumps({"bench_filter": results, "device": torch.cuda.get_device_name(0), "steps": args.steps, "blocks": args.blocks}))


if __name__ == "__main__":
    main()
