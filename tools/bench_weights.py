#!/usr/bin/env python3
"""What Normalization.weights costs on the MI355X (needs the GPU; fails without one).

Device-resident 4096 x 4096 arrays, HBM-sourced over rotating (in, out) pairs as bench.py does, timed with device events after warm-up.
Configurations: ndifft c128 axis 1 and axis 0, nddct2 f64 axis 1, ndifft_r2c f64 axis 1.  For each one, in the same run, alternating:
  default   the unweighted call under Normalization::Default (code this feature does not touch)
  weights   the same call under Normalization.weights (one extra pass over the weighted array)
  custom    the Normalization.custom round trip -- download, one host call per lane, upload -- ONE repetition, end to end with the synchronise
Byte model: a weighted call moves (2 in + in + out) bytes (pass before the transform) or (in + out + 2 out) (pass after it) against (in + out).
Prints one JSON line per configuration and a final JSON line with all of them.  --profile runs only the weighted calls, a few times, for a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_weights.py --profile): the pass's own kernel time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=4, help="rotating (in, out) pairs per configuration")
    ap.add_argument("--steps", type=int, default=40, help="timed calls per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks (default, weights, default, weights, ...)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--no-custom", action="store_true", help="skip the Custom(fn) round trip")
    ap.add_argument("--profile", action="store_true", help="weighted calls only, 5 per configuration (for a kernel trace)")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_weights.py needs an MI355X"
    from ndrustfft_amd import DctHandler, FftHandler, Normalization, R2cFftHandler, _lib, nddct2, ndifft, ndifft_r2c
    L = _lib.default()
    rows, n = args.rows, args.n
    rng = np.random.default_rng(7)
    configs = [
        ("ndifft c128 axis 1", ndifft, FftHandler, n, (rows, n), (rows, n), 1, torch.complex128, torch.complex128, True),
        ("ndifft c128 axis 0", ndifft, FftHandler, n, (n, rows), (n, rows), 0, torch.complex128, torch.complex128, True),
        ("nddct2 f64 axis 1", nddct2, DctHandler, n, (rows, n), (rows, n), 1, torch.float64, torch.float64, False),
        ("ndifft_r2c f64 axis 1", ndifft_r2c, R2cFftHandler, n, (rows, n // 2 + 1), (rows, n), 1, torch.complex128, torch.float64, True),
    ]
    results = []
    for what, fn, hcls, hn, sin, sout, axis, dtin, dtout, wcplx in configs:
        m = sin[axis] if fn is not ndifft else sout[axis]
        w = rng.uniform(0.5, 2.0, m) * (np.exp(2j * np.pi * rng.uniform(0, 1, m)) if wcplx else rng.choice([-1.0, 1.0], m))
        h_def = hcls(hn)
        h_w = hcls(hn).normalization(Normalization.weights(w))

        def cust(lane, w=w):
            lane *= w
        h_c = hcls(hn).normalization(Normalization.custom(cust))
        pairs = []
        for _ in range(args.pairs):
            x = torch.rand(sin, dtype=torch.float64, device="cuda") - 0.5
            if dtin.is_complex:
                x = torch.complex(x, torch.rand(sin, dtype=torch.float64, device="cuda") - 0.5)
            pairs.append((x.contiguous(), torch.zeros(sout, dtype=dtout, device="cuda")))
        bytes_in = pairs[0][0].numel() * pairs[0][0].element_size(); bytes_out = pairs[0][1].numel() * pairs[0][1].element_size()
        k = [0]

        def call(h):
            x, y = pairs[k[0] % len(pairs)]; k[0] += 1
            fn(x, y, h, axis)

        def block(h, steps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                call(h)
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / steps
        for _ in range(args.warmup):
            call(h_def); call(h_w)
        torch.cuda.synchronize()
        path_w = L.last_path()
        if args.profile:
            for _ in range(5):
                call(h_w)
            torch.cuda.synchronize()
            print(json.dumps({"config": what, "route": path_w, "profile_calls": 5}), flush=True)
            continue
        t_def, t_w = [], []
        for _ in range(args.blocks):
            t_def.append(block(h_def, args.steps)); t_w.append(block(h_w, args.steps))
        call(h_def); torch.cuda.synchronize(); path_def = L.last_path()
        t_custom = None
        if not args.no_custom:
            x, y = pairs[0]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn(x, y, h_c, axis)
            torch.cuda.synchronize(); t_custom = (time.perf_counter() - t0) * 1e6
        pre = fn is not ndifft
        model = (3 * bytes_in + bytes_out) if pre else (bytes_in + 3 * bytes_out)
        rec = {"config": what, "shape_in": list(sin), "route_default": path_def, "route_weights": path_w,
               "default_us": round(float(np.median(t_def)), 2), "default_us_blocks": [round(t, 2) for t in t_def],
               "weights_us": round(float(np.median(t_w)), 2), "weights_us_blocks": [round(t, 2) for t in t_w],
               "ratio": round(float(np.median(t_w) / np.median(t_def)), 3),
               "custom_round_trip_us": None if t_custom is None else round(t_custom, 0),
               "bytes_default": bytes_in + bytes_out, "bytes_weights_model": model, "bytes_ratio_model": round(model / (bytes_in + bytes_out), 3),
               "pass_us_by_difference": round(float(np.median(t_w) - np.median(t_def)), 2),
               "pass_TBps_by_difference": round(2 * (bytes_in if pre else bytes_out) / max(float(np.median(t_w) - np.median(t_def)), 1e-9) / 1e6, 3)}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del pairs
        torch.cuda.empty_cache()
    if not args.profile:
        print(json.dumps({"bench_weights": results, "device": torch.cuda.get_device_name(0), "steps": args.steps, "blocks": args.blocks, "pairs": args.pairs}))


if __name__ == "__main__":
    main()
