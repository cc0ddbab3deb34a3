#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric: batched 1-D C2C FFT along the contiguous axis of an
f64 array, GFFT-points/s (whole job) + achieved HBM GB/s vs the 8 TB/s roofline.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run does only what the headline figure needs: set up, ramp the clocks and warm up, time ONE block of EXACTLY K steps,
write the sampled outputs of the last timed step if --dump-outputs is given, print the result line.  Everything else below
(the median of --blocks blocks, no_ramp, the warm and strong regions, other_configs, host_api, xgmi, cpu_baseline and the numpy
self-check of the timed outputs) runs only with --full.

--dump-outputs DIR: after the timed steps, a fixed seeded sample of rows of what the last timed step wrote (the array a caller of
ndfft receives) as DIR/ndfft_out.npy (rank r > 0: ndfft_out_rank<r>.npy), float64 of shape (sampled rows, n, 2) = (re, im), 16 MiB
over all ranks; the rows are sorted(numpy.random.default_rng(20241008).choice(rows, count, replace=False)).  The timed steps start
at pair 0 of the rotation, so with the same arguments the last step's input, and thus its output, is the same from run to run.

N > 1 runs N ranks, one per GPU, over torch.distributed (RCCL):
  * under a launcher (`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`) the rank
    environment is already there and this process IS a rank;
  * started plainly (`python bench.py --gpus N`, no WORLD_SIZE in the environment) this process only spawns the N
    ranks as children -- before anything here touches the GPU or imports torch -- and exits with their status.

Primary line (the contract's `value`, `ms_per_step`, `roofline.frac`): the configuration BASELINE.json's metric is quoted on --
ndfft axis=1 on 4096x4096 Complex<f64> arrays, device resident -- PER GPU at every N ("scaling": "weak": N ranks hold the N
contiguous 4096-row blocks of a (4096 N) x 4096 array; lanes are independent, src/lib.rs:120-124 / 187-194, so
there is no data-path collective).  One "step" = one ndfft call over one whole resident array through the C ABI
(ndfft_exec_device).  The steps walk over ROTATING (in, out) pairs whose footprint (6 pairs = 3 GiB) exceeds the 256 MiB
Infinity Cache, so every step's input really comes from HBM: this is the HBM-sourced number (round 4; until round 3 the
headline re-read one 256 MiB input that the Infinity Cache partly holds -- that loop is now `roofline.frac_warm`).

With --full, every region is timed as --blocks (7) blocks of EXACTLY K steps each, every block between barrier + synchronize on both sides,
max over ranks per block; the line reports the MEDIAN block (`steps` = K, `ms_per_step`, `value`) and min / median / max over the
blocks under `blocks`, so that one ~2 ms sample does not decide the record.

With --full, more measurements ride in the same JSON line (each its own timed region, after the primary one):
  * roofline.frac_warm / roofline.warm -- the same call on ONE (in, out) pair re-used every step (Infinity-Cache assisted);
  * strong_cfg5 -- BASELINE configs[4]: the 65536x4096 array split in N contiguous row blocks, one per rank
    (N = 1: the whole 4 GiB + 4 GiB array on one GPU), i.e. STRONG scaling of the north star's multi-GPU target;
  * other_configs (N = 1) -- BASELINE configs[2] and [3] as driver-timed blocks: cfg3-A (ndfft_r2c axis 0, 8192x8192 f32), cfg3-B (ndfft axis 1 on
    its 4097x8192 c64 output), cfg4 (nddct2 axis 2, 256x256x512 f64), each HBM-sourced over rotating pairs with a numpy spot check;
  * roofline.frac_from_ms_per_step -- the primary fraction recomputed from the wall-clock ms_per_step instead of the HIP-event launch time.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (~6.3 TB/s achievable)
CFG5_ROWS = 65536              # BASELINE configs[4]


def usable_cpus():
    """CPUs this process may actually use: the affinity mask capped by the cgroup CPU quota (the GPU box
    shows 256 logical CPUs but grants 16 -- 128 OpenMP threads on 16 CPUs ran 5x SLOWER than 16)."""
    import math
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]                       # cgroup v2
        if q != "max":
            n = min(n, max(1, math.ceil(int(q) / int(per))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, math.ceil(q / per)))
        except Exception:
            pass
    return n


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(n, rows, budget_s=12.0):
    """The CPU oracle's restatement of ndfft_par (create_transform_par!, src/lib.rs:169-238, OpenMP
    standing in for rayon) on the host cores; bounded sample of the same workload.  A second, independent CPU
    number is scipy's pocketfft with workers = the same core count."""
    import numpy as np
    import synth
    from oracle import oracle_ctypes as orc
    x = synth.complex_array((rows, n))
    y = np.zeros_like(x)
    # timed with the restatement compiled for THIS host (-O3 -march=native) when that builds and still agrees with numpy; the parity tests keep -O2
    flags = orc.use_fast_build() or "-O2"
    h = orc.FftHandler(n)
    orc.ndfft_par(x, y, h, 1)                      # warm
    assert np.abs(y[:2] - np.fft.fft(x[:2], axis=1)).max() / np.abs(y[:2]).max() < 1e-12
    t0 = time.perf_counter(); reps = 0
    while True:
        orc.ndfft_par(x, y, h, 1); reps += 1
        el = time.perf_counter() - t0
        if el > budget_s or reps >= 500:
            break
    pts = rows * n * reps
    out = {"value": round(pts / el / 1e9, 4), "unit": "GFFT-points/s", "cores": orc.num_threads(), "kind": "port",
           "cpu_model": cpu_model(), "build": "gcc " + flags,
           "sample": f"{reps} x ndfft_par axis=1 on {rows}x{n} Complex<f64> (oracle/ndfft_oracle.c, OpenMP over lanes, "
                     f"{el:.1f} s; scalar C restatement of ndrustfft _par, NOT rustfft -- a lower bound on the reference's CPU speed)"}
    try:
        import scipy.fft as sfft
        w = orc.num_threads()
        sfft.fft(x, axis=1, workers=w)
        t0 = time.perf_counter(); reps = 0
        while True:
            sfft.fft(x, axis=1, workers=w); reps += 1
            el = time.perf_counter() - t0
            if el > budget_s / 2 or reps >= 500:
                break
        out["scipy_pocketfft"] = {"value": round(rows * n * reps / el / 1e9, 4), "unit": "GFFT-points/s", "workers": w,
                                  "sample": f"{reps} x scipy.fft.fft(axis=1, workers={w}) on the same array, {el:.1f} s (allocates its output)"}
    except Exception as e:                           # scipy missing on the box: say so, do not fail the bench
        out["scipy_pocketfft"] = {"value": None, "error": repr(e)}
    return out


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def spawn_ranks(ngpu):
    """Parent of a plain `python bench.py --gpus N`: start N ranks as children (nothing in this process has
    touched the GPU -- torch is not even imported), wait, and return the worst exit status."""
    port = os.environ.get("MASTER_PORT") or str(free_port())
    procs = []
    for r in range(ngpu):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(ngpu), LOCAL_WORLD_SIZE=str(ngpu),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for p in procs:
        p.wait()
        rc = rc or p.returncode
    return rc


def xgmi_block(dist, torch, dev, rank, ngpu, n, ndfft, FftHandler, sync_all, prow=2048, side_per_rank=1024, m=1024):
    """N > 1: the data movement of SURVEY 8e / 8f rank 3 over xGMI (never part of `value`: lanes that are born sharded need
    none of it).  Root scatter and gather of batch slices (point-to-point groups, one slice per link) and the all-to-all
    re-shard between the two axis passes of a sharded fft2; GB/s per link against the ~153 GB/s an xGMI link carries, and a
    correctness check of each.  Every rank makes the same sequence of collective calls (tests/test_distributed.py runs this
    function at world size 2 on gloo with the oracle as the executor)."""
    import numpy as np
    import synth
    from ndrustfft_amd import distributed as nd_dist
    out = {}
    gshape = (prow * ngpu, n)                                             # prow rows per rank: 2048 x 4096 c128 = 128 MiB per link
    full = synth.complex_array_torch(gshape, dev) if rank == 0 else None

    def best(fn, reps=3):
        ts = []; r = None
        for _ in range(reps):
            sync_all(); t0 = time.perf_counter(); r = fn(); sync_all(); ts.append(time.perf_counter() - t0)
        t = torch.tensor([min(ts)], device=dev, dtype=torch.float64); dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t[0]), r
    link_bytes = prow * n * 16
    h = FftHandler(n)
    t_sc, shard = best(lambda: nd_dist.scatter_lanes(full, gshape, torch.complex128, 1, 0, dev))
    yl = torch.empty_like(shard); ndfft(shard, yl, h, 1)
    t_ga, gathered = best(lambda: nd_dist.gather_lanes(yl, gshape, 0, 0))
    ok = True
    if rank == 0:
        ref = np.fft.fft(synth.complex_array((2, n), offset=(gshape[0] - 2) * n), axis=1)     # the last rank's last two lanes
        ok = bool(np.abs(gathered[-2:].cpu().numpy() - ref).max() / np.abs(ref).max() < 1e-10)
    out["scatter"] = {"bytes_per_link": link_bytes, "links": ngpu - 1, "ms": round(t_sc * 1e3, 3), "GBs_per_link": round(link_bytes / t_sc / 1e9, 1)}
    out["gather"] = {"bytes_per_link": link_bytes, "links": ngpu - 1, "ms": round(t_ga * 1e3, 3), "GBs_per_link": round(link_bytes / t_ga / 1e9, 1),
                     "scatter_transform_gather_matches_numpy": ok}
    del full, gathered
    # all-to-all: re-shard an (N side) x (N side) c128 array from row slabs to column slabs
    side = side_per_rank * ngpu
    slab = synth.complex_array_torch((side // ngpu, side), dev, offset=rank * (side // ngpu) * side)
    t_a2a, cols = best(lambda: nd_dist.reshard(slab, (side, side), 0, 1))
    pair_bytes = (side // ngpu) * (side // ngpu) * 16
    back = nd_dist.reshard(cols, (side, side), 1, 0)
    out["all_to_all_reshard"] = {"array": f"{side}x{side} c128", "bytes_per_pair": pair_bytes, "ms": round(t_a2a * 1e3, 3),
                                 "GBs_per_link": round(pair_bytes / t_a2a / 1e9, 1), "round_trip_exact": bool(torch.equal(back, slab))}
    # sharded fft2 (axis 1, all-to-all, axis 0) against numpy on an m x m array
    a_full = synth.complex_array((m, m))
    lo, hi = nd_dist.shard_bounds(m, ngpu)[rank]
    hm = FftHandler(m)
    yl2, gsh, dsh = nd_dist.transform_axes_sharded([(ndfft, hm, 1, m, torch.complex128), (ndfft, hm, 0, m, torch.complex128)],
                                                   torch.from_numpy(a_full[lo:hi]).to(dev), (m, m), 0)
    ref2 = np.fft.fft2(a_full)
    clo, chi = nd_dist.shard_bounds(m, ngpu)[rank]
    err2 = np.abs(yl2.cpu().numpy() - ref2[:, clo:chi]).max() / np.abs(ref2).max()
    e = torch.tensor([err2], device=dev, dtype=torch.float64); dist.all_reduce(e, op=dist.ReduceOp.MAX)
    out["sharded_fft2_rel_err"] = float(e[0])
    out["peak_GBs_per_link"] = 153.0
    return out


def other_configs_block(torch, np, synth, lib, dev, timed, steps=20, nblocks=3, ramp_ms=150.0):
    """BASELINE.json's remaining single-GPU configs as driver-timed blocks (never `value`):
    cfg3-A ndfft_r2c axis=0 on 8192x8192 f32, cfg3-B ndfft axis=1 on its 4097x8192 c64 output, cfg4 nddct2 axis=2 on 256x256x512 f64.
    Each: rotating (in, out) pairs whose inputs add up to >= 768 MiB (HBM-sourced, as the primary region), an untimed clock ramp + 5 warm-up calls, `nblocks` blocks of
    EXACTLY `steps` calls between barrier + synchronize; the median block is reported, with a numpy spot check of a timed output."""
    from ndrustfft_amd import DctHandler, FftHandler, R2cFftHandler, nddct2, ndfft, ndfft_r2c
    out = []

    def block(name, fn, h, axis, ins, outs, points, check):
        nbytes = ins[0].numel() * ins[0].element_size() + outs[0].numel() * outs[0].element_size()
        cnt = [0]

        def go(_i=0):
            k = cnt[0] % len(ins); cnt[0] += 1
            fn(ins[k], outs[k], h, axis)
        # the synthetic inputs were built on the host while the GPU idled: its clocks need tens of milliseconds of sustained work to come back
        # (see the primary region's ramp), far more than a few ~100 us launches -- keep it busy for >= ramp_ms, untimed, then the warm-up calls
        t_r = time.perf_counter()
        while (time.perf_counter() - t_r) * 1e3 < ramp_ms:
            for _ in range(20):
                go()
            torch.cuda.synchronize()
        for _ in range(max(5, len(ins))):
            go()
        res = sorted((timed(go, steps) for _ in range(nblocks)), key=lambda r: r[0])
        el, dev_ms = res[len(res) // 2]
        torch.cuda.synchronize()
        err = check(ins[0], outs[0])
        out.append({"workload": name, "steps": steps, "blocks": nblocks, "pairs": len(ins), "algorithmic_bytes_per_launch": nbytes,
                    "ms_per_step": round(el / steps * 1e3, 5), "avg_launch_us": round(dev_ms / steps * 1e3, 2),
                    "value": round(points * steps / el / 1e9, 3), "unit": "GFFT-points/s",
                    "frac": round(nbytes / (dev_ms / 1e3 / steps) / 1e9 / HBM_PEAK_GBS, 4),
                    "frac_from_ms_per_step": round(nbytes / (el / steps) / 1e9 / HBM_PEAK_GBS, 4),
                    "path": lib.last_path(), "input_policy": lib.last_input_policy(), "spot_check_rel_err": float(err), "ramp_ms": ramp_ms})

    # ---- cfg3-A then cfg3-B (BASELINE configs[2]): f32, tolerance 1e-4 relative (north_star)
    n = 8192; m = n // 2 + 1; K = 3
    xs = [torch.from_numpy(synth.real_array((n, n), np.float32)).to(dev)]
    xs += [xs[0].clone() for _ in range(K - 1)]                                # distinct buffers (what the cache sees); the same synthetic values
    ws = [torch.empty((m, n), dtype=torch.complex64, device=dev) for _ in range(K)]

    def chk_r2c(a, b):
        ref = np.fft.rfft(a[:, :4].cpu().numpy().astype(np.float64), axis=0)
        e = np.abs(b[:, :4].cpu().numpy() - ref).max() / np.abs(ref).max()
        assert e < 1e-4, f"cfg3-A output differs from numpy.fft.rfft: {e}"
        return e
    block(f"cfg3-A ndfft_r2c axis=0 on {n}x{n} f32 -> {m}x{n} Complex<f32> (BASELINE configs[2], first transform)",
          ndfft_r2c, R2cFftHandler(n, np.float32), 0, xs, ws, n * n, chk_r2c)
    del xs
    os_ = [torch.empty_like(ws[0]) for _ in range(K)]

    def chk_c2c(a, b):
        ref = np.fft.fft(a[:4].cpu().numpy().astype(np.complex128), axis=1)
        e = np.abs(b[:4].cpu().numpy() - ref).max() / np.abs(ref).max()
        assert e < 1e-4, f"cfg3-B output differs from numpy.fft.fft: {e}"
        return e
    block(f"cfg3-B ndfft axis=1 on {m}x{n} Complex<f32> (BASELINE configs[2], second transform, on cfg3-A's output)",
          ndfft, FftHandler(n, np.float32), 1, ws, os_, m * n, chk_c2c)
    del ws, os_

    # ---- cfg4 (BASELINE configs[3]): f64, tolerance 1e-10 relative
    shp = (256, 256, 512); nn = shp[2]; K = 3
    xs = [torch.from_numpy(synth.real_array(shp)).to(dev)]
    xs += [xs[0].clone() for _ in range(K - 1)]
    ys = [torch.empty_like(xs[0]) for _ in range(K)]

    def chk_dct2(a, b):
        j = np.arange(nn)
        C = 2.0 * np.cos(np.pi * np.outer(j, 2 * j + 1) / (2 * nn))            # y[k] = 2 sum_j x[j] cos(pi k (2j+1) / 2n), src/lib.rs:1257
        ref = a[0, :4].cpu().numpy() @ C.T
        e = np.abs(b[0, :4].cpu().numpy() - ref).max() / np.abs(ref).max()
        assert e < 1e-10, f"cfg4 output differs from the DCT-II definition: {e}"
        return e
    block("cfg4 nddct2 axis=2 on 256x256x512 f64 (BASELINE configs[3])", nddct2, DctHandler(nn), 2, xs, ys, shp[0] * shp[1] * shp[2], chk_dct2)
    del xs, ys
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ramp-ms", type=float, default=400.0, help="untimed busy period before the warm-up steps (clock ramp)")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=4096, help="lanes per GPU of the primary line (4096 = the metric's shape)")
    ap.add_argument("--cold-pairs", type=int, default=6, help="distinct (in, out) pairs the primary (HBM-sourced) region rotates over (>= 2; 6 pairs = 3 GiB)")
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement and check (median of --blocks blocks, no_ramp, warm, strong_cfg5, other_configs, "
                         "host_api, xgmi, cpu_baseline, numpy self-check); a plain run times one block of K steps and nothing else")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write a seeded sample of rows of the last timed step's output to DIR/ndfft_out*.npy (float64)")
    ap.add_argument("--blocks", type=int, default=None,
                    help="timed blocks of K steps per region (the line reports the median block and min / median / max); default 7 with --full, else 1")
    ap.add_argument("--no-warm", action="store_true", help="skip the Infinity-Cache-assisted side measurement (one pair re-used every step)")
    ap.add_argument("--strong-steps", type=int, default=20, help="timed steps of the cfg5 strong-scaling block (0 = skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the driver-timed blocks of cfg3-A / cfg3-B / cfg4 (`other_configs`)")
    ap.add_argument("--no-no-ramp", action="store_true", help="skip the `no_ramp` side measurement (W warm-ups from an idle GPU, then 20 steps, before the ramp)")
    ap.add_argument("--host-reps", type=int, default=15, help="repetitions of the host-array (PCIe-inclusive) side measurement")
    ap.add_argument("--no-host-api", action="store_true", help="skip the PCIe-inclusive ndfft_exec (host arrays) side measurement")
    ap.add_argument("--no-xgmi", action="store_true", help="N > 1: skip the scatter / gather / all-to-all measurements over xGMI")
    ap.add_argument("--profile-phase", default="", choices=["", "primary", "warm", "strong"],
                    help="profiling aid (tools/prof_bench.sh): run ONLY this timed region at full length so that rocprofv3's per-kernel "
                         "averages belong to it (the others shrink to one step / are skipped); the printed line is then not a bench result")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="gloo only with --dry (CPU rendezvous check)")
    ap.add_argument("--dry", action="store_true", help="rendezvous + rank count only, no GPU work (CPU test of the launch path)")
    ap.add_argument("--dist", action="store_true", help="initialise torch.distributed (RCCL) even at world size 1 (path check)")
    args = ap.parse_args()
    if args.profile_phase:                         # the profiled region must run: the others are switched off below
        args.full = True
    if args.blocks is None:
        args.blocks = 7 if args.full else 1
    if not args.full:                              # a plain run: the headline region and nothing else
        args.no_no_ramp = args.no_warm = args.no_other_configs = args.no_host_api = args.no_xgmi = args.no_cpu_baseline = True
        args.strong_steps = 0
    primary_steps = args.steps
    primary_blocks = warm_blocks = max(1, args.blocks)
    args.cold_pairs = max(2, args.cold_pairs)
    if args.profile_phase:
        args.no_cpu_baseline = args.no_host_api = args.no_xgmi = args.no_other_configs = True
        if args.profile_phase != "primary":
            primary_steps = 1; primary_blocks = 1; args.warmup = 1; args.ramp_ms = 0.0
        if args.profile_phase != "warm":
            args.no_warm = True
        if args.profile_phase != "strong":
            args.strong_steps = 0
        elif args.strong_steps < args.steps:
            args.strong_steps = args.steps

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))

    if "OMP_NUM_THREADS" not in os.environ:        # before libgomp is loaded (torch, the oracle): see usable_cpus()
        os.environ["OMP_NUM_THREADS"] = str(usable_cpus())

    import numpy as np
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(args.gpus, 1):
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: trusting the launcher", file=sys.stderr)
    use_dist = world > 1 or args.dist or args.dry
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1"); os.environ.setdefault("LOCAL_RANK", "0")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if args.dry:
        dist.init_process_group(args.backend if args.backend == "gloo" or torch.cuda.is_available() else "gloo")
        one = torch.ones(1, dtype=torch.int64)
        dist.all_reduce(one)
        if rank == 0:
            print(json.dumps({"metric": "dry run (rendezvous only)", "value": None, "n_gpus": dist.get_world_size(),
                              "ranks_seen": int(one[0]), "steps": 0, "warmup": 0}))
        dist.destroy_process_group()
        return

    import synth
    from ndrustfft_amd import FftHandler, _lib, ndfft

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if use_dist:
        dist.init_process_group("nccl", device_id=dev)
    ngpu = max(world, 1)
    ranks_seen = 1
    if use_dist:
        one = torch.ones(1, dtype=torch.int64, device=dev)
        dist.all_reduce(one)                        # an RCCL collective: every rank is really there
        ranks_seen = int(one[0])

    # which physical GPU each rank drives (name, PCI bus id, UUID): a SCALE run must show N DISTINCT devices
    me = {"rank": rank, "local_rank": local_rank}
    try:
        pr = torch.cuda.get_device_properties(local_rank)
        me.update({"name": pr.name,
                   "pci": "%04x:%02x:%02x" % (int(getattr(pr, "pci_domain_id", 0)), int(getattr(pr, "pci_bus_id", 0)), int(getattr(pr, "pci_device_id", 0))),
                   "uuid": str(getattr(pr, "uuid", "")),
                   "hip_visible_devices": os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES", ""))})
    except Exception as ex:                              # a diagnostic must never cost the bench line
        me["error"] = repr(ex)[:120]
    devices = [me]
    if use_dist and world > 1:
        try:
            got = [None] * world
            dist.all_gather_object(got, me)
            devices = got
        except Exception as ex:
            me["gather_error"] = repr(ex)[:120]

    n = args.n
    rows = args.rows
    h = FftHandler(n)
    lib = _lib.default()

    def sync_all():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, steps):
        """EXACTLY `steps` calls of fn(i) between barrier + synchronize; (wall s, device ms), max over ranks."""
        sync_all()
        ev0 = torch.cuda.Event(enable_timing=True); ev1 = torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record()                                # torch's current stream == the stream ndfft_exec_device launches on
        for i in range(steps):
            fn(i)
        ev1.record()
        sync_all()
        el = time.perf_counter() - t0
        dev_ms = ev0.elapsed_time(ev1)
        if use_dist:
            t = torch.tensor([el, dev_ms], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el, dev_ms = float(t[0]), float(t[1])
        return el, dev_ms

    def timed_blocks(fn, steps, nblocks):
        """nblocks blocks of EXACTLY `steps` calls each; returns (median block (wall s, device ms), summary dict)."""
        res = [timed(fn, steps) for _ in range(nblocks)]
        by_wall = sorted(res, key=lambda r: r[0])
        med = by_wall[len(by_wall) // 2]
        devs = sorted(r[1] for r in res)

        def mmm(vals, scale):
            return {"min": round(vals[0] * scale, 5), "median": round(vals[len(vals) // 2] * scale, 5), "max": round(vals[-1] * scale, 5)}
        return med, {"n": nblocks, "steps_each": steps,
                     "ms_per_step": mmm([r[0] for r in by_wall], 1e3 / steps),
                     "avg_launch_us": mmm(devs, 1e3 / steps)}

    # ------------------------------------------------------------------ primary: cfg2 per GPU, HBM-sourced (rotating pairs)
    # device-resident shard: rank r holds global rows [r*rows, (r+1)*rows) of the (ngpu*rows) x n array; pair p > 0 holds other
    # synthetic arrays of the same shape (the stream continued)
    x = synth.complex_array((rows, n), offset=rank * rows * n)
    xd = torch.from_numpy(x).to(dev)
    yd = torch.empty_like(xd)
    pairs = [(xd, yd)]
    for p in range(1, args.cold_pairs):
        xi = synth.complex_array_torch((rows, n), dev, offset=(rank + p * ngpu) * rows * n)
        pairs.append((xi, torch.empty_like(xi)))
    counter = [0]

    def step(_i=0):
        a, b = pairs[counter[0] % len(pairs)]
        counter[0] += 1
        ndfft(a, b, h, 1)

    def warm_step(_i=0):
        ndfft(xd, yd, h, 1)

    # Untimed preamble: the GPU's clocks need ~30-40 ms of sustained work to reach their steady state
    # (tools/kbench creep: 95-107 us per launch for the first ~400 launches, 85 us afterwards), far
    # longer than W launches of a ~90 us kernel.  Keep the device busy for --ramp-ms first, then do
    # the W warm-up steps the contract asks for.  Nothing in here is timed.
    # On a fresh box the settling can take longer than a fixed time: keep going (at most 3 s) until three consecutive 50-step batches
    # agree within 1 %.
    # What a caller who does NOT pre-heat the clocks sees (round 5): the contract's W warm-up steps from an idle GPU, then 20 timed
    # steps, once -- measured before the ramp and reported beside the ramped figure as `no_ramp` (never `value`).
    no_ramp = None
    if not args.profile_phase and not args.no_no_ramp:
        for _ in range(max(args.warmup, 1)):
            step()
        nr_el, nr_ms = timed(step, 20)
        no_ramp = {"what": f"{max(args.warmup, 1)} warm-up steps from an idle GPU, then 20 timed steps, once, BEFORE the clock ramp (same rotating pairs)",
                   "steps": 20, "ms_per_step": round(nr_el / 20 * 1e3, 5), "avg_launch_us": round(nr_ms / 20 * 1e3, 2),
                   "frac": round(2 * rows * n * 16 / (nr_ms / 1e3 / 20) / 1e9 / HBM_PEAK_GBS, 4)}
    t_ramp = time.perf_counter(); hist = []; ramp_steps = 0; ramped_ms = 0.0; settled = False
    while args.ramp_ms > 0:
        tb = time.perf_counter()
        for _ in range(50):
            step()
        torch.cuda.synchronize()
        ramp_steps += 50
        hist.append(time.perf_counter() - tb)
        ramped_ms = (time.perf_counter() - t_ramp) * 1e3
        settled = len(hist) >= 3 and max(hist[-3:]) <= 1.01 * min(hist[-3:])
        if (ramped_ms >= args.ramp_ms and settled) or ramped_ms >= max(3000.0, args.ramp_ms):
            break
    counter[0] = 0                                 # the ramp's length varies: restart the rotation so that every timed step's pair is fixed by the arguments
    for _ in range(max(args.warmup, 2 * len(pairs) if not args.profile_phase or args.profile_phase == "primary" else 1)):
        step()
    (el, dev_ms), blocks = timed_blocks(step, primary_steps, primary_blocks)
    path = lib.last_path()
    policy = lib.last_input_policy()

    # --dump-outputs: a fixed seeded sample of rows of the output of the last timed step (not timed), 16 MiB over all ranks
    if args.dump_outputs:
        last_out = pairs[(counter[0] - 1) % len(pairs)][1]
        count = min(rows, max(1, (16 << 20) // ngpu // (n * 16)))
        sel = np.sort(np.random.default_rng(20241008).choice(rows, count, replace=False))
        sample = torch.view_as_real(last_out.index_select(0, torch.from_numpy(sel).to(dev))).cpu().numpy()
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "ndfft_out.npy" if rank == 0 else f"ndfft_out_rank{rank}.npy"), sample.astype(np.float64))

    # quick self-check of the timed outputs on a few lanes against numpy's FFT (not timed; the oracle is only used by
    # the cpu_baseline leg below and by the tests): pair 0 and the last pair
    if rank == 0 and args.full:
        torch.cuda.synchronize()
        for a, b in (pairs[0], pairs[-1]) if primary_steps * primary_blocks + args.warmup >= len(pairs) else (pairs[0],):
            yo = np.fft.fft(a[:4].cpu().numpy(), axis=1)
            err = np.abs(b[:4].cpu().numpy() - yo).max() / np.abs(yo).max()
            assert err < 1e-10, f"bench output differs from numpy.fft: {err}"

    bytes_per_launch = 2 * rows * n * 16               # 32 B/point = one read + one write of c128
    kern_s = dev_ms / 1e3 / primary_steps              # average launch duration on the launch stream (HIP events), median block

    # ------------------------------------------------------------------ warm: ONE pair re-used every step (Infinity-Cache assisted)
    warm = None
    if not args.no_warm:
        for _ in range(5):
            warm_step()
        (w_el, w_ms), w_blocks = timed_blocks(warm_step, args.steps, warm_blocks)
        w_kern = w_ms / 1e3 / args.steps
        warm = {"what": "the same call on ONE (in, out) pair re-used every step: the 256 MiB Infinity Cache serves part of the re-read input "
                        "(FETCH_SIZE counts those hits) -- not an HBM-sourced number",
                "avg_launch_us": round(w_kern * 1e6, 2), "achieved": round(bytes_per_launch / w_kern / 1e9, 1),
                "ms_per_step": round(w_el / args.steps * 1e3, 5),
                "value": round(ngpu * rows * n * args.steps / w_el / 1e9, 3), "blocks": w_blocks,
                "input_policy": lib.last_input_policy()}
    del pairs[1:]

    # ------------------------------------------------------------------ strong scaling: cfg5 = 65536 x 4096 split in N
    strong = None
    if args.strong_steps > 0 and CFG5_ROWS % ngpu == 0:
        srows = CFG5_ROWS // ngpu
        xs = synth.complex_array_torch((srows, n), dev, offset=rank * srows * n)
        ys = torch.empty_like(xs)

        def strong_step(_i=0):
            ndfft(xs, ys, h, 1)
        for _ in range(3):
            strong_step()
        (s_el, s_ms), s_blocks = timed_blocks(strong_step, args.strong_steps, 1 if args.profile_phase else min(3, max(1, args.blocks)))
        s_bytes = 2 * srows * n * 16
        s_kern = s_ms / 1e3 / args.strong_steps
        if rank == 0:
            xo = synth.complex_array((2, n))            # rows 0, 1 of the global array
            err = np.abs(ys[:2].cpu().numpy() - np.fft.fft(xo, axis=1)).max() / np.abs(np.fft.fft(xo, axis=1)).max()
            assert err < 1e-10, f"cfg5 output differs from numpy.fft: {err}"
        strong = {"workload": f"ndfft axis=1 on {CFG5_ROWS}x{n} Complex<f64> (BASELINE configs[4]), {srows} rows per GPU, device-resident",
                  "scaling": "strong", "steps": args.strong_steps, "rows_per_gpu": srows,
                  "value": round(CFG5_ROWS * n * args.strong_steps / s_el / 1e9, 3), "unit": "GFFT-points/s",
                  "ms_per_step": round(s_el / args.strong_steps * 1e3, 5),
                  "avg_launch_us": round(s_kern * 1e6, 2),
                  "per_gpu_achieved_GBs": round(s_bytes / s_kern / 1e9, 1),
                  "per_gpu_frac": round(s_bytes / s_kern / 1e9 / HBM_PEAK_GBS, 4), "blocks": s_blocks}
        del xs, ys

    # ------------------------------------------------------------------ the other single-GPU configs of BASELINE.json, N = 1 only
    others = None
    if ngpu == 1 and not args.no_other_configs:
        try:
            others = other_configs_block(torch, np, synth, lib, dev, timed)
        except AssertionError:
            raise                                                             # a wrong result must fail the bench
        except Exception as ex:                                               # anything else must not cost the primary line
            others = [{"error": repr(ex)[:300]}]

    # ------------------------------------------------------------------ N > 1: the data movement of SURVEY 8e / 8f rank 3 over xGMI
    # (never part of `value`: lanes that are born sharded need none of it).  Root scatter and gather of batch slices
    # (point-to-point groups, one slice per link) and the all-to-all re-shard between the two axis passes of a sharded
    # fft2; GB/s per link against the ~153 GB/s an xGMI link carries, and a correctness check of each.
    xgmi = None
    if use_dist and ngpu > 1 and not args.no_xgmi:
        try:
            xgmi = xgmi_block(dist, torch, dev, rank, ngpu, n, ndfft, FftHandler, sync_all)
        except Exception as ex:                                           # never lose the bench line to this side measurement
            xgmi = {"error": repr(ex)[:300]}

    # ------------------------------------------------------------------ host-array API (PCIe both ways), N = 1 only
    host_api = None
    if rank == 0 and ngpu == 1 and not args.no_host_api:
        # the caller's own pageable arrays (numpy = malloc memory), as the reference's signature hands them over (src/lib.rs:105-115).
        # Default configuration: pinned bounce buffers filled by a host copy pool (`ms_per_call`).  With the opt-in registration cache
        # (ndfft_host_reg_cache: a caller that owns its arrays' lifetimes) the library registers an array on its second use and later
        # calls DMA straight from / to it (`registered`).  Neither is `value`.
        yh = np.empty_like(x)
        t0 = time.perf_counter(); ndfft(x, yh, h, 1); first = time.perf_counter() - t0
        reps = max(3, args.host_reps); hts = []
        for _ in range(reps):
            t0 = time.perf_counter(); ndfft(x, yh, h, 1); hts.append(time.perf_counter() - t0)
        hts.sort(); hel = hts[len(hts) // 2]
        assert np.abs(yh[:4] - np.fft.fft(x[:4], axis=1)).max() / np.abs(yh[:4]).max() < 1e-10
        lib.check(lib.c.ndfft_host_reg_cache(4 << 30))
        t0 = time.perf_counter(); ndfft(x, yh, h, 1); r1 = time.perf_counter() - t0      # first sighting: bounce buffers
        t0 = time.perf_counter(); ndfft(x, yh, h, 1); r2 = time.perf_counter() - t0      # second sighting: registers both arrays
        rts = []
        for _ in range(reps):
            t0 = time.perf_counter(); ndfft(x, yh, h, 1); rts.append(time.perf_counter() - t0)
        rts.sort(); rel = rts[len(rts) // 2]
        assert np.abs(yh[:4] - np.fft.fft(x[:4], axis=1)).max() / np.abs(yh[:4]).max() < 1e-10
        lib.check(lib.c.ndfft_host_reg_cache(0))                                          # drops the registrations before numpy frees the arrays
        host_api = {"what": "ndfft_exec on pageable host arrays (upload + transform + download), never `value`",
                    "ms_per_call": round(hel * 1e3, 3), "value": round(rows * n / hel / 1e9, 3), "unit": "GFFT-points/s",
                    "reps": reps, "ms_min": round(hts[0] * 1e3, 3), "ms_median": round(hel * 1e3, 3), "ms_max": round(hts[-1] * 1e3, 3),
                    "first_call_ms": round(first * 1e3, 3),
                    "registered": {"what": "opt-in registration cache (ndfft_host_reg_cache): same caller arrays, registered by the library on their second use",
                                   "steady_state_ms_per_call": round(rel * 1e3, 3), "value": round(rows * n / rel / 1e9, 3),
                                   "ms_min": round(rts[0] * 1e3, 3), "ms_max": round(rts[-1] * 1e3, 3),
                                   "first_sighting_ms": round(r1 * 1e3, 3), "registering_call_ms": round(r2 * 1e3, 3)},
                    "kernel_path": lib.last_path()}

    if rank == 0:
        points = ngpu * rows * n * primary_steps
        achieved = bytes_per_launch / kern_s / 1e9
        traffic = None; traffic_src = None
        tj = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tj):
            try:
                tdata = json.load(open(tj))
                traffic = tdata.get(f"{rows}x{n}")
                # the counters were collected for a particular kernel text: if the kernel sources have changed since, say so instead of
                # quoting stale bytes (tools/pmc_source_sha.py prints the hash that tools/prof_bench.sh stores beside the counters)
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import pmc_source_sha
                if tdata.get("kernel_source_sha") != pmc_source_sha.sha():
                    traffic = None
                traffic_src = tdata.get("source", "profiles/pmc_traffic.json (tools/pmc_traffic.sh: separate FETCH_SIZE / WRITE_SIZE "
                                                  "--pmc passes of this bench command, x2 gfx950 read correction)")
            except Exception:
                traffic = None
        cold_traffic = tdata.get("4096x4096_cold_rotating") if (traffic is not None and rows == 4096 and n == 4096) else None
        roof = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": cold_traffic,
                "traffic_source": traffic_src if cold_traffic is not None else "no PMC run on record for the current kernel sources (profiles/pmc_traffic.json is for older kernel text)",
                "traffic_note": "PMC bytes from an EARLIER profiling run of this command (not measured by this process)" if cold_traffic is not None else None,
                "kernel": "k_pow2<double,4096>", "algorithmic_bytes_per_launch": bytes_per_launch,
                "avg_launch_us": round(kern_s * 1e6, 2),
                # the same fraction from the line's one wall-clock quantity: algorithmic bytes / ms_per_step (includes the host's launch gaps)
                "frac_from_ms_per_step": round(bytes_per_launch / (el / primary_steps) / 1e9 / HBM_PEAK_GBS, 4),
                "source": f"HBM: {args.cold_pairs} rotating (in, out) pairs, footprint {args.cold_pairs * bytes_per_launch} B >> the 256 MiB Infinity Cache; "
                          "median of `blocks`",
                "pairs": args.cold_pairs, "footprint_bytes": args.cold_pairs * bytes_per_launch, "input_policy": policy,
                "blocks": blocks}
        roof["frac_cold"] = roof["frac"]               # the name rounds 2-3 used for this same region
        if warm:
            roof["frac_warm"] = round(warm["achieved"] / HBM_PEAK_GBS, 4)
            if traffic is not None:
                warm["traffic"] = traffic; warm["traffic_note"] = "FETCH_SIZE counts Infinity-Cache hits too"
            roof["warm"] = warm
        if strong and traffic is not None and ngpu == 1 and n == 4096:
            strong["traffic"] = tdata.get("65536x4096"); strong["traffic_source"] = traffic_src
        out = {
            "metric": "GFFT-points/s, batched 1-D C2C FFT f64 along the contiguous axis (+ achieved HBM GB/s vs roofline)",
            "value": round(points / el / 1e9, 3), "unit": "GFFT-points/s",
            "n_gpus": ngpu, "ranks_seen": ranks_seen, "devices": devices, "distinct_devices": len({d.get("uuid") or d.get("pci") or d["rank"] for d in devices}),
            "steps": primary_steps, "warmup": args.warmup,
            "ramp": {"what": "untimed launches of the same step BEFORE the W warm-up steps, until >= --ramp-ms have passed and three consecutive 50-step "
                             "batches agree within 1 % (at most 3 s): the GPU's clocks settle; `no_ramp` is the same measurement without it",
                     "ramp_ms_requested": args.ramp_ms, "ramp_ms_actual": round(ramped_ms, 1), "ramp_steps": ramp_steps, "settled": bool(settled)},
            "no_ramp": no_ramp,
            "ms_per_step": round(el / primary_steps * 1e3, 5),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "blocks": blocks["n"],
            "config": {"workload": f"ndfft axis=1 on {ngpu * rows}x{n} Complex<f64> "
                                   f"({'BASELINE configs[1] per GPU' if rows == 4096 else str(rows) + ' rows per GPU'}), "
                                   f"device-resident in HBM ({args.cold_pairs} rotating array pairs), splitmix64 U[-1,1) seed 20241008",
                       "lanes_per_gpu": rows, "lane_len": n, "kernel_path": path,
                       "sharding": "none" if ngpu == 1 else f"lanes split in {ngpu} contiguous blocks, one per GPU, no collective in the timed region"},
            "roofline": roof,
        }
        if args.profile_phase:
            out["profile_phase"] = args.profile_phase + " (profiling run: not a bench result)"
        if strong:
            out["strong_cfg5"] = strong
        if others:
            out["other_configs"] = others
        if xgmi:
            out["xgmi"] = xgmi
        if host_api:
            out["host_api"] = host_api
        if not args.no_cpu_baseline and ngpu == 1:
            out["cpu_baseline"] = cpu_baseline(n, min(rows, 4096))
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
