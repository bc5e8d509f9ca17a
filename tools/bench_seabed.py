#!/usr/bin/env python3
"""Seabed-line estimate of a memmap echogram without a stored seabed.npy, 1000 range rows x 20000 pings x 4 frequencies of
synthetic sv (320 MB of float32): three times, one JSON line.

  host_s    -- the estimate on the host through a reader stand-in: tools.make_golden_seabed.host_seabed, the numpy
               restatement of the reference's Echogram.get_seabed (data_reader.py:433-507; vectorised numpy instead of its
               scipy convolve2d passes and its per-ping Python loop, so it flatters the host), one run;
  gpu_s     -- tiled_inference.estimate_seabed_memm on the same stand-in: chunked upload of the host planes, transpose,
               crimac_seabed_columns, download, finishing step; host clock, ends in a synchronise (the download);
               one warm-up call, then one run;
  kernel_ms -- crimac_seabed_columns alone on the resident [F, pings, range] tensor: device events, median of --reps.
The two results are compared ping by ping (``equal``)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from crimac_classifiers_unet_amd import tiled_inference as ti  # noqa: E402
from tools.make_golden_seabed import EchogramStandIn, host_seabed  # noqa: E402


def synth(R, P, F, seed):
    """Log-uniform sv 1e-8 .. 1e-5, an undulating 1e-2 bottom per frequency, NaN / inf samples, two drop-out runs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    data = np.power(10.0, rng.uniform(-8.0, -5.0, size=(R, P, F)).astype(np.float32)).astype(np.float32)
    x = np.arange(P)[:, None]
    bottom = (0.7 * R + 0.12 * R * np.sin(x / 230.0) + rng.integers(-2, 3, size=(P, F))).astype(np.int64)
    data[np.arange(R)[:, None, None] >= bottom[None]] += np.float32(1e-2)
    w = max(1, P // 500)                                          # (drop-outs rarer than 1 ping in 65 stay below -8)
    data[:, P // 4:P // 4 + w, :2] = rng.uniform(1e-14, 1e-11, size=(R, w, min(F, 2))).astype(np.float32)
    data[:, P - w:, 1:] = rng.uniform(1e-14, 1e-11, size=(R, w, F - 1)).astype(np.float32)
    bad = rng.integers(0, [R, P, F], size=(R * P * F // 5000, 3))
    data[bad[:, 0], bad[:, 1], bad[:, 2]] = np.where(rng.random(len(bad)) < 0.5, np.nan, np.inf).astype(np.float32)
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[1000, 20000, 4], metavar=("RANGE", "PINGS", "FREQS"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_seabed: needs a GPU")
    R, P, F = args.shape
    data = synth(R, P, F, args.seed)
    eg = EchogramStandIn(data)

    t0 = time.perf_counter()
    host = host_seabed(eg.data_numpy())
    host_s = time.perf_counter() - t0

    ti.estimate_seabed_memm(eg)                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gpu = ti.estimate_seabed_memm(eg)
    gpu_s = time.perf_counter() - t0

    res = torch.from_numpy(np.ascontiguousarray(data.transpose(2, 1, 0))).cuda()
    idx = torch.empty((F, P), dtype=torch.int32, device="cuda")
    colmax = torch.empty((F, P), dtype=torch.float32, device="cuda")
    n = ti.seabed_rows(R)[0]
    ti.seabed_columns(res, 0, 0, n, idx, colmax)
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ti.seabed_columns(res, 0, 0, n, idx, colmax)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    kernel_ms = float(np.median(times))
    print(json.dumps({"shape": [R, P, F], "host_s": round(host_s, 3), "gpu_s": round(gpu_s, 4),
                      "kernel_ms": round(kernel_ms, 4), "kernel_ms_min_max": [round(min(times), 4), round(max(times), 4)],
                      "kernel_read_gbps": round(data.nbytes / kernel_ms / 1e6, 1),
                      "host_over_gpu": round(host_s / gpu_s, 1), "equal": bool(np.array_equal(host, gpu)),
                      "pings_differing": int((host != gpu).sum()), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
