#!/usr/bin/env python3
"""Test-set evaluation of a memm survey end to end: many small echograms (the reference's default ``data_mode: 'memm'``
layout), two ways, in one process, one JSON line.

The survey is the synthetic one of ``tools/bench_memm_survey.py``: ``--echograms`` (200) echograms of 500-6000 pings x
200-700 rows, four frequencies, schools of annotation ids, an undulating seabed; 256 x 256 patches, overlap 20, the default
inference precision ('h3p'), ``--eval-mode`` 'all'.

  loop   -- the per-echogram path: a Python loop over ``tiled_inference.evaluate_echogram_memm`` into one histogram;
  packed -- ``tiled_inference.evaluate_echograms_memm``: forward batches packed across echograms, pinned staging, uploads
            beside the compute.
Both legs: one warm-up pass over the survey, then ``--passes`` (3) timed passes, the legs ALTERNATING (other work shares
the host); host clock around a whole pass, which ends with the two histograms on the host.  Reported: patches/s (median
pass) of both legs, the ratio, the share of forward batches below 16 patches (where the eval forward loses its two-stream
form) in both, and whether the two legs' histograms are identical.

``--meta early|late``: the metadata survey and models of ``tools/bench_memm_survey.py``; the packed leg runs with
``pack_metadata=True``, the loop is what such a model gets without it."""
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
from tools.bench_memm_survey import FREQS, OVERLAP, PATCH, add_metadata, make_model, synth_memm_survey  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--echograms", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--eval-mode", default="all", choices=["all", "region", "trace"])
    ap.add_argument("--precision", default=None, help="inference precision (default: the package's, 'h3p')")
    ap.add_argument("--meta", default="none", choices=["none", "early", "late"], help="metadata model (module docstring)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_memm_survey_eval: needs a GPU")
    t0 = time.perf_counter()
    egs = synth_memm_survey(args.echograms, args.seed)
    if args.meta != "none":
        add_metadata(egs, args.seed)
    synth_s = time.perf_counter() - t0
    model, kw, kw_packed = make_model(args.meta, args.precision)

    class Pipe:
        frequencies = FREQS
        device = torch.device("cuda")
    pipe = Pipe()
    pipe.model = model.cuda().eval()
    step = max(args.batch, ti.INTERNAL_BATCH)
    counts = [len(ti.plan_eval_grid(eg.shape[0], eg._seabed, eg.shape[1], PATCH, OVERLAP, memm=True)) for eg in egs]
    loop_batches = [min(step, n - b0) for n in counts for b0 in range(0, n, step)]
    patches = sum(counts)

    def loop():
        hist = torch.zeros(2, ti.PR_BINS, dtype=torch.int32, device=pipe.device)
        for eg in egs:
            ti.evaluate_echogram_memm(eg, pipe, PATCH, OVERLAP, args.batch, eval_mode=args.eval_mode, hist=hist, **kw)
        return ti.finish_histograms(hist)

    stats = {}

    def packed():
        return ti.evaluate_echograms_memm(iter(egs), pipe, PATCH, OVERLAP, args.batch, eval_mode=args.eval_mode, stats=stats,
                                          **kw, **kw_packed)

    # warm-up passes (code objects, allocator, page-locking the staging), and the histograms of the two legs side by side
    a, b = loop(), packed()
    identical = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    moved = int(np.abs(np.cumsum(a[0]) - np.cumsum(b[0])).sum() + np.abs(np.cumsum(a[1]) - np.cumsum(b[1])).sum())
    times = {"loop": [], "packed": []}
    for _ in range(args.passes):
        for name, leg in (("loop", loop), ("packed", packed)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    small = lambda bs: round(sum(1 for p in bs if p < 16) / max(1, len(bs)), 4)                  # noqa: E731
    print(json.dumps({
        "echograms": len(egs), "patches": patches, "pixels": int(sum(eg.shape[0] * eg.shape[1] for eg in egs)),
        "precision": model.infer_precision, "eval_mode": args.eval_mode, "meta": args.meta,
        "loop_patches_per_s": round(patches / med["loop"], 1), "packed_patches_per_s": round(patches / med["packed"], 1),
        "packed_over_loop": round(med["loop"] / med["packed"], 3),
        "loop_pass_s": [round(t, 4) for t in times["loop"]], "packed_pass_s": [round(t, 4) for t in times["packed"]],
        "loop_batches": len(loop_batches), "loop_batches_below_16": small(loop_batches),
        "packed_groups": stats["groups"], "packed_batches": len(stats["batches"]),
        "packed_batches_below_16": small(stats["batches"]), "packed_solo_echograms": stats["solo_echograms"],
        "packed_fallback_echograms": stats["fallback_echograms"],
        "histograms_identical": identical, "valid_pixels": int(a[0].sum() + a[1].sum()), "pixels_in_another_bin": moved,
        "synth_s": round(synth_s, 1), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
