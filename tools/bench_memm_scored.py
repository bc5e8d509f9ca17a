#!/usr/bin/env python3
"""Scored echo integration of a memm survey end to end: the evaluation of ``tools/bench_memm_survey_eval.py`` -- the same
200 synthetic echograms, 256 x 256 patches, overlap 20, 'h3p', ``eval_mode`` 'all' -- with every echogram's sv integrated
by annotated and predicted class in the same pass, three ways, in one process, one JSON line.

  packed_set -- ``tiled_inference.evaluate_echograms_memm(..., integration=ScoredIntegrationSet(spec))``;
  loop       -- a Python loop over ``tiled_inference.evaluate_echogram_memm(..., integration=ScoredIntegration(spec))``,
                one holder and one ``result()`` per echogram;
  packed     -- ``evaluate_echograms_memm`` without ``integration``: what the scored integration adds to the packed pass.
One warm-up pass per leg, then ``--passes`` (3) timed passes, the legs ALTERNATING (other work shares the host); host clock
around a whole pass, which ends with the histograms and every echogram's result on the host.  Reported: patches/s (median
pass) of the three legs and the two ratios; the ``pixels`` of packed_set and loop must be equal, per echogram."""
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
from tools.bench_memm_survey import FREQS, OVERLAP, PATCH, make_model, synth_memm_survey  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--echograms", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--ping-bin", type=int, default=100)
    ap.add_argument("--range-bin", type=int, default=50)
    ap.add_argument("--precision", default=None, help="inference precision (default: the package's, 'h3p')")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_memm_scored: needs a GPU")
    egs = synth_memm_survey(args.echograms, args.seed)
    model, kw, _ = make_model("none", args.precision)

    class Pipe:
        frequencies = FREQS
        device = torch.device("cuda")
    pipe = Pipe()
    pipe.model = model.cuda().eval()
    spec = ti.IntegrationSpec(ping_bin=args.ping_bin, range_bin=args.range_bin)
    patches = sum(len(ti.plan_eval_grid(eg.shape[0], eg._seabed, eg.shape[1], PATCH, OVERLAP, memm=True)) for eg in egs)

    def packed_set():
        s = ti.ScoredIntegrationSet(spec)
        hist = ti.evaluate_echograms_memm(iter(egs), pipe, PATCH, OVERLAP, args.batch, integration=s, **kw)
        return hist, [res for _, res in s.results()]

    def loop():
        hist = torch.zeros(2, ti.PR_BINS, dtype=torch.int32, device=pipe.device)
        results = []
        for eg in egs:
            s = ti.ScoredIntegration(spec)
            ti.evaluate_echogram_memm(eg, pipe, PATCH, OVERLAP, args.batch, hist=hist, integration=s, **kw)
            results.append(s.result())
        return ti.finish_histograms(hist), results

    def packed():
        return ti.evaluate_echograms_memm(iter(egs), pipe, PATCH, OVERLAP, args.batch, **kw), None

    legs = (("packed_set", packed_set), ("loop", loop), ("packed", packed))
    # warm-up passes (code objects, allocator, page-locking the staging), and the results of the legs side by side
    warm = {name: leg() for name, leg in legs}
    (h_set, r_set), (h_loop, r_loop), (h_plain, _) = (warm[name] for name, _ in legs)
    assert len(r_set) == len(r_loop) == len(egs)
    assert all(np.array_equal(a["pixels"], b["pixels"]) for a, b in zip(r_set, r_loop)), "packed_set and loop count other pixels"
    sv_set, sv_loop = (sum(r["sv_sum"].sum(axis=(2, 3)) for r in rs) for rs in (r_set, r_loop))
    times = {name: [] for name, _ in legs}
    for _ in range(args.passes):
        for name, leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({
        "echograms": len(egs), "patches": patches, "precision": model.infer_precision, "eval_mode": "all",
        "ping_bin": spec.ping_bin, "range_bin": spec.range_bin, "cells": int(sum(r["pixels"][0, 0].size for r in r_set)),
        **{f"{k}_patches_per_s": round(patches / med[k], 1) for k in med},
        "packed_set_over_loop": round(med["loop"] / med["packed_set"], 3),
        "packed_set_over_packed": round(med["packed"] / med["packed_set"], 3),
        **{f"{k}_pass_s": [round(t, 4) for t in times[k]] for k in times},
        "pixels_equal": True, "counted_pixels": int(sum(int(r["pixels"][:, 2].sum()) for r in r_set)),
        "sv_sum_largest_relative_difference": float(np.max(np.abs(sv_set - sv_loop) / np.maximum(sv_loop, 1e-300))),
        "histograms_identical": bool(all(np.array_equal(a, b) and np.array_equal(a, c)
                                         for a, b, c in zip(h_set, h_loop, h_plain))),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
