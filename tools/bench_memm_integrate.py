#!/usr/bin/env python3
"""Echo integration of a memm survey, two ways, in one process, one JSON line: the survey, the model and the protocol of
tools/bench_memm_survey.py (200 seeded echograms, 256 x 256 patches, 'h3p'; one warm-up pass per leg, then ``--passes``
timed passes, the legs alternating; host clock around a whole pass, which ends with the last result on the host).

  loop   -- a Python loop over ``tiled_inference.integrate_echogram_memm``;
  packed -- ``tiled_inference.integrate_echograms_memm``: forward batches packed across echograms, one integrate launch per
            echogram after the group's scatters, the results through the pinned ring.

``--layers N`` (default 4; 0: the default surface spec, ``crimac_integrate_classes``) integrates N bottom layers of
``--range-bin`` rows counted from the limit ``seabed + --seabed-offset``.  The two legs' results are compared over the
survey: the share of cells whose counts are equal and the largest relative difference of a sum (the legs run the network
on batches of different sizes, which can move a float16 rounding of a probability and with it a pixel across a
threshold; with a predictor that does not depend on its batch the results are equal, tests/test_gpu_integrate_layers.py)."""
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
    ap.add_argument("--ping-bin", type=int, default=500)
    ap.add_argument("--range-bin", type=int, default=50)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--seabed-offset", type=int, default=-5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_memm_integrate: needs a GPU")
    egs = synth_memm_survey(args.echograms, args.seed)
    model, _, _ = make_model("none", None)

    class Pipe:
        frequencies = FREQS
        device = torch.device("cuda")
    pipe = Pipe()
    pipe.model = model.cuda().eval()
    if args.layers > 0:
        spec = ti.IntegrationSpec(args.ping_bin, args.range_bin, seabed_offset=args.seabed_offset, reference="seabed",
                                  layers=args.layers)
    else:
        spec = ti.IntegrationSpec(args.ping_bin, args.range_bin)
    patches = sum(len(ti.plan_eval_grid(eg.shape[0], eg._seabed, eg.shape[1], PATCH, OVERLAP, memm=True)) for eg in egs)
    stats = {}

    def loop():
        return [ti.integrate_echogram_memm(eg, pipe, PATCH, OVERLAP, args.batch, spec) for eg in egs]

    def packed():
        return [res for _, res in ti.integrate_echograms_memm(iter(egs), pipe, PATCH, OVERLAP, args.batch, spec, stats=stats)]

    a, b = loop(), packed()                                      # warm-up passes, and the two legs' results side by side
    torch.cuda.synchronize()
    cells = equal = 0
    worst = 0.0
    for x, y in zip(a, b):
        cells += x["pixels"].size
        equal += int((x["pixels"] == y["pixels"]).sum())
        both = (x["sv_sum"] > 0) & (y["sv_sum"] > 0)
        if both.any():
            worst = max(worst, float((np.abs(x["sv_sum"] - y["sv_sum"])[both] / x["sv_sum"][both]).max()))
    times = {"loop": [], "packed": []}
    for _ in range(args.passes):
        for name, leg in (("loop", loop), ("packed", packed)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    text = json.dumps({
        "bench": "integrate_echograms_memm", "echograms": len(egs), "patches": patches,
        "pixels": int(sum(eg.shape[0] * eg.shape[1] for eg in egs)), "precision": model.infer_precision,
        "ping_bin": args.ping_bin, "range_bin": args.range_bin, "layers": args.layers,
        "seabed_offset": args.seabed_offset if args.layers > 0 else None,
        "loop_patches_per_s": round(patches / med["loop"], 1), "packed_patches_per_s": round(patches / med["packed"], 1),
        "packed_over_loop": round(med["loop"] / med["packed"], 3),
        "loop_pass_s": [round(t, 4) for t in times["loop"]], "packed_pass_s": [round(t, 4) for t in times["packed"]],
        "packed_groups": stats["groups"], "packed_solo_echograms": stats["solo_echograms"],
        "cells": cells, "cells_with_equal_counts": equal, "largest_relative_sum_difference": worst,
        "device": torch.cuda.get_device_name(0)})
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
