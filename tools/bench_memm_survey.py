#!/usr/bin/env python3
"""A memm survey end to end: many small echograms (the reference's default ``data_mode: 'memm'`` layout), two ways, in one
process, one JSON line.

The survey is synthetic and seeded: ``--echograms`` (200) echograms, pings drawn from 500-6000, range from 200-700, four
frequencies of log-uniform sv with NaN / inf samples, schools of annotation ids, an undulating seabed; 256 x 256 patches,
overlap 20, the default inference precision ('h3p').  Every echogram owns contiguous [range, pings] float32 planes, as
the reader's memory maps are.

  loop   -- the per-echogram path: a Python loop over ``tiled_inference.predict_echogram_memm``;
  packed -- ``tiled_inference.predict_echograms_memm``: forward batches packed across echograms, pinned staging, uploads
            and downloads beside the compute.
Both legs: one warm-up pass over the survey, then ``--passes`` (3) timed passes, the legs ALTERNATING (other work shares
the host); host clock around a whole pass, which ends with the last result on the host.  Reported: patches/s (median
pass) of both legs, the ratio, the share of forward batches below 16 patches (where the eval forward loses its two-stream
form) in both, and the largest difference between the two legs' outputs over the whole survey (the bound is one float16
step, 2**-11: batches of another size).

``--meta early|late``: the same survey with metadata vectors (``add_metadata``) and a model that takes them -- all seven
planes as extra input channels (``UNet_Baseline(3, 11)``) or by late injection (``UNet_LateMetInject(3, 4, 7)``); the packed
leg then runs with ``pack_metadata=True``, the loop is what such a model gets without it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import synth  # noqa: E402
from crimac_classifiers_unet_amd import tiled_inference as ti  # noqa: E402
from tools.fake_reader import FakeEchogram  # noqa: E402

FREQS = [18, 38, 120, 200]
PATCH, OVERLAP = (256, 256), 20


def synth_memm_survey(n, seed, pings=(500, 6000), rows=(200, 700)):
    """``n`` echograms cut out of one pool of noise (every echogram a contiguous copy of its own)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pool = np.power(10.0, rng.uniform(-7.5, 0.0, size=(len(FREQS), rows[1], pings[1] + 512)).astype(np.float32))
    pool[0][rng.random(pool.shape[1:]) < 2e-4] = np.nan
    pool[2][rng.random(pool.shape[1:]) < 1e-4] = np.inf
    egs = []
    for i in range(n):
        P, R = int(rng.integers(pings[0], pings[1] + 1)), int(rng.integers(rows[0], rows[1] + 1))
        x0 = int(rng.integers(0, 512))
        sv = np.ascontiguousarray(pool[:, :R, x0:x0 + P])
        labels = np.zeros((R, P), dtype=np.int16)
        for val in (27, 1, 12, -1, 27, 1):
            for _ in range(3):
                px, py = int(rng.integers(0, P - 40)), int(rng.integers(0, R - 30))
                labels[py:py + int(rng.integers(6, 30)), px:px + int(rng.integers(8, 40))] = val
        x = np.arange(P)
        seabed = (0.75 * R + 0.12 * R * np.sin(x / 97.0 + i) + 0.03 * R * np.sin(x / 13.0)).astype(np.int64)
        egs.append(FakeEchogram(sv, labels, np.clip(seabed, 40, R - 5), frequencies=FREQS, name=f"echogram_{i:04d}"))
    return egs


def add_metadata(egs, seed):
    """The per-ping vectors and the scalar the metadata planes are built from (data_reader.py:98-100), seeded."""
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for i, eg in enumerate(egs):
        tv = 737000.5 + i + np.cumsum(rng.uniform(5e-6, 9e-6, size=eg.shape[1]))
        eg.portion_of_day_vector = tv % 1
        eg.portion_of_year_scalar = float(rng.uniform(0.3, 0.7))
        eg.time_vector_diff = np.concatenate((np.diff(tv), [tv[-1] - tv[-2]])) / 6e-6 - 1


def make_model(meta, precision):
    """``--meta`` none / early / late -> (the model with synthetic weights, the keywords of both legs, those of the packed)."""
    mc = {k: True for k in ti.META_FLAGS}
    if meta == "early":
        model = pkg.UNet_Baseline(3, len(FREQS) + 7, infer_precision=precision)
        model.load_state_dict(synth.synth_state_dict(seed=0, in_channels=len(FREQS) + 7))
    elif meta == "late":
        model = pkg.UNet_LateMetInject(3, len(FREQS), 7, infer_precision=precision)
        model.load_state_dict(synth.synth_state_dict(seed=0, meta_in_channels=7))
    else:
        model = pkg.UNet_Baseline(3, len(FREQS), infer_precision=precision)
        model.load_state_dict(synth.synth_state_dict(seed=0))
        return model, {}, {}
    return model, dict(meta_channels=mc), dict(pack_metadata=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--echograms", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--precision", default=None, help="inference precision (default: the package's, 'h3p')")
    ap.add_argument("--meta", default="none", choices=["none", "early", "late"], help="metadata model (module docstring)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_memm_survey: needs a GPU")
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

    def loop(keep=None):
        for eg in egs:
            out = ti.predict_echogram_memm(eg, pipe, PATCH, OVERLAP, args.batch, **kw)
            if keep is not None:
                keep.append(out.astype(np.float16))

    stats = {}

    def packed(keep=None):
        for eg, out in ti.predict_echograms_memm(iter(egs), pipe, PATCH, OVERLAP, args.batch, stats=stats, **kw,
                                                 **kw_packed):
            if keep is not None:
                keep.append(out.astype(np.float16))

    # warm-up passes (code objects, allocator, page-locking the staging), and the outputs of the two legs side by side
    a, b = [], []
    loop(a)
    packed(b)
    torch.cuda.synchronize()
    worst, differing, total = 0.0, 0, 0
    for x, y in zip(a, b):
        d = np.abs(x.astype(np.float32) - y.astype(np.float32))
        worst, differing, total = max(worst, float(d.max())), differing + int((d != 0).sum()), total + d.size
    del a, b
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
        "precision": model.infer_precision, "meta": args.meta,
        "loop_patches_per_s": round(patches / med["loop"], 1), "packed_patches_per_s": round(patches / med["packed"], 1),
        "packed_over_loop": round(med["loop"] / med["packed"], 3),
        "loop_pass_s": [round(t, 4) for t in times["loop"]], "packed_pass_s": [round(t, 4) for t in times["packed"]],
        "loop_batches": len(loop_batches), "loop_batches_below_16": small(loop_batches),
        "packed_groups": stats["groups"], "packed_batches": len(stats["batches"]),
        "packed_batches_below_16": small(stats["batches"]), "packed_solo_echograms": stats["solo_echograms"],
        "packed_fallback_echograms": stats["fallback_echograms"],
        "max_abs_difference": worst, "differing_pixel_share": round(differing / max(1, total), 8),
        "synth_s": round(synth_s, 1), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
