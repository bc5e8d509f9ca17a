#!/usr/bin/env python3
"""Time of the PR-histogram kernels alone on an evaluation-like batch: one JSON line, optionally appended to a file.

The batch: 32 x 3 x 256 x 256 fp32 logits, int16 labels; the lower third of every patch below the seabed (-50), 1 % of the
pixels label 1 and 1 % label 2 (anywhere), the rest background; logits such that about 95 % of the pixels above the
seabed have both foreground probabilities in float16 bins 0-3 (a confident background: subnormal probabilities), the other
5 % spread over all of [0, 1].

  a -- ``crimac_pr_histogram`` (sandeel only: the kernel every default path calls);
  b -- ``crimac_pr_histogram_classes`` with mask {1};
  c -- ``crimac_pr_histogram_classes`` with mask {1, 2} -- against 2 x a, the cost of one single-class pass per class.
Each: 5 warm-up launches, then 20 launches timed one by one with stream events; the median is reported, the raw times kept."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from crimac_classifiers_unet_amd import hip  # noqa: E402
from crimac_classifiers_unet_amd.hip import call, ptr  # noqa: E402

SHAPE = (32, 3, 256, 256)
WARMUP, LAUNCHES = 5, 20


def make_batch(seed=0):
    B, ncls, H, W = SHAPE
    rng = np.random.default_rng(seed)
    labels = np.zeros((B, H, W), dtype=np.int16)
    u = rng.random((B, H, W))
    labels[u < 0.01] = 1
    labels[(u >= 0.01) & (u < 0.02)] = 2
    labels[:, H - H // 3:, :] = -50
    # confident background: both foreground logits far below the background's -> float16 subnormals 0 .. 3 (k * 2^-24)
    z = np.zeros((B, ncls, H, W), dtype=np.float32)
    k = rng.integers(0, 4, (B, 2, H, W))
    z[:, 1:] = np.where(k == 0, -40.0, np.log(np.maximum(k, 1) * 2.0 ** -24)).astype(np.float32)
    spread = rng.random((B, H, W)) < 0.05
    z[:, 1:][np.broadcast_to(spread[:, None], (B, 2, H, W))] = rng.normal(0, 4, (int(spread.sum()) * 2)).astype(np.float32)
    return z, labels


def low_share(z, labels):
    """Share of the pixels above the seabed whose two foreground probabilities both round to bins 0-3."""
    e = np.exp(z.astype(np.float64) - z.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True))[:, 1:].astype(np.float16).view(np.uint16)
    above = labels != -50
    return float(((p <= 3).all(1) & above).sum() / above.sum())


def time_launches(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(LAUNCHES):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) * 1e3)            # microseconds
    return out


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              timeout=10).stdout.strip() or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--commit", default=None, help="commit the library was built from (default: git rev-parse, if it answers)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pr_histogram: needs a GPU")
    z, labels = make_batch()
    B, ncls, H, W = SHAPE
    zd, ld = torch.from_numpy(z).cuda(), torch.from_numpy(labels).cuda()
    old = torch.zeros(2, hip.PR_BINS, dtype=torch.int32, device="cuda")
    new = torch.zeros(ncls, 2, hip.PR_BINS, dtype=torch.int32, device="cuda")
    legs = {
        "a_pr_histogram": lambda: call("crimac_pr_histogram", ptr(zd), ncls, ptr(ld), 2, B, H, W, ptr(old[0]), ptr(old[1])),
        "b_classes_mask_1": lambda: call("crimac_pr_histogram_classes", ptr(zd), ncls, ptr(ld), 2, B, H, W, 2, ptr(new)),
        "c_classes_mask_1_2": lambda: call("crimac_pr_histogram_classes", ptr(zd), ncls, ptr(ld), 2, B, H, W, 6, ptr(new)),
    }
    raw = {name: time_launches(fn) for name, fn in legs.items()}
    # the three legs counted the same pixels: row 1 of the per-class kernel is the single-class kernel's result
    old.zero_(), new.zero_()
    legs["a_pr_histogram"](), legs["c_classes_mask_1_2"]()
    med = {k: float(np.median(v)) for k, v in raw.items()}
    line = {"shape": list(SHAPE), "pixels_in_bins_0_3_above_seabed": round(low_share(z, labels), 4),
            "warmup": WARMUP, "launches": LAUNCHES,
            "median_us": {k: round(v, 2) for k, v in med.items()},
            "c_over_2a": round(med["c_classes_mask_1_2"] / (2 * med["a_pr_histogram"]), 4),
            "b_over_a": round(med["b_classes_mask_1"] / med["a_pr_histogram"], 4),
            "row_1_equals_single_class_kernel": bool(torch.equal(new[1], old)),
            "raw_us": {k: [round(t, 2) for t in v] for k, v in raw.items()},
            "device": torch.cuda.get_device_name(0), "commit": args.commit or commit()}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
