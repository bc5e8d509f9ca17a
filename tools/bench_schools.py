#!/usr/bin/env python3
"""The predicted schools of a whole survey, patches/s of the two ways to get them on the same synthetic survey and model:

  A  host    -- tiled_inference.predict_survey(out_dtype=np.float16), every chunk downloaded, thresholded, labelled with
                scipy.ndimage.label and summed in numpy against the sv read a second time from the reader, the chunk seams
                joined by merge_school_chunks: what a user does today;
  B  device  -- tiled_inference.detect_schools_survey: crimac_schools_label / crimac_schools_stats per chunk, the school
                table and two label columns downloaded per chunk, the same seam merge;
  C  predict -- leg A's prediction part alone (the chunks are taken and dropped).

Survey, model and protocol of tools/bench_integrate.py: synth.SyntheticSurveyReader (sv [4, pings, 1024] fp32, flat seabed
900, NaN / inf samples), patch 256, overlap 20, h3p inference; the legs alternate in one process (A, B, C per round) after
one warm-up each; the figure of a leg is the median of its rounds.  Leg B is checked against leg A before anything is
printed: every integer field equal, every sv_sum within n * 2^-52 * ref (n = the school's sv_pixels).  No rate is fixed
in advance: the line states device_over_host (A / B, medians) next to the (max - min) / median spread of each leg's own
passes, and device_over_predict_alone (C / B).  Wall times of whole survey passes: the kernels' own time is not measured
here.  The last line is one JSON object; --out writes it to a file as well.

--score measures the schools SCORED against the annotations instead, same survey and protocol:

  A  host    -- leg A above, plus per chunk a second scipy.ndimage.label on the annotation ids of the class (read from the
                reader), a numpy pair count of (predicted, annotated) pixels with their sv, and the pixels on ignored ids;
                merge_school_chunks(index=True) and merge_school_overlaps join the chunks;
  B  device  -- tiled_inference.score_schools_survey;
  C  detect  -- tiled_inference.detect_schools_survey alone (leg B above).

Leg B is checked against leg A (both tables, the pairs, the ignored pixels: integers equal, sums within the bound); the line
states device_over_host (A / B) and score_over_detect (B / C: the cost of scoring over detection alone)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402
from scipy import ndimage  # noqa: E402

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import synth, tiled_inference as ti  # noqa: E402

INT_FIELDS = ("anchor", "pixels", "bbox", "row_sum", "ping_sum", "sv_pixels")


def host_chunk(plane, sv, thr, connectivity, min_pixels, keep_left, keep_right, start_ping, frequencies, klass):
    """The chunk-local table of one downloaded class plane [R, P] float16; ``sv`` [F, P, R] as the reader gives it."""
    mask = plane.astype(np.float32) >= np.float32(thr)
    R, P = mask.shape
    lab, n = ndimage.label(mask, structure=np.ones((3, 3)) if connectivity == 8 else None)
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    first = np.full(n, flat.size, dtype=np.int64)
    np.minimum.at(first, flat[idx] - 1, idx)                           # the anchor of every component
    rank = np.empty(n, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(n)                             # ascending anchor order
    of, rows, pings = rank[flat[idx] - 1], idx // P, idx % P
    pixels = np.bincount(of, minlength=n).astype(np.int64)
    keep = pixels >= min_pixels
    if keep_left:
        keep[of[pings == 0]] = True
    if keep_right:
        keep[of[pings == P - 1]] = True
    new = np.full(n + 1, -1, dtype=np.int64)
    new[:n][keep] = np.arange(keep.sum())
    edge = new[np.concatenate([[n], rank])[lab]]                       # [R, P] school index, -1 background / dropped
    of = new[of]
    sel = of >= 0
    of, rows, pings = of[sel], rows[sel], pings[sel]
    K, F = int(keep.sum()), sv.shape[0]

    def ext(fn, init, v):
        a = np.full(K, init, dtype=np.int64)
        fn.at(a, of, v)
        return a
    sv_sum, sv_pixels = np.zeros((F, K)), np.zeros((F, K), dtype=np.int64)
    for f in range(F):
        x = sv[f].T[rows, pings]
        ok = np.isfinite(x) & (x > 0)
        sv_sum[f] = np.bincount(of[ok], weights=x[ok].astype(np.float64), minlength=K)
        sv_pixels[f] = np.bincount(of[ok], minlength=K)
    big = np.iinfo(np.int32).max
    return {"anchor": np.sort(first)[keep], "pixels": pixels[keep],
            "bbox": np.stack([ext(np.minimum, big, rows), ext(np.maximum, 0, rows + 1), ext(np.minimum, big, pings),
                              ext(np.maximum, 0, pings + 1)], axis=1),
            "row_sum": ext(np.add, 0, rows), "ping_sum": ext(np.add, 0, pings), "sv_sum": sv_sum, "sv_pixels": sv_pixels,
            "edges": np.stack([edge[:, 0], edge[:, -1]]), "start_ping": start_ping, "n_pings": P, "n_range": R,
            "class": klass, "frequencies": frequencies, "rows": edge}


def host_pairs(pred, ann, sv):
    """The chunk-local overlap rows of two host_chunk tables (their ``"rows"`` planes), one row per pair: a numpy pair count."""
    ra, rb = pred["rows"], ann["rows"]
    rr, pp = np.nonzero((ra >= 0) & (rb >= 0))
    nb = max(len(ann["pixels"]), 1)
    keys, of = np.unique(ra[rr, pp] * nb + rb[rr, pp], return_inverse=True)
    M, F = len(keys), sv.shape[0]
    sv_sum, sv_pixels = np.zeros((F, M)), np.zeros((F, M), dtype=np.int64)
    for f in range(F):
        x = sv[f].T[rr, pp]
        ok = np.isfinite(x) & (x > 0)
        sv_sum[f] = np.bincount(of[ok], weights=x[ok].astype(np.float64), minlength=M)
        sv_pixels[f] = np.bincount(of[ok], minlength=M)
    return {"pred": keys // nb, "ann": keys % nb, "pixels": np.bincount(of, minlength=M).astype(np.int64), "sv_sum": sv_sum,
            "sv_pixels": sv_pixels}


def compare(got, want, fields):
    """(integer fields equal, sv_sum within n * 2^-52 * ref, the largest error over its bound)."""
    equal = all(np.array_equal(got[f], want[f]) for f in fields)
    if got["sv_sum"].shape != want["sv_sum"].shape:
        return equal, False, 0.0
    err, bound = np.abs(got["sv_sum"] - want["sv_sum"]), want["sv_pixels"] * 2.0 ** -52 * want["sv_sum"]
    return equal, bool((err <= bound).all()), float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pings", type=int, default=16384)
    ap.add_argument("--range", type=int, default=1024)
    ap.add_argument("--preload", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="h3p", help="infer_precision")
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--min-pixels", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--score", action="store_true", help="measure score_schools_survey (see the module docstring)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reader = synth.SyntheticSurveyReader(n_pings=a.pings, n_range=a.range, seabed_index=900, block=4096, schools=40,
                                         bad_frac=1e-4)
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg.update(save_model_params=False, data_mode="zarr", infer_precision=a.precision)
    pipe = pkg.SegPipeUNet(experiment_name="bench", **cfg)
    pipe.model.load_state_dict(synth.synth_state_dict(seed=0))
    pipe.model.to(pipe.device).eval()
    pipe.model_is_loaded = True
    patch, overlap = (256, 256), 20
    spec = ti.SchoolSpec(classes=(1, 2), connectivity=a.connectivity, min_pixels=a.min_pixels).bind(pipe.frequencies)
    chunks = ti.plan_chunks(0, a.pings, a.preload)
    patches = sum(len(ti.plan_grid(a.range, 900, s, e, patch, overlap)) for s, e in chunks)

    def leg_predict():
        for _ in ti.predict_survey(reader, pipe, patch, overlap, a.batch, a.preload, out_dtype=np.float16):
            pass

    def leg_host():
        tables = {k: [] for k in spec.classes}
        for s, e, out in ti.predict_survey(reader, pipe, patch, overlap, a.batch, a.preload, out_dtype=np.float16):
            sv = reader.get_data_slice(idx_ping=s, n_pings=e - s, frequencies=pipe.frequencies)[list(spec.channels)]
            for k in spec.classes:
                tables[k].append(host_chunk(out[k - 1], sv, spec.thresholds[k - 1], spec.connectivity, spec.min_pixels,
                                            s > 0, e < a.pings, s, spec.frequencies, ti.SCHOOL_CLASSES[k]))
        return {k: ti.merge_school_chunks(tables[k], spec.connectivity, spec.min_pixels) for k in spec.classes}

    def leg_device():
        return ti.detect_schools_survey(reader, pipe, patch, overlap, a.batch, a.preload, spec)

    def leg_host_score():
        chunk_scores = {k: [] for k in spec.classes}
        for s, e, out in ti.predict_survey(reader, pipe, patch, overlap, a.batch, a.preload, out_dtype=np.float16):
            sv = reader.get_data_slice(idx_ping=s, n_pings=e - s, frequencies=pipe.frequencies)[list(spec.channels)]
            ids = np.asarray(reader.get_label_slice(idx_ping=s, n_pings=e - s, return_numpy=True)).T
            ign = (ids != 0) & (ids != 27) & (ids != 1)
            for k in spec.classes:
                tail = (spec.connectivity, spec.min_pixels, s > 0, e < a.pings, s, spec.frequencies, ti.SCHOOL_CLASSES[k])
                pred = host_chunk(out[k - 1], sv, spec.thresholds[k - 1], *tail)
                ann = host_chunk((ids == ti.SCHOOL_IDS[k]).astype(np.float16), sv, 0.5, *tail)
                on = pred["rows"][(pred["rows"] >= 0) & ign]
                chunk_scores[k].append({"predicted": pred, "annotated": ann, "overlaps": host_pairs(pred, ann, sv),
                                        "ignored_pixels": np.bincount(on, minlength=len(pred["pixels"])).astype(np.int64)})
        return {k: ti._merge_school_scores(chunk_scores[k], spec) for k in spec.classes}

    def leg_device_score():
        return ti.score_schools_survey(reader, pipe, patch, overlap, a.batch, a.preload, spec)

    if a.score:
        return bench_score(a, spec, patches, len(chunks), {"host": leg_host_score, "device": leg_device_score, "detect": leg_device})
    legs = {"host": leg_host, "device": leg_device, "predict": leg_predict}
    times, last = run_legs(legs, a.rounds)
    ints_equal, within, worst = True, True, 0.0
    for k in spec.classes:
        equal, inside, ratio = compare(last["device"][k], last["host"][k], INT_FIELDS)
        ints_equal, within, worst = ints_equal and equal, within and inside, max(worst, ratio)
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()}
    line = {
        "bench": "detect_schools_survey", "pings": a.pings, "range": a.range, "preload": a.preload, "batch": a.batch,
        "precision": a.precision, "connectivity": a.connectivity, "min_pixels": a.min_pixels, "classes": list(spec.classes),
        "patches": patches, "chunks": len(chunks), "rounds": a.rounds,
        "seconds": {k: [round(t, 4) for t in v] for k, v in times.items()},
        "patches_per_s": {k: round(patches / t, 1) for k, t in med.items()}, "spread": spread,
        "device_over_host": round(med["host"] / med["device"], 4),
        "device_over_predict_alone": round(med["predict"] / med["device"], 4),
        "integers_equal": bool(ints_equal), "sums_within_bound": bool(within), "largest_error_over_bound": worst,
        "schools": {str(k): int(len(last["device"][k]["pixels"])) for k in spec.classes},
        "school_pixels": {str(k): int(last["device"][k]["pixels"].sum()) for k in spec.classes},
        "largest_box_area": {str(k): int(np.max(np.prod(np.diff(last["device"][k]["bbox"].reshape(-1, 2, 2), axis=2), axis=1),
                                                initial=0)) for k in spec.classes},
        "kernel_time_measured": False,
    }
    assert ints_equal and within, "detect_schools_survey disagrees with the host detector: " + json.dumps(line)
    report(a, legs, patches, med, line)


def run_legs(legs, rounds):
    """Alternating legs in one process, one warm-up round (staging, packed weights): (seconds per leg, the last results)."""
    times, last = {k: [] for k in legs}, {}
    for rnd in range(-1, rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if rnd >= 0:
                times[name].append(time.perf_counter() - t0)
    return times, last


def report(a, legs, patches, med, line):
    for k in legs:
        print(f"{k:8s}: {patches} patches, median {med[k]:.3f} s -> {patches / med[k]:.0f} patches/s", flush=True)
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def bench_score(a, spec, patches, n_chunks, legs):
    times, last = run_legs(legs, a.rounds)
    ints_equal, within, worst = True, True, 0.0
    for k in spec.classes:
        got, want = last["device"][k], last["host"][k]
        checks = [compare(got[side], want[side], INT_FIELDS) for side in ("predicted", "annotated")]
        checks.append(compare(got["overlaps"], want["overlaps"], ("pred", "ann", "pixels", "sv_pixels")))
        ints_equal = ints_equal and all(c[0] for c in checks) and np.array_equal(got["ignored_pixels"], want["ignored_pixels"])
        within = within and all(c[1] for c in checks)
        worst = max([worst] + [c[2] for c in checks])
    med = {k: float(np.median(v)) for k, v in times.items()}
    dev = last["device"]
    scores = {str(k): ti.school_detection_scores(dev[k]) for k in spec.classes}
    line = {
        "bench": "score_schools_survey", "pings": a.pings, "range": a.range, "preload": a.preload, "batch": a.batch,
        "precision": a.precision, "connectivity": a.connectivity, "min_pixels": a.min_pixels, "classes": list(spec.classes),
        "patches": patches, "chunks": n_chunks, "rounds": a.rounds,
        "seconds": {k: [round(t, 4) for t in v] for k, v in times.items()},
        "patches_per_s": {k: round(patches / t, 1) for k, t in med.items()},
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()},
        "device_over_host": round(med["host"] / med["device"], 4),
        "score_over_detect": round(med["device"] / med["detect"], 4),
        "integers_equal": bool(ints_equal), "sums_within_bound": bool(within), "largest_error_over_bound": worst,
        "predicted_schools": {str(k): int(len(dev[k]["predicted"]["pixels"])) for k in spec.classes},
        "annotated_schools": {str(k): int(len(dev[k]["annotated"]["pixels"])) for k in spec.classes},
        "pairs": {str(k): int(len(dev[k]["overlaps"]["pixels"])) for k in spec.classes},
        "ignored_pixels": {str(k): int(dev[k]["ignored_pixels"].sum()) for k in spec.classes},
        "recall_precision_at_0.5": {k: [None if np.isnan(x) else round(x, 6) for x in (v["recall"], v["precision"])]
                                    for k, v in scores.items()},
        "kernel_time_measured": False,
    }
    assert ints_equal and within, "score_schools_survey disagrees with the host scorer: " + json.dumps(line)
    report(a, legs, patches, med, line)


if __name__ == "__main__":
    main()
