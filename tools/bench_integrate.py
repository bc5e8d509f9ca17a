#!/usr/bin/env python3
"""Echo integration by predicted class over a whole survey, patches/s of the two ways to get it on the same synthetic survey
and model:

  A  host    -- tiled_inference.predict_survey(out_dtype=np.float16), every chunk downloaded, the sv read a second time from
                the reader, transposed, thresholded and binned in numpy: what a user does today;
  A0 predict -- leg A's prediction part alone (the chunks are taken and dropped);
  B  device  -- tiled_inference.integrate_survey: the chunk reduced on the GPU by crimac_integrate_classes, one download of a
                few kilobytes at the end.

Survey: synth.SyntheticSurveyReader (sv [4, pings, 1024] fp32, flat seabed 900, NaN / inf samples), patch 256, overlap 20,
h3p inference.  The legs alternate in one process (A0, A, B per round) after one warm-up each; the figure of a leg is the
median of its rounds.  Leg B is checked against leg A: counts equal, every sum within (n_cell_pixels + 2) * 2^-52 relative
(tests/test_gpu_integrate.py).  The last line is one JSON object; --out writes it to a file as well.

--layers N (> 0) adds the seabed-reference legs to every round, same survey, same protocol:

  L  layers      -- integrate_survey with IntegrationSpec(seabed_offset=--seabed-offset, reference="seabed", layers=N):
                    crimac_integrate_layers; its yardstick is leg B of the same run (the default spec);
  LH host_layers -- predict_survey float16 followed by the numpy bottom-layer integration of every downloaded chunk.

Leg L is checked against leg LH with the same bound, and the JSON line gains layers_over_device (B / L) and
layers_over_host (LH / L).

--edsu adds the EDSU leg to every round, same survey, same process, alternating with leg B:

  E  edsu -- integrate_survey with IntegrationSpec(ping_edges=table): crimac_integrate_edges.  The table is drawn with a
             fixed seed (--edsu-seed): as many cells as leg B has ping bins, widths from 0 to 4 x their mean, the mean equal
             to --ping-bin, a few cells of width 0.  Its yardstick is leg B of the same run: the JSON line gains
             edsu_over_device (B / E, medians) next to device_spread ((max - min) / median of leg B's own passes) -- the
             ratio is not fixed in advance.  After the rounds leg E is checked against one untimed host pass (predict_survey
             float16, numpy binning by the table) with the same bound.  Wall times of whole survey passes: the kernels' own
             time is not measured here.

--freqs 18,38,120,200 adds two legs to every round, same survey, same process, alternating:

  F  freqs      -- integrate_survey with IntegrationSpec(frequency=(18, 38, 120, 200)): ONE pass, crimac_integrate_freqs;
  FL freqs_loop -- the loop of single-frequency integrate_survey calls, one whole pass per frequency: what a user runs
                   today, on the code path of leg B.

After the rounds every frequency slice of leg F is checked against the loop's result for that frequency: counts equal,
every sum BIT-equal.  The JSON line gains freqs_over_loop (FL / F, medians: the claim is > 1 by more than the legs' own
spreads, freqs_spread and freqs_loop_spread = (max - min) / median of each leg's passes) and freqs_over_device (F / B:
what the extra planes cost next to one single-frequency pass).  Wall times of whole survey passes: the kernels' own time
is not measured here."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import synth, tiled_inference as ti  # noqa: E402


def host_chunk(acc, cnt, geo, out, sv, spec, s):
    """One downloaded chunk ``out`` [2, R, e - s] float16 and the reader's ``sv`` [e - s, R] into the host accumulators."""
    R, P = out.shape[1:]
    sv_t = np.ascontiguousarray(sv.T)                                     # [R, P], as the predictions lie
    ok = np.isfinite(sv_t) & (sv_t > 0)
    s64 = np.where(ok, sv_t, 0).astype(np.float64)
    p32 = out.astype(np.float32)
    if spec.mode == "threshold":
        member = p32 >= np.asarray(spec.thresholds, dtype=np.float32)[:, None, None]
        weight = member.astype(np.float64)
    else:
        member = p32 > 0
        weight = np.where(member, p32, 0).astype(np.float64)
    pb = (s + np.arange(P)) // spec.ping_bin
    p_starts = np.nonzero(np.diff(pb, prepend=pb[0] - 1))[0]
    r_starts = np.arange(0, R, spec.range_bin)

    def binned(a):
        return np.add.reduceat(np.add.reduceat(a, r_starts, axis=-2), p_starts, axis=-1).swapaxes(-1, -2)
    cells = slice(int(pb[0]), int(pb[-1]) + 1)
    acc[:, cells] += binned(np.stack([s64 * weight[0], s64 * weight[1], s64]))
    cnt[:, cells] += binned(np.stack([ok & member[0], ok & member[1], ok]).astype(np.int64))
    geo[cells] += binned(np.ones((R, P), dtype=np.int64))


def host_chunk_layers(acc, cnt, geo, out, sv, line, spec, s):
    """``host_chunk`` for a seabed-reference ``spec``: ``line`` [e - s] the reader's seabed rows; layer l of ping p covers
    rows [L - (l + 1) * range_bin, L - l * range_bin) below the limit L = clip(line + seabed_offset, 0, R)."""
    R, P = out.shape[1:]
    sv_t = np.ascontiguousarray(sv.T)
    L = np.clip(np.asarray(line).astype(np.int64) + spec.seabed_offset, 0, R)
    r = np.arange(R)[:, None]
    layer = (L[None, :] - 1 - r) // spec.range_bin
    inside = (r < L[None, :]) & (layer < spec.layers)
    ok = np.isfinite(sv_t) & (sv_t > 0) & inside
    s64 = np.where(ok, sv_t, 0).astype(np.float64)
    p32 = out.astype(np.float32)
    if spec.mode == "threshold":
        member = p32 >= np.asarray(spec.thresholds, dtype=np.float32)[:, None, None]
        weight = member.astype(np.float64)
    else:
        member = p32 > 0
        weight = np.where(member, p32, 0).astype(np.float64)
    n = acc[0].size
    at = np.where(inside, ((s + np.arange(P)) // spec.ping_bin)[None, :] * spec.layers + layer, 0)
    for k, (terms, counted) in enumerate(((s64 * weight[0], ok & member[0]), (s64 * weight[1], ok & member[1]), (s64, ok))):
        acc[k] += np.bincount(at[counted], weights=terms[counted], minlength=n).reshape(acc[k].shape)
        cnt[k] += np.bincount(at[counted], minlength=n).reshape(acc[k].shape)
    geo += np.bincount(at[inside], minlength=n).reshape(geo.shape)


def host_chunk_edges(acc, cnt, geo, out, sv, spec, s):
    """``host_chunk`` for a spec with an edge table: ping s + p lies in the cell pb with edges[pb] <= s + p < edges[pb + 1]."""
    R, P = out.shape[1:]
    edges = spec.ping_edges
    sv_t = np.ascontiguousarray(sv.T)
    g = s + np.arange(P)
    inside = np.broadcast_to(((g >= edges[0]) & (g < edges[-1]))[None, :], (R, P))
    ok = np.isfinite(sv_t) & (sv_t > 0) & inside
    s64 = np.where(ok, sv_t, 0).astype(np.float64)
    p32 = out.astype(np.float32)
    if spec.mode == "threshold":
        member = p32 >= np.asarray(spec.thresholds, dtype=np.float32)[:, None, None]
        weight = member.astype(np.float64)
    else:
        member = p32 > 0
        weight = np.where(member, p32, 0).astype(np.float64)
    n, n_rb = acc[0].size, acc.shape[2]
    pb = np.clip(np.searchsorted(edges, g, "right") - 1, 0, len(edges) - 2)
    at = pb[None, :] * n_rb + (np.arange(R) // spec.range_bin)[:, None]
    for k, (terms, counted) in enumerate(((s64 * weight[0], ok & member[0]), (s64 * weight[1], ok & member[1]), (s64, ok))):
        acc[k] += np.bincount(at[counted], weights=terms[counted], minlength=n).reshape(acc[k].shape)
        cnt[k] += np.bincount(at[counted], minlength=n).reshape(acc[k].shape)
    geo += np.bincount(at[inside], minlength=n).reshape(geo.shape)


def edsu_table(n_pings, ping_bin, seed):
    """An edge table over [0, n_pings) with ceil(n_pings / ping_bin) cells: widths ~ 4 x Beta(1, 3) x the mean (0 .. 4 x the
    mean, mean = n_pings / cells), every 16th cell of width 0."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = -(-n_pings // ping_bin)
    u = rng.beta(1.0, 3.0, size=n)
    u[::16] = 0
    w = np.minimum(u / u.sum() * n_pings, 4.0 * n_pings / n)
    edges = np.rint(np.concatenate([[0.0], np.cumsum(w)])).astype(np.int64)
    edges[-1] = n_pings
    return np.maximum.accumulate(edges)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pings", type=int, default=16384)
    ap.add_argument("--range", type=int, default=1024)
    ap.add_argument("--preload", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="h3p", help="infer_precision")
    ap.add_argument("--ping-bin", type=int, default=500)
    ap.add_argument("--range-bin", type=int, default=50)
    ap.add_argument("--mode", default="threshold")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="> 0: add the seabed-reference legs with this many layers")
    ap.add_argument("--seabed-offset", type=int, default=-5)
    ap.add_argument("--edsu", action="store_true", help="add the EDSU leg: integrate_survey with an edge table")
    ap.add_argument("--edsu-seed", type=int, default=20)
    ap.add_argument("--freqs", default=None, help="comma-separated frequencies: add the one-pass leg and the loop of passes")
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
    spec = ti.IntegrationSpec(a.ping_bin, a.range_bin, mode=a.mode)
    channel = spec.bind(pipe.frequencies).channel
    n_pb, n_rb = spec.bins(a.pings, a.range)
    patches = sum(len(ti.plan_grid(a.range, 900, s, e, patch, overlap)) for s, e in ti.plan_chunks(0, a.pings, a.preload))

    def leg_predict():
        for _ in ti.predict_survey(reader, pipe, patch, overlap, a.batch, a.preload, out_dtype=np.float16):
            pass

    def leg_host():
        acc, cnt = np.zeros((3, n_pb, n_rb)), np.zeros((3, n_pb, n_rb), dtype=np.int64)
        geo = np.zeros((n_pb, n_rb), dtype=np.int64)
        for s, e, out in ti.predict_survey(reader, pipe, patch, overlap, a.batch, a.preload, out_dtype=np.float16):
            sv = reader.get_data_slice(idx_ping=s, n_pings=e - s, frequencies=pipe.frequencies)[channel]
            host_chunk(acc, cnt, geo, out, sv, spec, s)
        return acc, cnt, geo

    def leg_device():
        return ti.integrate_survey(reader, pipe, patch, overlap, a.batch, a.preload, spec)

    legs = {"predict": leg_predict, "host": leg_host, "device": leg_device}
    if a.layers > 0:
        lspec = ti.IntegrationSpec(a.ping_bin, a.range_bin, mode=a.mode, seabed_offset=a.seabed_offset, reference="seabed",
                                   layers=a.layers)

        def leg_layers():
            return ti.integrate_survey(reader, pipe, patch, overlap, a.batch, a.preload, lspec)

        def leg_host_layers():
            acc, cnt = np.zeros((3, n_pb, a.layers)), np.zeros((3, n_pb, a.layers), dtype=np.int64)
            geo = np.zeros((n_pb, a.layers), dtype=np.int64)
            for s, e, out in ti.predict_survey(reader, pipe, patch, overlap, a.batch, a.preload, out_dtype=np.float16):
                sv = reader.get_data_slice(idx_ping=s, n_pings=e - s, frequencies=pipe.frequencies)[channel]
                host_chunk_layers(acc, cnt, geo, out, sv, reader.get_seabed(s, e - s, return_numpy=True), lspec, s)
            return acc, cnt, geo
        legs.update(layers=leg_layers, host_layers=leg_host_layers)
    if a.edsu:
        espec = ti.IntegrationSpec(None, a.range_bin, mode=a.mode, ping_edges=edsu_table(a.pings, a.ping_bin, a.edsu_seed))
        legs["edsu"] = lambda: ti.integrate_survey(reader, pipe, patch, overlap, a.batch, a.preload, espec)
    if a.freqs:
        freqs = tuple(int(f) for f in a.freqs.split(","))
        fspec = ti.IntegrationSpec(a.ping_bin, a.range_bin, frequency=freqs, mode=a.mode)
        legs["freqs"] = lambda: ti.integrate_survey(reader, pipe, patch, overlap, a.batch, a.preload, fspec)
        legs["freqs_loop"] = lambda: [ti.integrate_survey(reader, pipe, patch, overlap, a.batch, a.preload,
                                                          ti.IntegrationSpec(a.ping_bin, a.range_bin, frequency=f, mode=a.mode))
                                      for f in freqs]
    times, last = {k: [] for k in legs}, {}
    for rnd in range(-1, a.rounds):                                       # round -1: warm-up (staging, packed weights)
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if rnd >= 0:
                times[name].append(time.perf_counter() - t0)
    acc, cnt, geo = last["host"]
    got = last["device"]
    counts_equal = bool(np.array_equal(got["pixels"], cnt))
    err, bound = np.abs(got["sv_sum"] - acc), (geo[None] + 2) * 2.0 ** -52 * acc
    within = bool((err <= bound).all() and (got["sv_sum"][acc == 0] == 0).all())
    med = {k: float(np.median(v)) for k, v in times.items()}
    line = {
        "bench": "integrate_survey", "pings": a.pings, "range": a.range, "preload": a.preload, "batch": a.batch,
        "precision": a.precision, "ping_bin": a.ping_bin, "range_bin": a.range_bin, "mode": a.mode, "cells": [n_pb, n_rb],
        "patches": patches, "rounds": a.rounds, "seconds": {k: [round(t, 4) for t in v] for k, v in times.items()},
        "patches_per_s": {k: round(patches / t, 1) for k, t in med.items()},
        "device_over_host": round(med["host"] / med["device"], 4),
        "device_over_predict_alone": round(med["predict"] / med["device"], 4),
        "counts_equal": counts_equal, "sums_within_bound": within,
        "largest_error_over_bound": float((err[acc > 0] / bound[acc > 0]).max()),
        "classified_pixels": [int(cnt[0].sum()), int(cnt[1].sum()), int(cnt[2].sum())],
    }
    if a.layers > 0:
        lacc, lcnt, lgeo = last["host_layers"]
        lgot = last["layers"]
        lerr, lbound = np.abs(lgot["sv_sum"] - lacc), (lgeo[None] + 2) * 2.0 ** -52 * lacc
        counts_equal = counts_equal and bool(np.array_equal(lgot["pixels"], lcnt))
        within = within and bool((lerr <= lbound).all() and (lgot["sv_sum"][lacc == 0] == 0).all())
        line.update(layers=a.layers, seabed_offset=a.seabed_offset, counts_equal=counts_equal, sums_within_bound=within,
                    layers_over_device=round(med["device"] / med["layers"], 4),
                    layers_over_host=round(med["host_layers"] / med["layers"], 4),
                    layer_pixels=[int(lcnt[0].sum()), int(lcnt[1].sum()), int(lcnt[2].sum())])
    if a.edsu:
        eacc, ecnt, egeo = np.zeros((3, n_pb, n_rb)), np.zeros((3, n_pb, n_rb), dtype=np.int64), np.zeros((n_pb, n_rb), dtype=np.int64)
        for s, e, out in ti.predict_survey(reader, pipe, patch, overlap, a.batch, a.preload, out_dtype=np.float16):   # untimed
            sv = reader.get_data_slice(idx_ping=s, n_pings=e - s, frequencies=pipe.frequencies)[channel]
            host_chunk_edges(eacc, ecnt, egeo, out, sv, espec, s)
        egot = last["edsu"]
        eerr, ebound = np.abs(egot["sv_sum"] - eacc), (egeo[None] + 2) * 2.0 ** -52 * eacc
        counts_equal = counts_equal and bool(np.array_equal(egot["pixels"], ecnt))
        within = within and bool((eerr <= ebound).all() and (egot["sv_sum"][eacc == 0] == 0).all())
        widths = np.diff(espec.ping_edges)
        dev = times["device"]
        line.update(counts_equal=counts_equal, sums_within_bound=within, edsu_seed=a.edsu_seed,
                    edsu_widths={"cells": int(len(widths)), "min": int(widths.min()), "max": int(widths.max()),
                                 "mean": round(float(widths.mean()), 2), "empty": int((widths == 0).sum())},
                    edsu_over_device=round(med["device"] / med["edsu"], 4),
                    device_spread=round((max(dev) - min(dev)) / med["device"], 4),
                    edsu_pixels=[int(ecnt[0].sum()), int(ecnt[1].sum()), int(ecnt[2].sum())],
                    kernel_time_measured=False)
    if a.freqs:
        fgot, floop = last["freqs"], last["freqs_loop"]
        f_counts = all(np.array_equal(fgot["pixels"][i], floop[i]["pixels"]) for i in range(len(freqs)))
        f_bits = all(fgot["sv_sum"][i].tobytes() == floop[i]["sv_sum"].tobytes() for i in range(len(freqs)))
        counts_equal, within = counts_equal and f_counts, within and f_bits
        spread = {k: round((max(times[k]) - min(times[k])) / med[k], 4) for k in ("freqs", "freqs_loop", "device")}
        line.update(freqs=list(freqs), freqs_counts_equal=f_counts, freqs_sums_bit_equal=f_bits,
                    freqs_over_loop=round(med["freqs_loop"] / med["freqs"], 4),
                    freqs_over_device=round(med["freqs"] / med["device"], 4), freqs_spread=spread["freqs"],
                    freqs_loop_spread=spread["freqs_loop"], device_spread=spread["device"],
                    freqs_pixels=[int(fgot["pixels"][i, 2].sum()) for i in range(len(freqs))],
                    counts_equal=counts_equal, sums_within_bound=within, kernel_time_measured=False)
    for k in legs:
        print(f"{k:8s}: {patches} patches, median {med[k]:.3f} s -> {patches / med[k]:.0f} patches/s", flush=True)
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    assert counts_equal and within, "integrate_survey disagrees with the host integration"
    assert med["device"] <= 1.03 * med["predict"], \
        f"integrate_survey ({med['device']:.3f} s) is more than 3 % slower than the prediction alone ({med['predict']:.3f} s)"


if __name__ == "__main__":
    main()
