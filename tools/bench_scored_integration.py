#!/usr/bin/env python3
"""What scoring the echo integration against the annotations costs on top of the evaluation it rides on: the survey of
tools/bench_survey_eval.py (synth.SyntheticSurveyReader, 16384 pings x 1024 rows, patch 256, overlap 20, h3p) through

  plain  -- tiled_inference.evaluate_survey as it is,
  scored -- the same call with integration=ScoredIntegration(spec): one crimac_integrate_confusion launch per batch,

in ALTERNATING passes of one process (plain, scored, plain, scored, ...), the median of each.  Prints one JSON line.
``--legs plain`` runs the first leg alone -- the way to time another checkout's evaluate_survey with this same file;
``--parent-plain-s`` records such a figure (median seconds of the parent commit, same box, same session) in the line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import yaml  # noqa: E402

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import synth, tiled_inference as ti  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pings", type=int, default=16384)
    ap.add_argument("--range", type=int, default=1024)
    ap.add_argument("--preload", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="h3p", help="infer_precision")
    ap.add_argument("--ping-bin", type=int, default=500)
    ap.add_argument("--range-bin", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="plain,scored")
    ap.add_argument("--parent-plain-s", type=float, default=None)
    a = ap.parse_args()
    legs = a.legs.split(",")
    reader = synth.SyntheticSurveyReader(n_pings=a.pings, n_range=a.range, seabed_index=900, block=4096, schools=40,
                                         bad_frac=1e-4)
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg.update(save_model_params=False, data_mode="zarr", gpu_metrics=True, infer_precision=a.precision, eval_mode="all")
    pipe = pkg.SegPipeUNet(experiment_name="bench", **cfg)
    pipe.model.load_state_dict(synth.synth_state_dict(seed=0))
    pipe.model.to(pipe.device).eval()
    pipe.model_is_loaded = True
    patch, overlap = (256, 256), 20
    patches = len(ti.plan_eval_grid(a.range, reader.seabed, a.pings, patch, overlap))

    def run(leg):
        kw, s = {}, None
        if leg == "scored":
            s = ti.ScoredIntegration(ti.IntegrationSpec(ping_bin=a.ping_bin, range_bin=a.range_bin))
            kw["integration"] = s
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ti.evaluate_survey(reader, pipe, patch, overlap, a.batch, a.preload, **kw)
        res = None if s is None else s.result()           # (the download belongs to the scored leg)
        return time.perf_counter() - t0, res

    for leg in legs:                                       # warm-up (staging, packed weights, scratch)
        run(leg)
    seconds, res = {leg: [] for leg in legs}, None
    for _ in range(a.rounds):
        for leg in legs:
            dt, r = run(leg)
            seconds[leg].append(round(dt, 4))
            res = r if r is not None else res
    line = {"bench": "scored_integration", "pings": a.pings, "range": a.range, "preload": a.preload, "batch": a.batch,
            "precision": a.precision, "ping_bin": a.ping_bin, "range_bin": a.range_bin, "patches": patches,
            "rounds": a.rounds, "seconds": seconds,
            "median_s": {leg: round(statistics.median(v), 4) for leg, v in seconds.items()}}
    line["patches_per_s"] = {leg: round(patches / m, 1) for leg, m in line["median_s"].items()}
    if "plain" in legs and "scored" in legs:
        line["scored_over_plain"] = round(line["median_s"]["scored"] / line["median_s"]["plain"], 4)
    if a.parent_plain_s is not None:
        line["parent_plain_median_s"] = a.parent_plain_s
    if res is not None:
        line["counted_pixels"] = [int(v) for v in res["pixels"][:, 2].sum(axis=(1, 2))]
        line["sv_recall_sandeel"] = float(ti.ScoredIntegration._ratio(res["sv_sum"][1, 0].sum(), res["sv_sum"][1, 2].sum()))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
