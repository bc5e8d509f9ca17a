#!/usr/bin/env python3
"""Whole-survey test-set evaluation, patches/s of the two ways to feed it on the same synthetic survey and model:

  tiled      -- tiled_inference.evaluate_survey: chunk resident on the GPU, crops gathered by crimac_gather_eval_crops,
                label / data transforms, forward and PR histograms on the GPU;
  dataloader -- the gridded patches cropped per patch in numpy DataLoader workers (RAW crops: synth.raw_crop), collated and
                uploaded; SegPipe.use_gpu_test_transform + gpu_metrics do the transforms and the histograms on the GPU
                (validate_model_testing's loop, get_pr_histograms_dataloader).

Survey: synth.SyntheticSurveyReader (sv [4, pings, 1024] fp32, flat seabed 900, annotated schools, NaN / inf samples), patch
256, overlap 20, h3p inference.  Prints one line per leg with its valid-pixel count and max F1 (the legs differ at inf samples:
get_crop_zarr's nan_to_num keeps them as echoes, synth.raw_crop leaves them to remove_nan_inf)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import synth, tiled_inference as ti  # noqa: E402


class GridDataset:
    """The evaluation grid as a map-style dataset of RAW crops (what the reference's DatasetGriddedReader yields with
    label_transform_function = data_transform_function = None)."""

    def __init__(self, reader, grid, window):
        self.reader, self.grid, self.window = reader, grid, window

    def __len__(self):
        return len(self.grid)

    def __getitem__(self, i):
        c = self.grid[i].astype(np.int64)
        data, labels = synth.raw_crop(self.reader, c, self.window)
        return {"data": data, "labels": labels, "center_coordinates": c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pings", type=int, default=16384)
    ap.add_argument("--range", type=int, default=1024)
    ap.add_argument("--preload", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--precision", default="h3p", help="infer_precision")
    ap.add_argument("--legs", default="tiled,dataloader")
    a = ap.parse_args()
    reader = synth.SyntheticSurveyReader(n_pings=a.pings, n_range=a.range, seabed_index=900, block=4096, schools=40,
                                         bad_frac=1e-4)
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg.update(save_model_params=False, data_mode="zarr", gpu_metrics=True, infer_precision=a.precision, eval_mode="all")
    pipe = pkg.SegPipeUNet(experiment_name="bench", **cfg)
    pipe.model.load_state_dict(synth.synth_state_dict(seed=0))
    pipe.model.to(pipe.device).eval()
    pipe.model_is_loaded = True
    patch, overlap = (256, 256), 20
    grid = ti.plan_eval_grid(a.range, reader.seabed, a.pings, patch, overlap)
    if "tiled" in a.legs:
        ti.evaluate_survey(reader, pipe, patch, overlap, a.batch, a.preload)          # warm-up (staging, packed weights)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hp, hn = ti.evaluate_survey(reader, pipe, patch, overlap, a.batch, a.preload)
        dt = time.perf_counter() - t0
        f1 = pipe.compute_evaluation_metrics_from_histograms(hp, hn)["F1"].max()
        print(f"tiled evaluation {a.precision}: {len(grid)} patches in {dt:.3f} s -> {len(grid) / dt:.0f} patches/s "
              f"({hp.sum() + hn.sum()} valid pixels, max F1 {f1:.4f})", flush=True)
    if "dataloader" in a.legs:
        from torch.utils.data import DataLoader
        pipe.use_gpu_test_transform(reader, patch_overlap=overlap)
        dl = DataLoader(GridDataset(reader, grid, patch), batch_size=a.batch, shuffle=False, num_workers=a.workers)
        pipe.get_pr_histograms_dataloader([next(iter(dl))])                           # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hp, hn, _ = pipe.get_pr_histograms_dataloader(dl)
        dt = time.perf_counter() - t0
        f1 = pipe.compute_evaluation_metrics_from_histograms(hp, hn)["F1"].max()
        print(f"DataLoader-fed evaluation {a.precision}, {a.workers} workers: {len(grid)} patches in {dt:.3f} s -> "
              f"{len(grid) / dt:.0f} patches/s ({hp.sum() + hn.sum()} valid pixels, max F1 {f1:.4f})", flush=True)


if __name__ == "__main__":
    main()
