#!/usr/bin/env python3
"""Golden vectors for EARLY metadata injection in whole-echogram inference (save_reader_predictions_memm,
pipeline_train_predict/save_predict.py:222-265, with a model built as UNet_Baseline(in_channels = 4 + metadata planes),
pipeline.py:388-397): the REFERENCE's own DatasetGriddedReader with meta_channels (get_crop_memmap -> data planes and
metadata planes, batch/dataset.py:212-242), define_data_transform_test(use_metadata=True) (remove_nan_inf,
db_with_limits_scaled, set_data_border_value -- on the data planes; the batch is np.concatenate((data, meta))),
define_label_transform_test and fill_out_array, run on the fake in-memory Echogram carrying the three per-ping vectors.
The network is replaced by a fixed predictor that weighs EVERY input channel, data and metadata alike.  Build container
only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tools.make_golden_tiling as g  # noqa: E402,F401  (stubs the optional imports, puts the reference on sys.path)
from tools.fake_reader import FakeEchogram, synth_survey  # noqa: E402
from tools.make_golden_tiling import ref_fill_out_array  # noqa: E402
from oracle import tiling_oracle as orc  # noqa: E402

from batch.dataset import DatasetGriddedReader  # noqa: E402  (reference)
from batch.transforms import define_data_transform_test, define_label_transform_test  # noqa: E402

# input channel k of the batch: 4 frequency planes (scaled dB in [0, 1]), then the metadata planes in the order of
# get_crop_memmap (portion_year, sin / cos portion_day, time_diff, depth_rel, depth_abs_surface, depth_abs_seabed)
WEIGHTS = np.array([[1.5, -1.0, 1.2, 0.4, 0.8, -0.6, 0.5, 0.3, -0.9, 1.1, 0.7],
                    [-1.2, 1.4, 0.2, 0.9, -0.5, 0.7, -0.4, -0.2, 1.0, -0.8, 0.6],
                    [0.3, 0.5, -1.3, 0.1, 0.2, 0.4, 0.9, 0.5, -0.3, 0.6, -1.0]], dtype=np.float32)


def meta_predictor(x):
    """Stand-in for an early-injection network: softmax over 3 fixed linear maps of ALL C + Cm input channels.
    x [C + Cm, H, W] -> [3, H, W] float32."""
    z = np.tensordot(WEIGHTS[:, :x.shape[0]], x.astype(np.float32), axes=(1, 0))
    z = z - z.max(0, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(0, keepdims=True)).astype(np.float32)


def echogram(n_pings, n_range, seed, sb_max):
    sv, labels, seabed = synth_survey(n_pings=n_pings, n_range=n_range, seed=seed)
    eg = FakeEchogram(np.ascontiguousarray(sv.swapaxes(1, 2)), np.ascontiguousarray(labels.T),
                      np.clip(seabed, 40, sb_max))
    rng = np.random.Generator(np.random.PCG64(seed + 100))
    tv = 737000.25 + np.cumsum(rng.uniform(5e-6, 9e-6, size=n_pings))
    eg.portion_of_day_vector = tv % 1
    eg.portion_of_year_scalar = 0.58
    eg.time_vector_diff = np.concatenate((np.diff(tv), [tv[-1] - tv[-2]])) / 6e-6 - 1
    return eg


def run(tag, n_pings, n_range, seed, sb_max, mc):
    eg = echogram(n_pings, n_range, seed, sb_max)
    freqs, patch, overlap = [18, 38, 120, 200], [256, 256], 20
    ds = DatasetGriddedReader(eg, patch, freqs, meta_channels=mc, grid_start=0, grid_end=n_pings,
                              patch_overlap=overlap, augmentation_function=None,
                              label_transform_function=define_label_transform_test(freqs, label_masks="all",
                                                                                   patch_overlap=overlap),
                              data_transform_function=define_data_transform_test(True), grid_mode="all")
    assert not ds.data_preload
    out = np.zeros([2, n_range, n_pings])
    centres = []
    for i in range(len(ds)):
        item = ds[i]
        assert item["data"].shape[0] == 4 + sum(2 if k == "portion_day" else 1 for k in orc.META_KEYS if mc[k])
        preds = meta_predictor(item["data"]).astype(np.float16)          # save_predict.py:252
        ref_fill_out_array(out, preds, item["labels"], item["center_coordinates"], 0)
        centres.append(np.array(item["center_coordinates"]))
    print(f"{tag}: {len(ds)} patches, {item['data'].shape[0]} input channels, written {np.mean(out[0] != 0):.3f}")
    return {f"{tag}/out_f16": out.astype(np.float16), f"{tag}/centres": np.array(centres),
            f"{tag}/shape": np.array([n_pings, n_range, seed, sb_max]),
            f"{tag}/meta_channels": np.array([bool(mc[k]) for k in orc.META_KEYS]),
            f"{tag}/portion_day": eg.portion_of_day_vector, f"{tag}/time_diff": eg.time_vector_diff,
            f"{tag}/portion_year": np.array(eg.portion_of_year_scalar)}


def main():
    all_on = {k: True for k in orc.META_KEYS}
    subset = dict(all_on, portion_day=False, depth_rel=False)
    fix = {"weights": WEIGHTS}
    fix.update(run("all", 460, 300, 31, 280, all_on))
    fix.update(run("subset", 300, 200, 32, 190, subset))      # water column not deeper than a patch: centre row = H // 2
    path = os.path.join(ROOT, "tests", "golden", "early_meta.npz")
    np.savez_compressed(path, **fix)
    print("saved", os.path.getsize(path))


if __name__ == "__main__":
    main()
