"""Whole-survey evaluation on the tiled path, the parts that need no GPU: the patch grid and its chunking, the fixture's
consistency with sklearn's curve, the public surface of ``evaluate.py`` -- and the check that the predictor stub of the GPU
tests reproduces the reference's histograms exactly when the whole chain is restated with the CPU oracles alone.

Fixture: tests/golden/survey_eval.npz (tools/make_golden_survey_eval.py: the reference's own DatasetGriddedReader, test-time
transforms, get_predictions_dataloader and validate_model_testing masking on the surveys of
tools/fake_reader.synth_eval_survey)."""
import os

import numpy as np
import pytest

from oracle import labels_oracle as lorc
from oracle import tiling_oracle as torc
from tools.fake_reader import (FakeEchogram, FakeZarrReader, eval_stub_logits, holey_seabed_mask, synth_eval_survey)

CASES = ("zarr", "zarrmask", "memm", "memm_shallow", "zarr_shallow")
MODES = ("all", "region", "trace")


def load(golden_dir):
    return np.load(os.path.join(golden_dir, "survey_eval.npz"))


def make_reader(fix, case):
    n_pings, n_range, seed = (int(v) for v in fix[f"{case}/shape"])
    sv, labels, seabed, boxes = synth_eval_survey(n_pings, n_range, seed)
    if case.startswith("memm"):
        return FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), seabed, boxes=boxes)
    mask = holey_seabed_mask(seabed, n_range) if case == "zarrmask" else None
    return FakeZarrReader(sv, labels, seabed, mask=mask, boxes=boxes)


def golden_hist(fix, case, mode):
    out = []
    for name in ("pos", "neg"):
        h = np.zeros(16384, dtype=np.int64)
        h[fix[f"{case}/{mode}/hist_{name}_bins"]] = fix[f"{case}/{mode}/hist_{name}_counts"]
        out.append(h)
    return out


def test_grid_is_the_whole_surveys_and_chunking_partitions_it(golden_dir):
    """plan_eval_grid == the grid of the reference's DatasetGriddedReader(grid_start=None, grid_end=None, 'all') (with the
    memm centre adjustment of a shallow echogram); plan_eval_chunks deals every patch to exactly one chunk and every chunk
    covers the pings its patches touch -- for one chunk and for chunk sizes that cut patches in half."""
    from crimac_classifiers_unet_amd import tiled_inference as ti
    fix = load(golden_dir)
    pw, ph, overlap = (int(v) for v in fix["patch"])
    for case in CASES:
        n_pings, n_range, seed = (int(v) for v in fix[f"{case}/shape"])
        _, _, seabed, _ = synth_eval_survey(n_pings, n_range, seed)
        grid = ti.plan_eval_grid(n_range, seabed, n_pings, (pw, ph), overlap, memm=case.startswith("memm"))
        assert np.array_equal(grid, fix[f"{case}/centres"]), case
        for preload in (0, 5000, 200, 97, 32, 19):
            chunks = ti.plan_eval_chunks(grid, n_pings, (pw, ph), preload)
            idx = np.concatenate([c[0] for c in chunks])
            assert sorted(idx.tolist()) == list(range(len(grid))), (case, preload)
            assert len(chunks) == 1 if preload in (0, 5000) else len(chunks) >= 2
            for ids, lo, hi in chunks:
                x0 = grid[ids, 1] - pw // 2 + 1
                assert 0 <= lo < hi <= n_pings
                assert lo <= max(0, x0.min()) and hi >= min(n_pings, x0.max() + pw)
            if preload == 32:         # chunks narrower than a patch: patches reach across chunk borders
                assert any(hi - lo > 32 for _, lo, hi in chunks)


def test_metrics_from_golden_histograms_equal_the_reference_curve(golden_dir):
    """compute_evaluation_metrics_from_histograms on the golden histograms == the precision / recall / thresholds / F1
    arrays sklearn's precision_recall_curve gave for the reference's prediction vector."""
    from crimac_classifiers_unet_amd.pipeline import SegPipe
    fix = load(golden_dir)
    for case in CASES:
        for mode in MODES:
            hp, hn = golden_hist(fix, case, mode)
            m = SegPipe.compute_evaluation_metrics_from_histograms(hp, hn)
            for k in ("precision", "recall", "thresholds", "F1"):
                ref = fix[f"{case}/{mode}/{k}"]
                assert m[k].shape == ref.shape, (case, mode, k)
                assert np.allclose(m[k], ref, rtol=1e-12, atol=0), (case, mode, k)


def test_tiled_evaluation_asks_for_no_factory(golden_dir, tmp_path, monkeypatch):
    """validate_model_survey_zarr / _memm(tiled=True) need the readers only and write the csv through the shared tail;
    tiled=False without factories still raises the ImportError."""
    from crimac_classifiers_unet_amd import evaluate, tiled_inference as ti
    from crimac_classifiers_unet_amd.pipeline import SegPipe
    fix = load(golden_dir)
    hp, hn = golden_hist(fix, "zarr", "all")
    seen = {}

    def fake_survey(reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings, eval_mode="all", **kw):
        seen.update(reader=reader, preload=preload_n_pings, eval_mode=eval_mode)
        return hp, hn

    monkeypatch.setattr(ti, "evaluate_survey", fake_survey)
    pipe = object.__new__(SegPipe)
    pipe.model_is_loaded = True
    reader = make_reader(fix, "zarr")
    kw = dict(meta_channels={}, patch_size=[64, 64], patch_overlap=8, eval_mode="all", batch_size=4, num_workers=0,
              save_path_metrics=str(tmp_path), save_path_plot=str(tmp_path), survey="s1")
    m = evaluate.validate_model_survey_zarr([reader], pipe, preload_n_pings=100, tiled=True, **kw)
    assert seen["reader"] is reader and seen["preload"] == 100
    assert np.allclose(m["F1"], fix["zarr/all/F1"], rtol=1e-12)
    assert np.isnan(m["thresholds"][-1]) and len(m["thresholds"]) == len(m["F1"])
    rows = open(tmp_path / "s1_test.csv").read().strip().splitlines()
    assert rows[0] == ",precision,recall,thresholds,F1" and len(rows) == 1 + len(m["F1"])
    with pytest.raises(ImportError):
        evaluate.validate_model_survey_zarr([reader], pipe, **kw)
    with pytest.raises(ImportError):
        evaluate.validate_model_survey_memm([reader], pipe, **kw)
    with pytest.raises(AssertionError):          # the DataLoader path keeps its assert on preload_n_pings
        evaluate.validate_model_survey_zarr([reader], pipe, preload_n_pings=100, dataset_cls=object,
                                            data_transform_factory=lambda *a: None,
                                            label_transform_factory=lambda **k: None, **kw)


def oracle_chain(fix, case, mode):
    """The whole per-patch evaluation chain restated with the CPU oracles: (per-patch label counts, hist_pos, hist_neg,
    {patch index: (raw data, raw labels, dB data, labels)})."""
    n_pings, n_range, seed = (int(v) for v in fix[f"{case}/shape"])
    pw, ph, overlap = (int(v) for v in fix["patch"])
    sv, labels, seabed, boxes = synth_eval_survey(n_pings, n_range, seed)
    memm = case.startswith("memm")
    mask = holey_seabed_mask(seabed, n_range) if case == "zarrmask" else None
    if mask is not None:
        seabed = mask.argmax(axis=1)
    sv_hw = np.ascontiguousarray(sv.transpose(0, 2, 1))
    lab_hw = np.ascontiguousarray(labels.T)
    bb = None if mode == "all" else lorc.extend_boxes(boxes, mode, 20, n_range if memm else n_pings)
    values = fix["label_values"].tolist()
    hp, hn = np.zeros(16384, dtype=np.int64), np.zeros(16384, dtype=np.int64)
    counts, crops = [], {}
    for i, c in enumerate(fix[f"{case}/centres"]):
        raw = torc.crop(sv_hw, c, (ph, pw), 0).astype(np.float32)
        # zarr: nan_to_num in the crop (an inf sample stays a strong echo); memm: every non-finite sample -> 0
        raw = np.where(np.isfinite(raw), raw, np.float32(0)) if memm else np.nan_to_num(raw, nan=0.0)
        raw_l = torc.crop(lab_hw, c, (ph, pw), -100)
        lab = lorc.test_label_transform(raw, raw_l, c, 3, seabed, n_range, overlap, "memm" if memm else "zarr", mask,
                                        boxes_extended=bb)
        db, _ = torc.data_transform(raw)
        if memm:
            db[:, lab == -100] = 0.0                         # set_data_border_value
        z = eval_stub_logits(db[None], lambda a: np.floor(a).astype(np.int64), np.remainder, np.arange)
        z = np.stack([np.asarray(v, dtype=np.float32)[0] for v in z])
        e = np.exp(z - z.max(0, keepdims=True))
        prob = (e[1] / e.sum(0)).astype(np.float32)
        prob[lab == -50] = 0
        valid = ~np.isin(lab, (-100, -70, -30, -10))
        bits = prob.astype(np.float16).view(np.uint16).astype(np.int64)
        hp += np.bincount(bits[valid & (lab == 1)], minlength=16384)
        hn += np.bincount(bits[valid & (lab != 1)], minlength=16384)
        counts.append([int((lab == v).sum()) for v in values])
        crops[i] = (raw, raw_l, db, lab)
    return np.array(counts), hp, hn, crops


def test_stub_reproduces_the_reference_histograms_with_the_oracles_alone(golden_dir):
    """Crop (tiling oracle) -> test-time label transform (labels oracle) -> dB transform -> stub -> float32 softmax ->
    float16 bins, all in numpy: per-patch label counts and both histograms equal the reference's bin for bin, every case
    and eval mode -- the stub is reproducible, so the GPU flow may be held to exact equality.  Also pins the golden crops:
    the reference's raw crops (float64 in the zarr flavour, saturated to float32) and transformed labels are the oracles'."""
    fix = load(golden_dir)
    fmax = np.finfo(np.float32).max
    for case in CASES:
        for mode in MODES:
            counts, hp, hn, crops = oracle_chain(fix, case, mode)
            ghp, ghn = golden_hist(fix, case, mode)
            assert np.array_equal(counts, fix[f"{case}/{mode}/counts"]), (case, mode)
            assert np.array_equal(hp, ghp) and np.array_equal(hn, ghn), (case, mode)
            if mode != "all":
                continue
            seen_big = False
            for i in fix[f"{case}/crop_idx"].tolist():
                raw, raw_l, db, lab = crops[i]
                ref_raw = np.clip(fix[f"{case}/crop{i}/raw_data"], -fmax, fmax).astype(np.float32)
                seen_big |= bool((ref_raw == fmax).any())
                assert np.array_equal(raw, ref_raw), (case, i)
                assert np.array_equal(raw_l, fix[f"{case}/crop{i}/raw_labels"]), (case, i)
                assert np.array_equal(lab, fix[f"{case}/crop{i}/labels"]), (case, i)
                assert np.array_equal(np.floor(db), np.floor(fix[f"{case}/crop{i}/data"])), (case, i)
            assert seen_big == (not case.startswith("memm")), case     # zarr: inf survives the crop as a huge echo
