#!/usr/bin/env python3
"""Golden results of the WHOLE-SURVEY evaluation (validate_model_survey_zarr / _memm, pipeline_train_predict/
evaluate.py:39-117), produced by the REFERENCE's own chain on the in-memory readers of tools/fake_reader.py:
DatasetGriddedReader(grid_start=None, grid_end=None, grid_mode='all') -> get_crop_zarr / get_crop_memmap ->
define_label_transform_test(label_masks = eval mode) -> define_data_transform (zarr) / define_data_transform_test (memm)
-> DataLoader -> SegPipe.get_predictions_dataloader -> the masking of validate_model_testing (pipeline.py:347-353) ->
sklearn's precision_recall_curve + F1 (pipeline.py:284-295; called here directly: the reference passes the keyword
`probas_pred`, which current scikit-learn no longer accepts).  `predict_batch` is replaced by the stub
tools/fake_reader.eval_stub_logits, a function of floor(dB input) and the patch-local pixel position.

Stores only results (tests/golden/survey_eval.npz): grid centres, per-patch counts of every transformed label value, the
non-zero bins of hist_pos / hist_neg (float16 bit pattern of the sandeel probability over the valid pixels), the PR arrays,
and raw + transformed crops of a few border / NaN / inf patches.  The surveys are rebuilt from their seeds
(tools/fake_reader.synth_eval_survey).  Needs the reference checkout: tools/make_golden_survey_eval.py <crimac_unet dir>."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if len(sys.argv) < 2:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.abspath(sys.argv[1]))
for name in ("dask", "xarray", "numcodecs", "tqdm"):
    if name in sys.modules:
        continue
    try:
        __import__(name)
    except Exception:
        m = types.ModuleType(name)
        if name == "dask":
            m.config = types.SimpleNamespace(set=lambda **kw: None)
        if name == "numcodecs":
            m.Blosc = object
        if name == "tqdm":
            m.tqdm = lambda it, **kw: it
        sys.modules[name] = m

import torch  # noqa: E402
from sklearn.metrics import precision_recall_curve  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from tools.fake_reader import (FakeEchogram, FakeZarrReader, eval_stub_logits, holey_seabed_mask,  # noqa: E402
                               synth_eval_survey)

from batch.dataset import DatasetGriddedReader, get_crop  # noqa: E402  (reference)
from batch.transforms import (define_data_transform, define_data_transform_test,  # noqa: E402  (reference)
                              define_label_transform_test)
from pipeline_train_predict.pipeline import SegPipe  # noqa: E402  (reference)

FREQS, PATCH, OVERLAP = [18, 38, 120, 200], [64, 64], 8
LABEL_VALUES = (-100, -70, -50, -30, -10, -1, 0, 1, 2)
CASES = {"zarr": (437, 150, 21), "zarrmask": (437, 150, 21), "memm": (437, 150, 21), "memm_shallow": (301, 50, 22),
         "zarr_shallow": (301, 50, 22)}


def stub_margin():
    """Every sandeel probability the stub can produce, in float64, against the float16 rounding boundaries."""
    worst = np.inf
    for k in range(64):
        z = np.array([0.0, (k - 32) / 8, (k % 5 - 2) / 4])
        p = np.exp(z - z.max())
        p = p[1] / p.sum()
        h = np.float16(p)
        for nb in (np.nextafter(h, np.float16(0)), np.nextafter(h, np.float16(2))):
            edge = (float(h) + float(nb)) / 2          # a value beyond this edge rounds to the neighbour
            worst = min(worst, abs(p - edge) / p)
    return worst


class StubPipe(SegPipe):
    """The reference's SegPipe with the network replaced (nothing else is overridden)."""

    def __init__(self):
        self.model = torch.nn.Identity()
        self.device = torch.device("cpu")

    def predict_batch(self, batch, return_softmax=False):
        z = eval_stub_logits(batch["data"].float(), lambda a: torch.floor(a).long(), torch.remainder, torch.arange)
        return torch.stack([c.float() for c in z], dim=1)


def make_reader(case):
    n_pings, n_range, seed = CASES[case]
    sv, labels, seabed, boxes = synth_eval_survey(n_pings, n_range, seed)
    if case.startswith("memm"):
        return FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), seabed,
                            boxes=boxes), sv
    mask = holey_seabed_mask(seabed, n_range) if case == "zarrmask" else None
    return FakeZarrReader(sv, labels, seabed, mask=mask, boxes=boxes), sv


def run(case, mode, out):
    reader, sv = make_reader(case)
    memm = case.startswith("memm")
    lt = define_label_transform_test(frequencies=FREQS, label_masks=mode, patch_overlap=OVERLAP)
    dt = define_data_transform_test(False) if memm else define_data_transform(False)
    ds = DatasetGriddedReader(reader, PATCH, FREQS, meta_channels=[], grid_start=None, grid_end=None,
                              patch_overlap=OVERLAP, data_preload=False, augmentation_function=None,
                              label_transform_function=lt, data_transform_function=dt, grid_mode="all")
    items = [ds[i] for i in range(len(ds))]
    centres = np.array([it["center_coordinates"] for it in items])
    counts = np.array([[int((it["labels"] == v).sum()) for v in LABEL_VALUES] for it in items])
    assert counts.sum(1).tolist() == [PATCH[0] * PATCH[1]] * len(items), "a label value outside LABEL_VALUES"
    pipe = StubPipe()
    labels, preds, _ = pipe.get_predictions_dataloader(DataLoader(ds, batch_size=7, shuffle=False, num_workers=0),
                                                       disable_tqdm=True)
    preds[labels == -50] = 0                                    # validate_model_testing, pipeline.py:349-353
    labels, preds = pipe.select_valid_predictions(labels=labels, preds=preds)
    bits = preds.astype(np.float16).view(np.uint16).astype(np.int64)
    hp = np.bincount(bits[labels == 1], minlength=16384)
    hn = np.bincount(bits[labels != 1], minlength=16384)
    precision, recall, thresholds = precision_recall_curve(labels, preds, pos_label=1)
    den = recall + precision
    f1 = np.divide(2 * recall * precision, den, out=np.zeros_like(den), where=(den != 0))
    tag = f"{case}/{mode}"
    if mode == "all":
        out[f"{case}/centres"] = centres.astype(np.int32)
    else:
        assert np.array_equal(out[f"{case}/centres"], centres)
    out[f"{tag}/counts"] = counts.astype(np.int32)
    for name, h in (("pos", hp), ("neg", hn)):
        out[f"{tag}/hist_{name}_bins"] = np.nonzero(h)[0].astype(np.int32)
        out[f"{tag}/hist_{name}_counts"] = h[np.nonzero(h)[0]].astype(np.int64)
    out[f"{tag}/precision"], out[f"{tag}/recall"] = precision, recall
    out[f"{tag}/thresholds"], out[f"{tag}/F1"] = thresholds.astype(np.float64), f1
    print(f"{tag}: {len(ds)} patches, valid {hp.sum() + hn.sum()} (pos {hp.sum()}), bins {np.count_nonzero(hp + hn)}, "
          f"max F1 {f1.max():.4f}, labels {dict(zip(LABEL_VALUES, counts.sum(0).tolist()))}")
    if mode != "all":
        return
    # raw and transformed crops: the grid's corners, and the patches richest in NaN / inf samples
    nonfinite = []
    for c in centres:
        y0, x0 = c[0] - PATCH[0] // 2 + 1, c[1] - PATCH[1] // 2 + 1
        blk = sv[:, max(x0, 0):x0 + PATCH[1], max(y0, 0):y0 + PATCH[0]]
        nonfinite.append(int((~np.isfinite(blk)).sum()))
    picks = sorted({0, len(ds) - 1, len(ds) // 2, int(np.argmax(nonfinite))})
    out[f"{case}/crop_idx"] = np.array(picks, dtype=np.int32)
    for i in picks:
        raw_d, raw_l = get_crop(reader, np.array(centres[i]), PATCH, FREQS, [], ping_boundary=ds.ping_boundary)
        out[f"{case}/crop{i}/raw_data"] = np.asarray(raw_d)                      # float64 (zarr) / float32 (memm)
        out[f"{case}/crop{i}/raw_labels"] = np.asarray(raw_l).astype(np.int16)
        out[f"{case}/crop{i}/data"] = np.asarray(items[i]["data"]).astype(np.float32)
        out[f"{case}/crop{i}/labels"] = np.asarray(items[i]["labels"]).astype(np.int16)


def main():
    margin = stub_margin()
    print(f"stub: smallest relative distance of a probability to a float16 rounding boundary {margin:.2e}")
    assert margin > 1e-5, "the stub's probabilities must not sit near a float16 rounding boundary"
    out = {"patch": np.array(PATCH + [OVERLAP], dtype=np.int32), "label_values": np.array(LABEL_VALUES, dtype=np.int32)}
    for case in CASES:
        out[f"{case}/shape"] = np.array(CASES[case], dtype=np.int32)
        for mode in ("all", "region", "trace"):
            run(case, mode, out)
    path = os.path.join(ROOT, "tests", "golden", "survey_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
