"""Per-class PR curves / F1 from the per-class histograms, the parts that need no GPU: the C ABI of
``crimac_pr_histogram_classes``, the metrics of one row against a restated sklearn rule, the per-class files, the refused
``classes`` and the defaults of every signature that gained the keyword."""
import ctypes
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import build, evaluate, hip  # noqa: E402
from crimac_classifiers_unet_amd import tiled_inference as ti  # noqa: E402
from crimac_classifiers_unet_amd.pipeline import SegPipe, per_class_path  # noqa: E402

PR_BINS = hip.PR_BINS


def test_header_declares_the_entry_point_and_the_binding_follows():
    header = re.sub(r"/\*.*?\*/", " ", open(build.HEADER).read(), flags=re.S)
    m = re.search(r"int\s+crimac_pr_histogram_classes\s*\(([^)]*)\)", header)
    assert m, "crimac_pr_histogram_classes is not declared in include/crimac_unet_hip.h"
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["logits", "ncls", "labels", "label_bytes", "B", "H", "W", "class_mask", "hist", "stream"]
    i, vp = ctypes.c_int, ctypes.c_void_p
    want = [vp, i, vp, i, i, i, i, ctypes.c_uint, vp, vp]
    assert hip.PROTOTYPES["crimac_pr_histogram_classes"] == (i, want, True)
    assert hip.SIGNATURES["crimac_pr_histogram_classes"] == want
    # the single-class entry point is declared as it was
    assert hip.PROTOTYPES["crimac_pr_histogram"] == (i, [vp, i, vp, i, i, i, i, vp, vp, vp], True)


def three_class_histogram(seed=3):
    """[3, 2, 16384]: a few thousand pixels per row on ~200 bins (0, subnormals, mid-range, 1.0), pos and neg skewed apart."""
    rng = np.random.default_rng(seed)
    h = np.zeros((3, 2, PR_BINS), dtype=np.int64)
    for c in (1, 2):
        bins = np.unique(np.concatenate(([0, 1, 0x3C00], rng.integers(0, 0x3C01, 200))))
        w = bins / 0x3C00
        h[c, 0, bins] = rng.poisson(1 + 20 * w * c)
        h[c, 1, bins] = rng.poisson(1 + 30 * (1 - w))
        h[c, 1, 0] += 5000
    return h


def pr_reference(pos, neg):
    """sklearn's precision_recall_curve restated on the histogram: descending unique float16 scores, cumulative tp / fp,
    precision = tp / (tp + fp), recall = tp / tp[-1], both reversed, with the trailing (1, 0) point."""
    bins = np.nonzero(pos + neg)[0]
    score = bins.astype(np.uint16).view(np.float16).astype(np.float64)
    order = np.argsort(-score)
    tp, fp = np.cumsum(pos[bins][order]), np.cumsum(neg[bins][order])
    precision, recall = tp / (tp + fp), tp / tp[-1]
    precision, recall = np.append(precision[::-1], 1.0), np.append(recall[::-1], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        f1 = np.where(precision + recall > 0, 2 * precision * recall / (precision + recall), 0.0)
    return precision, recall, score[order][::-1], f1


@pytest.mark.parametrize("c", [1, 2])
def test_metrics_of_one_row_equal_the_restated_rule_and_sklearn(c):
    h = three_class_histogram()
    m = SegPipe.compute_evaluation_metrics_from_histograms(h[c, 0], h[c, 1])
    precision, recall, thr, f1 = pr_reference(h[c, 0], h[c, 1])
    assert np.array_equal(m["precision"], precision) and np.array_equal(m["recall"], recall)
    assert np.array_equal(m["thresholds"], thr) and np.allclose(m["F1"], f1, rtol=1e-15, atol=0)
    try:
        from sklearn.metrics import precision_recall_curve
    except ImportError:
        return
    # the per-pixel vectors the histogram stands for: label c for pos, another class for neg
    bins = np.arange(PR_BINS)
    scores = np.concatenate([np.repeat(bins, h[c, 0]), np.repeat(bins, h[c, 1])]).astype(np.uint16).view(np.float16)
    labels = np.concatenate([np.full(h[c, 0].sum(), c), np.full(h[c, 1].sum(), 3 - c)])
    p, r, t = precision_recall_curve(labels, scores, pos_label=c)
    assert np.allclose(m["precision"], p, rtol=1e-15) and np.allclose(m["recall"], r, rtol=1e-15)
    assert np.array_equal(m["thresholds"], t.astype(np.float64))


def cpu_pipe():
    pipe = object.__new__(SegPipe)
    pipe.model = types.SimpleNamespace(n_classes=3)
    return pipe


def test_per_class_files_and_the_sandeel_file_is_the_default_file(tmp_path, capsys):
    h = three_class_histogram()
    pipe = cpu_pipe()
    os.makedirs(tmp_path / "default")
    m1 = pipe.validate_model_testing_from_histograms(h[1, 0], h[1, 1], str(tmp_path / "default" / "s_test.csv"), None)
    assert capsys.readouterr().out == f"F1 score: {m1['F1'].max()}\n"
    out = pipe.validate_model_testing_from_histograms(h[[1, 2], 0], h[[1, 2], 1], str(tmp_path / "s_test.csv"),
                                                      str(tmp_path / "s_pr.png"), classes=(1, 2))
    assert sorted(out) == [1, 2]
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".csv")) == ["s_test_other.csv", "s_test_sandeel.csv"]
    assert open(tmp_path / "s_test_sandeel.csv", "rb").read() == open(tmp_path / "default" / "s_test.csv", "rb").read()
    assert open(tmp_path / "s_test_other.csv", "rb").read() != open(tmp_path / "s_test_sandeel.csv", "rb").read()
    assert not os.path.exists(tmp_path / "s_pr.png")                  # plots carry the class name too (when matplotlib draws)
    assert all(np.array_equal(out[1][k], m1[k], equal_nan=True) for k in ("precision", "recall", "thresholds", "F1"))
    m2 = SegPipe.compute_evaluation_metrics_from_histograms(h[2, 0], h[2, 1])
    assert np.array_equal(out[2]["F1"], m2["F1"])
    assert capsys.readouterr().out.splitlines()[-2:] == [f"F1 score (sandeel): {m1['F1'].max()}",
                                                         f"F1 score (other): {m2['F1'].max()}"]
    # rows follow `classes`
    swapped = pipe.validate_model_testing_from_histograms(h[[2, 1], 0], h[[2, 1], 1], None, None, classes=(2, 1))
    assert list(swapped) == [2, 1] and np.array_equal(swapped[1]["F1"], m1["F1"])
    assert per_class_path("a/b.c/s_test.csv", 3) == "a/b.c/s_test_class3.csv" and per_class_path(None, 1) is None
    with pytest.raises(ValueError, match="hist_pos"):
        pipe.validate_model_testing_from_histograms(h[1, 0], h[1, 1], None, None, classes=(1, 2))


@pytest.mark.parametrize("bad", [(0,), (3,), (1, 1), (), (1.5,), "12", 1])
def test_bad_classes_raise_value_error(bad):
    with pytest.raises(ValueError, match="classes"):
        ti.check_classes(bad, 3)
    pipe = cpu_pipe()
    with pytest.raises(ValueError, match="classes"):
        pipe.validate_model_testing_from_histograms(np.zeros((1, PR_BINS)), np.zeros((1, PR_BINS)), None, None, classes=bad)
    pipe.device, pipe.frequencies = "cpu", [18, 38, 120, 200]
    for flow in (lambda: ti.evaluate_survey(None, pipe, (64, 64), 8, 8, 0, classes=bad),             # before anything is read
                 lambda: ti.evaluate_echogram_memm(None, pipe, (64, 64), 8, 8, classes=bad),
                 lambda: ti.evaluate_echograms_memm(iter([]), pipe, (64, 64), 8, 8, classes=bad),
                 lambda: pipe.get_pr_histograms_dataloader([], classes=bad),
                 lambda: evaluate.validate_model_survey_memm([], pipe, {}, (64, 64), 8, "all", 8, 0, None, None, tiled=True,
                                                             eval_classes=bad)):
        with pytest.raises(ValueError, match="classes"):
            flow()


def test_good_classes_and_names():
    assert ti.check_classes(None, 3) is None
    assert ti.check_classes([2, 1], 3) == (2, 1) and ti.check_classes((np.int64(3),), 4) == (3,)
    assert [ti.class_name(c) for c in (1, 2, 3)] == ["sandeel", "other", "class3"]
    assert evaluate.parse_classes("1,2") == (1, 2) and evaluate.parse_classes("all", 4) == (1, 2, 3)
    assert evaluate.parse_classes(None) is None and evaluate.parse_classes([2]) == (2,)
    with pytest.raises(ValueError, match="--classes"):
        evaluate.parse_classes("1;2")
    h = three_class_histogram()
    hp, hn = ti.split_histograms(h, (2, 1))
    assert np.array_equal(hp, h[[2, 1], 0]) and np.array_equal(hn, h[[2, 1], 1])
    h[2, 0, PR_BINS - 1] = 1
    assert ti.split_histograms(h, (1,))[0].shape == (1, PR_BINS)
    with pytest.raises(ValueError, match=r"other probabilities.*class 2"):
        ti.split_histograms(h, (1, 2))


def test_misspelt_keyword_is_still_refused():
    pipe = cpu_pipe()
    pipe.device, pipe.frequencies = "cpu", [18, 38, 120, 200]
    for typo in ("classe", "clases", "classses"):
        with pytest.raises(TypeError, match="classes"):
            ti.evaluate_echograms_memm(iter([]), pipe, (32, 32), 4, 8, **{typo: (1, 2)})


def test_classes_without_a_histogram_path_are_refused(tmp_path):
    pipe = cpu_pipe()
    pipe.gpu_metrics = False
    for fn in (evaluate.validate_model_survey_zarr, evaluate.validate_model_survey_memm):
        with pytest.raises(ValueError, match="tiled"):
            fn([], pipe, {}, (64, 64), 8, "all", 8, 0, None, None, eval_classes=(1, 2))
    with pytest.raises(ValueError, match="gpu_metrics"):
        pipe.validate_model_testing([], None, None, classes=(1, 2))
    # the command line: --classes without --tiled (and without gpu_metrics in the yaml)
    yaml_path, ckpt = tmp_path / "exp.yaml", tmp_path / "run" / "best.pt"
    yaml_path.write_text("data_mode: memm\n")
    os.makedirs(ckpt.parent)
    ckpt.write_bytes(b"")
    argv = ["--yaml_path", str(yaml_path), "--checkpoint_path", str(ckpt), "--save_path_metrics", str(tmp_path),
            "--save_path_plot", str(tmp_path), "--classes", "1,2"]
    with pytest.raises(ValueError, match="--tiled"):
        evaluate.main(argv)
    # ... and a pipeline built with eval_classes but without gpu_metrics
    import yaml
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg["save_model_params"] = False
    with pytest.raises(ValueError, match="gpu_metrics"):
        pkg.SegPipeUNet(experiment_name="cpu", **{**cfg, "gpu_metrics": False, "eval_classes": [1, 2]})
    assert pkg.SegPipeUNet(experiment_name="cpu", **{**cfg, "gpu_metrics": True, "eval_classes": [1, 2]}).eval_classes == (1, 2)
    assert pkg.SegPipeUNet(experiment_name="cpu", **cfg).eval_classes is None


@pytest.mark.parametrize("fn, name", [
    (ti.ChunkPredictor.evaluate, "classes"), (ti.evaluate_survey, "classes"), (ti.evaluate_echogram_memm, "classes"),
    (ti.evaluate_echograms_memm, "classes"), (ti.finish_histograms, "classes"), (ti.add_pr_histograms, "classes"),
    (SegPipe.get_pr_histograms_dataloader, "classes"), (SegPipe.validate_model_testing_from_histograms, "classes"),
    (SegPipe.validate_model_testing, "classes"), (SegPipe.__init__, "eval_classes"),
    (evaluate.validate_model_survey_zarr, "eval_classes"), (evaluate.validate_model_survey_memm, "eval_classes")],
    ids=lambda v: getattr(v, "__qualname__", v))
def test_every_touched_signature_defaults_to_none(fn, name):
    p = inspect.signature(fn).parameters[name]
    assert p.default is None and p.kind is p.POSITIONAL_OR_KEYWORD


class Logger:
    def __init__(self):
        self.rows = {}

    def add_scalar(self, tag, scalar_value, global_step):
        self.rows[tag] = float(scalar_value)


def test_training_validation_logs_the_other_classes_and_keeps_the_sandeel_choice(monkeypatch):
    h = three_class_histogram()
    pipe = cpu_pipe()
    pipe.gpu_metrics, pipe.best_F1_val, pipe.checkpoint_dir = True, -np.inf, None
    asked = []

    def hists(dataloader, criterion=None, disable_tqdm=True, classes=None):
        asked.append(classes)
        return (h[1, 0], h[1, 1], 0.25) if classes is None else (h[list(classes), 0], h[list(classes), 1], 0.25)
    pipe.get_pr_histograms_dataloader = hists
    pipe.eval_classes = None
    base, log0 = pipe.validate_model_training(None, None, (lg := Logger()), 0), lg.rows
    pipe.eval_classes, pipe.best_F1_val = (2, 1), -np.inf
    m, log1 = pipe.validate_model_training(None, None, (lg := Logger()), 0), lg.rows
    assert asked == [None, (1, 2)]
    assert np.array_equal(m["F1"], base["F1"]) and pipe.best_F1_val == base["F1"].max()
    m2 = SegPipe.compute_evaluation_metrics_from_histograms(h[2, 0], h[2, 1])
    best = int(np.argmax(m2["F1"]))
    assert {k: v for k, v in log1.items() if k in log0} == log0
    assert set(log1) - set(log0) == {"test/F1_score_other", "test/precision_other", "test/recall_other"}
    assert log1["test/F1_score_other"] == m2["F1"][best] and log1["test/precision_other"] == m2["precision"][best]
    assert log1["test/recall_other"] == m2["recall"][best]
