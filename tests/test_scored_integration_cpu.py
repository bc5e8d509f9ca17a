"""CPU: the C ABI of ``crimac_integrate_confusion`` / ``crimac_eval_crop_origins`` (header, binding, exported symbols, scratch
formula, argument checks, which need no GPU) and the host side of the scored integration: ``ScoredIntegration`` and the
refusals of the evaluation flows."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()


def test_header_declares_the_entry_points_and_the_library_exports_them():
    m = re.search(r"int crimac_integrate_confusion\(([^;]*)\);", HEADER)
    assert m, "crimac_integrate_confusion is not declared in the header"
    assert " ".join(m.group(1).split()) == (
        "const float* logits, int ncls, const float* raw, int C, int channel, const short* labels, const int* origins, "
        "int P, int ph, int pw, int n_range, long ping_bin, int range_bin, long n_pb_total, float thr_sandeel, "
        "float thr_other, int mode, double* acc, long long* cnt, void* scratch, long scratch_bytes, void* stream")
    i, l, f, vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    want = [vp, i, vp, i, i, vp, vp, i, i, i, i, l, i, l, f, f, i, vp, vp, vp, l, vp]
    assert hip.PROTOTYPES["crimac_integrate_confusion"] == (i, want, True)
    assert hip.SIGNATURES["crimac_integrate_confusion"] == want            # (takes the stream: `call` launches it)
    assert hip.SIGNATURES["crimac_eval_crop_origins"] == [vp, i, i, i, i, i, vp, vp]
    lib = hip.load_library()
    assert hasattr(lib, "crimac_integrate_confusion") and hasattr(lib, "crimac_eval_crop_origins")


def test_abi_version_is_still_17():
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", HEADER).group(1)) == hip.ABI_VERSION == 17
    assert hip.load_library().crimac_version() == 17


def test_scratch_formula_matches_its_defines():
    assert re.search(r"#define CRIMAC_CONFUSION_SLOT_BYTES \(3 \* CRIMAC_INTEGRATE_SLOT_BYTES\)", HEADER)
    assert hip.DEFINES["CRIMAC_CONFUSION_SLOT_BYTES"] == 3 * hip.INTEGRATE_SLOT_BYTES == 144 == ti.CONFUSION_SLOT_BYTES
    assert hip.DEFINES["CRIMAC_CONFUSION_MAX_PATCHES"] == 1024 == ti.CONFUSION_MAX_PATCHES
    assert "P * (ceil(pw / ping_bin) + 1) * (ceil(ph / range_bin) + 1) * CRIMAC_CONFUSION_SLOT_BYTES" in HEADER
    # 9 fp64 sums + 9 int64 counts per (patch, window cell); the window of a 24 x 40 patch on 7-ping x 5-row cells is 7 x 6
    assert ti.confusion_scratch_bytes(5, 24, 40, 7, 5) == 5 * 7 * 6 * 144
    assert ti.confusion_scratch_bytes(1, 64, 64, 64, 64) == 4 * 144 and ti.confusion_scratch_bytes(2, 64, 64, 1000, 1) == 2 * 2 * 65 * 144
    # the library asks for exactly that: one byte less is refused, and the message states the formula
    lib = hip.load_library()
    p = ctypes.c_void_p(64)
    args = [p, 3, p, 4, 1, p, p, 5, 24, 40, 37, 7, 5, 9, 0.5, 0.5, 0, p, p, p, 5 * 7 * 6 * 144 - 1, None]
    assert lib.crimac_integrate_confusion(*args) == -22
    assert b"scratch" in lib.crimac_last_error() and b"CRIMAC_CONFUSION_SLOT_BYTES" in lib.crimac_last_error()


def test_argument_checks_need_no_gpu():
    lib = hip.load_library()
    p = ctypes.c_void_p(64)
    #       logits ncls raw C ch lab org P  ph  pw  R   pbin rbin n_pb thr0 thr1 mode acc cnt scratch bytes stream
    good = [p, 3, p, 4, 1, p, p, 5, 24, 40, 37, 7, 5, 9, 0.5, 0.5, 0, p, p, p, 0, None]      # (bytes = 0: stops at the scratch)
    assert lib.crimac_integrate_confusion(*good) == -22 and b"scratch" in lib.crimac_last_error()
    for at, value, word in ((1, 2, b"ncls"), (1, 4, b"ncls"), (4, 4, b"channel"), (4, -1, b"channel"), (7, 0, b"patches"),
                            (7, 1025, b"patches"), (8, 0, b"patch"), (9, 40000, b"patch"), (10, 0, b"n_range"),
                            (11, 0, b"ping_bin"), (12, 0, b"range_bin"), (13, 0, b"n_pb_total"), (14, 0.0, b"thr"),
                            (15, float("nan"), b"thr"), (16, 2, b"mode"), (0, None, b"null"), (6, None, b"null"),
                            (17, None, b"null"), (19, None, b"null")):
        bad = list(good)
        bad[at] = value
        assert lib.crimac_integrate_confusion(*bad) == -22, (at, value)
        assert word in lib.crimac_last_error(), (at, value, lib.crimac_last_error())
    for bad in ([None, 1, 8, 8, 10, 0, p, None], [p, 0, 8, 8, 10, 0, p, None], [p, 1, 8, 8, 10, 2, p, None],
                [p, 1, 8, 8, 0, 1, p, None]):
        assert lib.crimac_eval_crop_origins(*bad) == -22


def holder(n_pings=20, n_range=10, **kw):
    s = ti.ScoredIntegration(ti.IntegrationSpec(ping_bin=10, range_bin=5, **kw))
    return s.begin([18, 38, 120], 3, "cpu", n_pings, n_range)


def test_result_recall_and_precision_on_hand_made_accumulators():
    s = holder(n_pings=25)
    assert s.spec.channel == 1 and s.acc.shape == s.cnt.shape == (3, 3, 3, 2)
    assert s.acc.dtype == torch.float64 and s.cnt.dtype == torch.int64 and not s.acc.any() and not s.cnt.any()
    # cell (0, 0): 8 of the 10 annotated as sandeel found, 2 background and 0.5 other booked as sandeel
    s.acc[1, 0, 0, 0], s.acc[1, 2, 0, 0] = 8.0, 10.0
    s.acc[0, 0, 0, 0], s.acc[0, 2, 0, 0] = 2.0, 50.0
    s.acc[2, 0, 0, 0], s.acc[2, 1, 0, 0], s.acc[2, 2, 0, 0] = 0.5, 3.0, 4.0
    # cell (1, 1): sandeel annotated, none found, nothing booked as sandeel; cell (2, 0): nothing annotated, 1.0 booked
    s.acc[1, 2, 1, 1] = 6.0
    s.acc[0, 0, 2, 0], s.acc[0, 2, 2, 0] = 1.0, 7.0
    s.cnt[1, 2, 0, 0] = 12
    res = s.result()
    assert set(res) == {"sv_sum", "pixels", "annotated", "classes", "ping_edges", "range_edges"}
    assert res["annotated"] == ("background", "sandeel", "other") and res["classes"] == ("sandeel", "other", "all")
    assert res["sv_sum"].shape == res["pixels"].shape == (3, 3, 3, 2)
    assert res["sv_sum"].dtype == np.float64 and res["pixels"].dtype == np.int64 and res["pixels"][1, 2, 0, 0] == 12
    assert res["ping_edges"].tolist() == [0, 10, 20, 25] and res["range_edges"].tolist() == [0, 5, 10]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # empty cells give NaN without a warning
        rc, r = s.recall(1, res)
        pc, p = s.precision("sandeel", res)
        ro, r_other = s.recall("other")
        po, p_other = s.precision(2)
    assert rc.shape == pc.shape == (3, 2) and rc.dtype == np.float64
    assert rc[0, 0] == 0.8 and rc[1, 1] == 0.0 and np.isnan(rc[2, 0]) and np.isnan(rc[0, 1]) and np.isnan(rc).sum() == 4
    assert r == 8.0 / 16.0
    assert pc[0, 0] == 8.0 / 10.5 and pc[2, 0] == 0.0 and np.isnan(pc[1, 1]) and np.isnan(pc).sum() == 4
    assert p == 8.0 / 11.5
    assert ro[0, 0] == 0.75 and r_other == 0.75 and po[0, 0] == 1.0 and p_other == 1.0 and np.isnan(po[2, 0])
    # nasc takes the result as it is
    assert np.array_equal(ti.nasc(res, 0.19), 4.0 * np.pi * 1852.0 ** 2 * 0.19 * res["sv_sum"])
    for bad in (0, 3, "all", True, 1.0):
        with pytest.raises(ValueError, match="class"):
            s.recall(bad, res)
    # an all-empty result: NaN everywhere, survey-wide too
    e = holder()
    assert np.isnan(e.recall(1)[0]).all() and np.isnan(e.recall(1)[1]) and np.isnan(e.precision(2)[1])


def test_holder_lifecycle():
    s = ti.ScoredIntegration(ti.IntegrationSpec(10, 5, frequency=120, mode="probability"))
    with pytest.raises(ValueError, match="nothing was evaluated"):
        s.result()
    with pytest.raises(ValueError, match="begin"):
        s.add_batch(None, None, None, None, None, 10, False)
    s.begin([18, 38, 120], 3, "cpu", 20, 10)
    assert s.spec.channel == 2 and s.spec.mode == "probability"
    acc = s.acc
    assert s.begin([18, 38, 120], 3, "cpu", 20, 10).acc is acc            # the same extent: keeps accumulating
    with pytest.raises(ValueError, match="one holder per survey"):
        s.begin([18, 38, 120], 3, "cpu", 21, 10)
    with pytest.raises(ValueError, match="frequency 120"):
        ti.ScoredIntegration(ti.IntegrationSpec(10, 5, frequency=120)).begin([18, 38], 3, "cpu", 20, 10)
    with pytest.raises(TypeError, match="IntegrationSpec"):
        ti.ScoredIntegration({"ping_bin": 10})


def test_the_three_refusals():
    # 1. a seabed-aware spec
    for kw in (dict(seabed_offset=-3), dict(seabed_offset=0, reference="seabed", layers=4)):
        with pytest.raises(NotImplementedError, match="seabed"):
            ti.ScoredIntegration(ti.IntegrationSpec(10, 5, **kw))
    # 2. the packed flow names the per-echogram call (before it looks at anything else)
    s = ti.ScoredIntegration(ti.IntegrationSpec(10, 5))
    with pytest.raises(NotImplementedError, match="evaluate_echogram_memm"):
        ti.evaluate_echograms_memm([], None, (64, 64), 8, 4, integration=s)
    # 3. a model that does not have 3 classes: the holder, and both flows before they touch the data
    with pytest.raises(ValueError, match="n_classes=4"):
        s.begin([18, 38], 4, "cpu", 20, 10)
    pipe = types.SimpleNamespace(model=types.SimpleNamespace(n_classes=2), device="cpu", frequencies=[18, 38])
    reader = types.SimpleNamespace(shape=(20, 10))
    with pytest.raises(ValueError, match="n_classes=2"):
        ti.evaluate_survey(reader, pipe, (64, 64), 8, 4, 100, integration=s)
    with pytest.raises(ValueError, match="n_classes=2"):
        ti.evaluate_echogram_memm(None, pipe, (64, 64), 8, 4, integration=s)
    with pytest.raises(TypeError, match="ScoredIntegration"):
        ti.evaluate_survey(reader, pipe, (64, 64), 8, 4, 100, integration=ti.IntegrationSpec(10, 5))
    assert s.acc is None                                                    # nothing was allocated on the way


def test_flows_take_the_keyword_and_default_to_none():
    import inspect
    for fn in (ti.ChunkPredictor.evaluate, ti.evaluate_survey, ti.evaluate_echogram_memm, ti.evaluate_echograms_memm):
        assert inspect.signature(fn).parameters["integration"].default is None, fn.__name__
