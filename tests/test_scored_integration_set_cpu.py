"""CPU: the C ABI of ``crimac_integrate_confusion_multi`` / ``crimac_eval_crop_origins_multi`` (header, binding, exported
symbols, argument checks, which need no GPU) and the host side of the scored integration of a memm survey:
``ScoredIntegrationSet`` on hand-made per-echogram accumulators and the refusals of ``evaluate_echograms_memm``."""
import ctypes
import os
import re
import types
import warnings

import numpy as np
import pytest

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()


def test_header_declares_the_entry_points_and_the_library_exports_them():
    m = re.search(r"int crimac_integrate_confusion_multi\(([^;]*)\);", HEADER)
    assert m, "crimac_integrate_confusion_multi is not declared in the header"
    assert " ".join(m.group(1).split()) == (
        "const float* logits, int ncls, const float* raw, int C, int channel, const short* labels, const int* origins, "
        "const crimac_memm_desc* descs, int n_desc, const int* src, const long long* shares, int P, int ph, int pw, "
        "long ping_bin, int range_bin, float thr_sandeel, float thr_other, int mode, double* acc, long long* cnt, "
        "void* scratch, long scratch_bytes, void* stream")
    m = re.search(r"int crimac_eval_crop_origins_multi\(([^;]*)\);", HEADER)
    assert m, "crimac_eval_crop_origins_multi is not declared in the header"
    assert " ".join(m.group(1).split()) == ("const crimac_memm_desc* descs, int n_desc, const int* src, const int* centres, "
                                            "int P, int ph, int pw, int* origins, void* stream")
    i, l, f, vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    want = [vp, i, vp, i, i, vp, vp, vp, i, vp, vp, i, i, i, l, i, f, f, i, vp, vp, vp, l, vp]
    assert hip.PROTOTYPES["crimac_integrate_confusion_multi"] == (i, want, True)
    assert hip.SIGNATURES["crimac_integrate_confusion_multi"] == want
    assert hip.SIGNATURES["crimac_eval_crop_origins_multi"] == [vp, i, vp, vp, i, i, i, vp, vp]
    lib = hip.load_library()
    assert hasattr(lib, "crimac_integrate_confusion_multi") and hasattr(lib, "crimac_eval_crop_origins_multi")


def test_abi_version_is_still_17():
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", HEADER).group(1)) == hip.ABI_VERSION == 17
    assert hip.load_library().crimac_version() == 17


def test_argument_checks_need_no_gpu():
    lib = hip.load_library()
    p = ctypes.c_void_p(64)
    need = ti.confusion_scratch_bytes(5, 24, 40, 7, 5)
    assert need == 5 * 7 * 6 * 144
    #       0      1    2   3  4  5    6    7     8      9   10      11 12  13  14    15    16   17   18   19   20   21      22
    #       logits ncls raw C  ch lab  org  descs n_desc src shares  P  ph  pw  pbin  rbin  thr0 thr1 mode acc  cnt  scratch bytes
    good = [p, 3, p, 4, 1, p, p, p, 3, p, p, 5, 24, 40, 7, 5, 0.5, 0.5, 0, p, p, p, need - 1, None]
    assert lib.crimac_integrate_confusion_multi(*good) == -22              # one byte short: stops at the scratch
    err = lib.crimac_last_error()
    assert b"integrate_confusion_multi" in err and b"scratch" in err and b"CRIMAC_CONFUSION_SLOT_BYTES" in err
    for at, value, word in ((0, None, b"null"), (2, None, b"null"), (5, None, b"null"), (6, None, b"null"),
                            (7, None, b"null"), (9, None, b"null"), (10, None, b"null"), (19, None, b"null"),
                            (20, None, b"null"), (21, None, b"null"), (8, 0, b"n_desc"), (8, -1, b"n_desc"),
                            (11, 0, b"patches"), (11, 1025, b"patches"), (1, 2, b"ncls"), (1, 4, b"ncls"),
                            (4, 4, b"channel"), (4, -1, b"channel"), (12, 0, b"patch"), (13, 40000, b"patch"),
                            (14, 0, b"ping_bin"), (14, 2 ** 31, b"ping_bin"), (15, 0, b"range_bin"), (16, 0.0, b"thr"),
                            (17, float("nan"), b"thr"), (18, 2, b"mode"), (18, -1, b"mode")):
        bad = list(good)
        bad[at] = value
        assert lib.crimac_integrate_confusion_multi(*bad) == -22, (at, value)
        assert word in lib.crimac_last_error(), (at, value, lib.crimac_last_error())
    #     descs n_desc src centres P ph pw origins stream
    ok = [p, 3, p, p, 4, 8, 8, p, None]
    for at, value in ((0, None), (1, 0), (2, None), (3, None), (4, 0), (5, 0), (6, 0), (7, None)):
        bad = list(ok)
        bad[at] = value
        assert lib.crimac_eval_crop_origins_multi(*bad) == -22, (at, value)
        assert b"eval_crop_origins_multi" in lib.crimac_last_error()


# ---- the set on hand-made per-echogram accumulators ------------------------------------------------------------------
def record(name, n_pings, n_range):
    return types.SimpleNamespace(echogram=name, n_pings=n_pings, n_range=n_range)


def hand_made_set():
    s = ti.ScoredIntegrationSet(ti.IntegrationSpec(ping_bin=10, range_bin=5)).begin([18, 38, 120], 3)
    group = [record("a", 25, 10), record("b", 8, 3), record("c", 10, 12)]
    shares, total = s.shares(group)
    assert shares == [(0, (3, 2)), (54, (1, 1)), (63, (1, 3))] and total == 90
    sums, counts = np.zeros(total), np.zeros(total, dtype=np.int64)
    a = sums[:54].reshape(3, 3, 3, 2)
    # echogram a: cell (0, 0): 8 of the 10 annotated as sandeel found, 2 background and 0.5 other booked as sandeel
    a[1, 0, 0, 0], a[1, 2, 0, 0] = 8.0, 10.0
    a[0, 0, 0, 0], a[0, 2, 0, 0] = 2.0, 50.0
    a[2, 0, 0, 0], a[2, 1, 0, 0], a[2, 2, 0, 0] = 0.5, 3.0, 4.0
    a[1, 2, 1, 1] = 6.0                                      # cell (1, 1): sandeel annotated, none found
    counts[:54].reshape(3, 3, 3, 2)[1, 2, 0, 0] = 12
    # echogram b: nothing annotated as sandeel, 1.0 of the background booked as sandeel
    b = sums[54:63].reshape(3, 3)
    b[0, 0], b[0, 2] = 1.0, 7.0
    counts[54:63].reshape(3, 3)[0, 2] = 5
    # echogram c stays empty
    s.add_group(group, shares, sums, counts)
    return s


def test_results_totals_recall_and_precision():
    s = hand_made_set()
    assert s.spec.channel == 1
    res = s.results()
    assert [eg for eg, _ in res] == ["a", "b", "c"]
    ra, rb, rc = (r for _, r in res)
    for r, shape in ((ra, (3, 3, 3, 2)), (rb, (3, 3, 1, 1)), (rc, (3, 3, 1, 3))):
        assert set(r) == {"sv_sum", "pixels", "annotated", "classes", "ping_edges", "range_edges"}
        assert r["annotated"] == ("background", "sandeel", "other") and r["classes"] == ("sandeel", "other", "all")
        assert r["sv_sum"].shape == r["pixels"].shape == shape
        assert r["sv_sum"].dtype == np.float64 and r["pixels"].dtype == np.int64
    # every echogram has its own edges
    assert ra["ping_edges"].tolist() == [0, 10, 20, 25] and ra["range_edges"].tolist() == [0, 5, 10]
    assert rb["ping_edges"].tolist() == [0, 8] and rb["range_edges"].tolist() == [0, 3]
    assert rc["ping_edges"].tolist() == [0, 10] and rc["range_edges"].tolist() == [0, 5, 10, 12]
    assert ra["pixels"][1, 2, 0, 0] == 12 and ra["sv_sum"][1, 0, 0, 0] == 8.0 and rb["sv_sum"][0, 2, 0, 0] == 7.0
    assert not rc["sv_sum"].any() and not rc["pixels"].any()
    # a result is what a ScoredIntegration of that echogram returns: its recall takes it as it is, and so does nasc
    one = ti.ScoredIntegration(ti.IntegrationSpec(10, 5))
    assert one.recall(1, ra)[1] == 8.0 / 16.0
    assert np.array_equal(ti.nasc(ra, 0.19), 4.0 * np.pi * 1852.0 ** 2 * 0.19 * ra["sv_sum"])
    tot = s.totals()
    assert set(tot) == {"sv_sum", "pixels", "annotated", "classes"}
    assert tot["sv_sum"].shape == tot["pixels"].shape == (3, 3)
    assert tot["sv_sum"].dtype == np.float64 and tot["pixels"].dtype == np.int64
    assert tot["sv_sum"].tolist() == [[3.0, 0.0, 57.0], [8.0, 0.0, 16.0], [0.5, 3.0, 4.0]]
    assert tot["pixels"].tolist() == [[0, 0, 5], [0, 0, 12], [0, 0, 0]]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # empty denominators give NaN without a warning
        r_per, r = s.recall(1)
        p_per, p = s.precision("sandeel")
        ro_per, ro = s.recall("other")
        po_per, po = s.precision(2)
    assert r_per.shape == p_per.shape == (3,) and r_per.dtype == p_per.dtype == np.float64
    assert r_per[0] == 8.0 / 16.0 and np.isnan(r_per[1]) and np.isnan(r_per[2]) and r == 8.0 / 16.0
    assert p_per[0] == 8.0 / 10.5 and p_per[1] == 0.0 and np.isnan(p_per[2]) and p == 8.0 / 11.5
    assert ro_per[0] == 0.75 and np.isnan(ro_per[1:]).all() and ro == 0.75
    assert po_per[0] == 1.0 and np.isnan(po_per[1:]).all() and po == 1.0
    for bad in (0, 3, "all", True, 1.0):
        with pytest.raises(ValueError, match="class"):
            s.recall(bad)


def test_an_empty_set_and_a_child_result():
    e = ti.ScoredIntegrationSet(ti.IntegrationSpec(10, 5, frequency=120, mode="probability"))
    assert e.results() == [] and not e.totals()["sv_sum"].any() and not e.totals()["pixels"].any()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        per, r = e.recall(1)
        assert per.shape == (0,) and np.isnan(r) and np.isnan(e.precision(2)[1])
    assert e.begin([18, 38, 120], 3) is e and e.spec.channel == 2 and e.spec.mode == "probability"
    assert e.begin([18, 38, 120], 3) is e                   # the same model: keeps collecting
    with pytest.raises(ValueError, match="one set per model"):
        e.begin([120, 38], 3)
    # the per-echogram legs hand in what a ScoredIntegration of their own returns
    child = ti.ScoredIntegration(e.spec).begin([18, 38, 120], 3, "cpu", 20, 10)
    child.acc[2, 1, 1, 0], child.acc[2, 2, 1, 0] = 3.0, 4.0
    e.add("solo", child.result())
    assert e.results()[0][0] == "solo" and e.totals()["sv_sum"][2].tolist() == [0.0, 3.0, 4.0]
    assert e.recall(2)[0].tolist() == [0.75] and e.precision(2)[1] == 1.0


def test_the_refusals():
    # 1. a seabed-aware spec, and something that is no spec
    for kw in (dict(seabed_offset=-3), dict(seabed_offset=0, reference="seabed", layers=4)):
        with pytest.raises(NotImplementedError, match="seabed"):
            ti.ScoredIntegrationSet(ti.IntegrationSpec(10, 5, **kw))
    with pytest.raises(TypeError, match="IntegrationSpec"):
        ti.ScoredIntegrationSet({"ping_bin": 10})
    # 2. a model that does not have 3 classes: the set, and the flow before it touches the data
    s = ti.ScoredIntegrationSet(ti.IntegrationSpec(10, 5))
    with pytest.raises(ValueError, match="n_classes=4"):
        s.begin([18, 38], 4)
    with pytest.raises(ValueError, match="frequency 120"):
        ti.ScoredIntegrationSet(ti.IntegrationSpec(10, 5, frequency=120)).begin([18, 38], 3)

    def untouched():
        raise AssertionError("the echograms were touched")
        yield
    pipe = types.SimpleNamespace(model=types.SimpleNamespace(n_classes=4), device="cpu", frequencies=[18, 38])
    with pytest.raises(ValueError, match="n_classes=4"):
        ti.evaluate_echograms_memm(untouched(), pipe, (64, 64), 8, 4, integration=s)
    # 3. the wrong type to the flow: the type check comes first
    for wrong in (ti.IntegrationSpec(10, 5), "set", 1):
        with pytest.raises(TypeError, match="ScoredIntegrationSet"):
            ti.evaluate_echograms_memm(untouched(), None, (64, 64), 8, 4, integration=wrong)
    # 4. a ScoredIntegration has one ping axis: the packed flow still names the per-echogram call
    with pytest.raises(NotImplementedError, match="evaluate_echogram_memm"):
        ti.evaluate_echograms_memm(untouched(), None, (64, 64), 8, 4, integration=ti.ScoredIntegration(ti.IntegrationSpec(10, 5)))
    with pytest.raises(TypeError, match="integration"):     # a near miss of the keyword is a misspelling
        ti.evaluate_echograms_memm(untouched(), pipe, (64, 64), 8, 4, integrations=s)
    assert s.results() == []
