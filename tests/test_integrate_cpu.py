"""CPU: the C ABI of ``crimac_integrate_classes`` (header, binding, exported symbol, argument checks, which need no GPU) and
the host side of the echo-integration flows: ``IntegrationSpec``, ``finish_integration``, ``nasc``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import build, hip
from crimac_classifiers_unet_amd import tiled_inference as ti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point_and_the_library_exports_it():
    header = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()
    m = re.search(r"int crimac_integrate_classes\(([^;]*)\);", header)
    assert m, "crimac_integrate_classes is not declared in the header"
    assert " ".join(m.group(1).split()) == (
        "const void* pred, int pred_f16, int n_range, long n_pings, const float* sv, long data_pings, long sv_ping_off, "
        "float thr_sandeel, float thr_other, int mode, long ping_bin, int range_bin, long ping_origin, long n_pb_total, "
        "double* acc, long long* cnt, void* scratch, long scratch_bytes, void* stream")
    i, l, f, vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    want = [vp, i, i, l, vp, l, l, f, f, i, l, i, l, l, vp, vp, vp, l, vp]
    assert hip.PROTOTYPES["crimac_integrate_classes"] == (i, want, True)
    assert hip.SIGNATURES["crimac_integrate_classes"] == want
    assert "integrate.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "integrate.hip"))
    lib = hip.load_library()
    assert hasattr(lib, "crimac_integrate_classes")
    assert (hip.INTEGRATE_SPLIT_WGS, hip.INTEGRATE_SLOT_BYTES) == (1024, 48)


def test_abi_version_is_17():
    header = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION == 17
    assert hip.load_library().crimac_version() == 17


def test_argument_checks_need_no_gpu():
    lib = hip.load_library()
    p = ctypes.c_void_p(64)
    #       pred f16 R   P    sv data off thr0 thr1 mode pbin rbin origin n_pb acc cnt scratch bytes stream
    good = [p, 1, 70, 150, p, 160, 0, 0.5, 0.5, 0, 64, 32, 0, 3, p, p, p, 1 << 20, None]
    for at, value, word in ((7, 0.0, b"thr"), (8, -0.5, b"thr"), (7, float("nan"), b"thr"), (10, 0, b"ping_bin"),
                            (11, 0, b"range_bin"), (6, 11, b"sv extent"), (6, -1, b"sv extent"), (5, 149, b"sv extent"),
                            (12, 43, b"accumulator"), (13, 2, b"accumulator"), (9, 2, b"mode"), (1, 2, b"pred_f16"),
                            (17, 47, b"scratch"), (0, None, b"null"), (14, None, b"null"), (2, 0, b"empty")):
        bad = list(good)
        bad[at] = value
        assert lib.crimac_integrate_classes(*bad) == -22, (at, value)
        assert word in lib.crimac_last_error(), (at, value, lib.crimac_last_error())


def test_integration_spec_validation():
    spec = ti.IntegrationSpec(ping_bin=100, range_bin=64)
    assert (spec.ping_bin, spec.range_bin, spec.thresholds, spec.mode, spec.channel) == (100, 64, (0.5, 0.5), "threshold", None)
    assert spec.bind([18, 38, 120, 200]).channel == 1 and spec.bind([18, 38, 120, 200]).frequency == 38
    assert spec.bind([18000, 38000.0, 120000]).channel == 1                      # a zarr reader's frequencies are in Hz
    assert ti.IntegrationSpec(1, 1, frequency=200).bind([18, 38, 120, 200]).channel == 3
    assert spec.bins(700, 300) == (7, 5) and spec.bins(701, 320) == (8, 5) and ti.IntegrationSpec(1, 1).bins(5, 7) == (5, 7)
    with pytest.raises(ValueError, match="38 / 38000"):
        spec.bind([18, 70, 120])
    with pytest.raises(ValueError, match="frequency 333"):
        ti.IntegrationSpec(1, 1, frequency=333).bind([18, 38])
    for kw in (dict(ping_bin=0, range_bin=1), dict(ping_bin=1, range_bin=-3), dict(ping_bin=2.5, range_bin=1),
               dict(ping_bin=True, range_bin=1)):
        with pytest.raises(ValueError, match="positive integer"):
            ti.IntegrationSpec(**kw)
    for thr in ((0.0, 0.5), (0.5, -0.1), (0.5,), (0.5, float("nan")), (0.5, float("inf")), 0.5):
        with pytest.raises(ValueError, match="thresholds"):
            ti.IntegrationSpec(10, 10, thresholds=thr)
    with pytest.raises(ValueError, match="mode"):
        ti.IntegrationSpec(10, 10, mode="argmax")
    assert ti.IntegrationSpec(10, 10, mode="probability", thresholds=[0.25, 1]).thresholds == (0.25, 1.0)


def test_result_edges_and_shapes_for_a_survey_length_the_bins_do_not_divide():
    spec = ti.IntegrationSpec(ping_bin=100, range_bin=64)
    acc, cnt = ti.new_integration("cpu", spec, 730, 300)
    assert acc.shape == cnt.shape == (3, 8, 5) and acc.dtype == torch.float64 and cnt.dtype == torch.int64
    assert not acc.any() and not cnt.any()
    acc[1, 7, 4], cnt[2, 0, 0] = 2.5, 9
    res = ti.finish_integration(acc, cnt, spec, 730, 300)
    assert set(res) == {"sv_sum", "pixels", "ping_edges", "range_edges", "classes"}
    assert res["classes"] == ("sandeel", "other", "all")
    assert res["sv_sum"].shape == res["pixels"].shape == (3, 8, 5)
    assert res["sv_sum"].dtype == np.float64 and res["pixels"].dtype == np.int64
    assert res["sv_sum"][1, 7, 4] == 2.5 and res["pixels"][2, 0, 0] == 9 and res["sv_sum"].sum() == 2.5
    assert res["ping_edges"].tolist() == [0, 100, 200, 300, 400, 500, 600, 700, 730]
    assert res["range_edges"].tolist() == [0, 64, 128, 192, 256, 300]
    assert res["ping_edges"].dtype == res["range_edges"].dtype == np.int64


def test_nasc_arithmetic():
    res = {"sv_sum": np.array([[[1e-6, 0.0]], [[2e-6, 5e-7]], [[4e-6, 1e-6]]])}
    got = ti.nasc(res, 0.19)
    assert got.shape == (3, 1, 2) and got.dtype == np.float64
    assert np.array_equal(got, 4.0 * np.pi * 1852.0 ** 2 * 0.19 * res["sv_sum"])
    assert got[0, 0, 0] == pytest.approx(4 * 3.141592653589793 * 3429904.0 * 0.19e-6, rel=1e-15) and got[0, 0, 1] == 0
    assert "uniform" in ti.nasc.__doc__.lower()


def test_flows_have_the_documented_signatures():
    import inspect
    assert list(inspect.signature(ti.integrate_survey).parameters) == [
        "reader", "segpipe", "patch_size", "patch_overlap", "batch_size", "preload_n_pings", "spec", "start_ping",
        "labels_available", "predict_fn", "stats"]
    assert list(inspect.signature(ti.integrate_echogram_memm).parameters) == [
        "echogram", "segpipe", "patch_size", "patch_overlap", "batch_size", "spec", "predict_fn", "meta_channels", "seabed"]
    assert "predict_echograms_memm" in ti.integrate_echogram_memm.__doc__          # the packed flow is named as out of scope
    assert list(inspect.signature(ti.ChunkPredictor.integrate).parameters) == ["self", "acc", "cnt", "spec"]
