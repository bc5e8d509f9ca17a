"""CPU: the C ABI of ``crimac_integrate_layers`` (header, binding, exported symbol, argument checks, which need no GPU) and the
host side of seabed-aware echo integration: the ``IntegrationSpec`` keywords, ``finish_integration``, the signature and
the argument checks of ``integrate_echograms_memm``."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "crimac_unet_hip.h")) as f:
        return f.read()


def test_header_declares_the_entry_point_and_the_binding_derives_it():
    m = re.search(r"int crimac_integrate_layers\(([^;]*)\);", header())
    assert m, "crimac_integrate_layers is not declared in the header"
    assert " ".join(m.group(1).split()) == (
        "const void* pred, int pred_f16, int n_range, long n_pings, const float* sv, long data_pings, long sv_ping_off, "
        "float thr_sandeel, float thr_other, int mode, long ping_bin, int range_bin, long ping_origin, long n_pb_total, "
        "const int* seabed, long seabed_first, long seabed_len, int seabed_offset, int reference, int n_layers, "
        "double* acc, long long* cnt, void* scratch, long scratch_bytes, void* stream")
    i, l, f, vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    want = [vp, i, i, l, vp, l, l, f, f, i, l, i, l, l, vp, l, l, i, i, i, vp, vp, vp, l, vp]
    assert hip.PROTOTYPES["crimac_integrate_layers"] == (i, want, True)
    assert hip.SIGNATURES["crimac_integrate_layers"] == want
    # the arguments of crimac_integrate_classes, in its order, around the six new ones
    old = hip.SIGNATURES["crimac_integrate_classes"]
    assert want[:14] == old[:14] and want[20:] == old[14:]


def test_the_library_exports_the_symbol_and_the_abi_version_is_still_17():
    lib = hip.load_library()
    assert hasattr(lib, "crimac_integrate_layers")
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header()).group(1)) == hip.ABI_VERSION == 17
    assert lib.crimac_version() == 17
    assert "additive" in header().lower()                       # the header states the rule for additive entry points


def test_a_build_without_the_symbol_is_refused_with_the_rebuild_message(monkeypatch):
    """A library of the same ABI version from before the entry point was added: ``load_library`` must say "rebuild", not
    fail with an AttributeError at the first call.  The loaded library stands in for it, under a prototype it lacks."""
    hip.load_library()
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setitem(hip.PROTOTYPES, "crimac_integrate_layers_of_a_later_header", hip.PROTOTYPES["crimac_integrate_layers"])
    with pytest.raises(hip.HipLibraryError, match=r"crimac_integrate_layers_of_a_later_header.*rebuild"):
        hip.load_library()


def test_argument_checks_need_no_gpu():
    lib = hip.load_library()
    p = ctypes.c_void_p(64)
    #       pred f16 R   P    sv data off thr0 thr1 mode pbin rbin origin n_pb seabed first len offset ref layers acc cnt scratch bytes
    good = [p, 1, 70, 150, p, 160, 0, 0.5, 0.5, 0, 64, 32, 0, 3, p, 5, 155, -3, 1, 2, p, p, p, 1 << 20, None]
    # what crimac_integrate_classes checks
    old = ((7, 0.0, b"thr"), (8, -0.5, b"thr"), (7, float("nan"), b"thr"), (10, 0, b"ping_bin"), (11, 0, b"range_bin"),
           (6, 11, b"sv extent"), (6, -1, b"sv extent"), (5, 149, b"sv extent"), (12, 43, b"accumulator"),
           (13, 2, b"accumulator"), (9, 2, b"mode"), (1, 2, b"pred_f16"), (23, 47, b"scratch"), (0, None, b"null"),
           (20, None, b"null"), (2, 0, b"empty"))
    # what the new arguments add
    new = ((14, None, b"seabed"), (15, 6, b"seabed"), (15, -1, b"seabed"), (16, 154, b"seabed"), (18, 2, b"reference"),
           (18, -1, b"reference"), (19, 0, b"n_layers"), (19, -4, b"n_layers"))
    for at, value, word in old + new:
        bad = list(good)
        bad[at] = value
        assert lib.crimac_integrate_layers(*bad) == -22, (at, value)
        assert word in lib.crimac_last_error(), (at, value, lib.crimac_last_error())
        assert b"integrate_layers" in lib.crimac_last_error()
    # the surface reference does not read n_layers: with it the first failing check is the scratch, not the layer count
    surface = list(good)
    surface[18], surface[19], surface[23] = 0, 0, 47
    assert lib.crimac_integrate_layers(*surface) == -22 and b"scratch" in lib.crimac_last_error()
    # a scratch of (cells + CRIMAC_INTEGRATE_SPLIT_WGS) slots is refused one byte short of what the launch needs only:
    # cells = 3 ping bins x 2 layers, splits = min(ceil(1024 / 6), tiles of a whole column = 2 x 2) = 4
    short = list(good)
    short[23] = 6 * 4 * hip.INTEGRATE_SLOT_BYTES - 1
    assert lib.crimac_integrate_layers(*short) == -22 and b"scratch" in lib.crimac_last_error()


def test_spec_validation_of_the_seabed_keywords():
    spec = ti.IntegrationSpec(64, 32)
    assert (spec.seabed_offset, spec.reference, spec.layers) == (None, "surface", None) and not spec.seabed_aware
    assert list(inspect.signature(ti.IntegrationSpec.__init__).parameters) == [
        "self", "ping_bin", "range_bin", "frequency", "thresholds", "mode", "channel", "seabed_offset", "reference", "layers"]
    cut = ti.IntegrationSpec(64, 32, seabed_offset=-5)
    assert (cut.seabed_offset, cut.reference, cut.layers) == (-5, "surface", None) and cut.seabed_aware
    assert ti.IntegrationSpec(64, 32, seabed_offset=np.int64(10)).seabed_offset == 10
    assert ti.IntegrationSpec(64, 32, seabed_offset=0).seabed_aware
    lay = ti.IntegrationSpec(64, 32, seabed_offset=0, reference="seabed", layers=np.int32(4))
    assert (lay.seabed_offset, lay.reference, lay.layers) == (0, "seabed", 4) and type(lay.layers) is int
    with pytest.raises(ValueError, match="seabed_offset"):
        ti.IntegrationSpec(64, 32, reference="seabed", layers=4)
    with pytest.raises(ValueError, match="layers"):
        ti.IntegrationSpec(64, 32, reference="seabed", seabed_offset=0)
    with pytest.raises(ValueError, match="layers"):
        ti.IntegrationSpec(64, 32, seabed_offset=0, layers=4)
    with pytest.raises(ValueError, match="layers"):
        ti.IntegrationSpec(64, 32, layers=4)
    with pytest.raises(ValueError, match="reference"):
        ti.IntegrationSpec(64, 32, seabed_offset=0, reference="bottom")
    for bad in (1.5, True, False, "3", (1,)):
        with pytest.raises(ValueError, match="seabed_offset"):
            ti.IntegrationSpec(64, 32, seabed_offset=bad)
    for bad in (0, -2, 2.0, True, "4"):
        with pytest.raises(ValueError, match="layers"):
            ti.IntegrationSpec(64, 32, seabed_offset=0, reference="seabed", layers=bad)


def test_bins_and_bind_for_both_references():
    cut = ti.IntegrationSpec(100, 64, seabed_offset=-5)
    lay = ti.IntegrationSpec(100, 64, seabed_offset=3, reference="seabed", layers=7, mode="probability", thresholds=(0.25, 1))
    assert cut.bins(730, 300) == (8, 5) and lay.bins(730, 300) == (8, 7) and lay.bins(1, 10) == (1, 7)
    for spec in (cut, lay):
        bound = spec.bind([18, 38, 120, 200])
        assert bound.channel == 1 and bound.frequency == 38
        assert (bound.seabed_offset, bound.reference, bound.layers) == (spec.seabed_offset, spec.reference, spec.layers)
        assert (bound.ping_bin, bound.range_bin, bound.thresholds, bound.mode) == (100, 64, spec.thresholds, spec.mode)
        assert bound.bins(730, 300) == spec.bins(730, 300)
    acc, cnt = ti.new_integration("cpu", lay, 730, 300)
    assert acc.shape == cnt.shape == (3, 8, 7)
    assert "from the limit" in " ".join(ti.IntegrationSpec.__doc__.lower().split())


def test_finish_integration_keys_and_layer_edges():
    old_keys = {"sv_sum", "pixels", "ping_edges", "range_edges", "classes"}
    spec = ti.IntegrationSpec(100, 64)
    res = ti.finish_integration(*ti.new_integration("cpu", spec, 730, 300), spec, 730, 300)
    assert set(res) == old_keys and res["range_edges"].tolist() == [0, 64, 128, 192, 256, 300]
    cut = ti.IntegrationSpec(100, 64, seabed_offset=-5)
    res = ti.finish_integration(*ti.new_integration("cpu", cut, 730, 300), cut, 730, 300)
    assert set(res) == old_keys | {"reference", "seabed_offset"}
    assert (res["reference"], res["seabed_offset"]) == ("surface", -5)
    assert res["range_edges"].tolist() == [0, 64, 128, 192, 256, 300]
    lay = ti.IntegrationSpec(100, 64, seabed_offset=10, reference="seabed", layers=7)
    acc, cnt = ti.new_integration("cpu", lay, 730, 300)
    acc[0, 7, 6], cnt[2, 0, 0] = 1.5, 4
    res = ti.finish_integration(acc, cnt, lay, 730, 300)
    assert set(res) == old_keys | {"reference", "seabed_offset"}
    assert (res["reference"], res["seabed_offset"]) == ("seabed", 10)
    assert res["sv_sum"].shape == res["pixels"].shape == (3, 8, 7)
    assert res["sv_sum"][0, 7, 6] == 1.5 and res["pixels"][2, 0, 0] == 4
    # heights above the limit: not clipped to the column (7 layers of 64 rows reach past 300 rows)
    assert res["range_edges"].tolist() == [0, 64, 128, 192, 256, 320, 384, 448] and res["range_edges"].dtype == np.int64
    assert res["ping_edges"].tolist() == [0, 100, 200, 300, 400, 500, 600, 700, 730]
    assert "not from the surface" in " ".join(ti.finish_integration.__doc__.split())


def test_integrate_echograms_memm_signature_and_refusals():
    assert list(inspect.signature(ti.integrate_echograms_memm).parameters) == [
        "echograms", "segpipe", "patch_size", "patch_overlap", "batch_size", "spec", "predict_fn", "meta_channels", "seabed",
        "group_patches", "stats", "group_elems", "skip", "pack_metadata", "kwargs"]
    assert inspect.signature(ti.integrate_echograms_memm).parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert inspect.isgeneratorfunction(ti.integrate_echograms_memm)
    pipe, spec = None, ti.IntegrationSpec(64, 32)              # (the pipe is never touched: the checks come first)
    with pytest.raises(TypeError, match=r"integrate_echograms_memm: unknown keyword\(s\) 'group_patch' \(did you mean"):
        next(ti.integrate_echograms_memm(iter([]), pipe, (32, 32), 4, 8, spec, group_patch=40))
    for typo in ("group_elem", "seabeds", "stat", "specs", "pack_metadatas"):
        with pytest.raises(TypeError, match="integrate_echograms_memm: unknown keyword"):
            next(ti.integrate_echograms_memm(iter([]), pipe, (32, 32), 4, 8, spec, **{typo: None}))
    for bad in (np.zeros(10, dtype=np.int64), [np.zeros(10, dtype=np.int64)], "guess"):
        with pytest.raises(TypeError, match="integrate_echogram_memm takes one"):
            next(ti.integrate_echograms_memm(iter([]), pipe, (32, 32), 4, 8, spec, seabed=bad))
    assert "integrate_echograms_memm" in ti.integrate_echogram_memm.__doc__
    assert "integrate_echograms_memm" in ti.__doc__


def test_chunk_predictor_mask_line_is_the_first_masked_row(monkeypatch):
    """The limit line of a chunk that holds a 2-D mask (torch on whatever device holds it): first masked row, n_range where a
    ping has none -- holes below the first masked row do not move it."""
    cp = ti.ChunkPredictor.__new__(ti.ChunkPredictor)
    mask = np.zeros((6, 9), dtype=np.uint8)
    mask[0, 4:] = 1
    mask[1, :] = 1
    mask[3, 8] = 1
    mask[4, 2:5] = 1
    mask[4, 7:] = 1
    mask[5, 5] = 7                                              # (any non-zero value masks)
    cp.seabed, cp.mask, cp.mask_line, cp.n_range, cp.start_ping = None, torch.from_numpy(mask), None, 9, 40
    monkeypatch.setattr(ti, "ptr", lambda t, off=0: t)          # (no GPU here: hand the tensor itself back)
    line, first, length = cp._limit_line()
    assert (first, length) == (0, 6) and line.dtype == torch.int32 and line.tolist() == [4, 0, 9, 8, 2, 5]
    cp.mask = cp.mask_line = None
    with pytest.raises(ValueError, match="neither"):
        cp._limit_line()
