"""CPU: several frequencies in one pass -- the C ABI of ``crimac_integrate_freqs`` (header, binding, the argument checks,
which come before any HIP call) and the host side: a sequence ``frequency`` of ``IntegrationSpec``, the frequency axis of the
results, ``frequency_response``, the refusal by the scored holders.  The kernels: tests/test_gpu_integrate_freqs.py."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQS = [18, 38, 120, 200]
EDGES = [3, 3, 4, 10, 75, 75, 210, 297]


# ---- IntegrationSpec ------------------------------------------------------------------------------------------------------
def test_a_sequence_binds_to_channels_in_the_order_given():
    for seq in ((200, 18, 38), [200, 18, 38]):
        spec = ti.IntegrationSpec(64, 32, frequency=seq, thresholds=(0.25, 1), mode="probability")
        assert spec.multi and spec.n_freqs == 3 and spec.frequency == (200, 18, 38) and spec.channels is None
        bound = spec.bind(FREQS)
        assert bound.channels == (3, 0, 1) and bound.frequency == (200, 18, 38) and bound.n_freqs == 3
        assert type(bound) is ti.IntegrationSpec and (bound.mode, bound.thresholds, bound.ping_bin) == ("probability", (0.25, 1.0), 64)
        assert bound.bins(300, 70) == spec.bins(300, 70) == (5, 3) and bound.touched(100, 200) == 3
    one = ti.IntegrationSpec(64, 32, frequency=(120,)).bind(FREQS)
    assert one.multi and one.channels == (2,) and one.n_freqs == 1
    assert ti.IntegrationSpec(64, 32, frequency=(38000.0, 18000)).bind([18000, 38000, 120000]).channels == (1, 0)
    assert ti.INTEGRATE_MAX_FREQS == 8 and ti.IntegrationSpec(64, 32, frequency=tuple(range(8))).n_freqs == 8


def test_the_three_value_errors():
    with pytest.raises(ValueError, match="empty"):
        ti.IntegrationSpec(64, 32, frequency=())
    with pytest.raises(ValueError, match="twice"):
        ti.IntegrationSpec(64, 32, frequency=[38, 18, 38.0])
    with pytest.raises(ValueError, match=r"IntegrationSpec: frequency 70 is not among the model's frequencies \[18, 38, 120, 200\]"):
        ti.IntegrationSpec(64, 32, frequency=(18, 70)).bind(FREQS)
    with pytest.raises(ValueError, match="8 at most"):
        ti.IntegrationSpec(64, 32, frequency=tuple(range(9)))


def test_the_scalar_spec_is_unchanged():
    assert list(inspect.signature(ti.IntegrationSpec.__init__).parameters) == [
        "self", "ping_bin", "range_bin", "frequency", "thresholds", "mode", "channel", "seabed_offset", "reference", "layers"]
    assert list(inspect.signature(ti.EdsuIntegrationSpec.__init__).parameters)[-1] == "ping_edges"
    spec = ti.IntegrationSpec(64, 32)
    assert not spec.multi and spec.n_freqs == 1 and spec.channels == (None,) and spec.channel is None
    bound = spec.bind(FREQS)
    assert bound.channel == 1 and bound.channels == (1,) and bound.frequency == 38 and not bound.multi
    assert ti.IntegrationSpec(64, 32, frequency=200).bind(FREQS).channel == 3 and bound.bins(300, 70) == (5, 3)
    acc, cnt = ti.new_integration("cpu", bound, 300, 70)
    assert acc.shape == cnt.shape == (3, 5, 3)
    res = ti.integration_result(np.zeros((3, 5, 3)), np.zeros((3, 5, 3), dtype=np.int64), bound, 300, 70)
    assert set(res) == {"sv_sum", "pixels", "ping_edges", "range_edges", "classes"} and res["sv_sum"].shape == (3, 5, 3)
    with pytest.raises(ValueError, match="no frequency axis"):
        ti.frequency_response(res)


def test_the_sequence_is_kept_through_resolve_with_a_callable_table():
    asked = []
    spec = ti.IntegrationSpec(None, 32, frequency=(120, 38), seabed_offset=-3, ping_edges=lambda s: (asked.append(s), EDGES)[1])
    got = spec.bind(FREQS).resolve("reader")
    assert asked == ["reader"] and got.ping_edges.tolist() == EDGES and got.channels == (2, 1) and got.frequency == (120, 38)
    assert got.multi and got.seabed_offset == -3 and type(got) is ti.EdsuIntegrationSpec
    assert spec.resolve("other").channels is None and spec.resolve("other").frequency == (120, 38)
    assert got.bins(10, 70) == (7, 3) and got.touched(100, 200) == 1
    assert got.edges_on("cpu").tolist() == EDGES


def test_new_integration_and_the_group_layout_carry_the_frequency_axis():
    for kw, cols in ((dict(), 3), (dict(seabed_offset=3, reference="seabed", layers=7), 7)):
        spec = ti.IntegrationSpec(64, 32, frequency=(200, 18, 38), **kw).bind(FREQS)
        acc, cnt = ti.new_integration("cpu", spec, 300, 70)
        assert acc.shape == cnt.shape == (3, 3, *spec.bins(300, 70)) == (3, 3, 5, cols)
        assert acc.dtype == torch.float64 and cnt.dtype == torch.int64 and not acc.any()
    spec = ti.IntegrationSpec(64, 32, frequency=(200, 18, 38, 120)).bind(FREQS)
    group = [types.SimpleNamespace(echogram=f"eg{i}", n_pings=p, n_range=r) for i, (p, r) in enumerate([(300, 70), (40, 130), (64, 32)])]
    shares, total = ti.group_shares(group, spec, 3 * spec.n_freqs)
    assert [s for _, s in shares] == [(5, 3), (1, 5), (1, 1)] and [a for a, _ in shares] == [0, 180, 240] and total == 252
    sums, counts = np.arange(total, dtype=np.float64), np.arange(total, dtype=np.int64) * 2
    back = list(ti.group_results(group, shares, sums, counts, spec, 3 * spec.n_freqs))
    assert [eg for eg, _ in back] == ["eg0", "eg1", "eg2"]
    for (at, shape), (_, res) in zip(shares, back):
        n = 12 * shape[0] * shape[1]
        assert res["sv_sum"].shape == res["pixels"].shape == (4, 3, *shape) and res["frequencies"] == (200, 18, 38, 120)
        assert res["sv_sum"].reshape(-1).tolist() == sums[at:at + n].tolist() and "annotated" not in res
        assert res["pixels"].reshape(-1).tolist() == counts[at:at + n].tolist()
        assert not np.shares_memory(res["sv_sum"], sums)
    three = ti.IntegrationSpec(64, 32, frequency=(200, 18, 38)).bind(FREQS)              # 3 F = 9: not the scored layout
    shares, total = ti.group_shares(group[:1], three, 9)
    (_, res), = ti.group_results(group[:1], shares, np.zeros(total), np.zeros(total, dtype=np.int64), three, 9)
    assert "annotated" not in res and res["frequencies"] == (200, 18, 38) and res["sv_sum"].shape == (3, 3, 5, 3)
    scalar = ti.IntegrationSpec(64, 32).bind(FREQS)                                       # the scored layout as before
    (_, res), = ti.group_results(group[:1], shares, np.zeros(total), np.zeros(total, dtype=np.int64), scalar, 9)
    assert res["annotated"] == ti.ANNOTATED_CLASSES and "frequencies" not in res


# ---- the result helpers ---------------------------------------------------------------------------------------------------
def result_4d():
    spec = ti.IntegrationSpec(None, 32, frequency=(200, 38, 18), ping_edges=EDGES).bind(FREQS)
    rng = np.random.Generator(np.random.PCG64(1))
    sums = rng.uniform(0.5, 2.0, size=(3, 3, 7, 3))
    sums[:, :, [0, 4]] = 0                                        # the zero-width cells
    sums[1, 0, 2, 1] = 0                                          # the reference has nothing here
    sums[0, 1, 3, 2] = 0
    return ti.integration_result(sums, np.zeros(sums.shape, dtype=np.int64), spec, 300, 70), sums


def test_integration_result_names_the_frequencies_and_nasc_takes_the_axis():
    res, sums = result_4d()
    assert set(res) == {"sv_sum", "pixels", "ping_edges", "range_edges", "classes", "frequencies"}
    assert res["frequencies"] == (200, 38, 18) and res["ping_edges"].tolist() == EDGES
    total, mean = ti.nasc(res, 0.25), ti.mean_nasc(res, 0.25)
    assert total.shape == mean.shape == (3, 3, 7, 3)
    assert np.array_equal(total, 4.0 * np.pi * 1852.0 ** 2 * 0.25 * sums)
    width = np.diff(EDGES)
    assert np.isnan(mean[:, :, width == 0]).all() and np.isfinite(mean[:, :, width > 0]).all()
    assert np.array_equal(mean[:, :, width > 0], total[:, :, width > 0] / width[width > 0][None, None, :, None])
    fin = ti.finish_integration(torch.zeros((3, 3, 7, 3), dtype=torch.float64), torch.zeros((3, 3, 7, 3), dtype=torch.int64),
                                ti.IntegrationSpec(None, 32, frequency=(200, 38, 18), ping_edges=EDGES).bind(FREQS), 300, 70)
    assert fin["frequencies"] == (200, 38, 18) and fin["sv_sum"].shape == (3, 3, 7, 3)


def test_frequency_response_values_nans_and_errors():
    res, sums = result_4d()
    r = ti.frequency_response(res)                                # the default reference: 38, slice 1
    assert r.shape == sums.shape and r.dtype == np.float64
    has = sums[1] > 0
    for f in range(3):
        assert np.array_equal(r[f][has], sums[f][has] / sums[1][has]) and np.isnan(r[f][~has]).all()
    assert (r[1][has] == 1).all() and r[0, 1, 3, 2] == 0 and np.isnan(r[:, 0, 2, 1]).all() and np.isnan(r[:, :, [0, 4]]).all()
    assert np.array_equal(ti.frequency_response(res, 38), r, equal_nan=True)
    by_200 = ti.frequency_response(res, reference=200)
    assert (by_200[0][sums[0] > 0] == 1).all() and np.isnan(by_200[:, 1, 3, 2]).all()
    hz = dict(res, frequencies=(18000, 38000, 200000))
    assert np.array_equal(ti.frequency_response(hz), r, equal_nan=True)                  # 38 failing, 38000
    with pytest.raises(ValueError, match="reference 120 is not among"):
        ti.frequency_response(res, 120)
    with pytest.raises(ValueError, match="38 / 38000"):
        ti.frequency_response(dict(res, frequencies=(200, 120, 18)))
    with pytest.raises(ValueError, match="no frequency axis"):
        ti.frequency_response({"sv_sum": sums[0]})


# ---- the scored holders ---------------------------------------------------------------------------------------------------
def test_both_scored_holders_refuse_several_frequencies_before_any_data():
    for spec in (ti.IntegrationSpec(64, 32, frequency=(18, 38)), ti.IntegrationSpec(64, 32, frequency=[38])):
        for holder in (ti.ScoredIntegration, ti.ScoredIntegrationSet):
            with pytest.raises(NotImplementedError, match="several frequencies"):
                holder(spec)
    ti.ScoredIntegration(ti.IntegrationSpec(64, 32, frequency=38))
    ti.ScoredIntegrationSet(ti.IntegrationSpec(64, 32))


def test_launch_integration_needs_the_plane_stride_for_a_sequence():
    spec = ti.IntegrationSpec(64, 32, frequency=(18, 38)).bind(FREQS)
    with pytest.raises(ValueError, match="plane_stride"):
        ti.launch_integration(spec, None, True, 70, 300, None, 300, 0, 0, 5, None, None, None)


# ---- header, binding, argument checks -------------------------------------------------------------------------------------
def header():
    with open(os.path.join(ROOT, "include", "crimac_unet_hip.h")) as f:
        return f.read()


def test_header_declares_the_entry_point_and_the_version_stays_17():
    m = re.search(r"int crimac_integrate_freqs\(([^;]*)\);", header())
    assert m, "crimac_integrate_freqs is not declared in the header"
    assert " ".join(m.group(1).split()) == (
        "const void* pred, int pred_f16, int n_range, long n_pings, const float* sv, long plane_stride, int n_planes, "
        "const int* channels, int n_freqs, long data_pings, long sv_ping_off, float thr_sandeel, float thr_other, int mode, "
        "long ping_bin, const long long* edges_dev, const long long* edges_host, int range_bin, long ping_origin, "
        "long n_pb_total, const int* seabed, long seabed_first, long seabed_len, int seabed_offset, int reference, "
        "int n_layers, double* acc, long long* cnt, void* scratch, long scratch_bytes, void* stream")
    i, l, f, vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    want = [vp, i, i, l, vp, l, i, vp, i, l, l, f, f, i, l, vp, vp, i, l, l, vp, l, l, i, i, i, vp, vp, vp, l, vp]
    assert hip.PROTOTYPES["crimac_integrate_freqs"] == (i, want, True) and hip.SIGNATURES["crimac_integrate_freqs"] == want
    # the arguments of crimac_integrate_edges plus ping_bin, the plane arguments in place of nothing
    edges = hip.SIGNATURES["crimac_integrate_edges"]
    assert want[:5] + want[9:14] + want[15:] == edges and want[14] is l
    assert re.search(r"#define CRIMAC_INTEGRATE_MAX_FREQS 8\b", header()) and hip.DEFINES["CRIMAC_INTEGRATE_MAX_FREQS"] == 8
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header()).group(1)) == hip.ABI_VERSION == 17
    text = " ".join(header().split())
    assert "CRIMAC_INTEGRATE_SLOT_BYTES * n_freqs always suffices" in text


def test_the_library_exports_the_symbol():
    lib = hip.load_library()
    assert hasattr(lib, "crimac_integrate_freqs") and lib.crimac_version() == 17


def test_argument_errors_come_before_any_launch():
    """Every refusal precedes the first HIP call, so a pointer that is never dereferenced stands in for device memory."""
    lib = hip.load_library()
    p = ctypes.c_void_p(64)
    keep = (ctypes.c_longlong * len(EDGES))(*EDGES)
    table = ctypes.cast(keep, ctypes.c_void_p)

    def args(channels=(3, 1, 0), n_freqs=None, n_planes=4, stride=400 * 70, sv=p, pred=p, acc=p, cnt=p, scratch_p=p,
             scratch=1 << 22, edges=None, seabed=None, reference=0, layers=0, chan_null=False):
        chan = (ctypes.c_int * max(len(channels), 1))(*channels)
        return [pred, 1, 70, 150, sv, stride, n_planes, None if chan_null else chan, len(channels) if n_freqs is None else n_freqs,
                400, 37, 0.5, 0.5, 0, 64, edges, edges, 32, 0, 3 if edges is None else 7, seabed, 0, 150, -3, reference, layers,
                acc, cnt, scratch_p, scratch, None]
    assert lib.crimac_integrate_freqs(*args(scratch=0)) == -22 and b"scratch" in lib.crimac_last_error()     # (the good call but for it)
    for kw, word in ((dict(pred=None), b"null pointer"), (dict(sv=None), b"null pointer"), (dict(acc=None), b"null pointer"),
                     (dict(cnt=None), b"null pointer"), (dict(scratch_p=None), b"null pointer"),
                     (dict(chan_null=True), b"null pointer"), (dict(channels=(), n_freqs=0), b"n_freqs=0"),
                     (dict(channels=tuple(range(4)) * 3, n_freqs=9, n_planes=16), b"n_freqs=9"),
                     (dict(channels=(3, 4, 0)), b"channels[1]=4 of 4"), (dict(channels=(-1,)), b"channels[0]=-1"),
                     (dict(n_planes=0), b"n_planes=0"), (dict(stride=400 * 70 - 1), b"leave the sv extent"),
                     (dict(seabed=p, reference=2), b"reference"), (dict(seabed=p, reference=1, layers=0), b"n_layers")):
        assert lib.crimac_integrate_freqs(*args(**kw)) == -22, kw
        assert word in lib.crimac_last_error() and b"integrate_freqs" in lib.crimac_last_error(), (kw, lib.crimac_last_error())
    # the scratch: 3 ping bins x 3 range bins = 9 cells, 2 ping tiles x 1 row tile -> 2 splits, times n_freqs
    one = 9 * 2 * hip.INTEGRATE_SLOT_BYTES
    assert lib.crimac_integrate_freqs(*args(scratch=3 * one - 1)) == -22 and str(3 * one).encode() in lib.crimac_last_error()
    assert lib.crimac_integrate_freqs(*args(channels=(3, 1, 0, 2), scratch=one)) == -22
    assert str(4 * one).encode() in lib.crimac_last_error() and b"n_freqs" in lib.crimac_last_error()
    assert lib.crimac_integrate_freqs(*args(channels=(2,), scratch=one - 1)) == -22 and str(one).encode() in lib.crimac_last_error()
    # with the edge table: the geometry of crimac_integrate_edges (pings [0, 150) touch cells 0 .. 5 -> 18 cells, 135 pings
    # clipped to the launch's 150 -> 3 ping tiles), times n_freqs; a bad host table is refused as there
    assert lib.crimac_integrate_freqs(*args(edges=table, scratch=0)) == -22
    assert str(3 * 18 * 3 * hip.INTEGRATE_SLOT_BYTES).encode() in lib.crimac_last_error()
    bad = (ctypes.c_longlong * 8)(3, 3, 4, 10, 75, 74, 210, 297)
    assert lib.crimac_integrate_freqs(*args(edges=ctypes.cast(bad, ctypes.c_void_p))) == -22 and b"decrease" in lib.crimac_last_error()
    del keep


def test_the_documents_describe_the_feature():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    for word in ("Several frequencies in one pass", "frequency_response", "crimac_integrate_freqs", "NotImplementedError",
                 "[F, 3, n_pb, n_rb]"):
        assert word in text, word
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "frequency_response" in f.read()
