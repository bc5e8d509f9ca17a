"""CPU: echo integration per EDSU -- the C ABI of ``crimac_integrate_edges`` (header, binding, the host-side checks of the
edge table, which need no GPU) and the host side of the feature: ``ping_bin_edges``, the ``ping_edges`` keyword of
``IntegrationSpec``, ``mean_nasc``, the refusal by the scored holders.

``edges_numpy`` below is the numpy statement of the kernel with an edge table, the yardstick of
tests/test_gpu_integrate_edsu.py; it is checked here against a per-pixel Python loop."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("threshold", "probability")
EDGES = [3, 3, 4, 10, 75, 75, 210, 297]        # two zero-width cells, a 1-ping cell, a cell wider than two 64-ping tiles


# ---- the numpy statement of the kernel --------------------------------------------------------------------------------
def edges_numpy(acc, cnt, geo, pred, sv, thr, mode, edges, range_bin, ping_origin, sv_ping_off=0, line=None, offset=None,
                reference="surface"):
    """One launch of ``crimac_integrate_edges``, accumulated into ``acc`` float64 / ``cnt`` int64 [3, n_pb, n_cols] and
    ``geo`` int64 [n_pb, n_cols] (the pixels of the launch that lie in the cell, for the error bound).  ``pred`` [2, R, P] as
    stored (float16 / float32), ``sv`` [data_pings, R] float32, ``edges`` [n_pb + 1] global pings, ``ping_origin`` the global
    ping of pred's column 0.  ``offset`` given: ``line`` int [P] is the seabed row of every ping of the launch and rows at or
    below ``clip(line + offset, 0, R)`` count nowhere; ``reference`` "seabed": the columns are layers counted from it."""
    R, P = pred.shape[1:]
    n_pb, n_cols = acc.shape[1:]
    edges = np.asarray(edges, dtype=np.int64)
    assert len(edges) == n_pb + 1
    s = np.asarray(sv[sv_ping_off:sv_ping_off + P], dtype=np.float32).T               # [R, P]
    assert s.shape == (R, P)
    g = ping_origin + np.arange(P)
    pb = np.searchsorted(edges, g, "right") - 1                  # the LAST cell that starts at or before the ping
    inside = (g >= edges[0]) & (g < edges[-1])
    L = np.full(P, R) if offset is None else np.clip(np.asarray(line).astype(np.int64) + offset, 0, R)
    r = np.arange(R)[:, None]
    geom = inside[None, :] & (r < L[None, :])
    if reference == "seabed":
        col = (L[None, :] - 1 - r) // range_bin                  # layer 0 touches the limit
        geom = geom & (col < n_cols)                             # rows above the top layer are dropped
    else:
        col = np.broadcast_to(r // range_bin, (R, P))
    ok = geom & np.isfinite(s) & (s > 0)
    s64 = np.where(ok, s, 0).astype(np.float64)
    p32 = pred.astype(np.float32)                                # the stored value, widened exactly
    if mode == "threshold":
        member = p32 >= np.asarray(thr, dtype=np.float32)[:, None, None]             # a float32 comparison
        weight = member.astype(np.float64)
    else:
        member = p32 > 0
        weight = np.where(member, p32, 0).astype(np.float64)
    cell = np.broadcast_to(pb[None, :], (R, P)) * n_cols + col
    size = n_pb * n_cols
    geo += np.bincount(cell[geom], minlength=size).reshape(n_pb, n_cols)
    planes = ((s64 * weight[0], ok & member[0]), (s64 * weight[1], ok & member[1]), (s64, ok))
    for k, (terms, counted) in enumerate(planes):
        cnt[k] += np.bincount(cell[counted], minlength=size).reshape(n_pb, n_cols)
        acc[k] += np.bincount(cell[counted], weights=terms[counted], minlength=size).reshape(n_pb, n_cols)


def new_host(n_pb, n_cols):
    return np.zeros((3, n_pb, n_cols)), np.zeros((3, n_pb, n_cols), dtype=np.int64), np.zeros((n_pb, n_cols), dtype=np.int64)


def pixel_loop(pred, sv, thr, mode, edges, range_bin, ping_origin, n_cols, line, offset, reference):
    """The same, one pixel at a time: lists of terms per (plane, cell), summed exactly at the end."""
    R, P = pred.shape[1:]
    n_pb = len(edges) - 1
    terms = [[[[] for _ in range(n_cols)] for _ in range(n_pb)] for _ in range(3)]
    cnt = np.zeros((3, n_pb, n_cols), dtype=np.int64)
    for p in range(P):
        g = ping_origin + p
        cells = [k for k in range(n_pb) if edges[k] <= g < edges[k + 1]]
        assert len(cells) <= 1
        if not cells:
            continue
        L = R if offset is None else min(max(int(line[p]) + offset, 0), R)
        for r in range(R):
            v = float(sv[p, r])
            if r >= L or not (math.isfinite(v) and v > 0):
                continue
            col = (L - 1 - r) // range_bin if reference == "seabed" else r // range_bin
            if col >= n_cols:
                continue
            for k in range(2):
                a = float(np.float32(pred[k, r, p]))
                w = (1.0 if a >= float(np.float32(thr[k])) else 0.0) if mode == "threshold" else (a if a > 0 else 0.0)
                if w > 0:
                    terms[k][cells[0]][col].append(v * w)
                    cnt[k, cells[0], col] += 1
            terms[2][cells[0]][col].append(v)
            cnt[2, cells[0], col] += 1
    return np.array([[[math.fsum(c) for c in row] for row in plane] for plane in terms]), cnt


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("reference,offset", [("surface", None), ("surface", -1), ("seabed", 2)])
def test_edges_numpy_against_a_per_pixel_loop_on_9_x_23(reference, offset, mode):
    """Dyadic sv and float16 probabilities: every sum is exact in any order, so the two must agree with ``==``."""
    rng = np.random.Generator(np.random.PCG64(5))
    R, P, range_bin, origin = 9, 23, 4, 100
    edges = [102, 102, 103, 110, 110, 119, 121]                  # pings 100, 101 and 121, 122 lie in no cell
    pred = (rng.integers(0, 1025, size=(2, R, P)) / 1024.0).astype(np.float16)
    pred[rng.random(pred.shape) < 0.3] = 0
    sv = (rng.integers(1, 1 << 12, size=(P + 4, R)) * 2.0 ** -20).astype(np.float32)
    hit = rng.random(sv.shape) < 0.1
    sv[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.25], dtype=np.float32), size=int(hit.sum()))
    line = rng.integers(-2, R + 3, size=P)
    n_cols = 2 if reference == "seabed" else 3
    want_sum, want_cnt = pixel_loop(pred, sv[4:], (0.5, 0.25), mode, edges, range_bin, origin, n_cols, line, offset, reference)
    acc, cnt, geo = new_host(6, n_cols)
    edges_numpy(acc, cnt, geo, pred, sv, (0.5, 0.25), mode, edges, range_bin, origin, 4, line, offset, reference)
    assert np.array_equal(cnt, want_cnt) and np.array_equal(acc, want_sum)
    assert cnt[2].sum() > 20 and (cnt[:, [0, 3]] == 0).all() and (acc[:, [0, 3]] == 0).all()      # the zero-width cells
    assert (geo >= cnt[2]).all() and (geo[[0, 3]] == 0).all()
    if offset is None:
        assert geo.sum() == R * 19 and geo[1].tolist() == [4, 4, 1]                    # 19 pings inside, a 1-ping cell
    # two launches over the same pings add up to the one
    acc2, cnt2, geo2 = new_host(6, n_cols)
    for p0, p1 in ((0, 11), (11, P)):
        edges_numpy(acc2, cnt2, geo2, pred[:, :, p0:p1], sv, (0.5, 0.25), mode, edges, range_bin, origin + p0, 4 + p0,
                    line[p0:p1], offset, reference)
    assert np.array_equal(cnt2, cnt) and np.array_equal(acc2, acc) and np.array_equal(geo2, geo)


def test_edges_numpy_with_uniform_edges_is_the_uniform_binning():
    rng = np.random.Generator(np.random.PCG64(6))
    R, P = 10, 50
    pred = rng.random((2, R, P)).astype(np.float16)
    sv = (rng.integers(1, 1 << 12, size=(P, R)) * 2.0 ** -20).astype(np.float32)
    acc, cnt, geo = new_host(4, 3)
    edges_numpy(acc, cnt, geo, pred, sv, (0.5, 0.5), "threshold", np.arange(5) * 16, 4, 7)
    pb = (7 + np.arange(P)) // 16
    for b in range(4):
        for rb in range(3):
            block = sv[pb == b][:, 4 * rb:4 * rb + 4].astype(np.float64)
            assert acc[2, b, rb] == block.sum() and cnt[2, b, rb] == geo[b, rb] == block.size


# ---- header and binding ---------------------------------------------------------------------------------------------------
def header():
    with open(os.path.join(ROOT, "include", "crimac_unet_hip.h")) as f:
        return f.read()


def test_header_declares_the_entry_point_and_the_binding_derives_it():
    m = re.search(r"int crimac_integrate_edges\(([^;]*)\);", header())
    assert m, "crimac_integrate_edges is not declared in the header"
    assert " ".join(m.group(1).split()) == (
        "const void* pred, int pred_f16, int n_range, long n_pings, const float* sv, long data_pings, long sv_ping_off, "
        "float thr_sandeel, float thr_other, int mode, const long long* edges_dev, const long long* edges_host, "
        "int range_bin, long ping_origin, long n_pb_total, const int* seabed, long seabed_first, long seabed_len, "
        "int seabed_offset, int reference, int n_layers, double* acc, long long* cnt, void* scratch, long scratch_bytes, "
        "void* stream")
    i, l, f, vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    want = [vp, i, i, l, vp, l, l, f, f, i, vp, vp, i, l, l, vp, l, l, i, i, i, vp, vp, vp, l, vp]
    assert hip.PROTOTYPES["crimac_integrate_edges"] == (i, want, True)
    assert hip.SIGNATURES["crimac_integrate_edges"] == want
    # everything crimac_integrate_layers takes except ping_bin, the two tables in its place
    old = hip.SIGNATURES["crimac_integrate_layers"]
    assert want[:10] == old[:10] and want[12:] == old[11:] and len(want) == len(old) + 1
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header()).group(1)) == hip.ABI_VERSION == 17


def test_the_library_exports_the_symbol_and_the_uniform_prototypes_are_unchanged():
    lib = hip.load_library()
    assert hasattr(lib, "crimac_integrate_edges") and lib.crimac_version() == 17
    text = " ".join(header().split())
    assert ("int crimac_integrate_classes(const void* pred, int pred_f16, int n_range, long n_pings, const float* sv, "
            "long data_pings, long sv_ping_off, float thr_sandeel, float thr_other, int mode, long ping_bin, int range_bin, "
            "long ping_origin, long n_pb_total, double* acc, long long* cnt, void* scratch, long scratch_bytes, "
            "void* stream);") in text
    assert "(cells touched + CRIMAC_INTEGRATE_SPLIT_WGS) * CRIMAC_INTEGRATE_SLOT_BYTES" in text


def table(values):
    a = (ctypes.c_longlong * len(values))(*values)
    return a, ctypes.cast(a, ctypes.c_void_p)


def test_the_host_table_is_checked_without_a_gpu():
    """Every refusal comes before the launch, so a pointer that is never dereferenced stands in for device memory."""
    lib = hip.load_library()
    p = ctypes.c_void_p(64)
    keep, host = table(EDGES)

    def args(host=host, n_pb=7, origin=0, n_pings=300, seabed=None, reference=0, layers=0, scratch=1 << 20, dev=p):
        #       pred f16 R  P        sv data off thr0 thr1 mode edges        rbin origin n_pb seabed first len offset ref
        return [p, 1, 70, n_pings, p, 400, 37, 0.5, 0.5, 0, dev, host, 32, origin, n_pb, seabed, 0, 300, -3, reference,
                layers, p, p, p, scratch, None]
    for bad, word in (([3, 3, 4, 10, 75, 74, 210, 297], b"decrease"), ([-1, 3, 4, 10, 75, 75, 210, 297], b"negative"),
                      ([3, 3, 4, 10, 75, 75, 210, 210 + 2 ** 31], b"2^31")):
        keep_bad, host_bad = table(bad)
        assert lib.crimac_integrate_edges(*args(host=host_bad)) == -22, bad
        assert word in lib.crimac_last_error() and b"integrate_edges" in lib.crimac_last_error()
    for kw, word in ((dict(n_pb=0), b"accumulator"), (dict(host=None), b"edge table"), (dict(dev=None), b"edge table"),
                     (dict(origin=-1), b"accumulator"), (dict(seabed=p, reference=2), b"reference"),
                     (dict(seabed=p, reference=1, layers=0), b"n_layers")):
        assert lib.crimac_integrate_edges(*args(**kw)) == -22, kw
        assert word in lib.crimac_last_error(), (kw, lib.crimac_last_error())
    # the scratch: the launch over pings [0, 300) touches cells 0 .. 6 (the zero-width ones included) x 3 range bins = 21
    # cells; the widest, 135 pings -> (135 + 3 + 63) // 64 = 3 ping tiles x 1 row tile, splits = min(ceil(1024 / 21), 3) = 3
    need = 21 * 3 * hip.INTEGRATE_SLOT_BYTES
    assert need <= (21 + hip.INTEGRATE_SPLIT_WGS) * hip.INTEGRATE_SLOT_BYTES
    assert lib.crimac_integrate_edges(*args(scratch=need - 1)) == -22 and b"scratch" in lib.crimac_last_error()
    assert str(need).encode() in lib.crimac_last_error()
    # pings [100, 200) touch cells 5 only -> 3 cells; 135 pings clipped to the launch's 100 -> 2 ping tiles
    need = 3 * 2 * hip.INTEGRATE_SLOT_BYTES
    assert lib.crimac_integrate_edges(*args(origin=100, n_pings=100, scratch=need - 1)) == -22
    assert str(need).encode() in lib.crimac_last_error()
    # with uniform edges the same requirement as the uniform entry point states: 3 ping bins x 2 layers, 4 splits
    keep_u, host_u = table([0, 64, 128, 192])
    assert lib.crimac_integrate_edges(*args(host=host_u, n_pb=3, n_pings=150, seabed=p, reference=1, layers=2,
                                            scratch=6 * 4 * hip.INTEGRATE_SLOT_BYTES - 1)) == -22
    assert str(6 * 4 * hip.INTEGRATE_SLOT_BYTES).encode() in lib.crimac_last_error()
    # a launch that touches no cell is no error and launches nothing (no device is needed to return)
    assert lib.crimac_integrate_edges(*args(origin=297, n_pings=50, scratch=0)) == 0
    assert lib.crimac_integrate_edges(*args(origin=0, n_pings=3, scratch=0)) == 0
    del keep, keep_u


# ---- ping_bin_edges -------------------------------------------------------------------------------------------------------
def edges_by_loop(track, step, origin=None):
    track = [float(v) for v in track]
    origin = track[0] if origin is None else float(origin)
    K = math.floor((track[-1] - origin) / step) + 1
    out = []
    for k in range(K + 1):
        bound = origin + k * step
        out.append(sum(1 for v in track if v < bound))           # searchsorted 'left' on a sorted track
    out[-1] = len(track)
    return out


TRACKS = {
    "even": (np.arange(20) * 0.03, 0.1, None),
    "a gap of three units": ([0.0, 0.02, 0.05, 0.09, 0.41, 0.43, 0.5], 0.1, None),
    "repeats on a boundary": ([0.0, 0.05, 0.1, 0.1, 0.1, 0.15, 0.2, 0.2], 0.1, None),
    "a later origin": (np.arange(30) * 0.01, 0.1, 0.055),
    "an earlier origin": (np.arange(30) * 0.01 + 1.0, 0.1, 0.93),
    "step larger than the track": ([5.0, 5.5, 6.0, 7.25], 100.0, None),
    "a single ping": ([12.5], 1.0, None),
    "a standing vessel": ([3.0, 3.0, 3.0, 3.0], 0.1, None),
    "a time vector": (737000.5 + np.cumsum(np.full(50, 7e-6)), 1e-4, None),
}


@pytest.mark.parametrize("name", list(TRACKS))
def test_ping_bin_edges_against_a_brute_force_loop(name):
    track, step, origin = TRACKS[name]
    got = ti.ping_bin_edges(track, step, origin)
    assert got.dtype == np.int64 and got.ndim == 1 and got.tolist() == edges_by_loop(track, step, origin)
    assert got[-1] == len(track) and (np.diff(got) >= 0).all() and got[0] >= 0
    ti.IntegrationSpec(None, 5, ping_edges=got)                  # what it returns is a table the spec takes


def test_ping_bin_edges_on_hand_written_tracks():
    assert ti.ping_bin_edges([0.0, 0.02, 0.05, 0.09, 0.41, 0.43, 0.5], 0.1).tolist() == [0, 4, 4, 4, 4, 6, 7]   # zero-width cells
    assert ti.ping_bin_edges([0.0, 0.05, 0.1, 0.1, 0.1, 0.15, 0.2, 0.2], 0.1).tolist() == [0, 2, 6, 8]          # repeats: one cell
    assert ti.ping_bin_edges(np.arange(30) * 0.01, 0.1, origin=0.055).tolist() == [6, 16, 26, 30]                 # 6 pings uncounted
    assert ti.ping_bin_edges([5.0, 5.5, 6.0, 7.25], 100.0).tolist() == [0, 4]
    assert ti.ping_bin_edges([12.5], 1.0).tolist() == [0, 1]
    assert ti.ping_bin_edges(np.arange(6), 2).tolist() == [0, 2, 4, 6]                                            # an integer track


def test_ping_bin_edges_refuses_what_is_no_track():
    for bad in ([0.0, 0.2, 0.1], [0.0, np.nan, 1.0], [0.0, np.inf], [], np.zeros((2, 3))):
        with pytest.raises(ValueError, match="ping_bin_edges: track"):
            ti.ping_bin_edges(bad, 0.1)
    for step in (0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="step"):
            ti.ping_bin_edges([0.0, 1.0], step)
    for origin in (np.nan, 1.5):
        with pytest.raises(ValueError, match="origin"):
            ti.ping_bin_edges([0.0, 1.0], 0.1, origin=origin)


# ---- IntegrationSpec ------------------------------------------------------------------------------------------------------
def test_spec_validation_of_ping_edges():
    spec = ti.IntegrationSpec(None, 32, ping_edges=EDGES)
    assert isinstance(spec, ti.IntegrationSpec) and spec.ping_bin is None and spec.range_bin == 32
    assert spec.ping_edges.dtype == np.int64 and spec.ping_edges.tolist() == EDGES and not spec.ping_edges.flags.writeable
    assert ti.IntegrationSpec(ping_bin=None, range_bin=32, ping_edges=np.array(EDGES, dtype=np.uint16)).ping_edges.tolist() == EDGES
    assert "ping_edges" in inspect.signature(type(spec).__init__).parameters
    mine = np.array(EDGES)
    assert ti.IntegrationSpec(None, 32, ping_edges=mine).ping_edges is not mine and mine.flags.writeable
    with pytest.raises(ValueError, match="ping_bin=64 and ping_edges"):
        ti.IntegrationSpec(64, 32, ping_edges=EDGES)
    for neither in (lambda: ti.IntegrationSpec(None, 5), lambda: ti.IntegrationSpec(None, 5, ping_edges=None)):
        with pytest.raises(ValueError, match="ping_bin=None must be a positive integer"):
            neither()
    for bad in ([3, 3, 4, 10, 75, 74], [-1, 3], [[0, 5], [5, 9]], [0.0, 5.0], [7], [], [0, 2 ** 31], "edges", 5):
        with pytest.raises(ValueError, match="ping_edges"):
            ti.IntegrationSpec(None, 32, ping_edges=bad)
    with pytest.raises(ValueError, match="range_bin"):
        ti.IntegrationSpec(None, 0, ping_edges=EDGES)
    # without the keyword everything is as it was
    plain = ti.IntegrationSpec(64, 32)
    assert type(plain) is ti.IntegrationSpec and plain.ping_edges is None and plain.ping_bin == 64
    assert type(plain.bind([18, 38])) is ti.IntegrationSpec and plain.resolve(object()) is plain


def test_a_callable_is_asked_per_source_and_its_answer_checked():
    asked = []

    def per_source(source):
        asked.append(source)
        return source["edges"]
    spec = ti.IntegrationSpec(None, 32, ping_edges=per_source, seabed_offset=-3, mode="probability")
    assert spec.ping_edges is per_source and not asked
    with pytest.raises(ValueError, match="resolve"):
        spec.bins(300, 70)
    a, b = {"edges": EDGES}, {"edges": np.array([0, 10, 20])}
    ra, rb = spec.bind([18, 38]).resolve(a), spec.resolve(b)
    assert asked == [a, b] and ra.ping_edges.tolist() == EDGES and rb.ping_edges.tolist() == [0, 10, 20]
    assert (ra.channel, ra.seabed_offset, ra.mode, rb.channel) == (1, -3, "probability", None)
    assert ra.resolve(b) is ra                                    # a table stays
    with pytest.raises(ValueError, match="ping_edges"):
        spec.resolve({"edges": [5, 4]})
    with pytest.raises(ValueError, match="ping_edges"):
        spec.resolve({"edges": None})


def test_bind_keeps_the_edges_and_bins_counts_the_table():
    for kw in (dict(), dict(seabed_offset=-5), dict(seabed_offset=3, reference="seabed", layers=7, mode="probability")):
        spec = ti.IntegrationSpec(None, 32, thresholds=(0.25, 1), ping_edges=EDGES, **kw)
        bound = spec.bind([18, 38, 120, 200])
        assert bound.channel == 1 and bound.frequency == 38 and bound.ping_bin is None
        assert bound.ping_edges.tolist() == EDGES and type(bound) is type(spec)
        assert (bound.seabed_offset, bound.reference, bound.layers, bound.mode, bound.thresholds) == (
            spec.seabed_offset, spec.reference, spec.layers, spec.mode, (0.25, 1.0))
        n_cols = 7 if kw.get("reference") == "seabed" else 3
        assert spec.bins(300, 70) == bound.bins(300, 70) == (7, n_cols) and spec.bins(10, 70) == (7, n_cols)
        acc, cnt = ti.new_integration("cpu", ti.IntegrationSpec(64, 32, **kw), 300, 70)
        assert acc.shape == (3, 5, n_cols)
    spec = ti.IntegrationSpec(None, 32, ping_edges=EDGES)
    # the ping bins a launch touches, as the library counts them for the scratch
    assert [spec.touched(s, e) for s, e in ((0, 300), (100, 200), (0, 3), (297, 400), (3, 4), (4, 10), (74, 76), (0, 4))] == [
        7, 1, 0, 0, 1, 1, 3, 2]
    uniform = ti.IntegrationSpec(64, 32)
    table_u = ti.IntegrationSpec(None, 32, ping_edges=np.arange(4) * 64)
    for s, e in ((0, 150), (0, 100), (100, 150), (64, 128), (63, 65), (191, 192)):
        assert uniform.touched(s, e) == table_u.touched(s, e) == (e - 1) // 64 - s // 64 + 1


def test_integration_result_clips_the_table_to_the_survey():
    spec = ti.IntegrationSpec(None, 32, ping_edges=EDGES)
    n_pb, n_rb = spec.bins(250, 70)
    res = ti.integration_result(np.zeros((3, n_pb, n_rb)), np.zeros((3, n_pb, n_rb), dtype=np.int64), spec, 250, 70)
    assert set(res) == {"sv_sum", "pixels", "ping_edges", "range_edges", "classes"}
    assert res["ping_edges"].tolist() == [3, 3, 4, 10, 75, 75, 210, 250] and res["ping_edges"].dtype == np.int64
    assert res["range_edges"].tolist() == [0, 32, 64, 70]
    assert ti.integration_result(np.zeros((3, n_pb, n_rb)), np.zeros((3, n_pb, n_rb), dtype=np.int64), spec, 1000, 70)[
        "ping_edges"].tolist() == EDGES
    lay = ti.IntegrationSpec(None, 16, ping_edges=EDGES, seabed_offset=0, reference="seabed", layers=2)
    res = ti.finish_integration(torch.zeros((3, 7, 2), dtype=torch.float64), torch.zeros((3, 7, 2), dtype=torch.int64), lay,
                                100, 70)
    assert res["ping_edges"].tolist() == [3, 3, 4, 10, 75, 75, 100, 100] and res["range_edges"].tolist() == [0, 16, 32]
    assert (res["reference"], res["seabed_offset"]) == ("seabed", 0)


def test_mean_nasc_divides_by_the_pings_and_gives_nan_for_empty_cells():
    spec = ti.IntegrationSpec(None, 32, ping_edges=EDGES)
    sums = np.arange(3 * 7 * 3, dtype=np.float64).reshape(3, 7, 3) + 1
    sums[:, [0, 4]] = 0                                           # (what a zero-width cell holds)
    res = ti.integration_result(sums, np.zeros((3, 7, 3), dtype=np.int64), spec, 300, 70)
    total, mean = ti.nasc(res, 0.25), ti.mean_nasc(res, 0.25)
    assert mean.shape == total.shape == (3, 7, 3)
    width = np.diff(EDGES)
    assert np.isnan(mean[:, width == 0]).all() and np.isfinite(mean[:, width > 0]).all()
    assert np.array_equal(mean[:, width > 0], total[:, width > 0] / width[width > 0][None, :, None])
    assert mean[0, 2, 1] == total[0, 2, 1] / 6 and mean[0, 1, 0] == total[0, 1, 0]
    # on the uniform grid too: the partial last bin is divided by its own pings
    uni = ti.IntegrationSpec(100, 64)
    res = ti.integration_result(np.ones((3, 3, 2)), np.zeros((3, 3, 2), dtype=np.int64), uni, 230, 100)
    assert np.array_equal(ti.mean_nasc(res, 1.0)[0, :, 0], ti.nasc(res, 1.0)[0, :, 0] / np.array([100, 100, 30]))


def test_both_scored_holders_refuse_ping_edges_before_any_data():
    for spec in (ti.IntegrationSpec(None, 32, ping_edges=EDGES), ti.IntegrationSpec(None, 32, ping_edges=lambda source: EDGES)):
        for holder in (ti.ScoredIntegration, ti.ScoredIntegrationSet):
            with pytest.raises(NotImplementedError, match="ping_edges"):
                holder(spec)
    ti.ScoredIntegration(ti.IntegrationSpec(64, 32))
    ti.ScoredIntegrationSet(ti.IntegrationSpec(64, 32))


def test_launch_integration_refuses_a_table_of_another_length_and_an_unresolved_callable():
    spec = ti.IntegrationSpec(None, 32, ping_edges=EDGES).bind([38])
    with pytest.raises(ValueError, match="n_pb_total=6"):
        ti.launch_integration(spec, None, True, 70, 300, None, 300, 0, 0, 6, None, None, None)
    with pytest.raises(ValueError, match="resolve"):
        ti.launch_integration(ti.IntegrationSpec(None, 32, ping_edges=lambda s: EDGES).bind([38]), None, True, 70, 300, None,
                              300, 0, 0, 7, None, None, None)


def test_the_documents_describe_the_edsu_form():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    for word in ("ping_bin_edges", "mean_nasc", "ping_edges", "crimac_integrate_edges", "NotImplementedError"):
        assert word in text, word
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "ping_bin_edges" in f.read()
