"""GPU: echo integration per EDSU -- ``crimac_integrate_edges`` (csrc/integrate.hip) against numpy and against the uniform
entry points, and the flows that launch it with ``IntegrationSpec(ping_edges=...)``: ``integrate_survey``,
``integrate_echogram_memm`` and the packed ``integrate_echograms_memm``.

The comparison target is ``edges_numpy`` of tests/test_integrate_edsu_cpu.py (checked there against a per-pixel loop).
Counts must be equal.  Sums: the bound tests/test_gpu_integrate.py derives -- every term is >= 0, so any order of n fp64
additions is within n * 2^-53 relative of the exact sum, on both sides -- (pixels of the cell + 2) * 2^-52 * sum, and exactly
0 where the numpy sum is 0 (``check``).  With ``edges = arange(n + 1) * ping_bin`` the results must have the BITS of the
uniform entry point: the same kernels, the same split rule."""
import ctypes
import types

import numpy as np
import pytest
import torch

import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import hip, synth
from crimac_classifiers_unet_amd import tiled_inference as ti
from crimac_classifiers_unet_amd.hip import call, ptr
from tools.fake_reader import FakeEchogram, FakeZarrReader, synth_survey

from test_gpu_integrate import MULTI, check, hashed_predict_fn, operands, tensor  # noqa: E402
from test_gpu_integrate_layers import echogram, seabed_line  # noqa: E402
from test_integrate_edsu_cpu import EDGES, edges_numpy, new_host  # noqa: E402

pytestmark = pytest.mark.gpu

FREQS = [18, 38, 120, 200]
MODES = ("threshold", "probability")
REFERENCES = ("surface", "seabed")
THR = (0.5, 0.25)
POISON = 7.25


def new_device(n_pb, n_cols, fill=0):
    shape = (3, n_pb, n_cols)
    return (torch.full(shape, float(fill), dtype=torch.float64, device="cuda"),
            torch.full(shape, int(fill), dtype=torch.int64, device="cuda"))


def touched(edges, a, b):
    """The ping bins global pings [a, b) touch, as the header states them: the first cell that ends after ``a`` to the last
    that begins before ``b``, zero-width cells in between included."""
    e = np.asarray(edges)
    pb0 = max(int(np.searchsorted(e, a, "right")) - 1, 0)
    pb1 = min(int(np.searchsorted(e, b, "left")) - 1, len(e) - 2)
    return max(pb1 - pb0 + 1, 0)


def launch(acc, cnt, pred, sv, thr, mode, edges, range_bin, ping_origin, sv_ping_off=0, seabed=None, seabed_first=0, offset=0,
           reference="surface", n_layers=0, run=True, host=None, n_pb_total=None):
    """``crimac_integrate_edges`` on device tensors ``pred`` [2, R, P], ``sv`` [data_pings, R], ``seabed`` int32 [n] or None;
    the scratch is what the header states: (cells touched + SPLIT_WGS) slots.  ``host``: another host table than ``edges``."""
    _, R, P = pred.shape
    n_cols = acc.shape[2]
    edges = np.ascontiguousarray(edges, dtype=np.int64)
    host = edges if host is None else np.ascontiguousarray(host, dtype=np.int64)
    edges_d = tensor(edges)
    cells = touched(edges, ping_origin, ping_origin + P) * n_cols
    scratch = torch.empty((cells + hip.INTEGRATE_SPLIT_WGS) * hip.INTEGRATE_SLOT_BYTES // 8, dtype=torch.float64, device="cuda")
    args = [ptr(pred), int(pred.dtype == torch.float16), R, P, ptr(sv), sv.shape[0], sv_ping_off, float(thr[0]), float(thr[1]),
            MODES.index(mode), ptr(edges_d), ctypes.c_void_p(host.ctypes.data), range_bin, ping_origin,
            len(edges) - 1 if n_pb_total is None else n_pb_total, ptr(seabed), seabed_first,
            0 if seabed is None else seabed.numel(), offset, REFERENCES.index(reference), n_layers, ptr(acc), ptr(cnt),
            ptr(scratch), scratch.numel() * 8]
    if run:
        call("crimac_integrate_edges", *args)
    return args, (edges_d, host, scratch)                        # (the second: what the pointers point at)


# ---- the kernel alone ---------------------------------------------------------------------------------------------------
CASE = dict(n_range=70, n_pings=300, range_bin=32, sv_ping_off=37, seam=100)


def two_launches(dtype, mode, thr=(0.5, 0.5), seed=1, seabed=None):
    """70 rows x 300 pings in two launches, the seam at ping 100 inside the 135-ping cell; leading pings 0 .. 2 and
    trailing pings 297 .. 299 lie in no cell.  ``seabed`` = (offset, reference, n_layers): with the sloping line, whose
    limits clamp to 0 (pings 5 .. 8) and to n_range (pings 40 .. 46)."""
    c = CASE
    pred, sv, planted = operands(c["n_range"], c["n_pings"], c["sv_ping_off"] + c["n_pings"] + 9, c["sv_ping_off"], seed)
    offset, reference, n_layers = seabed or (None, "surface", 0)
    n_cols = n_layers if reference == "seabed" else -(-c["n_range"] // c["range_bin"])
    want = new_host(len(EDGES) - 1, n_cols)
    acc, cnt = new_device(len(EDGES) - 1, n_cols)
    sv_d = tensor(sv)
    line = seabed_line("slope", c["n_pings"], c["n_range"])
    lead = np.full(5, 10 ** 6, dtype=np.int32)                   # (read by mistake, it would exclude nothing)
    line_d = tensor(np.concatenate([lead, line, lead])) if seabed else None
    for p0, p1 in ((0, c["seam"]), (c["seam"], c["n_pings"])):
        part = tensor(pred[:, :, p0:p1], dtype)
        launch(acc, cnt, part, sv_d, thr, mode, EDGES, c["range_bin"], p0, c["sv_ping_off"] + p0, line_d, 5 + p0,
               offset or 0, reference, n_layers)
        edges_numpy(*want, part.cpu().numpy(), sv, thr, mode, EDGES, c["range_bin"], p0, c["sv_ping_off"] + p0,
                    line[p0:p1], offset, reference)
    return acc.cpu().numpy(), cnt.cpu().numpy(), want, (pred, sv, planted)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_two_launches_across_a_wide_cell_match_numpy(dtype, mode):
    got_sum, got_cnt, (want_sum, want_cnt, geo), (pred, sv, planted) = two_launches(dtype, mode, seed=2)
    assert geo.sum() == 70 * 294 and geo[:, 0].tolist() == [0, 32, 6 * 32, 65 * 32, 0, 135 * 32, 87 * 32]
    assert len(planted) >= 50                                    # NaN, +Inf, -Inf, 0, < 0 inside pixels both classes select
    check(got_sum, got_cnt, want_sum, want_cnt, geo)
    assert (want_cnt[:, [2, 3, 5, 6]] > 0).all() and (want_cnt[2, 1] > 0).all() and np.isfinite(got_sum).all()
    assert not got_cnt[:, [0, 4]].any() and not got_sum[:, [0, 4]].any()             # the zero-width cells: exact zeros
    inside = (planted[:, 1] >= 3) & (planted[:, 1] < 297)
    assert got_cnt[2].sum() == 70 * 294 - inside.sum()           # every other sample of the 294 pings is finite and > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seabed", [(-3, "surface", 0), (-3, "seabed", 3)], ids=["limited", "3 layers"])
def test_a_seabed_line_with_the_edge_table_matches_numpy(seabed, mode):
    got_sum, got_cnt, (want_sum, want_cnt, geo), _ = two_launches(torch.float16, mode, THR, seed=3, seabed=seabed)
    check(got_sum, got_cnt, want_sum, want_cnt, geo)
    assert want_cnt[2].sum() > 3000 and (want_cnt[:2].sum(axis=(1, 2)) > 0).all() and geo.sum() < 70 * 294
    assert not got_cnt[:, [0, 4]].any() and not got_sum[:, [0, 4]].any()
    line = seabed_line("slope", 300, 70)
    assert (np.clip(line[5:9] - 3, 0, 70) == 0).all() and (np.clip(line[40:47] - 3, 0, 70) == 70).all()


def test_the_two_launch_case_twice_gives_identical_bits():
    for seabed in (None, (-3, "seabed", 3)):
        a = two_launches(torch.float16, "probability", seabed=seabed)
        b = two_launches(torch.float16, "probability", seabed=seabed)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[1][2].sum() > 0


def uniform_pair(dtype, mode, seabed):
    """The MULTI case of tests/test_gpu_integrate.py through the uniform entry point and through the edge table
    arange(4) * 64, two launches each.  ``seabed`` = None or (offset, reference, n_layers)."""
    m = MULTI
    pred, sv, _ = operands(m["n_range"], m["n_pings"], m["sv_ping_off"] + m["n_pings"] + 9, m["sv_ping_off"], 4)
    edges = np.arange(m["n_pb_total"] + 1) * m["ping_bin"]
    offset, reference, n_layers = seabed or (0, "surface", 0)
    n_cols = n_layers if reference == "seabed" else -(-m["n_range"] // m["range_bin"])
    line = seabed_line("slope", m["n_pings"], m["n_range"])
    assert line.max() - line.min() > m["range_bin"]              # relief above range_bin inside a ping bin
    line_d, sv_d = tensor(line), tensor(sv)
    old, new = new_device(m["n_pb_total"], n_cols), new_device(m["n_pb_total"], n_cols)
    for p0, p1 in ((0, m["seam"]), (m["seam"], m["n_pings"])):
        part = tensor(pred[:, :, p0:p1], dtype)
        a, keep = launch(*new, part, sv_d, THR, mode, edges, m["range_bin"], p0, m["sv_ping_off"] + p0,
                         line_d if seabed else None, p0, offset, reference, n_layers)
        head = (*a[:10], m["ping_bin"], *a[12:15])
        if seabed:
            call("crimac_integrate_layers", *head, *a[15:21], ptr(old[0]), ptr(old[1]), *a[23:])
        else:
            call("crimac_integrate_classes", *head, ptr(old[0]), ptr(old[1]), *a[23:])
    return [t.cpu().numpy() for t in (*old, *new)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_uniform_edges_give_the_bits_of_crimac_integrate_classes(dtype, mode):
    old_sum, old_cnt, new_sum, new_cnt = uniform_pair(dtype, mode, None)
    assert new_sum.tobytes() == old_sum.tobytes() and np.array_equal(new_cnt, old_cnt) and (old_cnt > 0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("reference", REFERENCES)
def test_uniform_edges_with_a_seabed_line_give_the_bits_of_crimac_integrate_layers(reference, mode):
    old_sum, old_cnt, new_sum, new_cnt = uniform_pair(torch.float16, mode, (-3, reference, 2))
    assert new_sum.tobytes() == old_sum.tobytes() and np.array_equal(new_cnt, old_cnt) and old_cnt[2].sum() > 1000


ALIGN_EDGES = [7, 7, 30, 31, 101, 190, 205]     # pings 7 .. 204 of a launch at origin 5: off the 4-ping grid, one tile wide


@pytest.mark.parametrize("misalign", [False, True], ids=["16-byte reads", "4-byte reads"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_both_read_paths_of_sv_and_pred(dtype, misalign):
    """72 rows x 200 pings: extents that allow the 16- / 8-byte reads of both operands when the base addresses are aligned;
    one element off, the same extents take the 4-byte (pred float16: 2-byte) reads."""
    R, P = 72, 200
    pred, sv, _ = operands(R, P, P + 3, 2, seed=5, levels=False)
    want = new_host(6, 8)
    acc, cnt = new_device(6, 8)
    if misalign:
        pred_d = torch.zeros(pred.size + 1, dtype=dtype, device="cuda")[1:].view(pred.shape)
        sv_d = torch.zeros(sv.size + 1, dtype=torch.float32, device="cuda")[1:].view(sv.shape)
        pred_d.copy_(torch.from_numpy(pred))
        sv_d.copy_(torch.from_numpy(sv))
        assert pred_d.data_ptr() % 8 != 0 and sv_d.data_ptr() % 16 == 4
    else:
        pred_d, sv_d = tensor(pred, dtype), tensor(sv)
        assert pred_d.data_ptr() % 16 == 0 and sv_d.data_ptr() % 16 == 0
    launch(acc, cnt, pred_d, sv_d, (0.5, 0.4), "probability", ALIGN_EDGES, 10, 5, 2)
    edges_numpy(*want, pred_d.cpu().numpy(), sv, (0.5, 0.4), "probability", ALIGN_EDGES, 10, 5, 2)
    assert want[2].sum() == R * 198 and want[2][1, 7] == 23 * 2
    check(acc.cpu().numpy(), cnt.cpu().numpy(), *want)


def test_argument_errors_launch_nothing_and_leave_a_poisoned_accumulator():
    lib = hip.load_library()
    pred, sv, _ = operands(70, 300, 346, 37, seed=6)
    pred_d, sv_d = tensor(pred, torch.float16), tensor(sv)
    acc, cnt = new_device(7, 3, fill=POISON)
    cases = ((dict(host=[3, 3, 4, 10, 75, 74, 210, 297]), "decrease"),        # the HOST table decides; the device copy is good
             (dict(host=[-1, 3, 4, 10, 75, 75, 210, 297]), "negative"),
             (dict(n_pb_total=0), "accumulator"))
    for kw, word in cases:
        args, keep = launch(acc, cnt, pred_d, sv_d, THR, "threshold", EDGES, 32, 0, 37, run=False, **kw)
        with pytest.raises(hip.HipLibraryError, match=word):
            call("crimac_integrate_edges", *args)
        assert b"integrate_edges" in lib.crimac_last_error()
    args, keep = launch(acc, cnt, pred_d, sv_d, THR, "threshold", EDGES, 32, 0, 37, run=False)
    args[24] = 21 * 3 * hip.INTEGRATE_SLOT_BYTES - 1             # 21 cells x 3 splits: one byte short
    with pytest.raises(hip.HipLibraryError, match="scratch"):
        call("crimac_integrate_edges", *args)
    torch.cuda.synchronize()
    assert (acc == POISON).all() and (cnt == int(POISON)).all()
    args[24] += 1                                                # and with that byte it runs
    call("crimac_integrate_edges", *args)
    torch.cuda.synchronize()
    assert (acc[:, [0, 4]] == POISON).all() and (cnt[2, [1, 2, 3, 5, 6]] > int(POISON)).all()


# ---- the flows ----------------------------------------------------------------------------------------------------------
def make_pipe(model):
    return types.SimpleNamespace(model=model.cuda().eval(), device=torch.device("cuda"), frequencies=FREQS)


@pytest.fixture(scope="module")
def stub_pipe():
    return make_pipe(pkg.UNet_Baseline(3, 4, start_filts=8, precision="f32x6"))


def log_distance(n_pings, seed):
    """A log in nmi at a varying speed: stretches where the vessel stands still (repeated values) and one jump of several
    units between two pings (zero-width cells)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    step = rng.uniform(0.0005, 0.004, size=n_pings)
    step[n_pings // 5:n_pings // 5 + 7] = 0
    step[n_pings // 2] = 0.8
    return 10.0 + np.cumsum(step)


@pytest.fixture(scope="module")
def zarr_case(stub_pipe):
    """A 700-ping x 300-row survey in 3 chunks, its float16 predictions (computed once) and its EDSU table: 0.25 nmi from a
    later origin, so that the leading pings count nowhere."""
    sv, labels, seabed = synth_survey()
    sv, labels, seabed = sv[:, :700, :300].copy(), labels[:700, :300].copy(), np.clip(seabed[:700], 0, 260)
    reader = FakeZarrReader(sv, labels, seabed)
    reader.distance = log_distance(700, 1)
    chunks = [(s, out) for s, e, out in ti.predict_survey(reader, stub_pipe, (256, 256), 20, 3, 250, out_dtype=np.float16,
                                                         predict_fn=hashed_predict_fn)]
    assert [s for s, _ in chunks] == [0, 233, 466]
    edges = ti.ping_bin_edges(reader.distance, 0.25, origin=reader.distance[0] + 0.013)
    widths = np.diff(edges)
    assert edges[0] > 0 and edges[-1] == 700 and (widths == 0).sum() >= 2 and widths.max() > 64 and len(edges) > 8
    assert any(a < s < b for s, _ in chunks[1:] for a, b in zip(edges[:-1], edges[1:]))       # a cell cut by a chunk seam
    return reader, chunks, edges


def survey_by_numpy(spec, chunks, sv, line, edges, n_range):
    want = new_host(*spec.bins(0, n_range))
    for s, out in chunks:
        e = s + out.shape[2]
        edges_numpy(*want, out, sv, spec.thresholds, spec.mode, edges, spec.range_bin, s, s, line[s:e], spec.seabed_offset,
                    spec.reference)
    return want


SPECS = {"threshold": dict(mode="threshold", thresholds=(0.5, 0.4)), "probability": dict(mode="probability"),
         "limited": dict(thresholds=THR, seabed_offset=-4),
         "layers": dict(thresholds=THR, seabed_offset=-4, reference="seabed", layers=5, mode="probability")}


@pytest.mark.parametrize("which", list(SPECS))
def test_integrate_survey_with_an_edge_table_equals_predict_survey_then_numpy(stub_pipe, zarr_case, which, monkeypatch):
    reader, chunks, edges = zarr_case
    asked, names = [], []
    real = ti.call
    monkeypatch.setattr(ti, "call", lambda name, *a, **kw: (names.append(name), real(name, *a, **kw))[1])

    def per_source(source):
        asked.append(source)
        return ti.ping_bin_edges(source.distance, 0.25, origin=source.distance[0] + 0.013)
    spec = ti.IntegrationSpec(None, 16 if which == "layers" else 64, ping_edges=per_source, **SPECS[which])
    got = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 250, spec, predict_fn=hashed_predict_fn)
    assert asked == [reader] and names.count("crimac_integrate_edges") == 3
    assert not {"crimac_integrate_classes", "crimac_integrate_layers"} & set(names)
    table = ti.IntegrationSpec(None, spec.range_bin, ping_edges=edges, **SPECS[which])
    want_sum, want_cnt, geo = survey_by_numpy(table, chunks, reader.sv[1], reader.seabed, edges, 300)
    assert got["ping_edges"].tolist() == edges.tolist() and got["sv_sum"].shape == want_sum.shape
    check(got["sv_sum"], got["pixels"], want_sum, want_cnt, geo)
    assert want_cnt[2].sum() > 10000 and (want_cnt[:2].sum(axis=(1, 2)) > 0).all()
    assert not got["pixels"][:, np.diff(edges) == 0].any()
    if which in ("threshold", "probability"):
        assert got["pixels"][2].sum() == want_cnt[2].sum() > 0.99 * (700 - edges[0]) * 300
    # the table itself, another batch size: the same bits
    again = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 5, 250, table, predict_fn=hashed_predict_fn)
    assert again["sv_sum"].tobytes() == got["sv_sum"].tobytes() and np.array_equal(again["pixels"], got["pixels"])
    mean = ti.mean_nasc(got, 0.19)
    assert np.isnan(mean[:, np.diff(edges) == 0]).all() and np.isfinite(mean[:, np.diff(edges) > 0]).all()


def test_a_table_that_ends_before_the_survey_and_uniform_edges_in_the_flow(stub_pipe, zarr_case):
    reader, chunks, _ = zarr_case
    short = np.array([50, 120, 120, 240, 460])                   # pings 460 .. 699 count nowhere; the last chunk touches no cell
    spec = ti.IntegrationSpec(None, 64, ping_edges=short, thresholds=(0.5, 0.4))
    got = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 250, spec, predict_fn=hashed_predict_fn)
    want_sum, want_cnt, geo = survey_by_numpy(spec, chunks, reader.sv[1], reader.seabed, short, 300)
    check(got["sv_sum"], got["pixels"], want_sum, want_cnt, geo)
    assert geo.sum() == 410 * 300 and got["ping_edges"].tolist() == short.tolist()
    # uniform edges: the bits of the uniform spec
    uni = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 250, ti.IntegrationSpec(100, 64, thresholds=(0.5, 0.4)),
                              predict_fn=hashed_predict_fn)
    tab = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 250,
                              ti.IntegrationSpec(None, 64, ping_edges=np.arange(8) * 100, thresholds=(0.5, 0.4)),
                              predict_fn=hashed_predict_fn)
    assert tab["sv_sum"].tobytes() == uni["sv_sum"].tobytes() and np.array_equal(tab["pixels"], uni["pixels"])
    assert tab["ping_edges"].tolist() == uni["ping_edges"].tolist()


@pytest.mark.parametrize("mode", MODES)
def test_integrate_echogram_memm_with_an_edge_table_equals_predict_then_numpy(stub_pipe, mode):
    sv, labels, seabed = synth_survey(n_pings=300, n_range=90, seed=12)
    eg = FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), np.clip(seabed, 1, 80),
                      frequencies=FREQS)
    out = ti.predict_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, predict_fn=hashed_predict_fn).astype(np.float16)
    for kw in (dict(), dict(seabed_offset=3, reference="seabed", layers=3)):
        spec = ti.IntegrationSpec(None, 20 if kw else 40, frequency=120, mode=mode, ping_edges=lambda source: EDGES, **kw)
        want = new_host(7, 3)
        edges_numpy(*want, out, sv[FREQS.index(120)], spec.thresholds, mode, EDGES, spec.range_bin, 0, 0,
                    np.clip(seabed, 1, 80), spec.seabed_offset, spec.reference)
        got = ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn)
        assert got["ping_edges"].tolist() == EDGES and got["sv_sum"].shape == (3, 7, 3)
        check(got["sv_sum"], got["pixels"], *want)
        assert got["pixels"][:2].sum() > 0 and got["pixels"][2].sum() > 1000
        again = ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn)
        assert again["sv_sum"].tobytes() == got["sv_sum"].tobytes() and np.array_equal(again["pixels"], got["pixels"])


MEMM = [(300, 90), (40, 130), (170, 64), (64, 128), (101, 60)]             # pings x range


def own_table(eg):
    """A different table per echogram: 0.05 nmi on the echogram's own log."""
    return ti.ping_bin_edges(log_distance(eg.shape[1], 100 + eg.shape[1]), 0.05)


def same_result(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key], key
    assert a["sv_sum"].dtype == np.float64 and a["pixels"].dtype == np.int64


@pytest.mark.parametrize("which", ["default", "layers"])
def test_integrate_echograms_memm_with_a_table_per_echogram_equals_the_loop(stub_pipe, which, monkeypatch):
    """Dyadic sv (``echogram`` of tests/test_gpu_integrate_layers.py): sums are exact in any order, so the packed flow and
    the single-echogram flow must agree with ``==`` wherever the staging puts an echogram."""
    egs = [echogram(p, r, 60 + i, name=f"eg{i}") for i, (p, r) in enumerate(MEMM)]
    kw = {"default": dict(mode="probability"), "layers": dict(seabed_offset=-3, reference="seabed", layers=4)}[which]
    spec = ti.IntegrationSpec(None, 8 if which == "layers" else 40, thresholds=THR, ping_edges=own_table, **kw)
    names = []
    real = ti.call
    monkeypatch.setattr(ti, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    counts = [len(r.grid) for g in ti.iter_memm_groups(iter(egs), (64, 64), 6, 10 ** 9) for r in g]
    stats = {}
    got = list(ti.integrate_echograms_memm(iter(egs), stub_pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn,
                                           stats=stats, group_patches=counts[0] + counts[1] // 2))
    assert [eg for eg, _ in got] == egs and stats["groups"] >= 2 and stats["solo_echograms"] == 0
    assert names.count("crimac_integrate_edges") == 5
    tables = [own_table(eg) for eg in egs]
    assert len({len(t) for t in tables}) > 2 and all((np.diff(t) == 0).any() for t in tables)
    for (eg, res), table in zip(got, tables):
        assert res["ping_edges"].tolist() == table.tolist() and res["sv_sum"].shape[1] == len(table) - 1
        single = ti.IntegrationSpec(None, spec.range_bin, thresholds=THR, ping_edges=table, **kw)
        same_result(res, ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, single, predict_fn=hashed_predict_fn))
        assert res["pixels"][2].sum() > 0 and not res["pixels"][:, np.diff(table) == 0].any()
    assert sum(int(res["pixels"][:2].sum()) for _, res in got) > 0
    # an echogram too large for the staging takes the per-echogram path with its own table, in its place
    stats = {}
    solo = list(ti.integrate_echograms_memm(iter(egs[:3]), stub_pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn,
                                            stats=stats, group_elems=20000))
    assert stats["solo_echograms"] == 1 and [eg for eg, _ in solo] == egs[:3]
    for (_, a), (_, b) in zip(solo, got):
        same_result(a, b)
    ti.release_staging()


def test_integrate_survey_with_a_real_depth_3_network_and_an_edge_table():
    sv, labels, seabed = synth_survey(n_pings=230, n_range=120, seed=11)
    reader = FakeZarrReader(sv, labels, np.clip(seabed, 0, 100))
    model = pkg.UNet_Baseline(3, 4, depth=3, precision="h3p")
    model.load_state_dict(synth.synth_state_dict(depth=3, seed=4))
    pipe = make_pipe(model)
    edges = ti.ping_bin_edges(log_distance(230, 3), 0.1)
    spec = ti.IntegrationSpec(None, 25, mode="probability", ping_edges=edges)    # (whatever the network predicts, it weighs)
    chunks = [(s, out) for s, e, out in ti.predict_survey(reader, pipe, (64, 64), 6, 8, 120, out_dtype=np.float16)]
    assert len(chunks) == 2
    want = survey_by_numpy(spec, chunks, sv[1], np.clip(seabed, 0, 100), edges, 120)
    got = ti.integrate_survey(reader, pipe, (64, 64), 6, 8, 120, spec)
    check(got["sv_sum"], got["pixels"], *want)
    assert got["pixels"][2].sum() > 0.9 * 230 * 120 and (got["sv_sum"][:2].sum(axis=(1, 2)) > 0).all()
