"""GPU: several frequencies in one pass -- ``crimac_integrate_freqs`` (csrc/integrate.hip) against the single-frequency
entry points and against numpy, and the flows that launch it with ``IntegrationSpec(frequency=(f1, f2, ...))``.

Two yardsticks.  Frequency slice i of the accumulators must have THE BITS (``torch.equal``) of ``crimac_integrate_classes`` /
``_layers`` / ``_edges`` on plane ``channels[i]``: the same workgroups, split count and order of every sum.  And it must lie
within the bound of tests/test_gpu_integrate.py, (pixels of the cell + 2) * 2^-52 * sum, of ``edges_numpy``
(tests/test_integrate_edsu_cpu.py, checked there against a per-pixel loop), counts equal (``check``)."""
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

from test_gpu_integrate import check, hashed_predict_fn, operands, tensor  # noqa: E402
from test_gpu_integrate_layers import echogram, seabed_line  # noqa: E402
from test_integrate_edsu_cpu import EDGES, edges_numpy, new_host  # noqa: E402

pytestmark = pytest.mark.gpu

FREQS = [18, 38, 120, 200]
MODES = ("threshold", "probability")
REFERENCES = ("surface", "seabed")
THR = (0.5, 0.25)
POISON = 7.25
SLOT, WGS = hip.INTEGRATE_SLOT_BYTES, hip.INTEGRATE_SPLIT_WGS


def planes_of(n_planes, n_range, n_pings, data_pings, sv_ping_off, seed):
    """pred [2, R, P] and ``n_planes`` different sv planes [n_planes, data_pings, R], each with its own NaN / Inf / 0 / < 0."""
    pred, sv0, _ = operands(n_range, n_pings, data_pings, sv_ping_off, seed)
    planes = [sv0] + [operands(n_range, n_pings, data_pings, sv_ping_off, 100 * seed + k)[1] for k in range(1, n_planes)]
    return pred, np.stack(planes)


def touched(ping_bin, edges, a, b):
    if edges is None:
        return (b - 1) // ping_bin - a // ping_bin + 1
    e = np.asarray(edges)
    return max(min(int(np.searchsorted(e, b, "left")) - 1, len(e) - 2) - max(int(np.searchsorted(e, a, "right")) - 1, 0) + 1, 0)


def run(pred, planes, channels, dtype, mode, seams, sv_ping_off, range_bin, n_pb, ping_bin=None, edges=None, seabed=None,
        thr=THR, sv_dev=None, stride=None, numpy_too=True):
    """Launches over pings [seams[i], seams[i + 1]) into one accumulator, through ``crimac_integrate_freqs`` (all of
    ``channels`` at once) and, plane by plane, through the single-frequency entry point of the same geometry.  ``seabed`` =
    (offset, reference, n_layers).  ``sv_dev`` / ``stride``: the planes on the device elsewhere than in one contiguous tensor.
    Returns (multi sums, multi counts, single sums, single counts) as device tensors [F, 3, n_pb, n_cols] and the numpy
    reference (sums, counts, pixels covered) with the same leading axis."""
    n_planes, data_pings, R = planes.shape
    F = len(channels)
    offset, reference, n_layers = seabed or (0, "surface", 0)
    n_cols = n_layers if reference == "seabed" else -(-R // range_bin)
    shape = (F, 3, n_pb, n_cols)
    multi = torch.zeros(shape, dtype=torch.float64, device="cuda"), torch.zeros(shape, dtype=torch.int64, device="cuda")
    single = torch.zeros(shape, dtype=torch.float64, device="cuda"), torch.zeros(shape, dtype=torch.int64, device="cuda")
    want = [new_host(n_pb, n_cols) for _ in channels]
    sv_d = tensor(planes) if sv_dev is None else sv_dev
    stride = data_pings * R if stride is None else stride
    plane_d = [sv_d.reshape(-1)[c * stride:c * stride + data_pings * R].view(data_pings, R) for c in range(n_planes)]
    P_all = pred.shape[2]
    line = seabed_line("slope", P_all, R)
    lead = np.full(5, 10 ** 6, dtype=np.int32)
    line_d = tensor(np.concatenate([lead, line, lead])) if seabed else None
    table = np.arange(n_pb + 1) * ping_bin if edges is None else np.asarray(edges)
    edges_h = None if edges is None else np.ascontiguousarray(edges, dtype=np.int64)
    edges_d = None if edges is None else tensor(edges_h)
    chan = (ctypes.c_int * F)(*channels)
    for p0, p1 in zip(seams[:-1], seams[1:]):
        part = tensor(pred[:, :, p0:p1], dtype)
        cells = touched(ping_bin, edges, p0, p1) * n_cols
        scratch = torch.empty(F * (cells + WGS) * SLOT // 8, dtype=torch.float64, device="cuda")
        head = [ptr(part), int(dtype == torch.float16), R, p1 - p0]
        sb = [ptr(line_d), 5 + p0, 0 if line_d is None else line_d.numel(), offset, REFERENCES.index(reference), n_layers]
        call("crimac_integrate_freqs", *head, ptr(plane_d[0]), stride, n_planes, chan, F, data_pings, sv_ping_off + p0,
             float(thr[0]), float(thr[1]), MODES.index(mode), ping_bin or 0, ptr(edges_d),
             None if edges_h is None else ctypes.c_void_p(edges_h.ctypes.data), range_bin, p0, n_pb, *sb, ptr(multi[0]),
             ptr(multi[1]), ptr(scratch), scratch.numel() * 8)
        for i, c in enumerate(channels):
            mid = [ptr(plane_d[c]), data_pings, sv_ping_off + p0, float(thr[0]), float(thr[1]), MODES.index(mode)]
            tail = [ptr(single[0][i]), ptr(single[1][i]), ptr(scratch), scratch.numel() * 8]
            if edges is not None:
                call("crimac_integrate_edges", *head, *mid, ptr(edges_d), ctypes.c_void_p(edges_h.ctypes.data), range_bin, p0,
                     n_pb, *sb, *tail)
            elif seabed:
                call("crimac_integrate_layers", *head, *mid, ping_bin, range_bin, p0, n_pb, *sb, *tail)
            else:
                call("crimac_integrate_classes", *head, *mid, ping_bin, range_bin, p0, n_pb, *tail)
            if numpy_too:
                edges_numpy(*want[i], part.cpu().numpy(), planes[c], thr, mode, table, range_bin, p0, sv_ping_off + p0,
                            line[p0:p1] if seabed else None, offset if seabed else None, reference)
    torch.cuda.synchronize()
    return (*multi, *single), [np.stack([w[k] for w in want]) for k in range(3)]


def same_bits(got):
    m_sum, m_cnt, s_sum, s_cnt = got
    assert torch.equal(m_cnt, s_cnt)
    assert torch.equal(m_sum.view(torch.int64), s_sum.view(torch.int64))         # the bits, not the values


def within_bound(got, want):
    for i in range(got[0].shape[0]):
        check(got[0][i].cpu().numpy(), got[1][i].cpu().numpy(), want[0][i], want[1][i], want[2][i])


# ---- the kernel alone ---------------------------------------------------------------------------------------------------
BASE = dict(n_range=70, n_pings=150, range_bin=32, ping_bin=64, seams=(0, 100, 150), sv_ping_off=37, n_pb=3)


def base(channels, dtype, mode, seed=1, n_range=70, n_pings=150, **kw):
    b = BASE
    n_planes = 8 if max(channels) > 3 else 4
    pred, planes = planes_of(n_planes, n_range, n_pings, b["sv_ping_off"] + n_pings + 9, b["sv_ping_off"], seed)
    return run(pred, planes, channels, dtype, mode, b["seams"], b["sv_ping_off"], b["range_bin"], b["n_pb"],
               ping_bin=b["ping_bin"], **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("channels", [(3, 1, 0), (2,), (3, 1, 0, 2), (5, 0, 7, 2, 6, 1, 4, 3)], ids=["3 of 4", "1", "4", "8"])
def test_every_slice_has_the_bits_of_the_single_frequency_launch_and_matches_numpy(channels, dtype, mode):
    """70 rows x 150 pings in two launches cut at ping 100, inside ping bin 1; 4-byte sv reads (70 rows)."""
    got, want = base(channels, dtype, mode)
    same_bits(got)
    within_bound(got, want)
    assert (want[1] > 0).all() and want[2].sum() == len(channels) * 70 * 150
    assert len({got[0][i].cpu().numpy().tobytes() for i in range(len(channels))}) == len(channels)     # different planes


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("channels", [(3, 1, 0), (5, 0, 7, 2, 6, 1, 4, 3)], ids=["3 of 4", "8"])
def test_the_16_byte_sv_path_with_aligned_planes(channels, mode):
    """72 rows x 152 pings: every plane and every ping offset on the 16-byte grid (72 * 4 bytes = 18 * 16)."""
    got, want = base(channels, torch.float16, mode, seed=2, n_range=72, n_pings=152)
    same_bits(got)
    within_bound(got, want)


def test_planes_of_mixed_alignment_take_the_narrow_reads_and_stay_within_the_bound():
    """An odd plane stride: plane 0 on the 16-byte grid, plane 1 four bytes off, plane 2 eight.  Only the bound is asked."""
    b = BASE
    R, P = 72, 152
    pred, planes = planes_of(3, R, P, b["sv_ping_off"] + P + 9, b["sv_ping_off"], 3)
    size = planes.shape[1] * R
    stride = size + 1
    flat = torch.zeros(3 * stride, dtype=torch.float32, device="cuda")
    for c in range(3):
        flat[c * stride:c * stride + size] = tensor(planes[c]).reshape(-1)
    assert flat.data_ptr() % 16 == 0 and stride % 2 == 1
    got, want = run(pred, planes, (2, 0, 1), torch.float16, "probability", b["seams"], b["sv_ping_off"], b["range_bin"],
                    b["n_pb"], ping_bin=b["ping_bin"], sv_dev=flat, stride=stride)
    within_bound(got, want)
    assert torch.equal(got[1], got[3])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seabed", [(-3, "surface", 0), (-3, "seabed", 3)], ids=["limited", "3 layers"])
def test_the_seabed_forms_have_the_bits_of_crimac_integrate_layers(seabed, mode):
    line = seabed_line("slope", 150, 70)
    assert line[64:128].max() - line[64:128].min() > BASE["range_bin"]           # relief above range_bin inside a ping bin
    got, want = base((3, 1, 0), torch.float16, mode, seed=4, seabed=seabed)
    same_bits(got)
    within_bound(got, want)
    assert want[1][:, 2].sum() > 1000 and want[2].sum() < 3 * 70 * 150


@pytest.mark.parametrize("seabed", [None, (-3, "seabed", 3)], ids=["no line", "3 layers"])
def test_an_edge_table_has_the_bits_of_crimac_integrate_edges(seabed):
    """EDGES: zero-width cells, the 135-ping cell cut by the seam at ping 100, pings 0 .. 2 before the first edge."""
    pred, planes = planes_of(4, 70, 300, 37 + 300 + 9, 37, 5)
    got, want = run(pred, planes, (3, 1, 0), torch.float16, "probability", (0, 100, 300), 37, 32, len(EDGES) - 1, edges=EDGES,
                    seabed=seabed)
    same_bits(got)
    within_bound(got, want)
    assert not got[1][:, :, [0, 4]].any() and (want[1][:, 2, 5] > 0).all()
    if seabed is None:
        assert want[2].sum() == 3 * 70 * 294


@pytest.mark.parametrize("mode", MODES)
def test_bad_samples_in_one_frequency_are_absent_from_that_frequency_only(mode):
    rng = np.random.Generator(np.random.PCG64(6))
    pred = np.full((2, 70, 150), 1.0, dtype=np.float32)                         # both classes select every pixel
    planes = np.power(10.0, rng.uniform(-7.5, 0.0, size=(4, 150, 70))).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf, 0.0, -1e-3], dtype=np.float32)
    where = rng.choice(150 * 70, size=60, replace=False)
    planes[1].reshape(-1)[where] = np.tile(bad, 12)
    got, want = run(pred, planes, (3, 1, 0), torch.float16, mode, (0, 100, 150), 0, 32, 3, ping_bin=64, thr=(0.5, 0.5))
    same_bits(got)
    within_bound(got, want)
    cnt = got[1].cpu().numpy()
    assert (cnt[0] == cnt[2]).all() and cnt[0].sum(axis=(1, 2)).tolist() == [70 * 150] * 3
    assert cnt[1].sum(axis=(1, 2)).tolist() == [70 * 150 - 60] * 3              # absent from all three planes of frequency 1
    assert np.isfinite(got[0].cpu().numpy()).all()


def test_the_base_case_twice_gives_identical_bits():
    a, _ = base((3, 1, 0), torch.float16, "probability", numpy_too=False)
    b, _ = base((3, 1, 0), torch.float16, "probability", numpy_too=False)
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1], b[1]) and a[1].sum() > 0


def test_a_scratch_sized_for_one_frequency_is_refused_and_nothing_is_written():
    pred, planes = planes_of(4, 70, 150, 160, 0, 7)
    pred_d, sv_d = tensor(pred, torch.float16), tensor(planes)
    acc = torch.full((4, 3, 3, 3), POISON, dtype=torch.float64, device="cuda")
    cnt = torch.full((4, 3, 3, 3), int(POISON), dtype=torch.int64, device="cuda")
    one = 9 * 2 * SLOT                                           # one frequency: 9 cells x min(ceil(1024 / 9), 1 x 2 tiles) splits
    need = 4 * one
    scratch = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    chan = (ctypes.c_int * 4)(3, 1, 0, 2)
    args = [ptr(pred_d), 1, 70, 150, ptr(sv_d), 160 * 70, 4, chan, 4, 160, 0, 0.5, 0.5, 0, 64, None, None, 32, 0, 3, None, 0, 0,
            0, 0, 0, ptr(acc), ptr(cnt), ptr(scratch)]
    with pytest.raises(hip.HipLibraryError, match="scratch") as e:
        call("crimac_integrate_freqs", *args, one)
    assert str(need) in str(e.value)
    torch.cuda.synchronize()
    assert (acc == POISON).all() and (cnt == int(POISON)).all()
    call("crimac_integrate_freqs", *args, need)                  # with exactly what it states, it runs
    torch.cuda.synchronize()
    assert (cnt > int(POISON)).all()


# ---- the flows ----------------------------------------------------------------------------------------------------------
ORDER = (200, 18, 120, 38)                                      # all four frequencies, permuted


@pytest.fixture(scope="module")
def stub_pipe():
    return types.SimpleNamespace(model=pkg.UNet_Baseline(3, 4, start_filts=8, precision="f32x6").cuda().eval(),
                                 device=torch.device("cuda"), frequencies=FREQS)


@pytest.fixture(scope="module")
def reader():
    sv, labels, seabed = synth_survey()
    return FakeZarrReader(sv[:, :700, :300].copy(), labels[:700, :300].copy(), np.clip(seabed[:700], 0, 260))


def stacked(multi, singles):
    """The multi result against the stack of the single-frequency results: every sum bit for bit, every count."""
    assert multi["frequencies"] == ORDER and multi["sv_sum"].shape == (4, *singles[0]["sv_sum"].shape)
    assert multi["sv_sum"].dtype == np.float64 and multi["pixels"].dtype == np.int64
    assert multi["sv_sum"].tobytes() == np.stack([s["sv_sum"] for s in singles]).tobytes()
    assert np.array_equal(multi["pixels"], np.stack([s["pixels"] for s in singles]))
    for key in ("ping_edges", "range_edges"):
        assert np.array_equal(multi[key], singles[0][key])
    assert set(multi) == set(singles[0]) | {"frequencies"} and multi["pixels"][:, 2].sum() > 0


SURVEY_SPECS = {"default": dict(ping_bin=100), "layers": dict(ping_bin=100, seabed_offset=-5, reference="seabed", layers=3),
                "edges": dict(ping_bin=None, ping_edges=np.array([7, 7, 120, 250, 251, 610, 690]))}


@pytest.mark.parametrize("which", list(SURVEY_SPECS))
def test_integrate_survey_with_four_frequencies_equals_four_passes(reader, stub_pipe, which, monkeypatch):
    kw = dict(SURVEY_SPECS[which])
    ping_bin = kw.pop("ping_bin")
    names = []
    real = ti.call
    monkeypatch.setattr(ti, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    multi = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 250, ti.IntegrationSpec(ping_bin, 64, frequency=ORDER, **kw),
                                predict_fn=hashed_predict_fn)
    assert names.count("crimac_integrate_freqs") == 3 and not [n for n in names if n.startswith("crimac_integrate_")
                                                              and n != "crimac_integrate_freqs"]
    singles = [ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 250, ti.IntegrationSpec(ping_bin, 64, frequency=f, **kw),
                                   predict_fn=hashed_predict_fn) for f in ORDER]
    assert names.count("crimac_integrate_freqs") == 3            # a scalar frequency launches what it launched before
    stacked(multi, singles)
    assert len({s["sv_sum"].tobytes() for s in singles}) == 4
    r = ti.frequency_response(multi)
    assert r.shape == multi["sv_sum"].shape and np.array_equal(r[3][multi["sv_sum"][3] > 0], np.ones((multi["sv_sum"][3] > 0).sum()))
    assert ti.mean_nasc(multi, 0.19).shape == multi["sv_sum"].shape
    one = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 250, ti.IntegrationSpec(ping_bin, 64, frequency=[120], **kw),
                              predict_fn=hashed_predict_fn)
    assert one["frequencies"] == (120,) and one["sv_sum"][0].tobytes() == singles[2]["sv_sum"].tobytes()


def test_integrate_echogram_memm_with_four_frequencies_equals_four_passes(stub_pipe):
    sv, labels, seabed = synth_survey(n_pings=300, n_range=90, seed=12)
    eg = FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), np.clip(seabed, 1, 80),
                      frequencies=FREQS)
    for kw in (dict(ping_bin=64), dict(ping_bin=None, ping_edges=EDGES, seabed_offset=3, reference="seabed", layers=3)):
        kw = dict(kw)
        ping_bin = kw.pop("ping_bin")
        multi = ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, ti.IntegrationSpec(ping_bin, 20, frequency=ORDER,
                                           mode="probability", **kw), predict_fn=hashed_predict_fn)
        singles = [ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, ti.IntegrationSpec(ping_bin, 20, frequency=f,
                                              mode="probability", **kw), predict_fn=hashed_predict_fn) for f in ORDER]
        stacked(multi, singles)


MEMM = [(300, 92), (40, 132), (172, 64), (64, 128), (101, 60)]             # pings x range; 101 x 60: off the 16-byte grid


def test_integrate_echograms_memm_with_four_frequencies_equals_four_passes(stub_pipe, monkeypatch):
    """Every n_range here is a multiple of 4 and the planes of an echogram lie pings * n_range elements apart, so the planes
    of one echogram are all on or all off the 16-byte grid: the condition under which the slices have the bits of the
    single-frequency launches, whatever the echogram's place in the staging."""
    egs = [echogram(p, r, 80 + i, name=f"eg{i}") for i, (p, r) in enumerate(MEMM)]
    names = []
    real = ti.call
    monkeypatch.setattr(ti, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    counts = [len(r.grid) for g in ti.iter_memm_groups(iter(egs), (64, 64), 6, 10 ** 9) for r in g]
    kw = dict(thresholds=THR, seabed_offset=-3)
    stats = {}
    multi = list(ti.integrate_echograms_memm(iter(egs), stub_pipe, (64, 64), 6, 8, ti.IntegrationSpec(40, 16, frequency=ORDER, **kw),
                                             predict_fn=hashed_predict_fn, stats=stats, group_patches=counts[0] + counts[1] // 2))
    assert stats["groups"] >= 2 and stats["solo_echograms"] == 0 and names.count("crimac_integrate_freqs") == 5
    singles = [list(ti.integrate_echograms_memm(iter(egs), stub_pipe, (64, 64), 6, 8, ti.IntegrationSpec(40, 16, frequency=f, **kw),
                                                predict_fn=hashed_predict_fn, group_patches=counts[0] + counts[1] // 2))
               for f in ORDER]
    assert [eg for eg, _ in multi] == egs
    for k, (eg, res) in enumerate(multi):
        stacked(res, [s[k][1] for s in singles])
        assert res["sv_sum"].shape[2:] == ti.IntegrationSpec(40, 16).bins(*MEMM[k])
    ti.release_staging()


def test_a_real_narrow_network_with_four_frequencies_matches_predict_survey_then_numpy():
    sv, labels, seabed = synth_survey(n_pings=230, n_range=120, seed=11)
    reader = FakeZarrReader(sv, labels, np.clip(seabed, 0, 100))
    model = pkg.UNet_Baseline(3, 4, start_filts=8, precision="h3p")
    model.load_state_dict(synth.synth_state_dict(start_filts=8, seed=4))
    pipe = types.SimpleNamespace(model=model.cuda().eval(), device=torch.device("cuda"), frequencies=FREQS)
    spec = ti.IntegrationSpec(50, 25, frequency=ORDER, mode="probability")
    chunks = [(s, out) for s, e, out in ti.predict_survey(reader, pipe, (64, 64), 6, 8, 120, out_dtype=np.float16)]
    assert len(chunks) == 2
    got = ti.integrate_survey(reader, pipe, (64, 64), 6, 8, 120, spec)
    assert got["frequencies"] == ORDER and got["sv_sum"].shape == (4, 3, 5, 5)
    for i, f in enumerate(ORDER):
        want = new_host(5, 5)
        for s, out in chunks:
            edges_numpy(*want, out, sv[FREQS.index(f)], spec.thresholds, spec.mode, np.arange(6) * 50, 25, s, s)
        check(got["sv_sum"][i], got["pixels"][i], *want)
    assert got["pixels"][:, 2].sum() > 0.9 * 4 * 230 * 120 and (got["sv_sum"][:, :2].sum(axis=(2, 3)) > 0).all()
