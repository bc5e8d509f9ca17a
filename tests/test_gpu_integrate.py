"""GPU: echo integration by predicted class -- ``crimac_integrate_classes`` (csrc/integrate.hip) on synthetic operands, and
``integrate_survey`` / ``integrate_echogram_memm`` against the prediction flows they reduce.

The comparison target is ``integrate_numpy`` below: float64 numpy on the DOWNLOADED stored predictions and the host sv.
Counts must be equal exactly.  Sums: every term is >= 0, so any summation order of n terms in fp64 is within n * 2^-53
relative of the exact sum; the kernel's and numpy's orders differ, a probability-mode product (float32 x float32, exact in
fp64 on both sides) adds nothing, and accumulating launches / chunks into a cell adds fewer additions than the cell has
pixels.  The bound used is (n_cell_pixels + 2) * 2^-52 * sum per cell, n_cell_pixels = the pixels of the cell the launches
covered; a cell whose expected sum is 0 must be exactly 0."""
import types

import numpy as np
import pytest
import torch

import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import hip, synth
from crimac_classifiers_unet_amd import tiled_inference as ti
from crimac_classifiers_unet_amd.hip import call, ptr
from tools.fake_reader import FakeEchogram, FakeZarrReader, synth_survey

pytestmark = pytest.mark.gpu

FREQS = [18, 38, 120, 200]
MODES = ("threshold", "probability")


# ---- the numpy statement of the kernel --------------------------------------------------------------------------------
def integrate_numpy(acc, cnt, geo, pred, sv, thr, mode, ping_bin, range_bin, ping_origin, sv_ping_off=0):
    """One launch, accumulated into ``acc`` float64 / ``cnt`` int64 / ``geo`` int64 (the pixels covered, for the bound), all
    [3, n_pb_total, n_rb] ([n_pb_total, n_rb] for ``geo``).  ``pred`` [2, R, P] as stored (float16 / float32), ``sv``
    [data_pings, R] float32."""
    R, P = pred.shape[1:]
    s = np.asarray(sv[sv_ping_off:sv_ping_off + P], dtype=np.float32).T              # [R, P]
    assert s.shape == (R, P)
    ok = np.isfinite(s) & (s > 0)
    s64 = np.where(ok, s, 0).astype(np.float64)
    p32 = pred.astype(np.float32)                                                   # the stored value, widened exactly
    if mode == "threshold":
        member = p32 >= np.asarray(thr, dtype=np.float32)[:, None, None]            # a float32 comparison
        weight = member.astype(np.float64)
    else:
        member = p32 > 0
        weight = np.where(member, p32, 0).astype(np.float64)
    sums = np.stack([s64 * weight[0], s64 * weight[1], s64])
    counts = np.stack([ok & member[0], ok & member[1], ok]).astype(np.int64)
    pb = (ping_origin + np.arange(P)) // ping_bin
    p_starts = np.nonzero(np.diff(pb, prepend=pb[0] - 1))[0]
    r_starts = np.arange(0, R, range_bin)
    cells = (slice(None), slice(int(pb[0]), int(pb[-1]) + 1), slice(None))

    def binned(a):
        return np.add.reduceat(np.add.reduceat(a, r_starts, axis=-2), p_starts, axis=-1).swapaxes(-1, -2)
    acc[cells] += binned(sums)
    cnt[cells] += binned(counts)
    geo[cells[1:]] += binned(np.ones((R, P), dtype=np.int64))


def new_host(n_pb_total, n_range, range_bin):
    n_rb = -(-n_range // range_bin)
    return (np.zeros((3, n_pb_total, n_rb)), np.zeros((3, n_pb_total, n_rb), dtype=np.int64),
            np.zeros((n_pb_total, n_rb), dtype=np.int64))


def check(got_sum, got_cnt, want_sum, want_cnt, geo):
    assert got_sum.dtype == np.float64 and got_cnt.dtype == np.int64
    assert got_sum.shape == want_sum.shape and got_cnt.shape == want_cnt.shape
    assert np.array_equal(got_cnt, want_cnt)
    bound = (geo[None] + 2) * 2.0 ** -52 * want_sum
    err = np.abs(got_sum - want_sum)
    print(f"largest |sum error| / bound over the cells with a sum: "
          f"{float((err[want_sum > 0] / bound[want_sum > 0]).max()) if (want_sum > 0).any() else 0.0:.3f}")
    assert (err <= bound).all()
    assert (got_sum[want_sum == 0] == 0).all()


def launch(acc, cnt, pred, sv, thr, mode, ping_bin, range_bin, ping_origin, sv_ping_off=0, expect_ok=True):
    """``crimac_integrate_classes`` on device tensors ``pred`` [2, R, P] (float16 / float32) and ``sv`` [data_pings, R]."""
    _, R, P = pred.shape
    n_pb_total, n_rb = acc.shape[1:]
    cells = ((ping_origin + P - 1) // max(ping_bin, 1) - ping_origin // max(ping_bin, 1) + 1) * n_rb
    scratch = torch.empty((cells + hip.INTEGRATE_SPLIT_WGS) * hip.INTEGRATE_SLOT_BYTES // 8, dtype=torch.float64, device="cuda")
    args = (ptr(pred), int(pred.dtype == torch.float16), R, P, ptr(sv), sv.shape[0], sv_ping_off, float(thr[0]),
            float(thr[1]), MODES.index(mode), ping_bin, range_bin, ping_origin, n_pb_total, ptr(acc), ptr(cnt), ptr(scratch),
            scratch.numel() * 8)
    if expect_ok:
        call("crimac_integrate_classes", *args)
    return args


def new_device(n_pb_total, n_range, range_bin):
    shape = (3, n_pb_total, -(-n_range // range_bin))
    return torch.zeros(shape, dtype=torch.float64, device="cuda"), torch.zeros(shape, dtype=torch.int64, device="cuda")


F16_LEVELS = np.array([0, 0, 0.0999755859375, 0.25, 0.5, 0.7001953125, 0.89990234375, 1.0], dtype=np.float16)
THR_ON_A_LEVEL = (0.7001953125, 0.25)             # both are stored float16 values of F16_LEVELS


def operands(n_range, n_pings, data_pings, sv_ping_off, seed, levels=True):
    """pred float32 [2, R, P] whose values are float16-representable (``levels``: drawn from F16_LEVELS, so that a threshold
    can sit exactly on a stored value), sv float32 [data_pings, R] linear, with NaN, +Inf, -Inf, 0 and negative entries
    planted INSIDE pixels that both classes select."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if levels:
        pred = F16_LEVELS[rng.integers(0, len(F16_LEVELS), size=(2, n_range, n_pings))].astype(np.float32)
    else:
        pred = rng.random((2, n_range, n_pings)).astype(np.float16).astype(np.float32)
    sv = np.power(10.0, rng.uniform(-7.5, 0.0, size=(data_pings, n_range))).astype(np.float32)
    both = np.argwhere((pred[0] >= 0.89) & (pred[1] >= 0.89))                        # (row, ping) selected by both classes
    bad = np.array([np.nan, np.inf, -np.inf, 0.0, -1e-3], dtype=np.float32)
    planted = both[:len(bad) * (len(both) // len(bad))]
    for k, (r, p) in enumerate(planted):
        sv[sv_ping_off + p, r] = bad[k % len(bad)]
    return pred, sv, planted


def tensor(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


# ---- kernel-level cases ---------------------------------------------------------------------------------------------------
MULTI = dict(n_range=70, n_pings=150, range_bin=32, ping_bin=64, seam=100, sv_ping_off=37, n_pb_total=3)


def multi_launch(dtype, mode, thr, seed=1):
    """The multi-launch case: pings [0, 100) and [100, 150) into one accumulator; the seam lies inside ping bin 1, the last
    range bin (rows 64 .. 69) is partial; n_range = 70 takes the 4-byte sv reads, 100 pings the 16- / 8-byte pred reads,
    50 pings the scalar ones."""
    m = MULTI
    pred, sv, planted = operands(m["n_range"], m["n_pings"], m["sv_ping_off"] + m["n_pings"] + 9, m["sv_ping_off"], seed)
    want = new_host(m["n_pb_total"], m["n_range"], m["range_bin"])
    acc, cnt = new_device(m["n_pb_total"], m["n_range"], m["range_bin"])
    sv_d = tensor(sv)
    stored = []
    for p0, p1 in ((0, m["seam"]), (m["seam"], m["n_pings"])):
        part = tensor(pred[:, :, p0:p1], dtype)
        stored.append(part.cpu().numpy())
        launch(acc, cnt, part, sv_d, thr, mode, m["ping_bin"], m["range_bin"], p0, m["sv_ping_off"] + p0)
        integrate_numpy(*want, stored[-1], sv, thr, mode, m["ping_bin"], m["range_bin"], p0, m["sv_ping_off"] + p0)
    return acc.cpu().numpy(), cnt.cpu().numpy(), want, (pred, sv, planted)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_two_launches_across_a_ping_bin_match_numpy(dtype, mode):
    got_sum, got_cnt, (want_sum, want_cnt, geo), _ = multi_launch(dtype, mode, (0.5, 0.5))
    assert geo.sum() == 70 * 150 and geo[1, 2] == 64 * 6 and (want_cnt[:2] > 0).all()
    check(got_sum, got_cnt, want_sum, want_cnt, geo)


def test_a_threshold_equal_to_a_stored_float16_value_includes_the_pixel():
    got_sum, got_cnt, (want_sum, want_cnt, geo), (pred, sv, _) = multi_launch(torch.float16, "threshold", THR_ON_A_LEVEL)
    check(got_sum, got_cnt, want_sum, want_cnt, geo)
    # the pixels that sit exactly on the threshold are many, and a strict comparison would have lost them
    s = sv[MULTI["sv_ping_off"]:MULTI["sv_ping_off"] + 150].T
    ok = np.isfinite(s) & (s > 0)
    for k in (0, 1):
        on = ok & (pred[k] == np.float32(THR_ON_A_LEVEL[k]))
        assert on.sum() > 500
        assert got_cnt[k].sum() == (ok & (pred[k] >= np.float32(THR_ON_A_LEVEL[k]))).sum()
        assert got_cnt[k].sum() - on.sum() == (ok & (pred[k] > np.float32(THR_ON_A_LEVEL[k]))).sum()


@pytest.mark.parametrize("mode", MODES)
def test_bad_sv_samples_are_absent_from_every_plane(mode):
    got_sum, got_cnt, (want_sum, want_cnt, geo), (pred, sv, planted) = multi_launch(torch.float16, mode, (0.5, 0.5), seed=2)
    assert len(planted) >= 50                                                     # NaN, +Inf, -Inf, 0, < 0: ten or more each
    check(got_sum, got_cnt, want_sum, want_cnt, geo)
    assert np.isfinite(got_sum).all() and (got_sum >= 0).all()
    assert got_cnt[2].sum() == 70 * 150 - len(planted)                            # every other sample is finite and > 0
    s = sv[MULTI["sv_ping_off"]:MULTI["sv_ping_off"] + 150].T
    member = pred >= 0.5 if mode == "threshold" else pred > 0
    good = np.isfinite(s) & (s > 0)
    assert [int(got_cnt[k].sum()) for k in (0, 1)] == [int((member[k] & good).sum()) for k in (0, 1)]
    assert all(member[k][planted[:, 0], planted[:, 1]].all() for k in (0, 1))      # they were selected pixels


def test_the_multi_launch_case_twice_gives_identical_bits():
    for mode in MODES:
        a = multi_launch(torch.float16, mode, (0.5, 0.5))
        b = multi_launch(torch.float16, mode, (0.5, 0.5))
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


CASES = {
    # n_range, n_pings, range_bin, ping_bin, ping_origin, n_pb_total
    "one pixel per cell, 5 x 7": (5, 7, 1, 1, 0, 7),
    "one pixel per cell, from ping 3": (5, 7, 1, 1, 3, 10),
    "one cell larger than the array (8 tiles over 8 workgroups)": (72, 200, 1000, 5000, 300, 1),
    "16-byte paths, bins off the 4-element grid": (72, 200, 10, 30, 7, 7),
    "544 cells of 3 tiles over 2 splits each": (136, 520, 1, 130, 0, 4),
    "1040 cells of 3 tiles, no split": (260, 520, 1, 130, 0, 4),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("case", list(CASES))
def test_edge_geometries_match_numpy(case, dtype, mode):
    R, P, range_bin, ping_bin, origin, n_pb_total = CASES[case]
    pred, sv, _ = operands(R, P, P + 3, 2, seed=3, levels=False)
    want = new_host(n_pb_total, R, range_bin)
    acc, cnt = new_device(n_pb_total, R, range_bin)
    pred_d = tensor(pred, dtype)
    launch(acc, cnt, pred_d, tensor(sv), (0.5, 0.4), mode, ping_bin, range_bin, origin, 2)
    integrate_numpy(*want, pred_d.cpu().numpy(), sv, (0.5, 0.4), mode, ping_bin, range_bin, origin, 2)
    assert want[2].sum() == R * P
    check(acc.cpu().numpy(), cnt.cpu().numpy(), *want)


def test_operands_off_the_16_byte_grid_take_the_narrow_reads():
    """The same extents as the 16-byte case, but both base addresses one element off: still right."""
    R, P, range_bin, ping_bin, origin, n_pb_total = CASES["16-byte paths, bins off the 4-element grid"]
    pred, sv, _ = operands(R, P, P + 3, 2, seed=4, levels=False)
    want = new_host(n_pb_total, R, range_bin)
    acc, cnt = new_device(n_pb_total, R, range_bin)
    pred_d = torch.zeros(pred.size + 1, dtype=torch.float32, device="cuda")[1:].view(pred.shape)
    sv_d = torch.zeros(sv.size + 1, dtype=torch.float32, device="cuda")[1:].view(sv.shape)
    pred_d.copy_(torch.from_numpy(pred))
    sv_d.copy_(torch.from_numpy(sv))
    assert pred_d.data_ptr() % 16 == 4 and sv_d.data_ptr() % 16 == 4
    launch(acc, cnt, pred_d, sv_d, (0.5, 0.4), "threshold", ping_bin, range_bin, origin, 2)
    integrate_numpy(*want, pred, sv, (0.5, 0.4), "threshold", ping_bin, range_bin, origin, 2)
    check(acc.cpu().numpy(), cnt.cpu().numpy(), *want)


@pytest.mark.parametrize("mode", MODES)
def test_an_all_zero_pred_plane_gives_exact_zeros(mode):
    pred, sv, _ = operands(70, 150, 150, 0, seed=5)
    pred[1] = 0
    acc, cnt = new_device(3, 70, 32)
    launch(acc, cnt, tensor(pred, torch.float16), tensor(sv), (0.5, 0.5), mode, 64, 32, 0)
    got_sum, got_cnt = acc.cpu().numpy(), cnt.cpu().numpy()
    assert (got_sum[1] == 0).all() and (got_cnt[1] == 0).all()
    assert (got_sum[0] > 0).all() and (got_cnt[0] > 0).all() and (got_cnt[2] > got_cnt[0]).all()


def test_argument_errors_are_reported_and_launch_nothing():
    lib = hip.load_library()
    pred, sv, _ = operands(70, 150, 160, 0, seed=6)
    pred_d, sv_d = tensor(pred), tensor(sv)
    acc, cnt = new_device(3, 70, 32)
    good = dict(thr=(0.5, 0.5), ping_bin=64, range_bin=32, ping_origin=0, sv_ping_off=0)
    for change, word in ((dict(thr=(0.0, 0.5)), "thr"), (dict(thr=(0.5, -1.0)), "thr"), (dict(ping_bin=0), "ping_bin"),
                         (dict(range_bin=0), "range_bin"), (dict(sv_ping_off=11), "sv extent"),
                         (dict(sv_ping_off=-1), "sv extent"), (dict(ping_origin=64), "accumulator")):
        kw = dict(good, **change)
        args = launch(acc, cnt, pred_d, sv_d, kw["thr"], "threshold", kw["ping_bin"], kw["range_bin"], kw["ping_origin"],
                      kw["sv_ping_off"], expect_ok=False)
        with pytest.raises(hip.HipLibraryError, match=word):
            call("crimac_integrate_classes", *args)
        assert word.encode() in lib.crimac_last_error()
    args = list(launch(acc, cnt, pred_d, sv_d, (0.5, 0.5), "threshold", 64, 32, 0, expect_ok=False))
    for at, value, word in ((9, 2, "mode"), (17, 48, "scratch")):
        bad = list(args)
        bad[at] = value
        with pytest.raises(hip.HipLibraryError, match=word):
            call("crimac_integrate_classes", *bad)
    torch.cuda.synchronize()
    assert not acc.any() and not cnt.any()                                        # nothing was launched


# ---- flow-level cases -------------------------------------------------------------------------------------------------------
def hashed_predict_fn(x, P, H, W):
    """Fixed pseudo-random probabilities: a per-pixel hash of the four dB input channels, elementwise, so a patch's result
    cannot depend on the batch around it.  About a third of the pixels pass 0.5 in either class."""
    d = x.float().reshape(P, H, W, 16)[..., :4].permute(0, 3, 1, 2)
    h = d[:, 0] * 12.9898 + d[:, 1] * 78.233 + d[:, 2] * 37.719 + d[:, 3] * 4.581
    u = torch.frac(torch.sin(h) * 43758.5453).abs()
    v = torch.frac(torch.sin(h * 1.618) * 24634.6345).abs()
    sandeel = 0.02 + 0.96 * u * v.sqrt()
    other = (1 - sandeel) * v
    return torch.stack([1 - sandeel - other, sandeel, other], dim=1).contiguous()


def make_pipe(model):
    return types.SimpleNamespace(model=model.cuda().eval(), device=torch.device("cuda"), frequencies=FREQS)


@pytest.fixture(scope="module")
def stub_pipe():
    return make_pipe(pkg.UNet_Baseline(3, 4, start_filts=8, precision="f32x6"))


@pytest.fixture(scope="module")
def reader():
    sv, labels, seabed = synth_survey()
    sv, labels, seabed = sv[:, :700, :300].copy(), labels[:700, :300].copy(), np.clip(seabed[:700], 0, 260)
    return FakeZarrReader(sv, labels, seabed)


def survey_by_numpy(reader, pipe, patch, overlap, batch, preload, spec, **kw):
    """What a user does today: ``predict_survey(out_dtype=np.float16)``, then the integration on the host."""
    n_pings, n_range = reader.shape
    n_pb, n_rb = spec.bins(n_pings, n_range)
    want = new_host(n_pb, n_range, spec.range_bin)
    sv = reader.sv[FREQS.index(38)]
    chunks = []
    for s, e, out in ti.predict_survey(reader, pipe, patch, overlap, batch, preload, out_dtype=np.float16, **kw):
        assert out.dtype == np.float16
        integrate_numpy(*want, out, sv, spec.thresholds, spec.mode, spec.ping_bin, spec.range_bin, s, s)
        chunks.append((s, e))
    return want, chunks


@pytest.fixture(scope="module")
def stub_survey(reader, stub_pipe):
    """The references of the flow tests, computed once: per mode (spec, (sum, count, pixels covered), the chunks)."""
    out = {}
    for mode in MODES:
        spec = ti.IntegrationSpec(ping_bin=100, range_bin=64, mode=mode, thresholds=(0.5, 0.4))
        out[mode] = (spec, *survey_by_numpy(reader, stub_pipe, (256, 256), 20, 3, 250, spec, predict_fn=hashed_predict_fn))
    return out


@pytest.mark.parametrize("mode", MODES)
def test_integrate_survey_equals_predict_survey_then_numpy(reader, stub_pipe, stub_survey, mode):
    spec, (want_sum, want_cnt, geo), chunks = stub_survey[mode]
    assert chunks == [(0, 233), (233, 466), (466, 700)] and all(s % spec.ping_bin for s, _ in chunks[1:])
    stats = {}
    got = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 250, spec, predict_fn=hashed_predict_fn, stats=stats)
    assert got["classes"] == ("sandeel", "other", "all") and len(stats["gpu_events"]) == 3
    assert got["ping_edges"].tolist() == [0, 100, 200, 300, 400, 500, 600, 700]
    assert got["range_edges"].tolist() == [0, 64, 128, 192, 256, 300]
    check(got["sv_sum"], got["pixels"], want_sum, want_cnt, geo)
    assert (want_cnt[:2, :, :3] > 0).all()                                       # both classes are there above the seabed
    assert (want_cnt[2] >= want_cnt[0]).all() and want_cnt[2].sum() > 0.99 * 700 * 300
    # another batch size: the same bits
    again = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 5, 250, spec, predict_fn=hashed_predict_fn)
    assert again["sv_sum"].tobytes() == got["sv_sum"].tobytes() and np.array_equal(again["pixels"], got["pixels"])


def test_integrate_survey_from_a_later_start_ping_counts_nothing_before_it(reader, stub_pipe):
    spec = ti.IntegrationSpec(ping_bin=100, range_bin=300, thresholds=(0.5, 0.4))
    want, chunks = survey_by_numpy(reader, stub_pipe, (256, 256), 20, 4, 250, spec, predict_fn=hashed_predict_fn,
                                   start_ping=430)
    assert chunks[0][0] == 430
    got = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 4, 250, spec, start_ping=430, predict_fn=hashed_predict_fn)
    check(got["sv_sum"], got["pixels"], *want)
    assert not got["pixels"][:, :4].any() and got["pixels"][2, 4, 0] == want[1][2, 4, 0] > 0


def test_integrate_survey_with_a_real_small_network():
    sv, labels, seabed = synth_survey(n_pings=230, n_range=120, seed=11)
    reader = FakeZarrReader(sv, labels, np.clip(seabed, 0, 100))
    model = pkg.UNet_Baseline(3, 4, start_filts=8, precision="h3p")
    model.load_state_dict(synth.synth_state_dict(start_filts=8, seed=4))
    pipe = make_pipe(model)
    spec = ti.IntegrationSpec(ping_bin=48, range_bin=25, mode="probability")       # (whatever the network predicts, it weighs)
    want, chunks = survey_by_numpy(reader, pipe, (64, 64), 6, 8, 120, spec)
    assert len(chunks) == 2
    got = ti.integrate_survey(reader, pipe, (64, 64), 6, 8, 120, spec)
    check(got["sv_sum"], got["pixels"], *want)
    assert got["pixels"][2].sum() > 0.9 * 230 * 120 and (got["sv_sum"][:2].sum(axis=(1, 2)) > 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_integrate_echogram_memm_equals_predict_echogram_memm_then_numpy(stub_pipe, mode):
    sv, labels, seabed = synth_survey(n_pings=300, n_range=90, seed=12)
    eg = FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), np.clip(seabed, 1, 80),
                      frequencies=FREQS)
    spec = ti.IntegrationSpec(ping_bin=77, range_bin=40, frequency=120, mode=mode)
    out = ti.predict_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, predict_fn=hashed_predict_fn)
    stored = out.astype(np.float16)
    assert np.array_equal(stored.astype(np.float64), out)                           # (it returns the float16 values)
    want = new_host(4, 90, 40)
    integrate_numpy(*want, stored, sv[FREQS.index(120)], spec.thresholds, mode, 77, 40, 0)
    got = ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn)
    assert got["ping_edges"].tolist() == [0, 77, 154, 231, 300] and got["range_edges"].tolist() == [0, 40, 80, 90]
    check(got["sv_sum"], got["pixels"], *want)
    assert got["pixels"][:2].sum() > 0


def test_chunk_predictor_integrate_refuses_what_it_cannot_reduce(stub_pipe, reader):
    cp = ti.ChunkPredictor(stub_pipe.model, 300, (256, 256), 20, 4, out_f16=True)
    n = 233
    cp.load_chunk(reader.get_data_slice(0, n), 0, reader.get_label_slice(0, n), None, 0, n, seabed=reader.get_seabed(0, n),
                  wide=True)
    spec = ti.IntegrationSpec(100, 64).bind(FREQS)
    acc, cnt = ti.new_integration("cuda", spec, 700, 300)
    with pytest.raises(ValueError, match="wide"):
        cp.integrate(acc, cnt, spec)
    cp.load_chunk(reader.get_data_slice(0, n), 0, reader.get_label_slice(0, n), None, 0, n, seabed=reader.get_seabed(0, n))
    with pytest.raises(ValueError, match="bind"):
        cp.integrate(acc, cnt, ti.IntegrationSpec(100, 64))
    with pytest.raises(ValueError, match="acc float64"):
        cp.integrate(acc.float(), cnt, spec)
    with pytest.raises(ValueError, match="acc float64"):
        cp.integrate(acc[:, :2].contiguous(), cnt[:, :2].contiguous(), spec)
