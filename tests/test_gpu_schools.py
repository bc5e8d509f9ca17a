"""Schools from the predictions on the GPU: crimac_schools_label / crimac_schools_stats against the CPU reference detector
(tests/schools_ref.py: scipy.ndimage.label relabelled to anchors, float64 sums), exactly, at the smallest shapes where the
kernels can go wrong -- off every tile multiple in both axes, one tile and several --, and the flows end to end.

The sv bound: with n = sv_pixels of a school, |gpu - ref| <= n * 2^-52 * ref (all terms are positive, so any order of
summation is within (n - 1) u of the exact sum on each side).  The error flag of the union-find loops is NOT provoked
here: their bounds are checked on the host by tools/exp/ccl_host_check.cpp."""
import ctypes
import types

import numpy as np
import pytest
import torch

import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti
from crimac_classifiers_unet_amd.hip import call, ptr
from tools.fake_reader import FakeEchogram, FakeZarrReader, synth_survey

import schools_ref as ref
from test_gpu_integrate import hashed_predict_fn  # noqa: E402

pytestmark = pytest.mark.gpu
FREQS = (18, 38, 120, 200)
THR = 0.5


def tensor(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def planes_for(R, P, n_planes=4, sv_ping_off=0, extra=0, seed=0):
    """sv float32 [n_planes, data_pings, R] linear, with NaN, +-Inf, 0 and negative samples scattered through it."""
    rng = np.random.Generator(np.random.PCG64(seed + 17 * R + P))
    sv = np.power(10.0, rng.uniform(-7.5, 0.0, size=(n_planes, sv_ping_off + P + extra, R))).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf, 0.0, -1e-3], dtype=np.float32)
    flat = sv.reshape(-1)
    at = rng.choice(flat.size, size=max(flat.size // 9, 1), replace=False)
    flat[at] = bad[np.arange(len(at)) % len(bad)]
    return sv


def label_gpu(pred_t, thr, connectivity):
    R, P = pred_t.shape
    labels = torch.full((R, P), -9, dtype=torch.int32, device="cuda")
    status = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    call("crimac_schools_label", ptr(pred_t), 1 if pred_t.dtype == torch.float16 else 0, R, P, thr, connectivity, ptr(labels),
         ptr(status))
    return labels, status


def stats_gpu(labels, sv_t, channels, sv_ping_off=0, min_pixels=1, keep_left=False, keep_right=False, capacity=None):
    """One crimac_schools_stats; the table as numpy, cut to min(found, capacity), plus ``found`` and ``edges``."""
    R, P = labels.shape
    F = len(channels)
    K = capacity or R * P
    i32 = lambda *s: torch.full(s, -77, dtype=torch.int32, device="cuda")      # noqa: E731
    i64 = lambda *s: torch.full(s, -77, dtype=torch.int64, device="cuda")      # noqa: E731
    t = dict(anchor=i32(K), pixels=i64(K), bbox=i32(K, 4), row_sum=i64(K), ping_sum=i64(K),
             sv_sum=torch.full((F, K), -77.0, dtype=torch.float64, device="cuda"), sv_pixels=i64(F, K))
    found, edges = i64(1), i32(2, R)
    scratch = torch.empty((hip.DEFINES["CRIMAC_SCHOOLS_SCRATCH_PIXEL_BYTES"] * R * P + 16 + 7) // 8, dtype=torch.float64, device="cuda")
    call("crimac_schools_stats", ptr(labels), R, P, ptr(sv_t[0]), int(sv_t.stride(0)), int(sv_t.shape[0]),
         (ctypes.c_int * F)(*channels), F, int(sv_t.shape[1]), sv_ping_off, min_pixels, int(keep_left), int(keep_right), K,
         *(ptr(t[name]) for name in ti.SCHOOL_FIELDS), ptr(found), ptr(edges), ptr(scratch), scratch.numel() * 8)
    n = int(found.item())
    out = {name: (v[..., :min(n, K)] if name in ("sv_sum", "sv_pixels") else v[:min(n, K)]).cpu().numpy() for name, v in t.items()}
    rest = {name: (v[..., min(n, K):] if name in ("sv_sum", "sv_pixels") else v[min(n, K):]).cpu().numpy() for name, v in t.items()}
    assert all(np.all(v == -77) for v in rest.values()), "rows from min(found, capacity) on were written"
    out.update(found=n, edges=edges.cpu().numpy())
    return out


def check_case(mask, dtype, connectivity, sv, channels=(1,), sv_ping_off=0, **kw):
    pred = np.where(mask, 0.75, 0.25).astype(np.float32)
    labels, status = label_gpu(tensor(pred, dtype), THR, connectivity)
    want = ref.detect(mask, sv[list(channels), sv_ping_off:sv_ping_off + mask.shape[1]], connectivity, **kw)
    assert int(status.item()) == 0
    assert np.array_equal(labels.cpu().numpy(), want["labels"])
    got = stats_gpu(labels, tensor(sv), channels, sv_ping_off, **kw)
    assert got["found"] == len(want["anchor"])
    ref.same_schools(got, want, fields=ref.INT_FIELDS + ("edges",))
    return got, want, labels


# ---- the kernels against the reference, exactly ----------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_pattern_equals_the_reference_detector(shape, connectivity):
    R, P = shape
    sv = planes_for(R, P, n_planes=2)
    for name in ref.PATTERNS:
        mask = ref.pattern(name, R, P)
        for dtype in (torch.float16, torch.float32):
            got, want, _ = check_case(mask, dtype, connectivity, sv)
        if name == "checker":                          # (a single row or column has no diagonal neighbours)
            assert got["found"] == (1 if connectivity == 8 and min(R, P) > 1 else (R * P + 1) // 2)
        if name in ("serpentine", "spiral", "full"):
            assert got["found"] == 1 and got["pixels"][0] == mask.sum()
        if name == "empty":
            assert got["found"] == 0


# ---- edge rules ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_equality_is_foreground_and_nan_is_background(dtype):
    below = float(np.nextafter(np.float16(THR), np.float16(0))) if dtype == torch.float16 else float(np.nextafter(np.float32(THR), np.float32(0)))
    pred = np.array([[THR, below, THR, np.nan, THR, 0.0, THR]], dtype=np.float32)
    labels, status = label_gpu(tensor(pred, dtype), THR, 8)
    assert labels.cpu().numpy().tolist() == [[0, -1, 2, -1, 4, -1, 6]] and int(status.item()) == 0


def test_bad_sv_counts_in_pixels_only_and_the_sv_window_is_honoured():
    """sv <= 0, NaN and +-Inf are planted all over (planes_for); sv_ping_off > 0 and data_pings > n_pings."""
    R, P = 37, 70
    sv = planes_for(R, P, n_planes=3, sv_ping_off=11, extra=5)
    mask = ref.pattern("random60", R, P)
    got, want, _ = check_case(mask, torch.float16, 8, sv, channels=(2,), sv_ping_off=11)
    assert (got["sv_pixels"][0] < got["pixels"]).any() and got["sv_pixels"].sum() > 0
    assert np.all(np.isfinite(got["sv_sum"])) and np.all(got["sv_sum"] >= 0)


def test_several_frequencies_have_the_bits_of_the_single_calls_and_two_runs_are_bit_equal():
    R, P = 64, 256
    sv = planes_for(R, P, n_planes=4, sv_ping_off=3, extra=2)
    mask = ref.pattern("random60", R, P)
    sv_t = tensor(sv)
    labels, _ = label_gpu(tensor(np.where(mask, 0.75, 0.25).astype(np.float32), torch.float16), THR, 8)
    singles = [stats_gpu(labels, sv_t, (c,), 3) for c in range(4)]
    for channels in ((2, 0), (3, 1, 0, 2)):
        multi = stats_gpu(labels, sv_t, channels, 3)
        again = stats_gpu(labels, sv_t, channels, 3)
        assert multi["sv_sum"].tobytes() == again["sv_sum"].tobytes()
        for i, c in enumerate(channels):
            assert multi["sv_sum"][i].tobytes() == singles[c]["sv_sum"][0].tobytes()
            assert np.array_equal(multi["sv_pixels"][i], singles[c]["sv_pixels"][0])
        ref.same_schools(multi, ref.detect(mask, sv[list(channels), 3:3 + P], 8))
    assert len({s["sv_sum"].tobytes() for s in singles}) == 4


def test_a_capacity_below_the_count_states_the_count_and_the_rerun_gives_everything():
    R, P = 37, 70
    sv = planes_for(R, P, n_planes=2)
    mask = ref.pattern("random30", R, P)
    want = ref.detect(mask, sv[[1]], 4)
    n = len(want["anchor"])
    assert n > 40
    labels, _ = label_gpu(tensor(np.where(mask, 0.75, 0.25).astype(np.float32), torch.float16), THR, 4)
    short = stats_gpu(labels, tensor(sv), (1,), capacity=40)
    assert short["found"] == n and len(short["anchor"]) == 40
    ref.same_schools(short, {k: (v[..., :40] if k in ("sv_sum", "sv_pixels") else v[:40]) for k, v in want.items()
                             if k in ref.INT_FIELDS + ("sv_sum",)})
    full = stats_gpu(labels, tensor(sv), (1,), capacity=short["found"])
    ref.same_schools(full, want, fields=ref.INT_FIELDS + ("edges",))


@pytest.mark.parametrize("keep_left, keep_right", [(False, False), (True, False), (False, True), (True, True)])
def test_min_pixels_with_kept_edges(keep_left, keep_right):
    R, P = 37, 70
    sv = planes_for(R, P, n_planes=2)
    mask = ref.pattern("random30", R, P)
    got, want, _ = check_case(mask, torch.float16, 8, sv, min_pixels=6, keep_left=keep_left, keep_right=keep_right)
    small = got["pixels"] < 6
    assert small.any() == (keep_left or keep_right) and (~small).any()
    touches = ((got["bbox"][:, 2] == 0) & keep_left) | ((got["bbox"][:, 3] == P) & keep_right)
    assert np.all(touches[small])


def test_bad_arguments_are_refused_before_anything_is_launched():
    pred = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    labels = torch.full((4, 4), -9, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for args, word in (((4, 4, 0.0, 8), "threshold"), ((4, 4, 0.5, 6), "connectivity"), ((65536, 32768, 0.5, 8), "2\\^31")):
        with pytest.raises(hip.HipLibraryError, match=word):
            call("crimac_schools_label", ptr(pred), 0, args[0], args[1], args[2], args[3], ptr(labels), ptr(status))
    torch.cuda.synchronize()
    assert np.all(labels.cpu().numpy() == -9)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stub_pipe():
    return types.SimpleNamespace(model=pkg.UNet_Baseline(3, 4, start_filts=8, precision="f32x6").cuda().eval(),
                                 device=torch.device("cuda"), frequencies=FREQS)


@pytest.fixture(scope="module")
def survey():
    sv, labels, seabed = synth_survey(n_pings=300, n_range=100, seed=5)
    reader = FakeZarrReader(sv, labels, np.clip(seabed, 1, 90))
    return reader, sv


def reference_schools(out, sv, spec, channels):
    """The reference detector on a downloaded float16 prediction [2, R, P]; anchors and pings global, as the flows."""
    res = {}
    for k in spec.classes:
        mask = out[k - 1].astype(np.float32) >= np.float32(spec.thresholds[k - 1])
        w = ref.detect(mask, sv[list(channels)], spec.connectivity, spec.min_pixels)
        w["anchor"] = np.stack([w["anchor"] // mask.shape[1], w["anchor"] % mask.shape[1]], axis=1)
        res[k] = w
    return res


def test_detect_schools_survey_in_three_chunks_equals_one_chunk_and_the_reference(survey, stub_pipe):
    reader, sv = survey
    spec = ti.SchoolSpec(classes=(1, 2), thresholds=(0.5, 0.4), connectivity=8, min_pixels=3, frequency=(120, 38))
    three = ti.detect_schools_survey(reader, stub_pipe, (64, 64), 8, 4, 100, spec, predict_fn=hashed_predict_fn)
    one = ti.detect_schools_survey(reader, stub_pipe, (64, 64), 8, 4, 300, spec, predict_fn=hashed_predict_fn)
    out = np.zeros((2, 100, 300), dtype=np.float16)
    chunks = 0
    for s, e, part in ti.predict_survey(reader, stub_pipe, (64, 64), 8, 4, 100, out_dtype=np.float16, predict_fn=hashed_predict_fn):
        out[:, :, s:e] = part
        chunks += 1
    assert chunks == 3
    want = reference_schools(out, sv, spec, (2, 1))
    for k in (1, 2):
        assert len(want[k]["pixels"]) > 10 and three[k]["class"] == ti.SCHOOL_CLASSES[k] and three[k]["frequencies"] == (120, 38)
        assert (want[k]["bbox"][:, 2] < 100).any() and (want[k]["bbox"][:, 3] > 100).any()        # schools cross the seams
        ref.same_schools(three[k], one[k])
        ref.same_schools(three[k], want[k])
        ref.same_schools(one[k], want[k])
    boxes = ti.schools_to_boxes(three[1])
    assert boxes.dtype == np.int32 and np.array_equal(boxes, want[1]["bbox"])
    assert np.array_equal(ti.schools_to_boxes(three[1], 5) + np.array([5, -5, 5, -5]), boxes)


def test_a_table_that_overflows_is_reduced_again_with_the_stated_count(survey, stub_pipe):
    reader, sv = survey
    big = ti.detect_schools_survey(reader, stub_pipe, (64, 64), 8, 4, 100, ti.SchoolSpec(connectivity=4), predict_fn=hashed_predict_fn)
    tiny = ti.detect_schools_survey(reader, stub_pipe, (64, 64), 8, 4, 100, ti.SchoolSpec(connectivity=4, max_schools=5),
                                    predict_fn=hashed_predict_fn)
    assert len(big[1]["pixels"]) > 15
    ref.same_schools(tiny[1], big[1])
    assert tiny[1]["sv_sum"].tobytes() == big[1]["sv_sum"].tobytes()


def test_detect_schools_echogram_memm_equals_the_reference(stub_pipe):
    sv, labels, seabed = synth_survey(n_pings=150, n_range=90, seed=12)
    eg = FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), np.clip(seabed, 1, 80),
                      frequencies=FREQS)
    spec = ti.SchoolSpec(classes=(2, 1), connectivity=4, frequency=38)
    got = ti.detect_schools_echogram_memm(eg, stub_pipe, (64, 64), 8, 4, spec, predict_fn=hashed_predict_fn)
    out = ti.predict_echogram_memm(eg, stub_pipe, (64, 64), 8, 4, predict_fn=hashed_predict_fn).astype(np.float16)
    want = reference_schools(out, sv, spec, (1,))
    assert list(got) == [2, 1]
    for k in (1, 2):
        assert len(want[k]["pixels"]) > 10 and got[k]["frequencies"] == (38,)
        ref.same_schools(got[k], want[k])


def test_a_wide_chunk_and_an_unbound_spec_are_refused(stub_pipe):
    cp = ti.ChunkPredictor(stub_pipe.model, 16, (64, 64), 8, 4, out_f16=True)
    cp.wide, cp.out = True, None
    with pytest.raises(ValueError, match="wide=True"):
        cp.detect_schools(ti.SchoolSpec().bind(FREQS))
    cp.wide, cp.out = False, torch.zeros((2, 16, 8), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="bind"):
        cp.detect_schools(ti.SchoolSpec())
