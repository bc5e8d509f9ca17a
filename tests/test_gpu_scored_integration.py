"""Echo integration scored against the annotations (``crimac_integrate_confusion``, ``ScoredIntegration``): the kernel
against a numpy float64 reference at the smallest shapes where it can go wrong, its softmax against the PR histogram's, and
the evaluation flows (zarr, memm, predictor stub and real network) against a host binning of what ``on_batch`` saw."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_survey_eval import FREQS, make_pipe, stub_predict_fn  # noqa: E402
from tools.fake_reader import FakeEchogram, FakeZarrReader, synth_eval_survey  # noqa: E402

pytestmark = pytest.mark.gpu
FMAX = np.finfo(np.float32).max
GUARD = 64


# ---- the host reference ------------------------------------------------------------------------------------------------
def weights(logits, mode, thr):
    """logits float [..., 3, H, W] -> (w_sandeel, w_other, in_sandeel, in_other): float64 softmax rounded to float16."""
    z = logits.astype(np.float64)
    e = np.exp(z - z.max(axis=-3, keepdims=True))
    p = (e / e.sum(axis=-3, keepdims=True)).astype(np.float16)
    out = []
    for k in (1, 2):
        pk = np.take(p, k, axis=-3)
        if mode == 0:
            w = (pk.astype(np.float32) >= np.float32(thr[k - 1])).astype(np.float64)
        else:
            w = np.where(pk > 0, pk.astype(np.float64), 0.0)
        out.append(w)
    return out[0], out[1], out[0] > 0, out[1] > 0


def bin_reference(logits, sv_of, labels, origins, n_range, ping_bin, range_bin, n_pb, mode, thr, visits=None):
    """acc float64 / cnt int64 [3, 3, n_pb, n_rb] of patches logits [P, 3, ph, pw], labels [P, ph, pw] placed at origins
    [P, 2] = (row, ping); ``sv_of(p, rows, pings, inside)`` -> the sv of patch p's pixels."""
    n_rb = -(-n_range // range_bin)
    acc, cnt = np.zeros((3, 3, n_pb, n_rb)), np.zeros((3, 3, n_pb, n_rb), dtype=np.int64)
    P, _, ph, pw = logits.shape
    w0, w1, in0, in1 = weights(logits, mode, thr)
    for p in range(P):
        gy = origins[p][0] + np.arange(ph)[:, None] + np.zeros((1, pw), dtype=np.int64)
        gx = origins[p][1] + np.arange(pw)[None, :] + np.zeros((ph, 1), dtype=np.int64)
        inside = (gy >= 0) & (gy < n_range) & (gx >= 0) & (gx < n_pb * ping_bin)
        sv = sv_of(p, gy, gx, inside)
        with np.errstate(invalid="ignore"):
            ok = inside & (labels[p] >= 0) & (labels[p] <= 2) & np.isfinite(sv) & (sv > 0) & (sv < FMAX)
        a, pb, rb, s = labels[p][ok], gx[ok] // ping_bin, gy[ok] // range_bin, sv[ok].astype(np.float64)
        for k, (w, m) in enumerate(((w0[p][ok], in0[p][ok]), (w1[p][ok], in1[p][ok]), (np.ones(len(s)), np.ones(len(s), bool)))):
            np.add.at(acc, (a, k, pb, rb), s * w)
            np.add.at(cnt, (a, k, pb, rb), m.astype(np.int64))
        if visits is not None:
            np.add.at(visits, (gx[ok], gy[ok]), 1)
    return acc, cnt


def close(got, ref, rel):
    return bool((np.abs(got - ref) <= rel * ref).all())


# ---- a. the kernel -------------------------------------------------------------------------------------------------------
P_A, PH_A, PW_A, PING_BIN_A, RANGE_BIN_A, N_RANGE_A, N_PB_A = 5, 24, 40, 7, 5, 37, 9
#            straddles    off the top-left  past n_range and the last ping  on cell edges  overlaps 0, 3
ORIGINS_A = [(3, 5), (-10, -13), (20, 40), (10, 14), (12, 21)]


@pytest.fixture(scope="module")
def kernel_case():
    rng = np.random.Generator(np.random.PCG64(5))
    sv = np.power(10.0, rng.uniform(-7, 0, size=(P_A, 2, PH_A, PW_A))).astype(np.float32)
    sv[:, 0] = 777.0                                         # the plane that is NOT asked for
    junk = rng.random((P_A, PH_A, PW_A))
    for lo, v in ((0.00, np.nan), (0.03, np.inf), (0.06, -np.inf), (0.09, 0.0), (0.12, -1e-3), (0.15, FMAX)):
        sv[:, 1][(junk >= lo) & (junk < lo + 0.03)] = v
    labels = rng.choice(np.array([-100, -1, -50, 0, 1, 2], dtype=np.int16), size=(P_A, PH_A, PW_A),
                        p=[0.1, 0.1, 0.1, 0.3, 0.2, 0.2])
    org = np.array(ORIGINS_A, dtype=np.int32)
    for p in (1, 2):                                         # valid labels on the off-grid pixels
        gy, gx = org[p, 0] + np.arange(PH_A)[:, None], org[p, 1] + np.arange(PW_A)[None, :]
        off = (gy < 0) | (gy >= N_RANGE_A) | (gx < 0) | (gx >= N_PB_A * PING_BIN_A)
        assert off.sum() > 100
        labels[p][off] = 1
    logits = rng.choice(np.array([-4.0, 0.0, 4.0], dtype=np.float32), size=(P_A, 3, PH_A, PW_A))
    ref = {mode: bin_reference(logits, lambda p, gy, gx, inside: sv[p, 1], labels, org, N_RANGE_A, PING_BIN_A, RANGE_BIN_A,
                               N_PB_A, mode, (0.5, 0.5)) for mode in (0, 1)}
    dev = {"logits": torch.from_numpy(logits).cuda(), "sv": torch.from_numpy(sv).cuda(),
           "labels": torch.from_numpy(labels).cuda(), "origins": torch.from_numpy(org).cuda()}
    return dev, ref


def guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    buf[GUARD:GUARD + n] = 0
    return buf


def launch_a(dev, mode, acc, cnt, scratch, scratch_bytes):
    from crimac_classifiers_unet_amd.hip import call, ptr
    call("crimac_integrate_confusion", ptr(dev["logits"]), 3, ptr(dev["sv"]), 2, 1, ptr(dev["labels"]), ptr(dev["origins"]),
         P_A, PH_A, PW_A, N_RANGE_A, PING_BIN_A, RANGE_BIN_A, N_PB_A, 0.5, 0.5, mode, ptr(acc, GUARD), ptr(cnt, GUARD),
         ptr(scratch, GUARD), scratch_bytes)


def run_a(dev, mode, launches=1):
    from crimac_classifiers_unet_amd import tiled_inference as ti
    n = 9 * N_PB_A * 8
    words = ti.confusion_scratch_bytes(P_A, PH_A, PW_A, PING_BIN_A, RANGE_BIN_A) // 8
    acc, cnt = guarded(n, torch.float64, -7.0), guarded(n, torch.int64, -7)
    scratch = guarded(words, torch.float64, 12345.0)
    for _ in range(launches):
        launch_a(dev, mode, acc, cnt, scratch, words * 8)
    torch.cuda.synchronize()
    for buf, fill in ((acc, -7.0), (cnt, -7), (scratch, 12345.0)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all()), "a sentinel was overwritten"
    shape = (3, 3, N_PB_A, 8)
    return acc[GUARD:-GUARD].cpu().numpy().reshape(shape), cnt[GUARD:-GUARD].cpu().numpy().reshape(shape)


def test_kernel_threshold_mode_against_float64(kernel_case):
    dev, ref = kernel_case
    acc, cnt = run_a(dev, 0)
    ref_acc, ref_cnt = ref[0]
    assert ref_cnt[:, 2].sum() > 1000 and (ref_cnt[:, 0].sum(axis=(1, 2)) > 0).all() and (ref_cnt[:, 1].sum(axis=(1, 2)) > 0).all()
    assert np.array_equal(cnt, ref_cnt)
    assert close(acc, ref_acc, 1e-12), float(np.abs(acc - ref_acc).max())


def test_kernel_probability_mode_against_float64(kernel_case):
    dev, ref = kernel_case
    acc, cnt = run_a(dev, 1)
    ref_acc, ref_cnt = ref[1]
    assert np.array_equal(cnt, ref_cnt)                      # (every probability of logits in {-4, 0, 4} is > 0)
    assert close(acc, ref_acc, 2.0 ** -10 + 1e-12), float(np.abs(acc - ref_acc).max())
    assert close(acc[:, 2], ref_acc[:, 2], 1e-12)            # the `all` plane carries no weight


def test_kernel_accumulates_and_is_reproducible(kernel_case):
    dev, ref = kernel_case
    acc1, cnt1 = run_a(dev, 1)
    acc2, cnt2 = run_a(dev, 1, launches=2)
    assert np.array_equal(cnt2, 2 * ref[1][1]) and close(acc2, 2 * acc1, 1e-15)
    again, _ = run_a(dev, 1)
    assert np.array_equal(again.view(np.uint64), acc1.view(np.uint64))


def test_crop_origins_are_the_gathers():
    """crimac_eval_crop_origins against the crops crimac_gather_eval_crops cuts: a ramp that encodes (ping, row) comes back
    with pixel (0, 0) holding the origin -- both flavours, a deep and a shallow water column, even and odd patch size."""
    from crimac_classifiers_unet_amd.hip import call, ptr
    for H in (150, 50):
        Wd = 300
        ramp = (np.arange(Wd)[:, None] * 1000 + np.arange(H)[None, :] + 1).astype(np.float32)      # [Wd][H], > 0 inside
        data, lab = torch.from_numpy(ramp[None]).cuda(), torch.zeros((Wd, H), dtype=torch.int16, device="cuda")
        cen = torch.tensor([[H // 2, 150], [40, 100], [H - 3, 200]], dtype=torch.int32, device="cuda")
        for flavour in (0, 1):
            for size in (64, 63):
                raw = torch.empty((3, 1, size, size), device="cuda")
                out_l = torch.empty((3, size, size), dtype=torch.int16, device="cuda")
                org = torch.empty((3, 2), dtype=torch.int32, device="cuda")
                call("crimac_gather_eval_crops", ptr(data), 1, Wd, H, ptr(lab), ptr(cen), 3, size, size, flavour, ptr(raw),
                     ptr(out_l))
                call("crimac_eval_crop_origins", ptr(cen), 3, size, size, H, flavour, ptr(org))
                raw, org = raw.cpu().numpy()[:, 0], org.cpu().numpy()
                for p in range(3):
                    y, x = np.nonzero(raw[p] > 0)
                    v = raw[p][y[0], x[0]] - 1
                    assert (int(v) % 1000 - y[0], int(v) // 1000 - x[0]) == tuple(org[p]), (H, flavour, size, p)


# ---- b. the same arithmetic as the PR histogram ------------------------------------------------------------------------
def test_threshold_selects_the_pixels_the_pr_histogram_counted():
    from crimac_classifiers_unet_amd import hip, tiled_inference as ti
    from crimac_classifiers_unet_amd.hip import call, ptr
    rng = np.random.Generator(np.random.PCG64(11))
    P, S = 3, 32
    logits = torch.from_numpy((2.5 * rng.standard_normal((P, 3, S, S))).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(0, 3, size=(P, S, S)).astype(np.int16)).cuda()
    sv = torch.ones((P, 1, S, S), device="cuda")
    origins = torch.tensor([[0, 0], [0, S], [0, 2 * S]], dtype=torch.int32, device="cuda")
    hist = torch.zeros((3, 2, hip.PR_BINS), dtype=torch.int32, device="cuda")
    call("crimac_pr_histogram_classes", ptr(logits), 3, ptr(labels), 2, P, S, S, 0b110, ptr(hist))
    hist = hist.cpu().numpy().astype(np.int64)
    assert hist[1].sum() == hist[2].sum() == P * S * S and not hist[:, :, hip.PR_BINS - 1].any()
    scratch = torch.empty(ti.confusion_scratch_bytes(P, S, S, 16, 16) // 8, dtype=torch.float64, device="cuda")
    lab = labels.cpu().numpy()
    for t in (2.0 ** -10, float(np.float16(0.01)), float(np.float16(0.1)), 0.25, float(np.float16(1 / 3)), 0.5, 0.75,
              float(np.float16(0.999)), 1.0):
        assert float(np.float16(t)) == t and t >= 2.0 ** -10
        bits = int(np.float16(t).view(np.uint16))
        acc = torch.zeros((3, 3, 6, 2), dtype=torch.float64, device="cuda")
        cnt = torch.zeros((3, 3, 6, 2), dtype=torch.int64, device="cuda")
        call("crimac_integrate_confusion", ptr(logits), 3, ptr(sv), 1, 0, ptr(labels), ptr(origins), P, S, S, S, 16, 16, 6,
             t, t, 0, ptr(acc), ptr(cnt), ptr(scratch), scratch.numel() * 8)
        cnt, acc = cnt.cpu().numpy(), acc.cpu().numpy()
        for c in (1, 2):                                     # class c: plane c - 1, histogram row c
            others = [a for a in range(3) if a != c]
            assert cnt[c, c - 1].sum() == hist[c, 0, bits:].sum(), (t, c)
            assert cnt[others, c - 1].sum() == hist[c, 1, bits:].sum(), (t, c)
        assert [int(cnt[a, 2].sum()) for a in range(3)] == [int((lab == a).sum()) for a in range(3)]
        assert np.array_equal(acc, cnt.astype(np.float64))   # sv = 1: the sums are the counts


# ---- c, d, e. the flows --------------------------------------------------------------------------------------------------
class Batches:
    """on_batch hook: the centres, transformed labels and logits of every batch, on the host."""

    def __init__(self):
        self.cen, self.lab, self.logits = [], [], []

    def __call__(self, centres, labels, logits):
        self.cen.append(np.array(centres))
        self.lab.append(labels.cpu().numpy())
        self.logits.append(logits.float().cpu().numpy())

    def reference(self, sv_pr, spec, size, memm, visits=None):
        """The host binning: the reader's sv [pings, range] indexed GLOBALLY, the hook's labels and logits."""
        cen, lab, logits = np.concatenate(self.cen), np.concatenate(self.lab), np.concatenate(self.logits)
        n_pings, n_range = sv_pr.shape
        cy = np.full(len(cen), n_range // 2) if memm and n_range <= size else cen[:, 0]
        half = (size + 1) // 2 if memm else size // 2          # getGrid / patch_coord_to_data_coord
        origins = np.stack([cy - half + 1, cen[:, 1] - half + 1], axis=1)
        n_pb, _ = spec.bins(n_pings, n_range)

        def sv_of(p, gy, gx, inside):
            # (pings past the survey's end but inside the last ping bin: no data)
            out = np.zeros(gy.shape, dtype=np.float32)
            have = inside & (gx < n_pings)
            out[have] = sv_pr[gx[have], gy[have]]
            return out
        from crimac_classifiers_unet_amd import tiled_inference as ti
        return bin_reference(logits, sv_of, lab, origins, n_range, spec.ping_bin, spec.range_bin, n_pb,
                             ti.IntegrationSpec.MODES.index(spec.mode), spec.thresholds, visits)


SIZE, OVERLAP = 64, 8


@pytest.fixture(scope="module")
def pipe():
    return make_pipe("h3p")


@pytest.fixture(scope="module")
def zarr_survey():
    sv, labels, seabed, boxes = synth_eval_survey(300, 150, 33)
    return sv, FakeZarrReader(sv, labels, seabed, boxes=boxes)


def test_evaluate_survey_zarr(pipe, zarr_survey):
    from crimac_classifiers_unet_amd import tiled_inference as ti
    sv, reader = zarr_survey
    fn = stub_predict_fn(pipe.model.infer_engine)
    spec = ti.IntegrationSpec(ping_bin=37, range_bin=11, frequency=200, thresholds=(0.5, 0.25))     # channel 3 holds +Inf samples
    runs = {}
    for batch in (3, 16):
        s, seen = ti.ScoredIntegration(spec), Batches()
        hist = ti.evaluate_survey(reader, pipe, (SIZE, SIZE), OVERLAP, batch, 128, predict_fn=fn, on_batch=seen, integration=s)
        runs[batch] = (s.result(), hist, seen)
    plain = ti.evaluate_survey(reader, pipe, (SIZE, SIZE), OVERLAP, 16, 128, predict_fn=fn)
    res, hist, seen = runs[16]
    assert np.array_equal(hist[0], plain[0]) and np.array_equal(hist[1], plain[1])       # the return value is unchanged
    assert res["sv_sum"].shape == (3, 3, 9, 14) and res["ping_edges"][-1] == 300 and res["range_edges"][-1] == 150
    visits = np.zeros((300, 150), dtype=np.int64)
    ref_acc, ref_cnt = seen.reference(sv[3], s.spec, SIZE, False, visits)
    assert np.array_equal(res["pixels"], ref_cnt)
    assert close(res["sv_sum"], ref_acc, 1e-12)
    assert (ref_cnt[:, 0].sum(axis=(1, 2)) > 0).all() and (ref_cnt[1:, 1].sum(axis=(1, 2)) > 0).all()
    # every survey pixel with a valid label and a countable sv exactly once
    assert visits.max() == 1 and res["pixels"][:, 2].sum() == visits.sum() > 20000
    with np.errstate(invalid="ignore"):
        countable = np.isfinite(sv[3]) & (sv[3] > 0)
    assert np.isinf(sv[3]).any() and not visits[~countable].any()
    # batch size: other batches, the same pixels, sums that differ by their order only
    small = runs[3][0]
    assert np.array_equal(small["pixels"], res["pixels"]) and close(small["sv_sum"], res["sv_sum"], 1e-12)
    assert np.array_equal(runs[3][1][0], hist[0])
    rc, r = s.recall("sandeel", res)
    assert 0.0 < r <= 1.0 and rc.shape == (9, 14)


@pytest.mark.parametrize("mode", ["all", "region"])
def test_evaluate_echogram_memm_shallow(pipe, mode):
    """n_range 50 < patch 64: the crop's centre row is H / 2; 'region' with one box: the -1 pixels count nowhere."""
    from crimac_classifiers_unet_amd import tiled_inference as ti
    sv, labels, seabed, boxes = synth_eval_survey(200, 50, 34)
    eg = FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), seabed, boxes=boxes[:1])
    fn = stub_predict_fn(pipe.model.infer_engine)
    s, seen = ti.ScoredIntegration(ti.IntegrationSpec(ping_bin=23, range_bin=9, mode="probability")), Batches()
    hist = ti.evaluate_echogram_memm(eg, pipe, (SIZE, SIZE), OVERLAP, 4, eval_mode=mode, predict_fn=fn, on_batch=seen,
                                     integration=s)
    plain = ti.evaluate_echogram_memm(eg, pipe, (SIZE, SIZE), OVERLAP, 4, eval_mode=mode, predict_fn=fn)
    assert np.array_equal(hist[0], plain[0]) and np.array_equal(hist[1], plain[1])
    res = s.result()
    assert s.spec.channel == 1 and res["sv_sum"].shape == (3, 3, 9, 6)
    lab = np.concatenate(seen.lab)
    assert bool((lab == -1).any()) == (mode == "region")
    # (memm: every non-finite sample of the crop is 0, which the pixel rule drops like the reader's NaN)
    ref_acc, ref_cnt = seen.reference(sv[1], s.spec, SIZE, True)
    assert np.array_equal(res["pixels"], ref_cnt) and ref_cnt[:, 2].sum() > (100 if mode == "region" else 5000)
    assert close(res["sv_sum"], ref_acc, 2.0 ** -10 + 1e-12)
    assert close(res["sv_sum"][:, 2], ref_acc[:, 2], 1e-12)


def test_real_network_all_plane_is_the_counted_sv(pipe):
    from crimac_classifiers_unet_amd import tiled_inference as ti
    sv, labels, seabed, boxes = synth_eval_survey(200, 100, 35)
    reader = FakeZarrReader(sv, labels, seabed, boxes=boxes)
    s, seen = ti.ScoredIntegration(ti.IntegrationSpec(ping_bin=50, range_bin=32)), Batches()
    ti.evaluate_survey(reader, pipe, (SIZE, SIZE), OVERLAP, 8, 0, on_batch=seen, integration=s)
    res = s.result()
    assert np.isfinite(res["sv_sum"]).all() and res["sv_sum"].shape == (3, 3, 4, 4)
    ref_acc, ref_cnt = seen.reference(sv[1], s.spec, SIZE, False)
    assert close(res["sv_sum"][:, 2].sum(axis=0), ref_acc[:, 2].sum(axis=0), 1e-12)
    assert np.array_equal(res["pixels"][:, 2], ref_cnt[:, 2]) and ref_cnt[:, 2].sum() > 8000
    assert (res["sv_sum"][:, :2] <= res["sv_sum"][:, 2:] * (1 + 1e-12)).all()
