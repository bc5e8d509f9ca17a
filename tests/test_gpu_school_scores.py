"""Schools scored against the annotations on the GPU: crimac_schools_label_ids / crimac_schools_label_both /
crimac_schools_pair_anchors against the CPU reference (tests/school_scores_ref.py: scipy.ndimage.label on the id rule and on
the intersection, numpy pair counts), exactly, at the shapes and patterns of tests/test_gpu_schools.py, and the scoring
flows end to end.

The sv bound is that of schools_ref.same_schools: with n = sv_pixels of a pair, |gpu - ref| <= n * 2^-52 * ref."""
import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti
from crimac_classifiers_unet_amd.hip import call, ptr
from tools.fake_reader import FakeEchogram, synth_survey

import school_scores_ref as sref
import schools_ref as ref
from test_gpu_schools import (FREQS, hashed_predict_fn, label_gpu, planes_for, stats_gpu, stub_pipe, survey,  # noqa: F401
                              tensor)

pytestmark = pytest.mark.gpu
IGNORED = hip.DEFINES["CRIMAC_SCHOOLS_IDS_IGNORED"]


def label_ids_gpu(ids_t, off, R, P, select, connectivity):
    labels = torch.full((R, P), -9, dtype=torch.int32, device="cuda")
    status = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    call("crimac_schools_label_ids", ptr(ids_t), int(ids_t.shape[0]), off, R, P, select, connectivity, ptr(labels), ptr(status))
    return labels, status


def label_mask_gpu(mask, connectivity):
    """The labels of a boolean plane through the probability entry (the predicted side of a pair)."""
    return label_gpu(tensor(np.where(mask, 0.75, 0.25).astype(np.float32), torch.float16), 0.5, connectivity)[0]


def label_both_gpu(a, b, connectivity):
    R, P = a.shape
    labels = torch.full((R, P), -9, dtype=torch.int32, device="cuda")
    status = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    call("crimac_schools_label_both", ptr(a), ptr(b), R, P, connectivity, ptr(labels), ptr(status))
    return labels, status


def pairs_gpu(table, capacity, a, b):
    """crimac_schools_pair_anchors on the (full-capacity, device) columns a stats_gpu-like call left: int32 [capacity, 2]."""
    pair = torch.full((capacity, 2), -77, dtype=torch.int32, device="cuda")
    anchor = torch.full((capacity,), -5, dtype=torch.int32, device="cuda")
    n = min(table["found"], capacity)
    anchor[:n] = tensor(table["anchor"][:n])
    found = torch.tensor([table["found"]], dtype=torch.int64, device="cuda")
    call("crimac_schools_pair_anchors", ptr(anchor), ptr(found), capacity, ptr(a), ptr(b), ptr(pair))
    got = pair.cpu().numpy()
    assert np.all(got[n:] == -77), "rows from min(found, capacity) on were written"
    return got[:n]


def overlap_rows(table, pair, a_table, b_table):
    """The chunk-local overlap dict of SchoolOverlaps.numpy() from test-side pieces."""
    return {"anchor": table["anchor"], "pixels": table["pixels"], "sv_sum": table["sv_sum"], "sv_pixels": table["sv_pixels"],
            "pred": ti._rows_of_anchors(a_table["anchor"], pair[:, 0]), "ann": ti._rows_of_anchors(b_table["anchor"], pair[:, 1])}


def summed(rows, n_a, n_b):
    return ti.merge_school_overlaps([rows], [np.arange(n_a)], [np.arange(n_b)])


# ---- crimac_schools_label_ids against the reference labelling -------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_label_ids_equals_the_reference_for_every_pattern_and_selector(shape, connectivity):
    R, P = shape
    for name in ref.PATTERNS:
        mask = ref.pattern(name, R, P)
        for code, select in ((27, 27), (1, 1), (None, IGNORED)):
            ids = sref.ids_for(mask, code)                                  # [P, R]: background from {0, 1, 27, 12, 5000, -1}
            rule = sref.ignored_mask(ids.T) if code is None else ids.T == code
            assert np.array_equal(rule, mask)
            want = ref.label(rule, connectivity)
            labels, status = label_ids_gpu(tensor(ids), 0, R, P, select, connectivity)
            assert int(status.item()) == 0
            assert np.array_equal(labels.cpu().numpy(), want), (name, code)


@pytest.mark.parametrize("shape", [(37, 70), (129, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_label_ids_honours_the_ping_window(shape):
    """ids_ping_off > 0 and spare pings on both sides, filled with the selected id: a read outside the window would join."""
    R, P = shape
    off, extra = 5, 3
    for name, code, select in (("random60", 27, 27), ("combs", 1, 1), ("random30", None, IGNORED)):
        mask = ref.pattern(name, R, P)
        wide = np.full((off + P + extra, R), 12 if code is None else code, dtype=np.int16)
        wide[off:off + P] = sref.ids_for(mask, code)
        labels, status = label_ids_gpu(tensor(wide), off, R, P, select, 8)
        assert int(status.item()) == 0 and np.array_equal(labels.cpu().numpy(), ref.label(mask, 8))


# ---- crimac_schools_label_both, the table of the intersection and the pairs -----------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape, pa, pb", [((37, 70), "random60", "combs"), ((129, 257), "random60", "random30"),
                                            ((64, 256), "serpentine", "checker"), ((1, 130), "random60", "full")],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else v)
def test_label_both_gives_the_pair_table(shape, pa, pb, connectivity):
    R, P = shape
    A, B = ref.pattern(pa, R, P), ref.pattern(pb, R, P, seed=3)
    sv = planes_for(R, P, n_planes=2)
    la, lb = label_mask_gpu(A, connectivity), label_ids_gpu(tensor(sref.ids_for(B, 27)), 0, R, P, 27, connectivity)[0]
    both, status = label_both_gpu(la, lb, connectivity)
    wa, wb = ref.detect(A, sv[[1]], connectivity), ref.detect(B, sv[[1]], connectivity)
    assert int(status.item()) == 0
    assert np.array_equal(la.cpu().numpy(), wa["labels"]) and np.array_equal(lb.cpu().numpy(), wb["labels"])
    assert np.array_equal(both.cpu().numpy(), ref.label(A & B, connectivity))
    table = stats_gpu(both, tensor(sv), (1,))
    ref.same_schools(table, ref.detect(A & B, sv[[1]], connectivity))
    pair = pairs_gpu(table, R * P, la, lb)
    # every component lies in ONE pair: all of its pixels carry the anchors the kernel read at its anchor
    comp = both.cpu().numpy()
    inside = comp >= 0
    slot = np.searchsorted(table["anchor"], comp[inside])
    assert np.array_equal(wa["labels"][inside], pair[slot, 0]) and np.array_equal(wb["labels"][inside], pair[slot, 1])
    got = summed(overlap_rows(table, pair, wa, wb), len(wa["anchor"]), len(wb["anchor"]))
    want = sref.pair_table(wa, wb, sv[[1]])
    assert np.array_equal(got["pixels"], want["pixels"])
    sref.same_overlaps(got, want)
    assert len(table["anchor"]) >= len(want["pixels"]) > 0


def test_pairs_of_dropped_schools_translate_to_minus_one():
    R, P, connectivity = 37, 70, 8
    A, B = ref.pattern("random30", R, P), ref.pattern("combs", R, P)
    sv = planes_for(R, P, n_planes=2)
    la, lb = label_mask_gpu(A, connectivity), label_mask_gpu(B, connectivity)
    a_table, b_table = stats_gpu(la, tensor(sv), (0,), min_pixels=6), stats_gpu(lb, tensor(sv), (0,))
    wa, wb = ref.detect(A, sv[[0]], connectivity, min_pixels=6), ref.detect(B, sv[[0]], connectivity)
    ref.same_schools(a_table, wa)
    both, _ = label_both_gpu(la, lb, connectivity)
    table = stats_gpu(both, tensor(sv), (0,))
    rows = overlap_rows(table, pairs_gpu(table, R * P, la, lb), a_table, b_table)
    want = sref.overlap_chunk(wa, wb, sv[[0]], connectivity)
    assert np.array_equal(rows["pred"], want["pred"]) and np.array_equal(rows["ann"], want["ann"])
    assert (rows["pred"] < 0).any() and (rows["pred"] >= 0).any() and (rows["ann"] >= 0).all()
    sref.same_overlaps(summed(rows, len(wa["anchor"]), len(wb["anchor"])), sref.pair_table(wa, wb, sv[[0]]))


def test_an_intersection_table_that_overflows_states_the_count_and_the_rerun_gives_everything():
    R, P, connectivity = 37, 70, 4
    A, B = ref.pattern("random60", R, P), ref.pattern("random60", R, P, seed=9)
    sv = planes_for(R, P, n_planes=2)
    la, lb = label_mask_gpu(A, connectivity), label_mask_gpu(B, connectivity)
    both, _ = label_both_gpu(la, lb, connectivity)
    want = ref.detect(A & B, sv[[1]], connectivity)
    n = len(want["anchor"])
    assert n > 40
    short = stats_gpu(both, tensor(sv), (1,), capacity=40)
    assert short["found"] == n and len(short["anchor"]) == 40
    few = pairs_gpu(short, 40, la, lb)                                      # (rows 40 .. are not read: found > capacity)
    full = stats_gpu(both, tensor(sv), (1,), capacity=short["found"])
    ref.same_schools(full, want)
    pair = pairs_gpu(full, n, la, lb)
    assert np.array_equal(pair[:40], few)
    wa, wb = ref.detect(A, sv[[1]], connectivity), ref.detect(B, sv[[1]], connectivity)
    sref.same_overlaps(summed(overlap_rows(full, pair, wa, wb), len(wa["anchor"]), len(wb["anchor"])), sref.pair_table(wa, wb, sv[[1]]))


def test_two_runs_are_bit_equal_and_several_frequencies_have_the_bits_of_the_single_calls():
    R, P, connectivity = 64, 256, 8
    A, B = ref.pattern("random60", R, P), ref.pattern("random60", R, P, seed=4)
    sv = planes_for(R, P, n_planes=4, sv_ping_off=3, extra=2)
    sv_t = tensor(sv)

    def run(channels):
        la, lb = label_mask_gpu(A, connectivity), label_ids_gpu(tensor(sref.ids_for(B, 1)), 0, R, P, 1, connectivity)[0]
        both, _ = label_both_gpu(la, lb, connectivity)
        table = stats_gpu(both, sv_t, channels, 3)
        table["pair"] = pairs_gpu(table, R * P, la, lb)
        table["labels"] = both.cpu().numpy()
        return table
    singles = [run((c,)) for c in range(4)]
    for channels in ((2, 0), (3, 1, 0, 2)):
        multi, again = run(channels), run(channels)
        for name in multi:
            assert np.asarray(multi[name]).tobytes() == np.asarray(again[name]).tobytes(), name
        for i, c in enumerate(channels):
            assert multi["sv_sum"][i].tobytes() == singles[c]["sv_sum"][0].tobytes()
            assert np.array_equal(multi["sv_pixels"][i], singles[c]["sv_pixels"][0])
            assert np.array_equal(multi["pair"], singles[c]["pair"])
    assert len({s["sv_sum"].tobytes() for s in singles}) == 4


def test_bad_arguments_are_refused_before_anything_is_launched():
    ids = torch.zeros((8, 4), dtype=torch.int16, device="cuda")
    a = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
    labels = torch.full((4, 4), -9, dtype=torch.int32, device="cuda")
    status = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    pair = torch.full((4, 2), -9, dtype=torch.int32, device="cuda")
    found = torch.ones(1, dtype=torch.int64, device="cuda")
    L, S = ptr(labels), ptr(status)
    bad_ids = [((None, 8, 0, 4, 4, 27, 8, L, S), "null pointer"), ((ptr(ids), 8, 0, 4, 4, 27, 8, None, S), "null pointer"),
               ((ptr(ids), 8, 0, 0, 4, 27, 8, L, S), "empty plane"), ((ptr(ids), 8, 0, 4, 0, 27, 8, L, S), "empty plane"),
               ((ptr(ids), 32768, 0, 65536, 32768, 27, 8, L, S), "2\\^31"),
               ((ptr(ids), 8, 5, 4, 4, 27, 8, L, S), "outside the id extent"), ((ptr(ids), 8, -1, 4, 4, 27, 8, L, S), "outside the id extent"),
               ((ptr(ids), 3, 0, 4, 4, 27, 8, L, S), "outside the id extent"),
               ((ptr(ids), 8, 0, 4, 4, 27, 6, L, S), "connectivity=6"), ((ptr(ids), 8, 0, 4, 4, -1, 8, L, S), "select=-1"),
               ((ptr(ids), 8, 0, 4, 4, IGNORED - 1, 8, L, S), "select=")]
    for args, word in bad_ids:
        with pytest.raises(hip.HipLibraryError, match="schools_label_ids.*" + word):
            call("crimac_schools_label_ids", *args)
    bad_both = [((None, ptr(a), 4, 4, 8, L, S), "null pointer"), ((ptr(a), ptr(a), 4, 4, 8, L, None), "null pointer"),
                ((ptr(a), ptr(a), 0, 4, 8, L, S), "empty plane"), ((ptr(a), ptr(a), 65536, 32768, 8, L, S), "2\\^31"),
                ((ptr(a), ptr(a), 4, 4, 5, L, S), "connectivity=5")]
    for args, word in bad_both:
        with pytest.raises(hip.HipLibraryError, match="schools_label_both.*" + word):
            call("crimac_schools_label_both", *args)
    bad_pair = [((None, ptr(found), 4, ptr(a), ptr(a), ptr(pair)), "null pointer"), ((L, ptr(found), 4, ptr(a), ptr(a), None), "null pointer"),
                ((L, None, 4, ptr(a), ptr(a), ptr(pair)), "null pointer"), ((L, ptr(found), 0, ptr(a), ptr(a), ptr(pair)), "capacity=0"),
                ((L, ptr(found), 2 ** 31, ptr(a), ptr(a), ptr(pair)), "capacity=")]
    for args, word in bad_pair:
        with pytest.raises(hip.HipLibraryError, match="schools_pair_anchors.*" + word):
            call("crimac_schools_pair_anchors", *args)
    torch.cuda.synchronize()
    assert np.all(labels.cpu().numpy() == -9) and np.all(pair.cpu().numpy() == -9) and int(status.item()) == 7


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def reference_scores(out, sv, ids, spec, channels):
    """school_scores_ref.score on a downloaded float16 prediction [2, R, P] and the survey's ids [P, R]."""
    return {k: sref.score(out[k - 1].astype(np.float32) >= np.float32(spec.thresholds[k - 1]), ids, k, sv[list(channels)],
                          spec.connectivity, spec.min_pixels, spec.frequencies) for k in spec.classes}


def same_score(got, want):
    for side in ("predicted", "annotated"):
        ref.same_schools(got[side], want[side])
    sref.same_overlaps(got["overlaps"], want["overlaps"])
    assert got["ignored_pixels"].dtype == np.int64 and np.array_equal(got["ignored_pixels"], want["ignored_pixels"])


def test_score_schools_survey_in_three_chunks_equals_one_chunk_the_reference_and_the_detector(survey, stub_pipe):  # noqa: F811
    reader, sv = survey
    assert {27, 1, 12, -1} <= set(np.unique(reader.labels).tolist())
    spec = ti.SchoolSpec(classes=(1, 2), thresholds=(0.5, 0.4), connectivity=8, min_pixels=3, frequency=(120, 38))
    args = (reader, stub_pipe, (64, 64), 8, 4)
    three = ti.score_schools_survey(*args, 100, spec, predict_fn=hashed_predict_fn)
    one = ti.score_schools_survey(*args, 300, spec, predict_fn=hashed_predict_fn)
    tiny = ti.score_schools_survey(*args, 100, ti.SchoolSpec(classes=(1, 2), thresholds=(0.5, 0.4), connectivity=8, min_pixels=3,
                                                             frequency=(120, 38), max_schools=5), predict_fn=hashed_predict_fn)
    detected = ti.detect_schools_survey(*args, 100, spec, predict_fn=hashed_predict_fn)
    out = np.zeros((2, 100, 300), dtype=np.float16)
    for s, e, part in ti.predict_survey(*args, 100, out_dtype=np.float16, predict_fn=hashed_predict_fn):
        out[:, :, s:e] = part
    want = reference_scores(out, sv, reader.labels, spec, (2, 1))
    for k in (1, 2):
        w = want[k]
        assert len(w["overlaps"]["pixels"]) > 5 and len(w["annotated"]["pixels"]) > 3 and w["ignored_pixels"].sum() > 0
        assert (w["annotated"]["bbox"][:, 2] < 100).any() and (w["annotated"]["bbox"][:, 3] > 100).any()
        same_score(three[k], one[k])
        same_score(three[k], w)
        same_score(one[k], w)
        same_score(tiny[k], three[k])                # every table of every chunk overflowed and was reduced again
        for side in ("predicted", "annotated"):
            assert tiny[k][side]["sv_sum"].tobytes() == three[k][side]["sv_sum"].tobytes()
        assert tiny[k]["overlaps"]["sv_sum"].tobytes() == three[k]["overlaps"]["sv_sum"].tobytes()
        assert set(three[k]["predicted"]) == set(detected[k])
        for name, v in detected[k].items():           # field for field, bit for bit
            g = three[k]["predicted"][name]
            assert (g.dtype == v.dtype and g.tobytes() == v.tobytes()) if isinstance(v, np.ndarray) else g == v, name
        assert three[k]["annotated"]["class"] == ti.SCHOOL_CLASSES[k] and three[k]["annotated"]["frequencies"] == (120, 38)
        scores = ti.school_detection_scores(three[k], min_iou=0.1)
        assert scores["predicted"] == len(w["predicted"]["pixels"]) and scores["annotated"] == len(w["annotated"]["pixels"])
        assert scores["sv_recall"].shape == (2,) and np.all(scores["sv_recall"] <= 1.0)
    plain = ti.score_schools_survey(*args, 100, spec, predict_fn=hashed_predict_fn, ignored=False)
    assert not plain[1]["ignored_pixels"].any() and np.array_equal(plain[1]["overlaps"]["pixels"], three[1]["overlaps"]["pixels"])


def test_score_schools_echogram_memm_equals_the_reference(stub_pipe):  # noqa: F811
    sv, labels, seabed = synth_survey(n_pings=150, n_range=90, seed=12)
    eg = FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), np.clip(seabed, 1, 80),
                      frequencies=FREQS)
    spec = ti.SchoolSpec(classes=(2, 1), connectivity=4, frequency=38)
    got = ti.score_schools_echogram_memm(eg, stub_pipe, (64, 64), 8, 4, spec, predict_fn=hashed_predict_fn)
    out = ti.predict_echogram_memm(eg, stub_pipe, (64, 64), 8, 4, predict_fn=hashed_predict_fn).astype(np.float16)
    want = reference_scores(out, sv, labels, spec.bind(FREQS), (1,))
    assert list(got) == [2, 1]
    for k in (1, 2):
        assert len(want[k]["overlaps"]["pixels"]) > 5
        same_score(got[k], want[k])


def test_a_wide_chunk_an_unbound_spec_and_a_chunk_without_labels_are_refused(stub_pipe):  # noqa: F811
    cp = ti.ChunkPredictor(stub_pipe.model, 16, (64, 64), 8, 4, out_f16=True)
    cp.wide, cp.out = True, None
    with pytest.raises(ValueError, match="score_schools.*wide=True"):
        cp.score_schools(ti.SchoolSpec().bind(FREQS))
    cp.wide, cp.out = False, torch.zeros((2, 16, 8), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="score_schools.*bind"):
        cp.score_schools(ti.SchoolSpec())
    cp.load_chunk(np.ones((4, 8, 16), dtype=np.float32), 0, None, None, 0, 8, seabed=np.full(8, 12))
    with pytest.raises(ValueError, match="without labels"):
        cp.score_schools(ti.SchoolSpec().bind(FREQS))
