"""Schools scored against the annotations, host side: ``merge_school_chunks(index=True)``, ``merge_school_overlaps`` against
the pair table of the whole plane, and the pure helpers on hand-made tables.  No GPU."""
import numpy as np
import pytest

from crimac_classifiers_unet_amd import hip, parallel
from crimac_classifiers_unet_amd import tiled_inference as ti

import school_scores_ref as sref
import schools_ref as ref
from test_schools_cpu import chunked, sv_for, whole


# ---- merging across seams ----------------------------------------------------------------------------------------------------
def two_masks(R, P, fill_a, fill_b, seed):
    """Two planes that overlap a lot and differ a lot: b is a shifted, partly re-drawn copy of a."""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.random((R, P)) < fill_a
    b = np.roll(a, (1, 2), axis=(0, 1)) | (rng.random((R, P)) < fill_b)
    b &= rng.random((R, P)) < 0.9
    return a, b


@pytest.mark.parametrize("cuts", [(40, 41, 97), (64, 128)])
@pytest.mark.parametrize("min_pixels", [1, 4])
def test_the_index_reproduces_the_merge_and_the_default_is_unchanged(cuts, min_pixels):
    mask, _ = two_masks(45, 150, 0.3, 0.1, 3)
    sv = sv_for(45, 150)
    chunks = chunked(mask, sv, cuts, 8, min_pixels, start=1000)
    plain = ti.merge_school_chunks(chunks, 8, min_pixels)
    got = ti.merge_school_chunks(chunks, 8, min_pixels, index=True)
    assert "index" not in plain and set(got) == set(plain) | {"index"}
    for name in plain:
        assert np.array_equal(got[name], plain[name]) if isinstance(plain[name], np.ndarray) else got[name] == plain[name]
    index = got["index"]
    assert len(index) == len(chunks) and all(i.dtype == np.int64 and len(i) == len(c["anchor"]) for i, c in zip(index, chunks))
    K = len(plain["pixels"])
    pixels, sv_sum, dropped = np.zeros(K, np.int64), np.zeros((2, K)), 0
    for c, i in zip(chunks, index):
        np.add.at(pixels, i[i >= 0], c["pixels"][i >= 0])
        for f in range(2):
            np.add.at(sv_sum[f], i[i >= 0], c["sv_sum"][f][i >= 0])
        dropped += int((i < 0).sum())
        assert i.max(initial=-1) < K
    assert np.array_equal(pixels, plain["pixels"]) and sv_sum.tobytes() == plain["sv_sum"].tobytes()
    assert (dropped > 0) == (min_pixels > 1)          # (a seam school that stays small is dropped after the merge only)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("cuts", [(), (75,), (13, 50, 90, 140)], ids=["1", "2", "5"])
@pytest.mark.parametrize("min_pixels", [1, 5])
def test_overlaps_merged_from_chunks_equal_the_whole_plane_pair_table(cuts, connectivity, min_pixels):
    a, b = two_masks(45, 150, 0.45, 0.15, 11)
    sv = sv_for(45, 150)
    ca, cb = chunked(a, sv, cuts, connectivity, min_pixels), chunked(b, sv, cuts, connectivity, min_pixels)
    edges = [0, *cuts, 150]
    ov = [sref.overlap_chunk(x, y, sv[:, s:e], connectivity) for x, y, s, e in zip(ca, cb, edges, edges[1:])]
    ma = ti.merge_school_chunks(ca, connectivity, min_pixels, index=True)
    mb = ti.merge_school_chunks(cb, connectivity, min_pixels, index=True)
    got = ti.merge_school_overlaps(ov, ma["index"], mb["index"])
    wa, wb = ref.detect(a, sv, connectivity, min_pixels), ref.detect(b, sv, connectivity, min_pixels)
    ref.same_schools(ma, whole(a, sv, connectivity, min_pixels))
    want = sref.pair_table(wa, wb, sv)
    assert len(want["pixels"]) > 10
    sref.same_overlaps(got, want)
    assert got["pred"].dtype == got["ann"].dtype == got["pixels"].dtype == np.int64 and got["sv_sum"].shape == (2, len(want["pixels"]))
    order = np.lexsort((got["ann"], got["pred"]))
    assert np.array_equal(order, np.arange(len(order)))
    if cuts:                                          # pairs whose overlap crosses a seam: more chunk rows than pairs
        assert sum(len(c["pixels"]) for c in ov) > len(got["pixels"])
    if min_pixels > 1:
        assert any((c["pred"] < 0).any() or (c["ann"] < 0).any() for c in ov)


def test_sv_sums_are_added_in_chunk_then_anchor_order():
    """Three rows of one pair whose fp64 sum depends on the order: (big + small) + -big ... with positive terms only the
    order still shows in the last bits."""
    vals = [[1.0, 2.0 ** -53, 2.0 ** -53], [2.0 ** -53]]
    ov = [{"pred": np.zeros(len(v), np.int64), "ann": np.zeros(len(v), np.int64), "pixels": np.ones(len(v), np.int64),
           "sv_sum": np.array([v]), "sv_pixels": np.ones((1, len(v)), np.int64)} for v in vals]
    got = ti.merge_school_overlaps(ov, [np.array([0])] * 2, [np.array([0])] * 2)
    want = ((1.0 + 2.0 ** -53) + 2.0 ** -53) + 2.0 ** -53          # = 1.0: every small term is rounded away in this order
    assert got["sv_sum"].tolist() == [[want]] and want == 1.0 and got["pixels"].tolist() == [4]
    with pytest.raises(ValueError, match="per chunk"):
        ti.merge_school_overlaps(ov, [np.array([0])], [np.array([0])] * 2)


# ---- the helpers on hand-made tables -------------------------------------------------------------------------------------------
def hand_score(pred_px, ann_px, pairs, ignored=None, ann_sv=None, ov_sv=None):
    """pairs: (pred, ann, pixels), given sorted by (pred, ann)."""
    p = np.array(pairs, dtype=np.int64).reshape(-1, 3)
    M = len(p)
    return {"predicted": {"pixels": np.array(pred_px, np.int64)},
            "annotated": {"pixels": np.array(ann_px, np.int64),
                          "sv_sum": np.array(ann_sv if ann_sv is not None else [np.ones(len(ann_px))], np.float64)},
            "overlaps": {"pred": p[:, 0], "ann": p[:, 1], "pixels": p[:, 2],
                         "sv_sum": np.array(ov_sv if ov_sv is not None else [np.zeros(M)], np.float64),
                         "sv_pixels": np.zeros((1, M), np.int64)},
            "ignored_pixels": np.array(ignored if ignored is not None else np.zeros(len(pred_px)), np.int64)}


def test_school_iou_is_the_mask_iou_of_every_pair():
    s = hand_score([10, 20], [10, 8, 30], [(0, 0, 10), (1, 1, 4), (1, 2, 15)])
    assert ti.school_iou(s).tolist() == [1.0, 4 / 24, 15 / 35]
    assert ti.school_iou(hand_score([3], [4], [])).shape == (0,)


def test_above_one_half_the_match_is_unique_and_does_not_depend_on_the_order():
    # pred 0 overlaps ann 0 (IoU 0.6) and ann 1 (small); pred 1 overlaps ann 1 with IoU 0.75
    s = hand_score([10, 8], [6, 6], [(0, 0, 6), (0, 1, 1), (1, 1, 6)])
    iou = ti.school_iou(s)
    assert iou.tolist() == [0.6, 1 / 15, 0.75]
    m = ti.match_schools(s, 0.5)
    assert m["pred"].tolist() == [1, 0] and m["ann"].tolist() == [1, 0] and m["iou"].tolist() == [0.75, 0.6]
    per_pred, per_ann = np.bincount(s["overlaps"]["pred"][iou > 0.5]), np.bincount(s["overlaps"]["ann"][iou > 0.5])
    assert per_pred.max() == 1 and per_ann.max() == 1          # (no school has two partners above one half)
    assert ti.match_schools(s, 0.7)["pred"].tolist() == [1] and len(ti.match_schools(s, 0.8)["pred"]) == 0
    assert ti.match_schools(s, 0.6)["pred"].tolist() == [1, 0]                  # (equality is a match)


def test_at_a_low_threshold_ties_are_taken_in_pred_then_ann_order_and_each_school_is_used_once():
    # (0, 0) and (1, 0) tie at 1 / 3: pred 0 comes first and takes ann 0, so pred 1 stays without a partner; (2, 1) is better
    s = hand_score([8, 8, 5], [8, 13], [(0, 0, 4), (0, 1, 4), (1, 0, 4), (1, 1, 4), (2, 1, 5)])
    iou = ti.school_iou(s)
    assert iou.tolist() == [4 / 12, 4 / 17, 4 / 12, 4 / 17, 5 / 13]
    m = ti.match_schools(s, 0.3)
    assert list(zip(m["pred"].tolist(), m["ann"].tolist())) == [(2, 1), (0, 0)]
    assert m["iou"].tolist() == [5 / 13, 4 / 12]
    low = ti.match_schools(s, 0.2)                    # (0, 1), (1, 0) and (1, 1) come later and find a school used
    assert list(zip(low["pred"].tolist(), low["ann"].tolist())) == [(2, 1), (0, 0)]
    assert len(ti.match_schools(s, 0.51)["pred"]) == 0


def test_detection_scores_count_matches_and_leave_ignored_predictions_out():
    # pred 0 matches ann 0; pred 1 lies on ignored ids (6 of 10 pixels); pred 2 partly (5 of 10: not more than half); ann 1 is missed
    s = hand_score([10, 10, 10], [10, 7], [(0, 0, 8), (2, 1, 1)], ignored=[0, 6, 5],
                   ann_sv=[[4.0, 1.0], [0.0, 2.0]], ov_sv=[[3.0, 0.5], [0.0, 1.0]])
    d = ti.school_detection_scores(s)
    assert (d["true_positives"], d["false_positives"], d["false_negatives"], d["excluded"]) == (1, 1, 1, 1)
    assert (d["predicted"], d["annotated"]) == (3, 2)
    assert d["recall"] == 0.5 and d["precision"] == 0.5 and d["f1"] == 0.5
    assert d["sv_recall"].tolist() == [3.5 / 5.0, 0.5]
    assert d["school_sv_recall"][0].tolist() == [0.75, 0.5] and np.isnan(d["school_sv_recall"][1, 0]) and d["school_sv_recall"][1, 1] == 0.5
    assert d["matches"]["pred"].tolist() == [0]
    loose = ti.school_detection_scores(s, max_ignored=0.4)
    assert (loose["false_positives"], loose["excluded"]) == (0, 2) and loose["precision"] == 1.0
    # a matched school is never excluded, however much of it is ignored
    s["ignored_pixels"] = np.array([10, 6, 5])
    assert ti.school_detection_scores(s)["true_positives"] == 1 and ti.school_detection_scores(s)["excluded"] == 1


def test_divisions_by_zero_give_nan():
    none = ti.school_detection_scores(hand_score([], [], [], ann_sv=[[]], ov_sv=[[]]))
    assert none["true_positives"] == 0 and all(np.isnan(none[k]) for k in ("recall", "precision", "f1"))
    assert np.isnan(none["sv_recall"]).all() and none["school_sv_recall"].shape == (1, 0)
    missed = ti.school_detection_scores(hand_score([], [5], []))
    assert missed["recall"] == 0.0 and np.isnan(missed["precision"]) and np.isnan(missed["f1"])
    assert missed["sv_recall"].tolist() == [0.0]
    wrong = ti.school_detection_scores(hand_score([5], [5], []))
    assert wrong["recall"] == 0.0 and wrong["precision"] == 0.0 and np.isnan(wrong["f1"])
    only_ignored = ti.school_detection_scores(hand_score([4], [], [], ignored=[4], ann_sv=[[]], ov_sv=[[]]))
    assert only_ignored["excluded"] == 1 and only_ignored["false_positives"] == 0 and np.isnan(only_ignored["precision"])


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_the_flows_refuse_a_process_group_before_they_read_anything(monkeypatch):
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"read .{name}")
    monkeypatch.setattr(parallel, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="one rank"):
        ti.score_schools_survey(Untouchable(), Untouchable(), (64, 64), 8, 4, 100, ti.SchoolSpec())


def test_the_entries_are_declared_and_the_selector_is_negative():
    assert {"crimac_schools_label_ids", "crimac_schools_label_both", "crimac_schools_pair_anchors"} <= set(hip.SIGNATURES)
    assert hip.DEFINES["CRIMAC_SCHOOLS_IDS_IGNORED"] < 0 and ti.SCHOOLS_IDS_IGNORED == hip.DEFINES["CRIMAC_SCHOOLS_IDS_IGNORED"]
    assert ti.SCHOOL_IDS == sref.CODES
