"""Schools from the predictions, host side: ``SchoolSpec``, ``merge_school_chunks`` against the reference detector on the
whole array, the helpers, the single-rank refusal and the documentation.  No GPU."""
import os

import numpy as np
import pytest

from crimac_classifiers_unet_amd import hip, parallel
from crimac_classifiers_unet_amd import tiled_inference as ti

import schools_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQS = (18, 38, 120, 200)


# ---- SchoolSpec --------------------------------------------------------------------------------------------------------------
def test_the_defaults_are_the_documented_ones():
    s = ti.SchoolSpec()
    assert (s.classes, s.thresholds, s.connectivity, s.min_pixels, s.frequency, s.max_schools) == \
        ((1,), (0.5, 0.5), 8, 1, None, 65536)
    assert s.channels is None


@pytest.mark.parametrize("kwargs, word", [
    (dict(classes=()), "classes"), (dict(classes=(0,)), "classes"), (dict(classes=(1, 1)), "classes"), (dict(classes=(3,)), "classes"),
    (dict(classes=5), "classes"), (dict(classes=(True,)), "classes"),
    (dict(thresholds=(0.5,)), "thresholds"), (dict(thresholds=(0.0, 0.5)), "thresholds"), (dict(thresholds=(0.5, float("inf"))), "thresholds"),
    (dict(thresholds=0.5), "thresholds"), (dict(thresholds=(0.5, float("nan"))), "thresholds"),
    (dict(connectivity=6), "connectivity"), (dict(connectivity=8.0), "connectivity"),
    (dict(min_pixels=0), "min_pixels"), (dict(min_pixels=1.5), "min_pixels"), (dict(min_pixels=True), "min_pixels"),
    (dict(max_schools=0), "max_schools"), (dict(max_schools=2 ** 31), "max_schools"),
    (dict(frequency=()), "frequency"), (dict(frequency=(38, 38.0)), "frequency"), (dict(frequency=tuple(range(1, 10))), "frequencies"),
])
def test_a_bad_argument_is_refused_by_name(kwargs, word):
    with pytest.raises(ValueError, match=word):
        ti.SchoolSpec(**kwargs)


def test_bind_looks_the_channels_up():
    assert ti.SchoolSpec().bind(FREQS).channels == (1,) and ti.SchoolSpec().bind(FREQS).frequency == 38
    assert ti.SchoolSpec().bind((18000, 38000)).channels == (1,) and ti.SchoolSpec().bind((18000, 38000)).frequencies == (38000,)
    b = ti.SchoolSpec(classes=(2, 1), frequency=(200, 18), connectivity=4, min_pixels=3, thresholds=(0.25, 0.75), max_schools=7).bind(FREQS)
    assert b.channels == (3, 0) and b.frequencies == (200, 18)
    assert (b.classes, b.connectivity, b.min_pixels, b.thresholds, b.max_schools) == ((2, 1), 4, 3, (0.25, 0.75), 7)
    assert ti.SchoolSpec(frequency=120).bind(FREQS).channels == (2,)
    assert ti.SchoolSpec(frequency=[120]).bind(FREQS).frequency == (120,)
    with pytest.raises(ValueError, match="frequency 70"):
        ti.SchoolSpec(frequency=(38, 70)).bind(FREQS)
    with pytest.raises(ValueError, match="38 / 38000"):
        ti.SchoolSpec().bind((18, 120))
    assert ti.SCHOOLS_MAX_FREQS == hip.DEFINES["CRIMAC_INTEGRATE_MAX_FREQS"]


# ---- merge_school_chunks -----------------------------------------------------------------------------------------------------
def sv_for(R, P, F=2, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    sv = np.power(10.0, rng.uniform(-7.5, 0.0, size=(F, P, R))).astype(np.float32)
    sv[:, ::7, ::5] = np.nan                       # some pixels that count in `pixels` only
    sv[:, 3::11, 2::3] = 0.0
    return sv


def chunked(mask, sv, cuts, connectivity, min_pixels=1, start=0):
    """The reference detector per chunk, as the survey flow runs the kernels: seam schools kept, min_pixels per chunk."""
    edges = [0, *cuts, mask.shape[1]]
    return [ref.detect(mask[:, a:b], sv[:, a:b], connectivity, min_pixels, keep_left=a > 0, keep_right=b < mask.shape[1],
                       start_ping=start + a, frequencies=(38, 120)) for a, b in zip(edges, edges[1:])]


def whole(mask, sv, connectivity, min_pixels=1, start=0):
    w = ref.detect(mask, sv, connectivity, min_pixels, frequencies=(38, 120))
    P = mask.shape[1]
    w["anchor"] = np.stack([w["anchor"] // P, w["anchor"] % P + start], axis=1)
    w["bbox"] = w["bbox"].astype(np.int64) + np.array([0, 0, start, start])
    w["ping_sum"] = w["ping_sum"] + start * w["pixels"]
    return w


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("fill, cuts", [(0.3, (40, 41, 97)), (0.3, (64, 128)), (0.6, (13, 50, 90, 140)), (0.6, (75, 76))])
def test_random_masks_merged_from_chunks_equal_the_whole_array(fill, cuts, connectivity):
    rng = np.random.Generator(np.random.PCG64(int(fill * 10) + len(cuts)))
    mask = rng.random((45, 150)) < fill
    sv = sv_for(45, 150)
    for min_pixels in (1, 4):
        got = ti.merge_school_chunks(chunked(mask, sv, cuts, connectivity, min_pixels, start=1000), connectivity, min_pixels)
        want = whole(mask, sv, connectivity, min_pixels, start=1000)
        ref.same_schools(got, want)
        assert got["frequencies"] == (38, 120) and got["class"] == "sandeel" and got["sv_sum"].shape == (2, len(want["pixels"]))
        assert got["anchor"].shape == (len(want["pixels"]), 2)
        order = np.lexsort((got["anchor"][:, 1], got["anchor"][:, 0]))
        assert np.array_equal(order, np.arange(len(order)))


def hand(rows):
    return np.array([[c == "#" for c in row] for row in rows])


def test_a_school_that_spans_three_chunks_is_one():
    mask = hand(["............",
                 ".##########.",
                 "............"])
    got = ti.merge_school_chunks(chunked(mask, sv_for(3, 12), (4, 8), 4), 4, 1)
    assert got["pixels"].tolist() == [10] and got["bbox"].tolist() == [[1, 2, 1, 11]] and got["anchor"].tolist() == [[1, 1]]
    ref.same_schools(got, whole(mask, sv_for(3, 12), 4))


def test_two_schools_of_chunk_0_that_join_only_through_chunk_1():
    mask = hand(["#####...",
                 "....#...",
                 "....#...",
                 "....#...",
                 "#####..."])                       # the bottom of the U lies in chunk 1: column 4
    per_chunk = chunked(mask, sv_for(5, 8), (4,), 4)
    assert len(per_chunk[0]["anchor"]) == 2 and len(per_chunk[1]["anchor"]) == 1
    got = ti.merge_school_chunks(per_chunk, 4, 1)
    assert got["pixels"].tolist() == [13] and got["anchor"].tolist() == [[0, 0]]
    ref.same_schools(got, whole(mask, sv_for(5, 8), 4))


def test_a_diagonal_touch_at_a_seam_is_one_school_with_8_and_two_with_4():
    mask = hand(["........",
                 "..##....",
                 "....##..",
                 "........"])
    sv = sv_for(4, 8)
    for connectivity, count in ((8, 1), (4, 2)):
        got = ti.merge_school_chunks(chunked(mask, sv, (4,), connectivity), connectivity, 1)
        assert len(got["pixels"]) == count
        ref.same_schools(got, whole(mask, sv, connectivity))


def test_a_one_pixel_seam_school_is_kept_per_chunk_and_judged_after_the_merge():
    lone = hand(["........",
                 "...#....",
                 "........"])
    joined = hand(["........",
                   "...#####",
                   "........"])
    sv = sv_for(3, 8)
    per_chunk = chunked(lone, sv, (4,), 8, min_pixels=5)
    assert per_chunk[0]["pixels"].tolist() == [1]                                    # kept: it touches the seam
    assert len(ti.merge_school_chunks(per_chunk, 8, 5)["pixels"]) == 0                # dropped after the merge
    per_chunk = chunked(joined, sv, (4,), 8, min_pixels=5)
    assert per_chunk[0]["pixels"].tolist() == [1] and per_chunk[1]["pixels"].tolist() == [4]
    got = ti.merge_school_chunks(per_chunk, 8, 5)
    assert got["pixels"].tolist() == [5]                                             # the merged school reaches 5
    ref.same_schools(got, whole(joined, sv, 8, 5))


def test_chunks_out_of_order_and_a_bad_connectivity_are_refused():
    mask = np.ones((3, 8), bool)
    a, b = chunked(mask, sv_for(3, 8), (4,), 8)
    with pytest.raises(ValueError, match="ping order"):
        ti.merge_school_chunks([b, a], 8, 1)
    with pytest.raises(ValueError, match="connectivity"):
        ti.merge_school_chunks([a, b], 6, 1)


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def test_the_helpers():
    mask = hand(["##......",
                 "##...###",
                 "........"])
    sv = np.full((2, 8, 3), 0.5, np.float32)
    sv[1] = 0.25
    sv[0, 6, 1] = 0.0                               # the second school has no reference sv at one pixel
    res = ti.merge_school_chunks(chunked(mask, sv, (), 8, start=100), 8, 1)
    assert np.array_equal(ti.school_centroids(res), np.array([[0.5, 100.5], [1.0, 106.0]]))
    assert np.array_equal(ti.school_nasc(res, 0.2), 4.0 * np.pi * 1852.0 ** 2 * 0.2 * res["sv_sum"])
    r = ti.school_frequency_response(res)
    assert np.array_equal(r[0], [1.0, 1.0]) and np.array_equal(r[1], [0.5, 0.75])
    assert np.array_equal(ti.school_frequency_response(res, reference=120)[1], [1.0, 1.0])
    with pytest.raises(ValueError, match="reference 70"):
        ti.school_frequency_response(res, reference=70)
    boxes = ti.schools_to_boxes(res)
    assert boxes.dtype == np.int32 and boxes.tolist() == [[0, 2, 100, 102], [1, 2, 105, 108]]
    assert ti.schools_to_boxes(res, extend_size=20).tolist() == [[-20, 22, 80, 122], [-19, 22, 85, 128]]


# ---- one rank only -----------------------------------------------------------------------------------------------------------
def test_more_than_one_rank_is_refused_before_anything_is_read(monkeypatch):
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the reader was asked for {name}")
    monkeypatch.setattr(parallel, "rank_world", lambda: (1, 2))
    with pytest.raises(NotImplementedError, match="one rank"):
        ti.detect_schools_survey(Untouchable(), Untouchable(), (64, 64), 8, 4, 100, ti.SchoolSpec())


# ---- the names are declared and documented -----------------------------------------------------------------------------------
def test_the_entries_are_in_the_header_and_the_flows_in_the_documentation():
    assert {"crimac_schools_label", "crimac_schools_stats"} <= set(hip.SIGNATURES)
    assert hip.DEFINES["CRIMAC_SCHOOLS_MAX_FREQS"] == hip.DEFINES["CRIMAC_INTEGRATE_MAX_FREQS"]
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert "Schools from the predictions" in doc
    for name in ("SchoolSpec", "detect_schools_survey", "detect_schools_echogram_memm", "merge_school_chunks", "school_centroids",
                 "school_nasc", "school_frequency_response", "schools_to_boxes", "crimac_schools_label", "crimac_schools_stats"):
        assert name in doc, name
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "detect_schools_survey" in f.read()
