"""CPU: the host side of the survey-level memm evaluation (tiled_inference.evaluate_echograms_memm): argument checks, the
box-offset table, what an echogram's boxes add to its share of the staging, the callback's optional keyword, and the C ABI
of the four multi-source entry points of the evaluation chain."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti
from tools.fake_reader import FakeEchogram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("crimac_gather_eval_crops_multi", "crimac_labels_test_transform_multi", "crimac_labels_extend_mask_multi",
           "crimac_gather_patches_memm_labels_multi")


def echogram(n_range, n_pings, seabed, name, boxes=None):
    sv = np.zeros((4, n_range, n_pings), dtype=np.float32)
    return FakeEchogram(sv, np.zeros((n_range, n_pings), dtype=np.int16), np.full(n_pings, seabed), name=name, boxes=boxes)


def test_arguments_are_checked_before_anything_is_read():
    pipe = None                                       # (never touched: the checks come first)
    with pytest.raises(TypeError, match=r"'group_patch' \(did you mean 'group_patches'\?\)"):
        ti.evaluate_echograms_memm(iter([]), pipe, (32, 32), 4, 8, group_patch=40)
    for typo in ("group_elem", "seabeds", "stat", "evalmode", "on_batchs", "extend_sizes"):
        with pytest.raises(TypeError, match="evaluate_echograms_memm: unknown keyword"):
            ti.evaluate_echograms_memm(iter([]), pipe, (32, 32), 4, 8, **{typo: None})
    for bad in (np.zeros(10, dtype=np.int64), [np.zeros(10, dtype=np.int64)], "guess"):
        with pytest.raises(TypeError, match="single echogram"):
            ti.evaluate_echograms_memm(iter([]), pipe, (32, 32), 4, 8, seabed=bad)
    with pytest.raises(ValueError, match="eval_mode"):
        ti.evaluate_echograms_memm(iter([]), pipe, (32, 32), 4, 8, eval_mode="schools")
    # the prediction sibling words its refusals as before
    with pytest.raises(TypeError, match=r"predict_echograms_memm: unknown keyword\(s\) 'group_patch' \(did you mean"):
        next(ti.predict_echograms_memm(iter([]), pipe, (32, 32), 4, 8, group_patch=40))


def test_box_table_lays_the_echograms_boxes_one_after_the_other():
    a = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], dtype=np.int64)
    b = np.array([[9, 10, 11, 12]], dtype=np.int32)
    off, rows = ti.memm_box_table([a, None, np.zeros((0, 4), int), b])
    assert off.dtype == rows.dtype == np.int32 and rows.flags.c_contiguous
    assert off.tolist() == [0, 2, 2, 2, 3]
    assert rows.tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]]
    off, rows = ti.memm_box_table([None, None])
    assert off.tolist() == [0, 0, 0] and rows.shape == (0, 4)
    off, rows = ti.memm_box_table([])
    assert off.tolist() == [0] and rows.shape == (0, 4)


def test_boxes_count_towards_an_echograms_share_of_the_staging_on_the_evaluation_side_only():
    many = [(0, 5, i, i + 3) for i in range(4000)]
    eg = echogram(60, 100, 40, "e", boxes=many)
    plain = ti._MemmRecord(eg, eg.get_seabed(0, 100).astype(np.int32), (32, 32), 4)
    for mode in ("all", "region", "trace"):
        r = ti._MemmEvalRecord(eg, eg.get_seabed(0, 100).astype(np.int32), (32, 32), 4, eval_mode=mode, extend_size=7)
        assert np.array_equal(r.grid, plain.grid) and r.pixels == plain.pixels
        if mode == "all":
            assert r.boxes is None and r.elems == plain.elems == 60 * 100
        else:
            assert np.array_equal(r.boxes, ti.eval_boxes(eg, mode, 7)) and r.boxes.shape == (4000, 4)
            assert r.elems >= ti.MEMM_MISC_SHARE * (4 * 4000 + 2) > plain.elems
    # the words of a group -- descriptors, centres, src, seabed lines, box offsets, boxes -- fit the int32 staging
    egs = [echogram(60, 100, 40, f"e{i}", boxes=many[:50 * i]) for i in range(6)]
    cap = 1 << 14
    record = functools.partial(ti._MemmEvalRecord, eval_mode="region")
    groups = list(ti.iter_memm_groups(iter(egs), (32, 32), 4, 10 ** 9, max_elems=cap, record=record))
    assert len(groups) == 4 and [r.echogram.name for g in groups for r in g] == [eg.name for eg in egs]
    for g in groups:
        words = sum(2 * hip.MEMM_DESC_WORDS + 3 * len(r.grid) + r.n_pings + 4 * len(r.boxes) for r in g) + len(g) + 1
        assert words <= cap // ti.MEMM_MISC_SHARE + 2 * hip.MEMM_DESC_WORDS
    # prediction plans the same echograms by their pixels alone
    assert len(list(ti.iter_memm_groups(iter(egs), (32, 32), 4, 10 ** 9, max_elems=cap))) == 3


def test_callback_gets_the_echograms_only_when_it_declares_them():
    assert not ti._takes_keyword(lambda cen, lab, logits: None, "echograms")
    assert ti._takes_keyword(lambda cen, lab, logits, echograms=None: None, "echograms")
    assert ti._takes_keyword(lambda cen, lab, logits, *, echograms: None, "echograms")
    assert ti._takes_keyword(lambda *a, **kw: None, "echograms")
    assert not ti._takes_keyword(lambda *a: None, "echograms")

    class Hook:
        def __call__(self, cen, lab, logits, *, echograms=None):
            pass
    assert ti._takes_keyword(Hook(), "echograms")


def test_header_declares_the_four_entries_and_the_binding_picks_them_up():
    header = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION >= 13
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    for name in ENTRIES:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert proto, f"{name} is not declared in the header"
        args = [a.strip() for a in proto.group(1).split(",")]
        want = [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
        assert args[-1] == "void* stream" and want == hip.SIGNATURES[name], name
        assert "const crimac_memm_desc* descs" in args or name == "crimac_labels_extend_mask_multi"
    assert hip.MEMM_DESC_WORDS == 6                   # the table's layout did not change
    # the library exports them; argument checks precede any HIP call (the pointers are never dereferenced)
    lib = hip.load_library()
    assert lib.crimac_version() == hip.ABI_VERSION
    one, f = ctypes.c_void_p(16), ctypes.c_float
    assert lib.crimac_gather_eval_crops_multi(one, 0, one, 4, one, 1, 32, 32, one, one, None) < 0           # empty table
    assert lib.crimac_gather_eval_crops_multi(one, 1, None, 4, one, 1, 32, 32, one, one, None) < 0          # no src
    assert lib.crimac_gather_patches_memm_labels_multi(9, one, 1, one, 4, one, 1, 32, 32, one, 16, one, None) < 0
    assert b"precision" in lib.crimac_last_error()
    assert lib.crimac_gather_patches_memm_labels_multi(0, one, 1, one, 4, one, 1, 32, 32, one, 16, None, None) < 0
    assert b"transformed labels" in lib.crimac_last_error()
    assert lib.crimac_labels_test_transform_multi(one, 2, one, 3, f(1e-7), f(1e-4), one, None, 1, one, 10, 4, one, 1, 4,
                                                  32, 32, None) < 0                                          # no table
    assert lib.crimac_labels_test_transform_multi(one, 2, one, 3, f(1e-7), f(1e-4), one, one, 1, one, 10, 16, one, 1, 4,
                                                  32, 32, None) < 0                                          # overlap eats the patch
    assert lib.crimac_labels_extend_mask_multi(one, one, 4, one, one, None, 1, one, -1, 1, 32, 32, None) < 0    # no offsets
    assert lib.crimac_labels_extend_mask_multi(one, one, 4, one, one, one, 1, one, -1, 1, 512, 512, None) < 0   # patch too large
