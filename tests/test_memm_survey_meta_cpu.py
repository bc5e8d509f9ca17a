"""CPU: the host side of packing metadata models across echograms (tiled_inference, ``pack_metadata=True``): the C ABI of
the second descriptor table and its two entry points, what an echogram's metadata vectors add to its share of the staging,
the staged table itself, and the argument checks of the two survey flows."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti
from tools.fake_reader import FakeEchogram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("crimac_gather_patches_memm_meta_multi", "crimac_meta_planes_multi")
FREQS = [18, 38, 120, 200]
MC = {k: True for k in ti.META_FLAGS}


def echogram(n_range, n_pings, seabed, name, n_vec=None):
    """``n_vec``: the length of the two time vectors when it is not the echogram's pings."""
    sv = np.zeros((4, n_range, n_pings), dtype=np.float32)
    eg = FakeEchogram(sv, np.zeros((n_range, n_pings), dtype=np.int16), np.full(n_pings, seabed), frequencies=FREQS, name=name)
    n_vec = n_pings if n_vec is None else n_vec
    eg.portion_of_year_scalar = 0.25 + 0.001 * n_pings
    eg.portion_of_day_vector = np.linspace(0.1, 0.9, n_vec)
    eg.time_vector_diff = np.linspace(-1.0, 1.0, n_vec)
    return eg


def test_header_declares_the_metadata_table_and_the_binding_picks_it_up():
    header = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION >= 14
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long}
    for name in ENTRIES:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert proto, f"{name} is not declared in the header"
        args = [a.strip() for a in proto.group(1).split(",")]
        want = [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
        assert args[-1] == "void* stream" and want == hip.SIGNATURES[name], name
        assert "const crimac_memm_meta_desc* metas" in args
    # the descriptor: seven 64-bit fields -- a double, then (pointer, long long) three times; the main header names the
    # type, include/crimac_memm_meta.h lays it out and the binding's mirror is read from there
    assert re.search(r"typedef struct crimac_memm_meta_desc crimac_memm_meta_desc;", code)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crimac_memm_meta.h")).read(), flags=re.S)
    assert hip.MemmMetaDesc._fields_ == hip.parse_header(code)[1]["crimac_memm_meta_desc"]
    body = re.search(r"typedef struct crimac_memm_meta_desc \{(.*?)\} crimac_memm_meta_desc;", code, flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert len(fields) == 7 and fields[0] == "double portion_year"
    assert all("*" in f for f in fields[1::2]) and all(f.startswith("long long n_") for f in fields[2::2])
    assert [n for n, _ in hip.MemmMetaDesc._fields_] == ["portion_year", "portion_day", "n_day", "time_diff", "n_td",
                                                         "seabed", "n_sb"]
    assert all(ctypes.sizeof(t) == 8 for _, t in hip.MemmMetaDesc._fields_)
    assert hip.MEMM_META_WORDS == 7 and ctypes.sizeof(hip.MemmMetaDesc) == 56
    assert hip.MEMM_DESC_WORDS == 6 and ctypes.sizeof(hip.MemmDesc) == 48        # the first table did not change
    # the library exports both; argument checks precede any HIP call (the pointers are never dereferenced)
    lib = hip.load_library()
    assert lib.crimac_version() == hip.ABI_VERSION
    one = ctypes.c_void_p(16)
    gather = lib.crimac_gather_patches_memm_meta_multi
    assert gather(9, one, one, 1, one, 4, one, 1, 32, 32, one, 16, None, 1, 63, None) < 0
    assert b"precision" in lib.crimac_last_error()
    assert gather(0, one, None, 1, one, 4, one, 1, 32, 32, one, 16, None, 1, 63, None) < 0           # no metadata table
    assert gather(0, None, one, 1, one, 4, one, 1, 32, 32, one, 16, None, 1, 63, None) < 0           # no descriptor table
    assert gather(0, one, one, 1, one, 4, one, 1, 32, 32, one, 16, None, 1, 0, None) < 0             # flags: no plane
    assert gather(0, one, one, 1, one, 4, one, 1, 32, 32, one, 16, None, 1, 64, None) < 0            # flags past bit 5
    assert gather(0, one, one, 1, one, 4, one, 1, 32, 32, one, 8, None, 1, 63, None) < 0             # 4 + 7 channels, ld 8
    assert b"do not fit" in lib.crimac_last_error()
    assert gather(0, one, one, 0, one, 4, one, 1, 32, 32, one, 16, None, 1, 63, None) < 0            # empty table
    planes = lib.crimac_meta_planes_multi
    assert planes(None, 1, one, one, 1, 32, 32, 63, one, None) < 0
    assert planes(one, 1, None, one, 1, 32, 32, 63, one, None) < 0
    assert planes(one, 0, one, one, 1, 32, 32, 63, one, None) < 0
    assert planes(one, 1, one, one, 1, 32, 32, 0, one, None) < 0
    assert planes(one, 1, one, one, 1, 32, 32, 64, one, None) < 0


def survey():
    """Seven echograms, two of them slivers (1 and 2 rows x many pings) whose vectors outweigh their pixels."""
    return [echogram(60, 100, 40, "a"), echogram(1, 2000, 0, "sliver"), echogram(60, 40, 30, "b"),
            echogram(2, 1500, 1, "thin"), echogram(90, 150, 70, "c"), echogram(17, 17, 5, "tiny", n_vec=9),
            echogram(60, 100, 40, "d")]


def records(record, **kw):
    """The survey's records; echogram "b" is left without patches (its words still travel with its group)."""
    out = [record(eg, eg.get_seabed(0, eg.shape[1]).astype(np.int32), (32, 32), 4, **kw) for eg in survey()]
    out[2].grid = out[2].grid[:0]
    return out


def test_metadata_words_count_towards_an_echograms_share_of_the_staging():
    eg = echogram(1, 3000, 0, "sliver")
    sb = eg.get_seabed(0, 3000).astype(np.int32)
    plain = ti._MemmRecord(eg, sb, (32, 32), 4)
    r = ti._MemmRecord(eg, sb, (32, 32), 4, meta=True)
    assert plain.meta is None and plain.meta_words == 0
    assert r.meta_words == hip.MEMM_META_WORDS + 3 * 3000
    assert r.elems == max(plain.elems, ti.MEMM_META_SHARE * r.meta_words) > plain.elems > plain.pixels
    py, day, td, seabed = r.meta
    assert py == eg.portion_of_year_scalar and day.dtype == td.dtype == np.float64 and seabed.dtype == np.int64
    assert np.array_equal(day, eg.portion_of_day_vector) and np.array_equal(td, eg.time_vector_diff)
    # the evaluation record takes the same, on top of its boxes
    e = ti._MemmEvalRecord(eg, sb, (32, 32), 4, eval_mode="region", meta=True)
    assert e.meta_words == r.meta_words and e.elems >= r.elems
    # the seabed vector of the planes: the reader's own when the survey's `seabed` is None, else the line that was made
    eg._seabed = np.arange(3000)
    line = np.full(3000, 7, dtype=np.int32)
    assert np.array_equal(ti._MemmRecord(eg, line, (32, 32), 4, meta=True).meta[3], np.arange(3000))
    assert np.array_equal(ti._MemmRecord(eg, line, (32, 32), 4, meta=True, own_seabed=False).meta[3], line)


@pytest.mark.parametrize("record", [ti._MemmRecord, functools.partial(ti._MemmEvalRecord, eval_mode="region")])
def test_every_planned_group_fits_both_stagings(record):
    cap = 1 << 15
    stage = ti._MemmGroupStage(torch.device("cpu"), 4, cap, FREQS, meta=True)
    assert stage.table["meta"] == (cap // ti.MEMM_META_SHARE + hip.MEMM_META_WORDS, torch.float64)
    recs = records(record, meta=True)
    assert len(recs[2].grid) == 0 and recs[1].elems == ti.MEMM_META_SHARE * recs[1].meta_words > 8 * recs[1].pixels
    groups = list(ti.plan_memm_groups(iter(recs), 10 ** 9, cap, key=ti._MemmRecord.key))
    assert [r for g in groups for r in g] == recs and len(groups) >= 3
    assert any(len(r.grid) == 0 for g in groups if len(g) > 1 for r in g)      # the one without patches joined a group
    for g in groups:
        assert g[0].elems <= cap                                               # (nothing here is too large to be staged)
        words64 = sum(r.meta_words for r in g)
        assert words64 == sum(hip.MEMM_META_WORDS + len(r.echogram.portion_of_day_vector) + len(r.echogram.time_vector_diff)
                              + r.n_pings for r in g)
        assert words64 <= stage.n_meta
        assert stage._read_meta(np.zeros(stage.n_meta), 4096, g) == words64    # the write's own guard agrees
        words32 = sum(2 * hip.MEMM_DESC_WORDS + 3 * len(r.grid) + r.n_pings for r in g)
        assert words32 <= stage.n_misc
        assert sum(r.pixels for r in g) <= cap
    # a sliver whose vectors alone exceed the staging is a group of its own: the per-echogram path, nothing staged
    big = echogram(1, 3000, 0, "big")
    r = record(big, big.get_seabed(0, 3000).astype(np.int32), (32, 32), 4, meta=True)
    assert r.pixels < cap < r.elems
    assert [len(g) for g in ti.plan_memm_groups(iter([recs[0], r, recs[2]]), 10 ** 9, cap, key=ti._MemmRecord.key)] == [1, 1, 1]


def test_without_metadata_packing_the_plan_and_the_staging_are_unchanged():
    cap = 1 << 15
    plain = list(ti.iter_memm_groups(iter(survey()), (32, 32), 4, 10 ** 9, max_elems=cap))
    # the plan of the parent commit for this input: every echogram by its pixels, or -- the slivers -- by its int32 words
    flat = [r for g in plain for r in g]
    elems = [max(r.n_range * r.n_pings, ti.MEMM_MISC_SHARE * (2 * hip.MEMM_DESC_WORDS + 3 * len(r.grid) + r.n_pings))
             for r in flat]
    assert elems[0] == 6000 and elems[1] > 8 * 2000 and elems[5] == max(289, 8 * (12 + 3 + 17))
    want = list(ti.plan_memm_groups(list(zip(range(7), elems)), 10 ** 9, cap, key=lambda it: (1, it[1])))
    assert [[r.echogram.name for r in g] for g in plain] == [[survey()[i].name for i, _ in g] for g in want]
    assert [r.elems for r in flat] == elems and all(r.meta is None and r.meta_words == 0 for r in flat)
    assert len(plain) >= 2
    stage = ti._MemmGroupStage(torch.device("cpu"), 4, cap, FREQS)
    assert sorted(stage.table) == ["data", "lab", "misc"] and not stage.meta
    assert stage.table["misc"] == (cap // ti.MEMM_MISC_SHARE + 2 * hip.MEMM_DESC_WORDS, torch.int32)


def test_the_stage_writes_the_table_and_the_vectors_as_64_bit_words():
    egs = [echogram(60, 100, 40, "a"), echogram(17, 17, 5, "tiny", n_vec=9)]
    egs[1]._seabed = np.arange(17) + 3
    recs = [ti._MemmRecord(eg, eg.get_seabed(0, eg.shape[1]).astype(np.int32), (32, 32), 4, meta=True) for eg in egs]
    stage = ti._MemmGroupStage(torch.device("cpu"), 4, 1 << 14, FREQS, meta=True)
    words = np.full(stage.n_meta, np.nan)
    base = 0x7F0000001000
    end = stage._read_meta(words, base, recs)
    M = hip.MEMM_META_WORDS
    assert end == sum(r.meta_words for r in recs) == 2 * M + 3 * 100 + 9 + 9 + 17
    assert np.isnan(words[end:]).all()
    ints = words.view(np.int64)
    at = 2 * M
    for i, (eg, r) in enumerate(zip(egs, recs)):
        d = hip.MemmMetaDesc.from_buffer_copy(words[M * i:M * (i + 1)].tobytes())
        assert d.portion_year == eg.portion_of_year_scalar
        for ptr_, n, src, view in ((d.portion_day, d.n_day, eg.portion_of_day_vector, words),
                                   (d.time_diff, d.n_td, eg.time_vector_diff, words), (d.seabed, d.n_sb, eg._seabed, ints)):
            assert ptr_ == base + 8 * at and n == len(src) and np.array_equal(view[at:at + n], src)
            at += n
    assert at == end
    small = ti._MemmGroupStage(torch.device("cpu"), 4, 64, FREQS, meta=True)
    with pytest.raises(AssertionError, match="staging too small"):
        small._read_meta(np.zeros(small.n_meta), base, recs)


def fake_pipe(lmi, in_channels, meta_channels=0):
    eng = types.SimpleNamespace(lmi=lmi, in_channels=in_channels, meta_channels=meta_channels)
    model = types.SimpleNamespace(infer_engine=eng)
    model.to = lambda dev: model
    model.eval = lambda: model
    return types.SimpleNamespace(model=model, device=torch.device("cpu"), frequencies=FREQS)


def test_the_metadata_arguments_are_checked_before_any_echogram_is_read():
    taken = []

    def source():
        for i in range(3):
            taken.append(i)
            yield echogram(60, 100, 40, f"e{i}")

    def both(pipe, **kw):
        yield lambda: next(ti.predict_echograms_memm(source(), pipe, (32, 32), 4, 8, **kw))
        yield lambda: ti.evaluate_echograms_memm(source(), pipe, (32, 32), 4, 8, **kw)

    early, late = fake_pipe(False, 11), fake_pipe(True, 4, 7)
    for run in both(early, pack_metadata=True):
        with pytest.raises(ValueError, match=r"takes 11 input channels for 4 frequencies \(metadata planes as input "
                                             r"channels\): pass meta_channels"):
            run()
    for run in both(late, pack_metadata=True):
        with pytest.raises(ValueError, match="pass meta_channels"):
            run()
    two = dict(MC, depth_rel=False, depth_abs_seabed=False)                # five planes
    for pipe in (early, late):
        for run in both(pipe, pack_metadata=True, meta_channels=two):
            with pytest.raises(ValueError, match="takes 7 metadata .* meta_channels builds 5"):
                run()
        for run in both(pipe, pack_metadata=True, meta_channels={"portion_year": True}):
            with pytest.raises(ValueError, match="dict of booleans with the keys"):
                run()
    # a near miss of the new keyword is a misspelling, for a model of any kind
    for run in both(None, pack_metadatas=True):
        with pytest.raises(TypeError, match=r"'pack_metadatas' \(did you mean 'pack_metadata'\?\)"):
            run()
    assert taken == []
