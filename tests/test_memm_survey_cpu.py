"""CPU: the host side of the survey-level memm prediction (tiled_inference.predict_echograms_memm): the grouping planner, the
rank sharding of groups, the lazy consumption of the echogram iterator, and the C ABI of the two multi-source entry points."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti
from tools.fake_reader import FakeEchogram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def groups_of(counts, group_patches, elems=None, max_elems=None):
    """plan_memm_groups over (index, patches, elems) items -> the groups as lists of indices."""
    elems = [0] * len(counts) if elems is None else elems
    items = list(zip(range(len(counts)), counts, elems))
    return [[it[0] for it in g] for g in ti.plan_memm_groups(items, group_patches, max_elems, key=lambda it: it[1:])]


def test_planner_empty_input_and_zero_patches():
    assert groups_of([], 10) == []
    assert groups_of([0], 10) == [[0]]                       # an echogram without patches is still handed out
    assert groups_of([4, 0, 6, 0], 10) == [[0, 1, 2], [3]]   # it joins the open group; a trailing one forms the last
    with pytest.raises(ValueError):
        list(ti.plan_memm_groups([(1, 0)], 0))


def test_planner_closes_a_group_when_its_patches_reach_the_threshold():
    assert groups_of([3, 3, 4, 5, 5, 1], 10) == [[0, 1, 2], [3, 4], [5]]          # exact fills
    assert groups_of([10, 10], 10) == [[0], [1]]
    assert groups_of([7, 7, 7, 7], 10) == [[0, 1], [2, 3]]                        # crossed inside an echogram's run
    assert groups_of([1] * 7, 3) == [[0, 1, 2], [3, 4, 5], [6]]
    # one echogram larger than group_patches is a group of its own, wherever it stands
    assert groups_of([25], 10) == [[0]]
    assert groups_of([2, 25, 2, 2], 10) == [[0], [1], [2, 3]]
    assert groups_of([25, 30], 10) == [[0], [1]]


def test_planner_respects_the_element_bound():
    # 100 elements fit: the third echogram would overflow the open group; the fourth is larger than the bound on its own
    assert groups_of([1, 1, 1, 1, 1], 10, elems=[40, 50, 30, 500, 20], max_elems=100) == [[0, 1], [2], [3], [4]]
    assert groups_of([1, 1], 10, elems=[60, 40], max_elems=100) == [[0, 1]]        # an exact fill of the bound
    for g in ti.plan_memm_groups([(1, e) for e in (30, 30, 30, 30, 30, 90, 5)], 100, 100):
        assert sum(e for _, e in g) <= 100


def test_planner_keeps_every_item_once_and_in_order():
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(20):
        counts = [int(c) for c in rng.integers(0, 40, size=int(rng.integers(1, 30)))]
        gp = int(rng.integers(1, 60))
        groups = groups_of(counts, gp)
        assert [i for g in groups for i in g] == list(range(len(counts)))
        for g, nxt in zip(groups[:-1], groups[1:]):
            # closed by reaching the threshold -- or by an echogram that is a group of its own -- and not before
            assert sum(counts[i] for i in g) >= gp or counts[nxt[0]] >= gp
            assert sum(counts[i] for i in g[:-1]) < gp


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_rank_sharding_is_disjoint_complete_and_order_preserving(world):
    groups = groups_of([5, 6, 1, 1, 9, 12, 3, 3, 3, 2, 30, 1], 10)
    assert len(groups) >= 5
    shares = [list(ti.shard_memm_groups(iter(groups), r, world)) for r in range(world)]
    flat = [tuple(g) for s in shares for g in s]
    assert len(flat) == len(set(flat)) == len(groups)                               # disjoint and complete
    for r, s in enumerate(shares):
        assert s == groups[r::world]                                                # round-robin, input order kept
        idx = [i for g in s for i in g]
        assert idx == sorted(idx)
    with pytest.raises(ValueError):
        ti.shard_memm_groups(iter(groups), world, world)


def echogram(n_range, n_pings, seabed_row, name):
    sv = np.full((4, n_range, n_pings), 1e-5, dtype=np.float32)
    return FakeEchogram(sv, np.zeros((n_range, n_pings), dtype=np.int16), np.full(n_pings, seabed_row), name=name)


def test_groups_are_planned_lazily_from_an_iterator_of_echograms():
    """The host half of the generator (iter_memm_groups: seabed line, grid, grouping, sharding) takes echograms from the
    iterator only as far as the group it hands out needs them.  Only this half runs without a device: the generator itself
    and the chunk feed's lazy ``__iter__`` (which predict_survey and evaluate_survey run through too) need pinned memory and
    streams, and their laziness is checked in tests/test_gpu_memm_survey.py."""
    taken = []

    def source():
        for i in range(50):
            taken.append(i)
            yield echogram(60, 100, 40, f"e{i}")
    one = len(ti.plan_eval_grid(60, np.full(100, 40), 100, (32, 32), 4, memm=True))
    assert one == 15                                                                # 3 rows x 5 columns of stride 24
    groups = ti.iter_memm_groups(source(), (32, 32), 4, group_patches=2 * one + 1)
    first = next(groups)
    assert [r.echogram.name for r in first] == ["e0", "e1", "e2"] and taken == [0, 1, 2]
    assert all(len(r.grid) == one and r.seabed.dtype == np.int32 and r.seabed.shape == (100,) for r in first)
    assert np.array_equal(first[0].grid, ti.plan_eval_grid(60, np.full(100, 40), 100, (32, 32), 4, memm=True))
    second = next(groups)
    assert [r.echogram.name for r in second] == ["e3", "e4", "e5"] and taken == list(range(6))
    # a rank of a world of 2 skips the other rank's groups, and still reads no further than its own group
    taken.clear()
    mine = ti.iter_memm_groups(source(), (32, 32), 4, group_patches=2 * one + 1, rank=1, world=2)
    assert [r.echogram.name for r in next(mine)] == ["e3", "e4", "e5"] and taken == list(range(6))
    rest = list(mine)
    assert [r.echogram.name for r in rest[0]] == ["e9", "e10", "e11"] and len(taken) == 50


def test_ranks_that_see_different_files_still_cover_the_survey_exactly_once():
    """save_predictions_memm(resume=True) with several ranks: every rank asks the file system which echograms exist while
    the others write, so the ranks' skip sets differ.  The groups and their owners are planned over the whole input and the
    skip rule is applied to a rank's own echograms afterwards: every echogram is computed by its owner or skipped BY ITS
    OWNER, never twice and never by nobody."""
    names = [f"e{i}" for i in range(23)]
    sizes = [(60, 100), (60, 40), (90, 150)]

    def survey():
        return (echogram(*sizes[i % 3], 40, n) for i, n in enumerate(names))

    def shares(world, skips):
        return [[r.echogram.name for g in ti.iter_memm_groups(survey(), (32, 32), 4, 30, rank=r, world=world,
                                                                skip=None if skips is None else
                                                                (lambda eg, r=r: eg.name in skips[r])) for r in g]
                for r in range(world)]
    for world in (2, 3):
        owner = {n: r for r, share in enumerate(shares(world, None)) for n in share}
        assert sorted(owner) == sorted(names) and len(set(owner.values())) == world
        # rank 0 started late and finds the files of the others' first groups; rank 1 sees two of rank 0's; rank 2 none
        skips = [{n for n in names[:12] if owner[n] != 0} | {"e0", "e5"}, {"e1", "e2", "e20"}, set()][:world]
        got = shares(world, skips)
        flat = [n for share in got for n in share]
        assert len(flat) == len(set(flat))                                          # disjoint
        for r, share in enumerate(got):
            assert share == [n for n in names if owner[n] == r and n not in skips[r]]      # its own, in order, minus ITS skips
        skipped_by_owner = {n for n in names if n in skips[owner[n]]}
        assert set(flat) | skipped_by_owner == set(names) and not set(flat) & skipped_by_owner      # complete
    # a group of which nothing is left is dropped, not handed out empty
    assert list(ti.iter_memm_groups(survey(), (32, 32), 4, 30, skip=lambda eg: True)) == []


def ordered_run(kinds, ticket=True):
    """_ordered_groups over fake groups ("packed" / "solo" by position k) -> (the event log, the yielded items)."""
    log = []

    def fake(k, kind):
        if kind == "solo":
            return types.SimpleNamespace(k=k, offs=None, group=[types.SimpleNamespace(echogram=k)], solo=("sb", "meta"))
        return types.SimpleNamespace(k=k, offs=[0], group=[types.SimpleNamespace(echogram=k)])

    def single(echogram, seabed, meta_channels):
        assert (seabed, meta_channels) == ("sb", "meta")
        log.append(("single", echogram))
        return "single", echogram

    def enqueue(g):
        log.append(("enqueue", g.k))
        return g.k if ticket else None

    def take(k):
        log.append(("take", k))
        yield "take", k
    return log, list(ti._ordered_groups((fake(k, kind) for k, kind in enumerate(kinds)), single, enqueue, take))


def test_the_ordered_group_loop_overlaps_downloads_and_keeps_input_order():
    """The one ordering rule of the memm survey flows: group k's download is awaited (take) only after group k + 1 has
    been enqueued, a solo echogram runs in its place -- after the ticket that is kept -- and the last ticket is taken at
    the end; the results come out in that take / single order."""
    log, items = ordered_run(["packed", "packed", "solo", "packed", "packed"])
    assert log == [("enqueue", 0), ("enqueue", 1), ("take", 0), ("take", 1), ("single", 2), ("enqueue", 3), ("enqueue", 4),
                   ("take", 3), ("take", 4)]
    assert items == [("take", 0), ("take", 1), ("single", 2), ("take", 3), ("take", 4)]
    # the loop is lazy: a group is enqueued only when the consumer asks for more
    seen = []
    gen = ti._ordered_groups(iter([types.SimpleNamespace(k=0, offs=[0]), types.SimpleNamespace(k=1, offs=[0])]),
                             None, lambda g: seen.append(g.k) or g.k, lambda k: [k])
    assert seen == [] and next(gen) == 0 and seen == [0, 1]


def test_the_ordered_group_loop_never_takes_when_nothing_comes_back():
    log, items = ordered_run(["packed", "packed", "solo", "packed"], ticket=False)
    assert log == [("enqueue", 0), ("enqueue", 1), ("single", 2), ("enqueue", 3)] and items == [("single", 2)]


def test_the_ordered_group_loop_of_an_empty_plan_calls_nothing():
    assert ordered_run([]) == ([], [])


def test_the_ordered_group_loop_of_solo_groups_only_neither_enqueues_nor_takes():
    log, items = ordered_run(["solo", "solo", "solo"])
    assert log == items == [("single", 0), ("single", 1), ("single", 2)]


def test_a_misspelt_knob_is_refused_and_config_keys_are_ignored():
    for bad in ("group_patch", "group_elem", "seabeds", "stat"):
        with pytest.raises(TypeError, match=bad):
            next(ti.predict_echograms_memm(iter([]), None, (32, 32), 4, 8, **{bad: 1}))
    with pytest.raises(AttributeError):               # num_workers, data_mode ...: ignored, the call goes on to the model
        next(ti.predict_echograms_memm(iter([]), None, (32, 32), 4, 8, num_workers=4, data_mode="memm"))


def test_each_echogram_keeps_its_own_grid():
    """The grid of an echogram is plan_eval_grid(..., memm=True) with its own seabed: the deepest seabed of one echogram does
    not extend its neighbour's, and a water column not deeper than the patch gets the centre-row adjustment."""
    egs = [echogram(200, 64, 20, "shallow"), echogram(200, 64, 150, "deep"), echogram(17, 17, 5, "tiny")]
    (group,) = list(ti.iter_memm_groups(iter(egs), (32, 32), 4, group_patches=1000))
    for r, eg in zip(group, egs):
        want = ti.plan_eval_grid(eg.shape[0], eg._seabed, eg.shape[1], (32, 32), 4, memm=True)
        assert np.array_equal(r.grid, want)
    assert len(group[0].grid) < len(group[1].grid)
    assert (group[2].grid[:, 0] == 17 // 2).all()


def test_seabed_argument_is_checked_before_anything_is_read():
    pipe = None                                       # (never touched: the check comes first)
    for bad in (np.zeros(10, dtype=np.int64), [np.zeros(10, dtype=np.int64)], "guess"):
        with pytest.raises(TypeError, match="single echogram"):
            next(ti.predict_echograms_memm(iter([]), pipe, (32, 32), 4, 8, seabed=bad))
    with pytest.raises(ValueError, match="integer array"):
        next(ti.iter_memm_groups(iter([echogram(60, 100, 40, "e")]), (32, 32), 4, 10, seabed=lambda eg: np.zeros(3, int)))
    (g,) = list(ti.iter_memm_groups(iter([echogram(60, 100, 40, "e")]), (32, 32), 4, 10,
                                    seabed=lambda eg: np.full(eg.shape[1], 7)))
    assert (g[0].seabed == 7).all()


def test_header_binding_and_abi_number_agree_for_the_multi_source_entries():
    header = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION >= 11
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long}
    for name in ("crimac_gather_patches_memm_multi", "crimac_scatter_patches_multi"):
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert proto, f"{name} is not declared in the header"
        args = [a.strip() for a in proto.group(1).split(",")]
        want = [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
        assert args[-1] == "void* stream" and want == hip.SIGNATURES[name], name
    # the descriptor: six 64-bit fields, written by the host as int64 words
    body = re.search(r"typedef struct crimac_memm_desc \{(.*?)\} crimac_memm_desc;", code, flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert len(fields) == 5 and fields[-1].startswith("long long") and fields[-1].count(",") == 1
    assert all("*" in f for f in fields[:4])
    assert hip.MEMM_DESC_WORDS == 6
    # the library exports both and refuses an unknown precision with the code of the single-source kernels
    lib = hip.load_library()
    assert lib.crimac_version() == hip.ABI_VERSION
    one = ctypes.c_void_p(16)                         # (argument checks precede any HIP call: never dereferenced)
    rc_multi = lib.crimac_gather_patches_memm_multi(9, one, 1, one, 4, one, 1, 32, 32, one, 16, None)
    rc_single = lib.crimac_gather_patches_memm(9, one, 4, 10, 10, one, 1, 32, 32, one, 16, one, None)
    assert rc_multi == rc_single < 0
    assert lib.crimac_gather_patches_memm_multi(-1, one, 1, one, 4, one, 1, 32, 32, one, 16, None) == rc_single
    assert b"precision" in lib.crimac_last_error()
    assert lib.crimac_gather_patches_memm_multi(0, None, 1, one, 4, one, 1, 32, 32, one, 16, None) < 0
    assert lib.crimac_gather_patches_memm_multi(0, one, 1, one, 17, one, 1, 32, 32, one, 16, None) < 0
    assert lib.crimac_scatter_patches_multi(one, 2, one, 1, one, one, 1, 32, 32, 4, 10, 1, None) < 0     # ncls < 3
    assert lib.crimac_scatter_patches_multi(one, 3, one, 1, one, one, 1, 32, 32, 16, 10, 1, None) < 0    # overlap eats the patch
    assert lib.crimac_scatter_patches_multi(one, 3, one, 0, one, one, 1, 32, 32, 4, 10, 1, None) < 0     # empty table
