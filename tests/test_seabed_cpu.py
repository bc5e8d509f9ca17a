"""CPU: the seabed-estimate fixture (tests/golden/seabed_estimate.npz, written by tools/make_golden_seabed.py from the
reference's own Echogram.get_seabed, data_reader.py:433-507), the host finishing step against it, and the C ABI of the new
entry point."""
import ctypes
import os
import re

import numpy as np
import pytest

from crimac_classifiers_unet_amd import build, hip
from crimac_classifiers_unet_amd import tiled_inference as ti
from tools.make_golden_seabed import EXACT_CASES, REAL_CASE, columns_numpy, decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {tag: shape for tag, shape, _ in EXACT_CASES + [REAL_CASE]}


@pytest.fixture(scope="module")
def fix(golden_dir):
    with np.load(os.path.join(golden_dir, "seabed_estimate.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_loads_and_holds_the_cases_of_the_issue(fix):
    assert list(fix["tags"]) == list(SHAPES)
    assert [SHAPES[t] for t in "abcde"] == [(200, 400, 3), (300, 330, 4), (203, 70, 2), (24, 1, 1), (24, 2, 1)]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "seabed_estimate.npz")) <= 1000000
    for tag, (R, P, F) in SHAPES.items():
        data = decode(fix, tag)
        assert data.shape == (R, P, F) and data.dtype == np.float32
        assert np.isnan(data).any() or np.isinf(data).any()
        assert fix[tag + "/idx"].shape == (F, P) and fix[tag + "/colmax"].shape == (F, P)
        assert fix[tag + "/ref"].shape == (P,)
        if str(fix[tag + "/kind"]) == "exact":          # multiples of 2^-30 below 8: exact fp64 stencil sums in any order
            fin = data[np.isfinite(data)].astype(np.float64)
            assert np.array_equal(fin * 2.0 ** 30, np.rint(fin * 2.0 ** 30)) and fin.max() < 8 and fin.min() >= 0


@pytest.mark.parametrize("tag", list(SHAPES))
def test_finishing_step_reproduces_the_reference_vector(fix, tag):
    """finish_seabed on the per-frequency argmax rows and column maxima == the reference's get_seabed, every ping."""
    runs = []
    got = ti.finish_seabed(fix[tag + "/idx"], fix[tag + "/colmax"], SHAPES[tag][0], runs=runs)
    assert got.dtype == np.dtype(int) and np.array_equal(got, fix[tag + "/ref"])
    want = {"a": {"behind", "front", "mean"}, "b": {"behind", "front", "mean"}, "c": {"behind", "mean"}, "d": set(),
            "e": set(), "real": {"mean"}}[tag]
    assert {r[3] for r in runs} == want
    if tag == "b":          # even F: the median averages two rows; the run at pings 0-1 is never seen, the one to P - 2 is
        assert SHAPES[tag][2] % 2 == 0
        assert not any(i0 < 2 for _, i0, _, _ in runs) and (2, 327, 328, "front") in runs and (0, 2, 3, "behind") in runs


def test_repair_works_per_run_and_keeps_the_reference_quirks():
    """Hand-made lines of 1000 pings (a drop-out ping is below -8 only while drop-outs are rarer than 1 in 65).  Line 0:
    runs at 0-4 (seen from index 2 on: takes the value behind it), 10-12 (mean of the neighbours), 997-999 (reaches the
    end: the value in front).  Line 1: a single ping (mean) and a run that starts at P - 2 (never seen)."""
    P, R = 1000, 1000
    n, a = ti.seabed_rows(R)
    assert (n, a) == (60, 4)
    idx = (np.arange(P, dtype=np.int32) * 7 % 50)[None].repeat(2, 0)
    colmax = np.ones((2, P), dtype=np.float32)
    colmax[0, [0, 1, 2, 3, 4, 10, 11, 12, 997, 998, 999]] = 1e-30
    colmax[1, [998, 999]] = 1e-30
    colmax[1, 500] = 1e-30
    runs = []
    ti.finish_seabed(idx, colmax, R, runs=runs)
    assert runs == [(0, 2, 4, "behind"), (0, 10, 12, "mean"), (0, 997, 999, "front"), (1, 500, 500, "mean")]
    # one frequency alone: its repaired line is the result
    got = ti.finish_seabed(idx[:1], colmax[:1], R)
    raw = idx[0].astype(np.int64) + n - a
    want = raw.astype(np.float64)
    want[2:5] = raw[5]
    want[10:13] = (raw[9] + raw[13]) / 2
    want[997:] = raw[996]
    assert np.array_equal(got, np.rint(want).astype(int))
    assert np.array_equal(got[:2], raw[:2])


def test_restatement_reproduces_the_fixture_columns(fix):
    """columns_numpy (the numpy statement of crimac_seabed_columns the GPU tests compare against) on the decoded inputs ==
    the fixture's per-frequency rows and maxima, in both accumulation orders where the data are exact."""
    for tag in SHAPES:
        data = decode(fix, tag)
        i0, c0 = columns_numpy(data, 0)
        assert np.array_equal(i0, fix[tag + "/idx"]) and np.array_equal(c0, fix[tag + "/colmax"])
        if str(fix[tag + "/kind"]) == "exact":
            assert np.array_equal(columns_numpy(data, 1)[0], i0)


def test_header_binding_and_abi_version_agree_on_the_entry_point():
    header = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()
    m = re.search(r"int crimac_seabed_columns\(([^;]*)\);", header)
    assert m, "crimac_seabed_columns is not declared in the header"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    C = ctypes
    kinds = [C.c_void_p if "*" in a else C.c_long if a.startswith("long ") else C.c_int for a in args]
    assert kinds == hip.SIGNATURES["crimac_seabed_columns"]
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION >= 10
    assert "seabed.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "seabed.hip"))
    lib = hip.load_library()
    assert lib.crimac_version() == hip.ABI_VERSION
    # argument validation needs no GPU: bad row offset, a chunk that owns no ping, a result narrower than the chunk
    p = C.c_void_p(64)
    for bad in ((p, 1, 4, 24, 0, 0, 24, p, p, 4, None), (p, 1, 2, 24, 1, 1, 11, p, p, 4, None),
                (p, 1, 4, 24, 0, 0, 11, p, p, 3, None), (None, 1, 4, 24, 0, 0, 11, p, p, 4, None),
                (p, 1, 4, 24, 2, 0, 11, p, p, 4, None)):
        assert lib.crimac_seabed_columns(*bad) == -22
        assert b"seabed_columns" in lib.crimac_last_error()


def test_seabed_argument_of_the_memm_paths_is_checked():
    with pytest.raises(ValueError, match="estimate"):
        ti._memm_seabed(None, "guess", 10, None, [18])
    with pytest.raises(ValueError, match="integer array"):
        ti._memm_seabed(None, np.zeros(10, dtype=np.float32), 10, None, [18])
    with pytest.raises(ValueError, match="integer array"):
        ti._memm_seabed(None, np.zeros(9, dtype=np.int64), 10, None, [18])
    got = ti._memm_seabed(None, np.arange(10, dtype=np.int64), 10, None, [18])
    assert got.dtype == np.int32 and np.array_equal(got, np.arange(10))
