"""CPU: the operands and the numpy reference of tests/test_gpu_integrate_exact.py, checked here without a GPU.

The GPU module compares ``crimac_integrate_classes`` / ``_layers`` / ``_edges`` / ``_freqs`` with ``reference`` below by
``np.array_equal``, sums included.  That is only fair if every sum is exact in fp64 WHATEVER its order, which the operands
guarantee: a good sv sample is k * 2^-8 with 1 <= k <= 255, a probability-mode weight is 2^-1 .. 2^-4 (threshold mode: 1),
so a term is a multiple of 2^-12 below 1 with at most 12 significant bits; a cell has fewer than 2^14 pixels, so every
partial sum is a multiple of 2^-12 below 2^14: 26 bits, far inside the 53 of a double.  No addition rounds, in the kernel's
order or in numpy's.

Checked here for every case the GPU module runs: the reference has a non-empty cell in each of its three planes (sandeel,
other, all counted pixels), its sums equal ``math.fsum`` of the same terms cell by cell, and it agrees with ``edges_numpy``
(tests/test_integrate_edsu_cpu.py, itself checked against a per-pixel loop there)."""
import functools
import itertools
import math

import numpy as np
import pytest

from test_integrate_edsu_cpu import edges_numpy, new_host

MODES = ("threshold", "probability")
THR = (0.5, 0.25)
# float16 values: both thresholds, their float16 neighbours on either side, and the ends
LEVELS = np.array([0, 0.2498779296875, 0.25, 0.250244140625, 0.499755859375, 0.5, 0.50048828125, 1.0], dtype=np.float16)
WEIGHTS = np.array([0, 0.5, 0.25, 0.125, 0.0625], dtype=np.float16)
SHAPES = {"4-byte": (70, 150), "16-byte": (72, 152)}            # n_range, n_pings
N_PLANES = 8
ORIGIN = 2            # the global ping of pred's column 0: cells start 2 columns off the 4-column grid
SEAM = 100            # the launches are columns [0, 100) and [100, P): they meet at global ping 102, inside ping bin 1
SV_OFF = 37
PING_BIN, RANGE_BIN = 100, 50                                    # a cell: 2 tiles along the pings, 2 splits
GRIDS = {"uniform": None, "table": (5, 5, 47, 130, 131, 150)}    # pings 2 .. 4 and 150 .. 153 in no cell, a cell of width 0
# offset, reference, layers, range_bin.  "low layers": 20 rows each, so that all three hold pixels of most pings
SEABEDS = {"none": None, "limited": (-3, "surface", 0, RANGE_BIN), "3 layers": (-3, "seabed", 3, RANGE_BIN),
           "3 low layers": (-3, "seabed", 3, 20)}


def launches(n_pings):
    return ((0, SEAM), (SEAM, n_pings))


def seabed_line(n_pings, n_range):
    """A sawtooth of 5 rows per ping between row 10 and n_range + 29: 90 rows of relief inside a ping bin, above either
    range_bin; ping 7 has limit 0 after the offset, ping 40 (and the teeth's tips) n_range."""
    line = 10 + (5 * np.arange(n_pings)) % (n_range + 20)
    line[7] = -7
    line[40] = n_range + 11
    return line.astype(np.int32)


@functools.lru_cache(maxsize=None)
def operands(shape, mode):
    """pred float32 [2, R, P] of float16 values, planes float32 [N_PLANES, data_pings, R]; both read-only."""
    R, P = SHAPES[shape]
    rng = np.random.Generator(np.random.PCG64(1000 * R + MODES.index(mode)))
    if mode == "threshold":
        pred = LEVELS[rng.integers(0, len(LEVELS), size=(2, R, P))].astype(np.float32)
    else:
        pred = WEIGHTS[rng.integers(0, len(WEIGHTS), size=(2, R, P))].astype(np.float32)
        hit = rng.random(pred.shape) < 0.01
        pred[hit] = rng.choice(np.array([np.nan, -0.5], dtype=np.float32), size=int(hit.sum()))
    planes = (rng.integers(1, 256, size=(N_PLANES, SV_OFF + P + 9, R)) * 2.0 ** -8).astype(np.float32)
    hit = rng.random(planes.shape) < 0.05
    planes[hit] = rng.choice(np.array([0.0, -2.0 ** -8, np.nan, np.inf], dtype=np.float32), size=int(hit.sum()))
    stored = pred.astype(np.float16).astype(np.float32)
    assert np.array_equal(stored, pred, equal_nan=True)
    pred.setflags(write=False)
    planes.setflags(write=False)
    return pred, planes


def geometry(shape, grid, seabed):
    """(edge table over global pings, n_pb, n_cols, range_bin) of a case."""
    R, P = SHAPES[shape]
    n_pb = -(-(ORIGIN + P) // PING_BIN)
    table = np.arange(n_pb + 1) * PING_BIN if GRIDS[grid] is None else np.array(GRIDS[grid])
    sb = SEABEDS[seabed]
    range_bin = sb[3] if sb else RANGE_BIN
    n_cols = sb[2] if sb and sb[1] == "seabed" else -(-R // range_bin)
    return table, len(table) - 1, n_cols, range_bin


def launch_terms(pred, sv, mode, table, range_bin, n_cols, origin, line, sb):
    """The counted pixels of one launch, per plane: (cell index [n], term float64 [n]).  ``pred`` [2, R, P], ``sv`` [P, R]."""
    R, P = pred.shape[1:]
    s = sv.T
    g = origin + np.arange(P)
    pb = np.searchsorted(table, g, "right") - 1
    L = np.full(P, R) if sb is None else np.clip(line.astype(np.int64) + sb[0], 0, R)
    r = np.arange(R)[:, None]
    ok = ((g >= table[0]) & (g < table[-1]))[None, :] & (r < L[None, :]) & np.isfinite(s) & (s > 0)
    if sb is not None and sb[1] == "seabed":
        col = (L[None, :] - 1 - r) // range_bin
        ok &= col < n_cols
    else:
        col = np.broadcast_to(r // range_bin, (R, P))
    cell = np.broadcast_to(pb[None, :], (R, P)) * n_cols + col
    s64 = np.where(ok, s, 0).astype(np.float64)
    if mode == "threshold":
        member = pred >= np.asarray(THR, dtype=np.float32)[:, None, None]
        weight = np.ones(pred.shape)
    else:
        member = pred > 0                                        # (a NaN or negative weight selects nothing)
        weight = np.where(member, pred, 0).astype(np.float64)
    return [(cell[ok & member[k]], (s64 * weight[k])[ok & member[k]]) for k in (0, 1)] + [(cell[ok], s64[ok])]


@functools.lru_cache(maxsize=None)
def reference(shape, mode, grid, seabed, channel, exact=False):
    """(sums float64, counts int64) [3, n_pb, n_cols] of both launches on plane ``channel``; read-only, computed once.
    ``exact``: every cell's sum by ``math.fsum`` over all its terms instead of ``np.bincount`` launch by launch."""
    R, P = SHAPES[shape]
    pred, planes = operands(shape, mode)
    table, n_pb, n_cols, range_bin = geometry(shape, grid, seabed)
    line = seabed_line(P, R)
    size = n_pb * n_cols
    sums, counts = np.zeros((3, size)), np.zeros((3, size), dtype=np.int64)
    kept = [[], [], []]
    for p0, p1 in launches(P):
        sv = planes[channel, SV_OFF + p0:SV_OFF + p1]
        for k, (cell, terms) in enumerate(launch_terms(pred[:, :, p0:p1], sv, mode, table, range_bin, n_cols, ORIGIN + p0,
                                                        line[p0:p1], SEABEDS[seabed])):
            counts[k] += np.bincount(cell, minlength=size)
            sums[k] += np.bincount(cell, weights=terms, minlength=size)
            kept[k].append((cell, terms))
    if exact:
        for k in range(3):
            cell, terms = (np.concatenate(x) for x in zip(*kept[k]))
            sums[k] = [math.fsum(terms[cell == c]) for c in range(size)]
    sums, counts = sums.reshape(3, n_pb, n_cols), counts.reshape(3, n_pb, n_cols)
    sums.setflags(write=False)
    counts.setflags(write=False)
    return sums, counts


CASES = list(itertools.product(SHAPES, MODES, GRIDS, SEABEDS))


@pytest.mark.parametrize("shape,mode,grid,seabed", CASES)
def test_the_reference_of_every_case_is_exact_and_non_empty(shape, mode, grid, seabed):
    R, P = SHAPES[shape]
    for channel in range(N_PLANES):
        sums, counts = reference(shape, mode, grid, seabed, channel)
        for k in range(3):                                       # a non-empty cell in each plane
            assert (counts[k] > 0).any() and (sums[k] > 0).any()
        assert counts.max() < 2 ** 14
        exact, _ = reference(shape, mode, grid, seabed, channel, exact=True)
        assert np.array_equal(sums, exact)
    # the same cases by the yardstick of the other integrate tests
    pred, planes = operands(shape, mode)
    table, n_pb, n_cols, range_bin = geometry(shape, grid, seabed)
    sb = SEABEDS[seabed]
    line = seabed_line(P, R)
    want = new_host(n_pb, n_cols)
    for p0, p1 in launches(P):
        edges_numpy(*want, pred[:, :, p0:p1], planes[3], THR, mode, table, range_bin, ORIGIN + p0, SV_OFF + p0,
                    line[p0:p1] if sb else None, sb[0] if sb else None, sb[1] if sb else "surface")
    sums, counts = reference(shape, mode, grid, seabed, 3)
    assert np.array_equal(want[0], sums) and np.array_equal(want[1], counts)


def test_the_cases_reach_what_they_are_meant_to_reach():
    for shape, (R, P) in SHAPES.items():
        line = seabed_line(P, R)
        L = np.clip(line.astype(np.int64) - 3, 0, R)
        assert L[7] == 0 and L[40] == R and line[7] - 3 < 0 and line[40] - 3 > R      # one limit clamps to 0, one to n_range
        for a, b in ((0, PING_BIN - ORIGIN), (PING_BIN - ORIGIN, P)):                  # relief above range_bin in each ping bin
            assert L[a:b].max() - L[a:b].min() > RANGE_BIN
        assert (ORIGIN + SEAM) % 4 != 0 and (ORIGIN + SEAM) // PING_BIN == (ORIGIN + SEAM - 1) // PING_BIN == 1
        assert all(reference(shape, "threshold", "uniform", "3 low layers", 0)[1][2, :, l].sum() > 0 for l in range(3))
        pred, planes = operands(shape, "probability")
        bad = ~(np.isfinite(planes) & (planes > 0))
        assert 0.03 < bad.mean() < 0.07 and np.isnan(planes).any() and np.isinf(planes).any() and (planes < 0).any()
        assert np.isnan(pred).any() and (pred < 0).any()
    e = np.array(GRIDS["table"])
    assert e[0] > ORIGIN and (np.diff(e) == 0).any() and e[-1] < ORIGIN + min(P for _, P in SHAPES.values())
    assert SHAPES["16-byte"][0] % 4 == 0 and SHAPES["16-byte"][1] % 4 == 0 and SEAM % 4 == 0 and SHAPES["4-byte"][0] % 4 != 0
