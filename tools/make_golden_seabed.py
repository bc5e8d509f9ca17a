#!/usr/bin/env python3
"""Golden vectors for the seabed-line estimate of a memmap echogram (tests/golden/seabed_estimate.npz): the REFERENCE's
own ``Echogram.get_seabed`` (crimac_unet/data/data_reader.py:433-507), called unbound on a stand-in that carries what the
method touches (``_seabed = None``, a temporary ``path``, ``shape``, ``data_numpy()``).  Needs the reference checkout:
``python tools/make_golden_seabed.py /path/to/CRIMAC-classifiers-unet/crimac_unet`` (or CRIMAC_REFERENCE).

The module is also the home of the numpy restatement of the streaming part (``columns_numpy``: what
``crimac_seabed_columns`` computes, in two accumulation orders) and of the decoders of the fixture's compact inputs, which
the tests and tools/bench_seabed.py import; only ``main()`` needs the reference.

Exact cases: samples k / 1024 (k < 64) plus a bottom band of +4, a few NaN / inf samples, drop-out columns scaled by 2^-20
(every sample a multiple of 2^-30 below 8: every fp64 stencil sum is exact whatever its order).  Realistic case: log-uniform
sv 1e-8 .. 1e-5 (float32 values with the low 16 mantissa bits clear, stored as their high halves) with a 1e-2 bottom
band; kept only if the restatement reproduces the reference's final vector at every ping in both accumulation orders."""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DROP_SCALE = np.float32(2.0 ** -20)

# (tag, (R, P, F), drop-out events [(first ping, last ping, frequencies)]).  A ping counts as a drop-out when its
# standardised log maximum is below -8, i.e. -sqrt((1 - q) / q) < -8 for a fraction q of drop-out pings: q < 1 / 65.
EXACT_CASES = [
    ("a", (200, 400, 3), [(100, 101, (0, 1)), (1, 2, (1, 2)), (397, 399, (0, 2))]),       # interior | from index 2 | to the end
    ("b", (300, 330, 4), [(50, 51, (0, 1, 2)), (2, 3, (0, 1)), (327, 328, (2, 3)), (0, 1, (3,))]),   # even F; run to P - 2; unseen
    ("c", (203, 70, 2), [(2, 2, (0,)), (40, 40, (1,))]),
    ("d", (24, 1, 1), []),
    ("e", (24, 2, 1), []),
]
REAL_CASE = ("real", (200, 400, 3), [(200, 201, (0, 1))])


# ---- the fixture's compact inputs ---------------------------------------------------------------------------------------
def bottom_rows(shape, rng):
    """An undulating bottom row per (ping, frequency), below the rows the estimate skips."""
    R, P, F = shape
    n = 10 + int(0.05 * R)
    x = np.arange(P)[:, None]
    b = 0.7 * R + 0.12 * R * np.sin(x / 23.0 + rng.uniform(0, 6)) + rng.integers(-2, 3, size=(P, F))
    return np.clip(b.astype(np.int64), n + 2, R - 3).astype(np.int16)


def drop_mask(shape, events):
    R, P, F = shape
    m = np.zeros((P, F), dtype=np.uint8)
    for p0, p1, fs in events:
        m[p0:p1 + 1, list(fs)] = 1
    return m


def decode(fix, tag):
    """The float32 echogram [R, P, F] of one fixture case (``Echogram.data_numpy()`` layout) from its compact inputs."""
    kind = str(fix[tag + "/kind"])
    codes = fix[tag + "/codes"]
    if kind == "exact":
        data = codes.astype(np.float32) / np.float32(1024)
        band = np.float32(4)
    else:
        data = (codes.astype(np.uint32) << 16).view(np.float32).copy()
        band = np.float32(1e-2)
    R, P, F = data.shape
    drop = fix[tag + "/drop"].astype(bool)
    below = np.arange(R)[:, None, None] >= fix[tag + "/bottom"][None].astype(np.int64)
    data = np.where(below & ~drop[None], data + band, data).astype(np.float32)
    data = np.where(drop[None], data * DROP_SCALE, data).astype(np.float32)
    bad = fix[tag + "/bad"]                                  # [k, 4]: row, ping, frequency, 0 NaN / 1 +inf / 2 -inf
    vals = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    data[bad[:, 0], bad[:, 1], bad[:, 2]] = vals[bad[:, 3]]
    return data


# ---- numpy restatement of crimac_seabed_columns ---------------------------------------------------------------------------
def columns_numpy(data, order=0):
    """data float32 [R, P, F] -> (idx int32 [F, P], colmax float32 [F, P]): per frequency the first argmax over rows n ..
    R - 1 (relative to n) of ``(grad_1 > 0) * grad_2`` and the maximum of the sanitised data over those rows; the two true
    3x3 convolutions in float64 with zero padding.  ``order`` 0 is the kernel's order of additions (row sums first), 1 adds
    the nine taps one by one, column by column."""
    R, P, F = data.shape
    n = 10 + int(0.05 * R)
    idx = np.empty((F, P), dtype=np.int32)
    colmax = np.empty((F, P), dtype=np.float32)
    for f in range(F):
        d32 = np.where(np.isfinite(data[:, :, f]), data[:, :, f], np.float32(0)).astype(np.float32)
        d = np.zeros((R + 2, P + 2), dtype=np.float64)
        d[1:-1, 1:-1] = d32
        lf, ce, rt = d[:, :-2], d[:, 1:-1], d[:, 2:]              # columns p - 1, p, p + 1 (all padded rows)
        if order == 0:
            s1 = (lf + 2.0 * ce) + rt
            s2 = (lf + 5.0 * ce) + rt
            g1 = s1[2:] - s1[:-2]
            g2 = (s2[:-2] - 2.0 * s2[1:-1]) + s2[2:]
        else:
            up, me, dn = slice(0, R), slice(1, R + 1), slice(2, R + 2)      # rows r - 1, r, r + 1
            g1 = np.zeros((R, P))
            g2 = np.zeros((R, P))
            for col, w1, w2 in ((rt, 1.0, 1.0), (ce, 2.0, 5.0), (lf, 1.0, 1.0)):
                g1 = (g1 - w1 * col[up]) + w1 * col[dn]
                g2 = ((g2 + w2 * col[dn]) - 2.0 * w2 * col[me]) + w2 * col[up]
        score = np.where(g1 > 0, g2, 0.0)
        idx[f] = np.argmax(score[n:], axis=0)
        colmax[f] = d32[n:].max(axis=0)
    return idx, colmax


def host_seabed(data):
    """The whole estimate on the host: the restatement above + the package's finishing step."""
    from crimac_classifiers_unet_amd.tiled_inference import finish_seabed
    idx, colmax = columns_numpy(data)
    return finish_seabed(idx, colmax, data.shape[0])


class EchogramStandIn:
    """What ``estimate_seabed_memm`` (and the reference's ``get_seabed``) reads of a memmap echogram without a stored
    seabed: ``shape``, every frequency plane [range, pings], ``data_numpy()`` [range, pings, F]."""
    data_format = "memmap"
    _seabed = None

    def __init__(self, data, path=None):
        self.data = data
        self.shape = data.shape[:2]
        self.frequencies = [18, 38, 120, 200, 333, 70][:data.shape[2]]
        self.path = path

    def data_memmaps(self, frequencies=None):
        fs = self.frequencies if frequencies is None else list(frequencies)
        return [self.data[:, :, self.frequencies.index(int(f))] for f in fs]

    def data_numpy(self, frequencies=None):
        return np.stack(self.data_memmaps(frequencies), axis=-1).astype("float32")


# ---- the reference ------------------------------------------------------------------------------------------------------
def import_reference(ref_root):
    sys.path.insert(0, ref_root)
    for name in ("dask", "xarray", "numcodecs", "tqdm", "pandas", "matplotlib", "matplotlib.colors", "matplotlib.pyplot",
                 "paths", "zarr"):
        if name in sys.modules:
            continue
        try:
            __import__(name)
        except Exception:
            m = types.ModuleType(name)
            if name == "dask":
                m.config = types.SimpleNamespace(set=lambda **kw: None)
            if name == "numcodecs":
                m.Blosc = object
            sys.modules[name] = m
    import collections
    import collections.abc
    if not hasattr(collections, "Iterable"):          # (py < 3.10 idiom of the reference)
        collections.Iterable = collections.abc.Iterable
    for alias in ("int", "float", "bool"):
        if alias not in np.__dict__:
            setattr(np, alias, {"int": int, "float": float, "bool": bool}[alias])
    from data.data_reader import Echogram
    return Echogram


def reference_seabed(Echogram, data):
    with tempfile.TemporaryDirectory() as tmp:
        eg = EchogramStandIn(data.copy(), path=tmp)
        with np.errstate(all="ignore"):
            out = Echogram.get_seabed(eg, 0, data.shape[1])
        assert os.path.isfile(os.path.join(tmp, "seabed.npy"))
    return np.asarray(out).astype(np.int64)


_RUNS = []          # every run the finishing step repaired, over all cases


def make_case(Echogram, tag, shape, events, kind, seed):
    from crimac_classifiers_unet_amd import tiled_inference as ti
    rng = np.random.Generator(np.random.PCG64(seed))
    R, P, F = shape
    if kind == "exact":
        codes = rng.integers(0, 64, size=shape).astype(np.uint8)
    else:
        sv = np.power(10.0, rng.uniform(-8.0, -5.0, size=shape)).astype(np.float32)
        codes = (sv.view(np.uint32) >> 16).astype(np.uint16)
    n_bad = max(2, (R * P * F) // 4000)
    bad = np.stack([rng.integers(0, R, n_bad), rng.integers(0, P, n_bad), rng.integers(0, F, n_bad),
                    rng.integers(0, 3, n_bad)], axis=1).astype(np.int32)
    fix = {f"{tag}/kind": np.array(kind), f"{tag}/codes": codes, f"{tag}/bottom": bottom_rows(shape, rng),
           f"{tag}/drop": drop_mask(shape, events), f"{tag}/bad": bad}
    data = decode(fix, tag)
    assert data.dtype == np.float32 and data.shape == shape and not np.isfinite(data).all()
    ref = reference_seabed(Echogram, data)
    i0, c0 = columns_numpy(data, 0)
    i1, c1 = columns_numpy(data, 1)
    assert np.array_equal(c0, c1)
    if kind == "exact":
        assert np.array_equal(i0, i1), f"{tag}: the two accumulation orders disagree on an exact case"
    runs = []
    ours = [ti.finish_seabed(i0, c0, R, runs=runs), ti.finish_seabed(i1, c0, R)]
    ok = all(np.array_equal(o, ref) for o in ours)
    if kind == "exact":
        assert ok, f"{tag}: restatement != reference at pings {np.nonzero(ours[0] != ref)[0][:10]}"
    elif not ok:
        return None
    if events:                                        # the repair must have fired, and must show in the result
        want = {(f, max(p0, 2), p1) for p0, p1, fs in events for f in fs if p1 >= 2 and max(p0, 2) < P - 2}
        assert {r[:3] for r in runs} == want, f"{tag}: repaired runs {sorted(runs)} != planned {sorted(want)}"
        n, a = ti.seabed_rows(R)
        raw = np.rint(np.median((i0.T.astype(np.float64) + (n - a)), axis=1)).astype(int)
        assert not np.array_equal(raw, ref), f"{tag}: the repair branch changed nothing"
    _RUNS.extend(runs)
    fix.update({f"{tag}/idx": i0.astype(np.int16), f"{tag}/colmax": c0, f"{tag}/ref": ref.astype(np.int32)})
    print(f"{tag}: {shape} seed {seed}: reference reproduced, {int(fix[tag + '/drop'].sum())} drop-out columns, "
          f"repairs {sorted({r[3] for r in runs})}, seabed {ref.min()}..{ref.max()}")
    return fix


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CRIMAC_REFERENCE")
    if not ref_root:
        sys.exit("usage: make_golden_seabed.py <reference checkout>/crimac_unet")
    Echogram = import_reference(ref_root)
    fix = {}
    for k, (tag, shape, events) in enumerate(EXACT_CASES):
        fix.update(make_case(Echogram, tag, shape, events, "exact", 100 + k))
    tag, shape, events = REAL_CASE
    for seed in range(200, 232):
        got = make_case(Echogram, tag, shape, events, "real", seed)
        if got is not None:
            fix.update(got)
            break
        print(f"{tag}: seed {seed} rejected (an accumulation order moves the result)")
    else:
        raise SystemExit("no seed of the realistic case is order-independent")
    assert all(any(c == case for *_, c in _RUNS) for case in ("behind", "front", "mean"))
    fix["tags"] = np.array([c[0] for c in EXACT_CASES] + [REAL_CASE[0]])
    path = os.path.join(ROOT, "tests", "golden", "seabed_estimate.npz")
    np.savez_compressed(path, **fix)
    print("saved", os.path.getsize(path))
    assert os.path.getsize(path) <= 1000000


if __name__ == "__main__":
    main()
