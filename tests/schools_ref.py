"""CPU reference of the school detector (tests only): ``scipy.ndimage.label`` relabelled to anchors, float64 numpy sums.

``detect(mask, sv, ...)`` gives the chunk-local table ``SchoolTable.numpy()`` gives -- the input of
``merge_school_chunks`` -- so the same function is the reference of the kernels (one chunk), of the merge (per chunk
against the whole array) and of the flows."""
import numpy as np
from scipy import ndimage

SHAPES = [(1, 1), (1, 130), (67, 1), (37, 70), (64, 256), (129, 257)]          # n_range x n_pings: off every tile multiple
PATTERNS = ("empty", "full", "checker", "serpentine", "spiral", "combs", "random30", "random60")


def pattern(name, R, P, seed=0):
    """The masks of tools/exp/ccl_host_check.cpp (the random ones by numpy's generator)."""
    m = np.zeros((R, P), dtype=bool)
    rr, pp = np.mgrid[0:R, 0:P]
    if name == "full":
        m[:] = True
    elif name == "checker":
        m = (rr + pp) % 2 == 0
    elif name == "serpentine":                      # even rows full, odd rows one pixel at alternating ends: one long path
        m[0::2] = True
        for r in range(1, R, 2):
            m[r, P - 1 if (r // 2) % 2 == 0 else 0] = True
    elif name == "spiral":                          # a one-pixel path that winds inwards, one gap wide
        def is_set(r, p):
            return 0 <= r < R and 0 <= p < P and m[r, p]

        def is_open(r, p, dr, dp):
            nr, np_ = r + dr, p + dp
            return 0 <= nr < R and 0 <= np_ < P and not m[nr, np_] and not is_set(nr + dr, np_ + dp)
        r = p = dr = 0
        dp = 1
        for _ in range(R * P):
            m[r, p] = True
            if not is_open(r, p, dr, dp):
                dr, dp = dp, -dr
                if not is_open(r, p, dr, dp):
                    break
            r, p = r + dr, p + dp
    elif name == "combs":                           # a spine every 24 rows, teeth every third ping, 20 rows: they cross tiles
        m = (rr % 24 == 0) | ((pp % 3 == 0) & (rr % 24 <= 20))
    elif name in ("random30", "random60"):
        rng = np.random.Generator(np.random.PCG64(seed + R * 1000 + P))
        m = rng.random((R, P)) < (0.3 if name == "random30" else 0.6)
    elif name != "empty":
        raise ValueError(name)
    return np.ascontiguousarray(m)


def label(mask, connectivity):
    """int32 [R, P]: -1 for background, otherwise the linear index of the component's first pixel in raster order."""
    mask = np.asarray(mask, dtype=bool)
    lab, n = ndimage.label(mask, structure=np.ones((3, 3)) if connectivity == 8 else None)
    out = np.full(mask.shape, -1, dtype=np.int32)
    if n:
        flat = lab.ravel()
        idx = np.flatnonzero(flat)
        first = np.full(n + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, flat[idx], idx)
        out.ravel()[idx] = first[flat[idx]]
    return out


def detect(mask, sv, connectivity, min_pixels=1, keep_left=False, keep_right=False, start_ping=0, frequencies=(38,),
           klass="sandeel"):
    """The chunk-local table of ``mask`` bool [R, P]; ``sv`` float [F, P, R] (range fastest, as the chunk's data), the
    pixel rule of the integration: finite and > 0.  Kept: ``pixels >= min_pixels``, or the school touches a kept edge."""
    mask = np.asarray(mask, dtype=bool)
    R, P = mask.shape
    lab = label(mask, connectivity)
    anchors = np.flatnonzero(lab.ravel() == np.arange(R * P))
    slot = np.full(R * P + 1, -1, dtype=np.int64)
    slot[anchors] = np.arange(len(anchors))
    idx = np.flatnonzero(lab.ravel() >= 0)
    of = slot[lab.ravel()[idx]]
    K = len(anchors)
    rows, pings = idx // P, idx % P
    pixels = np.bincount(of, minlength=K).astype(np.int64)
    touch = np.zeros(K, dtype=bool)
    if keep_left:
        touch[of[pings == 0]] = True
    if keep_right:
        touch[of[pings == P - 1]] = True
    keep = (pixels >= min_pixels) | touch
    new = np.full(K + 1, -1, dtype=np.int64)
    new[:K][keep] = np.arange(keep.sum())
    of = new[of]
    sel = of >= 0
    of, rows, pings = of[sel], rows[sel], pings[sel]
    K = int(keep.sum())

    def ext(fn, init, v):
        a = np.full(K, init, dtype=np.int64)
        fn.at(a, of, v)
        return a
    big = np.iinfo(np.int32).max
    F = sv.shape[0]
    sv_sum, sv_pixels = np.zeros((F, K), np.float64), np.zeros((F, K), np.int64)
    for f in range(F):
        x = np.asarray(sv[f], dtype=np.float32).T[rows, pings]
        ok = np.isfinite(x) & (x > 0)
        np.add.at(sv_sum[f], of[ok], x[ok].astype(np.float64))
        np.add.at(sv_pixels[f], of[ok], 1)
    edge = new[slot[lab]] if lab.size else lab            # [R, P] school index (-1 background / dropped)
    return {"anchor": anchors[keep].astype(np.int32), "pixels": pixels[keep],
            "bbox": np.stack([ext(np.minimum, big, rows), ext(np.maximum, 0, rows + 1), ext(np.minimum, big, pings),
                              ext(np.maximum, 0, pings + 1)], axis=1).astype(np.int32),
            "row_sum": ext(np.add, 0, rows), "ping_sum": ext(np.add, 0, pings), "sv_sum": sv_sum, "sv_pixels": sv_pixels,
            "edges": np.stack([edge[:, 0], edge[:, -1]]).astype(np.int32), "start_ping": start_ping, "n_pings": P,
            "n_range": R, "class": klass, "frequencies": tuple(frequencies), "labels": lab}


INT_FIELDS = ("anchor", "pixels", "bbox", "row_sum", "ping_sum", "sv_pixels")


def same_schools(got, want, fields=INT_FIELDS):
    """Every integer field equal, and ``sv_sum`` within n * 2^-52 * ref, n = the school's ``sv_pixels``: all terms are
    positive, so any order of summation is within (n - 1) u of the exact sum on each side."""
    for name in fields:
        assert np.array_equal(np.asarray(got[name]), np.asarray(want[name])), name
    bound = want["sv_pixels"] * 2.0 ** -52 * want["sv_sum"]
    assert np.all(np.abs(got["sv_sum"] - want["sv_sum"]) <= bound), float(np.max(np.abs(got["sv_sum"] - want["sv_sum"]) - bound))
