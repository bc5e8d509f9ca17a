"""CPU reference of the school scores (tests only): ``scipy.ndimage.label`` (through ``schools_ref``) on ``ids == code``, on
``mask_a & mask_b`` and on the ignored rule, and pair counts with numpy.

``pair_table`` is the whole-plane reference of ``merge_school_overlaps`` / the flows; ``overlap_chunk`` gives the
chunk-local rows ``SchoolOverlaps.numpy()`` gives, so the merge can be checked without a GPU."""
import numpy as np

import schools_ref as ref

CODES = {1: 27, 2: 1}                                 # the raw annotation id of class k
FILL = (0, 1, 27, 12, 5000, -1)                       # what a background pixel of a test's id plane is filled from


def ignored_mask(ids):
    """The ids the label transform ignores: anything but 0, 27 and 1."""
    ids = np.asarray(ids)
    return (ids != 0) & (ids != 27) & (ids != 1)


def ids_for(mask, code, seed=0):
    """int16 [P, R] (range fastest, the chunk layout): ``code`` where ``mask`` [R, P] is set, elsewhere values of FILL other
    than ``code`` (for ``code`` None -- the ignored rule -- elsewhere 0 / 1 / 27 and inside 12 / 5000 / -1)."""
    rng = np.random.Generator(np.random.PCG64(seed + 31 * mask.shape[0] + mask.shape[1]))
    if code is None:
        inside, outside = np.array([12, 5000, -1]), np.array([0, 1, 27])
    else:
        inside, outside = np.array([code]), np.array([v for v in FILL if v != code])
    ids = np.where(mask, inside[rng.integers(0, len(inside), mask.shape)], outside[rng.integers(0, len(outside), mask.shape)])
    return np.ascontiguousarray(ids.T.astype(np.int16))


def rows_of(table, labels_at):
    """Chunk-local rows of the schools with the given anchors in ``table`` (-1: not in the table)."""
    where = {int(a): i for i, a in enumerate(table["anchor"])}
    return np.array([where.get(int(a), -1) for a in labels_at], dtype=np.int64)


def pair_table(a, b, sv):
    """The pair overlaps of two ``ref.detect`` tables of one plane (their ``"labels"`` planes and kept rows): ``"pred"``,
    ``"ann"``, ``"pixels"`` [M], ``"sv_sum"`` / ``"sv_pixels"`` [F, M] sorted by (pred, ann); ``sv`` float [F, P, R]."""
    la, lb = a["labels"], b["labels"]
    rr, pp = np.nonzero((la >= 0) & (lb >= 0))
    ra, rb = rows_of(a, la[rr, pp]), rows_of(b, lb[rr, pp])
    keep = (ra >= 0) & (rb >= 0)
    rr, pp, ra, rb = rr[keep], pp[keep], ra[keep], rb[keep]
    pairs, of = np.unique(np.stack([ra, rb], axis=1), axis=0, return_inverse=True)
    of = of.reshape(-1)
    M, F = len(pairs), sv.shape[0]
    out = {"pred": pairs[:, 0], "ann": pairs[:, 1], "pixels": np.bincount(of, minlength=M).astype(np.int64),
           "sv_sum": np.zeros((F, M), np.float64), "sv_pixels": np.zeros((F, M), np.int64)}
    for f in range(F):
        x = np.asarray(sv[f], dtype=np.float32).T[rr, pp]
        ok = np.isfinite(x) & (x > 0)
        np.add.at(out["sv_sum"][f], of[ok], x[ok].astype(np.float64))
        np.add.at(out["sv_pixels"][f], of[ok], 1)
    return out


def overlapped_pixels(a, other_mask):
    """Per kept row of the ``ref.detect`` table ``a``: its pixels that lie in ``other_mask``."""
    la = a["labels"]
    rows = rows_of(a, la[(la >= 0) & other_mask])
    return np.bincount(rows[rows >= 0], minlength=len(a["anchor"])).astype(np.int64)


def overlap_chunk(a, b, sv, connectivity):
    """The chunk-local overlap rows of two ``ref.detect`` tables of one chunk, as ``SchoolOverlaps.numpy()``: one row per
    connected component of the intersection plane in ascending anchor order, ``"pred"`` / ``"ann"`` = rows of a / b (-1: dropped)."""
    la, lb = a["labels"], b["labels"]
    t = ref.detect((la >= 0) & (lb >= 0), sv, connectivity)
    at = np.asarray(t["anchor"], dtype=np.int64)
    return {"anchor": t["anchor"], "pixels": t["pixels"], "sv_sum": t["sv_sum"], "sv_pixels": t["sv_pixels"],
            "pred": rows_of(a, la.ravel()[at]), "ann": rows_of(b, lb.ravel()[at])}


def same_overlaps(got, want):
    """Pairs and integer fields equal; ``sv_sum`` within n * 2^-52 * ref, n = the pair's ``sv_pixels`` (``ref.same_schools``)."""
    ref.same_schools(got, want, fields=("pred", "ann", "pixels", "sv_pixels"))


def score(pred_mask, ids, klass, sv, connectivity, min_pixels=1, frequencies=(38,)):
    """One class of what the scoring flows return, on whole arrays: ``pred_mask`` bool [R, P], ``ids`` [P, R], ``sv`` [F, P, R];
    anchors as (row, ping)."""
    ids = np.asarray(ids).T
    pred = ref.detect(pred_mask, sv, connectivity, min_pixels, frequencies=frequencies)
    ann = ref.detect(ids == CODES[klass], sv, connectivity, min_pixels, frequencies=frequencies)
    res = {"overlaps": pair_table(pred, ann, sv), "ignored_pixels": overlapped_pixels(pred, ignored_mask(ids))}
    P = pred_mask.shape[1]
    for name, t in (("predicted", pred), ("annotated", ann)):
        t = dict(t)
        t["anchor"] = np.stack([t["anchor"] // P, t["anchor"] % P], axis=1)
        res[name] = t
    return res
