"""GPU: per-class PR histograms from one pass (``crimac_pr_histogram_classes`` and the ``classes=`` keyword of the tiled
evaluation flows).

The kernel cases place the probability of ONE class per pixel at the centre of a chosen float16 bin (the construction of
tests/test_gpu_loss_opt_kernels.py), the other logits 0, so the expected counts are exact integers: all
[ncls][2][16384] counters are compared, no pixel is left out, nothing has a tolerance.  The flows are compared with
themselves: the default call, and a direct kernel call on the batches the flow hands to ``on_batch``."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import hip  # noqa: E402
from crimac_classifiers_unet_amd import tiled_inference as ti  # noqa: E402
from crimac_classifiers_unet_amd.hip import call, ptr  # noqa: E402
from tools.fake_reader import FakeEchogram, FakeZarrReader, eval_stub_logits, synth_eval_survey  # noqa: E402

pytestmark = pytest.mark.gpu

PR_BINS = hip.PR_BINS
NAN_BIN = PR_BINS - 1
ONE_BIN = 0x3C00                          # float16 1.0
SKIPPED = (-70, -30, -100, -10)
SEABED = -50
LABEL_DTYPES = {2: np.int16, 4: np.int32, 8: np.int64}
HIST_SHAPE = (2, 125, 125)                # per selected class; H * W is odd, so thread ranges straddle images
SENTINEL = 123456789
FREQS = [18, 38, 120, 200]
DEV = "cuda"
# A float32 softmax (an exp within 2 ulp, the additions of the sum, one division) is within 6e-7 of the exact probability,
# relatively; a probability at least TIE_MARGIN (relative) away from every float16 rounding boundary therefore rounds to the
# same float16 in float32 and in the float64 reference.
TIE_MARGIN = 1e-5


def _seed(*key):
    s = 29
    for k in key:
        s = (s * 1000003 + int(k) + 1000) % (2 ** 31 - 1)
    return s


def softmax64(z, axis=1):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis, keepdims=True))
    return e / e.sum(axis, keepdims=True)


def half_of_bits(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)


def logit_for_bin(bits, ncls):
    """z_c (fp32; the other ``ncls - 1`` logits 0) whose softmax probability rounds to the float16 with this bit pattern."""
    bits = np.asarray(bits, dtype=np.int64)
    h = half_of_bits(np.clip(bits, 1, ONE_BIN - 1))
    z = np.log((ncls - 1) * h / (1 - h)).astype(np.float32)
    return np.where(bits == 0, np.float32(-200.0), np.where(bits == ONE_BIN, np.float32(200.0), z)).astype(np.float32)


def tie_margin(prob):
    """Relative distance of every probability from the nearer float16 rounding boundary, minimum over the class axis."""
    h = prob.astype(np.float16)
    out = np.full(prob.shape, np.inf)
    for to in (-np.inf, np.inf):
        tie = (h.astype(np.float64) + np.nextafter(h, np.float16(to)).astype(np.float64)) / 2
        out = np.minimum(out, np.abs(prob - tie) / np.maximum(prob, 1e-300))
    return out.min(axis=1)


def reference(z, labels, classes):
    """[ncls][2][16384] int64: row c of ``classes`` = (pos, neg) of float16(softmax64(z)[c]); labels -70 / -30 / -100 / -10
    are skipped, -50 counts as probability 0 in neg, label c goes to pos, every other label to neg; other rows zero."""
    B, ncls = z.shape[:2]
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    prob = np.moveaxis(softmax64(z, 1), 1, 0).reshape(ncls, -1)
    keep = ~np.isin(lab, SKIPPED)
    out = np.zeros((ncls, 2, PR_BINS), dtype=np.int64)
    for c in classes:
        p = np.where(lab == SEABED, 0.0, prob[c])
        bits = p.astype(np.float16).view(np.uint16).astype(np.int64)
        bits = np.where(bits > ONE_BIN, NAN_BIN, bits)
        pos = keep & (lab == c)
        out[c, 0] = np.bincount(bits[pos], minlength=PR_BINS)
        out[c, 1] = np.bincount(bits[keep & ~pos], minlength=PR_BINS)
    return out


@functools.lru_cache(maxsize=None)
def bin_case(ncls, lbytes, classes):
    """Pixels in a random order.  For every class c of ``classes``: every bin 0 .. 0x3C00 of c once with label c and once
    with another class's label, each of the skipped ids and -50 at several bins; the rest of the shape cycles the bins with
    labels of every kind.  The class whose logit is set has its probability at the bin's centre, the other logits are 0;
    where that puts ANOTHER selected class's probability within TIE_MARGIN of a float16 rounding boundary (with three
    classes: (1 - h) / 2 near 0.5 - 2^-13, some 1300 bins around h = 2^-12) the other foreground logits are -200 instead
    -- probability 0, bin 0 -- and the set class keeps its bin centre against the background alone."""
    B, H, W = HIST_SHAPE[0] * len(classes), HIST_SHAPE[1], HIST_SHAPE[2]
    npix = B * H * W
    rng = np.random.default_rng(_seed(ncls, lbytes, *classes))
    every = np.arange(ONE_BIN + 1)
    special = np.array([0, 1, 0x1234, 0x3800, 0x3BFF, ONE_BIN])
    bins, labs, tgt = [], [], []
    for c in classes:
        others = np.array([k for k in range(ncls) if k != c])
        bins += [every, every] + [special] * 5
        labs += [np.full_like(every, c), others[every % len(others)]] + [np.full(6, l) for l in SKIPPED + (SEABED,)]
        tgt += [np.full(2 * len(every) + 30, c)]
    bins, labs, tgt = np.concatenate(bins), np.concatenate(labs), np.concatenate(tgt)
    fill = npix - len(bins)
    assert fill >= 0 and (H * W) % 2 == 1
    kinds = np.array(tuple(range(ncls)) + tuple(classes) + SKIPPED + (SEABED,))
    bins = np.concatenate([bins, (np.arange(fill) * 7) % (ONE_BIN + 1)])
    labs = np.concatenate([labs, kinds[rng.integers(0, len(kinds), fill)]])
    tgt = np.concatenate([tgt, np.array(classes)[np.arange(fill) % len(classes)]])
    perm = rng.permutation(npix)
    bins, labs, tgt = bins[perm], labs[perm], tgt[perm]
    onehot = (tgt[:, None] == np.arange(ncls)[None, :])
    z = np.where(onehot, logit_for_bin(bins, ncls)[:, None], np.float32(0)).astype(np.float32)
    unsafe = tie_margin(softmax64(z, 1)[:, list(classes)]) <= TIE_MARGIN
    alone = np.where(onehot, logit_for_bin(bins, 2)[:, None], np.float32(-200.0)).astype(np.float32)
    alone[:, 0] = 0
    z[unsafe] = alone[unsafe]
    assert unsafe.mean() < 0.1
    assert tie_margin(softmax64(z, 1)[:, list(classes)]).min() > TIE_MARGIN
    got_bits = softmax64(z, 1)[np.arange(npix), tgt].astype(np.float16).view(np.uint16)
    assert np.array_equal(got_bits, bins)                      # the set class sits in the bin that was asked for
    z = np.ascontiguousarray(z.reshape(B, H, W, ncls).transpose(0, 3, 1, 2))
    c = types.SimpleNamespace(B=B, H=H, W=W, ncls=ncls, z=z, labels=labs.reshape(B, H, W).astype(LABEL_DTYPES[lbytes]),
                              npix=npix, classes=classes, want=reference(z, labs, classes))
    for a in (z, c.labels, c.want):
        a.setflags(write=False)
    return c


def mask_of(classes):
    return sum(1 << c for c in classes)


def run(z, labels, classes, hist):
    zd, ld = torch.from_numpy(np.array(z)).to(DEV), torch.from_numpy(np.array(labels)).to(DEV)      # (writable copies)
    B, ncls, H, W = z.shape
    call("crimac_pr_histogram_classes", ptr(zd), ncls, ptr(ld), labels.itemsize, B, H, W, mask_of(classes), ptr(hist))
    return hist.cpu().numpy().astype(np.int64)


def run_old(z, labels):
    zd, ld = torch.from_numpy(np.array(z)).to(DEV), torch.from_numpy(np.array(labels)).to(DEV)      # (writable copies)
    B, ncls, H, W = z.shape
    hist = torch.zeros(2, PR_BINS, dtype=torch.int32, device=DEV)
    call("crimac_pr_histogram", ptr(zd), ncls, ptr(ld), labels.itemsize, B, H, W, ptr(hist[0]), ptr(hist[1]))
    return hist.cpu().numpy().astype(np.int64)


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lbytes", [2, 4, 8])
@pytest.mark.parametrize("ncls,classes", [(2, (1,)), (3, (1, 2)), (3, (2,)), (4, (1, 3)), (4, (1, 2, 3))])
def test_every_bin_of_every_selected_class(ncls, classes, lbytes):
    c = bin_case(ncls, lbytes, classes)
    for k in classes:                  # every bin once as positive and once as negative, at the least
        assert (c.want[k, :, :ONE_BIN + 1] >= 1).all() and not c.want[k, :, ONE_BIN + 1:].any()
    hist = torch.zeros(ncls, 2, PR_BINS, dtype=torch.int32, device=DEV)
    rest = [k for k in range(ncls) if k not in classes]
    hist[rest] = SENTINEL              # row 0 and the rows that are not selected
    got = run(c.z, c.labels, classes, hist)
    assert np.array_equal(got[list(classes)], c.want[list(classes)])
    assert (got[rest] == SENTINEL).all()
    if 1 in classes:                   # ... and row 1 is the single-class kernel's result
        assert np.array_equal(got[1], run_old(c.z, c.labels))


@pytest.mark.parametrize("classes", [(1,), (1, 2)])
def test_row_1_equals_the_single_class_kernel_on_random_logits(classes):
    rng = np.random.default_rng(11)
    B, ncls, H, W = 2, 3, 65, 33
    z = (4 * rng.standard_normal((B, ncls, H, W))).astype(np.float32)
    kinds = np.array((0, 1, 2) + SKIPPED + (SEABED,))
    labels = kinds[rng.integers(0, len(kinds), (B, H, W))].astype(np.int16)
    got = run(z, labels, classes, torch.zeros(ncls, 2, PR_BINS, dtype=torch.int32, device=DEV))
    want = run_old(z, labels)
    assert np.array_equal(got[1], want) and want[0].sum() > 0 and want[1].sum() > 0
    assert not got[0].any() and (got[2].sum() == want.sum() if 2 in classes else not got[2].any())


def test_skewed_batch_counts_exactly():
    """90 % of the pixels below the seabed, the rest in bins 0-2 of both classes: nearly every count lands on a handful of
    counters -- the aggregation's counter width, its flush and the grid-stride tail (1025 rows: not a multiple of the
    workgroups' stride)."""
    B, ncls, H, W = 1, 3, 1025, 1024
    npix = H * W
    rng = np.random.default_rng(12)
    labels = np.full(npix, SEABED, dtype=np.int16)
    rest = rng.permutation(npix)[:npix // 10]
    kinds = np.array((0, 0, 0, 0, 1, 2) + SKIPPED)
    labels[rest] = kinds[rng.integers(0, len(kinds), len(rest))]
    z = np.zeros((npix, ncls), dtype=np.float32)
    tgt = rng.integers(1, 3, npix)
    z[np.arange(npix), 3 - tgt] = -200.0                       # the other foreground class: bin 0, and no share of the sum
    z[np.arange(npix), tgt] = logit_for_bin(rng.integers(0, 3, npix), 2)      # (so: against the background alone)
    z = np.ascontiguousarray(z.T.reshape(1, ncls, H, W))
    labels = labels.reshape(B, H, W)
    want = reference(z, labels, (1, 2))
    assert tie_margin(np.moveaxis(softmax64(z, 1), 1, -1).reshape(-1, ncls)[:, 1:]).min() > TIE_MARGIN
    got = run(z, labels, (1, 2), torch.zeros(ncls, 2, PR_BINS, dtype=torch.int32, device=DEV))
    assert np.array_equal(got, want)
    valid = int((~np.isin(labels, SKIPPED)).sum())
    assert got[1].sum() == got[2].sum() == valid and not got[:, :, 3:].any() and got[1, 1, 0] > 0.9 * npix


def test_two_calls_accumulate_onto_a_prefilled_histogram():
    c = bin_case(3, 2, (1, 2))
    pre = np.random.default_rng(5).integers(0, 1000, (3, 2, PR_BINS))
    hist = torch.from_numpy(pre.astype(np.int32)).to(DEV)
    assert np.array_equal(run(c.z, c.labels, (1, 2), hist), pre + c.want)
    assert np.array_equal(run(c.z, c.labels, (1, 2), hist), pre + 2 * c.want)


def test_nan_logit_lands_in_the_nan_bin_of_every_selected_row_and_the_wrapper_names_the_class():
    z = np.zeros((1, 3, 4, 5), dtype=np.float32)
    z[0, 0, 1, 2] = np.nan
    labels = np.zeros((1, 4, 5), dtype=np.int16)
    labels[0, 1, 2] = 2
    hist = torch.zeros(3, 2, PR_BINS, dtype=torch.int32, device=DEV)
    got = run(z, labels, (1, 2), hist)
    assert got[1, 1, NAN_BIN] == 1 and got[2, 0, NAN_BIN] == 1 and got[:, :, NAN_BIN].sum() == 2
    assert got[1].sum() == got[2].sum() == 20 and not got[0].any()
    with pytest.raises(ValueError, match=r"NaN \(sandeel"):
        ti.finish_histograms(hist, all_reduce=False, classes=(1, 2))
    with pytest.raises(ValueError, match=r"NaN \(other probabilities.*class 2"):
        ti.finish_histograms(hist, all_reduce=False, classes=(2,))
    hist[1, 1, NAN_BIN] = 0
    hp, hn = ti.finish_histograms(hist, all_reduce=False, classes=(1,))
    assert hp.shape == hn.shape == (1, PR_BINS) and hp.dtype == hn.dtype == np.int64 and hn.sum() == 19


def test_bad_arguments_are_refused_before_any_launch():
    z = torch.zeros(1, 3, 4, 5, device=DEV)
    lab = torch.zeros(1, 4, 5, dtype=torch.int16, device=DEV)
    hist = torch.zeros(3, 2, PR_BINS, dtype=torch.int32, device=DEV)
    lib = hip.load_library()
    for mask in (0, 1, 3, 8, 2 | 8, 1 << 31):                      # none, the background, a class the model does not have
        with pytest.raises(hip.HipLibraryError, match="class_mask"):
            call("crimac_pr_histogram_classes", ptr(z), 3, ptr(lab), 2, 1, 4, 5, mask, ptr(hist))
        assert b"class_mask" in lib.crimac_last_error()
    for args in ((None, 3, ptr(lab), 2, 1, 4, 5, 6, ptr(hist)), (ptr(z), 3, None, 2, 1, 4, 5, 6, ptr(hist)),
                 (ptr(z), 3, ptr(lab), 2, 1, 4, 5, 6, None), (ptr(z), 3, ptr(lab), 3, 1, 4, 5, 6, ptr(hist)),
                 (ptr(z), 9, ptr(lab), 2, 1, 4, 5, 6, ptr(hist)), (ptr(z), 3, ptr(lab), 2, 0, 4, 5, 6, ptr(hist))):
        with pytest.raises(hip.HipLibraryError, match="pr_histogram_classes"):
            call("crimac_pr_histogram_classes", *args)
    torch.cuda.synchronize()
    assert not bool(hist.any())


# ---- the flows -----------------------------------------------------------------------------------------------------------
def decode(x, eng):
    """NHWC activations [N, 16] of the engine's storage type -> float32 (h3p: 8-channel groups of [8 x hi][8 x lo] halves)."""
    if eng.is_hp:
        h = x.contiguous().view(torch.float16).reshape(-1, 2, 2, 8).float()
        return (h[:, :, 0] + h[:, :, 1]).reshape(-1, 16)
    return x.float()


def stub_predict_fn(eng):
    def fn(x, P, H, W):
        db = decode(x, eng).reshape(P, H, W, 16)[..., :4].permute(0, 3, 1, 2)
        ar = lambda n: torch.arange(n, device=x.device)          # noqa: E731
        z = eval_stub_logits(db, lambda a: torch.floor(a).long(), torch.remainder, ar)
        return torch.stack([c.float() for c in z], dim=1).contiguous()
    return fn


def make_pipe(model):
    pipe = types.SimpleNamespace(model=model.to(DEV).eval(), device=torch.device(DEV), frequencies=FREQS)
    pipe.fn = stub_predict_fn(pipe.model.infer_engine)
    return pipe


@pytest.fixture(scope="module")
def stub_pipe():
    return make_pipe(pkg.UNet_Baseline(3, 4, start_filts=8, precision="f32x6"))


class Direct:
    """on_batch hook: the per-class histograms of a direct ``crimac_pr_histogram_classes`` call on every batch, summed."""

    def __init__(self, classes, ncls=3):
        self.classes, self.batches = classes, 0
        self.hist = torch.zeros(ncls, 2, PR_BINS, dtype=torch.int32, device=DEV)

    def __call__(self, centres, labels, logits, **kw):
        B, nc, H, W = logits.shape
        call("crimac_pr_histogram_classes", ptr(logits), nc, ptr(labels), labels.element_size(), B, H, W,
             mask_of(self.classes), ptr(self.hist))
        self.batches += 1

    def rows(self):
        h = self.hist.cpu().numpy().astype(np.int64)[list(self.classes)]
        return h[:, 0], h[:, 1]


def check_flow(flow):
    """``flow(**kw) -> (hist_pos, hist_neg)``: the checks every flow with ``classes`` has to pass."""
    hp1, hn1 = flow()
    hook = Direct((1, 2))
    hp, hn = flow(classes=(1, 2), on_batch=hook)
    assert hp.shape == hn.shape == (2, PR_BINS) and hp.dtype == hn.dtype == np.int64
    assert np.array_equal(hp[0], hp1) and np.array_equal(hn[0], hn1)             # sandeel: the default call, exactly
    dp, dn = hook.rows()
    assert hook.batches >= 2 and np.array_equal(hp, dp) and np.array_equal(hn, dn)
    assert hp[0].sum() > 0 and hp[1].sum() > 0 and hn[1].sum() > 1000
    assert hp[0].sum() + hn[0].sum() == hp[1].sum() + hn[1].sum()               # the same valid pixels for every class
    sp, sn = flow(classes=(2, 1))
    assert np.array_equal(sp, hp[::-1]) and np.array_equal(sn, hn[::-1])
    return hp, hn


def test_evaluate_survey_with_classes(stub_pipe):
    sv, labels, seabed, boxes = synth_eval_survey(437, 150, 21)
    reader = FakeZarrReader(sv, labels, seabed, boxes=boxes)
    check_flow(lambda **kw: ti.evaluate_survey(reader, stub_pipe, (64, 64), 8, 8, 97, predict_fn=stub_pipe.fn, **kw))
    for bad in ((0,), (3,), (1, 1), ()):
        with pytest.raises(ValueError, match="classes"):
            ti.evaluate_survey(None, stub_pipe, (64, 64), 8, 8, 97, classes=bad)          # (refused before the reader is used)
    ti.release_staging()


EXTENTS = [(300, 90), (40, 200), (17, 17), (130, 64)]          # pings x range; the third is smaller than the patch
SMALL = 1 << 19


def make_arrays(n_pings, n_range, seed):
    """sv [4, pings, range] linear with NaN / Inf, raw labels [pings, range] int16 (sandeel 27, other 1, ignored and
    negative ids), seabed [pings]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sv = np.power(10.0, rng.uniform(-8.5, 0.5, size=(4, n_pings, n_range))).astype(np.float32)
    sv[0][rng.random((n_pings, n_range)) < 0.01] = np.nan
    sv[2][rng.random((n_pings, n_range)) < 0.01] = np.inf
    labels = np.zeros((n_pings, n_range), dtype=np.int16)
    for val in (27, -1, 1, -100, 12, 1):
        w, h = max(1, n_pings // 5), max(1, n_range // 4)
        x0, y0 = int(rng.integers(0, n_pings - w + 1)), int(rng.integers(0, n_range - h + 1))
        labels[x0:x0 + w, y0:y0 + h] = val
    seabed = (0.6 * n_range + 0.25 * n_range * np.sin(np.arange(n_pings) / 11.0 + seed)).astype(np.int64)
    return sv, labels, np.clip(seabed, 1, n_range + 3)


@pytest.fixture(scope="module")
def echograms():
    out = []
    for i, (n_pings, n_range) in enumerate(EXTENTS):
        sv, labels, seabed = make_arrays(n_pings, n_range, seed=10 + i)
        out.append(FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), seabed,
                                frequencies=FREQS, name=f"eg{i}"))
    return out


def test_evaluate_echograms_memm_packed_with_classes(echograms, stub_pipe):
    stats = {}

    def packed(**kw):
        return ti.evaluate_echograms_memm(iter(echograms), stub_pipe, (32, 32), 4, 8, predict_fn=stub_pipe.fn,
                                          group_elems=SMALL, stats=stats, **kw)
    hp, hn = check_flow(packed)
    assert stats["groups"] >= 1 and stats["fallback_echograms"] == stats["solo_echograms"] == 0
    lp = ln = 0                        # the loop over the per-echogram call
    for eg in echograms:
        a, b = ti.evaluate_echogram_memm(eg, stub_pipe, (32, 32), 4, 8, predict_fn=stub_pipe.fn, classes=(1, 2))
        lp, ln = lp + a, ln + b
    assert np.array_equal(hp, lp) and np.array_equal(hn, ln)
    # a histogram handed in is accumulated into and must have the per-class form
    hist = torch.ones(3, 2, PR_BINS, dtype=torch.int32, device=DEV)
    assert packed(classes=(1, 2), hist=hist) is hist
    h = hist.cpu().numpy().astype(np.int64) - 1
    assert np.array_equal(h[1:, 0], hp) and np.array_equal(h[1:, 1], hn) and not h[0].any()
    with pytest.raises(ValueError, match="hist"):
        packed(classes=(1, 2), hist=torch.zeros(2, PR_BINS, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError, match="classes"):
        packed(classe=(1, 2))
    ti.release_staging()


def test_evaluate_echograms_memm_each_alone_with_classes(echograms):
    """A model with metadata input channels takes the per-echogram leg (``each_alone``)."""
    mc = {k: True for k in ti.META_FLAGS}
    pipe = make_pipe(pkg.UNet_Baseline(3, 11, start_filts=64, precision="f32x6"))
    egs = []
    for i in (3, 1):
        src = echograms[i]
        n_pings = src.shape[1]
        tv = 737000.5 + np.cumsum(np.random.Generator(np.random.PCG64(50 + i)).uniform(5e-6, 9e-6, size=n_pings))
        eg = FakeEchogram(src.sv, src.labels, src._seabed, frequencies=FREQS, name=src.name)
        eg.portion_of_day_vector, eg.portion_of_year_scalar = tv % 1, 0.61
        eg.time_vector_diff = np.concatenate((np.diff(tv), [tv[-1] - tv[-2]])) / 6e-6 - 1
        egs.append(eg)
    stats = {}
    check_flow(lambda **kw: ti.evaluate_echograms_memm(iter(egs), pipe, (64, 64), 6, 4, predict_fn=pipe.fn,
                                                       meta_channels=mc, stats=stats, **kw))
    assert stats["fallback_echograms"] == len(egs) and stats["groups"] == 0
