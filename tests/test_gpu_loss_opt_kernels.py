"""The scalar kernels that close every training step and every validation pass, against float64 references at their edges:
crimac_wce_fwd / crimac_wce_bwd (weighted cross entropy), crimac_softmax_nchw, crimac_pr_histogram, crimac_sgd_momentum,
crimac_grad_overflow_flag and crimac_sgd_momentum_guarded.

The case builders, the float64 references and the comparison functions below are plain numpy on the CPU (importing this
module needs no GPU); tests/test_loss_opt_reference_cpu.py checks the references against torch in float64, the
preconditions of the histogram inputs, and that every comparison function rejects a numpy emulation of a plausibly wrong
kernel.  Only the test bodies touch the GPU.  Each comparison function returns (and each test prints) the largest
observed error as a fraction of its bound.

Tolerances are bounds derived from fp32 arithmetic, eps = 2^-24 (one rounding to nearest: |fl(x) - x| <= eps |x|); none is
fitted to what the kernels give:

  * wce_fwd: per pixel nll = (mx + logf(den)) - z_y with den = sum expf(z_o - mx) in [1, ncls]: one rounding each of
    mx + logf(den) and of the subtraction, 1-ulp expf / logf, one rounding of w_y * nll; the pixels are summed in fp64:
        |sums[0] - ref| <= sum_pixels w_y * 4 eps (|max z| + |z_y| + 2),     |sums[1] - ref| <= 2^-50 npix max w
    (the weights are small integers, so sums[1] is in fact exact in any order).
  * wce_bwd: dl = k (e_o / den - onehot), k = w_y * (upstream / (float)sums[1]): elementwise |dl - ref| <= 8 eps |k|
    (|softmax - onehot| <= 1; three roundings in k, 1-ulp expf, the roundings of den, the division, the subtraction and the
    product).  Ignored pixels: +0.0 bit for bit in every class plane.
  * softmax_nchw: |out - ref| <= eps (|z_o - max z| + 4) ref + 2^-149 (the rounded argument of expf moves it by
    eps |z_o - mx| relative; expf, den and the division share the 4; 2^-149 is the smallest fp32 subnormal).  The 4 is what
    independent roundings add up to, not the worst case (2 for a 1-ulp expf, < 3 for the expf errors inside den, ncls - 1
    additions and the division: ncls + 5): a faithful fp32 emulation reaches 0.98 of this bound on the CPU.
  * pr_histogram: exact -- the inputs put every probability within 0.01 bin spacings of a chosen float16 value.
  * SGD: v' = m v + g s, p' = p - lr v' with or without FMA contraction:
        |v' - ref| <= 2 eps (|m v| + |g s|),      |p' - ref| <= eps |p| + lr bound(v') + 2 eps lr |v'|.

Largest error / bound over all cases on an MI355X: wce_fwd 0.03 (the bound adds the pixels' worst cases, the errors cancel),
wce_bwd 0.51, softmax_nchw 0.93, SGD velocity 0.65 and parameter 0.998 (a sharp bound: half-ulp roundings of p are met among
4 M elements).

Paths (elementwise.hip, tiling.hip) and the cases that reach them:
  * wce_fwd four-pixels-per-thread path (HW % 4 == 0, 16-byte aligned base): 2x16x16 in one workgroup, 1x64x64 with two
    grid-stride iterations, 1x1025x1024 at the 512-workgroup cap; one-pixel path: 3x5x7 (odd HW, thread ranges straddle
    images), 5x33x31 (with a loop), 2x16x16 on a base offset by one float (alignment alone);
  * wce_bwd / softmax_nchw beyond 256 workgroups (the whole-rounds grid): 1x1025x1024 and 1x513x512;
  * pr_histogram: every bin 0 .. 0x3C00 with label 1 and with label 0 / 2, the four skipped ids, the -50 rule, three label
    widths, ncls 2, 3, 4, 8, guard words, accumulation, and 3x419x419 > 2048 * 256 pixels (two grid-stride iterations);
  * SGD family: n = 1, 2, 3 (tail only), 4 (no tail), 5, 7, 1027 (one workgroup), 262147 (several, beyond 256 workgroups of
    1024 floats), 4194307 (the 2048-workgroup loop).

The planted +-88 pixel of the cross-entropy cases sits just INSIDE the range of expf (e^88 < FLT_MAX), so a kernel that
forgot the max subtraction would still be right there; the cases therefore also plant a +-100 pixel, which such a kernel
turns into inf (tests/test_loss_opt_reference_cpu.py shows both).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd.hip import call, ptr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
CLASS_W = (10.0, 300.0, 250.0, 1.0)
LABEL_DTYPES = {2: np.int16, 4: np.int32, 8: np.int64}
SENTINEL = -7.5
PR_BINS = hip.PR_BINS
ONE_BIN = 0x3C00                          # float16 1.0
SKIPPED = (-70, -30, -100, -10)
SEABED = -50
HIST_GUARD = 64
LR, MOM = 0.005, 0.95

# (B, H, W, base offset in floats)
CE_SMALL = [(2, 16, 16, 0), (1, 64, 64, 0), (3, 5, 7, 0), (5, 33, 31, 0), (2, 16, 16, 1)]
CE_BIG = (1, 1025, 1024, 0)
SOFTMAX_BIG = (1, 513, 512, 0)
SGD_NS = [1, 2, 3, 4, 5, 7, 1027, 262147, 2097152 * 2 + 3]
HIST_SHAPE, HIST_BIG_SHAPE = (2, 125, 125), (3, 419, 419)


def _seed(*key):
    s = 23
    for k in key:
        s = (s * 1000003 + int(k) + 1000) % (2 ** 31 - 1)
    return s


def _frac(err, bound):
    """max err / bound over the elements with a positive bound (a zero bound demands err == 0, asserted by the caller)."""
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


# ---- weighted cross entropy and softmax: cases, float64 references, comparisons (CPU only) -----------------------------------

def softmax64(z, axis=1):
    z = np.asarray(z, dtype=np.float64)
    mx = z.max(axis, keepdims=True)
    e = np.exp(z - mx)
    return e / e.sum(axis, keepdims=True)


@functools.lru_cache(maxsize=None)
def ce_case(B, H, W, ncls, ignore=-100, last_valid=False, neg_inf=True):
    """Logits (Gaussian, scale 3) with planted pixels, labels with ~10 % (and one whole image, when B >= 2) ignored, and
    the float64 reference of crimac_wce_fwd on them.  The planted pixels are the first ones of the last image."""
    rng = np.random.default_rng(_seed(1, B, H, W, ncls, ignore, last_valid, neg_inf))
    z = (3.0 * rng.standard_normal((B, ncls, H, W))).astype(np.float32)
    y = rng.integers(0, ncls, (B, H, W)).astype(np.int64)
    y[rng.random((B, H, W)) < 0.1] = ignore
    if B >= 2:
        y[(B - 1) // 2] = ignore
    zl, yl = z[B - 1].reshape(ncls, -1), y[B - 1].reshape(-1)        # (views)
    zl[:, 0], yl[0] = 1.5, 0                                          # all classes equal
    zl[:, 1], zl[ncls - 1, 1], yl[1] = -88.0, 88.0, ncls - 1          # one class at +88, the rest at -88: nll = 0 ...
    zl[:, 2], zl[0, 2], yl[2] = -88.0, 88.0, 1                        # ... and nll = 176
    zl[1, 3], yl[3] = -88.0, 1                                        # the label's class at -88: a large nll
    yl[4] = 0
    if neg_inf:
        zl[1, 4] = -np.inf                                            # a non-label class at -inf
    zl[:, 5], zl[0, 5], yl[5] = -100.0, 100.0, 0                      # beyond the range of expf without the max subtraction
    zl[:, 6], zl[0, 6], yl[6] = -100.0, 100.0, 1
    yl[-1] = int(rng.integers(0, ncls)) if last_valid else ignore     # the last pixel of the tensor
    w = np.array(CLASS_W[:ncls], dtype=np.float32)
    c = SimpleNamespace(B=B, H=H, W=W, ncls=ncls, ignore=ignore, z=z, y=y, w=w, npix=B * H * W)
    zt = np.moveaxis(z.astype(np.float64), 1, -1).reshape(-1, ncls)
    yf = y.reshape(-1)
    c.valid = yf != ignore
    yy = np.where(c.valid, yf, 0)
    mx = zt.max(1)
    with np.errstate(divide="ignore"):
        lse = mx + np.log(np.exp(zt - mx[:, None]).sum(1))
    zy = zt[np.arange(c.npix), yy]
    c.wy = np.where(c.valid, w.astype(np.float64)[yy], 0.0)          # w_y per pixel, 0 where ignored
    c.yy = yy
    c.nll = lse - zy
    c.s0 = math.fsum((c.wy * c.nll)[c.valid])
    c.s1 = math.fsum(c.wy)
    c.bound0 = math.fsum((c.wy * 4 * EPS * (np.abs(mx) + np.abs(zy) + 2))[c.valid])
    c.bound1 = 2.0 ** -50 * c.npix * float(w.max())
    c.soft = np.moveaxis(softmax64(zt, 1).reshape(B, H, W, ncls), -1, 1)
    for a in (z, y, c.valid, c.wy, c.nll, c.soft):
        a.setflags(write=False)                                       # shared among tests: left unchanged
    return c


def ce_grad_reference(c, upstream):
    """(dlogits [B][ncls][H][W] float64, k = upstream w_y / sum w per pixel [B][1][H][W]); exactly 0 where ignored."""
    k = (float(np.float32(upstream)) * c.wy / c.s1).reshape(c.B, 1, c.H, c.W)
    onehot = np.zeros((c.npix, c.ncls))
    onehot[np.arange(c.npix), c.yy] = 1.0
    onehot = np.moveaxis(onehot.reshape(c.B, c.H, c.W, c.ncls), -1, 1)
    return k * (c.soft - onehot), k


def check_ce_sums(sums, c, times=1):
    """sums: the two float64 accumulators after `times` calls of crimac_wce_fwd on a zeroed buffer."""
    e0, e1 = abs(float(sums[0]) - times * c.s0), abs(float(sums[1]) - times * c.s1)
    b0, b1 = times * c.bound0, times * c.bound1
    msg = (f"wce_fwd B={c.B} {c.H}x{c.W} ncls={c.ncls}: |sums[0] - ref| = {e0:.3e} (bound {b0:.3e}, ref {times * c.s0:.9e}), "
           f"|sums[1] - ref| = {e1:.3e} (bound {b1:.3e}, ref {times * c.s1:.9e})")
    assert e0 <= b0 and e1 <= b1, msg            # (a NaN fails both)
    return e0 / b0


def check_ce_grad(dl, c, upstream):
    """dl: crimac_wce_bwd's output (float32, pre-filled with SENTINEL by the caller)."""
    dl = np.ascontiguousarray(dl, dtype=np.float32)
    ref, k = ce_grad_reference(c, upstream)
    ign = np.broadcast_to(~c.valid.reshape(c.B, 1, c.H, c.W), dl.shape)
    bits = dl.view(np.uint32)
    assert (bits[ign] == 0).all(), (f"wce_bwd: {int((bits[ign] != 0).sum())} values at ignored pixels are not +0.0 "
                                    f"(first: {dl[ign][bits[ign] != 0][:4]})")
    err = np.abs(dl.astype(np.float64) - ref)
    bound = np.broadcast_to(8 * EPS * np.abs(k), dl.shape)
    bad = ~(err <= bound) & ~ign                 # (NaN counts as bad)
    frac = _frac(err[~ign], bound[~ign])
    assert not bad.any(), (f"wce_bwd B={c.B} {c.H}x{c.W} ncls={c.ncls} upstream={upstream}: {int(bad.sum())} elements beyond "
                           f"8 eps |k|; largest error / bound = {frac:.3f}")
    return frac


def check_softmax(out, z):
    """out: crimac_softmax_nchw's output (pre-filled with NaN by the caller) on logits z [B][ncls][H][W]."""
    out = np.asarray(out)
    assert not np.isnan(out).any(), f"softmax_nchw: {int(np.isnan(out).sum())} NaN left"
    z64 = z.astype(np.float64)
    ref = softmax64(z64, 1)
    bound = EPS * (np.abs(z64 - z64.max(1, keepdims=True)) + 4) * ref + 2.0 ** -149
    err = np.abs(out.astype(np.float64) - ref)
    frac = _frac(err, bound)
    assert (err <= bound).all(), (f"softmax_nchw {z.shape}: {int((err > bound).sum())} elements beyond the bound; largest "
                                  f"error / bound = {frac:.3f}")
    return frac


# ---- PR histogram --------------------------------------------------------------------------------------------------------

def half_of_bits(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)


def logit_for_bin(bits, ncls):
    """z_1 (fp32; every other class 0) whose softmax probability rounds to the float16 with this bit pattern."""
    bits = np.asarray(bits, dtype=np.int64)
    h = half_of_bits(np.clip(bits, 1, ONE_BIN - 1))
    z1 = np.log((ncls - 1) * h / (1 - h)).astype(np.float32)
    return np.where(bits == 0, np.float32(-200.0), np.where(bits == ONE_BIN, np.float32(200.0), z1)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def hist_case(ncls, lbytes, shape=HIST_SHAPE):
    """Pixels in a random order: every bin 0 .. 0x3C00 with label 1 and with label 0 / 2, each of the skipped ids and -50
    at several bins, the rest of the shape filled by cycling the bins with labels of every kind."""
    B, H, W = shape
    npix = B * H * W
    rng = np.random.default_rng(_seed(2, ncls, lbytes, *shape))
    every = np.arange(ONE_BIN + 1)
    special_bins = np.array([0, 1, 0x1234, 0x3800, 0x3BFF, ONE_BIN])
    bins = [every, every] + [special_bins] * 5
    labs = [np.ones_like(every), np.where(every % 2 == 0, 0, 2)] + [np.full(6, l) for l in SKIPPED + (SEABED,)]
    bins, labs = np.concatenate(bins), np.concatenate(labs)
    fill = npix - len(bins)
    assert fill >= 0 and (H * W) % 2 == 1
    kinds = np.array((0, 1, 2, 1, 0, 1) + SKIPPED + (SEABED,))
    bins = np.concatenate([bins, (np.arange(fill) * 7) % (ONE_BIN + 1)])
    labs = np.concatenate([labs, kinds[rng.integers(0, len(kinds), fill)]])
    perm = rng.permutation(npix)
    bins, labs = bins[perm], labs[perm]
    z = np.zeros((B, ncls, H, W), dtype=np.float32)
    z[:, 1] = logit_for_bin(bins, ncls).reshape(B, H, W)
    c = SimpleNamespace(B=B, H=H, W=W, ncls=ncls, z=z, labels=labs.reshape(B, H, W).astype(LABEL_DTYPES[lbytes]),
                        bins=bins, npix=npix)
    c.pos, c.neg = hist_reference(z, c.labels)
    for a in (z, c.labels, c.pos, c.neg):
        a.setflags(write=False)
    return c


def hist_reference(z, labels):
    """(hist_pos, hist_neg): the bin is the bit pattern of float16(softmax64(z)[1]); labels -70 / -30 / -100 / -10 are
    skipped, -50 counts as probability 0 in hist_neg, label 1 goes to hist_pos, every other label to hist_neg."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    prob = softmax64(z, 1)[:, 1].reshape(-1)
    prob = np.where(lab == SEABED, 0.0, prob)
    bits = prob.astype(np.float16).view(np.uint16).astype(np.int64)
    keep = ~np.isin(lab, SKIPPED)
    pos = keep & (lab == 1)
    return (np.bincount(bits[pos], minlength=PR_BINS).astype(np.int64),
            np.bincount(bits[keep & ~pos], minlength=PR_BINS).astype(np.int64))


def hist_buffer(prefill=None):
    """int64 host image of [guard | hist_pos | guard | hist_neg | guard] (the device buffer holds it as uint32 words)."""
    buf = np.zeros(3 * HIST_GUARD + 2 * PR_BINS, dtype=np.int64)
    if prefill is not None:
        buf[HIST_GUARD:HIST_GUARD + PR_BINS] = prefill[0]
        buf[2 * HIST_GUARD + PR_BINS:2 * HIST_GUARD + 2 * PR_BINS] = prefill[1]
    return buf


def check_hist(buf, pos, neg, prefill=None):
    """buf: the whole buffer after the call(s); pos / neg: what the calls must have added to `prefill`."""
    want = hist_buffer(prefill)
    want[HIST_GUARD:HIST_GUARD + PR_BINS] += pos
    want[2 * HIST_GUARD + PR_BINS:2 * HIST_GUARD + 2 * PR_BINS] += neg
    buf = np.asarray(buf, dtype=np.int64)
    guards = np.r_[buf[:HIST_GUARD], buf[HIST_GUARD + PR_BINS:2 * HIST_GUARD + PR_BINS], buf[2 * HIST_GUARD + 2 * PR_BINS:]]
    assert not guards.any(), "pr_histogram wrote outside its 16384 bins"
    diff = np.flatnonzero(buf != want)
    assert diff.size == 0, (f"pr_histogram: {diff.size} bins differ; first at buffer word {diff[0]} "
                            f"(got {buf[diff[0]]}, want {want[diff[0]]})")


# ---- SGD with momentum and the overflow guard --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sgd_case(n):
    rng = np.random.default_rng(_seed(3, n))
    p, g, v = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    for a in (p, g, v):
        a.setflags(write=False)
    return p, g, v


def sgd_reference(p, g, v, lr, mom, scale):
    """float64 v' = m v + g s, p' = p - lr v' on the fp32 values the kernel is handed, and the two elementwise bounds."""
    lr, mom, scale = (float(np.float32(x)) for x in (lr, mom, scale))
    p, g, v = (np.asarray(a, dtype=np.float64) for a in (p, g, v))
    v1 = mom * v + g * scale
    p1 = p - lr * v1
    bv = 2 * EPS * (np.abs(mom * v) + np.abs(g * scale))
    bp = EPS * np.abs(p) + lr * bv + 2 * EPS * lr * np.abs(v1)
    return SimpleNamespace(p=p1, v=v1, bv=bv, bp=bp)


def check_sgd(p1, v1, g1, ref, g0, zero_grad):
    """p1, v1, g1: the three buffers after one crimac_sgd_momentum call; g0: the gradient before it."""
    ev, ep = np.abs(v1.astype(np.float64) - ref.v), np.abs(p1.astype(np.float64) - ref.p)
    fv, fp = _frac(ev, ref.bv), _frac(ep, ref.bp)
    assert (ev <= ref.bv).all(), f"sgd n={len(g0)}: {int((~(ev <= ref.bv)).sum())} velocities beyond the bound (x{fv:.3f})"
    assert (ep <= ref.bp).all(), f"sgd n={len(g0)}: {int((~(ep <= ref.bp)).sum())} parameters beyond the bound (x{fp:.3f})"
    if zero_grad:
        assert not g1.view(np.uint32).any(), "sgd: zero_grad = 1 must leave g exactly +0.0"
    else:
        assert np.array_equal(g1.view(np.uint32), g0.view(np.uint32)), "sgd: zero_grad = 0 must leave g bit-unchanged"
    return fv, fp


def check_guard_state(state, flag, skipped):
    assert list(map(int, state)) == [flag, skipped], f"guard state {list(map(int, state))}, want {[flag, skipped]}"


def overflow_positions(n):
    """Element 0, the last element of the vector body, every tail element, and mid-buffer."""
    body = 4 * (n // 4)
    return sorted({0, n // 2, *([body - 1] if body else []), *range(body, n)})


def finite_extremes(g):
    """A finite gradient holding +-FLT_MAX and subnormals."""
    g = g.copy()
    vals = np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, 1e-45, -1e-45, 1e-39], dtype=np.float32)
    idx = np.linspace(0, len(g) - 1, num=min(len(g), len(vals))).astype(np.int64)
    g[idx] = vals[:len(idx)]
    g[-1] = vals[len(g) % 2]                     # (the last tail element too)
    return g


# ---- GPU tests -----------------------------------------------------------------------------------------------------------

def _dev(a):
    return torch.tensor(np.asarray(a)).cuda()             # (a copy: the cases are read-only)


def _dev_offset(a, off):
    """A device copy of `a` that starts `off` elements into a larger allocation -> (keep-alive buffer, view)."""
    flat = torch.tensor(np.asarray(a)).reshape(-1)
    buf = torch.zeros(flat.numel() + 8, dtype=flat.dtype, device="cuda")
    buf[off:off + flat.numel()] = flat.cuda()
    return buf, buf[off:off + flat.numel()]


IGNORES = [(-100, False), (-1, True)]             # (ignore_index, the last pixel of the tensor is valid)
CE_PARAMS = [(shape, ncls, lb, *ign) for shape in CE_SMALL for ncls in (2, 3, 4) for lb in (2, 4, 8) for ign in IGNORES]
CE_PARAMS.append((CE_BIG, 3, 2, *IGNORES[0]))     # the big shape runs once
CE_IDS = [f"{'x'.join(map(str, s[:3]))}+{s[3]}-ncls{n}-int{8 * lb}-ign{-ig}" for s, n, lb, ig, _ in CE_PARAMS]


def _ce_inputs(shape, ncls, lb, ignore, last_valid):
    B, H, W, off = shape
    c = ce_case(B, H, W, ncls, ignore, last_valid)
    keep, zd = _dev_offset(c.z, off)
    assert zd.data_ptr() % 16 == 4 * off
    return c, keep, zd, _dev(c.y.astype(LABEL_DTYPES[lb])), _dev(c.w)


@pytest.mark.parametrize("shape,ncls,lb,ignore,last_valid", CE_PARAMS, ids=CE_IDS)
def test_wce_fwd(shape, ncls, lb, ignore, last_valid):
    c,_keep, zd, yd, wd = _ce_inputs(shape, ncls, lb, ignore, last_valid)
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    args = (ptr(zd), ptr(yd), lb, ptr(wd), ncls, ignore, c.B, c.H, c.W, ptr(sums))
    call("crimac_wce_fwd", *args)
    once = sums.cpu().numpy()
    call("crimac_wce_fwd", *args)                 # accumulates
    twice = sums.cpu().numpy()
    f1, f2 = check_ce_sums(once, c), check_ce_sums(twice, c, times=2)
    print(f"wce_fwd error/bound {max(f1, f2):.4f}")


@pytest.mark.parametrize("shape,ncls,lb,ignore,last_valid", CE_PARAMS, ids=CE_IDS)
def test_wce_bwd(shape, ncls, lb, ignore, last_valid):
    c,_keep, zd, yd, wd = _ce_inputs(shape, ncls, lb, ignore, last_valid)
    sums = _dev(np.array([c.s0, c.s1]))
    for upstream in (1.0, 65536.0):
        dl = torch.full((c.B, ncls, c.H, c.W), SENTINEL, dtype=torch.float32, device="cuda")
        call("crimac_wce_bwd", ptr(zd), ptr(yd), lb, ptr(wd), ncls, ignore, c.B, c.H, c.W, ptr(sums), upstream, ptr(dl))
        print(f"wce_bwd error/bound {check_ce_grad(dl.cpu().numpy(), c, upstream):.4f}")


@pytest.mark.parametrize("ncls", [2, 3, 4])
@pytest.mark.parametrize("shape", CE_SMALL + [SOFTMAX_BIG], ids=lambda s: f"{'x'.join(map(str, s[:3]))}+{s[3]}")
def test_softmax_nchw(shape, ncls):
    B, H, W, off = shape
    c = ce_case(B, H, W, ncls, -100, True, neg_inf=False)
    _keep, zd = _dev_offset(c.z, off)
    out = torch.full((B, ncls, H, W), float("nan"), dtype=torch.float32, device="cuda")
    call("crimac_softmax_nchw", ptr(zd), ptr(out), B, ncls, H, W)
    print(f"softmax_nchw error/bound {check_softmax(out.cpu().numpy(), c.z):.4f}")


def _run_hist(c, lbytes, buf):
    zd, ld = _dev(c.z), _dev(c.labels)
    assert c.labels.itemsize == lbytes
    call("crimac_pr_histogram", ptr(zd), c.ncls, ptr(ld), lbytes, c.B, c.H, c.W, ptr(buf, HIST_GUARD),
         ptr(buf, 2 * HIST_GUARD + PR_BINS))
    return buf.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("lbytes", [2, 4, 8])
@pytest.mark.parametrize("ncls", [2, 3, 4, 8])
def test_pr_histogram_places_every_bin(ncls, lbytes):
    c = hist_case(ncls, lbytes)
    buf = torch.zeros(3 * HIST_GUARD + 2 * PR_BINS, dtype=torch.int32, device="cuda")
    check_hist(_run_hist(c, lbytes, buf), c.pos, c.neg)


def test_pr_histogram_accumulates_onto_a_prefilled_histogram():
    c = hist_case(3, 2)
    rng = np.random.default_rng(5)
    pre = rng.integers(0, 1000, (2, PR_BINS))
    buf = torch.from_numpy(hist_buffer(pre).astype(np.int32)).cuda()
    check_hist(_run_hist(c, 2, buf), c.pos, c.neg, pre)
    check_hist(_run_hist(c, 2, buf), 2 * c.pos, 2 * c.neg, pre)


def test_pr_histogram_grid_stride_loop():
    c = hist_case(3, 2, HIST_BIG_SHAPE)
    assert c.npix > 2048 * 256
    buf = torch.zeros(3 * HIST_GUARD + 2 * PR_BINS, dtype=torch.int32, device="cuda")
    check_hist(_run_hist(c, 2, buf), c.pos, c.neg)


SGD_VARIANTS = [(MOM, 1.0, 1), (MOM, 1.0, 0), (0.0, 1.0, 1), (MOM, 2.0 ** -16, 1)]


@pytest.mark.parametrize("n", SGD_NS)
def test_sgd_momentum(n):
    p0, g0, v0 = sgd_case(n)
    for mom, scale, zero_grad in SGD_VARIANTS:
        p, g, v = _dev(p0), _dev(g0), _dev(v0)
        call("crimac_sgd_momentum", ptr(p), ptr(g), ptr(v), n, LR, mom, scale, zero_grad)
        fv, fp = check_sgd(p.cpu().numpy(), v.cpu().numpy(), g.cpu().numpy(), sgd_reference(p0, g0, v0, LR, mom, scale), g0,
                           zero_grad)
        print(f"sgd_momentum m={mom} s={scale}: v error/bound {fv:.4f}, p error/bound {fp:.4f}")


def test_sgd_family_refuses_misaligned_buffers_and_empty_input():
    n = 16
    bufs = [torch.zeros(n + 4, device="cuda") for _ in range(3)]
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    for bad in range(3):
        args = [ptr(b, 1 if i == bad else 0) for i, b in enumerate(bufs)]
        with pytest.raises(hip.HipLibraryError):
            call("crimac_sgd_momentum", *args, n, LR, MOM, 1.0, 1)
        with pytest.raises(hip.HipLibraryError):
            call("crimac_sgd_momentum_guarded", *args, n, LR, MOM, 1.0, 1, ptr(state))
    with pytest.raises(hip.HipLibraryError):
        call("crimac_grad_overflow_flag", ptr(bufs[1], 1), n, ptr(state))
    args = [ptr(b) for b in bufs]
    with pytest.raises(hip.HipLibraryError):
        call("crimac_sgd_momentum", *args, 0, LR, MOM, 1.0, 1)
    with pytest.raises(hip.HipLibraryError):
        call("crimac_sgd_momentum_guarded", *args, 0, LR, MOM, 1.0, 1, ptr(state))
    with pytest.raises(hip.HipLibraryError):
        call("crimac_grad_overflow_flag", ptr(bufs[1]), 0, ptr(state))
    torch.cuda.synchronize()
    assert all(float(b.abs().max()) == 0 for b in bufs) and not state.any()


@pytest.mark.parametrize("n", SGD_NS)
def test_grad_overflow_flag(n):
    g = _dev(finite_extremes(sgd_case(n)[1]))
    bads = [float("inf"), float("-inf"), float("nan")]
    pos = overflow_positions(n)
    # one state row per launch, read back once: rows 0 / 1 the finite gradient on a clear / a set flag
    states = torch.zeros(2 + len(pos) * len(bads), 2, dtype=torch.int32, device="cuda")
    states[:, 1] = 5
    states[1, 0] = 1
    call("crimac_grad_overflow_flag", ptr(g), n, ptr(states[0]))
    call("crimac_grad_overflow_flag", ptr(g), n, ptr(states[1]))
    row = 2
    for i in pos:
        keep = g[i].clone()
        for bad in bads:
            g[i] = bad
            call("crimac_grad_overflow_flag", ptr(g), n, ptr(states[row]))
            row += 1
        g[i] = keep
    got = states.cpu().numpy()
    check_guard_state(got[0], 0, 5)               # +-FLT_MAX and subnormals are finite
    check_guard_state(got[1], 1, 5)               # the kernel only ORs
    for r in range(2, len(got)):
        assert list(got[r]) == [1, 5], f"n={n}: {bads[(r - 2) % 3]} at element {pos[(r - 2) // 3]} -> state {list(got[r])}"


@pytest.mark.parametrize("n", SGD_NS)
def test_sgd_momentum_guarded(n):
    p0, g0, v0 = sgd_case(n)
    for zero_grad in (1, 0):
        p, g, v = _dev(p0), _dev(g0), _dev(v0)
        call("crimac_sgd_momentum", ptr(p), ptr(g), ptr(v), n, LR, MOM, 1.0, zero_grad)
        pg, gg, vg = _dev(p0), _dev(g0), _dev(v0)
        state = torch.tensor([0, 5], dtype=torch.int32, device="cuda")
        call("crimac_sgd_momentum_guarded", ptr(pg), ptr(gg), ptr(vg), n, LR, MOM, 1.0, zero_grad, ptr(state))
        for a, b in ((p, pg), (g, gg), (v, vg)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))       # clear flag: the unguarded step, bit for bit
        check_guard_state(state.cpu().numpy(), 0, 5)
        ps, gs, vs = _dev(p0), _dev(g0), _dev(v0)
        state = torch.tensor([1, 5], dtype=torch.int32, device="cuda")
        call("crimac_sgd_momentum_guarded", ptr(ps), ptr(gs), ptr(vs), n, LR, MOM, 1.0, zero_grad, ptr(state))
        check_guard_state(state.cpu().numpy(), 1, 6)                            # one increment, however many workgroups ran
        for a, a0 in ((ps, p0), (vs, v0), (gs, g0)):                            # a skipped step leaves g too, also with zero_grad
            assert np.array_equal(a.cpu().numpy().view(np.uint32), a0.view(np.uint32))


def test_flag_then_guarded_skips_once_then_applies():
    n = 1027
    p0, g0, v0 = sgd_case(n)
    p, g, v = _dev(p0), _dev(g0), _dev(v0)
    g[n - 2] = float("inf")
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    call("crimac_grad_overflow_flag", ptr(g), n, ptr(state))
    call("crimac_sgd_momentum_guarded", ptr(p), ptr(g), ptr(v), n, LR, MOM, 1.0, 1, ptr(state))
    check_guard_state(state.cpu().numpy(), 1, 1)
    assert np.array_equal(p.cpu().numpy().view(np.uint32), p0.view(np.uint32))
    assert np.array_equal(v.cpu().numpy().view(np.uint32), v0.view(np.uint32))
    g[n - 2] = float(g0[n - 2])
    state[0] = 0
    call("crimac_grad_overflow_flag", ptr(g), n, ptr(state))
    call("crimac_sgd_momentum_guarded", ptr(p), ptr(g), ptr(v), n, LR, MOM, 1.0, 1, ptr(state))
    check_guard_state(state.cpu().numpy(), 0, 1)
    check_sgd(p.cpu().numpy(), v.cpu().numpy(), g.cpu().numpy(), sgd_reference(p0, g0, v0, LR, MOM, 1.0), g0, 1)
