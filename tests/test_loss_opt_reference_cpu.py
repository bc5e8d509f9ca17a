"""The CPU side of tests/test_gpu_loss_opt_kernels.py, run without a GPU:
  * its float64 references against torch in float64 (F.cross_entropy with autograd, torch.softmax, torch.optim.SGD) and
    against a direct numpy float16 count;
  * the preconditions of the histogram inputs (every probability within 0.01 bin spacings of its float16 target, every bin
    0 .. 0x3C00 hit with label 1 and with another label);
  * its comparison functions: each accepts a faithful fp32 numpy emulation of the kernel (so no bound is unattainable) and
    rejects an emulation of a plausibly wrong kernel (so no bound is vacuous)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_loss_opt_kernels as lo

SMALL = [(B, H, W, ncls, ign, lv) for B, H, W, _ in lo.CE_SMALL[:4] for ncls in (2, 3, 4) for ign, lv in lo.IGNORES]
f32 = np.float32


# ---- fp32 emulations of the kernels (and of wrong ones) ---------------------------------------------------------------------

def emu_pixels(c, no_max=False):
    """Per pixel, in fp32 as the kernels compute them: (e_o = expf(z_o - mx), den, nll)."""
    zt = np.moveaxis(c.z, 1, -1).reshape(-1, c.ncls)
    mx = np.zeros(c.npix, dtype=f32) if no_max else zt.max(1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(zt - mx[:, None])
        den = e[:, 0].copy()
        for o in range(1, c.ncls):
            den = den + e[:, o]
        nll = (mx + np.log(den)) - zt[np.arange(c.npix), c.yy]
    assert e.dtype == f32 and den.dtype == f32 and nll.dtype == f32
    return e, den, nll


def emu_wce_fwd(c, no_max=False, drop=0):
    _, _, nll = emu_pixels(c, no_max)
    wy = c.wy.astype(f32)
    keep = c.valid.copy()
    if drop:
        keep[-drop:] = False
    with np.errstate(invalid="ignore"):
        return np.array([(wy * nll).astype(np.float64)[keep].sum(), c.wy[keep].sum()])


def emu_wce_bwd(c, upstream, fill=0.0, twice=False):
    e, den, _ = emu_pixels(c)
    inv = f32(upstream) / f32(c.s1)
    k = c.wy.astype(f32) * inv * (f32(upstream) if twice else f32(1))
    onehot = np.zeros((c.npix, c.ncls), dtype=f32)
    onehot[np.arange(c.npix), c.yy] = 1
    dl = k[:, None] * (e / den[:, None] - onehot)
    dl[~c.valid] = fill
    return np.ascontiguousarray(np.moveaxis(dl.reshape(c.B, c.H, c.W, c.ncls), -1, 1))


def emu_softmax(z, dtype=f32):
    zt = z.astype(dtype)
    e = np.exp(zt - zt.max(1, keepdims=True))
    den = e[:, 0].copy()
    for o in range(1, z.shape[1]):
        den = den + e[:, o]
    return (e / den[:, None]).astype(f32)


def emu_hist(c, truncate=False, seabed="neg"):
    lab = c.labels.astype(np.int64).reshape(-1)
    prob = emu_softmax(c.z)[:, 1].reshape(-1)
    prob = np.where(lab == lo.SEABED, f32(0), prob)
    h = prob.astype(np.float16)
    if truncate:
        h = np.where(h.astype(f32) > prob, np.nextafter(h, np.float16(0)), h)
    bits = h.view(np.uint16).astype(np.int64)
    keep = ~np.isin(lab, lo.SKIPPED)
    pos = keep & (lab == 1)
    if seabed == "pos":
        pos |= lab == lo.SEABED
    elif seabed == "skip":
        keep &= lab != lo.SEABED
    buf = lo.hist_buffer()
    buf[lo.HIST_GUARD:lo.HIST_GUARD + lo.PR_BINS] = np.bincount(bits[pos], minlength=lo.PR_BINS)
    buf[2 * lo.HIST_GUARD + lo.PR_BINS:2 * lo.HIST_GUARD + 2 * lo.PR_BINS] = np.bincount(bits[keep & ~pos], minlength=lo.PR_BINS)
    return buf


def emu_sgd(p, g, v, lr, mom, scale, miss_tail=False, old_v=False):
    lr, mom, scale = f32(lr), f32(mom), f32(scale)
    v1 = mom * v + g * scale
    p1 = p - lr * (v if old_v else v1)
    assert v1.dtype == f32 and p1.dtype == f32
    if miss_tail:
        body = 4 * (len(p) // 4)
        v1[body:], p1[body:] = v[body:], p[body:]
    return p1, v1


# ---- the references ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,ncls,ignore,last_valid", SMALL)
def test_ce_reference_is_torch_cross_entropy_in_float64(B, H, W, ncls, ignore, last_valid):
    c = lo.ce_case(B, H, W, ncls, ignore, last_valid)
    assert bool(c.valid[-1]) == last_valid
    assert B < 2 or not c.valid.reshape(B, -1)[(B - 1) // 2].any()              # one whole image ignored
    assert 0.05 < 1 - c.valid.mean() < (0.2 if B < 2 else 0.2 + 1 / B)
    z = torch.tensor(c.z).double().requires_grad_(True)
    loss = F.cross_entropy(z, torch.tensor(c.y), weight=torch.tensor(c.w).double(), ignore_index=ignore)
    for upstream in (1.0, 65536.0):
        z.grad = None
        (loss * upstream).backward(retain_graph=True)
        ref, _ = lo.ce_grad_reference(c, upstream)
        assert np.allclose(ref, z.grad.numpy(), rtol=1e-12, atol=1e-300 + 1e-14 * upstream * float(c.w.max()) / c.s1)
        assert not ref[np.broadcast_to(~c.valid.reshape(B, 1, H, W), ref.shape)].any()
    assert abs(c.s0 / c.s1 - loss.item()) <= 1e-13 * abs(loss.item())
    assert c.s1 == float(c.w.astype(np.float64)[c.y[c.y != ignore]].sum())
    assert np.allclose(c.soft, torch.softmax(z.detach(), 1).numpy(), rtol=1e-13, atol=1e-300)


def test_hist_reference_is_a_direct_float16_count():
    for ncls, lb in ((2, 2), (3, 4), (8, 8)):
        c = lo.hist_case(ncls, lb)
        prob = torch.softmax(torch.tensor(c.z).double(), 1)[:, 1].numpy().reshape(-1)
        lab = c.labels.reshape(-1)
        pos, neg = np.zeros(lo.PR_BINS, dtype=np.int64), np.zeros(lo.PR_BINS, dtype=np.int64)
        for l, pr in zip(lab.tolist(), prob.tolist()):
            if l in lo.SKIPPED:
                continue
            b = int(np.float16(0.0 if l == lo.SEABED else pr).view(np.uint16))
            (pos if l == 1 else neg)[b] += 1
        assert np.array_equal(pos, c.pos) and np.array_equal(neg, c.neg)
        assert pos.sum() + neg.sum() == c.npix - np.isin(lab, lo.SKIPPED).sum()


def test_sgd_reference_is_three_steps_of_torch_sgd_in_float64():
    rng = np.random.default_rng(11)
    n = 1027
    p0 = rng.standard_normal(n).astype(f32)
    grads = [rng.standard_normal(n).astype(f32) for _ in range(3)]
    pt = torch.tensor(p0).double().requires_grad_(True)
    opt = torch.optim.SGD([pt], lr=float(f32(lo.LR)), momentum=float(f32(lo.MOM)))
    p, v = p0.astype(np.float64), np.zeros(n)
    for g in grads:
        pt.grad = torch.tensor(g).double()
        opt.step()
        r = lo.sgd_reference(p, g, v, lo.LR, lo.MOM, 1.0)
        p, v = r.p, r.v
    assert np.allclose(p, pt.detach().numpy(), rtol=1e-14, atol=1e-15)
    r = lo.sgd_reference(p0, grads[0], grads[1], lo.LR, 0.0, 2.0 ** -16)
    assert np.array_equal(r.v, grads[0].astype(np.float64) * 2.0 ** -16)


# ---- the preconditions of the histogram inputs ------------------------------------------------------------------------------

@pytest.mark.parametrize("ncls,lb,shape", [(n, lb, lo.HIST_SHAPE) for n in (2, 3, 4, 8) for lb in (2, 4, 8)]
                         + [(3, 2, lo.HIST_BIG_SHAPE)])
def test_histogram_inputs_sit_on_their_bins(ncls, lb, shape):
    c = lo.hist_case(ncls, lb, shape)
    assert (c.H * c.W) % 2 == 1 and c.labels.dtype.itemsize == lb
    prob = lo.softmax64(c.z, 1)[:, 1].reshape(-1)
    target = lo.half_of_bits(c.bins)
    below = lo.half_of_bits(np.maximum(c.bins, 1) - 1)
    spacing = np.where(c.bins == 0, lo.half_of_bits([1])[0], target - below)     # the gap to the lower neighbour: the smaller one
    assert (np.abs(prob - target) <= 0.01 * spacing).all(), float((np.abs(prob - target) / spacing).max())
    lab = c.labels.reshape(-1)
    every = np.arange(lo.ONE_BIN + 1)
    assert np.array_equal(np.unique(c.bins[lab == 1]), every)
    assert np.array_equal(np.unique(c.bins[(lab == 0) | (lab == 2)]), every)
    for l in lo.SKIPPED + (lo.SEABED,):
        assert len(np.unique(c.bins[lab == l])) >= 6
    # only the -50 pixels move (to bin 0 of hist_neg); nothing lands beyond 1.0
    assert c.pos[lo.ONE_BIN + 1:].sum() == 0 and c.neg[lo.ONE_BIN + 1:].sum() == 0
    assert np.array_equal(c.pos, np.bincount(c.bins[lab == 1], minlength=lo.PR_BINS))


# ---- the comparison functions accept the kernels' arithmetic ... ------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,ncls,ignore,last_valid", SMALL)
def test_faithful_fp32_cross_entropy_and_softmax_pass(B, H, W, ncls, ignore, last_valid):
    c = lo.ce_case(B, H, W, ncls, ignore, last_valid)
    assert lo.check_ce_sums(emu_wce_fwd(c), c) < 1
    assert lo.check_ce_sums(2 * emu_wce_fwd(c), c, times=2) < 1
    for upstream in (1.0, 65536.0):
        assert lo.check_ce_grad(emu_wce_bwd(c, upstream), c, upstream) <= 1
    s = lo.ce_case(B, H, W, ncls, -100, True, neg_inf=False)
    assert np.isfinite(s.z).all()
    assert lo.check_softmax(emu_softmax(s.z), s.z) <= 1


def test_faithful_fp32_histogram_and_sgd_pass():
    c = lo.hist_case(3, 2)
    lo.check_hist(emu_hist(c), c.pos, c.neg)
    for n in lo.SGD_NS[:8]:
        p, g, v = lo.sgd_case(n)
        for mom, scale, zero_grad in lo.SGD_VARIANTS:
            p1, v1 = emu_sgd(p, g, v, lo.LR, mom, scale)
            lo.check_sgd(p1, v1, np.zeros_like(g) if zero_grad else g.copy(), lo.sgd_reference(p, g, v, lo.LR, mom, scale), g,
                         zero_grad)


# ---- ... and reject wrong kernels ----------------------------------------------------------------------------------------------

def test_ce_without_max_subtraction_is_rejected():
    c = lo.ce_case(3, 5, 7, 3, -1, True)
    planted = (c.B - 1) * c.H * c.W + np.arange(7)
    _, _, good = emu_pixels(c)
    _, _, bad = emu_pixels(c, no_max=True)
    # e^88 < FLT_MAX: at the +-88 pixels the wrong kernel is still right (nll 0 and 176) ...
    assert np.array_equal(bad[planted[1:3]], good[planted[1:3]]) and list(good[planted[1:3]]) == [0.0, 176.0]
    # ... the +-100 pixels are what it gets wrong
    assert not np.isfinite(bad[planted[5:7]]).any() and list(good[planted[5:7]]) == [0.0, 200.0]
    with pytest.raises(AssertionError, match="wce_fwd"):
        lo.check_ce_sums(emu_wce_fwd(c, no_max=True), c)


def test_ce_that_drops_the_last_pixels_is_rejected():
    c = lo.ce_case(3, 5, 7, 3, -1, True)
    assert c.npix % 4 == 1 and c.valid[-1]
    with pytest.raises(AssertionError, match="wce_fwd"):
        lo.check_ce_sums(emu_wce_fwd(c, drop=c.npix % 4), c)


def test_ce_backward_wrong_kernels_are_rejected():
    c = lo.ce_case(3, 5, 7, 3, -100, False)
    with pytest.raises(AssertionError, match=r"not \+0.0"):
        lo.check_ce_grad(emu_wce_bwd(c, 1.0, fill=lo.SENTINEL), c, 1.0)
    with pytest.raises(AssertionError, match=r"not \+0.0"):
        lo.check_ce_grad(emu_wce_bwd(c, 1.0, fill=-0.0), c, 1.0)
    with pytest.raises(AssertionError, match="beyond"):
        lo.check_ce_grad(emu_wce_bwd(c, 65536.0, twice=True), c, 65536.0)
    dl = emu_wce_bwd(c, 1.0)
    dl[0, 0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        lo.check_ce_grad(dl, c, 1.0)


def test_softmax_in_float16_is_rejected():
    c = lo.ce_case(3, 5, 7, 3, -100, True, neg_inf=False)
    with pytest.raises(AssertionError, match="beyond"):
        lo.check_softmax(emu_softmax(c.z, np.float16), c.z)
    out = emu_softmax(c.z)
    out[-1, -1, -1, -1] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        lo.check_softmax(out, c.z)


def test_wrong_histograms_are_rejected():
    c = lo.hist_case(3, 2)
    for wrong in (dict(truncate=True), dict(seabed="pos"), dict(seabed="skip")):
        with pytest.raises(AssertionError, match="bins differ"):
            lo.check_hist(emu_hist(c, **wrong), c.pos, c.neg)
    buf = emu_hist(c)
    buf[lo.HIST_GUARD + lo.PR_BINS] = 1
    with pytest.raises(AssertionError, match="outside"):
        lo.check_hist(buf, c.pos, c.neg)


def test_wrong_sgd_steps_are_rejected():
    p, g, v = lo.sgd_case(1027)
    ref = lo.sgd_reference(p, g, v, lo.LR, lo.MOM, 1.0)
    for wrong in (dict(miss_tail=True), dict(old_v=True)):
        p1, v1 = emu_sgd(p, g, v, lo.LR, lo.MOM, 1.0, **wrong)
        with pytest.raises(AssertionError, match="beyond"):
            lo.check_sgd(p1, v1, np.zeros_like(g), ref, g, 1)
    p1, v1 = emu_sgd(p, g, v, lo.LR, lo.MOM, 1.0)
    with pytest.raises(AssertionError, match="zero_grad"):
        lo.check_sgd(p1, v1, g.copy(), ref, g, 1)
    with pytest.raises(AssertionError, match="zero_grad"):
        lo.check_sgd(p1, v1, np.zeros_like(g), ref, g, 0)


def test_a_guard_that_counts_once_per_workgroup_is_rejected():
    lo.check_guard_state([1, 6], 1, 6)
    with pytest.raises(AssertionError, match="guard state"):
        lo.check_guard_state([1, 5 + 2048], 1, 6)
    with pytest.raises(AssertionError, match="guard state"):
        lo.check_guard_state([0, 6], 1, 6)


def test_overflow_positions_cover_body_end_and_tail():
    assert lo.overflow_positions(1) == [0] and lo.overflow_positions(4) == [0, 2, 3]
    assert lo.overflow_positions(7) == [0, 3, 4, 5, 6] and lo.overflow_positions(1027) == [0, 513, 1023, 1024, 1025, 1026]
    for n in lo.SGD_NS[:7]:
        assert np.isfinite(lo.finite_extremes(lo.sgd_case(n)[1])).all()
    gx = lo.finite_extremes(lo.sgd_case(1027)[1])
    assert np.abs(gx).max() == np.finfo(f32).max and ((gx != 0) & (np.abs(gx) < np.finfo(f32).tiny)).any()
