"""crimac_head_meta_fwd and crimac_head_meta_bwd (csrc/meta.hip), each alone through the C ABI.  First the forward:

Acceptance bar: `torch.equal` with the three launches it replaces -- crimac_head_fwd on the packed 64 columns,
crimac_meta_mlp_fwd, crimac_meta_inject_fwd -- run in the same test on the same REAL-valued inputs, for every storage type
crimac_head_fwd takes for x (fp32, bf16, fp16, fp16 plane pairs; with the on-the-fly BatchNorm the h3p input is the fp32
conv output), Cm in {1, 3, 7, 8}, ncls in {2, 3, 4}, with and without BatchNorm, with and without softmax.

Shapes: one workgroup; a ragged one whose workgroups straddle images (HW = 768, B = 3: 2304 = 9 x 256 pixels, image
borders inside workgroups 3 and 6; and (3, 17, 19) = 969 pixels: ragged tail, HW no multiple of 8, so the 8-pixel lane
groups straddle images too); two images of two workgroups; and 1032 workgroups' worth of pixels over the grid cap of 1024,
so that eight workgroups take a second turn of the grid-stride loop with the perceptron's weights still in LDS.

The logits lie in front of a sentinel guard, every input between NaN guards (helpers of tests/test_gpu_meta_kernels.py).
crimac_head_meta_bwd: see the second half of this file.
"""
import functools
import re

import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd.hip import call, ptr
from test_gpu_h3p import hp_pack
from test_gpu_meta_kernels import (GUARD, LIMIT, OUTPUTS, SENTINEL, U, WKEYS, _mlp_weights, chain_length, dev_in, dev_out,
                                   exact_case, guard_untouched, real_case)

C = 64
GRID_CAP = 1024                                # workgroups of 256 pixels (head_meta_fwd_launch)
SHAPES = [(1, 16, 16), (3, 16, 48), (3, 17, 19), (2, 32, 16), (1, 516, 512)]
assert -(-SHAPES[-1][1] * SHAPES[-1][2] // 256) == GRID_CAP + 8
STORAGE = {"fp32": hip.PREC_F32X6, "bf16": hip.PREC_BF16, "fp16": hip.PREC_FP16, "pairs": hip.PREC_H3P}
ALL_PARAMS = [(cm, nc) for cm in (1, 3, 7, 8) for nc in (2, 3, 4)]
FEW_PARAMS = [(1, 2), (7, 3), (8, 4)]           # at the large shape


def _x_device(x, storage, bn):
    """x [npix, 64] fp32 (cpu) in the storage the precision reads: 16-bit, fp32, or plane pairs (h3p without BatchNorm)."""
    if storage == "bf16":
        return x.bfloat16().cuda()
    if storage == "fp16":
        return x.half().cuda()
    if storage == "pairs" and not bn:
        return hp_pack(x).cuda()
    return x.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_forward_equals_the_three_launches_bit_for_bit(shape, storage):
    B, H, W = shape
    npix = B * H * W
    prec = STORAGE[storage]
    g = torch.Generator().manual_seed(1000 * B + H + W)
    x = torch.randn(npix, C, generator=g)
    meta_all = torch.rand(B, 8, H, W, generator=g) * 1.5 - 0.25
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    runs = 0
    for cm, ncls in (FEW_PARAMS if npix > 100000 else ALL_PARAMS):
        p, _ = _mlp_weights(cm, 11 + cm)
        wfull = torch.randn(ncls, C + 1, generator=g) / 8
        bias = torch.randn(ncls, generator=g)
        meta = meta_all[:, :cm].contiguous()
        d_w = [dev_in(p[k]) for k in WKEYS]
        d_meta, d_wfull, d_bias = dev_in(meta), dev_in(wfull), dev_in(bias)
        d_w64, d_wm = dev_in(wfull[:, :C].contiguous()), dev_in(wfull[:, C].contiguous())
        d_scale, d_shift = dev_in(scale), dev_in(shift)
        for bn in (False, True):
            d_x = _x_device(x, storage, bn)
            bn_args = (ptr(d_scale), ptr(d_shift)) if bn else (None, None)
            for softmax in (0, 1):
                n = B * ncls * H * W
                # the chain: head on the packed columns (no softmax), perceptron into m, injection (+ softmax)
                want = dev_out(n, init=torch.full((n,), SENTINEL))
                m = dev_out(npix)
                call("crimac_head_fwd", prec, ptr(d_x), C, C, ptr(d_w64), ptr(d_bias), ptr(want), B, H, W, ncls, 0, *bn_args)
                call("crimac_meta_mlp_fwd", ptr(d_meta), cm, B, H, W, *[ptr(t) for t in d_w], ptr(m))
                call("crimac_meta_inject_fwd", ptr(m), ptr(d_wm), ptr(want), B, H, W, ncls, softmax)
                got = dev_out(n, init=torch.full((n,), SENTINEL))
                call("crimac_head_meta_fwd", prec, ptr(d_x), C, ptr(d_wfull), ptr(d_bias), ptr(d_meta), cm,
                     *[ptr(t) for t in d_w], ptr(got), B, H, W, ncls, softmax, *bn_args)
                torch.cuda.synchronize()
                what = f"Cm={cm} ncls={ncls} bn={bn} softmax={softmax}"
                assert bool(torch.isfinite(want[:n]).all()) and float(want[:n].abs().max()) > 0, what
                bad = torch.nonzero(got[:n] != want[:n]).flatten()
                assert bad.numel() == 0, (f"{what}: {bad.numel()} of {n} logits differ from the chain, first "
                                          f"{bad[:6].tolist()}: {got[bad[:6]].tolist()} vs {want[bad[:6]].tolist()}")
                assert guard_untouched(got, n), f"{what}: crimac_head_meta_fwd wrote behind the logits"
                runs += 1
    assert runs == 4 * (len(FEW_PARAMS) if npix > 100000 else len(ALL_PARAMS))


@pytest.mark.gpu
def test_a_pixel_does_not_depend_on_the_batch_around_it():
    """The same image alone and as image 5 of 7 (HW = 17 x 19: every lane group and workgroup boundary falls elsewhere)."""
    H, W, cm, ncls = 17, 19, 7, 3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(7, H * W, C, generator=g)
    meta = torch.rand(7, cm, H, W, generator=g)
    p, _ = _mlp_weights(cm, 18)
    wfull, bias = torch.randn(ncls, C + 1, generator=g) / 8, torch.randn(ncls, generator=g)
    d_w = [p[k].cuda() for k in WKEYS]
    outs = []
    for xs, ms in ((x[5:6], meta[5:6]), (x, meta)):
        B = xs.shape[0]
        out = torch.empty(B, ncls, H, W, device="cuda")
        d_x, d_m, d_wf, d_b = xs.reshape(-1, C).cuda(), ms.contiguous().cuda(), wfull.cuda(), bias.cuda()
        call("crimac_head_meta_fwd", hip.PREC_F32X6, ptr(d_x), C, ptr(d_wf), ptr(d_b), ptr(d_m), cm,
             *[ptr(t) for t in d_w], ptr(out), B, H, W, ncls, 1, None, None)
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0][0], outs[1][5])


def _refuses(text):
    return pytest.raises(hip.HipLibraryError, match=re.escape(text))


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_nothing_is_launched():
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")      # noqa: E731
    x, wf, b, meta, out = z(16, C), z(4, C + 1), z(4), z(1, 8, 4, 4), torch.full((1, 4, 4, 4), SENTINEL, device="cuda")
    w = [z(32, 8), z(32), z(32, 32), z(32), z(1, 32), z(1)]

    def run(cm=8, ncls=3, meta_p=ptr(meta), x_ld=C, prec=hip.PREC_F32X6):
        call("crimac_head_meta_fwd", prec, ptr(x), x_ld, ptr(wf), ptr(b), meta_p, cm, *[ptr(t) for t in w], ptr(out),
             1, 4, 4, ncls, 0, None, None)

    for cm in (0, 9):
        with _refuses(f"head_meta_fwd: {cm} metadata channels (1..8 supported)"):
            run(cm=cm)
    for ncls in (1, 5):
        with _refuses(f"head_meta_fwd: ncls={ncls} unsupported (2..4)"):
            run(ncls=ncls)
    with _refuses("head_meta_fwd: bad arguments"):
        run(meta_p=None)
    with _refuses("head_meta_fwd: bad pixel stride"):
        run(x_ld=60)
    with _refuses("head_meta_fwd: bad precision"):
        run(prec=hip.PREC_H3F_BWD)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    run()                                            # ... and the same arguments, valid, do launch
    torch.cuda.synchronize()
    assert bool((out[:, :3] == 0).all()) and bool((out[:, 3] == SENTINEL).all())


# ======================================================================================================================
# crimac_head_meta_bwd: one pass over dlogits
# ======================================================================================================================
# Float64 restatement: the perceptron part is test_gpu_meta_kernels.mlp_reference (checked there against autograd); the
# head part is written out here: da = dl . W[:, :64], dW[:, :64] = dl^T . act, db = sum dl, and the BatchNorm-backward
# sums of the block da feeds, sum dz and sum dz * xhat with dz = da where the activation is positive.
#
# EXACT cases: integer-valued fp32 data, every product and partial sum an integer below 2^24 (asserted on the CPU for
# every case), so every output must equal the restatement bit for bit in whatever order the kernel adds.  With the fused
# sums the BatchNorm vectors are mean 0, invstd 1, scale 1, shift 0 and x = NULL: the activation is rebuilt as relu(y)
# and xhat = y, integers too.
#
# REAL cases: |got - ref64| <= L * 2^-24 * sum|terms| with L the longest fp32 chain the launch geometry allows.  Geometry
# of head_meta_bwd_launch: grid = min(ceil(npix / 256), 512) workgroups, iters = ceil(npix / (256 * grid)) turns each.
#   perceptron gradients: 256 pixel terms per thread and turn, one atomic per workgroup, the 32-term dot product inside
#                         dh1: 256 * iters + grid + 32 (test_gpu_meta_kernels.chain_length)
#   dW[:, :64]:           8 pixels per thread and turn, 32 threads per channel through LDS atomics, one atomic per
#                         workgroup: 8 * iters + 32 + grid
#   db, dW[:, 64], gb3:   one pixel per thread and turn, 64 lanes, 4 waves, one atomic per workgroup: iters + 68 + grid;
#                         dW[:, 64] also carries m's forward error, 64 (the bound of test_gpu_meta_kernels)
#   da:                   ncls terms
# so L = 256 * iters + grid + 32 + 64 covers every output.  The two-launch chain is held to the same form with its own
# geometry (crimac_meta_bwd: chain_length; crimac_head_bwd: grid = min(ceil(npix / 1024), 1024), ceil(npix / (32 * grid))
# pixels per thread, 32 threads per channel, one atomic per workgroup), + 64 likewise.
# Measured on an MI355X, max |got - ref| / (2^-24 sum|terms|), fused / two-launch chain:
#   (3, 19, 23) Cm 7 ncls 3, L 358 / 358:    da 2.19 / 2.19, dW[:, :64] 0.39 / 0.38, db 0.04 / 0.08, dW[:, 64] 0.005 / 0.004,
#                                            gw1 0.14 / 0.16, gb1 0.15 / 0.15, gw2 0.44 / 0.68, gb2 0.42 / 0.73, gw3 0.04 / 0.06
#   (3, 211, 209) Cm 7 ncls 3, L 1120 / 1120: da 2.83 / 2.83, dW[:, :64] 0.16 / 0.05, gw1 0.27 / 0.18, gw2 0.85 / 0.85, gb2 0.28 / 0.28
BWD_CAP = 512
BWD_SHAPES = [(1, 16, 16), (3, 16, 48), (2, 32, 16)]
BWD_LARGE = (1, 258, 512)                       # 516 workgroups' worth over the cap of 512: four take a second turn
assert -(-BWD_LARGE[1] * BWD_LARGE[2] // 256) == BWD_CAP + 4
BWD_EXACT = [(s, cm, nc) for s in BWD_SHAPES for cm in (1, 3, 7, 8) for nc in (2, 3, 4)] + \
            [(BWD_LARGE, cm, nc) for cm, nc in FEW_PARAMS]
BWD_REAL = [((3, 19, 23), 7, 3), ((3, 19, 23), 3, 2), ((3, 211, 209), 7, 3)]
MLP_OUT = OUTPUTS[1:]                           # gw1 .. gb3 (dwm is column 64 of dw here)


def _bid(case):
    (B, H, W), cm, nc = case
    return f"{B}x{H}x{W}-Cm{cm}-ncls{nc}"


def head_reference(x, w64, dl, bn):
    """float64 head backward on x [npix, 64] (bn: the conv output y, activation relu(y), xhat = y), and sum|terms|."""
    B, ncls, H, W = dl.shape
    d = dl.double().permute(0, 2, 3, 1).reshape(-1, ncls)
    xd = x.double()
    act = xd.clamp_min(0) if bn else xd
    da = d @ w64.double()
    out = {"da": da, "gw": d.T @ act, "db": d.sum(0)}
    ab = {"da": d.abs() @ w64.double().abs(), "gw": d.abs().T @ act.abs(), "db": d.abs().sum(0)}
    if bn:
        dz, dza = da * (xd > 0), ab["da"] * (xd > 0)
        out["s1"], out["s2"] = dz.sum(0), (dz * xd).sum(0)
        ab["s1"], ab["s2"] = dza.sum(0), (dza * xd.abs()).sum(0)
    return out, ab


@functools.lru_cache(maxsize=None)
def bwd_exact_case(case):
    (B, H, W), cm, ncls = case
    c = dict(exact_case(case))
    g = torch.Generator().manual_seed(77 + B + H + W + cm + ncls)
    c["x"] = torch.randint(-2, 3, (B * H * W, C), generator=g).float()
    sign = torch.randint(0, 2, (ncls, C), generator=g).float() * 2 - 1
    c["w64"] = sign * (torch.rand((ncls, C), generator=g) < 0.5).float()
    c["head"] = {bn: head_reference(c["x"], c["w64"], c["dl"], bn) for bn in (False, True)}
    return c


@pytest.mark.parametrize("case", BWD_EXACT, ids=_bid)
def test_backward_exact_case_preconditions_hold(case):
    """Integers everywhere and every sum of |terms|, doubled for the second accumulating call, below 2^24."""
    c = bwd_exact_case(case)
    worst = 0.0
    for k in OUTPUTS:
        assert bool((c["ref"]["grads"][k] == c["ref"]["grads"][k].round()).all()), k
        worst = max(worst, 2 * float(c["ref"]["grads_abs"][k].max()))
    for bn in (False, True):
        out, ab = c["head"][bn]
        for k in out:
            assert bool((out[k] == out[k].round()).all()), k
            worst = max(worst, 2 * float(ab[k].max()))
        assert float(out["gw"].abs().max()) > 0 and float(out["da"].abs().max()) > 0
    print(f"{_bid(case)}: 2 x max sum|terms| = {worst:.0f}")
    assert worst < LIMIT


def _guarded(n):
    """n zeroed floats between two sentinel guard bands; returns (whole buffer, the n floats)."""
    full = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    full[GUARD:GUARD + n] = 0.0
    return full, full[GUARD:GUARD + n]


def _guards_untouched(full, n):
    return bool((full[:GUARD] == SENTINEL).all()) and bool((full[GUARD + n:] == SENTINEL).all())


class _Bwd:
    """Device buffers of one backward call; run() launches crimac_head_meta_bwd on them (accumulating)."""

    def __init__(self, c, shape, bn, reps=2):
        self.B, self.H, self.W = shape
        self.cm, self.ncls = c["meta"].shape[1], c["wm"].numel()
        npix = self.B * self.H * self.W
        self.w = [dev_in(c["p"][k]) for k in WKEYS]
        self.dl, self.meta = dev_in(c["dl"]), dev_in(c["meta"])
        self.wfull = dev_in(torch.cat((c["w64"], c["wm"].reshape(-1, 1)), dim=1))
        self.x = dev_in(c["x"]).reshape(npix, C)
        self.da_full, self.da = _guarded(npix * C)
        self.dw_full, self.dw = _guarded(self.ncls * (C + 1))
        self.db_full, self.db = _guarded(self.ncls)
        self.g = {k: dev_out(c["ref"]["grads"][k].numel()) for k in MLP_OUT}
        self.bn, self.reps = bn, reps
        if bn:        # mean | invstd | scale | shift rows; replica accumulators [reps][64] doubles
            self.vec = torch.stack([torch.zeros(C), torch.ones(C), torch.ones(C), torch.zeros(C)]).cuda()
            self.s1 = torch.zeros(reps, C, dtype=torch.float64, device="cuda")
            self.s2 = torch.zeros(reps, C, dtype=torch.float64, device="cuda")

    def run(self, prec=None):
        prec = hip.PREC_F32X6 if prec is None else prec
        bnb = (ptr(self.x), C, ptr(self.vec), C, ptr(self.s1), ptr(self.s2), self.reps) if self.bn else \
              (None, 0, None, 0, None, None, 1)
        xa = (None, 0) if self.bn else (ptr(self.x), C)       # (fused sums: the activation is rebuilt from y)
        call("crimac_head_meta_bwd", prec, ptr(self.dl), *xa, ptr(self.wfull), ptr(self.da), C, ptr(self.dw),
             ptr(self.db), ptr(self.meta) if self.meta is not None else None, self.cm, *[ptr(t) for t in self.w],
             *[ptr(self.g[k]) for k in MLP_OUT],
             self.B, self.H, self.W, self.ncls, *bnb)
        torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("case", BWD_EXACT, ids=_bid)
def test_exact_backward_once_and_twice(case):
    shape, cm, ncls = case
    c = bwd_exact_case(case)
    ref = c["ref"]["grads"]
    for bn in (False, True):
        out, _ = c["head"][bn]
        b = _Bwd(c, shape, bn)
        for times in (1, 2):                         # every gradient output accumulates: the second call doubles it
            b.run()
            what = f"bn={bn}, call {times}"
            dw = b.dw.cpu().double().reshape(ncls, C + 1)            # row stride 65
            assert torch.equal(dw[:, :C], times * out["gw"]), f"{what}: dW[:, :64]"
            assert torch.equal(dw[:, C], times * ref["dwm"].reshape(-1)), f"{what}: dW[:, 64]"
            assert torch.equal(b.db.cpu().double(), times * out["db"]), f"{what}: db"
            assert torch.equal(b.da.cpu().double().reshape(-1, C), out["da"]), f"{what}: da"      # (overwritten)
            for k in MLP_OUT:
                n = ref[k].numel()
                assert torch.equal(b.g[k][:n].cpu().double(), times * ref[k].reshape(-1)), f"{what}: {k}"
                assert guard_untouched(b.g[k], n), f"{what}: {k} guard"
            if bn:
                assert torch.equal(b.s1.sum(0).cpu(), times * out["s1"]), f"{what}: sum dz"
                assert torch.equal(b.s2.sum(0).cpu(), times * out["s2"]), f"{what}: sum dz xhat"
            assert _guards_untouched(b.dw_full, ncls * (C + 1)), f"{what}: wrote outside the [ncls, 65] gradient"
            assert _guards_untouched(b.db_full, ncls) and _guards_untouched(b.da_full, b.da.numel()), what


def _ratio(got, ref, terms):
    diff = (got.double() - ref).abs()
    return float(torch.where(diff == 0, torch.zeros_like(diff), diff / (U * terms)).max())


def fused_chain_length(npix):
    grid = min(-(-npix // 256), BWD_CAP)
    iters = -(-npix // (256 * grid))
    return 256 * iters + grid + 32 + 64


def old_chain_length(npix):
    grid = min(-(-npix // 1024), 1024)
    return max(chain_length(npix), -(-npix // (32 * grid)) + 32 + grid) + 64


def test_chain_lengths_follow_the_grid_rules():
    assert fused_chain_length(256) == 256 + 1 + 96 and fused_chain_length(3 * 211 * 209) == 2 * 256 + 512 + 96
    assert old_chain_length(3 * 19 * 23) == chain_length(3 * 19 * 23) + 64


@pytest.mark.gpu
@pytest.mark.parametrize("case", BWD_REAL, ids=_bid)
def test_real_valued_backward_within_the_chain_length_bound_and_so_is_the_old_chain(case):
    shape, cm, ncls = case
    B, H, W = shape
    npix = B * H * W
    c = dict(real_case(case))
    g = torch.Generator().manual_seed(9 + cm)
    c["x"] = torch.randn(npix, C, generator=g)
    c["w64"] = torch.randn(ncls, C, generator=g) / 8
    out, ab = head_reference(c["x"], c["w64"], c["dl"], False)
    ref, terms = c["ref"]["grads"], c["ref"]["grads_abs"]
    want = {"da": out["da"].reshape(-1), "gw": out["gw"].reshape(-1), "db": out["db"], "dwm": ref["dwm"].reshape(-1)}
    wabs = {"da": ab["da"].reshape(-1), "gw": ab["gw"].reshape(-1), "db": ab["db"], "dwm": terms["dwm"].reshape(-1)}
    for k in MLP_OUT:
        want[k], wabs[k] = ref[k].reshape(-1), terms[k].reshape(-1)
    # the fused kernel
    b = _Bwd(c, shape, False)
    b.run()
    dw = b.dw.cpu().reshape(ncls, C + 1)
    got = {"da": b.da.cpu(), "gw": dw[:, :C].reshape(-1), "db": b.db.cpu(), "dwm": dw[:, C]}
    got.update({k: b.g[k][:want[k].numel()].cpu() for k in MLP_OUT})
    # the two-launch chain on the same data
    z = lambda n: torch.zeros(n, dtype=torch.float32, device="cuda")      # noqa: E731
    o = {k: z(want[k].numel()) for k in want}
    w64d, wmd = c["w64"].cuda(), c["wm"].cuda()
    call("crimac_meta_bwd", ptr(b.dl), ptr(b.meta), cm, B, H, W, ncls, ptr(wmd), *[ptr(t) for t in b.w], ptr(o["dwm"]),
         *[ptr(o[k]) for k in MLP_OUT])
    call("crimac_head_bwd", hip.PREC_F32X6, ptr(b.dl), ptr(b.x), C, C, ptr(w64d), ptr(o["da"]), C, ptr(o["gw"]),
         ptr(o["db"]), B, H, W, ncls, None, 0, None, 0, None, None, 1)
    torch.cuda.synchronize()
    Lf, Lo = fused_chain_length(npix), old_chain_length(npix)
    rf = {k: _ratio(got[k], want[k], wabs[k]) for k in want}
    ro = {k: _ratio(o[k].cpu(), want[k], wabs[k]) for k in want}
    print(f"{_bid(case)}: fused L = {Lf}: " + ", ".join(f"{k} {v:.3f}" for k, v in rf.items()))
    print(f"{_bid(case)}: chain L = {Lo}: " + ", ".join(f"{k} {v:.3f}" for k, v in ro.items()))
    assert all(v <= Lf for v in rf.values()), rf
    assert all(v <= Lo for v in ro.values()), ro
    assert _guards_untouched(b.dw_full, ncls * (C + 1))


# ---- every storage type, both forms of the head input ----------------------------------------------------------------
# prec -> (storage of dx and of bnb.y, storage of x / of the rebuilt activation, unit roundoff of each).  The inputs are
# rounded to their storage on the CPU first, so the float64 reference starts from the values the kernel reads.  On top of
# L * 2^-24 * sum|terms|:
#   da is stored in T: + roundoff(T) * |ref| (half an ulp of the storage), + 2^-25 absolute in fp16, whose subnormal
#     spacing (2^-24) is reached by the unscaled gradients of this test;
#   fused-sums form: the activation is rebuilt as round_TX(relu(y * scale + shift)) in fp32, where the reference rounds
#     the float64 value: an element on a rounding boundary may land on the neighbour, one ulp = 2 * roundoff(TX) of its
#     term in dW; the sums read da as stored, one ulp of T of each term likewise.  Elements whose float64 pre-activation
#     is within 1e-4 of zero are moved away from the gate beforehand (none is left out).
def _hp(t):
    hi = t.half()
    return hi.float() + (t - hi.float()).half().float()


STORAGE_BWD = {"fp32": (hip.PREC_F32X6, lambda t: t, lambda t: t, 2.0 ** -24, 2.0 ** -24),
               "bf16": (hip.PREC_BF16, lambda t: t.bfloat16().float(), lambda t: t.bfloat16().float(), 2.0 ** -8, 2.0 ** -8),
               "fp16": (hip.PREC_FP16, lambda t: t.half().float(), lambda t: t.half().float(), 2.0 ** -11, 2.0 ** -11),
               "pairs": (hip.PREC_H3P, lambda t: t, _hp, 2.0 ** -24, 2.0 ** -22)}


def _store(t, storage, pairs_ok):
    """fp32 [n, 64] (cpu, already rounded) -> the device tensor of that storage."""
    if storage == "bf16":
        return t.bfloat16().cuda()
    if storage == "fp16":
        return t.half().cuda()
    if storage == "pairs" and pairs_ok:
        return hp_pack(t).cuda()
    return t.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["x", "fused-sums"])
@pytest.mark.parametrize("storage", list(STORAGE_BWD))
def test_real_valued_backward_in_every_storage_type(storage, form):
    case = ((3, 19, 23), 7, 3)
    shape, cm, ncls = case
    B, H, W = shape
    npix = B * H * W
    prec, round_t, round_x, eps_t, eps_x = STORAGE_BWD[storage]
    bn = form == "fused-sums"
    c = real_case(case)
    g = torch.Generator().manual_seed(23)
    w64 = torch.randn(ncls, C, generator=g) / 8
    d = c["dl"].double().permute(0, 2, 3, 1).reshape(npix, ncls)
    if bn:
        y = round_t(torch.randn(npix, C, generator=g))
        mean, invstd = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
        scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        pre = y.double() * scale.double() + shift.double()
        y = torch.where(pre.abs() < 1e-4, round_t(torch.ones(())), y)               # away from the gate
        pre = y.double() * scale.double() + shift.double()
        assert float(pre.abs().min()) >= 1e-4
        act = round_x(pre.clamp_min(0).float()).double()
    else:
        act = round_x(torch.randn(npix, C, generator=g)).double()
    da = d @ w64.double()
    da_abs = d.abs() @ w64.double().abs()
    want = {"da": da.reshape(-1), "gw": (d.T @ act).reshape(-1), "db": d.sum(0), "dwm": c["ref"]["grads"]["dwm"].reshape(-1)}
    wabs = {"da": da_abs.reshape(-1), "gw": (d.abs().T @ act.abs()).reshape(-1), "db": d.abs().sum(0),
            "dwm": c["ref"]["grads_abs"]["dwm"].reshape(-1)}
    extra = {k: torch.zeros_like(v) for k, v in want.items()}
    extra["da"] = eps_t * want["da"].abs() + (2.0 ** -25 if storage == "fp16" else 0.0)
    if bn:
        extra["gw"] = 2 * eps_x * wabs["gw"]
        gate = (pre > 0).double()
        xhat = (y.double() - mean.double()) * invstd.double()
        want["s1"], want["s2"] = (da * gate).sum(0), (da * gate * xhat).sum(0)
        wabs["s1"], wabs["s2"] = (da_abs * gate).sum(0), (da_abs * gate * xhat.abs()).sum(0)
        extra["s1"], extra["s2"] = 2 * eps_t * wabs["s1"], 2 * eps_t * wabs["s2"]
    for k in MLP_OUT:
        want[k], wabs[k] = c["ref"]["grads"][k].reshape(-1), c["ref"]["grads_abs"][k].reshape(-1)
        extra[k] = torch.zeros_like(want[k])
    # device side
    w = [dev_in(c["p"][k]) for k in WKEYS]
    dl, meta = dev_in(c["dl"]), dev_in(c["meta"])
    wfull = dev_in(torch.cat((w64, c["wm"].reshape(-1, 1)), dim=1))
    dx = torch.zeros(npix, C, device="cuda", dtype={"bf16": torch.bfloat16, "fp16": torch.float16}.get(storage, torch.float32))
    dw_full, dw = _guarded(ncls * (C + 1))
    db_full, db = _guarded(ncls)
    gout = {k: dev_out(want[k].numel()) for k in MLP_OUT}
    if bn:
        yd = _store(y, storage, pairs_ok=False)                       # (h3p: the conv output y is fp32)
        vec = torch.stack([mean, invstd, scale, shift]).cuda()
        s1 = torch.zeros(2, C, dtype=torch.float64, device="cuda")
        s2 = torch.zeros(2, C, dtype=torch.float64, device="cuda")
        xa, bnb = (None, 0), (ptr(yd), C, ptr(vec), C, ptr(s1), ptr(s2), 2)
    else:
        xd = _store(act.float(), storage, pairs_ok=True)
        xa, bnb = (ptr(xd), C), (None, 0, None, 0, None, None, 1)
    call("crimac_head_meta_bwd", prec, ptr(dl), *xa, ptr(wfull), ptr(dx), C, ptr(dw), ptr(db), ptr(meta), cm,
         *[ptr(t) for t in w], *[ptr(gout[k]) for k in MLP_OUT], B, H, W, ncls, *bnb)
    torch.cuda.synchronize()
    dwc = dw.cpu().reshape(ncls, C + 1)
    got = {"da": dx.float().cpu().reshape(-1), "gw": dwc[:, :C].reshape(-1), "db": db.cpu(), "dwm": dwc[:, C]}
    got.update({k: gout[k][:want[k].numel()].cpu() for k in MLP_OUT})
    if bn:
        got["s1"], got["s2"] = s1.sum(0).cpu(), s2.sum(0).cpu()
    L = fused_chain_length(npix)
    worst = {}
    for k in want:
        diff = (got[k].double() - want[k]).abs()
        bound = L * U * wabs[k] + extra[k]
        worst[k] = float(torch.where(diff == 0, torch.zeros_like(diff), diff / bound).max())
    print(f"{storage} {form}: |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1 for v in worst.values()), worst
    assert _guards_untouched(dw_full, ncls * (C + 1)) and _guards_untouched(db_full, ncls)


@pytest.mark.gpu
def test_backward_refuses_bad_arguments_and_launches_nothing():
    c = bwd_exact_case(((1, 16, 16), 8, 3))
    b = _Bwd(c, (1, 16, 16), False)
    for cm in (0, 9):
        b.cm = cm
        with _refuses(f"head_meta_bwd: {cm} metadata channels (1..8 supported)"):
            b.run()
    b.cm = 8
    b.ncls = 5
    with _refuses("head_meta_bwd: ncls=5 unsupported (2..4)"):
        b.run()
    b.ncls = 3
    keep = b.meta
    b.meta = None
    with _refuses("head_meta_bwd: bad arguments"):
        b.run()
    b.meta = keep
    with _refuses("head_meta_bwd: bad precision"):
        b.run(prec=hip.PREC_H3F_BWD)
    torch.cuda.synchronize()
    assert float(b.dw.abs().max()) == 0 and float(b.da.abs().max()) == 0 and float(b.g["gw2"][:1024].abs().max()) == 0
