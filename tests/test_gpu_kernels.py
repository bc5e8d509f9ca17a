"""GPU parity tests, one kernel at a time, through the C ABI (include/crimac_unet_hip.h).

Each HIP kernel is compared with the torch CPU fp32 op the reference dispatches for the same step
(the oracle of a single op is that op itself, run on the host).  Tolerances:
  * 'f32x6' (parity mode): 2e-6 of max|ref| -- 3-plane split, ~2^-24 per product (fp32-equivalent);
  * 'f32x3': 1e-4 of max|ref| -- 2-plane split-bf16 products carry ~2^-16 relative error;
  * 'bf16' / 'fp16' (16-bit storage modes): inputs are pre-rounded on the host, so what is left is the
    rounding of the OUTPUT (2^-8 / 2^-11 relative) and accumulation order: 1e-2 / 2e-3 of max|ref|.

The BatchNorm / ReLU / max-pool / unpool kernels (colstats, colsum_f32, sum_replicas, bn_finalize, bn_train_act_pool,
bn_act_pool, unpool_add, bn_bwd_reduce and the four bn_bwd_apply paths) have their direct tests in
tests/test_gpu_bn_kernels.py: a float64 reference, data on which the ReLU and arg-max decisions are exact, element-wise
bounds, edge channel counts, strided / sliced / guarded buffers and capped grids.  The tests of those kernels below compare
them at the workload's shapes and with one another.

The MFMA contraction kernels (conv3x3, its pool / cols / input-gradient uses, the transposed convolution, the weight
gradients) have their exact tests in tests/test_gpu_conv_exact.py: ternary operands on which every kernel form and
precision must equal a float64 reference bit for bit, images smaller than a tile (down to 1x1), guarded and sliced
buffers.  The tests of those kernels below compare them norm-wise on Gaussian data, which a single wrong product at
K = 9 * Cin >= 576 passes in the 16-bit modes.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd.hip import call, ptr

pytestmark = pytest.mark.gpu

PRECS = ["f32x6", "f32x3", "bf16", "fp16"]
LOWP = ("bf16", "fp16")                 # 16-bit storage modes: same kernels, instantiated per element type
TOL = {"f32x6": 5e-6, "f32x3": 1e-4, "bf16": 1e-2, "fp16": 2e-3}      # fp16 output rounding is 2^-11
NPL = {"f32x6": 3, "f32x3": 2, "bf16": 1, "fp16": hip.PLANES_FP16, "f32h3": hip.PLANES_F32H3}     # `planes` argument
_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _dt(prec):
    return _DT.get(prec, torch.float32)


def _round(x, prec):
    """Host-side rounding of kernel INPUTS to the activation storage type."""
    return x.to(_DT[prec]).float() if prec in _DT else x


def to_nhwc(x, prec, ld=None):
    """[B,C,H,W] fp32 (cpu) -> device [B*H*W, ld] activation matrix."""
    B, C, H, W = x.shape
    ld = ld or C
    out = torch.zeros(B * H * W, ld, dtype=_dt(prec), device="cuda")
    out[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C).to(_dt(prec)).cuda()
    return out


def from_nhwc(t, B, H, W, C=None):
    C = C or t.shape[1]
    return t[:, :C].float().cpu().reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def pack_conv(w, prec, cin_pad=None, scale=None, dgrad=True):
    Co, Ci = w.shape[:2]
    cin_pad = cin_pad or Ci
    wd = w.float().cuda().contiguous()
    i16 = dict(dtype=torch.int16, device="cuda")
    npl = NPL[prec]
    fh, fl = torch.empty(9 * Co * cin_pad, **i16), torch.empty(2 * 9 * Co * cin_pad, **i16)
    dh = torch.empty(9 * Ci * Co, **i16) if dgrad and cin_pad == Ci else None
    dl = torch.empty(2 * 9 * Ci * Co, **i16) if dgrad and cin_pad == Ci else None
    sc = scale.float().cuda() if scale is not None else None
    call("crimac_pack_conv3x3", ptr(wd), Co, Ci, cin_pad, ptr(sc), npl, ptr(fh), ptr(fl), ptr(dh), ptr(dl))
    torch.cuda.synchronize()
    return fh, fl, dh, dl


def conv3x3(prec, x_nhwc, ld, B, H, W, Cin, Cout, w_hi, w_lo, bias, relu=False):
    out = torch.empty(B * H * W, Cout, dtype=_dt(prec), device="cuda")
    call("crimac_igemm_conv", hip.PREC_NAMES[prec], ptr(x_nhwc), ld, B, H, W, H, W, Cin, Cout, 9, 3, 1, 1,
         ptr(w_hi), ptr(w_lo), ptr(bias), Cout, ptr(out), Cout, 1 if relu else 0, 0, 0)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(2, 16, 16, 64, 64), (1, 16, 32, 128, 128), (3, 8, 8, 256, 64),
                                   (2, 16, 16, 4, 64), (1, 24, 40, 64, 192)])
def test_conv3x3_forward(prec, shape):
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(1)
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    b = torch.randn(Co, generator=g)
    cin_pad = 16 if Ci < 16 else Ci
    fh, fl, _, _ = pack_conv(w, prec, cin_pad, dgrad=False)
    wr = _round(w, prec)
    ref = F.conv2d(x, wr, b, padding=1)
    xin = to_nhwc(x, prec, ld=cin_pad)
    out = conv3x3(prec, xin, cin_pad, B, H, W, cin_pad, Co, fh, fl, b.cuda())
    assert relerr(from_nhwc(out, B, H, W), ref) < TOL[prec]
    # fused bias+ReLU epilogue (eval-mode folded path)
    out = conv3x3(prec, xin, cin_pad, B, H, W, cin_pad, Co, fh, fl, b.cuda(), relu=True)
    assert relerr(from_nhwc(out, B, H, W), torch.relu(ref)) < TOL[prec]


@pytest.mark.parametrize("prec", PRECS)
def test_conv3x3_bn_fold_scale_and_strided_io(prec):
    """BatchNorm folding scale in the packer; input/output living in channel slices (ld > C)."""
    B, H, W, Ci, Co = 2, 16, 16, 64, 64
    g = torch.Generator().manual_seed(2)
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / 24
    s = torch.rand(Co, generator=g) + 0.5
    fh, fl, _, _ = pack_conv(w, prec, scale=s, dgrad=False)
    ref = F.conv2d(x, _round(w * s[:, None, None, None], prec), None, padding=1)
    big_in = torch.zeros(B * H * W, 2 * Ci, dtype=_dt(prec), device="cuda")
    big_in[:, Ci:] = to_nhwc(x, prec)
    big_out = torch.full((B * H * W, 3 * Co), 7.0, dtype=_dt(prec), device="cuda")
    call("crimac_igemm_conv", hip.PREC_NAMES[prec], ptr(big_in, Ci), 2 * Ci, B, H, W, H, W, Ci, Co, 9, 3,
         1, 1, ptr(fh), ptr(fl), None, 0, ptr(big_out, Co), 3 * Co, 0, 0, 0)
    torch.cuda.synchronize()
    assert relerr(from_nhwc(big_out[:, Co:2 * Co].contiguous(), B, H, W), ref) < TOL[prec]
    assert float((big_out[:, :Co].float() - 7).abs().max()) == 0 and \
        float((big_out[:, 2 * Co:].float() - 7).abs().max()) == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(2, 16, 16, 64, 64), (1, 16, 16, 128, 256)])
def test_conv3x3_dgrad(prec, shape):
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(3)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    dy = _round(torch.randn(B, Co, H, W, generator=g), prec)
    _, _, dh, dl = pack_conv(w, prec)
    ref = torch.nn.grad.conv2d_input((B, Ci, H, W), _round(w, prec), dy, padding=1)
    out = torch.empty(B * H * W, Ci, dtype=_dt(prec), device="cuda")
    dyn = to_nhwc(dy, prec)       # keep every device operand alive in a variable until the sync
    call("crimac_igemm_conv", hip.PREC_NAMES[prec], ptr(dyn), Co, B, H, W, H, W, Co, Ci, 9,
         3, 1, 1, ptr(dh), ptr(dl), None, 0, ptr(out), Ci, 0, 0, 0)
    torch.cuda.synchronize()
    assert relerr(from_nhwc(out, B, H, W), ref) < TOL[prec]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(2, 8, 8, 128, 64), (1, 4, 8, 256, 128), (2, 24, 40, 128, 64), (1, 16, 16, 64, 32),
                                   (2, 64, 64, 256, 128),       # many workgroups in flight (timing hazards)
                                   (1, 5, 20, 128, 128), (2, 7, 33, 256, 64)])   # odd rows / ragged columns, 128- and 64-wide S
def test_upconv2x2_forward_dgrad_wgrad(prec, shape):
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(4)
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    w = torch.randn(Ci, Co, 2, 2, generator=g) / Ci ** 0.5
    b = torch.randn(Co, generator=g)
    i16 = dict(dtype=torch.int16, device="cuda")
    n = 4 * Ci * Co
    fh, fl, dh, dl = (torch.empty(2 * n, **i16) for _ in range(4))
    wd, bd, xn = w.cuda(), b.cuda(), to_nhwc(x, prec)
    call("crimac_pack_upconv2x2", ptr(wd), Ci, Co, NPL[prec], ptr(fh), ptr(fl), ptr(dh), ptr(dl))
    wr = _round(w, prec)
    ref = F.conv_transpose2d(x, wr, b, stride=2)
    # forward writes into the first half of a [M, 2*Co] "concat" buffer
    cat = torch.zeros(B * 4 * H * W, 2 * Co, dtype=_dt(prec), device="cuda")
    P = hip.PREC_NAMES[prec]
    call("crimac_igemm_conv", P, ptr(xn), Ci, B, H, W, H, W, Ci, 4 * Co, 1, 1, 0, 1,
         ptr(fh), ptr(fl), ptr(bd), Co, ptr(cat), 2 * Co, 0, 1, Co)
    torch.cuda.synchronize()
    assert relerr(from_nhwc(cat[:, :Co].contiguous(), B, 2 * H, 2 * W), ref) < TOL[prec]
    assert float(cat[:, Co:].float().abs().max()) == 0
    # input gradient
    dy = _round(torch.randn(B, Co, 2 * H, 2 * W, generator=g), prec)
    xg = x.clone().requires_grad_(True)
    wg = wr.clone().requires_grad_(True)
    F.conv_transpose2d(xg, wg, None, stride=2).backward(dy)
    dyn = to_nhwc(dy, prec)
    dx = torch.empty(B * H * W, Ci, dtype=_dt(prec), device="cuda")
    call("crimac_igemm_conv", P, ptr(dyn), Co, B, 2 * H, 2 * W, H, W, Co, Ci, 4, 2, 0, 2, ptr(dh), ptr(dl),
         None, 0, ptr(dx), Ci, 0, 0, 0)
    torch.cuda.synchronize()
    assert relerr(from_nhwc(dx, B, H, W), xg.grad) < TOL[prec]
    # weight gradient
    dwp = torch.zeros(4 * Ci * Co, dtype=torch.float32, device="cuda")
    call("crimac_wgrad", P, 1, ptr(xn), Ci, Ci, ptr(dyn), Co, Co, B, H, W, ptr(dwp), 2)   # multi-tile loops
    grad = torch.empty(Ci, Co, 2, 2, dtype=torch.float32, device="cuda")
    call("crimac_unpack_wgrad_upconv2x2", ptr(dwp), Ci, Co, ptr(grad))
    torch.cuda.synchronize()
    assert relerr(grad.cpu(), wg.grad) < (2e-3 if prec in LOWP else TOL[prec])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("target_blocks", [1, 3, 64])     # 1: one workgroup loops over ALL pixel tiles
@pytest.mark.parametrize("shape", [(2, 16, 16, 64, 64), (1, 8, 32, 128, 64), (2, 16, 16, 4, 64),
                                   (1, 12, 20, 64, 128), (3, 24, 48, 64, 64)])
def test_conv3x3_wgrad(prec, shape, target_blocks):
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(5)
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    dy = _round(torch.randn(B, Co, H, W, generator=g), prec)
    ref = torch.nn.grad.conv2d_weight(x, (Co, Ci, 3, 3), dy, padding=1)
    cin_pad = 16 if Ci < 16 else Ci
    dwp = torch.zeros(9 * Co * cin_pad, dtype=torch.float32, device="cuda")
    dyn, xn = to_nhwc(dy, prec), to_nhwc(x, prec, ld=cin_pad)
    call("crimac_wgrad", hip.PREC_NAMES[prec], 0, ptr(dyn), Co, Co,
         ptr(xn), cin_pad, cin_pad, B, H, W, ptr(dwp), target_blocks)
    grad = torch.empty(Co, Ci, 3, 3, dtype=torch.float32, device="cuda")
    call("crimac_unpack_wgrad_conv3x3", ptr(dwp), Co, Ci, cin_pad, ptr(grad))
    torch.cuda.synchronize()
    # inputs are exact in both modes; the contraction accumulates in fp32
    assert relerr(grad.cpu(), ref) < (1e-4 if prec != "f32x6" else 5e-6)


@pytest.mark.parametrize("mode,shape", [(0, (2, 128, 128, 128, 64)), (0, (1, 256, 256, 64, 64)),
                                        (0, (2, 100, 120, 64, 128)), (1, (2, 64, 64, 128, 64)),
                                        (1, (2, 64, 64, 256, 128)), (1, (4, 128, 128, 128, 64)),
                                        (0, (2, 128, 128, 16, 64))])      # (the last: first-layer narrow-S kernel)
@pytest.mark.parametrize("prec", LOWP)
def test_wgrad_many_workgroups_auto_split(mode, shape, prec):
    """bf16 weight gradient with the library's own pixel split (target_blocks = 0): hundreds of workgroups in
    flight, several tiles per workgroup -- the hand-placed LDS-read pipeline (asm loads, counted waits) only
    shows ordering mistakes under this kind of load.  mode 0: conv3x3, mode 1: transposed conv."""
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(17)
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    P = hip.PREC_NAMES[prec]
    if mode == 0:
        dy = _round(torch.randn(B, Co, H, W, generator=g), prec)
        ref = torch.nn.grad.conv2d_weight(x, (Co, Ci, 3, 3), dy, padding=1)
        dwp = torch.zeros(9 * Co * Ci, dtype=torch.float32, device="cuda")
        dyn, xn = to_nhwc(dy, prec), to_nhwc(x, prec)       # (kept alive: the call is asynchronous)
        call("crimac_wgrad", P, 0, ptr(dyn), Co, Co, ptr(xn), Ci, Ci, B, H, W, ptr(dwp), 0)
        grad = torch.empty(Co, Ci, 3, 3, dtype=torch.float32, device="cuda")
        call("crimac_unpack_wgrad_conv3x3", ptr(dwp), Co, Ci, Ci, ptr(grad))
    else:
        dy = _round(torch.randn(B, Co, 2 * H, 2 * W, generator=g), prec)
        wg = torch.zeros(Ci, Co, 2, 2, requires_grad=True)
        F.conv_transpose2d(x, wg, None, stride=2).backward(dy)
        ref = wg.grad
        dwp = torch.zeros(4 * Ci * Co, dtype=torch.float32, device="cuda")
        dyn, xn = to_nhwc(dy, prec), to_nhwc(x, prec)
        call("crimac_wgrad", P, 1, ptr(xn), Ci, Ci, ptr(dyn), Co, Co, B, H, W, ptr(dwp), 0)
        grad = torch.empty(Ci, Co, 2, 2, dtype=torch.float32, device="cuda")
        call("crimac_unpack_wgrad_upconv2x2", ptr(dwp), Ci, Co, ptr(grad))
    torch.cuda.synchronize()
    assert relerr(grad.cpu(), ref) < 2e-4


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", [64, 256, 1024])
def test_batchnorm_train_forward_backward_pool(prec, C):
    B, H, W = 2, 8, 8
    M = B * H * W
    g = torch.Generator().manual_seed(6)
    y = _round(torch.randn(B, C, H, W, generator=g) * 2 + 0.5, prec)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    P = hip.PREC_NAMES[prec]
    d = "cuda"
    yn = to_nhwc(y, prec)
    s = torch.zeros(2, C, dtype=torch.float64, device=d)
    call("crimac_colstats", P, ptr(yn), C, M, C, ptr(s[0]), ptr(s[1]))
    rm_d, rv_d, gamma_d, beta_d = rm.to(d), rv.to(d), gamma.to(d), beta.to(d)
    nbt = torch.zeros((), dtype=torch.int64, device=d)
    st = torch.zeros(4, C, dtype=torch.float32, device=d)   # mean, invstd, scale, shift
    call("crimac_bn_finalize", ptr(s[0]), ptr(s[1]), 1, M, C, ptr(gamma_d), ptr(beta_d), 1e-5, 0.1,
         ptr(rm_d), ptr(rv_d), ptr(nbt), ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]))
    a = torch.empty(M, C, dtype=_dt(prec), device=d)
    pool = torch.empty(M // 4, C, dtype=_dt(prec), device=d)
    call("crimac_bn_act_pool", P, ptr(yn), C, ptr(st[2]), ptr(st[3]), 1, ptr(a), C, ptr(pool), C, B, H, W, C)
    torch.cuda.synchronize()
    # reference
    yr = y.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm_r, rv_r = rm.clone(), rv.clone()
    z = F.batch_norm(yr, rm_r, rv_r, gr, br, training=True, momentum=0.1, eps=1e-5)
    ar = torch.relu(z)
    pr = F.max_pool2d(ar, 2, 2)
    tol = TOL[prec]
    assert relerr(from_nhwc(a, B, H, W), ar) < tol
    assert relerr(from_nhwc(pool, B, H // 2, W // 2), pr) < tol
    assert relerr(rm_d.cpu(), rm_r) < 1e-5 and relerr(rv_d.cpu(), rv_r) < 1e-5 and int(nbt) == 1
    # backward: da = ds + unpool(dp)
    dp = _round(torch.randn(B, C, H // 2, W // 2, generator=g), prec)
    ds = _round(torch.randn(B, C, H, W, generator=g), prec)
    (pr * dp).sum().backward(retain_graph=True)
    (ar * ds).sum().backward()
    da = torch.empty(M, C, dtype=_dt(prec), device=d)
    dpn, dsn = to_nhwc(dp, prec), to_nhwc(ds, prec)
    call("crimac_unpool_add", P, ptr(dpn), C, ptr(a), C, ptr(dsn), C, ptr(da), C,
         B, H, W, C, None, 0, None, 0, None, None, 1)
    s2 = torch.zeros(2, C, dtype=torch.float64, device=d)
    call("crimac_bn_bwd_reduce", P, ptr(da), C, ptr(yn), C, ptr(st[2]), ptr(st[3]), ptr(st[0]), ptr(st[1]), M,
         C, ptr(s2[0]), ptr(s2[1]))
    # the same sums taken inside unpool_add (7 replicas), identical da
    R = 7
    vec = torch.stack([st[0], st[1], st[2], st[3]]).contiguous()          # mean, invstd, scale, shift
    rep = torch.zeros(2, R, C, dtype=torch.float64, device=d)
    da_f = torch.empty_like(da)
    call("crimac_unpool_add", P, ptr(dpn), C, ptr(a), C, ptr(dsn), C, ptr(da_f), C,
         B, H, W, C, ptr(yn), C, ptr(vec), C, ptr(rep[0]), ptr(rep[1]), R)
    torch.cuda.synchronize()
    assert torch.equal(da_f, da)
    assert relerr(rep[0].sum(0).cpu(), s2[0].cpu()) < 1e-5 and relerr(rep[1].sum(0).cpu(), s2[1].cpu()) < 1e-5
    dy = torch.empty(M, C, dtype=_dt(prec), device=d)
    dg, db, dbias = (torch.zeros(C, dtype=torch.float32, device=d) for _ in range(3))
    call("crimac_bn_bwd_apply", P, ptr(da), C, ptr(yn), C, ptr(st[2]), ptr(st[3]), ptr(st[0]), ptr(st[1]),
         ptr(s2[0]), ptr(s2[1]), M, 0, C, ptr(dy), C, ptr(dg), ptr(db), ptr(dbias))
    torch.cuda.synchronize()
    if prec in LOWP:
        # bf16-rounded activations tie inside 2x2 windows far more often than fp32 ones; a tie routes
        # the pooled gradient to another pixel, so compare in L2 instead of max-norm
        d_out, d_ref = from_nhwc(dy, B, H, W).double(), yr.grad.double()
        assert float((d_out - d_ref).norm() / d_ref.norm()) < 0.1
    else:
        assert relerr(from_nhwc(dy, B, H, W), yr.grad) < 2e-4
    assert relerr(dg.cpu(), gr.grad) < (2e-2 if prec in LOWP else 2e-4)
    assert relerr(db.cpu(), br.grad) < (2e-2 if prec in LOWP else 2e-4)


@pytest.mark.parametrize("prec", PRECS + ["h3p"])
@pytest.mark.parametrize("C,R,pooled", [(64, 64, True), (48, 5, False), (256, 32, True), (1024, 8, False), (16, 1, True)])
def test_batchnorm_statistics_finished_inside_the_consumer(prec, C, R, pooled):
    """crimac_bn_train_act_pool == crimac_bn_finalize + crimac_bn_act_pool and crimac_bn_bwd_apply_replicas ==
    crimac_sum_replicas + crimac_bn_bwd_apply, from the same [replicas][C] accumulators: identical tensors."""
    B, H, W = 3, 8, 12
    M = B * H * W
    P = hip.PREC_NAMES[prec]
    d = "cuda"
    g = torch.Generator().manual_seed(C + R)
    hp = prec == "h3p"
    dt_y = torch.float32 if hp else _dt(prec)
    y = (torch.randn(M, C, generator=g) * 2 + 0.5).to(dt_y).to(d)
    # replica accumulators as a producer leaves them: partial sums of disjoint pixel subsets
    rep = torch.zeros(2, R, C, dtype=torch.float64, device=d)
    owner = torch.randint(0, R, (M,), generator=g).to(d)
    yd = y.double()
    rep[0].index_add_(0, owner, yd)
    rep[1].index_add_(0, owner, yd * yd)
    gamma = (torch.rand(C, generator=g) + 0.5).to(d)
    beta = (torch.randn(C, generator=g) * 0.2).to(d)

    def run(fused):
        rm, rv = torch.full((C,), 0.25, device=d), torch.full((C,), 1.5, device=d)
        nbt = torch.zeros((), dtype=torch.int64, device=d)
        ld = C + 8                                             # (row stride of the vector block > C)
        vec = torch.zeros(4, ld, dtype=torch.float32, device=d)
        a = torch.zeros(M, C, dtype=y.dtype, device=d)          # (h3p: fp32-sized plane pairs)
        pool = torch.zeros(M // 4, C, dtype=a.dtype, device=d) if pooled else None
        if fused:
            call("crimac_bn_train_act_pool", P, ptr(y), C, ptr(rep[0]), ptr(rep[1]), R, M, ptr(gamma), ptr(beta), 1e-5,
                 0.1, ptr(rm), ptr(rv), ptr(nbt), ptr(vec), ld, 1, ptr(a), C, ptr(pool) if pooled else None,
                 C if pooled else 0, B, H, W, C)
        else:
            call("crimac_bn_finalize", ptr(rep[0]), ptr(rep[1]), R, M, C, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(rm),
                 ptr(rv), ptr(nbt), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(vec[3]))
            call("crimac_bn_act_pool", P, ptr(y), C, ptr(vec[2]), ptr(vec[3]), 1, ptr(a), C,
                 ptr(pool) if pooled else None, C if pooled else 0, B, H, W, C)
        torch.cuda.synchronize()
        return vec[:, :C].clone(), a, pool, rm, rv, int(nbt)

    v0, a0, p0, rm0, rv0, n0 = run(False)
    v1, a1, p1, rm1, rv1, n1 = run(True)
    # (the two forms add the replicas in a different order: the fp64 sums may differ in their last bit)
    assert relerr(v1.cpu(), v0.cpu()) < 1e-6 and n0 == n1 == 1
    assert relerr(rm1.cpu(), rm0.cpu()) < 1e-6 and relerr(rv1.cpu(), rv0.cpu()) < 1e-6
    if torch.equal(v1, v0):
        assert torch.equal(a1.view(torch.uint8), a0.view(torch.uint8))
        assert not pooled or torch.equal(p1.view(torch.uint8), p0.view(torch.uint8))
    elif not hp:
        assert relerr(a1.float().cpu(), a0.float().cpu()) < TOL.get(prec, 1e-5)
    # backward
    da = torch.randn(M, C, generator=g).to(dt_y).to(d)
    repb = torch.zeros(2, R, C, dtype=torch.float64, device=d)
    act = yd * v0[2].double() + v0[3].double() > 0
    dz = da.double() * act
    repb[0].index_add_(0, owner, dz)
    repb[1].index_add_(0, owner, dz * (yd - v0[0].double()) * v0[1].double())
    vec = torch.zeros(4, C + 8, dtype=torch.float32, device=d)
    vec[:, :C] = v0
    outs = []
    for fused in (False, True):
        dy = torch.zeros(M, C, dtype=torch.float32 if hp else dt_y, device=d)
        dg, db = torch.zeros(C, device=d), torch.zeros(C, device=d)
        if fused:
            call("crimac_bn_bwd_apply_replicas", P, ptr(da), C, ptr(y), C, ptr(vec), C + 8, ptr(repb[0]), ptr(repb[1]),
                 R, M, 0, C, ptr(dy), C, ptr(dg), ptr(db))
        else:
            s2 = torch.zeros(2, C, dtype=torch.float64, device=d)
            call("crimac_sum_replicas", ptr(repb[0]), R, C, C, ptr(s2[0]), None, ptr(repb[1]), ptr(s2[1]))
            call("crimac_bn_bwd_apply", P, ptr(da), C, ptr(y), C, ptr(vec[2]), ptr(vec[3]), ptr(vec[0]), ptr(vec[1]),
                 ptr(s2[0]), ptr(s2[1]), M, 0, C, ptr(dy), C, ptr(dg), ptr(db), None)
        torch.cuda.synchronize()
        outs.append((dy, dg, db))
    (dy0, dg0, db0), (dy1, dg1, db1) = outs
    assert relerr(dg1.cpu(), dg0.cpu()) < 1e-6 and relerr(db1.cpu(), db0.cpu()) < 1e-6
    if hp:
        hi0, lo0 = dy0.view(torch.float16).view(M, C // 8, 2, 8).float().unbind(2)
        hi1, lo1 = dy1.view(torch.float16).view(M, C // 8, 2, 8).float().unbind(2)
        assert relerr((hi1 + lo1).cpu(), (hi0 + lo0).cpu()) < 1e-5
    else:
        assert relerr(dy1.float().cpu(), dy0.float().cpu()) < TOL.get(prec, 1e-5)


@pytest.mark.parametrize("prec", PRECS)
def test_unpool_first_max_tie_rule(prec):
    """Ties inside a 2x2 window: gradient goes to the FIRST maximum in scan order (aten max_pool2d)."""
    B, C, H, W = 1, 8, 2, 2
    a = torch.tensor([[1.0, 3.0], [3.0, 3.0]]).expand(B, C, H, W).contiguous()
    ar = a.clone().requires_grad_(True)
    F.max_pool2d(ar, 2, 2).sum().backward()
    dp = torch.ones(B, C, 1, 1)
    da = torch.empty(4, C, dtype=_dt(prec), device="cuda")
    dpn, an = to_nhwc(dp, prec), to_nhwc(a, prec)
    call("crimac_unpool_add", hip.PREC_NAMES[prec], ptr(dpn), C, ptr(an), C,
         None, 0, ptr(da), C, B, H, W, C, None, 0, None, 0, None, None, 1)
    torch.cuda.synchronize()
    assert torch.equal(from_nhwc(da, B, H, W), ar.grad)


@pytest.mark.parametrize("prec", PRECS)
def test_head_with_batchnorm_relu_applied_on_the_fly(prec):
    """head_fwd(bn_scale, bn_shift) on the raw conv output == head_fwd on the stored activation; head_bwd with
    x == NULL rebuilds that activation from bnb_y: identical dw / db / dx / fused sums."""
    B, H, W, C, ncls = 2, 24, 40, 64, 3
    g = torch.Generator().manual_seed(31)
    P, d = hip.PREC_NAMES[prec], "cuda"
    M = B * H * W
    y = (torch.randn(M, C, generator=g) * 1.3 + 0.2).to(_dt(prec)).cuda()
    vec = torch.stack([torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5,
                       torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3]).contiguous().cuda()
    wd = (torch.randn(ncls, C, generator=g) / 8).cuda()
    bd = (torch.randn(ncls, generator=g) * 0.1).cuda()
    a = torch.empty_like(y)                      # the activation as bn_act stores it
    call("crimac_bn_act_pool", P, ptr(y), C, ptr(vec[2]), ptr(vec[3]), 1, ptr(a), C, None, 0, B, H, W, C)
    z_ref = torch.empty(B, ncls, H, W, dtype=torch.float32, device=d)
    z = torch.empty_like(z_ref)
    call("crimac_head_fwd", P, ptr(a), C, C, ptr(wd), ptr(bd), ptr(z_ref), B, H, W, ncls, 0, None, None)
    call("crimac_head_fwd", P, ptr(y), C, C, ptr(wd), ptr(bd), ptr(z), B, H, W, ncls, 0, ptr(vec[2]), ptr(vec[3]))
    torch.cuda.synchronize()
    assert torch.equal(z, z_ref)
    dl = torch.randn(B, ncls, H, W, generator=g).cuda()
    outs = []
    for xin in (a, None):
        dx = torch.empty(M, C, dtype=_dt(prec), device=d)
        dw = torch.zeros(ncls, C, dtype=torch.float32, device=d)
        db = torch.zeros(ncls, dtype=torch.float32, device=d)
        rep = torch.zeros(2, 4, C, dtype=torch.float64, device=d)
        call("crimac_head_bwd", P, ptr(dl), ptr(xin) if xin is not None else None, C if xin is not None else 0, C,
             ptr(wd), ptr(dx), C, ptr(dw), ptr(db), B, H, W, ncls, ptr(y), C, ptr(vec), C, ptr(rep[0]), ptr(rep[1]), 4)
        torch.cuda.synchronize()
        outs.append((dx, dw, db, rep.sum(1)))
    assert torch.equal(outs[0][0], outs[1][0])
    assert relerr(outs[1][1], outs[0][1]) < 1e-5 and relerr(outs[1][2], outs[0][2]) < 1e-5
    assert relerr(outs[1][3], outs[0][3]) < 1e-5          # (fp32 partials meet in a run-dependent atomic order)
    with pytest.raises(hip.HipLibraryError):     # x == NULL without the fused sums
        call("crimac_head_bwd", P, ptr(dl), None, 0, C, ptr(wd), ptr(dx), C, ptr(dw), ptr(db), B, H, W, ncls,
             None, 0, None, 0, None, None, 1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ncls", [3, 2])
def test_head_and_weighted_ce(prec, ncls):
    B, H, W, C = 2, 16, 16, 64
    g = torch.Generator().manual_seed(7)
    x = _round(torch.randn(B, C, H, W, generator=g), prec)
    w = torch.randn(ncls, C, 1, 1, generator=g) / 8
    b = torch.randn(ncls, generator=g) * 0.1
    labels = torch.randint(0, ncls, (B, H, W), generator=g)
    labels[torch.rand(B, H, W, generator=g) < 0.1] = -100
    cw = torch.tensor([10.0, 300.0, 250.0][:ncls])
    P, d = hip.PREC_NAMES[prec], "cuda"
    xn = to_nhwc(x, prec)
    wd, bd, cwd = w.to(d), b.to(d), cw.to(d)
    logits = torch.empty(B, ncls, H, W, dtype=torch.float32, device=d)
    soft = torch.empty_like(logits)
    call("crimac_head_fwd", P, ptr(xn), C, C, ptr(wd), ptr(bd), ptr(logits), B, H, W, ncls, 0, None, None)
    call("crimac_head_fwd", P, ptr(xn), C, C, ptr(wd), ptr(bd), ptr(soft), B, H, W, ncls, 1, None, None)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    zr = F.conv2d(xr, wr, br)
    loss_r = F.cross_entropy(zr, labels, weight=cw, ignore_index=-100)
    loss_r.backward()
    torch.cuda.synchronize()
    assert relerr(logits.cpu(), zr.detach()) < 1e-5
    assert relerr(soft.cpu(), torch.softmax(zr.detach(), 1)) < 1e-5
    for lab_dtype in (torch.int64, torch.int16, torch.int32):
        lab = labels.to(lab_dtype).to(d)
        sums = torch.zeros(2, dtype=torch.float64, device=d)
        call("crimac_wce_fwd", ptr(logits), ptr(lab), lab.element_size(), ptr(cwd), ncls, -100, B, H, W,
             ptr(sums))
        assert abs(float(sums[0] / sums[1]) - float(loss_r)) < 1e-5 * abs(float(loss_r))
    dl = torch.empty_like(logits)
    call("crimac_wce_bwd", ptr(logits), ptr(lab), lab.element_size(), ptr(cwd), ncls, -100, B, H, W,
         ptr(sums), 1.0, ptr(dl))
    dx = torch.empty(B * H * W, C, dtype=_dt(prec), device=d)
    dw = torch.zeros(ncls, C, dtype=torch.float32, device=d)
    dbv = torch.zeros(ncls, dtype=torch.float32, device=d)
    call("crimac_head_bwd", P, ptr(dl), ptr(xn), C, C, ptr(wd), ptr(dx), C, ptr(dw), ptr(dbv), B, H, W, ncls,
         None, 0, None, 0, None, None, 1)
    torch.cuda.synchronize()
    # fused BatchNorm-backward sums of the block dx feeds == bn_bwd_reduce on the stored dx
    Mh = B * H * W
    yb = torch.randn(Mh, C, generator=g).to(_dt(prec)).cuda()
    vec = torch.stack([torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5,
                       torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3]).contiguous().cuda()
    rep = torch.zeros(2, 5, C, dtype=torch.float64, device=d)
    dx2, dw2, db2 = torch.empty_like(dx), torch.zeros_like(dw), torch.zeros_like(dbv)
    call("crimac_head_bwd", P, ptr(dl), ptr(xn), C, C, ptr(wd), ptr(dx2), C, ptr(dw2), ptr(db2), B, H, W, ncls,
         ptr(yb), C, ptr(vec), C, ptr(rep[0]), ptr(rep[1]), 5)
    ref = torch.zeros(2, C, dtype=torch.float64, device=d)
    call("crimac_bn_bwd_reduce", P, ptr(dx2), C, ptr(yb), C, ptr(vec[2]), ptr(vec[3]), ptr(vec[0]), ptr(vec[1]), Mh,
         C, ptr(ref[0]), ptr(ref[1]))
    torch.cuda.synchronize()
    # (the two instantiations may contract the 3-term dot products differently: last-bit differences in dx)
    assert relerr(dx2, dx) < (1e-2 if prec in LOWP else 1e-6)
    assert relerr(rep[0].sum(0).cpu(), ref[0].cpu()) < 1e-5 and relerr(rep[1].sum(0).cpu(), ref[1].cpu()) < 1e-5
    assert relerr(from_nhwc(dx, B, H, W), xr.grad) < (1e-2 if prec in LOWP else 1e-4)
    assert relerr(dw.cpu().reshape(ncls, C, 1, 1), wr.grad) < 1e-4
    assert relerr(dbv.cpu(), br.grad) < 1e-4
    # every pixel ignored -> 0/0 = NaN like torch
    lab_all = torch.full((B, H, W), -100, dtype=torch.int64, device=d)
    sums = torch.zeros(2, dtype=torch.float64, device=d)
    call("crimac_wce_fwd", ptr(logits), ptr(lab_all), 8, ptr(cwd), ncls, -100, B, H, W, ptr(sums))
    assert bool(torch.isnan(sums[0] / sums[1]))


def test_sgd_momentum_matches_torch():
    g = torch.Generator().manual_seed(8)
    n = 1000 + 3
    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(3)]
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([pr], lr=0.005, momentum=0.95)
    p, v = p0.cuda(), torch.zeros(n, device="cuda")
    for gr in grads:
        pr.grad = gr.clone()
        opt.step()
        gd = gr.cuda()
        call("crimac_sgd_momentum", ptr(p), ptr(gd), ptr(v), n, 0.005, 0.95, 1.0, 1)
        torch.cuda.synchronize()
        assert float(gd.abs().max()) == 0.0
    assert relerr(p.cpu(), pr.detach()) < 1e-6


def test_nchw_to_nhwc_padding():
    x = torch.randn(2, 4, 8, 8)
    for prec in PRECS:
        out = torch.full((2 * 64, 16), 9.0, dtype=_dt(prec), device="cuda")
        xd = x.cuda()
        call("crimac_nchw_to_nhwc", hip.PREC_NAMES[prec], ptr(xd), ptr(out), 2, 4, 8, 8, 16)
        torch.cuda.synchronize()
        assert relerr(from_nhwc(out, 2, 8, 8, 4), _round(x, prec)) < 1e-6
        assert float(out[:, 4:].float().abs().max()) == 0


def test_bad_arguments_fail_loudly():
    t = torch.zeros(64, 64, device="cuda")
    with pytest.raises(hip.HipLibraryError, match="Cin"):
        call("crimac_igemm_conv", 0, ptr(t), 64, 1, 8, 8, 8, 8, 24, 64, 9, 3, 1, 1, ptr(t), None, None, 0,
             ptr(t), 64, 0, 0, 0)
    with pytest.raises(hip.HipLibraryError):
        hip.ptr(torch.zeros(4))          # CPU tensor: no fallback


# ---- conv3x3.hip: halo-staged kernel (the one the engine uses) -------------------------------------
def conv3x3_halo(prec, x_nhwc, in_ld, B, H, W, Cin, Cout, w_hi, w_lo, bias, relu=False, out=None,
                 out_ld=None, out_off=0, stats=None):
    if out is None:
        out = torch.empty(B * H * W, Cout, dtype=_dt(prec), device="cuda")
    out_ld = out_ld or Cout
    call("crimac_conv3x3", hip.PREC_NAMES[prec], ptr(x_nhwc), in_ld, B, H, W, Cin, Cout, ptr(w_hi),
         ptr(w_lo), ptr(bias), ptr(out, out_off), out_ld, 1 if relu else 0, 1 if stats is not None else 0,
         ptr(stats[0]) if stats is not None else None, ptr(stats[1]) if stats is not None else None,
         stats.shape[1] if stats is not None else 1, None, 0, None, 0)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(2, 16, 16, 64, 64), (1, 16, 32, 128, 128), (3, 8, 16, 256, 64),
                                   (2, 16, 16, 4, 64), (1, 24, 40, 64, 192), (2, 12, 20, 32, 128),
                                   (1, 32, 32, 576, 128), (5, 100, 120, 128, 64), (3, 256, 256, 64, 64),
                                   (2, 64, 64, 256, 256), (3, 21, 37, 4, 64), (2, 256, 256, 4, 64),
                                   (10, 100, 120, 64, 64),        # (persistent 64->64 kernel, ragged tiles)
                                   (5, 250, 200, 64, 128), (3, 120, 136, 128, 256)])   # (channel-split kernel, more than
                                   # two resident rounds of workgroups: 1040 / 432 tiles, ragged on both edges, 1 and 2 chunks)
def test_conv3x3_halo_forward_stats(prec, shape):
    """Forward incl. fused bias/ReLU and fused BatchNorm statistics; partial tiles (H%8, W%16 != 0);
    odd number of (chunk, tap) steps (Cin = 64, 576) and even (Cin = 128); the last two shapes have more
    tiles than CUs, so the persistent N = 64 kernel walks several tiles per workgroup."""
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(11)
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    b = torch.randn(Co, generator=g)
    cin_pad = 16 if Ci < 16 else Ci
    fh, fl, _, _ = pack_conv(w, prec, cin_pad, dgrad=False)
    ref = F.conv2d(x, _round(w, prec), b, padding=1)
    xin, bd = to_nhwc(x, prec, ld=cin_pad), b.cuda()
    stats = torch.zeros(2, 5, Co, dtype=torch.float64, device="cuda")      # 5 replicas
    out = conv3x3_halo(prec, xin, cin_pad, B, H, W, cin_pad, Co, fh, fl, bd, stats=stats)
    assert relerr(from_nhwc(out, B, H, W), ref) < TOL[prec]
    stored = out.double()
    assert relerr(stats[0].sum(0).cpu(), stored.sum(0).cpu()) < 1e-5
    assert relerr(stats[1].sum(0).cpu(), (stored * stored).sum(0).cpu()) < 1e-5
    out = conv3x3_halo(prec, xin, cin_pad, B, H, W, cin_pad, Co, fh, fl, bd, relu=True)
    assert relerr(from_nhwc(out, B, H, W), torch.relu(ref)) < TOL[prec]


@pytest.mark.parametrize("prec", PRECS)
def test_conv3x3_halo_strided_io_and_dgrad(prec):
    B, H, W, Ci, Co = 2, 16, 16, 64, 128
    g = torch.Generator().manual_seed(12)
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / 24
    fh, fl, dh, dl = pack_conv(w, prec)
    ref = F.conv2d(x, _round(w, prec), None, padding=1)
    big_in = torch.zeros(B * H * W, 2 * Ci, dtype=_dt(prec), device="cuda")
    big_in[:, Ci:] = to_nhwc(x, prec)
    big_out = torch.full((B * H * W, 3 * Co), 7.0, dtype=_dt(prec), device="cuda")
    call("crimac_conv3x3", hip.PREC_NAMES[prec], ptr(big_in, Ci), 2 * Ci, B, H, W, Ci, Co, ptr(fh), ptr(fl),
         None, ptr(big_out, Co), 3 * Co, 0, 0, None, None, 1, None, 0, None, 0)
    torch.cuda.synchronize()
    assert relerr(from_nhwc(big_out[:, Co:2 * Co].contiguous(), B, H, W), ref) < TOL[prec]
    assert float((big_out[:, :Co].float() - 7).abs().max()) == 0 and \
        float((big_out[:, 2 * Co:].float() - 7).abs().max()) == 0
    dy = _round(torch.randn(B, Co, H, W, generator=g), prec)
    refg = torch.nn.grad.conv2d_input((B, Ci, H, W), _round(w, prec), dy, padding=1)
    dyn = to_nhwc(dy, prec)
    dx = conv3x3_halo(prec, dyn, Co, B, H, W, Co, Ci, dh, dl, None)
    assert relerr(from_nhwc(dx, B, H, W), refg) < TOL[prec]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(2, 16, 16, 64, 128), (1, 24, 40, 128, 64), (2, 32, 32, 128, 256),
                                   (3, 256, 256, 64, 64), (5, 256, 256, 64, 64), (7, 120, 100, 64, 64),     # (persistent 64->64 kernel: 768 / 1280 tiles)
                                   (5, 250, 200, 128, 64), (3, 120, 136, 256, 128)])     # (dgrad to 128 / 256 channels, > 2 resident rounds)
def test_conv3x3_dgrad_with_fused_bn_backward_sums(prec, shape):
    """stat_mode 2: the dgrad convolution also produces sum dz / sum dz*xhat of the BatchNorm block its
    output feeds (== crimac_bn_bwd_reduce on (da, y))."""
    B, H, W, Ci, Co = shape          # conv Ci -> Co forward; dgrad maps dy[Co] -> da[Ci]
    g = torch.Generator().manual_seed(21)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    dy = _round(torch.randn(B, Co, H, W, generator=g), prec)
    y_prev = _round(torch.randn(B, Ci, H, W, generator=g) * 1.5 + 0.3, prec)     # saved conv output of the fed block
    mean, invstd = torch.randn(Ci, generator=g) * 0.2, torch.rand(Ci, generator=g) + 0.5
    scale, shift = (torch.rand(Ci, generator=g) + 0.5) * invstd, torch.randn(Ci, generator=g) * 0.3
    _, _, dh, dl = pack_conv(w, prec)
    M = B * H * W
    R = 7
    dyn, yn = to_nhwc(dy, prec), to_nhwc(y_prev, prec)
    vec = torch.stack([mean, invstd, scale, shift]).contiguous().cuda()      # row stride Ci
    acc = torch.zeros(2, R, Ci, dtype=torch.float64, device="cuda")
    da = torch.empty(M, Ci, dtype=_dt(prec), device="cuda")
    call("crimac_conv3x3", hip.PREC_NAMES[prec], ptr(dyn), Co, B, H, W, Co, Ci, ptr(dh), ptr(dl), None, ptr(da), Ci,
         0, 2, ptr(acc[0]), ptr(acc[1]), R, ptr(yn), Ci, ptr(vec), Ci)
    # reference: the stand-alone reduction kernel on the SAME stored da
    ref = torch.zeros(2, Ci, dtype=torch.float64, device="cuda")
    call("crimac_bn_bwd_reduce", hip.PREC_NAMES[prec], ptr(da), Ci, ptr(yn), Ci, ptr(vec[2]), ptr(vec[3]),
         ptr(vec[0]), ptr(vec[1]), M, Ci, ptr(ref[0]), ptr(ref[1]))
    out = torch.zeros(2, Ci, dtype=torch.float64, device="cuda")
    call("crimac_sum_replicas", ptr(acc[0]), R, Ci, Ci, ptr(out[0]), None, ptr(acc[1]), ptr(out[1]))
    torch.cuda.synchronize()
    refg = torch.nn.grad.conv2d_input((B, Ci, H, W), _round(w, prec), dy, padding=1)
    assert relerr(from_nhwc(da, B, H, W), refg) < TOL[prec]
    assert relerr(out[0].cpu(), ref[0].cpu()) < 1e-5 and relerr(out[1].cpu(), ref[1].cpu()) < 1e-5


@pytest.mark.parametrize("shape", [(2, 8, 8, 128, 64), (1, 12, 20, 256, 128), (2, 64, 64, 256, 128)])
@pytest.mark.parametrize("prec", LOWP)
def test_upconv_dgrad_with_fused_bn_backward_sums(shape, prec):
    """crimac_upconv2x2_dgrad_bnb == crimac_igemm_conv (input gradient) + crimac_bn_bwd_reduce on its output."""
    B, H, W, Ci, Co = shape          # transposed conv Ci -> Co (coarse H x W -> fine 2H x 2W)
    g = torch.Generator().manual_seed(23)
    w = torch.randn(Ci, Co, 2, 2, generator=g) / Ci ** 0.5
    dy = _round(torch.randn(B, Co, 2 * H, 2 * W, generator=g), prec)
    y_prev = _round(torch.randn(B, Ci, H, W, generator=g) * 1.5 + 0.3, prec)
    mean, invstd = torch.randn(Ci, generator=g) * 0.2, torch.rand(Ci, generator=g) + 0.5
    scale, shift = (torch.rand(Ci, generator=g) + 0.5) * invstd, torch.randn(Ci, generator=g) * 0.3
    i16 = dict(dtype=torch.int16, device="cuda")
    n = 4 * Ci * Co
    fh, fl, dh, dl = (torch.empty(2 * n, **i16) for _ in range(4))
    wd = w.cuda()
    call("crimac_pack_upconv2x2", ptr(wd), Ci, Co, NPL[prec], ptr(fh), ptr(fl), ptr(dh), ptr(dl))
    M, R = B * H * W, 6
    dyn, yn = to_nhwc(dy, prec), to_nhwc(y_prev, prec)
    vec = torch.stack([mean, invstd, scale, shift]).contiguous().cuda()
    acc = torch.zeros(2, R, Ci, dtype=torch.float64, device="cuda")
    dx = torch.empty(M, Ci, dtype=_dt(prec), device="cuda")
    P = hip.PREC_NAMES[prec]
    if prec == "bf16":               # (the entry point without `prec` is the bf16 form)
        call("crimac_upconv2x2_dgrad_bnb", ptr(dyn), Co, B, H, W, Co, Ci, ptr(dh), ptr(dx), Ci, ptr(yn), Ci, ptr(vec),
             Ci, ptr(acc[0]), ptr(acc[1]), R)
    else:
        call("crimac_upconv2x2_dgrad_bnb_prec", P, ptr(dyn), Co, B, H, W, Co, Ci, ptr(dh), ptr(dx), Ci, ptr(yn), Ci,
             ptr(vec), Ci, ptr(acc[0]), ptr(acc[1]), R)
    plain = torch.empty(M, Ci, dtype=_dt(prec), device="cuda")
    call("crimac_igemm_conv", P, ptr(dyn), Co, B, 2 * H, 2 * W, H, W, Co, Ci, 4, 2, 0, 2, ptr(dh), ptr(dl),
         None, 0, ptr(plain), Ci, 0, 0, 0)
    ref = torch.zeros(2, Ci, dtype=torch.float64, device="cuda")
    call("crimac_bn_bwd_reduce", P, ptr(dx), Ci, ptr(yn), Ci, ptr(vec[2]), ptr(vec[3]), ptr(vec[0]), ptr(vec[1]),
         M, Ci, ptr(ref[0]), ptr(ref[1]))
    out = torch.zeros(2, Ci, dtype=torch.float64, device="cuda")
    call("crimac_sum_replicas", ptr(acc[0]), R, Ci, Ci, ptr(out[0]), None, ptr(acc[1]), ptr(out[1]))
    torch.cuda.synchronize()
    assert torch.equal(dx, plain)
    xg = torch.zeros(B, Ci, H, W, requires_grad=True)
    F.conv_transpose2d(xg, _round(w, prec), None, stride=2).backward(dy)
    assert relerr(from_nhwc(dx, B, H, W), xg.grad) < TOL[prec]
    assert relerr(out[0].cpu(), ref[0].cpu()) < 1e-5 and relerr(out[1].cpu(), ref[1].cpu()) < 1e-5
    # shapes the kernel does not cover fail loudly
    with pytest.raises(hip.HipLibraryError):
        call("crimac_upconv2x2_dgrad_bnb", ptr(dyn), Co, B, H, W, Co, 96, ptr(dh), ptr(dx), 96, ptr(yn), 96, ptr(vec), 96,
             ptr(acc[0]), ptr(acc[1]), R)


@pytest.mark.parametrize("shape", [(2, 24, 40, 128, 256), (3, 256, 256, 64, 128), (1, 16, 16, 64, 128)])
@pytest.mark.parametrize("prec", LOWP)
def test_conv3x3_cols_two_ranges_equal_the_full_convolution(shape, prec):
    """crimac_conv3x3_cols on [0, N/2) and [N/2, N) (weights / bias / out / accumulators of the FULL convolution)
    reproduces crimac_conv3x3 bit for bit, statistics included; unsupported ranges fail loudly.  The second shape
    takes the persistent 64-channel kernel for each half, the first the channel-split kernel, the third (64-channel halves
    on a small image) the tall form."""
    B, H, W, Ci, Co = shape
    P = hip.PREC_NAMES[prec]
    g = torch.Generator().manual_seed(41)
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    bd = torch.randn(Co, generator=g).cuda()
    fh, fl, _, _ = pack_conv(w, prec, Ci, dgrad=False)
    xin = to_nhwc(x, prec)
    M = B * H * W
    full = torch.empty(M, Co, dtype=_dt(prec), device="cuda")
    st_full = torch.zeros(2, 4, Co, dtype=torch.float64, device="cuda")
    call("crimac_conv3x3", P, ptr(xin), Ci, B, H, W, Ci, Co, ptr(fh), ptr(fl), ptr(bd), ptr(full), Co, 1, 1,
         ptr(st_full[0]), ptr(st_full[1]), 4, None, 0, None, 0)
    half = Co // 2
    parts = torch.zeros(M, Co, dtype=_dt(prec), device="cuda")
    st = torch.zeros(2, 4, Co, dtype=torch.float64, device="cuda")
    args = lambda n0, n=half: ("crimac_conv3x3_cols", P, ptr(xin), Ci, B, H, W, Ci, Co, ptr(fh), ptr(fl), ptr(bd), ptr(parts), Co,
                               1, 1, ptr(st[0]), ptr(st[1]), 4, None, 0, None, 0, n0, n)
    # ranges are multiples of 64 channels (128: channel-split kernel; 64 of a 64-input-channel convolution with >= 512
    # tiles: persistent kernel; any other 64: the tall form) -- anything else fails loudly
    with pytest.raises(hip.HipLibraryError):
        call(*args(0, 32))
    with pytest.raises(hip.HipLibraryError):
        call(*args(Co - 64, 128))
    call(*args(0))
    call(*args(half))
    torch.cuda.synchronize()
    assert torch.equal(parts, full)
    assert relerr(st.sum(1), st_full.sum(1)) < 1e-6       # (fp32 partial sums are grouped differently)


@pytest.mark.parametrize("planes", [1, 2, 3, hip.PLANES_FP16, hip.PLANES_F32H3])
def test_whole_network_pack_and_unpack_equal_the_per_layer_kernels(planes):
    """crimac_pack_layers / crimac_unpack_wgrad_layers (one launch for all layers) are bit-identical to
    the per-layer kernels, incl. the padded first layer (Ci = 4 -> 16, no dgrad planes)."""
    import ctypes
    g = torch.Generator().manual_seed(5)
    layers = [(0, 64, 4, 16), (0, 128, 64, 64), (1, 64, 128, 128), (0, 64, 192, 192), (1, 32, 64, 64)]
    keep, descs = [], (hip.LayerDesc * len(layers))()
    i16 = torch.int16
    for d, (kind, Co, Ci, Cp) in zip(descs, layers):
        T = 9 if kind == 0 else 4
        shape = (Co, Ci, 3, 3) if kind == 0 else (Ci, Co, 2, 2)
        w = torch.randn(*shape, generator=g).cuda()
        n = T * Co * Cp
        dw = torch.randn(n, generator=g).cuda()
        has_dg = Cp == Ci
        nl = max((planes & 15) - 1, 1)
        new = {k: torch.full((m,), -1, dtype=i16, device="cuda") for k, m in
               (("fwd_hi", n), ("fwd_lo", nl * n), ("dg_hi", n), ("dg_lo", nl * n))}
        old = {k: torch.full_like(v, -1) for k, v in new.items()}
        grad_new, grad_old = torch.zeros_like(w), torch.zeros_like(w)
        if kind == 0:
            call("crimac_pack_conv3x3", ptr(w), Co, Ci, Cp, None, planes, ptr(old["fwd_hi"]), ptr(old["fwd_lo"]),
                 ptr(old["dg_hi"]) if has_dg else None, ptr(old["dg_lo"]) if has_dg else None)
            call("crimac_unpack_wgrad_conv3x3", ptr(dw), Co, Ci, Cp, ptr(grad_old))
        else:
            call("crimac_pack_upconv2x2", ptr(w), Ci, Co, planes, ptr(old["fwd_hi"]), ptr(old["fwd_lo"]),
                 ptr(old["dg_hi"]), ptr(old["dg_lo"]))
            call("crimac_unpack_wgrad_upconv2x2", ptr(dw), Ci, Co, ptr(grad_old))
        d.w, d.grad, d.dw = w.data_ptr(), grad_new.data_ptr(), dw.data_ptr()
        d.fwd_hi, d.fwd_lo = new["fwd_hi"].data_ptr(), new["fwd_lo"].data_ptr()
        d.dg_hi = new["dg_hi"].data_ptr() if has_dg else None
        d.dg_lo = new["dg_lo"].data_ptr() if has_dg else None
        d.kind, d.Co, d.Ci, d.Ci_pad = kind, Co, Ci, Cp
        keep.append((w, dw, new, old, grad_new, grad_old, has_dg))
    call("crimac_pack_layers", ctypes.byref(descs), len(layers), planes)
    call("crimac_unpack_wgrad_layers", ctypes.byref(descs), len(layers))
    # a sub-range of the table (what the engine does per backward group)
    torch.cuda.synchronize()
    for li, (w, dw, new, old, grad_new, grad_old, has_dg) in enumerate(keep):
        for k in new:
            if (planes & 15) == 1 and k.endswith("_lo"):
                continue
            assert torch.equal(new[k], old[k]), (li, k)
        assert torch.equal(grad_new, grad_old), li
    keep[2][4].zero_()
    keep[1][4].zero_()
    call("crimac_unpack_wgrad_layers", ctypes.byref(descs, 2 * ctypes.sizeof(hip.LayerDesc)), 1)
    torch.cuda.synchronize()
    assert torch.equal(keep[2][4], keep[2][5]) and float(keep[1][4].abs().max()) == 0


def _wfrag_index(t, r, c, R, K):
    """common.h wfrag_index, vectorised (c % 8 == 0: position of the 8 columns c .. c + 7 of row r at tap t)."""
    blk = (t * (R // 32) + r // 32) * (K // 64) + c // 64
    return ((blk * 4 + ((c % 64) // 32) * 2 + (r % 32) // 16) * 64 + ((c % 32) // 8) * 16 + r % 16) * 8


@pytest.mark.parametrize("prec", LOWP)
@pytest.mark.parametrize("shape", [(2, 32, 48, 128, 128), (1, 24, 40, 128, 256), (3, 16, 16, 256, 128), (2, 64, 32, 128, 64),
                                   (1, 40, 24, 64, 192)])
def test_rows_form_of_the_channel_split_convolution(prec, shape):
    """CRIMAC_EPI_WROWS (round 5): 64-channel x (32 x 16)-pixel tiles, a wave = 16 channels x all 32 image rows, the loop over
    halo rows (every fragment meets the three row taps).  Same products as the tap loop in another order: against the
    row-major launch to the storage type's last bit (statistics / BatchNorm-backward sums to fp32 round-off), against a
    float64 convolution of the same rounded operands to the storage rounding; images that are not multiples of the tile
    (24 x 40, 16 x 16), 64-channel outputs and ranges, forward with statistics and input gradient with the fused sums."""
    import ctypes
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(37)
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)).cuda()
    planes = hip.PREC_PLANES_ARG[hip.PREC_NAMES[prec]]
    n = 9 * Co * Ci
    i16 = torch.int16
    bufs = {}
    for tag, kind in (("row", 0), ("frag", hip.LAYER_FWD_FRAG | hip.LAYER_DG_FRAG)):
        d = (hip.LayerDesc * 1)()
        bufs[tag] = {k: torch.full((n,), -1, dtype=i16, device="cuda") for k in ("fwd_hi", "dg_hi")}
        lo = torch.zeros(8, dtype=i16, device="cuda")
        d[0].w = w.data_ptr()
        d[0].fwd_hi, d[0].fwd_lo = bufs[tag]["fwd_hi"].data_ptr(), lo.data_ptr()
        d[0].dg_hi, d[0].dg_lo = bufs[tag]["dg_hi"].data_ptr(), lo.data_ptr()
        d[0].kind, d[0].Co, d[0].Ci, d[0].Ci_pad = kind, Co, Ci, Ci
        call("crimac_pack_layers", ctypes.byref(d), 1, planes)
    x4 = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    dy4 = _round(torch.randn(B, Co, H, W, generator=g), prec)
    x, dy = to_nhwc(x4, prec), to_nhwc(dy4, prec)
    bias = torch.randn(Co, generator=g).cuda()
    yprev = to_nhwc(_round(torch.randn(B, Ci, H, W, generator=g) * 1.5 + 0.3, prec), prec)
    vec = torch.stack([torch.randn(Ci, generator=g) * 0.2, torch.rand(Ci, generator=g) + 0.5,
                       torch.rand(Ci, generator=g) + 0.5, torch.randn(Ci, generator=g) * 0.3]).contiguous().cuda()
    M, P = B * H * W, hip.PREC_NAMES[prec]
    res = {}
    for tag, flag in (("row", 0), ("frag", hip.EPI_WFRAG | hip.EPI_WROWS)):
        out = torch.empty(M, Co, dtype=_dt(prec), device="cuda")
        st = torch.zeros(2, 3, Co, dtype=torch.float64, device="cuda")
        call("crimac_conv3x3", P, ptr(x), Ci, B, H, W, Ci, Co, ptr(bufs[tag]["fwd_hi"]), None, ptr(bias), ptr(out), Co,
             hip.EPI_RELU | flag, 1, ptr(st[0]), ptr(st[1]), 3, None, 0, None, 0)
        da = torch.empty(M, Ci, dtype=_dt(prec), device="cuda")
        acc = torch.zeros(2, 3, Ci, dtype=torch.float64, device="cuda")
        call("crimac_conv3x3", P, ptr(dy), Co, B, H, W, Co, Ci, ptr(bufs[tag]["dg_hi"]), None, None, ptr(da), Ci, flag, 2,
             ptr(acc[0]), ptr(acc[1]), 3, ptr(yprev), Ci, ptr(vec), Ci)
        half = torch.zeros(M, Ci, dtype=_dt(prec), device="cuda")      # the second 64-channel range of the input gradient alone
        if Ci >= 128:
            call("crimac_conv3x3_cols", P, ptr(dy), Co, B, H, W, Co, Ci, ptr(bufs[tag]["dg_hi"]), None, None, ptr(half), Ci,
                 flag, 0, None, None, 1, None, 0, None, 0, 64, 64)
        torch.cuda.synchronize()
        res[tag] = (out, st.sum(1), da, acc.sum(1), half)
    ulp = 2.0 ** -7 if prec == "bf16" else 2.0 ** -10          # spacing of the storage type relative to a binade's lower end
    for k in (0, 2):
        a, b = res["frag"][k].double(), res["row"][k].double()
        assert float(((a - b).abs() / b.abs().clamp_min(1e-2)).max()) <= 1.01 * ulp, k      # the storage type's last bit
        assert float((a != b).double().mean()) < 0.02
    assert relerr(res["frag"][1].cpu(), res["row"][1].cpu()) < 1e-4 and relerr(res["frag"][3].cpu(), res["row"][3].cpu()) < 2e-3
    if Ci >= 128:
        assert torch.equal(res["frag"][4][:, 64:128], res["frag"][2][:, 64:128]) and float(res["frag"][4][:, :64].float().abs().max()) == 0
    if Ci > 128:
        assert float(res["frag"][4][:, 128:].float().abs().max()) == 0
    # float64 convolution of the rounded operands (weights as packed: the plane's rounding)
    wq = _round(w.cpu(), prec).double()
    ref = torch.relu(torch.nn.functional.conv2d(x4.double(), wq, bias.cpu().double(), padding=1))
    got = res["frag"][0].double().cpu().reshape(B, H, W, Co).permute(0, 3, 1, 2)
    assert relerr(got, ref) < 1.5 * ulp
    refd = torch.nn.functional.conv_transpose2d(dy4.double(), wq, padding=1)
    gotd = res["frag"][2].double().cpu().reshape(B, H, W, Ci).permute(0, 3, 1, 2)
    assert relerr(gotd, refd) < 1.5 * ulp


@pytest.mark.parametrize("prec", LOWP)
@pytest.mark.parametrize("shape", [(2, 32, 48, 128, 128), (1, 24, 40, 128, 256), (3, 16, 16, 256, 128)])
def test_fragment_major_weight_planes_pack_and_convolve_bit_for_bit(prec, shape):
    """CRIMAC_LAYER_FWD_FRAG / CRIMAC_LAYER_DG_FRAG + CRIMAC_EPI_WFRAG (round 5): crimac_pack_layers writes the planes the
    channel-split kernel reads in fragment-major order -- a permutation of the row-major plane in 16-byte units -- and the
    convolution on them (forward with statistics, input gradient with the fused BatchNorm-backward sums, a 128-channel range of
    the input gradient) is BIT-identical to the convolution on the row-major plane."""
    import ctypes
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(31)
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)).cuda()
    planes = hip.PREC_PLANES_ARG[hip.PREC_NAMES[prec]]
    n = 9 * Co * Ci
    i16 = torch.int16
    bufs = {}
    for tag, kind in (("row", 0), ("frag", hip.LAYER_FWD_FRAG | hip.LAYER_DG_FRAG)):
        d = (hip.LayerDesc * 1)()
        bufs[tag] = {k: torch.full((n,), -1, dtype=i16, device="cuda") for k in ("fwd_hi", "dg_hi")}
        lo = torch.zeros(8, dtype=i16, device="cuda")
        d[0].w = w.data_ptr()
        d[0].fwd_hi, d[0].fwd_lo = bufs[tag]["fwd_hi"].data_ptr(), lo.data_ptr()
        d[0].dg_hi, d[0].dg_lo = bufs[tag]["dg_hi"].data_ptr(), lo.data_ptr()
        d[0].kind, d[0].Co, d[0].Ci, d[0].Ci_pad = kind, Co, Ci, Ci
        call("crimac_pack_layers", ctypes.byref(d), 1, planes)
    torch.cuda.synchronize()
    # the fragment-major plane is the row-major plane with its 16-byte units moved to wfrag_index
    for key, R, K in (("fwd_hi", Co, Ci), ("dg_hi", Ci, Co)):
        t, r, c = np.meshgrid(np.arange(9), np.arange(R), np.arange(0, K, 8), indexing="ij")
        src = ((t * R + r) * K + c).reshape(-1)
        dst = _wfrag_index(t, r, c, R, K).reshape(-1)
        assert len(set(dst.tolist())) == len(dst) and dst.max() == 9 * R * K - 8
        row = bufs["row"][key].cpu().numpy().reshape(-1, 8)
        frag = bufs["frag"][key].cpu().numpy().reshape(-1, 8)
        assert np.array_equal(frag[dst // 8], row[src // 8]), key
    x = to_nhwc(_round(torch.randn(B, Ci, H, W, generator=g), prec), prec)
    dy = to_nhwc(_round(torch.randn(B, Co, H, W, generator=g), prec), prec)
    bias = torch.randn(Co, generator=g).cuda()
    yprev = to_nhwc(_round(torch.randn(B, Ci, H, W, generator=g) * 1.5 + 0.3, prec), prec)
    vec = torch.stack([torch.randn(Ci, generator=g) * 0.2, torch.rand(Ci, generator=g) + 0.5,
                       torch.rand(Ci, generator=g) + 0.5, torch.randn(Ci, generator=g) * 0.3]).contiguous().cuda()
    M, P = B * H * W, hip.PREC_NAMES[prec]
    res = {}
    for tag, flag in (("row", 0), ("frag", hip.EPI_WFRAG)):
        out = torch.empty(M, Co, dtype=_dt(prec), device="cuda")
        st = torch.zeros(2, 3, Co, dtype=torch.float64, device="cuda")
        call("crimac_conv3x3", P, ptr(x), Ci, B, H, W, Ci, Co, ptr(bufs[tag]["fwd_hi"]), None, ptr(bias), ptr(out), Co,
             hip.EPI_RELU | flag, 1, ptr(st[0]), ptr(st[1]), 3, None, 0, None, 0)
        da = torch.empty(M, Ci, dtype=_dt(prec), device="cuda")
        acc = torch.zeros(2, 3, Ci, dtype=torch.float64, device="cuda")
        call("crimac_conv3x3", P, ptr(dy), Co, B, H, W, Co, Ci, ptr(bufs[tag]["dg_hi"]), None, None, ptr(da), Ci, flag, 2,
             ptr(acc[0]), ptr(acc[1]), 3, ptr(yprev), Ci, ptr(vec), Ci)
        half = None
        if Ci % 256 == 0:                      # the second 128-channel range of the input gradient alone (decoder conv1)
            half = torch.zeros(M, Ci, dtype=_dt(prec), device="cuda")
            call("crimac_conv3x3_cols", P, ptr(dy), Co, B, H, W, Co, Ci, ptr(bufs[tag]["dg_hi"]), None, None, ptr(half), Ci,
                 flag, 0, None, None, 1, None, 0, None, 0, Ci // 2, Ci // 2)
        torch.cuda.synchronize()
        res[tag] = (out, st.sum(1), da, half)
    assert torch.equal(res["row"][0], res["frag"][0]) and torch.equal(res["row"][2], res["frag"][2])
    assert relerr(res["frag"][1].cpu(), res["row"][1].cpu()) < 1e-9
    if res["row"][3] is not None:
        assert torch.equal(res["row"][3], res["frag"][3]) and float(res["frag"][3][:, Ci // 2:].float().abs().max()) > 0
        assert torch.equal(res["frag"][3][:, Ci // 2:], res["frag"][2][:, Ci // 2:])
    # and what the planes cannot serve fails loudly: a 64-channel range, a split precision
    with pytest.raises(hip.HipLibraryError, match="fragment-major"):
        call("crimac_conv3x3_cols", P, ptr(dy), Co, B, H, W, Co, Ci, ptr(bufs["frag"]["dg_hi"]), None, None, ptr(res["frag"][2]),
             Ci, hip.EPI_WFRAG, 0, None, None, 1, None, 0, None, 0, 0, 64)
    with pytest.raises(hip.HipLibraryError, match="fragment-major"):
        call("crimac_conv3x3", hip.PREC_F32X6, ptr(x), Ci, B, H, W, Ci, Co, ptr(bufs["frag"]["fwd_hi"]), ptr(bufs["frag"]["fwd_hi"]),
             None, ptr(res["frag"][0]), Co, hip.EPI_WFRAG, 0, None, None, 1, None, 0, None, 0)


@pytest.mark.parametrize("prec", ["bf16", "fp16", "f32x3"])
@pytest.mark.parametrize("mode,shape", [(0, (2, 64, 64, 64, 128)), (1, (2, 32, 32, 128, 64)), (0, (1, 40, 24, 16, 64))])
def test_wgrad_partial_slabs_sum_to_the_atomic_result_and_are_reproducible(prec, mode, shape):
    """crimac_wgrad_partials: one slab per pixel split by plain stores (no zero fill, no atomics);
    crimac_unpack_wgrad_layers adds the slabs in order.  Equals crimac_wgrad (+ per-layer unpack) and the torch
    reference, and two runs are bit-identical (the atomic form is not)."""
    import ctypes
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(29)
    P = hip.PREC_NAMES[prec]
    lib = hip.load_library()
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    if mode == 0:
        dy = _round(torch.randn(B, Co, H, W, generator=g), prec)
        ref = torch.nn.grad.conv2d_weight(x, (Co, Ci, 3, 3), dy, padding=1)
        F_, S_, CF, CS, taps, shape_w, kind = to_nhwc(dy, prec), to_nhwc(x, prec), Co, Ci, 9, (Co, Ci, 3, 3), 0
    else:
        dy = _round(torch.randn(B, Co, 2 * H, 2 * W, generator=g), prec)
        wg = torch.zeros(Ci, Co, 2, 2, requires_grad=True)
        F.conv_transpose2d(x, wg, None, stride=2).backward(dy)
        ref = wg.grad
        F_, S_, CF, CS, taps, shape_w, kind = to_nhwc(x, prec), to_nhwc(dy, prec), Ci, Co, 4, (Ci, Co, 2, 2), 1
    n = taps * CF * CS
    for target in (0, 24):
        sp = lib.crimac_wgrad_splits(P, mode, CF, CS, B, H, W, target)
        assert sp >= 1
        stride = n + 64
        outs = []
        for rep in range(2):
            slabs = torch.full((sp * stride,), float("nan"), dtype=torch.float32, device="cuda")   # no zero fill needed
            call("crimac_wgrad_partials", P, mode, ptr(F_), CF, CF, ptr(S_), CS, CS, B, H, W, ptr(slabs), stride, target)
            grad = torch.zeros(*shape_w, dtype=torch.float32, device="cuda")
            d = (hip.LayerDesc * 1)()
            d[0].grad, d[0].dw, d[0].kind = grad.data_ptr(), slabs.data_ptr(), kind
            d[0].Co, d[0].Ci, d[0].Ci_pad = Co, Ci, Ci
            d[0].dw_splits, d[0].dw_stride = sp, stride
            if Co % 32 == 0 and (kind == 0 or Ci % 32 == 0):
                call("crimac_unpack_wgrad_layers", ctypes.byref(d), 1)
                torch.cuda.synchronize()
            else:
                torch.cuda.synchronize()
                summed = slabs.view(sp, stride)[:, :n].sum(0)
                grad = (summed.view(9, Co, Ci).permute(1, 2, 0).reshape(Co, Ci, 3, 3) if kind == 0
                        else summed.view(4, Ci, Co).permute(1, 2, 0).reshape(Ci, Co, 2, 2)).contiguous()
            assert bool(torch.isfinite(slabs.view(sp, stride)[:, :n]).all())        # every slab element was written
            outs.append(grad.clone())
        assert torch.equal(outs[0], outs[1])
        assert relerr(outs[0].cpu(), ref) < (2e-4 if prec in LOWP else 1e-4)
        dwp = torch.zeros(n, dtype=torch.float32, device="cuda")
        call("crimac_wgrad", P, mode, ptr(F_), CF, CF, ptr(S_), CS, CS, B, H, W, ptr(dwp), target)
        torch.cuda.synchronize()
        summed = (dwp.view(9, Co, Ci).permute(1, 2, 0).reshape(Co, Ci, 3, 3) if kind == 0
                  else dwp.view(4, Ci, Co).permute(1, 2, 0).reshape(Ci, Co, 2, 2))
        assert relerr(outs[0], summed) < 1e-5


@pytest.mark.parametrize("shape", [(2, 16, 16, 64, 64), (1, 16, 32, 128, 128), (2, 16, 16, 4, 64), (1, 24, 40, 64, 192)])
def test_conv3x3_forward_f32h3_fp16_planes(shape):
    """CRIMAC_PREC_F32H3: fp32 storage, two fp16 planes per operand (weights packed x 2^8, undone in the epilogue),
    3 MFMAs per product: ~2^-21 per product -- fp32-class, 30x tighter than the bf16 2-plane split (f32x3)."""
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, Ci, H, W, generator=g) * 3.0
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    b = torch.randn(Co, generator=g)
    cin_pad = 16 if Ci < 16 else Ci
    fh, fl, _, _ = pack_conv(w, "f32h3", cin_pad, dgrad=False)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).float()
    xin = to_nhwc(x, "f32h3", ld=cin_pad)
    out = torch.empty(B * H * W, Co, dtype=torch.float32, device="cuda")
    bd = b.cuda()
    call("crimac_conv3x3", hip.PREC_NAMES["f32h3"], ptr(xin), cin_pad, B, H, W, cin_pad, Co, ptr(fh), ptr(fl), ptr(bd),
         ptr(out), Co, 1, 0, None, None, 1, None, 0, None, 0)
    torch.cuda.synchronize()
    e = relerr(from_nhwc(out, B, H, W), torch.relu(ref))
    assert e < 2e-6, e
    out2 = conv3x3("f32h3", xin, cin_pad, B, H, W, cin_pad, Co, fh, fl, bd)          # gather implementation
    assert relerr(from_nhwc(out2, B, H, W), ref) < 2e-6
    # the backward-only entry point refuses the forward-operand mode
    dwp = torch.zeros(9 * Co * cin_pad, dtype=torch.float32, device="cuda")
    with pytest.raises(hip.HipLibraryError, match="forward-operand"):
        call("crimac_wgrad", hip.PREC_NAMES["f32h3"], 0, ptr(out), Co, Co, ptr(xin), cin_pad, cin_pad, B, H, W, ptr(dwp), 0)


@pytest.mark.parametrize("prec", ["bf16", "fp16", "f32x3"])
@pytest.mark.parametrize("shape", [(2, 32, 32, 128, 128), (3, 256, 256, 64, 64), (9, 256, 256, 64, 64), (1, 24, 40, 64, 64),
                                   (2, 16, 48, 256, 128)])
def test_conv3x3_with_fused_maxpool_equals_conv_then_pool(prec, shape):
    """crimac_conv3x3_pool (eval encoder tail): the output equals crimac_conv3x3 bit for bit and pool_out equals
    crimac_bn_act_pool (identity + 2x2 max-pool) of it -- channel-split kernel, persistent 64-channel kernel
    (3 x 256 x 256: 768 tiles), pixel-split kernel with partial tiles, and the fp32 register-staged kernel."""
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(51)
    P = hip.PREC_NAMES[prec]
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    bd = torch.randn(Co, generator=g).cuda()
    fh, fl, _, _ = pack_conv(w, prec, Ci, dgrad=False)
    xin = to_nhwc(x, prec)
    M = B * H * W
    ld_o, ld_p = Co + 8, Co + 16                       # channel slices of wider buffers
    ref = torch.zeros(M, ld_o, dtype=_dt(prec), device="cuda")
    call("crimac_conv3x3", P, ptr(xin), Ci, B, H, W, Ci, Co, ptr(fh), ptr(fl), ptr(bd), ptr(ref), ld_o, 1, 0,
         None, None, 1, None, 0, None, 0)
    pool_ref = torch.zeros(M // 4, ld_p, dtype=_dt(prec), device="cuda")
    call("crimac_bn_act_pool", P, ptr(ref), ld_o, None, None, 0, None, 0, ptr(pool_ref), ld_p, B, H, W, Co)
    out = torch.zeros(M, ld_o, dtype=_dt(prec), device="cuda")
    pool = torch.zeros(M // 4, ld_p, dtype=_dt(prec), device="cuda")
    call("crimac_conv3x3_pool", P, ptr(xin), Ci, B, H, W, Ci, Co, ptr(fh), ptr(fl), ptr(bd), ptr(out), ld_o, 1,
         ptr(pool), ld_p)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert torch.equal(pool, pool_ref) and float(pool[:, :Co].float().abs().max()) > 0
    pr = F.max_pool2d(torch.relu(F.conv2d(x, _round(w, prec), bd.cpu(), padding=1)), 2, 2)
    assert relerr(from_nhwc(pool, B, H // 2, W // 2, Co), pr) < TOL[prec]
    with pytest.raises(hip.HipLibraryError):           # odd size: refused, not silently wrong
        call("crimac_conv3x3_pool", P, ptr(xin), Ci, B, H - 1, W, Ci, Co, ptr(fh), ptr(fl), ptr(bd), ptr(out), ld_o, 1,
             ptr(pool), ld_p)


@pytest.mark.parametrize("prec", LOWP)
@pytest.mark.parametrize("target", [2, 8, 24])
def test_wgrad_two_teams_long_tile_queue(prec, target):
    """The 8-wave weight-gradient kernel (16-bit conv3x3): few workgroups with LONG tile queues (target_blocks 2 ->
    one workgroup per channel pair with 256 tiles, 8 -> 64 tiles, 24 -> a ragged last split), so both teams take many
    tiles from the queue in LDS, finish at different times and meet in the accumulator exchange; against torch."""
    B, H, W, Ci, Co = 2, 128, 128, 128, 64
    g = torch.Generator().manual_seed(91)
    x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
    dy = _round(torch.randn(B, Co, H, W, generator=g), prec)
    ref = torch.nn.grad.conv2d_weight(x, (Co, Ci, 3, 3), dy, padding=1)
    P = hip.PREC_NAMES[prec]
    dyn, xn = to_nhwc(dy, prec), to_nhwc(x, prec)
    outs = []
    for rep in range(2):
        dwp = torch.zeros(9 * Co * Ci, dtype=torch.float32, device="cuda")
        call("crimac_wgrad", P, 0, ptr(dyn), Co, Co, ptr(xn), Ci, Ci, B, H, W, ptr(dwp), target)
        grad = torch.empty(Co, Ci, 3, 3, dtype=torch.float32, device="cuda")
        call("crimac_unpack_wgrad_conv3x3", ptr(dwp), Co, Ci, Ci, ptr(grad))
        torch.cuda.synchronize()
        outs.append(grad.cpu())
        assert relerr(outs[-1], ref) < 1e-4
    # (the queue makes the tile -> team assignment timing dependent: equal up to the order of fp32 additions)
    assert relerr(outs[0], outs[1]) < 1e-5


@pytest.mark.parametrize("prec", LOWP)
@pytest.mark.parametrize("items", [0, 24])
def test_grouped_weight_gradients_equal_the_torch_reference(prec, items):
    """crimac_wgrad_group: the conv3x3 weight gradients of several layers through ONE persistent launch with per-XCD item
    queues -- full-size tiles with hundreds of items per queue, ragged images (partial tiles on both edges), channel
    counts that are not multiples of the 64 x 64 tile, a layer that lives in a channel slice of a wider buffer (ld > C),
    layers with fewer splits than XCDs -- each against torch's conv2d_weight on the same (16-bit exact) operands.
    items = 24: a plan with few, long items per layer (every workgroup runs several tiles per item and several items)."""
    import ctypes
    lib = hip.load_library()
    P = hip.PREC_NAMES[prec]
    g = torch.Generator().manual_seed(41)
    #        B,  H,   W,  Ci,  Co, ld_x (0: Ci)
    specs = [(2, 128, 128, 64, 64, 0), (2, 100, 120, 64, 128, 0), (2, 20, 24, 128, 64, 256), (2, 16, 16, 256, 96, 0),
             (2, 8, 48, 72, 64, 0), (2, 32, 32, 512, 256, 0)]
    B = 2
    keep, arr = [], (hip.WgradGroupLayer * len(specs))()
    for d, (_, H, W, Ci, Co, ldx) in zip(arr, specs):
        x = _round(torch.randn(B, Ci, H, W, generator=g), prec)
        dy = _round(torch.randn(B, Co, H, W, generator=g), prec)
        ref = torch.nn.grad.conv2d_weight(x, (Co, Ci, 3, 3), dy, padding=1)
        xn = to_nhwc(x, prec, ld=ldx or Ci)
        dyn = to_nhwc(dy, prec)
        dwp = torch.zeros(9 * Co * Ci, dtype=torch.float32, device="cuda")
        keep.append((xn, dyn, dwp, ref, Ci, Co))
        d.f, d.f_ld, d.CF = dyn.data_ptr(), Co, Co
        d.s, d.s_ld, d.CS = xn.data_ptr(), ldx or Ci, Ci
        d.Hf, d.Wf, d.dw = H, W, dwp.data_ptr()
    counts = (ctypes.c_int * 8)()
    cap = lib.crimac_wgrad_group_plan(P, arr, len(specs), B, items, None, 0, counts)
    assert cap > 0, lib.crimac_last_error()
    host = torch.zeros(8 * cap * 2, dtype=torch.int32)
    assert lib.crimac_wgrad_group_plan(P, arr, len(specs), B, items, ctypes.c_void_p(host.data_ptr()), cap, counts) == cap
    dev_items = host.cuda()
    ctr = torch.zeros(8, dtype=torch.int32, device="cuda")
    call("crimac_wgrad_group", P, ctypes.byref(arr), len(specs), B, ptr(dev_items), cap, ctypes.byref(counts), ptr(ctr))
    torch.cuda.synchronize()
    assert ctr.cpu().tolist() >= list(counts)          # every queue was drained (workgroups overshoot by their last fetch)
    for (xn, dyn, dwp, ref, Ci, Co), sp in zip(keep, specs):
        grad = torch.empty(Co, Ci, 3, 3, dtype=torch.float32, device="cuda")
        call("crimac_unpack_wgrad_conv3x3", ptr(dwp), Co, Ci, Ci, ptr(grad))
        torch.cuda.synchronize()
        assert relerr(grad.cpu(), ref) < 2e-4, sp
    # a second launch on the same queues needs fresh counters: with the old ones nothing runs (and nothing hangs)
    before = keep[0][2].clone()
    call("crimac_wgrad_group", P, ctypes.byref(arr), len(specs), B, ptr(dev_items), cap, ctypes.byref(counts), ptr(ctr))
    torch.cuda.synchronize()
    assert torch.equal(before, keep[0][2])


@pytest.mark.parametrize("prec", list(LOWP) + ["h3p"])
def test_backward_with_grouped_weight_gradients_equals_the_ungrouped_backward(prec):
    """The engine's backward pass with the conv3x3 weight gradients grouped per gradient range (the default), grouped three
    layers at a time, and with one launch per layer (UNetEngine.wgrad_group = False) -- on the SAME saved forward pass (two forward
    passes of a 16-bit net differ at rounding level and their gradients by O(10 %)): every gradient equal up
    to the order of the fp32 atomics."""
    import crimac_classifiers_unet_amd as pkg
    from crimac_classifiers_unet_amd import synth
    x = torch.from_numpy(synth.synth_echogram_batch(3, 4, 64, 96, seed=81)).cuda()
    lab = torch.from_numpy(synth.synth_labels(3, 64, 96, seed=82)).cuda()
    cw = torch.tensor([10.0, 300.0, 250.0], device="cuda")
    m = pkg.UNet_Baseline(3, 4, precision=prec)
    m.load_state_dict(synth.synth_state_dict(seed=0))
    m.cuda().train()
    eng = m.engine
    logits = eng.forward(x, training=True)
    sums, labels = eng.ce_forward(logits, lab, cw)
    dl = eng.ce_backward(logits, labels, cw, sums, float(eng.loss_scale))
    res = {}
    eng.wgrad_group_h3p = True                    # (off by default for plane pairs: slower in the step; still tested)
    for tag, grouped, nlayers in (("base", False, 16), ("again", False, 16), ("range", True, 16), ("three", True, 3)):
        eng.wgrad_group, eng.wgrad_group_layers = grouped, nlayers
        eng.backward(dl)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(eng.flat_g).all())
        res[tag] = eng.flat_g.clone()
        assert eng._wg_launches == {"base": 0, "again": 0, "range": 4, "three": 7}[tag]
    base = res["base"]
    assert float(base.abs().max()) > 0

    def dist(a):
        return float((a - base).double().norm() / base.double().norm())
    # two runs of the SAME backward pass already differ: the BatchNorm-backward sums are added up by fp32 atomics in
    # arrival order, an output gradient that lands on the other side of a 16-bit rounding boundary moves by an ulp
    # (bf16: 0.4 %), and the layers below see it.  The grouped launches must sit inside that noise.
    noise = dist(res["again"])
    print(f"{prec}: run-to-run {noise:.2e}, grouped per range {dist(res['range']):.2e}, three at a time {dist(res['three']):.2e}")
    for k in ("range", "three"):
        assert dist(res[k]) < max(3 * noise, 1e-3), (k, dist(res[k]), noise)
    # and the weight gradient of the LAST decoder convolution -- the first dy of the backward pass, computed before any
    # such rounding difference exists -- agrees to the order of its fp32 atomics
    o, n, _ = eng.layout[f"up_convs.{eng.depth - 2}.conv2.weight"]
    for k in ("range", "three"):
        a, b = res[k][o:o + n].double(), base[o:o + n].double()
        assert float((a - b).norm() / b.norm()) < 3e-4, k


@pytest.mark.parametrize("prec", ["bf16", "fp16", "f32x6", "h3p", "h3f"])
@pytest.mark.parametrize("shape", [(2, 16, 24, 64), (1, 8, 8, 512), (3, 32, 32, 128), (2, 64, 64, 64)])
def test_unpool_bn_bwd_apply_rebuilds_the_gradient_bit_for_bit(prec, shape):
    """crimac_unpool_bn_bwd_apply_replicas (round 4) against the two kernels it replaces on the same inputs and the SAME
    replica accumulators: crimac_unpool_add stores da = ds + unpool(dp) and takes the BatchNorm-backward sums,
    crimac_bn_bwd_apply_replicas turns (da, y) into dy; the fused kernel rebuilds da from (dp, ds, y).  dy, dgamma, dbeta:
    identical bits, in every storage family (h3p: dy as fp16 plane pairs; h3f: fp32 in, fp16 dy)."""
    B, H, W, C = shape
    M, Mp = B * H * W, B * (H // 2) * (W // 2)
    g = torch.Generator().manual_seed(91)
    fwd = {"h3p": hip.PREC_H3P, "h3f": hip.PREC_H3P}.get(prec, hip.PREC_NAMES.get(prec))       # precision of unpool_add
    app = {"h3p": hip.PREC_H3P, "h3f": hip.PREC_H3F_BWD}.get(prec, hip.PREC_NAMES.get(prec))   # ... of the apply pass
    dt = _DT.get(prec, torch.float32)                        # storage of dp, ds, y, da
    dy_dt = {"h3p": torch.float32, "h3f": torch.float16}.get(prec, dt)      # (plane pairs: 4 bytes per element)
    y = (torch.randn(M, C, generator=g) * 2).to(dt).cuda()
    # ties in the pooled activation (equal maxima, and whole windows at zero after the ReLU) are the interesting case
    y[: M // 3] = (y[: M // 3].float().round()).to(dt)
    dp = torch.randn(Mp, C, generator=g).to(dt).cuda()
    ds = torch.randn(M, C, generator=g).to(dt).cuda()
    stride = C + 8
    vec = torch.zeros(4, stride)
    vec[0, :C] = torch.randn(C, generator=g) * 0.3                       # mean
    vec[1, :C] = torch.rand(C, generator=g) + 0.5                        # invstd
    vec[2, :C] = (torch.rand(C, generator=g) + 0.5) * vec[1, :C]         # scale = gamma * invstd
    vec[3, :C] = torch.randn(C, generator=g) * 0.5 - vec[0, :C] * vec[2, :C]
    vec = vec.cuda()
    nrep = 16
    s0 = torch.zeros(nrep, C, dtype=torch.float64, device="cuda")
    s1 = torch.zeros(nrep, C, dtype=torch.float64, device="cuda")
    da = torch.empty(M, C, dtype=dt, device="cuda")
    a_dummy = torch.zeros(8, dtype=torch.float32, device="cuda")         # (not read when the sums are fused)
    call("crimac_unpool_add", fwd, ptr(dp), C, ptr(a_dummy), C, ptr(ds), C, ptr(da), C, B, H, W, C,
         ptr(y), C, ptr(vec), stride, ptr(s0), ptr(s1), nrep)
    # the sums-only form accumulates the same sums (fp64 atomics: compare after the replicas are added up)
    t0, t1 = torch.zeros_like(s0), torch.zeros_like(s1)
    call("crimac_unpool_add", fwd, ptr(dp), C, ptr(a_dummy), C, ptr(ds), C, None, 0, B, H, W, C,
         ptr(y), C, ptr(vec), stride, ptr(t0), ptr(t1), nrep)
    torch.cuda.synchronize()
    assert relerr(t0.sum(0), s0.sum(0)) < 1e-5 and relerr(t1.sum(0), s1.sum(0)) < 1e-5      # (fp32 partial sums per workgroup)
    out = {}
    for fused in (False, True):
        dy = torch.full((M, C), float("nan"), dtype=dy_dt, device="cuda")
        dg = torch.empty(C, dtype=torch.float32, device="cuda")
        db = torch.empty(C, dtype=torch.float32, device="cuda")
        if fused:
            call("crimac_unpool_bn_bwd_apply_replicas", app, ptr(dp), C, ptr(ds), C, ptr(y), C, ptr(vec), stride, ptr(s0),
                 ptr(s1), nrep, M, ptr(dy), C, B, H, W, C, ptr(dg), ptr(db))
        else:
            call("crimac_bn_bwd_apply_replicas", app, ptr(da), C, ptr(y), C, ptr(vec), stride, ptr(s0), ptr(s1), nrep, M, M, C,
                 ptr(dy), C, ptr(dg), ptr(db))
        torch.cuda.synchronize()
        out[fused] = (dy, dg, db)
    raw = (lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16))
    if not torch.equal(raw(out[True][0]), raw(out[False][0])):
        a_, b_ = out[True][0].float(), out[False][0].float()
        bad = (a_ != b_).nonzero()
        i0 = bad[0]
        raise AssertionError(f"dy differs at {len(bad)} of {a_.numel()} elements, first {i0.tolist()}: {a_[tuple(i0)].item()!r} vs "
                             f"{b_[tuple(i0)].item()!r}; max abs diff {float((a_ - b_).abs().max())}")
    assert torch.equal(out[True][1], out[False][1]) and torch.equal(out[True][2], out[False][2])
    assert bool(torch.isfinite(out[True][0].float()).all()) or prec == "h3p"
    # ... and without a skip gradient (ds = NULL)
    dy2 = torch.empty(M, C, dtype=dy_dt, device="cuda")
    call("crimac_unpool_bn_bwd_apply_replicas", app, ptr(dp), C, None, 0, ptr(y), C, ptr(vec), stride, ptr(s0), ptr(s1), nrep,
         M, ptr(dy2), C, B, H, W, C, ptr(out[True][1]), ptr(out[True][2]))
    da0 = torch.empty(M, C, dtype=dt, device="cuda")
    u0, u1 = torch.zeros_like(s0), torch.zeros_like(s1)
    call("crimac_unpool_add", fwd, ptr(dp), C, ptr(a_dummy), C, None, 0, ptr(da0), C, B, H, W, C, ptr(y), C, ptr(vec), stride,
         ptr(u0), ptr(u1), nrep)
    dy3 = torch.empty(M, C, dtype=dy_dt, device="cuda")
    call("crimac_bn_bwd_apply_replicas", app, ptr(da0), C, ptr(y), C, ptr(vec), stride, ptr(s0), ptr(s1), nrep, M, M, C,
         ptr(dy3), C, ptr(out[False][1]), ptr(out[False][2]))
    torch.cuda.synchronize()
    assert torch.equal(raw(dy2), raw(dy3))


def test_mfma_calibration_kernel_reports_a_plausible_rate_and_clock():
    """crimac_mfma_calibrate (bench.py's in-run ceiling, VERDICT r3 #1c): an MFMA-only launch of a known FLOP count -- its
    HIP-event time gives a dense bf16 rate between 1 and 2.6 PFLOP/s on an MI355X, the per-workgroup s_memtime /
    s_memrealtime stamps a shader clock between 1 and 2.6 GHz, and twice the iterations take about twice the time."""
    blocks = 512
    st = torch.zeros(2 * blocks, dtype=torch.int64, device="cuda")
    sink = torch.zeros(4, dtype=torch.float32, device="cuda")

    def run(iters):
        ts = []
        for k in range(4):
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record()
            call("crimac_mfma_calibrate", iters, blocks, ptr(st), ptr(sink))
            e_.record()
            e_.synchronize()
            if k:
                ts.append(s_.elapsed_time(e_))
        return sorted(ts)[1]
    ms = run(8000)
    tf = 2.0 * 16 * 16 * 32 * 8 * 8000 * 4 * blocks / (ms * 1e-3) / 1e12
    v = st.cpu().numpy().reshape(blocks, 2).astype(np.float64)
    ghz = float(np.median(v[:, 0] / np.maximum(v[:, 1], 1.0)) * 0.1)
    assert 1000.0 < tf < 2600.0, tf
    assert 1.0 < ghz < 2.6, ghz
    assert 1.7 < run(16000) / ms < 2.3
