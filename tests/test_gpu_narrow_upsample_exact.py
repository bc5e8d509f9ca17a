"""Exact-integer tests of the narrow kernels (narrow.hip), of the weight gradients at the narrow channel counts (wgrad.hip)
and of the up_mode="upsample" kernels (upsample.hip).

The recipe, the helpers and the guard-row buffers are those of tests/test_gpu_conv_exact.py (imported, not copied): ternary
operands, integer biases, power-of-two fold scales, every product and partial sum an integer below 2^24, every output exact
in bf16 and fp16 -- so no assertion here has a tolerance.  The bilinear kernels add the weights 1/16, 3/16, 9/16, 1/4, 3/4:
their operands are integers of at most 16 in magnitude, their outputs k / 16 with |k| <= 256, still exact in every storage
type and in any order of summation.  The preconditions (max|ref| <= 256 and 16-bit exact, per-channel sum(ref^2) < 2^24 where
statistics are fused, |ref| < 2^24 for weight gradients, |z| <= 16 and 16 * ref an integer for the bilinear cases) are
asserted ON THE REFERENCE by the builders; tests/test_narrow_upsample_exact_data_cpu.py runs every builder, the B = 800
ones included, without a GPU.  Importing this module needs no GPU.

Inputs and outputs live in channel slices (ld > C) with guard rows (4096 around inputs, 7 around outputs) asserted untouched
after every call; the transposed convolution and the bilinear forward write the up half of a concat buffer whose skip half
keeps its sentinel, their input gradients read the up half of a d(concat) buffer whose skip half holds 4096.

Kernel forms, what dispatches them, and the cases that reach them ("tall" = 1x1, 1x17, 3x2, 7x9, 17x33, 33x17; "wide" =
tall + 19x35; B = 2; "pairs" = the nine (Cin, N) of start_filts 8 / 16 / 32, "first" = w_cin 4 padded to Cin 16, N 8 / 16 / 32):
  * conv3x3_narrow_mfma_kernel<bf16_t | half_t, N> -- crimac_conv3x3_narrow in the 16-bit modes; 16 x 16 tiles, K = 9 Cin in
    steps of 32 (Cin = 8: 72 values in 3 steps, 24 zero weights; N = 8: half a fragment): pairs + first, wide (33 columns =
    three tile columns, the last ragged both ways), with ReLU, bias, scale and statistics; the input gradient
    (CRIMAC_NARROW_DGRAD) of every pair, whole and as the two halves of a decoder conv1 (w_col0 = cin / 2);
  * conv3x3_narrow_kernel<float, float, N> (f32x6), <hp_t, float, N> (h3p) and <hp_t, hp_t, N> (h3p with
    CRIMAC_EPI_OUT_PLANES) -- the 4-byte modes; 16 x 32 tiles (33x17: two tile rows): the same cases; plane-pair output on
    the first half of the two-halves input gradient;
  * the persistent loop of both: PERSIST_PARAMS, 800 images of 17 x 17 = 3200 (MFMA) / 1600 (VALU) tiles on at most
    4 x CUs workgroups, (8, 8) and (32, 64), bf16 and h3p, forward with statistics (tile % reps) and one input gradient;
  * upconv_narrow_fwd_kernel<TI, TO, 8 | 16 | 32> / upconv_narrow_dgrad_kernel<TI, TO, 16 | 32 | 64> --
    crimac_upconv2x2_narrow / crimac_upconv2x2_dgrad_narrow: (16, 8), (32, 16), (64, 32) on UP_SIZES; (TI, TO) = bf16, fp16,
    float / float, hp_t / float and, forward only, hp_t / hp_t;
  * crimac_wgrad at (CF, CS) = (N, Cin) (mode 0) and (Cin, Cout) (mode 1), target_blocks 0 / 1 / 3, then
    crimac_unpack_wgrad_conv3x3 / _upconv2x2.  The branch of wgrad_run each case takes:
      - bf16 / fp16, mode 0, CS <= 16 -- (8, 8), (8, 16), (16, 16), (16, 32), (16, 8) and first (CS = 16, CF = 8 / 16 / 32):
        launch<T, 1, 0, true, 2>, the two-team kernel's first-layer form (one 16-channel S fragment; CS = 8 fills half of it);
      - bf16 / fp16, mode 0, CS = 32 / 64 -- (32, 32), (32, 64), (32, 16), (64, 32): launch<T, 1, 0, false, 2>, the two-team
        kernel on partial channel tiles (CF < 64 and / or CS < 64);
      - bf16 / fp16, mode 1: launch<T, 1, 1>, the 4-wave kernel, CF = 16 / 32 / 64, CS = 8 / 16 / 32;
      - f32x3 (also the backward pass of f32h3): launch<float, 2, mode>; f32x6: launch<float, 3, mode>;
      - h3p: launch<hp_t, 2, mode>, the register-staged kernel -- wgrad_pp_kernel wants CF % 64 == 0 and CS % 64 == 0 or
        CS == 16, wgrad_up_pp_kernel CF % 128 == 0: no narrow layer meets either;
      - h3f's backward personality is not driven: the engine refuses precision 'h3f' for every transposed convolution with
        Cout % 64 != 0, i.e. for every narrow net;
  * up2x_kernel<T, T> behind crimac_igemm_conv (ntaps 1) -- crimac_conv1x1_up2x, bf16 / fp16 / f32x6; hp_to_f32_kernel, the
    F32H3 GEMM and up2x_kernel<float, hp_t> in h3p: (128, 64), (256, 128), (1024, 512) on UP_SIZES (H = 1, W = 1: the
    border clamp i1 = min(i0 + 1, n - 1));
  * up2x_adjoint_kernel<TP, TF> -- crimac_up2x_adjoint: ternary dy in the up half, C = 64 / 128 / 512, UP_SIZES;
  * crimac_conv1x1_dgrad (crimac_igemm_conv ntaps 1; F32H3 on fp32 dz in h3p) on freshly drawn ternary dz, UP_SIZES;
  * wgrad1x1_kernel<TF, TP> -- crimac_conv1x1_wgrad, accumulating into a pre-filled dw: M = 1, 9, 4100.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_conv_exact as ce
from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd.hip import call, ptr
from test_gpu_conv_exact import (IN_GUARD, OUT_GUARD, REPL, TALL, TINY, UP_SIZES, Guarded, g_in, g_out, nchw, nhwc,
                                 ternary)

gpu = pytest.mark.gpu

# (Cin, N) of every narrow conv3x3 of start_filts 8, 16, 32; Cin = 4: the first layer (4 channels padded to 16)
PAIRS = [(8, 8), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (16, 8), (32, 16), (64, 32)]
FIRST = [(4, 8), (4, 16), (4, 32)]
UP_PAIRS = [(16, 8), (32, 16), (64, 32)]
WIDE = ce._imgs(TALL + [(19, 35)])
FWD_PRECS = ("bf16", "fp16", "f32x6", "h3p", "h3p_planes")
BWD_PRECS = ("bf16", "fp16", "f32x6", "h3p")
WGRAD_PRECS = ("bf16", "fp16", "f32x3", "f32x6", "h3p")          # every backward precision of a narrow net (not h3f)
FWD_PARAMS = [(ci, n, p, img) for ci, n in PAIRS + FIRST for p in FWD_PRECS for img in WIDE]
DGRAD_PARAMS = [(ci, co, p, img) for ci, co in PAIRS for p in BWD_PRECS for img in WIDE]
HALVES_PARAMS = [(ci, co, p, img) for ci, co in PAIRS if ci == 2 * co for p in BWD_PRECS for img in WIDE]      # decoder conv1
# persistent loop: 17 x 17 images; the tile count must exceed 4 x CUs and be no multiple of the CU count
PERSIST_B, PERSIST_HW, PERSIST_LEVELS = 800, 17, 16
PERSIST_PARAMS = [(ci, n, p) for ci, n in ((8, 8), (32, 64)) for p in ("bf16", "h3p")]
UPN_FWD_PARAMS = [c + (p, img) for c in UP_PAIRS for p in FWD_PRECS for img in UP_SIZES]
UPN_BWD_PARAMS = [c + (p, img) for c in UP_PAIRS for p in BWD_PRECS for img in UP_SIZES]
WGRAD_PARAMS = [(0, ci, n, p, img) for ci, n in PAIRS + FIRST for p in WGRAD_PRECS for img in ce._imgs(TINY + [(9, 17)])] + \
               [(1,) + c + (p, img) for c in UP_PAIRS for p in WGRAD_PRECS for img in UP_SIZES]
UP1_CH = [(128, 64), (256, 128), (1024, 512)]
# operand density per cin (P(non-zero) = 2 / levels for x and for w): keeps z = W x + b within [-16, 16]
UP1_LEVELS = {128: 12, 256: 16, 1024: 32}
UP1_PARAMS = [c + (p, img) for c in UP1_CH for p in BWD_PRECS for img in UP_SIZES]
WG1_M = (1, 9, 4100)
WG1_PARAMS = [c + (p, m) for c in UP1_CH for p in BWD_PRECS for m in WG1_M]


# ---- data builders (CPU only) -------------------------------------------------------------------------------------------

def narrow_fwd_case(B, H, W, Ci, Co, levels=8):
    """ce.fwd_case with the statistics precondition (the fused sums of every narrow forward are asserted)."""
    return ce.fwd_case(B, H, W, Ci, Co, True, True, levels)


@functools.lru_cache(maxsize=None)
def narrow_dgrad_case(B, H, W, Ci, Co, sums=False):
    """ce.dgrad_case; sums: the column sums of the first half are fused (two-halves form) -> their precondition too."""
    c = ce.dgrad_case(B, H, W, Ci, Co)
    if sums:
        assert float((c["ref"] * c["ref"]).sum((0, 2, 3)).max()) < 2 ** 24, "precondition: per-channel sum(ref^2) < 2^24"
    return c


def _sixteenths(v, what):
    k = v * 16
    assert torch.equal(k, k.round()) and float(k.abs().max()) <= 256, f"precondition: {what} = k / 16 with |k| <= 256"
    assert torch.equal(v.bfloat16().double(), v) and torch.equal(v.half().double(), v), "precondition: 16-bit exact"


@functools.lru_cache(maxsize=None)
def up1x1_case(B, H, W, Ci, Co):
    """Upsample(bilinear, x2) + conv1x1 on the coarse grid H x W: x, w, b with z = W x + b an integer, |z| <= 16;
    ref = conv2d(interpolate(x)) = up(z); ternary dy -> dz = the adjoint; freshly drawn ternary dzt -> dx = W^T dzt."""
    g = torch.Generator().manual_seed(ce._seed(5, B, H, W, Ci, Co))
    lv = UP1_LEVELS[Ci]
    x, w = ternary((B, Ci, H, W), g, lv), ternary((Co, Ci, 1, 1), g, lv)
    b = torch.randint(-3, 4, (Co,), generator=g).double()
    z = F.conv2d(x, w, b)
    assert torch.equal(z, z.round()) and 0 < float(z.abs().max()) <= 16, "precondition: z an integer, |z| <= 16"
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False), w, b)
    _sixteenths(ref, "up(z)")
    ce._check_output(ref, False)
    dy = ternary((B, Co, 2 * H, 2 * W), g)
    zz = torch.zeros(B, Co, H, W, dtype=torch.float64, requires_grad=True)
    F.interpolate(zz, scale_factor=2, mode="bilinear", align_corners=False).backward(dy)
    dz = zz.grad
    _sixteenths(dz, "up^T(dy)")
    dzt = ternary((B, Co, H, W), g)
    dx = F.conv_transpose2d(dzt, w)
    ce._check_output(dx, False)
    return dict(x=x, w=w, b=b, z=z, ref=ref, dy=dy, dz=dz, dzt=dzt, dx=dx)


@functools.lru_cache(maxsize=None)
def wgrad1x1_case(M, Ci, Co):
    """conv1x1 weight gradient over M pixels, accumulated into dw0: ref = dz^T x + dw0 ([Co, Ci], integers)."""
    g = torch.Generator().manual_seed(ce._seed(6, M, Ci, Co))
    dz, x = ternary((M, Co), g), ternary((M, Ci), g)
    dw0 = torch.randint(-3, 4, (Co, Ci), generator=g).double()
    ref = dz.t() @ x + dw0
    assert float(ref.abs().max()) < 2 ** 24, "precondition: |ref| < 2^24"
    assert float((ref - dw0).abs().max()) > 0
    return dict(dz=dz, x=x, dw0=dw0, ref=ref)


def persist_tiles(prec):
    """Tiles of the persistent cases: 16 x 16 (MFMA form, 16-bit storage) or 16 wide x 32 high (VALU form)."""
    th = 16 if prec in ce.LOWP else 32
    return PERSIST_B * -(-PERSIST_HW // 16) * -(-PERSIST_HW // th)


def case_builders():
    """Every (builder, arguments) pair the GPU tests below use."""
    out = []
    out += [(narrow_fwd_case, img + (ci, n)) for ci, n, _, img in FWD_PARAMS]
    out += [(narrow_dgrad_case, img + (ci, co)) for ci, co, _, img in DGRAD_PARAMS]
    out += [(narrow_dgrad_case, img + (ci, co, True)) for ci, co, _, img in HALVES_PARAMS]
    for ci, n, _ in PERSIST_PARAMS:
        out.append((narrow_fwd_case, (PERSIST_B, PERSIST_HW, PERSIST_HW, ci, n, PERSIST_LEVELS)))
        out.append((narrow_dgrad_case, (PERSIST_B, PERSIST_HW, PERSIST_HW, ci, n)))
    out += [(ce.up_case, img + (ci, co)) for ci, co, _, img in UPN_FWD_PARAMS + UPN_BWD_PARAMS]
    out += [(ce.wgrad_case, (m,) + img + (ci, co)) for m, ci, co, _, img in WGRAD_PARAMS]
    out += [(up1x1_case, img + (ci, co)) for ci, co, _, img in UP1_PARAMS]
    out += [(wgrad1x1_case, (m, ci, co)) for ci, co, _, m in WG1_PARAMS]
    return sorted(set(out), key=lambda t: (t[0].__name__, tuple(map(int, t[1]))))


# ---- device helpers ------------------------------------------------------------------------------------------------------

def conv_narrow(prec, xin, B, H, W, Cin, N, wd, w_cin, col0, flags, scale, bias, out, out_col=0, st=None, stat_ld=0):
    """crimac_conv3x3_narrow into columns [out_col, out_col + N) of `out`; st: [2, REPL, stat_ld] accumulators."""
    s0, s1 = (ptr(st[0]), ptr(st[1])) if st is not None else (None, None)
    call("crimac_conv3x3_narrow", ce._P(prec), xin.p(), xin.ld, B, H, W, Cin, N, ptr(wd), w_cin, col0, flags, ptr(scale),
         ptr(bias), out.p(out_col), out.ld, s0, s1, REPL, stat_ld)
    torch.cuda.synchronize()


def replica_sums(ref, prec, reps=REPL):
    """[2, reps, C] float64: what each statistics replica must hold -- the sums over the tiles t with t % reps == r, tile
    index (b * tiles_y + by) * tiles_x + bx on 16 x 16 tiles (16-bit modes) or 16 wide x 32 high ones (4-byte modes)."""
    B, C, H, W = ref.shape
    th = 16 if ce._base(prec) in ce.LOWP else 32
    ty, tx = -(-H // th), -(-W // 16)
    tile = (torch.arange(B)[:, None, None] * ty + (torch.arange(H) // th)[None, :, None]) * tx + (torch.arange(W) // 16)
    out = torch.zeros(2, reps, C, dtype=torch.float64)
    for r in range(reps):
        m = (tile % reps == r)[:, None].double()
        out[0, r], out[1, r] = (ref * m).sum((0, 2, 3)), (ref * ref * m).sum((0, 2, 3))
    return out


def assert_replicas(st, ref, prec, c0=0, c1=None):
    """The sums over the replicas are exact (ce.assert_stats) and every replica holds the tiles the kernels assign to it:
    spreading the fp64 atomics over the replicas is the point of having them."""
    ce.assert_stats(st, ref, c0, c1)
    assert torch.equal(st.cpu()[:, :, c0:c1], replica_sums(ref[:, c0:c1], prec))


def narrow_forward(prec, c, B, H, W, w_cin, Cin_k, N, relus=(0, hip.EPI_RELU)):
    """Forward on case c with bias, eval-mode scale and fused statistics: output, sums, guards -- all exact."""
    planes = prec.endswith("_planes")
    wd, sc, bd = c["w"].float().cuda().contiguous(), c["s"].float().cuda(), c["b"].float().cuda()
    xin = g_in(c["x"], prec, W, Cin_k)
    for relu in relus:
        ref = torch.relu(c["ref"]) if relu else c["ref"]
        out, st = g_out(B * H * W, N, prec, W, planes), ce.stat_bufs(N)
        conv_narrow(prec, xin, B, H, W, Cin_k, N, wd, w_cin, 0, relu | (hip.EPI_OUT_PLANES if planes else 0), sc, bd, out,
                    st=st, stat_ld=N)
        assert torch.equal(nchw(out.values(), B, H, W), ref)
        out.assert_guards()
        assert_replicas(st, ref, prec)
    xin.assert_guards(0, 0)


def narrow_dgrad(prec, c, B, H, W, ci, co):
    """The whole layer's input gradient: dy [B, co] -> dx [B, ci] (kernel Cin = co, N = ci)."""
    wd = c["w"].float().cuda().contiguous()
    dyn = g_in(c["dy"], prec, W)
    out = g_out(B * H * W, ci, prec, W)
    conv_narrow(prec, dyn, B, H, W, co, ci, wd, ci, 0, hip.NARROW_DGRAD, None, None, out)
    assert torch.equal(nchw(out.values(), B, H, W), c["ref"])
    out.assert_guards()
    dyn.assert_guards(0, 0)


def concat_in(mat, C_other, prec, W, planes):
    """[M, C] operand in the up half (columns 0 .. C) of a guarded [M, C + C_other] buffer whose skip half holds 4096."""
    full = torch.cat([mat, torch.full((mat.shape[0], C_other), IN_GUARD, dtype=mat.dtype)], 1)
    return Guarded(full.shape[0], full.shape[1], ce._dt(prec), IN_GUARD, W, mat=full, planes=planes)


# ---- conv3x3_narrow -----------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("ci,n,prec,img", FWD_PARAMS)
def test_conv3x3_narrow_forward_is_exact(ci, n, prec, img):
    B, H, W = img
    narrow_forward(prec, narrow_fwd_case(B, H, W, ci, n), B, H, W, ci, 16 if ci == 4 else ci, n)


@gpu
@pytest.mark.parametrize("ci,co,prec,img", DGRAD_PARAMS)
def test_conv3x3_narrow_dgrad_is_exact(ci, co, prec, img):
    B, H, W = img
    narrow_dgrad(prec, narrow_dgrad_case(B, H, W, ci, co), B, H, W, ci, co)


@gpu
@pytest.mark.parametrize("ci,co,prec,img", HALVES_PARAMS)
def test_conv3x3_narrow_dgrad_in_two_halves_is_exact(ci, co, prec, img):
    """A decoder conv1 (ci = 2 co): d(concat) in two launches (w_col0 = 0 and ci / 2), the first with its column sums (the
    transposed convolution's bias gradient) and, in h3p, as plane pairs -- as the engine issues them."""
    B, H, W = img
    c = narrow_dgrad_case(B, H, W, ci, co, True)
    h = ci // 2
    wd = c["w"].float().cuda().contiguous()
    dyn = g_in(c["dy"], prec, W)
    out, st = g_out(B * H * W, ci, prec, W), ce.stat_bufs(ci)
    pl = prec == "h3p"
    conv_narrow(prec, dyn, B, H, W, co, h, wd, ci, 0, hip.NARROW_DGRAD | (hip.EPI_OUT_PLANES if pl else 0), None, None, out, 0,
                st=st, stat_ld=ci)
    conv_narrow(prec, dyn, B, H, W, co, h, wd, ci, h, hip.NARROW_DGRAD, None, None, out, h)
    first = out.values(0, h)
    if pl:
        first = ce.hp_unpack(out.buf[out.G:out.G + out.M, out.off:out.off + h]).double()
    assert torch.equal(nchw(first, B, H, W), c["ref"][:, :h])
    assert torch.equal(nchw(out.values(h, ci), B, H, W), c["ref"][:, h:])
    out.assert_guards()
    assert_replicas(st, c["ref"], prec, 0, h)
    dyn.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("ci,n,prec", PERSIST_PARAMS)
def test_conv3x3_narrow_persistent_loop_is_exact(ci, n, prec):
    """More tiles than any grid the launchers choose (at most 4 workgroups per CU), and no multiple of it: every workgroup
    walks several tiles through the same LDS, some one more than others; the statistics replica is tile % reps."""
    B, H, W = PERSIST_B, PERSIST_HW, PERSIST_HW
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = persist_tiles(prec)
    assert 4 * cus < tiles, (cus, tiles)
    assert all(tiles % (k * cus) != 0 for k in (1, 2, 3, 4)), (cus, tiles)
    narrow_forward(prec, narrow_fwd_case(B, H, W, ci, n, PERSIST_LEVELS), B, H, W, ci, ci, n, relus=(0,))
    narrow_dgrad(prec, narrow_dgrad_case(B, H, W, ci, n), B, H, W, ci, n)


# ---- transposed convolution on the narrow kernels -----------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("ci,co,prec,img", UPN_FWD_PARAMS)
def test_upconv2x2_narrow_forward_is_exact(ci, co, prec, img):
    B, H, W = img
    c = ce.up_case(B, H, W, ci, co)
    planes = prec.endswith("_planes")
    wd, bd = c["w"].float().cuda().contiguous(), c["b"].float().cuda()
    xin = g_in(c["x"], prec, W)
    cat = g_out(B * 4 * H * W, 2 * co, prec, 2 * W, planes)            # [up | skip]
    call("crimac_upconv2x2_narrow", ce._P(prec), xin.p(), xin.ld, B, H, W, ci, co, ptr(wd), ptr(bd), cat.p(), cat.ld,
         hip.EPI_OUT_PLANES if planes else 0)
    torch.cuda.synchronize()
    assert torch.equal(nchw(cat.values(0, co), B, 2 * H, 2 * W), c["ref"])
    cat.assert_guards(0, co)                                           # (the skip half keeps its sentinel)
    xin.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("ci,co,prec,img", UPN_BWD_PARAMS)
def test_upconv2x2_narrow_dgrad_is_exact(ci, co, prec, img):
    B, H, W = img
    c = ce.up_case(B, H, W, ci, co)
    wd = c["w"].float().cuda().contiguous()
    dcat = concat_in(nhwc(c["dy"]), co, prec, 2 * W, prec == "h3p")
    dx = g_out(B * H * W, ci, prec, W)
    call("crimac_upconv2x2_dgrad_narrow", ce._P(prec), dcat.p(), dcat.ld, B, H, W, co, ci, ptr(wd), dx.p(), dx.ld)
    torch.cuda.synchronize()
    assert torch.equal(nchw(dx.values(), B, H, W), c["dx"])
    dx.assert_guards()
    dcat.assert_guards(0, 0)


# ---- weight gradients at the narrow channel counts ----------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("mode,ci,co,prec,img", WGRAD_PARAMS)
def test_wgrad_narrow_channel_counts_is_exact(mode, ci, co, prec, img):
    B, H, W = img
    c = ce.wgrad_case(mode, B, H, W, ci, co)
    cpad = 16 if (mode == 0 and ci == 4) else ci
    f, CF, s, CS, taps = ce.wgrad_operands(mode, c, prec, W, cpad)
    n = taps * CF * CS
    for target in (0, 1, 3):
        dwp = torch.zeros(n + 128, dtype=torch.float32, device="cuda")      # beyond one dW: 64 zeros, then 64 sentinels
        dwp[n + 64:] = OUT_GUARD
        call("crimac_wgrad", ce._P(prec), mode, f.p(), f.ld, CF, s.p(), s.ld, CS, B, H, W, ptr(dwp), target)
        assert torch.equal(ce.unpack(mode, dwp, ci, co, cpad), c["ref"]), target
        assert float(dwp[n:n + 64].abs().max()) == 0 and float((dwp[n + 64:] - OUT_GUARD).abs().max()) == 0, target
    f.assert_guards(0, 0)
    s.assert_guards(0, 0)


# ---- up_mode="upsample": bilinear 2x + conv1x1 --------------------------------------------------------------------------

def _pack1x1(w, prec):
    from test_gpu_upsample import pack1x1
    return pack1x1(w, prec)


@gpu
@pytest.mark.parametrize("ci,co,prec,img", UP1_PARAMS)
def test_conv1x1_up2x_is_exact(ci, co, prec, img):
    B, H, W = img
    c = up1x1_case(B, H, W, ci, co)
    M = B * H * W
    fh, fl, _, _, _ = _pack1x1(c["w"], prec)
    xin = g_in(c["x"], prec, W)
    cat = g_out(4 * M, 2 * co, prec, 2 * W, prec == "h3p")              # [up | skip]; plane pairs in h3p
    nwork = M * (co + ci)
    work = torch.full((nwork + 64,), OUT_GUARD, dtype=torch.float32, device="cuda")
    bd = c["b"].float().cuda()
    call("crimac_conv1x1_up2x", ce._P(prec), xin.p(), xin.ld, B, H, W, ci, co, ptr(fh), ptr(fl), ptr(bd), ptr(work), cat.p(),
         cat.ld)
    torch.cuda.synchronize()
    assert torch.equal(nchw(cat.values(0, co), B, 2 * H, 2 * W), c["ref"])
    cat.assert_guards(0, co)
    assert float((work[nwork:] - OUT_GUARD).abs().max()) == 0
    xin.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("ci,co,prec,img", UP1_PARAMS)
def test_up2x_adjoint_and_conv1x1_dgrad_are_exact(ci, co, prec, img):
    B, H, W = img
    c = up1x1_case(B, H, W, ci, co)
    M = B * H * W
    P = ce._P(prec)
    PB = hip.PREC_BACKWARD.get(P, P)
    dcat = concat_in(nhwc(c["dy"]), co, prec, 2 * W, prec == "h3p")
    dz = g_out(M, co, prec, W)                                          # (fp32 in h3p, else the storage type)
    call("crimac_up2x_adjoint", PB, dcat.p(), dcat.ld, B, H, W, co, dz.p(), dz.ld)
    torch.cuda.synchronize()
    assert torch.equal(nchw(dz.values(), B, H, W), c["dz"])
    dz.assert_guards()
    dcat.assert_guards(0, 0)
    # input gradient of the conv1x1 from a freshly drawn ternary dz (in the adjoint's output storage)
    _, _, dh, dl, _ = _pack1x1(c["w"], prec)
    dzt = Guarded(M, co, ce._dt_out(prec), IN_GUARD, W, mat=nhwc(c["dzt"]))
    dx = g_out(M, ci, prec, W)
    call("crimac_conv1x1_dgrad", PB, dzt.p(), dzt.ld, B, H, W, co, ci, ptr(dh), ptr(dl), dx.p(), dx.ld)
    torch.cuda.synchronize()
    assert torch.equal(nchw(dx.values(), B, H, W), c["dx"])
    dx.assert_guards()
    dzt.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("ci,co,prec,M", WG1_PARAMS)
def test_conv1x1_wgrad_accumulates_exactly(ci, co, prec, M):
    c = wgrad1x1_case(M, ci, co)
    P = ce._P(prec)
    PB = hip.PREC_BACKWARD.get(P, P)
    dz = Guarded(M, co, ce._dt_out(prec), IN_GUARD, 4, mat=c["dz"])
    x = Guarded(M, ci, ce._dt(prec), IN_GUARD, 4, mat=c["x"], planes=prec == "h3p")
    dw = torch.full((co * ci + 64,), OUT_GUARD, dtype=torch.float32, device="cuda")
    dw[:co * ci] = c["dw0"].float().reshape(-1).cuda()
    call("crimac_conv1x1_wgrad", PB, dz.p(), dz.ld, co, x.p(), x.ld, ci, M, ptr(dw))
    torch.cuda.synchronize()
    assert torch.equal(dw[:co * ci].cpu().double().view(co, ci), c["ref"])
    assert float((dw[co * ci:] - OUT_GUARD).abs().max()) == 0
    dz.assert_guards(0, 0)
    x.assert_guards(0, 0)
