"""Exact-integer tests of the MFMA contraction kernels (conv3x3.hip, conv3x3_glds.hip, igemm.hip, upconv.hip, wgrad.hip).

Operands on which EVERY kernel form, in EVERY precision mode, must reproduce a float64 reference bit for bit: activations,
output gradients and weights drawn from {-1, 0, +1} with P(non-zero) = 1/4, biases integers in [-3, 3], BatchNorm-fold
scales in {1, 2}.  These are exact in bf16 and fp16 and in the hi plane of every split (the lo planes are 0); every product
and partial sum is an integer below 2^24, so fp32 accumulation is exact in any order (atomics and per-workgroup statistics
included); outputs are integers of at most 256 in magnitude (or twice such an integer), exact in the bf16 store.  So no
assertion here has a tolerance: one dropped, duplicated or misplaced product fails ``torch.equal``.  The norm-wise tests of
tests/test_gpu_kernels.py / test_gpu_h3p.py cannot see such a term at K = 9 * Cin >= 576 in the 16-bit modes.
tests/test_gpu_narrow_upsample_exact.py holds narrow.hip, upsample.hip and the weight gradients at the narrow channel counts
to the same bar, with the helpers of this module.

The preconditions (max|ref| <= 256 and bf16-exact, per-channel sum(ref^2) < 2^24 where statistics are fused, |ref| < 2^24
for weight gradients, per-channel sum|terms| < 2^24 for the BatchNorm-backward sums) are asserted ON THE REFERENCE by the
builders below; tests/test_conv_exact_data_cpu.py runs the builders of every case (except the two persistent-kernel
shapes) without a GPU.  Importing this module needs no GPU.

Inputs and outputs live in channel slices (ld > C) of larger allocations with guard rows before and after: 4096 in the
input guards (a read past the image shows up in the sum), 7 in the output guards, asserted untouched after every call.

stat_mode 2 (BatchNorm-backward sums): y integers in [-3, 3], mean integers, invstd and |scale| in {0.5, 1, 2}, shift an integer
plus 0.25 (never a tie) -- the ReLU decision y * scale + shift > 0 and every term dz * (y - mean) * invstd are exact dyadic numbers
in every form, so both sums are asserted exactly too: no form needed the tolerance fallback.

Kernel forms, the dispatch condition that selects them, and the cases that reach them ("tiny" = images 1x1, 1x17, 3x2, 7x9,
17x33 at B = 2; "tall" = tiny + 33x17):
  * first-layer kernel conv3x3_c16_kernel -- crimac_conv3x3, 16-bit prec, Cin == 16, N == 64 (conv3x3_run); plane pairs with
    CRIMAC_EPI_CIN4 (fp32 and plane-pair output): FWD_FORMS "c16", tiny + (3, 21, 37);
  * channel-split kernel, 128-channel form launch_wch<.., 0> -- 16-bit / plane pairs, Cin % 64 == 0, N % 128 == 0, tensor
    below 2 GB (glds_dispatch, crimac_conv3x3_glds_hp): "wch128" 64 -> 128 tiny, DEEP (1, 5, 7, 1024, 256);
  * the same with the fragment-major plane (CRIMAC_EPI_WFRAG, launch_wch<.., 0, true>): "wch128_frag", DEEP;
  * tall form launch_wch<.., 2> -- N == 64 and Cin != 64 (16-bit), 64-channel ranges of crimac_conv3x3_cols on < 512 tiles,
    every 64-channel range of plane pairs: "tall" 128 -> 64 (and plane pairs 64 -> 64), COLS cases with 64-channel ranges;
  * rows form launch_wch<.., 3, true> -- CRIMAC_EPI_WFRAG | CRIMAC_EPI_WROWS: "rows64" 64 -> 64, "rows128" 128 -> 128, tall;
  * pixel-split kernel with the LDS weight ring launch_w4<64> -- 16-bit, Cin == 64, N % 128 != 0, fewer than 512 full
    tiles: "w4" 64 -> 64 tiny, (1, 9, 18, 64, 192);
  * persistent 64 -> 64 kernel launch_p64 -- 16-bit, N == Cin == 64, H, W % 16 == 0, >= 512 tiles: P64_SHAPES
    (2, 256, 256) and (1, 304, 432) = 513 tiles, statistics, BatchNorm-backward sums and the fused pool;
  * register-staged kernel conv3x3_kernel -- the fp32 split modes (f32x3, f32x6, f32h3) at any Cin % 16 == 0, 16-bit modes
    at Cin % 64 != 0; BK = 32 when Cin % 32 == 0 (Cin = 64 included), else 16; BN = 128 / 64 by N % 128: "staged*" (64, 128),
    (96, 64), (48, 128); the fp32 precisions of the "c16" rows (Cin = 16, N = 64) take this kernel with BK = 16, NOT the
    first-layer kernel;
  * igemm_kernel through crimac_igemm_conv with 9 taps: the same channel counts; BK = 64 when Cin % 64 == 0 and fewer than
    three planes, else 32 / 16: IGEMM_CASES (16-bit and fp32 modes; the entry point takes plane pairs for the transposed
    convolution only);
  * crimac_conv3x3_pool on 2x2, 2x18, 18x34: POOL_FORMS (128-channel form row- and fragment-major, tall, rows64, rows128,
    pixel-split, register-staged; plane pairs to fp32 and to plane pairs; the persistent kernel in the P64 test);
    crimac_conv3x3_cols with n_first != 0: COLS_CASES, and the persistent kernel's 64-channel range in the P64 test;
  * input gradient = the dgrad planes through the same forms: DGRAD_CASES 128 -> 64 (dy has 64 channels: N = 128, wch128)
    and 64 -> 128 (N = 64, Cin = 128: tall); stat_mode 2 on 7x9 and 17x33; fragment-major dgrad planes (128-channel and rows
    forms): DGRAD_FRAG_CASES;
  * 'h3f' = CRIMAC_PREC_H3F_BWD, the backward personality of that mode (fp16 gradient operand, plane-pair activation operand
    read through its hi plane, fp32 output; crimac_conv3x3_glds_16_f32out forms 0 / 2 / 3, fp16 output with
    CRIMAC_EPI_OUT_PLANES): the input gradient with and without stat_mode 2, row- and fragment-major,
    crimac_upconv2x2_dgrad_bnb_prec, crimac_wgrad modes 0 / 1 (4-byte element size on the activation operand) and
    crimac_wgrad_group.  Not its first-layer weight gradient (CS = 16): tests/test_gpu_h3p.py does not drive that either;
  * transposed convolution: upconv_wch_kernel when crimac_upconv_wch_ok (16-bit, K % 64 == 0, N % 128 == 0): 128 -> 64 and
    256 -> 128, forward scatter and input gradient; igemm_kernel otherwise: every fp32 mode, and 64 -> 48 in the 16-bit
    modes (forward N = 192, input gradient K = 48: both rejected by crimac_upconv_wch_ok); plane pairs forward with
    plane-pair output; crimac_upconv2x2_dgrad_bnb[_prec] on 5x20 and 7x33;
  * weight gradients: two-team kernel (16-bit, mode 0), its narrow-S form (CS == 16), the 4-wave kernel (mode 1, fp32
    splits), wgrad_pp_kernel / wgrad_up_pp_kernel (plane pairs): WGRAD_CASES with target_blocks 0, 1, 3; crimac_wgrad_partials;
    crimac_wgrad_group (the entry point takes 3x3 layers with Cin >= 64 only: a three-layer list of those, each layer at its
    own resolution); f32x6 (three planes) on two images per family.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd.hip import call, ptr

gpu = pytest.mark.gpu

TINY = [(1, 1), (1, 17), (3, 2), (7, 9), (17, 33)]
TALL = TINY + [(33, 17)]
B_TINY = 2
IN_GUARD, OUT_GUARD = 4096.0, 7.0
_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
LOWP = ("bf16", "fp16")
F32 = ("f32x3", "f32x6", "f32h3")
REPL = 3                                   # replicas of the fused statistics accumulators


# ---- data builders (CPU only) -------------------------------------------------------------------------------------------

def _seed(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return s


def ternary(shape, g, levels=8):
    """{-1, 0, +1} with P(+1) = P(-1) = 1 / levels (1/8 unless a case thins its operands), float64."""
    v = torch.randint(0, levels, shape, generator=g)
    return (v == 0).double() - (v == 1).double()


def _check_output(ref, stats):
    assert float(ref.abs().max()) <= 256, "precondition: max|ref| <= 256"
    assert torch.equal(ref.bfloat16().double(), ref) and torch.equal(ref.half().double(), ref), "precondition: 16-bit exact"
    assert float(ref.abs().max()) > 0
    if stats:
        assert float((ref * ref).sum((0, 2, 3)).max()) < 2 ** 24, "precondition: per-channel sum(ref^2) < 2^24"


@functools.lru_cache(maxsize=None)
def fwd_case(B, H, W, Ci, Co, scaled=True, stats=True, levels=8):
    """conv3x3 forward: x, w, power-of-two fold scale s, bias b, ref = conv2d(x, w * s, b) in float64."""
    g = torch.Generator().manual_seed(_seed(1, B, H, W, Ci, Co))
    x, w = ternary((B, Ci, H, W), g, levels), ternary((Co, Ci, 3, 3), g, levels)
    s = (2.0 ** torch.randint(0, 2, (Co,), generator=g)).double() if scaled else torch.ones(Co, dtype=torch.float64)
    b = torch.randint(-3, 4, (Co,), generator=g).double()
    ref = F.conv2d(x, w * s[:, None, None, None], b, padding=1)
    _check_output(ref, stats)
    return dict(x=x, w=w, s=s, b=b, ref=ref)


def bnb_vectors(C, g):
    """mean | invstd | scale | shift rows on which the BatchNorm-backward terms are exact dyadic numbers."""
    mean = torch.randint(-2, 3, (C,), generator=g).double()
    invstd = 2.0 ** torch.randint(-1, 2, (C,), generator=g).double()
    scale = 2.0 ** torch.randint(-1, 2, (C,), generator=g).double() * (1 - 2 * torch.randint(0, 2, (C,), generator=g).double())
    shift = torch.randint(-2, 2, (C,), generator=g).double() + 0.25
    return torch.stack([mean, invstd, scale, shift])


def bnb_reference(da, y, vec):
    """da, y: [B, C, H, W] float64 -> (sum dz, sum dz * xhat) per channel; asserts the exactness precondition."""
    v = vec[:, None, :, None, None]
    dz = da * ((y * v[2] + v[3]) > 0)
    t2 = dz * (y - v[0]) * v[1]
    assert float(t2.abs().sum((0, 2, 3)).max()) < 2 ** 24 and float(dz.abs().sum((0, 2, 3)).max()) < 2 ** 24, \
        "precondition: per-channel sum|terms| < 2^24"
    return dz.sum((0, 2, 3)), t2.sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def dgrad_case(B, H, W, Ci, Co, bnb=False):
    """conv3x3 input gradient: dy [B, Co], w [Co, Ci, 3, 3], ref = conv2d_input in float64 ([B, Ci]); bnb: the saved
    forward output y [B, Ci] and the BatchNorm vectors of the layer whose `da` this gradient is."""
    g = torch.Generator().manual_seed(_seed(2, B, H, W, Ci, Co))
    dy, w = ternary((B, Co, H, W), g), ternary((Co, Ci, 3, 3), g)
    ref = torch.nn.grad.conv2d_input((B, Ci, H, W), w, dy, padding=1)
    _check_output(ref, False)
    c = dict(dy=dy, w=w, ref=ref)
    if bnb:
        c["y"] = torch.randint(-3, 4, (B, Ci, H, W), generator=g).double()
        c["vec"] = bnb_vectors(Ci, g)
        c["sums"] = bnb_reference(ref, c["y"], c["vec"])
    return c


@functools.lru_cache(maxsize=None)
def up_case(B, H, W, Ci, Co, bnb=False):
    """ConvTranspose2d k2 s2 on the coarse grid H x W: forward reference and input-gradient reference."""
    g = torch.Generator().manual_seed(_seed(3, B, H, W, Ci, Co))
    x, w = ternary((B, Ci, H, W), g), ternary((Ci, Co, 2, 2), g)
    b = torch.randint(-3, 4, (Co,), generator=g).double()
    dy = ternary((B, Co, 2 * H, 2 * W), g)
    ref = F.conv_transpose2d(x, w, b, stride=2)
    dx = F.conv2d(dy, w, None, stride=2)             # the adjoint of the forward: [B, Ci, H, W]
    _check_output(ref, False)
    _check_output(dx, False)
    c = dict(x=x, w=w, b=b, dy=dy, ref=ref, dx=dx)
    if bnb:
        c["y"] = torch.randint(-3, 4, (B, Ci, H, W), generator=g).double()
        c["vec"] = bnb_vectors(Ci, g)
        c["sums"] = bnb_reference(dx, c["y"], c["vec"])
    return c


@functools.lru_cache(maxsize=None)
def wgrad_case(mode, B, H, W, Ci, Co):
    """mode 0: conv3x3 weight gradient [Co, Ci, 3, 3]; mode 1: transposed-conv weight gradient [Ci, Co, 2, 2] (H x W coarse)."""
    g = torch.Generator().manual_seed(_seed(4, mode, B, H, W, Ci, Co))
    x = ternary((B, Ci, H, W), g)
    if mode == 0:
        dy = ternary((B, Co, H, W), g)
        ref = torch.nn.grad.conv2d_weight(x, (Co, Ci, 3, 3), dy, padding=1)
    else:
        dy = ternary((B, Co, 2 * H, 2 * W), g)
        wz = torch.zeros(Ci, Co, 2, 2, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(x, wz, None, stride=2).backward(dy)
        ref = wz.grad
    assert float(ref.abs().max()) < 2 ** 24, "precondition: |ref| < 2^24"
    assert float(ref.abs().max()) > 0 or B * H * W < 4
    return dict(x=x, dy=dy, ref=ref)


# ---- case tables (shared with tests/test_conv_exact_data_cpu.py) ---------------------------------------------------------

def _imgs(images, B=B_TINY):
    return [(B, h, w) for h, w in images]


# name -> (Cin as the caller sees it, Cin as the kernel sees it, N, epilogue flags, pack flags, precisions, images (B, H, W))
FWD_FORMS = {
    "c16": (4, 16, 64, 0, 0, LOWP + F32 + ("h3p_cin4", "h3p_cin4_planes"), _imgs(TINY) + [(3, 21, 37)]),
    "wch128": (64, 64, 128, 0, 0, LOWP + ("h3p", "h3p_planes"), _imgs(TINY)),
    "wch128_frag": (64, 64, 128, hip.EPI_WFRAG, hip.PLANES_FWD_FRAG, LOWP + ("h3p",), _imgs(TINY)),
    "tall": (128, 128, 64, 0, 0, LOWP + ("h3p",), _imgs(TALL)),
    "tall_hp64": (64, 64, 64, 0, 0, ("h3p", "h3p_planes"), _imgs(TALL)),
    "rows64": (64, 64, 64, hip.EPI_WFRAG | hip.EPI_WROWS, hip.PLANES_FWD_FRAG, LOWP, _imgs(TALL)),
    "rows128": (128, 128, 128, hip.EPI_WFRAG | hip.EPI_WROWS, hip.PLANES_FWD_FRAG, LOWP, _imgs(TALL)),
    "w4": (64, 64, 64, 0, 0, LOWP, _imgs(TINY)),
    "w4_192": (64, 64, 192, 0, 0, LOWP, [(1, 9, 18)]),
    "staged64_128": (64, 64, 128, 0, 0, F32, _imgs(TINY)),
    "staged96_64": (96, 96, 64, 0, 0, F32 + LOWP, _imgs(TINY[1:])),
    "staged48_128": (48, 48, 128, 0, 0, F32 + LOWP, _imgs(TINY[:4])),
}
FWD_PARAMS = [(f, p, img) for f, v in FWD_FORMS.items() for p in v[5] for img in v[6]]
DEEP = (1, 5, 7, 1024, 256)
P64_SHAPES = [(2, 256, 256), (1, 304, 432)]
IGEMM_CASES = [(ci, co, p, img) for ci, co in ((64, 128), (96, 64), (48, 128)) for p in LOWP + F32
               for img in _imgs([(3, 2), (17, 33)])]
POOL_IMAGES = _imgs([(2, 2), (2, 18), (18, 34)])
POOL_FORMS = {"wch128": (64, 128, 0, 0, LOWP + ("h3p", "h3p_planes")), "tall": (128, 64, 0, 0, LOWP + ("h3p",)),
              "wch128_frag": (64, 128, hip.EPI_WFRAG, hip.PLANES_FWD_FRAG, LOWP + ("h3p",)), "w4": (64, 64, 0, 0, LOWP),
              "rows64": (64, 64, hip.EPI_WFRAG | hip.EPI_WROWS, hip.PLANES_FWD_FRAG, LOWP),
              "rows128": (128, 128, hip.EPI_WFRAG | hip.EPI_WROWS, hip.PLANES_FWD_FRAG, LOWP),
              "staged": (96, 64, 0, 0, ("f32x3", "bf16"))}
POOL_PARAMS = [(f, p, img) for f, v in POOL_FORMS.items() for p in v[4] for img in POOL_IMAGES]
# (Cin, N, n_first, n_count): 128-channel ranges -> 128-channel form; 64-channel ranges on few tiles -> tall form
COLS_CASES = [(64, 256, 128, 128), (128, 256, 128, 128), (64, 128, 64, 64), (128, 192, 64, 64), (128, 192, 128, 64)]
COLS_PARAMS = [c + (p, img) for c in COLS_CASES for p in LOWP for img in _imgs([(3, 2), (17, 33)])]
DGRAD_CASES = [(128, 64), (64, 128)]              # (Ci, Co) of the forward layer
DGRAD_PARAMS = [c + (p, img) for c in DGRAD_CASES for p in LOWP + ("f32x3", "h3p", "h3f") for img in _imgs(TINY)] + \
               [c + ("f32x6", img) for c in DGRAD_CASES for img in _imgs([(3, 2), (17, 33)])]
DGRAD_BNB_PARAMS = [c + (p, img) for c in DGRAD_CASES + [(64, 64)] for p in LOWP + ("f32x3", "h3p", "h3f")
                    for img in _imgs([(7, 9), (17, 33)])]
# input gradient through a FRAGMENT-MAJOR dgrad plane (crimac_pack_layers, CRIMAC_LAYER_DG_FRAG): (Ci, Co, epilogue flags);
# 128 -> 64: N = 128, the 128-channel form (and the rows form); 64 -> 128: N = 64, the rows form
DGRAD_FRAG_CASES = [(128, 64, hip.EPI_WFRAG), (128, 64, hip.EPI_WFRAG | hip.EPI_WROWS), (64, 128, hip.EPI_WFRAG | hip.EPI_WROWS)]
DGRAD_FRAG_PARAMS = [c + (p, img) for c in DGRAD_FRAG_CASES for p in LOWP + ("h3f",) for img in _imgs([(1, 17), (3, 2), (33, 17)])]
UP_SIZES = _imgs([(1, 1), (1, 9), (3, 2), (5, 20), (7, 33)])
UP_CHANNELS = [(128, 64), (256, 128), (64, 48)]
UP_PARAMS = [c + (p, img) for c in UP_CHANNELS for p in LOWP + ("f32x3", "f32x6") for img in UP_SIZES]
UP_HP_PARAMS = [c + img for c in UP_CHANNELS[:2] for img in UP_SIZES]
UP_BNB_PARAMS = [c + (p, img) for c in UP_CHANNELS[:2] for p in LOWP + ("h3f",) for img in _imgs([(1, 9), (5, 20), (7, 33)])]
WGRAD_CH = [(64, 64), (128, 64), (64, 128), (4, 64)]           # (Ci, Co); Ci = 4: the first layer (CS = 16)
WGRAD_PARAMS = [(0,) + c + (p, img) for c in WGRAD_CH for p in LOWP + ("f32x3", "h3p") for img in _imgs(TINY + [(9, 17)])] + \
               [(0,) + c + ("h3f", img) for c in WGRAD_CH[:3] for img in _imgs(TINY + [(9, 17)])] + \
               [(0,) + c + ("f32x6", img) for c in WGRAD_CH for img in _imgs([(3, 2), (17, 33)])]
WGRAD_UP_PARAMS = [(1,) + c + (p, img) for c in UP_CHANNELS[:2] for p in LOWP + ("f32x3", "h3p", "h3f") for img in UP_SIZES] + \
                  [(1,) + c + ("f32x6", img) for c in UP_CHANNELS[:2] for img in _imgs([(3, 2), (7, 33)])]
PARTIAL_PARAMS = [(0, 128, 64, (2, 17, 33)), (1, 128, 64, (2, 7, 33))]
# crimac_wgrad_group: (Ci, Co, H, W) per layer -- every layer its own resolution, as the engine groups them
GROUP_LISTS = [[(64, 64, 17, 33), (128, 64, 7, 9), (64, 128, 3, 2)], [(64, 64, 3, 2), (128, 64, 17, 33), (64, 128, 7, 9)]]


def case_builders():
    """Every (builder, arguments) pair the GPU tests below use, except the persistent-kernel shapes."""
    out = []
    for f, _, (B, H, W) in FWD_PARAMS:
        out.append((fwd_case, (B, H, W, FWD_FORMS[f][0], FWD_FORMS[f][2])))
    out.append((fwd_case, DEEP + (False, False)))
    out += [(fwd_case, img + (ci, co)) for ci, co, _, img in IGEMM_CASES]
    out += [(fwd_case, img + POOL_FORMS[f][:2] + (True, False)) for f, _, img in POOL_PARAMS]
    out += [(fwd_case, img + (ci, n)) for ci, n, _, _, _, img in COLS_PARAMS]
    out += [(dgrad_case, img + (ci, co)) for ci, co, _, img in DGRAD_PARAMS]
    out += [(dgrad_case, img + (ci, co, True)) for ci, co, _, img in DGRAD_BNB_PARAMS]
    out += [(up_case, img + (ci, co)) for ci, co, _, img in UP_PARAMS]
    out += [(up_case, img + (ci, co, True)) for ci, co, _, img in UP_BNB_PARAMS]
    out += [(wgrad_case, (m,) + img + (ci, co)) for m, ci, co, _, img in WGRAD_PARAMS + WGRAD_UP_PARAMS]
    out += [(wgrad_case, (m,) + img + (ci, co)) for m, ci, co, img in PARTIAL_PARAMS]
    out += [(dgrad_case, img + (ci, co)) for ci, co, _, _, img in DGRAD_FRAG_PARAMS]
    out += [(wgrad_case, (0, B_TINY, h, w, ci, co)) for lst in GROUP_LISTS for ci, co, h, w in lst]
    return sorted(set(out), key=lambda t: (t[0].__name__, tuple(map(int, t[1]))))


# ---- device helpers ------------------------------------------------------------------------------------------------------

def _base(prec):
    return prec.split("_")[0]


def _P(prec):
    """'h3f' here is the BACKWARD personality of that mode (CRIMAC_PREC_H3F_BWD): gradient operands fp16, activation operands
    plane pairs read through their hi plane, weight planes packed as for fp16, outputs fp32."""
    return hip.PREC_H3F_BWD if prec == "h3f" else hip.PREC_NAMES[_base(prec)]


def _planes_arg(prec):
    return hip.PLANES_FP16 if prec == "h3f" else hip.PREC_PLANES_ARG[_P(prec)]


def _dt(prec):
    """storage type of a 16-bit or fp32 INPUT operand (h3f: the gradient operand)."""
    return torch.float16 if prec == "h3f" else _DT.get(_base(prec), torch.float32)


def _dt_out(prec):
    return torch.float32 if _base(prec) in ("h3p", "h3f") else _dt(prec)


def hp_pack(m):
    """[M, C] fp32 (cpu) -> [M, C] 'float32' tensor whose bytes are fp16 plane pairs [8 hi | 8 lo] of m."""
    M, C = m.shape
    hi = m.half()
    lo = (m - hi.float()).half()
    return torch.stack([hi.view(M, C // 8, 8), lo.view(M, C // 8, 8)], dim=2).contiguous().view(torch.float32).view(M, C).clone()


def hp_unpack(t):
    M, C = t.shape
    h = t.contiguous().cpu().view(torch.float16).view(M, C // 8, 2, 8).float()
    return (h[:, :, 0] + h[:, :, 1]).reshape(M, C)


def nhwc(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C)


def nchw(m, B, H, W):
    return m.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


class Guarded:
    """An [M, C] activation matrix in columns [off, off + C) of rows [G, G + M) of a [M + 2 G, ld] allocation filled with
    `fill`.  planes: the tensor holds fp16 plane pairs (fp32 addressing)."""

    def __init__(self, M, C, dtype, fill, W, mat=None, planes=False, off=8, extra=24):
        self.M, self.C, self.off, self.ld, self.G, self.planes, self.fill = M, C, off, C + extra, 2 * W + 8, planes, fill
        host = torch.full((M + 2 * self.G, self.ld), fill, dtype=torch.float32)
        if mat is not None:
            host[self.G:self.G + M, off:off + C] = mat.float()
        self.host = hp_pack(host) if planes else host.to(dtype)
        self.buf = self.host.cuda()

    def p(self, col=0):
        return ptr(self.buf, self.G * self.ld + self.off + col)

    def values(self, c0=0, c1=None):
        """float64 [M, c1 - c0] of what the kernel left in the inner block."""
        inner = self.buf[self.G:self.G + self.M, self.off:self.off + self.C]
        v = hp_unpack(inner) if self.planes else inner.float().cpu()
        return v[:, c0:c1].double()

    def assert_guards(self, c0=0, c1=None):
        """Everything outside columns [c0, c1) of the inner block still holds the fill pattern."""
        got = self.buf.cpu().clone().view(torch.uint8).view(self.host.shape[0], -1)
        want = self.host.clone().view(torch.uint8).view(self.host.shape[0], -1)
        es = self.host.element_size()
        c1 = self.C if c1 is None else c1
        lo, hi = (self.off + c0) * es, (self.off + c1) * es
        got[self.G:self.G + self.M, lo:hi] = 0
        want[self.G:self.G + self.M, lo:hi] = 0
        assert torch.equal(got, want), "a guard element (or an input) was written"


def g_in(x, prec, W, cpad=None, act=False):
    """[B, C, H, W] float64 -> guarded device input (channels zero-padded to cpad).  act: the operand is a forward
    ACTIVATION (h3f: plane pairs; its gradient operands are fp16)."""
    m = nhwc(x)
    if cpad and cpad > m.shape[1]:
        m = torch.cat([m, torch.zeros(m.shape[0], cpad - m.shape[1], dtype=m.dtype)], 1)
    planes = _base(prec) == "h3p" or (prec == "h3f" and act)
    return Guarded(m.shape[0], m.shape[1], _dt(prec), IN_GUARD, W, mat=m, planes=planes)


def g_out(M, C, prec, W, planes=False, dtype=None):
    return Guarded(M, C, dtype or _dt_out(prec), OUT_GUARD, W, planes=planes)


def pack_conv(w, prec, cin_pad=None, scale=None, flags=0, dgrad=False):
    Co, Ci = w.shape[:2]
    cin_pad = cin_pad or Ci
    P = _P(prec)
    wd = w.float().cuda().contiguous()
    i16 = dict(dtype=torch.int16, device="cuda")
    fh, fl = torch.zeros(2 * 9 * Co * cin_pad, **i16), torch.zeros(2 * 9 * Co * cin_pad + 8, **i16)
    dh = torch.zeros(2 * 9 * Ci * Co, **i16) if dgrad else None
    dl = torch.zeros(2 * 9 * Ci * Co + 8, **i16) if dgrad else None
    sc = scale.float().cuda() if scale is not None else None
    call("crimac_pack_conv3x3", ptr(wd), Co, Ci, cin_pad, ptr(sc), _planes_arg(prec) | flags, ptr(fh), ptr(fl), ptr(dh), ptr(dl))
    torch.cuda.synchronize()
    return fh, fl, dh, dl


def pack_dgrad_frag(w, prec):
    """The input-gradient plane of a 3x3 layer, FRAGMENT-MAJOR (crimac_pack_layers with CRIMAC_LAYER_DG_FRAG)."""
    Co, Ci = w.shape[:2]
    wd = w.float().cuda().contiguous()
    i16 = dict(dtype=torch.int16, device="cuda")
    bufs = [torch.zeros(2 * 9 * Co * Ci + 8, **i16) for _ in range(4)]
    d = (hip.LayerDesc * 1)()
    d[0].w = wd.data_ptr()
    d[0].fwd_hi, d[0].fwd_lo, d[0].dg_hi, d[0].dg_lo = (t.data_ptr() for t in bufs)
    d[0].kind, d[0].Co, d[0].Ci, d[0].Ci_pad = hip.LAYER_DG_FRAG, Co, Ci, Ci
    call("crimac_pack_layers", ctypes.byref(d), 1, _planes_arg(prec))
    torch.cuda.synchronize()
    return bufs[2], bufs[3]


def pack_up(w, prec):
    Ci, Co = w.shape[:2]
    n = 4 * Ci * Co
    i16 = dict(dtype=torch.int16, device="cuda")
    bufs = [torch.zeros(2 * n + 8, **i16) for _ in range(4)]
    wd = w.float().cuda().contiguous()
    call("crimac_pack_upconv2x2", ptr(wd), Ci, Co, _planes_arg(prec), *[ptr(t) for t in bufs])
    torch.cuda.synchronize()
    return bufs


def stat_bufs(N):
    return torch.zeros(2, REPL, N, dtype=torch.float64, device="cuda")


def bnb_dev(c, prec, W):
    """(guarded y in the output's storage type, device vectors with row stride > C)."""
    C = c["y"].shape[1]
    y = Guarded(c["y"].numel() // C, C, _dt_out(prec), IN_GUARD, W, mat=nhwc(c["y"]))
    vec = torch.zeros(4, C + 8, dtype=torch.float32)
    vec[:, :C] = c["vec"].float()
    return y, vec.cuda()


def conv3x3(prec, xin, B, H, W, Cin, N, wts, bias, out, flags=0, stat=None, bnb=None, cols=None, pool=None):
    P = _P(prec)
    if prec.startswith("h3p_cin4"):
        flags |= hip.EPI_CIN4
    if out.planes or (prec == "h3f" and out.buf.dtype == torch.float16):     # (h3f: an fp16 output is asked for the same way)
        flags |= hip.EPI_OUT_PLANES
    mode, s0, s1, by, by_ld, bv, bs = 0, None, None, None, 0, None, 0
    if stat is not None:
        mode, s0, s1 = 1, ptr(stat[0]), ptr(stat[1])
    if bnb is not None:
        y, vec, st = bnb
        mode, s0, s1, by, by_ld, bv, bs = 2, ptr(st[0]), ptr(st[1]), y.p(), y.ld, ptr(vec), vec.shape[1]
    bd = bias.float().cuda() if bias is not None else None
    head = (P, xin.p(), xin.ld, B, H, W, Cin, N, ptr(wts[0]), ptr(wts[1]), ptr(bd), out.p(), out.ld, flags)
    if pool is not None:
        call("crimac_conv3x3_pool", *head, pool.p(), pool.ld)
    elif cols is not None:
        call("crimac_conv3x3_cols", *head, mode, s0, s1, REPL, by, by_ld, bv, bs, cols[0], cols[1])
    else:
        call("crimac_conv3x3", *head, mode, s0, s1, REPL, by, by_ld, bv, bs)
    torch.cuda.synchronize()


def assert_stats(st, ref, c0=0, c1=None):
    s = st.sum(1).cpu()
    c1 = ref.shape[1] if c1 is None else c1
    assert torch.equal(s[0, c0:c1], ref.sum((0, 2, 3))[c0:c1]) and torch.equal(s[1, c0:c1], (ref * ref).sum((0, 2, 3))[c0:c1])
    keep = torch.ones(s.shape[1], dtype=torch.bool)
    keep[c0:c1] = False
    assert float(s[:, keep].abs().sum()) == 0


def forward_exact(prec, c, B, H, W, Cin_k, N, eflags, pflags, stats=True):
    """crimac_conv3x3 on case c: output, fused statistics, ReLU epilogue, guards -- all exact."""
    planes = prec.endswith("_planes")
    wts = pack_conv(c["w"], prec, Cin_k, c["s"], pflags)
    xin = g_in(c["x"], prec, W, Cin_k)
    for relu in (0, hip.EPI_RELU):
        ref = torch.relu(c["ref"]) if relu else c["ref"]
        out = g_out(B * H * W, N, prec, W, planes)
        st = stat_bufs(N) if stats else None
        conv3x3(prec, xin, B, H, W, Cin_k, N, wts, c["b"], out, eflags | relu, stat=st)
        assert torch.equal(nchw(out.values(), B, H, W), ref)
        out.assert_guards()
        if stats:
            assert_stats(st, ref)
    xin.assert_guards(0, 0)


# ---- conv3x3 forward ----------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("form,prec,img", FWD_PARAMS)
def test_conv3x3_forward_is_exact(form, prec, img):
    Ci, Cin_k, N, eflags, pflags, _, _ = FWD_FORMS[form]
    B, H, W = img
    forward_exact(prec, fwd_case(B, H, W, Ci, N), B, H, W, Cin_k, N, eflags, pflags)


@gpu
@pytest.mark.parametrize("prec,eflags,pflags", [("bf16", 0, 0), ("fp16", 0, 0), ("bf16", hip.EPI_WFRAG, hip.PLANES_FWD_FRAG),
                                                ("fp16", hip.EPI_WFRAG, hip.PLANES_FWD_FRAG), ("h3p", 0, 0),
                                                ("h3p", hip.EPI_WFRAG, hip.PLANES_FWD_FRAG)])
def test_conv3x3_deep_layer_is_exact(prec, eflags, pflags):
    """K = 9 * 1024: the 128-channel form of the channel-split kernel walks 16 channel chunks; one wrong 16-byte unit of one
    tap moves an output by under 1 % of max|ref| -- below the 16-bit tolerances of the norm-wise tests."""
    B, H, W, Ci, N = DEEP
    forward_exact(prec, fwd_case(*DEEP, False, False), B, H, W, Ci, N, eflags, pflags, stats=False)


@gpu
@pytest.mark.parametrize("prec", LOWP)
@pytest.mark.parametrize("img", P64_SHAPES)
def test_conv3x3_persistent_64_to_64_is_exact(prec, img):
    """>= 512 full tiles: the persistent kernel; 513 tiles = an odd count on more than twice the CUs' worth of tiles.  Forward
    with statistics kept in fp32 across a workgroup's tiles, the fused pool, and the input gradient with stat_mode 2."""
    B, H, W = img
    c = fwd_case(B, H, W, 64, 64, False, True)
    wts = pack_conv(c["w"], prec, 64, None, 0)
    xin = g_in(c["x"], prec, W)
    out, st = g_out(B * H * W, 64, prec, W), stat_bufs(64)
    conv3x3(prec, xin, B, H, W, 64, 64, wts, c["b"], out, 0, stat=st)
    assert torch.equal(nchw(out.values(), B, H, W), c["ref"])
    out.assert_guards()
    assert_stats(st, c["ref"])
    out, pool = g_out(B * H * W, 64, prec, W), g_out(B * H * W // 4, 64, prec, W // 2)
    conv3x3(prec, xin, B, H, W, 64, 64, wts, c["b"], out, hip.EPI_RELU, pool=pool)
    rr = torch.relu(c["ref"])
    assert torch.equal(nchw(out.values(), B, H, W), rr)
    assert torch.equal(nchw(pool.values(), B, H // 2, W // 2), F.max_pool2d(rr, 2, 2))
    out.assert_guards()
    pool.assert_guards()
    # BatchNorm-backward sums: the reference output doubles as the saved forward output y (integers, |y| <= 256 is too wide
    # for the sum bound: clamp to [-3, 3])
    g = torch.Generator().manual_seed(5)
    d = dict(y=c["ref"].clamp(-3, 3), vec=bnb_vectors(64, g))
    d["vec"][1] = 1.0
    sums = bnb_reference(c["ref"] - c["b"][None, :, None, None], d["y"], d["vec"])
    y, vec = bnb_dev(d, prec, W)
    out, st = g_out(B * H * W, 64, prec, W), stat_bufs(64)
    conv3x3(prec, xin, B, H, W, 64, 64, wts, None, out, 0, bnb=(y, vec, st))
    assert torch.equal(nchw(out.values(), B, H, W), c["ref"] - c["b"][None, :, None, None])
    s = st.sum(1).cpu()
    assert torch.equal(s[0], sums[0]) and torch.equal(s[1], sums[1])
    out.assert_guards()
    # crimac_conv3x3_cols: the 64-channel range [64, 128) of a 64 -> 128 convolution on >= 512 full tiles also takes the
    # persistent kernel (glds_dispatch: n_count == 64, Cin == 64).  Channels 64.. carry this case's weights and bias, so the
    # cached reference is theirs; channels 0..63 (other weights) must stay untouched.
    g = torch.Generator().manual_seed(6)
    w128 = torch.cat([ternary((64, 64, 3, 3), g), c["w"]])
    wts128 = pack_conv(w128, prec, 64, None, 0)
    out, st = g_out(B * H * W, 128, prec, W), stat_bufs(128)
    conv3x3(prec, xin, B, H, W, 64, 128, wts128, torch.cat([torch.zeros(64, dtype=torch.float64), c["b"]]), out, 0, stat=st,
            cols=(64, 64))
    assert torch.equal(nchw(out.values(64, 128), B, H, W), c["ref"])
    out.assert_guards(64, 128)
    assert_stats(st, torch.cat([c["ref"], c["ref"]], 1), 64, 128)
    xin.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("ci,co,prec,img", IGEMM_CASES)
def test_igemm_conv3x3_is_exact(ci, co, prec, img):
    B, H, W = img
    c = fwd_case(B, H, W, ci, co)
    wts = pack_conv(c["w"], prec, ci, c["s"])
    xin = g_in(c["x"], prec, W)
    bd = c["b"].float().cuda()
    for relu in (0, 1):
        out = g_out(B * H * W, co, prec, W)
        call("crimac_igemm_conv", _P(prec), xin.p(), xin.ld, B, H, W, H, W, ci, co, 9, 3, 1, 1, ptr(wts[0]), ptr(wts[1]),
             ptr(bd), co, out.p(), out.ld, relu, 0, 0)
        torch.cuda.synchronize()
        assert torch.equal(nchw(out.values(), B, H, W), torch.relu(c["ref"]) if relu else c["ref"])
        out.assert_guards()
    xin.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("form,prec,img", POOL_PARAMS)
def test_conv3x3_pool_is_exact(form, prec, img):
    ci, co, eflags, pflags, _ = POOL_FORMS[form]
    B, H, W = img
    c = fwd_case(B, H, W, ci, co, True, False)
    planes = prec.endswith("_planes")
    wts = pack_conv(c["w"], prec, ci, c["s"], pflags)
    xin = g_in(c["x"], prec, W)
    out, pool = g_out(B * H * W, co, prec, W, planes), g_out(B * H * W // 4, co, prec, W // 2, planes)
    conv3x3(prec, xin, B, H, W, ci, co, wts, c["b"], out, eflags | hip.EPI_RELU, pool=pool)
    rr = torch.relu(c["ref"])
    assert torch.equal(nchw(out.values(), B, H, W), rr)
    assert torch.equal(nchw(pool.values(), B, H // 2, W // 2), F.max_pool2d(rr, 2, 2))
    out.assert_guards()
    pool.assert_guards()
    xin.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("ci,n,n_first,n_count,prec,img", COLS_PARAMS)
def test_conv3x3_cols_is_exact(ci, n, n_first, n_count, prec, img):
    B, H, W = img
    c = fwd_case(B, H, W, ci, n)
    wts = pack_conv(c["w"], prec, ci, c["s"])
    xin = g_in(c["x"], prec, W)
    out, st = g_out(B * H * W, n, prec, W), stat_bufs(n)
    conv3x3(prec, xin, B, H, W, ci, n, wts, c["b"], out, 0, stat=st, cols=(n_first, n_count))
    assert torch.equal(nchw(out.values(n_first, n_first + n_count), B, H, W), c["ref"][:, n_first:n_first + n_count])
    out.assert_guards(n_first, n_first + n_count)                  # the other columns of the output are untouched too
    assert_stats(st, c["ref"], n_first, n_first + n_count)
    xin.assert_guards(0, 0)


# ---- conv3x3 input gradient ---------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("ci,co,prec,img", DGRAD_PARAMS)
def test_conv3x3_dgrad_is_exact(ci, co, prec, img):
    B, H, W = img
    c = dgrad_case(B, H, W, ci, co)
    _, _, dh, dl = pack_conv(c["w"], prec, dgrad=True)
    dyn = g_in(c["dy"], prec, W)
    out = g_out(B * H * W, ci, prec, W)
    conv3x3(prec, dyn, B, H, W, co, ci, (dh, dl), None, out)
    assert torch.equal(nchw(out.values(), B, H, W), c["ref"])
    out.assert_guards()
    if prec == "h3f":          # ... and as an fp16 output (the up half of a decoder block's d(concat)): the fp16 mode's launch
        out = g_out(B * H * W, ci, prec, W, dtype=torch.float16)
        conv3x3(prec, dyn, B, H, W, co, ci, (dh, dl), None, out)
        assert torch.equal(nchw(out.values(), B, H, W), c["ref"])
        out.assert_guards()
    dyn.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("ci,co,eflags,prec,img", DGRAD_FRAG_PARAMS)
def test_conv3x3_dgrad_fragment_major_is_exact(ci, co, eflags, prec, img):
    """The input gradient through a fragment-major dgrad plane: the 128-channel form and the rows form of the channel-split
    kernel, 16-bit and H3F_BWD (fp16 in, fp32 out: crimac_conv3x3_glds_16_f32out)."""
    B, H, W = img
    c = dgrad_case(B, H, W, ci, co)
    dh, dl = pack_dgrad_frag(c["w"], prec)
    dyn = g_in(c["dy"], prec, W)
    out = g_out(B * H * W, ci, prec, W)
    conv3x3(prec, dyn, B, H, W, co, ci, (dh, dl), None, out, eflags)
    assert torch.equal(nchw(out.values(), B, H, W), c["ref"])
    out.assert_guards()
    dyn.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("ci,co,prec,img", DGRAD_BNB_PARAMS)
def test_conv3x3_dgrad_bn_backward_sums_are_exact(ci, co, prec, img):
    B, H, W = img
    c = dgrad_case(B, H, W, ci, co, True)
    _, _, dh, dl = pack_conv(c["w"], prec, dgrad=True)
    dyn = g_in(c["dy"], prec, W)
    y, vec = bnb_dev(c, prec, W)
    out, st = g_out(B * H * W, ci, prec, W), stat_bufs(ci)
    conv3x3(prec, dyn, B, H, W, co, ci, (dh, dl), None, out, bnb=(y, vec, st))
    assert torch.equal(nchw(out.values(), B, H, W), c["ref"])
    s = st.sum(1).cpu()
    assert torch.equal(s[0], c["sums"][0]) and torch.equal(s[1], c["sums"][1])
    out.assert_guards()
    y.assert_guards(0, 0)


# ---- transposed convolution ---------------------------------------------------------------------------------------------

def up_forward(prec, c, B, H, W, ci, co, planes=False):
    fh, fl, dh, dl = pack_up(c["w"], prec)
    xin = g_in(c["x"], prec, W)
    cat = g_out(B * 4 * H * W, co, prec, 2 * W, planes)
    bd = c["b"].float().cuda()
    call("crimac_igemm_conv", _P(prec), xin.p(), xin.ld, B, H, W, H, W, ci, 4 * co, 1, 1, 0, 1, ptr(fh), ptr(fl), ptr(bd), co,
         cat.p(), cat.ld, hip.EPI_OUT_PLANES if planes else 0, 1, co)
    torch.cuda.synchronize()
    assert torch.equal(nchw(cat.values(), B, 2 * H, 2 * W), c["ref"])
    cat.assert_guards()
    xin.assert_guards(0, 0)
    return dh, dl


@gpu
@pytest.mark.parametrize("ci,co,prec,img", UP_PARAMS)
def test_upconv2x2_forward_and_dgrad_are_exact(ci, co, prec, img):
    B, H, W = img
    c = up_case(B, H, W, ci, co)
    dh, dl = up_forward(prec, c, B, H, W, ci, co)
    dyn = g_in(c["dy"], prec, 2 * W)
    dx = g_out(B * H * W, ci, prec, W)
    call("crimac_igemm_conv", _P(prec), dyn.p(), dyn.ld, B, 2 * H, 2 * W, H, W, co, ci, 4, 2, 0, 2, ptr(dh), ptr(dl), None, 0,
         dx.p(), dx.ld, 0, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(nchw(dx.values(), B, H, W), c["dx"])
    dx.assert_guards()
    dyn.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("ci,co,B,H,W", UP_HP_PARAMS)
def test_upconv2x2_plane_pairs_are_exact(ci, co, B, H, W):
    """Plane-pair forward with plane-pair output (the concat half), input gradient to fp32."""
    c = up_case(B, H, W, ci, co)
    dh, dl = up_forward("h3p", c, B, H, W, ci, co, planes=True)
    dyn = g_in(c["dy"], "h3p", 2 * W)
    dx = g_out(B * H * W, ci, "h3p", W)
    call("crimac_igemm_conv", hip.PREC_H3P, dyn.p(), dyn.ld, B, 2 * H, 2 * W, H, W, co, ci, 4, 2, 0, 2, ptr(dh), ptr(dl), None, 0,
         dx.p(), dx.ld, 0, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(nchw(dx.values(), B, H, W), c["dx"])
    dx.assert_guards()


@gpu
@pytest.mark.parametrize("ci,co,prec,img", UP_BNB_PARAMS)
def test_upconv2x2_dgrad_bnb_is_exact(ci, co, prec, img):
    B, H, W = img
    c = up_case(B, H, W, ci, co, True)
    _, _, dh, _ = pack_up(c["w"], prec)
    dyn = g_in(c["dy"], prec, 2 * W)
    y, vec = bnb_dev(c, prec, W)
    entries = ["crimac_upconv2x2_dgrad_bnb_prec"] + (["crimac_upconv2x2_dgrad_bnb"] if prec == "bf16" else [])
    for name in entries:
        dx, st = g_out(B * H * W, ci, prec, W), stat_bufs(ci)
        head = (_P(prec),) if name.endswith("_prec") else ()
        call(name, *head, dyn.p(), dyn.ld, B, H, W, co, ci, ptr(dh), dx.p(), dx.ld, y.p(), y.ld, ptr(vec), vec.shape[1],
             ptr(st[0]), ptr(st[1]), REPL)
        torch.cuda.synchronize()
        assert torch.equal(nchw(dx.values(), B, H, W), c["dx"])
        s = st.sum(1).cpu()
        assert torch.equal(s[0], c["sums"][0]) and torch.equal(s[1], c["sums"][1])
        dx.assert_guards()
    dyn.assert_guards(0, 0)


# ---- weight gradients ---------------------------------------------------------------------------------------------------

def wgrad_operands(mode, c, prec, W, cpad):
    """(F, CF, S, CS, taps): mode 0 F = dY, S = X; mode 1 F = X, S = dY (fine grid)."""
    if mode == 0:
        f, s = g_in(c["dy"], prec, W), g_in(c["x"], prec, W, cpad, act=True)
        return f, f.C, s, s.C, 9
    f, s = g_in(c["x"], prec, W, act=True), g_in(c["dy"], prec, 2 * W)
    return f, f.C, s, s.C, 4


def unpack(mode, dwp, ci, co, cpad):
    grad = torch.full((co, ci, 3, 3) if mode == 0 else (ci, co, 2, 2), OUT_GUARD, dtype=torch.float32, device="cuda")
    if mode == 0:
        call("crimac_unpack_wgrad_conv3x3", ptr(dwp), co, ci, cpad, ptr(grad))
    else:
        call("crimac_unpack_wgrad_upconv2x2", ptr(dwp), ci, co, ptr(grad))
    torch.cuda.synchronize()
    return grad.cpu().double()


@gpu
@pytest.mark.parametrize("mode,ci,co,prec,img", WGRAD_PARAMS + WGRAD_UP_PARAMS)
def test_wgrad_is_exact(mode, ci, co, prec, img):
    B, H, W = img
    c = wgrad_case(mode, B, H, W, ci, co)
    cpad = 16 if ci < 16 else ci
    f, CF, s, CS, taps = wgrad_operands(mode, c, prec, W, cpad)
    for target in (0, 1, 3):
        dwp = torch.zeros(taps * CF * CS + 64, dtype=torch.float32, device="cuda")
        dwp[taps * CF * CS:] = OUT_GUARD
        call("crimac_wgrad", _P(prec), mode, f.p(), f.ld, CF, s.p(), s.ld, CS, B, H, W, ptr(dwp), target)
        assert torch.equal(unpack(mode, dwp, ci, co, cpad), c["ref"]), target
        assert float((dwp[taps * CF * CS:] - OUT_GUARD).abs().max()) == 0
    f.assert_guards(0, 0)
    s.assert_guards(0, 0)


@gpu
@pytest.mark.parametrize("prec", LOWP + ("f32x3", "f32x6"))
@pytest.mark.parametrize("mode,ci,co,img", PARTIAL_PARAMS)
def test_wgrad_partial_slabs_sum_exactly(mode, ci, co, img, prec):
    B, H, W = img
    c = wgrad_case(mode, B, H, W, ci, co)
    f, CF, s, CS, taps = wgrad_operands(mode, c, prec, W, ci)
    lib = hip.load_library()
    n = taps * CF * CS
    for target in (0, 3):
        sp = lib.crimac_wgrad_splits(_P(prec), mode, CF, CS, B, H, W, target)
        assert sp >= 1
        stride = n + 64
        slabs = torch.full((sp, stride), float("nan"), dtype=torch.float32, device="cuda")
        slabs[:, n:] = OUT_GUARD
        call("crimac_wgrad_partials", _P(prec), mode, f.p(), f.ld, CF, s.p(), s.ld, CS, B, H, W, ptr(slabs), stride, target)
        torch.cuda.synchronize()
        assert float((slabs[:, n:] - OUT_GUARD).abs().max()) == 0
        summed = slabs[:, :n].double().sum(0).float().contiguous()
        assert torch.equal(unpack(mode, summed, ci, co, ci), c["ref"])


@gpu
@pytest.mark.parametrize("prec", LOWP + ("h3p", "h3f"))
@pytest.mark.parametrize("GROUP_LAYERS", GROUP_LISTS, ids=["big_first", "small_first"])
def test_wgrad_group_is_exact(GROUP_LAYERS, prec):
    """crimac_wgrad_group takes conv3x3 layers with Cin >= 64 (the struct has no mode field, group_check in wgrad.hip wants
    CS >= 64): three of them in one launch, each at its own resolution (per-layer tile bookkeeping of the plan)."""
    B = B_TINY
    lib = hip.load_library()
    P = _P(prec)
    arr, keep = (hip.WgradGroupLayer * len(GROUP_LAYERS))(), []
    for d, (ci, co, H, W) in zip(arr, GROUP_LAYERS):
        c = wgrad_case(0, B, H, W, ci, co)
        f, s = g_in(c["dy"], prec, W), g_in(c["x"], prec, W, act=True)
        dwp = torch.zeros(9 * co * ci, dtype=torch.float32, device="cuda")
        keep.append((f, s, dwp, c, ci, co))
        d.f, d.f_ld, d.CF = f.p().value, f.ld, co
        d.s, d.s_ld, d.CS = s.p().value, s.ld, ci
        d.Hf, d.Wf, d.dw = H, W, dwp.data_ptr()
    counts = (ctypes.c_int * 8)()
    cap = lib.crimac_wgrad_group_plan(P, arr, len(GROUP_LAYERS), B, 0, None, 0, counts)
    assert cap > 0, lib.crimac_last_error()
    host = torch.zeros(8 * cap * 2, dtype=torch.int32)
    assert lib.crimac_wgrad_group_plan(P, arr, len(GROUP_LAYERS), B, 0, ctypes.c_void_p(host.data_ptr()), cap, counts) == cap
    items, ctr = host.cuda(), torch.zeros(8, dtype=torch.int32, device="cuda")
    call("crimac_wgrad_group", P, ctypes.byref(arr), len(GROUP_LAYERS), B, ptr(items), cap, ctypes.byref(counts), ptr(ctr))
    torch.cuda.synchronize()
    for f, s, dwp, c, ci, co in keep:
        assert torch.equal(unpack(0, dwp, ci, co, ci), c["ref"]), (ci, co)
        f.assert_guards(0, 0)
        s.assert_guards(0, 0)
