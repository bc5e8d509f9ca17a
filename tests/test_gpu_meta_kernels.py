"""The three late-metadata-injection kernels of csrc/meta.hip, one at a time, through the C ABI:
crimac_meta_mlp_fwd, crimac_meta_inject_fwd, crimac_meta_bwd.

Reference: a float64 restatement written in this file (`mlp_reference`), whose hand-written backward pass (explicit
gates h > 0) is checked against torch.autograd on the CPU.  Next to every value it returns the sum of the absolute
values of the terms that enter it, with the absolute values propagated through the layers (|b| + sum |w| * S of the layer
below), so that the figure bounds every partial sum the kernel can form in whatever order.

Two kinds of GPU test:

* EXACT (integer-valued fp32 data).  Every product and partial sum is an integer below 2^24, hence exact in fp32 and
  independent of summation order, FMA contraction and atomics: the kernel must `torch.equal` the reference.  A dropped,
  duplicated or mis-indexed pixel, a stale LDS row or a wrong tail mask is an inequality.  The condition (integers, sum of
  |terms| + |prefill| < 2^24, no degenerate all-zero output) is asserted on the CPU, for every case, by an unmarked test.
  Every input lies between two NaN guards (a read outside the tensor poisons the result), every output is followed by a
  sentinel guard (a write outside it is seen).
* ACCURACY (synthetic weights and metadata planes, Gaussian dlogits / npix).  |got - ref| <= L * 2^-24 * sum|terms| with L
  the longest fp32 accumulation chain the kernel's structure allows (`chain_length`); the forward bound is 64 * 2^-24 *
  sum|terms| as the three dot products (8, 32, 32 terms) propagate it.  Pixels with a float64 pre-activation within 1e-4
  of zero are re-drawn on the CPU beforehand, so no gate can differ between fp32 and float64; none is left out.

Measured on an MI355X, max over the elements of |got - ref| / (2^-24 * sum|terms|), per output (bound: 64 for m, L for
the gradients).  The gradient sums end in atomics, so their last bits depend on the order the workgroups arrive in: each
gradient figure is the larger of two runs (m is the same in both).

    (Cm, ncls), (B, H, W)      L      m    dwm    gw1    gb1    gw2    gb2    gw3    gb3
    (7, 3), (3, 19, 23)      294  0.407  0.004  0.162  0.145  0.676  0.730  0.056  0.032
    (3, 2), (3, 19, 23)      294  0.071  0.004  0.153  0.141  0.612  0.249  0.070  0.043
    (7, 3), (3, 211, 209)   1056  0.765  0.001  0.175  0.134  0.846  0.279  0.006  0.021
    (3, 2), (3, 211, 209)   1056  0.071  0.001  0.037  0.048  0.096  0.058  0.004  0.018

(softmax: max |p - p_ref| 1.3e-7 against 1e-6; max |sum p - 1| 1.4e-7 against 4 * 2^-24 * ncls = 7.2e-7 at ncls = 3.)
"""
import functools
import math
import re

import numpy as np
import pytest
import torch

import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import hip, synth
from crimac_classifiers_unet_amd.hip import call, ptr
from oracle import unet_oracle as orc

HID = 32                    # hidden width of MetaPostProcessing
U = 2.0 ** -24              # unit roundoff of fp32
LIMIT = 2.0 ** 24           # integers below it are exact in fp32
GUARD = 256                 # floats of guard around inputs / behind outputs
SENTINEL = -12345.0
CHUNK = 1 << 16             # pixels per slice of the float64 reference (bounds its memory at the large shapes)
OUTPUTS = ("dwm", "gw1", "gb1", "gw2", "gb2", "gw3", "gb3")       # argument order of crimac_meta_bwd
WKEYS = ("w1", "b1", "w2", "b2", "w3", "b3")
SEED0 = 3                   # chosen on the CPU: the first offset at which no exact case is degenerate

SMALL_SHAPES = [(1, 3, 5), (3, 5, 7), (2, 16, 16), (3, 19, 23)]
LARGE_BWD = (3, 211, 209)   # 517 blocks over the backward grid of 512: five workgroups iterate twice, ragged end
LARGE_FWD = (3, 419, 418)   # 2053 blocks over the forward grid of 2048; the backward kernel iterates five times
EXACT_CASES = [(s, cm, nc) for s in SMALL_SHAPES for cm in (1, 3, 7, 8) for nc in (2, 3, 4)] + \
              [(s, cm, nc) for s in (LARGE_BWD, LARGE_FWD) for cm, nc in ((1, 2), (7, 3), (8, 4))]
REAL_CASES = [(s, cm, nc) for s in ((3, 19, 23), LARGE_BWD) for cm, nc in ((7, 3), (3, 2))]


def _id(case):
    (B, H, W), cm, nc = case
    return f"{B}x{H}x{W}-Cm{cm}-ncls{nc}"


# ---- the float64 reference -------------------------------------------------------------------------------------------
def mlp_reference(meta, p, wm=None, dl=None, drop_unit=None):
    """m = W3 . relu(W2 . relu(W1 . x + b1) + b2) + b3 per pixel of meta [B][Cm][H][W], in float64, and (with `dl`
    [B][ncls][H][W] and `wm` [ncls]) the backward pass of logits[:, o] += wm[o] * m written out by hand.

    Returns a dict: m [npix], m_abs [npix] (sum |terms| of the three dot products, propagated), gate [npix] (smallest
    |pre-activation| of the pixel's 64 hidden units), grads / grads_abs {name: tensor} in the shapes of the kernel's
    outputs.  `drop_unit` forces that unit of the first hidden layer to zero (precondition checks only)."""
    B, Cm, H, W = meta.shape
    npix = B * H * W
    x_all = meta.double().permute(0, 2, 3, 1).reshape(npix, Cm)          # pixel p = b*HW + hw, as the kernels count
    w1, b1, w2, b2 = (p[k].double() for k in WKEYS[:4])
    w3, b3 = p["w3"].double().reshape(HID), p["b3"].double().reshape(())
    out = {"m": torch.empty(npix, dtype=torch.float64), "m_abs": torch.empty(npix, dtype=torch.float64),
           "gate": torch.empty(npix, dtype=torch.float64)}
    if dl is not None:
        ncls = dl.shape[1]
        d_all = dl.double().permute(0, 2, 3, 1).reshape(npix, ncls)
        wmd = wm.double().reshape(ncls)
        shapes = {"dwm": (ncls,), "gw1": (HID, Cm), "gb1": (HID,), "gw2": (HID, HID), "gb2": (HID,), "gw3": (HID,),
                  "gb3": (1,)}
        g = {k: torch.zeros(s, dtype=torch.float64) for k, s in shapes.items()}
        ga = {k: torch.zeros(s, dtype=torch.float64) for k, s in shapes.items()}
    for s in range(0, npix, CHUNK):
        e = min(s + CHUNK, npix)
        x = x_all[s:e]
        a1 = x @ w1.T + b1
        s1 = x.abs() @ w1.abs().T + b1.abs()
        if drop_unit is not None:
            a1[:, drop_unit] = 0.0
        h1 = torch.where(a1 > 0, a1, torch.zeros_like(a1))
        a2 = h1 @ w2.T + b2
        s2 = s1 @ w2.abs().T + b2.abs()
        h2 = torch.where(a2 > 0, a2, torch.zeros_like(a2))
        m = h2 @ w3 + b3
        out["m"][s:e] = m
        out["m_abs"][s:e] = s2 @ w3.abs() + b3.abs()
        out["gate"][s:e] = torch.minimum(a1.abs().min(dim=1).values, a2.abs().min(dim=1).values)
        if dl is None:
            continue
        d = d_all[s:e]
        gate1, gate2 = (h1 > 0).double(), (h2 > 0).double()
        dm = d @ wmd                                           # dm[p] = sum_o dl[o][p] * wm[o]
        dm_abs = d.abs() @ wmd.abs()
        dh2 = gate2 * dm[:, None] * w3[None, :]
        dh2_abs = gate2 * dm_abs[:, None] * w3.abs()[None, :]
        dh1 = gate1 * (dh2 @ w2)                               # dh1[p][i] = sum_j w2[j][i] * dh2[p][j]
        dh1_abs = gate1 * (dh2_abs @ w2.abs())
        g["dwm"] += d.T @ m
        ga["dwm"] += d.abs().T @ out["m_abs"][s:e]
        g["gb3"] += dm.sum()
        ga["gb3"] += dm_abs.sum()
        g["gw3"] += (dm[:, None] * h2).sum(dim=0)
        ga["gw3"] += (dm_abs[:, None] * gate2 * s2).sum(dim=0)
        g["gb2"] += dh2.sum(dim=0)
        ga["gb2"] += dh2_abs.sum(dim=0)
        g["gw2"] += dh2.T @ h1
        ga["gw2"] += dh2_abs.T @ (gate1 * s1)
        g["gb1"] += dh1.sum(dim=0)
        ga["gb1"] += dh1_abs.sum(dim=0)
        g["gw1"] += dh1.T @ x
        ga["gw1"] += dh1_abs.T @ x.abs()
    if dl is not None:
        out["grads"], out["grads_abs"] = g, ga
    return out


def logits_reference(logits0, wm, m, softmax=False):
    B, ncls, H, W = logits0.shape
    z = logits0.double() + wm.double().view(1, ncls, 1, 1) * m.view(B, 1, H, W)
    return torch.softmax(z, dim=1) if softmax else z


def logits_abs(logits0, wm, m_abs):
    B, ncls, H, W = logits0.shape
    return logits0.double().abs() + wm.double().abs().view(1, ncls, 1, 1) * m_abs.view(B, 1, H, W)


def chain_length(npix):
    """Longest fp32 accumulation chain crimac_meta_bwd allows for one gradient element: the grid rule of the entry point
    (one workgroup per 256 pixels, at most 512), 256 pixel terms per thread and iteration, one atomic per workgroup, and
    the 32-term dot product inside dh1."""
    grid = min((npix + 255) // 256, 512)
    iters = -(-npix // (256 * grid))
    return 256 * iters + grid + HID


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _ternary(g, shape, density):
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * (torch.rand(shape, generator=g) < density).float()


def dlogits_density(shape, cm, ncls):
    """{-1, 0, 1} dlogits: nonzero with probability 1/8; 1/2 on the four small shapes, whose few pixels would otherwise
    leave whole gradient tensors zero (their sums stay far below 2^24).  At LARGE_FWD the 1/8 stands for every
    combination run there: the largest sum |terms| + |prefill| is measured by the precondition test."""
    B, H, W = shape
    return 0.5 if B * H * W < 2048 else 0.125


@functools.lru_cache(maxsize=None)
def exact_case(case):
    """Integer-valued inputs of one exact case and their float64 reference; computed once, shared, never modified."""
    (B, H, W), cm, ncls = case
    g = torch.Generator().manual_seed(SEED0 + 7919 * B + 1009 * H + 101 * W + 17 * cm + ncls)
    meta = torch.randint(-2, 3, (B, cm, H, W), generator=g).float()
    p = {"w1": _ternary(g, (HID, cm), 0.25), "b1": _ternary(g, (HID,), 0.25), "w2": _ternary(g, (HID, HID), 0.25),
         "b2": _ternary(g, (HID,), 0.25), "w3": _ternary(g, (1, HID), 0.25), "b3": _ternary(g, (1,), 0.25)}
    wm = _ternary(g, (ncls,), 0.25)
    # adjustments of the recipe, made on the CPU: a metadata column that is all zero would switch the whole backward
    # pass off (P = 0.56 at ncls = 2), and hidden unit 31 -- the one whose padded w1 columns lie past the end of w1 --
    # must be alive and reach m (through unit 31 of the second layer) for a wrong padding to matter
    wm[int(torch.randint(0, ncls, (1,), generator=g))] = 1.0
    p["w1"][HID - 1, 0] = 1.0
    p["b1"][HID - 1] = 1.0
    p["w2"][HID - 1] = 0.0
    p["w2"][HID - 1, HID - 1] = 1.0
    p["b2"][HID - 1] = 1.0
    p["w3"][0, HID - 1] = 1.0
    logits0 = torch.randint(-3, 4, (B, ncls, H, W), generator=g).float()
    dl = _ternary(g, (B, ncls, H, W), dlogits_density((B, H, W), cm, ncls))
    ref = mlp_reference(meta, p, wm, dl)
    prefill = {k: (torch.arange(v.numel(), dtype=torch.float64) - v.numel() // 2).reshape(v.shape)
               for k, v in ref["grads"].items()}                       # distinct small integers
    return {"meta": meta, "p": p, "wm": wm, "logits0": logits0, "dl": dl, "ref": ref, "prefill": prefill}


def _mlp_weights(cm, seed):
    """post_processing_weights.* and column 64 of conv_final.weight as synth.synth_state_dict(seed=seed,
    meta_in_channels=cm) holds them (the same per-key generator, without drawing the 31 M weights of the U-Net body)."""
    shapes = synth.unet_state_shapes(meta_in_channels=cm)
    t = {k: torch.from_numpy(np.ascontiguousarray(synth.synth_tensor(k, shapes[k], seed)))
         for k in shapes if k.startswith("post_processing_weights.") or k == "conv_final.weight"}
    pre = "post_processing_weights.main."
    p = {"w1": t[pre + "0.weight"], "b1": t[pre + "0.bias"], "w2": t[pre + "2.weight"], "b2": t[pre + "2.bias"],
         "w3": t[pre + "4.weight"], "b3": t[pre + "4.bias"]}
    return p, t["conv_final.weight"][:, 64, 0, 0].contiguous()


GATE_MARGIN = 1e-4


@functools.lru_cache(maxsize=None)
def real_case(case):
    """Real-valued inputs of one accuracy case.  Pixels whose float64 pre-activation in either hidden layer is within
    GATE_MARGIN of zero get fresh metadata until none is left (fp32 rounding could open a gate float64 closes)."""
    (B, H, W), cm, ncls = case
    seed = 11 + cm
    p, wcol = _mlp_weights(cm, seed)
    meta = torch.from_numpy(synth.synth_metadata(B, cm, H, W, seed=seed + 1))
    g = torch.Generator().manual_seed(100 * cm + ncls + H)
    # (conv_final has three rows: a fourth class, which only the CPU test against autograd asks for, is drawn alike)
    wm = torch.cat((wcol, (torch.rand(1, generator=g) * 2 - 1) / 65 ** 0.5))[:ncls].clone()
    flat = meta.permute(0, 2, 3, 1).reshape(-1, cm).clone()
    redrawn = 0
    for _ in range(64):
        gate = mlp_reference(flat.t().reshape(1, cm, -1, 1), p)["gate"]
        bad = torch.nonzero(gate < GATE_MARGIN).flatten()
        if bad.numel() == 0:
            break
        redrawn += bad.numel()
        flat[bad] = torch.rand((bad.numel(), cm), generator=g) * 1.5 - 0.25
    meta = flat.reshape(B, H, W, cm).permute(0, 3, 1, 2).contiguous()
    logits0 = torch.randn((B, ncls, H, W), generator=g)
    dl = torch.randn((B, ncls, H, W), generator=g) / (B * H * W)
    ref = mlp_reference(meta, p, wm, dl)
    return {"meta": meta, "p": p, "wm": wm, "logits0": logits0, "dl": dl, "ref": ref, "redrawn": redrawn}


# ---- CPU tests -------------------------------------------------------------------------------------------------------
def _autograd_grads(meta, p, wm, dl):
    leaves = {k: p[k].double().clone().requires_grad_(True) for k in WKEYS}
    wmd = wm.double().clone().requires_grad_(True)
    B, cm, H, W = meta.shape
    h = meta.double().permute(0, 2, 3, 1)
    h = torch.relu(torch.nn.functional.linear(h, leaves["w1"], leaves["b1"]))
    h = torch.relu(torch.nn.functional.linear(h, leaves["w2"], leaves["b2"]))
    m = torch.nn.functional.linear(h, leaves["w3"], leaves["b3"]).permute(0, 3, 1, 2)          # [B][1][H][W]
    logits = wmd.view(1, -1, 1, 1) * m
    gs = torch.autograd.grad((logits * dl.double()).sum(), [wmd] + [leaves[k] for k in WKEYS])
    return {n: t.reshape(-1) for n, t in zip(OUTPUTS, gs)}, m.detach().reshape(-1)


@pytest.mark.parametrize("case", [((3, 5, 7), 1, 2), ((3, 19, 23), 8, 4), ((3, 19, 23), 7, 3)], ids=_id)
@pytest.mark.parametrize("kind", ["integer", "real"])
def test_handwritten_backward_equals_autograd_in_float64(case, kind):
    c = exact_case(case) if kind == "integer" else real_case(case)
    want, m = _autograd_grads(c["meta"], c["p"], c["wm"], c["dl"])
    ref = c["ref"]
    assert float((ref["m"] - m).abs().max()) <= 1e-12 * float(m.abs().max())
    for k in OUTPUTS:
        got = ref["grads"][k].reshape(-1)
        scale = float(want[k].abs().max())
        assert scale > 0, k
        assert float((got - want[k]).abs().max()) <= 1e-12 * scale, k
        assert bool((ref["grads_abs"][k].reshape(-1) >= got.abs() * (1 - 1e-12)).all()), k


def _is_integer(t):
    return bool((t == t.round()).all())


@pytest.mark.parametrize("case", EXACT_CASES, ids=_id)
def test_exact_case_preconditions_hold_on_the_reference_side(case):
    """What makes `torch.equal` the right comparison, checked without a GPU: every reference value is an integer, every
    sum of |terms| (+ |prefill|) stays below 2^24, no output is degenerate, and (Cm < 8) hidden unit 31 matters."""
    c = exact_case(case)
    ref = c["ref"]
    (B, H, W), cm, ncls = case
    assert _is_integer(ref["m"]) and float(ref["m_abs"].max()) < LIMIT
    assert int((ref["m"] != 0).sum()) > 0
    z = logits_reference(c["logits0"], c["wm"], ref["m"])
    assert _is_integer(z) and float(logits_abs(c["logits0"], c["wm"], ref["m_abs"]).max()) < LIMIT
    worst = 0.0
    for k in OUTPUTS:
        assert _is_integer(ref["grads"][k]), k
        total = float((ref["grads_abs"][k] + c["prefill"][k].abs()).max())
        worst = max(worst, total)
        assert total < LIMIT, (k, total)
        # (gb3 is one sum of signed terms and may cancel to zero: it is its terms that must exist)
        live = ref["grads_abs"][k] if k == "gb3" else ref["grads"][k]
        assert int((live != 0).sum()) > 0, f"{k}: all zero, the case would test nothing"
    print(f"{_id(case)}: max sum|terms| + |prefill| = {worst:.0f} = 2^{math.log2(max(worst, 1)):.2f}")
    if cm < 8:
        dead = mlp_reference(c["meta"], c["p"], drop_unit=HID - 1)["m"]
        assert not torch.equal(dead, ref["m"]), "hidden unit 31 does not reach m: a wrong w1 padding would go unseen"


@pytest.mark.parametrize("case", REAL_CASES, ids=_id)
def test_accuracy_case_has_no_pixel_near_a_gate(case):
    c = real_case(case)
    near = int((c["ref"]["gate"] < GATE_MARGIN).sum())
    print(f"{_id(case)}: {c['redrawn']} pixels re-drawn, {near} left within {GATE_MARGIN} of a gate")
    assert near == 0                     # the cap on pixels left out of the comparison is zero
    assert c["meta"].dtype == torch.float32 and bool(torch.isfinite(c["meta"]).all())
    for k in OUTPUTS:
        assert float(c["ref"]["grads"][k].abs().max()) > 0, k


def test_chain_length_follows_the_grid_rule():
    assert chain_length(15) == 256 + 1 + 32
    assert chain_length(1311) == 256 + 6 + 32
    assert chain_length(512 * 256) == 256 + 512 + 32
    assert chain_length(3 * 211 * 209) == 2 * 256 + 512 + 32
    assert chain_length(3 * 419 * 418) == 5 * 256 + 512 + 32


# ---- GPU helpers -----------------------------------------------------------------------------------------------------
def dev_in(t):
    """An input on the device between two NaN guards: a read outside the tensor poisons what it feeds."""
    n = t.numel()
    full = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    full[GUARD:GUARD + n] = t.reshape(-1).float().cuda()
    return full[GUARD:GUARD + n]


def dev_out(n, init=None):
    """An output of n floats followed by a sentinel guard; returns the whole buffer (the kernel gets its start)."""
    full = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    if init is None:
        full[:n] = 0.0
    else:
        full[:n] = init.reshape(-1).float().cuda()
    return full


def guard_untouched(full, n):
    return bool((full[n:] == SENTINEL).all())


def run_mlp_fwd(c, shape):
    B, H, W = shape
    cm = c["meta"].shape[1]
    m = dev_out(B * H * W, init=torch.full((B * H * W,), SENTINEL))
    w = [dev_in(c["p"][k]) for k in WKEYS]
    meta = dev_in(c["meta"])            # (every device tensor keeps a name until the kernel has finished)
    call("crimac_meta_mlp_fwd", ptr(meta), cm, B, H, W, *[ptr(t) for t in w], ptr(m))
    torch.cuda.synchronize()
    return m


def run_inject(c, shape, m_dev, softmax):
    B, H, W = shape
    ncls = c["wm"].numel()
    logits = dev_out(B * ncls * H * W, init=c["logits0"])
    wm = dev_in(c["wm"])
    call("crimac_meta_inject_fwd", ptr(m_dev), ptr(wm), ptr(logits), B, H, W, ncls, 1 if softmax else 0)
    torch.cuda.synchronize()
    return logits


def run_bwd(c, shape, prefill=None):
    B, H, W = shape
    cm, ncls = c["meta"].shape[1], c["wm"].numel()
    ref = c["ref"]["grads"]
    outs = {k: dev_out(ref[k].numel(), None if prefill is None else prefill[k]) for k in OUTPUTS}
    w = [dev_in(c["p"][k]) for k in WKEYS]
    dl, meta, wm = dev_in(c["dl"]), dev_in(c["meta"]), dev_in(c["wm"])
    call("crimac_meta_bwd", ptr(dl), ptr(meta), cm, B, H, W, ncls, ptr(wm),
         *[ptr(t) for t in w], *[ptr(outs[k]) for k in OUTPUTS])
    torch.cuda.synchronize()
    return outs


# ---- exact GPU tests -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", EXACT_CASES, ids=_id)
def test_exact_forward_kernels(case):
    shape, cm, ncls = case
    B, H, W = shape
    npix = B * H * W
    c = exact_case(case)
    m = run_mlp_fwd(c, shape)
    want_m = c["ref"]["m"].float()
    bad = torch.nonzero(m[:npix].cpu() != want_m).flatten()
    assert bad.numel() == 0, f"m differs at {bad.numel()} pixels, first {bad[:8].tolist()}"
    assert guard_untouched(m, npix), "crimac_meta_mlp_fwd wrote behind m[npix]"
    logits = run_inject(c, shape, m[:npix], softmax=False)
    want = logits_reference(c["logits0"], c["wm"], c["ref"]["m"]).float().reshape(-1)
    n = want.numel()
    bad = torch.nonzero(logits[:n].cpu() != want).flatten()
    assert bad.numel() == 0, f"logits differ at {bad.numel()} elements, first {bad[:8].tolist()}"
    assert guard_untouched(logits, n), "crimac_meta_inject_fwd wrote behind the logits"


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXACT_CASES, ids=_id)
def test_exact_backward_kernel_into_zeroed_and_into_prefilled_buffers(case):
    shape, cm, ncls = case
    c = exact_case(case)
    ref = c["ref"]["grads"]
    for prefill in (None, c["prefill"]):            # the engine zeroes once and lets the kernel ADD
        outs = run_bwd(c, shape, prefill)
        what = "zeroed" if prefill is None else "prefilled"
        for k in OUTPUTS:
            want = ref[k] if prefill is None else ref[k] + prefill[k]
            want = want.float().reshape(-1)
            n = want.numel()
            got = outs[k][:n].cpu()
            bad = torch.nonzero(got != want).flatten()
            assert bad.numel() == 0, (f"{k} ({what}): {bad.numel()} of {n} differ, first {bad[:6].tolist()}: "
                                      f"got {got[bad[:6]].tolist()}, want {want[bad[:6]].tolist()}")
            assert guard_untouched(outs[k], n), f"{k} ({what}): crimac_meta_bwd wrote behind its {n} elements"


# ---- accuracy GPU tests ----------------------------------------------------------------------------------------------
def _ratio(got, ref, terms):
    """max over the elements of |got - ref| / (2^-24 * sum|terms|); an element without terms must be matched exactly."""
    diff = (got.double() - ref).abs()
    r = torch.where(diff == 0, torch.zeros_like(diff), diff / (U * terms))
    return float(r.max())


@pytest.mark.gpu
@pytest.mark.parametrize("case", REAL_CASES, ids=_id)
def test_forward_accuracy_within_the_chain_length_bound(case):
    shape, cm, ncls = case
    B, H, W = shape
    npix = B * H * W
    c = real_case(case)
    assert int((c["ref"]["gate"] < GATE_MARGIN).sum()) == 0
    m = run_mlp_fwd(c, shape)
    r = _ratio(m[:npix].cpu(), c["ref"]["m"], c["ref"]["m_abs"])
    print(f"{_id(case)}: m ratio {r:.3f} (bound 64)")
    assert r <= 64, f"|m - ref| / (2^-24 sum|terms|) = {r:.3f} > 64"
    assert guard_untouched(m, npix)
    # softmax = 0 on real data: one product and one sum on top of m
    lg = run_inject(c, shape, m[:npix], softmax=False)
    n = B * ncls * H * W
    want = logits_reference(c["logits0"], c["wm"], c["ref"]["m"]).reshape(-1)
    r0 = _ratio(lg[:n].cpu(), want, logits_abs(c["logits0"], c["wm"], c["ref"]["m_abs"]).reshape(-1))
    assert r0 <= 64 + 2, f"logits ratio {r0:.3f} > 66"
    sm = run_inject(c, shape, m[:npix], softmax=True)
    want = logits_reference(c["logits0"], c["wm"], c["ref"]["m"], softmax=True)
    got = sm[:n].cpu().double().reshape(B, ncls, H, W)
    err = float((got - want).abs().max())
    one = float((got.sum(dim=1) - 1).abs().max())
    print(f"{_id(case)}: logits ratio {r0:.3f}, softmax max err {err:.3e}, max |sum p - 1| {one:.3e}")
    assert err <= 1e-6, f"softmax differs from float64 by {err:.3e}"
    assert one <= 4 * U * ncls, f"probabilities sum to 1 within {one:.3e} > {4 * U * ncls:.3e}"
    assert guard_untouched(sm, n)


@pytest.mark.gpu
@pytest.mark.parametrize("case", REAL_CASES, ids=_id)
def test_gradient_accuracy_within_the_chain_length_bound(case):
    shape, cm, ncls = case
    B, H, W = shape
    c = real_case(case)
    assert int((c["ref"]["gate"] < GATE_MARGIN).sum()) == 0
    L = chain_length(B * H * W)
    outs = run_bwd(c, shape)
    ratios = {}
    for k in OUTPUTS:
        ref, terms = c["ref"]["grads"][k].reshape(-1), c["ref"]["grads_abs"][k].reshape(-1)
        ratios[k] = _ratio(outs[k][:ref.numel()].cpu(), ref, terms)
        assert guard_untouched(outs[k], ref.numel()), k
    msg = f"{_id(case)}: L = {L}; max |got - ref| / (2^-24 sum|terms|): " + \
          ", ".join(f"{k} {v:.3f}" for k, v in ratios.items())
    print(msg)
    assert all(v <= L for v in ratios.values()), msg


# ---- the ragged path from the public surface -------------------------------------------------------------------------
def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.gpu
def test_late_injection_net_at_a_crop_whose_plane_is_no_multiple_of_256():
    """depth 3 at B = 3, 20 x 28: HW = 560, so the workgroups of the metadata kernels straddle images and the last one is
    ragged -- a geometry no depth-5 net (H, W % 16 == 0) can produce.  Tolerances: those of tests/test_lmi.py for f32x6."""
    B, H, W, cm = 3, 20, 28, 3
    sd = synth.synth_state_dict(depth=3, seed=4, meta_in_channels=cm)
    x = torch.from_numpy(synth.synth_echogram_batch(B, 4, H, W, seed=5))
    meta = torch.from_numpy(synth.synth_metadata(B, cm, H, W, seed=6))
    lab = torch.from_numpy(synth.synth_labels(B, H, W, seed=7))
    m = pkg.UNet_LateMetInject(3, 4, cm, depth=3, precision="f32x6")
    m.load_state_dict(sd)
    m.cuda().eval()
    with torch.no_grad():
        out = m(x.cuda(), meta.cuda())
    assert _rel(out, orc.predict(sd, x, meta=meta)) < 2e-5
    ref_loss, ref_logits, ref_grads, _ = orc.loss_and_grads(sd, x, lab, meta=meta)
    m.train()
    crit = pkg.WeightedCrossEntropy([10.0, 300.0, 250.0]).cuda()
    logits = m(x.cuda(), meta.cuda())
    loss = crit(logits, lab.long().cuda())
    loss.backward()
    assert _rel(logits.detach(), ref_logits) < 2e-5
    assert abs(float(loss.detach()) - float(ref_loss)) < 1e-5 * abs(float(ref_loss))
    checked = 0
    for k, p in m.named_parameters():
        if k.startswith("post_processing_weights.") or k.startswith("conv_final."):
            want = ref_grads[k].double()
            e = float((p.grad.double().cpu() - want).norm() / want.norm())
            assert e < 2e-3, (k, e)
            checked += 1
    assert checked == 8


# ---- argument checks (nothing is launched) ---------------------------------------------------------------------------
def _tiny():
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")      # noqa: E731
    return {"meta": z(1, 8, 4, 4), "w": [z(32, 8), z(32), z(32, 32), z(32), z(1, 32), z(1)], "wm": z(4), "m": z(16),
            "logits": z(1, 4, 4, 4), "g": [z(4), z(32, 8), z(32), z(32, 32), z(32), z(32), z(1)]}


def _refuses(text):
    return pytest.raises(hip.HipLibraryError, match=re.escape(text))


@pytest.mark.gpu
@pytest.mark.parametrize("cm", [0, 9])
def test_channel_counts_outside_1_to_8_are_refused(cm):
    t = _tiny()
    with _refuses(f"meta_mlp_fwd: {cm} metadata channels (1..8 supported)"):
        call("crimac_meta_mlp_fwd", ptr(t["meta"]), cm, 1, 4, 4, *[ptr(w) for w in t["w"]], ptr(t["m"]))
    with _refuses(f"meta_bwd: {cm} metadata channels (1..8 supported)"):
        call("crimac_meta_bwd", ptr(t["logits"]), ptr(t["meta"]), cm, 1, 4, 4, 3, ptr(t["wm"]),
             *[ptr(w) for w in t["w"]], *[ptr(g) for g in t["g"]])


@pytest.mark.gpu
@pytest.mark.parametrize("ncls", [1, 5])
def test_class_counts_outside_2_to_4_are_refused(ncls):
    t = _tiny()
    with _refuses(f"meta_inject_fwd: ncls={ncls} unsupported (2..4)"):
        call("crimac_meta_inject_fwd", ptr(t["m"]), ptr(t["wm"]), ptr(t["logits"]), 1, 4, 4, ncls, 0)
    with _refuses(f"meta_bwd: ncls={ncls} unsupported (2..4)"):
        call("crimac_meta_bwd", ptr(t["logits"]), ptr(t["meta"]), 8, 1, 4, 4, ncls, ptr(t["wm"]),
             *[ptr(w) for w in t["w"]], *[ptr(g) for g in t["g"]])


@pytest.mark.gpu
def test_null_pointers_and_empty_batches_are_refused():
    t = _tiny()
    for missing in range(7):                    # each of the seven gradient outputs in turn
        g = [None if i == missing else ptr(v) for i, v in enumerate(t["g"])]
        with _refuses("meta_bwd: bad arguments"):
            call("crimac_meta_bwd", ptr(t["logits"]), ptr(t["meta"]), 8, 1, 4, 4, 3, ptr(t["wm"]),
                 *[ptr(w) for w in t["w"]], *g)
    with _refuses("meta_bwd: bad arguments"):
        call("crimac_meta_bwd", ptr(t["logits"]), ptr(t["meta"]), 8, 0, 4, 4, 3, ptr(t["wm"]),
             *[ptr(w) for w in t["w"]], *[ptr(g) for g in t["g"]])
    with _refuses("meta_mlp_fwd: bad arguments"):
        call("crimac_meta_mlp_fwd", ptr(t["meta"]), 8, 0, 4, 4, *[ptr(w) for w in t["w"]], ptr(t["m"]))
    with _refuses("meta_mlp_fwd: bad arguments"):
        call("crimac_meta_mlp_fwd", ptr(t["meta"]), 8, 1, 4, 4, *[ptr(w) for w in t["w"]], None)
    with _refuses("meta_inject_fwd: bad arguments"):
        call("crimac_meta_inject_fwd", ptr(t["m"]), ptr(t["wm"]), ptr(t["logits"]), 0, 4, 4, 3, 0)
    # the refusals left every buffer as it was
    torch.cuda.synchronize()
    assert all(float(g.abs().max()) == 0 for g in t["g"]) and float(t["m"].abs().max()) == 0
