"""Tiled evaluation with eval_mode 'region' / 'trace' for every model kind (no metadata, metadata input channels, late
injection): ``crimac_gather_patches_memm_labels`` -- the memm gather whose set_data_border_value goes by the TRANSFORMED
labels of the patch -- and ``ChunkPredictor.evaluate`` / ``evaluate_echogram_memm`` on top of it.

The dB transform itself is pinned by tests/test_tiling.py (gather kernels against the oracle); here it is restated in
numpy to the tolerances of that test, and everything the new kernel adds -- which pixels the border rule zeroes, the crop
placement, the channel order, the metadata planes, the padding -- is held to bit equality against the existing kernels."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_survey_eval as se  # noqa: E402
from oracle import tiling_oracle as torc  # noqa: E402
from test_survey_eval_cpu import golden_hist, load, make_reader  # noqa: E402

pytestmark = pytest.mark.gpu
PRECISIONS = ["bf16", "fp16", "f32x6", "h3p"]
STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32x6": torch.float32, "h3p": torch.float32}
ALL_META = {k: True for k in torc.META_KEYS}
C, WD, H, PING0, N_META = 4, 40, 48, 7, 60
# (range idx, GLOBAL ping idx): over the top, bottom, left and right edge of the chunk, fully inside, over a corner
CENTRES = np.array([[3, PING0 + 20], [46, PING0 + 20], [24, PING0 + 2], [24, PING0 + 38], [24, PING0 + 20],
                    [1, PING0 + 39]], dtype=np.int32)
# (flags, db_scaled): no planes (a model without metadata, or late injection), 2 planes, all 7 -- C + 7 = 11 of 16 channels
PLANE_CASES = [(0, 0), (2, 1), (63, 1)]


def decode(x, precision):
    """NHWC activations [N, 16] of a storage type -> float32 (h3p: 8-channel groups of [8 x hi][8 x lo] halves)."""
    if precision == "h3p":
        h = x.contiguous().view(torch.float16).reshape(-1, 2, 2, 8).float()
        return (h[:, :, 0] + h[:, :, 1]).reshape(-1, 16)
    return x.float()


def zero_data_channels(x, rows, precision):
    """Storage-type rows ``rows`` of x [N, 16]: channels 0..C-1 := +0.0 (C = 4 <= 8: the first 8-channel group)."""
    x = x.clone()
    if precision == "h3p":
        v = x.view(torch.float16).reshape(-1, 2, 2, 8)          # [row][group][hi / lo][channel in group]
        v[rows, 0, :, :C] = 0
    else:
        x[rows, :C] = 0
    return x


@pytest.fixture(scope="module")
def chunk():
    """One small chunk, built once: data [C, WD, H] linear sv with NaN / inf samples, raw ids [WD, H] with a block of
    -100 and a block of -1, the per-ping metadata vectors, and per-patch 'transformed' labels for 16 x 16 and 40 x 24
    patches (-100 inside every patch, -1, -50, -70 and ordinary classes)."""
    rng = np.random.Generator(np.random.PCG64(11))
    data = np.power(10.0, rng.uniform(-7.5, 0.0, size=(C, WD, H))).astype(np.float32)
    data[0][rng.random((WD, H)) < 0.01] = np.nan
    data[2][rng.random((WD, H)) < 0.01] = np.inf
    raw = np.zeros((WD, H), dtype=np.int16)
    raw[5:12, 30:40] = 27
    raw[16:20, 20:24] = -100          # block A: raw id -100 (the extended mask may turn it into -1)
    raw[22:26, 26:30] = -1            # block B: raw id -1 (ignore -> -100 after the label transform)
    data[:, 16:20, 20:24] = np.float32(2e-3)          # block A carries a plain echo: its dB value is far from 0
    labels_t = {}
    for ph, pw in ((16, 16), (40, 24)):
        lt = rng.choice(np.array([-100, -1, 0, 1, 2, -50, -70], dtype=np.int16), size=(len(CENTRES), ph, pw),
                        p=[0.25, 0.15, 0.3, 0.1, 0.1, 0.05, 0.05])
        assert all((lt[p] == -100).any() and (lt[p] != -100).any() for p in range(len(CENTRES)))
        labels_t[(ph, pw)] = lt
    meta = dict(portion_year=0.37, portion_day=rng.random(N_META), time_diff=rng.uniform(-1, 1, N_META),
                seabed=rng.integers(30, 46, N_META).astype(np.int64))
    return types.SimpleNamespace(data=data, raw=raw, labels_t=labels_t, meta=meta)


class Launcher:
    """The chunk on the GPU and the three gather entry points into fresh sentinel-filled buffers."""

    def __init__(self, chunk, precision, ph, pw, centres=CENTRES):
        from crimac_classifiers_unet_amd import hip
        self.prec, self.precision, self.ph, self.pw, self.P = hip.PREC_NAMES[precision], precision, ph, pw, len(centres)
        self.data = torch.from_numpy(chunk.data).cuda()
        self.raw = torch.from_numpy(chunk.raw).cuda()
        loc = centres.copy()
        loc[:, 1] -= PING0
        self.loc_host = loc
        self.loc, self.cen = torch.from_numpy(loc).cuda(), torch.from_numpy(np.ascontiguousarray(centres)).cuda()
        m = chunk.meta
        self.vec = {k: torch.from_numpy(m[k]).cuda() for k in ("portion_day", "time_diff", "seabed")}
        self.year = m["portion_year"]

    def out(self):
        return torch.full(((self.P + 1) * self.ph * self.pw, 16), 3.0, dtype=STORAGE[self.precision], device="cuda")

    def _meta_args(self, flags):
        from crimac_classifiers_unet_amd.hip import ptr
        v = self.vec
        return (flags, self.year, ptr(v["portion_day"]), N_META, ptr(v["time_diff"]), N_META, ptr(v["seabed"]), N_META,
                ptr(self.cen))

    def head(self, x):
        from crimac_classifiers_unet_amd.hip import ptr
        return (self.prec, ptr(self.data), C, WD, H, ptr(self.loc), self.P, self.ph, self.pw, ptr(x), 16)

    def by_patch_labels(self, labels_t, flags, scaled):
        from crimac_classifiers_unet_amd.hip import call, ptr
        x, lt = self.out(), torch.from_numpy(np.ascontiguousarray(labels_t)).cuda()
        call("crimac_gather_patches_memm_labels", *self.head(x), ptr(lt), scaled, *self._meta_args(flags))
        torch.cuda.synchronize()
        return x

    def by_raw_ids(self, raw_ids, flags, scaled):
        """crimac_gather_patches_memm (no planes) / crimac_gather_patches_memm_meta with the border rule by ``raw_ids``."""
        from crimac_classifiers_unet_amd.hip import call, ptr
        x = self.out()
        if flags:
            call("crimac_gather_patches_memm_meta", *self.head(x), ptr(raw_ids), scaled, *self._meta_args(flags))
        else:
            assert not scaled
            call("crimac_gather_patches_memm", *self.head(x), ptr(raw_ids))
        torch.cuda.synchronize()
        return x

    def without_border_rule(self, flags, scaled):
        """Crop + dB transform (+ planes) and no border rule at all, by the existing kernels: crimac_gather_patches (the
        zarr gather: -75 dB outside the chunk), or crimac_gather_patches_memm_meta over all-zero ids (scaled: the 0.0 it
        writes outside the chunk IS the scaled -75 dB, 1 + (-75) / 75)."""
        from crimac_classifiers_unet_amd.hip import call
        if flags or scaled:
            assert flags and scaled
            return self.by_raw_ids(torch.zeros_like(self.raw), flags, scaled)
        x = self.out()
        call("crimac_gather_patches", *self.head(x))
        torch.cuda.synchronize()
        return x

    def raw_label_crops(self):
        from crimac_classifiers_unet_amd.hip import call, ptr
        d = torch.empty((self.P, C, self.ph, self.pw), dtype=torch.float32, device="cuda")
        lab = torch.empty((self.P, self.ph, self.pw), dtype=torch.int16, device="cuda")
        call("crimac_gather_eval_crops", ptr(self.data), C, WD, H, ptr(self.raw), ptr(self.loc), self.P, self.ph, self.pw, 1,
             ptr(d), ptr(lab))
        torch.cuda.synchronize()
        return lab.cpu().numpy()


def restate_data_channels(data, loc, labels_t, ph, pw, scaled):
    """The data channels of x in numpy, float32 [P, ph, pw, C]: get_crop_memmap's crop (getGrid placement, 0 outside,
    non-finite -> 0), db_with_limits (_scaled), set_data_border_value by the given labels."""
    out = np.zeros((len(loc), ph, pw, C), dtype=np.float32)
    for p, (cy, cx) in enumerate(loc):
        ys, xs = cy - (ph + 1) // 2 + 1 + np.arange(ph), cx - (pw + 1) // 2 + 1 + np.arange(pw)
        crop = np.zeros((C, ph, pw), dtype=np.float32)
        iy, ix = (ys >= 0) & (ys < H), (xs >= 0) & (xs < WD)
        crop[:, iy[:, None] & ix[None, :]] = data[:, xs[ix]][:, :, ys[iy]].transpose(0, 2, 1).reshape(C, -1)
        crop[~np.isfinite(crop)] = 0
        db = np.clip(np.float32(10) * np.log10(crop + np.float32(1e-10)), np.float32(-75), np.float32(0)).astype(np.float32)
        if scaled:
            db = np.float32(1) + db / np.float32(75)
        db[:, labels_t[p] == -100] = 0
        out[p] = db.transpose(1, 2, 0)
    return out


def data_tolerance(ref, precision, scaled):
    """Per element.  fp32 storage: what tests/test_tiling.py allows the dB transform against numpy on values up to 75
    (2e-5; plane pairs 4e-5), divided by 75 for the scaled form plus one rounding of 1 + dB / 75 near 1 (2^-24).  16-bit
    storage: that plus ONE rounding to the type, half an ulp of the value (bf16 8, fp16 11 significand bits) -- at 75 dB
    0.25 for bf16, inside the flat 0.3 of that test."""
    base = 4e-5 if precision == "h3p" else 2e-5
    tol = np.full(ref.shape, base / 75 + 2.0 ** -24 if scaled else base)
    if precision in ("bf16", "fp16"):
        e = np.floor(np.log2(np.maximum(np.abs(ref), 1e-30)))
        tol = tol + 2.0 ** (e - (8 if precision == "bf16" else 11))
    return tol


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", [(16, 16), (40, 24)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gather_by_patch_labels_against_a_cpu_restatement(chunk, precision, patch):
    """Six patches (over each of the four edges, inside, over a corner) of 16 x 16 and of 40 x 24 pixels (more than one
    tile, no multiple of it) from a 40-ping x 48-row chunk whose first ping is global ping 7; 0, 2 and 7 metadata planes.
    Data channels: the numpy restatement within ``data_tolerance``; the whole output -- data, planes, padding -- equal BIT
    FOR BIT to the existing kernels' crop without a border rule with the data channels of the -100 pixels set to 0.0, which
    makes the planes bit-identical to crimac_gather_patches_memm_meta's; the sentinel rows after the last patch untouched."""
    ph, pw = patch
    run = Launcher(chunk, precision, ph, pw)
    lt = chunk.labels_t[patch]
    n = run.P * ph * pw
    border = torch.from_numpy((lt == -100).reshape(-1)).cuda()
    for flags, scaled in PLANE_CASES:
        got = run.by_patch_labels(lt, flags, scaled)
        sentinel = run.out()
        assert torch.equal(got[n:].view(torch.uint8), sentinel[n:].view(torch.uint8)), (flags, "sentinel rows")
        want = zero_data_channels(run.without_border_rule(flags, scaled)[:n], border, precision)
        assert torch.equal(got[:n].view(torch.uint8), want.view(torch.uint8)), (flags, "bits")
        val = decode(got[:n], precision).cpu().numpy().reshape(run.P, ph, pw, 16)
        n_planes = bin(flags).count("1") + (1 if flags & 2 else 0)
        assert (val[..., C + n_planes:] == 0).all(), (flags, "padding")
        assert not n_planes or all((val[..., C + k] != 0).any() for k in range(n_planes)), (flags, "planes are written")
        ref = restate_data_channels(chunk.data, run.loc_host, lt, ph, pw, scaled)
        err = np.abs(val[..., :C] - ref)
        tol = data_tolerance(ref, precision, scaled)
        print(f"{precision} {patch} flags {flags}: largest data error {err.max():.3e}, largest share of the tolerance "
              f"{(err / tol).max():.3f}")
        assert (err <= tol).all(), (flags, float((err / tol).max()))
        assert (val[..., :C][lt == -100] == 0).all() and (val[..., :C][lt != -100] != 0).any()


def test_gather_by_patch_labels_refuses_bad_arguments(chunk):
    from crimac_classifiers_unet_amd.hip import HipLibraryError, call, ptr
    run = Launcher(chunk, "f32x6", 16, 16)
    x, lt = run.out(), torch.from_numpy(chunk.labels_t[(16, 16)]).cuda()
    with pytest.raises(HipLibraryError, match="transformed labels"):
        call("crimac_gather_patches_memm_labels", *run.head(x), None, 0, *run._meta_args(0))
    with pytest.raises(HipLibraryError, match="flags"):
        call("crimac_gather_patches_memm_labels", *run.head(x), ptr(lt), 0, *run._meta_args(64))
    with pytest.raises(HipLibraryError, match="seabed"):
        call("crimac_gather_patches_memm_labels", *run.head(x), ptr(lt), 1, 8, 0.0, None, 0, None, 0, None, 0, ptr(run.cen))
    with pytest.raises(HipLibraryError, match="do not fit"):          # 12 data + 7 metadata channels in 16
        call("crimac_gather_patches_memm_labels", run.prec, ptr(run.data), 12, WD, H, ptr(run.loc), run.P, 16, 16, ptr(x), 16,
             ptr(lt), 1, *run._meta_args(63))
    torch.cuda.synchronize()
    assert torch.equal(x, run.out())


# ---- 2. where the border rule takes its labels from -------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_border_rule_follows_the_transformed_labels_not_the_raw_ids(chunk, precision):
    """One patch over block A (raw id -100) and block B (raw id -1).  Transformed as the extended mask leaves them -- A
    became -1, B -100 -- the new kernel writes A's plain dB value where the raw-id kernels write 0.0, and the same bytes
    everywhere else; without and with metadata planes."""
    centre = np.array([[24, PING0 + 20]], dtype=np.int32)            # rows 17..32, pings 13..28 of the chunk
    run = Launcher(chunk, precision, 16, 16, centre)
    raw_crop = run.raw_label_crops()
    block_a = raw_crop == -100
    assert block_a.sum() == 16 and (raw_crop == -1).sum() == 16
    lt = np.where(raw_crop < 0, -100, raw_crop).astype(np.int16)
    lt[block_a] = -1
    a_rows = torch.from_numpy(block_a.reshape(-1)).cuda()
    for flags, scaled in ((0, 0), (63, 1)):
        new = decode(run.by_patch_labels(lt, flags, scaled)[:256], precision)
        old = decode(run.by_raw_ids(run.raw, flags, scaled)[:256], precision)
        assert torch.equal(new[~a_rows], old[~a_rows])
        assert bool((old[a_rows, :C] == 0).all()) and bool((new[a_rows, :C] != 0).all())
        assert torch.equal(new[a_rows, C:], old[a_rows, C:])
        plain = decode(run.without_border_rule(flags, scaled)[:256], precision)
        assert torch.equal(new[a_rows], plain[a_rows])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_with_the_labels_of_eval_mode_all_it_is_the_existing_kernels(chunk, precision):
    """Transformed labels that are -100 exactly where the raw id is negative or the pixel lies outside the chunk (what
    eval_mode 'all' leaves): the output equals crimac_gather_patches_memm's and crimac_gather_patches_memm_meta's bit for
    bit, on the six edge patches."""
    run = Launcher(chunk, precision, 16, 16)
    raw_crop = run.raw_label_crops()
    lt = np.where(raw_crop < 0, -100, raw_crop).astype(np.int16)
    assert (raw_crop[4] >= 0).any() and (raw_crop[0] == -100).any()
    for flags, scaled in PLANE_CASES:
        if flags == 0:
            assert not scaled
        new, old = run.by_patch_labels(lt, flags, scaled), run.by_raw_ids(run.raw, flags, scaled)
        assert torch.equal(new.view(torch.uint8), old.view(torch.uint8)), flags


# ---- 3. the whole path with a linear stub, exact -----------------------------------------------------------------------------
def linear_stub(precision, scaled):
    """x [N, 16] -> three logits per pixel, a fixed linear map over ALL 16 channels (weights of the dB channels sized to
    their range: 75 unscaled, 1 scaled), accumulated channel by channel with elementwise operations only: the same bits
    whatever the batch."""
    w = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).uniform(-1, 1, size=(16, 3)).astype(np.float32)).cuda()
    if not scaled:
        w[:C] *= 0.04

    def core(xf, P, Hh, Ww):
        z = torch.zeros((xf.shape[0], 3), dtype=torch.float32, device=xf.device)
        for k in range(16):
            z = z + xf[:, k:k + 1] * w[k]
        return z.reshape(P, Hh, Ww, 3).permute(0, 3, 1, 2).contiguous()

    def fn(x, P, Hh, Ww):
        return core(decode(x, precision), P, Hh, Ww)
    return fn, core


def meta_model(kind, precision):
    import crimac_classifiers_unet_amd as pkg
    from crimac_classifiers_unet_amd import synth
    if kind == "late":
        model = pkg.UNet_LateMetInject(3, 4, 7, precision=precision)
        model.load_state_dict(synth.synth_state_dict(seed=3, meta_in_channels=7))
    elif kind == "early":
        model = pkg.UNet_Baseline(3, 11, precision=precision)
        model.load_state_dict(synth.synth_state_dict(seed=3, in_channels=11))
    else:
        model = pkg.UNet_Baseline(3, 4, precision=precision)
        model.load_state_dict(synth.synth_state_dict(seed=3))
    return model


@pytest.mark.parametrize("precision", ["h3p", "bf16"])
@pytest.mark.parametrize("kind", ["none", "early", "late"])
def test_evaluate_region_and_trace_equal_the_per_batch_pieces(golden_dir, kind, precision):
    """ChunkPredictor.evaluate (eval_mode 'region' and 'trace', linear stub) on the memm echogram of the survey fixture
    (schools, seabed, ignore ids), int32 for int32 against a histogram built per batch from the existing pieces:
    crimac_gather_eval_crops -> crimac_labels_test_transform + crimac_labels_extend_mask -> x restated on the CPU -> the
    same stub -> crimac_pr_histogram.

    The restated x takes its dB values (and, for the early-injection model, its planes) from the existing augment kernel
    over the raw crops -- a linear stub turns the last bit of a host log10 into other float16 bins, and the dB transform is
    not what is new here -- and applies set_data_border_value on the CPU: data channels of the pixels whose transformed
    label is -100 := 0.0.  Without metadata the histogram also equals the one of raw_crops_to_logits(border_to_0db=True),
    the masked_fill + augment_batch route this path took before."""
    from crimac_classifiers_unet_amd import tiled_inference as ti
    from crimac_classifiers_unet_amd.hip import call, ptr
    fix = load(golden_dir)
    pw, ph, overlap = (int(v) for v in fix["patch"])
    pipe = se.make_pipe(model=meta_model(kind, precision))
    eng = pipe.model.infer_engine
    early = kind == "early"
    eg = se.meta_echogram(fix)
    fn, core = linear_stub(precision, early)
    batch = 8
    cp, seabed = ti._load_echogram_memm(eg, pipe, (pw, ph), overlap, batch, None if kind == "none" else ALL_META,
                                        out_f16=False, wide=True)
    grid = ti.plan_eval_grid(cp.n_range, seabed, cp.end_ping, (pw, ph), overlap, memm=True)
    for mode in ("region", "trace"):
        boxes = torch.from_numpy(ti.eval_boxes(eg, mode)).cuda()
        hist = torch.zeros(2, ti.PR_BINS, dtype=torch.int32, device="cuda")
        seen = []
        cp.evaluate(grid, hist, mode, boxes, predict_fn=fn, on_batch=lambda c, l, z: seen.append(l.cpu().numpy().copy()))
        want = torch.zeros_like(hist)
        detour = torch.zeros_like(hist)
        moved = 0
        for b0 in range(0, len(grid), batch):
            cen = grid[b0:b0 + batch].astype(np.int32)
            P = len(cen)
            cen_d = torch.from_numpy(np.ascontiguousarray(cen)).cuda()          # (data_ping0 = 0: local == global)
            cen64 = cen_d.long().contiguous()
            raw = torch.empty((P, C, ph, pw), dtype=torch.float32, device="cuda")
            lab = torch.empty((P, ph, pw), dtype=torch.int16, device="cuda")
            call("crimac_gather_eval_crops", ptr(cp.data), C, cp.data.shape[1], cp.n_range, ptr(cp.labels), ptr(cen_d), P,
                 ph, pw, 1, ptr(raw), ptr(lab))
            lt = torch.empty_like(lab)
            call("crimac_labels_test_transform", ptr(lab), 2, ptr(raw), C - 1, 1e-7, 1e-4, ptr(cen64), ptr(cp.seabed), 0,
                 cp.seabed.numel(), None, 0, 0, cp.n_range, ti.SEABED_PAD, 1, overlap, ptr(lt), P, C, ph, pw)
            call("crimac_labels_extend_mask", ptr(lt), ptr(raw), C, ptr(cen64), ptr(boxes), int(boxes.shape[0]), -1, P, ph,
                 pw)
            assert np.array_equal(lt.cpu().numpy(), seen[b0 // batch])
            if early:
                both = torch.cat((raw, cp.meta_source.planes(cen_d, (pw, ph))), 1).contiguous()
                xdb, _ = eng.augment_batch(both, None, 0, do_noise=False, do_flip=False, db_scaled=True, n_data=C)
            else:
                xdb, _ = eng.augment_batch(raw, None, 0, do_noise=False, do_flip=False)
            xe = decode(xdb, precision).cpu().numpy()
            border = (lt.cpu().numpy() == -100).reshape(-1)
            xe[border, :C] = 0.0                                                  # set_data_border_value
            logits = core(torch.from_numpy(xe).cuda(), P, ph, pw)
            call("crimac_pr_histogram", ptr(logits), 3, ptr(lt), 2, P, ph, pw, ptr(want[0]), ptr(want[1]))
            # the rule by the raw ids would zero other pixels: the test can tell the two label sources apart
            moved += int(((lab.cpu().numpy() < 0) != (lt.cpu().numpy() == -100)).sum())
            if kind == "none":
                z, lt2 = ti.raw_crops_to_logits(
                    eng, raw, lab, cen64, thr_channel=C - 1, seabed=cp.seabed, seabed_ping0=0,
                    seabed_pings=cp.seabed.numel(), mask=None, mask_ping0=0, mask_pings=0, n_range=cp.n_range,
                    pad=ti.SEABED_PAD, seabed_rule=1, overlap=overlap, boxes=boxes, predict_fn=fn, split=True,
                    border_to_0db=True)
                assert torch.equal(lt2, lt)
                call("crimac_pr_histogram", ptr(z), 3, ptr(lt2), 2, P, ph, pw, ptr(detour[0]), ptr(detour[1]))
        torch.cuda.synchronize()
        assert moved > 0, mode
        assert int(want.sum()) > 1000 and int((want > 0).sum()) > 50, (mode, "the stub spreads over the bins")
        diff = int((hist.long() - want.long()).abs().sum())
        print(f"{kind} {precision} {mode}: {int(hist.sum())} pixels in {int((hist > 0).sum())} bins, |difference| {diff}")
        assert torch.equal(hist, want), (mode, diff)
        if kind == "none":
            assert torch.equal(hist, detour), (mode, int((hist.long() - detour.long()).abs().sum()))


# ---- 4. the whole path with the real networks --------------------------------------------------------------------------------
class ValidPixels:
    """on_batch hook: the pixels crimac_pr_histogram counts, from the transformed labels (set_label_ignore_val,
    pipeline.py:222-239: -70, -30, -100 and -10 are ignored; -50 counts as background)."""

    def __init__(self):
        self.n = 0

    def __call__(self, centres, labels, logits):
        self.n += int((~torch.isin(labels, torch.tensor([-70, -30, -100, -10], dtype=labels.dtype,
                                                         device=labels.device))).sum())
        assert bool(torch.isfinite(logits).all())


@pytest.mark.parametrize("kind", ["late", "early"])
def test_metadata_models_evaluate_in_region_mode(golden_dir, kind, tmp_path):
    """UNet_LateMetInject and an early-injection UNet_Baseline (h3p, synthetic weights) through evaluate_echogram_memm
    (eval_mode 'region') on the memm echogram of the survey fixture: the call returns, the histograms' total is the number
    of valid pixels of the transformed labels -- which is the reference's own total for this echogram and mode (fixture) --
    and the PR curve / F1 are finite.  validate_model_survey_memm(tiled=True) gives the same curve.

    The DataLoader flow of this repository (SegPipe._predict_raw_batch with use_gpu_test_transform) takes zarr readers
    only -- it refuses a memmap reader -- so it does not cover this combination and there is no second flow to compare the
    bins with: test_evaluate_region_and_trace_equal_the_per_batch_pieces is the exact check."""
    from crimac_classifiers_unet_amd import evaluate, tiled_inference as ti
    from crimac_classifiers_unet_amd.pipeline import SegPipe
    fix = load(golden_dir)
    pw, ph, overlap = (int(v) for v in fix["patch"])
    pipe = se.make_pipe(model=meta_model(kind, "h3p"))
    eg = se.meta_echogram(fix)
    valid = ValidPixels()
    hp, hn = ti.evaluate_echogram_memm(eg, pipe, (pw, ph), overlap, 4, eval_mode="region", meta_channels=ALL_META,
                                       on_batch=valid)
    ghp, ghn = golden_hist(fix, "memm", "region")
    assert hp.sum() + hn.sum() == valid.n > 1000
    assert hp.sum() == ghp.sum() > 0 and hn.sum() == ghn.sum()
    m = SegPipe.compute_evaluation_metrics_from_histograms(hp, hn)
    assert all(np.isfinite(m[k]).all() for k in ("precision", "recall", "F1")) and len(m["F1"]) > 1
    # the public function: needs a pipeline object that writes the csv
    pipe.model_is_loaded = True
    pipe.validate_model_testing_from_histograms = lambda a, b, **kw: SegPipe.compute_evaluation_metrics_from_histograms(a, b)
    m2 = evaluate.validate_model_survey_memm([eg], pipe, ALL_META, (pw, ph), overlap, "region", 4, 0, str(tmp_path),
                                             None, tiled=True)
    assert np.array_equal(m2["F1"], m["F1"])
