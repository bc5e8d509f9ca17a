"""Whole-survey evaluation on the tiled GPU path (tiled_inference.evaluate_survey / evaluate_echogram_memm): the
``crimac_gather_eval_crops`` kernel, the whole flow against the reference's results (tests/golden/survey_eval.npz, predictor
stub), against this repository's DataLoader-fed path (real network), on two ranks, with metadata models and NaN weights."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import tiling_oracle as torc  # noqa: E402
from test_survey_eval_cpu import CASES, MODES, golden_hist, load, make_reader  # noqa: E402
from tools.fake_reader import eval_stub_logits, synth_eval_survey  # noqa: E402

pytestmark = pytest.mark.gpu
FREQS = [18, 38, 120, 200]
FMAX = np.finfo(np.float32).max

# Measured on an MI355X with the DataLoader-fed path (use_gpu_test_transform + get_pr_histograms_dataloader, infer_precision
# 'h3p', synthetic weights) run against ITSELF at batch sizes 8 and 32 on the 'zarr' survey of the fixture: share of the
# valid pixels that change their float16 bin (sum |cumsum difference| / valid pixels), and |max F1 difference|.  The tiled
# flow cuts other batches again (one per chunk), so it is allowed twice that.
SELF_MOVED_SHARE = 0.0
SELF_F1_DIFF = 0.0
# evaluate_echogram_memm against itself with internal batches of 8 and of 32 patches, both metadata models: largest
# difference of a sandeel probability
SELF_PROB_DIFF = 0.0


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


def make_pipe(precision="h3p", model=None, seed=0):
    import crimac_classifiers_unet_amd as pkg
    from crimac_classifiers_unet_amd import synth
    if model is None:
        model = pkg.UNet_Baseline(3, 4, precision=precision)
        model.load_state_dict(synth.synth_state_dict(seed=seed))
    model.cuda().eval()
    return types.SimpleNamespace(model=model, device=torch.device("cuda"), frequencies=FREQS)


class Counts:
    """on_batch hook: per-patch counts of every transformed label value, keyed by centre."""

    def __init__(self, values):
        self.values, self.rows = values, []

    def __call__(self, centres, labels, logits):
        lab = labels.cpu().numpy()
        for c, l in zip(centres, lab):
            self.rows.append((tuple(int(v) for v in c), [int((l == v).sum()) for v in self.values]))


# ---- 4. the kernel -------------------------------------------------------------------------------------------------------
def run_kernel(data, labels, centres, size, flavour):
    from crimac_classifiers_unet_amd.hip import call, ptr
    C, Wd, H = data.shape
    d = torch.from_numpy(data).cuda()
    l = torch.from_numpy(labels.astype(np.int16)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(np.asarray(centres, dtype=np.int32))).cuda()
    P = len(centres)
    out_d = torch.full((P, C, size, size), -7.0, dtype=torch.float32, device="cuda")
    out_l = torch.full((P, size, size), 77, dtype=torch.int16, device="cuda")
    call("crimac_gather_eval_crops", ptr(d), C, Wd, H, ptr(l), ptr(c), P, size, size, flavour, ptr(out_d), ptr(out_l))
    torch.cuda.synchronize()
    return out_d.cpu().numpy(), out_l.cpu().numpy()


def expected_crop(sv_hw, lab_hw, c, size, flavour):
    c = np.array(c)
    if flavour == 1 and sv_hw.shape[1] <= size:
        c[0] = sv_hw.shape[1] // 2
    raw = torc.crop(sv_hw, c, (size, size), 0).astype(np.float32)
    raw = np.where(np.isfinite(raw), raw, np.float32(0)) if flavour == 1 else np.nan_to_num(raw, nan=0.0)
    return raw, torc.crop(lab_hw, c, (size, size), -100).astype(np.int16)


@pytest.mark.parametrize("shape", [(437, 150, 21), (301, 50, 22)])
def test_gather_eval_crops_is_bit_exact(shape):
    """crimac_gather_eval_crops against the tiling oracle's crop (pinned to the reference's new_get_crop_2d / 3d; for the
    even sizes used here get_crop_zarr places the patch identically) with the flavour's non-finite rule: bit-exact data
    and labels, both flavours, patch sizes 64 / 96 / 128 / 256, centres inside, on every border, fully outside -- on a
    range axis longer (150) and shorter (50) than every patch."""
    n_pings, n_range, seed = shape
    sv, labels, _, _ = synth_eval_survey(n_pings, n_range, seed)
    sv_hw, lab_hw = np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T)
    centres = [(n_range // 2, n_pings // 2), (0, 0), (n_range - 1, n_pings - 1), (3, n_pings // 3), (n_range - 2, 200),
               (n_range // 2, 5), (n_range // 3, n_pings - 4), (-40, 100), (n_range + 500, 50), (20, -700),
               (10, n_pings + 300), (31, 31), (n_range // 2 + 1, 257)]
    for flavour in (0, 1):
        for size in (64, 96, 128, 256):
            got_d, got_l = run_kernel(sv, labels, centres, size, flavour)
            nonfinite_seen = False
            for p, c in enumerate(centres):
                want_d, want_l = expected_crop(sv_hw, lab_hw, c, size, flavour)
                assert np.array_equal(got_d[p].view(np.uint32), want_d.view(np.uint32)), (flavour, size, c)
                assert np.array_equal(got_l[p], want_l), (flavour, size, c)
                nonfinite_seen |= bool((want_d == FMAX).any())
            assert nonfinite_seen == (flavour == 0)
    # a chunk that is a slice of the survey: centres relative to the slice, the slice covering the patches
    lo, hi = 120, 330
    got_d, got_l = run_kernel(np.ascontiguousarray(sv[:, lo:hi]), labels[lo:hi], [(40, 225 - lo), (n_range - 5, 160 - lo)], 64, 0)
    for p, c in enumerate([(40, 225), (n_range - 5, 160)]):
        want_d, want_l = expected_crop(sv_hw, lab_hw, c, 64, 0)
        assert np.array_equal(got_d[p], want_d) and np.array_equal(got_l[p], want_l)
    # an odd patch size takes the scalar stores; getGrid (memm) and patch_coord_to_data_coord (zarr) then place the patch
    # one pixel apart: the zarr crop around c is the getGrid crop around c + 1
    for flavour in (0, 1):
        got_d, got_l = run_kernel(sv, labels, [(30, 100), (2, n_pings - 3)], 63, flavour)
        for p, c in enumerate([(30, 100), (2, n_pings - 3)]):
            cc = (c[0] + 1, c[1] + 1) if flavour == 0 else c
            if flavour == 1 and n_range <= 63:
                cc = (n_range // 2, c[1])
            want_d, want_l = expected_crop(sv_hw, lab_hw, cc, 63, flavour)
            assert np.array_equal(got_d[p], want_d) and np.array_equal(got_l[p], want_l), (flavour, c)


def test_gather_eval_crops_equals_the_references_own_crops(golden_dir):
    """... and against the crops the reference's get_crop_zarr / get_crop_memmap produced (fixture): raw data (the zarr
    flavour's float64 crop holds nan_to_num's 1.8e308 for an inf sample: saturated to the largest float32) and raw labels."""
    fix = load(golden_dir)
    for case in CASES:
        n_pings, n_range, seed = (int(v) for v in fix[f"{case}/shape"])
        sv, labels, _, _ = synth_eval_survey(n_pings, n_range, seed)
        idx = fix[f"{case}/crop_idx"].tolist()
        centres = fix[f"{case}/centres"][idx]
        got_d, got_l = run_kernel(sv, labels, centres, 64, 1 if case.startswith("memm") else 0)
        for p, i in enumerate(idx):
            want = np.clip(fix[f"{case}/crop{i}/raw_data"], -FMAX, FMAX).astype(np.float32)
            assert np.array_equal(got_d[p], want), (case, i)
            assert np.array_equal(got_l[p], fix[f"{case}/crop{i}/raw_labels"]), (case, i)


# ---- 5. the whole flow with the stub against the reference -----------------------------------------------------------------
@pytest.mark.parametrize("precision", ["h3p", "f32x6"])
def test_whole_flow_with_the_stub_equals_the_reference(golden_dir, precision):
    """evaluate_survey / evaluate_echogram_memm with the predictor stub: per-patch label-value counts and both histograms
    equal the reference's bin for bin -- zarr (vector seabed, holey mask, shallow), memm (deep, shallow), eval_mode all /
    region / trace, chunk sizes from the whole survey down to chunks narrower than a patch."""
    from crimac_classifiers_unet_amd import tiled_inference as ti
    fix = load(golden_dir)
    pw, ph, overlap = (int(v) for v in fix["patch"])
    pipe = make_pipe(precision)
    fn = stub_predict_fn(pipe.model.infer_engine)
    values = fix["label_values"].tolist()
    for case in CASES:
        reader = make_reader(fix, case)
        centres = [tuple(int(v) for v in c) for c in fix[f"{case}/centres"]]
        for mode in MODES:
            ghp, ghn = golden_hist(fix, case, mode)
            want = {}
            for c, row in zip(centres, fix[f"{case}/{mode}/counts"].tolist()):
                want.setdefault(c, []).append(row)       # (a shallow echogram's grid holds every centre twice)
            preloads = (None,) if case.startswith("memm") else ((0, 200, 97, 32) if mode == "all" else (0, 97))
            for preload in preloads:
                counts = Counts(values)
                if preload is None:
                    hp, hn = ti.evaluate_echogram_memm(reader, pipe, (pw, ph), overlap, 8, eval_mode=mode, predict_fn=fn,
                                                       on_batch=counts)
                else:
                    hp, hn = ti.evaluate_survey(reader, pipe, (pw, ph), overlap, 8, preload, eval_mode=mode,
                                                predict_fn=fn, on_batch=counts)
                got = {}
                for c, row in counts.rows:
                    got.setdefault(c, []).append(row)
                assert got == want, (case, mode, preload)
                assert np.array_equal(hp, ghp) and np.array_equal(hn, ghn), (case, mode, preload,
                                                                            int(np.abs(hp - ghp).sum()), int(np.abs(hn - ghn).sum()))
    ti.release_staging()


# ---- 6. real network against the DataLoader-fed path -----------------------------------------------------------------------
def raw_batches(fix, case, batch_size):
    """RAW crops of the fake zarr reader as the reference's gridded Dataset (label / data transform functions None) hands
    them: get_crop_zarr's data (nan_to_num, here in float32), raw annotation ids, centre coordinates."""
    n_pings, n_range, seed = (int(v) for v in fix[f"{case}/shape"])
    sv, labels, _, _ = synth_eval_survey(n_pings, n_range, seed)
    sv_hw, lab_hw = np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T)
    pw, ph, _ = (int(v) for v in fix["patch"])
    centres = fix[f"{case}/centres"]
    out = []
    for b0 in range(0, len(centres), batch_size):
        cs = centres[b0:b0 + batch_size]
        out.append({"data": torch.from_numpy(np.stack([np.nan_to_num(torc.crop(sv_hw, c, (ph, pw), 0).astype(np.float32),
                                                                    nan=0.0) for c in cs])),
                    "labels": torch.from_numpy(np.stack([torc.crop(lab_hw, c, (ph, pw), -100).astype(np.int16) for c in cs])),
                    "center_coordinates": torch.from_numpy(np.asarray(cs, dtype=np.int64))})
    return out


def moved_share(a, b):
    (hp0, hn0), (hp1, hn1) = a, b
    moved = np.abs(np.cumsum(hp0) - np.cumsum(hp1)).sum() + np.abs(np.cumsum(hn0) - np.cumsum(hn1)).sum()
    return moved / max(hp0.sum() + hn0.sum(), 1)


def max_f1(pipe, h):
    return float(pipe.compute_evaluation_metrics_from_histograms(h[0], h[1])["F1"].max())


def segpipe(**over):
    import yaml
    import crimac_classifiers_unet_amd as pkg
    from crimac_classifiers_unet_amd import synth
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg.update(save_model_params=False, data_mode="zarr", gpu_metrics=True)
    cfg.update(over)
    pipe = pkg.SegPipeUNet(experiment_name="t", **cfg)
    pipe.model.load_state_dict(synth.synth_state_dict(seed=0))
    pipe.model.to(pipe.device).eval()
    pipe.model_is_loaded = True
    return pipe


@pytest.mark.parametrize("mode", ["all", "region"])
def test_real_network_against_the_dataloader_fed_path(golden_dir, mode, tmp_path):
    """evaluate_survey (h3p inference, synthetic weights) against use_gpu_test_transform + the gpu_metrics histograms fed
    RAW crops of the same reader: the totals of hist_pos and hist_neg are equal exactly (same pixels, same labels); bins
    may differ through batch composition only.

    Measured on an MI355X: the DataLoader-fed path against itself at batch sizes 8 and 32 moves a share of
    SELF_MOVED_SHARE of the valid pixels to another float16 bin and changes max F1 by SELF_F1_DIFF (constants above; both
    0: an eval-mode forward does not depend on the batch it runs in); allowed here: twice that."""
    from crimac_classifiers_unet_amd import evaluate, tiled_inference as ti
    fix = load(golden_dir)
    pw, ph, overlap = (int(v) for v in fix["patch"])
    pipe = segpipe(eval_mode=mode)
    reader = make_reader(fix, "zarr")
    pipe.use_gpu_test_transform(reader, patch_overlap=overlap)
    ref = {b: pipe.get_pr_histograms_dataloader(raw_batches(fix, "zarr", b))[:2] for b in (8, 32)}
    pipe.use_gpu_test_transform(None)
    self_moved, self_f1 = moved_share(ref[8], ref[32]), abs(max_f1(pipe, ref[8]) - max_f1(pipe, ref[32]))
    print(f"DataLoader path, batch 8 vs 32 ({mode}): moved share {self_moved:.3e}, max-F1 difference {self_f1:.3e}")
    assert ref[8][0].sum() == ref[32][0].sum() and ref[8][1].sum() == ref[32][1].sum()
    for preload in (0, 97):
        got = ti.evaluate_survey(reader, pipe, (pw, ph), overlap, 8, preload, eval_mode=mode)
        moved, f1d = moved_share(ref[8], got), abs(max_f1(pipe, ref[8]) - max_f1(pipe, got))
        print(f"tiled (preload {preload}) vs DataLoader path: moved share {moved:.3e}, max-F1 difference {f1d:.3e}")
        assert got[0].sum() == ref[8][0].sum() and got[1].sum() == ref[8][1].sum()
        assert got[0].sum() > 100 and got[1].sum() > 10000
        assert moved <= 2 * SELF_MOVED_SHARE, moved
        assert f1d <= 2 * SELF_F1_DIFF, f1d
    # the public function: same histograms -> same metrics, csv written through the shared tail
    m = evaluate.validate_model_survey_zarr([reader], pipe, {}, (pw, ph), overlap, mode, 8, 0, str(tmp_path), None,
                                            preload_n_pings=97, survey="s", tiled=True)
    assert np.array_equal(m["F1"], pipe.compute_evaluation_metrics_from_histograms(*got)["F1"])
    assert os.path.exists(tmp_path / "s_test.csv")
    ti.release_staging()


# ---- 7. two ranks ----------------------------------------------------------------------------------------------------------
def _eval_rank_worker(rank, world, port, golden_dir, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", CRIMAC_DIST_BACKEND="gloo")
    from crimac_classifiers_unet_amd import evaluate, parallel, tiled_inference as ti
    parallel.init_distributed(backend="gloo")          # two ranks share the one GPU of the box: gloo, not RCCL
    fix = load(golden_dir)
    pw, ph, overlap = (int(v) for v in fix["patch"])
    pipe = make_pipe("f32x6")
    fn = stub_predict_fn(pipe.model.infer_engine)
    stats = {}
    out[f"zarr{rank}"] = ti.evaluate_survey(make_reader(fix, "zarr"), pipe, (pw, ph), overlap, 8, 97, predict_fn=fn, stats=stats)
    out[f"patches{rank}"] = stats["patches"]
    out[f"net{rank}"] = ti.evaluate_survey(make_reader(fix, "zarr"), pipe, (pw, ph), overlap, 8, 97)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_merge_to_the_single_rank_histograms(golden_dir):
    """Chunks dealt to two gloo ranks on one GPU, histograms all-reduced once: every rank returns the survey's histograms,
    equal to the single-rank ones exactly (stub: the reference's; real network: the single-process run's -- a chunk is
    evaluated by one rank in the same batches whoever owns it)."""
    import socket
    import torch.multiprocessing as mp
    from crimac_classifiers_unet_amd import tiled_inference as ti
    fix = load(golden_dir)
    pw, ph, overlap = (int(v) for v in fix["patch"])
    pipe = make_pipe("f32x6")
    single = ti.evaluate_survey(make_reader(fix, "zarr"), pipe, (pw, ph), overlap, 8, 97)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        procs = [ctx.Process(target=_eval_rank_worker, args=(r, 2, port, golden_dir, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
        res = dict(out)
    ghp, ghn = golden_hist(fix, "zarr", "all")
    assert res["patches0"] > 0 and res["patches1"] > 0 and res["patches0"] + res["patches1"] == len(fix["zarr/centres"])
    for r in range(2):
        assert np.array_equal(res[f"zarr{r}"][0], ghp) and np.array_equal(res[f"zarr{r}"][1], ghn)
        assert np.array_equal(res[f"net{r}"][0], single[0]) and np.array_equal(res[f"net{r}"][1], single[1])
    ti.release_staging()


# ---- 8. metadata models on the memm flavour ----------------------------------------------------------------------------------
def meta_echogram(fix):
    eg = make_reader(fix, "memm")
    n = eg.shape[1]
    rng = np.random.Generator(np.random.PCG64(9))
    tv = 737000.5 + np.cumsum(rng.uniform(5e-6, 9e-6, size=n))
    eg.portion_of_day_vector = tv % 1
    eg.portion_of_year_scalar = 0.61
    eg.time_vector_diff = np.concatenate((np.diff(tv), [tv[-1] - tv[-2]])) / 6e-6 - 1
    return eg


class Probs:
    """on_batch hook: sandeel probability of every pixel the scatter rule of predict_echogram_memm writes, by data
    coordinate (the interiors of the grid's patches are disjoint)."""

    def __init__(self, shape):
        self.p = np.full(shape, np.nan, dtype=np.float32)

    def __call__(self, centres, labels, logits):
        lab = labels.cpu().numpy()
        sm = torch.softmax(logits, 1)[:, 1].cpu().numpy()
        H, W = lab.shape[1:]
        for c, l, s in zip(centres, lab, sm):
            yl, xl = np.nonzero(~np.isin(l, (-70, -50, -100)))           # fill_out_array's rule (save_predict.py:41-65)
            self.p[yl + c[0] - H // 2 + 1, xl + c[1] - W // 2 + 1] = s[yl, xl]


@pytest.mark.parametrize("kind", ["late", "early"])
def test_metadata_models_on_the_memm_flavour(golden_dir, kind, monkeypatch):
    """A late-injection and a metadata-input model through evaluate_echogram_memm: the histograms' totals equal the stub
    run's (the reference's: same pixels, same labels), and the sandeel probabilities agree with predict_echogram_memm's
    where that writes them.  predict_echogram_memm returns float16-rounded probabilities (half an ulp below 1: 2^-12 of
    the value, at most 2.44e-4); on top of that twice SELF_PROB_DIFF, the largest difference the flow shows against itself
    with internal batches of 8 and of 32 patches (measured on an MI355X, constant above)."""
    import crimac_classifiers_unet_amd as pkg
    from crimac_classifiers_unet_amd import synth, tiled_inference as ti
    fix = load(golden_dir)
    pw, ph, overlap = (int(v) for v in fix["patch"])
    mc = {k: True for k in torc.META_KEYS}
    if kind == "late":
        model = pkg.UNet_LateMetInject(3, 4, 7, precision="h3p")
        model.load_state_dict(synth.synth_state_dict(seed=3, meta_in_channels=7))
    else:
        model = pkg.UNet_Baseline(3, 11, precision="h3p")
        model.load_state_dict(synth.synth_state_dict(seed=3, in_channels=11))
    pipe = make_pipe(model=model)
    eg = meta_echogram(fix)
    ghp, ghn = golden_hist(fix, "memm", "all")
    runs = {}
    for ib in (8, 32, None):
        if ib is not None:
            monkeypatch.setattr(ti, "INTERNAL_BATCH", ib)
        else:
            monkeypatch.undo()
        probs = Probs(eg.shape)
        hp, hn = ti.evaluate_echogram_memm(eg, pipe, (pw, ph), overlap, 4, meta_channels=mc, on_batch=probs)
        assert hp.sum() == ghp.sum() and hn.sum() == ghn.sum(), (kind, ib)
        runs[ib] = probs.p
    assert np.array_equal(np.isnan(runs[8]), np.isnan(runs[32]))
    self_diff = float(np.nanmax(np.abs(runs[8] - runs[32])))
    print(f"{kind}: evaluate_echogram_memm, internal batch 8 vs 32: largest probability difference {self_diff:.3e}")
    out = ti.predict_echogram_memm(eg, pipe, (pw, ph), overlap, 4, meta_channels=mc)[0]
    written = ~np.isnan(runs[None])
    assert written.sum() > 10000 and not (out[~written] != 0).any()
    diff = float(np.abs(out[written] - runs[None][written]).max())
    print(f"{kind}: against predict_echogram_memm: largest probability difference {diff:.3e}")
    assert diff <= 2.0 ** -12 + 2 * SELF_PROB_DIFF, diff
    with pytest.raises(NotImplementedError):
        ti.evaluate_survey(make_reader(fix, "zarr"), pipe, (pw, ph), overlap, 4, 0)


# ---- 9. NaN weights ----------------------------------------------------------------------------------------------------------
def test_nan_weights_raise_the_dataloader_paths_error(golden_dir):
    from crimac_classifiers_unet_amd import tiled_inference as ti
    fix = load(golden_dir)
    pw, ph, overlap = (int(v) for v in fix["patch"])
    pipe = make_pipe("h3p")
    with torch.no_grad():
        pipe.model.conv_final.weight.fill_(float("nan"))
    with pytest.raises(ValueError, match="Input contains NaN"):
        ti.evaluate_survey(make_reader(fix, "zarr"), pipe, (pw, ph), overlap, 8, 0)
    with pytest.raises(ValueError, match="Input contains NaN"):
        ti.evaluate_echogram_memm(make_reader(fix, "memm"), pipe, (pw, ph), overlap, 8)
    ti.release_staging()
