"""Early metadata injection on the GPU data paths: metadata planes as extra INPUT channels of UNet_Baseline (the
reference's default late_meta_inject: False; the Dataset hands np.concatenate((data, meta)), batch/dataset.py:109).

  * crimac_augment_db_meta_nhwc: noise / NaN rule / scaled dB on the frequency planes exactly as crimac_augment_db_nhwc,
    the flip on everything, the metadata planes otherwise untouched (add_noise_metadata / flip_x_axis_metadata);
  * the training step and SegPipeUNet(gpu_augment=True, gpu_meta_input=True) against the oracles;
  * in-training validation from raw crops (use_gpu_test_transform);
  * crimac_gather_patches_memm_meta through ChunkPredictor / predict_echogram_memm against the reference golden
    (tools/make_golden_early_meta.py) and against the same network fed per-crop oracle inputs;
  * the refusals of the paths that cannot build the metadata planes."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import synth  # noqa: E402
from crimac_classifiers_unet_amd import tiled_inference as ti  # noqa: E402
from crimac_classifiers_unet_amd.hip import call, ptr  # noqa: E402
from oracle import augment_oracle as aorc  # noqa: E402
from oracle import tiling_oracle as torc  # noqa: E402
from oracle import unet_oracle as orc  # noqa: E402
from test_early_meta_cpu import PATCH, OVERLAP, early_meta_case, oracle_inputs, predictor  # noqa: E402
from tools.fake_reader import FakeEchogram, FakeZarrReader, synth_survey  # noqa: E402

NF, CM, HW = 4, 7, 64
PRECISIONS = ["bf16", "fp16", "f32x6", "h3p"]
ALL_META = {k: True for k in torc.META_KEYS}


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def decode(x, precision):
    """NHWC activations [N, 16] of the engine's storage type -> float32 values (h3p: fp16 plane pairs, 8-channel groups
    of [8 x hi][8 x lo])."""
    if precision == "h3p":
        h = x.contiguous().view(torch.float16).reshape(-1, 2, 2, 8).float()
        return (h[:, :, 0] + h[:, :, 1]).reshape(-1, 16)
    return x.float()


def to_storage(t, precision):
    """fp32 values rounded once to the storage type, as float32."""
    if precision == "bf16":
        return t.bfloat16().float()
    if precision == "fp16":
        return t.half().float()
    if precision == "h3p":
        h = t.half().float()
        return h + (t - h).half().float()
    return t


def raw_batch(B=2, seed=1):
    x_lin = torch.pow(10.0, torch.from_numpy(synth.synth_echogram_batch(B, NF, HW, HW, seed=seed)) / 10.0)
    meta = torch.from_numpy(synth.synth_metadata(B, CM, HW, HW, seed=seed + 2))
    lab = torch.from_numpy(synth.synth_labels(B, HW, HW, seed=seed + 1))
    return x_lin, meta, lab


def _aug(eng, data, labels, seed, n_data=None, aux=False):
    """One launch of the old (n_data None) or the new augment entry into fresh buffers: (x, labels, aux)."""
    B, C, H, W = data.shape
    x = torch.zeros((B * H * W, 16), dtype=eng.act_dtype, device="cuda")
    lab = torch.zeros((B, H, W), dtype=torch.int16, device="cuda")
    am = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda") if aux else None
    args = (eng.prec, ptr(data), ptr(labels), labels.element_size(), ptr(x), ptr(lab), ptr(am), NF - 1, 1e-7, 1e-4,
            B, C, H, W, 16, seed, 1, 1, 1)
    if n_data is None:
        call("crimac_augment_db_nhwc", *args)
    else:
        call("crimac_augment_db_meta_nhwc", *args, n_data)
    torch.cuda.synchronize()
    return x, lab, am


def _flip_seed(x_lin, lab):
    for seed in range(40, 80):            # a seed under which one sample is flipped and the other is not
        _, _, noisy, flipped = aorc.augment_db(x_lin.numpy(), lab.numpy(), seed)
        if flipped[0] != flipped[1] and noisy.any():
            return seed
    raise AssertionError("no seed flips exactly one sample")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_augment_meta_entry_splits_data_and_metadata_planes(precision):
    x_lin, meta, lab = raw_batch()
    x_lin[0, 0, 5, 7] = float("nan")          # a data NaN: label rule / aux bit 1
    x_lin[1, 2, 9, 3] = float("inf")
    meta[0, 3, 11, 13] = float("nan")         # a metadata NaN passes through as it is
    seed = _flip_seed(x_lin, lab)
    m = pkg.UNet_Baseline(3, NF + CM, precision=precision).cuda()
    eng = m.engine
    eng.bind()
    both = torch.cat((x_lin, meta), 1).cuda().contiguous()
    data = x_lin.cuda().contiguous()
    labels = lab.cuda()
    for aux in (False, True):
        xn, ln, an = _aug(eng, both, labels, seed, n_data=NF, aux=aux)
        xo, lo, ao = _aug(eng, data, labels, seed, aux=aux)
        dn, do = decode(xn, precision), decode(xo, precision)
        assert torch.equal(dn[:, :NF], do[:, :NF])                       # same draws, same transform
        assert torch.equal(ln, lo) and (an is None or torch.equal(an, ao))
        assert (an is None or bool((an & 2).any())) and bool((ln == -100).any())
        assert bool((dn[:, NF + CM:] == 0).all())
        flipped = torch.empty_like(meta).cuda()
        call("crimac_augment_flip_planes", ptr(meta.cuda().contiguous()), ptr(flipped), 2, CM, HW, HW, seed, 1)
        torch.cuda.synchronize()
        want = to_storage(flipped.permute(0, 2, 3, 1).reshape(-1, CM), precision)
        torch.testing.assert_close(dn[:, NF:NF + CM], want, rtol=0, atol=0, equal_nan=True)
    # the metadata planes did take the flip of their sample (the seed flips exactly one of the two)
    _, _, _, fl = aorc.augment_db(x_lin.numpy(), lab.numpy(), seed)
    b = int(np.argmax(fl))
    torch.testing.assert_close(flipped[b].cpu(), meta[b].flip(-1), rtol=0, atol=0, equal_nan=True)
    # n_data == C: the old entry, byte for byte
    x4, l4, a4 = _aug(eng, data, labels, seed, n_data=NF, aux=True)          # (xo, lo, ao: the aux=True launch above)
    assert torch.equal(x4.view(torch.uint8), xo.view(torch.uint8)) and torch.equal(l4, lo) and torch.equal(a4, ao)
    # the label facts read data channels only
    with pytest.raises(Exception, match="threshold channel"):
        eng.augment_batch(both, labels, seed, refine_labels=(NF, 1e-7, 1e-4), n_data=NF)


@pytest.mark.gpu
def test_training_step_and_pipeline_with_metadata_input_channels():
    x_lin, meta, lab = raw_batch()
    seed = _flip_seed(x_lin, lab)
    sd = synth.synth_state_dict(seed=0, in_channels=NF + CM)
    xa, la, noisy, flipped = aorc.augment_db(x_lin.numpy(), lab.numpy(), seed, scaled=True)
    meta_a = torch.stack([meta[b].flip(-1) if flipped[b] else meta[b] for b in range(2)])
    ref_loss, _, ref_grads, _ = orc.loss_and_grads(sd, torch.cat((torch.from_numpy(xa), meta_a), 1),
                                                   torch.from_numpy(la))
    m = pkg.UNet_Baseline(3, NF + CM, precision="f32x6")
    m.load_state_dict(sd)
    m.cuda().train()
    eng = m.engine
    cw = torch.tensor([10.0, 300.0, 250.0], device="cuda")
    both = torch.cat((x_lin, meta), 1)
    loss = eng.train_step_augmented(both.cuda(), lab.cuda(), cw, lr=0.0, momentum=0.0, seed=seed, n_data=NF)
    assert abs(float(loss) - float(ref_loss)) < 1e-4 * abs(float(ref_loss))
    for k in ("down_convs.0.main.0.weight", "conv_final.weight", "down_convs.4.main.3.weight"):
        e = float((eng.G[k].double().cpu() - ref_grads[k].double()).norm() / ref_grads[k].double().norm())
        assert e < 2e-2, (k, e)
    with pytest.raises(ValueError, match="input channels"):
        eng.train_step_augmented(x_lin.cuda(), lab.cuda(), cw, lr=0.0, momentum=0.0, seed=seed, n_data=NF)
    with pytest.raises(ValueError):
        eng.train_step_augmented(both.cuda(), lab.cuda(), cw, lr=0.0, momentum=0.0, seed=seed, n_data=NF,
                                 meta=meta.cuda())
    # through the pipeline: the batch dict carries data | metadata planes, the yaml opts in with gpu_meta_input
    import yaml
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg.update(save_model_params=False, late_meta_inject=False, precision="f32x6", gpu_augment=True,
               gpu_meta_input=True, lr=0.0, log_step=10 ** 9, lr_step=10 ** 9, random_seed=0, meta_channels=ALL_META)
    pipe = pkg.SegPipeUNet(experiment_name="t", **{k: v for k, v in cfg.items() if k != "experiment_name"})
    pipe.model.load_state_dict(sd)
    pipe.train_model([{"data": both, "labels": lab}], [], None)
    xa0, la0, _, fl0 = aorc.augment_db(x_lin.numpy(), lab.numpy(), 0, scaled=True)       # seed of step 0, rank 0
    m0 = torch.stack([meta[b].flip(-1) if fl0[b] else meta[b] for b in range(2)])
    l0, _, _, _ = orc.loss_and_grads(sd, torch.cat((torch.from_numpy(xa0), m0), 1), torch.from_numpy(la0))
    s = pipe.model.engine.last_loss_sums.cpu()
    assert abs(float(s[0] / s[1]) - float(l0)) < 1e-4 * abs(float(l0))


@pytest.mark.gpu
def test_validation_from_raw_crops_with_metadata_input_channels():
    """use_gpu_test_transform on an early-injection pipeline: labels = the reference's test-time label transform of the
    frequency planes, logits = the network on [db_with_limits_scaled(data) | metadata planes]."""
    import yaml
    from oracle import labels_oracle as lorc
    sv, labels, seabed = synth_survey(n_pings=400, n_range=240, seed=5)
    reader = FakeZarrReader(sv, labels, seabed)
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg.update(save_model_params=False, data_mode="zarr", late_meta_inject=False, meta_channels=ALL_META,
               precision="f32x6", infer_precision="f32x6")
    pipe = pkg.SegPipeUNet(experiment_name="t", **{k: v for k, v in cfg.items() if k != "experiment_name"})
    pipe.model.load_state_dict(synth.synth_state_dict(seed=4, in_channels=NF + CM))
    pipe.model.to(pipe.device)
    size, centres = 96, [(120, 60), (180, 300)]
    lin = np.stack([torc.crop(np.ascontiguousarray(sv.transpose(0, 2, 1)), c, (size, size), 0) for c in centres])
    lin = lin.astype(np.float32)
    raw_lab = np.stack([torc.crop(np.ascontiguousarray(labels.T), c, (size, size), -100) for c in centres])
    meta = synth.synth_metadata(2, CM, size, size, seed=8)
    batch = {"data": torch.from_numpy(np.concatenate((lin, meta), 1)),
             "labels": torch.from_numpy(raw_lab.astype(np.int16)), "center_coordinates": torch.tensor(centres)}
    pipe.use_gpu_test_transform(reader, patch_overlap=20)
    logits, lab = pipe._predict_raw_batch(batch)
    want_lab = np.stack([lorc.test_label_transform(lin[b], raw_lab[b].astype(np.int64), centres[b], NF - 1, seabed,
                                                   sv.shape[2], 20) for b in range(2)])
    assert np.array_equal(lab.cpu().numpy(), want_lab) and (want_lab == -100).any()
    db = np.stack([torc.data_transform(x)[0] for x in lin])
    host = {"data": torch.from_numpy(np.concatenate(((1 + db / np.float32(75)).astype(np.float32), meta), 1))}
    assert rel(logits, pipe.predict_batch(host)) < 1e-5
    pipe.use_gpu_test_transform(None)


def _meta_source(eg, mc):
    return ti.MetaSource(mc, eg.portion_of_year_scalar, eg.portion_of_day_vector, eg.time_vector_diff, eg._seabed, "cuda")


def _golden_echogram(fix, tag):
    sv_hw, labels_hw, seabed, mc, py, pd, td = early_meta_case(fix, tag)
    eg = FakeEchogram(sv_hw, labels_hw, seabed)
    eg.portion_of_year_scalar, eg.portion_of_day_vector, eg.time_vector_diff = py, pd, td
    return eg, mc


@pytest.fixture(scope="module")
def fix(golden_dir):
    return np.load(os.path.join(golden_dir, "early_meta.npz"))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["all", "subset"])
def test_gather_with_metadata_planes_reproduces_reference_golden(fix, tag):
    """ChunkPredictor with an early-injection model: crimac_gather_patches_memm_meta builds [scaled dB | metadata planes]
    per crop; the golden's stand-in predictor applied to that NHWC input reproduces the reference's output array."""
    eg, mc = _golden_echogram(fix, tag)
    n_planes = sum(2 if k == "portion_day" else 1 for k in torc.META_KEYS if mc[k])
    K = NF + n_planes
    model = pkg.UNet_Baseline(3, K, precision="f32x6").cuda().eval()
    w = torch.from_numpy(fix["weights"][:, :K]).cuda()
    refs = {tuple(c): x for c, x, _ in oracle_inputs(*early_meta_case(fix, tag))}
    seen = []

    def predict_fn(x, P, H, W):
        v = x.float().reshape(P, H, W, 16)
        assert bool((v[..., K:] == 0).all())
        seen.append(v[..., :K].permute(0, 3, 1, 2).cpu().numpy())
        return torch.softmax(torch.einsum("phwc,oc->pohw", v[..., :K], w), 1).contiguous()

    pipe = types.SimpleNamespace(model=model, device=torch.device("cuda"), frequencies=[18, 38, 120, 200])
    out = ti.predict_echogram_memm(eg, pipe, PATCH, OVERLAP, 4, predict_fn=predict_fn, meta_channels=mc)
    ref = fix[f"{tag}/out_f16"].astype(np.float64)
    assert np.array_equal(out != 0, ref != 0) and (ref != 0).any()
    assert np.abs(out - ref).max() <= 1e-3                      # float16-rounded probabilities
    # the gathered input itself, crop by crop, against the oracle: data planes to the dB transform's last bits,
    # metadata planes exact but for sin / cos of the time of day (device libm vs numpy)
    got = np.concatenate(seen)
    trig = [NF + 1, NF + 2] if mc["portion_day"] else []
    for p, c in enumerate(fix[f"{tag}/centres"]):
        want = refs[tuple(c)]
        assert np.abs(got[p, :NF] - want[:NF]).max() <= 1e-6
        for k in range(NF, K):
            if k in trig:
                assert np.abs(got[p, k] - want[k]).max() <= 1.2e-7
            else:
                assert np.array_equal(got[p, k], want[k]), (p, k)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32x6", "h3p"])
def test_early_injection_model_through_tiled_inference(fix, precision):
    """predict_echogram_memm with a real early-injection UNet_Baseline(3, 11): equal to feeding the SAME network the
    oracle's per-crop inputs and scattering with the oracle's fill_out_array."""
    eg, mc = _golden_echogram(fix, "all")
    model = pkg.UNet_Baseline(3, NF + CM, precision=precision)
    model.load_state_dict(synth.synth_state_dict(seed=3, in_channels=NF + CM))
    model.cuda().eval()
    pipe = types.SimpleNamespace(model=model, device=torch.device("cuda"), frequencies=[18, 38, 120, 200])
    out = ti.predict_echogram_memm(eg, pipe, PATCH, OVERLAP, 4, meta_channels=mc)
    ref = np.zeros(out.shape)
    for c, x, lab in oracle_inputs(*early_meta_case(fix, "all")):
        with torch.no_grad():
            sm = torch.softmax(model(torch.from_numpy(x[None]).cuda()), 1)[0].cpu().numpy()
        torc.fill_out_array(ref, sm.astype(np.float16), lab, c, 0)
    assert np.array_equal(out != 0, ref != 0) and (out != 0).any()
    assert np.abs(out - ref).max() <= 2e-3                      # float16-rounded probabilities


@pytest.mark.gpu
def test_paths_without_the_metadata_planes_refuse_an_early_injection_model(fix):
    eg, mc = _golden_echogram(fix, "all")
    model = pkg.UNet_Baseline(3, NF + CM, precision="f32x6").cuda().eval()
    pipe = types.SimpleNamespace(model=model, device=torch.device("cuda"), frequencies=[18, 38, 120, 200])
    with pytest.raises(ValueError, match="meta_channels"):
        ti.predict_echogram_memm(eg, pipe, PATCH, OVERLAP, 4)
    data = np.stack([m.T for m in eg.data_memmaps()]).astype(np.float32)        # [C, pings, range]
    n_range, n_pings = eg.shape
    grid = ti.plan_grid(n_range, int(eg._seabed.max()), 0, n_pings)
    cp = ti.ChunkPredictor(model, n_range, PATCH, OVERLAP, 4, out_f16=True)
    cp.load_chunk(data, 0, eg.labels.T, None, 0, n_pings, seabed=eg._seabed, flavour="memm")
    with pytest.raises(ValueError, match="meta_source"):
        cp.predict(grid)
    cp.meta_source = _meta_source(eg, dict(ALL_META, portion_day=False))          # 5 planes for a 7-plane model
    with pytest.raises(ValueError, match="metadata input channels"):
        cp.predict(grid)
    sv, labels, seabed = synth_survey(n_pings=300, n_range=200, seed=6)
    with pytest.raises(NotImplementedError, match="metadata"):
        next(ti.predict_survey(FakeZarrReader(sv, labels, seabed), pipe, PATCH, OVERLAP, 4, 1000))
