"""precision='h3f' (the h3p forward, the 1-MFMA fp16 backward) for UNet_LateMetInject, on the tests/golden/lmi.npz case
(reference unet.py:346-391), and the batch independence of the late-injection eval forward.

The bounds are those the same properties are held to elsewhere: the gradients against the golden take the comparison of
tests/test_lmi.py::test_late_injection_hip_path_matches_reference_golden for h3p (L2-relative error below 2e-3 per
tensor) on the median of three passes (tests/test_gpu_h3p.py::_golden_gradient_errors says why a median); the three-step
trajectory takes the 2e-3 of test_h3f_training_trajectory_and_other_shapes, against h3p's own three steps."""
import os

import numpy as np
import pytest
import torch

import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import synth

pytestmark = pytest.mark.gpu
CM, HW = 7, 64
CW = [10.0, 300.0, 250.0]
META_CFG = {"portion_year": True, "portion_day": True, "depth_rel": True, "depth_abs_surface": True,
            "depth_abs_seabed": True, "time_diff": True}


@pytest.fixture(scope="module")
def case(golden_dir):
    fix = np.load(os.path.join(golden_dir, "lmi.npz"))
    sd = synth.synth_state_dict(seed=0, meta_in_channels=CM)
    x = torch.from_numpy(synth.synth_echogram_batch(2, 4, HW, HW, seed=1)).cuda()
    meta = torch.from_numpy(synth.synth_metadata(2, CM, HW, HW, seed=3)).cuda()
    lab = torch.from_numpy(synth.synth_labels(2, HW, HW, seed=2)).cuda()
    return fix, sd, x, meta, lab


def _model(sd, precision):
    m = pkg.UNet_LateMetInject(3, 4, CM, precision=precision)
    m.load_state_dict(sd)
    return m.cuda()


def _l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def _train_passes(m, x, meta, lab, fix, repeats=3):
    """Median over `repeats` autograd passes of the L2-relative error of every gradient the golden holds, and what the
    first pass left: logits, loss, BatchNorm running statistics."""
    crit = pkg.WeightedCrossEntropy(CW).cuda()
    errs, first = {}, None
    m.train()
    for _ in range(repeats):
        for p in m.parameters():
            p.grad = None
        logits = m(x, meta)
        loss = crit(logits, lab.long())
        loss.backward()
        if first is None:
            first = (logits.detach().clone(), float(loss.detach()),
                     {k: v.detach().clone() for k, v in m.state_dict().items() if "running" in k})
        for k, p in m.named_parameters():
            if "grad/" + k in fix.files:
                errs.setdefault(k, []).append(_l2(p.grad, fix["grad/" + k]))
    return {k: sorted(v)[len(v) // 2] for k, v in errs.items()}, first


def test_h3f_forward_is_h3ps_and_every_gradient_meets_the_h3p_tolerance(case):
    fix, sd, x, meta, lab = case
    mf, mp = _model(sd, "h3f"), _model(sd, "h3p")
    mf.eval(), mp.eval()
    with torch.no_grad():
        assert torch.equal(mf(x, meta), mp(x, meta))                       # eval logits: bit for bit
        assert torch.equal(mf.predict_softmax(x, meta), mp.predict_softmax(x, meta))
    ef, (lf, lossf, runf) = _train_passes(mf, x, meta, lab, fix)
    ep, (lp, lossp, runp) = _train_passes(mp, x, meta, lab, fix)
    # h3f's train forward is h3p's: the same kernels on the same operands.  Whether two such forwards are bit-identical
    # is decided here by three further h3p models: if all agree with the first, h3f must EQUAL h3p; if not (the BatchNorm
    # statistics are summed by atomics in arrival order), h3f is held to what h3p differs from itself by: per quantity (the
    # running statistics pooled into one relative figure) TWICE the largest of the three measured h3p-h3p differences, and
    # never less than one fp32 ulp of the quantity's scale, the quantum such a difference comes in.  Why twice: h3f - h3p is
    # a fourth draw of the same noise, and a fourth draw exceeds the largest of three once in four runs; each figure is a
    # maximum over 24576 logits or ~6000 statistics and varies little between draws (2.2e-6, 2.3e-6, 2.7e-6 measured for
    # the logits), so twice the largest lies far outside that spread -- and three orders of magnitude below what another
    # forward arithmetic is allowed (tests/test_lmi.py holds the bf16 forward to 6e-2 of the largest logit).
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())      # noqa: E731
    same, noise_l, noise_loss, noise_run = True, 0.0, 0.0, 0.0
    for _ in range(3):
        _, (lq, lossq, runq) = _train_passes(_model(sd, "h3p"), x, meta, lab, fix, repeats=1)
        same = same and torch.equal(lp, lq) and lossp == lossq and all(torch.equal(runp[k], runq[k]) for k in runp)
        noise_l, noise_loss = max(noise_l, float((lp - lq).abs().max())), max(noise_loss, abs(lossp - lossq))
        noise_run = max(noise_run, max(rel(runq[k], runp[k]) for k in runp))
    print(f"h3p vs h3p train forward (3 draws): identical {same}, max |dlogit| {noise_l:.3e}, |dloss| {noise_loss:.3e}, "
          f"running statistics {noise_run:.3e}; h3f vs h3p: {float((lf - lp).abs().max()):.3e}, {abs(lossf - lossp):.3e}, "
          f"{max(rel(runf[k], runp[k]) for k in runp):.3e}")
    if same:
        assert torch.equal(lf, lp) and lossf == lossp
        for k in runp:
            assert torch.equal(runf[k], runp[k]), k
    else:
        ulp = 2.0 ** -23
        assert float((lf - lp).abs().max()) <= max(2 * noise_l, ulp * float(lp.abs().max()))
        assert abs(lossf - lossp) <= max(2 * noise_loss, ulp * abs(lossp))
        for k in runp:
            assert rel(runf[k], runp[k]) <= max(2 * noise_run, ulp), (k, rel(runf[k], runp[k]), noise_run)
    assert abs(lossf - float(fix["loss"])) < 1e-5 * abs(float(fix["loss"]))
    tol = 2e-3
    mlp_and_head = [k for k in ef if k.startswith("post_processing_weights.") or k.startswith("conv_final.")]
    assert len(mlp_and_head) == 8, mlp_and_head
    for k in ef:
        print(f"{k}: h3f / tol {ef[k] / tol:.2e}   h3p / tol {ep[k] / tol:.2e}")
    bad = [(k, ef[k]) for k in ef if not ef[k] < tol]
    assert not bad, bad
    assert mf.engine.skipped_steps() == 0


def test_three_fused_h3f_steps_track_h3p_and_an_overflowing_step_is_skipped(case):
    fix, sd, *_ = case
    B, S = 2, 32                                       # the smallest crop depth 5 allows
    x = torch.from_numpy(synth.synth_echogram_batch(B, 4, S, S, seed=21)).cuda()
    meta = torch.from_numpy(synth.synth_metadata(B, CM, S, S, seed=23)).cuda()
    lab = torch.from_numpy(synth.synth_labels(B, S, S, seed=22)).cuda()
    cw = torch.tensor(CW, device="cuda")
    losses = {}
    for prec in ("h3p", "h3f"):
        eng = _model(sd, prec).train().engine
        losses[prec] = [float(eng.train_step(x, lab, cw, lr=0.005, momentum=0.95, meta=meta)) for _ in range(3)]
        assert eng.skipped_steps() == 0
    print("h3f losses", losses["h3f"], "h3p", losses["h3p"])
    for a, b in zip(losses["h3f"], losses["h3p"]):
        assert abs(a - b) < 2e-3 * abs(b)
    m = _model(sd, "h3f").train()
    eng = m.engine
    eng.train_step(x, lab, cw, lr=0.005, momentum=0.0, meta=meta)
    # forced overflow (as tests/test_gpu_unet.py does for the baseline model)
    eng.loss_scale = 2.0 ** 40
    p0, v0 = eng.flat_p.clone(), eng.flat_v.clone()
    loss = eng.train_step(x, lab, cw, lr=0.005, momentum=0.95, meta=meta)
    assert bool(torch.isfinite(loss))
    assert torch.equal(eng.flat_p, p0) and torch.equal(eng.flat_v, v0)
    assert eng.skipped_steps() == 1
    eng.loss_scale = 2.0 ** 16
    eng.train_step(x, lab, cw, lr=0.005, momentum=0.95, meta=meta)
    assert eng.skipped_steps() == 1 and not torch.equal(eng.flat_p, p0) and bool(torch.isfinite(eng.flat_p).all())


def test_train_step_augmented_takes_the_metadata_in_h3f(case):
    fix, sd, x, meta, lab = case
    x_lin = torch.pow(10.0, x / 10.0)
    cw = torch.tensor(CW, device="cuda")
    seed = 41
    got = {}
    for prec in ("h3p", "h3f"):
        eng = _model(sd, prec).train().engine
        xa, la = eng.augment_batch(x_lin, lab, seed, db_scaled=True)
        flipped = eng.flip_planes(meta, seed)
        loss = eng.train_step_augmented(x_lin, lab, cw, lr=0.0, momentum=0.0, seed=seed, meta=meta)
        got[prec] = (xa.clone(), la.clone(), flipped.clone(), float(loss))
        assert eng.skipped_steps() == 0
    assert got["h3f"][0].dtype == got["h3p"][0].dtype
    assert torch.equal(got["h3f"][0].view(torch.int32), got["h3p"][0].view(torch.int32))      # the same augmented input
    assert torch.equal(got["h3f"][1], got["h3p"][1]) and torch.equal(got["h3f"][2], got["h3p"][2])
    assert abs(got["h3f"][3] - got["h3p"][3]) <= 1e-6 * abs(got["h3p"][3])


def test_pipeline_trains_and_predicts_the_late_injection_model_in_h3f(case):
    import yaml
    fix, sd, x, meta, lab = case
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg.update(save_model_params=False, late_meta_inject=True, precision="h3f", log_step=10 ** 9, lr_step=10 ** 9,
               random_seed=0, meta_channels=META_CFG)
    pipe = pkg.SegPipeUNet(experiment_name="t", **{k: v for k, v in cfg.items() if k != "experiment_name"})
    assert isinstance(pipe.model, pkg.UNet_LateMetInject) and pipe.model.engine.bwd16
    pipe.model.load_state_dict(sd)
    small = slice(0, 32)
    batches = [{"data": torch.cat((x, meta), dim=1)[:, :, small, small].cpu().double().roll(i, 0),
                "labels": lab[:, small, small].cpu().roll(i, 0)} for i in range(2)]
    pipe.train_model(batches, [], None)
    s = pipe.model.engine.last_loss_sums.cpu()
    assert bool(torch.isfinite(s).all()) and float(s[1]) > 0
    out = pipe.predict_batch(batches[0])
    assert tuple(out.shape) == (2, 3, 32, 32) and bool(torch.isfinite(torch.as_tensor(out)).all())


def test_the_eval_forward_of_a_patch_does_not_depend_on_its_batch(case):
    fix, sd, *_ = case
    m = _model(sd, "h3p").eval()
    x = torch.from_numpy(synth.synth_echogram_batch(16, 4, 32, 32, seed=31)).cuda()
    meta = torch.from_numpy(synth.synth_metadata(16, CM, 32, 32, seed=33)).cuda()
    with torch.no_grad():
        whole = m(x, meta).clone()
        for i in (0, 9):
            alone = m(x[i:i + 1].contiguous(), meta[i:i + 1].contiguous())
            assert torch.equal(alone[0], whole[i]), f"patch {i}: {int((alone[0] != whole[i]).sum())} logits differ"
        # 256 x 256, one patch against seventeen
        x = torch.from_numpy(synth.synth_echogram_batch(17, 4, 256, 256, seed=35)).cuda()
        meta = torch.from_numpy(synth.synth_metadata(17, CM, 256, 256, seed=37)).cuda()
        whole = m(x, meta)[11].clone()
        alone = m(x[11:12].contiguous(), meta[11:12].contiguous())[0]
    n = int((alone != whole).sum())
    print(f"256 x 256, 1 patch against 17: {n} of {whole.numel()} logits differ, max |diff| "
          f"{float((alone - whole).abs().max()):.3e}")
    assert n == 0
