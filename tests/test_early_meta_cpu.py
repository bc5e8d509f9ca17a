"""Early metadata injection (metadata planes as extra INPUT channels of UNet_Baseline, the reference's default
late_meta_inject: False, pipeline.py:388-397), CPU side: the oracle composition of the memm prediction path against the
reference's own Dataset + transforms + fill_out_array (tools/make_golden_early_meta.py), and the pipeline's yaml surface."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import tiling_oracle as orc  # noqa: E402
from tools.fake_reader import synth_survey  # noqa: E402

PATCH, OVERLAP = (256, 256), 20


@pytest.fixture(scope="module")
def fix(golden_dir):
    return np.load(os.path.join(golden_dir, "early_meta.npz"))


def early_meta_case(fix, tag):
    """(sv_hw, labels_hw, seabed, meta_channels, portion_year, portion_day, time_diff) of a golden echogram."""
    n_pings, n_range, seed, sb_max = (int(v) for v in fix[f"{tag}/shape"])
    sv, labels, seabed = synth_survey(n_pings=n_pings, n_range=n_range, seed=seed)
    mc = {k: bool(v) for k, v in zip(orc.META_KEYS, fix[f"{tag}/meta_channels"])}
    return (np.ascontiguousarray(sv.swapaxes(1, 2)), np.ascontiguousarray(labels.T), np.clip(seabed, 40, sb_max), mc,
            float(fix[f"{tag}/portion_year"]), fix[f"{tag}/portion_day"], fix[f"{tag}/time_diff"])


def predictor(weights):
    """The golden's stand-in network: softmax over 3 fixed linear maps of ALL input channels (data + metadata)."""
    def f(x):
        z = np.tensordot(weights[:, :x.shape[0]], x.astype(np.float32), axes=(1, 0))
        z = z - z.max(0, keepdims=True)
        e = np.exp(z)
        return (e / e.sum(0, keepdims=True)).astype(np.float32)
    return f


def oracle_inputs(sv_hw, labels_hw, seabed, mc, py, pd, td):
    """Per crop of save_reader_predictions_memm's grid: (centre, input [4 + Cm, H, W] float32, transformed labels).
    Data planes: crop, remove_nan_inf, db_with_limits_scaled (1 + dB / 75), set_data_border_value; then the metadata
    planes of get_crop_memmap, untouched by the data transform (batch/dataset.py:241)."""
    n_range, n_pings = sv_hw.shape[1:]
    grid = orc.get_data_grid(n_range, int(np.max(seabed)), 0, n_pings, PATCH, OVERLAP)
    for c in grid:
        c = np.array(c)
        if n_range <= PATCH[0]:
            c[0] = n_range // 2
        d = orc.crop(sv_hw, c, PATCH, 0)
        d = np.where(np.isfinite(d), d, d.dtype.type(0))
        lab = orc.patch_labels(labels_hw, {"local": tuple(c), "global": tuple(c)}, PATCH, seabed, n_range, OVERLAP, None,
                               seabed_rule="memm")
        db, _ = orc.data_transform(d)
        db = (np.float32(1) + db / np.float32(75)).astype(np.float32)
        db[:, lab == orc.LABEL_BOUNDARY_VAL] = 0.0
        meta = orc.meta_planes(c, PATCH, mc, py, pd, td, seabed).astype(np.float32)
        yield c, np.concatenate((db, meta)), lab


@pytest.mark.parametrize("tag", ["all", "subset"])
def test_oracle_composition_matches_reference_golden(fix, tag):
    sv_hw, labels_hw, seabed, mc, py, pd, td = early_meta_case(fix, tag)
    f = predictor(fix["weights"])
    out = np.zeros([2] + list(labels_hw.shape))
    n = 0
    for c, x, lab in oracle_inputs(sv_hw, labels_hw, seabed, mc, py, pd, td):
        assert x.shape[0] == 4 + sum(2 if k == "portion_day" else 1 for k in orc.META_KEYS if mc[k])
        orc.fill_out_array(out, f(x).astype(np.float16), lab, c, 0)
        n += 1
    assert n == len(fix[f"{tag}/centres"])
    ref = fix[f"{tag}/out_f16"].astype(np.float64)
    assert np.array_equal(out != 0, ref != 0) and (ref != 0).mean() > 0.5
    assert np.abs(out - ref).max() <= 1e-3          # float16-rounded probabilities (float32 vs float64 dB upstream)


def _cfg(**kw):
    import yaml
    import crimac_classifiers_unet_amd as pkg
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg.update(save_model_params=False, late_meta_inject=False,
               meta_channels={k: True for k in orc.META_KEYS}, **kw)
    return {k: v for k, v in cfg.items() if k != "experiment_name"}


def test_gpu_meta_input_is_an_opt_in_that_needs_gpu_augment():
    import crimac_classifiers_unet_amd as pkg
    assert _cfg()["gpu_meta_input"] is False                                   # the yaml documents the key, off
    with pytest.raises(NotImplementedError, match="extra INPUT channels.*gpu_meta_input"):
        pkg.SegPipeUNet(experiment_name="t", **_cfg(gpu_augment=True))
    with pytest.raises(ValueError, match="gpu_meta_input needs gpu_augment"):
        pkg.SegPipeUNet(experiment_name="t", **_cfg(gpu_meta_input=True))
    pipe = pkg.SegPipeUNet(experiment_name="t", **_cfg(gpu_augment=True, gpu_meta_input=True))
    assert isinstance(pipe.model, pkg.UNet_Baseline) and pipe.model.in_channels == 11 and pipe.early_meta
