"""CPU: the up_mode="upsample" model surface (reference unet.py:47-56, :184-188) -- state_dict keys, shapes and seeded
initialisation equal the reference's (tests/golden/upsample.npz, tools/make_golden_upsample.py)."""
import os

import numpy as np
import pytest
import torch

import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import synth


@pytest.fixture(scope="module")
def fix(golden_dir):
    return np.load(os.path.join(golden_dir, "upsample.npz"))


def test_upsample_state_dict_keys_shapes_and_seeded_init_equal_the_reference(fix):
    torch.manual_seed(10)
    sd = pkg.UNet_Baseline(3, 4, up_mode="upsample").state_dict()
    assert list(sd.keys()) == [str(k) for k in fix["keys"]]
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(int(d) for d in fix["shape/" + k]), k
        assert torch.equal(v.reshape(-1)[:8].double(), torch.from_numpy(fix["init_head/" + k])), k
        s = float(fix["init_sum/" + k])
        assert abs(float(v.double().sum()) - s) <= 1e-9 * max(1.0, abs(s)), k
    assert sd["up_convs.0.upconv.1.weight"].shape == (512, 1024, 1, 1)


def test_merge_mode_add_still_raises_whatever_the_up_mode():
    for up in ("transpose", "upsample"):
        with pytest.raises(NotImplementedError):
            pkg.UNet_Baseline(3, 4, up_mode=up, merge_mode="add")
    with pytest.raises(ValueError):
        pkg.UNet_Baseline(3, 4, up_mode="nearest")


def test_synth_shapes_follow_the_up_mode():
    m = pkg.UNet_Baseline(3, 4, up_mode="upsample")
    shapes = synth.unet_state_shapes(up_mode="upsample")
    sd = m.state_dict()
    assert list(sd.keys()) == list(shapes.keys())
    assert all(tuple(sd[k].shape) == shapes[k] for k in sd)
    m.load_state_dict(synth.synth_state_dict(up_mode="upsample"))
    # transpose mode (the default) is unchanged
    assert synth.unet_state_shapes() == synth.unet_state_shapes(up_mode="transpose")
    t = synth.unet_state_shapes()
    assert t["up_convs.0.upconv.weight"] == (1024, 512, 2, 2) and "up_convs.0.upconv.1.weight" not in t
    assert sum(int(np.prod(s)) for k, s in t.items() if "running" not in k and "num_batches" not in k) == 31044227
    a, b = synth.synth_state_dict(), synth.synth_state_dict(up_mode="transpose")
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_h3f_refuses_the_upsample_decoder_at_construction():
    m = pkg.UNet_Baseline(3, 4, up_mode="upsample", precision="h3f")
    from crimac_classifiers_unet_amd.engine import UNetEngine
    with pytest.raises(NotImplementedError, match="upsample"):
        UNetEngine(m, "h3f")
