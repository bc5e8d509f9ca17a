"""The data builders of tests/test_gpu_conv_exact.py, run without a GPU: every case's float64 reference alone meets the
preconditions of the exact-integer tests (max|ref| <= 256 and exact in bf16 / fp16, per-channel sum(ref^2) < 2^24 where
statistics are fused, |ref| < 2^24 for weight gradients, per-channel sum|terms| < 2^24 for the BatchNorm-backward sums) --
the builders assert them -- before anything reaches a kernel.  The two persistent-kernel shapes are left to the GPU run."""
import pytest
import torch

import test_gpu_conv_exact as ce

BUILDERS = ce.case_builders()


def test_the_recipe_is_ternary_with_a_quarter_non_zero():
    g = torch.Generator().manual_seed(0)
    v = ce.ternary((1 << 16,), g)
    assert set(v.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert abs(float((v != 0).double().mean()) - 0.25) < 0.01 and abs(float(v.mean())) < 0.01
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(v.to(dt).double(), v)


def test_plane_pairs_of_the_recipe_have_a_zero_lo_plane():
    m = torch.tensor([[-1.0, 0.0, 1.0, 3.0, -3.0, 256.0, 4096.0, 7.0]])
    packed = ce.hp_pack(m)
    halves = packed.view(torch.float16).view(1, 1, 2, 8)
    assert torch.equal(halves[0, 0, 0].float(), m[0]) and float(halves[0, 0, 1].abs().max()) == 0
    assert torch.equal(ce.hp_unpack(packed), m)


@pytest.mark.parametrize("builder,args", BUILDERS, ids=[f"{b.__name__}-{'x'.join(map(str, map(int, a)))}" for b, a in BUILDERS])
def test_reference_meets_the_preconditions(builder, args):
    c = builder(*args)                      # (asserts the preconditions)
    assert c["ref"].dtype == torch.float64
    assert torch.equal(c["ref"], c["ref"].round())        # integers
    if "sums" in c:
        assert all(torch.equal(2 * s, (2 * s).round()) for s in c["sums"])


def test_bn_backward_vectors_keep_every_term_dyadic():
    g = torch.Generator().manual_seed(3)
    vec = ce.bnb_vectors(256, g)
    assert set(vec[1].tolist()) <= {0.5, 1.0, 2.0} and set(vec[2].abs().tolist()) <= {0.5, 1.0, 2.0}
    assert torch.equal(vec[0], vec[0].round()) and torch.equal((vec[3] - 0.25), (vec[3] - 0.25).round())
    y = torch.arange(-3, 4).double()[:, None]
    z = y * vec[2] + vec[3]
    assert torch.equal(z.float().double(), z) and float(z.abs().min()) > 0      # the ReLU decision never sits on a tie
