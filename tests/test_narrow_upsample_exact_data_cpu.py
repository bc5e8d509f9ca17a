"""The data builders of tests/test_gpu_narrow_upsample_exact.py, run without a GPU: every case's float64 reference alone
meets the preconditions of the exact tests (max|ref| <= 256 and exact in bf16 / fp16, per-channel sum(ref^2) < 2^24 where
statistics are fused, |ref| < 2^24 for weight gradients; for the bilinear kernels z = W x + b an integer with |z| <= 16 and
every output k / 16 with |k| <= 256) -- the builders assert them -- before anything reaches a kernel.  The B = 800 cases of
the persistent loop are built here too."""
import pytest
import torch

import test_gpu_narrow_upsample_exact as nu

BUILDERS = nu.case_builders()


def test_thinned_operands_stay_ternary():
    g = torch.Generator().manual_seed(0)
    for levels in (8, 12, 16, 32):
        v = nu.ternary((1 << 16,), g, levels)
        assert set(v.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert abs(float((v != 0).double().mean()) - 2 / levels) < 0.01 and abs(float(v.mean())) < 0.01


def test_the_default_density_draws_what_it_drew_before():
    g, h = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    v = torch.randint(0, 8, (4096,), generator=h)
    assert torch.equal(nu.ternary((4096,), g), (v == 0).double() - (v == 1).double())


@pytest.mark.parametrize("builder,args", BUILDERS, ids=[f"{b.__name__}-{'x'.join(map(str, map(int, a)))}" for b, a in BUILDERS])
def test_reference_meets_the_preconditions(builder, args):
    c = builder(*args)                      # (asserts the preconditions)
    assert c["ref"].dtype == torch.float64
    k = c["ref"] * (16 if builder is nu.up1x1_case else 1)
    assert torch.equal(k, k.round())
    if builder is nu.up1x1_case:
        assert torch.equal(c["z"], c["z"].round()) and float(c["z"].abs().max()) <= 16
        assert torch.equal(16 * c["dz"], (16 * c["dz"]).round()) and torch.equal(c["dx"], c["dx"].round())


def test_every_narrow_layer_of_the_three_widths_is_a_case():
    """(Cin, N) of the conv3x3 layers and (Cin, Cout) of the transposed convolutions of start_filts 8, 16, 32 with a
    channel count below 64 (engine.py: l.narrow), depth 5."""
    convs, ups = set(), set()
    for sf in (8, 16, 32):
        for i in range(5):
            c = sf * 2 ** i
            convs |= {(4 if i == 0 else c // 2, c), (c, c)}
        for j in range(4):
            c = sf * 2 ** (4 - j) // 2
            ups.add((2 * c, c))
            convs |= {(2 * c, c), (c, c)}
    narrow = {p for p in convs if min(p) < 64}
    assert narrow == set(nu.PAIRS + nu.FIRST)
    assert {p for p in ups if min(p) < 64} == set(nu.UP_PAIRS)


@pytest.mark.parametrize("prec", ["bf16", "h3p_planes"])
def test_replica_sums_partition_the_image_by_tile(prec):
    c = nu.narrow_fwd_case(2, 33, 17, 8, 8)
    r = nu.replica_sums(c["ref"], prec)
    assert torch.equal(r.sum(1)[0], c["ref"].sum((0, 2, 3))) and torch.equal(r.sum(1)[1], (c["ref"] ** 2).sum((0, 2, 3)))
    # 33 x 17: tiles (by, bx) of image 0 are 0 .. 5 on 16 x 16 tiles, 0 .. 3 on 16 x 32 ones; tile 1 = columns 16 .. of rows 0 ..
    th = 16 if prec == "bf16" else 32
    ones = torch.zeros(2, 1, 33, 17, dtype=torch.float64)
    ones[0, 0, :th, 16:] = 1
    assert nu.replica_sums(ones, prec)[0, :, 0].tolist() == [0.0, float(th), 0.0]


@pytest.mark.parametrize("prec", ["bf16", "h3p"])
def test_persistent_cases_outnumber_the_grid_of_an_mi355x(prec):
    """256 CUs, at most 4 workgroups per CU: more tiles than workgroups, and no whole number of rounds (the GPU test asserts
    the same against the device it runs on)."""
    tiles = nu.persist_tiles(prec)
    assert tiles == (3200 if prec == "bf16" else 1600)
    assert tiles > 4 * 256 and all(tiles % (k * 256) for k in (1, 2, 3, 4))
