"""GPU: the seabed-line estimate of a memmap echogram (crimac_seabed_columns + tiled_inference.estimate_seabed) against the
reference's own Echogram.get_seabed (tests/golden/seabed_estimate.npz, tools/make_golden_seabed.py): exact, every ping."""
import os
import types

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import tiled_inference as ti
from tools.fake_reader import FakeEchogram
from tools.make_golden_seabed import EXACT_CASES, REAL_CASE, EchogramStandIn, decode

pytestmark = pytest.mark.gpu

TAGS = [c[0] for c in EXACT_CASES + [REAL_CASE]]
PATCH, OVERLAP = (64, 64), 8


@pytest.fixture(scope="module")
def fix(golden_dir):
    with np.load(os.path.join(golden_dir, "seabed_estimate.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases(fix):
    """tag -> (data float32 [R, P, F], its planes [F][R, P] as data_memmaps() hands them out); decoded once."""
    out = {}
    for tag in TAGS:
        data = decode(fix, tag)
        out[tag] = (data, [np.ascontiguousarray(data[:, :, f]) for f in range(data.shape[2])])
    return out


def run_columns(data, splits):
    """crimac_seabed_columns over the chunks [s, e) of ``splits``, each uploaded with its halo pings."""
    R, P, F = data.shape
    n = ti.seabed_rows(R)[0]
    fpr = torch.from_numpy(np.ascontiguousarray(data.transpose(2, 1, 0))).cuda()          # [F, P, R]
    idx = torch.full((F, P), -99, dtype=torch.int32, device="cuda")
    colmax = torch.full((F, P), -99.0, dtype=torch.float32, device="cuda")
    for s, e in splits:
        lo, hi = max(0, s - 1), min(P, e + 1)
        ti.seabed_columns(fpr[:, lo:hi].contiguous(), lo < s, hi > e, n, idx, colmax, ping0=s)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), colmax.cpu().numpy()


@pytest.mark.parametrize("tag", TAGS)
def test_kernel_columns_equal_the_restatement(fix, cases, tag):
    """idx and colmax of every (frequency, ping) == the numpy restatement (same order of fp64 additions; on the exact cases
    any order): the whole echogram in one launch (no halo: zero padding on both edges), and cut into uneven chunks with
    a left halo, a right halo, both, and a chunk of one ping."""
    data = cases[tag][0]
    P = data.shape[1]
    cuts = sorted({0, min(1, P), min(2, P), P // 3, P // 3 + 1, (2 * P) // 3, P})
    for splits in ([(0, P)], list(zip(cuts[:-1], cuts[1:]))):
        idx, colmax = run_columns(data, splits)
        assert np.array_equal(idx, fix[tag + "/idx"]), (tag, splits)
        assert np.array_equal(colmax, fix[tag + "/colmax"]), (tag, splits)


@pytest.mark.parametrize("tag", TAGS)
def test_estimate_equals_the_reference_vector(fix, cases, tag):
    """estimate_seabed == Echogram.get_seabed of the reference: no tolerance, no excluded ping; whole, in chunks of 64
    pings and of 1 ping (halos on both sides of a single-ping chunk), and from the resident [F, pings, range] tensor."""
    data, planes = cases[tag]
    ref = fix[tag + "/ref"]
    for chunk_pings in (None, 64, 1):
        got = ti.estimate_seabed(planes, chunk_pings=chunk_pings)
        assert got.dtype == np.dtype(int) and np.array_equal(got, ref), (tag, chunk_pings)
    resident = torch.from_numpy(np.ascontiguousarray(data.transpose(2, 1, 0))).cuda()
    assert np.array_equal(ti.estimate_seabed(resident), ref)


@pytest.mark.parametrize("tag", ["b", "c", "real"])
def test_estimate_memm_reads_every_frequency_of_the_echogram(fix, cases, tag):
    eg = EchogramStandIn(cases[tag][0])
    asked = []
    plain = eg.data_memmaps
    eg.data_memmaps = lambda frequencies=None: asked.append(frequencies) or plain(frequencies)
    assert np.array_equal(ti.estimate_seabed_memm(eg, chunk_pings=100), fix[tag + "/ref"])
    assert asked == [None]


def stub_predict_fn(x, P, H, W):
    d = x.float().reshape(P, H, W, 16)[..., :4].permute(0, 3, 1, 2)
    z = torch.stack([0 * d[:, 0], 0.02 * d[:, 0] - 0.01 * d[:, 1], 0.015 * d[:, 2] - 0.02 * d[:, 3]], dim=1)
    return torch.softmax(z, dim=1).contiguous()


@pytest.fixture(scope="module")
def pipe():
    import crimac_classifiers_unet_amd as pkg
    model = pkg.UNet_Baseline(3, 4, precision="f32x6").cuda().eval()
    return types.SimpleNamespace(model=model, device=torch.device("cuda"), frequencies=[18, 38, 120, 200])


def memm_echogram(data, seabed):
    R, P, F = data.shape
    labels = np.zeros((R, P), dtype=np.int16)
    labels[R // 3:R // 2, P // 4:P // 2] = 27
    return FakeEchogram(np.ascontiguousarray(data.transpose(2, 0, 1)), labels, seabed)


@pytest.mark.parametrize("order", ["same", "reversed"])
def test_memm_prediction_with_the_estimate_equals_the_reference_vector_passed_in(fix, cases, pipe, order):
    """predict_echogram_memm(seabed="estimate") == the same call with the reference's vector as an array, bit for bit --
    with the model's frequencies the echogram's (the resident tensor is reused) and in another order (every plane of the
    echogram is uploaded for the estimate); the reader's get_seabed is not asked in either."""
    data, ref = cases["b"][0], fix["b/ref"]
    eg = memm_echogram(data, np.zeros_like(ref))

    def refuse(*a, **k):
        raise AssertionError("get_seabed was called")
    eg.get_seabed = refuse
    p = types.SimpleNamespace(**vars(pipe))
    if order == "reversed":
        p.frequencies = pipe.frequencies[::-1]
    want = ti.predict_echogram_memm(eg, p, PATCH, OVERLAP, 8, predict_fn=stub_predict_fn, seabed=ref.astype(np.int64))
    got = ti.predict_echogram_memm(eg, p, PATCH, OVERLAP, 8, predict_fn=stub_predict_fn, seabed="estimate")
    assert want.shape == (2, data.shape[0], data.shape[1]) and (want != 0).any()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # the vector matters: another line masks other pixels
    other = ti.predict_echogram_memm(eg, p, PATCH, OVERLAP, 8, predict_fn=stub_predict_fn, seabed=ref.astype(np.int64) - 60)
    assert not np.array_equal(other, want)


def test_memm_paths_still_ask_the_reader_by_default(fix, cases, pipe):
    """seabed=None: the reader's get_seabed(0, n_pings) is the line, as before; evaluate_echogram_memm takes the same
    three forms and gives the same histograms for the estimate and for the reference's vector."""
    data, ref = cases["b"][0], fix["b/ref"]
    eg = memm_echogram(data, ref)
    calls = []
    plain = eg.get_seabed
    eg.get_seabed = lambda *a, **k: calls.append(a) or plain(*a, **k)
    out = ti.predict_echogram_memm(eg, pipe, PATCH, OVERLAP, 8, predict_fn=stub_predict_fn)
    assert calls == [(0, data.shape[1])]
    given = ti.predict_echogram_memm(eg, pipe, PATCH, OVERLAP, 8, predict_fn=stub_predict_fn, seabed=ref)
    assert len(calls) == 1 and np.array_equal(out, given)
    h_none = ti.evaluate_echogram_memm(eg, pipe, PATCH, OVERLAP, 8, predict_fn=stub_predict_fn)
    assert len(calls) == 2 and calls[1] == (0, data.shape[1])
    h_est = ti.evaluate_echogram_memm(eg, pipe, PATCH, OVERLAP, 8, predict_fn=stub_predict_fn, seabed="estimate")
    assert len(calls) == 2
    assert h_none[0].sum() + h_none[1].sum() > 0
    assert np.array_equal(h_none[0], h_est[0]) and np.array_equal(h_none[1], h_est[1])
