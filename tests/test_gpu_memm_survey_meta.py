"""GPU: metadata models packed across echograms in the memm survey flows (``pack_metadata=True``).

  * crimac_gather_patches_memm_meta_multi / crimac_meta_planes_multi against the single-source entry points, bit for bit;
  * predict_echograms_memm / evaluate_echograms_memm against the per-echogram calls (predictor stub that reads the metadata
    channels: equal; real networks: one float16 step / the loop's own self-difference);
  * the default (no ``pack_metadata``) still takes the per-echogram path."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import hip, synth  # noqa: E402
from crimac_classifiers_unet_amd import tiled_inference as ti  # noqa: E402
from crimac_classifiers_unet_amd.hip import call, ptr  # noqa: E402
from test_gpu_memm_survey import C, EXTENTS, FREQS, PATCHES, SMALL, STORAGE, SURVEY, make_arrays, raw, with_metadata  # noqa: E402
from test_gpu_survey_eval import moved_share  # noqa: E402
from tools.fake_reader import FakeEchogram  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLAG_SETS = [63, 2, 4 | 8]            # all seven planes; portion_day alone (two planes); time_diff and depth_rel
MC = {k: True for k in ti.META_FLAGS}
TAIL = 3                              # rows past P that must keep the sentinel


# ---- the kernels -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sources():
    """The four echograms of the survey tests, each with its own scalar and vectors; source 1's vectors are shorter than its
    pings (its own index clamp acts), and every seabed vector is 0 at a few pings (inf / NaN in the depth planes)."""
    out = []
    for i, (n_pings, n_range) in enumerate(EXTENTS):
        sv, labels, seabed = make_arrays(n_pings, n_range, seed=10 + i)
        rng = np.random.Generator(np.random.PCG64(70 + i))
        n_vec = 25 if i == 1 else n_pings
        tv = 737000.5 + np.cumsum(rng.uniform(5e-6, 9e-6, size=n_vec + 1))
        sb = seabed[:n_vec].astype(np.int64).copy()
        sb[[0, n_vec // 2, n_vec - 1]] = 0
        out.append(types.SimpleNamespace(
            n_pings=n_pings, n_range=n_range, data=torch.from_numpy(sv).to(DEV), lab=torch.from_numpy(labels).to(DEV),
            year=0.11 + 0.2 * i, day=torch.from_numpy(tv[:-1] % 1).to(DEV),
            td=torch.from_numpy(np.diff(tv) / 6e-6 - 1).to(DEV), sb=torch.from_numpy(sb).to(DEV)))
    return out


def tables(sources):
    rows = [(s.data.data_ptr(), s.lab.data_ptr(), 0, 0, s.n_pings, s.n_range) for s in sources]
    descs = torch.tensor(rows, dtype=torch.int64)
    metas = torch.zeros((len(sources), hip.MEMM_META_WORDS), dtype=torch.float64)
    ints = metas.view(torch.int64)
    for i, s in enumerate(sources):
        metas[i, 0] = s.year
        for j, v in enumerate((s.day, s.td, s.sb)):
            ints[i, 1 + 2 * j], ints[i, 2 + 2 * j] = v.data_ptr(), v.numel()
    assert descs.shape[1] == hip.MEMM_DESC_WORDS
    return descs.to(DEV), metas.to(DEV)


def vectors(s):
    return (s.year, ptr(s.day), s.day.numel(), ptr(s.td), s.td.numel(), ptr(s.sb), s.sb.numel())


def edge_patches(sources, ph, pw):
    """Centres on and beyond every edge and inside, of every source, shuffled: neighbours come from different sources."""
    cen, src = [], []
    for i, s in enumerate(sources):
        for cy in (-ph, 0, s.n_range // 2, s.n_range - 1, s.n_range + ph):
            for cx in (-pw, 0, s.n_pings // 2, s.n_pings - 1, s.n_pings + pw):
                cen.append((cy, cx))
                src.append(i)
    order = np.random.Generator(np.random.PCG64(5)).permutation(len(cen))
    cen, src = np.array(cen, dtype=np.int32)[order], np.array(src, dtype=np.int32)[order]
    assert (src[1:] != src[:-1]).mean() > 0.5
    return cen, src


@pytest.mark.parametrize("patch,overlap", PATCHES)
def test_gather_meta_multi_equals_the_single_source_entry_points_bit_for_bit(sources, patch, overlap):
    pw, ph = patch
    cen, src = edge_patches(sources, ph, pw)
    P, n, rows = len(cen), len(sources), ph * pw
    cen_d, src_d = torch.from_numpy(cen).to(DEV), torch.from_numpy(src).to(DEV)
    descs, metas = tables(sources)
    idx = [np.nonzero(src == i)[0] for i in range(n)]
    idx_d = [torch.from_numpy(ix).to(DEV) for ix in idx]
    # transformed labels of the patches: -100 inside and outside the extent, other ignore values, classes
    rng = np.random.Generator(np.random.PCG64(8))
    lt = torch.from_numpy(rng.choice(np.array([-100, -100, -1, 0, 0, 1, 2], dtype=np.int16), size=(P, ph, pw))).to(DEV)
    for flags in FLAG_SETS:
        for prec, dtype in STORAGE.items():
            code = hip.PREC_NAMES[prec]
            for labelled in (False, True):
                x = torch.empty(((P + TAIL) * rows, 16), dtype=dtype, device=DEV)
                raw(x).fill_(0x5A5A)
                call("crimac_gather_patches_memm_meta_multi", code, ptr(descs), ptr(metas), n, ptr(src_d), C, ptr(cen_d), P,
                     ph, pw, ptr(x), 16, ptr(lt) if labelled else None, 1, flags)
                got = raw(x).view(P + TAIL, rows, -1)
                assert bool((got[P:] == 0x5A5A).all()), (flags, prec, labelled)
                for i, s in enumerate(sources):
                    k = len(idx[i])
                    want = torch.empty((k * rows, 16), dtype=dtype, device=DEV)
                    own = cen_d[idx_d[i]].contiguous()
                    if labelled:
                        call("crimac_gather_patches_memm_labels", code, ptr(s.data), C, s.n_pings, s.n_range, ptr(own), k, ph,
                             pw, ptr(want), 16, ptr(lt[idx_d[i]].contiguous()), 1, flags, *vectors(s), ptr(own))
                    else:
                        call("crimac_gather_patches_memm_meta", code, ptr(s.data), C, s.n_pings, s.n_range, ptr(own), k, ph,
                             pw, ptr(want), 16, ptr(s.lab), 1, flags, *vectors(s), ptr(own))
                    assert torch.equal(got[idx_d[i]], raw(want).view(k, rows, -1)), (flags, prec, labelled, i)
                assert bool((got[:P] != 0).any())
    # a patch whose src lies outside the table, or whose descriptor lacks a vector the flags need, is skipped: nothing written
    x = torch.zeros((3 * rows, 16), dtype=torch.float32, device=DEV)
    bad = torch.tensor([n, -1], dtype=torch.int32, device=DEV)
    for labelled in (False, True):
        call("crimac_gather_patches_memm_meta_multi", hip.PREC_F32X6, ptr(descs), ptr(metas), n, ptr(bad), C, ptr(cen_d), 2,
             ph, pw, ptr(x), 16, ptr(lt) if labelled else None, 1, 63)
        assert bool((x == 0).all())
    lacking = metas.clone()
    lacking.view(torch.int64)[2, 3] = 0                                    # source 2: time_diff NULL
    lacking.view(torch.int64)[3, 6] = 0                                    # source 3: a seabed vector of length 0
    three = torch.tensor([2, 3, 0], dtype=torch.int32, device=DEV)
    call("crimac_gather_patches_memm_meta_multi", hip.PREC_F32X6, ptr(descs), ptr(lacking), n, ptr(three), C, ptr(cen_d), 3,
         ph, pw, ptr(x), 16, None, 1, 4 | 8)
    assert bool((x[:2 * rows] == 0).all()) and bool((x[2 * rows:] != 0).any())
    x.zero_()
    call("crimac_gather_patches_memm_meta_multi", hip.PREC_F32X6, ptr(descs), ptr(lacking), n, ptr(three), C, ptr(cen_d), 3,
         ph, pw, ptr(x), 16, None, 1, 2)                                   # portion_day alone: nothing is lacking
    assert all(bool((x[k * rows:(k + 1) * rows] != 0).any()) for k in range(3))


@pytest.mark.parametrize("patch,overlap", PATCHES)
def test_meta_planes_multi_equals_the_single_source_entry_point_bit_for_bit(sources, patch, overlap):
    pw, ph = patch
    cen, src = edge_patches(sources, ph, pw)
    P, n = len(cen), len(sources)
    cen_d, src_d = torch.from_numpy(cen).to(DEV), torch.from_numpy(src).to(DEV)
    _, metas = tables(sources)
    special = 0
    for flags in FLAG_SETS:
        Cm = bin(flags).count("1") + ((flags >> 1) & 1)
        out = torch.full((P + TAIL, Cm, ph, pw), -7.0, dtype=torch.float32, device=DEV)
        call("crimac_meta_planes_multi", ptr(metas), n, ptr(src_d), ptr(cen_d), P, ph, pw, flags, ptr(out))
        assert bool((out[P:] == -7.0).all())
        for i, s in enumerate(sources):
            ix = torch.from_numpy(np.nonzero(src == i)[0]).to(DEV)
            want = torch.empty((len(ix), Cm, ph, pw), dtype=torch.float32, device=DEV)
            call("crimac_meta_planes", ptr(cen_d[ix].contiguous()), len(ix), ph, pw, flags, *vectors(s), ptr(want))
            assert torch.equal(out[ix].view(torch.int32), want.view(torch.int32)), (flags, i)      # (inf / NaN compare too)
        special += int((~torch.isfinite(out[:P])).sum())
    assert special > 0                                                     # the seabed of 0 did reach the depth planes
    bad = torch.tensor([n, -1], dtype=torch.int32, device=DEV)
    out = torch.full((2, 7, ph, pw), -7.0, dtype=torch.float32, device=DEV)
    call("crimac_meta_planes_multi", ptr(metas), n, ptr(bad), ptr(cen_d), 2, ph, pw, 63, ptr(out))
    assert bool((out == -7.0).all())


# ---- the flows ---------------------------------------------------------------------------------------------------------
BOXES = [(5, 40, 5, 60), (30, 60, 90, 125)]


def meta_survey(indices=(0, 1, 2, 3, 4, 5), shift=3):
    """Echograms of the survey tests with metadata and school boxes.  ``shift``: get_seabed answers a line ``shift`` rows
    below the reader's ``_seabed`` -- the line that masks and grids is then not the vector the depth planes go by."""
    egs = []
    for i in indices:
        n_pings, n_range = SURVEY[i]
        sv, labels, seabed = make_arrays(n_pings, n_range, seed=30 + i)
        eg = with_metadata(FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), seabed,
                                        frequencies=FREQS, name=f"eg{i}"), 50 + i)
        eg.object_bounding_boxes = np.array(BOXES, dtype=int)
        if shift:
            eg.get_seabed = lambda idx_ping=None, n_pings=1, eg=eg, **kw: eg._seabed[idx_ping:idx_ping + n_pings] + shift
        egs.append(eg)
    return egs


def make_pipe(model):
    return types.SimpleNamespace(model=model.to(DEV).eval(), device=torch.device(DEV), frequencies=FREQS)


def meta_model(kind, precision, weights=True):
    if kind == "late":
        model = pkg.UNet_LateMetInject(3, 4, 7, depth=3, precision=precision)
        sd = synth.synth_state_dict(depth=3, seed=4, meta_in_channels=7)
    else:
        model = pkg.UNet_Baseline(3, 11, depth=3, precision=precision)
        sd = synth.synth_state_dict(depth=3, seed=3, in_channels=11)
    if weights:
        model.load_state_dict(sd)
    return model


def stub_logits(x, P, H, W):
    """Per pixel and elementwise (the result of a patch cannot depend on its batch), reading the four data channels AND the
    seven metadata channels of an early-injection input (float32 storage); inf / NaN planes (seabed 0) are made finite."""
    d = x.float().reshape(P, H, W, 16).permute(0, 3, 1, 2)
    m = torch.nan_to_num(d[:, 4:11], nan=0.5, posinf=2.0, neginf=-2.0).clamp(-4.0, 4.0)
    z1 = 0.9 * d[:, 0] - 0.7 * d[:, 1] + 0.31 * m[:, 0] + 0.23 * m[:, 1] - 0.19 * m[:, 2] + 0.17 * m[:, 3]
    z2 = 0.8 * d[:, 2] - 1.1 * d[:, 3] + 0.29 * m[:, 4] - 0.13 * m[:, 5] + 0.37 * m[:, 6]
    return torch.stack([0 * z1, z1, z2], dim=1).contiguous()


def stub_probs(x, P, H, W):
    return torch.softmax(stub_logits(x, P, H, W), dim=1).contiguous()


@pytest.fixture(scope="module")
def early_stub_pipe():
    return make_pipe(meta_model("early", "f32x6", weights=False))


def flat_line(eg):
    return np.full(eg.shape[1], 12, dtype=np.int64)


def single_seabed(seabed, eg):
    return seabed(eg) if callable(seabed) else seabed


@pytest.mark.parametrize("patch,overlap", PATCHES)
def test_packed_prediction_of_a_metadata_model_equals_the_per_echogram_call(early_stub_pipe, patch, overlap):
    egs, pipe = meta_survey(), early_stub_pipe
    counts = [len(r.grid) for g in ti.iter_memm_groups(iter(egs), patch, overlap, 10 ** 9) for r in g]
    batch = 8 if patch == (32, 32) else 3
    group_patches = counts[0] + counts[1] // 2
    assert any(sum(counts[:k]) % batch for k in range(1, len(egs)))               # a batch spans two echograms
    stats = {}
    got = list(ti.predict_echograms_memm(iter(egs), pipe, patch, overlap, batch, predict_fn=stub_probs, meta_channels=MC,
                                         pack_metadata=True, group_patches=group_patches, group_elems=SMALL, stats=stats))
    assert [eg for eg, _ in got] == egs
    assert stats["fallback_echograms"] == stats["solo_echograms"] == 0 and stats["groups"] >= 2
    assert sum(stats["batches"]) == sum(counts) and max(stats["batches"]) == batch
    for eg, out in got:
        want = ti.predict_echogram_memm(eg, pipe, patch, overlap, batch, predict_fn=stub_probs, meta_channels=MC)
        assert np.array_equal(out, want) and (out != 0).any() and (out == 0).any(), eg.name
    # the planes do reach the stub: another scalar changes the result
    other = meta_survey()
    other[0].portion_of_year_scalar = 0.2
    moved = next(iter(ti.predict_echograms_memm(iter(other[:1]), pipe, patch, overlap, batch, predict_fn=stub_probs,
                                                meta_channels=MC, pack_metadata=True, group_elems=SMALL)))[1]
    assert not np.array_equal(moved, got[0][1])
    # the same survey without the keyword: the per-echogram path, as before
    stats = {}
    again = list(ti.predict_echograms_memm(iter(egs), pipe, patch, overlap, batch, predict_fn=stub_probs, meta_channels=MC,
                                           stats=stats))
    assert stats["fallback_echograms"] == len(egs) and stats["groups"] == 0
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(again, got))
    ti.release_staging()


def bright_bottom(egs):
    """Finite samples with a bright bottom echo (the estimate is a real line), and a stored ``_seabed`` of zeros that no
    path may use once a line is estimated or called."""
    out = []
    for eg in egs:
        sv = np.nan_to_num(eg.sv, nan=1e-7, posinf=1e-7, neginf=1e-7)
        for x in range(eg.shape[1]):
            sv[:, min(int(eg._seabed[x]), eg.shape[0] - 2), x] = 5.0
        new = with_metadata(FakeEchogram(sv, eg.labels, np.zeros_like(eg._seabed), frequencies=FREQS, name=eg.name), 90)
        new.portion_of_day_vector, new.time_vector_diff = eg.portion_of_day_vector, eg.time_vector_diff
        out.append(new)
    return out


@pytest.mark.parametrize("seabed", ["estimate", flat_line], ids=["estimate", "callable"])
def test_the_depth_planes_go_by_the_estimated_or_called_line(early_stub_pipe, seabed):
    egs, pipe = bright_bottom(meta_survey((0, 1, 3, 5), shift=0)), early_stub_pipe
    stats = {}
    got = list(ti.predict_echograms_memm(iter(egs), pipe, (32, 32), 4, 8, predict_fn=stub_probs, meta_channels=MC,
                                         pack_metadata=True, seabed=seabed, group_patches=40, group_elems=SMALL, stats=stats))
    assert stats["fallback_echograms"] == 0 and stats["groups"] >= 2 and len(got) == len(egs)
    for eg, out in got:
        want = ti.predict_echogram_memm(eg, pipe, (32, 32), 4, 8, predict_fn=stub_probs, meta_channels=MC,
                                        seabed=single_seabed(seabed, eg))
        assert np.array_equal(out, want) and (out != 0).any(), eg.name
    ti.release_staging()


def test_packed_prediction_of_a_late_injection_model_with_a_predictor_stub():
    """With a ``predict_fn`` no planes are built (as ChunkPredictor.predict): the packing itself, for a late-injection model."""
    egs, pipe = meta_survey(), make_pipe(meta_model("late", "f32x6", weights=False))
    stats = {}
    got = list(ti.predict_echograms_memm(iter(egs), pipe, (32, 32), 4, 8, predict_fn=stub_probs, meta_channels=MC,
                                         pack_metadata=True, group_patches=40, group_elems=SMALL, stats=stats))
    assert stats["fallback_echograms"] == 0 and stats["groups"] >= 2
    for eg, out in got:
        assert np.array_equal(out, ti.predict_echogram_memm(eg, pipe, (32, 32), 4, 8, predict_fn=stub_probs, meta_channels=MC))
    ti.release_staging()


class Batches:
    def __init__(self):
        self.names = []

    def __call__(self, centres, labels, logits, *, echograms=None):
        self.names.append({eg.name for eg in echograms})


def loop_sum(egs, pipe, patch, overlap, batch, seabed=None, **kw):
    hp = hn = 0
    for eg in egs:
        a, b = ti.evaluate_echogram_memm(eg, pipe, patch, overlap, batch, seabed=single_seabed(seabed, eg), **kw)
        hp, hn = hp + a, hn + b
    return hp, hn


@pytest.mark.parametrize("mode", ["all", "region"])
def test_packed_evaluation_of_a_metadata_model_equals_the_sum_of_the_per_echogram_calls(early_stub_pipe, mode):
    egs, pipe = meta_survey(), early_stub_pipe
    kw = dict(eval_mode=mode, predict_fn=stub_logits, meta_channels=MC)
    want = loop_sum(egs, pipe, (32, 32), 4, 8, **kw)
    stats, hook = {}, Batches()
    got = ti.evaluate_echograms_memm(iter(egs), pipe, (32, 32), 4, 8, pack_metadata=True, group_patches=40,
                                     group_elems=SMALL, stats=stats, on_batch=hook, **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0].sum() > 0 and got[1].sum() > 1000
    assert stats["fallback_echograms"] == stats["solo_echograms"] == 0 and stats["groups"] >= 2
    assert any(len(b) >= 2 for b in hook.names)                                   # a batch holds several echograms
    stats = {}
    again = ti.evaluate_echograms_memm(iter(egs), pipe, (32, 32), 4, 8, stats=stats, **kw)
    assert stats["fallback_echograms"] == len(egs) and np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    ti.release_staging()


def test_an_echogram_larger_than_the_staging_takes_the_solo_path_with_its_metadata(early_stub_pipe):
    egs, pipe = meta_survey(), early_stub_pipe
    cap = 130 * 64 + 17 * 17 + 1000                                               # the 300 x 90 echogram does not fit
    for seabed in (None, flat_line):
        stats = {}
        got = list(ti.predict_echograms_memm(iter(egs), pipe, (32, 32), 4, 8, predict_fn=stub_probs, meta_channels=MC,
                                             pack_metadata=True, seabed=seabed, group_elems=cap, stats=stats))
        assert stats["solo_echograms"] == 1 and stats["fallback_echograms"] == 0 and [eg for eg, _ in got] == egs
        for eg, out in got:
            assert np.array_equal(out, ti.predict_echogram_memm(eg, pipe, (32, 32), 4, 8, predict_fn=stub_probs,
                                                                meta_channels=MC, seabed=single_seabed(seabed, eg))), eg.name
        kw = dict(eval_mode="region", predict_fn=stub_logits, meta_channels=MC)
        stats = {}
        hist = ti.evaluate_echograms_memm(iter(egs), pipe, (32, 32), 4, 8, pack_metadata=True, seabed=seabed, group_elems=cap,
                                          stats=stats, **kw)
        want = loop_sum(egs, pipe, (32, 32), 4, 8, seabed=seabed, **kw)
        assert stats["solo_echograms"] == 1 and np.array_equal(hist[0], want[0]) and np.array_equal(hist[1], want[1])
    ti.release_staging()


# ---- real networks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32x6", "h3p"])
@pytest.mark.parametrize("kind", ["late", "early"])
def test_real_networks_packed_against_the_per_echogram_calls(kind, precision, monkeypatch):
    """Prediction: batches of another composition move a float16 rounding by at most one step, 2**-11 just below 1.0 (the
    bound of test_generator_with_the_real_network_is_within_one_float16_step).  Evaluation ('region'): the totals of both
    histograms are the loop's exactly; the share of pixels in another bin is at most twice what the loop over
    evaluate_echogram_memm shows against itself with internal batches of 8 and of 32 patches, measured here; where that
    is zero the histograms are equal.  Both figures are printed."""
    pipe = make_pipe(meta_model(kind, precision))
    egs = meta_survey((0, 1, 2, 3, 5))
    patch, overlap = (64, 64), 6
    stats = {}
    got = list(ti.predict_echograms_memm(iter(egs), pipe, patch, overlap, 4, meta_channels=MC, pack_metadata=True,
                                         group_elems=SMALL, stats=stats))
    assert stats["fallback_echograms"] == stats["solo_echograms"] == 0 and stats["groups"] >= 1
    worst = 0.0
    for eg, out in got:
        want = ti.predict_echogram_memm(eg, pipe, patch, overlap, 4, meta_channels=MC)
        assert np.array_equal(out != 0, want != 0) and (out != 0).any(), eg.name
        worst = max(worst, float(np.abs(out - want).max()))
    print(f"{kind} {precision}: prediction, largest difference {worst:.3e}, batches {stats['batches']}")
    assert worst <= 2 ** -11
    kw = dict(eval_mode="region", meta_channels=MC)
    runs = {}
    for ib in (8, 32):
        monkeypatch.setattr(ti, "INTERNAL_BATCH", ib)
        runs[ib] = loop_sum(egs, pipe, patch, overlap, 4, **kw)
    monkeypatch.undo()
    yardstick = moved_share(runs[8], runs[32])
    want = loop_sum(egs, pipe, patch, overlap, 4, **kw)
    stats, hook = {}, Batches()
    hist = ti.evaluate_echograms_memm(iter(egs), pipe, patch, overlap, 4, pack_metadata=True, group_elems=SMALL, stats=stats,
                                      on_batch=hook, **kw)
    moved = moved_share(want, hist)
    print(f"{kind} {precision}: evaluation, moved share packed vs loop {moved:.3e}, loop vs itself (internal batch 8 / 32) "
          f"{yardstick:.3e}, batches {stats['batches']}")
    assert stats["fallback_echograms"] == 0 and any(len(b) >= 2 for b in hook.names)
    assert hist[0].sum() == want[0].sum() > 0 and hist[1].sum() == want[1].sum() > 1000
    assert moved <= 2 * yardstick, (moved, yardstick)
    if yardstick == 0.0:
        assert np.array_equal(hist[0], want[0]) and np.array_equal(hist[1], want[1])
    ti.release_staging()
