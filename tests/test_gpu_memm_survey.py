"""GPU: survey-level memm prediction -- batches packed from several echograms (tiled_inference.predict_echograms_memm).

  * crimac_gather_patches_memm_multi / crimac_scatter_patches_multi against the single-source kernels, bit for bit;
  * the generator against predict_echogram_memm per echogram (predictor stub: equal; real network: one float16 step);
  * seabed="estimate", the per-echogram path of metadata models, save_predictions_memm."""
import os
import types

import numpy as np
import pytest
import torch

import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import hip, synth
from crimac_classifiers_unet_amd import tiled_inference as ti
from crimac_classifiers_unet_amd.hip import call, ptr
from tools.fake_reader import FakeEchogram

pytestmark = pytest.mark.gpu

C = 4
EXTENTS = [(300, 90), (40, 200), (17, 17), (130, 64)]          # pings x range; the third is smaller than either patch
PATCHES = [((32, 32), 4), ((64, 64), 6)]                        # (patch_size, patch_overlap)
STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32x6": torch.float32, "h3p": torch.float32}
FREQS = [18, 38, 120, 200]
SMALL = 1 << 19                                                  # group_elems of the tests: 2 MB planes, not 256 MB


def make_arrays(n_pings, n_range, seed):
    """sv [C, pings, range] linear with NaN / Inf, raw labels [pings, range] int16 with negative ids, seabed [pings]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sv = np.power(10.0, rng.uniform(-8.5, 0.5, size=(C, n_pings, n_range))).astype(np.float32)
    sv[0][rng.random((n_pings, n_range)) < 0.01] = np.nan
    sv[2][rng.random((n_pings, n_range)) < 0.01] = np.inf
    sv[3][rng.random((n_pings, n_range)) < 0.005] = -np.inf
    labels = np.zeros((n_pings, n_range), dtype=np.int16)
    for val in (27, -1, 1, -100, 12, -1):
        w, h = max(1, n_pings // 5), max(1, n_range // 4)
        x0, y0 = int(rng.integers(0, n_pings - w + 1)), int(rng.integers(0, n_range - h + 1))
        labels[x0:x0 + w, y0:y0 + h] = val
    x = np.arange(n_pings)
    seabed = (0.6 * n_range + 0.25 * n_range * np.sin(x / 11.0 + seed)).astype(np.int64)
    return sv, labels, np.clip(seabed, 1, n_range + 3)


@pytest.fixture(scope="module")
def sources():
    """The four echograms, resident as the single-source kernels take them, made once."""
    out = []
    for i, (n_pings, n_range) in enumerate(EXTENTS):
        sv, labels, seabed = make_arrays(n_pings, n_range, seed=10 + i)
        out.append(types.SimpleNamespace(
            n_pings=n_pings, n_range=n_range, sv=sv, labels=labels, seabed=seabed,
            data=torch.from_numpy(sv).cuda(), lab=torch.from_numpy(labels).cuda(),
            sb=torch.from_numpy(seabed.astype(np.int32)).cuda()))
    return out


def desc_table(sources, outs=None, seabeds=None):
    rows = [(s.data.data_ptr(), s.lab.data_ptr(), 0 if seabeds is None else seabeds[i].data_ptr(),
             0 if outs is None else outs[i].data_ptr(), s.n_pings, s.n_range) for i, s in enumerate(sources)]
    t = torch.tensor(rows, dtype=torch.int64)
    assert t.shape[1] == hip.MEMM_DESC_WORDS
    return t.cuda()


def raw(x):
    return x.view(torch.int16) if x.element_size() == 2 else x.view(torch.int32)


@pytest.mark.parametrize("patch,overlap", PATCHES)
def test_gather_multi_equals_the_single_source_kernel_bit_for_bit(sources, patch, overlap):
    pw, ph = patch
    rng = np.random.Generator(np.random.PCG64(5))
    cen, src = [], []
    for i, s in enumerate(sources):              # centres on and beyond every edge, and inside
        for cy in (-ph, 0, s.n_range // 2, s.n_range - 1, s.n_range + ph):
            for cx in (-pw, 0, s.n_pings // 2, s.n_pings - 1, s.n_pings + pw):
                cen.append((cy, cx))
                src.append(i)
    order = rng.permutation(len(cen))
    cen, src = np.array(cen, dtype=np.int32)[order], np.array(src, dtype=np.int32)[order]
    P, rows = len(cen), ph * pw
    cen_d, src_d = torch.from_numpy(cen).cuda(), torch.from_numpy(src).cuda()
    table = desc_table(sources)
    for prec, dtype in STORAGE.items():
        code = hip.PREC_NAMES[prec]
        x = torch.empty(((P + 3) * rows, 16), dtype=dtype, device="cuda")
        raw(x).fill_(0x5A5A)                                                       # sentinel, rows >= P must keep it
        call("crimac_gather_patches_memm_multi", code, ptr(table), len(sources), ptr(src_d), C, ptr(cen_d), P, ph, pw,
             ptr(x), 16)
        got = raw(x).view(P + 3, rows, -1)
        assert bool((got[P:] == 0x5A5A).all()), prec
        for i, s in enumerate(sources):
            idx = np.nonzero(src == i)[0]
            want = torch.empty((len(idx) * rows, 16), dtype=dtype, device="cuda")
            own = torch.from_numpy(cen[idx]).cuda()
            call("crimac_gather_patches_memm", code, ptr(s.data), C, s.n_pings, s.n_range, ptr(own), len(idx), ph, pw,
                 ptr(want), 16, ptr(s.lab))
            assert torch.equal(got[torch.from_numpy(idx).cuda()], raw(want).view(len(idx), rows, -1)), (prec, i)
        # channels >= C are zero (plane pairs: 8 channels = [8 hi][8 lo] halves, two such groups per pixel)
        h = x[:P * rows].view(torch.int16).view(P * rows, -1)
        pad = h[:, C:] if prec in ("bf16", "fp16") else \
            torch.cat([h[:, C:8], h[:, 8 + C:]], 1) if prec == "h3p" else x[:P * rows, C:].view(torch.int32)
        assert bool((pad == 0).all()), prec
        assert bool((h[:, :C] != 0).any())
    # a patch whose src lies outside the table is skipped, not read
    x = torch.zeros((2 * rows, 16), dtype=torch.float32, device="cuda")
    bad = torch.tensor([len(sources), -1], dtype=torch.int32, device="cuda")
    call("crimac_gather_patches_memm_multi", hip.PREC_F32X6, ptr(table), len(sources), ptr(bad), C, ptr(cen_d), 2, ph, pw,
         ptr(x), 16)
    assert bool((x == 0).all())


@pytest.mark.parametrize("out_f16", [True, False])
@pytest.mark.parametrize("patch,overlap", PATCHES)
def test_scatter_multi_equals_the_single_destination_kernel_bit_for_bit(sources, patch, overlap, out_f16):
    pw, ph = patch
    rng = np.random.Generator(np.random.PCG64(6))
    # seabed lines that cut patches in half (the sources' undulating lines) and one that lies wholly above its patches
    lines = [s.sb for s in sources]
    lines[1] = torch.full_like(lines[1], 3)
    cen, src = [], []
    # the echogram's own grid: the rim beyond every edge, interiors disjoint (without the memm centre-row adjustment, which
    # stacks the rows of a shallow echogram on one centre: equal patches there, but these probabilities are random)
    for i, s in enumerate(sources):
        g = ti.plan_eval_grid(s.n_range, np.full(s.n_pings, s.n_range), s.n_pings, patch, overlap)
        assert len(np.unique(g, axis=0)) == len(g)
        cen.append(g)
        src += [i] * len(g)
    order = rng.permutation(len(src))
    cen, src = np.concatenate(cen).astype(np.int32)[order], np.array(src, dtype=np.int32)[order]
    P = len(cen)
    probs = torch.from_numpy(rng.random((P, 3, ph, pw), dtype=np.float32)).cuda()
    dtype = torch.float16 if out_f16 else torch.float32
    GAP, SENT, FILL = 5, -3.0, 7.0               # an odd gap: the destinations are aligned to their element only
    sizes = [2 * s.n_range * s.n_pings for s in sources]
    flat = torch.full((sum(sizes) + GAP * (len(sizes) + 1),), SENT, dtype=dtype, device="cuda")
    outs, gaps, off = [], [], 0
    for n in sizes:
        gaps.append(flat[off:off + GAP])
        outs.append(flat[off + GAP:off + GAP + n])
        outs[-1].fill_(FILL)
        off += GAP + n
    gaps.append(flat[off:])
    table = desc_table(sources, outs, lines)
    cen_d, src_d = torch.from_numpy(cen).cuda(), torch.from_numpy(src).cuda()
    call("crimac_scatter_patches_multi", ptr(probs), 3, ptr(table), len(sources), ptr(src_d), ptr(cen_d), P, ph, pw, overlap,
         ti.SEABED_PAD, int(out_f16))
    assert all(bool((g == SENT).all()) for g in gaps)
    for i, s in enumerate(sources):
        idx = np.nonzero(src == i)[0]
        want = torch.full((2, s.n_range, s.n_pings), FILL, dtype=dtype, device="cuda")
        own_probs, own_cen = probs[torch.from_numpy(idx).cuda()].contiguous(), torch.from_numpy(cen[idx]).cuda()
        call("crimac_scatter_patches_ex", ptr(own_probs), 3, ptr(own_cen), len(idx), ph, pw, overlap, 0, s.n_pings,
             s.n_range, ptr(s.lab), None, 0, s.n_pings, ptr(lines[i]), 0, s.n_pings, None, 0, s.n_pings, ti.SEABED_PAD, 1,
             ptr(want), int(out_f16))
        assert torch.equal(raw(outs[i]), raw(want.view(-1))), i
        written = want != FILL
        assert bool(written.any()) and not bool(written.all())               # labels, seabed and the rim all masked some
    # the line of echogram 1 lies above everything but its first rows: background below it stays unwritten
    bg = (sources[1].lab.t() == 0)
    deep = torch.arange(sources[1].n_range, device="cuda")[:, None] >= 3 + ti.SEABED_PAD
    assert bool((outs[1].view(2, sources[1].n_range, -1)[0][bg & deep] == FILL).all())


# ---- the generator ---------------------------------------------------------------------------------------------------
SURVEY = [(300, 90), (40, 200), (17, 17), (130, 64), (100, 50), (64, 128), (200, 33)]      # pings x range


def stub_predict_fn(x, P, H, W):
    """Per-pixel and elementwise (no reduction over the batch): the result of a patch cannot depend on its batch."""
    d = x.float().reshape(P, H, W, 16)[..., :4].permute(0, 3, 1, 2)
    z = [0 * d[:, 0], 0.02 * d[:, 0] - 0.01 * d[:, 1], 0.015 * d[:, 2] - 0.02 * d[:, 3]]
    m = torch.maximum(torch.maximum(z[0], z[1]), z[2])
    e = [torch.exp(v - m) for v in z]
    den = (e[0] + e[1]) + e[2]
    return torch.stack([v / den for v in e], dim=1).contiguous()


@pytest.fixture(scope="module")
def survey():
    egs = []
    for i, (n_pings, n_range) in enumerate(SURVEY):
        sv, labels, seabed = make_arrays(n_pings, n_range, seed=30 + i)
        if i == 4:
            labels[:] = 0                                                         # no labelled pixel at all
        egs.append(FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), seabed,
                                frequencies=FREQS, name=f"eg{i}"))
    return egs


def make_pipe(model):
    return types.SimpleNamespace(model=model.cuda().eval(), device=torch.device("cuda"), frequencies=FREQS)


@pytest.fixture(scope="module")
def stub_pipe():
    return make_pipe(pkg.UNet_Baseline(3, 4, start_filts=8, precision="f32x6"))


@pytest.mark.parametrize("patch,overlap", PATCHES)
def test_generator_equals_the_per_echogram_call_with_a_predictor_stub(survey, stub_pipe, patch, overlap):
    counts = [len(r.grid) for g in ti.iter_memm_groups(iter(survey), patch, overlap, 10 ** 9) for r in g]
    assert counts[2] == 1                                                         # the 17 x 17 echogram: a single patch
    batch = 8 if patch == (32, 32) else 3
    # a threshold that is crossed INSIDE an echogram's patch run (groups hold whole echograms: the group ends behind it)
    group_patches = counts[0] + counts[1] // 2
    groups = list(ti.plan_memm_groups(list(zip(counts, [0] * 7)), group_patches))
    assert len(groups) >= 2 and sum(c for c, _ in groups[0]) > group_patches
    assert any(sum(counts[:k]) % batch for k in range(1, 7))                     # a batch spans two echograms
    stats = {}
    got = list(ti.predict_echograms_memm(iter(survey), stub_pipe, patch, overlap, batch, predict_fn=stub_predict_fn,
                                         group_patches=group_patches, group_elems=SMALL, stats=stats))
    assert [eg for eg, _ in got] == survey                                        # input order, the same objects
    per_group = [sum(c for c, _ in g) for g in groups]
    assert stats["groups"] == len(groups) and stats["fallback_echograms"] == stats["solo_echograms"] == 0
    assert stats["batches"] == [min(batch, n - b0) for n in per_group for b0 in range(0, n, batch)]     # only a group's last is short
    for eg, out in got:
        want = ti.predict_echogram_memm(eg, stub_pipe, patch, overlap, batch, predict_fn=stub_predict_fn)
        assert out.dtype == np.float64 and out.shape == (2,) + tuple(eg.shape)
        assert np.array_equal(out, want), eg.name
        assert (out != 0).any() and (out == 0).any()


def test_an_echogram_larger_than_the_staging_takes_the_per_echogram_path_in_its_place(survey, stub_pipe):
    stats = {}
    cap = 130 * 64 + 17 * 17 + 1000                                               # the 300 x 90 echogram does not fit
    got = list(ti.predict_echograms_memm(iter(survey), stub_pipe, (32, 32), 4, 8, predict_fn=stub_predict_fn,
                                         group_elems=cap, stats=stats))
    assert [eg.name for eg, _ in got] == [eg.name for eg in survey] and stats["solo_echograms"] == 1
    for eg, out in got:
        assert np.array_equal(out, ti.predict_echogram_memm(eg, stub_pipe, (32, 32), 4, 8, predict_fn=stub_predict_fn))


def test_generator_consumes_its_echograms_lazily(stub_pipe):
    sv, labels, seabed = make_arrays(40, 50, seed=3)
    taken = []

    def source():
        for i in range(60):
            taken.append(i)
            yield FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), seabed,
                               frequencies=FREQS, name=f"e{i}")
    gen = ti.predict_echograms_memm(source(), stub_pipe, (32, 32), 4, 8, predict_fn=stub_predict_fn, group_patches=12,
                                    group_elems=SMALL)
    first = next(gen)
    assert first[0].name == "e0" and 0 < len(taken) < 30                          # a few groups ahead, not the survey
    names = ["e0"] + [eg.name for eg, _ in gen]
    assert names == [f"e{i}" for i in range(60)]


@pytest.mark.parametrize("precision", ["h3p", "bf16"])
def test_generator_with_the_real_network_is_within_one_float16_step(survey, precision):
    """Batches of another size and composition: eval forwards agree to ~1e-6 across batch sizes, which can move a float16
    rounding by one step (2**-11 just below 1.0) and no more."""
    model = pkg.UNet_Baseline(3, 4, start_filts=8, precision=precision)
    model.load_state_dict(synth.synth_state_dict(start_filts=8, seed=4))
    pipe = make_pipe(model)
    stats = {}
    got = list(ti.predict_echograms_memm(iter(survey), pipe, (64, 64), 6, 8, group_elems=SMALL, stats=stats))
    assert len(stats["batches"]) == 1 and stats["batches"][0] >= 16              # one packed batch, the two-stream forward
    worst, differing, total = 0.0, 0, 0
    for eg, out in got:
        want = ti.predict_echogram_memm(eg, pipe, (64, 64), 6, 8)
        assert np.array_equal(out != 0, want != 0) and (out != 0).any()
        d = np.abs(out - want)
        worst, differing, total = max(worst, float(d.max())), differing + int((d != 0).sum()), total + d.size
    print(f"{precision}: largest difference {worst:.3e}, differing pixels {differing} of {total} "
          f"({100.0 * differing / total:.4f} %)")
    assert worst <= 2 ** -11


def test_seabed_estimate_through_the_generator(survey, stub_pipe):
    def refuse(*a, **k):
        raise AssertionError("get_seabed was called")
    egs = []
    for i in (0, 1, 3, 5):                       # finite samples with a bright bottom echo: the estimate is a real line
        eg = survey[i]
        sv = np.nan_to_num(eg.sv, nan=1e-7, posinf=1e-7, neginf=1e-7)
        for x in range(eg.shape[1]):
            sv[:, min(int(eg._seabed[x]), eg.shape[0] - 2), x] = 5.0
        egs.append(FakeEchogram(sv, eg.labels, np.zeros_like(eg._seabed), frequencies=FREQS, name=eg.name))
    for eg in egs:
        eg.get_seabed = refuse
    got = list(ti.predict_echograms_memm(iter(egs), stub_pipe, (32, 32), 4, 8, predict_fn=stub_predict_fn,
                                         seabed="estimate", group_patches=40, group_elems=SMALL))
    assert len(got) == len(egs)
    for (eg, out), src in zip(got, egs):
        assert eg is src
        want = ti.predict_echogram_memm(eg, stub_pipe, (32, 32), 4, 8, predict_fn=stub_predict_fn, seabed="estimate")
        assert np.array_equal(out, want) and (out != 0).any()
    # a callable is asked once per echogram and its line is the one that masks
    line = lambda eg: np.full(eg.shape[1], 12, dtype=np.int64)                   # noqa: E731
    for eg, out in ti.predict_echograms_memm(iter(egs[:2]), stub_pipe, (32, 32), 4, 8, predict_fn=stub_predict_fn,
                                             seabed=line, group_elems=SMALL):
        assert np.array_equal(out, ti.predict_echogram_memm(eg, stub_pipe, (32, 32), 4, 8, predict_fn=stub_predict_fn,
                                                            seabed=line(eg)))


def with_metadata(eg, seed):
    n_pings = eg.shape[1]
    rng = np.random.Generator(np.random.PCG64(seed))
    tv = 737000.5 + np.cumsum(rng.uniform(5e-6, 9e-6, size=n_pings))
    eg = FakeEchogram(eg.sv, eg.labels, eg._seabed, frequencies=FREQS, name=eg.name)
    eg.portion_of_day_vector = tv % 1
    eg.portion_of_year_scalar = 0.61
    eg.time_vector_diff = np.concatenate((np.diff(tv), [tv[-1] - tv[-2]])) / 6e-6 - 1
    return eg


@pytest.mark.parametrize("kind", ["late", "early"])
def test_metadata_models_take_the_per_echogram_path(survey, kind):
    mc = {k: True for k in ti.META_FLAGS}
    if kind == "late":
        model = pkg.UNet_LateMetInject(3, 4, 7, depth=3, precision="f32x6")
        model.load_state_dict(synth.synth_state_dict(depth=3, seed=4, meta_in_channels=7))
    else:
        model = pkg.UNet_Baseline(3, 11, precision="f32x6")
        model.load_state_dict(synth.synth_state_dict(seed=3, in_channels=11))
    pipe = make_pipe(model)
    egs = [with_metadata(survey[i], 50 + i) for i in (3, 5, 0)]
    stats = {}
    got = list(ti.predict_echograms_memm(iter(egs), pipe, (64, 64), 6, 4, meta_channels=mc, stats=stats))
    assert stats["fallback_echograms"] == 3 and stats["groups"] == 0 and stats["batches"] == []
    assert [eg for eg, _ in got] == egs
    for eg, out in got:
        want = ti.predict_echogram_memm(eg, pipe, (64, 64), 6, 4, meta_channels=mc)
        assert np.array_equal(out, want) and (out != 0).any()


def test_save_predictions_memm_writes_one_file_per_echogram_and_resumes(survey, stub_pipe, tmp_path):
    calls = []

    def counting(x, P, H, W):
        calls.append(P)
        return stub_predict_fn(x, P, H, W)
    kw = dict(predict_fn=counting, group_patches=40, group_elems=SMALL)
    want = dict((eg.name, out) for eg, out in ti.predict_echograms_memm(iter(survey), stub_pipe, (32, 32), 4, 8, **kw))
    n_calls = len(calls)
    assert n_calls > 0
    assert ti.save_predictions_memm(iter(survey[:5]), stub_pipe, str(tmp_path), (32, 32), 4, 8, **kw) == 5
    assert sorted(os.listdir(tmp_path)) == sorted(eg.name + ".npy" for eg in survey[:5])
    # resume: only the two missing echograms are computed ...
    calls.clear()
    assert ti.save_predictions_memm(iter(survey), stub_pipe, str(tmp_path), (32, 32), 4, 8, resume=True, **kw) == 2
    assert 0 < len(calls) < n_calls
    # ... and a second call computes nothing
    calls.clear()
    assert ti.save_predictions_memm(iter(survey), stub_pipe, str(tmp_path), (32, 32), 4, 8, resume=True, **kw) == 0
    assert calls == []
    for eg in survey:
        assert np.array_equal(np.load(os.path.join(tmp_path, eg.name + ".npy")), want[eg.name])
    # an empty survey, and one of which everything exists: nothing is computed (and no staging is set up)
    assert ti.save_predictions_memm(iter([]), stub_pipe, str(tmp_path), (32, 32), 4, 8, **kw) == 0 and calls == []
    # resume=False writes every file again
    assert ti.save_predictions_memm(iter(survey[:2]), stub_pipe, str(tmp_path), (32, 32), 4, 8, resume=False, **kw) == 2
    assert sum(calls) > 0
