"""GPU: survey-level memm evaluation -- batches packed from several echograms (tiled_inference.evaluate_echograms_memm).

  * the four multi-source entry points of the evaluation chain against their single-source kernels, bit for bit;
  * the packed path against the sum of evaluate_echogram_memm per echogram (predictor stub: equal integers; real network:
    the measured self-difference of the per-echogram path, twice);
  * the per-echogram cases (metadata models, an echogram larger than the staging), validate_model_survey_memm(tiled=True)."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import evaluate, hip, synth  # noqa: E402
from crimac_classifiers_unet_amd import tiled_inference as ti  # noqa: E402
from crimac_classifiers_unet_amd.hip import call, ptr  # noqa: E402
from crimac_classifiers_unet_amd.pipeline import SegPipe  # noqa: E402
from test_gpu_memm_survey import C, EXTENTS, FREQS, PATCHES, SMALL, STORAGE, make_arrays, raw, with_metadata  # noqa: E402
from test_gpu_survey_eval import moved_share, stub_predict_fn  # noqa: E402
from tools.fake_reader import FakeEchogram  # noqa: E402

pytestmark = pytest.mark.gpu

# Measured on an MI355X: evaluate_echogram_memm (UNet_Baseline depth 3, 'h3p', synthetic weights) over the four echograms
# of this file against ITSELF with internal batches of 8 and of 32 patches (test_real_network_..., which prints them),
# 64 x 64 patches: share of the valid pixels that change their float16 bin, largest difference of a sandeel probability.
# Both 0: an eval-mode forward does not depend on the batch it runs in -- so the packed path, which cuts its batches
# differently again (allowed: twice these), must give the same bins and the same probabilities.
SELF_MOVED_SHARE = 0.0
SELF_PROB_DIFF = 0.0

# school boxes (y0, y1, x0, x1) per echogram, not yet extended: the same box in echograms 0 and 3, none in echogram 2
# (whose 17 x 17 extent that box would cover entirely)
BOXES = [[(5, 40, 5, 60), (50, 80, 200, 290)], [(100, 150, 10, 30)], [], [(5, 40, 5, 60), (30, 60, 90, 125)]]
MODES = ["all", "region", "trace"]
DEV = "cuda"


def extended(boxes, n_range, mode="region", size=20):
    eg = types.SimpleNamespace(get_object_bounding_boxes=lambda: np.array(boxes, dtype=np.int64).reshape(-1, 4),
                               shape=(n_range, 0))
    return ti.eval_boxes(eg, mode, size)


@pytest.fixture(scope="module")
def sources():
    """The four echograms, resident as the single-source kernels take them, made once."""
    out = []
    for i, (n_pings, n_range) in enumerate(EXTENTS):
        sv, labels, seabed = make_arrays(n_pings, n_range, seed=10 + i)
        out.append(types.SimpleNamespace(
            n_pings=n_pings, n_range=n_range, sv=sv, labels=labels, seabed=seabed,
            data=torch.from_numpy(sv).to(DEV), lab=torch.from_numpy(labels).to(DEV),
            sb=torch.from_numpy(seabed.astype(np.int32)).to(DEV)))
    return out


@pytest.fixture(scope="module")
def echograms(sources):
    return [FakeEchogram(np.ascontiguousarray(s.sv.transpose(0, 2, 1)), np.ascontiguousarray(s.labels.T), s.seabed,
                         frequencies=FREQS, name=f"eg{i}", boxes=BOXES[i]) for i, s in enumerate(sources)]


def desc_table(sources, seabeds):
    rows = [(s.data.data_ptr(), s.lab.data_ptr(), 0 if seabeds[i] is None else seabeds[i].data_ptr(), 0, s.n_pings,
             s.n_range) for i, s in enumerate(sources)]
    t = torch.tensor(rows, dtype=torch.int64)
    assert t.shape[1] == hip.MEMM_DESC_WORDS
    return t.to(DEV)


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


SENT_F, SENT_L = -7.0, 77
TAIL = 3                   # rows past P that must keep the sentinel


@pytest.mark.parametrize("patch,overlap", PATCHES)
def test_the_multi_source_chain_equals_the_single_source_kernels_bit_for_bit(sources, patch, overlap):
    pw, ph = patch
    cen, src = edge_patches(sources, ph, pw)
    P, n = len(cen), len(sources)
    cen_d, src_d = torch.from_numpy(cen).to(DEV), torch.from_numpy(src).to(DEV)
    cen64 = cen_d.long().contiguous()
    lines = [s.sb for s in sources]
    lines[1] = None                                          # a NULL seabed: no seabed rule for that echogram
    table = desc_table(sources, lines)
    bad = torch.tensor([n, -1], dtype=torch.int32, device=DEV)      # a src outside the table: skipped
    idx = [np.nonzero(src == i)[0] for i in range(n)]
    idx_d = [torch.from_numpy(ix).to(DEV) for ix in idx]
    assert all(len(ix) for ix in idx)

    # ---- crimac_gather_eval_crops_multi ------------------------------------------------------------------------------
    crop = torch.full((P + TAIL, C, ph, pw), SENT_F, dtype=torch.float32, device=DEV)
    lab = torch.full((P + TAIL, ph, pw), SENT_L, dtype=torch.int16, device=DEV)
    call("crimac_gather_eval_crops_multi", ptr(table), n, ptr(src_d), C, ptr(cen_d), P, ph, pw, ptr(crop), ptr(lab))
    assert bool((crop[P:] == SENT_F).all()) and bool((lab[P:] == SENT_L).all())
    for i, s in enumerate(sources):
        k = len(idx[i])
        want_d = torch.empty((k, C, ph, pw), dtype=torch.float32, device=DEV)
        want_l = torch.empty((k, ph, pw), dtype=torch.int16, device=DEV)
        own_cen = cen_d[idx_d[i]].contiguous()       # (named: a temporary's memory is free for the next allocation)
        call("crimac_gather_eval_crops", ptr(s.data), C, s.n_pings, s.n_range, ptr(s.lab), ptr(own_cen), k, ph, pw, 1,
             ptr(want_d), ptr(want_l))
        assert torch.equal(crop[idx_d[i]].view(torch.int32), want_d.view(torch.int32)), i
        assert torch.equal(lab[idx_d[i]], want_l), i
    assert bool((lab[:P] == -100).any()) and bool((lab[:P] > 0).any()) and bool((crop[:P] != 0).any())
    two_d = torch.full((2, C, ph, pw), SENT_F, dtype=torch.float32, device=DEV)
    two_l = torch.full((2, ph, pw), SENT_L, dtype=torch.int16, device=DEV)
    call("crimac_gather_eval_crops_multi", ptr(table), n, ptr(bad), C, ptr(cen_d), 2, ph, pw, ptr(two_d), ptr(two_l))
    assert bool((two_d == SENT_F).all()) and bool((two_l == SENT_L).all())
    crop, lab = crop[:P].contiguous(), lab[:P].contiguous()
    # the batch of every source on its own, as the single-source kernels take it
    own = [types.SimpleNamespace(cen=cen_d[ix].contiguous(), cen64=cen64[ix].contiguous(), crop=crop[ix].contiguous(),
                                 lab=lab[ix].contiguous()) for ix in idx_d]

    # ---- crimac_labels_test_transform_multi ----------------------------------------------------------------------------
    thr = (C - 1, 1e-7, 1e-4)
    lt = torch.full((P + TAIL, ph, pw), SENT_L, dtype=torch.int16, device=DEV)
    call("crimac_labels_test_transform_multi", ptr(lab), 2, ptr(crop), *thr, ptr(cen64), ptr(table), n, ptr(src_d),
         ti.SEABED_PAD, overlap, ptr(lt), P, C, ph, pw)
    assert bool((lt[P:] == SENT_L).all())
    for i, s in enumerate(sources):
        k = len(idx[i])
        want = torch.empty((k, ph, pw), dtype=torch.int16, device=DEV)
        call("crimac_labels_test_transform", ptr(own[i].lab), 2, ptr(own[i].crop), *thr, ptr(own[i].cen64), ptr(lines[i]), 0,
             0 if lines[i] is None else s.n_pings, None, 0, 0, s.n_range, ti.SEABED_PAD, 1, overlap, ptr(want), k, C, ph, pw)
        assert torch.equal(lt[idx_d[i]], want), i
    assert bool((lt[idx_d[0]] == -50).any()) and bool((lt[idx_d[3]] == -50).any())       # the seabed lines cut patches
    assert not bool((lt[idx_d[1]] == -50).any())                                            # ... and a NULL line none
    two_l.fill_(SENT_L)
    call("crimac_labels_test_transform_multi", ptr(lab), 2, ptr(crop), *thr, ptr(cen64), ptr(table), n, ptr(bad),
         ti.SEABED_PAD, overlap, ptr(two_l), 2, C, ph, pw)
    assert bool((two_l == SENT_L).all())
    lt = lt[:P].contiguous()

    # ---- crimac_labels_extend_mask_multi -------------------------------------------------------------------------------
    per = [extended(BOXES[i], s.n_range) for i, s in enumerate(sources)]
    off, rows = ti.memm_box_table(per)
    off_d, rows_d = torch.from_numpy(off).to(DEV), torch.from_numpy(rows).to(DEV)
    lm = torch.cat([lt, torch.full((TAIL, ph, pw), SENT_L, dtype=torch.int16, device=DEV)])
    call("crimac_labels_extend_mask_multi", ptr(lm), ptr(crop), C, ptr(cen64), ptr(rows_d), ptr(off_d), n, ptr(src_d), -1, P,
         ph, pw)
    assert bool((lm[P:] == SENT_L).all())
    for i, s in enumerate(sources):
        k = len(idx[i])
        want = lt[idx_d[i]].contiguous()
        bx = torch.from_numpy(per[i]).to(DEV)
        call("crimac_labels_extend_mask", ptr(want), ptr(own[i].crop), C, ptr(own[i].cen64), ptr(bx) if len(per[i]) else None,
             len(per[i]), -1, k, ph, pw)
        assert torch.equal(lm[idx_d[i]], want), i
    # the box shared by the tables of echograms 0 and 3 covers echogram 2's extent as well, and is not in its table:
    # nothing of echogram 2 stays unmasked, something of echograms 0 and 3 does
    assert bool(torch.isin(lm[idx_d[2]], torch.tensor([-1, -100], dtype=torch.int16, device=DEV)).all())
    assert all(bool((lm[idx_d[i]] >= 0).any()) for i in (0, 3))
    two_l.fill_(SENT_L)
    call("crimac_labels_extend_mask_multi", ptr(two_l), ptr(crop), C, ptr(cen64), ptr(rows_d), ptr(off_d), n, ptr(bad), -1, 2,
         ph, pw)
    assert bool((two_l == SENT_L).all())
    lm = lm[:P].contiguous()
    assert bool((lm == -100).any()) and bool((lm == -1).any())

    # ---- crimac_gather_patches_memm_labels_multi, every storage type ----------------------------------------------------
    rows_px = ph * pw
    for prec, dtype in STORAGE.items():
        code = hip.PREC_NAMES[prec]
        x = torch.empty(((P + TAIL) * rows_px, 16), dtype=dtype, device=DEV)
        raw(x).fill_(0x5A5A)
        call("crimac_gather_patches_memm_labels_multi", code, ptr(table), n, ptr(src_d), C, ptr(cen_d), P, ph, pw, ptr(x), 16,
             ptr(lm))
        got = raw(x).view(P + TAIL, rows_px, -1)
        assert bool((got[P:] == 0x5A5A).all()), prec
        for i, s in enumerate(sources):
            k = len(idx[i])
            want = torch.empty((k * rows_px, 16), dtype=dtype, device=DEV)
            own_lm = lm[idx_d[i]].contiguous()
            call("crimac_gather_patches_memm_labels", code, ptr(s.data), C, s.n_pings, s.n_range, ptr(own[i].cen), k, ph, pw,
                 ptr(want), 16, ptr(own_lm), 0, 0, 0.0, None, 0, None, 0, None, 0, None)
            assert torch.equal(got[idx_d[i]], raw(want).view(k, rows_px, -1)), (prec, i)
        assert bool((got[:P] != 0).any())
    x = torch.zeros((2 * rows_px, 16), dtype=torch.float32, device=DEV)
    call("crimac_gather_patches_memm_labels_multi", hip.PREC_F32X6, ptr(table), n, ptr(bad), C, ptr(cen_d), 2, ph, pw, ptr(x),
         16, ptr(lm))
    assert bool((x == 0).all())


# ---- the path ----------------------------------------------------------------------------------------------------------
def make_pipe(model):
    return types.SimpleNamespace(model=model.to(DEV).eval(), device=torch.device(DEV), frequencies=FREQS)


@pytest.fixture(scope="module")
def stub_pipe():
    pipe = make_pipe(pkg.UNet_Baseline(3, 4, start_filts=8, precision="f32x6"))
    pipe.fn = stub_predict_fn(pipe.model.infer_engine)
    return pipe


class Labels:
    """on_batch hook: the transformed labels (and, ``probs``, the sandeel probabilities) of every patch, keyed by
    (echogram, centre); ``batches``: the echograms every batch holds."""

    def __init__(self, eg=None, probs=False):
        self.eg, self.probs, self.rows, self.batches = eg, probs, {}, []

    def __call__(self, centres, labels, logits, *, echograms=None):
        lab = labels.cpu().numpy()
        sm = torch.softmax(logits, 1)[:, 1].cpu().numpy() if self.probs else [None] * len(lab)
        egs = [self.eg] * len(lab) if echograms is None else echograms
        assert len(egs) == len(lab) == len(centres) == logits.shape[0]
        self.batches.append({eg.name for eg in egs})
        for c, l, s, eg in zip(centres, lab, sm, egs):
            self.rows.setdefault((eg.name, int(c[0]), int(c[1])), []).append((l, s))


def loop_sum(echograms, pipe, patch, overlap, batch, probs=False, **kw):
    """The yardstick: evaluate_echogram_memm per echogram, summed; + the hook's rows of all echograms."""
    hp = hn = 0
    rows = {}
    seabed = kw.pop("seabed", None)
    for eg in echograms:
        hook = Labels(eg, probs)
        a, b = ti.evaluate_echogram_memm(eg, pipe, patch, overlap, batch, on_batch=hook,
                                         seabed=seabed(eg) if callable(seabed) else seabed, **kw)
        hp, hn = hp + a, hn + b
        rows.update(hook.rows)
    return (hp, hn), rows


def flat_line(eg):
    return np.full(eg.shape[1], 12, dtype=np.int64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("patch,overlap", PATCHES)
def test_packed_path_equals_the_sum_of_the_per_echogram_calls_with_a_predictor_stub(echograms, stub_pipe, patch, overlap, mode):
    batch = 8 if patch == (32, 32) else 3
    for seabed in (None, "estimate", flat_line):
        counts = [len(r.grid) for g in ti.iter_memm_groups(iter(echograms), patch, overlap, 10 ** 9, seabed=seabed,
                                                           device=stub_pipe.device) for r in g]
        group_patches = counts[0] + counts[1] // 2           # crossed inside echogram 1's run: the group ends behind it
        per_group = [sum(c for c, _ in g) for g in ti.plan_memm_groups(list(zip(counts, [0] * 4)), group_patches)]
        assert len(per_group) >= 2
        want, want_rows = loop_sum(echograms, stub_pipe, patch, overlap, batch, eval_mode=mode, predict_fn=stub_pipe.fn,
                                   seabed=seabed)
        stats, hook = {}, Labels()
        got = ti.evaluate_echograms_memm(iter(echograms), stub_pipe, patch, overlap, batch, eval_mode=mode,
                                         predict_fn=stub_pipe.fn, seabed=seabed, on_batch=hook, group_patches=group_patches,
                                         group_elems=SMALL, stats=stats)
        assert got[0].dtype == got[1].dtype == np.int64
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (seabed, mode)
        assert got[0].sum() > 0 and got[1].sum() > 1000
        assert stats["groups"] == len(per_group) and stats["fallback_echograms"] == stats["solo_echograms"] == 0
        assert stats["batches"] == [min(batch, n - b0) for n in per_group for b0 in range(0, n, batch)]   # only a group's last is short
        assert any(len(b) >= 2 for b in hook.batches)                                 # a batch spans echograms
        assert hook.rows.keys() == want_rows.keys()
        for key, ls in hook.rows.items():
            assert len(ls) == len(want_rows[key])
            assert all(np.array_equal(a[0], b[0]) for a, b in zip(ls, want_rows[key])), key
    # a callback that does not declare the keyword gets the three arguments it always got
    seen = []
    ti.evaluate_echograms_memm(iter(echograms[2:]), stub_pipe, patch, overlap, batch, eval_mode=mode, predict_fn=stub_pipe.fn,
                               on_batch=lambda cen, lab, logits: seen.append(len(cen)), group_elems=SMALL)
    assert sum(seen) > 0
    ti.release_staging()


def test_hist_given_accumulates_without_finishing(echograms, stub_pipe):
    want, _ = loop_sum(echograms, stub_pipe, (32, 32), 4, 8, predict_fn=stub_pipe.fn)
    hist = torch.ones(2, ti.PR_BINS, dtype=torch.int32, device=DEV)
    out = ti.evaluate_echograms_memm(echograms, stub_pipe, (32, 32), 4, 8, predict_fn=stub_pipe.fn, hist=hist,
                                     group_elems=SMALL)
    assert out is hist
    h = hist.cpu().numpy().astype(np.int64) - 1
    assert np.array_equal(h[0], want[0]) and np.array_equal(h[1], want[1])
    ti.release_staging()


# ---- per-echogram cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["late", "early"])
def test_metadata_models_take_the_per_echogram_path(echograms, kind):
    mc = {k: True for k in ti.META_FLAGS}
    if kind == "late":
        model = pkg.UNet_LateMetInject(3, 4, 7, depth=3, precision="f32x6")
        model.load_state_dict(synth.synth_state_dict(depth=3, seed=4, meta_in_channels=7))
    else:
        model = pkg.UNet_Baseline(3, 11, precision="f32x6")
        model.load_state_dict(synth.synth_state_dict(seed=3, in_channels=11))
    pipe = make_pipe(model)
    egs = []
    for i in (3, 1, 0):
        eg = with_metadata(echograms[i], 50 + i)
        eg.object_bounding_boxes = echograms[i].object_bounding_boxes
        egs.append(eg)
    want, _ = loop_sum(egs, pipe, (64, 64), 6, 4, eval_mode="region", meta_channels=mc)
    stats, hook = {}, Labels()
    got = ti.evaluate_echograms_memm(iter(egs), pipe, (64, 64), 6, 4, eval_mode="region", meta_channels=mc, stats=stats,
                                     on_batch=hook)
    assert stats["fallback_echograms"] == len(egs) and stats["groups"] == 0 and stats["batches"] == []
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].sum() > 1000
    assert all(len(b) == 1 for b in hook.batches) and {n for b in hook.batches for n in b} == {eg.name for eg in egs}


def test_solo_echogram_empty_survey_and_refused_arguments(echograms, stub_pipe):
    kw = dict(predict_fn=stub_pipe.fn, eval_mode="region")
    want, _ = loop_sum(echograms, stub_pipe, (32, 32), 4, 8, **kw)
    stats = {}
    cap = 130 * 64 + 17 * 17 + 1000                                               # the 300 x 90 echogram does not fit
    got = ti.evaluate_echograms_memm(iter(echograms), stub_pipe, (32, 32), 4, 8, group_elems=cap, stats=stats, **kw)
    assert stats["solo_echograms"] == 1 and stats["fallback_echograms"] == 0 and stats["groups"] >= 2
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    stats = {}
    hp, hn = ti.evaluate_echograms_memm(iter([]), stub_pipe, (32, 32), 4, 8, stats=stats, **kw)
    assert hp.shape == hn.shape == (ti.PR_BINS,) and hp.dtype == np.int64 and not hp.any() and not hn.any()
    assert stats == dict(groups=0, batches=[], fallback_echograms=0, solo_echograms=0)
    with pytest.raises(TypeError, match="group_patches"):
        ti.evaluate_echograms_memm(iter(echograms), stub_pipe, (32, 32), 4, 8, group_patch=40, **kw)
    with pytest.raises(TypeError, match="callable"):
        ti.evaluate_echograms_memm(iter(echograms), stub_pipe, (32, 32), 4, 8, seabed=echograms[0]._seabed, **kw)
    ti.release_staging()


# ---- real network --------------------------------------------------------------------------------------------------------
def prob_diff(a, b):
    assert a.keys() == b.keys()
    return max(float(np.abs(x[1] - y[1]).max()) for k in a for x, y in zip(a[k], b[k]))


@pytest.mark.parametrize("patch,overlap", PATCHES[1:])          # (64, 64): 16 x 16 at the bottom of a depth-3 network
def test_real_network_packed_against_the_loop(echograms, patch, overlap, monkeypatch):
    """UNet_Baseline(depth 3, 'h3p', synthetic weights): the packed path against the loop over evaluate_echogram_memm.  The
    totals of both histograms are equal exactly (same pixels, same labels).  Bins and probabilities may differ through
    batch composition only: the loop against itself with internal batches of 8 and of 32 patches moves a share of
    SELF_MOVED_SHARE of the valid pixels to another float16 bin and changes a sandeel probability by at most
    SELF_PROB_DIFF (measured on an MI355X, printed here, constants above; both 0.0); allowed: twice that, i.e. equality."""
    model = pkg.UNet_Baseline(3, 4, depth=3, precision="h3p")
    model.load_state_dict(synth.synth_state_dict(depth=3, seed=4))
    pipe = make_pipe(model)
    runs = {}
    for ib in (8, 32):
        monkeypatch.setattr(ti, "INTERNAL_BATCH", ib)
        runs[ib] = loop_sum(echograms, pipe, patch, overlap, 4, probs=True)
    monkeypatch.undo()
    self_moved, self_diff = moved_share(runs[8][0], runs[32][0]), prob_diff(runs[8][1], runs[32][1])
    print(f"loop, internal batch 8 vs 32 {patch}: moved share {self_moved:.3e}, largest probability difference {self_diff:.3e}")
    want, want_rows = loop_sum(echograms, pipe, patch, overlap, 4, probs=True)
    stats, hook = {}, Labels(probs=True)
    got = ti.evaluate_echograms_memm(iter(echograms), pipe, patch, overlap, 4, on_batch=hook, group_elems=SMALL, stats=stats)
    moved, diff = moved_share(want, got), prob_diff(want_rows, hook.rows)
    print(f"packed vs loop {patch}: moved share {moved:.3e}, largest probability difference {diff:.3e}, "
          f"batches {stats['batches']}")
    assert any(len(b) >= 2 for b in hook.batches) and stats["fallback_echograms"] == stats["solo_echograms"] == 0
    assert got[0].sum() == want[0].sum() and got[1].sum() == want[1].sum()
    assert got[0].sum() > 0 and got[1].sum() > 1000
    assert moved <= 2 * SELF_MOVED_SHARE, moved
    assert diff <= 2 * SELF_PROB_DIFF, diff
    if SELF_MOVED_SHARE == 0.0:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ti.release_staging()


# ---- the public function -----------------------------------------------------------------------------------------------------
def test_validate_model_survey_memm_tiled_writes_the_csv_of_the_summed_histograms(echograms, stub_pipe, tmp_path, monkeypatch):
    pipe = object.__new__(SegPipe)
    pipe.model, pipe.device, pipe.frequencies, pipe.model_is_loaded = stub_pipe.model, stub_pipe.device, FREQS, True
    want, _ = loop_sum(echograms, stub_pipe, (32, 32), 4, 8, eval_mode="region", predict_fn=stub_pipe.fn)
    os.makedirs(tmp_path / "want")
    m_want = pipe.validate_model_testing_from_histograms(*want, save_path_metrics=str(tmp_path / "want" / "s_test.csv"),
                                                         save_path_plot=None)
    stats = {}
    # (the public function takes no predictor: the stub and the small groups go in underneath it)
    monkeypatch.setattr(ti, "evaluate_echograms_memm",
                        functools.partial(ti.evaluate_echograms_memm, predict_fn=stub_pipe.fn, group_patches=60,
                                          group_elems=SMALL, stats=stats))
    m = evaluate.validate_model_survey_memm(echograms, pipe, {}, (32, 32), 4, "region", 8, 0, str(tmp_path), None,
                                            survey="s", tiled=True)
    assert stats["groups"] >= 2 and stats["fallback_echograms"] == 0
    assert all(np.array_equal(m[k], m_want[k], equal_nan=True) for k in ("precision", "recall", "thresholds", "F1"))
    assert open(tmp_path / "s_test.csv").read() == open(tmp_path / "want" / "s_test.csv").read()
    assert len(m["F1"]) > 2
    ti.release_staging()
