"""GPU: the scored integration of a packed memm survey (``crimac_integrate_confusion_multi``,
``crimac_eval_crop_origins_multi``, ``ScoredIntegrationSet``).

  a. the kernel against a numpy float64 reference per echogram, at the shapes of test_gpu_scored_integration.py;
  b. one multi launch against one single-source launch per echogram, bit for bit;
  c. the multi origins against the single-source origins per echogram;
  d. ``evaluate_echograms_memm(..., integration=ScoredIntegrationSet(spec))`` against the loop over
     ``evaluate_echogram_memm(..., integration=ScoredIntegration(spec))`` with a predictor stub;
  e. the same with a real network."""
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
from test_gpu_memm_survey import EXTENTS, PATCHES, SMALL  # noqa: E402
from test_gpu_memm_survey_eval import SELF_MOVED_SHARE, echograms, edge_patches, make_pipe, sources, stub_pipe  # noqa: E402, F401
from test_gpu_scored_integration import FMAX, GUARD, bin_reference, close  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ---- a, b. the kernel --------------------------------------------------------------------------------------------------------
PH, PW, PING_BIN, RANGE_BIN = 24, 40, 7, 5
N_RANGE = (37, 17, 64)                    # 17 < PH: a water column not deeper than the patch
N_PB = (9, 6, 4)
N_DESC = 3
#          (src, (row, ping) of pixel (0, 0) in the patch's own echogram)
PATCHES_A = [(0, (3, 5)),                 # straddles cells
             (1, (3, 5)),                 # the same origin in another echogram
             (2, (-10, -13)),             # off the top-left
             (0, (12, 21)),               # overlaps patch 0 of the same echogram
             (-1, (3, 5)),                # names no echogram: skipped
             (1, (-4, 20)),               # above row 0, below n_range = 17 and past the last ping (42)
             (2, (50, 10)),               # below n_range = 64 and past the last ping (28)
             (0, (20, 40)),               # below n_range = 37 and past the last ping (63)
             (N_DESC, (10, 14)),          # names no echogram: skipped
             (1, (0, -13)),               # off the left edge
             (2, (10, 14)),               # on cell edges
             (0, (-10, -13))]             # off the top-left
SRC_A = np.array([s for s, _ in PATCHES_A], dtype=np.int32)
ORG_A = np.array([o for _, o in PATCHES_A], dtype=np.int32)
P_A = len(PATCHES_A)
SKIPPED = [p for p in range(P_A) if not 0 <= SRC_A[p] < N_DESC]
BLOCK = [9 * N_PB[e] * -(-N_RANGE[e] // RANGE_BIN) for e in range(N_DESC)]      # words of every echogram's share
FIRST = [3, 3 + BLOCK[0] + 7, 3 + BLOCK[0] + 7 + BLOCK[1] + 13]                  # unequal gaps in front of every share
WORDS = FIRST[2] + BLOCK[2] + 5
ACC_FILL, CNT_FILL, SCRATCH_FILL = -7.0, -7, 12345.0


def shape_of(e):
    return (3, 3, N_PB[e], -(-N_RANGE[e] // RANGE_BIN))


@pytest.fixture(scope="module")
def kernel_case():
    rng = np.random.Generator(np.random.PCG64(7))
    sv = np.power(10.0, rng.uniform(-7, 0, size=(P_A, 2, PH, PW))).astype(np.float32)
    sv[:, 0] = 777.0                                         # the plane that is NOT asked for
    junk = rng.random((P_A, PH, PW))
    for lo, v in ((0.00, np.nan), (0.03, np.inf), (0.06, -np.inf), (0.09, 0.0), (0.12, -1e-3), (0.15, FMAX)):
        sv[:, 1][(junk >= lo) & (junk < lo + 0.03)] = v
    labels = rng.choice(np.array([-100, -1, -50, 0, 1, 2], dtype=np.int16), size=(P_A, PH, PW),
                        p=[0.1, 0.1, 0.1, 0.3, 0.2, 0.2])
    for p in range(P_A):                                     # valid labels on the off-grid pixels
        if p in SKIPPED:
            continue
        e = SRC_A[p]
        gy, gx = ORG_A[p, 0] + np.arange(PH)[:, None], ORG_A[p, 1] + np.arange(PW)[None, :]
        labels[p][(gy < 0) | (gy >= N_RANGE[e]) | (gx < 0) | (gx >= N_PB[e] * PING_BIN)] = 1
    logits = rng.choice(np.array([-4.0, 0.0, 4.0], dtype=np.float32), size=(P_A, 3, PH, PW))
    idx = [np.nonzero(SRC_A == e)[0] for e in range(N_DESC)]
    assert [len(ix) for ix in idx] == [4, 3, 3] and (SRC_A[1:] != SRC_A[:-1]).all()
    assert (ORG_A[0] == ORG_A[1]).all() and SRC_A[0] != SRC_A[1]

    def reference(ix, n_range, n_pb, mode):
        return bin_reference(logits[ix], lambda p, gy, gx, inside: sv[ix[p], 1], labels[ix], ORG_A[ix], n_range, PING_BIN,
                             RANGE_BIN, n_pb, mode, (0.5, 0.5))
    ref = {mode: [reference(idx[e], N_RANGE[e], N_PB[e], mode) for e in range(N_DESC)] for mode in (0, 1)}
    for mode in (0, 1):
        for e, (_, cnt) in enumerate(ref[mode]):
            assert cnt.shape == shape_of(e)
            assert (cnt[:, 2].sum(axis=(1, 2)) > 0).all(), "an annotated class without pixels"
            assert cnt[:, 0].sum() > 0 and cnt[:, 1].sum() > 0, "a predicted plane without pixels"
    for p in SKIPPED:                                        # what a skipped patch would have counted in echogram 0
        _, cnt = reference(np.array([p]), N_RANGE[0], N_PB[0], 0)
        assert cnt[:, 2].sum() > 100
    table = torch.tensor([(0, 0, 0, 0, N_PB[e] * PING_BIN, N_RANGE[e]) for e in range(N_DESC)], dtype=torch.int64)
    assert table.shape[1] == hip.MEMM_DESC_WORDS
    shares = torch.tensor([(FIRST[e], N_PB[e]) for e in range(N_DESC)], dtype=torch.int64)
    dev = {"logits": torch.from_numpy(logits).to(DEV), "sv": torch.from_numpy(sv).to(DEV),
           "labels": torch.from_numpy(labels).to(DEV), "origins": torch.from_numpy(ORG_A).to(DEV),
           "src": torch.from_numpy(SRC_A).to(DEV), "table": table.to(DEV), "shares": shares.to(DEV)}
    return dev, ref, idx


def run_multi(dev, mode, launches=1):
    """-> the shares [(acc, cnt)] per echogram; the guards, the gaps between the shares and the slots of the skipped
    patches are checked on the way."""
    words = ti.confusion_scratch_bytes(P_A, PH, PW, PING_BIN, RANGE_BIN) // 8
    per_patch = words // P_A
    acc = torch.full((WORDS + 2 * GUARD,), ACC_FILL, dtype=torch.float64, device=DEV)
    cnt = torch.full((WORDS + 2 * GUARD,), CNT_FILL, dtype=torch.int64, device=DEV)
    scratch = torch.full((words + 2 * GUARD,), SCRATCH_FILL, dtype=torch.float64, device=DEV)
    own = torch.zeros(WORDS + 2 * GUARD, dtype=torch.bool, device=DEV)
    for e in range(N_DESC):
        own[GUARD + FIRST[e]:GUARD + FIRST[e] + BLOCK[e]] = True
    acc[own], cnt[own] = 0, 0
    for _ in range(launches):
        call("crimac_integrate_confusion_multi", ptr(dev["logits"]), 3, ptr(dev["sv"]), 2, 1, ptr(dev["labels"]),
             ptr(dev["origins"]), ptr(dev["table"]), N_DESC, ptr(dev["src"]), ptr(dev["shares"]), P_A, PH, PW, PING_BIN,
             RANGE_BIN, 0.5, 0.5, mode, ptr(acc, GUARD), ptr(cnt, GUARD), ptr(scratch, GUARD), words * 8)
    torch.cuda.synchronize()
    assert bool((acc[~own] == ACC_FILL).all()) and bool((cnt[~own] == CNT_FILL).all()), "a word outside the shares was written"
    assert bool((scratch[:GUARD] == SCRATCH_FILL).all()) and bool((scratch[-GUARD:] == SCRATCH_FILL).all())
    for p in SKIPPED:
        assert bool((scratch[GUARD + p * per_patch:GUARD + (p + 1) * per_patch] == SCRATCH_FILL).all()), "a skipped patch wrote"
    acc, cnt = acc[GUARD:-GUARD].cpu().numpy(), cnt[GUARD:-GUARD].cpu().numpy()
    return [(acc[FIRST[e]:FIRST[e] + BLOCK[e]].reshape(shape_of(e)), cnt[FIRST[e]:FIRST[e] + BLOCK[e]].reshape(shape_of(e)))
            for e in range(N_DESC)]


def run_single(dev, idx, e, mode):
    """crimac_integrate_confusion over echogram e's patches of the batch, in batch order, from zeroed accumulators."""
    ix = torch.from_numpy(idx[e]).to(DEV)
    logits, sv, labels, origins = (dev[k][ix].contiguous() for k in ("logits", "sv", "labels", "origins"))
    acc = torch.zeros(shape_of(e), dtype=torch.float64, device=DEV)
    cnt = torch.zeros(shape_of(e), dtype=torch.int64, device=DEV)
    scratch = torch.empty(ti.confusion_scratch_bytes(len(ix), PH, PW, PING_BIN, RANGE_BIN) // 8, dtype=torch.float64, device=DEV)
    call("crimac_integrate_confusion", ptr(logits), 3, ptr(sv), 2, 1, ptr(labels), ptr(origins), len(ix), PH, PW, N_RANGE[e],
         PING_BIN, RANGE_BIN, N_PB[e], 0.5, 0.5, mode, ptr(acc), ptr(cnt), ptr(scratch), scratch.numel() * 8)
    return acc.cpu().numpy(), cnt.cpu().numpy()


def test_kernel_threshold_mode_against_float64(kernel_case):
    dev, ref, _ = kernel_case
    for e, (acc, cnt) in enumerate(run_multi(dev, 0)):
        ref_acc, ref_cnt = ref[0][e]
        assert np.array_equal(cnt, ref_cnt), e
        assert close(acc, ref_acc, 1e-12), (e, float(np.abs(acc - ref_acc).max()))


def test_kernel_probability_mode_against_float64(kernel_case):
    dev, ref, _ = kernel_case
    for e, (acc, cnt) in enumerate(run_multi(dev, 1)):
        ref_acc, ref_cnt = ref[1][e]
        assert np.array_equal(cnt, ref_cnt), e                # (every probability of logits in {-4, 0, 4} is > 0)
        assert close(acc, ref_acc, 2.0 ** -10 + 1e-12), (e, float(np.abs(acc - ref_acc).max()))
        assert close(acc[:, 2], ref_acc[:, 2], 1e-12), e      # the `all` plane carries no weight


@pytest.mark.parametrize("mode", [0, 1])
def test_multi_equals_single_bit_for_bit(kernel_case, mode):
    dev, ref, idx = kernel_case
    multi = run_multi(dev, mode)
    for e in range(N_DESC):
        acc, cnt = run_single(dev, idx, e, mode)
        assert np.array_equal(multi[e][1], cnt), e
        assert np.array_equal(multi[e][0].view(np.uint64), acc.view(np.uint64)), e
    twice, again = run_multi(dev, mode, launches=2), run_multi(dev, mode)
    for e in range(N_DESC):
        assert np.array_equal(twice[e][1], 2 * ref[mode][e][1]) and close(twice[e][0], 2 * multi[e][0], 1e-15), e
        assert np.array_equal(again[e][0].view(np.uint64), multi[e][0].view(np.uint64)), e
        assert np.array_equal(again[e][1], multi[e][1]), e


# ---- c. the origins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch,overlap", PATCHES)
def test_multi_origins_equal_the_single_source_origins(patch, overlap):
    pw, ph = patch
    extents = [types.SimpleNamespace(n_pings=w, n_range=h) for w, h in EXTENTS]
    assert any(s.n_range <= ph for s in extents) and any(s.n_range > ph for s in extents)      # both centre-row rules
    cen, src = edge_patches(extents, ph, pw)
    n = len(extents)
    cen = np.concatenate([cen, cen[:2]])                     # two patches that name no echogram
    src = np.concatenate([src, np.array([-1, n], dtype=np.int32)])
    P = len(cen)
    table = torch.tensor([(0, 0, 0, 0, s.n_pings, s.n_range) for s in extents], dtype=torch.int64).to(DEV)
    cen_d, src_d = torch.from_numpy(cen).to(DEV), torch.from_numpy(src).to(DEV)
    SENT = -12345
    got = torch.full((P + 3, 2), SENT, dtype=torch.int32, device=DEV)
    call("crimac_eval_crop_origins_multi", ptr(table), n, ptr(src_d), ptr(cen_d), P, ph, pw, ptr(got))
    got = got.cpu().numpy()
    assert (got[P - 2:] == SENT).all()                       # the skipped patches and the rows past P
    for i, s in enumerate(extents):
        ix = np.nonzero(src == i)[0]
        own = torch.from_numpy(cen[ix]).to(DEV)
        want = torch.empty((len(ix), 2), dtype=torch.int32, device=DEV)
        call("crimac_eval_crop_origins", ptr(own), len(ix), ph, pw, s.n_range, 1, ptr(want))
        assert np.array_equal(got[ix], want.cpu().numpy()), i
        if s.n_range <= ph:                                  # the centre row is H / 2 whatever the centre says
            assert (got[ix, 0] == s.n_range // 2 - (ph + 1) // 2 + 1).all()


# ---- d, e. the flow --------------------------------------------------------------------------------------------------------
def loop(echograms, pipe, patch, overlap, batch, spec, **kw):
    """The yardstick: evaluate_echogram_memm with a ScoredIntegration per echogram -> (summed histograms, [result])."""
    hp = hn = 0
    results = []
    for eg in echograms:
        s = ti.ScoredIntegration(spec)
        a, b = ti.evaluate_echogram_memm(eg, pipe, patch, overlap, batch, integration=s, **kw)
        hp, hn = hp + a, hn + b
        results.append(s.result())
    return (hp, hn), results


def same_results(set_, echograms, want):
    """Per echogram: the same pixels; per cell the same sum up to the order of its terms -- both sides add the same n
    positive fp64 terms in different batch cuts, each within (n - 1) * 2^-53 of the exact sum."""
    got = set_.results()
    assert [eg.name for eg, _ in got] == [eg.name for eg in echograms]
    for (eg, res), ref in zip(got, want):
        assert set(res) == set(ref) and res["annotated"] == ref["annotated"] and res["classes"] == ref["classes"]
        assert np.array_equal(res["ping_edges"], ref["ping_edges"]) and np.array_equal(res["range_edges"], ref["range_edges"])
        assert res["pixels"].dtype == np.int64 and np.array_equal(res["pixels"], ref["pixels"]), eg.name
        n = int(ref["pixels"].max())
        err = np.abs(res["sv_sum"] - ref["sv_sum"])
        assert (err <= 2 * n * 2.0 ** -53 * ref["sv_sum"]).all(), (eg.name, float(err.max()))
    tot = set_.totals()
    assert np.array_equal(tot["pixels"], sum(r["pixels"].sum(axis=(2, 3)) for r in want))
    assert np.allclose(tot["sv_sum"], sum(r["sv_sum"].sum(axis=(2, 3)) for r in want), rtol=1e-12, atol=0)


@pytest.mark.parametrize("mode", ["all", "region"])
@pytest.mark.parametrize("patch,overlap", PATCHES)
def test_packed_set_equals_the_loop_with_a_predictor_stub(echograms, stub_pipe, patch, overlap, mode):  # noqa: F811
    batch = 8 if patch == (32, 32) else 3
    spec = ti.IntegrationSpec(ping_bin=23, range_bin=9, thresholds=(0.5, 0.25),
                              mode="threshold" if mode == "all" else "probability")
    kw = dict(eval_mode=mode, predict_fn=stub_pipe.fn)
    want_hist, want = loop(echograms, stub_pipe, patch, overlap, batch, spec, **kw)
    counts = [len(r.grid) for g in ti.iter_memm_groups(iter(echograms), patch, overlap, 10 ** 9, device=stub_pipe.device)
              for r in g]
    group_patches = counts[0] + counts[1] // 2               # crossed inside echogram 1's run: at least two groups
    set_, stats = ti.ScoredIntegrationSet(spec), {}
    got = ti.evaluate_echograms_memm(iter(echograms), stub_pipe, patch, overlap, batch, group_patches=group_patches,
                                     group_elems=SMALL, stats=stats, integration=set_, **kw)
    plain = ti.evaluate_echograms_memm(iter(echograms), stub_pipe, patch, overlap, batch, group_patches=group_patches,
                                       group_elems=SMALL, **kw)
    assert stats["groups"] >= 2 and stats["fallback_echograms"] == stats["solo_echograms"] == 0
    for a, b, c in zip(got, plain, want_hist):               # the return value is unchanged
        assert a.dtype == np.int64 and np.array_equal(a, b) and np.array_equal(a, c)
    same_results(set_, echograms, want)
    assert sum(int(r["pixels"][:, 2].sum()) for r in want) > 1000
    assert {r["sv_sum"].shape for r in want} == {(3, 3, -(-w // 23), -(-h // 9)) for w, h in EXTENTS}
    r_per, r = set_.recall("other")
    assert r_per.shape == (len(echograms),) and (np.isnan(r) or 0.0 <= r <= 1.0)
    ti.release_staging()


def test_a_solo_echogram_lands_in_its_place(echograms, stub_pipe):  # noqa: F811
    spec = ti.IntegrationSpec(ping_bin=23, range_bin=9, mode="probability")
    kw = dict(eval_mode="region", predict_fn=stub_pipe.fn)
    want_hist, want = loop(echograms, stub_pipe, (32, 32), 4, 8, spec, **kw)
    cap = 130 * 64 + 17 * 17 + 1000                          # the 300 x 90 echogram does not fit
    set_, stats = ti.ScoredIntegrationSet(spec), {}
    got = ti.evaluate_echograms_memm(iter(echograms[1:] + echograms[:1]), stub_pipe, (32, 32), 4, 8, group_elems=cap,
                                     stats=stats, integration=set_, **kw)
    assert stats["solo_echograms"] == 1 and stats["fallback_echograms"] == 0 and stats["groups"] >= 2
    assert np.array_equal(got[0], want_hist[0]) and np.array_equal(got[1], want_hist[1])
    same_results(set_, echograms[1:] + echograms[:1], want[1:] + want[:1])
    ti.release_staging()


def test_real_network_packed_set_against_the_loop(echograms):  # noqa: F811
    """UNet_Baseline(depth 3, 'h3p', synthetic weights), 64 x 64 patches.  The `all` plane carries no prediction: the same
    pixels, the same sums up to their order.  The class planes may move with the batch composition by what
    test_gpu_memm_survey_eval.py measured for the packed path against the loop and allows there: twice SELF_MOVED_SHARE
    of the pixels, which is 0 -- so they are held to the same criteria."""
    patch, overlap = PATCHES[1]
    model = pkg.UNet_Baseline(3, 4, depth=3, precision="h3p")
    model.load_state_dict(synth.synth_state_dict(depth=3, seed=4))
    pipe = make_pipe(model)
    spec = ti.IntegrationSpec(ping_bin=50, range_bin=32, thresholds=(0.3, 0.3))
    want_hist, want = loop(echograms, pipe, patch, overlap, 4, spec)
    set_, stats = ti.ScoredIntegrationSet(spec), {}
    got = ti.evaluate_echograms_memm(iter(echograms), pipe, patch, overlap, 4, group_elems=SMALL, stats=stats, integration=set_)
    assert stats["fallback_echograms"] == stats["solo_echograms"] == 0
    assert np.array_equal(got[0], want_hist[0]) and np.array_equal(got[1], want_hist[1])
    results = set_.results()
    for (eg, res), ref in zip(results, want):                # the `all` plane
        assert np.array_equal(res["pixels"][:, 2], ref["pixels"][:, 2]), eg.name
        n = int(ref["pixels"].max())
        assert (np.abs(res["sv_sum"][:, 2] - ref["sv_sum"][:, 2]) <= 2 * n * 2.0 ** -53 * ref["sv_sum"][:, 2]).all(), eg.name
    moved = sum(int(np.abs(res["pixels"][:, :2] - ref["pixels"][:, :2]).sum()) for (_, res), ref in zip(results, want))
    total = sum(int(ref["pixels"][:, 2].sum()) for ref in want)
    print(f"class planes, packed set vs loop: {moved} of {total} pixels booked differently")
    assert total > 1000 and moved <= 2 * SELF_MOVED_SHARE * total, moved
    if SELF_MOVED_SHARE == 0.0:
        same_results(set_, echograms, want)
    ti.release_staging()
