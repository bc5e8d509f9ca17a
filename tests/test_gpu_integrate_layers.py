"""GPU: seabed-aware echo integration -- ``crimac_integrate_layers`` (csrc/integrate.hip) against numpy, and the flows that
launch it: ``integrate_survey`` / ``integrate_echogram_memm`` with seabed specs, and the packed ``integrate_echograms_memm``.

Exactness.  sv is drawn from the dyadic grid k * 2^-20, k < 2^12 (with NaN, +-Inf, 0 and negative samples mixed in) and the
probabilities are float16 values, so every term sv or sv * prob is a multiple of 2^-44 below 2^-8: a cell of fewer than
2^16 pixels sums to less than 2^8, which fp64 holds exactly -- every partial sum is exact in ANY order, and sums are
compared with ``==``.  Counts are always exact.  The one case with a real network reads non-dyadic sv: counts equal and
|got - want| <= (n - 1) * 2^-53 * sum|terms| per cell (the fp64 summation bound, n = the cell's counted pixels, ``want``
the exactly rounded ``math.fsum``)."""
import math
import types

import numpy as np
import pytest
import torch

import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import hip, synth
from crimac_classifiers_unet_amd import tiled_inference as ti
from crimac_classifiers_unet_amd.hip import call, ptr
from tools.fake_reader import FakeEchogram, FakeZarrReader, holey_seabed_mask, synth_survey

pytestmark = pytest.mark.gpu

FREQS = [18, 38, 120, 200]
MODES = ("threshold", "probability")
REFERENCES = ("surface", "seabed")
THR = (0.5, 0.25)


# ---- the numpy statement of the kernel --------------------------------------------------------------------------------
def layers_numpy(acc, cnt, pred, sv, thr, mode, ping_bin, range_bin, ping_origin, line, offset, reference, sums=None):
    """One launch accumulated into ``acc`` float64 / ``cnt`` int64 [3, n_pb_total, n_cols].  ``pred`` [2, R, P] as stored,
    ``sv`` [P, R] float32 (the launch's pings), ``line`` int [P] (the seabed row of every ping of the launch);
    ``offset`` None: no limit.  ``sums(terms [n]) -> float`` (default ``np.sum``: exact on the dyadic grid)."""
    R, P = pred.shape[1:]
    n_cols = acc.shape[2]
    s = np.asarray(sv, dtype=np.float32).T
    assert s.shape == (R, P)
    L = np.full(P, R) if offset is None else np.clip(np.asarray(line).astype(np.int64) + offset, 0, R)
    r = np.arange(R)[:, None]
    ok = np.isfinite(s) & (s > 0) & (r < L[None, :])
    if reference == "seabed":
        col = (L[None, :] - 1 - r) // range_bin                  # layer 0 touches the limit
        ok &= col < n_cols                                       # rows above the top layer are dropped
    else:
        col = np.broadcast_to(r // range_bin, (R, P))
    s64 = np.where(ok, s, 0).astype(np.float64)
    p32 = pred.astype(np.float32)
    if mode == "threshold":
        member = p32 >= np.asarray(thr, dtype=np.float32)[:, None, None]
        weight = member.astype(np.float64)
    else:
        member = p32 > 0
        weight = np.where(member, p32, 0).astype(np.float64)
    pb = np.broadcast_to(((ping_origin + np.arange(P)) // ping_bin)[None, :], (R, P))
    planes = ((s64 * weight[0], ok & member[0]), (s64 * weight[1], ok & member[1]), (s64, ok))
    for k, (terms, counted) in enumerate(planes):
        at = pb[counted] * n_cols + col[counted]
        cnt[k] += np.bincount(at, minlength=acc[k].size).reshape(acc[k].shape)
        if sums is None:
            acc[k] += np.bincount(at, weights=terms[counted], minlength=acc[k].size).reshape(acc[k].shape)
        else:
            for cell in np.unique(at):
                acc[k].reshape(-1)[cell] += sums(terms[counted][at == cell])


def new_host(n_pb_total, n_cols):
    return np.zeros((3, n_pb_total, n_cols)), np.zeros((3, n_pb_total, n_cols), dtype=np.int64)


def new_device(n_pb_total, n_cols):
    shape = (3, n_pb_total, n_cols)
    return torch.zeros(shape, dtype=torch.float64, device="cuda"), torch.zeros(shape, dtype=torch.int64, device="cuda")


def tensor(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def dyadic_sv(rng, shape, bad=0.02):
    """float32 k * 2^-20, 1 <= k < 2^12, with NaN / +Inf / -Inf / 0 / negative samples at a share ``bad``."""
    sv = (rng.integers(1, 1 << 12, size=shape) * 2.0 ** -20).astype(np.float32)
    hit = rng.random(shape) < bad
    sv[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -2.0 ** -10], dtype=np.float32), size=int(hit.sum()))
    return sv


def operands(n_range, n_pings, data_pings, seed):
    """pred float32 [2, R, P] of float16 values m / 1024, a third of them 0; sv float32 [data_pings, R] dyadic."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pred = (rng.integers(0, 1025, size=(2, n_range, n_pings)) / 1024.0).astype(np.float32)
    pred[rng.random(pred.shape) < 0.33] = 0
    assert np.array_equal(pred.astype(np.float16).astype(np.float32), pred)
    return pred, dyadic_sv(rng, (data_pings, n_range))


def launch(acc, cnt, pred, sv, thr, mode, ping_bin, range_bin, ping_origin, sv_ping_off, seabed, seabed_first, offset,
           reference, n_layers, run=True):
    """``crimac_integrate_layers`` on device tensors: ``pred`` [2, R, P], ``sv`` [data_pings, R], ``seabed`` int32 [n]."""
    _, R, P = pred.shape
    n_pb_total, n_cols = acc.shape[1:]
    cells = ((ping_origin + P - 1) // ping_bin - ping_origin // ping_bin + 1) * n_cols
    scratch = torch.empty((cells + hip.INTEGRATE_SPLIT_WGS) * hip.INTEGRATE_SLOT_BYTES // 8, dtype=torch.float64, device="cuda")
    args = (ptr(pred), int(pred.dtype == torch.float16), R, P, ptr(sv), sv.shape[0], sv_ping_off, float(thr[0]),
            float(thr[1]), MODES.index(mode), ping_bin, range_bin, ping_origin, n_pb_total, ptr(seabed), seabed_first,
            seabed.numel(), offset, REFERENCES.index(reference), n_layers, ptr(acc), ptr(cnt), ptr(scratch), scratch.numel() * 8)
    if run:
        call("crimac_integrate_layers", *args)
    return args


def seabed_line(kind, n_pings, n_range):
    """Seabed rows per ping.  'flat': constant, not a multiple of 4.  'slope': a sawtooth of 3 rows per ping -- 189 rows of
    relief inside one 64-ping bin, across 64-row tiles and 32-row layers -- with stretches at or above row 0 (limit 0: the
    whole column excluded, also after the offset) and at or below the last row (nothing excluded)."""
    p = np.arange(n_pings)
    if kind == "flat":
        return np.full(n_pings, min(n_range - 9, 53), dtype=np.int32)
    line = -20 + (3 * p) % (n_range + 60)
    line[5:9] = -7
    line[40:47] = n_range + 11
    return line.astype(np.int32)


def run_case(n_range, n_pings, seams, kind, offset, reference, n_layers, mode, dtype, seed=1, ping_bin=64, range_bin=32,
             sv_ping_off=37, seabed_lead=5, misalign=False):
    """Launches over pings [seams[i], seams[i + 1]) into one accumulator; the seabed array starts ``seabed_lead`` pings
    before ping 0.  Returns (got sums, got counts, want sums, want counts)."""
    pred, sv = operands(n_range, n_pings, sv_ping_off + n_pings + 9, seed)
    line = seabed_line(kind, n_pings, n_range)
    n_pb = -(-n_pings // ping_bin)
    n_cols = n_layers if reference == "seabed" else -(-n_range // range_bin)
    want = new_host(n_pb, n_cols)
    acc, cnt = new_device(n_pb, n_cols)
    lead = np.full(seabed_lead, 10 ** 6, dtype=np.int32)         # (read by mistake, it would exclude nothing)
    seabed_d = tensor(np.concatenate([lead, line, lead]))
    if misalign:                                                 # both base addresses one element off the 16-byte grid
        sv_d = torch.zeros(sv.size + 1, dtype=torch.float32, device="cuda")[1:].view(sv.shape)
        sv_d.copy_(torch.from_numpy(sv))
        assert sv_d.data_ptr() % 16 == 4
    else:
        sv_d = tensor(sv)
    for p0, p1 in zip(seams[:-1], seams[1:]):
        part = pred[:, :, p0:p1]
        if misalign:
            part_d = torch.zeros(part.size + 1, dtype=dtype, device="cuda")[1:].view(part.shape)
            part_d.copy_(torch.from_numpy(np.ascontiguousarray(part)))
            assert part_d.data_ptr() % 8 != 0
        else:
            part_d = tensor(part, dtype)
        launch(acc, cnt, part_d, sv_d, THR, mode, ping_bin, range_bin, p0, sv_ping_off + p0, seabed_d, seabed_lead + p0,
               offset, reference, n_layers)
        layers_numpy(*want, part_d.cpu().numpy(), sv[sv_ping_off + p0:sv_ping_off + p1], THR, mode, ping_bin, range_bin, p0,
                     line[p0:p1], offset, reference)
    return acc.cpu().numpy(), cnt.cpu().numpy(), *want


def check_exact(got_sum, got_cnt, want_sum, want_cnt):
    assert got_sum.dtype == np.float64 and got_cnt.dtype == np.int64
    assert got_sum.shape == want_sum.shape and got_cnt.shape == want_cnt.shape
    assert np.array_equal(got_cnt, want_cnt)
    assert np.array_equal(got_sum, want_sum)                     # exact: see the module docstring


# ---- the kernel alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("reference", REFERENCES)
def test_two_launches_across_a_ping_bin_match_numpy(reference, dtype, mode):
    """70 rows x 150 pings (4-byte sv reads; 100 pings take the 16- / 8-byte pred reads, 50 the scalar ones), the seam
    inside ping bin 1, a sloping line with limits 0 and n_range; 2 layers of 32 rows: the rows above are dropped."""
    got = run_case(70, 150, (0, 100, 150), "slope", -3, reference, 2, mode, dtype)
    check_exact(*got)
    assert got[3][2].sum() > 1000 and (got[3][:2].sum(axis=(1, 2)) > 0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("reference", REFERENCES)
@pytest.mark.parametrize("kind,offset", [("flat", 0), ("slope", -3), ("slope", 10)])
def test_wide_reads_300_rows_600_pings_match_numpy(kind, offset, reference, mode):
    """Extents and addresses that take the 16-byte reads of both operands; relief of 189 rows inside a ping bin; 4 layers
    (too few: rows above are dropped), the top layers cut by row 0 where the limit is small."""
    got = run_case(300, 600, (0, 600), kind, offset, reference, 4, mode, torch.float16, seed=2)
    check_exact(*got)
    assert got[3][2].sum() > 10000


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("reference", REFERENCES)
def test_misaligned_base_pointers_take_the_narrow_reads(reference, dtype):
    check_exact(*run_case(72, 200, (0, 200), "slope", -3, reference, 3, "probability", dtype, seed=3, misalign=True))


def test_a_seabed_line_on_the_tile_grid_and_layers_of_one_row():
    """range_bin 1 (one layer per row above the limit, 70 layers: every row has one) and a ping bin of one tile."""
    check_exact(*run_case(70, 150, (0, 150), "slope", 0, "seabed", 70, "threshold", torch.float16, seed=4, range_bin=1))
    check_exact(*run_case(70, 150, (0, 150), "flat", 11, "seabed", 3, "threshold", torch.float16, seed=4, ping_bin=1000))


@pytest.mark.parametrize("mode", MODES)
def test_enough_layers_add_up_to_the_surface_reference(mode):
    """layers >= ceil(n_range / range_bin): every counted pixel has a layer, so per ping bin the total over the layers equals
    the total over the surface cells with the same offset, in every plane (exact sums)."""
    surf = run_case(300, 600, (0, 250, 600), "slope", -3, "surface", 0, mode, torch.float16, seed=5)
    lay = run_case(300, 600, (0, 250, 600), "slope", -3, "seabed", 10, mode, torch.float16, seed=5)
    check_exact(*surf)
    check_exact(*lay)
    assert np.array_equal(lay[1].sum(axis=2), surf[1].sum(axis=2)) and np.array_equal(lay[0].sum(axis=2), surf[0].sum(axis=2))
    assert surf[1][2].sum() > 10000
    # and without a limit in reach (offset beyond every row) the surface reference is crimac_integrate_classes
    pred, sv = operands(70, 150, 150, 6)
    acc, cnt = new_device(3, 3)
    old_acc, old_cnt = new_device(3, 3)
    pred_d, sv_d, line = tensor(pred, torch.float16), tensor(sv), tensor(np.zeros(150, dtype=np.int32))
    args = launch(acc, cnt, pred_d, sv_d, THR, mode, 64, 32, 0, 0, line, 0, 1000, "surface", 0)
    call("crimac_integrate_classes", *args[:14], ptr(old_acc), ptr(old_cnt), *args[22:])
    assert torch.equal(cnt, old_cnt) and acc.cpu().numpy().tobytes() == old_acc.cpu().numpy().tobytes() and bool(cnt.any())


def test_the_multi_launch_case_twice_gives_identical_bits():
    for reference in REFERENCES:
        a = run_case(70, 150, (0, 100, 150), "slope", -3, reference, 2, "probability", torch.float16)
        b = run_case(70, 150, (0, 100, 150), "slope", -3, reference, 2, "probability", torch.float16)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def test_argument_errors_are_reported_and_launch_nothing():
    pred, sv = operands(70, 150, 160, 7)
    pred_d, sv_d, line = tensor(pred), tensor(sv), tensor(np.full(155, 30, dtype=np.int32))
    acc, cnt = new_device(3, 2)
    args = list(launch(acc, cnt, pred_d, sv_d, THR, "threshold", 64, 32, 0, 0, line, 5, -3, "seabed", 2, run=False))
    for at, value, word in ((14, None, "seabed"), (15, 6, "seabed"), (15, -1, "seabed"), (16, 149, "seabed"),
                            (18, 2, "reference"), (19, 0, "n_layers"), (9, 2, "mode"), (23, 48, "scratch")):
        bad = list(args)
        bad[at] = value
        with pytest.raises(hip.HipLibraryError, match=word):
            call("crimac_integrate_layers", *bad)
    torch.cuda.synchronize()
    assert not acc.any() and not cnt.any()


# ---- the flows ----------------------------------------------------------------------------------------------------------
def hashed_predict_fn(x, P, H, W):
    """Fixed pseudo-random probabilities: a per-pixel hash of the four dB input channels, elementwise, so a patch's result
    cannot depend on the batch around it."""
    d = x.float().reshape(P, H, W, 16)[..., :4].permute(0, 3, 1, 2)
    h = d[:, 0] * 12.9898 + d[:, 1] * 78.233 + d[:, 2] * 37.719 + d[:, 3] * 4.581
    u = torch.frac(torch.sin(h) * 43758.5453).abs()
    v = torch.frac(torch.sin(h * 1.618) * 24634.6345).abs()
    sandeel = 0.02 + 0.96 * u * v.sqrt()
    other = (1 - sandeel) * v
    return torch.stack([1 - sandeel - other, sandeel, other], dim=1).contiguous()


def make_pipe(model):
    return types.SimpleNamespace(model=model.cuda().eval(), device=torch.device("cuda"), frequencies=FREQS)


@pytest.fixture(scope="module")
def stub_pipe():
    return make_pipe(pkg.UNet_Baseline(3, 4, start_filts=8, precision="f32x6"))


def specs(**kw):
    """The seabed-aware specs of the flow tests: a backstep on the surface grid, and bottom layers."""
    return [ti.IntegrationSpec(100, 64, thresholds=THR, seabed_offset=-4, **kw),
            ti.IntegrationSpec(100, 16, thresholds=THR, seabed_offset=-4, reference="seabed", layers=5, **kw)]


def result_by_numpy(spec, chunks, sv, line, n_pings, n_range, sums=None):
    """``chunks``: (start ping, stored predictions [2, R, e - s]); ``sv`` [pings, R]; ``line`` [pings]."""
    want = new_host(*spec.bins(n_pings, n_range))
    for s, out in chunks:
        e = s + out.shape[2]
        layers_numpy(*want, out, sv[s:e], spec.thresholds, spec.mode, spec.ping_bin, spec.range_bin, s, line[s:e],
                     spec.seabed_offset, spec.reference, sums=sums)
    return want


def dyadic_survey(n_pings, n_range, seed):
    sv, labels, seabed = synth_survey(n_pings=n_pings, n_range=n_range, seed=seed)
    return dyadic_sv(np.random.Generator(np.random.PCG64(seed)), sv.shape, bad=0.001), labels, seabed


@pytest.fixture(scope="module")
def zarr_case(stub_pipe):
    """A 520-ping x 300-row survey in 3 chunks, and its float16 predictions, computed once."""
    sv, labels, seabed = dyadic_survey(520, 300, 21)
    seabed = np.clip(seabed, 0, 260)
    reader = FakeZarrReader(sv, labels, seabed)
    chunks = [(s, out) for s, e, out in ti.predict_survey(reader, stub_pipe, (256, 256), 20, 3, 200, out_dtype=np.float16,
                                                         predict_fn=hashed_predict_fn)]
    assert [s for s, _ in chunks] == [0, 173, 346]
    return reader, chunks


@pytest.mark.parametrize("mode", MODES)
def test_integrate_survey_with_seabed_specs_equals_predict_survey_then_numpy(stub_pipe, zarr_case, mode):
    reader, chunks = zarr_case
    for spec in specs(mode=mode):
        want = result_by_numpy(spec, chunks, reader.sv[1], reader.seabed, 520, 300)
        got = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 200, spec, predict_fn=hashed_predict_fn)
        check_exact(got["sv_sum"], got["pixels"], *want)
        assert (got["reference"], got["seabed_offset"]) == (spec.reference, -4)
        assert got["pixels"][2].sum() > 20000 and (got["pixels"][:2].sum(axis=(1, 2)) > 0).all()
    assert got["range_edges"].tolist() == [0, 16, 32, 48, 64, 80] and got["sv_sum"].shape == (3, 6, 5)


def test_a_default_spec_still_takes_crimac_integrate_classes_with_the_same_bits(stub_pipe, zarr_case, monkeypatch):
    reader, chunks = zarr_case
    names = []
    real = ti.call
    monkeypatch.setattr(ti, "call", lambda name, *a, **kw: (names.append(name), real(name, *a, **kw))[1])
    spec = ti.IntegrationSpec(100, 64, thresholds=THR)
    got = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 200, spec, predict_fn=hashed_predict_fn)
    assert names.count("crimac_integrate_classes") == 3 and "crimac_integrate_layers" not in names
    assert set(got) == {"sv_sum", "pixels", "ping_edges", "range_edges", "classes"}
    # the direct calls, chunk by chunk
    acc, cnt = new_device(6, 5)
    sv_d = tensor(reader.sv[1])
    for s, out in chunks:
        n = out.shape[2]
        scratch = torch.empty((3 * 5 + hip.INTEGRATE_SPLIT_WGS) * hip.INTEGRATE_SLOT_BYTES // 8, dtype=torch.float64,
                              device="cuda")                      # (a chunk touches at most 3 ping bins x 5 range bins)
        real("crimac_integrate_classes", ptr(tensor(out)), 1, 300, n, ptr(sv_d), 520, s, THR[0], THR[1], 0, 100, 64, s, 6,
             ptr(acc), ptr(cnt), ptr(scratch), scratch.numel() * 8)
    assert np.array_equal(got["pixels"], cnt.cpu().numpy()) and got["sv_sum"].tobytes() == acc.cpu().numpy().tobytes()
    # the bottom echo is in the `all` plane of the default spec and not above a limit
    cut = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 200, specs()[0], predict_fn=hashed_predict_fn)
    assert (cut["pixels"][2] <= got["pixels"][2]).all() and cut["pixels"][2].sum() < got["pixels"][2].sum()


def test_a_zarr_chunk_loaded_with_a_mask_uses_the_first_masked_row(stub_pipe, monkeypatch):
    sv, labels, seabed = dyadic_survey(520, 300, 22)
    mask = holey_seabed_mask(np.clip(seabed, 0, 260), 300)
    reader = FakeZarrReader(sv, labels, None, mask=mask)
    line = np.where(mask.any(axis=1), mask.argmax(axis=1), 300)
    assert (line[100:131] == 300).all() and (mask[300:341].sum(axis=1) < 300 - line[300:341]).all()      # no bottom; holes
    chunks = [(s, out) for s, e, out in ti.predict_survey(reader, stub_pipe, (256, 256), 20, 3, 200, out_dtype=np.float16,
                                                         predict_fn=hashed_predict_fn)]
    seen = []
    real = ti.ChunkPredictor._limit_line
    monkeypatch.setattr(ti.ChunkPredictor, "_limit_line", lambda cp: (seen.append(cp.mask is not None), real(cp))[1])
    for spec in specs():
        want = result_by_numpy(spec, chunks, sv[1], line, 520, 300)
        got = ti.integrate_survey(reader, stub_pipe, (256, 256), 20, 3, 200, spec, predict_fn=hashed_predict_fn)
        check_exact(got["sv_sum"], got["pixels"], *want)
    assert seen == [False, True, False] * 2                      # (pings 300-340, the holes, lie in the middle chunk)


def test_a_chunk_with_neither_a_mask_nor_a_vector_raises(stub_pipe):
    sv, labels, _ = dyadic_survey(120, 70, 23)
    cp = ti.ChunkPredictor(stub_pipe.model, 70, (64, 64), 6, 4, out_f16=True)
    cp.load_chunk(sv, 0, labels, None, 0, 120)
    spec = specs()[0].bind(FREQS)
    acc, cnt = ti.new_integration("cuda", spec, 120, 70)
    with pytest.raises(ValueError, match="neither"):
        cp.integrate(acc, cnt, spec)
    plain = ti.IntegrationSpec(100, 64).bind(FREQS)               # (a spec without a limit needs no line)
    cp.integrate(*ti.new_integration("cuda", plain, 120, 70), plain)


def test_integrate_survey_with_a_real_small_network_and_bottom_layers():
    sv, labels, seabed = synth_survey(n_pings=230, n_range=120, seed=11)
    seabed = np.clip(seabed, 0, 100)
    reader = FakeZarrReader(sv, labels, seabed)
    model = pkg.UNet_Baseline(3, 4, start_filts=8, precision="h3p")
    model.load_state_dict(synth.synth_state_dict(start_filts=8, seed=4))
    pipe = make_pipe(model)
    spec = ti.IntegrationSpec(48, 25, mode="probability", seabed_offset=-2, reference="seabed", layers=3)
    chunks = [(s, out) for s, e, out in ti.predict_survey(reader, pipe, (64, 64), 6, 8, 120, out_dtype=np.float16)]
    assert len(chunks) == 2
    want_sum, want_cnt = result_by_numpy(spec, chunks, sv[1], seabed, 230, 120, sums=math.fsum)
    got = ti.integrate_survey(reader, pipe, (64, 64), 6, 8, 120, spec)
    assert np.array_equal(got["pixels"], want_cnt) and want_cnt[2].sum() > 10000 and (want_cnt[:2].sum(axis=(1, 2)) > 0).all()
    bound = np.maximum(want_cnt - 1, 0) * 2.0 ** -53 * want_sum          # (every term is >= 0: sum|terms| = the sum)
    err = np.abs(got["sv_sum"] - want_sum)
    print("largest |sum error| / bound:", float((err[bound > 0] / bound[bound > 0]).max()))
    assert (err <= bound).all()


# ---- memm ---------------------------------------------------------------------------------------------------------------
def echogram(n_pings, n_range, seed, name="eg"):
    """A memmap echogram of any extent (17 x 17 included): dyadic sv, a few label blocks (sandeel 27, other 1, an unused
    species, ignore), an undulating seabed line with a metadata source next to it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sv = dyadic_sv(rng, (4, n_pings, n_range), bad=0.001)
    labels = np.zeros((n_pings, n_range), dtype=np.int16)
    for k, val in enumerate((27, 1, 12, -1)):
        w, h = max(1, n_pings // 6), max(1, n_range // 5)
        x, y = int(rng.integers(0, n_pings - w + 1)), int(rng.integers(0, n_range - h + 1))
        labels[x:x + w, y:y + h] = val
    x = np.arange(n_pings)
    seabed = np.clip((0.7 * n_range + 0.15 * n_range * np.sin(x / 23.0) + 2 * np.sin(x / 3.0)).astype(np.int64), 1,
                     max(1, n_range - 10))
    eg = FakeEchogram(np.ascontiguousarray(sv.transpose(0, 2, 1)), np.ascontiguousarray(labels.T), seabed, frequencies=FREQS,
                      name=name)
    tv = 737000.5 + np.cumsum(np.random.Generator(np.random.PCG64(seed)).uniform(5e-6, 9e-6, size=n_pings))
    eg.portion_of_day_vector, eg.portion_of_year_scalar = tv % 1, 0.61
    eg.time_vector_diff = np.concatenate((np.diff(tv), [tv[-1] - tv[-2]])) / 6e-6 - 1
    return eg


def memm_by_numpy(eg, pipe, spec, line, **kw):
    out = ti.predict_echogram_memm(eg, pipe, (64, 64), 6, 8, predict_fn=hashed_predict_fn, **kw).astype(np.float16)
    R, P = eg.shape
    return result_by_numpy(spec, [(0, out)], eg.sv[FREQS.index(spec.frequency or 38)].T, line, P, R)


@pytest.mark.parametrize("mode", MODES)
def test_integrate_echogram_memm_with_seabed_specs_equals_predict_then_numpy(stub_pipe, mode):
    eg = echogram(300, 90, 31)
    given = np.clip(eg._seabed - 17, 1, 80)
    for spec in (ti.IntegrationSpec(77, 40, frequency=120, mode=mode, seabed_offset=-4),
                 ti.IntegrationSpec(77, 20, frequency=120, mode=mode, seabed_offset=3, reference="seabed", layers=3)):
        for line, kw in ((eg._seabed, {}), (given, dict(seabed=given))):
            want = memm_by_numpy(eg, stub_pipe, spec, line, **kw)
            got = ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn, **kw)
            check_exact(got["sv_sum"], got["pixels"], *want)
            assert got["pixels"][:2].sum() > 0 and got["ping_edges"].tolist() == [0, 77, 154, 231, 300]


def test_the_scatter_rule_as_a_limit_keeps_the_class_planes_and_cuts_the_all_plane(stub_pipe):
    """seabed_offset = +SEABED_PAD is the row rule of the memm scatter: no pixel at or below it holds a prediction, so the
    class planes of the default spec are unchanged (exactly) and `all` loses exactly the pixels at or below the line."""
    eg = echogram(300, 90, 32)
    eg.labels[:] = 0                     # (the scatter's seabed rule acts on background pixels: all of them are)
    base = ti.IntegrationSpec(77, 40, thresholds=THR)
    cut = ti.IntegrationSpec(77, 40, thresholds=THR, seabed_offset=ti.SEABED_PAD)
    a = ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, base, predict_fn=hashed_predict_fn)
    b = ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, cut, predict_fn=hashed_predict_fn)
    assert np.array_equal(a["pixels"][:2], b["pixels"][:2]) and np.array_equal(a["sv_sum"][:2], b["sv_sum"][:2])
    assert a["pixels"][:2].sum() > 0
    s = eg.sv[1]                                                  # [R, P]
    below = np.isfinite(s) & (s > 0) & (np.arange(90)[:, None] >= (eg._seabed + ti.SEABED_PAD)[None, :])
    lost_cnt, lost_sum = np.zeros((4, 3), dtype=np.int64), np.zeros((4, 3))
    for r, p in np.argwhere(below):
        lost_cnt[p // 77, r // 40] += 1
        lost_sum[p // 77, r // 40] += float(s[r, p])
    assert lost_cnt.sum() > 1000
    assert np.array_equal(a["pixels"][2] - b["pixels"][2], lost_cnt) and np.array_equal(a["sv_sum"][2] - b["sv_sum"][2], lost_sum)


def test_integrate_echogram_memm_with_the_estimated_line(stub_pipe):
    eg = echogram(300, 90, 33)
    line = ti.estimate_seabed_memm(eg)
    spec = ti.IntegrationSpec(77, 20, seabed_offset=-2, reference="seabed", layers=2)
    want = memm_by_numpy(eg, stub_pipe, spec, line, seabed="estimate")
    got = ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn, seabed="estimate")
    check_exact(got["sv_sum"], got["pixels"], *want)
    assert got["pixels"][2].sum() > 0


SURVEY = [(300, 90), (40, 200), (17, 17), (130, 64), (500, 120), (100, 50), (64, 128)]      # pings x range
CAP = 40000                              # group_elems: the fifth echogram (60000 pixels) exceeds it


def survey():
    return [echogram(p, r, 40 + i, name=f"eg{i}") for i, (p, r) in enumerate(SURVEY)]


def same_result(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key], key
    assert a["sv_sum"].dtype == np.float64 and a["pixels"].dtype == np.int64


@pytest.mark.parametrize("which", ["default", "surface", "seabed"])
def test_integrate_echograms_memm_equals_the_loop_over_the_echograms(stub_pipe, which):
    egs = survey()
    spec = {"default": ti.IntegrationSpec(77, 40, thresholds=THR, mode="probability"),
            "surface": ti.IntegrationSpec(77, 40, thresholds=THR, seabed_offset=-3),
            "seabed": ti.IntegrationSpec(77, 8, thresholds=THR, seabed_offset=-3, reference="seabed", layers=4,
                                         mode="probability")}[which]
    counts = [len(r.grid) for g in ti.iter_memm_groups(iter(egs), (64, 64), 6, 10 ** 9) for r in g]
    stats = {}
    kw = dict(predict_fn=hashed_predict_fn, group_patches=counts[0] + counts[1] // 2, group_elems=CAP)
    got = list(ti.integrate_echograms_memm(iter(egs), stub_pipe, (64, 64), 6, 8, spec, stats=stats, **kw))
    assert [eg for eg, _ in got] == egs                          # input order, the solo echogram in its place
    assert stats["solo_echograms"] == 1 and stats["fallback_echograms"] == 0 and stats["groups"] >= 4
    assert sum(stats["batches"]) == sum(counts) - counts[4] and max(stats["batches"]) == 8
    for eg, res in got:
        same_result(res, ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn))
        assert res["pixels"][2].sum() > 0
    assert sum(int(res["pixels"][:2].sum()) for _, res in got) > 0
    # skip: asked per echogram, after the plan; what is left keeps its order and its results
    stats = {}
    kept = list(ti.integrate_echograms_memm(iter(egs), stub_pipe, (64, 64), 6, 8, spec, stats=stats,
                                            skip=lambda eg: eg.name in ("eg1", "eg4"), **kw))
    assert [eg.name for eg, _ in kept] == ["eg0", "eg2", "eg3", "eg5", "eg6"] and stats["solo_echograms"] == 0
    for (eg, res), want in zip(kept, [got[i][1] for i in (0, 2, 3, 5, 6)]):
        same_result(res, want)
    # a callable line and the estimate go to the kernel as they go to the scatter
    if which == "seabed":
        def line(eg):
            return np.clip(eg._seabed - 9, 1, None)
        for (eg, res) in ti.integrate_echograms_memm(iter(egs[:4]), stub_pipe, (64, 64), 6, 8, spec, seabed=line, **kw):
            same_result(res, ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn,
                                                        seabed=line(eg)))
        for (eg, res) in ti.integrate_echograms_memm(iter(egs[:1]), stub_pipe, (64, 64), 6, 8, spec, seabed="estimate", **kw):
            same_result(res, ti.integrate_echogram_memm(eg, stub_pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn,
                                                        seabed="estimate"))
    ti.release_staging()


def test_a_late_injection_model_takes_the_per_echogram_path_unless_packed():
    pipe = make_pipe(pkg.UNet_LateMetInject(3, 4, 7, depth=3, precision="f32x6"))
    mc = {k: True for k in ti.META_FLAGS}
    egs = survey()[:4]
    spec = ti.IntegrationSpec(77, 8, thresholds=THR, seabed_offset=-3, reference="seabed", layers=4)
    stats = {}
    alone = list(ti.integrate_echograms_memm(iter(egs), pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn,
                                             meta_channels=mc, stats=stats, group_elems=CAP))
    assert stats["fallback_echograms"] == 4 and stats["groups"] == 0 and [eg for eg, _ in alone] == egs
    stats = {}
    packed = list(ti.integrate_echograms_memm(iter(egs), pipe, (64, 64), 6, 8, spec, predict_fn=hashed_predict_fn,
                                              meta_channels=mc, pack_metadata=True, stats=stats, group_elems=CAP))
    assert stats["fallback_echograms"] == 0 and stats["groups"] >= 1 and [eg for eg, _ in packed] == egs
    for (eg, a), (_, b) in zip(alone, packed):
        same_result(a, b)
        assert a["pixels"][:2].sum() > 0
    ti.release_staging()
