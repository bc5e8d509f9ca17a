"""GPU: every form of the integrate kernel (csrc/integrate.hip) against numpy with NO tolerance.

The other integrate modules compare the several-frequency launch with the single-frequency one by bits and both with numpy
inside the fp64 reordering bound.  All entry points run one kernel body, so a mistake in a shared step -- a row dropped at a
tile tail, a pixel staged twice -- moves them together and can stay inside that bound.  Here the operands make every sum
exact in fp64 whatever its order (tests/test_integrate_exact_data_cpu.py: terms are multiples of 2^-12 below 1, cells have
fewer than 2^14 pixels, so no addition rounds below 2^53), and sums and counts are compared with ``np.array_equal``.

Forms: prediction dtype x 16-byte / 4-byte sv reads x 16- (8-) byte / scalar prediction reads x seabed or not, reached by
the two shapes of the CPU module (70 x 150: 4-byte sv reads, the 50-ping launch reads the predictions one by one;
72 x 152: the wide reads of both) and, on the second shape, by base pointers one element off the 16-byte grid.  Every form
runs both modes on the uniform grid (ping_bin 100, range_bin 50: two tiles and two splits per cell, two launches that meet
at global ping 102) and on the edge table, through the entry point a spec of that kind launches."""
import ctypes

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd.hip import call, ptr

from test_integrate_exact_data_cpu import (GRIDS, MODES, N_PLANES, ORIGIN, PING_BIN, SEABEDS, SHAPES, SV_OFF, THR, geometry,
                                           launches, operands, reference, seabed_line)  # noqa: E402

pytestmark = pytest.mark.gpu

REFERENCES = ("surface", "seabed")
SLOT, WGS = hip.INTEGRATE_SLOT_BYTES, hip.INTEGRATE_SPLIT_WGS
# name -> (shape, sv base one element off the grid, prediction base one element off the grid)
READS = {"4-byte sv": ("4-byte", False, False), "wide": ("16-byte", False, False), "sv off the grid": ("16-byte", True, False),
         "pred off the grid": ("16-byte", False, True), "both off the grid": ("16-byte", True, True)}
CHANNELS = {1: (2,), 3: (3, 1, 0), 8: (5, 0, 7, 2, 6, 1, 4, 3)}


def device(a, dtype, off):
    """``a`` on the device as ``dtype``, its base on the 16-byte grid or (``off``) one element past it."""
    flat = torch.zeros(a.size + 4, dtype=dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    t = flat[1 if off else 0:][:a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.array(a, order="C")))                    # (a copy: the shared operands are read-only)
    assert (t.data_ptr() % 16 != 0) == off and (t.data_ptr() % 8 != 0) == off
    return t


def run(reads, dtype, mode, grid, seabed, channels=None):
    """Both launches of a case into one accumulator.  ``channels`` None: plane 0 through the single-frequency entry point
    of the case's kind; a tuple: those planes through ``crimac_integrate_freqs``.  Returns (sums, counts) as numpy."""
    shape, sv_off, pred_off = READS[reads]
    R, P = SHAPES[shape]
    pred, planes = operands(shape, mode)
    table, n_pb, n_cols, range_bin = geometry(shape, grid, seabed)
    sb = SEABEDS[seabed]
    F = len(channels or (0,))
    lead = (F,) if channels else ()
    acc = torch.zeros((*lead, 3, n_pb, n_cols), dtype=torch.float64, device="cuda")
    cnt = torch.zeros((*lead, 3, n_pb, n_cols), dtype=torch.int64, device="cuda")
    sv_d = device(planes, torch.float32, sv_off)
    stride = planes[0].size
    assert (R % 4 == 0 and not sv_off) == (reads in ("wide", "pred off the grid"))                  # who takes the 16-byte sv reads
    line_d = device(np.concatenate([np.full(5, 10 ** 6, dtype=np.int32), seabed_line(P, R)]), torch.int32, False)
    edges_h = None if GRIDS[grid] is None else np.ascontiguousarray(table, dtype=np.int64)
    edges_d = None if edges_h is None else torch.from_numpy(edges_h).cuda()
    host = None if edges_h is None else ctypes.c_void_p(edges_h.ctypes.data)
    scratch = torch.empty(F * (n_pb * n_cols + WGS) * SLOT // 8, dtype=torch.float64, device="cuda")
    chan = (ctypes.c_int * F)(*(channels or (0,)))
    for p0, p1 in launches(P):
        part = device(pred[:, :, p0:p1], dtype, pred_off)
        head = (ptr(part), int(dtype == torch.float16), R, p1 - p0)
        rule = (planes.shape[1], SV_OFF + p0, THR[0], THR[1], MODES.index(mode))
        where = (range_bin, ORIGIN + p0, n_pb)
        sbs = (ptr(line_d) if sb else None, 5 + p0 if sb else 0, line_d.numel() if sb else 0, sb[0] if sb else 0,
               REFERENCES.index(sb[1]) if sb else 0, sb[2] if sb else 0)
        tail = (ptr(acc), ptr(cnt), ptr(scratch), scratch.numel() * 8)
        if channels:
            call("crimac_integrate_freqs", *head, ptr(sv_d), stride, N_PLANES, chan, F, *rule, 0 if edges_h is not None else PING_BIN,
                 ptr(edges_d), host, *where, *sbs, *tail)
        elif edges_h is not None:
            call("crimac_integrate_edges", *head, ptr(sv_d[0]), *rule, ptr(edges_d), host, *where, *sbs, *tail)
        elif sb:
            call("crimac_integrate_layers", *head, ptr(sv_d[0]), *rule, PING_BIN, *where, *sbs, *tail)
        else:
            call("crimac_integrate_classes", *head, ptr(sv_d[0]), *rule, PING_BIN, *where, *tail)
    torch.cuda.synchronize()
    return acc.cpu().numpy(), cnt.cpu().numpy()


def check(got, reads, mode, grid, seabed, channels=None):
    shape = READS[reads][0]
    for i, c in enumerate(channels or (0,)):
        want_sum, want_cnt = reference(shape, mode, grid, seabed, c)
        got_sum, got_cnt = (got[0][i], got[1][i]) if channels else got
        assert np.array_equal(got_cnt, want_cnt), (reads, mode, grid, seabed, c)
        assert np.array_equal(got_sum, want_sum), (reads, mode, grid, seabed, c)          # exact: see the module docstring


@pytest.mark.parametrize("seabed", list(SEABEDS))
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("reads", list(READS))
def test_every_single_frequency_form_equals_numpy_exactly(reads, dtype, seabed):
    for grid in GRIDS:
        for mode in MODES:
            check(run(reads, dtype, mode, grid, seabed), reads, mode, grid, seabed)


@pytest.mark.parametrize("seabed", list(SEABEDS))
@pytest.mark.parametrize("reads", list(READS))
@pytest.mark.parametrize("F", list(CHANNELS))
def test_the_several_frequency_launch_equals_numpy_exactly(F, reads, seabed):
    for grid in GRIDS:
        for mode, dtype in zip(MODES, (torch.float16, torch.float32)):
            check(run(reads, dtype, mode, grid, seabed, CHANNELS[F]), reads, mode, grid, seabed, CHANNELS[F])
