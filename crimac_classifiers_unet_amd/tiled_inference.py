"""Tiled whole-survey inference on the GPU: the ``save_predict.py`` path of the reference.

Mirrors ``save_survey_predictions_zarr`` (crimac_unet/pipeline_train_predict/save_predict.py:137-220, the zarr
preload flavour) and ``save_reader_predictions_memm`` (:222-265, the memmap flavour): the survey is cut into
chunks of at most ``preload_n_pings`` pings (utils/preload_data_split.py:22-30), every chunk is gridded into
overlapping patches (batch/samplers/gridded.py:22-54), each patch is cropped + dB-transformed, pushed through the
U-Net + softmax, and the valid interior of its SANDEEL / OTHER probabilities is scattered into a
``[2, range, pings]`` array (save_predict.py:41-65).

Here a chunk is uploaded ONCE and stays in HBM; crop, transform, forward, softmax and scatter all run on the GPU
(``crimac_gather_patches`` -> U-Net engine -> ``crimac_scatter_patches_ex``); only the finished
``[2, range, pings]`` chunk comes back -- as float16, which is what the reference stores (save_predict.py:212,
:252).  The reference does the crop / transform / ``argwhere`` scatter per patch in numpy DataLoader workers and
moves 786 kB of softmax per patch over PCIe.

Host side of ``predict_survey`` (what bounded configs[3] in round 1): the reader thread copies the next chunk
straight into PINNED staging buffers, the upload runs on a copy stream, the seabed mask is evaluated in the scatter
kernel from the seabed vector (no [pings, range] mask is built or uploaded), and the result returns through a
pinned float16 buffer.

With ``torch.distributed`` initialised, patches of a chunk are dealt round-robin to the ranks
(``parallel.shard_indices``) and the per-rank float16 outputs are summed (valid interiors are disjoint, x + 0 is
exact).  Writing zarr / npy is the caller's business: ``predict_survey`` yields numpy chunks
that a caller appends with the reference's ``create_xarray_ds_predictions`` / ``append_to_zarr``;
``predict_echogram_memm`` returns the array ``save_reader_predictions_memm`` would ``np.save``;
``predict_echograms_memm`` does so for a whole memm survey, its forward batches packed across the echograms, and
``evaluate_echograms_memm`` evaluates one (PR histograms) in the same way.  ``integrate_survey`` /
``integrate_echogram_memm`` / ``integrate_echograms_memm`` (a whole memm survey, packed) reduce the predictions on the GPU
instead of returning them: echo integration by predicted class (``crimac_integrate_classes``), the sv of one frequency
summed per class and (ping bin x range bin) cell -- or, with a seabed-aware ``IntegrationSpec``
(``crimac_integrate_layers``), only above a per-ping limit at the seabed line and per bottom layer counted from it.
"""
from __future__ import annotations

import contextlib
import ctypes
import difflib
import functools
import inspect
import itertools
import os
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import hip, parallel
from .hip import call, ptr

SEABED_PAD = 10        # mask_label_seabed.py:50-52
SEABED_MARGIN = 50     # gridded.py:150-156
INTERNAL_BATCH = 96    # patches per forward call (eval mode: results do not depend on the batch size)


def plan_chunks(start_ping, n_pings, preload_n_pings):
    """``get_data_split([[start, n_pings]], preload_n_pings)`` (preload_data_split.py:22-30)."""
    max_n = preload_n_pings if preload_n_pings > 0 else 5000          # save_predict.py:160-166
    n_splits = int(np.ceil((n_pings - start_ping) / max_n))
    edges = np.linspace(start_ping, n_pings, n_splits + 1).astype(int)
    return [(int(edges[i]), int(edges[i + 1])) for i in range(n_splits)]


def plan_grid(n_range, max_seabed, start_ping, end_ping, patch_size=(256, 256), patch_overlap=20):
    """Patch centres (range idx, ping idx), ping fastest: ``get_data_grid(mode='all')``
    (gridded.py:35-54) with the range extent capped at max seabed + 50 (:150-159)."""
    end_range = min(n_range, int(max_seabed) + SEABED_MARGIN)
    assert end_range > 0 and end_ping > start_ping
    pw, ph = patch_size
    ys = np.arange(-(patch_overlap + 1), end_range - (patch_overlap + 1), ph - 2 * patch_overlap) + ph // 2
    xs = np.arange(start_ping - (patch_overlap + 1), end_ping - (patch_overlap + 1),
                   pw - 2 * patch_overlap) + pw // 2
    return np.array(np.meshgrid(ys, xs)).T.reshape(-1, 2)


META_FLAGS = {"portion_year": 1, "portion_day": 2, "time_diff": 4, "depth_rel": 8, "depth_abs_surface": 16,
              "depth_abs_seabed": 32}          # planes come out in this order (batch/dataset.py:288-351)


def meta_flags(meta_channels):
    """The yaml's ``meta_channels`` dict -> (the `flags` of the metadata kernels, the number of planes they build)."""
    if set(meta_channels) != set(META_FLAGS) or not all(isinstance(v, bool) for v in meta_channels.values()):
        raise ValueError(f"meta_channels must be a dict of booleans with the keys {sorted(META_FLAGS)}")    # dataset.py:60-66
    flags = sum(f for k, f in META_FLAGS.items() if meta_channels[k])
    if flags == 0:
        raise ValueError("no metadata channel is switched on")
    return flags, sum((2 if k == "portion_day" else 1) for k in META_FLAGS if meta_channels[k])


class MetaSource:
    """The per-ping vectors the metadata planes of an echogram are built from (data_reader.py:98-100), resident on the
    GPU: ``crimac_meta_planes`` turns them into the ``[P, Cm, H, W]`` planes of a batch of crops -- what the reference's
    ``get_crop_memmap`` builds per patch in numpy DataLoader workers (batch/dataset.py:288-351)."""

    def __init__(self, meta_channels, portion_year, portion_day_vector, time_vector_diff, seabed, device):
        self.flags, self.n_planes = meta_flags(meta_channels)
        self.portion_year = float(portion_year)

        def dev(a, dt):
            return torch.as_tensor(np.ascontiguousarray(np.asarray(a)).astype(dt)).to(device)
        self.portion_day = dev(portion_day_vector, np.float64)
        self.time_diff = dev(time_vector_diff, np.float64)
        self.seabed = dev(seabed, np.int64)

    @classmethod
    def from_echogram(cls, echogram, meta_channels, device, seabed=None):
        """``seabed``: the vector to build the depth planes from when it is not the reader's own ``_seabed``."""
        return cls(meta_channels, echogram.portion_of_year_scalar, echogram.portion_of_day_vector,
                   echogram.time_vector_diff, echogram._seabed if seabed is None else seabed, device)

    def planes(self, centres_dev, patch_size):
        """centres_dev int32 [P, 2] (range idx, ping idx) on the GPU -> float32 [P, Cm, H, W]."""
        P = centres_dev.shape[0]
        H, W = int(patch_size[1]), int(patch_size[0])
        out = torch.empty((P, self.n_planes, H, W), dtype=torch.float32, device=centres_dev.device)
        with torch.cuda.device(centres_dev.device):
            call("crimac_meta_planes", ptr(centres_dev), P, H, W, self.flags, self.portion_year, ptr(self.portion_day),
                 self.portion_day.numel(), ptr(self.time_diff), self.time_diff.numel(), ptr(self.seabed),
                 self.seabed.numel(), ptr(out))
        return out


class ChunkPredictor:
    """GPU state of one preloaded chunk: data, labels, seabed; gathers, predicts, scatters."""

    def __init__(self, model, n_range, patch_size=(256, 256), patch_overlap=20, batch_size=32, out_f16=False):
        self.model = model
        self.engine = model.infer_engine        # (eval-mode forwards: the model's inference precision)
        self.n_range = n_range
        self.patch_size = tuple(int(v) for v in patch_size)
        self.patch_overlap = int(patch_overlap)
        self.batch_size = int(batch_size)
        self.out_f16 = bool(out_f16)
        self.flavour = "zarr"
        self.seabed = self.mask = self.mask_line = None
        # MetaSource: needed by a UNet_LateMetInject model (metadata planes per crop) and by an early-injection model
        # (UNet_Baseline whose input channels are the data planes + the metadata planes, gathered into the same crop)
        self.meta_source = None

    def _device(self):
        return self.engine.device or next(self.model.parameters()).device

    def load_chunk(self, data, data_ping0, labels, seabed_mask, start_ping, end_ping, seabed=None, seabed_ping0=None,
                   flavour="zarr", stream=None, wide=False):
        """data [C, pings, range] fp32 (global ping of column 0 = data_ping0; numpy or a pinned CPU tensor);
        labels [end-start, range] (or None); for pings [start_ping, end_ping) either ``seabed_mask``
        [end-start, range] uint8/bool (1 below the seabed, as the reader's get_seabed_mask(..., seabed_pad=0)) or
        -- cheaper, nothing to build on the host -- ``seabed`` [n] int seabed index per ping starting at global ping
        ``seabed_ping0`` (default start_ping).  ``stream``: copy stream for the uploads (the caller orders it).
        ``wide`` (the chunk of ``evaluate``): ``labels`` and ``seabed_mask`` cover the pings of ``data`` -- every ping a
        patch can touch -- not only [start_ping, end_ping), and no prediction array is allocated."""
        dev = self._device()
        nb = stream is not None

        def up(a, dtype):
            if a is None:
                return None
            if torch.is_tensor(a):          # already a tensor (pinned host staging or device resident): keep its dtype
                t = a
            else:
                t = torch.as_tensor(np.ascontiguousarray(np.asarray(a).astype(dtype, copy=False)))
            if stream is not None:
                with torch.cuda.stream(stream):
                    return t.to(dev, non_blocking=nb)
            return t.to(dev)

        self.data = up(data, np.float32)
        self.data_ping0 = int(data_ping0)
        self.labels = up(labels, np.int16)
        self.mask = up(seabed_mask, np.uint8)
        self.mask_line = None                # (the mask's limit line, built by the first seabed-aware integrate())
        self.seabed = up(seabed, np.int32)
        self.seabed_ping0 = int(start_ping if seabed_ping0 is None else seabed_ping0)
        self.start_ping, self.end_ping = int(start_ping), int(end_ping)
        self.flavour = flavour
        self.wide = bool(wide)
        if self.wide:
            self.out = None
            return
        self.out = torch.zeros((2, self.n_range, self.end_ping - self.start_ping),
                               dtype=torch.float16 if self.out_f16 else torch.float32, device=dev)

    def predict(self, grid, predict_fn=None, centres_dev=None, share_patches=True):
        """Run all patches of ``grid`` ([P,2] global centres) and scatter them into ``self.out``.

        ``share_patches`` (with torch.distributed initialised): the patches of THIS chunk are dealt round-robin to the
        ranks and the per-rank outputs are summed (one collective per chunk); False: this rank computes the whole chunk
        on its own (``predict_survey`` with chunk sharding: the ranks own different chunks, no collective at all).

        ``predict_fn(x_nhwc, P, H, W) -> probs [P,3,H,W]`` overrides the network (tests).
        ``centres_dev``: int32 [2, P, 2] on the GPU = (global centres, centres relative to the data slice), uploaded
        by the caller (a pageable host-to-device copy here would block the host until the stream has drained and
        serialise the enqueue of a chunk with the execution of the previous one)."""
        if self.wide:
            raise ValueError("ChunkPredictor.predict: the chunk was loaded for evaluate() (wide=True)")
        eng = self.engine
        eng.bind()
        ph, pw = self.patch_size[1], self.patch_size[0]
        rank, world = parallel.rank_world() if share_patches else (0, 1)
        mine = parallel.shard_indices(len(grid), rank, world)
        memm = self.flavour == "memm"
        self._check_meta()
        step = max(self.batch_size, INTERNAL_BATCH) if predict_fn is None else self.batch_size
        for b0 in range(0, len(mine), step):
            idx = mine[b0:b0 + step]
            P = len(idx)
            if centres_dev is not None and world == 1:
                cen_d, loc_d = centres_dev[0, b0:b0 + P], centres_dev[1, b0:b0 + P]
            else:
                cen_d, loc_d = self._centres(np.asarray(grid)[idx])
            x = self._gather(cen_d, loc_d, P)
            if predict_fn is not None:
                probs = predict_fn(x, P, ph, pw)
            elif eng.lmi:
                self._need_meta_source()
                meta = self.meta_source.planes(cen_d.contiguous(), self.patch_size)
                probs = eng.forward_nhwc(x, P, ph, pw, False, softmax=True, meta=meta)
            else:
                probs = eng.forward_nhwc_eval_split(x, P, ph, pw, softmax=True)
            call("crimac_scatter_patches_ex", ptr(probs), probs.shape[1], ptr(cen_d), P, ph, pw,
                 self.patch_overlap, self.start_ping, self.end_ping - self.start_ping, self.n_range,
                 ptr(self.labels), ptr(self.mask), self.start_ping, self.end_ping - self.start_ping,
                 ptr(self.seabed), self.seabed_ping0, 0 if self.seabed is None else self.seabed.numel(),
                 None if memm else ptr(self.data[0]), self.data_ping0, self.data.shape[1], SEABED_PAD,
                 1 if memm else 0, ptr(self.out), 1 if self.out_f16 else 0)
        if world > 1:
            torch.distributed.all_reduce(self.out)      # interiors are disjoint: sum == union (exact in fp16 too)
        return self.out

    def integrate(self, acc, cnt, spec):
        """Echo integration of the chunk ``predict`` has just filled (``crimac_integrate_classes``): the linear sv of
        ``self.data[spec.channel]`` summed per class and cell into ``acc`` float64 / ``cnt`` int64
        ``[3, n_pb_total, n_rb]`` on the GPU (``new_integration``), which cover global pings from 0.  ``spec``: a bound
        ``IntegrationSpec``; with a sequence of F frequencies ``acc`` / ``cnt`` are ``[F, 3, n_pb_total, n_rb]`` and ONE
        launch (``crimac_integrate_freqs``) reads the predictions once for all of them.  Launches on the current stream,
        after the scatter; nothing comes back.
        A seabed-aware spec (``seabed_offset`` given) runs ``crimac_integrate_layers`` with the chunk's seabed line
        (``_limit_line``: the vector, or the first masked row per ping of a chunk loaded with a 2-D mask); with the seabed
        reference the accumulators are ``[3, n_pb_total, layers]``.  A spec with ``ping_edges`` (a table: ``resolve`` a
        callable first) runs ``crimac_integrate_edges``; ``n_pb_total`` is then the table's number of cells exactly."""
        if self.wide or self.out is None:
            raise ValueError("ChunkPredictor.integrate: the chunk was loaded for evaluate() (wide=True) and has no predictions")
        if spec.channels is None or spec.channels[0] is None:
            raise ValueError("ChunkPredictor.integrate: bind the spec to the model's frequencies first (IntegrationSpec.bind)")
        for ch in spec.channels:
            if not 0 <= ch < self.data.shape[0]:
                raise ValueError(f"ChunkPredictor.integrate: channel {ch} of {self.data.shape[0]} data planes")
        n_pb, n_rb = spec.bins(self.end_ping, self.n_range)
        lead = (spec.n_freqs, 3) if spec.multi else (3,)
        n_acc = int(acc.shape[-2]) if acc.dim() == len(lead) + 2 else -1
        want = (*lead, n_acc, n_rb)
        if acc.dtype != torch.float64 or cnt.dtype != torch.int64 or tuple(acc.shape) != want or tuple(cnt.shape) != want \
                or n_acc < n_pb or (spec.ping_edges is not None and n_acc != n_pb) \
                or not acc.is_contiguous() or not cnt.is_contiguous():
            raise ValueError(f"ChunkPredictor.integrate: acc float64 / cnt int64, contiguous {list(lead)} + [>= {n_pb}, {n_rb}]; "
                             f"got {acc.dtype} {tuple(acc.shape)}, {cnt.dtype} {tuple(cnt.shape)}")
        n = self.end_ping - self.start_ping
        cells = spec.touched(self.start_ping, self.end_ping) * n_rb
        scratch = integration_scratch(self.engine, cells, spec.n_freqs)
        data = self.data
        if spec.multi and not data.is_contiguous():
            raise ValueError("ChunkPredictor.integrate: several frequencies need the chunk's data contiguous [C, pings, range]")
        sv = data[0] if spec.multi else data[spec.channel]           # (several frequencies: plane 0 and the plane stride)
        with torch.cuda.device(self.out.device):
            launch_integration(spec, ptr(self.out), self.out_f16, self.n_range, n, ptr(sv), int(sv.shape[0]),
                               self.start_ping - self.data_ping0, self.start_ping, n_acc, ptr(acc), ptr(cnt),
                               scratch, seabed=self._limit_line() if spec.seabed_aware else None,
                               plane_stride=int(data.stride(0)), n_planes=int(data.shape[0]))

    def detect_schools(self, spec, keep_left=False, keep_right=False):
        """The schools of the chunk ``predict`` has just filled: per class of ``spec`` (a bound ``SchoolSpec``) one
        ``crimac_schools_label`` of its plane of ``self.out`` and one ``crimac_schools_stats`` against the resident sv
        planes, on the current stream.  Returns a list of ``SchoolTable`` (device tensors, nothing has been waited for);
        ``SchoolTable.numpy()`` downloads one.  ``keep_left`` / ``keep_right``: keep every school that touches the first /
        last ping column whatever its size (the chunk has a neighbour there: ``merge_school_chunks``)."""
        self._check_schools("detect_schools", spec)
        return [SchoolTable(self, spec, k, bool(keep_left), bool(keep_right)) for k in spec.classes]

    def _check_schools(self, name, spec):
        if self.wide or self.out is None:
            raise ValueError(f"ChunkPredictor.{name}: the chunk was loaded for evaluate() (wide=True) and has no predictions")
        if spec.channels is None:
            raise ValueError(f"ChunkPredictor.{name}: bind the spec to the model's frequencies first (SchoolSpec.bind)")
        for ch in spec.channels:
            if not 0 <= ch < self.data.shape[0]:
                raise ValueError(f"ChunkPredictor.{name}: channel {ch} of {self.data.shape[0]} data planes")
        if not self.data.is_contiguous():
            raise ValueError(f"ChunkPredictor.{name}: the chunk's data must be contiguous [C, pings, range]")

    def score_schools(self, spec, keep_left=False, keep_right=False, ignored=True):
        """``detect_schools`` plus, per class, the ANNOTATED schools of the chunk -- the connected regions of the class's raw
        annotation id (27 / 1) in ``self.labels``, with the same connectivity, ``min_pixels`` and keep flags -- and the
        overlap of every (predicted, annotated) pair: pixels and per-frequency sv sums, from the table of the components of
        the intersection plane (``SchoolOverlaps``).  ``ignored``: also the pixels every predicted school shares with ids the
        label transform ignores (any id but 0, 27, 1).  All on the current stream; returns a list of ``SchoolScore`` (device
        tensors, nothing has been waited for).  Refuses what ``detect_schools`` refuses, and a chunk loaded without labels."""
        self._check_schools("score_schools", spec)
        n = self.end_ping - self.start_ping
        if self.labels is None:
            raise ValueError("ChunkPredictor.score_schools: the chunk was loaded without labels: there are no annotated schools "
                             "to score against")
        if self.labels.dtype != torch.int16 or tuple(self.labels.shape) != (n, self.n_range) or not self.labels.is_contiguous():
            raise ValueError(f"ChunkPredictor.score_schools: the chunk's labels must be contiguous int16 [{n}, {self.n_range}] "
                             f"(pings, range); got {self.labels.dtype} {tuple(self.labels.shape)}")
        plane = None
        if ignored:                                  # one plane for all classes: the ids no class maps to
            plane = types.SimpleNamespace(labels=self.engine._buf("schools.ignored", (self.n_range, n), torch.int32),
                                          status=torch.empty(1, dtype=torch.int32, device=self.out.device))
            with torch.cuda.device(self.out.device):
                call("crimac_schools_label_ids", ptr(self.labels), n, 0, self.n_range, n, SCHOOLS_IDS_IGNORED,
                     spec.connectivity, ptr(plane.labels), ptr(plane.status))
        return [SchoolScore(self, spec, k, bool(keep_left), bool(keep_right), plane) for k in spec.classes]

    def _limit_line(self):
        """The seabed line of a seabed-aware integration, as ``(pointer, index of ping start_ping, length)``: the chunk's
        seabed vector; for a chunk that holds a 2-D mask instead -- a zarr block the vector could not express
        (``seabed_vector_or_mask``) -- the first masked row of every ping, ``n_range`` where a ping has none, computed on
        the device once per chunk; a chunk with neither has no line: ValueError."""
        if self.seabed is not None:
            return ptr(self.seabed), self.start_ping - self.seabed_ping0, self.seabed.numel()
        if self.mask is None:
            raise ValueError("ChunkPredictor.integrate: a spec with seabed_offset needs the chunk's seabed vector or mask, "
                             "and the chunk was loaded with neither")
        if self.mask_line is None:
            below = self.mask != 0                               # [pings, range]; argmax: the FIRST maximal element
            first = below.to(torch.uint8).argmax(dim=1)
            self.mask_line = torch.where(below.any(dim=1), first, torch.full_like(first, self.n_range)).to(torch.int32)
        return ptr(self.mask_line), 0, self.mask_line.numel()

    def _early(self):       # metadata planes as extra input channels
        return not self.engine.lmi and self.engine.in_channels > self.data.shape[0]

    def _check_meta(self):
        """Early-injection models: what the chunk must bring along."""
        eng, ms, C = self.engine, self.meta_source, self.data.shape[0]
        if self._early():
            if ms is None:
                raise ValueError(f"the model takes {eng.in_channels} input channels and the chunk has {C} data planes: "
                                 "an early-injection model needs the metadata planes, set ChunkPredictor.meta_source "
                                 "(MetaSource.from_echogram(...))")
            if ms.n_planes != eng.in_channels - C:
                raise ValueError(f"the model takes {eng.in_channels - C} metadata input channels, meta_source builds "
                                 f"{ms.n_planes}")
            if self.flavour != "memm":
                raise NotImplementedError("metadata input channels: memm flavour only (the reference's preload path "
                                          "builds no metadata, batch/dataset.py:210-216)")

    def _need_meta_source(self):
        if self.meta_source is None:
            raise ValueError("a UNet_LateMetInject model needs the metadata planes: set ChunkPredictor.meta_source "
                             "(MetaSource.from_echogram(...))")

    def _centres(self, cen):
        """Grid rows [P, 2] (global centres) -> int32 [P, 2] (global centres, centres relative to the data slice) on the
        device, in one upload."""
        cen = np.asarray(cen).astype(np.int32)
        local = cen.copy()
        local[:, 1] -= self.data_ping0
        both = torch.from_numpy(np.ascontiguousarray(np.stack([cen, local]))).to(self.data.device)
        return both[0], both[1]

    def _gather(self, cen_d, loc_d, P, labels_t=None):
        """The network input of a batch of P patches, [P*ph*pw, 16] in the engine's storage type, cropped from the chunk by
        the gather kernel of its kind: zarr -- the data planes through db_with_limits; memm -- + set_data_border_value by
        the raw annotation ids; early injection -- + the metadata planes in channels C.., and db_with_limits_scaled
        (transforms.py:57-64).  ``labels_t`` int16 [P, ph, pw] (memm, ``evaluate`` with eval_mode 'region' / 'trace'): the
        transformed labels of the patches, which set_data_border_value then goes by instead of the raw ids."""
        eng, ms = self.engine, self.meta_source
        ph, pw = self.patch_size[1], self.patch_size[0]
        C, Wd = self.data.shape[0], self.data.shape[1]
        x = eng._buf("tiled.x", (P * ph * pw, 16))
        early = self._early()
        if labels_t is not None:
            vec = (ms.flags, ms.portion_year, ptr(ms.portion_day), ms.portion_day.numel(), ptr(ms.time_diff),
                   ms.time_diff.numel(), ptr(ms.seabed), ms.seabed.numel(), ptr(cen_d.contiguous())) if early else \
                  (0, 0.0, None, 0, None, 0, None, 0, None)
            call("crimac_gather_patches_memm_labels", eng.prec, ptr(self.data), C, Wd, self.n_range, ptr(loc_d), P, ph, pw,
                 ptr(x), 16, ptr(labels_t), 1 if early else 0, *vec)
        elif early:
            call("crimac_gather_patches_memm_meta", eng.prec, ptr(self.data), C, Wd, self.n_range, ptr(loc_d), P, ph, pw,
                 ptr(x), 16, ptr(self.labels), 1, ms.flags, ms.portion_year, ptr(ms.portion_day), ms.portion_day.numel(),
                 ptr(ms.time_diff), ms.time_diff.numel(), ptr(ms.seabed), ms.seabed.numel(), ptr(cen_d.contiguous()))
        elif self.flavour == "memm":
            call("crimac_gather_patches_memm", eng.prec, ptr(self.data), C, Wd, self.n_range, ptr(loc_d), P, ph, pw,
                 ptr(x), 16, ptr(self.labels))
        else:
            call("crimac_gather_patches", eng.prec, ptr(self.data), C, Wd, self.n_range, ptr(loc_d), P, ph, pw,
                 ptr(x), 16)
        return x

    def evaluate(self, grid, hist, eval_mode="all", boxes=None, predict_fn=None, on_batch=None, classes=None,
                 integration=None):
        """Test-set evaluation of the patches of ``grid`` ([P, 2] global centres) on a ``wide`` chunk: what the reference's
        gridded test Dataset + ``get_predictions_dataloader`` + the masking of ``validate_model_testing`` do per patch
        (batch/dataset.py:207-242; pipeline.py:242-282, :347-353), accumulated into ``hist`` (int32 [2, 16384] on the GPU:
        the float16 sandeel probability of the valid pixels, by label == SANDEEL / the rest).

        Per internal batch: ``crimac_gather_eval_crops`` (RAW linear-sv crops and raw annotation ids) ->
        ``crimac_labels_test_transform`` (+ ``crimac_labels_extend_mask`` with ``boxes`` for ``eval_mode`` 'region' /
        'trace'; ``boxes`` int32 [n, 4] on the GPU, already extended: ``eval_boxes``) -> network input -> eval forward
        (logits) -> ``crimac_pr_histogram``.  The network input follows the reference's per-patch chain: zarr -- the raw
        crop through remove_nan_inf + db_with_limits (``augment_batch``; the crop's nan_to_num came first, so an inf
        sample reaches the network as 0 dB, not as -75 dB as on the preload path); memm -- gathered straight from the
        chunk, ending with set_data_border_value (define_data_transform_test): 'all' -- by the raw ids,
        ``crimac_gather_patches_memm`` (``_meta``) exactly as ``predict`` feeds it; 'region' / 'trace' -- the extended mask
        has turned -100 pixels outside the boxes into -1 BEFORE set_data_border_value looks for -100
        (batch/dataset.py:229-235), so the rule goes by the TRANSFORMED labels: ``crimac_gather_patches_memm_labels``,
        with or without metadata planes.
        ``predict_fn(x_nhwc, P, H, W) -> logits [P, 3, H, W]`` replaces the network; ``on_batch(centres [P, 2] numpy,
        labels int16 [P, H, W], logits [P, 3, H, W])`` sees the transformed labels and the logits of every batch, on the
        GPU (tests).
        ``classes`` (a tuple of foreground class indices, ``check_classes``): ``hist`` is int32 [n_classes, 2, 16384] and
        row c takes the float16 probability of class c, by label == c / the rest, for every c of ``classes`` in one
        ``crimac_pr_histogram_classes`` pass per batch; a below-seabed pixel counts in ``neg`` of each with probability 0.
        ``integration`` (a ``ScoredIntegration`` that has begun): every batch is also reduced by
        ``crimac_integrate_confusion``, right after its histograms and on the same stream, from the raw crops, the
        transformed labels and the logits it has on the GPU anyway; None: no launch, no buffer."""
        classes = model_classes(classes, self.engine, hist)
        if integration is not None:
            if not isinstance(integration, ScoredIntegration):
                raise TypeError(f"integration is a ScoredIntegration, got {type(integration).__name__}")
            if self.engine.n_classes != 3:
                raise ValueError(f"integration=: the model has n_classes={self.engine.n_classes}, the scored integration "
                                 "is that of a 3-class model")
        if not self.wide:
            raise ValueError("ChunkPredictor.evaluate needs a chunk loaded with wide=True (labels and seabed for every "
                             "ping a patch can touch)")
        if eval_mode not in ("all", "region", "trace"):
            raise ValueError(f"eval_mode={eval_mode!r}: 'all', 'region' or 'trace' (batch/transforms.py:87)")
        if (boxes is not None) != (eval_mode != "all"):
            raise ValueError(f"eval_mode={eval_mode!r} goes with boxes {'given' if eval_mode != 'all' else 'None'}")
        if self.labels is None:
            raise ValueError("ChunkPredictor.evaluate needs the annotation ids of the chunk")
        eng = self.engine
        eng.bind()
        ph, pw = self.patch_size[1], self.patch_size[0]
        C, Wd = self.data.shape[0], self.data.shape[1]
        if tuple(self.labels.shape) != (Wd, self.n_range):
            raise ValueError(f"labels {tuple(self.labels.shape)} do not cover the data extent {(Wd, self.n_range)}")
        memm = self.flavour == "memm"
        self._check_meta()
        early = self._early()
        if eng.lmi:
            self._need_meta_source()
        if (eng.lmi or early) and not memm:
            raise NotImplementedError("metadata planes: memm flavour only (the zarr path builds none)")
        grid = np.asarray(grid)
        step = max(self.batch_size, INTERNAL_BATCH) if predict_fn is None else self.batch_size
        for b0 in range(0, len(grid), step):
            cen = grid[b0:b0 + step].astype(np.int32)
            P = len(cen)
            cen_d, loc_d = self._centres(cen)
            raw = eng._buf("eval.raw", (P, C, ph, pw), torch.float32)
            lab = eng._buf("eval.lab", (P, ph, pw), torch.int16)
            call("crimac_gather_eval_crops", ptr(self.data), C, Wd, self.n_range, ptr(self.labels), ptr(loc_d), P, ph,
                 pw, 1 if memm else 0, ptr(raw), ptr(lab))
            chain = dict(thr_channel=C - 1, seabed=self.seabed, seabed_ping0=self.seabed_ping0,
                         seabed_pings=0 if self.seabed is None else self.seabed.numel(), mask=self.mask,
                         mask_ping0=self.data_ping0, mask_pings=0 if self.mask is None else self.mask.shape[0],
                         n_range=self.n_range, pad=SEABED_PAD, seabed_rule=1 if memm else 0, overlap=self.patch_overlap,
                         boxes=boxes)
            cen64 = cen_d.long().contiguous()
            if memm:
                labels_t = transform_test_labels(raw, lab, cen64, **chain)
                x = self._gather(cen_d, loc_d, P, labels_t if boxes is not None else None)
                meta = self.meta_source.planes(cen_d, self.patch_size) if eng.lmi else None
                logits = eval_logits(eng, x, P, ph, pw, meta=meta, predict_fn=predict_fn, split=True)
            else:
                logits, labels_t = raw_crops_to_logits(eng, raw, lab, cen64, predict_fn=predict_fn, split=True, **chain)
            if on_batch is not None:
                on_batch(cen, labels_t, logits)
            add_pr_histograms(logits, labels_t, hist, classes)
            if integration is not None:
                integration.add_batch(eng, logits, raw, labels_t, cen_d, self.n_range, memm)
        return hist


def transform_test_labels(data, labels, centres, *, thr_channel, seabed, seabed_ping0, seabed_pings, mask, mask_ping0,
                          mask_pings, n_range, pad, seabed_rule, overlap, boxes):
    """define_label_transform_test (batch/transforms.py:78-92) of a batch of RAW crops on the GPU: data [B, C, H, W] fp32
    linear sv, labels [B, H, W] raw annotation ids, centres int64 [B, 2] (range idx, global ping idx) -> transformed int16
    labels [B, H, W].  ``crimac_labels_test_transform`` (seabed vector OR mask, as ``crimac_scatter_patches_ex`` takes
    them) -> ``crimac_labels_extend_mask`` when ``boxes`` is given (eval_mode 'region' / 'trace')."""
    B, C, H, W = data.shape
    out = torch.empty((B, H, W), dtype=torch.int16, device=data.device)
    with torch.cuda.device(data.device):
        call("crimac_labels_test_transform", ptr(labels), labels.element_size(), ptr(data), thr_channel, 1e-7, 1e-4,
             ptr(centres), ptr(seabed), seabed_ping0, seabed_pings, ptr(mask), mask_ping0, mask_pings, n_range, pad,
             seabed_rule, overlap, ptr(out), B, C, H, W)
        if boxes is not None:
            call("crimac_labels_extend_mask", ptr(out), ptr(data), C, ptr(centres), ptr(boxes), int(boxes.shape[0]), -1,
                 B, H, W)
    return out


def eval_logits(eng, x, B, H, W, meta=None, predict_fn=None, split=False):
    """Eval forward of a network input ``x`` [B*H*W, 16] -> logits [B, ncls, H, W]: ``predict_fn(x, B, H, W)`` when given,
    else the engine (``split``: the two-stream form of the tiled path, which takes no metadata planes)."""
    with torch.no_grad(), torch.cuda.device(x.device):
        if predict_fn is not None:
            return predict_fn(x, B, H, W)
        if split and meta is None:
            return eng.forward_nhwc_eval_split(x, B, H, W, softmax=False)
        return eng.forward_nhwc(x, B, H, W, training=False, meta=meta)


def raw_crops_to_logits(eng, data, labels, centres, *, thr_channel, seabed, seabed_ping0, seabed_pings, mask, mask_ping0,
                        mask_pings, n_range, pad, seabed_rule, overlap, boxes, db_scaled=False, meta=None, batch_in=None,
                        n_data=None, predict_fn=None, split=False, border_to_0db=False):
    """Batches of RAW crops that have no resident chunk behind them -- the DataLoader flow
    (``SegPipe._predict_raw_batch``) and the zarr flavour of ``ChunkPredictor.evaluate``: data [B, C, H, W] fp32 linear sv,
    labels [B, H, W] raw annotation ids, centres int64 [B, 2] (range idx, global ping idx), all on the GPU ->
    (logits [B, ncls, H, W], transformed int16 labels [B, H, W]).

    ``transform_test_labels`` -> network input: remove_nan_inf + db_with_limits of
    ``data`` -- of ``batch_in`` = data | metadata planes with ``n_data`` data channels for an early-injection model ->
    ``eval_logits``.
    ``border_to_0db``: set_data_border_value by the TRANSFORMED labels (the memm flavour's define_data_transform_test,
    transforms.py:57-64): a pixel whose label came out as -100 enters the dB transform as 1.0 and leaves it as 0.0 dB.
    (A resident memm chunk gets the same from ``crimac_gather_patches_memm_labels`` in one pass.)"""
    B, C, H, W = data.shape
    out = transform_test_labels(data, labels, centres, thr_channel=thr_channel, seabed=seabed, seabed_ping0=seabed_ping0,
                                seabed_pings=seabed_pings, mask=mask, mask_ping0=mask_ping0, mask_pings=mask_pings,
                                n_range=n_range, pad=pad, seabed_rule=seabed_rule, overlap=overlap, boxes=boxes)
    with torch.no_grad(), torch.cuda.device(data.device):
        if border_to_0db:
            data = data.masked_fill((out == -100).unsqueeze(1), 1.0)
        if batch_in is not None:         # remove_nan_inf + db_with_limits_scaled of the data planes, the rest as it is
            x, _ = eng.augment_batch(batch_in, None, 0, do_noise=False, do_flip=False, db_scaled=True, n_data=n_data)
        else:
            x, _ = eng.augment_batch(data, None, 0, do_noise=False, do_flip=False, db_scaled=db_scaled)
    return eval_logits(eng, x, B, H, W, meta=meta, predict_fn=predict_fn, split=split), out


def eval_boxes(reader, eval_mode, extend_size=20):
    """School bounding boxes (y0, y1, x0, x1) as ``crimac_labels_extend_mask`` takes them for ``eval_mode`` 'region' /
    'trace' (get_extended_label_mask_for_crop, extend_label_masks.py:57-80), int32 [n, 4] numpy; None for 'all'.  The
    reference asks the reader for get_object_bounding_boxes(), which only its memmap Echogram defines
    (data_reader.py:404) -- a zarr reader without it fails there with an AttributeError."""
    if eval_mode == "all":
        return None
    if eval_mode not in ("region", "trace"):
        raise ValueError(f"eval_mode={eval_mode!r}: 'all', 'region' or 'trace' (batch/transforms.py:87)")
    if not hasattr(reader, "get_object_bounding_boxes"):
        raise NotImplementedError(
            f"eval_mode={eval_mode!r}: the reader has no get_object_bounding_boxes() (the reference's "
            "get_extended_label_mask_for_crop needs it, extend_label_masks.py:67); use eval_mode='all'")
    bb = np.array(reader.get_object_bounding_boxes(), dtype=np.int64).reshape(-1, 4)
    if eval_mode == "region":
        bb[:, 0] -= int(extend_size)
        bb[:, 1] += int(extend_size)
    else:
        bb[:, 0] = 0
        bb[:, 1] = int(reader.shape[0])          # (the reference's `echogram.shape[0]`, :78)
    bb[:, 2] -= int(extend_size)
    bb[:, 3] += int(extend_size)
    return np.ascontiguousarray(bb.astype(np.int32))


def seabed_vector_or_mask(reader, s, e, n_range, sb, sb_ping0):
    """The scatter kernel rebuilds the reader's 2-D seabed mask (``get_seabed_mask``: 1 below the seabed, what
    ``mask_label_seabed`` uses, mask_label_seabed.py:47-49) from the seabed VECTOR as ``range >= seabed[ping]``.  The zarr
    reader derives that vector as ``argmax(range)`` of the stored mask (data_reader.py:864-865), so the two agree only
    where the mask of a ping is exactly "zeros, then ones to the end": a ping with NO detected bottom has an all-zero
    mask (``fillna(0)``) and argmax 0 -- the vector rule would mask its whole water column, the reference masks
    nothing -- a mask with holes is not a threshold at all, and a reader whose ``get_seabed`` is independent of its mask
    (the memmap reader's seabed.npy) may simply disagree with it.  Checked here per chunk, EXACTLY, on the reader's own
    mask (read once) for the pings [s, e) the chunk writes: the mask must equal ``arange(n_range) >= vector`` element for
    element; no-bottom pings get seabed = n_range (nothing below it); anything the vector cannot express is returned as
    uint8 [e - s, n_range] to be uploaded instead (``ChunkPredictor.load_chunk``).

    Returns (seabed vector to upload, mask or None).  ``sb`` covers pings [sb_ping0, sb_ping0 + len(sb))."""
    if not hasattr(reader, "get_seabed_mask"):
        return sb, None
    m = reader.get_seabed_mask(int(s), int(e - s), 0, int(n_range), return_numpy=True)
    m = np.asarray(getattr(m, "values", m))
    if m.shape != (e - s, n_range):
        raise ValueError(f"get_seabed_mask returned {m.shape}, expected {(e - s, n_range)}")
    below = m != 0
    vec = np.asarray(sb[s - sb_ping0:e - sb_ping0]).astype(np.int64)
    none = ~below.any(axis=1)
    vec_eff = np.where(none, n_range, vec)                   # no bottom detected: nothing lies below it
    if np.array_equal(below, np.arange(n_range)[None, :] >= vec_eff[:, None]):
        if none.any():
            sb = sb.copy()
            sb[s - sb_ping0:e - sb_ping0] = vec_eff
        return sb, None
    return sb, np.ascontiguousarray(below.astype(np.uint8))


class _OrderedHandoff:
    """Chunk-sharded inference, one writer: ranks r > 0 send each finished chunk to rank 0, which yields the whole survey
    in ping order (``predict_survey(ordered_to_rank0=True)``).  Point-to-point only: ``isend`` / ``irecv`` of one
    ``[2, n_range, pings]`` tensor per chunk -- under RCCL ("nccl") the DEVICE tensor the scatter kernel wrote (device to
    device over xGMI; the sender does no D2H copy at all), under gloo a host tensor.  Chunk i belongs to rank i % N, so
    rank 0 walks the survey in rounds of N chunks: it posts the N - 1 receives of a round, runs its own chunk of the
    round (its pipeline already works on the next one), then takes the received chunks in rank order."""

    MAX_IN_FLIGHT = 2          # sends a rank keeps outstanding before it waits for the oldest (back-pressure)

    def __init__(self, rank, world, all_chunks, n_range, out_dtype):
        self.rank, self.world, self.all_chunks, self.n_range = rank, world, all_chunks, n_range
        self.device_tensors = torch.distributed.get_backend() == "nccl"
        self.tdtype = torch.float16 if out_dtype == np.float16 else torch.float32
        self.inflight = []
        self.bufs = {}

    # -- ranks r > 0 --------------------------------------------------------------------------------------------
    def send(self, out):
        t = out if self.device_tensors else out.cpu()       # (cp.out is a fresh tensor per chunk: safe to keep)
        self.inflight.append((torch.distributed.isend(t.contiguous(), dst=0), t))
        while len(self.inflight) > self.MAX_IN_FLIGHT:
            self.inflight.pop(0)[0].wait()

    def flush(self):
        for req, _ in self.inflight:
            req.wait()
        self.inflight = []
        if self.device_tensors:
            torch.cuda.current_stream().synchronize()

    # -- rank 0 -------------------------------------------------------------------------------------------------
    def _buf(self, r, n_pings, device):
        key = (r, n_pings)
        if key not in self.bufs:
            self.bufs[key] = torch.empty((2, self.n_range, n_pings), dtype=self.tdtype,
                                         device=device if self.device_tensors else "cpu")
        return self.bufs[key]

    def merge(self, own):
        """``own``: rank 0's generator over ITS chunks (0, N, 2N, ...) -> every chunk of the survey in ping order."""
        device = torch.device("cuda", torch.cuda.current_device()) if self.device_tensors else None
        own = iter(own)
        for k0 in range(0, len(self.all_chunks), self.world):
            reqs = []
            for r in range(1, self.world):
                if k0 + r < len(self.all_chunks):
                    s, e = self.all_chunks[k0 + r]
                    buf = self._buf(r, e - s, device)
                    reqs.append((s, e, buf, torch.distributed.irecv(buf, src=r)))
            yield next(own)
            for s, e, buf, req in reqs:
                req.wait()
                yield s, e, buf.cpu().numpy() if self.device_tensors else buf.numpy().copy()      # (.cpu() is a fresh array; the host buffer is reused)


_STAGING = {}          # _ChunkFeed.key -> the staging set (pinned host slots, device slots, the caller's extras) kept last


def release_staging():
    """Give back the staging buffers ``predict_survey`` keeps between surveys of the same geometry (for a 4096-ping
    preload: ~0.5 GB of pinned host memory and ~0.3 GB of device memory)."""
    _STAGING.clear()


class _ChunkFeed:
    """The chunk pipeline of ``predict_survey``, ``evaluate_survey`` and ``_MemmSurveyFlow`` (the memm survey flows, whose
    chunk is a group of echograms): reader threads fill pinned host slots ahead of the GPU, a copy stream uploads each
    chunk into one of two device slots while the chunk before it computes.  ``jobs`` is any iterable, taken from lazily.

    ``table`` {name: (elements, dtype)}: the flat buffers a chunk is staged in, one of each per host slot and per device
    slot.  The set (+ the caller's ``extra()`` buffers) is kept in ``_STAGING`` between surveys of the same key -- ``tag``
    (names the flow and whatever ``extra`` depends on), device, table, ``host_slots`` -- and is busy inside ``with``.
    ``read(job, slot) -> (uploads, payload)`` runs on a reader thread and makes no GPU call of its own: ``slot()`` waits
    until the host slot may be overwritten and returns its {name: pinned buffer}; ``uploads`` {name: view of that
    buffer, or None} goes to the device, ``payload`` is whatever else the chunk's compute needs.
    Iterating yields ``({name: device view or None}, payload)`` per job, ordered before the current stream; the caller
    enqueues the chunk's compute there and then calls ``computed()``.  ``note(key, t0)``: host-timing hook
    (``wait_fetch_s``, ``enq_upload_s``); ``t_taken`` / ``t_uploaded``: when the read was taken / the uploads enqueued."""
    # Slot reuse.  Chunk j lives in host slot j % host_slots and in device slot j & 1.  host_slots is the read-ahead depth
    # + 1: while chunk i is uploaded the reads of chunks i+1 .. i+depth run.  The read of chunk j is SUBMITTED only after the
    # `uploaded` event of chunk j - host_slots, the last user of its host slot, has been RECORDED: the reader's wait on that
    # event is then a wait for that very upload.  The upload of chunk j waits for the `computed` event of chunk j - 2.

    def __init__(self, dev, tag, table, host_slots, jobs, read, extra=None, note=None):
        self.dev, self.table, self.slots, self.jobs, self.read, self.extra = dev, dict(table), host_slots, jobs, read, extra
        self.note = note or (lambda key, t0: None)
        self.key = (tag, str(dev), tuple(self.table.items()), host_slots)

    def _allocate(self):
        def slot(**where):
            return {name: torch.empty(n, dtype=dt, **where) for name, (n, dt) in self.table.items()}
        return dict({"host": [{name: t.pin_memory() for name, t in slot().items()} for _ in range(self.slots)],
                     "dev": [slot(device=self.dev) for _ in range(2)], "busy": False}, **(self.extra() if self.extra else {}))

    def __enter__(self):
        self.uploaded = [torch.cuda.Event() for _ in range(self.slots)]   # host slot may be overwritten once this has passed
        self.computed_ev = [torch.cuda.Event() for _ in range(2)]         # device slot may be overwritten once this has passed
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.main = torch.cuda.current_stream()
        self.n_uploaded = self.n_submitted = 0        # (a feed is iterated once per ``with``)
        bufs = _STAGING.get(self.key)
        if bufs is None or bufs["busy"]:     # (busy: another flow over the same geometry is still running: a private set)
            fresh = self._allocate()
            if bufs is None:
                _STAGING.clear()             # (one geometry at a time: the buffers are large)
                _STAGING[self.key] = fresh
            bufs = fresh
        self.pool = ThreadPoolExecutor(max_workers=self.slots - 1)
        self.bufs = bufs
        bufs["busy"] = True
        return self

    def __exit__(self, *exc):
        self.pool.shutdown(wait=True)                 # (no reader of this survey still writes the staging ...
        torch.cuda.current_stream().synchronize()     #  ... and nothing on the GPU still reads or writes it)
        self.bufs["busy"] = False

    def _submit(self, j, job):
        assert j - self.slots < self.n_uploaded, "chunk feed: the last upload from this host slot has not been recorded"
        ev, host = self.uploaded[j % self.slots], self.bufs["host"][j % self.slots]

        def slot():
            ev.synchronize()                          # (no-op until the slot has been used)
            return host
        return self.pool.submit(self.read, job, slot)

    def __iter__(self):
        # ``jobs`` is any iterable and is consumed lazily, on this thread: job i + depth is taken from it when job i is
        # handed out (``predict_echograms_memm`` plans its groups from an iterator of echograms as it goes)
        depth, jobs, futs = self.slots - 1, iter(self.jobs), []

        def submit():
            for job in itertools.islice(jobs, 1):
                futs.append(self._submit(self.n_submitted, job))
                self.n_submitted += 1
        assert self.n_submitted == 0, "chunk feed: iterated twice inside one `with`"
        for _ in range(depth):
            submit()
        i = -1
        while futs:
            i += 1
            t0 = time.perf_counter()
            uploads, payload = futs.pop(0).result()
            self.note("wait_fetch_s", t0)
            self.t_taken = time.perf_counter()
            submit()
            self.slot = i & 1
            views = dict.fromkeys(uploads)
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(self.computed_ev[self.slot])
                for name, t in uploads.items():
                    if t is not None:
                        views[name] = self.bufs["dev"][self.slot][name][:t.numel()].view(t.shape)
                        views[name].copy_(t, non_blocking=True)
                self.uploaded[i % self.slots].record()
            self.n_uploaded = i + 1
            self.note("enq_upload_s", self.t_taken)
            self.t_uploaded = time.perf_counter()
            self.main.wait_stream(self.copy_stream)
            yield views, payload

    def computed(self):
        """The compute of the chunk handed out last has been enqueued on the current stream."""
        self.computed_ev[self.slot].record()


def _load_staged(cp, data, lo, labels, s, e, seabed, mask, wide=False):
    """``load_chunk`` of an uploaded chunk whose data (and ``seabed`` vector) start at ping ``lo``: by the seabed vector,
    or -- ``seabed_vector_or_mask`` found a mask the vector rule cannot express -- by that mask, uploaded as it is."""
    if mask is None:
        cp.load_chunk(data, lo, labels, None, s, e, seabed=seabed, seabed_ping0=lo, wide=wide)
    else:
        cp.load_chunk(data, lo, labels, mask, s, e, wide=wide)


class _SurveyChunks:
    """What ``predict_survey`` and ``integrate_survey`` share: the chunk plan of a zarr survey, the reader-thread ``fetch``
    into pinned staging, the staging table of their ``_ChunkFeed``, and the per-chunk loop body -- load the uploaded chunk,
    predict it, mark its device slot computed.  ``name``: the caller, for messages; ``f16``: the type of ``cp.out``."""

    def __init__(self, name, reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings, start_ping,
                 labels_available, f16, stats, predict_fn, share_patches):
        self.name, self.reader, self.segpipe, self.stats, self.predict_fn = name, reader, segpipe, stats, predict_fn
        self.patch_size, self.patch_overlap, self.labels_available = patch_size, patch_overlap, labels_available
        self.share_patches = share_patches
        self.n_pings, self.n_range = reader.shape
        self.dev = segpipe.device
        model = segpipe.model.to(self.dev).eval()
        self.cp = ChunkPredictor(model, self.n_range, patch_size, patch_overlap, batch_size, out_f16=f16)
        self.all_chunks = self.chunks = plan_chunks(start_ping, self.n_pings, preload_n_pings)
        self.n_freq = len(segpipe.frequencies)

    def note(self, key, t0):
        if self.stats is not None:
            self.stats.setdefault(key, []).append(time.perf_counter() - t0)

    def own(self, rank, world):
        """Chunk sharding: this rank keeps chunks rank, rank + world, ..."""
        self.chunks = self.chunks[rank::world]

    def check_model(self):
        cp, n_freq = self.cp, self.n_freq
        if not cp.engine.lmi and cp.engine.in_channels > n_freq:
            raise NotImplementedError(f"{self.name}: the model takes {cp.engine.in_channels} input channels for "
                                      f"{n_freq} frequencies (metadata planes as input channels); the zarr preload path has "
                                      "no metadata (batch/dataset.py:210-216) -- use predict_echogram_memm(meta_channels=...)")

    def feed(self, tag, extra=None):
        """The ``_ChunkFeed`` over this rank's chunks (3 host slots: two chunks are being read while one is uploaded)."""
        patch_size, patch_overlap, n_range, n_freq = self.patch_size, self.patch_overlap, self.n_range, self.n_freq
        self.widest = widest = max(e - s for s, e in self.chunks)
        halo = patch_size[1]
        n_data = n_freq * (widest + 2 * halo) * n_range
        max_patches = 4 * (widest // (patch_size[0] - 2 * patch_overlap) + 2) * (n_range // (patch_size[1] - 2 * patch_overlap) + 2)
        self.n_misc = (widest + 2 * halo) + 4 * max_patches       # int32: seabed | global centres | slice-relative centres
        # staging (pinned host + device) is kept between surveys of the same geometry: page-locking 3 x 75 MB + the result
        # buffers costs 10-20 ms per call, a tenth of a 65536-ping survey
        table = {"data": (n_data, torch.float32), "lab": (widest * n_range, torch.int16), "misc": (self.n_misc, torch.int32)}
        return _ChunkFeed(self.dev, tag, table, 3, self.chunks, self.fetch, extra=extra, note=self.note)

    def fetch(self, chunk, slot):
        reader, segpipe, patch_size, patch_overlap = self.reader, self.segpipe, self.patch_size, self.patch_overlap
        n_pings, n_range, n_freq, n_misc = self.n_pings, self.n_range, self.n_freq, self.n_misc
        t0 = time.perf_counter()
        s, e = chunk
        # ping extent of the data a patch of the chunk can touch (dataset.py:175-177): the patch columns depend on
        # (s, e) only, so the seabed of [lo, hi) -- which contains [s, e) -- is read ONCE (the zarr reader derives it from
        # the full 2-D mask every time, data_reader.py:864-865)
        xs = np.arange(s - (patch_overlap + 1), e - (patch_overlap + 1), patch_size[0] - 2 * patch_overlap) + patch_size[0] // 2
        lo = max(0, int(xs[0]) - patch_size[1] // 2)
        hi = min(n_pings, int(xs[-1]) + patch_size[1] // 2)
        sb = np.asarray(reader.get_seabed(lo, hi - lo, return_numpy=True)).astype(np.int32)
        seabed = sb[max(s - lo, 0):e - lo] if lo <= s else np.asarray(reader.get_seabed(s, e - s, return_numpy=True)).astype(np.int32)
        grid = plan_grid(n_range, int(seabed.max()), s, e, patch_size, patch_overlap)
        assert lo == max(0, int(grid[0, 1]) - patch_size[1] // 2) and hi == min(n_pings, int(grid[-1, 1]) + patch_size[1] // 2)
        host = slot()
        data = reader.get_data_slice(idx_ping=lo, n_pings=hi - lo, frequencies=segpipe.frequencies,
                                     return_numpy=True)
        d_t = host["data"][:n_freq * (hi - lo) * n_range].view(n_freq, hi - lo, n_range)     # contiguous
        np.copyto(d_t.numpy(), data, casting="same_kind")
        l_t = None
        if self.labels_available:
            lab = reader.get_label_slice(idx_ping=s, n_pings=e - s, return_numpy=True)
            l_t = host["lab"][:(e - s) * n_range].view(e - s, n_range)
            np.copyto(l_t.numpy(), lab, casting="unsafe")
        # the seabed of every ping a patch of the chunk can touch (the scatter kernel evaluates the mask from it)
        sb, mask = seabed_vector_or_mask(reader, s, e, n_range, sb, lo)
        P = len(grid)
        assert (hi - lo) + 4 * P <= n_misc, "misc staging too small"
        m = host["misc"].numpy()
        m[:hi - lo] = sb
        cen = np.asarray(grid, dtype=np.int32)
        m[hi - lo:hi - lo + 2 * P] = cen.reshape(-1)
        loc = cen.copy()
        loc[:, 1] -= lo
        m[hi - lo + 2 * P:hi - lo + 4 * P] = loc.reshape(-1)
        self.note("fetch_s", t0)
        return {"data": d_t, "lab": l_t, "misc": host["misc"][:hi - lo + 4 * P]}, (s, e, lo, hi, grid, mask)

    def predicted(self, feed, then=None):
        """Per chunk of ``feed``: load, predict, ``then(cp)`` -- whatever else reads the chunk's device slot --, mark the
        slot computed; yields ``(i, s, e, cp.out)`` with all of that enqueued."""
        cp, stats, note = self.cp, self.stats, self.note
        for i, (d, (s, e, lo, hi, grid, mask)) in enumerate(feed):
            P = len(grid)
            if stats is not None:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
            _load_staged(cp, d["data"], lo, d["lab"], s, e, d["misc"][:hi - lo], mask)
            note("enq_load_s", feed.t_uploaded)
            t1 = time.perf_counter()
            out = cp.predict(grid, predict_fn=self.predict_fn, centres_dev=d["misc"][hi - lo:].view(2, P, 2),
                             share_patches=self.share_patches)
            note("enq_predict_s", t1)
            if then is not None:
                then(cp)
            if stats is not None:
                ev1.record()
                stats.setdefault("gpu_events", []).append((ev0, ev1))
            feed.computed()
            yield i, s, e, out


def predict_survey(reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings,
                   start_ping=0, labels_available=True, out_dtype=np.float32, stats=None, predict_fn=None,
                   shard="chunk", ordered_to_rank0=False, **kwargs):
    """Generator over chunks: yields ``(start_ping, end_ping, out[2, n_range, end-start] numpy)``.

    Multi-GPU (torch.distributed initialised, one process per GPU).  EVERY rank must iterate the
    generator to its end.
      ``shard="chunk"`` (default) -- rank r owns chunks r, r + N, r + 2N, ...: every rank reads, uploads and predicts
          only ITS ping ranges; the reader I/O and the PCIe traffic scale with the ranks too.  What the generators yield
          is set by ``ordered_to_rank0``:
            True (opt-in) -- the finished float16 / float32 chunks are handed to rank 0
              point-to-point (one send per chunk, 16.8 MB as float16; RCCL: device to device over xGMI, off the compute
              stream; gloo: host tensors) and RANK 0 YIELDS EVERY CHUNK OF THE SURVEY IN PING ORDER, the other ranks
              yield nothing: the reference's strictly sequential writer (``append_to_zarr`` with
              ``append_dim='ping_time'`` and resume by ``sizes['ping_time']``, save_predict.py:107-134) runs unchanged on
              rank 0, and a caller that writes on rank 0 only loses nothing.  Rank 0 MUST then consume every chunk: the
              other ranks block in their sends (gloo) or queue them on RCCL's stream until rank 0 has posted the matching
              receive -- a consumer that stops early on rank 0 (exception, ``break``, resume logic) strands them until the
              process group's timeout, which is why this form has to be asked for;
            False (default) -- no communication at all: each rank yields its OWN chunks only (disjoint ping ranges); for
              callers that write regions themselves.
      ``shard="patch"`` -- every rank walks every chunk, takes patches p = rank (mod N) of it and the per-rank float16
          outputs are summed (one all-reduce of the chunk per chunk): every rank yields every chunk.

    ``reader``: the reference's zarr reader API (shape, get_data_slice, get_label_slice, get_seabed);
    ``segpipe``: a ``SegPipeUNet`` with loaded parameters.  ``out_dtype=np.float16`` returns what the reference
    stores (save_predict.py:212) and halves the bytes that come back; float32 (default) keeps full probabilities.
    ``predict_fn(x_nhwc, P, H, W) -> probs [P,3,H,W]`` replaces the network (tests of the plumbing).

    Three stages overlap: a host thread reads chunk i+1 from ``reader`` straight into pinned staging buffers
    (numpy / zarr I/O, no GPU calls) while the GPU uploads (copy stream), gathers, predicts and scatters chunk i, and
    the result of chunk i-1 comes back through a pinned buffer (asynchronous D2H) before it is handed to the caller.
    """
    f16 = np.dtype(out_dtype) == np.float16
    flow = _SurveyChunks("predict_survey", reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings,
                         start_ping, labels_available, f16, stats, predict_fn, share_patches=shard == "patch")
    n_range, note = flow.n_range, flow.note
    if shard not in ("chunk", "patch"):
        raise ValueError(f"predict_survey: shard must be 'chunk' or 'patch', got {shard!r}")
    share_patches = shard == "patch"
    rank, world = parallel.rank_world()
    multi = world > 1
    if ordered_to_rank0 and share_patches:
        raise ValueError("predict_survey: ordered_to_rank0 belongs to shard='chunk' (with shard='patch' every rank already "
                         "yields every chunk)")
    ordered = multi and not share_patches and bool(ordered_to_rank0)
    if multi and not share_patches:
        flow.own(rank, world)
    sender = ordered and rank != 0
    hand = _OrderedHandoff(rank, world, flow.all_chunks, n_range, np.dtype(out_dtype)) if ordered else None
    if not flow.chunks:
        return
    flow.check_model()
    tick = time.perf_counter
    out_t = torch.float16 if f16 else torch.float32

    def result_ring():                   # flat: every chunk's [2, range, e - s] view of it is contiguous
        return {"pinned": [torch.empty(2 * n_range * flow.widest, dtype=out_t).pin_memory() for _ in range(2)]}

    with flow.feed(("predict", f16), extra=result_ring) as feed:
        pinned = feed.bufs["pinned"]
        events = [torch.cuda.Event() for _ in range(2)]

        def take(s, e, ring):            # the chunk whose D2H copy went into pinned[ring]
            t0 = tick()
            events[ring].synchronize()
            note("wait_gpu_s", t0)
            t0 = tick()
            res = pinned[ring][:2 * n_range * (e - s)].view(2, n_range, e - s).numpy().copy()
            note("copy_out_s", t0)
            return s, e, res

        def _loop():
            pending = None                      # (s, e, ring) of the chunk whose D2H copy is in flight
            for i, s, e, out in flow.predicted(feed):
                if sender:                            # ordered hand-off: the chunk goes to rank 0, nothing comes back here
                    hand.send(out)
                    note("enqueue_s", feed.t_taken)
                    continue
                pinned[i & 1][:out.numel()].view(out.shape).copy_(out, non_blocking=True)
                events[i & 1].record()
                note("enqueue_s", feed.t_taken)
                if pending is not None:
                    yield take(*pending)
                pending = (s, e, i & 1)
            if sender:
                hand.flush()
            else:
                yield take(*pending)

        if ordered and rank == 0:
            yield from hand.merge(_loop())
        else:
            yield from _loop()


# ---- echo integration by predicted class: the reduction of the prediction flows (csrc/integrate.hip) ---------------------
INTEGRATION_CLASSES = ("sandeel", "other", "all")
INTEGRATE_MAX_FREQS = hip.DEFINES["CRIMAC_INTEGRATE_MAX_FREQS"]      # frequencies of one crimac_integrate_freqs launch


class IntegrationSpec:
    """What to integrate and on which grid.  ``ping_bin`` / ``range_bin``: the cell size in pings / range rows (cell
    (pb, rb) = global pings [pb * ping_bin, (pb + 1) * ping_bin) x rows [rb * range_bin, (rb + 1) * range_bin), the last
    bin of either axis may be partial).  ``frequency``: the frequency whose linear sv is summed, a value of
    ``segpipe.frequencies``; None takes 38 (kHz, the memm readers and the yaml) or, failing that, 38000 (Hz, the zarr
    readers).  ``mode`` "threshold": a pixel belongs to class k when its stored probability >= ``thresholds[k]``
    (sandeel, other; it may belong to both); "probability": its sv counts with weight = the stored probability.
    ``thresholds`` must be > 0 in both modes.  ``bind(frequencies)`` returns the spec with ``channel`` looked up.

    **Several frequencies** (``crimac_integrate_freqs``).  ``frequency`` as a tuple or list of distinct values, at most
    ``INTEGRATE_MAX_FREQS``: all of them are integrated in ONE pass over the predictions, and every result has a leading
    frequency axis in the order given (``sv_sum`` / ``pixels`` ``[F, 3, n_pb, n_rb]``, ``"frequencies"``), also for a
    sequence of one.  ``bind`` looks up ``channels``; ``n_freqs`` is their number.  A scalar ``frequency`` is the form
    above: ``channels == (channel,)``, ``n_freqs == 1``, no frequency axis.

    **Seabed** (``crimac_integrate_layers``).  ``seabed_offset`` = an integer k (it may be negative): ping p has the row
    limit ``L[p] = clamp(seabed[p] + k, 0, n_range)`` and rows ``r >= L[p]`` count in NO plane, neither sums nor pixels;
    k < 0 is the usual backstep above the detected bottom, k = ``+SEABED_PAD`` the row rule of the memm scatter.  None
    (default): no limit, the bottom echo counts in the ``all`` plane.  ``reference`` "surface" (default): the cells above,
    each ping's rows cut at its limit.  ``reference`` "seabed" (needs ``seabed_offset`` and ``layers``, a positive
    integer): the range axis of the result is ``layers`` bottom layers -- layer l of ping p covers rows
    ``[L[p] - (l + 1) * range_bin, L[p] - l * range_bin)`` clipped to ``[0, n_range)``.  Layer rows are counted FROM THE
    LIMIT, not from the surface: layer 0 touches it, a layer follows the relief inside a ping bin, and rows above the
    top layer belong to no layer and are dropped.

    **EDSU** (``crimac_integrate_edges``).  ``ping_edges`` (with ``ping_bin`` None): the ping axis of the cells as an edge
    table instead of a width -- cell pb covers global pings ``[ping_edges[pb], ping_edges[pb + 1])``, as many ping bins as
    the table has intervals, whatever the survey's length.  A 1-D integer array, non-negative and non-decreasing (a
    zero-width cell is legal and stays 0; pings before the first or from the last edge on count nowhere), or a callable
    ``source -> array`` asked for every reader / echogram that is integrated (``resolve``): a memm survey has one ping
    axis per echogram.  ``ping_bin_edges`` builds the table from a log-distance or time vector.  Range bins, seabed limit
    and layers are as above."""
    MODES = ("threshold", "probability")
    REFERENCES = ("surface", "seabed")

    def __new__(cls, *args, **kwargs):
        # ``ping_edges=`` is the keyword of the EDSU form, a subclass with that one parameter more: the parameter list of
        # this ``__init__`` stays the uniform grid's, which callers and tests introspect
        return object.__new__(EdsuIntegrationSpec if cls is IntegrationSpec and "ping_edges" in kwargs else cls)

    def __init__(self, ping_bin, range_bin, frequency=None, thresholds=(0.5, 0.5), mode="threshold", channel=None,
                 seabed_offset=None, reference="surface", layers=None):
        self._setup(ping_bin, range_bin, frequency, thresholds, mode, channel, seabed_offset, reference, layers, None)

    def _setup(self, ping_bin, range_bin, frequency, thresholds, mode, channel, seabed_offset, reference, layers, ping_edges):
        def integer(v):
            return not isinstance(v, bool) and isinstance(v, (int, np.integer))
        if ping_edges is not None:
            if ping_bin is not None:
                raise ValueError(f"IntegrationSpec: ping_bin={ping_bin!r} and ping_edges: the ping axis is one or the other "
                                 "(ping_bin=None with an edge table)")
            if not callable(ping_edges):
                ping_edges = self._checked_edges(ping_edges)
        for name, v in (("ping_bin", ping_bin), ("range_bin", range_bin))[ping_edges is not None:]:
            if not integer(v) or v < 1:
                raise ValueError(f"IntegrationSpec: {name}={v!r} must be a positive integer")
        if seabed_offset is not None and not (integer(seabed_offset) and abs(int(seabed_offset)) < 2 ** 30):
            raise ValueError(f"IntegrationSpec: seabed_offset={seabed_offset!r} must be None or an integer (rows; negative: "
                             "above the seabed line)")
        if reference not in self.REFERENCES:
            raise ValueError(f"IntegrationSpec: reference={reference!r}: 'surface' or 'seabed'")
        if reference == "seabed":
            if seabed_offset is None:
                raise ValueError("IntegrationSpec: reference='seabed' needs seabed_offset (an integer; 0: layers end at the "
                                 "seabed line)")
            if not integer(layers) or layers < 1 or int(layers) * int(range_bin) >= 2 ** 31:
                raise ValueError(f"IntegrationSpec: reference='seabed' needs layers, a positive integer (layers * range_bin "
                                 f"below 2^31); got layers={layers!r}")
        elif layers is not None:
            raise ValueError(f"IntegrationSpec: layers={layers!r} belongs to reference='seabed' (the surface grid has "
                             "ceil(n_range / range_bin) range bins)")
        if mode not in self.MODES:
            raise ValueError(f"IntegrationSpec: mode={mode!r}: 'threshold' or 'probability'")
        try:
            thresholds = tuple(float(t) for t in thresholds)
        except TypeError:
            raise ValueError(f"IntegrationSpec: thresholds={thresholds!r}: two numbers (sandeel, other)") from None
        if len(thresholds) != 2 or not all(0.0 < t < float("inf") for t in thresholds):
            raise ValueError(f"IntegrationSpec: thresholds={thresholds!r}: two finite numbers > 0 (pixels the scatter left "
                             "at 0 belong to no class)")
        if isinstance(frequency, (tuple, list)):
            frequency = tuple(frequency)
            if not frequency:
                raise ValueError("IntegrationSpec: frequency is an empty sequence: name at least one frequency")
            if len({float(f) for f in frequency}) != len(frequency):
                raise ValueError(f"IntegrationSpec: frequency={list(frequency)} names a frequency twice")
            if len(frequency) > INTEGRATE_MAX_FREQS:
                raise ValueError(f"IntegrationSpec: {len(frequency)} frequencies, one pass takes {INTEGRATE_MAX_FREQS} at most")
            if channel is not None:
                channel = tuple(int(c) for c in channel)
                if len(channel) != len(frequency):
                    raise ValueError(f"IntegrationSpec: channel={channel} for {len(frequency)} frequencies")
        self.ping_bin, self.range_bin, self.frequency = None if ping_bin is None else int(ping_bin), int(range_bin), frequency
        self.ping_edges, self._edges_dev = ping_edges, {}
        self.thresholds, self.mode, self.channel = thresholds, mode, channel
        self.seabed_offset = None if seabed_offset is None else int(seabed_offset)
        self.reference, self.layers = reference, None if layers is None else int(layers)

    @staticmethod
    def _checked_edges(edges):
        """``edges`` as the contiguous int64 table of the kernel; ValueError unless it is a 1-D integer array of at least
        two edges, non-negative, non-decreasing, no cell wider than 2^31 - 1 pings."""
        e = np.asarray(edges)
        if e.ndim != 1 or e.size < 2 or e.dtype.kind not in "iu":
            raise ValueError(f"IntegrationSpec: ping_edges is a 1-D integer array of at least two edges (or a callable "
                             f"source -> array), got {e.dtype} {e.shape}")
        if e.dtype.kind == "u" and e.size and int(e.max()) >= 2 ** 63:
            raise ValueError("IntegrationSpec: ping_edges beyond 2^63 - 1")
        e = np.array(e, dtype=np.int64)                      # (a copy: it is frozen below)
        if e[0] < 0 or np.any(e[1:] < e[:-1]) or np.any(e[1:] - e[:-1] >= 2 ** 31):
            raise ValueError("IntegrationSpec: ping_edges must be non-negative and non-decreasing, no cell wider than "
                             "2^31 - 1 pings")
        e.setflags(write=False)
        return e

    def _with(self, channel, frequency, ping_edges):
        return IntegrationSpec(self.ping_bin, self.range_bin, frequency, self.thresholds, self.mode, channel,
                               seabed_offset=self.seabed_offset, reference=self.reference, layers=self.layers,
                               **({} if ping_edges is None else {"ping_edges": ping_edges}))

    def resolve(self, source):
        """The spec with ``ping_edges`` as a table: a callable is asked for ``source`` (the reader or echogram that is
        integrated) and its answer checked; a spec with a table, or with ``ping_bin``, is returned as it is."""
        if not callable(self.ping_edges):
            return self
        return self._with(self.channel, self.frequency, self._checked_edges(self.ping_edges(source)))

    def edges_on(self, dev):
        """The device copy of the edge table on ``dev``, uploaded at the first call (``new_integration`` makes it, before
        the feed starts) and kept with the spec: never per launch."""
        if self.ping_edges is None or callable(self.ping_edges):
            raise ValueError("IntegrationSpec: no edge table (ping_edges is None, or a callable that resolve(source) has "
                             "not been asked yet)")
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._edges_dev:
            self._edges_dev[dev] = torch.from_numpy(self.ping_edges.copy()).to(dev)
        return self._edges_dev[dev]

    def touched(self, start_ping, end_ping):
        """How many ping bins global pings [start_ping, end_ping) touch, as the library counts them for the scratch: with
        a table the first cell that ends after ``start_ping`` to the last that begins before ``end_ping``."""
        if self.ping_edges is None:
            return (end_ping - 1) // self.ping_bin - start_ping // self.ping_bin + 1
        e = self.ping_edges
        pb0 = max(int(np.searchsorted(e, start_ping, "right")) - 1, 0)
        pb1 = min(int(np.searchsorted(e, end_ping, "left")) - 1, len(e) - 2)
        return max(pb1 - pb0 + 1, 0)

    @property
    def multi(self):
        """Whether ``frequency`` is a sequence: results carry a leading frequency axis (``crimac_integrate_freqs``)."""
        return isinstance(self.frequency, tuple)

    @property
    def channels(self):
        """The data planes that are integrated, in the order of ``frequency``: ``(channel,)`` for the scalar form; None for
        a sequence that ``bind`` has not looked up yet."""
        return self.channel if self.multi else (self.channel,)

    @property
    def n_freqs(self):
        return len(self.frequency) if self.multi else 1

    @property
    def seabed_aware(self):
        """Whether the spec needs the seabed line (``crimac_integrate_layers``) or not (``crimac_integrate_classes``)."""
        return self.seabed_offset is not None

    def bind(self, frequencies):
        """The spec with ``channel`` = the index of its frequency in ``frequencies`` (a sequence: the tuple of indices, in
        the order given); ValueError if one is not there."""
        freqs = [float(f) for f in frequencies]
        if self.multi:
            for f in self.frequency:
                if float(f) not in freqs:
                    raise ValueError(f"IntegrationSpec: frequency {f} is not among the model's frequencies {list(frequencies)}")
            return self._with(tuple(freqs.index(float(f)) for f in self.frequency), self.frequency, self.ping_edges)
        wanted = (38, 38000) if self.frequency is None else (self.frequency,)
        for f in wanted:
            if float(f) in freqs:
                return self._with(freqs.index(float(f)), f, self.ping_edges)
        raise ValueError(f"IntegrationSpec: frequency {' / '.join(str(f) for f in wanted)} is not among the model's "
                         f"frequencies {list(frequencies)}")

    def bins(self, n_pings, n_range):
        """(ping bins, range bins) that cover global pings [0, n_pings) and rows [0, n_range); with the seabed reference
        (ping bins, ``layers``).  With ``ping_edges`` the ping bins are the table's, whatever ``n_pings``."""
        if callable(self.ping_edges):
            raise ValueError("IntegrationSpec: ping_edges is a callable: resolve(source) it first")
        n_pb = len(self.ping_edges) - 1 if self.ping_edges is not None else -(-int(n_pings) // self.ping_bin)
        return n_pb, self.layers if self.reference == "seabed" else -(-int(n_range) // self.range_bin)


class EdsuIntegrationSpec(IntegrationSpec):
    """What ``IntegrationSpec(None, range_bin, ..., ping_edges=...)`` constructs: the spec whose ping axis is an edge
    table (or a callable that gives one per source).  Everything else is ``IntegrationSpec``'s."""

    def __init__(self, ping_bin, range_bin, frequency=None, thresholds=(0.5, 0.5), mode="threshold", channel=None,
                 seabed_offset=None, reference="surface", layers=None, ping_edges=None):
        self._setup(ping_bin, range_bin, frequency, thresholds, mode, channel, seabed_offset, reference, layers, ping_edges)


def new_integration(dev, spec, n_pings, n_range):
    """Zeroed accumulators of ``ChunkPredictor.integrate`` on ``dev``: (acc float64, cnt int64), both [3, n_pb, n_rb]
    ([F, 3, n_pb, n_rb] for a spec with a sequence of F frequencies).
    A spec with an edge table: its device copy goes up here (``IntegrationSpec.edges_on``), once per survey."""
    shape = ((spec.n_freqs,) if spec.multi else ()) + (3, *spec.bins(n_pings, n_range))
    if spec.ping_edges is not None:
        spec.edges_on(dev)
    return torch.zeros(shape, dtype=torch.float64, device=dev), torch.zeros(shape, dtype=torch.int64, device=dev)


def integration_scratch(engine, cells, n_freqs=1):
    """The scratch of an integrate launch of ``cells`` = (ping bins it touches) x (range bins or layers), from the
    engine's buffer cache: (cells + INTEGRATE_SPLIT_WGS) slots always suffice, ``n_freqs`` times that for a launch over
    several frequencies."""
    return engine._buf("integrate.scratch", (n_freqs * (cells + hip.INTEGRATE_SPLIT_WGS) * hip.INTEGRATE_SLOT_BYTES // 8,),
                       torch.float64)


def launch_integration(spec, pred, pred_f16, n_range, n_pings, sv, data_pings, sv_ping_off, ping_origin, n_pb_total, acc,
                       cnt, scratch, seabed=None, edges=None, plane_stride=None, n_planes=None):
    """One integrate launch by a bound ``spec``: ``crimac_integrate_classes``, or -- a seabed-aware spec --
    ``crimac_integrate_layers`` with ``seabed`` = (pointer to an int32 line, index of pred's column 0 in it, its length).
    ``pred`` / ``sv`` / ``acc`` / ``cnt``: device pointers (``hip.ptr``); ``scratch``: a float64 tensor.
    A spec with an edge table runs ``crimac_integrate_edges`` (with or without ``seabed``); ``edges``: the device pointer
    of a copy of ``spec.ping_edges`` the caller has uploaded with other tables (default: ``spec.edges_on`` the current
    device); ``n_pb_total`` must be the table's intervals.
    A spec with a sequence of frequencies runs ``crimac_integrate_freqs`` whatever its grid: ``sv`` is then PLANE 0 of the
    source, ``plane_stride`` the elements between its ``n_planes`` planes, and ``acc`` / ``cnt`` are ``[F, 3, ...]``."""
    mode = IntegrationSpec.MODES.index(spec.mode)
    if spec.multi and (plane_stride is None or n_planes is None):
        raise ValueError("launch_integration: a spec with several frequencies needs plane_stride and n_planes (sv: plane 0)")
    table = spec.ping_edges
    if table is not None:
        if callable(table):
            raise ValueError("launch_integration: ping_edges is a callable: IntegrationSpec.resolve(source) it first")
        if n_pb_total != len(table) - 1:
            raise ValueError(f"launch_integration: n_pb_total={n_pb_total} for an edge table of {len(table) - 1} cells")
        if edges is None:
            edges = ptr(spec.edges_on(torch.device("cuda", torch.cuda.current_device())))
    if spec.multi and spec.channels is None:
        raise ValueError("launch_integration: bind the spec to the model's frequencies first (IntegrationSpec.bind)")
    # the argument groups of the four entry points, each built once
    head = (pred, 1 if pred_f16 else 0, n_range, n_pings, sv)
    rule = (data_pings, sv_ping_off, spec.thresholds[0], spec.thresholds[1], mode)
    grid = (spec.range_bin, ping_origin, n_pb_total)
    edge_pair = (None, None) if table is None else (edges, ctypes.c_void_p(table.ctypes.data))
    sb = (*(seabed if spec.seabed_aware else (None, 0, 0)), spec.seabed_offset or 0,
          IntegrationSpec.REFERENCES.index(spec.reference), spec.layers or 0)
    tail = (acc, cnt, ptr(scratch), scratch.numel() * 8)
    if spec.multi:
        channels = (ctypes.c_int * spec.n_freqs)(*spec.channels)      # a host array: it lives until the call returns
        call("crimac_integrate_freqs", *head, plane_stride, n_planes, channels, spec.n_freqs, *rule, spec.ping_bin or 0,
             *edge_pair, *grid, *sb, *tail)
    elif table is not None:
        call("crimac_integrate_edges", *head, *rule, *edge_pair, *grid, *sb, *tail)
    elif spec.seabed_aware:
        call("crimac_integrate_layers", *head, *rule, spec.ping_bin, *grid, *sb, *tail)
    else:
        call("crimac_integrate_classes", *head, *rule, spec.ping_bin, *grid, *tail)


def finish_integration(acc, cnt, spec, n_pings, n_range, all_reduce=True):
    """The accumulators -> the result of the integration flows (numpy, ONE download): ``sv_sum`` float64 and ``pixels``
    int64 ``[3, n_pb, n_rb]`` (planes ``classes`` = sandeel, other, all counted pixels), ``ping_edges`` int64 [n_pb + 1]
    and ``range_edges`` int64 [n_rb + 1] (the last edge is the survey's end, so a partial last bin shows).  With several
    ranks the accumulators are all-reduced first (sum), the one collective of the flow.  A seabed-aware spec
    (``seabed_offset`` given) adds ``"reference"`` and ``"seabed_offset"``; with the seabed reference the range axis holds
    the layers and ``range_edges`` their heights ABOVE THE LIMIT, ``arange(layers + 1) * range_bin`` (layer l: rows
    ``[L - range_edges[l + 1], L - range_edges[l])`` of each ping, counted from its limit L, not from the surface)."""
    if all_reduce and parallel.rank_world()[1] > 1:
        torch.distributed.all_reduce(acc)
        torch.distributed.all_reduce(cnt)
    return integration_result(acc.cpu().numpy(), cnt.cpu().numpy(), spec, n_pings, n_range)


def integration_result(sv_sum, pixels, spec, n_pings, n_range):
    """The result dict of ``finish_integration`` around downloaded accumulators (numpy ``[3, n_pb, n_rb]``; a spec with a
    sequence of frequencies: ``[F, 3, n_pb, n_rb]``, and the result names them as ``"frequencies"``).  With
    ``spec.ping_edges`` the result's ``ping_edges`` are the table clipped to ``n_pings``."""
    n_pb, n_rb = spec.bins(n_pings, n_range)
    edges = np.arange(n_rb + 1, dtype=np.int64) * spec.range_bin
    ping_edges = np.arange(n_pb + 1, dtype=np.int64) * spec.ping_bin if spec.ping_edges is None else spec.ping_edges
    res = {"sv_sum": sv_sum, "pixels": pixels, "ping_edges": np.minimum(ping_edges, int(n_pings)),
           "range_edges": edges if spec.reference == "seabed" else np.minimum(edges, int(n_range)),
           "classes": INTEGRATION_CLASSES}
    if spec.seabed_aware:
        res.update(reference=spec.reference, seabed_offset=spec.seabed_offset)
    if spec.multi:                                           # (sv_sum / pixels [F, 3, n_pb, n_rb], in this order)
        res["frequencies"] = spec.frequency
    return res


def group_shares(group, spec, planes):
    """The layout of a packed group's flat accumulators by a bound ``spec``: ``([(first word, (n_pb, range bins or
    layers))] per record, words)`` -- the echograms' blocks of ``planes`` cells each (3: ``[3, n_pb, n_rb]``, 9: the scored
    ``[3, 3, n_pb, n_rb]``, 3 F with a spec of F frequencies: ``[F, 3, n_pb, n_rb]``) one after the other.  A record that carries its own spec (``_MemmEdgeRecord``: the spec with
    the echogram's edge table) goes by that one."""
    shares, total = [], 0
    for r in group:
        shape = getattr(r, "spec", spec).bins(r.n_pings, r.n_range)
        shares.append((total, shape))
        total += planes * shape[0] * shape[1]
    return shares, total


def group_results(group, shares, sums, counts, spec, planes):
    """The inverse of ``group_shares``: ``(echogram, integration_result)`` per record from a group's downloaded flat
    accumulators (numpy; copied, the pinned buffer is used again); 9 planes: with the ``"annotated"`` classes."""
    lead = (planes // 3, 3) if spec.multi else (3,) if planes == 3 else (3, 3)       # (scored holders take no multi spec)
    for r, (at, shape) in zip(group, shares):
        n = planes * shape[0] * shape[1]
        res = integration_result(sums[at:at + n].reshape(*lead, *shape).copy(), counts[at:at + n].reshape(*lead, *shape).copy(),
                                 getattr(r, "spec", spec), r.n_pings, r.n_range)
        if planes == 9 and not spec.multi:
            res["annotated"] = ANNOTATED_CLASSES
        yield r.echogram, res


def integrate_survey(reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings, spec, start_ping=0,
                     labels_available=True, predict_fn=None, stats=None):
    """Echo integration by predicted class over one zarr survey: ``predict_survey``'s chunk feed, staging and upload
    overlap, but each chunk's float16 predictions -- the values the reference would save -- are reduced on the GPU
    (``ChunkPredictor.integrate``) against the sv plane that is resident anyway, instead of being downloaded: no result
    ring, no per-chunk copy, one download of a few kilobytes at the end.

    Pixel rule: a pixel is counted when its sv (of ``spec.frequency``) is finite and > 0; it belongs to a class by
    ``spec.mode``; pixels without a prediction (overlap border, below the seabed) belong to none but count in the ``all``
    plane; pings before ``start_ping`` are not visited and count nowhere.  Returns ``{"sv_sum": float64 [3, n_pb, n_rb] (sum of linear sv: sandeel, other, all
    counted pixels), "pixels": int64 [3, n_pb, n_rb], "ping_edges", "range_edges", "classes"}`` (``finish_integration``);
    ``nasc`` turns ``sv_sum`` into area backscattering.  Bins count global pings from 0 whatever ``start_ping``.
    A spec with ``ping_edges`` (EDSU cells; a callable is asked for ``reader``) integrates on the table's cells: its device
    copy is uploaded once, before the feed starts, and ``"ping_edges"`` of the result is the table clipped to the survey.
    With torch.distributed initialised the chunks are dealt to the ranks as in ``predict_survey(shard="chunk")`` and the
    accumulators all-reduced once at the end: every rank must call it and every rank returns the survey's result.  Sums
    are fp64 in a fixed order: bit-reproducible for a given chunking and rank count, whatever ``batch_size``."""
    flow = _SurveyChunks("integrate_survey", reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings,
                         start_ping, labels_available, True, stats, predict_fn, share_patches=False)
    spec = spec.bind(segpipe.frequencies).resolve(reader)
    acc, cnt = new_integration(flow.dev, spec, flow.n_pings, flow.n_range)
    rank, world = parallel.rank_world()
    if world > 1:
        flow.own(rank, world)
    if flow.chunks:
        flow.check_model()
        with flow.feed(("integrate",)) as feed:
            for _ in flow.predicted(feed, then=lambda cp: cp.integrate(acc, cnt, spec)):
                flow.note("enqueue_s", feed.t_taken)
    return finish_integration(acc, cnt, spec, flow.n_pings, flow.n_range)


def nasc(result, range_step_m):
    """Nautical area scattering coefficient per cell and class from an integration result: ``4 pi 1852^2 * range_step_m *
    sv_sum`` (m^2 nmi^-2 summed over the cell's pings; divide by the pings of a cell, ``np.diff(result["ping_edges"])``,
    for the cell's mean NASC: ``mean_nasc``).  Assumes a UNIFORM range grid: every sample is ``range_step_m`` metres thick."""
    return 4.0 * np.pi * 1852.0 ** 2 * float(range_step_m) * np.asarray(result["sv_sum"], dtype=np.float64)


def mean_nasc(result, range_step_m):
    """The cell's MEAN NASC, what a survey reports per EDSU: ``nasc`` divided by the pings of the cell,
    ``np.diff(result["ping_edges"])``; NaN for a cell without pings (a zero-width cell of an edge table)."""
    pings = np.diff(np.asarray(result["ping_edges"])).astype(np.float64)[:, None]
    total = nasc(result, range_step_m)
    return np.divide(total, pings, out=np.full(total.shape, np.nan), where=pings > 0)


def frequency_response(result, reference=None):
    """The frequency response r(f) = s_A(f) / s_A(reference) per class and cell of a result with a frequency axis (a spec
    with a sequence of frequencies): ``sv_sum[f] / sv_sum[reference]``, float64 of ``sv_sum``'s shape ``[F, 3, n_pb, n_rb]``,
    NaN where the reference sum is 0.  ``reference``: one of ``result["frequencies"]``; None takes 38 or, failing that,
    38000 (as ``IntegrationSpec.bind``).  ValueError: a result without a frequency axis, a reference that is not there."""
    if "frequencies" not in result:
        raise ValueError("frequency_response: the result has no frequency axis (integrate with IntegrationSpec(frequency="
                         "(f1, f2, ...)))")
    freqs = [float(f) for f in result["frequencies"]]
    wanted = (38, 38000) if reference is None else (reference,)
    at = next((freqs.index(float(f)) for f in wanted if float(f) in freqs), None)
    if at is None:
        raise ValueError(f"frequency_response: reference {' / '.join(str(f) for f in wanted)} is not among the result's "
                         f"frequencies {list(result['frequencies'])}")
    sums = np.asarray(result["sv_sum"], dtype=np.float64)
    ref = np.broadcast_to(sums[at], sums.shape)
    return np.divide(sums, ref, out=np.full(sums.shape, np.nan), where=ref > 0)


def ping_bin_edges(track, step, origin=None):
    """The edge table of EDSU cells (``IntegrationSpec(ping_edges=...)``) from a per-ping ``track`` -- the log distance in
    nmi, the reader's ``time_vector``, anything finite and non-decreasing: cell k holds the pings whose track value lies
    in ``[origin + k * step, origin + (k + 1) * step)``, ``origin`` defaulting to ``track[0]``.  ``edges[k] =
    searchsorted(track, origin + k * step, 'left')`` for k = 0 .. K with K = floor((track[-1] - origin) / step) + 1; the
    last edge is ``len(track)``.  A gap in the track gives zero-width cells, repeated values stay in one cell, pings
    before a later ``origin`` lie before the first edge and count nowhere.  ValueError: an empty, non-finite or
    decreasing track, ``step`` not > 0, an ``origin`` that is not finite or lies beyond the track's end."""
    t = np.asarray(track, dtype=np.float64)
    if t.ndim != 1 or t.size == 0 or not np.all(np.isfinite(t)) or np.any(t[1:] < t[:-1]):
        raise ValueError(f"ping_bin_edges: track is a finite, non-decreasing vector with at least one ping, got shape {t.shape}"
                         + ("" if t.ndim != 1 or t.size == 0 else " with non-finite or decreasing values"))
    step = float(step)
    if not (step > 0.0 and np.isfinite(step)):
        raise ValueError(f"ping_bin_edges: step={step!r} must be a finite number > 0")
    origin = float(t[0] if origin is None else origin)
    if not np.isfinite(origin) or origin > t[-1]:
        raise ValueError(f"ping_bin_edges: origin={origin!r} must be finite and not beyond the track's end {t[-1]!r}")
    K = int(np.floor((t[-1] - origin) / step)) + 1
    edges = np.searchsorted(t, origin + np.arange(K + 1, dtype=np.float64) * step, "left").astype(np.int64)
    edges[-1] = len(t)                                   # (whatever the rounding of origin + K * step)
    return edges


# ---- echo integration scored against the annotations (the evaluation flows) --------------------------------------------
ANNOTATED_CLASSES = ("background", "sandeel", "other")
CONFUSION_SLOT_BYTES, CONFUSION_MAX_PATCHES = hip.DEFINES["CRIMAC_CONFUSION_SLOT_BYTES"], hip.DEFINES["CRIMAC_CONFUSION_MAX_PATCHES"]


def confusion_scratch_bytes(P, ph, pw, ping_bin, range_bin):
    """The scratch of one ``crimac_integrate_confusion`` launch, as the header states it: one slot per patch and cell of
    the window of cells a patch can overlap."""
    return P * (-(-pw // ping_bin) + 1) * (-(-ph // range_bin) + 1) * CONFUSION_SLOT_BYTES


class _ScoredHolder:
    """What ``ScoredIntegration`` and ``ScoredIntegrationSet`` share: the checks of the spec and of the model, the class
    names and the NaN-safe ratio of their recall / precision."""

    @classmethod
    def _checked(cls, spec):
        """``spec`` if a scored holder takes it (``ScoredIntegrationSet`` makes the same checks)."""
        if not isinstance(spec, IntegrationSpec):
            raise TypeError(f"{cls.__name__}: spec is an IntegrationSpec, got {type(spec).__name__}")
        if spec.multi:
            raise NotImplementedError(f"{cls.__name__}: a spec with several frequencies is not scored: the confusion kernels "
                                      "sum one sv plane (score one frequency per holder)")
        if spec.ping_edges is not None:
            raise NotImplementedError(f"{cls.__name__}: a spec with ping_edges (EDSU cells) is not scored: the confusion "
                                      "kernels size a patch's window of cells from a uniform ping_bin")
        if spec.seabed_aware or spec.reference != "surface":
            raise NotImplementedError(f"{cls.__name__}: a seabed-aware spec (seabed_offset / reference='seabed') is not "
                                      "scored: the transformed labels already exclude the pixels below the seabed")
        return spec

    @classmethod
    def _bound(cls, spec, frequencies, n_classes):
        """``spec`` bound to the model's ``frequencies``, after the check that the model has 3 classes."""
        if int(n_classes) != 3:
            raise ValueError(f"{cls.__name__}: the model has n_classes={n_classes}; the planes (sandeel, other, all) and "
                             "the annotated classes (background, sandeel, other) are those of a 3-class model")
        return spec.bind(frequencies)

    def _confusion_batches(self, engine, logits, raw, labels_t, hint=""):
        """The operands of an ``add_batch`` checked at the call, then lazily ``(first patch, patches, origins int32 [n][2],
        scratch)`` of every sub-batch of at most ``CONFUSION_MAX_PATCHES``: the holder launches its two kernels on each."""
        name = type(self).__name__
        P, _, ph, pw = logits.shape
        C = raw.shape[1]
        if logits.dtype != torch.float32 or not logits.is_contiguous() or tuple(raw.shape) != (P, C, ph, pw) \
                or tuple(labels_t.shape) != (P, ph, pw) or labels_t.dtype != torch.int16 or not labels_t.is_contiguous():
            raise ValueError(f"{name}: logits {logits.dtype} {tuple(logits.shape)}, raw {tuple(raw.shape)}, labels "
                             f"{labels_t.dtype} {tuple(labels_t.shape)}: contiguous fp32 [P, 3, H, W], fp32 [P, C, H, W], "
                             "int16 [P, H, W]")
        spec = self.spec
        if spec.channel is None or not 0 <= spec.channel < C:
            raise ValueError(f"{name}: channel {spec.channel} of {C} data planes{hint}")

        def batches():
            for b0 in range(0, P, CONFUSION_MAX_PATCHES):
                n = min(CONFUSION_MAX_PATCHES, P - b0)
                yield b0, n, engine._buf("confusion.origins", (n, 2), torch.int32), engine._buf(
                    "confusion.scratch", (confusion_scratch_bytes(n, ph, pw, spec.ping_bin, spec.range_bin) // 8,), torch.float64)
        return batches()

    @staticmethod
    def _class(k):
        k = {"sandeel": 1, "other": 2}.get(k, k)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k not in (1, 2):
            raise ValueError(f"scored integration: class {k!r}: 1 / 'sandeel' or 2 / 'other'")
        return int(k)

    @staticmethod
    def _ratio(num, den):
        num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
        return np.divide(num, den, out=np.full(num.shape, np.nan), where=den > 0)


class ScoredIntegration(_ScoredHolder):
    """Echo integration scored against the annotations: hand one to ``evaluate_survey`` / ``evaluate_echogram_memm`` /
    ``ChunkPredictor.evaluate`` as ``integration=`` and every evaluation batch is reduced on the GPU
    (``crimac_integrate_confusion``), while its raw crops, transformed labels and logits are resident, to the linear sv of
    ``spec.frequency`` per ANNOTATED class, predicted class and cell.  ``spec``: an ``IntegrationSpec`` (cells, frequency,
    ``mode``, ``thresholds``); the flow binds it to the model's frequencies (``begin``) and the holder owns the device
    accumulators.  A pixel counts when its transformed label is 0, 1 or 2 -- the pixels the PR histograms see, minus those
    below the seabed -- and its sv is finite and > 0; its class weights come from the float16 softmax probabilities the
    histograms bin, so a threshold read off the PR curve selects the same pixels here.

    A seabed-aware spec (``seabed_offset`` / ``reference="seabed"``) is refused: the labels already exclude the pixels
    below the seabed, and bottom layers are not scored."""

    def __init__(self, spec):
        self.spec = self._checked(spec)
        self.acc = self.cnt = None
        self.n_pings = self.n_range = None

    def begin(self, frequencies, n_classes, dev, n_pings, n_range):
        """What a flow does first: bind the spec to the model's ``frequencies``, check the model (3 classes) and allocate
        the zeroed accumulators, float64 / int64 ``[3, 3, n_pb, n_rb]`` on ``dev``, for a survey of ``n_pings`` x
        ``n_range``.  A holder that has begun keeps accumulating when the extent is the same one and raises otherwise."""
        spec = self._bound(self.spec, frequencies, n_classes)
        extent = (int(n_pings), int(n_range))
        if self.acc is not None:
            if (self.n_pings, self.n_range) != extent or spec.channel != self.spec.channel:
                raise ValueError(f"ScoredIntegration: begun for {self.n_pings} pings x {self.n_range} rows (channel "
                                 f"{self.spec.channel}), now asked for {extent[0]} x {extent[1]} (channel {spec.channel}): "
                                 "one holder per survey")
            return self
        self.spec = spec
        self.n_pings, self.n_range = extent
        shape = (3, 3, *spec.bins(*extent))
        self.acc = torch.zeros(shape, dtype=torch.float64, device=dev)
        self.cnt = torch.zeros(shape, dtype=torch.int64, device=dev)
        return self

    def add_batch(self, engine, logits, raw, labels_t, centres, n_range, memm):
        """One evaluation batch: ``logits`` fp32 [P, 3, ph, pw], ``raw`` fp32 [P, C, ph, pw] linear sv, ``labels_t`` int16
        [P, ph, pw] transformed labels, ``centres`` int32 [P, 2] GLOBAL centres, all on the GPU; ``n_range`` / ``memm``:
        the water column and the crop flavour of the gather that cut ``raw``, whose placement ``crimac_eval_crop_origins``
        restates.  Launches on the current stream; nothing comes back."""
        if self.acc is None:
            raise ValueError("ScoredIntegration: begin() first (the evaluation flows do)")
        batches = self._confusion_batches(engine, logits, raw, labels_t)
        (_, ncls, ph, pw), C, spec = logits.shape, raw.shape[1], self.spec
        centres = centres.contiguous()
        with torch.cuda.device(logits.device):
            for b0, n, origins, scratch in batches:
                call("crimac_eval_crop_origins", ptr(centres[b0:b0 + n]), n, ph, pw, n_range, 1 if memm else 0, ptr(origins))
                call("crimac_integrate_confusion", ptr(logits[b0:b0 + n]), ncls, ptr(raw[b0:b0 + n]), C, spec.channel,
                     ptr(labels_t[b0:b0 + n]), ptr(origins), n, ph, pw, self.n_range, spec.ping_bin, spec.range_bin,
                     int(self.acc.shape[2]), spec.thresholds[0], spec.thresholds[1], IntegrationSpec.MODES.index(spec.mode),
                     ptr(self.acc), ptr(self.cnt), ptr(scratch), scratch.numel() * 8)

    def all_reduce(self):
        """Sum the accumulators over the ranks (where ``evaluate_survey`` reduces its histograms)."""
        if self.acc is not None and parallel.rank_world()[1] > 1:
            torch.distributed.all_reduce(self.acc)
            torch.distributed.all_reduce(self.cnt)

    def result(self):
        """ONE download -> ``{"sv_sum": float64 [3, 3, n_pb, n_rb], "pixels": int64, same shape, "annotated":
        ("background", "sandeel", "other"), "classes": ("sandeel", "other", "all"), "ping_edges", "range_edges"}``:
        ``sv_sum[a, k]`` is the linear sv of the counted pixels annotated ``a`` that the model books in plane ``k`` (plane
        "all": every counted pixel annotated ``a``), ``pixels`` their numbers; edges as ``finish_integration`` builds them.
        ``nasc`` takes the result as it is."""
        if self.acc is None:
            raise ValueError("ScoredIntegration: nothing was evaluated into this holder yet")
        res = integration_result(self.acc.cpu().numpy(), self.cnt.cpu().numpy(), self.spec, self.n_pings, self.n_range)
        res["annotated"] = ANNOTATED_CLASSES
        return res

    def recall(self, k, result=None):
        """sv-weighted recall of class ``k`` (1 / "sandeel", 2 / "other"): of the backscatter ANNOTATED ``k``, the share
        the model books as ``k`` -- ``sv_sum[k, k - 1] / sv_sum[k, 2]``.  Returns ``(per cell float64 [n_pb, n_rb], over
        the survey float)``; NaN where nothing is annotated ``k``.  ``result``: a ``result()`` already downloaded."""
        k = self._class(k)
        sv = (self.result() if result is None else result)["sv_sum"]
        return self._ratio(sv[k, k - 1], sv[k, 2]), float(self._ratio(sv[k, k - 1].sum(), sv[k, 2].sum()))

    def precision(self, k, result=None):
        """sv-weighted precision of class ``k``: of the backscatter the model books as ``k``, the share that is annotated
        ``k`` -- ``sv_sum[k, k - 1] / sv_sum[:, k - 1].sum(0)``.  Returns as ``recall``; NaN where nothing is booked."""
        k = self._class(k)
        sv = (self.result() if result is None else result)["sv_sum"]
        booked = sv[:, k - 1].sum(axis=0)
        return self._ratio(sv[k, k - 1], booked), float(self._ratio(sv[k, k - 1].sum(), booked.sum()))


class ScoredIntegrationSet(_ScoredHolder):
    """``ScoredIntegration`` for a memm survey of many echograms, each with its own ping axis: hand one to
    ``evaluate_echograms_memm`` as ``integration=``.  Every packed evaluation batch is reduced on the GPU by
    ``crimac_integrate_confusion_multi`` into its echograms' shares of the group's accumulators; echograms that take the
    per-echogram path are scored by a ``ScoredIntegration`` of their own.  ``spec``: as ``ScoredIntegration`` takes it, the
    refusal of a seabed-aware spec included.  Afterwards ``results()`` has every echogram's result, ``totals()`` /
    ``recall`` / ``precision`` the survey's figures."""

    def __init__(self, spec):
        self.spec = self._checked(spec)
        self._results, self._reduced = [], None

    def begin(self, frequencies, n_classes):
        """What the flow does first: bind the spec to the model's ``frequencies`` and check the model (3 classes).  A set
        that has begun keeps collecting when the channel is the same one and raises otherwise."""
        spec = self._bound(self.spec, frequencies, n_classes)
        if self.spec.channel is not None and spec.channel != self.spec.channel:
            raise ValueError(f"ScoredIntegrationSet: begun for channel {self.spec.channel}, now asked for channel "
                             f"{spec.channel}: one set per model")
        self.spec = spec
        return self

    def shares(self, group):
        """``group_shares`` of a packed group's flat accumulators: the echograms' ``[3, 3, n_pb, n_rb]`` blocks."""
        return group_shares(group, self.spec, 9)

    def add_batch(self, engine, logits, raw, labels_t, cen, src, at, descs, n_desc, shares, acc, cnt):
        """One packed evaluation batch: ``logits`` fp32 [P, 3, ph, pw], ``raw`` fp32 [P, C, ph, pw], ``labels_t`` int16
        [P, ph, pw] as ``ScoredIntegration.add_batch`` takes them; ``cen`` / ``src``: the group's centres int32 [.][2] and
        src int32 [.] on the GPU, of which the batch is patches ``at`` ...; ``descs`` / ``shares`` / ``acc`` / ``cnt``: device
        pointers (``hip.ptr``) of the group's descriptor table, its share table int64 [n_desc][2] and its flat
        accumulators.  Launches on the current stream; nothing comes back."""
        batches = self._confusion_batches(engine, logits, raw, labels_t, hint=" (begin() binds it)")
        (_, ncls, ph, pw), C, spec = logits.shape, raw.shape[1], self.spec
        for b0, n, origins, scratch in batches:
            call("crimac_eval_crop_origins_multi", descs, n_desc, ptr(src, at + b0), ptr(cen, 2 * (at + b0)), n, ph, pw,
                 ptr(origins))
            call("crimac_integrate_confusion_multi", ptr(logits[b0:b0 + n]), ncls, ptr(raw[b0:b0 + n]), C, spec.channel,
                 ptr(labels_t[b0:b0 + n]), ptr(origins), descs, n_desc, ptr(src, at + b0), shares, n, ph, pw, spec.ping_bin,
                 spec.range_bin, spec.thresholds[0], spec.thresholds[1], IntegrationSpec.MODES.index(spec.mode), acc, cnt,
                 ptr(scratch), scratch.numel() * 8)

    def add(self, echogram, result):
        """``result`` (what ``ScoredIntegration.result()`` returns for ``echogram`` alone) as the next of the set."""
        self._results.append((echogram, result))
        self._reduced = None

    def add_group(self, group, shares, sums, counts):
        """The downloaded accumulators of a packed group (numpy, flat, laid out by ``shares``): one result per record."""
        for echogram, res in group_results(group, shares, sums, counts, self.spec, 9):
            self.add(echogram, res)

    def results(self):
        """``[(echogram, result)]`` in evaluation order (with several ranks: this rank's echograms); every ``result`` is
        what ``ScoredIntegration.result()`` returns for that echogram alone, its own ``ping_edges`` / ``range_edges``
        included.  ``nasc`` takes a result as it is."""
        return list(self._results)

    def _own_totals(self):
        sv, px = np.zeros((3, 3), dtype=np.float64), np.zeros((3, 3), dtype=np.int64)
        for _, res in self._results:
            sv += res["sv_sum"].sum(axis=(2, 3))
            px += res["pixels"].sum(axis=(2, 3))
        return sv, px

    def all_reduce(self, dev):
        """Sum the totals over the ranks (where ``evaluate_echograms_memm`` reduces its histograms); ``results()`` stay
        the rank's own."""
        if parallel.rank_world()[1] > 1:
            sv, px = (torch.from_numpy(a).to(dev) for a in self._own_totals())
            torch.distributed.all_reduce(sv)
            torch.distributed.all_reduce(px)
            self._reduced = (sv.cpu().numpy(), px.cpu().numpy())

    def totals(self):
        """``{"sv_sum": float64 [3, 3], "pixels": int64 [3, 3], "annotated", "classes"}``: ``results()`` summed over cells
        and echograms -- with several ranks over every rank's echograms, reduced once at the end of the flow."""
        sv, px = self._own_totals() if self._reduced is None else self._reduced
        return {"sv_sum": sv, "pixels": px, "annotated": ANNOTATED_CLASSES, "classes": INTEGRATION_CLASSES}

    def recall(self, k):
        """sv-weighted recall of class ``k`` (1 / "sandeel", 2 / "other") by ``ScoredIntegration.recall``'s formula:
        ``(per echogram float64 [n], over the survey float)``; NaN where nothing is annotated ``k``."""
        k = self._class(k)
        per = np.array([[res["sv_sum"][k, k - 1].sum(), res["sv_sum"][k, 2].sum()] for _, res in self._results]).reshape(-1, 2)
        sv = self.totals()["sv_sum"]
        return self._ratio(per[:, 0], per[:, 1]), float(self._ratio(sv[k, k - 1], sv[k, 2]))

    def precision(self, k):
        """sv-weighted precision of class ``k`` by ``ScoredIntegration.precision``'s formula; returns as ``recall``; NaN
        where nothing is booked as ``k``."""
        k = self._class(k)
        per = np.array([[res["sv_sum"][k, k - 1].sum(), res["sv_sum"][:, k - 1].sum()] for _, res in self._results]).reshape(-1, 2)
        sv = self.totals()["sv_sum"]
        return self._ratio(per[:, 0], per[:, 1]), float(self._ratio(sv[k, k - 1], sv[:, k - 1].sum()))


class _DownloadRing:
    """How the results of a packed group leave the GPU without blocking the feed: ONE flat buffer on the device for the
    group at work and two pinned buffers with an event each, group ``k`` in slot ``k & 1`` (``_ordered_groups`` awaits a
    download right after the next group is enqueued).  ``device`` / ``pinned`` given: the caller's buffers, large enough
    for every group (the float16 predictions, in the feed's staging cache); otherwise they grow on demand (the fp64
    accumulators [sums | counts] of the flows that reduce on the GPU, a few kilobytes)."""

    def __init__(self, dev, dtype, device=None, pinned=None):
        self.dev, self.dtype, self.device = dev, dtype, device
        self.pinned, self.events = pinned or [None, None], [torch.cuda.Event() for _ in range(2)]

    def zeroed(self, k, n):
        """The device buffer, its first ``n`` elements zeroed, for group ``k`` (all-zero bits: 0.0 and 0 alike)."""
        if self.device is None or n > self.device.numel():
            self.device = torch.empty(n, dtype=self.dtype, device=self.dev)
        if self.pinned[k & 1] is None or self.pinned[k & 1].numel() < n:
            self.pinned[k & 1] = torch.empty(self.device.numel(), dtype=self.dtype).pin_memory()
        self.device[:n].zero_()
        return self.device

    def download(self, k, n):
        """Enqueue the download of the first ``n`` elements for group ``k``; returns the ticket that ``wait`` takes."""
        host, event = self.pinned[k & 1][:n], self.events[k & 1]
        host.copy_(self.device[:n], non_blocking=True)
        event.record()
        return host, event

    @staticmethod
    def wait(ticket):
        """The downloaded elements of a ticket: a view of its pinned buffer, valid until the group after next."""
        host, event = ticket
        event.synchronize()
        return host

    @classmethod
    def wait_sums_counts(cls, ticket):
        """(sums float64 [total], counts int64 [total]) of downloaded accumulators: numpy views of the pinned buffer."""
        sums, counts = cls.wait(ticket).view(2, -1)
        return sums.numpy(), counts.view(torch.int64).numpy()


# ---- seabed line of a memmap echogram without a stored seabed.npy (Echogram.get_seabed, data_reader.py:433-507) ---------
SEABED_REPAIR_THRESHOLD = -8       # data_reader.py:471: standardised log column maximum below which a ping is a drop-out
SEABED_REPAIR_EDGE = 2             # data_reader.py:474 (i_edge)
SEABED_CHUNK_PINGS = 4096          # pings uploaded per launch by estimate_seabed (1000 rows x 4 frequencies: 66 MB)


def seabed_rows(n_range):
    """(n, a) of data_reader.py:461-463: the rows at the top that the argmax skips, and the upward shift of the line."""
    return 10 + int(0.05 * n_range), int(0.004 * n_range)


def seabed_columns(chunk, has_left, has_right, n, idx, colmax, ping0=0):
    """``crimac_seabed_columns`` on one chunk: ``chunk`` float32 [F, Pc, R] on the GPU (up to one halo ping on each side,
    flagged by ``has_left`` / ``has_right``); writes the owned pings' argmax rows (relative to row ``n``) and column
    maxima into ``idx`` int32 / ``colmax`` float32 [F, P] from ping ``ping0`` on."""
    F, Pc, R = (int(v) for v in chunk.shape)
    owned = Pc - int(bool(has_left)) - int(bool(has_right))
    if chunk.dtype != torch.float32 or not chunk.is_contiguous():
        raise ValueError("seabed_columns: the chunk is a contiguous float32 [F, pings, range] tensor")
    if idx.dtype != torch.int32 or colmax.dtype != torch.float32 or idx.shape != colmax.shape or idx.shape[0] != F \
            or not idx.is_contiguous() or not colmax.is_contiguous():
        raise ValueError("seabed_columns: idx int32 / colmax float32, both contiguous [F, P]")
    if ping0 < 0 or ping0 + owned > idx.shape[1]:
        raise ValueError(f"seabed_columns: pings [{ping0}, {ping0 + owned}) outside the result's {idx.shape[1]}")
    with torch.cuda.device(chunk.device):
        call("crimac_seabed_columns", ptr(chunk), F, Pc, R, int(bool(has_left)), int(bool(has_right)), int(n),
             ptr(idx, ping0), ptr(colmax, ping0), int(idx.shape[1]))


def finish_seabed(idx, colmax, n_range, runs=None):
    """The host end of ``Echogram.get_seabed`` (data_reader.py:466-504) from the per-column results: ``idx`` int [F, P]
    (argmax rows relative to row n), ``colmax`` float32 [F, P] -> the seabed vector int64 [P].  It needs every ping at
    once (the mean and the standard deviation run over the whole echogram) and works in the reference's dtypes, with the
    reference's own numpy calls on arrays of the reference's layout ([P, F], C order): float32 ``log(1e-10 + max)``
    standardised per frequency, float64 rows, ``np.rint(np.median(., axis=1))``.  Drop-out runs (standardised value
    < -8) are repaired per run as the reference's per-ping loop does (:481-502), quirks included: the scan starts at
    index 2 and ends before P - 2, so a run is not seen before index 2 (one that covers index 2 counts from there and takes
    the value BEHIND it), a run reaching P - 2 or further takes the value in front of it, every other run the mean of
    its two neighbours.  ``runs`` (a list): receives ``(frequency, idx_0, idx_1, case)`` of every repaired run, case
    'behind' / 'front' / 'mean'."""
    n, a = seabed_rows(n_range)
    idx = np.asarray(idx)
    seabed = np.ascontiguousarray((idx.astype(np.int64) + (n - a)).T).astype(np.float64)          # [P, F] (:466-468)
    sb_max = np.ascontiguousarray(np.asarray(colmax, dtype=np.float32).T)                          # [P, F] (:476)
    P = sb_max.shape[0]
    with np.errstate(all="ignore"):          # (a constant column: 0 * inf = nan, which is below no threshold)
        sb_max = np.log(1e-10 + sb_max)
        sb_max -= np.mean(sb_max, axis=0)
        sb_max *= 1 / np.std(sb_max, axis=0)
    e0 = SEABED_REPAIR_EDGE
    if P > 2 * e0:
        below = sb_max < SEABED_REPAIR_THRESHOLD
        for f in range(sb_max.shape[1]):
            d = np.diff(np.concatenate(([0], below[e0:, f].astype(np.int8), [0])))
            starts, ends = np.nonzero(d == 1)[0] + e0, np.nonzero(d == -1)[0] + e0 - 1     # [idx_0, idx_1] of every run
            for i0, i1 in zip(starts.tolist(), ends.tolist()):
                if i0 >= P - e0:
                    break                                                    # (the scan has ended: not seen)
                if i0 <= e0:
                    case, v = "behind", seabed[i1 + 1, f]                    # (IndexError if it reaches the end, as there)
                elif i1 >= P - e0:
                    case, v = "front", seabed[i0 - 1, f]
                else:
                    case, v = "mean", np.mean(seabed[[i0 - 1, i1 + 1], f])
                seabed[i0:i1 + 1, f] = v
                if runs is not None:
                    runs.append((f, i0, i1, case))
    return np.rint(np.median(seabed, axis=1)).astype(int)


def estimate_seabed(planes, chunk_pings=SEABED_CHUNK_PINGS, device=None):
    """The seabed line ``Echogram.get_seabed`` estimates for an echogram without a stored one, from ALL its frequency
    planes: int64 [n_pings], the reference's values.  ``planes``: the F arrays [n_range, n_pings] of ``data_memmaps()``
    (uploaded in chunks of ``chunk_pings`` pings plus one halo ping on each side, transposed on the GPU), or a float32
    tensor [F, n_pings, n_range] that is already resident (one launch, nothing uploaded).  The stencils, the gated
    argmax and the column maxima run in ``crimac_seabed_columns``; ``finish_seabed`` ends on the host."""
    if isinstance(planes, torch.Tensor) and planes.is_cuda:
        F, P, R = (int(v) for v in planes.shape)
        dev = planes.device
    else:
        planes = list(planes)
        F, (R, P) = len(planes), (int(v) for v in planes[0].shape)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if any(tuple(m.shape) != (R, P) for m in planes):
            raise ValueError("estimate_seabed: the frequency planes differ in shape")
    n = seabed_rows(R)[0]
    if n >= R:
        raise ValueError(f"estimate_seabed: {R} range rows leave nothing below the {n} rows the estimate skips")
    idx = torch.empty((F, P), dtype=torch.int32, device=dev)
    colmax = torch.empty((F, P), dtype=torch.float32, device=dev)
    if isinstance(planes, torch.Tensor):
        seabed_columns(planes.contiguous(), 0, 0, n, idx, colmax)
    else:
        step = P if not chunk_pings or chunk_pings <= 0 else int(chunk_pings)
        for s in range(0, P, step):
            e = min(P, s + step)
            lo, hi = max(0, s - 1), min(P, e + 1)
            slab = torch.stack([torch.as_tensor(np.ascontiguousarray(m[:, lo:hi], dtype=np.float32)) for m in planes])
            chunk = slab.to(dev).permute(0, 2, 1).contiguous()                        # [F, pings, range]
            seabed_columns(chunk, lo < s, hi > e, n, idx, colmax, ping0=s)
    return finish_seabed(idx.cpu().numpy(), colmax.cpu().numpy(), R)


def estimate_seabed_memm(echogram, chunk_pings=SEABED_CHUNK_PINGS, device=None):
    """``estimate_seabed`` for a memmap echogram: every frequency it has (``data_memmaps()`` with no selection, as
    ``data_numpy()`` in data_reader.py:465), whatever subset the model reads."""
    return estimate_seabed(echogram.data_memmaps(), chunk_pings=chunk_pings, device=device)


def _memm_seabed(echogram, seabed, n_pings, data, frequencies):
    """The seabed vector of ``predict_echogram_memm`` / ``evaluate_echogram_memm``: ``seabed`` None -> the reader's
    ``get_seabed``; "estimate" -> the GPU estimate (``data``, the resident [C, pings, range] tensor, is reused when the
    model's frequencies are exactly the echogram's); an integer array [n_pings] -> taken as given."""
    if seabed is None:
        return np.asarray(echogram.get_seabed(0, n_pings)).astype(np.int32)
    if isinstance(seabed, str):
        if seabed != "estimate":
            raise ValueError(f"seabed must be None, 'estimate' or an integer array, got {seabed!r}")
        own = getattr(echogram, "frequencies", None)
        if own is not None and [int(f) for f in own] == [int(f) for f in frequencies]:
            return estimate_seabed(data).astype(np.int32)
        return estimate_seabed_memm(echogram, device=data.device).astype(np.int32)
    sb = np.asarray(seabed)
    if sb.dtype.kind not in "iu" or sb.shape != (n_pings,):
        raise ValueError(f"seabed: an integer array of the echogram's {n_pings} pings, got {sb.dtype} {sb.shape}")
    return sb.astype(np.int32)


def _load_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, meta_channels, out_f16, wide,
                        seabed=None):
    """One memmap echogram as ONE resident chunk (ping_start 0): the arrays are transposed to the ping-major layout of the
    gather kernel on the GPU.  Returns (the loaded ``ChunkPredictor``, the seabed vector)."""
    n_range, n_pings = (int(v) for v in echogram.shape)
    dev = segpipe.device
    model = segpipe.model.to(dev).eval()
    eng = model.infer_engine
    if not eng.lmi and eng.in_channels > len(segpipe.frequencies) and not meta_channels:
        raise ValueError(f"the model takes {eng.in_channels} input channels for {len(segpipe.frequencies)} frequencies "
                         "(metadata planes as input channels): pass meta_channels")
    data = torch.stack([torch.as_tensor(np.ascontiguousarray(m, dtype=np.float32))
                        for m in echogram.data_memmaps(segpipe.frequencies)]).to(dev)
    data = data.permute(0, 2, 1).contiguous()                                     # [C, pings, range]
    given = seabed is not None
    seabed = _memm_seabed(echogram, seabed, n_pings, data, segpipe.frequencies)
    labels = torch.as_tensor(np.ascontiguousarray(echogram.label_memmap()).astype(np.int16)).to(dev).t().contiguous()
    cp = ChunkPredictor(model, n_range, patch_size, patch_overlap, batch_size, out_f16=out_f16)
    if meta_channels:                    # metadata planes (late or early injection): built on the GPU, per batch of crops
        cp.meta_source = MetaSource.from_echogram(echogram, meta_channels, dev, seabed=seabed if given else None)
    cp.load_chunk(data, 0, labels, None, 0, n_pings, seabed=seabed, flavour="memm", wide=wide)
    return cp, seabed


def predict_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, predict_fn=None, meta_channels=None,
                          seabed=None, **kwargs):
    """``save_reader_predictions_memm`` (save_predict.py:222-265) for one memmap echogram: returns the
    ``[2, n_range, n_pings]`` float64 array the reference ``np.save``s (probabilities rounded to float16 first, :252).

    ``echogram``: the reference's ``Echogram`` API -- ``shape = (n_range, n_pings)``, ``data_memmaps(freqs)`` ->
    list of [n_range, n_pings] arrays, ``label_memmap()``, ``get_seabed(idx_ping, n_pings)``.  The whole echogram is
    one grid (ping_start 0); the arrays are transposed to the ping-major layout of the gather kernel on the GPU.
    ``meta_channels`` (the yaml's dict): the metadata planes of a UNet_LateMetInject model, or -- required for a model
    whose input channels outnumber the frequencies (early injection) -- its extra input channels, gathered into the
    crop with the data planes (which then take db_with_limits_scaled, transforms.py:57-64).
    ``seabed``: None -- the reader's ``get_seabed`` (which, for an echogram without a stored seabed.npy, estimates it on
    the host); ``"estimate"`` -- the same estimate on the GPU (``estimate_seabed``), the reader is not asked; an integer
    array [n_pings] -- taken as given.
    """
    cp, seabed = _load_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, meta_channels,
                                     out_f16=True, wide=False, seabed=seabed)
    grid = plan_eval_grid(cp.n_range, seabed, cp.end_ping, patch_size, patch_overlap, memm=True)
    out = cp.predict(grid, predict_fn=predict_fn)
    return out.cpu().numpy().astype(np.float64)


def integrate_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, spec, predict_fn=None,
                            meta_channels=None, seabed=None):
    """``integrate_survey`` for ONE memmap echogram: ``predict_echogram_memm``'s prediction (same arguments, the float16
    values it would return) reduced on the GPU against the resident sv plane; same pixel rule, same return value; the
    accumulators are not all-reduced (every rank that calls it returns the echogram's whole result).  A seabed-aware
    ``spec`` goes by the line the prediction used (``seabed``: None, an array or "estimate"); a callable
    ``spec.ping_edges`` is asked for ``echogram``.  For a whole memm survey
    ``integrate_echograms_memm`` is the integrating form of the packed flow (``predict_echograms_memm``)."""
    cp, seabed = _load_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, meta_channels,
                                     out_f16=True, wide=False, seabed=seabed)
    spec = spec.bind(segpipe.frequencies).resolve(echogram)
    grid = plan_eval_grid(cp.n_range, seabed, cp.end_ping, patch_size, patch_overlap, memm=True)
    cp.predict(grid, predict_fn=predict_fn)
    acc, cnt = new_integration(segpipe.device, spec, cp.end_ping, cp.n_range)
    cp.integrate(acc, cnt, spec)
    return finish_integration(acc, cnt, spec, cp.end_ping, cp.n_range, all_reduce=False)


# ---- schools from the predictions: connected regions of a class (csrc/schools.hip) ----------------------------------------
SCHOOL_CLASSES = {1: "sandeel", 2: "other"}          # class k reads plane k - 1 of the predictions
SCHOOLS_MAX_FREQS = hip.DEFINES["CRIMAC_SCHOOLS_MAX_FREQS"]
SCHOOL_FIELDS = ("anchor", "pixels", "bbox", "row_sum", "ping_sum", "sv_sum", "sv_pixels")


class SchoolSpec:
    """What a school is.  ``classes``: a subset of (1, 2) = (sandeel, other); class k is detected on plane k - 1 of the
    predictions with ``thresholds[k - 1]``: a pixel is foreground when its stored probability >= the threshold (> 0, so
    that pixels the scatter never wrote are background).  ``connectivity`` 4 or 8.  ``min_pixels``: schools with fewer
    pixels are dropped (after the chunks of a survey have been merged).  ``frequency``: the frequencies whose linear sv
    is summed per school, a value of ``segpipe.frequencies`` or a sequence of distinct ones (at most ``SCHOOLS_MAX_FREQS``);
    None takes 38 (kHz) or, failing that, 38000 (Hz), as ``IntegrationSpec``.  Results always carry a frequency axis
    (``sv_sum`` ``[F, K]``), F = 1 for a scalar.  ``max_schools``: the rows of the device table of one chunk and class; a
    chunk with more schools is reduced a second time with the count it reported.  ``bind(frequencies)`` returns the spec
    with ``channels`` looked up."""

    def __init__(self, classes=(1,), thresholds=(0.5, 0.5), connectivity=8, min_pixels=1, frequency=None, max_schools=65536):
        def integer(v):
            return not isinstance(v, bool) and isinstance(v, (int, np.integer))
        try:
            classes = tuple(classes)
        except TypeError:
            raise ValueError(f"SchoolSpec: classes={classes!r}: a sequence out of (1, 2) = (sandeel, other)") from None
        if not classes or len(set(classes)) != len(classes) or not all(integer(k) and k in SCHOOL_CLASSES for k in classes):
            raise ValueError(f"SchoolSpec: classes={classes!r}: a non-empty sequence of distinct classes out of (1, 2) = "
                             "(sandeel, other)")
        try:
            thresholds = tuple(float(t) for t in thresholds)
        except TypeError:
            raise ValueError(f"SchoolSpec: thresholds={thresholds!r}: two numbers (sandeel, other)") from None
        if len(thresholds) != 2 or not all(0.0 < t < float("inf") for t in thresholds):
            raise ValueError(f"SchoolSpec: thresholds={thresholds!r}: two finite numbers > 0 (pixels the scatter left at 0 "
                             "are background)")
        if connectivity not in (4, 8) or not integer(connectivity):
            raise ValueError(f"SchoolSpec: connectivity={connectivity!r}: 4 or 8")
        if not integer(min_pixels) or min_pixels < 1:
            raise ValueError(f"SchoolSpec: min_pixels={min_pixels!r} must be a positive integer")
        if not integer(max_schools) or not 1 <= max_schools < 2 ** 31:
            raise ValueError(f"SchoolSpec: max_schools={max_schools!r} must be a positive integer below 2^31")
        if isinstance(frequency, (tuple, list)):
            frequency = tuple(frequency)
            if not frequency:
                raise ValueError("SchoolSpec: frequency is an empty sequence: name at least one frequency")
            if len({float(f) for f in frequency}) != len(frequency):
                raise ValueError(f"SchoolSpec: frequency={list(frequency)} names a frequency twice")
            if len(frequency) > SCHOOLS_MAX_FREQS:
                raise ValueError(f"SchoolSpec: {len(frequency)} frequencies, one pass takes {SCHOOLS_MAX_FREQS} at most")
        self.classes = tuple(int(k) for k in classes)
        self.thresholds, self.connectivity, self.min_pixels = thresholds, int(connectivity), int(min_pixels)
        self.frequency, self.max_schools = frequency, int(max_schools)
        self.channels = None               # the data planes of ``frequencies``, looked up by ``bind``

    @property
    def frequencies(self):
        """The frequencies as a tuple; None for a scalar spec that ``bind`` has not resolved (None: 38 or 38000)."""
        if isinstance(self.frequency, tuple):
            return self.frequency
        return None if self.frequency is None else (self.frequency,)

    def bind(self, frequencies):
        """The spec with ``channels`` = the indices of its frequencies in ``frequencies``; ValueError if one is not there."""
        freqs = [float(f) for f in frequencies]
        wanted = self.frequencies
        if wanted is None:
            wanted = next(((f,) for f in (38, 38000) if float(f) in freqs), None)
            if wanted is None:
                raise ValueError(f"SchoolSpec: frequency 38 / 38000 is not among the model's frequencies {list(frequencies)}")
        for f in wanted:
            if float(f) not in freqs:
                raise ValueError(f"SchoolSpec: frequency {f} is not among the model's frequencies {list(frequencies)}")
        bound = SchoolSpec(self.classes, self.thresholds, self.connectivity, self.min_pixels,
                           wanted if isinstance(self.frequency, tuple) else wanted[0], self.max_schools)
        bound.channels = tuple(freqs.index(float(f)) for f in wanted)
        return bound


class SchoolTable:
    """The schools of one class of one resident chunk, on the GPU (``ChunkPredictor.detect_schools``): ``labels`` int32
    ``[n_range, n_pings]`` (-1 background, otherwise the linear index of the school's first pixel in raster order, its
    anchor), the table ``anchor`` / ``pixels`` / ``bbox`` / ``row_sum`` / ``ping_sum`` ``[capacity]``, ``sv_sum`` /
    ``sv_pixels`` ``[F, capacity]`` in ascending anchor order, ``found`` int64 [1] (the true count), ``edges`` int32
    ``[2, n_range]`` (the first and last ping column as school indices) and ``status`` int32 [1].  Everything is enqueued
    on the stream that was current; nothing has been waited for.
    ``plane``: the name of the label plane's engine buffer (``schools.<plane>.<class>``).  ``select``: None labels the
    predictions of the class; an annotation id (or ``SCHOOLS_IDS_IGNORED``) labels the chunk's raw ids instead
    (``crimac_schools_label_ids``): the annotated schools, same table."""

    def __init__(self, cp, spec, klass, keep_left, keep_right, plane="labels", select=None):
        self.cp, self.spec, self.klass, self.keep = cp, spec, klass, (keep_left, keep_right)
        self.n_range, self.n_pings, self.start_ping = cp.n_range, cp.end_ping - cp.start_ping, cp.start_ping
        self.min_pixels = spec.min_pixels
        dev = cp.out.device
        self.labels = cp.engine._buf(f"schools.{plane}.{klass}", (self.n_range, self.n_pings), torch.int32)
        self.status = torch.empty(1, dtype=torch.int32, device=dev)
        self.found = torch.empty(1, dtype=torch.int64, device=dev)
        self.edges = torch.empty((2, self.n_range), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            self._label(select)
        self._stats(spec.max_schools)

    def _label(self, select):
        cp, spec = self.cp, self.spec
        if select is None:
            call("crimac_schools_label", ptr(cp.out[self.klass - 1]), 1 if cp.out_f16 else 0, self.n_range, self.n_pings,
                 spec.thresholds[self.klass - 1], spec.connectivity, ptr(self.labels), ptr(self.status))
        else:
            call("crimac_schools_label_ids", ptr(cp.labels), int(cp.labels.shape[0]), 0, self.n_range, self.n_pings, select,
                 spec.connectivity, ptr(self.labels), ptr(self.status))

    def _stats(self, capacity):
        cp, spec, F = self.cp, self.spec, len(self.spec.channels)
        dev = cp.out.device
        self.capacity = K = int(capacity)
        i32 = torch.empty(5 * K, dtype=torch.int32, device=dev)
        i64 = torch.empty((3 + F) * K, dtype=torch.int64, device=dev)
        self.anchor, self.bbox = i32[:K], i32[K:].view(K, 4)
        self.pixels, self.row_sum, self.ping_sum, self.sv_pixels = i64[:K], i64[K:2 * K], i64[2 * K:3 * K], i64[3 * K:].view(F, K)
        self.sv_sum = torch.empty((F, K), dtype=torch.float64, device=dev)
        n = self.n_range * self.n_pings
        scratch = cp.engine._buf("schools.scratch", ((hip.DEFINES["CRIMAC_SCHOOLS_SCRATCH_PIXEL_BYTES"] * n + 16 + 7) // 8,),
                                 torch.float64)
        channels = (ctypes.c_int * F)(*spec.channels)          # a host array: it lives until the call returns
        with torch.cuda.device(dev):
            call("crimac_schools_stats", ptr(self.labels), self.n_range, self.n_pings, ptr(cp.data[0]), int(cp.data.stride(0)),
                 int(cp.data.shape[0]), channels, F, int(cp.data.shape[1]), cp.start_ping - cp.data_ping0, self.min_pixels,
                 int(self.keep[0]), int(self.keep[1]), K, ptr(self.anchor), ptr(self.pixels), ptr(self.bbox), ptr(self.row_sum),
                 ptr(self.ping_sum), ptr(self.sv_sum), ptr(self.sv_pixels), ptr(self.found), ptr(self.edges), ptr(scratch),
                 scratch.numel() * 8)

    def numpy(self):
        """Download the table (this waits for the stream): a chunk-local dict for ``merge_school_chunks`` -- the
        ``SCHOOL_FIELDS`` cut to the schools found, ``"edges"``, ``"start_ping"``, ``"n_pings"``, ``"n_range"``, ``"class"``,
        ``"frequencies"``.  A chunk with more schools than the table's rows is reduced once more with the count it
        reported -- the one case that launches again; the chunk must still be resident, so download before the next
        ``load_chunk``."""
        found = int(self.found.item())
        if int(self.status.item()) != 0:
            raise hip.HipLibraryError("crimac_schools_label: a union-find loop exceeded its iteration bound (status 1): the "
                                      "labels of this chunk are invalid")
        if found > self.capacity:
            self._stats(found)
            found = int(self.found.item())
        res = {name: getattr(self, name)[..., :found].cpu().numpy() if name in ("sv_sum", "sv_pixels")
               else getattr(self, name)[:found].cpu().numpy() for name in SCHOOL_FIELDS}
        if self.edges is not None:
            res["edges"] = self.edges.cpu().numpy()
        res.update(start_ping=self.start_ping, n_pings=self.n_pings, n_range=self.n_range)
        res["class"] = SCHOOL_CLASSES[self.klass]
        res["frequencies"] = self.spec.frequencies
        return res


# ---- schools scored against the annotations: the overlap of two label planes is a third labelling ----------------------------
SCHOOL_IDS = {1: 27, 2: 1}                           # the raw annotation id of class k (the mapping of csrc/labels.hip)
SCHOOLS_IDS_IGNORED = hip.DEFINES["CRIMAC_SCHOOLS_IDS_IGNORED"]      # `select` of the ids the label transform ignores


class SchoolOverlaps(SchoolTable):
    """The overlap of the schools of two label planes of one chunk (``a`` a ``SchoolTable``; ``b`` one, or any object with
    ``labels`` and ``status``): ``crimac_schools_label_both``, ``crimac_schools_stats`` with ``min_pixels`` 1, no kept edges
    and no edge columns, and ``crimac_schools_pair_anchors``.  Every row is one connected component of ``a >= 0 && b >= 0``
    and lies in exactly one (school of a, school of b) pair: ``pair`` int32 ``[capacity, 2]`` holds the two anchors."""

    def __init__(self, a, b, plane):
        self.a, self.b = a, b
        super().__init__(a.cp, a.spec, a.klass, False, False, plane=plane)

    def _label(self, select):
        self.min_pixels, self.edges = 1, None
        call("crimac_schools_label_both", ptr(self.a.labels), ptr(self.b.labels), self.n_range, self.n_pings,
             self.spec.connectivity, ptr(self.labels), ptr(self.status))

    def _stats(self, capacity):
        super()._stats(capacity)
        self.pair = torch.empty((self.capacity, 2), dtype=torch.int32, device=self.anchor.device)
        with torch.cuda.device(self.anchor.device):
            call("crimac_schools_pair_anchors", ptr(self.anchor), ptr(self.found), self.capacity, ptr(self.a.labels),
                 ptr(self.b.labels), ptr(self.pair))

    def numpy(self, a_anchor, b_anchor=None):
        """The rows as a dict: ``"anchor"``, ``"pixels"``, ``"sv_sum"`` / ``"sv_pixels"`` ``[F, n]`` in ascending anchor order,
        and ``"pred"`` (``"ann"``): the row of the component's school in the DOWNLOADED table of ``a`` (``b``), whose anchor
        column is given -- so after that table's own second pass, if it had one --, -1 for a school its table dropped.
        ``b_anchor`` None: no ``"ann"``."""
        if int(self.b.status.item()) != 0:
            raise hip.HipLibraryError("crimac_schools_label_ids: a union-find loop exceeded its iteration bound (status 1): the "
                                      "labels of this chunk are invalid")
        t = super().numpy()                          # (a table that overflowed: _stats again, the pairs with it)
        pair = self.pair[:len(t["anchor"])].cpu().numpy()
        res = {name: t[name] for name in ("anchor", "pixels", "sv_sum", "sv_pixels")}
        for name, col, anchors in (("pred", 0, a_anchor), ("ann", 1, b_anchor)):
            if anchors is not None:
                res[name] = _rows_of_anchors(anchors, pair[:, col])
        return res


def _rows_of_anchors(anchors, wanted):
    """The index of every ``wanted`` anchor in the ascending ``anchors``, int64; -1 for one that is not there."""
    anchors, wanted = np.asarray(anchors, dtype=np.int64), np.asarray(wanted, dtype=np.int64)
    if not len(anchors):
        return np.full(len(wanted), -1, dtype=np.int64)
    at = np.minimum(np.searchsorted(anchors, wanted), len(anchors) - 1)
    return np.where(anchors[at] == wanted, at, -1).astype(np.int64)


class SchoolScore:
    """The predicted schools of one class of one resident chunk against the annotated ones, on the GPU
    (``ChunkPredictor.score_schools``): ``predicted`` and ``annotated`` (``SchoolTable``), ``overlaps`` and -- with
    ``ignored`` -- ``ignored`` (``SchoolOverlaps`` of the predicted plane with the annotated plane / the plane of the ids
    the label transform ignores).  Nothing has been waited for."""

    def __init__(self, cp, spec, klass, keep_left, keep_right, ignored_plane):
        self.klass = klass
        self.predicted = SchoolTable(cp, spec, klass, keep_left, keep_right)
        self.annotated = SchoolTable(cp, spec, klass, keep_left, keep_right, plane="annotated", select=SCHOOL_IDS[klass])
        self.overlaps = SchoolOverlaps(self.predicted, self.annotated, "overlaps")
        self.ignored = None if ignored_plane is None else SchoolOverlaps(self.predicted, ignored_plane, "overlaps_ignored")

    def numpy(self):
        """Download (this waits for the stream; before the next ``load_chunk``, as ``SchoolTable.numpy``): ``"predicted"`` and
        ``"annotated"`` chunk-local tables, ``"overlaps"`` (``SchoolOverlaps.numpy``: rows of the two tables as downloaded)
        and ``"ignored_pixels"`` int64 per predicted row (zeros without ``ignored``)."""
        pred, ann = self.predicted.numpy(), self.annotated.numpy()
        res = {"predicted": pred, "annotated": ann, "overlaps": self.overlaps.numpy(pred["anchor"], ann["anchor"]),
               "ignored_pixels": np.zeros(len(pred["anchor"]), dtype=np.int64)}
        if self.ignored is not None:
            ign = self.ignored.numpy(pred["anchor"])
            hit = ign["pred"] >= 0
            np.add.at(res["ignored_pixels"], ign["pred"][hit], ign["pixels"][hit])
        return res


def merge_school_chunks(chunks, connectivity, min_pixels, index=False):
    """The schools of a survey from the chunk-local tables of ONE class (``SchoolTable.numpy()``; numpy only), ``chunks``
    in ascending ping order, each starting where the one before ends.  Schools of neighbouring chunks are one school when
    a foreground pixel of the last column of chunk i and one of the first column of chunk i + 1 lie in rows that differ by
    0 (``connectivity`` 4) or by at most 1 (8) -- read from the ``"edges"`` columns.  Merging adds ``pixels``, ``row_sum``,
    ``ping_sum``, ``sv_pixels`` and (in ascending chunk order) ``sv_sum``, unites the boxes and takes the smallest (row,
    global ping) anchor; ``min_pixels`` is applied after the merge.  Returns a dict of arrays sorted by (anchor row, anchor
    ping), pings global: ``"anchor"`` int64 [K, 2], ``"pixels"``, ``"bbox"`` [K, 4] (r0, r1, p0, p1 half-open), ``"row_sum"``,
    ``"ping_sum"``, ``"sv_sum"`` float64 [F, K], ``"sv_pixels"`` int64 [F, K], ``"frequencies"``, ``"class"``."""
    if connectivity not in (4, 8):
        raise ValueError(f"merge_school_chunks: connectivity={connectivity!r}: 4 or 8")
    if not chunks:
        raise ValueError("merge_school_chunks: no chunks")
    for a, b in zip(chunks, chunks[1:]):
        if a["start_ping"] + a["n_pings"] != b["start_ping"] or a["n_range"] != b["n_range"]:
            raise ValueError("merge_school_chunks: the chunks must follow each other in ping order with one range axis")
    first = np.cumsum([0] + [len(c["anchor"]) for c in chunks])        # the global id of a chunk's school 0
    parent = np.arange(first[-1])

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, (a, b) in enumerate(zip(chunks, chunks[1:])):
        right, left = np.asarray(a["edges"][1], dtype=np.int64), np.asarray(b["edges"][0], dtype=np.int64)
        n = len(right)
        for d in ((0,) if connectivity == 4 else (-1, 0, 1)):            # row of the right chunk = row of the left + d
            ra, rb = right[max(0, -d):n - max(0, d)], left[max(0, d):n - max(0, -d)]
            both = (ra >= 0) & (rb >= 0)
            for x, y in np.unique(np.stack([ra[both] + first[i], rb[both] + first[i + 1]], axis=1), axis=0):
                x, y = find(x), find(y)
                if x != y:
                    parent[max(x, y)] = min(x, y)
    total = int(first[-1])
    root = np.array([find(x) for x in range(total)], dtype=np.int64)
    roots, group = np.unique(root, return_inverse=True)
    G, F = len(roots), chunks[0]["sv_sum"].shape[0]
    out = {"pixels": np.zeros(G, np.int64), "row_sum": np.zeros(G, np.int64), "ping_sum": np.zeros(G, np.int64),
           "sv_sum": np.zeros((F, G), np.float64), "sv_pixels": np.zeros((F, G), np.int64)}
    big = np.iinfo(np.int64).max
    box = np.tile(np.array([big, 0, big, 0], np.int64), (G, 1))
    key = np.full(G, big, np.int64)                                       # the anchor as row * (survey end) + global ping
    end = int(chunks[-1]["start_ping"] + chunks[-1]["n_pings"])
    for i, c in enumerate(chunks):
        g = group[first[i]:first[i + 1]]
        s, w = int(c["start_ping"]), int(c["n_pings"])
        px = np.asarray(c["pixels"], np.int64)
        np.add.at(out["pixels"], g, px)
        np.add.at(out["row_sum"], g, c["row_sum"])
        np.add.at(out["ping_sum"], g, np.asarray(c["ping_sum"], np.int64) + s * px)
        for f in range(F):
            np.add.at(out["sv_sum"][f], g, c["sv_sum"][f])
            np.add.at(out["sv_pixels"][f], g, c["sv_pixels"][f])
        b = np.asarray(c["bbox"], np.int64).reshape(-1, 4)
        np.minimum.at(box[:, 0], g, b[:, 0])
        np.maximum.at(box[:, 1], g, b[:, 1])
        np.minimum.at(box[:, 2], g, b[:, 2] + s)
        np.maximum.at(box[:, 3], g, b[:, 3] + s)
        a = np.asarray(c["anchor"], np.int64)
        np.minimum.at(key, g, (a // w) * end + (a % w) + s)
    keep = out["pixels"] >= int(min_pixels)
    order = np.flatnonzero(keep)[np.argsort(key[keep], kind="stable")]
    res = {"anchor": np.stack([key[order] // end, key[order] % end], axis=1), "pixels": out["pixels"][order],
           "bbox": box[order], "row_sum": out["row_sum"][order], "ping_sum": out["ping_sum"][order],
           "sv_sum": out["sv_sum"][:, order], "sv_pixels": out["sv_pixels"][:, order],
           "frequencies": chunks[0]["frequencies"], "class": chunks[0]["class"]}
    if index:
        row = np.full(G, -1, dtype=np.int64)
        row[order] = np.arange(len(order))
        res["index"] = [row[group[first[i]:first[i + 1]]] for i in range(len(chunks))]
    return res


def merge_school_overlaps(overlap_chunks, pred_index, ann_index):
    """The pair overlaps of a survey from the chunk-local overlap rows (``SchoolScore.numpy()["overlaps"]``; numpy only), one
    per chunk in ascending ping order.  ``pred_index`` / ``ann_index``: the ``"index"`` of ``merge_school_chunks(..., index=True)``
    over the predicted / annotated tables of the same chunks; a row whose school was dropped on either side (-1 in the row
    itself or in the index) is dropped.  The rows of equal (pred, ann) pairs are added up: ``pixels`` and ``sv_pixels``
    exactly, ``sv_sum`` in ascending chunk order and, inside a chunk, in ascending component-anchor order.  Returns
    ``"pred"``, ``"ann"``, ``"pixels"`` int64 [M], ``"sv_sum"`` float64 / ``"sv_pixels"`` int64 [F, M], sorted by (pred, ann)."""
    if not overlap_chunks or not len(overlap_chunks) == len(pred_index) == len(ann_index):
        raise ValueError("merge_school_overlaps: one overlap table and one index of each side per chunk, at least one chunk")
    F = np.asarray(overlap_chunks[0]["sv_sum"]).shape[0]
    rows = {"pred": [], "ann": [], "pixels": [], "sv_sum": [], "sv_pixels": []}
    for c, pi, ai in zip(overlap_chunks, pred_index, ann_index):
        def merged(local, index):
            local, index = np.asarray(local, dtype=np.int64), np.asarray(index, dtype=np.int64)
            out = np.full(len(local), -1, dtype=np.int64)
            out[local >= 0] = index[local[local >= 0]]
            return out
        p, a = merged(c["pred"], pi), merged(c["ann"], ai)
        keep = (p >= 0) & (a >= 0)
        rows["pred"].append(p[keep])
        rows["ann"].append(a[keep])
        rows["pixels"].append(np.asarray(c["pixels"], dtype=np.int64)[keep])
        rows["sv_sum"].append(np.asarray(c["sv_sum"], dtype=np.float64).reshape(F, -1)[:, keep])
        rows["sv_pixels"].append(np.asarray(c["sv_pixels"], dtype=np.int64).reshape(F, -1)[:, keep])
    rows = {k: np.concatenate(v, axis=-1) for k, v in rows.items()}
    pairs, of = np.unique(np.stack([rows["pred"], rows["ann"]], axis=1), axis=0, return_inverse=True)
    of = of.reshape(-1)
    M = len(pairs)
    out = {"pred": pairs[:, 0], "ann": pairs[:, 1], "pixels": np.zeros(M, np.int64), "sv_sum": np.zeros((F, M), np.float64),
           "sv_pixels": np.zeros((F, M), np.int64)}
    np.add.at(out["pixels"], of, rows["pixels"])
    for f in range(F):                               # (np.add.at adds in the order of the rows: chunk, then anchor)
        np.add.at(out["sv_sum"][f], of, rows["sv_sum"][f])
        np.add.at(out["sv_pixels"][f], of, rows["sv_pixels"][f])
    return out


def _merge_school_scores(chunks, spec):
    """``{"predicted", "annotated", "overlaps", "ignored_pixels"}`` of ONE class from its ``SchoolScore.numpy()`` per chunk."""
    pred = merge_school_chunks([c["predicted"] for c in chunks], spec.connectivity, spec.min_pixels, index=True)
    ann = merge_school_chunks([c["annotated"] for c in chunks], spec.connectivity, spec.min_pixels, index=True)
    p_index, a_index = pred.pop("index"), ann.pop("index")
    ignored = np.zeros(len(pred["pixels"]), dtype=np.int64)
    for c, index in zip(chunks, p_index):
        np.add.at(ignored, index[index >= 0], c["ignored_pixels"][index >= 0])
    return {"predicted": pred, "annotated": ann, "ignored_pixels": ignored,
            "overlaps": merge_school_overlaps([c["overlaps"] for c in chunks], p_index, a_index)}


def detect_schools_survey(reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings, spec, start_ping=0,
                          labels_available=True, predict_fn=None, stats=None):
    """The predicted schools of one zarr survey: ``integrate_survey``'s chunk loop (the same feed, staging and upload
    overlap), but each chunk's float16 predictions are labelled and reduced to a table of schools on the GPU
    (``ChunkPredictor.detect_schools``); per chunk the table and the first and last ping column (as school indices) come
    back, and ``merge_school_chunks`` joins the schools that a chunk seam cut.  Returns ``{class k: result}`` for the
    classes of ``spec`` (a ``SchoolSpec``), each the dict of ``merge_school_chunks`` with global pings.  Single rank only:
    under an initialised process group of more than one rank it raises NotImplementedError before it reads anything."""
    if parallel.rank_world()[1] > 1:
        raise NotImplementedError("detect_schools_survey: one rank only (a school can span the chunks of several ranks); "
                                  "run it on one rank of the process group")
    flow = _SurveyChunks("detect_schools_survey", reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings,
                         start_ping, labels_available, True, stats, predict_fn, share_patches=False)
    spec = spec.bind(segpipe.frequencies)
    if not flow.chunks:
        raise ValueError(f"detect_schools_survey: no pings from start_ping={start_ping} on")
    tables = {k: [] for k in spec.classes}
    first, last = flow.chunks[0][0], flow.chunks[-1][1]

    def detect(cp):                              # (downloads before the chunk's device slot is handed back)
        for t in cp.detect_schools(spec, keep_left=cp.start_ping > first, keep_right=cp.end_ping < last):
            tables[t.klass].append(t.numpy())
    flow.check_model()
    with flow.feed(("schools",)) as feed:
        for _ in flow.predicted(feed, then=detect):
            flow.note("enqueue_s", feed.t_taken)
    return {k: merge_school_chunks(tables[k], spec.connectivity, spec.min_pixels) for k in spec.classes}


def detect_schools_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, spec, predict_fn=None,
                                 meta_channels=None, seabed=None):
    """``detect_schools_survey`` for ONE memmap echogram: ``predict_echogram_memm``'s prediction (same arguments, the
    float16 values it would return) labelled and reduced on the GPU.  The whole echogram is one chunk: no seams.  Returns
    ``{class k: result}`` as ``detect_schools_survey``."""
    cp, seabed = _load_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, meta_channels,
                                     out_f16=True, wide=False, seabed=seabed)
    spec = spec.bind(segpipe.frequencies)
    grid = plan_eval_grid(cp.n_range, seabed, cp.end_ping, patch_size, patch_overlap, memm=True)
    cp.predict(grid, predict_fn=predict_fn)
    return {t.klass: merge_school_chunks([t.numpy()], spec.connectivity, spec.min_pixels) for t in cp.detect_schools(spec)}


def score_schools_survey(reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings, spec, start_ping=0,
                         labels_available=True, predict_fn=None, stats=None, ignored=True):
    """``detect_schools_survey`` scored against the annotations in the same chunk pass (``ChunkPredictor.score_schools``):
    per chunk the predicted table, the table of the annotated schools (regions of the raw annotation id of the class, as
    stored) and the overlap rows come back; ``merge_school_chunks`` joins both kinds of schools across the seams and
    ``merge_school_overlaps`` adds the overlaps up per pair.  Returns ``{class k: {"predicted": result, "annotated": result,
    "overlaps": ..., "ignored_pixels": int64 [K predicted]}}``; ``"predicted"`` is what ``detect_schools_survey`` returns,
    ``"overlaps"`` refers to the rows of the two results.  ``school_iou`` / ``match_schools`` / ``school_detection_scores``
    take one class of it.  Single rank only, as ``detect_schools_survey``; a survey without labels is refused."""
    if parallel.rank_world()[1] > 1:
        raise NotImplementedError("score_schools_survey: one rank only (a school can span the chunks of several ranks); "
                                  "run it on one rank of the process group")
    flow = _SurveyChunks("score_schools_survey", reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings,
                         start_ping, labels_available, True, stats, predict_fn, share_patches=False)
    spec = spec.bind(segpipe.frequencies)
    if not flow.chunks:
        raise ValueError(f"score_schools_survey: no pings from start_ping={start_ping} on")
    scores = {k: [] for k in spec.classes}
    first, last = flow.chunks[0][0], flow.chunks[-1][1]

    def score(cp):                               # (downloads before the chunk's device slot is handed back)
        for t in cp.score_schools(spec, keep_left=cp.start_ping > first, keep_right=cp.end_ping < last, ignored=ignored):
            scores[t.klass].append(t.numpy())
    flow.check_model()
    with flow.feed(("schools",)) as feed:
        for _ in flow.predicted(feed, then=score):
            flow.note("enqueue_s", feed.t_taken)
    return {k: _merge_school_scores(scores[k], spec) for k in spec.classes}


def score_schools_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, spec, predict_fn=None,
                                meta_channels=None, seabed=None, ignored=True):
    """``score_schools_survey`` for ONE memmap echogram (``detect_schools_echogram_memm``'s prediction; one chunk, no seams)."""
    cp, seabed = _load_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, meta_channels,
                                     out_f16=True, wide=False, seabed=seabed)
    spec = spec.bind(segpipe.frequencies)
    grid = plan_eval_grid(cp.n_range, seabed, cp.end_ping, patch_size, patch_overlap, memm=True)
    cp.predict(grid, predict_fn=predict_fn)
    return {t.klass: _merge_school_scores([t.numpy()], spec) for t in cp.score_schools(spec, ignored=ignored)}


def school_iou(score):
    """Per overlap row of one class of a score: ``pixels / (predicted pixels + annotated pixels - pixels)``, float64 [M] --
    the mask IoU of COCO "segm" of the (predicted, annotated) pair."""
    ov = score["overlaps"]
    both = np.asarray(ov["pixels"], dtype=np.float64)
    union = (np.asarray(score["predicted"]["pixels"], np.int64)[ov["pred"]]
             + np.asarray(score["annotated"]["pixels"], np.int64)[ov["ann"]] - np.asarray(ov["pixels"], np.int64))
    return both / union.astype(np.float64)


def match_schools(score, min_iou=0.5):
    """One-to-one matches of predicted and annotated schools: the pairs with IoU >= ``min_iou`` are taken in descending
    IoU, ties in ascending (pred, ann), and a pair is a match when neither school has been used.  Above 0.5 a school has
    at most one such partner, so the match is unique.  Returns ``"pred"``, ``"ann"`` int64 and ``"iou"`` float64 [m], in the
    order taken."""
    ov, iou = score["overlaps"], school_iou(score)
    cand = np.flatnonzero(iou >= float(min_iou))
    cand = cand[np.lexsort((ov["ann"][cand], ov["pred"][cand], -iou[cand]))]
    used_p, used_a, taken = set(), set(), []
    for i in cand:
        p, a = int(ov["pred"][i]), int(ov["ann"][i])
        if p not in used_p and a not in used_a:
            used_p.add(p), used_a.add(a), taken.append(i)
    taken = np.asarray(taken, dtype=np.int64)
    return {"pred": np.asarray(ov["pred"], np.int64)[taken], "ann": np.asarray(ov["ann"], np.int64)[taken], "iou": iou[taken]}


def school_detection_scores(score, min_iou=0.5, max_ignored=0.5):
    """Object-level scores of one class of a score.  A match (``match_schools``) is a true positive; an annotated school
    without one a false negative; a predicted school without one a false positive -- unless more than ``max_ignored`` of
    its pixels lie on ids the label transform ignores: then it counts neither way (``"excluded"``).  Returns the counts
    ``"true_positives"``, ``"false_positives"``, ``"false_negatives"``, ``"excluded"``, ``"predicted"``, ``"annotated"``;
    ``"recall"``, ``"precision"``, ``"f1"``; ``"sv_recall"`` float64 [F]: the overlap ``sv_sum`` over the annotated ``sv_sum``,
    all schools; ``"school_sv_recall"`` [F, K annotated]: the same per annotated school; and ``"matches"``.  A division by
    zero gives NaN, as ``frequency_response``."""
    m = match_schools(score, min_iou)
    pred_px = np.asarray(score["predicted"]["pixels"], dtype=np.float64)
    n_pred, n_ann, tp = len(pred_px), len(score["annotated"]["pixels"]), len(m["pred"])
    unmatched = np.ones(n_pred, dtype=bool)
    unmatched[m["pred"]] = False
    excluded = int(np.count_nonzero(unmatched & (np.asarray(score["ignored_pixels"], np.float64) > float(max_ignored) * pred_px)))
    fp, fn = n_pred - tp - excluded, n_ann - tp

    def ratio(num, den):
        num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
        return np.divide(num, den, out=np.full(np.broadcast(num, den).shape, np.nan), where=den > 0)
    recall, precision = float(ratio(tp, tp + fn)), float(ratio(tp, tp + fp))
    ov, ann_sv = score["overlaps"], np.asarray(score["annotated"]["sv_sum"], dtype=np.float64)
    per_school = np.zeros_like(ann_sv)
    for f in range(ann_sv.shape[0]):
        np.add.at(per_school[f], ov["ann"], ov["sv_sum"][f])
    return {"true_positives": tp, "false_positives": fp, "false_negatives": fn, "excluded": excluded, "predicted": n_pred,
            "annotated": n_ann, "recall": recall, "precision": precision,
            "f1": float(ratio(2.0 * precision * recall, precision + recall)),
            "sv_recall": ratio(np.asarray(ov["sv_sum"], np.float64).sum(axis=1), ann_sv.sum(axis=1)),
            "school_sv_recall": ratio(per_school, ann_sv), "matches": m}


def school_centroids(result):
    """The centroid (row, global ping) of every school of a result, float64 [K, 2]: ``row_sum`` / ``ping_sum`` over ``pixels``."""
    px = np.asarray(result["pixels"], dtype=np.float64)
    return np.stack([np.asarray(result["row_sum"], np.float64) / px, np.asarray(result["ping_sum"], np.float64) / px], axis=1)


def school_nasc(result, range_step_m):
    """The scaling of ``nasc`` per school and frequency: ``4 pi 1852^2 * range_step_m * sv_sum``, float64 [F, K] (summed over
    the school's pings; a uniform range grid is assumed)."""
    return 4.0 * np.pi * 1852.0 ** 2 * float(range_step_m) * np.asarray(result["sv_sum"], dtype=np.float64)


def school_frequency_response(result, reference=None):
    """r(f) = sv_sum[f] / sv_sum[reference] per school, float64 [F, K], NaN where the reference sum is 0.  ``reference``: one
    of ``result["frequencies"]``; None takes 38 or, failing that, 38000 (as ``frequency_response``)."""
    freqs = [float(f) for f in result["frequencies"]]
    wanted = (38, 38000) if reference is None else (reference,)
    at = next((freqs.index(float(f)) for f in wanted if float(f) in freqs), None)
    if at is None:
        raise ValueError(f"school_frequency_response: reference {' / '.join(str(f) for f in wanted)} is not among the result's "
                         f"frequencies {list(result['frequencies'])}")
    sums = np.asarray(result["sv_sum"], dtype=np.float64)
    ref = np.broadcast_to(sums[at], sums.shape)
    return np.divide(sums, ref, out=np.full(sums.shape, np.nan), where=ref > 0)


def schools_to_boxes(result, extend_size=0):
    """The schools' boxes as int32 [K, 4] = (y0, y1, x0, x1), the format of ``eval_boxes`` /
    ``get_object_bounding_boxes`` (rows, then pings, half-open), grown by ``extend_size`` on every side as ``eval_boxes``
    grows a 'region' box (not clipped), so that predicted and annotated schools are comparable."""
    b = np.asarray(result["bbox"], dtype=np.int64).reshape(-1, 4)
    e = int(extend_size)
    return np.stack([b[:, 0] - e, b[:, 1] + e, b[:, 2] - e, b[:, 3] + e], axis=1).astype(np.int32)


# ---- a memm survey: many small echograms in one prediction feed ----------------------------------------------------------
MEMM_GROUP_BATCHES = 4            # default ``group_patches``: this many forward batches per group
MEMM_GROUP_ELEMS = 1 << 24        # pixels (range x pings) a group stages at most: 268 MB of fp32 planes at 4 frequencies
MEMM_MISC_SHARE = 8               # the int32 staging (descriptors, centres, src, seabed lines) is 1 / 8 of the pixels
MEMM_META_SHARE = 4               # the 64-bit staging of packed metadata (table, three vectors per echogram): 1 / 4 of them


def plan_memm_groups(items, group_patches, max_elems=None, key=None):
    """Cut a run of echograms into groups, lazily: yields lists of consecutive ``items``.  ``key(item)`` (default: the
    item itself) is ``(patches, elems)``.  A group is closed as soon as its patches reach ``group_patches``; an item that
    reaches ``group_patches`` alone, or whose ``elems`` exceed ``max_elems`` alone, is a group of its own; no other group
    holds more than ``max_elems`` elements.  An item without patches joins the group that is open."""
    if group_patches < 1:
        raise ValueError(f"group_patches must be positive, got {group_patches}")
    group, n, size = [], 0, 0
    for item in items:
        c, e = key(item) if key else item
        own = c >= group_patches or (max_elems is not None and e > max_elems)
        if group and (own or (max_elems is not None and size + e > max_elems)):
            yield group
            group, n, size = [], 0, 0
        group.append(item)
        n, size = n + c, size + e
        if own or n >= group_patches:
            yield group
            group, n, size = [], 0, 0
    if group:
        yield group


def shard_memm_groups(groups, rank, world):
    """Groups rank, rank + world, ... of ``groups`` (lazily), as ``predict_survey(shard="chunk")`` deals its chunks: the
    ranks' shares are disjoint, complete and keep the input order; no collective."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside the world of {world}")
    return itertools.islice(groups, rank, None, world)


class _MemmRecord:
    """One echogram of a memm survey as the planner sees it: extents, seabed line, patch grid.  ``meta`` (the flow packs
    metadata): + its metadata source as ``_MemmGroupStage`` stages it, ``(portion_of_year_scalar, portion_of_day_vector
    float64, time_vector_diff float64, seabed int64)`` -- the seabed vector being the one ``_load_echogram_memm`` hands to
    ``MetaSource.from_echogram``: the reader's ``_seabed`` when the survey's ``seabed`` argument is None (``own_seabed``),
    else the line estimated / called, ``seabed``.  Its 64-bit words count towards the echogram's share of the staging."""

    def __init__(self, echogram, seabed, patch_size, patch_overlap, meta=False, own_seabed=True):
        self.echogram = echogram
        self.n_range, self.n_pings = (int(v) for v in echogram.shape)
        self.seabed = seabed
        self.grid = plan_eval_grid(self.n_range, seabed, self.n_pings, patch_size, patch_overlap, memm=True)
        self.pixels = self.n_range * self.n_pings
        # what the echogram takes of a group's staging: its pixels, or -- a sliver with many pings -- its int32 words
        self.elems = max(self.pixels, MEMM_MISC_SHARE * (2 * hip.MEMM_DESC_WORDS + 3 * len(self.grid) + self.n_pings))
        self.meta, self.meta_words = None, 0
        if meta:
            def vec(a, dt):
                return np.ascontiguousarray(np.asarray(a)).astype(dt).reshape(-1)
            self.meta = (float(echogram.portion_of_year_scalar), vec(echogram.portion_of_day_vector, np.float64),
                         vec(echogram.time_vector_diff, np.float64), vec(echogram._seabed if own_seabed else seabed, np.int64))
            self.meta_words = hip.MEMM_META_WORDS + sum(len(v) for v in self.meta[1:])
            self.elems = max(self.elems, MEMM_META_SHARE * self.meta_words)

    def key(self):
        return len(self.grid), self.elems


class _MemmEdgeRecord(_MemmRecord):
    """A record of ``integrate_echograms_memm`` with EDSU cells: + ``spec``, the flow's bound spec with THIS echogram's
    edge table (``IntegrationSpec.resolve``).  The table travels as int64 words in the tail of the group's ``misc`` and
    counts towards the echogram's share of the staging."""

    def __init__(self, echogram, seabed, patch_size, patch_overlap, spec=None, **meta):
        super().__init__(echogram, seabed, patch_size, patch_overlap, **meta)
        self.spec = spec.resolve(echogram)
        words = 2 * hip.MEMM_DESC_WORDS + 3 * len(self.grid) + self.n_pings + 2 * len(self.spec.ping_edges) + 2
        self.elems = max(self.elems, MEMM_MISC_SHARE * words)


def _memm_survey_seabed(echogram, seabed, device):
    """The seabed line of one echogram of a survey: ``seabed`` None -> the reader's ``get_seabed``; "estimate" -> the GPU
    estimate, on a stream of its own (its read-back does not wait for the survey's forwards); a callable -> its result for
    this echogram."""
    n_pings = int(echogram.shape[1])
    if seabed is None:
        return np.asarray(echogram.get_seabed(0, n_pings)).astype(np.int32)
    if isinstance(seabed, str):
        if seabed != "estimate":
            raise ValueError(f"seabed must be None, 'estimate' or a callable, got {seabed!r}")
        with torch.cuda.stream(_seabed_stream(device)):
            return estimate_seabed_memm(echogram, device=device).astype(np.int32)
    return _memm_seabed(echogram, np.asarray(seabed(echogram)), n_pings, None, None)


_SEABED_STREAMS = {}


def _seabed_stream(device):
    device = torch.device(device)
    if device not in _SEABED_STREAMS:
        _SEABED_STREAMS[device] = torch.cuda.Stream(device=device)
    return _SEABED_STREAMS[device]


def iter_memm_groups(echograms, patch_size, patch_overlap, group_patches, seabed=None, max_elems=MEMM_GROUP_ELEMS,
                     rank=0, world=1, device=None, skip=None, record=_MemmRecord):
    """The host-side plan of ``predict_echograms_memm``: consumes ``echograms`` lazily and yields this rank's groups, each
    a list of records (``.echogram``, ``.seabed`` int32 [n_pings], ``.grid`` = ``plan_eval_grid(..., memm=True)`` with the
    echogram's own seabed).  Every rank walks every echogram's seabed line (the grouping depends on the patch counts) and
    reads the data of its own groups only.
    ``skip(echogram) -> bool`` (the resume rule of ``save_predictions_memm``) is asked AFTER the deal, about the echograms of
    this rank's own groups only: the groups and their owners are planned over the whole input, which is the same on every
    rank, so what one rank skips -- files another rank is writing meanwhile -- cannot move an echogram to another rank or
    to none.  A group of which nothing is left is dropped.
    ``record``: the record class (``evaluate_echograms_memm`` plans with ``_MemmEvalRecord``, which carries the boxes; a flow
    that packs metadata binds ``meta`` / ``own_seabed`` to it)."""
    records = (record(eg, _memm_survey_seabed(eg, seabed, device), patch_size, patch_overlap) for eg in echograms)
    mine = shard_memm_groups(plan_memm_groups(records, group_patches, max_elems, key=_MemmRecord.key), rank, world)
    if skip is None:
        return mine
    kept = ([r for r in g if not skip(r.echogram)] for g in mine)
    return (g for g in kept if g)


def _refuse_near_misses(name, kwargs, own):
    """``kwargs`` takes the other keys of the reference's ``config_args``; a keyword that is a near miss of one of the
    function's ``own`` (``difflib.get_close_matches``) is a misspelling: TypeError."""
    typos = {k: difflib.get_close_matches(k, own, n=1, cutoff=0.8) for k in kwargs}
    typos = {k: m[0] for k, m in typos.items() if m}
    if typos:
        raise TypeError(f"{name}: unknown keyword(s) " +
                        ", ".join(f"{k!r} (did you mean {m!r}?)" for k, m in sorted(typos.items())))


def _check_survey_seabed(name, seabed, single):
    if not (seabed is None or callable(seabed) or (isinstance(seabed, str) and seabed == "estimate")):
        raise TypeError(f"{name}: seabed is None, 'estimate' or a callable(echogram) -> integer array "
                        f"[n_pings], got {type(seabed).__name__}; an array belongs to a single echogram "
                        f"({single} takes one)")


class _MemmGroupStage:
    """What ``_MemmSurveyFlow`` needs to move a group of echograms through a ``_ChunkFeed``: the ``table`` of flat staging
    buffers (``cap`` pixels of ``C`` planes and of labels, ``n_misc`` int32 words), the transposed planes per device slot
    (``extra``), the reader thread's copy of a group into a pinned slot (``read``) and the transposes on the copy stream
    (``transpose``).  ``misc`` holds, in this order: the descriptor table int64 [n][MEMM_DESC_WORDS] | the centres int32
    [P][2] | src int32 [P] | the seabed lines | the caller's tail.
    ``meta`` (the flow packs metadata; the records carry ``.meta``): + the buffer ``meta`` of ``n_meta`` 64-bit words, held
    as float64 and written through int64 / float64 views: the table [n][MEMM_META_WORDS] (crimac_memm_meta_desc) | per
    echogram portion_of_day_vector | time_vector_diff | the int64 seabed vector.  It travels in the group's pinned upload."""

    def __init__(self, dev, C, cap, frequencies, meta=False):
        self.dev, self.C, self.cap, self.frequencies, self.meta = dev, C, cap, frequencies, bool(meta)
        self.n_misc = cap // MEMM_MISC_SHARE + 2 * hip.MEMM_DESC_WORDS
        self.table = {"data": (C * cap, torch.float32), "lab": (cap, torch.int16), "misc": (self.n_misc, torch.int32)}
        if self.meta:
            self.n_meta = cap // MEMM_META_SHARE + hip.MEMM_META_WORDS
            self.table["meta"] = (self.n_meta, torch.float64)

    def extra(self):
        return {"data_t": [torch.empty(self.C * self.cap, dtype=torch.float32, device=self.dev) for _ in range(2)],
                "lab_t": [torch.empty(self.cap, dtype=torch.int16, device=self.dev) for _ in range(2)]}

    def read(self, bufs, host, k, group, out=None, tail=None):
        """Group ``k`` (device slot k & 1) into the pinned slot ``host``; the descriptors point at the transposed planes,
        at the seabed lines inside the uploaded ``misc`` and -- ``out``: the flat float16 prediction buffer -- at the
        echogram's [2, range, pings] share of it.  ``tail(group, misc, at) -> end``: writes the caller's words behind the
        seabed lines.  Returns (uploads, the pixel offset of every echogram, the group's pixels, where the tail starts)."""
        C, W = self.C, hip.MEMM_DESC_WORDS
        n, P = len(group), sum(len(r.grid) for r in group)
        misc = host["misc"].numpy()
        desc = misc[:2 * W * n].view(np.int64).reshape(n, W)
        o_cen, o_src, o_sb = 2 * W * n, 2 * W * n + 2 * P, 2 * W * n + 3 * P
        offs, off, p0 = [], 0, 0
        for i, r in enumerate(group):
            R, Wp, npx, Pe = r.n_range, r.n_pings, r.pixels, len(r.grid)
            assert o_sb + Wp <= self.n_misc and off + npx <= self.cap, "memm group staging too small"
            d = host["data"][C * off:C * (off + npx)].view(C, R, Wp).numpy()
            for c, m in enumerate(r.echogram.data_memmaps(self.frequencies)):
                np.copyto(d[c], m, casting="unsafe")
            np.copyto(host["lab"][off:off + npx].view(R, Wp).numpy(), r.echogram.label_memmap(), casting="unsafe")
            misc[o_sb:o_sb + Wp] = r.seabed
            misc[o_cen + 2 * p0:o_cen + 2 * (p0 + Pe)] = np.asarray(r.grid, dtype=np.int32).reshape(-1)
            misc[o_src + p0:o_src + p0 + Pe] = i
            desc[i] = (bufs["data_t"][k & 1].data_ptr() + 4 * C * off, bufs["lab_t"][k & 1].data_ptr() + 2 * off,
                       bufs["dev"][k & 1]["misc"].data_ptr() + 4 * o_sb,
                       0 if out is None else out.data_ptr() + 2 * 2 * off, Wp, R)
            offs.append(off)
            off, p0, o_sb = off + npx, p0 + Pe, o_sb + Wp
        o_tail = o_sb
        if tail is not None:
            o_sb = tail(group, misc, o_sb)
            assert o_tail <= o_sb <= self.n_misc, "memm group staging too small"
        uploads = {"data": host["data"][:C * off], "lab": host["lab"][:off], "misc": host["misc"][:o_sb]}
        if self.meta:
            uploads["meta"] = host["meta"][:self._read_meta(host["meta"].numpy(), bufs["dev"][k & 1]["meta"].data_ptr(),
                                                            group)]
        return uploads, offs, off, o_tail

    def _read_meta(self, words, base, group):
        """The metadata table and vectors of ``group`` into ``words`` (float64 view of the pinned slot); the descriptors
        point into the device copy at ``base``, as the seabed lines of ``misc`` do.  Returns the words written."""
        M, n = hip.MEMM_META_WORDS, len(group)
        ints = words.view(np.int64)
        at = M * n
        for i, r in enumerate(group):
            assert at + r.meta_words - M <= self.n_meta, "memm group staging too small (metadata)"
            words[M * i] = r.meta[0]
            for j, v in enumerate(r.meta[1:]):
                ints[M * i + 1 + 2 * j:M * i + 3 + 2 * j] = (base + 8 * at, len(v))
                (ints if v.dtype == np.int64 else words)[at:at + len(v)] = v
                at += len(v)
        return at

    def transpose(self, feed, k, d, group, offs):
        """The uploaded planes of group ``k`` to the ping-major layout of the gather kernels, on the copy stream; the
        main stream waits for it."""
        C = self.C
        data_t, lab_t = feed.bufs["data_t"][k & 1], feed.bufs["lab_t"][k & 1]
        with torch.cuda.stream(feed.copy_stream):
            for r, off in zip(group, offs):
                R, Wp, npx = r.n_range, r.n_pings, r.pixels
                data_t[C * off:C * (off + npx)].view(C, Wp, R).copy_(
                    d["data"][C * off:C * (off + npx)].view(C, R, Wp).permute(0, 2, 1))
                lab_t[off:off + npx].view(Wp, R).copy_(d["lab"][off:off + npx].view(R, Wp).t())
        feed.main.wait_stream(feed.copy_stream)


def _ordered_groups(groups, single, enqueue, take):
    """The ONE loop of the memm survey flows over ``groups`` (namespaces as ``_MemmSurveyFlow`` stages them): results in
    input order while the download of group k overlaps the enqueue of group k + 1.  A packed group: ``enqueue(g)``
    launches everything for it (``feed.computed()`` and the start of its download included) and returns the ticket of its
    results, or None when nothing comes back; only THEN is the previous ticket taken -- ``take(ticket)``: an iterable of
    results, which waits for the download.  A solo group (``g.offs is None``, ``g.solo`` = seabed and meta_channels): the
    ticket that is kept is taken first, then ``single(echogram, seabed, meta_channels)`` runs, in its place in the order.
    The last ticket is taken at the end.  Yields what ``take`` and ``single`` produce."""
    pending = None
    for g in groups:
        ticket = None if g.offs is None else enqueue(g)
        if pending is not None:
            yield from take(pending)
        pending = ticket
        if g.offs is None:
            yield single(g.group[0].echogram, *g.solo)
    if pending is not None:
        yield from take(pending)


class _MemmSurveyFlow:
    """What ``predict_echograms_memm``, ``integrate_echograms_memm`` and ``evaluate_echograms_memm`` share: a memm survey
    -- many small echograms -- moved through ONE ``_ChunkFeed``, forward batches packed across echograms.  Each of them is
    this flow, its closures ``single`` / ``enqueue`` / ``take`` and one ``run``; the ordering rule: ``_ordered_groups``.

    ``echograms``: any iterable of the reference's ``Echogram`` API, consumed lazily (a few groups ahead of the group at
    work).  Consecutive echograms form *groups* (``plan_memm_groups``): a group is closed when its patches reach
    ``group_patches`` (default ``MEMM_GROUP_BATCHES`` forward batches) or its pixels ``group_elems`` (default
    ``MEMM_GROUP_ELEMS``: the staging is allocated for that many).  All patches of a group form ONE patch list, cut into
    forward batches of ``max(batch_size, INTERNAL_BATCH)`` (``batch_size`` with a ``predict_fn``, as in
    ``ChunkPredictor.predict``): only the last batch of a group is short.  The ``_multi`` entry points take each patch's
    source (and destination) from a descriptor table that goes up with the group's centres and seabed lines in one pinned
    copy (``_MemmGroupStage``); reader threads copy the next groups' memmaps into pinned staging, the copy stream uploads
    and transposes them while the current group computes.
    ``seabed``: None (the reader's ``get_seabed``), ``"estimate"`` (``estimate_seabed_memm`` per echogram) or a callable
    ``echogram -> integer array [n_pings]``; not an array, which belongs to one echogram.
    **Models with metadata planes** (``UNet_LateMetInject``, or metadata input channels): the metadata sources are per
    echogram.  By default these models take the per-echogram path (``alone``, ``each_alone``): the caller's
    single-echogram sibling for one echogram after the other; same interface, same results, none of the packing.
    ``pack_metadata=True`` (opt-in; no effect on a model without metadata) packs them like any other model: the group's
    metadata table and vectors go up with it (``_MemmGroupStage``), and ``crimac_gather_patches_memm_meta_multi`` (input
    channels) / ``crimac_meta_planes_multi`` (late injection) take each patch's scalar and vectors from that table.  It
    needs ``meta_channels``, whose planes must be the model's.
    An echogram larger than ``group_elems`` takes the per-echogram path, in its place in the order.
    Multi-GPU (torch.distributed initialised): the *groups* (``alone``: the echograms) are dealt round-robin to the ranks.
    ``skip(echogram) -> bool``: echograms to leave out; it is asked after the groups have been planned and dealt over the
    WHOLE input (``iter_memm_groups``), so every echogram keeps its rank whatever the ranks skip.
    ``stats`` (a dict): receives ``groups``, ``batches`` (the patches of every packed forward batch),
    ``fallback_echograms`` (per-echogram path: metadata model) and ``solo_echograms`` (too large for the staging).
    ``kwargs``: the other keys of the reference's ``config_args``, accepted and ignored as by the sibling calls; a near
    miss of one of the caller's ``own`` keywords (``difflib.get_close_matches``: ``group_patch``, ``seabeds``, ``stat``
    ...) is refused as a misspelling.  The checks come before anything is read."""
    KNOBS = ("group_patches", "group_elems", "seabed", "stats", "predict_fn", "meta_channels", "pack_metadata")   # + ``own``

    def __init__(self, name, own, kwargs, echograms, segpipe, patch_size, patch_overlap, batch_size, predict_fn, seabed,
                 group_patches, group_elems, stats, skip=None, eval_mode=None, meta_channels=None, pack_metadata=False):
        _refuse_near_misses(name, kwargs, self.KNOBS + own)
        _check_survey_seabed(name, seabed, name.replace("echograms", "echogram"))
        if eval_mode not in (None, "all", "region", "trace"):
            raise ValueError(f"eval_mode={eval_mode!r}: 'all', 'region' or 'trace' (batch/transforms.py:87)")
        self.echograms, self.seabed, self.skip = echograms, seabed, skip
        self.patch_size, self.patch_overlap, self.frequencies = patch_size, patch_overlap, segpipe.frequencies
        self.dev, self.C = segpipe.device, len(segpipe.frequencies)
        self.eng = segpipe.model.to(self.dev).eval().infer_engine
        (self.pw, self.ph), self.overlap = (int(v) for v in patch_size), int(patch_overlap)
        self.step = max(int(batch_size), INTERNAL_BATCH) if predict_fn is None else int(batch_size)
        self.group_patches = MEMM_GROUP_BATCHES * self.step if group_patches is None else int(group_patches)
        self.cap = MEMM_GROUP_ELEMS if group_elems is None else int(group_elems)
        self.rank, self.world = parallel.rank_world()
        self.stats = {} if stats is None else stats
        self.stats.update(groups=0, batches=[], fallback_echograms=0, solo_echograms=0)
        eng = self.eng
        self.early = not eng.lmi and eng.in_channels > self.C            # metadata planes as extra input channels
        self.pack = (eng.lmi or self.early) and bool(pack_metadata)     # ... packed across echograms
        self.alone = (eng.lmi or self.early) and not self.pack          # ... or the per-echogram path
        self.meta_channels, self.flags, self._ring = meta_channels, 0, None
        if self.pack:
            if not meta_channels and self.early:
                raise ValueError(f"the model takes {eng.in_channels} input channels for {self.C} frequencies "
                                 "(metadata planes as input channels): pass meta_channels")
            if not meta_channels:
                raise ValueError("a UNet_LateMetInject model needs the metadata planes: pass meta_channels")
            self.flags, n_planes = meta_flags(meta_channels)
            takes = eng.meta_channels if eng.lmi else eng.in_channels - self.C
            if n_planes != takes:
                raise ValueError(f"the model takes {takes} metadata {'planes' if eng.lmi else 'input channels'}, "
                                 f"meta_channels builds {n_planes}")

    def solo(self, r):
        """``(seabed, meta_channels)`` of the single-echogram call for record ``r``, an echogram too large for the staging.
        With packed metadata the call must build the ``MetaSource`` a direct call would: the caller's None stays None (the
        depth planes then go by the reader's ``_seabed``), an estimated / called line is given as the array it is."""
        if self.pack:
            return (None if self.seabed is None else r.seabed), self.meta_channels
        return r.seabed, None

    def meta_planes(self, g, b0, Pb):
        """Late injection: the metadata planes float32 [Pb, Cm, ph, pw] of the batch at ``b0`` of staged group ``g``."""
        out = torch.empty((Pb, self.eng.meta_channels, self.ph, self.pw), dtype=torch.float32, device=self.dev)
        call("crimac_meta_planes_multi", ptr(g.meta), g.n, ptr(g.src, b0), ptr(g.cen, 2 * b0), Pb, self.ph, self.pw,
             self.flags, ptr(out))
        return out

    def each_alone(self):
        """This rank's echograms, each a solo "group" with the ``seabed`` argument of the single-echogram functions."""
        given = self.seabed is None or isinstance(self.seabed, str)
        for eg in shard_memm_groups(self.echograms, self.rank, self.world):
            if self.skip is None or not self.skip(eg):
                self.stats["fallback_echograms"] += 1
                sb = self.seabed if given else _memm_survey_seabed(eg, self.seabed, self.dev)
                yield types.SimpleNamespace(offs=None, group=[types.SimpleNamespace(echogram=eg)],
                                            solo=(sb, self.meta_channels))

    def ring(self, dtype, fixed=False):
        """The flow's ``_DownloadRing``, made when the first packed group asks for it (there is a group: the staging
        exists).  ``fixed``: around the staged ``out`` and ``pinned`` buffers of the caller's ``extra()``."""
        if self._ring is None:
            bufs = self.feed.bufs
            self._ring = _DownloadRing(self.dev, dtype, *((bufs["out"], bufs["pinned"]) if fixed else ()))
        return self._ring

    def run(self, tag, single, enqueue=None, take=None, **staging):
        """The flow: ``_ordered_groups`` over this rank's groups with the caller's three closures.  ``staging``: what
        ``staged`` takes; a flow that goes ``alone`` stages nothing and every echogram is a solo group."""
        if self.alone:
            yield from _ordered_groups(self.each_alone(), single, enqueue, take)
            return
        with self.staged(tag, **staging) as groups:
            yield from _ordered_groups(groups, single, enqueue, take)

    def batches(self, P):
        """``(first patch, patches)`` of every forward batch of a group of ``P`` patches."""
        for b0 in range(0, P, self.step):
            Pb = min(self.step, P - b0)
            self.stats["batches"].append(Pb)
            yield b0, Pb

    def gather_input(self, g, b0, Pb, labels_t=None):
        """The network input ``tiled.x`` of the batch at ``b0`` of staged group ``g``; ``labels_t`` (int16 [Pb, ph, pw],
        ``eval_mode`` 'region' / 'trace'): the transformed labels the data are masked by."""
        eng, C, ph, pw = self.eng, self.C, self.ph, self.pw
        x = eng._buf("tiled.x", (Pb * ph * pw, 16))
        lab = None if labels_t is None else ptr(labels_t)
        if self.pack and self.early:
            call("crimac_gather_patches_memm_meta_multi", eng.prec, ptr(g.misc), ptr(g.meta), g.n, ptr(g.src, b0), C,
                 ptr(g.cen, 2 * b0), Pb, ph, pw, ptr(x), 16, lab, 1, self.flags)
        elif labels_t is not None:
            call("crimac_gather_patches_memm_labels_multi", eng.prec, ptr(g.misc), g.n, ptr(g.src, b0), C,
                 ptr(g.cen, 2 * b0), Pb, ph, pw, ptr(x), 16, lab)
        else:
            call("crimac_gather_patches_memm_multi", eng.prec, ptr(g.misc), g.n, ptr(g.src, b0), C,
                 ptr(g.cen, 2 * b0), Pb, ph, pw, ptr(x), 16)
        return x

    def predict_group(self, g, predict_fn):
        """The forward batches of staged group ``g``: gather, predict, scatter into the float16 predictions the group's
        descriptors point at (``staged(out=...)``, zeroed by the caller)."""
        eng, ph, pw = self.eng, self.ph, self.pw
        for b0, Pb in self.batches(g.P):
            x = self.gather_input(g, b0, Pb)
            if predict_fn is not None:
                probs = predict_fn(x, Pb, ph, pw)
            elif eng.lmi:
                probs = eng.forward_nhwc(x, Pb, ph, pw, False, softmax=True, meta=self.meta_planes(g, b0, Pb))
            else:
                probs = eng.forward_nhwc_eval_split(x, Pb, ph, pw, softmax=True)
            call("crimac_scatter_patches_multi", ptr(probs), probs.shape[1], ptr(g.misc), g.n, ptr(g.src, b0),
                 ptr(g.cen, 2 * b0), Pb, ph, pw, self.overlap, SEABED_PAD, 1)

    @contextlib.contextmanager
    def staged(self, tag, record=_MemmRecord, extra=None, out=None, tail=None):
        """Plans this rank's groups; inside ``with``: an iterator that stages them one by one and yields each as a
        namespace -- ``k``, ``group`` (the records), ``offs`` (the pixel offset of every echogram; None: ONE echogram too
        large for the staging, nothing staged: it takes the per-echogram path with ``solo``), ``total`` (pixels), ``n`` / ``P``
        (echograms / patches), ``misc`` (the int32 staging) with its views ``cen`` [P][2] and ``src`` [P], ``o_tail``
        (where the caller's tail starts), ``meta`` (packed metadata: the 64-bit staging, the table first).  The caller enqueues the group's ``batches(P)`` and then calls
        ``feed.computed()`` (done already for a group too large).  Nothing is allocated for an empty plan.
        ``extra()``: the caller's buffers next to the stage's; ``out``: the name of the one the descriptors' ``out``
        point into; ``tail(group, misc, at) -> end`` writes the caller's words behind the seabed lines."""
        if self.pack:
            record = functools.partial(record, meta=True, own_seabed=self.seabed is None)
        groups = iter_memm_groups(self.echograms, self.patch_size, self.patch_overlap, self.group_patches, self.seabed,
                                  self.cap, self.rank, self.world, self.dev, self.skip, record)
        first = next(groups, None)
        if first is None:                                # nothing to do (an empty survey, everything skipped): no staging
            yield iter(())
            return
        groups = itertools.chain([first], groups)
        stage = _MemmGroupStage(self.dev, self.C, self.cap, self.frequencies, meta=self.pack)

        def read(job, slot):
            k, group = job
            if group[0].elems > self.cap:                # too large for the staging: nothing staged
                return {}, (group, None, 0, 0)
            uploads, *staged = stage.read(feed.bufs, slot(), k, group, out=feed.bufs.get(out), tail=tail)
            return uploads, (group, *staged)

        with _ChunkFeed(self.dev, (tag, self.C), stage.table, 3, enumerate(groups), read,
                        extra=lambda: dict(stage.extra(), **(extra() if extra else {}))) as feed:
            self.feed = feed
            self.eng.bind()
            yield self._staged_groups(feed, stage)

    def _staged_groups(self, feed, stage):
        W = hip.MEMM_DESC_WORDS
        for k, (d, (group, offs, total, o_tail)) in enumerate(feed):
            self.stats["groups"] += 1
            g = types.SimpleNamespace(k=k, group=group, offs=offs, total=total, o_tail=o_tail)
            if offs is None:                         # the per-echogram path, in its place in the order
                feed.computed()
                self.stats["solo_echograms"] += 1
                g.solo = self.solo(group[0])
            else:
                g.n, g.P = len(group), sum(len(r.grid) for r in group)
                stage.transpose(feed, k, d, group, offs)         # to the ping-major layout of the gather kernels
                g.misc, g.meta = d["misc"], d.get("meta")
                g.cen, g.src = g.misc[2 * W * g.n:], g.misc[2 * W * g.n + 2 * g.P:]
            yield g


def predict_echograms_memm(echograms, segpipe, patch_size, patch_overlap, batch_size, predict_fn=None, meta_channels=None,
                           seabed=None, group_patches=None, stats=None, group_elems=None, skip=None, pack_metadata=False,
                           **kwargs):
    """``save_reader_predictions_memm`` (save_predict.py:222-265) for a whole memm survey -- a directory of many small
    echograms: a generator of ``(echogram, float64 [2, n_range, n_pings])`` in input order, every array equal to
    ``predict_echogram_memm`` of that echogram (probabilities rounded to float16 on the GPU, then widened); each rank
    yields the echograms of its own groups only, no collective.

    Groups, batches, ``seabed``, metadata models and ``pack_metadata``, ``skip`` (``save_predictions_memm``'s resume rule),
    ``stats`` and ``kwargs``: ``_MemmSurveyFlow``.  Per batch ``crimac_gather_patches_memm_multi`` (packed metadata input
    channels: ``crimac_gather_patches_memm_meta_multi``) -> forward (packed late injection: with the planes of
    ``crimac_meta_planes_multi``) -> ``crimac_scatter_patches_multi``; the float16 results of a group leave through the
    flow's download ring, around buffers of the staging cache."""
    flow = _MemmSurveyFlow("predict_echograms_memm", ("skip",), kwargs, echograms, segpipe, patch_size, patch_overlap,
                           batch_size, predict_fn, seabed, group_patches, group_elems, stats, skip=skip,
                           meta_channels=meta_channels, pack_metadata=pack_metadata)

    def single(eg, sb, meta):            # the per-echogram path
        return eg, predict_echogram_memm(eg, segpipe, patch_size, patch_overlap, batch_size, predict_fn=predict_fn,
                                         meta_channels=meta, seabed=sb)

    def extra():            # the group's predictions, the pinned buffers of the download ring
        return dict(out=torch.empty(2 * flow.cap, dtype=torch.float16, device=flow.dev),
                    pinned=[torch.empty(2 * flow.cap, dtype=torch.float16).pin_memory() for _ in range(2)])

    def enqueue(g):
        ring = flow.ring(torch.float16, fixed=True)
        ring.zeroed(g.k, 2 * g.total)
        flow.predict_group(g, predict_fn)
        flow.feed.computed()
        return g.group, g.offs, ring.download(g.k, 2 * g.total)

    def take(ticket):
        group, offs, download = ticket
        host = _DownloadRing.wait(download)
        for r, off in zip(group, offs):
            res = host[2 * off:2 * (off + r.pixels)].view(2, r.n_range, r.n_pings)
            yield r.echogram, res.numpy().astype(np.float64)

    yield from flow.run("memm", single, enqueue, take, extra=extra, out="out")


def integrate_echograms_memm(echograms, segpipe, patch_size, patch_overlap, batch_size, spec, predict_fn=None,
                             meta_channels=None, seabed=None, group_patches=None, stats=None, group_elems=None, skip=None,
                             pack_metadata=False, **kwargs):
    """Echo integration by predicted class for a whole memm survey: ``predict_echograms_memm``'s packed feed with every
    echogram's predictions reduced on the GPU instead of downloaded.  A generator of ``(echogram, result)`` in input
    order, every result that of ``integrate_echogram_memm`` for the echogram: the same counts; the same sums bit for bit
    when the echogram's place in the group's staging keeps the 16-byte alignment of its operands, otherwise the same
    terms added in another fixed order (the kernel's narrow reads deal the pixels to the threads differently).  Each rank
    yields the echograms of its own groups, no collective.

    Groups, batches, ``seabed`` (None, ``"estimate"`` or a callable; a seabed-aware ``spec`` goes by the same line),
    metadata models and ``pack_metadata``, ``skip``, ``stats`` and ``kwargs``: ``_MemmSurveyFlow``.  After a group's
    scatters one integrate launch per echogram (``crimac_integrate_classes`` / ``crimac_integrate_layers`` by ``spec``)
    reads the echogram's float16 predictions, its plane of the transposed staging and its seabed line inside the group's
    uploaded ``misc``, and accumulates into the echogram's share of ONE flat fp64 / int64 buffer; the group's few
    kilobytes leave through the flow's download ring, nothing in the feed blocks.
    A spec with ``ping_edges`` (EDSU cells, ``crimac_integrate_edges``): every echogram has its own table -- a callable is
    asked per echogram while the groups are planned (``_MemmEdgeRecord``), a table given as an array serves them all --
    and the tables of a group go up in the tail of its ``misc``, in the group's one pinned copy."""
    flow = _MemmSurveyFlow("integrate_echograms_memm", ("spec", "skip"), kwargs, echograms, segpipe, patch_size,
                           patch_overlap, batch_size, predict_fn, seabed, group_patches, group_elems, stats, skip=skip,
                           meta_channels=meta_channels, pack_metadata=pack_metadata)
    spec = spec.bind(segpipe.frequencies)
    edsu = spec.ping_edges is not None
    C, W = flow.C, hip.MEMM_DESC_WORDS
    planes = 3 * spec.n_freqs                # per echogram [3, n_pb, n_rb], or [F, 3, n_pb, n_rb] (crimac_integrate_freqs)

    def single(eg, sb, meta):            # the per-echogram path
        return eg, integrate_echogram_memm(eg, segpipe, patch_size, patch_overlap, batch_size, spec, predict_fn=predict_fn,
                                           meta_channels=meta, seabed=sb)

    def tail(group, misc, at):                           # the edge tables int64, one after the other, 8-byte aligned
        at += at & 1
        for r in group:
            n = 2 * len(r.spec.ping_edges)
            assert at + n <= len(misc), "memm group staging too small (edge tables)"
            misc[at:at + n].view(np.int64)[:] = r.spec.ping_edges
            at += n
        return at

    def enqueue(g):
        ring, out = flow.ring(torch.float64), flow.feed.bufs["out"]
        shares, total = group_shares(g.group, spec, planes)
        o_edges = g.o_tail + (g.o_tail & 1)
        acc = ring.zeroed(g.k, 2 * total)            # [sums | counts]
        out[:2 * g.total].zero_()
        flow.predict_group(g, predict_fn)
        scratch = integration_scratch(flow.eng, max(s[0] * s[1] for _, s in shares), spec.n_freqs)
        data_t = flow.feed.bufs["data_t"][g.k & 1]
        o_sb = 2 * W * g.n + 3 * g.P              # the seabed lines inside ``misc``, one after the other
        for r, off, (at, shape) in zip(g.group, g.offs, shares):
            launch_integration(r.spec if edsu else spec, ptr(out, 2 * off), True, r.n_range, r.n_pings,
                               ptr(data_t, C * off + (0 if spec.multi else spec.channel) * r.pixels), r.n_pings, 0, 0,
                               shape[0], ptr(acc, at), ptr(acc, total + at), scratch, seabed=(ptr(g.misc, o_sb), 0, r.n_pings),
                               edges=ptr(g.misc, o_edges) if edsu else None, plane_stride=r.pixels, n_planes=C)
            o_sb += r.n_pings
            o_edges += 2 * (shape[0] + 1) if edsu else 0
        flow.feed.computed()
        return g.group, shares, ring.download(g.k, 2 * total)

    def take(ticket):
        group, shares, download = ticket
        return group_results(group, shares, *_DownloadRing.wait_sums_counts(download), spec, planes)

    staging = dict(record=functools.partial(_MemmEdgeRecord, spec=spec), tail=tail) if edsu else {}
    yield from flow.run("memm_integrate", single, enqueue, take, out="out", **staging,
                        extra=lambda: dict(out=torch.empty(2 * flow.cap, dtype=torch.float16, device=flow.dev)))


def save_predictions_memm(echograms, segpipe, target_dir, patch_size, patch_overlap, batch_size, resume=True,
                          suffix=".npy", **kwargs):
    """The loop over ``save_reader_predictions_memm`` (save_predict.py:222-265, :304-307) for a memm survey: one
    ``<echogram.name><suffix>`` per echogram in ``target_dir`` (the reference's caller names them ``<name>_pred.npy``),
    written with ``np.save`` from ``predict_echograms_memm``; ``resume``: an echogram whose file exists is skipped
    (:233-235) -- nothing of its data is read; its seabed line still is, because the groups and their ranks are planned
    over ALL echograms (``iter_memm_groups``): with several ranks writing into ``target_dir`` at once, the files a rank
    happens to see cannot change which rank owns an echogram.  ``kwargs`` go to ``predict_echograms_memm``.  Returns the
    number of files written (with several ranks: by this rank)."""
    os.makedirs(target_dir, exist_ok=True)

    def path(eg):
        return os.path.join(target_dir, eg.name + suffix)
    skip = (lambda eg: os.path.isfile(path(eg))) if resume else None
    written = 0
    for eg, out in predict_echograms_memm(echograms, segpipe, patch_size, patch_overlap, batch_size, skip=skip, **kwargs):
        np.save(path(eg), out)
        written += 1
    return written


# ---- whole-survey evaluation (evaluate.py:39-117 of the reference) on the tiled path -------------------------------------
PR_BINS = hip.PR_BINS      # CRIMAC_PR_BINS: float16 bit patterns of [0, 1] are 0 .. 0x3C00


def plan_eval_grid(n_range, seabed, n_pings, patch_size, patch_overlap, memm=False):
    """The patch grid of the reference's evaluation: ``DatasetGriddedReader(grid_start=None, grid_end=None,
    grid_mode='all')`` (evaluate.py:39-117; batch/dataset.py:148-160) -- ONE grid over the whole survey / echogram, range
    extent capped at the survey's deepest seabed + 50.  ``memm``: get_crop_memmap's centre adjustment for a water column
    not deeper than the patch (dataset.py:259-261; it writes into the Dataset's own grid, so ``center_coordinates`` and
    the label transform see the adjusted row too)."""
    grid = plan_grid(n_range, int(np.max(seabed)), 0, n_pings, patch_size, patch_overlap)
    if memm and n_range <= patch_size[1]:
        grid = grid.copy()
        grid[:, 0] = n_range // 2
    return grid


def plan_eval_chunks(grid, n_pings, patch_size, preload_n_pings):
    """Cut the survey's grid into chunks by CENTRE ping: ``[(patch indices, lo, hi)]`` for every chunk of ``plan_chunks``
    that owns a patch, with [lo, hi) the pings its patches touch (clipped to the survey).  Every patch belongs to exactly
    one chunk whatever the chunk size, so the chunk size cannot change the result."""
    chunks = plan_chunks(0, n_pings, preload_n_pings)
    starts = np.array([s for s, _ in chunks])
    owner = np.searchsorted(starts, np.clip(grid[:, 1], 0, n_pings - 1), side="right") - 1
    pw = int(patch_size[0])
    out = []
    for k in range(len(chunks)):
        idx = np.nonzero(owner == k)[0]
        if len(idx):
            x0 = grid[idx, 1] - pw // 2 + 1            # first ping of a patch (patch_coord_to_data_coord)
            out.append((idx, max(0, int(x0.min())), min(n_pings, int(x0.max()) + pw)))
    return out


CLASS_NAMES = {1: "sandeel", 2: "other"}      # crimac_unet/constants.py:20-22; further foreground classes: class{k}


def class_name(c):
    return CLASS_NAMES.get(int(c), f"class{int(c)}")


def check_classes(classes, n_classes, hist=None):
    """``classes`` of the evaluation flows: None (the sandeel histograms, [2, 16384]) or foreground class indices in
    1 .. n_classes - 1 without duplicates -> None / a tuple of ints; anything else: ValueError.  ``hist``: the histogram
    tensor a caller handed in must have the form that goes with it, [2, 16384] / [n_classes, 2, 16384]."""
    if classes is not None:
        if isinstance(classes, (str, bytes)) or not hasattr(classes, "__iter__"):
            raise ValueError(f"classes={classes!r}: a tuple of foreground class indices, e.g. (1, 2)")
        got = tuple(classes)
        if not got or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) for c in got):
            raise ValueError(f"classes={classes!r}: a non-empty tuple of integer class indices")
        got = tuple(int(c) for c in got)
        bad = [c for c in got if not 1 <= c < n_classes]
        if bad:
            raise ValueError(f"classes={got}: {bad} outside the foreground classes 1 .. {n_classes - 1} of a "
                             f"{n_classes}-class model (0 is the background)")
        if len(set(got)) != len(got):
            raise ValueError(f"classes={got}: a class is named twice")
        classes = got
    if hist is not None:
        want = (2, PR_BINS) if classes is None else (n_classes, 2, PR_BINS)
        if tuple(hist.shape) != want or hist.dtype != torch.int32 or not hist.is_contiguous():
            raise ValueError(f"hist {tuple(hist.shape)} {hist.dtype}: classes={classes} takes contiguous int32 {want}")
    return classes


def model_classes(classes, model, hist=None):
    """``check_classes`` against ``model.n_classes`` (a model or its engine); None asks nothing of the model."""
    return None if classes is None else check_classes(classes, model.n_classes, hist)


def new_histograms(dev, classes=None, model=None):
    """Zeroed PR histograms on ``dev``: int32 [2, 16384], with ``classes`` [model.n_classes, 2, 16384]."""
    shape = (2, PR_BINS) if classes is None else (model.n_classes, 2, PR_BINS)
    return torch.zeros(*shape, dtype=torch.int32, device=dev)


def add_pr_histograms(logits, labels, hist, classes=None):
    """One batch into ``hist``: ``crimac_pr_histogram`` (sandeel, [2, 16384]) or, with ``classes``,
    ``crimac_pr_histogram_classes`` (rows ``classes`` of [n_classes, 2, 16384])."""
    B, nc, H, W = logits.shape
    if classes is None:
        call("crimac_pr_histogram", ptr(logits), nc, ptr(labels), labels.element_size(), B, H, W, ptr(hist[0]),
             ptr(hist[1]))
    else:
        call("crimac_pr_histogram_classes", ptr(logits), nc, ptr(labels), labels.element_size(), B, H, W,
             sum(1 << c for c in classes), ptr(hist))


def finish_histograms(hist, all_reduce=True, classes=None):
    """int32 [2, 16384] on the GPU -> (hist_pos, hist_neg) int64 numpy; with several ranks the ONE collective of the flow
    (the histograms are the metric's sufficient statistic, as in ``SegPipe.get_pr_histograms_dataloader``).
    ``classes``: int32 [n_classes, 2, 16384] -> (hist_pos [K, 16384], hist_neg [K, 16384]), rows in the order of
    ``classes``; still one collective."""
    if hist.dim() == 3 or classes is not None:
        if classes is None:
            raise ValueError(f"hist {tuple(hist.shape)} holds one row per class: name the rows to return with classes=")
        classes = check_classes(classes, hist.shape[0], hist)
    if all_reduce and parallel.rank_world()[1] > 1:
        torch.distributed.all_reduce(hist)
    return split_histograms(hist.cpu().numpy(), classes)


def split_histograms(h, classes=None):
    """The histograms on the host, [2, 16384] / with ``classes`` [n_classes, 2, 16384] -> (hist_pos, hist_neg) int64
    ([K, 16384] each, rows in the order of ``classes``); a count in CRIMAC_PR_NAN_BIN raises, as sklearn's
    precision_recall_curve does on a NaN score."""
    h = np.asarray(h).astype(np.int64)
    if classes is not None:
        h = h[list(classes)]
        for c, row in zip(classes, h):
            if row[:, PR_BINS - 1].any():
                raise ValueError(f"Input contains NaN ({class_name(c)} probabilities of the validation set, class {c})")
        return np.ascontiguousarray(h[:, 0]), np.ascontiguousarray(h[:, 1])
    if h[:, PR_BINS - 1].any():           # CRIMAC_PR_NAN_BIN: sklearn raises on NaN scores as well
        raise ValueError("Input contains NaN (sandeel probabilities of the validation set)")
    return h[0], h[1]


def evaluate_survey(reader, segpipe, patch_size, patch_overlap, batch_size, preload_n_pings, eval_mode="all",
                    extend_size=20, predict_fn=None, on_batch=None, stats=None, classes=None, integration=None, **kwargs):
    """Test-set evaluation of one zarr survey (``validate_model_survey_zarr``, evaluate.py:39-81) on the tiled path:
    returns ``(hist_pos, hist_neg)`` int64 numpy [16384] -- what ``SegPipe.get_pr_histograms_dataloader`` returns for the
    reference's gridded test DataLoader over the same survey; ``SegPipe.validate_model_testing_from_histograms`` turns
    them into the PR curve / F1.

    The grid is the whole survey's (``plan_eval_grid``); it is cut into chunks of at most ``preload_n_pings`` centre
    pings (``plan_eval_chunks``), every chunk is read ONCE over the pings its patches touch -- data, annotation ids and
    seabed (``seabed_vector_or_mask``, checked on exactly those pings) -- into pinned staging, uploaded on a copy stream
    while the previous chunk computes, and evaluated by ``ChunkPredictor.evaluate``; nothing but the two histograms comes
    back.  With torch.distributed initialised the chunks are dealt to the ranks (``parallel.shard_indices``) and the
    histograms all-reduced once at the end; every rank returns the survey's histograms.
    ``reader``: the reference's zarr reader API (shape, get_data_slice, get_label_slice, get_seabed, get_seabed_mask;
    get_object_bounding_boxes for ``eval_mode`` 'region' / 'trace').
    ``classes`` (e.g. ``(1, 2)``, ``check_classes``): the histograms of each named foreground class from the same pass --
    ``(hist_pos [K, 16384], hist_neg [K, 16384])``, rows in the order of ``classes``; row ``classes.index(1)`` is what
    the call without ``classes`` returns.
    ``integration`` (a ``ScoredIntegration``): the same pass also integrates the survey's sv by annotated and predicted
    class (``ChunkPredictor.evaluate``); the return value is unchanged and the holder has the result
    (``integration.result()``).  With several ranks its accumulators are sum-reduced where the histograms are."""
    if classes is not None:
        classes = check_classes(classes, segpipe.model.n_classes)
    n_pings, n_range = (int(v) for v in reader.shape)
    dev = segpipe.device
    if integration is not None:
        if not isinstance(integration, ScoredIntegration):
            raise TypeError(f"evaluate_survey: integration is a ScoredIntegration, got {type(integration).__name__}")
        integration.begin(segpipe.frequencies, segpipe.model.n_classes, dev, n_pings, n_range)
    model = segpipe.model.to(dev).eval()
    cp = ChunkPredictor(model, n_range, patch_size, patch_overlap, batch_size)
    n_freq = len(segpipe.frequencies)
    if cp.engine.lmi or cp.engine.in_channels > n_freq:
        raise NotImplementedError("evaluate_survey: metadata planes (late or early injection) exist on the memm flavour "
                                  "only (batch/dataset.py:210-216) -- use evaluate_echogram_memm(meta_channels=...)")
    boxes = eval_boxes(reader, eval_mode, extend_size)
    if boxes is not None:
        boxes = torch.from_numpy(boxes).to(dev)
    sb_all = np.asarray(reader.get_seabed(0, n_pings, return_numpy=True)).astype(np.int32)
    grid = plan_eval_grid(n_range, sb_all, n_pings, patch_size, patch_overlap)
    chunks = plan_eval_chunks(grid, n_pings, patch_size, preload_n_pings)
    rank, world = parallel.rank_world()
    mine = [chunks[i] for i in parallel.shard_indices(len(chunks), rank, world)]
    hist = new_histograms(dev, classes, cp.engine)
    if stats is not None:
        stats["patches"] = int(sum(len(c[0]) for c in mine))
        stats["chunks"] = len(mine)
    if not mine:
        if integration is not None:
            integration.all_reduce()
        return finish_histograms(hist, classes=classes)
    widest = max(hi - lo for _, lo, hi in mine)

    def fetch(job, slot):
        _, lo, hi = job
        n = hi - lo
        host = slot()
        data = reader.get_data_slice(idx_ping=lo, n_pings=n, frequencies=segpipe.frequencies, return_numpy=True)
        d_t = host["data"][:n_freq * n * n_range].view(n_freq, n, n_range)
        np.copyto(d_t.numpy(), data, casting="same_kind")
        lab = np.asarray(reader.get_label_slice(idx_ping=lo, n_pings=n, return_numpy=True))
        if lab.dtype.kind == "f":                             # get_crop_zarr: nan_to_num(labels, nan=LABEL_BOUNDARY_VAL)
            lab = np.nan_to_num(lab, nan=-100.0)
        l_t = host["lab"][:n * n_range].view(n, n_range)
        np.copyto(l_t.numpy(), lab, casting="unsafe")
        sb, mask = seabed_vector_or_mask(reader, lo, hi, n_range, sb_all, 0)
        s_t = host["sb"][:n]
        s_t.numpy()[:] = sb[lo:hi]
        return {"data": d_t, "lab": l_t, "sb": s_t}, mask

    t_start = time.perf_counter()
    table = {"data": (n_freq * widest * n_range, torch.float32), "lab": (widest * n_range, torch.int16),
             "sb": (widest, torch.int32)}
    with _ChunkFeed(dev, "eval", table, 2, mine, fetch) as feed:      # 2 host slots: one chunk is read while one is uploaded
        for (idx, lo, hi), (d, mask) in zip(mine, feed):
            _load_staged(cp, d["data"], lo, d["lab"], lo, hi, d["sb"], mask, wide=True)
            cp.evaluate(grid[idx], hist, eval_mode, boxes, predict_fn=predict_fn, on_batch=on_batch, classes=classes,
                        integration=integration)
            feed.computed()
        if integration is not None:
            integration.all_reduce()
        out = finish_histograms(hist, classes=classes)
    if stats is not None:
        stats["seconds"] = time.perf_counter() - t_start
    return out


def evaluate_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, eval_mode="all", extend_size=20,
                           predict_fn=None, meta_channels=None, hist=None, on_batch=None, seabed=None, classes=None,
                           integration=None, **kwargs):
    """Test-set evaluation of one memmap echogram (one Dataset of ``validate_model_survey_memm``, evaluate.py:84-117) on
    the tiled path.  The echogram is one resident chunk, its grid the echogram's (``plan_eval_grid``); metadata models
    (late injection and metadata input channels) take ``meta_channels`` and ``seabed`` (None / "estimate" / an integer
    array) exactly as ``predict_echogram_memm`` does.

    ``hist`` (int32 [2, 16384] on the GPU): accumulate into it and return it -- a survey of several echograms, whose caller
    finishes with ``finish_histograms``; None: returns this echogram's ``(hist_pos, hist_neg)`` int64 numpy (no
    collective: every rank that calls it evaluates the echogram it passes).
    ``classes``: per-class histograms as ``evaluate_survey`` returns them; ``hist`` is then int32 [n_classes, 2, 16384].
    ``integration`` (a ``ScoredIntegration``): the echogram's sv by annotated and predicted class from the same pass, as in
    ``evaluate_survey``; no collective, and the return value is unchanged."""
    if classes is not None:            # (the default path asks nothing new of its arguments)
        classes = check_classes(classes, segpipe.model.n_classes, hist)
    if integration is not None:
        if not isinstance(integration, ScoredIntegration):
            raise TypeError(f"evaluate_echogram_memm: integration is a ScoredIntegration, got {type(integration).__name__}")
        if segpipe.model.n_classes != 3:            # (before the echogram is uploaded)
            raise ValueError(f"evaluate_echogram_memm: integration= with a model of n_classes={segpipe.model.n_classes}; the "
                             "scored integration is that of a 3-class model")
    cp, seabed = _load_echogram_memm(echogram, segpipe, patch_size, patch_overlap, batch_size, meta_channels,
                                     out_f16=False, wide=True, seabed=seabed)
    dev = segpipe.device
    boxes = eval_boxes(echogram, eval_mode, extend_size)
    if boxes is not None:
        boxes = torch.from_numpy(boxes).to(dev)
    grid = plan_eval_grid(cp.n_range, seabed, cp.end_ping, patch_size, patch_overlap, memm=True)
    own = hist is None
    if own:
        hist = new_histograms(dev, classes, cp.engine)
    if integration is not None:
        integration.begin(segpipe.frequencies, segpipe.model.n_classes, dev, cp.end_ping, cp.n_range)
    cp.evaluate(grid, hist, eval_mode, boxes, predict_fn=predict_fn, on_batch=on_batch, classes=classes,
                integration=integration)
    return finish_histograms(hist, all_reduce=False, classes=classes) if own else hist


# ---- a memm survey: many small echograms in one evaluation feed ------------------------------------------------------------
def memm_box_table(boxes):
    """The box table of a group as ``crimac_labels_extend_mask_multi`` takes it: ``boxes`` -- per echogram an int [n, 4]
    array of ALREADY extended boxes (``eval_boxes``) or None -> (box_off int32 [echograms + 1], boxes int32 [total, 4]), the
    tables one after the other.  Patches of echogram i are tested against rows [box_off[i], box_off[i + 1])."""
    rows = [np.zeros((0, 4), np.int32) if b is None else np.asarray(b, dtype=np.int32).reshape(-1, 4) for b in boxes]
    off = np.zeros(len(rows) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(b) for b in rows])
    return off, np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4), np.int32))


class _MemmEvalRecord(_MemmRecord):
    """``_MemmRecord`` + the echogram's extended school boxes (None for eval_mode 'all'); the int32 words of the boxes and
    of the echogram's entry in the offset table count towards what the echogram takes of a group's staging; ``scored``
    (the flow has a ``ScoredIntegrationSet``): + its entry in the share table, and the word that aligns the table."""

    def __init__(self, echogram, seabed, patch_size, patch_overlap, eval_mode="all", extend_size=20, scored=False, **meta):
        super().__init__(echogram, seabed, patch_size, patch_overlap, **meta)
        self.boxes = eval_boxes(echogram, eval_mode, extend_size)
        words = 2 * hip.MEMM_DESC_WORDS + 3 * len(self.grid) + self.n_pings + 2 + \
            (0 if self.boxes is None else 4 * len(self.boxes)) + (5 if scored else 0)
        self.elems = max(self.elems, MEMM_MISC_SHARE * words)


def _takes_keyword(fn, name):
    """Whether ``fn`` declares the keyword ``name`` (or ``**kwargs``)."""
    try:
        params = inspect.signature(fn).parameters.values()
    except (TypeError, ValueError):
        return False
    return any(p.kind is p.VAR_KEYWORD or (p.name == name and p.kind in (p.KEYWORD_ONLY, p.POSITIONAL_OR_KEYWORD))
               for p in params)


def evaluate_echograms_memm(echograms, segpipe, patch_size, patch_overlap, batch_size, eval_mode="all", extend_size=20,
                            predict_fn=None, meta_channels=None, seabed=None, hist=None, on_batch=None, group_patches=None,
                            group_elems=None, stats=None, pack_metadata=False, classes=None, integration=None, **kwargs):
    """Test-set evaluation of a whole memm survey (``validate_model_survey_memm``, evaluate.py:84-117) on the tiled path:
    ``(hist_pos, hist_neg)`` int64 numpy [16384], the sum of ``evaluate_echogram_memm`` over ``echograms``.

    Groups, batches, ``seabed``, metadata models and ``pack_metadata``, ``stats`` and ``kwargs``: ``_MemmSurveyFlow``, the plan of
    ``predict_echograms_memm`` with every echogram's own ``plan_eval_grid(..., memm=True)`` -- the int32 words of an
    echogram's boxes count towards its share of the staging.  Nothing but the two histograms comes back.  Per batch:
    ``crimac_gather_eval_crops_multi`` -> ``crimac_labels_test_transform_multi`` (-> ``crimac_labels_extend_mask_multi``
    with the group's box table, ``eval_boxes`` per echogram, for ``eval_mode`` 'region' / 'trace') -> network input
    (``_MemmSurveyFlow.gather_input``, for 'region' / 'trace' with the transformed labels, as ``ChunkPredictor.evaluate``
    chooses) -> ``eval_logits`` (packed late injection: with the planes of ``crimac_meta_planes_multi``) ->
    ``crimac_pr_histogram``.

    ``hist`` (int32 [2, 16384] on the GPU): accumulate into it and return it, no collective (as
    ``evaluate_echogram_memm``); None: ``finish_histograms`` -- with several ranks the histograms are all-reduced once,
    and every rank returns the survey's.
    ``on_batch(centres [P, 2] numpy, labels int16 [P, H, W], logits [P, 3, H, W])`` sees every batch; a callback that
    declares the keyword ``echograms`` also gets the echogram of every patch of the batch (a list of P).
    ``classes``: per-class histograms as ``evaluate_survey`` returns them, from ``crimac_pr_histogram_classes`` on the
    packed and on the per-echogram leg alike; ``hist`` is then int32 [n_classes, 2, 16384].
    ``integration`` (a ``ScoredIntegrationSet``): the same pass also integrates every echogram's sv by annotated and
    predicted class; the return value is unchanged and the set has the results -- ``integration.results()``: ``[(echogram,
    result)]`` in evaluation order, every result that of ``evaluate_echogram_memm(..., integration=ScoredIntegration(spec))``
    for the echogram: the same pixels, the same fp64 terms added in the order of the packed batches.  Per group ONE flat
    fp64 / int64 buffer holds every echogram's ``[3, 3, n_pb, n_rb]`` share (the share table goes up behind the group's
    ``misc``); every internal batch launches ``crimac_eval_crop_origins_multi`` -> ``crimac_integrate_confusion_multi``
    right after its histograms, on the same stream, and the group's few kilobytes leave through the flow's download
    ring: nothing in the feed blocks.  Metadata models without ``pack_metadata`` and echograms larger than
    ``group_elems`` are scored by a ``ScoredIntegration`` of their own, in their place in the order.  With several ranks
    ``results()`` holds the rank's own echograms (no collective) and ``totals()`` is sum-reduced once, where the histograms
    are; with ``hist`` given nothing is reduced.  None: no buffer, no launch.  A ``ScoredIntegration`` has ONE ping axis
    and is refused -- NotImplementedError; call ``evaluate_echogram_memm(..., integration=ScoredIntegration(spec))`` per
    echogram, or pass a set."""
    if integration is not None:
        if isinstance(integration, ScoredIntegration):
            raise NotImplementedError("evaluate_echograms_memm: integration= is not available on the packed flow (every "
                                      "echogram has its own ping axis); call evaluate_echogram_memm(echogram, ..., "
                                      "integration=ScoredIntegration(spec)) per echogram, or pass a ScoredIntegrationSet")
        if not isinstance(integration, ScoredIntegrationSet):
            raise TypeError(f"evaluate_echograms_memm: integration is a ScoredIntegrationSet, got {type(integration).__name__}")
        integration.begin(segpipe.frequencies, segpipe.model.n_classes)            # (before any data is touched)
    if classes is not None:            # (the default path asks nothing new of its arguments)
        classes = check_classes(classes, segpipe.model.n_classes, hist)
    flow = _MemmSurveyFlow("evaluate_echograms_memm",
                           ("eval_mode", "extend_size", "hist", "on_batch", "classes", "integration"), kwargs, echograms,
                           segpipe, patch_size, patch_overlap, batch_size, predict_fn, seabed, group_patches, group_elems,
                           stats, eval_mode=eval_mode, meta_channels=meta_channels, pack_metadata=pack_metadata)
    eng, dev, C, ph, pw = flow.eng, flow.dev, flow.C, flow.ph, flow.pw
    own = hist is None
    if own:
        hist = new_histograms(dev, classes, eng)
    tell = on_batch is not None and _takes_keyword(on_batch, "echograms")

    def emit(cen, labels_t, logits, egs):
        if tell:
            on_batch(cen, labels_t, logits, echograms=egs())
        elif on_batch is not None:
            on_batch(cen, labels_t, logits)

    def single(eg, sb, meta):            # the per-echogram path
        hook = None if on_batch is None else lambda cen, lab, logits: emit(cen, lab, logits, lambda: [eg] * len(cen))
        child = None if integration is None else ScoredIntegration(integration.spec)
        evaluate_echogram_memm(eg, segpipe, patch_size, patch_overlap, batch_size, eval_mode=eval_mode,
                               extend_size=extend_size, predict_fn=predict_fn, meta_channels=meta, hist=hist, on_batch=hook,
                               seabed=sb, classes=classes, integration=child)
        if child is not None:
            integration.add(eg, child.result())

    def done():
        if integration is not None and own:
            integration.all_reduce(dev)
        return finish_histograms(hist, classes=classes) if own else hist

    masked, scored = eval_mode != "all", integration is not None

    def tail(group, misc, at):                       # box_off [n + 1] | boxes [total][4]
        off, rows = memm_box_table([r.boxes for r in group])
        end = at + len(off) + rows.size
        assert end <= len(misc), "memm group staging too small (boxes)"
        misc[at:at + len(off)] = off
        misc[at + len(off):end] = rows.reshape(-1)
        return end

    def share_at(group, at):                         # the share table: behind the boxes, on an 8-byte boundary
        if masked:
            at += len(group) + 1 + 4 * sum(0 if r.boxes is None else len(r.boxes) for r in group)
        return at + (at & 1)

    def tail_scored(group, misc, at):                # ... | shares int64 [n][2] = (first word, n_pb)
        if masked:
            tail(group, misc, at)
        at = share_at(group, at)
        end = at + 4 * len(group)
        assert end <= len(misc), "memm group staging too small (shares)"
        misc[at:end].view(np.int64).reshape(-1, 2)[:] = [(first, shape[0]) for first, shape in integration.shares(group)[0]]
        return end

    def enqueue(g):
        misc, n, P, cen, src = g.misc, g.n, g.P, g.cen, g.src
        if scored:
            ring = flow.ring(torch.float64)
            shares, total = integration.shares(g.group)
            acc = ring.zeroed(g.k, 2 * total)        # [sums | counts]
            o_shares = share_at(g.group, g.o_tail)
        cen64 = cen[:2 * P].view(P, 2).long()            # the label kernels take `center_coordinates` as int64
        box_off, boxes = misc[g.o_tail:], misc[g.o_tail + n + 1:]
        if on_batch is not None:
            cen_h = np.concatenate([np.asarray(r.grid, dtype=np.int32).reshape(-1, 2) for r in g.group])
            egs_h = [r.echogram for r in g.group for _ in range(len(r.grid))]
        for b0, Pb in flow.batches(P):
            raw = eng._buf("eval.raw", (Pb, C, ph, pw), torch.float32)
            lab = eng._buf("eval.lab", (Pb, ph, pw), torch.int16)
            call("crimac_gather_eval_crops_multi", ptr(misc), n, ptr(src, b0), C, ptr(cen, 2 * b0), Pb, ph, pw,
                 ptr(raw), ptr(lab))
            labels_t = torch.empty((Pb, ph, pw), dtype=torch.int16, device=dev)
            call("crimac_labels_test_transform_multi", ptr(lab), lab.element_size(), ptr(raw), C - 1, 1e-7, 1e-4,
                 ptr(cen64, 2 * b0), ptr(misc), n, ptr(src, b0), SEABED_PAD, flow.overlap, ptr(labels_t), Pb, C, ph, pw)
            if masked:
                call("crimac_labels_extend_mask_multi", ptr(labels_t), ptr(raw), C, ptr(cen64, 2 * b0), ptr(boxes),
                     ptr(box_off), n, ptr(src, b0), -1, Pb, ph, pw)
            x = flow.gather_input(g, b0, Pb, labels_t if masked else None)
            meta = flow.meta_planes(g, b0, Pb) if eng.lmi and predict_fn is None else None
            logits = eval_logits(eng, x, Pb, ph, pw, meta=meta, predict_fn=predict_fn, split=True)
            if on_batch is not None:
                emit(cen_h[b0:b0 + Pb], labels_t, logits, lambda: egs_h[b0:b0 + Pb])
            add_pr_histograms(logits, labels_t, hist, classes)
            if scored:
                integration.add_batch(eng, logits, raw, labels_t, cen, src, b0, ptr(misc), n, ptr(misc, o_shares),
                                      ptr(acc), ptr(acc, total))
        flow.feed.computed()
        return (g.group, shares, ring.download(g.k, 2 * total)) if scored else None

    def take(ticket):
        group, shares, download = ticket
        integration.add_group(group, shares, *_DownloadRing.wait_sums_counts(download))
        return ()

    record = functools.partial(_MemmEvalRecord, eval_mode=eval_mode, extend_size=extend_size, scored=scored)
    for _ in flow.run("memm-eval", single, enqueue, take, record=record,
                      tail=tail_scored if scored else tail if masked else None):
        pass
    return done()
