#!/usr/bin/env python3
"""Early metadata injection (metadata planes as extra INPUT channels of UNet_Baseline) at B = 32, 256 x 256:

  * the augmented training step (train_step_augmented) with in_channels 4 against 11 (4 frequencies + 7 planes);
  * crimac_augment_db_meta_nhwc alone against its byte floor (11 fp32 planes in, int64 labels in, 16-channel NHWC
    activations + int16 labels out);
  * memm tiled prediction (predict_echogram_memm) in patches/s without and with the metadata planes, h3p and bf16.

Prints one line per measurement and a JSON summary line at the end."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import synth, tiled_inference as ti  # noqa: E402
from crimac_classifiers_unet_amd.hip import call, ptr  # noqa: E402
from tools.fake_reader import FakeEchogram  # noqa: E402

NF, CM = 4, 7
HBM_BYTES_PER_S = 6.0e12
ALL_META = {k: True for k in ti.META_FLAGS}


def gpu_time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def bench_train(B, S, precision, steps, warmup):
    x_lin = torch.pow(10.0, torch.from_numpy(synth.synth_echogram_batch(B, NF, S, S, seed=1)) / 10.0).cuda()
    meta = torch.from_numpy(synth.synth_metadata(B, CM, S, S, seed=3)).cuda()
    lab = torch.from_numpy(synth.synth_labels(B, S, S, seed=2)).cuda()
    cw = torch.tensor([10.0, 300.0, 250.0], device="cuda")
    res = {}
    for cin in (NF, NF + CM):
        m = pkg.UNet_Baseline(3, cin, precision=precision)
        m.load_state_dict(synth.synth_state_dict(seed=0, in_channels=cin))
        m.cuda().train()
        eng = m.engine
        data = x_lin if cin == NF else torch.cat((x_lin, meta), 1).contiguous()
        kw = {} if cin == NF else {"n_data": NF}
        step = [0]

        def run():
            step[0] += 1
            eng.train_step_augmented(data, lab, cw, lr=1e-6, momentum=0.9, seed=step[0], **kw)
        res[cin] = gpu_time(run, steps, warmup)
        print(f"train_step_augmented {precision} B={B} {S}x{S} in_channels={cin}: {res[cin] * 1e3:.2f} ms/step",
              flush=True)
        if cin == NF + CM:
            lab64 = lab.long()
            x = eng._buf("x_nhwc", (B * S * S, 16))
            lo = eng._buf("aug.labels", (B, S, S), torch.int16)
            t = gpu_time(lambda: call("crimac_augment_db_meta_nhwc", eng.prec, ptr(data), ptr(lab64), 8, ptr(x), ptr(lo),
                                      None, 0, 0.0, 0.0, B, cin, S, S, 16, 7, 1, 1, 1, NF), steps * 4, warmup)
            nbytes = data.numel() * 4 + lab64.numel() * 8 + x.numel() * x.element_size() + lo.numel() * 2
            floor = nbytes / HBM_BYTES_PER_S
            res["augment_s"], res["augment_floor_s"], res["augment_bytes"] = t, floor, nbytes
            print(f"crimac_augment_db_meta_nhwc {precision}: {t * 1e6:.1f} us for {nbytes / 1e6:.0f} MB "
                  f"(floor {floor * 1e6:.1f} us at 6 TB/s, {floor / t * 100:.0f} %)", flush=True)
        del m, eng
        torch.cuda.empty_cache()
    return res


def bench_memm(precision, n_pings, n_range, batch, reps):
    rng = np.random.Generator(np.random.PCG64(1))
    sv = np.power(10.0, rng.uniform(-7.5, 0, size=(NF, n_range, n_pings))).astype(np.float32)
    labels = np.zeros((n_range, n_pings), dtype=np.int16)
    eg = FakeEchogram(sv, labels, np.full(n_pings, n_range - 100, dtype=np.int64))
    tv = 737000.25 + np.cumsum(rng.uniform(5e-6, 9e-6, size=n_pings))
    eg.portion_of_day_vector, eg.portion_of_year_scalar = tv % 1, 0.5
    eg.time_vector_diff = np.concatenate((np.diff(tv), [tv[-1] - tv[-2]])) / 6e-6 - 1
    n_patches = len(ti.plan_grid(n_range, n_range - 100, 0, n_pings))
    res = {}
    for cin, mc in ((NF, None), (NF + CM, ALL_META)):
        model = pkg.UNet_Baseline(3, cin, precision=precision)
        model.load_state_dict(synth.synth_state_dict(seed=0, in_channels=cin))

        class Pipe:
            frequencies = [18, 38, 120, 200]
            device = torch.device("cuda")
        pipe = Pipe()
        pipe.model = model
        ti.predict_echogram_memm(eg, pipe, (256, 256), 20, batch, meta_channels=mc)        # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            ti.predict_echogram_memm(eg, pipe, (256, 256), 20, batch, meta_channels=mc)
        dt = (time.perf_counter() - t0) / reps
        res[cin] = n_patches / dt
        print(f"predict_echogram_memm {precision} in_channels={cin}: {n_patches} patches in {dt * 1e3:.1f} ms -> "
              f"{res[cin]:.0f} patches/s", flush=True)
        del model, pipe
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pings", type=int, default=4096)
    ap.add_argument("--range", type=int, default=700)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    out = {"train_bf16": bench_train(a.batch, a.size, "bf16", a.steps, a.warmup)}
    for p in ("h3p", "bf16"):
        out["memm_" + p] = bench_memm(p, a.pings, a.range, a.batch, a.reps)
    print(json.dumps({k: {str(kk): vv for kk, vv in v.items()} for k, v in out.items()}))


if __name__ == "__main__":
    main()
