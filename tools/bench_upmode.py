#!/usr/bin/env python3
"""up_mode 'transpose' vs 'upsample' in one process, B = 32 x 4 x 256 x 256, start_filts 64: the bf16 training step
(engine.train_step), the h3p eval forward, and the per-launch microseconds of the up-sampling layers' kernels (median
over the profiled passes; the weight-gradient launches run on the side stream, their events time them there).
usage: bench_upmode.py [steps] -> one JSON line"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import hip, synth  # noqa: E402

B, HW = 32, 256
UP_KERNELS = ("crimac_conv1x1_up2x", "crimac_up2x_adjoint", "crimac_conv1x1_dgrad", "crimac_conv1x1_wgrad",
              "crimac_igemm_conv", "crimac_upconv2x2_dgrad_bnb_prec", "crimac_wgrad")


def timed(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def launches(fn, passes=5):
    """name -> summed median us per pass of the launches of the up-sampling layers (and their transposed-conv peers)."""
    fn()
    torch.cuda.synchronize()
    hip.PROFILE = []
    for _ in range(passes):
        fn()
    torch.cuda.synchronize()
    prof, hip.PROFILE = hip.PROFILE, None
    k = len(prof) // passes
    out = {}
    for p in range(k):
        name = prof[p][0]
        if name not in UP_KERNELS:
            continue
        med = statistics.median(prof[s * k + p][2].elapsed_time(prof[s * k + p][3]) for s in range(passes))
        out[name] = out.get(name, 0.0) + 1e3 * med
    return {n: round(v, 1) for n, v in out.items()}


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    x = torch.from_numpy(synth.synth_echogram_batch(B, 4, HW, HW, seed=1)).cuda()
    lab = torch.from_numpy(synth.synth_labels(B, HW, HW, seed=2)).long().cuda()
    cw = torch.tensor([10.0, 300.0, 250.0], device="cuda")
    res = {}
    for mode in ("transpose", "upsample"):
        m = pkg.UNet_Baseline(3, 4, up_mode=mode, precision="bf16")
        m.load_state_dict(synth.synth_state_dict(seed=0, up_mode=mode))
        m = m.cuda().train()
        eng = m.engine
        step = lambda: eng.train_step(x, lab, cw, 1e-4, 0.9)          # noqa: E731
        res[f"bf16_step_ms_{mode}"] = round(timed(step, steps), 3)
        res[f"bf16_step_launch_us_{mode}"] = launches(step)
        mi = pkg.UNet_Baseline(3, 4, up_mode=mode, precision="h3p")
        mi.load_state_dict(synth.synth_state_dict(seed=0, up_mode=mode))
        mi = mi.cuda().eval()
        with torch.no_grad():
            fwd = lambda: mi(x)                                        # noqa: E731
            res[f"h3p_eval_ms_{mode}"] = round(timed(fwd, steps), 3)
            mi.infer_engine.eval_two_streams = False                   # (serial launches for the per-launch table)
            res[f"h3p_eval_launch_us_{mode}"] = launches(fwd)
            mi.infer_engine.eval_two_streams = True
        del m, mi, eng
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
