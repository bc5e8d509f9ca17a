"""Late-injection model, B = 32, UNet_LateMetInject(3, 4, 7) at 256 x 256: fused train step and eval forward per precision.

    python tools/bench_lmi.py --precisions h3p h3f --passes 3 --label this > line.json

Median of `--passes` alternating passes in ONE process (every pass times every quantity once, in turn); a precision the
checked-out tree refuses is reported as null.  One JSON line; profiles/lmi_h3f_bench.json keeps the lines of two checkouts
(the commit that brought the one-launch head and its parent, labelled so), taken alternately on one MI355X."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crimac_classifiers_unet_amd as pkg  # noqa: E402
from crimac_classifiers_unet_amd import synth  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", nargs="+", default=["h3p", "h3f"])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    B, S, cm = a.batch, 256, 7
    x = torch.from_numpy(synth.synth_echogram_batch(B, 4, S, S, seed=1)).cuda()
    meta = torch.from_numpy(synth.synth_metadata(B, cm, S, S, seed=3)).cuda()
    lab = torch.from_numpy(synth.synth_labels(B, S, S, seed=2)).cuda()
    cw = torch.tensor([10.0, 300.0, 250.0], device="cuda")
    sd = synth.synth_state_dict(seed=0, meta_in_channels=cm)
    jobs = {}
    for prec in a.precisions:
        try:
            m = pkg.UNet_LateMetInject(3, 4, cm, precision=prec)
            m.load_state_dict(sd)
            m.cuda().train()
            eng = m.engine
            eng.bind()
        except NotImplementedError as e:
            print(f"[bench_lmi] {prec}: {e}", file=sys.stderr)
            jobs[prec + "_train_ms"] = None
            continue
        jobs[prec + "_train_ms"] = (lambda eng=eng: eng.train_step(x, lab, cw, lr=0.0, momentum=0.0, meta=meta))
        if prec == "h3p":
            me = pkg.UNet_LateMetInject(3, 4, cm, precision=prec)
            me.load_state_dict(sd)
            me.cuda().eval()

            def fwd(me=me):
                with torch.no_grad():
                    me(x, meta)
            jobs[prec + "_eval_ms"] = fwd
    for fn in jobs.values():                     # warm-up: packing, buffers, occupancy look-ups
        if fn is not None:
            timed(fn, 3)
    samples = {k: [] for k in jobs}
    for _ in range(a.passes):
        for k, fn in jobs.items():
            if fn is not None:
                samples[k].append(timed(fn, a.iters))
    out = {"label": a.label, "batch": B, "patch": S, "meta_channels": cm, "passes": a.passes, "iters": a.iters}
    for k, v in samples.items():
        out[k] = sorted(v)[len(v) // 2] if v else None
        out[k + "_all"] = v
    print(json.dumps(out))


if __name__ == "__main__":
    main()
