#!/usr/bin/env python3
"""Launch trace of two training steps and one eval forward with softmax: every entry-point call (name, arguments, stream)
and every event record / stream wait between them, with pointers, streams and events numbered by first appearance.
Run it at two commits and diff the outputs: an engine change that keeps the launch order leaves them byte-identical.
usage: launch_trace.py [--precision P] [--start-filts N] [--up-mode M] [--lmi] [--shape B H W] [--wgrad-streams N]
                       [--set ATTR=VALUE ...]     (--set: engine attributes, e.g. fold_bn_finalize=False)"""
import argparse, ast, ctypes, os, re, sys
ap = argparse.ArgumentParser()
ap.add_argument("--precision", default="bf16")
ap.add_argument("--start-filts", type=int, default=64)
ap.add_argument("--up-mode", default="transpose")
ap.add_argument("--lmi", action="store_true", help="UNet_LateMetInject (7 metadata planes)")
ap.add_argument("--shape", type=int, nargs=3, default=(1, 64, 64), metavar=("B", "H", "W"))
ap.add_argument("--wgrad-streams", type=int, default=1)
ap.add_argument("--set", nargs="*", default=[], metavar="ATTR=VALUE")
a = ap.parse_args()
os.environ["CRIMAC_WGRAD_STREAM"] = str(a.wgrad_streams)      # (read when engine.py is imported)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import engine, hip, synth

trace, names, keep, depth = [], {}, [], [0]


def num(kind, key, obj=None):
    keep.append(obj)              # (an id() or a host address must not come back as a later object's)
    return names.setdefault((kind, key), f"{kind}{sum(k[0] == kind for k in names)}")


def norm(v):
    if isinstance(v, ctypes.c_void_p):
        return num("p", v.value)
    if isinstance(v, (ctypes.Array, ctypes.Structure)):
        return num("p", ctypes.addressof(v), v)
    if type(v).__name__ == "CArgObject":          # byref(array, offset): only its repr tells the address
        return num("p", int(re.search(r"0x[0-9a-f]+", repr(v)).group(), 16), v)
    return repr(v)


def stream(s=None):
    return num("s", (s or torch.cuda.current_stream()).cuda_stream)


def call(name, *args, flops=None, mfmas=1, _real=hip.call):
    trace.append(f"{name}({', '.join(map(norm, args))}, flops={flops!r}, mfmas={mfmas!r}) {stream()}")
    _real(name, *args, flops=flops, mfmas=mfmas)


def wrap(cls, meth, line):
    real = getattr(cls, meth)

    def traced(self, *args):
        if not depth[0]:                          # (Stream.wait_stream is a record + wait_event inside torch: one line)
            trace.append(line(self, *args))
        depth[0] += 1
        try:
            return real(self, *args)
        finally:
            depth[0] -= 1
    setattr(cls, meth, traced)


hip.call = engine.call = call                     # (engine.py imports `call` by name)
wrap(torch.cuda.Event, "record", lambda e, s=None: f"record {num('e', id(e), e)} {stream(s)}")
wrap(torch.cuda.Stream, "wait_event", lambda s, e: f"wait_event {num('e', id(e), e)} {stream(s)}")
wrap(torch.cuda.Stream, "wait_stream", lambda s, o: f"wait_stream {stream(o)} {stream(s)}")

B, H, W = a.shape
nm = 7 if a.lmi else 0
kw = dict(start_filts=a.start_filts, up_mode=a.up_mode, precision=a.precision)
m = pkg.UNet_LateMetInject(3, 4, nm, **kw) if a.lmi else pkg.UNet_Baseline(3, 4, **kw)
m.load_state_dict(synth.synth_state_dict(start_filts=a.start_filts, seed=0, meta_in_channels=nm, up_mode=a.up_mode))
eng = m.cuda().engine
for kv in a.set:
    setattr(eng, kv.split("=")[0], ast.literal_eval(kv.split("=", 1)[1]))
x = torch.from_numpy(synth.synth_echogram_batch(B, 4, H, W, seed=1)).cuda()
lab = torch.from_numpy(synth.synth_labels(B, H, W, seed=2)).cuda()
meta = torch.from_numpy(synth.synth_metadata(B, nm, H, W, seed=3)).cuda() if a.lmi else None
cw = torch.tensor([10.0, 300.0, 250.0], device="cuda")
for what in ("train_step 1", "train_step 2", "eval forward, softmax"):
    trace.append(f"# {what}")
    if what.startswith("train"):
        eng.train_step(x, lab, cw, 0.005, 0.95, meta=meta)
    else:
        eng.forward(x, training=False, softmax=True, meta=meta)
torch.cuda.synchronize()
print("\n".join(trace))
