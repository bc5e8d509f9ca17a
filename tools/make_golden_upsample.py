#!/usr/bin/env python3
"""Generate tests/golden/upsample.npz: the reference U-Net with up_mode="upsample" (Upsample(bilinear, x2) + conv1x1 in
every decoder stage, crimac_unet/models/unet.py:47-56), run by the *imported reference* on the CPU.

Runs only where the reference can be imported (never on the GPU box).  Outputs only: weights and inputs are regenerated
from seeds by ``crimac_classifiers_unet_amd.synth``.  Contents:
  keys / shapes of the state_dict; the seeded-init fingerprint (torch seed 10: per-tensor sum and first 8 values);
  B = 2, 128 x 128: eval logits, train-mode logits, loss, BatchNorm running statistics after one train forward, the
  losses of three SGD steps; gradients: norms and fp32-vs-fp64 noise of every tensor (gnoise, as tools/make_golden.py),
  full tensors of conv_final and of the small upconv.1 layers, a fixed index sample of the large ones.

Usage: python tools/make_golden_upsample.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "/root/reference/crimac_unet"
sys.path.insert(0, REF)

from crimac_classifiers_unet_amd import synth  # noqa: E402

import models.unet as ref_models  # noqa: E402  (the reference)

OUT = os.path.join(ROOT, "tests", "golden", "upsample.npz")
HW, B = 128, 2
FULL_MAX = 8192            # gradients up to this many elements are stored whole
N_SAMPLE = 512             # fixed index sample of the larger ones
CLASS_W = [10.0, 300.0, 250.0]


def sample_index(n):
    return np.random.Generator(np.random.PCG64(n)).choice(n, size=min(N_SAMPLE, n), replace=False).astype(np.int64)


def main():
    torch.set_num_threads(8)
    fix = {}
    # seeded default initialisation (what UNet_Baseline(..., up_mode="upsample") must reproduce)
    torch.manual_seed(10)
    init = ref_models.UNet_Baseline(n_classes=3, in_channels=4, up_mode="upsample").state_dict()
    fix["keys"] = np.array(list(init.keys()))
    for k, v in init.items():
        fix["shape/" + k] = np.array(v.shape, dtype=np.int64)
        fix["init_sum/" + k] = np.float64(v.double().sum())
        fix["init_head/" + k] = v.reshape(-1)[:8].double().numpy()

    sd = synth.synth_state_dict(seed=0, up_mode="upsample")
    x = torch.from_numpy(synth.synth_echogram_batch(B, 4, HW, HW, seed=1))
    lab = torch.from_numpy(synth.synth_labels(B, HW, HW, seed=2)).long()
    net = ref_models.UNet_Baseline(n_classes=3, in_channels=4, up_mode="upsample")
    net.load_state_dict(sd)
    net.eval()
    with torch.no_grad():
        fix["logits_eval"] = net(x).numpy()

    net.train()
    crit = torch.nn.CrossEntropyLoss(weight=torch.tensor(CLASS_W))
    opt = torch.optim.SGD(net.parameters(), lr=0.005, momentum=0.95)
    losses, grads = [], None
    for it in range(3):
        opt.zero_grad()
        out = net(x)
        loss = crit(out, lab)
        loss.backward()
        if it == 0:
            fix["logits_train"] = out.detach().numpy()
            grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
            for k, v in net.state_dict().items():
                if "running" in k:
                    fix["stat1/" + k] = v.numpy().copy()
        opt.step()
        losses.append(float(loss))
    fix["losses"] = np.asarray(losses, dtype=np.float64)

    net64 = ref_models.UNet_Baseline(n_classes=3, in_channels=4, up_mode="upsample").double()
    net64.load_state_dict(sd)
    net64.train()
    crit64 = torch.nn.CrossEntropyLoss(weight=torch.tensor(CLASS_W, dtype=torch.float64))
    loss64 = crit64(net64(x.double()), lab)
    loss64.backward()
    fix["loss64"] = np.float64(loss64.detach())
    for k, g in grads.items():
        g64 = dict(net64.named_parameters())[k].grad.detach()
        fix["gnorm/" + k] = np.float64(g.double().norm())
        fix["gnoise/" + k] = np.float64((g.double() - g64).norm() / g64.norm().clamp_min(1e-300))
        if "upconv.1." in k or k.startswith("conv_final."):
            flat = g.reshape(-1).numpy()
            if flat.size <= FULL_MAX:
                fix["grad/" + k] = g.numpy()
            else:
                idx = sample_index(flat.size)
                fix["gidx/" + k] = idx
                fix["gval/" + k] = flat[idx]
    np.savez_compressed(OUT, **fix)
    print(OUT, os.path.getsize(OUT), "bytes; losses", losses, "loss64", float(loss64))


if __name__ == "__main__":
    main()
