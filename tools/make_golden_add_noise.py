#!/usr/bin/env python3
"""Golden vectors for tests/test_augment.py::test_reference_add_noise_has_the_same_distribution: the REFERENCE's
add_noise (batch/data_augmentation/add_noise.py) called 200 times on constant 4 x 32 x 32 crops (value 1e-3) with
numpy's global generator seeded once (3); stored are the factors out / 1e-3 of every call.

Usage: python tools/make_golden_add_noise.py <reference crimac_unet directory>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, SHAPE, VALUE, SEED = 200, (4, 32, 32), 1e-3, 3


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from batch.data_augmentation.add_noise import add_noise
    np.random.seed(SEED)
    ratios = np.empty((CALLS,) + SHAPE, dtype=np.float64)
    for i in range(CALLS):
        out, _, _ = add_noise(np.full(SHAPE, VALUE), None, None)
        ratios[i] = out / VALUE
    path = os.path.join(ROOT, "tests", "golden", "add_noise.npz")
    np.savez_compressed(path, ratios=ratios, seed=SEED, value=VALUE)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
