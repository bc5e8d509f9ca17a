"""eval_mode 'region' / 'trace' with metadata models on the tiled path, the parts that need no GPU: the new gather entry
point in header, binding and library, and the refusals of ``ChunkPredictor.evaluate`` that come before any GPU work."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd import tiled_inference as ti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "crimac_gather_patches_memm_labels"


def test_entry_point_is_declared_bound_and_exported_with_matching_arguments():
    header = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION >= 12
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double}

    def argtypes(name):
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert proto, f"{name} is not declared in the header"
        args = [a.strip() for a in proto.group(1).split(",")]
        assert args[-1] == "void* stream"
        return [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args], args
    want, args = argtypes(NAME)
    assert want == hip.SIGNATURES[NAME] and len(want) == 23
    # everything crimac_gather_patches_memm_meta takes, with the per-patch labels in the place of the chunk's raw ids
    meta_types, meta_args = argtypes("crimac_gather_patches_memm_meta")
    assert want == meta_types
    assert [a for a in args if a not in meta_args] == ["const short* patch_labels"]
    # argument checks precede any HIP call: refused without a GPU, with the error text of the library
    lib = hip.load_library()
    assert lib.crimac_version() == hip.ABI_VERSION
    fn = getattr(lib, NAME)
    one = ctypes.c_void_p(16)                         # (never dereferenced)
    ok = dict(prec=0, C=4, ld=16, labels=one, flags=0, vec=None, n=0, cen=None)

    def rc(**over):
        a = dict(ok, **over)
        return fn(a["prec"], one, a["C"], 10, 10, one, 1, 32, 32, one, a["ld"], a["labels"], 1, a["flags"], 0.5, a["vec"],
                  a["n"], a["vec"], a["n"], a["vec"], a["n"], a["cen"], None)
    assert rc(labels=None) < 0 and b"transformed labels" in lib.crimac_last_error()
    assert rc(flags=64) < 0 and rc(flags=-1) < 0 and b"flags" in lib.crimac_last_error()
    assert rc(flags=1) < 0 and b"centres" in lib.crimac_last_error()              # planes without meta_centres
    assert rc(flags=2, cen=one) < 0 and b"portion_day" in lib.crimac_last_error()
    assert rc(flags=4, cen=one) < 0 and b"time_diff" in lib.crimac_last_error()
    assert rc(flags=32, cen=one) < 0 and b"seabed" in lib.crimac_last_error()
    assert rc(prec=9) < 0 and b"precision" in lib.crimac_last_error()
    assert rc(C=17) < 0
    assert rc(C=12, flags=63, vec=one, n=5, cen=one) < 0 and b"do not fit" in lib.crimac_last_error()
    assert rc(ld=12) < 0


def predictor(lmi=False, in_channels=4, flavour="memm", wide=True, labels=True):
    eng = types.SimpleNamespace(lmi=lmi, in_channels=in_channels, device=torch.device("cpu"), bind=lambda: None)
    cp = ti.ChunkPredictor(types.SimpleNamespace(infer_engine=eng), 48, (16, 16), 2, 4)
    cp.data = torch.zeros(4, 40, 48)
    cp.labels = torch.zeros(40, 48, dtype=torch.int16) if labels else None
    cp.wide, cp.flavour = wide, flavour
    return cp


@pytest.mark.parametrize("model", [dict(), dict(lmi=True), dict(in_channels=11)])
def test_evaluate_keeps_its_argument_checks_for_every_model_kind(model):
    grid, boxes = np.array([[24, 20]]), torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="wide=True"):
        predictor(wide=False, **model).evaluate(grid, None, "region", boxes)
    cp = predictor(**model)
    with pytest.raises(ValueError, match="'all', 'region' or 'trace'"):
        cp.evaluate(grid, None, "box", boxes)
    for mode in ("region", "trace"):
        with pytest.raises(ValueError, match=f"eval_mode='{mode}' goes with boxes given"):
            cp.evaluate(grid, None, mode, None)
    with pytest.raises(ValueError, match="eval_mode='all' goes with boxes None"):
        cp.evaluate(grid, None, "all", boxes)
    with pytest.raises(ValueError, match="annotation ids"):
        predictor(labels=False, **model).evaluate(grid, None, "region", boxes)
    cp.labels = torch.zeros(39, 48, dtype=torch.int16)
    with pytest.raises(ValueError, match="do not cover the data extent"):
        cp.evaluate(grid, None, "region", boxes)


@pytest.mark.parametrize("model", [dict(lmi=True), dict(in_channels=11)])
@pytest.mark.parametrize("mode", ["all", "region"])
def test_a_zarr_chunk_with_metadata_still_raises(model, mode):
    cp = predictor(flavour="zarr", **model)
    cp.meta_source = types.SimpleNamespace(n_planes=7)
    boxes = None if mode == "all" else torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="memm flavour only"):
        cp.evaluate(np.array([[24, 20]]), None, mode, boxes)
    # a memm chunk without its metadata source is told what is missing, as before
    cp = predictor(**model)
    with pytest.raises(ValueError, match="meta_source"):
        cp.evaluate(np.array([[24, 20]]), None, mode, boxes)


def test_the_refusal_of_region_and_trace_with_metadata_is_gone():
    src = open(os.path.join(ROOT, "crimac_classifiers_unet_amd", "tiled_inference.py")).read()
    assert "with metadata planes on the tiled path" not in src
