"""CPU: the C-ABI library loads and exports every symbol include/crimac_unet_hip.h declares (no
compute calls without a GPU), and host-side logic of the drop-in surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import yaml

import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import build, hip, parallel, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(crimac_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    build.build()
    lib = ctypes.CDLL(build.LIB_PATH)
    syms = _declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in the header but not exported"
    # and the binding table covers the header exactly (plus version / last_error)
    assert set(hip.SIGNATURES) | {"crimac_version", "crimac_last_error", "crimac_wgrad_splits", "crimac_layer_desc_size",
                                  "crimac_wgrad_group_plan", "crimac_wgrad_group_layer_size"} == set(syms)
    # the split planner is a host-only query (no GPU): the level-0 shape fills one resident round
    lib2 = hip.load_library()
    assert lib2.crimac_wgrad_splits(0, 0, 64, 64, 32, 256, 256, 0) == 256        # bf16: one 8-wave workgroup per CU
    assert lib2.crimac_wgrad_splits(1, 0, 64, 64, 32, 256, 256, 0) == 512        # fp32 planes: two 4-wave workgroups
    assert lib2.crimac_wgrad_splits(0, 0, 1024, 1024, 32, 16, 16, 0) >= 1
    assert lib2.crimac_wgrad_splits(0, 2, 64, 64, 32, 256, 256, 0) < 0          # bad mode
    assert lib2.crimac_wgrad_splits(9, 0, 64, 64, 32, 256, 256, 0) < 0          # bad precision
    # ABI identity: the binding refuses a library of another version or with another descriptor layout
    header = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION
    assert lib2.crimac_version() == hip.ABI_VERSION
    assert lib2.crimac_layer_desc_size() == ctypes.sizeof(hip.LayerDesc)
    assert lib2.crimac_wgrad_group_layer_size() == ctypes.sizeof(hip.WgradGroupLayer)


def _header_text():
    return open(build.HEADER).read()


def test_binding_reads_these_prototypes_from_the_header():
    """Written out by hand from include/crimac_unet_hip.h: every scalar type of the parser's map, struct pointers, both
    return types, entry points with and without a stream."""
    i, l, f, d, vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
    u64 = ctypes.c_ulonglong
    protos, _, _ = hip.parse_header(_header_text())
    assert protos == hip.PROTOTYPES
    want = {
        "crimac_meta_planes": (i, [vp, i, i, i, i, d, vp, i, vp, i, vp, i, vp, vp], True),
        "crimac_augment_db_nhwc": (i, [i, vp, vp, i, vp, vp, vp, i, f, f, i, i, i, i, l, u64, i, i, i, vp], True),
        "crimac_gather_patches_memm_multi": (i, [i, vp, i, vp, i, vp, i, i, i, vp, l, vp], True),
        "crimac_wgrad_group_plan": (i, [i, vp, i, i, i, vp, i, vp], False),
        "crimac_version": (i, [], False),
        "crimac_last_error": (ctypes.c_char_p, [], False),
        "crimac_mfma_calibrate": (i, [i, i, vp, vp, vp], True),
        "crimac_labels_test_transform": (i, [vp, i, vp, i, f, f, vp, vp, i, i, vp, i, i, i, i, i, i, vp, i, i, i, i, vp], True),
        "crimac_labels_extend_mask": (i, [vp, vp, i, vp, vp, i, i, i, i, i, vp], True),
    }
    for name, proto in want.items():
        assert protos[name] == proto, name
    # the remaining scalar types of the map, on header text of the same form
    # (a pointer is a c_void_p whatever its base type: `short` is no scalar of the map, `short*` is a pointer like any other)
    text = 'extern "C" {\nint crimac_x(long long a, unsigned int b, const unsigned int* c, short* d, void* stream);\n}\n'
    assert hip.parse_header(text)[0] == {"crimac_x": (i, [ctypes.c_longlong, ctypes.c_uint, vp, vp, vp], True)}


def test_every_declared_function_is_bound_as_the_header_declares_it():
    lib = hip.load_library()
    assert sorted(hip.PROTOTYPES) == _declared_symbols() and len(hip.PROTOTYPES) >= 70
    for name, (restype, argtypes, takes_stream) in hip.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        assert takes_stream == (name in hip.SIGNATURES), name
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    with_stream = set(re.findall(r"\b(crimac_[a-z0-9_]+)\s*\([^()]*,\s*void\*\s*stream\s*\)", text))
    assert set(hip.SIGNATURES) == with_stream
    assert all(hip.SIGNATURES[name] is hip.PROTOTYPES[name][1] for name in with_stream)


@pytest.mark.parametrize("decl, named", [
    ("int crimac_bad(int a, short n, void* stream);", "crimac_bad"),                       # unknown scalar type
    ("int crimac_bad(int a, const float*, void* stream);", "crimac_bad"),                  # parameter without a name
    ("int crimac_bad(int, void* stream);", "crimac_bad"),
    ("int crimac_bad(float** rows, void* stream);", "crimac_bad"),
    ("typedef struct crimac_s { int a; short b; } crimac_s;", "crimac_s"),                 # struct field of an unknown type
    ("typedef struct crimac_s { const float* p, q; } crimac_s;", "crimac_s"),              # (q would not be a pointer)
    ("short crimac_bad(int a);", "crimac_bad"),                                            # unknown return type
    ("#define CRIMAC_BAD (CRIMAC_LATER | 1)\n#define CRIMAC_LATER 2", "CRIMAC_BAD"),       # not an earlier define
    ("#define CRIMAC_BAD sizeof(int)", "CRIMAC_BAD"),
    ("#define CRIMAC_BAD (2**31)", "CRIMAC_BAD"),                                          # Python's power, not C
])
def test_header_parser_refuses_what_it_does_not_recognise(decl, named):
    ok = 'extern "C" {\n%s\nint crimac_good(int a, void* stream);\n}\n'
    assert "crimac_good" in hip.parse_header(ok % "")[0]
    with pytest.raises(hip.HipLibraryError, match=named):
        hip.parse_header(ok % decl)


def test_header_parser_evaluates_defines_in_order_and_across_continued_lines():
    text = ('#define CRIMAC_A 3 /* three */\n#define CRIMAC_B (CRIMAC_A << 4)\n'
            '#define CRIMAC_C (1 | CRIMAC_B | \\\n                  (CRIMAC_A << 8))\n#define CRIMAC_D (-2147483647 - 1)\n'
            'extern "C" {\n}\n')
    assert hip.parse_header(text)[2] == {"CRIMAC_A": 3, "CRIMAC_B": 48, "CRIMAC_C": 1 | 48 | 768, "CRIMAC_D": -2 ** 31}
    assert hip.DEFINES["CRIMAC_PLANES_H3P"] == 2 | 16 | 32 | 64 | 128 | (8 << 8)          # the header's own continued line
    assert hip.ABI_VERSION == hip.DEFINES["CRIMAC_ABI_VERSION"] and hip.PR_BINS == hip.DEFINES["CRIMAC_PR_BINS"] == 16384
    from crimac_classifiers_unet_amd import pipeline, tiled_inference
    assert pipeline.SegPipe.PR_BINS == tiled_inference.PR_BINS == hip.PR_BINS


def test_struct_mirrors_have_the_fields_of_the_header():
    i, l, vp = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    structs = hip.parse_header(_header_text())[1]
    assert structs == {
        "crimac_layer_desc": [("w", vp), ("grad", vp), ("dw", vp), ("fwd_hi", vp), ("fwd_lo", vp), ("dg_hi", vp),
                              ("dg_lo", vp), ("kind", i), ("Co", i), ("Ci", i), ("Ci_pad", i), ("dw_splits", i),
                              ("dw_stride", l)],
        "crimac_wgrad_group_layer": [("f", vp), ("f_ld", l), ("CF", i), ("s", vp), ("s_ld", l), ("CS", i), ("Hf", i),
                                     ("Wf", i), ("dw", vp), ("tiles_y", i), ("tiles_x", i), ("ntiles", l),
                                     ("tiles_per_block", i), ("nsplits", i)],
        "crimac_memm_desc": [("data", vp), ("labels", vp), ("seabed", vp), ("out", vp), ("n_pings", ctypes.c_longlong),
                             ("n_range", ctypes.c_longlong)],
    }
    # several declarations on one line and comma lists keep their order
    one_line = 'extern "C" {\ntypedef struct crimac_t { const void* f; long f_ld; int CF, CS; float x; } crimac_t;\n}\n'
    assert hip.parse_header(one_line)[1] == {"crimac_t": [("f", vp), ("f_ld", l), ("CF", i), ("CS", i), ("x", ctypes.c_float)]}
    for cls, tag in ((hip.LayerDesc, "crimac_layer_desc"), (hip.WgradGroupLayer, "crimac_wgrad_group_layer"),
                     (hip.MemmDesc, "crimac_memm_desc")):
        assert cls._fields_ == structs[tag]
    lib = hip.load_library()
    assert ctypes.sizeof(hip.LayerDesc) == 88 == lib.crimac_layer_desc_size()
    assert ctypes.sizeof(hip.WgradGroupLayer) == 88 == lib.crimac_wgrad_group_layer_size()
    assert ctypes.sizeof(hip.MemmDesc) == 48 == 8 * hip.MEMM_DESC_WORDS


# hip name -> the #define it mirrors
MIRRORED = {
    "PREC_BF16": "CRIMAC_PREC_BF16", "PREC_F32X3": "CRIMAC_PREC_F32X3", "PREC_F32X6": "CRIMAC_PREC_F32X6",
    "PREC_FP16": "CRIMAC_PREC_FP16", "PREC_F32H3": "CRIMAC_PREC_F32H3", "PREC_H3P": "CRIMAC_PREC_H3P",
    "PREC_H3F_BWD": "CRIMAC_PREC_H3F_BWD",
    "PLANES_FP16": "CRIMAC_PLANES_FP16", "PLANES_F32H3": "CRIMAC_PLANES_F32H3", "PLANES_FWD_FRAG": "CRIMAC_PLANES_FWD_FRAG",
    "PLANES_INTERLEAVED": "CRIMAC_PLANES_INTERLEAVED", "PLANES_H3P": "CRIMAC_PLANES_H3P",
    "EPI_RELU": "CRIMAC_EPI_RELU", "EPI_OUT_PLANES": "CRIMAC_EPI_OUT_PLANES", "EPI_CIN4": "CRIMAC_EPI_CIN4",
    "EPI_WFRAG": "CRIMAC_EPI_WFRAG", "EPI_WROWS": "CRIMAC_EPI_WROWS",
    "LAYER_FWD_FRAG": "CRIMAC_LAYER_FWD_FRAG", "LAYER_DG_FRAG": "CRIMAC_LAYER_DG_FRAG",
    "NARROW_DGRAD": "CRIMAC_NARROW_DGRAD", "MASK_PER_PATCH": "CRIMAC_MASK_PER_PATCH",
    "WGRAD_GROUP_MAX_LAYERS": "CRIMAC_WGRAD_GROUP_MAX_LAYERS", "ABI_VERSION": "CRIMAC_ABI_VERSION", "PR_BINS": "CRIMAC_PR_BINS",
}
# defines of the four mirrored families that hip.py deliberately has no name for
UNMIRRORED = {
    "CRIMAC_EPI_STAT_RAW",         # no Python caller passes it
    "CRIMAC_PLANES_DG_SCALED",     # only ever part of CRIMAC_PLANES_H3P
    "CRIMAC_PLANES_FWD_FP16",      # the two _FP16 bits: only ever part of PLANES_FP16 / PLANES_F32H3 / PLANES_H3P
    "CRIMAC_PLANES_DG_FP16",
    "CRIMAC_PREC_MAX",             # the library's own range check
}


def test_every_mirrored_constant_equals_its_define():
    defines = hip.parse_header(_header_text())[2]
    assert len(defines) >= 34
    for name, define in MIRRORED.items():
        assert getattr(hip, name) == defines[define], name
    families = {d for d in defines if re.match(r"CRIMAC_(PREC|PLANES|EPI|LAYER)_", d)}
    assert families - set(MIRRORED.values()) == UNMIRRORED and not UNMIRRORED & set(MIRRORED.values())
    # kind bits 0-1 of crimac_layer_desc have no names in the header, only its comment
    assert (hip.LAYER_CONV3X3, hip.LAYER_UPCONV2X2, hip.LAYER_CONV1X1) == (0, 1, 2)


def test_call_refuses_a_name_that_takes_no_stream(monkeypatch):
    def unreachable():
        raise AssertionError("hip.call reached the library")
    monkeypatch.setattr(hip, "load_library", unreachable)
    monkeypatch.setattr(hip, "_stream", unreachable)
    with pytest.raises(hip.HipLibraryError, match="crimac_wgrad_splits"):
        hip.call("crimac_wgrad_splits", 0, 0, 64, 64, 32, 256, 256, 0)
    with pytest.raises(hip.HipLibraryError, match="crimac_nonexistent"):
        hip.call("crimac_nonexistent")
    # ... and what `call` launches is the function load_library bound, for exactly the entry points that take a stream
    monkeypatch.undo()
    lib = hip.load_library()
    assert set(hip._entry) == set(hip.SIGNATURES) and all(hip._entry[n] is getattr(lib, n) for n in hip.SIGNATURES)


def test_grouped_weight_gradient_plan_covers_every_item_exactly_once():
    """crimac_wgrad_group_plan (host only): for the encoder shapes of the benchmark and for ragged tiny shapes, every
    (layer, channel-tile pair, pixel split) appears in exactly one of the 8 queues; whole rounds of 8 splits put split s
    in queue s % 8 (the XCD that keeps its pixel range in L2); longest items come first."""
    lib = hip.load_library()
    cases = [(32, [(64, 64, 256, 256), (128, 64, 128, 128), (128, 128, 128, 128), (256, 128, 64, 64), (1024, 512, 16, 16)]),
             (2, [(64, 64, 32, 48), (128, 128, 16, 24), (512, 256, 4, 6)]), (1, [(64, 128, 8, 16)])]
    for B, shapes in cases:
        arr = (hip.WgradGroupLayer * len(shapes))()
        for d, (cf, cs, h, w) in zip(arr, shapes):
            d.CF, d.CS, d.f_ld, d.s_ld, d.Hf, d.Wf = cf, cs, cf, cs, h, w
        counts = (ctypes.c_int * 8)()
        cap = lib.crimac_wgrad_group_plan(0, arr, len(shapes), B, 0, None, 0, counts)
        assert cap > 0 and max(counts) == cap
        items = (ctypes.c_int * (8 * cap * 2))()
        assert lib.crimac_wgrad_group_plan(0, arr, len(shapes), B, 0, items, cap, counts) == cap
        seen = set()
        for x in range(8):
            last_cost = None
            for k in range(counts[x]):
                li, qs = items[2 * (x * cap + k)], items[2 * (x * cap + k) + 1]
                qt, sp = qs >> 16, qs & 0xFFFF
                d = arr[li]
                assert 0 <= sp < d.nsplits and 0 <= qt < ((d.CF + 63) // 64) * ((d.CS + 63) // 64)
                if d.nsplits % 8 == 0:
                    assert sp % 8 == x
                assert (li, qt, sp) not in seen
                seen.add((li, qt, sp))
                assert last_cost is None or d.tiles_per_block <= last_cost
                last_cost = d.tiles_per_block
        total = sum(d.nsplits * ((d.CF + 63) // 64) * ((d.CS + 63) // 64) for d in arr)
        assert len(seen) == total == sum(counts)
        for d in arr:
            assert d.ntiles == B * d.tiles_y * d.tiles_x and d.tiles_per_block * d.nsplits >= d.ntiles
            assert d.tiles_per_block * (d.nsplits - 1) < d.ntiles          # no empty split
    # the first layer (4 channels padded to 16) is refused: it keeps its own launch
    arr = (hip.WgradGroupLayer * 1)()
    arr[0].CF, arr[0].CS, arr[0].f_ld, arr[0].s_ld, arr[0].Hf, arr[0].Wf = 64, 16, 64, 16, 64, 64
    assert lib.crimac_wgrad_group_plan(0, arr, 1, 2, 0, None, 0, (ctypes.c_int * 8)()) < 0


def test_binding_refuses_a_library_with_another_abi_version(monkeypatch):
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "ABI_VERSION", hip.ABI_VERSION + 1)
    with pytest.raises(hip.HipLibraryError, match="ABI version"):
        hip.load_library()


def test_argument_validation_runs_without_gpu():
    """Argument checks precede any HIP call, so they are testable on the CPU box."""
    lib = hip.load_library()
    rc = lib.crimac_conv3x3(0, None, 64, 1, 8, 8, 24, 64, None, None, None, None, 64, 0, 0, None, None, 1,
                            None, 0, None, 0, None)
    assert rc < 0 and b"Cin" in lib.crimac_last_error()
    rc = lib.crimac_sgd_momentum(None, None, None, 0, 0.1, 0.9, 1.0, 0, None)
    assert rc < 0


def test_module_surface_matches_reference_layout():
    m = pkg.UNet_Baseline(n_classes=3, in_channels=4)
    sd = m.state_dict()
    shapes = synth.unet_state_shapes()
    assert list(sd.keys()) == list(shapes.keys())
    assert all(tuple(sd[k].shape) == shapes[k] for k in sd)
    assert sum(p.numel() for p in m.parameters()) == 31044227
    m.load_state_dict(synth.synth_state_dict())          # reference-style checkpoint loads
    with pytest.raises(ValueError):
        pkg.UNet_Baseline(3, 4, up_mode="bogus")
    with pytest.raises(ValueError):
        pkg.UNet_Baseline(3, 4, merge_mode="bogus")
    with pytest.raises(NotImplementedError):
        pkg.UNet_Baseline(3, 4, merge_mode="add")


def test_same_seed_gives_reference_style_init():
    torch.manual_seed(10)
    a = pkg.UNet_Baseline(3, 4).state_dict()
    torch.manual_seed(10)
    b = pkg.UNet_Baseline(3, 4).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    w = a["down_convs.1.main.0.weight"]
    assert abs(float(w.abs().max()) - 1 / (64 * 9) ** 0.5) < 1e-3


def test_segpipe_accepts_the_reference_yaml_keys():
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg["save_model_params"] = False
    pipe = pkg.SegPipeUNet(experiment_name="cpu", **cfg)
    assert pipe.frequencies == [18, 38, 120, 200] and pipe.window_size == [256, 256]
    assert pipe.model.in_channels == 4 and pipe.model_name == "cpu"
    crit = pipe.get_criterion()
    assert crit.weight.tolist() == [10.0, 300.0, 250.0]
    lab = torch.tensor([-100, -70, -50, -30, -10, 0, 1, 2])
    assert pipe.set_label_ignore_val(lab.clone()).tolist() == [-100, -100, 0, -100, -100, 0, 1, 2]
    with pytest.raises(AssertionError):
        pkg.SegPipeUNet(checkpoint_dir=None, experiment_name="x", **{**cfg, "save_model_params": True})
    with pytest.raises(ValueError):
        pkg.SegPipeUNet(experiment_name="x", **{**cfg, "loss_type": "Focal"}).get_criterion()
    assert pkg.get_in_channels([]) == 0
    assert pkg.get_in_channels({"portion_year": True, "portion_day": True, "depth_rel": False,
                                "depth_abs_surface": True, "depth_abs_seabed": False,
                                "time_diff": False}) == 4


def test_cpu_forward_fails_loudly_not_silently():
    m = pkg.UNet_Baseline(3, 4)
    with pytest.raises(Exception, match="no CPU fallback"):
        m(torch.zeros(1, 4, 32, 32))
    with pytest.raises(hip.HipLibraryError):
        hip.ptr(torch.zeros(3))


def test_metric_helpers_f1():
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(pkg.__file__), "configs", "pipeline_config.yaml")))
    cfg["save_model_params"] = False
    pipe = pkg.SegPipeUNet(experiment_name="cpu", **cfg)
    labels = np.array([1, 1, 0, 0, 2, -100], dtype=np.int8)
    preds = np.array([0.9, 0.8, 0.1, 0.7, 0.2, 0.99], dtype=np.float16)
    l, p = pipe.select_valid_predictions(labels.copy(), preds)
    assert len(l) == 5
    m = pipe.compute_evaluation_metrics(l, p)
    assert abs(m["F1"].max() - 1.0) < 1e-6      # threshold 0.8 separates both sandeel pixels


def test_bucket_and_shard_plans():
    assert parallel.bucket_bounds(10, 4) == [(0, 4), (4, 8), (8, 10)]
    assert parallel.shard_indices(10, 1, 4) == [1, 5, 9]
    allidx = sorted(i for r in range(8) for i in parallel.shard_indices(95, r, 8))
    assert allidx == list(range(95))             # 95 patches of one 4096-ping chunk


def test_pr_report_csv_has_the_reference_dataframe_layout(tmp_path):
    """validate_model_testing's csv (reference pipeline.py:358-361 writes DataFrame(metrics).to_csv): index column,
    precision / recall / thresholds / F1, NaN threshold in the last row."""
    import csv
    import numpy as np
    from crimac_classifiers_unet_amd.pipeline import SegPipe, write_pr_csv
    hp = np.zeros(16384, dtype=np.int64)
    hn = np.zeros(16384, dtype=np.int64)
    bits = lambda v: int(np.float16(v).view(np.uint16))
    hp[bits(0.9)], hp[bits(0.6)], hn[bits(0.7)], hn[bits(0.1)] = 3, 1, 2, 10
    m = SegPipe.compute_evaluation_metrics_from_histograms(hp, hn)
    # same numbers as sklearn on the expanded vectors
    from sklearn.metrics import precision_recall_curve
    y = np.r_[np.ones(4), np.zeros(12)]
    sc = np.r_[[0.9] * 3, [0.6], [0.7] * 2, [0.1] * 10].astype(np.float16)
    p, r, t = precision_recall_curve(y, sc, pos_label=1)
    assert np.allclose(m["precision"], p) and np.allclose(m["recall"], r) and np.allclose(m["thresholds"], t)
    m["thresholds"] = np.append(m["thresholds"], np.nan)
    write_pr_csv(m, tmp_path / "pr.csv")
    rows = list(csv.reader(open(tmp_path / "pr.csv")))
    assert rows[0] == ["", "precision", "recall", "thresholds", "F1"]
    assert len(rows) == len(p) + 1 and rows[-1][3] == "" and rows[1][0] == "0"
    assert abs(float(rows[1][1]) - p[0]) < 1e-15


def test_evaluate_flow_needs_the_reference_data_stack_or_injected_factories():
    import inspect
    from crimac_classifiers_unet_amd import evaluate
    with pytest.raises(ImportError, match="dataset_cls"):
        evaluate.validate_model_survey_memm([], None, [], [256, 256], 20, "all", 4, 0, "/tmp", "/tmp")
    with pytest.raises(ImportError, match="label_transform_factory"):
        evaluate.validate_model_survey_zarr([1], None, [], [256, 256], 20, "all", 4, 0, "/tmp", "/tmp",
                                            dataset_cls=object, data_transform_factory=lambda m: None)
    # the product module never imports the reference package by itself: only from a path the caller names
    src = inspect.getsource(evaluate)
    assert "from batch" not in src and "import batch" not in src
    with pytest.raises(ImportError, match="host data stack"):
        evaluate.data_stack_factories("/nonexistent/path", memm=True)


def test_spawned_ranks_time_out_and_are_reaped():
    import sys
    from crimac_classifiers_unet_amd import launch
    rc, _ = launch.spawn_ranks([sys.executable, "-c", "import time; time.sleep(60)"], 2, timeout=2)
    assert rc != 0


def test_planes_argument_layout_matches_the_header():
    text = open(os.path.join(ROOT, "include", "crimac_unet_hip.h")).read()
    assert "#define CRIMAC_PLANES_FWD_FP16 16" in text and "#define CRIMAC_PLANES_DG_FP16 32" in text
    assert "#define CRIMAC_F32H3_WSHIFT 8" in text
    assert hip.PLANES_FP16 == 1 | 16 | 32 and hip.PLANES_F32H3 == 2 | 16 | (8 << 8)
    # ('h3f' is an engine mode: forward launches carry H3P, the backward pass's contractions CRIMAC_PREC_H3F_BWD)
    assert hip.PREC_NAMES == {"bf16": 0, "f32x3": 1, "f32x6": 2, "fp16": 3, "f32h3": 4, "h3p": 5, "h3f": 5}
    assert "#define CRIMAC_PREC_H3F_BWD 6" in text and hip.PREC_H3F_BWD == 6
    assert hip.PREC_BACKWARD[hip.PREC_F32H3] == hip.PREC_F32X3
    lib = hip.load_library()
    # argument checks of the packers run without a GPU: a plane count of 0 or stray bits are refused
    assert lib.crimac_pack_layers(None, 1, 1, None) < 0
    import ctypes
    d = (hip.LayerDesc * 1)()
    assert lib.crimac_pack_layers(ctypes.byref(d), 1, 0, None) < 0
    assert lib.crimac_pack_layers(ctypes.byref(d), 1, 2 | 64, None) < 0


class _F64Crops(torch.utils.data.Dataset):
    """What the reference's zarr Dataset hands over (batch/dataset.py:361): float64 data, int16 labels, int64 centres."""

    def __len__(self):
        return 12

    def __getitem__(self, i):
        rng = np.random.default_rng(i)
        return {"data": np.power(10.0, rng.uniform(-9, -1, (4, 16, 16))), "labels": rng.integers(-1, 3, (16, 16)).astype(np.int16),
                "center_coordinates": np.array([i, 2 * i], dtype=np.int64)}


@pytest.mark.parametrize("workers", [0, 2])
def test_collate_float32_gives_the_values_of_the_reference_cast(workers):
    """`collate_float32` (yaml key of the same name; staging.py): the training DataLoader's float64 crops are cast per sample in
    the collate -- the batch equals `default_collate(...)['data'].float()` (pipeline.py:163) bit for bit, the other keys are
    untouched, a DataLoader with a collate function of its own is left alone, and the early page release still recognises
    the batches as worker-collated."""
    from torch.utils.data import DataLoader, default_collate
    from crimac_classifiers_unet_amd import staging
    ds = _F64Crops()
    ref = list(DataLoader(ds, batch_size=4, shuffle=False, num_workers=0))
    dl = DataLoader(ds, batch_size=4, shuffle=False, num_workers=workers)
    assert staging.use_collate_float32(dl) and dl.collate_fn is staging.collate_float32
    assert staging.collated_in_worker(dl) == (workers > 0)
    got = list(dl)
    assert len(got) == len(ref) == 3
    for g, r in zip(got, ref):
        assert r["data"].dtype == torch.float64 and g["data"].dtype == torch.float32
        assert torch.equal(g["data"], r["data"].float())
        assert g["labels"].dtype == torch.int16 and torch.equal(g["labels"], r["labels"])
        assert torch.equal(g["center_coordinates"], r["center_coordinates"])
    own = DataLoader(ds, batch_size=4, collate_fn=lambda s: default_collate(s))
    assert not staging.use_collate_float32(own)
    assert not staging.use_collate_float32(DataLoader(ds, batch_size=None))           # no automatic batching: nothing to collate
    # samples that are not dicts, and float32 data, pass through default_collate unchanged
    t = staging.collate_float32([np.ones(3), np.zeros(3)])
    assert t.dtype == torch.float64 and t.shape == (2, 3)
    f = staging.collate_float32([{"data": np.ones((2, 2), np.float32)}, {"data": np.zeros((2, 2), np.float32)}])
    assert f["data"].dtype == torch.float32


def test_environment_switches_are_the_ones_integration_md_lists():
    """Every CRIMAC_* variable the C library (getenv) or the package (os.environ) reads is a row of the table "Environment
    switches that exist" in INTEGRATION.md, and every row of that table is still read somewhere: a switch can neither be
    added without being documented nor stay documented after it is gone."""
    import glob
    read = set()
    for path in glob.glob(os.path.join(ROOT, "crimac_classifiers_unet_amd", "csrc", "*")):
        read |= set(re.findall(r"getenv\(\s*\"(CRIMAC_[A-Z0-9_]+)\"", open(path).read()))
    for path in glob.glob(os.path.join(ROOT, "crimac_classifiers_unet_amd", "**", "*.py"), recursive=True):
        read |= set(re.findall(r"os\.environ(?:\.get\(|\[)\s*\"(CRIMAC_[A-Z0-9_]+)\"", open(path).read()))
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text.split("### Environment switches that exist", 1)[1]
    table = next(par for par in section.split("\n\n") if par.startswith("|"))
    rows = table.splitlines()
    listed = set(re.findall(r"^\|\s*`(CRIMAC_[A-Z0-9_]+)`", "\n".join(rows), flags=re.M))
    assert len(rows) == len(listed) + 2, "one name per row below the two header lines"
    assert read == listed, f"read but not listed: {sorted(read - listed)}; listed but not read: {sorted(listed - read)}"
