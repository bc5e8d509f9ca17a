"""GPU: what the shared launchers of the tiling / label kernel families could silently lose -- every entry point's own
refusals (worded with its own name, made on the host before any launch), and the descriptor branch of the gather and
eval-crop kernels at its edge: a patch whose src names no descriptor is left untouched, its neighbours equal the scalar
branch bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd.hip import call, ptr

pytestmark = pytest.mark.gpu

DEV = "cuda"
C, PH, PW = 4, 16, 16
STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32x6": torch.float32, "h3p": torch.float32}
GATHERS = ("crimac_gather_patches", "crimac_gather_patches_memm", "crimac_gather_patches_memm_meta",
           "crimac_gather_patches_memm_labels", "crimac_gather_patches_memm_multi",
           "crimac_gather_patches_memm_labels_multi")


def refusal_cases(buf):
    """[(entry point, what is wrong, arguments without the stream)]: the valid call of every entry point -- real buffers
    ``buf(name)`` of one 16 x 16 patch -- with ONE argument changed."""
    f = ctypes.c_float
    data, lab, cen, cen64, out = buf("data"), buf("lab"), buf("cen"), buf("cen64"), buf("out")
    descs, src, plab, crop, boxes, off, vec = (buf("descs"), buf("src"), buf("plab"), buf("crop"), buf("boxes"), buf("off"),
                                               buf("vec"))
    meta = dict(db_scaled=1, flags=1, year=0.5, day=None, n_day=0, td=None, n_td=0, sb=None, n_sb=0, meta_cen=cen)
    one = dict(prec=0, data=data, C=C, Wd=16, H=16, cen=cen, P=1, ph=PH, pw=PW, out=out, ld=16)
    multi = dict(prec=0, descs=descs, n_desc=2, src=src, C=C, cen=cen, P=1, ph=PH, pw=PW, out=out, ld=16)
    chain = dict(labels_in=lab, label_bytes=2, data=crop, thr_channel=C - 1, lo=f(1e-7), hi=f(1e-4), cen=cen64)
    valid = {
        "crimac_gather_patches": one,
        "crimac_gather_patches_memm": dict(one, border=lab),
        "crimac_gather_patches_memm_meta": dict(one, border=lab, **meta),
        "crimac_gather_patches_memm_labels": dict(one, plab=plab, **dict(meta, flags=0, meta_cen=None)),
        "crimac_gather_patches_memm_multi": multi,
        "crimac_gather_patches_memm_labels_multi": dict(multi, plab=plab),
        "crimac_gather_eval_crops": dict(data=data, C=C, Wd=16, H=16, labels=lab, cen=cen, P=1, ph=PH, pw=PW, flavour=1,
                                         data_out=crop, labels_out=plab),
        "crimac_gather_eval_crops_multi": dict(descs=descs, n_desc=2, src=src, C=C, cen=cen, P=1, ph=PH, pw=PW,
                                               data_out=crop, labels_out=plab),
        "crimac_labels_test_transform": dict(chain, seabed=vec, ping0=0, pings=16, mask=None, mask_ping0=0, mask_pings=0,
                                             n_range=16, pad=10, rule=1, overlap=2, labels_out=plab, P=1, C=C, H=PH, W=PW),
        "crimac_labels_test_transform_multi": dict(chain, descs=descs, n_desc=2, src=src, pad=10, overlap=2,
                                                   labels_out=plab, P=1, C=C, H=PH, W=PW),
        "crimac_labels_extend_mask": dict(labels=plab, data=crop, C=C, cen=cen64, boxes=boxes, n_boxes=1, ignore=-1, P=1,
                                          H=PH, W=PW),
        "crimac_labels_extend_mask_multi": dict(labels=plab, data=crop, C=C, cen=cen64, boxes=boxes, off=off, n_desc=2,
                                                src=src, ignore=-1, P=1, H=PH, W=PW),
    }
    wrong = {name: [("P = 0", dict(P=0))] for name in valid}                       # the common rule
    for name in GATHERS:
        wrong[name] += [("prec above the range", dict(prec=7)), ("prec below the range", dict(prec=-1)),
                        ("ld = 12", dict(ld=12)), ("P = 65536", dict(P=65536))]
    for name in valid:
        if name.endswith("_multi") and "extend" not in name:
            wrong[name].append(("NULL descs", dict(descs=None)))
    for name in ("crimac_gather_eval_crops", "crimac_gather_eval_crops_multi"):
        wrong[name].append(("P = 65536", dict(P=65536)))
    for name in ("crimac_gather_patches_memm", "crimac_gather_patches_memm_meta"):
        wrong[name].append(("NULL border_labels", dict(border=None)))
    wrong["crimac_gather_patches_memm_meta"].append(("flags = 0", dict(flags=0)))
    wrong["crimac_gather_patches_memm_labels"].append(("NULL patch_labels", dict(plab=None)))
    wrong["crimac_gather_patches_memm_labels_multi"].append(("NULL patch_labels", dict(plab=None)))
    wrong["crimac_gather_eval_crops"].append(("flavour = 2", dict(flavour=2)))
    for name in ("crimac_labels_test_transform", "crimac_labels_test_transform_multi"):
        wrong[name].append(("odd H", dict(H=15)))
    wrong["crimac_labels_test_transform"] += [("seabed vector and mask", dict(mask=vec)), ("n_range = 0", dict(n_range=0))]
    wrong["crimac_labels_extend_mask"].append(("n_boxes < 0", dict(n_boxes=-1)))
    wrong["crimac_labels_extend_mask_multi"].append(("NULL box_off", dict(off=None)))
    return [(name, what, list(dict(valid[name], **over).values())) for name in valid for what, over in wrong[name]]


def check_refusals(buf):
    lib = hip.load_library()
    cases = refusal_cases(buf)
    assert {name for name, _, _ in cases} >= set(GATHERS) and len({name for name, _, _ in cases}) == 12
    for name, what, args in cases:
        rc = getattr(lib, name)(*args, None)
        msg = lib.crimac_last_error().decode()
        assert rc != 0, (name, what)
        assert msg.startswith(name[len("crimac_"):] + ":"), (name, what, msg)


def test_every_entry_point_keeps_its_refusals_under_its_own_name():
    t = dict(data=torch.full((C, 16, 16), 1e-3, device=DEV), lab=torch.zeros((16, 16), dtype=torch.int16, device=DEV),
             cen=torch.tensor([[8, 8]], dtype=torch.int32, device=DEV),
             cen64=torch.tensor([[8, 8]], dtype=torch.int64, device=DEV),
             out=torch.zeros((PH * PW, 16), dtype=torch.float32, device=DEV),
             src=torch.zeros(1, dtype=torch.int32, device=DEV), plab=torch.zeros((1, PH, PW), dtype=torch.int16, device=DEV),
             crop=torch.zeros((1, C, PH, PW), device=DEV), boxes=torch.tensor([[0, 8, 0, 8]], dtype=torch.int32, device=DEV),
             off=torch.tensor([0, 1, 1], dtype=torch.int32, device=DEV),
             vec=torch.full((16,), 12, dtype=torch.int32, device=DEV))
    row = (t["data"].data_ptr(), t["lab"].data_ptr(), t["vec"].data_ptr(), 0, 16, 16)
    t["descs"] = torch.tensor([row, row], dtype=torch.int64).to(DEV)
    assert t["descs"].shape[1] == hip.MEMM_DESC_WORDS
    check_refusals(lambda name: ptr(t[name]))
    torch.cuda.synchronize()                                 # (nothing was launched: nothing to fail here either)
    assert bool((t["out"] == 0).all()) and bool((t["plab"] == 0).all())


# ---- the descriptor edge: src = [1, -1, 0] over two sources -------------------------------------------------------------
EXTENTS = [(40, 24), (21, 37)]                                # pings x range
SRC = [1, -1, 0]
CEN = [(3, 20), (12, 12), (20, 1)]                            # (range, ping): over an edge of source 1, -, of source 0
SENT_F, SENT_L, SENT_X = -7.0, 77, 0x5A5A


def raw(x):
    return x.view(torch.int16) if x.element_size() == 2 else x.view(torch.int32)


@pytest.fixture(scope="module")
def edge():
    rng = np.random.Generator(np.random.PCG64(3))
    src = []
    for n_pings, n_range in EXTENTS:
        sv = np.power(10.0, rng.uniform(-8.5, 0.5, size=(C, n_pings, n_range))).astype(np.float32)
        sv[0][rng.random((n_pings, n_range)) < 0.02] = np.nan
        sv[2][rng.random((n_pings, n_range)) < 0.02] = np.inf
        lab = rng.choice(np.array([0, 0, 0, 27, 1, 12, -1, -100], dtype=np.int16), size=(n_pings, n_range))
        src.append((torch.from_numpy(sv).to(DEV), torch.from_numpy(lab).to(DEV), n_pings, n_range))
    table = torch.tensor([(d.data_ptr(), l.data_ptr(), 0, 0, w, h) for d, l, w, h in src], dtype=torch.int64).to(DEV)
    cen = torch.tensor(CEN, dtype=torch.int32, device=DEV)
    each = [cen[p:p + 1].contiguous() for p in range(3)]
    # the labels of the patches AFTER a label transform, as the border rule by patch labels reads them: some -100
    plab = torch.from_numpy(rng.choice(np.array([0, 1, 2, -100], dtype=np.int16), size=(3, PH, PW))).to(DEV)
    return src, table, torch.tensor(SRC, dtype=torch.int32, device=DEV), cen, each, plab


def test_eval_crops_descriptor_branch_skips_a_bad_src_and_equals_the_scalar_branch(edge):
    src, table, src_d, cen, each, _ = edge
    crop = torch.full((3, C, PH, PW), SENT_F, device=DEV)
    lab = torch.full((3, PH, PW), SENT_L, dtype=torch.int16, device=DEV)
    call("crimac_gather_eval_crops_multi", ptr(table), 2, ptr(src_d), C, ptr(cen), 3, PH, PW, ptr(crop), ptr(lab))
    assert bool((crop[1] == SENT_F).all()) and bool((lab[1] == SENT_L).all())
    for p in (0, 2):
        d, l, w, h = src[SRC[p]]
        want_d, want_l = torch.empty((1, C, PH, PW), device=DEV), torch.empty((1, PH, PW), dtype=torch.int16, device=DEV)
        call("crimac_gather_eval_crops", ptr(d), C, w, h, ptr(l), ptr(each[p]), 1, PH, PW, 1, ptr(want_d), ptr(want_l))
        assert torch.equal(crop[p].view(torch.int32), want_d[0].view(torch.int32)) and torch.equal(lab[p], want_l[0]), p
        assert bool((want_l == -100).any()) and bool((want_d != 0).any())            # the patch does cross an edge


@pytest.mark.parametrize("by_patch_labels", [False, True])
def test_gather_descriptor_branch_skips_a_bad_src_and_equals_the_scalar_branch(edge, by_patch_labels):
    src, table, src_d, cen, each, plab = edge
    px = PH * PW
    for prec, dtype in STORAGE.items():
        code = hip.PREC_NAMES[prec]
        x = torch.empty((3 * px, 16), dtype=dtype, device=DEV)
        raw(x).fill_(SENT_X)
        if by_patch_labels:
            call("crimac_gather_patches_memm_labels_multi", code, ptr(table), 2, ptr(src_d), C, ptr(cen), 3, PH, PW, ptr(x),
                 16, ptr(plab))
        else:
            call("crimac_gather_patches_memm_multi", code, ptr(table), 2, ptr(src_d), C, ptr(cen), 3, PH, PW, ptr(x), 16)
        got = raw(x).view(3, px, -1)
        assert bool((got[1] == SENT_X).all()), prec
        for p in (0, 2):
            d, l, w, h = src[SRC[p]]
            want = torch.empty((px, 16), dtype=dtype, device=DEV)
            if by_patch_labels:
                own = plab[p:p + 1].contiguous()
                call("crimac_gather_patches_memm_labels", code, ptr(d), C, w, h, ptr(each[p]), 1, PH, PW, ptr(want), 16,
                     ptr(own), 0, 0, 0.0, None, 0, None, 0, None, 0, None)
            else:
                call("crimac_gather_patches_memm", code, ptr(d), C, w, h, ptr(each[p]), 1, PH, PW, ptr(want), 16, ptr(l))
            assert torch.equal(got[p], raw(want)), (prec, p)
            assert bool((raw(want)[:, :C] != 0).any())
