"""precision='h3f' for UNet_LateMetInject, the parts that need no GPU: the engine builds, the other h3f refusals stand, and
the fused late-injection head is declared in the C-ABI header the binding is derived from."""
import re

import pytest

import crimac_classifiers_unet_amd as pkg
from crimac_classifiers_unet_amd import hip
from crimac_classifiers_unet_amd.build import HEADER
from crimac_classifiers_unet_amd.engine import UNetEngine


@pytest.mark.parametrize("cm", [1, 7])
def test_h3f_engine_of_the_late_injection_model_constructs(cm):
    eng = UNetEngine(pkg.UNet_LateMetInject(3, 4, cm), "h3f")
    assert eng.lmi and eng.bwd16 and eng.meta_channels == cm
    assert eng.prec == hip.PREC_H3P and eng.prec_bwd == hip.PREC_H3F_BWD          # h3p's forward, the fp16 backward
    assert eng.loss_scale == 2.0 ** 16 and eng.dynamic_loss_scale
    m = pkg.UNet_LateMetInject(3, 4, cm, precision="h3f")
    assert m.late_meta_inject and m.meta_in_channels == cm


def test_the_other_h3f_refusals_still_raise():
    with pytest.raises(NotImplementedError, match="precision 'h3f' with up_mode='upsample'"):
        UNetEngine(pkg.UNet_Baseline(3, 4, up_mode="upsample"), "h3f")
    with pytest.raises(NotImplementedError, match="precision 'h3f': transposed convolutions"):
        UNetEngine(pkg.UNet_Baseline(3, 4, start_filts=16), "h3f")
    with pytest.raises(NotImplementedError, match="precision 'h3f' with up_mode='upsample'"):
        UNetEngine(pkg.UNet_LateMetInject(3, 4, 7, up_mode="upsample"), "h3f")
    with pytest.raises(ValueError):                        # 9 metadata channels: refused in every precision
        UNetEngine(pkg.UNet_LateMetInject(3, 4, 9), "h3f")


def test_header_declares_the_fused_head_and_its_prototypes_load():
    header = open(HEADER).read()
    assert re.search(r"\bint crimac_head_meta_fwd\(int prec, const void\* x, long x_ld, const float\* w,", header)
    for cite in ("unet.py:346-391", "pipeline.py:170-174", "pipeline.py:210-216"):
        assert cite in header[header.index("The late-injection head in one launch each way"):header.index("int crimac_head_meta_fwd")]
    assert int(re.search(r"#define CRIMAC_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION
    assert re.search(r"\bint crimac_head_meta_bwd\(int prec, const float\* dlogits, const void\* x, long x_ld,", header)
    assert len(hip.SIGNATURES["crimac_head_meta_fwd"]) == 22            # 21 arguments and the stream
    assert len(hip.SIGNATURES["crimac_head_meta_bwd"]) == 35            # 34 arguments and the stream
    # the built library exports both, with the parsed prototypes bound (argument checks precede any HIP call)
    lib = hip.load_library()
    assert lib.crimac_version() == hip.ABI_VERSION
    for name in ("crimac_head_meta_fwd", "crimac_head_meta_bwd"):
        fn = getattr(lib, name)
        assert list(fn.argtypes) == list(hip.SIGNATURES[name])
    # the chain they replace stays exported, unchanged
    for name in ("crimac_head_fwd", "crimac_meta_mlp_fwd", "crimac_meta_inject_fwd", "crimac_meta_bwd", "crimac_head_bwd"):
        assert name in hip.SIGNATURES and hasattr(lib, name)
