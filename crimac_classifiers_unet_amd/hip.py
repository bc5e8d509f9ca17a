"""ctypes binding of libcrimac_unet_hip.so (the C ABI declared in include/crimac_unet_hip.h).

PyTorch is used only for device memory and streams: tensors are passed as raw ``data_ptr()``s plus
the current ``torch.cuda`` stream handle.  There is NO CPU fallback: if the library is missing or a
tensor is not on a GPU, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch

from . import build as _build

PREC_BF16 = 0
PREC_F32X3 = 1
PREC_F32X6 = 2
PREC_FP16 = 3
PREC_F32H3 = 4
PREC_H3P = 5             # pre-split fp16 plane pairs (CRIMAC_PREC_H3P): F32H3's arithmetic on the LDS-DMA kernels
PREC_H3F_BWD = 6         # CRIMAC_PREC_H3F_BWD: the backward pass of 'h3f' (fp16 MFMA operands, everything else as H3P)
# 'h3f': the forward pass of 'h3p' (same kernels, same bits) with fp16 MFMA operands in the BACKWARD pass -- an engine-level
# mode (engine.py): forward launches carry PREC_H3P, the backward pass's contractions and BatchNorm-backward PREC_H3F_BWD
PREC_NAMES = {"bf16": PREC_BF16, "f32x3": PREC_F32X3, "f32x6": PREC_F32X6, "fp16": PREC_FP16, "f32h3": PREC_F32H3,
              "h3p": PREC_H3P, "h3f": PREC_H3P}
MFMAS_PER_PRODUCT = {PREC_BF16: 1, PREC_FP16: 1, PREC_F32X3: 3, PREC_F32H3: 3, PREC_H3P: 3, PREC_F32X6: 6, PREC_H3F_BWD: 1}
PREC_PLANES = {PREC_BF16: 1, PREC_F32X3: 2, PREC_F32X6: 3, PREC_FP16: 1, PREC_F32H3: 2, PREC_H3P: 2}   # 16-bit planes per operand
# `planes` argument of the packing entry points (CRIMAC_PLANES_* of the header): bits 0-3 planes, bit 4 / 5 forward /
# input-gradient planes in IEEE half, bits 8-15 log2 of the scale on the forward planes
PLANES_FP16 = 1 | 16 | 32
PLANES_F32H3 = 2 | 16 | (8 << 8)
PLANES_FWD_FRAG = 65536       # crimac_pack_conv3x3: the forward plane fragment-major (CRIMAC_PLANES_FWD_FRAG)
PLANES_INTERLEAVED = 64      # both planes in the `hi` buffer, [32 hi | 32 lo] per 32-channel block of a row
PLANES_H3P = 2 | 16 | 32 | PLANES_INTERLEAVED | 128 | (8 << 8)        # CRIMAC_PLANES_H3P
PREC_PLANES_ARG = {PREC_BF16: 1, PREC_F32X3: 2, PREC_F32X6: 3, PREC_FP16: PLANES_FP16, PREC_F32H3: PLANES_F32H3,
                   PREC_H3P: PLANES_H3P}
EPI_RELU, EPI_OUT_PLANES, EPI_CIN4 = 1, 2, 4      # `relu` argument of the convolution entry points (CRIMAC_EPI_*)
EPI_WFRAG = 16                # ... the weight plane is fragment-major (CRIMAC_EPI_WFRAG)
EPI_WROWS = 32                # ... and the channel-split kernel's rows form reads it (CRIMAC_EPI_WROWS)
NARROW_DGRAD = 64             # crimac_conv3x3_narrow: the input gradient (CRIMAC_NARROW_DGRAD)
LAYER_FWD_FRAG, LAYER_DG_FRAG = 16, 32      # crimac_layer_desc.kind flags (CRIMAC_LAYER_*_FRAG)
LAYER_CONV3X3, LAYER_UPCONV2X2, LAYER_CONV1X1 = 0, 1, 2     # crimac_layer_desc.kind bits 0-1
# precision the BACKWARD kernels (input gradients, weight gradients) are called with: F32H3 is a forward-operand
# mode (fp16 planes have no range for gradients), its backward pass runs on the 2-plane bf16 split
PREC_BACKWARD = {PREC_F32H3: PREC_F32X3}
PREC_16BIT = (PREC_BF16, PREC_FP16)


class HipLibraryError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "unsigned int": C.c_uint,
            "unsigned long long": C.c_ulonglong, "float": C.c_float, "double": C.c_double}
_KEYWORDS = {"const", "void", "char", "short", "signed", "struct", *" ".join(_SCALARS).split()}


def _declarator(decl: str, where: str):
    """``const float* w`` / ``long long n`` -> (name, ctype).  Every pointer is a c_void_p (so ``byref``, ctypes arrays and
    ``None`` pass at every call site) whatever it points to -- `short* p` and `crimac_x* p` alike: ctypes never looks
    through it, so the base type needs no entry in the map; scalars come from the closed map above.  Anything else raises."""
    toks = decl.replace("*", " * ").split()
    if toks[:1] == ["const"]:
        del toks[0]
    *kind, name = toks or [""]
    if not kind or not re.fullmatch(r"[A-Za-z_]\w*", name) or name in _KEYWORDS:
        raise HipLibraryError(f"{where}: `{decl.strip()}` is not `<type> <name>`")
    if len(kind) >= 2 and kind[-1] == "*" and "*" not in kind[:-1]:
        return name, C.c_void_p
    if " ".join(kind) not in _SCALARS:
        raise HipLibraryError(f"{where}: unknown type `{' '.join(kind)}` in `{decl.strip()}`")
    return name, _SCALARS[" ".join(kind)]


def parse_header(text: str):
    """The C ABI as include/crimac_unet_hip.h states it: (prototypes, structs, defines).
    prototypes: name -> (restype, argtypes, takes_stream), takes_stream = the last parameter is ``void* stream``;
    structs: tag -> [(field, ctype)] in declaration order; defines: every ``#define CRIMAC_<NAME> <integer expression>``,
    evaluated in order (``typedef struct crimac_x crimac_x;`` only names a struct that another header lays out: nothing
    to record).  A declaration this does not recognise raises HipLibraryError naming it: it never guesses."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S).replace("\\\n", " ")
    protos, structs, defines = {}, {}, {}
    for line in re.findall(r"^[ \t]*(#.*?)\s*$", text, flags=re.M):
        m = re.fullmatch(r"#\s*define\s+(CRIMAC_\w+)\s+(\S.*)", line)
        if m:
            expr = re.sub(r"CRIMAC_\w+", lambda n: f"({defines.get(n.group(), '?')})", m.group(2))
            if not re.fullmatch(r"[\d\s()|&<>+*~-]+", expr) or "**" in expr:       # (`**` is Python, not C)
                raise HipLibraryError(f"#define {m.group(1)}: `{m.group(2)}` is not an integer expression of earlier defines")
            try:
                defines[m.group(1)] = int(eval(expr, {"__builtins__": {}}))
            except Exception as e:
                raise HipLibraryError(f"#define {m.group(1)}: cannot evaluate `{m.group(2)}` ({e})") from None
        elif not re.fullmatch(r"#\s*(ifn?def\s+\w+|endif|define\s+\w+)", line):       # include guard, __cplusplus
            raise HipLibraryError(f"cannot parse the directive `{line}`")

    def struct(m):
        fields = structs.setdefault(m.group(1), [])
        for decl in filter(None, map(str.strip, m.group(2).split(";"))):
            first, *more = map(str.strip, decl.split(","))
            name, ctype = _declarator(first, f"struct {m.group(1)}")
            if more and (ctype is C.c_void_p or not all(re.fullmatch(r"[A-Za-z_]\w*", n) for n in more)):
                raise HipLibraryError(f"struct {m.group(1)}: cannot parse the field list `{decl}`")
            fields += [(n, ctype) for n in (name, *more)]
        return ""

    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s+(crimac_\w+)\s*\{([^{}]*)\}\s*\1\s*;", struct, text)
    body = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, flags=re.S)
    if not body:
        raise HipLibraryError('the declarations are not one `extern "C" { ... }` block')
    for stmt in filter(None, map(str.strip, body.group(1).split(";"))):
        if re.fullmatch(r"typedef\s+struct\s+(crimac_\w+)\s+\1", stmt):      # names a struct that another header lays out
            continue
        m = re.fullmatch(r"(int|const\s+char\s*\*)\s*(crimac_\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m:
            raise HipLibraryError(f"cannot parse the declaration `{' '.join(stmt.split())}`")
        params = [] if m.group(3).strip() == "void" else m.group(3).split(",")
        protos[m.group(2)] = (C.c_int if m.group(1) == "int" else C.c_char_p,
                              [_declarator(a, m.group(2))[1] for a in params],
                              bool(params) and params[-1].replace("*", " * ").split() == ["void", "*", "stream"])
    return protos, structs, defines


try:
    with open(_build.HEADER) as _header:
        PROTOTYPES, STRUCTS, DEFINES = parse_header(_header.read())
    with open(_build.MEMM_META_HEADER) as _header:          # (crimac_unet_hip.h names its struct, this one lays it out)
        MEMM_META_STRUCTS = parse_header(_header.read())[1]
except OSError as e:
    raise HipLibraryError(f"cannot read the C-ABI header {e.filename} ({e.strerror}): the binding is derived from it, so the "
                          "package needs include/ next to it (also with a CRIMAC_LIB override)") from None
del _header

ABI_VERSION = DEFINES["CRIMAC_ABI_VERSION"]      # a built library of another version is stale (load_library)
PR_BINS = DEFINES["CRIMAC_PR_BINS"]
# scratch of crimac_integrate_classes / crimac_integrate_layers: (cells of the launch + INTEGRATE_SPLIT_WGS) slots of INTEGRATE_SLOT_BYTES
INTEGRATE_SPLIT_WGS, INTEGRATE_SLOT_BYTES = DEFINES["CRIMAC_INTEGRATE_SPLIT_WGS"], DEFINES["CRIMAC_INTEGRATE_SLOT_BYTES"]
# name -> argtypes of every entry point that returns a status and takes the stream as its last argument (`call`)
SIGNATURES = {name: args for name, (res, args, stream) in PROTOTYPES.items() if stream and res is C.c_int}


class LayerDesc(C.Structure):
    """crimac_layer_desc (include/crimac_unet_hip.h): one Conv2d / ConvTranspose2d layer's buffers."""
    _fields_ = STRUCTS["crimac_layer_desc"]


class WgradGroupLayer(C.Structure):
    """crimac_wgrad_group_layer (include/crimac_unet_hip.h): one conv3x3 layer of a grouped weight-gradient launch."""
    _fields_ = STRUCTS["crimac_wgrad_group_layer"]


class MemmDesc(C.Structure):
    """crimac_memm_desc (include/crimac_unet_hip.h): one echogram of a multi-source gather / scatter."""
    _fields_ = STRUCTS["crimac_memm_desc"]


if any(C.sizeof(t) != 8 for _, t in MemmDesc._fields_):
    raise HipLibraryError("crimac_memm_desc has a field that is not 64 bits wide: the host writes the table as int64 words")
MEMM_DESC_WORDS = C.sizeof(MemmDesc) // 8      # data, labels, seabed, out (device addresses), n_pings, n_range


class MemmMetaDesc(C.Structure):
    """crimac_memm_meta_desc (include/crimac_memm_meta.h): the metadata source of one echogram of a multi-source launch."""
    _fields_ = MEMM_META_STRUCTS["crimac_memm_meta_desc"]


if any(C.sizeof(t) != 8 for _, t in MemmMetaDesc._fields_):
    raise HipLibraryError("crimac_memm_meta_desc has a field that is not 64 bits wide: the host writes the table as 64-bit "
                          "words")
MEMM_META_WORDS = C.sizeof(MemmMetaDesc) // 8      # portion_year (float64), then (device address, length) of three vectors

WGRAD_GROUP_MAX_LAYERS = 16      # CRIMAC_WGRAD_GROUP_MAX_LAYERS
MASK_PER_PATCH = -2147483648      # CRIMAC_MASK_PER_PATCH

_lib = None
_entry = {}          # name -> bound function of every SIGNATURES entry point, filled by load_library (`call` looks up here)


def library_path() -> str:
    return os.environ.get("CRIMAC_LIB") or _build.LIB_PATH       # override: kernel experiments only


def load_library():
    """dlopen the in-tree library and declare every prototype.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise HipLibraryError(
            f"{path} is missing: build it with `python -m crimac_classifiers_unet_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback for the U-Net hot path.")
    lib = C.CDLL(path)

    def declare(name):
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype, fn.argtypes = PROTOTYPES[name][:2]
        return fn

    ver = declare("crimac_version")()
    if ver != ABI_VERSION:
        raise HipLibraryError(f"{path} has ABI version {ver}, this binding needs {ABI_VERSION}: rebuild it "
                              "(`python -m crimac_classifiers_unet_amd.build --force`)")
    if not hasattr(lib, "crimac_layer_desc_size"):
        raise HipLibraryError(f"{path} does not export crimac_layer_desc_size: stale build")
    for size_fn, mirror in (("crimac_layer_desc_size", LayerDesc), ("crimac_wgrad_group_layer_size", WgradGroupLayer)):
        size = declare(size_fn)()
        if size != C.sizeof(mirror):
            raise HipLibraryError(f"{path}: {size_fn[:-5]} is {size} bytes in the library, {C.sizeof(mirror)} in this binding")
    # additive entry points do not bump the ABI version: a build of the same version from before one was added is stale too
    missing = [name for name in PROTOTYPES if not hasattr(lib, name)]
    if missing:
        raise HipLibraryError(f"{path} does not export {', '.join(missing)}: stale build, rebuild it "
                              "(`python -m crimac_classifiers_unet_amd.build --force`)")
    for name in PROTOTYPES:
        fn = declare(name)
        if name in SIGNATURES:
            _entry[name] = fn
    _lib = lib
    return lib


def _check(rc: int, name: str):
    if rc != 0:
        msg = load_library().crimac_last_error().decode(errors="replace")
        raise HipLibraryError(f"{name} failed ({rc}): {msg}")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, offset_elems: int = 0):
    """Raw device pointer of a tensor (+ element offset); None -> NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HipLibraryError("tensor is not on a GPU: the HIP path has no CPU fallback")
    return C.c_void_p(t.data_ptr() + offset_elems * t.element_size())


class Act:
    """A channel slice of an NHWC activation buffer: base tensor + channel offset + pixel stride."""

    __slots__ = ("t", "off", "ld", "C")

    def __init__(self, t, C_, off=0, ld=None):
        self.t = t
        self.off = off
        self.ld = ld if ld is not None else t.shape[-1]
        self.C = C_

    @property
    def p(self):
        return ptr(self.t, self.off)

    def slice(self, off, C_):
        return Act(self.t, C_, self.off + off, self.ld)


# When set to a list (bench.py), every call that passes ``flops=`` is bracketed by HIP events on
# the current stream and (name, flops, start, end) is appended.
PROFILE = None


def _entry_point(name: str):
    """What `call` falls back to when `_entry` has no such name: the first launch of the process, or a name to refuse."""
    if name not in SIGNATURES:
        raise HipLibraryError(f"{name} is not an entry point that takes a stream (include/crimac_unet_hip.h): "
                              "call a stream-less one through load_library()")
    load_library()
    return _entry[name]


def call(name: str, *args, flops=None, mfmas=1):
    """``flops``: algorithmic FLOPs of the launch (profiled launches only); ``mfmas``: MFMAs the kernel spends per
    algorithmic product (1 for 16-bit operands, 3 for plane pairs ...): flops * mfmas is what the MFMA pipe executes, the
    figure a roofline against the dense 16-bit peak needs when one step mixes precisions ('h3f')."""
    fn = _entry.get(name) or _entry_point(name)
    if PROFILE is not None and flops is not None:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        _check(fn(*args, _stream()), name)
        e.record()
        PROFILE.append((name, flops, s, e, mfmas))
        return
    _check(fn(*args, _stream()), name)
