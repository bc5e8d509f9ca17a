"""``UNet_Baseline`` for MI355X: the reference's module surface over hand-written HIP kernels.

Drop-in for ``crimac_unet/models/unet.py`` (``UNet_Baseline`` :304-343, ``UNet.__init__`` :200-289):
same constructor signature, same ``state_dict`` keys / shapes / dtypes (so reference ``.pt``
checkpoints load and vice versa, pipeline.py:109-130), same ``forward(x[B,C,H,W] fp32) -> logits
[B,n_classes,H,W] fp32`` in train and eval mode, same default parameter initialisation (the torch
layer objects are kept as parameter containers, constructed in the reference's order, so a given
seed yields the same initial weights).

What differs is only *who computes*: ``forward``/``backward`` run the CDNA4 kernels of
libcrimac_unet_hip.so through :class:`~crimac_classifiers_unet_amd.engine.UNetEngine`.  No torch
conv/BN/pool/CE kernel is ever dispatched and there is no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .engine import UNetEngine


class _EncoderStage(nn.Module):
    """Parameter container with the reference's key names ``main.{0,1,3,4}`` (unet.py:76-83)."""

    def __init__(self, cin, cout, pooling):
        super().__init__()
        self.pooling = pooling
        self.main = nn.Sequential(
            nn.Conv2d(cin, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU(),
            nn.Conv2d(cout, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU())
        if pooling:
            self.pool = nn.MaxPool2d(2, 2)     # parameter-free; keeps the module tree identical


class _DecoderStage(nn.Module):
    """Parameter container with the reference's key names upconv/conv1/conv2/bn1/bn2 (unet.py:112-122).

    up_mode 'upsample' (unet.py:50-56): ``upconv`` is Sequential(Upsample(bilinear, x2), Conv2d(cin, cout, 1)) -- keys
    ``upconv.1.weight`` / ``upconv.1.bias``, registered in the reference's order (same seeded initialisation)."""

    def __init__(self, cin, cout, up_mode="transpose"):
        super().__init__()
        if up_mode == "transpose":
            self.upconv = nn.ConvTranspose2d(cin, cout, kernel_size=2, stride=2)
        else:
            self.upconv = nn.Sequential(nn.Upsample(mode="bilinear", scale_factor=2), nn.Conv2d(cin, cout, kernel_size=1))
        self.conv1 = nn.Conv2d(2 * cout, cout, 3, padding=1)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        self.bn1 = nn.BatchNorm2d(cout)
        self.bn2 = nn.BatchNorm2d(cout)


class _UNetFunction(torch.autograd.Function):
    """One autograd node for the whole network: forward and backward are HIP kernel chains.

    The activations a backward pass needs live in the ENGINE (one set of buffers, overwritten by every
    train-mode forward), not in the autograd graph.  Each forward is therefore stamped with a generation
    number; a backward through a node whose activations have since been overwritten raises instead of silently
    differentiating the wrong forward (torch keeps one set of activations per node; the reference loop,
    pipeline.py:167-178, only ever has one forward in flight).  Gradients ACCUMULATE into ``.grad`` like torch's:
    whatever ``.grad`` holds when backward starts is added to the new gradient, so backward-twice-then-step
    (micro-batching) works and ``zero_grad`` (either form) starts afresh.
    """

    @staticmethod
    def forward(ctx, x, engine, meta, *params):
        ctx.engine = engine
        ctx.nparams = len(params)
        out = engine.forward(x, training=True, meta=meta)
        ctx.generation = engine.forward_generation
        return out

    @staticmethod
    def backward(ctx, dlogits):
        eng = ctx.engine
        if ctx.generation != eng.forward_generation or eng.saved is None:
            raise RuntimeError(
                "UNet_Baseline (MI355X build): backward() of a forward pass whose activations were overwritten by a "
                "later train-mode forward (or already consumed by an earlier backward).  The HIP engine keeps the "
                "activations of the LAST train-mode forward only: run forward -> loss -> backward per micro-batch "
                "(gradients accumulate in .grad across backward calls until zero_grad).")
        # torch semantics: backward ADDS to whatever .grad holds.  Gradients that alias the flat buffer are
        # carried through one clone of it; foreign .grad tensors (assigned by the user) are added per parameter.
        carry, aliased = {}, 0
        for name, p in eng.P.items():
            g = p.grad
            if g is None:
                continue
            if g.data_ptr() == eng.G[name].data_ptr():
                aliased += 1
            else:
                carry[name] = g
        none_grad = [name for name, p in eng.P.items() if p.grad is None]
        prev = eng.flat_g.clone() if (aliased or eng.accumulate_grads) else None
        ls = float(eng.loss_scale)        # fp16 storage: activation gradients travel scaled, .grad holds true values
        eng.backward(dlogits * ls if ls != 1.0 else dlogits)
        if ls != 1.0:
            eng.flat_g.mul_(1.0 / ls)     # (an overflowed gradient stays inf: SGDMomentum.step skips that step)
        eng.saved = None                  # consumed: a second backward through this node must not run on stale buffers
        if prev is not None:
            if none_grad and not eng.accumulate_grads:        # set_to_none on some parameters: those start afresh
                for name in none_grad:
                    o, n, _ = eng.layout[name]
                    prev[o:o + n].zero_()
            eng.flat_g.add_(prev)
        for name, p in eng.P.items():
            if name in carry:
                eng.G[name].add_(carry[name])
            p.grad = eng.G[name]     # .grad aliases the flat buffer (zero_grad(set_to_none) undoes it)
        # gradients were written straight into the flat buffer; return None so autograd does not
        # add them a second time
        return (None, None, None) + (None,) * ctx.nparams


class UNet_Baseline(nn.Module):
    """U-Net of the reference pipeline (pipeline.py:390-398) on MI355X.

    Extra keyword (defaults keep the reference call sites working unchanged):
      precision: 'bf16'  -- bf16 activations / MFMA, fp32 accumulate (throughput mode)
                 'f32x3' -- fp32 activations, 2-plane split-bf16 MFMA (~2^-16 per product)
                 'f32x6' -- fp32 activations, 3-plane split, 6 MFMAs per product (fp32-equivalent:
                            the parity mode, <=1e-3 on logits with bit-exact argmax masks)
                 'f32h3' -- fp32 activations; forward products on a 2-plane fp16 split (~2^-21 per product, 3 MFMAs:
                            fp32-class logits at half the MFMAs of 'f32x6'), backward on the 2-plane bf16 split
                 'h3p'   -- the fast parity mode: f32h3's forward arithmetic with the operands stored as fp16 PLANE PAIRS
                            (hi + lo) split once by the kernel that produces them, so every contraction runs on the LDS-DMA
                            kernels; the backward pass runs on loss-scaled fp16 plane pairs as well (overflow skip as 'fp16')
                 'h3f'   -- parity TRAINING at speed: the 'h3p' forward (bit-identical logits) with a 1-MFMA fp16 backward --
                            output gradients, the up-half of d(concat) and the input-gradient weight planes in plain
                            fp16, conv outputs and activation gradients in fp32 (ReLU / max-pool decisions as in 'h3p'),
                            weight gradients on the hi plane of the saved activations; every gradient tensor inside the
                            tolerance 'h3p' is held to (worst 0.76 of it); 1.39x the training rate of 'h3p'.  Covers
                            UNet_LateMetInject too (not the narrow nets and up_mode='upsample': 'h3p' there)
                 'fp16'  -- fp16 activations / MFMA, fp32 accumulate, loss-scaled gradients with overflow skip
                            (BASELINE configs[4]); same kernels and rate as 'bf16'
      infer_precision: precision of EVAL-mode forwards (``model.eval()``; ``predict_softmax``; tiled inference).

    Defaults.  ``UNet_Baseline(n_classes, in_channels)`` -- the reference's call -- trains in 'bf16' (throughput) and
    predicts in 'h3p': eval-mode logits within 1e-5 of the reference's with identical argmax masks, which is what the
    saved predictions of the reference pipeline promise (bf16 inference differs from the reference at ~0.4 % of the
    pixels of the golden crop).  An explicit ``precision=`` applies to both modes unless ``infer_precision=`` is given
    too.  The two modes share the parameters (one flat fp32 buffer); each keeps its own packed MFMA operands.
    """

    DEFAULT_TRAIN_PRECISION = "bf16"
    DEFAULT_INFER_PRECISION = "h3p"
    # argmax flips vs the reference on the golden crop (2 x 256 x 256 = 131072 pixels, tests/golden/full64_256.npz,
    # eval mode), measured by bench.py's golden_parity: precisions that do NOT meet the north-star parity bar
    PARITY_FAILING = {"bf16": "558 of 131072 pixels (0.43 %)", "fp16": "about 0.05 % of the pixels"}

    def __init__(self, n_classes, in_channels, meta_in_channels=0, late_meta_inject=False, depth=5,
                 start_filts=64, up_mode="transpose", merge_mode="concat", precision=None, infer_precision=None):
        super().__init__()
        if up_mode not in ("transpose", "upsample"):
            raise ValueError('"{}" is not a valid mode for upsampling. Only "transpose" and '
                             '"upsample" are allowed.'.format(up_mode))
        if merge_mode not in ("concat", "add"):
            raise ValueError('"{}" is not a valid mode for merging up and down paths. Only "concat" '
                             'and "add" are allowed.'.format(merge_mode))
        if merge_mode != "concat":
            # the reference pipeline always passes concat (pipeline.py:396-397)
            raise NotImplementedError("the MI355X hot path implements merge_mode='concat' (with up_mode 'transpose' -- "
                                      "what the pipeline uses -- or 'upsample')")
        if late_meta_inject and type(self) is UNet_Baseline:
            raise ValueError("late_meta_inject=True is the UNet_LateMetInject model (pipeline.py:400-410)")
        self.late_meta_inject = bool(late_meta_inject)
        self.n_classes, self.in_channels = n_classes, in_channels
        self.meta_in_channels = meta_in_channels
        self.depth, self.start_filts = depth, start_filts
        self.up_mode, self.merge_mode = up_mode, merge_mode

        enc, outs = [], in_channels
        for i in range(depth):
            ins, outs = (in_channels if i == 0 else outs), start_filts * 2 ** i
            enc.append(_EncoderStage(ins, outs, pooling=i < depth - 1))
        dec = []
        for _ in range(depth - 1):
            ins, outs = outs, outs // 2
            dec.append(_DecoderStage(ins, outs, up_mode))
        self.down_convs = nn.Sequential(*enc)
        self.up_convs = nn.Sequential(*dec)
        if not self.late_meta_inject:
            self.conv_final = nn.Conv2d(outs, n_classes, kernel_size=1)
        else:
            # registration order of the reference (unet.py:283-289): conv_final, then post_processing_weights
            self.conv_final = nn.Conv2d(outs + meta_in_channels, n_classes, kernel_size=1)
            self.post_processing_weights = _MetaPostProcessing(meta_in_channels, 1)
        if infer_precision is None:
            infer_precision = self.DEFAULT_INFER_PRECISION if precision is None else precision
        if precision is None:
            precision = self.DEFAULT_TRAIN_PRECISION
        self._precision = precision
        self._infer_precision = infer_precision
        self._engine = None
        self._infer_engine = None

    # -- engine plumbing -----------------------------------------------------------------------
    @property
    def engine(self) -> UNetEngine:
        """The training engine (owner of the flat parameter / gradient / momentum buffers)."""
        if self._engine is None:
            try:
                eng = UNetEngine(self, self._precision)
            except AttributeError as e:   # nn.Module.__getattr__ would swallow it as "no attribute engine"
                raise RuntimeError(f"cannot create the HIP engine: {e}") from e
            object.__setattr__(self, "_engine", eng)
        return self._engine

    @property
    def infer_engine(self) -> UNetEngine:
        """The engine of eval-mode forwards: the training engine itself when the two precisions agree, otherwise a
        follower on the same parameters."""
        if self._infer_precision == self._precision:
            return self.engine
        if self._infer_engine is None:
            try:
                eng = UNetEngine(self, self._infer_precision, leader=self.engine)
            except AttributeError as e:
                raise RuntimeError(f"cannot create the HIP engine: {e}") from e
            object.__setattr__(self, "_infer_engine", eng)
        return self._infer_engine

    @property
    def precision(self):
        return self._precision

    @property
    def infer_precision(self):
        return self._infer_precision

    def set_precision(self, precision, infer_precision=None):
        """Change the precision (both modes, or ``infer_precision`` separately); engines are rebuilt on next use."""
        infer_precision = infer_precision or precision
        if precision != self._precision or infer_precision != self._infer_precision:
            self._precision, self._infer_precision = precision, infer_precision
            object.__setattr__(self, "_engine", None)
            object.__setattr__(self, "_infer_engine", None)
        return self

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        if self._engine is not None:
            self._engine.mark_dirty()      # (followers included)
        return out

    def load_state_dict(self, *a, **kw):
        out = super().load_state_dict(*a, **kw)
        if self._engine is not None:
            self._engine.mark_dirty()
        return out

    # -- the hot path --------------------------------------------------------------------------
    def forward(self, x):
        if self.training and torch.is_grad_enabled():
            eng = self.engine
            eng.bind()
            return _UNetFunction.apply(x, eng, None, *eng.P.values())
        if self.training:
            return self.engine.forward(x, training=True)
        return self.infer_engine.forward(x, training=False)

    def predict_softmax(self, x):
        """Eval forward with F.softmax(dim=1) fused into the 1x1 head (pipeline.py:205-219)."""
        return self.infer_engine.forward(x, training=False, softmax=True)


class _MetaPostProcessing(nn.Module):
    """Parameter container with the reference's key names ``main.{0,2,4}`` (MetaPostProcessing, unet.py:140-166):
    Linear(Cm, 32) / ReLU / Linear(32, 32) / ReLU / Linear(32, out) applied over the channel axis of [N, C, H, W]."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.hidden_channels_1 = self.hidden_channels_2 = 32
        self.main = nn.Sequential(nn.Linear(in_channels, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU(),
                                  nn.Linear(32, out_channels))


class UNet_LateMetInject(UNet_Baseline):
    """U-Net with late metadata injection (reference unet.py:346-391) on MI355X.

    ``forward(x, meta_tensor)``: the U-Net body runs on ``x`` [B, in_channels, H, W]; ``meta_tensor`` [B, Cm, H, W]
    goes through the per-pixel perceptron ``post_processing_weights`` (Cm -> 32 -> 32 -> 1) and its output plane is
    concatenated behind the 64 decoder channels in front of ``conv_final`` -- which the reference hard-codes as
    ``conv1x1(65, 3)`` (unet.py:370), so ``start_filts`` must be 64 and ``n_classes`` 3, whatever the constructor
    arguments of the base class computed.  Same ``state_dict`` keys and shapes as the reference module."""

    def __init__(self, n_classes, in_channels, meta_in_channels, late_meta_inject=True, depth=5, start_filts=64,
                 up_mode="transpose", merge_mode="concat", precision=None, infer_precision=None):
        super().__init__(n_classes, in_channels, meta_in_channels, True, depth, start_filts, up_mode, merge_mode,
                         precision, infer_precision)
        if start_filts != 64 or n_classes != 3:
            raise ValueError("UNet_LateMetInject hard-codes conv_final = conv1x1(65, 3) (reference unet.py:370): "
                             "start_filts must be 64 and n_classes 3")
        self.conv_final = nn.Conv2d(65, 3, kernel_size=1)

    def forward(self, x, meta_tensor):
        if self.training and torch.is_grad_enabled():
            eng = self.engine
            eng.bind()
            return _UNetFunction.apply(x, eng, meta_tensor, *eng.P.values())
        if self.training:
            return self.engine.forward(x, training=True, meta=meta_tensor)
        return self.infer_engine.forward(x, training=False, meta=meta_tensor)

    def predict_softmax(self, x, meta_tensor):
        return self.infer_engine.forward(x, training=False, softmax=True, meta=meta_tensor)
