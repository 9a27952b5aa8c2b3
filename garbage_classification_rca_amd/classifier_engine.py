"""One backbone + a linear head over libmmrca: the engine of the single-modality classifiers (classifiers.py; the reference's
``main_image.py`` / ``main_text.py`` models, models.py and CVPR_code/text_models.py).

The backbone code is :class:`~garbage_classification_rca_amd.engine.MMRCAEngine`'s own -- ``_vision_forward`` / ``_vision_backward``
(ViT-B/16, ViT-L/16, class-token tail included), :class:`~garbage_classification_rca_amd.conv_engine.ConvEncoder` (EfficientNetV2-M/-L,
ShuffleNetV2, MobileNetV3-Large) and ``_text_forward`` / ``_text_backward`` (DistilBERT, BERT, RoBERTa, packed captions) -- run over a smaller arena:

    image_model.* | head.weight [C, F], head.bias [C]        or        text_model.* | head.weight, head.bias

The head is ``mmrca_linear_cls_fwd`` / ``_bwd`` (csrc/classifier.hip): fp32 arithmetic on the backbone feature in whatever dtype the
backbone produced it, dropout from the same counter hash and mask epoch as every other dropout site.  Same ``forward`` / ``backward`` /
``trainable_spans`` / ``groups`` contract as the two-backbone engine, so the flat optimizers, ``GradSync``, ``hip_train_step`` and
``GraphedTrainStep`` drive it unchanged.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import lib as L
from . import spec as S
from .conv_engine import CLASSIFIER_CONV_MODELS, CONV_MODELS, ConvEncoder
from .engine import Arena, MMRCAEngine, TextPack

IMAGE_MODELS = tuple(S.VISION_SPECS) + ("eff_v2_medium", "eff_v2_large", "shuffle_net") + tuple(CLASSIFIER_CONV_MODELS)
_CONV = set(CONV_MODELS) | set(CLASSIFIER_CONV_MODELS)
TEXT_MODELS = tuple(S.TEXT_SPECS)


class ClassifierEngine(MMRCAEngine):
    """Owns parameters, gradients and activations of one single-backbone classifier replica on one GPU."""

    def __init__(self, backbone: str, n_classes: int = 4, dtype="bf16x3f", device="cuda", image_size: int = 224,
                 gemm_impl: int = L.IMPL_AUTO, attn_impl: int = L.IMPL_AUTO):
        """dtype: the four modes of MMRCAEngine (bf16 | fp32 | bf16x3 | bf16x3f, conv backbones in bf16 under bf16x3f)."""
        L.load()
        name = dtype.lower() if isinstance(dtype, str) else ""
        self.x3 = name in ("bf16x3", "x3", "bf16x3f", "x3f")
        self.x3f = name in ("bf16x3f", "x3f")
        if self.x3:
            dtype = torch.float32
        elif isinstance(dtype, str):
            dtype = {"bf16": torch.bfloat16, "fp32": torch.float32, "f32": torch.float32}[dtype.lower()]
        if backbone in S.TEXT_SPECS:
            self.kind = "text"
        elif backbone in S.VISION_SPECS or backbone in _CONV:
            self.kind = "image"
        else:
            raise ValueError(f"Invalid Model: {backbone}")
        self.backbone = backbone
        self.ts = S.TEXT_SPECS.get(backbone)
        self.vs = S.VISION_SPECS.get(backbone)
        self.n_classes, self.reverse, self.mode = int(n_classes), True, 0
        if not 1 <= self.n_classes <= 16:
            raise ValueError(f"n_classes must be in [1, 16], got {n_classes}")
        self.dtype, self.device = dtype, torch.device(device)
        self.dt = L.dtype_code(dtype)
        self.gdtype = torch.bfloat16 if self.x3f else dtype
        self.bdt = L.BF16 if self.x3f else self.dt
        self.gemm_impl, self.attn_impl = gemm_impl, attn_impl
        self.conv_dtype = torch.bfloat16 if (self.x3f and backbone in _CONV) else None
        self.conv = ConvEncoder(backbone, self, image_size) if (self.kind == "image" and self.vs is None) else None
        if self.kind == "text":
            prefix, enc = "text_model.", S.text_params(self.ts)
            self.feat_dim = self.ts.dim
        else:
            prefix, enc = "image_model.", (S.vision_params(self.vs) if self.vs is not None else self.conv.param_entries())
            self.feat_dim = self.vs.dim if self.vs is not None else self.conv.dim
        self.d_txt = self.ts.dim if self.ts is not None else 0
        self.d_img = self.feat_dim if self.kind == "image" else 0
        ents = [(prefix + k, s) for k, s in enc]
        self.head_keys = [("head.weight", (self.n_classes, self.feat_dim)), ("head.bias", (self.n_classes,))]
        ents += self.head_keys
        self.arena = Arena(ents, self.device, with_lp=(dtype == torch.bfloat16 or self.x3), with_lo=self.x3)
        self.param_keys = [k for k, _ in ents]
        self.encoder_span = self.arena.span(ents[0][0], prefix + enc[-1][0])
        if self.conv is not None:
            self.conv.init_buffers(self.device)
        self.head_span = self.arena.span("head.weight", "head.bias")
        self._bufs: Dict[Tuple, torch.Tensor] = {}
        self._g_planes = self.x3
        self._plane_valid, self._plane_fresh = set(), set()
        self._ln_planes = self._g_planes
        self._gelu_act = L.ACT_GELU_SAVE_GRAD_BF16 if self.x3f else L.ACT_GELU_SAVE_GRAD
        self._hdt = torch.bfloat16 if self.x3f else None
        self._saved = None
        self.groups: Dict[str, Tuple[int, int]] = {}
        starts = []
        for k in self.param_keys:
            gname = self._group_of(k)
            if not starts or starts[-1][0] != gname:
                starts.append((gname, self.arena.offsets[k][0]))
        for j, (gname, lo) in enumerate(starts):
            hi = starts[j + 1][1] if j + 1 < len(starts) else self.arena.total
            self.groups[gname] = (lo, hi)
        self.grad_sync = None
        self._side_v = self._side_t = self._side = None
        self._text_stream = None
        if self.kind == "text":
            for i in range(self.ts.layers):
                K = S.text_layer_keys(self.ts, i)
                o = [self.arena.offsets["text_model." + K[n] + ".weight"] for n in ("q", "k", "v")]
                assert o[1][0] == o[0][0] + o[0][2] and o[2][0] == o[1][0] + o[1][2], "qkv weights not adjacent"

    # ------------------------------------------------------------------ whole model
    def forward(self, ids, mask, images, drop_p: float = 0.0, seed: int = 0, save: bool = True, enc_drop_p: float = 0.0,
                text_pack: Optional[TextPack] = None, bn_train: bool = False):
        """image models read `images` fp32 [B,3,H,W], text models `ids` / `mask` int64 [B,T] (the other inputs are ignored; None is fine)
        -> logits fp32 [B, n_classes].  drop_p: the dropout in front of the Linear; enc_drop_p: the text encoder's own dropout."""
        used = ((images, "images"),) if self.kind == "image" else ((ids, "input ids"), (mask, "attention mask"))
        for t, nm in used:
            if t is None or not t.is_cuda:
                raise L.MmrcaError(f"{nm} must be in HBM; the classifier path has no CPU fallback")
        self.refresh_working_copy()
        self._plane_valid.clear()
        self._plane_fresh.clear()
        if self.kind == "text":
            feat, esv = self._text_forward(ids, mask, save, enc_drop_p, int(seed), text_pack)
        elif self.conv is not None:
            feat, esv = self.conv.forward(images, save, bn_train, int(seed)), None
        else:
            feat, esv = self._vision_forward(images, save)
        B = feat.shape[0]
        logits = torch.empty(B, self.n_classes, dtype=torch.float32, device=self.device)
        # the same seed stride per step as the encoders' site seeds: replay r of a captured step draws eager step seed + r's mask
        head_seed = self._site_seed(int(seed), 255, 0)
        L.linear_cls_fwd(feat, feat.stride(0), self.arena.view("head.weight"), self.arena.view("head.bias"), logits, B, self.feat_dim,
                         self.n_classes, float(drop_p), head_seed, L.dtype_code(feat.dtype))
        self._saved = dict(B=B, feat=feat, enc=esv, drop_p=float(drop_p), seed=head_seed, full=save)
        return logits

    def backward(self, dlogits, train_text: bool = True, train_image: bool = True):
        """accumulates into the gradient arena: the head always, the backbone when its flag (train_image / train_text) is set"""
        sv = self._saved
        if sv is None:
            raise L.MmrcaError("backward() without a forward()")
        train_enc = bool(train_text if self.kind == "text" else train_image)
        if train_enc and not sv["full"]:
            raise L.MmrcaError("backward through the backbone needs forward(save=True)")
        B, feat = sv["B"], sv["feat"]
        dl = dlogits.to(torch.float32).contiguous()
        dfeat = torch.empty(B, self.feat_dim, dtype=feat.dtype, device=self.device) if train_enc else None
        L.linear_cls_bwd(dl, feat, feat.stride(0), self.arena.view("head.weight"), self.arena.view("head.weight", "g"),
                         self.arena.view("head.bias", "g"), dfeat, B, self.feat_dim, self.n_classes, sv["drop_p"], sv["seed"],
                         L.dtype_code(feat.dtype))
        self._ready("head", flush=not train_enc)
        if train_enc:
            if self.kind == "text":
                self._text_backward(dfeat, sv["enc"])
            elif self.conv is not None:
                self.conv.backward(dfeat)
                self._ready("image_emb", flush=True)
            else:
                self._vision_backward(dfeat, sv["enc"])
        self.arena.lp_valid = False

    def trainable_spans(self, train_text: bool, train_image: bool):
        """[lo, hi) slices an optimizer step / all-reduce covers: the whole arena, or the head alone while the backbone is frozen"""
        train_enc = train_text if self.kind == "text" else train_image
        return [(0, self.arena.total)] if train_enc else [(self.groups["head"][0], self.arena.total)]
