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

The constructor keeps the backbone selection and hands everything else to ``MMRCAEngine._build``; ``forward`` / ``backward`` use the
base's step preamble and reach the backbone through ``_encoder_forward`` / ``_encoder_backward``, the pair a subclass with an encoder
of its own (mobilebert_engine) overrides.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import lib as L
from . import spec as S
from .conv_engine import CLASSIFIER_CONV_MODELS, CONV_MODELS
from .engine import MMRCAEngine, TextPack, parse_dtype

IMAGE_MODELS = tuple(S.VISION_SPECS) + ("eff_v2_medium", "eff_v2_large", "shuffle_net") + tuple(CLASSIFIER_CONV_MODELS)
_CONV = set(CONV_MODELS) | set(CLASSIFIER_CONV_MODELS)
TEXT_MODELS = tuple(S.TEXT_SPECS)


class ClassifierEngine(MMRCAEngine):
    """Owns parameters, gradients and activations of one single-backbone classifier replica on one GPU.  A subclass with an encoder of
    its own (MobileBertEngine) overrides ``_encoder_forward`` / ``_encoder_backward``."""

    OVERLAP_ENCODERS = False
    PATH_NAME = "classifier"
    ENCODER_WORD = "backbone"

    def __init__(self, backbone: str, n_classes: int = 4, dtype="bf16x3f", device="cuda", image_size: int = 224,
                 gemm_impl: int = L.IMPL_AUTO, attn_impl: int = L.IMPL_AUTO):
        """dtype: the four modes of MMRCAEngine (bf16 | fp32 | bf16x3 | bf16x3f, conv backbones in bf16 under bf16x3f)."""
        L.load()
        mode_flags = parse_dtype(dtype)
        if backbone in S.TEXT_SPECS:
            self.kind = "text"
        elif backbone in S.VISION_SPECS or backbone in _CONV:
            self.kind = "image"
        else:
            raise ValueError(f"Invalid Model: {backbone}")
        self.backbone = backbone
        if not 1 <= int(n_classes) <= 16:
            raise ValueError(f"n_classes must be in [1, 16], got {n_classes}")
        self.reverse, self.mode = True, 0
        self._build(mode_flags, device, int(n_classes), gemm_impl, attn_impl, S.TEXT_SPECS.get(backbone),
                    backbone if self.kind == "image" else None, image_size)

    def _head_entries(self):
        self.feat_dim = self.d_txt or self.d_img
        return [("head.weight", (self.n_classes, self.feat_dim)), ("head.bias", (self.n_classes,))]

    # ------------------------------------------------------------------ whole model
    def _encoder_forward(self, ids, mask, images, save, enc_drop_p, seed, text_pack, bn_train, taps):
        """-> (feature [B, feat_dim] in whatever dtype the backbone produced it, what ``_encoder_backward`` reads back)"""
        if self.kind == "text":
            return self._text_forward(ids, mask, save, enc_drop_p, seed, text_pack, taps)
        if self.conv is not None:
            return self.conv.forward(images, save, bn_train, seed), None
        return self._vision_forward(images, save)

    def _encoder_backward(self, dfeat, esv):
        if self.kind == "text":
            self._text_backward(dfeat, esv)
        else:
            self._image_backward(dfeat, esv)

    def forward(self, ids, mask, images=None, drop_p: float = 0.0, seed: int = 0, save: bool = True, enc_drop_p: float = 0.0,
                text_pack: Optional[TextPack] = None, bn_train: bool = False, taps=None):
        """image models read `images` fp32 [B,3,H,W], text models `ids` / `mask` int64 [B,T] (the other inputs are ignored; None is fine)
        -> logits fp32 [B, n_classes].  drop_p: the dropout in front of the Linear; enc_drop_p: the text encoder's own dropout.
        taps (text models): ``hidden_states`` indices whose class-token rows [B, D] are kept as ``last_taps[n]``."""
        self._check_resident(*(((images, "images"),) if self.kind == "image" else ((ids, "input ids"), (mask, "attention mask"))))
        self._begin_step()
        feat, esv = self._encoder_forward(ids, mask, images, save, enc_drop_p, int(seed), text_pack, bn_train, taps)
        self.last_taps = esv["taps"] if self.kind == "text" else {}
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
        train_enc = bool(train_text if self.kind == "text" else train_image)
        sv, dl = self._begin_backward(dlogits, train_enc)
        B, feat = sv["B"], sv["feat"]
        dfeat = torch.empty(B, self.feat_dim, dtype=feat.dtype, device=self.device) if train_enc else None
        L.linear_cls_bwd(dl, feat, feat.stride(0), self.arena.view("head.weight"), self.arena.view("head.weight", "g"),
                         self.arena.view("head.bias", "g"), dfeat, B, self.feat_dim, self.n_classes, sv["drop_p"], sv["seed"],
                         L.dtype_code(feat.dtype))
        self._ready("head", flush=not train_enc)
        if train_enc:
            self._encoder_backward(dfeat, sv["enc"])
        self.arena.lp_valid = False

    def trainable_spans(self, train_text: bool, train_image: bool = False):
        """[lo, hi) slices an optimizer step / all-reduce covers: the whole arena, or the head alone while the backbone is frozen"""
        train_enc = train_text if self.kind == "text" else train_image
        return [(0, self.arena.total)] if train_enc else [(self.groups["head"][0], self.arena.total)]
