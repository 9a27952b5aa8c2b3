"""Single-modality classifiers on the HIP path: drop-ins for the reference's image models (models.py: ``VisionB16``, ``VisionL16``,
``EffNetV2_M``, ``EffNetV2_L``, ``ShuffleNetV2``) and text models (CVPR_code/text_models.py: ``DistilBert``, ``Bert``, ``Roberta``,
``MobileBert``).

Each factory returns a module whose arithmetic runs in :class:`~garbage_classification_rca_amd.classifier_engine.ClassifierEngine`
(one backbone + ``mmrca_linear_cls_*``).  ``forward(images)`` / ``forward(_input_ids, _attention_mask)`` returns fp32 logits through one
autograd node (``loss.backward()`` runs the HIP backward and accumulates into ``param.grad``, views of the flat gradient arena).
``state_dict()`` keys are the reference modules' own, so a checkpoint loads into torchvision / transformers with ``strict=True``:

* ViT: torchvision's ``vit_b_16`` / ``vit_l_16`` keys, head ``heads.head.*``;
* EfficientNetV2: ``features.0`` .. ``features.8`` (BatchNorm buffers included), head ``classifier.1.*``;
* ShuffleNetV2: ``conv1``, ``stage2`` .. ``stage4``, ``conv5``, head ``fc.*``;
* MobileNetV3-Large: ``features.0`` .. ``features.16`` and ``classifier.0`` (BatchNorm buffers included), head ``classifier.3.*``;
* text: ``model.<transformers keys>`` (RoBERTa's unused ``model.pooler`` included, as ``RobertaModel`` builds it), head ``out.*``;
* MobileBERT: ``model.mobilebert.*`` and the head ``model.classifier.*`` -- ``MobileBertForSequenceClassification``'s own keys under
  the reference's attribute ``model`` (mobilebert_engine.py; fp32 or bf16, no dropout in front of the head).

What the head sees (models.py / text_models.py): ViT the ``encoder.ln`` output of the class token, no dropout (torchvision's ``heads`` is
a Linear alone); EfficientNetV2 the average-pooled ``features.8`` output behind ``classifier[0] = Dropout(0.3 / 0.4)``; ShuffleNetV2 the
mean-pooled ``conv5`` output, no dropout; MobileNetV3-Large the hard-swish of ``classifier.0`` (Linear 960 -> 1280 on the pooled
``features.16`` output) behind ``Dropout(0.2)``; text models ``last_hidden_state[:, 0]`` behind ``Dropout(drop_ratio)``, with the encoders'
own dropout of 0.1 in train mode.

Freezing follows the reference: an image model with ``transfer_learning=True`` freezes its backbone (the head stays trainable), a text
model always freezes its encoder in the constructor.  No pretrained weights can be fetched here: parameters are initialised as
``MM_RCA`` initialises them (engine.init_parameters).  Additive keyword arguments: ``dtype`` (the ``MM_RCA`` modes, default
``"bf16x3f"``), ``device``, ``init_seed``, and ``image_size`` for the conv backbones (default 480 EfficientNetV2, 320 MobileNetV3, 224 else).
"""
from __future__ import annotations

import re
from typing import Dict, Optional

import torch

from . import spec as S
from .classifier_engine import ClassifierEngine
from .multimodal_model import HashingTokenizer, ParamTree, _EngineFunction

# dropout in front of the Linear (torchvision efficientnet_v2_m / _l: classifier = Sequential(Dropout(p), Linear))
# (mobilenet_v3_large: classifier = Sequential(Linear(960, 1280), Hardswish, Dropout(0.2), Linear) -- the first two are the backbone's)
IMAGE_HEAD_DROPOUT = {"transformer_B16": 0.0, "transformer_L16": 0.0, "eff_v2_medium": 0.3, "eff_v2_large": 0.4, "shuffle_net": 0.0, "mb": 0.2}
HEAD_NAME = {"transformer_B16": "heads.head", "transformer_L16": "heads.head", "eff_v2_medium": "classifier.1",
             "eff_v2_large": "classifier.1", "shuffle_net": "fc", "mb": "classifier.3", "distilbert": "out", "bert": "out", "roberta": "out",
             "mobile_bert": "model.classifier"}
DEFAULT_IMAGE_SIZE = {"eff_v2_medium": 480, "eff_v2_large": 480, "mb": 320}      # (main_image.py: the reference's input sizes; others 224)
# the EfficientNetV2 extractor's attribute names (conv_engine.py, the MM_RCA checkpoint names) -> torchvision's `features` index
_EFF_FEATURES = {"stem.0": "features.0", "stem.1": "features.1", "stage1": "features.2", "stage2": "features.3", "stage3": "features.4",
                 "stage4": "features.5", "stage5": "features.6", "stage6": "features.7", "final_conv": "features.8"}
_EFF_RE = re.compile(r"^(stem\.[01]|stage\d|final_conv)\.")
TOKENIZER_NAMES = {"bert": "bert-base-uncased", "distilbert": "distilbert-base-uncased", "roberta": "roberta-base",
                   "mobile_bert": "google/mobilebert-uncased"}


def external_name(backbone: str, key: str) -> str:
    """engine arena / buffer key -> the reference module's state_dict key"""
    if key.startswith("head."):
        return HEAD_NAME[backbone] + key[len("head"):]
    if key.startswith("text_model."):
        return "model." + key[len("text_model."):]
    if key.startswith("image_model."):
        key = key[len("image_model."):]
    if backbone in ("eff_v2_medium", "eff_v2_large"):
        m = _EFF_RE.match(key)
        if m is None:
            raise KeyError(f"unexpected EfficientNetV2 key {key}")
        return _EFF_FEATURES[m.group(1)] + key[m.end(1):]
    return key


class SingleBackboneClassifier(torch.nn.Module):
    """One backbone + Linear head on the HIP path.  ``kind`` is "image" or "text"."""

    def __init__(self, backbone: str, n_classes: int = 4, head_dropout: float = 0.0, freeze_backbone: bool = False,
                 dtype="bf16x3f", device="cuda", init_seed: int = 0, image_size: Optional[int] = None):
        super().__init__()
        if isinstance(dtype, str) and dtype.lower() in ("bf16", "fp32", "f32"):
            dtype = torch.bfloat16 if dtype.lower() == "bf16" else torch.float32
        self.backbone = backbone
        if backbone in S.VISION_SPECS:
            self.image_size = S.VISION_SPECS[backbone].image
        else:
            self.image_size = int(image_size or DEFAULT_IMAGE_SIZE.get(backbone, 224))
        self.engine = self._make_engine(backbone, n_classes, dtype, device)
        self.engine.init_parameters(init_seed)
        self.kind, self.n_classes = self.engine.kind, n_classes
        self.drop_ratio = float(head_dropout)
        self.enc_dropout = 0.1 if self.kind == "text" else 0.0    # HF encoders' hidden / attention dropout; torchvision's ViT has none
        self._fwd_count, self._drop_seed = 0, 0x5EED
        ar = self.engine.arena
        self._arena_params: Dict[str, torch.nn.Parameter] = {}
        for k in self.engine.param_keys:
            p = torch.nn.Parameter(ar.view(k))
            self._arena_params[k] = p
            self._add(external_name(backbone, k), p, param=True)
            if not k.startswith("head.") and freeze_backbone:
                p.requires_grad = False
        self._attach_grads()
        if self.engine.conv is not None:
            for k, t in self.engine.conv.buffers.items():
                self._add(external_name(backbone, k), t, param=False)
        if backbone == "roberta":
            # RobertaModel builds a pooler (add_pooling_layer=True) that the classifier never reads: present for checkpoint
            # interchange, outside the arena, never receives a gradient (as in the reference, whose loss does not reach it)
            d = self.engine.ts.dim
            g = torch.Generator().manual_seed(init_seed + 1)
            self._add("model.pooler.dense.weight", torch.nn.Parameter((torch.randn(d, d, generator=g) * 0.02).to(device)), param=True)
            self._add("model.pooler.dense.bias", torch.nn.Parameter(torch.zeros(d, device=device)), param=True)
            if freeze_backbone:
                self.model.pooler.dense.weight.requires_grad = False
                self.model.pooler.dense.bias.requires_grad = False
        self._anchor = torch.zeros(1, device=device, requires_grad=True)

    def _make_engine(self, backbone, n_classes, dtype, device):
        return ClassifierEngine(backbone, n_classes, dtype, device, image_size=self.image_size)

    def _add(self, dotted, t, param):
        node = self
        parts = dotted.split(".")
        for name in parts[:-1]:
            if name not in node._modules:
                node.add_module(name, ParamTree())
            node = node._modules[name]
        if param:
            node.register_parameter(parts[-1], t)
        else:
            node.register_buffer(parts[-1], t)

    def _attach_grads(self):
        for k, p in self._arena_params.items():
            p.grad = self.engine.arena.view(k, "g")

    # ------------------------------------------------------------------ reference API
    def get_tokenizer(self):
        """text_models.py: the model's HF tokenizer; the offline hashing tokenizer when its files are not cached (no network)."""
        if self.kind != "text":
            raise AttributeError("image classifiers have no tokenizer")
        name = TOKENIZER_NAMES[self.backbone]
        try:
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(name, local_files_only=True)
        except Exception as e:
            print(f"[mmrca] tokenizer files for {name} unavailable ({type(e).__name__}); using the offline HashingTokenizer")
            self.tokenizer = HashingTokenizer(self.engine.ts.vocab, model_max_length=self.get_max_token_size())
        return self.tokenizer

    def get_max_token_size(self):
        """text_models.py: ``<Config>().max_position_embeddings`` -- 512 for all three (RobertaConfig()'s default, not roberta-base's 514)"""
        if self.kind != "text":
            raise AttributeError("image classifiers have no token size")
        return 512

    def get_image_size(self):
        return (self.image_size, self.image_size)

    # ------------------------------------------------------------------ what training.py drives (hip_train_step / GraphedTrainStep)
    def _train_flags(self):
        enc = next(p for k, p in self._arena_params.items() if not k.startswith("head.")).requires_grad
        return (enc, False) if self.kind == "text" else (False, enc)

    def drop_modalities(self, _eval, remove_image, remove_text):
        """one modality: nothing to drop (the MM_RCA step calls this between staging a batch and launching it)"""

    def _engine_backward(self, dlogits):
        if any(p.grad is None for p in self._arena_params.values()):
            self.engine.arena.g.zero_()        # optimizer.zero_grad(set_to_none=True) dropped the views
            self._attach_grads()
        tt, ti = self._train_flags()
        self.engine.backward(dlogits, train_text=tt, train_image=ti)

    def load_state_dict(self, state_dict, strict=True, **kw):
        r = super().load_state_dict(state_dict, strict=strict, **kw)
        self.engine.arena.lp_valid = False
        conv = self.engine.conv
        if conv is not None:                   # num_batches_tracked continues from the loaded count
            for k, t in conv.buffers.items():
                if k.endswith("num_batches_tracked"):
                    conv._nbt_base[k] = int(t) - conv.n_train_forwards
        return r

    def state_dict(self, *a, **kw):
        if self.engine.conv is not None:
            self.engine.conv.sync_buffers()
        return super().state_dict(*a, **kw)

    def _apply(self, fn, *a, **kw):
        # parameters live in the engine's arenas: .to() / .cuda() / .cpu() would detach them (save_model_weights' model.to("cpu")
        # round trip becomes a no-op; state_dict() tensors are copied out instead)
        return self

    def _run(self, ids, mask, images):
        self._fwd_count += 1
        tt, ti = self._train_flags()
        return _EngineFunction.apply(self._anchor, self, ids, mask, images, self.drop_ratio if self.training else 0.0,
                                     self._drop_seed + self._fwd_count, bool(torch.is_grad_enabled() and (tt or ti)),
                                     self.enc_dropout if self.training else 0.0)


class ImageClassifier(SingleBackboneClassifier):
    def forward(self, images):
        return self._run(None, None, images)


class TextClassifier(SingleBackboneClassifier):
    def forward(self, _input_ids, _attention_mask):
        return self._run(_input_ids, _attention_mask, None)


def _image(backbone, num_classes, transfer_learning, kw):
    return ImageClassifier(backbone, num_classes, IMAGE_HEAD_DROPOUT[backbone], bool(transfer_learning), **kw)


def VisionB16(num_classes=4, transfer_learning=False, **kw):
    """models.py VisionB16: torchvision vit_b_16, heads.head = Linear(768, num_classes)"""
    return _image("transformer_B16", num_classes, transfer_learning, kw)


def VisionL16(num_classes=4, transfer_learning=False, **kw):
    """models.py VisionL16: torchvision vit_l_16, heads.head = Linear(1024, num_classes)"""
    return _image("transformer_L16", num_classes, transfer_learning, kw)


def EffNetV2_M(num_classes=4, transfer_learning=False, **kw):
    """models.py EffNetV2_M: torchvision efficientnet_v2_m, classifier = (Dropout(0.3), Linear(1280, num_classes))"""
    return _image("eff_v2_medium", num_classes, transfer_learning, kw)


def EffNetV2_L(num_classes=4, transfer_learning=False, **kw):
    """models.py EffNetV2_L: torchvision efficientnet_v2_l, classifier = (Dropout(0.4), Linear(1280, num_classes))"""
    return _image("eff_v2_large", num_classes, transfer_learning, kw)


def ShuffleNetV2(num_classes=4, transfer_learning=False, **kw):
    """models.py ShuffleNetV2: torchvision shufflenet_v2_x2_0, fc = Linear(2048, num_classes)"""
    return _image("shuffle_net", num_classes, transfer_learning, kw)


def MBNetLarge(num_classes=4, transfer_learning=False, **kw):
    """models.py MBNetLarge: torchvision mobilenet_v3_large, classifier[3] = Linear(1280, num_classes) behind Dropout(0.2); the
    transfer-learning freeze covers features.* and classifier.0 (the backbone), the head classifier.3 stays trainable"""
    return _image("mb", num_classes, transfer_learning, kw)


def DistilBert(n_classes, drop_ratio, **kw):
    """text_models.py DistilBert: DistilBertModel (frozen), Dropout(drop_ratio), out = Linear(768, n_classes)"""
    return TextClassifier("distilbert", n_classes, drop_ratio, True, **kw)


def Bert(n_classes, drop_ratio, **kw):
    """text_models.py Bert: BertModel (frozen), Dropout(drop_ratio), out = Linear(768, n_classes)"""
    return TextClassifier("bert", n_classes, drop_ratio, True, **kw)


def Roberta(n_classes, drop_ratio, **kw):
    """text_models.py Roberta: RobertaModel (frozen), Dropout(drop_ratio), out = Linear(768, n_classes)"""
    return TextClassifier("roberta", n_classes, drop_ratio, True, **kw)


class MobileBertClassifier(TextClassifier):
    """the same module over :class:`~garbage_classification_rca_amd.mobilebert_engine.MobileBertEngine`"""

    def __init__(self, *a, spec=None, **kw):
        object.__setattr__(self, "_spec", spec)         # (tests build shallow models: a MobileBertSpec with fewer layers)
        super().__init__(*a, **kw)

    def _make_engine(self, backbone, n_classes, dtype, device):
        from .mobilebert_engine import MOBILEBERT, MobileBertEngine
        return MobileBertEngine(n_classes, dtype, device, spec=self._spec or MOBILEBERT)


def MobileBERT(n_classes, dtype="fp32", **kw):
    """text_models.py MobileBert: MobileBertForSequenceClassification (frozen) with classifier = Linear(512, n_classes), trainable; no
    dropout argument (the model's classifier dropout is 0).  dtype: "fp32" (default, the compliant mode) or "bf16"."""
    return MobileBertClassifier("mobile_bert", n_classes, 0.0, True, dtype=dtype, **kw)


IMAGE_FACTORIES = {"transformer_B16": VisionB16, "transformer_L16": VisionL16, "eff_v2_medium": EffNetV2_M, "eff_v2_large": EffNetV2_L,
                   "shuffle_net": ShuffleNetV2, "mb": MBNetLarge}
TEXT_FACTORIES = {"distilbert": DistilBert, "bert": Bert, "roberta": Roberta, "mobile_bert": MobileBERT}


def build_text_classifier(name, n_classes, model_dropout, dtype, device):
    """what main_text.py / calculate_test_accuracy_text.py construct for --text_model=name: the reference's call per model
    (``MobileBERT(n)`` takes no dropout).  MobileBERT has no split-bf16 mode: under the scripts' default --dtype it runs in fp32."""
    if name == "mobile_bert":
        if isinstance(dtype, str) and dtype.lower() not in ("fp32", "f32", "bf16"):
            print("mobile_bert: --dtype {} is not built for this model; using fp32 (pass --dtype bf16 for the bf16 mode)".format(dtype))
            dtype = "fp32"
        return MobileBERT(n_classes, dtype=dtype, device=device)
    return TEXT_FACTORIES[name](n_classes, model_dropout, dtype=dtype, device=device)
