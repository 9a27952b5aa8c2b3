"""Two backbones + the hierarchical late-fusion head over libmmrca: the engine of ``multimodal_model.Hierarchical`` (the reference's
``Hierarchical.forward``, CVPR_code/multimodal_model.py:729-818, launched by slurm_files/multimodal/hierarchical_fusion.sh).

The encoders are :class:`~garbage_classification_rca_amd.engine.MMRCAEngine`'s own (``_text_forward`` / ``_text_backward`` with class-token
taps at ``hidden_states[2]`` and ``[4]``; :class:`~garbage_classification_rca_amd.conv_engine.ConvEncoder` with pooled taps behind
``stage3`` and ``stage6``) over the arena

    text_model.* | image_model.* | final_hierarchical_image | final_hierarchical_text | final_hierarchical_all

The head (csrc/hier_head.hip + ``mmrca_linear_cls_*``) is fp32 in every ``dtype`` mode:

    raw [B, 8192] = f 1280 | AvgPool7(stage3) 2560 | AvgPool6(stage6) 2048 | t0 768 | t2 768 | t4 768
    x = dropout(each segment / its L2 norm)           xi = x[:, :5888] and xt = x[:, 5888:] draw independent masks
    h = relu(xi Wi^T + bi) | relu(xt Wt^T + bt)       [B, 1024]
    logits = h Wa^T + ba

Same ``forward`` / ``backward`` / ``trainable_spans`` / ``groups`` contract as the MM-RCA engine, so the flat optimizers, ``GradSync`` and
``hip_train_step`` drive it unchanged.  The text encoder and the image encoder run one after the other on the caller's stream: the
two-stream overlap of the MM-RCA engine is not used here (the taps would need cross-stream hand-overs at two more points per encoder).

The constructor keeps the configuration guard and hands the rest to ``MMRCAEngine._build`` (the segment offsets and the head keys
come from the ``_head_entries`` hook); ``forward`` / ``backward`` stay this class's own, because the taps land in the head's ``raw``
buffer between the encoders, and start with the base's ``_check_resident`` / ``_begin_step`` / ``_begin_backward``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import lib as L
from . import spec as S
from .engine import MMRCAEngine, TextPack, parse_dtype

HIER_IMAGE_MODELS = ("eff_v2_medium", "EffNetv2-Medium")
HIER_HIDDEN = 512
HIER_TEXT_TAPS = (2, 4)                     # hidden_states indices, for every text model (as the reference)
HIER_STAGES = (("stage3", 7, 160, 2560), ("stage6", 6, 512, 2048))       # (tap, AvgPool2d window, channels, width the Linear expects)


def stage_map_sizes(image_size: int) -> Tuple[int, int]:
    """side of EfficientNetV2-M's stage3 / stage6 output maps: four / five stride-2 3x3 convolutions with padding 1"""
    s = int(image_size)
    sides = []
    for n in range(5):
        s = (s - 1) // 2 + 1
        sides.append(s)
    return sides[3], sides[4]


def check_hierarchical_config(text_model: str, image_model: str, image_size: int):
    """the three linears fix the configuration; anything else fails here, naming the offending value"""
    if image_model not in HIER_IMAGE_MODELS:
        raise ValueError(f"Wrong image model for late_fusion=hierarchical: {image_model!r} (final_hierarchical_image is built for "
                         f"EfficientNetV2-M's stage maps; use eff_v2_medium)")
    if text_model not in S.TEXT_SPECS:
        raise ValueError(f"Wrong text model: {text_model}")
    if S.TEXT_SPECS[text_model].dim != 768:
        raise ValueError(f"Wrong text model for late_fusion=hierarchical: {text_model!r} is {S.TEXT_SPECS[text_model].dim} wide, "
                         f"final_hierarchical_text expects 3 x 768 features")
    h3, h6 = stage_map_sizes(image_size)
    for (name, k, c, want), side in zip(HIER_STAGES, (h3, h6)):
        got = c * (side // k) ** 2
        if got != want:
            raise ValueError(f"Wrong image size for late_fusion=hierarchical: {image_size} gives a {side} x {side} {name} map, which "
                             f"AvgPool2d({k}) turns into {got} features where final_hierarchical_image expects {want} "
                             f"(448, 480 and 512 fit)")


class HierarchicalEngine(MMRCAEngine):
    """Owns parameters, gradients and activations of one hierarchical-fusion replica on one GPU."""

    OVERLAP_ENCODERS = False
    PATH_NAME = "hierarchical"

    def __init__(self, text_model: str, image_model: str = "eff_v2_medium", n_classes: int = 4, dtype="bf16x3f", device="cuda",
                 image_size: int = 480, gemm_impl: int = L.IMPL_AUTO, attn_impl: int = L.IMPL_AUTO):
        """dtype: the four modes of MMRCAEngine (bf16 | fp32 | bf16x3 | bf16x3f; the conv backbone runs bf16 under bf16x3f).  The head
        is fp32 in all of them."""
        check_hierarchical_config(text_model, image_model, image_size)
        if not 1 <= int(n_classes) <= 16:
            raise ValueError(f"n_classes must be in [1, 16], got {n_classes}")
        L.load()
        self.reverse, self.mode = True, 0
        self._build(parse_dtype(dtype), device, int(n_classes), gemm_impl, attn_impl, S.TEXT_SPECS[text_model], image_model, image_size)

    def _head_entries(self):
        # columns of raw / x: f | pool(stage3) | pool(stage6) | t0 | t2 | t4
        widths = [self.d_img] + [w for _, _, _, w in HIER_STAGES] + [self.d_txt] * 3
        self.seg_off = [0]
        for w in widths:
            self.seg_off.append(self.seg_off[-1] + w)
        self.n_img_segs = 1 + len(HIER_STAGES)
        self.w_img, self.w_all = self.seg_off[self.n_img_segs], self.seg_off[-1]
        self.w_txt = self.w_all - self.w_img
        return [("final_hierarchical_image.weight", (HIER_HIDDEN, self.w_img)), ("final_hierarchical_image.bias", (HIER_HIDDEN,)),
                ("final_hierarchical_text.weight", (HIER_HIDDEN, self.w_txt)), ("final_hierarchical_text.bias", (HIER_HIDDEN,)),
                ("final_hierarchical_all.weight", (self.n_classes, 2 * HIER_HIDDEN)), ("final_hierarchical_all.bias", (self.n_classes,))]

    def _hbuf(self, name, B, cols):
        return self.buf("hier_" + name, B, cols, torch.float32)

    def _linear_ws(self, B):
        need = L.hier_linear_workspace_bytes(B, HIER_HIDDEN, self.w_img)
        key = ("hier_ws", need)
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return t

    # ------------------------------------------------------------------ whole model
    def forward(self, ids, mask, images, drop_p: float = 0.0, seed: int = 0, save: bool = True, enc_drop_p: float = 0.0,
                text_pack: Optional[TextPack] = None, bn_train: bool = False):
        """ids/mask int64 [B,T] and images fp32 [B,3,H,W] in HBM -> logits fp32 [B, n_classes].  drop_p: the dropout on xi and on xt."""
        self._check_resident((ids, "input ids"), (mask, "attention mask"), (images, "images"))
        if images.shape[-1] != self.conv.image or images.shape[-2] != self.conv.image:
            raise ValueError(f"images must be [B,3,{self.conv.image},{self.conv.image}], got {tuple(images.shape)}")
        self._begin_step()
        B, ld, so = ids.shape[0], self.w_all, self.seg_off
        raw, x, h = self._hbuf("raw", B, ld), self._hbuf("x", B, ld), self._hbuf("h", B, 2 * HIER_HIDDEN)
        inv = self._hbuf("inv", B, len(so) - 1)
        cls, tsv = self._text_forward(ids, mask, save, enc_drop_p, int(seed), text_pack, taps=HIER_TEXT_TAPS)
        taps = {name: (k, raw[:, so[1 + j]:], ld) for j, (name, k, _, _) in enumerate(HIER_STAGES)}
        feat = self.conv.forward(images, save, bn_train, int(seed), taps=taps)
        L.hier_pool_fwd(feat, raw, ld, B, 1, 1, self.d_img, 1, L.dtype_code(feat.dtype))
        for j, rows in enumerate([cls] + [tsv["taps"][n] for n in HIER_TEXT_TAPS]):
            L.hier_pool_fwd(rows, raw[:, so[self.n_img_segs + j]:], ld, B, 1, 1, self.d_txt, 1, L.dtype_code(rows.dtype))
        # the same seed stride per step as the encoders' site seeds: replay r of a captured step draws eager step seed + r's masks
        seed_i, seed_t = self._site_seed(int(seed), 255, 0), self._site_seed(int(seed), 255, 1)
        L.hier_norm_fwd(raw, x, inv, B, ld, so, self.n_img_segs, float(drop_p), seed_i, seed_t)
        ws = self._linear_ws(B)
        A = self.arena.view
        L.hier_linear_relu_fwd(x, ld, A("final_hierarchical_image.weight"), A("final_hierarchical_image.bias"), h, 2 * HIER_HIDDEN, ws,
                               B, HIER_HIDDEN, self.w_img)
        L.hier_linear_relu_fwd(x[:, self.w_img:], ld, A("final_hierarchical_text.weight"), A("final_hierarchical_text.bias"), h[:, HIER_HIDDEN:],
                               2 * HIER_HIDDEN, ws, B, HIER_HIDDEN, self.w_txt)
        logits = torch.empty(B, self.n_classes, dtype=torch.float32, device=self.device)
        L.linear_cls_fwd(h, 2 * HIER_HIDDEN, A("final_hierarchical_all.weight"), A("final_hierarchical_all.bias"), logits, B, 2 * HIER_HIDDEN,
                         self.n_classes, 0.0, 0, L.F32)
        self._saved = dict(B=B, raw=raw, x=x, h=h, inv=inv, text=tsv, drop_p=float(drop_p), seeds=(seed_i, seed_t), full=save)
        return logits

    def backward(self, dlogits, train_text: bool = True, train_image: bool = True):
        """accumulates into the gradient arena: the three head linears always, each backbone when its flag is set"""
        sv, dl = self._begin_backward(dlogits, train_text or train_image)
        B, ld, so, x, h = sv["B"], self.w_all, self.seg_off, sv["x"], sv["h"]
        A, H2 = self.arena.view, 2 * HIER_HIDDEN
        dh = self._hbuf("dh", B, H2)
        L.linear_cls_bwd(dl, h, H2, A("final_hierarchical_all.weight"), A("final_hierarchical_all.weight", "g"),
                         A("final_hierarchical_all.bias", "g"), dh, B, H2, self.n_classes, 0.0, 0, L.F32)
        dxc, ws = self._hbuf("dx", B, ld), self._linear_ws(B)
        L.hier_linear_relu_bwd(dh, H2, h, H2, x, ld, A("final_hierarchical_image.weight"), A("final_hierarchical_image.weight", "g"),
                               A("final_hierarchical_image.bias", "g"), dxc if train_image else None, ld, ws, B, HIER_HIDDEN, self.w_img)
        L.hier_linear_relu_bwd(dh[:, HIER_HIDDEN:], H2, h[:, HIER_HIDDEN:], H2, x[:, self.w_img:], ld, A("final_hierarchical_text.weight"),
                               A("final_hierarchical_text.weight", "g"), A("final_hierarchical_text.bias", "g"),
                               dxc[:, self.w_img:] if train_text else None, ld, ws, B, HIER_HIDDEN, self.w_txt)
        self._ready("head", flush=not (train_image or train_text))
        if train_image or train_text:
            draw = self._hbuf("draw", B, ld)
            # (all six segments in one launch; the half whose backbone is frozen holds a stale gradient nobody reads)
            L.hier_norm_bwd(dxc, sv["raw"], sv["inv"], draw, B, ld, so, self.n_img_segs, sv["drop_p"], *sv["seeds"])
            if train_image:
                dtaps = {name: (draw[:, so[1 + j]:], ld) for j, (name, _, _, _) in enumerate(HIER_STAGES)}
                self.conv.backward(draw[:B, :self.d_img], dtaps=dtaps)
                self._ready("image_emb", flush=True)
            if train_text:
                t0 = so[self.n_img_segs]
                dtaps = {n: draw[:B, so[self.n_img_segs + 1 + j]: so[self.n_img_segs + 2 + j]] for j, n in enumerate(HIER_TEXT_TAPS)}
                self._text_backward(draw[:B, t0: t0 + self.d_txt].to(self.dtype), sv["text"], dtaps=dtaps)
        self.arena.lp_valid = False
