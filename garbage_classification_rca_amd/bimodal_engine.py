"""Two backbones + the bimodal GRU late-fusion head over libmmrca: the engine of ``multimodal_model.HierarchicalBimodalFusion`` (the
reference's forward of that name, CVPR_code/multimodal_model.py:835-888, selected by ``--late_fusion=bimodal``, main_both.py:328-340).

The encoders are :class:`~garbage_classification_rca_amd.engine.MMRCAEngine`'s own, every backbone it takes and any image size: the
head reads the text class token and the pooled image feature only.  The arena is

    text_model.* | image_model.* | modality_text_to_dim | modality_image_to_dim | gru_text | gru_audio | fusion | gru_bimodal |
    concat_fc | classifier

The head (csrc/gru.hip + ``mmrca_hier_norm_*``) is fp32 in every ``dtype`` mode:

    x = t / |t|  |  f / |f|                                          [B, d_txt + d_img]
    x_text = modality_text_to_dim(t / |t|)    x_image = modality_image_to_dim(f / |f|)        [B, 400]
    ctx_text = gru_text(x_text)               ctx_audio = gru_audio(x_image)                  [B, 400]
    fused = tanh(ctx_text * kernel1 + ctx_audio * kernel2 + bias)                             [B, 400]
    ctx_fused = gru_bimodal(fused)                                                            [B, 500]
    proj = dropout2(relu(concat_fc(fused | dropout1(ctx_fused))))                             [B, 450]
    logits = classifier(proj)                                                                 [B, 4]

**The GRUs run over the batch.**  Each receives a 2-D tensor, which torch reads as ONE unbatched sequence of length T = B: row b of
the batch is time step b, h_{-1} = 0, so sample b's logits depend on samples 0 .. b - 1 and permuting the batch changes them.  That
is the reference's behaviour and it is reproduced here; under data parallelism every rank runs the recurrence over its own local
batch.  ``drop_p`` of ``forward`` is the probability of dropout1 and dropout2 (the module passes the reference's fixed 0.86 in train
mode; ``--model_dropout`` has no effect on this forward, and ``gru_bimodal``'s ``dropout=0.35`` none on a single layer).

``forward`` / ``backward`` / ``trainable_spans`` / ``groups`` ARE the MM-RCA engine's (constructor, two-stream encoders and step
preamble inherited); this class supplies the head through the hooks ``_head_entries``, ``_head_forward`` and ``_head_grads``.  So the
flat optimizers, ``GradSync``, ``hip_train_step`` and ``GraphedTrainStep`` drive it unchanged.
"""
from __future__ import annotations

import math
import torch

from . import lib as L
from .engine import MMRCAEngine

BIMODAL_DIM, BIMODAL_HIDDEN, BIMODAL_PROJ, BIMODAL_CLASSES = 400, 500, 450, 4      # multimodal_model.py:302-305 (num_classes = 4 is hard-coded)
BIMODAL_DROPOUT = 0.86                                                              # dropout1 / dropout2, whatever --model_dropout says
GRUS = (("gru_text", BIMODAL_DIM, BIMODAL_DIM), ("gru_audio", BIMODAL_DIM, BIMODAL_DIM), ("gru_bimodal", BIMODAL_DIM, BIMODAL_HIDDEN))


def _gru_entries(name, n_in, hid):
    return [(f"{name}.weight_ih_l0", (3 * hid, n_in)), (f"{name}.weight_hh_l0", (3 * hid, hid)),
            (f"{name}.bias_ih_l0", (3 * hid,)), (f"{name}.bias_hh_l0", (3 * hid,))]


class BimodalEngine(MMRCAEngine):
    """Owns parameters, gradients and activations of one bimodal-fusion replica on one GPU.  ``forward`` / ``backward`` are the base
    engine's: the two-stream encoders around this class's ``_head_forward`` / ``_head_grads``."""

    PATH_NAME = "bimodal"

    def __init__(self, text_model: str, image_model: str = "eff_v2_medium", n_classes: int = 4, dtype="bf16x3f", device="cuda",
                 image_size: int = 480, gemm_impl: int = L.IMPL_AUTO, attn_impl: int = L.IMPL_AUTO):
        """dtype: the four modes of MMRCAEngine.  The head is fp32 in all of them.  n_classes does not size anything here: the
        reference's classifier is Linear(450, 4) whatever the dataset has."""
        super().__init__(text_model, image_model, n_classes, True, 0, dtype, device, gemm_impl, attn_impl, image_size)
        self.n_logits = BIMODAL_CLASSES

    # ------------------------------------------------------------------ parameters
    def _head_entries(self):
        D, Hh, P = BIMODAL_DIM, BIMODAL_HIDDEN, BIMODAL_PROJ
        ents = [("modality_text_to_dim.weight", (D, self.d_txt)), ("modality_text_to_dim.bias", (D,)),
                ("modality_image_to_dim.weight", (D, self.d_img)), ("modality_image_to_dim.bias", (D,))]
        ents += _gru_entries(*GRUS[0]) + _gru_entries(*GRUS[1])
        ents += [("fusion.kernel1", (D,)), ("fusion.kernel2", (D,)), ("fusion.bias", (D,))]
        ents += _gru_entries(*GRUS[2])
        ents += [("concat_fc.weight", (P, D + Hh)), ("concat_fc.bias", (P,)),
                 ("classifier.weight", (BIMODAL_CLASSES, P)), ("classifier.bias", (BIMODAL_CLASSES,))]
        return ents

    def _head_struct(self, which):
        return None                            # (the MM-RCA head's pointer table: not this head)

    def init_parameters(self, seed: int = 0):
        """the encoders and the four linears as MMRCAEngine; torch's defaults for the rest: every GRU parameter U(-1/sqrt(H), 1/sqrt(H)),
        fusion.kernel1 / kernel2 standard normal, fusion.bias zero"""
        super().init_parameters(seed)
        g = torch.Generator(device="cpu").manual_seed(seed + 0x6B1)
        with torch.no_grad():
            for name, _, hid in GRUS:
                bound = 1.0 / math.sqrt(hid)
                for leaf in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                    v = self.arena.view(f"{name}.{leaf}")
                    v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) * bound)
            for leaf in ("kernel1", "kernel2"):
                v = self.arena.view("fusion." + leaf)
                v.copy_(torch.randn(v.shape, generator=g))
            self.arena.view("fusion.bias").zero_()
        self.arena.lp_valid = False

    # ------------------------------------------------------------------ head
    def _hbuf(self, name, rows, cols):
        return self.buf("bim_" + name, rows, cols, torch.float32)

    def _head_forward(self, cls, feat, B, drop_p, seeds):
        """cls [B, d_txt], feat [B, d_img] in the encoders' dtypes -> logits fp32 [B, 4]; keeps what the backward reads.  drop_p:
        dropout1's and dropout2's probability, seeds: their two mask seeds.  Row b of the batch is time step b of the three GRUs."""
        if not 0.0 <= drop_p < 1.0:
            raise ValueError(f"drop_p must be in [0, 1), got {drop_p}")
        A, D, Hh, P = self.arena.view, BIMODAL_DIM, BIMODAL_HIDDEN, BIMODAL_PROJ
        dt, di = self.d_txt, self.d_img
        ld, so = dt + di, [0, dt, dt + di]
        raw, x, inv = self._hbuf("raw", B, ld), self._hbuf("x", B, ld), self._hbuf("inv", B, 2)
        L.hier_pool_fwd(cls, raw, ld, B, 1, 1, dt, 1, L.dtype_code(cls.dtype))
        L.hier_pool_fwd(feat, raw[:, dt:], ld, B, 1, 1, di, 1, L.dtype_code(feat.dtype))
        L.hier_norm_fwd(raw, x, inv, B, ld, so, 1, 0.0, 0, 0)
        xm = self._hbuf("xm", B, 2 * D)                          # x_text | x_image
        L.gru_linear_fwd(x, ld, A("modality_text_to_dim.weight"), A("modality_text_to_dim.bias"), xm, 2 * D, B, D, dt)
        L.gru_linear_fwd(x[:, dt:], ld, A("modality_image_to_dim.weight"), A("modality_image_to_dim.bias"), xm[:, D:], 2 * D, B, D, di)
        st = {}
        for j, (name, n_in, hid) in enumerate(GRUS):
            # hseq: row 0 = h_{-1} = 0 (buf() hands out zeros and no kernel writes that row), row t + 1 = h_t
            st[name] = dict(gi=self._hbuf(name + "_gi", B, 3 * hid), hseq=self._hbuf(name + "_h", B + 1, hid),
                            gates=self._hbuf(name + "_gates", B, 3 * hid), hn=self._hbuf(name + "_hn", B, hid))
        for j, name in enumerate(("gru_text", "gru_audio")):
            L.gru_linear_fwd(xm[:, j * D:], 2 * D, A(name + ".weight_ih_l0"), A(name + ".bias_ih_l0"), st[name]["gi"], 3 * D, B, 3 * D, D)
        two = [st["gru_text"], st["gru_audio"]]
        L.gru_fwd([s["gi"] for s in two], [A("gru_text.weight_hh_l0"), A("gru_audio.weight_hh_l0")],
                  [A("gru_text.bias_hh_l0"), A("gru_audio.bias_hh_l0")], [s["hseq"] for s in two], [s["gates"] for s in two],
                  [s["hn"] for s in two], B, D)
        comb = self._hbuf("comb", B, D + Hh)                     # fused | dropout1(ctx_fused)
        L.hadamard_fwd(two[0]["hseq"][1:], D, two[1]["hseq"][1:], D, A("fusion.kernel1"), A("fusion.kernel2"), A("fusion.bias"), comb, D + Hh, B, D)
        sb = st["gru_bimodal"]
        L.gru_linear_fwd(comb, D + Hh, A("gru_bimodal.weight_ih_l0"), A("gru_bimodal.bias_ih_l0"), sb["gi"], 3 * Hh, B, 3 * Hh, D)
        L.gru_fwd([sb["gi"]], [A("gru_bimodal.weight_hh_l0")], [A("gru_bimodal.bias_hh_l0")], [sb["hseq"]], [sb["gates"]], [sb["hn"]], B, Hh)
        L.dropout_f32(sb["hseq"][1:], Hh, comb[:, D:], D + Hh, B, Hh, drop_p, seeds[0])
        h2, proj = self._hbuf("h2", B, P), self._hbuf("proj", B, P)
        L.gru_linear_fwd(comb, D + Hh, A("concat_fc.weight"), A("concat_fc.bias"), h2, P, B, P, D + Hh, relu=True)
        L.dropout_f32(h2, P, proj, P, B, P, drop_p, seeds[1])
        logits = torch.empty(B, BIMODAL_CLASSES, dtype=torch.float32, device=self.device)
        L.gru_linear_fwd(proj, P, A("classifier.weight"), A("classifier.bias"), logits, BIMODAL_CLASSES, B, BIMODAL_CLASSES, P)
        return logits, dict(raw=raw, x=x, inv=inv, xm=xm, st=st, comb=comb, h2=h2, proj=proj, drop_p=drop_p, seeds=seeds)

    def _gru_param_grads(self, name, s, x, ldx, dx, lddx, B, n_in, hid):
        """the products over all T behind the backward chain: dW_ih, db_ih, dx from dgi; dW_hh, db_hh from dgh and h_{t-1}"""
        A = self.arena.view
        L.gru_linear_bwd(s["dgi"], 3 * hid, None, 0, x, ldx, A(name + ".weight_ih_l0"), A(name + ".weight_ih_l0", "g"), A(name + ".bias_ih_l0", "g"),
                         dx, lddx, B, 3 * hid, n_in)
        L.gru_linear_bwd(s["dgh"], 3 * hid, None, 0, s["hseq"], hid, A(name + ".weight_hh_l0"), A(name + ".weight_hh_l0", "g"),
                         A(name + ".bias_hh_l0", "g"), None, 0, B, 3 * hid, hid)

    def _head_backward(self, dl, sv, B, need_dx):
        """accumulates the head's parameter gradients; returns the gradient at raw = cls | feat (fp32 [B, d_txt + d_img]) when asked"""
        A, D, Hh, P = self.arena.view, BIMODAL_DIM, BIMODAL_HIDDEN, BIMODAL_PROJ
        dt, di = self.d_txt, self.d_img
        ld, so = dt + di, [0, dt, dt + di]
        st, comb, h2, proj, xm = sv["st"], sv["comb"], sv["h2"], sv["proj"], sv["xm"]
        drop_p, seeds = sv["drop_p"], sv["seeds"]
        dproj = self._hbuf("dproj", B, P)
        L.gru_linear_bwd(dl, BIMODAL_CLASSES, None, 0, proj, P, A("classifier.weight"), A("classifier.weight", "g"), A("classifier.bias", "g"),
                         dproj, P, B, BIMODAL_CLASSES, P)
        L.dropout_f32(dproj, P, dproj, P, B, P, drop_p, seeds[1])
        dcomb = self._hbuf("dcomb", B, D + Hh)
        L.gru_linear_bwd(dproj, P, h2, P, comb, D + Hh, A("concat_fc.weight"), A("concat_fc.weight", "g"), A("concat_fc.bias", "g"),
                         dcomb, D + Hh, B, P, D + Hh)
        L.dropout_f32(dcomb[:, D:], D + Hh, dcomb[:, D:], D + Hh, B, Hh, drop_p, seeds[0])
        for name, _, hid in GRUS:
            s = st[name]
            for k, cols in (("carry", hid), ("dgi", 3 * hid), ("dgh", 3 * hid)):
                s[k] = self._hbuf(name + "_" + k, B, cols)
        sb = st["gru_bimodal"]
        L.gru_bwd([A("gru_bimodal.weight_hh_l0")], [sb["hseq"]], [sb["gates"]], [sb["hn"]], [dcomb[:, D:]], [D + Hh], [sb["carry"]], [sb["dgi"]],
                  [sb["dgh"]], B, Hh)
        dfused = self._hbuf("dfused", B, D)                      # gru_bimodal's share; concat_fc's is dcomb[:, :D]
        self._gru_param_grads("gru_bimodal", sb, comb, D + Hh, dfused, D, B, D, Hh)
        dctx = self._hbuf("dctx", B, 2 * D)                      # d ctx_text | d ctx_audio
        two = [st["gru_text"], st["gru_audio"]]
        L.hadamard_bwd(dcomb, D + Hh, dfused, D, two[0]["hseq"][1:], D, two[1]["hseq"][1:], D, comb, D + Hh, A("fusion.kernel1"), A("fusion.kernel2"),
                       dctx, 2 * D, dctx[:, D:], 2 * D, A("fusion.kernel1", "g"), A("fusion.kernel2", "g"), A("fusion.bias", "g"), B, D)
        L.gru_bwd([A("gru_text.weight_hh_l0"), A("gru_audio.weight_hh_l0")], [s["hseq"] for s in two], [s["gates"] for s in two],
                  [s["hn"] for s in two], [dctx, dctx[:, D:]], [2 * D, 2 * D], [s["carry"] for s in two], [s["dgi"] for s in two],
                  [s["dgh"] for s in two], B, D)
        dxm = self._hbuf("dxm", B, 2 * D)
        for j, name in enumerate(("gru_text", "gru_audio")):
            self._gru_param_grads(name, st[name], xm[:, j * D:], 2 * D, dxm[:, j * D:], 2 * D, B, D, D)
        x = sv["x"]
        dx = self._hbuf("dx", B, ld) if need_dx else None
        L.gru_linear_bwd(dxm, 2 * D, None, 0, x, ld, A("modality_text_to_dim.weight"), A("modality_text_to_dim.weight", "g"),
                         A("modality_text_to_dim.bias", "g"), dx, ld, B, D, dt)
        L.gru_linear_bwd(dxm[:, D:], 2 * D, None, 0, x[:, dt:], ld, A("modality_image_to_dim.weight"), A("modality_image_to_dim.weight", "g"),
                         A("modality_image_to_dim.bias", "g"), None if dx is None else dx[:, dt:], ld, B, D, di)
        if dx is None:
            return None
        draw = self._hbuf("draw", B, ld)
        L.hier_norm_bwd(dx, sv["raw"], sv["inv"], draw, B, ld, so, 1, 0.0, 0, 0)
        return draw

    def _head_grads(self, dl, sv, train_text, train_image):
        B = sv["B"]
        draw = self._head_backward(dl, sv["head"], B, train_text or train_image)
        self._ready("head", flush=not (train_image or train_text))
        dimg = draw[:B, self.d_txt:].to(self.dtype).contiguous() if train_image else None
        dtxt = draw[:B, :self.d_txt].to(self.dtype).contiguous() if train_text else None
        return dtxt, dimg
