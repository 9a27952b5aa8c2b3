"""MobileBERT + a linear head over libmmrca: the engine of ``classifiers.MobileBERT`` (the reference's ``MobileBert``,
CVPR_code/text_models.py:162-188: ``MobileBertForSequenceClassification`` with ``classifier`` replaced by ``Linear(512, n_classes)``).

The network is not BERT's (transformers modeling_mobilebert.py): a 512-wide stream ``h`` between layers, 128-wide bottlenecks inside
them, four feed-forward blocks per layer, ReLU, trigram input embeddings, and ``NoNorm`` (y = x * weight + bias) wherever BERT has a
LayerNorm.  One layer, rows = tokens:

    li = NoNorm(bottleneck.input.dense(h))             sh = NoNorm(bottleneck.attention.dense(h))                       512 -> 128
    q | k = query(sh) | key(sh)    v = value(h)        one [rows, 384] buffer through the GEMM's ldc column windows
    ctx = softmax(q k^T / sqrt(32) + key mask) v       mmrca_mha_fwd, H = 4, dh = 32, attention-probability dropout
    a = NoNorm(attention.output.dense(ctx) + li)
    3 x:  a = NoNorm(ffn.j.output.dense(relu(ffn.j.intermediate.dense(a))) + a)                                  128 -> 512 -> 128
    o = NoNorm(output.dense(relu(intermediate.dense(a))) + a)
    h = NoNorm(output.bottleneck.dense(o) + h)                                                                          128 -> 512

Embeddings: h = NoNorm(embedding_transformation(trigram(word[ids])) + position[t] + token_type[0]).  Logits = head(h[:, 0]).

Kernels: ``mmrca_nonorm_*`` and ``mmrca_trigram_embed_*`` (csrc/mobilebert.hip) are this model's own; the GEMMs, the attention,
``mmrca_bias_act_*`` (ReLU on the 512-wide pre-activations, which also adds the bias the GEMM leaves out), ``mmrca_embed_*`` on the
position table (position[t] + token_type[0]) and ``mmrca_linear_cls_*`` are the library's.  The NoNorm backward hands every Linear
in front of a NoNorm its bias gradient (gamma * column sums of dy), so no bias column-sum pass runs for those.

Arena:  text_model.mobilebert.* (transformers' order; NoNorm registers bias before weight) | head.weight [C, 512] | head.bias.
``MobileBertEngine`` derives from ``ClassifierEngine``: ``forward`` / ``backward`` / ``trainable_spans`` and the linear head are that
class's, and this one supplies its spec checks, ``_text_entries``, ``_group_of``, ``init_parameters`` and the encoder
(``_encoder_forward`` / ``_encoder_backward``).  So the flat optimizers, ``GradSync``, ``hip_train_step`` and ``GraphedTrainStep`` drive
it unchanged.  Compute modes: fp32 (the compliant one) and bf16.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import lib as L
from .classifier_engine import ClassifierEngine
from .engine import ROWPAD, TextPack, _round_up, parse_dtype


@dataclass(frozen=True)
class MobileBertSpec:
    """``MobileBertConfig()`` with ``classifier_activation=False`` (google/mobilebert-uncased).  Tests vary ``layers`` and ``vocab``."""
    name: str = "mobile_bert"
    vocab: int = 30522
    emb: int = 128                 # embedding_size
    dim: int = 512                 # hidden_size: the stream between layers, and the head's input
    layers: int = 24
    heads: int = 4
    ffn: int = 512                 # intermediate_size
    inner: int = 128               # intra_bottleneck_size = true_hidden_size
    n_ffn: int = 4                 # num_feedforward_networks (n_ffn - 1 `ffn.j` blocks + intermediate / output)
    max_pos: int = 512
    type_vocab: int = 2
    pad_id: int = 0
    attn_dropout: float = 0.1      # attention_probs_dropout_prob; hidden_dropout_prob is 0


MOBILEBERT = MobileBertSpec()
MODES = ("fp32", "bf16")


def mobilebert_layer_keys(i: int) -> Dict[str, str]:
    """short name -> transformers' module path of every Linear / NoNorm of layer i"""
    P = f"mobilebert.encoder.layer.{i}."
    K = {"q": P + "attention.self.query", "k": P + "attention.self.key", "v": P + "attention.self.value",
         "o": P + "attention.output.dense", "o_n": P + "attention.output.LayerNorm",
         "f1": P + "intermediate.dense", "f2": P + "output.dense", "f2_n": P + "output.LayerNorm",
         "ob": P + "output.bottleneck.dense", "ob_n": P + "output.bottleneck.LayerNorm",
         "bi": P + "bottleneck.input.dense", "bi_n": P + "bottleneck.input.LayerNorm",
         "ba": P + "bottleneck.attention.dense", "ba_n": P + "bottleneck.attention.LayerNorm"}
    return K


def mobilebert_params(s: MobileBertSpec):
    """(key, shape) of ``MobileBertForSequenceClassification``'s encoder in state_dict order (1,111 tensors at 24 layers; the pooler of
    ``classifier_activation=False`` has no parameters)"""
    E, D, I, F = s.emb, s.dim, s.inner, s.ffn
    ents = [("mobilebert.embeddings.word_embeddings.weight", (s.vocab, E)),
            ("mobilebert.embeddings.position_embeddings.weight", (s.max_pos, D)),
            ("mobilebert.embeddings.token_type_embeddings.weight", (s.type_vocab, D)),
            ("mobilebert.embeddings.embedding_transformation.weight", (D, 3 * E)),
            ("mobilebert.embeddings.embedding_transformation.bias", (D,)),
            ("mobilebert.embeddings.LayerNorm.bias", (D,)), ("mobilebert.embeddings.LayerNorm.weight", (D,))]

    def lin(path, n_out, n_in):
        return [(path + ".weight", (n_out, n_in)), (path + ".bias", (n_out,))]

    def norm(path, n):
        return [(path + ".bias", (n,)), (path + ".weight", (n,))]

    for i in range(s.layers):
        K = mobilebert_layer_keys(i)
        ents += lin(K["q"], I, I) + lin(K["k"], I, I) + lin(K["v"], I, D) + lin(K["o"], I, I) + norm(K["o_n"], I)
        ents += lin(K["f1"], F, I) + lin(K["f2"], I, F) + norm(K["f2_n"], I) + lin(K["ob"], D, I) + norm(K["ob_n"], D)
        ents += lin(K["bi"], I, D) + norm(K["bi_n"], I) + lin(K["ba"], I, D) + norm(K["ba_n"], I)
        for j in range(s.n_ffn - 1):
            P = f"mobilebert.encoder.layer.{i}.ffn.{j}."
            ents += lin(P + "intermediate.dense", F, I) + lin(P + "output.dense", I, F) + norm(P + "output.LayerNorm", I)
    return ents


class MobileBertEngine(ClassifierEngine):
    """Owns parameters, gradients and activations of one MobileBERT classifier replica on one GPU: ``ClassifierEngine``'s step and
    head around this class's encoder."""

    ENCODER_WORD = "encoder"

    def __init__(self, n_classes: int = 4, dtype="fp32", device="cuda", spec: MobileBertSpec = MOBILEBERT,
                 gemm_impl: int = L.IMPL_AUTO, attn_impl: int = L.IMPL_AUTO):
        """dtype: "fp32" (every product on the fp32 pipes: the mode whose logits meet the 1e-3 bound) or "bf16" (bf16 storage and
        matrix cores, fp32 accumulation).  The split-bf16 modes of the other engines are not built for this model: every product
        here contracts over 128 or 512 on a few dozen to a few thousand rows, shapes the three-pass kernels do not take (DESIGN K9
        has the measured breakdown of a step)."""
        L.load()
        if isinstance(dtype, str) and dtype.lower() not in ("fp32", "f32", "bf16"):
            raise ValueError(f"MobileBERT runs in {' or '.join(MODES)}, not {dtype!r} (the split-bf16 modes are not built for this model)")
        mode_flags = parse_dtype(dtype)
        if mode_flags[0] not in (torch.float32, torch.bfloat16):
            raise ValueError(f"MobileBERT runs in {' or '.join(MODES)}, not {dtype}")
        s = spec
        if s.inner % s.heads or (s.inner // s.heads) % 4 or s.inner // s.heads > 128:
            raise ValueError("head dim must be a multiple of 4, at most 128")
        self.kind, self.backbone = "text", s.name
        if not 1 <= int(n_classes) <= 16:
            raise ValueError(f"n_classes must be in [1, 16], got {n_classes}")
        self.reverse, self.mode = True, 0
        self._build(mode_flags, device, int(n_classes), gemm_impl, attn_impl, s)

    def _text_entries(self):
        return mobilebert_params(self.ts)

    @staticmethod
    def _group_of(key: str) -> str:
        m = re.match(r"text_model\.mobilebert\.encoder\.layer\.(\d+)\.", key)
        if m:
            return f"text_layer_{int(m.group(1))}"
        return "text_emb" if key.startswith("text_model.") else "head"

    def init_parameters(self, seed: int = 0):
        """transformers' ``_init_weights`` for the encoder: Linear and embedding weights N(0, 0.02), the pad row zero, biases 0,
        NoNorm (1, 0); the head as the reference's fresh ``nn.Linear`` (torch's default, uniform in +-1/sqrt(512))"""
        g = torch.Generator(device="cpu").manual_seed(seed)
        with torch.no_grad():
            for k in self.param_keys:
                v = self.arena.view(k)
                leaf = k.rsplit(".", 1)[-1]
                if k.startswith("head."):
                    bound = 1.0 / math.sqrt(self.feat_dim)
                    v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) * bound)
                elif ".LayerNorm." in k:
                    v.fill_(1.0 if leaf == "weight" else 0.0)
                elif leaf == "bias":
                    v.zero_()
                else:
                    v.copy_(torch.randn(v.shape, generator=g) * 0.02)
                    if k.endswith("word_embeddings.weight"):
                        v[self.ts.pad_id].zero_()
        self.arena.lp_valid = False

    # ------------------------------------------------------------------ op helpers
    def _mm(self, x, ldx, wkey, out, ldo, M, N, K, bias=True, addend=None):
        """out[:, :N] (row pitch ldo) = x[:, :K] W^T (+ bias) (+ addend, same pitch as out); W = `wkey`.weight [N, K]"""
        L.gemm(x, self.W(wkey + ".weight"), out, bias=(self.W(wkey + ".bias") if bias else None), addend=addend, M=M, N=N, K=K,
               lda=ldx, ldb=K, ldc=ldo, a_layout=L.ROWK, b_layout=L.ROWK, dtype=self.dt, impl=self.gemm_impl)

    def _mm_bwd(self, dy, lddy, x, ldx, wkey, dx, lddx, M, N, K, addend=None):
        """dW += dy^T x over the rows (buffers are zero beyond row M up to the next multiple of 64); dx = dy W (+ addend)"""
        L.gemm(dy, x, self.G(wkey + ".weight"), M=N, N=K, K=_round_up(M, 64), lda=lddy, ldb=ldx, ldc=K, a_layout=L.KROW,
               b_layout=L.KROW, accum=True, dtype=self.dt, impl=self.gemm_impl)
        if dx is not None:
            L.gemm(dy, self.W(wkey + ".weight"), dx, addend=addend, M=M, N=K, K=N, lda=lddy, ldb=K, ldc=lddx, a_layout=L.ROWK,
                   b_layout=L.KROW, dtype=self.dt, impl=self.gemm_impl)

    def _nn(self, x, res, nkey, sum_out, y, M, D):
        L.nonorm_fwd(x, res, self.W(nkey + ".weight"), self.W(nkey + ".bias"), sum_out, y, M, D, D, D, D, D, self.dt)

    def _nn_bwd(self, dy, s, nkey, ds, bias_key, M, D, cap):
        """ds = dy * gamma; the NoNorm's own gradients; the bias gradient of the Linear `bias_key` that fed it"""
        ws = self._bufs.get(("nn_ws", cap))
        if ws is None:
            ws = self._bufs[("nn_ws", cap)] = torch.empty(L.nonorm_bwd_workspace_bytes(cap, self.ts.dim) // 4, dtype=torch.float32,
                                                          device=self.device)
        L.nonorm_bwd(dy, s, self.W(nkey + ".weight"), None, ds, self.G(nkey + ".weight"), self.G(nkey + ".bias"),
                     self.G(bias_key + ".bias"), ws, M, D, D, D, D, D, self.dt)

    # ------------------------------------------------------------------ encoder
    def _encoder_forward(self, ids, mask, images, save, drop_p, drop_seed, pack: Optional[TextPack], bn_train=False, taps=None):
        """drop_p: the attention-probability dropout (0.1 in train mode; the model has no other).  taps: ``hidden_states`` indices n in
        [1, layers] whose class-token rows [B, 512] come back as ``saved["taps"][n]`` (``last_taps`` after a ``forward``)."""
        s, P = self.ts, "text_model."
        B, T = ids.shape
        if T > s.max_pos:
            raise L.MmrcaError(f"MobileBERT has {s.max_pos} positions, got captions of {T} tokens")
        cap, E, D, I, F, H = B * T, s.emb, s.dim, s.inner, s.ffn, s.heads
        dh = I // H
        ids32 = ids.to(torch.int32).contiguous()
        pos = torch.arange(T, device=ids.device, dtype=torch.int32).repeat(B)
        if pack is not None:
            if (pack.B, pack.T) != (B, T):
                raise L.MmrcaError(f"text pack was built for a [{pack.B},{pack.T}] batch, got [{B},{T}]")
            M, cu, first, mask32 = pack.M, pack.cu, pack.first, pack.mask
            perm = pack.perm.to(torch.int32)
            pos = pos[pack.perm].contiguous()
        else:
            M, cu, perm = cap, None, None
            first = torch.arange(B, device=ids.device, dtype=torch.int64) * T
            mask32 = mask.to(torch.int32).contiguous()
        fb = lambda name, cols, l=0: self.buf("mb_" + name, cap, cols, None, l if save else 0)
        zeros = self.buf("mb_zero_ids", cap, 1, torch.int32)
        # embeddings: trigram gather, 384 -> 512, + (position[t] + token_type[0]), NoNorm
        tri, et, pt = fb("tri", 3 * E), fb("et", D), fb("pt", D)
        L.trigram_embed_fwd(ids32, perm, self.W(P + "mobilebert.embeddings.word_embeddings.weight"), tri, M, B, T, E, s.vocab, self.dt)
        self._mm(tri, 3 * E, P + "mobilebert.embeddings.embedding_transformation", et, D, M, D, 3 * E)
        L.embed_fwd(pos, zeros, self.W(P + "mobilebert.embeddings.position_embeddings.weight"),
                    self.W(P + "mobilebert.embeddings.token_type_embeddings.weight"), None, pt, M, D, self.dt)
        s0 = fb("s_h", D, 0)
        h = self.buf("mb_h", cap, D, None, 0)
        self._nn(et, pt, P + "mobilebert.embeddings.LayerNorm", s0, h, M, D)
        dp = float(drop_p)
        layers, tap_rows = [], {}
        for i in range(s.layers):
            K = {n: P + k for n, k in mobilebert_layer_keys(i).items()}
            xli, xsh, li, sh = fb("xli", I, i), fb("xsh", I, i), fb("li", I), fb("sh", I, i)
            self._mm(h, D, K["bi"], xli, I, M, I, D)
            self._nn(xli, None, K["bi_n"], None, li, M, I)
            self._mm(h, D, K["ba"], xsh, I, M, I, D)
            self._nn(xsh, None, K["ba_n"], None, sh, M, I)
            qkv, ctx = fb("qkv", 3 * I, i), fb("ctx", I, i)
            lse = self.vec("mb_lse", _round_up(B * H * T, ROWPAD), torch.float32, i if save else 0)
            self._mm(sh, I, K["q"], qkv, 3 * I, M, I, I)
            self._mm(sh, I, K["k"], qkv[:, I:], 3 * I, M, I, I)
            self._mm(h, D, K["v"], qkv[:, 2 * I:], 3 * I, M, I, D)
            L.mha_fwd(qkv, mask32, ctx, lse, B, H, T, dh, dh ** -0.5, self.dt, self.attn_impl, drop_p=dp,
                      drop_seed=self._site_seed(drop_seed, i, 1), cu=cu)
            att = fb("att", I)
            self._mm(ctx, I, K["o"], att, I, M, I, I)
            s_a, a = fb("s_a", I, i), fb("a0", I, i)
            self._nn(att, li, K["o_n"], s_a, a, M, I)
            blocks = []
            for j in range(s.n_ffn):
                last = j == s.n_ffn - 1
                Fk = f"{P}mobilebert.encoder.layer.{i}.ffn.{j}."
                k1, k2, kn = (K["f1"], K["f2"], K["f2_n"]) if last else (Fk + "intermediate.dense", Fk + "output.dense", Fk + "output.LayerNorm")
                pre, act, out = fb(f"pre{j}", F, i), fb(f"act{j}", F, i), fb("ffo", I)
                self._mm(a, I, k1, pre, F, M, F, I, bias=False)
                L.bias_act_fwd(pre, self.W(k1 + ".bias"), act, M, F, L.CONV_RELU, self.dt)
                self._mm(act, F, k2, out, I, M, I, F)
                s_f, a_n = fb(f"s_f{j}", I, i), fb(f"a{j + 1}", I, i)
                self._nn(out, a, kn, s_f, a_n, M, I)
                blocks.append(dict(a_in=a, pre=pre, act=act, s=s_f, k1=k1, k2=k2, kn=kn))
                a = a_n
            hb = fb("hb", D)
            self._mm(a, I, K["ob"], hb, D, M, D, I)
            s_h = fb("s_h", D, i + 1)
            h_n = self.buf("mb_h", cap, D, None, (i + 1) if save else (i + 1) % 2)
            self._nn(hb, h, K["ob_n"], s_h, h_n, M, D)
            layers.append(dict(h=h, xli=xli, xsh=xsh, sh=sh, qkv=qkv, ctx=ctx, lse=lse, s_a=s_a, blocks=blocks, o=a, s_h=s_h, K=K))
            h = h_n
            if taps and (i + 1) in taps:
                tap_rows[i + 1] = h.index_select(0, first)
        cls = h.index_select(0, first)
        return cls, dict(B=B, T=T, M=M, cap=cap, cu=cu, first=first, ids32=ids32, perm=perm, pos=pos, zeros=zeros, mask32=mask32, tri=tri,
                         s0=s0, layers=layers, drop_p=dp, drop_seed=drop_seed, taps=tap_rows)

    def _encoder_backward(self, dcls, sv):
        s, P = self.ts, "text_model."
        B, T, M, cap, cu = sv["B"], sv["T"], sv["M"], sv["cap"], sv["cu"]
        E, D, I, F, H = s.emb, s.dim, s.inner, s.ffn, s.heads
        dh = I // H
        gb = lambda name, cols: self.buf("mbg_" + name, cap, cols)
        dx = gb("dh", D)            # gradient of the stream: each layer reads it first (NoNorm backward) and writes it last
        dx[:M].zero_()
        dx.index_copy_(0, sv["first"], dcls.to(dx.dtype))
        bsum = self.buf("mbg_qkv_bias", s.layers, 3 * I, torch.float32)
        bsum.zero_()
        for i in reversed(range(s.layers)):
            a, K = sv["layers"][i], sv["layers"][i]["K"]
            ds_h = gb("ds_h", D)                                   # gradient of output.bottleneck.dense's output AND of the stream h
            self._nn_bwd(dx, a["s_h"], K["ob_n"], ds_h, K["ob"], M, D, cap)
            d_a = gb("d_a", I)          # gradient of the 128-wide stream: same read-first, write-last pattern per block
            self._mm_bwd(ds_h, D, a["o"], I, K["ob"], d_a, I, M, D, I)
            for j in reversed(range(s.n_ffn)):
                b = a["blocks"][j]
                ds = gb("ds_f", I)
                self._nn_bwd(d_a, b["s"], b["kn"], ds, b["k2"], M, I, cap)
                d_act, d_pre = gb("d_act", F), gb("d_pre", F)
                self._mm_bwd(ds, I, b["act"], F, b["k2"], d_act, F, M, I, F)
                L.bias_act_bwd(d_act, b["pre"], self.W(b["k1"] + ".bias"), d_pre, self.G(b["k1"] + ".bias"), M, F, L.CONV_RELU, self.dt)
                self._mm_bwd(d_pre, F, b["a_in"], I, b["k1"], d_a, I, M, F, I, addend=ds)
            ds_a = gb("ds_a", I)                                   # gradient of attention.output.dense's output AND of li
            self._nn_bwd(d_a, a["s_a"], K["o_n"], ds_a, K["o"], M, I, cap)
            dctx = gb("dctx", I)
            self._mm_bwd(ds_a, I, a["ctx"], I, K["o"], dctx, I, M, I, I)
            dqkv = gb("dqkv", 3 * I)
            L.mha_bwd(a["qkv"], sv["mask32"], a["ctx"], dctx, a["lse"], dqkv, B, H, T, dh, dh ** -0.5, self.dt, self.attn_impl,
                      drop_p=sv["drop_p"], drop_seed=self._site_seed(sv["drop_seed"], i, 1), colsum=bsum[i], cu=cu, rows=M)
            torch._foreach_add_([self.G(K[n] + ".bias") for n in ("q", "k", "v")], list(bsum[i].split(I)))
            dsh1, dsh = gb("dsh1", I), gb("dsh", I)
            self._mm_bwd(dqkv, 3 * I, a["sh"], I, K["q"], dsh1, I, M, I, I)
            self._mm_bwd(dqkv[:, I:], 3 * I, a["sh"], I, K["k"], dsh, I, M, I, I, addend=dsh1)
            dh1 = gb("dh1", D)
            self._mm_bwd(dqkv[:, 2 * I:], 3 * I, a["h"], D, K["v"], dh1, D, M, I, D, addend=ds_h)
            ds_sh = gb("ds_sh", I)
            self._nn_bwd(dsh, a["xsh"], K["ba_n"], ds_sh, K["ba"], M, I, cap)
            dh2 = gb("dh2", D)
            self._mm_bwd(ds_sh, I, a["h"], D, K["ba"], dh2, D, M, I, D, addend=dh1)
            ds_li = gb("ds_li", I)
            self._nn_bwd(ds_a, a["xli"], K["bi_n"], ds_li, K["bi"], M, I, cap)
            self._mm_bwd(ds_li, I, a["h"], D, K["bi"], dx, D, M, I, D, addend=dh2)
            self._ready(f"text_layer_{i}")
        Ek = P + "mobilebert.embeddings."
        ds0 = gb("ds_h", D)
        self._nn_bwd(dx, sv["s0"], Ek + "LayerNorm", ds0, Ek + "embedding_transformation", M, D, cap)
        dtri = gb("dtri", 3 * E)
        self._mm_bwd(ds0, D, sv["tri"], 3 * E, Ek + "embedding_transformation", dtri, 3 * E, M, D, 3 * E)
        L.trigram_embed_bwd(dtri, sv["ids32"], sv["perm"], self.G(Ek + "word_embeddings.weight"), M, B, T, E, s.vocab, s.pad_id, self.dt)
        # position[t] + token_type[0]: the position table plays mmrca_embed_bwd's word table, the type table (row 0) its position table
        L.embed_bwd(ds0, sv["pos"], sv["zeros"], self.G(Ek + "position_embeddings.weight"), self.G(Ek + "token_type_embeddings.weight"),
                    None, M, D, self.dt)
        self._ready("text_emb", flush=True)
