"""MobileBERT on the MI355X: the NoNorm and trigram-embedding kernels against float64, the whole classifier against the golden file
(transformers' own class in float64) and against the float64 restatement (tests/mobilebert_ref.py) loaded from the model's own state
dict, attention dropout, training through autograd, the flat optimizer and a captured HIP graph, and the text driver / evaluator end to
end."""
import contextlib
import functools
import glob
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import classifiers as C     # noqa: E402
from garbage_classification_rca_amd import lib as L             # noqa: E402
from garbage_classification_rca_amd.engine import TextPack      # noqa: E402
from garbage_classification_rca_amd.mobilebert_engine import MobileBertSpec  # noqa: E402
from tests.mobilebert_ref import GOLDEN, GOLDEN_GRADS, GOLDEN_ROW_STRIDE, MobileBertRef, golden_inputs, proc_state  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _rel(a, ref):
    ref = ref.double().cpu()
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------- NoNorm
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [128, 512])
@pytest.mark.parametrize("rows", [1, 67, 300])
def test_nonorm_matches_float64(rows, D, dtype):
    """s = x (+ res), y = s * gamma + beta and its backward against float64 on the same (rounded) operands: with and without `res`, a
    row pitch larger than D, `sum_out` aliasing `x`, gradients accumulating onto 0.5, `dbias` on and off, the fused `dres` add, and two
    calls giving the same bits.  Bounds of the project's row-op tests: fp32 1e-5 forward and ds, 1e-4 on the row sums; bf16 storage
    2^-8 forward and ds (relative to the largest entry), 1e-4 on the fp32 sums of the rounded operands."""
    g = torch.Generator().manual_seed(rows * 7 + D)
    dt = L.dtype_code(dtype)
    tol = 1e-5 if dtype == torch.float32 else 2 ** -8
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(dtype)
    gamma, beta = (1.0 + rnd(D, scale=0.2).float()).to(dtype), rnd(D, scale=0.1)
    g64, b64 = gamma.double(), beta.double()
    pitch = D + 24                                            # a row pitch larger than D (still a multiple of 8: the 16-byte path)
    for with_res in (False, True):
        for ld in (D, pitch):
            xf = rnd(rows, ld)
            rf = rnd(rows, ld) if with_res else None
            x, res = xf.to(DEV), (rf.to(DEV) if with_res else None)
            s_ref = xf[:, :D].double() + (rf[:, :D].double() if with_res else 0.0)
            # (a) separate sum_out, (b) sum_out aliasing x, (c) no sum_out
            y, s_out = torch.zeros(rows, ld, dtype=dtype, device=DEV), torch.zeros(rows, ld, dtype=dtype, device=DEV)
            L.nonorm_fwd(x, res, gamma.to(DEV), beta.to(DEV), s_out, y, rows, D, ld, ld, ld, ld, dt)
            y2 = torch.zeros(rows, ld, dtype=dtype, device=DEV)
            L.nonorm_fwd(x, res, gamma.to(DEV), beta.to(DEV), None, y2, rows, D, ld, ld, 0, ld, dt)
            xa = x.clone()
            y3 = torch.zeros(rows, ld, dtype=dtype, device=DEV)
            L.nonorm_fwd(xa, res, gamma.to(DEV), beta.to(DEV), xa, y3, rows, D, ld, ld, ld, ld, dt)
            torch.cuda.synchronize()
            assert _rel(s_out[:, :D], s_ref) < tol and torch.equal(xa[:, :D], s_out[:, :D]) and torch.equal(y3, y)
            assert _rel(y[:, :D], s_out[:, :D].double().cpu() * g64 + b64) < tol           # y from the sum as stored
            assert _rel(y2[:, :D], s_ref * g64 + b64) < tol
            if ld > D:                                        # nothing written between the rows
                assert float(y[:, D:].abs().max()) == 0.0 and float(s_out[:, D:].abs().max()) == 0.0
                assert torch.equal(xa[:, D:], x[:, D:])
    # backward
    ws = torch.empty(L.nonorm_bwd_workspace_bytes(rows, D) // 4, dtype=torch.float32, device=DEV)
    for ld, with_dres, with_dbias in ((D, False, True), (pitch, True, False), (D, True, True)):
        dyf, sf = rnd(rows, ld), rnd(rows, ld)
        drf = rnd(rows, ld) if with_dres else None
        ds_ref = dyf[:, :D].double() * g64 + (drf[:, :D].double() if with_dres else 0.0)
        dg_ref = 0.5 + (dyf[:, :D].double() * sf[:, :D].double()).sum(0)
        db_ref = 0.5 + dyf[:, :D].double().sum(0)
        dbias_ref = 0.5 + g64 * dyf[:, :D].double().sum(0)
        outs = []
        for _ in range(2):
            ds = torch.zeros(rows, ld, dtype=dtype, device=DEV)
            dg, db, dbias = (torch.full((D,), 0.5, device=DEV) for _ in range(3))
            L.nonorm_bwd(dyf.to(DEV), sf.to(DEV), gamma.to(DEV), drf.to(DEV) if with_dres else None, ds, dg, db,
                         dbias if with_dbias else None, ws, rows, D, ld, ld, ld if with_dres else 0, ld, dt)
            torch.cuda.synchronize()
            outs.append((ds, dg, db, dbias))
        ds, dg, db, dbias = outs[0]
        assert _rel(ds[:, :D], ds_ref) < tol
        assert _rel(dg, dg_ref) < 1e-4 and _rel(db, db_ref) < 1e-4
        if with_dbias:
            assert _rel(dbias, dbias_ref) < 1e-4
        else:
            assert float((dbias - 0.5).abs().max()) == 0.0
        if ld > D:
            assert float(ds[:, D:].abs().max()) == 0.0
        for a, b in zip(outs[0], outs[1]):
            assert torch.equal(a, b)


def test_nonorm_element_path_for_unaligned_shapes():
    """D = 6 with a pitch of 7: nothing qualifies for the 16-byte path; same bounds (fp32)"""
    g = torch.Generator().manual_seed(3)
    rows, D, ld = 37, 6, 7
    x, res, dy = (torch.randn(rows, ld, generator=g) for _ in range(3))
    gamma, beta = 1.0 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    y, s = torch.zeros(rows, ld, device=DEV), torch.zeros(rows, ld, device=DEV)
    L.nonorm_fwd(x.to(DEV), res.to(DEV), gamma.to(DEV), beta.to(DEV), s, y, rows, D, ld, ld, ld, ld, L.F32)
    s_ref = x[:, :D].double() + res[:, :D].double()
    ws = torch.empty(L.nonorm_bwd_workspace_bytes(rows, D) // 4, dtype=torch.float32, device=DEV)
    ds, dg, db = torch.zeros(rows, ld, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    L.nonorm_bwd(dy.to(DEV), s, gamma.to(DEV), None, ds, dg, db, None, ws, rows, D, ld, ld, 0, ld, L.F32)
    torch.cuda.synchronize()
    assert _rel(y[:, :D], s_ref * gamma.double() + beta.double()) < 1e-5 and float(y[:, D:].abs().max()) == 0.0
    assert _rel(ds[:, :D], dy[:, :D].double() * gamma.double()) < 1e-5
    assert _rel(dg, (dy[:, :D].double() * s_ref).sum(0)) < 1e-4 and _rel(db, dy[:, :D].double().sum(0)) < 1e-4


# ---------------------------------------------------------------------------------------------------- trigram embedding
def _trigram_ref(ids, word, perm):
    """index-based restatement: [M, 3E] rows of cat(e shifted to t+1, e, e shifted to t-1) over the padded [B, T] ids"""
    e = word[ids]                                              # [B, T, E]
    z = torch.zeros_like(e[:, :1])
    tri = torch.cat([torch.cat([e[:, 1:], z], 1), e, torch.cat([z, e[:, :-1]], 1)], dim=2).reshape(-1, 3 * word.shape[1])
    return tri if perm is None else tri[perm.long()]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("E", [8, 128])
def test_trigram_embedding_forward_is_exact_and_backward_matches_float64(E, packed, dtype):
    """B = 3, T = 7, live lengths 7, 3, 1, V = 50, repeated ids; padded (no perm) and packed (the live rows plus one padding row of
    caption 1, as make_text_pack's rounding adds).  Forward: exact.  Backward: float64 autograd of F.embedding(padding_idx=0) and the
    shifts, 1e-5 of the largest entry; the pad row of dword is untouched."""
    B, T, V = 3, 7, 50
    g = torch.Generator().manual_seed(E)
    ids = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate((7, 3, 1)):
        ids[b, :n] = torch.randint(1, 12, (n,), generator=g)     # 11 values over 11 slots: ids repeat
        ids[b, 0] = 5
    word = torch.randn(V, E, generator=g).to(dtype)              # (row 0 = the pad id's row is NOT zero here: the gather must read it)
    perm = torch.tensor(list(range(7)) + [7, 8, 9, 10] + [14], dtype=torch.int32) if packed else None
    M = B * T if perm is None else perm.numel()
    dt = L.dtype_code(dtype)
    ids32, perm_d = ids.to(torch.int32).to(DEV), (None if perm is None else perm.to(DEV))
    out = torch.full((M, 3 * E), 7.0, dtype=dtype, device=DEV)
    L.trigram_embed_fwd(ids32, perm_d, word.to(DEV), out, M, B, T, E, V, dt)
    torch.cuda.synchronize()
    ref = _trigram_ref(ids, word, perm)
    assert torch.equal(out.cpu(), ref)
    rows = {int(p): r for r, p in enumerate(range(B * T) if perm is None else perm.tolist())}
    o = out.cpu()
    # the last live token's "next" slot holds word[pad id]; t = 0 has no previous and t = T - 1 no next token
    assert torch.equal(o[rows[1 * T + 2], :E], word[0]) and torch.equal(o[rows[2 * T + 0], :E], word[0])
    for b in range(B):
        assert float(o[rows[b * T], 2 * E:].abs().max()) == 0.0
    assert float(o[rows[0 * T + T - 1], :E].abs().max()) == 0.0            # caption 0 fills the row: zeros, not caption 1's class token
    assert not torch.equal(o[rows[1 * T + 2], :E], word[ids[2, 0]])        # caption 1's last live row never reads caption 2
    # backward
    dout = torch.randn(M, 3 * E, generator=g).to(dtype)
    w64 = word.double().requires_grad_(True)
    e = F.embedding(ids, w64, padding_idx=0)
    z = torch.zeros_like(e[:, :1])
    tri = torch.cat([torch.cat([e[:, 1:], z], 1), e, torch.cat([z, e[:, :-1]], 1)], dim=2).reshape(-1, 3 * E)
    tri = tri if perm is None else tri[perm.long()]
    (tri * dout.double()).sum().backward()
    dword = torch.full((V, E), 0.5, device=DEV)
    L.trigram_embed_bwd(dout.to(DEV), ids32, perm_d, dword, M, B, T, E, V, 0, dt)
    torch.cuda.synchronize()
    assert float((dword[0] - 0.5).abs().max()) == 0.0
    assert _rel(dword - 0.5, w64.grad) < 1e-5


# ---------------------------------------------------------------------------------------------------- the whole classifier
def _model(layers, dtype):
    m = C.MobileBERT(4, dtype=dtype, device=DEV, spec=MobileBertSpec(layers=layers))
    sd = proc_state({k[len("model."):]: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({"model." + k: v for k, v in sd.items()}, strict=True)
    return m.eval()


def _hand_pack(mask):
    """the packed layout of a [3, 16] batch (make_text_pack declines B*T = 48: not a multiple of 64): live rows only"""
    B, T = mask.shape
    lens = mask.sum(1)
    perm = torch.cat([b * T + torch.arange(int(n)) for b, n in enumerate(lens)])
    cu = torch.zeros(B + 1, dtype=torch.int64)
    cu[1:] = torch.cumsum(lens, 0)
    M = int(cu[-1])
    return TextPack(perm.to(DEV), cu.to(torch.int32).to(DEV), torch.ones(M, dtype=torch.int32, device=DEV), cu[:-1].to(DEV), M, B, T)


@functools.lru_cache(maxsize=None)
def _reference(layers):
    """float64 restatement on the procedural weights: logits and every parameter gradient of sum(logits * dlogits); and the logits
    of the same network run entirely in bfloat16 on the CPU.  Computed once per depth."""
    ids, mask, dl = golden_inputs()
    ref = MobileBertRef(4, layers).double().eval()
    ref.load_state_dict({k: v.double() for k, v in proc_state(ref).items()}, strict=True)
    out = ref(ids, mask)
    (out * dl.double()).sum().backward()
    grads = {k: p.grad.clone() for k, p in ref.named_parameters()}
    with torch.no_grad():
        low = MobileBertRef(4, layers).eval()
        low.load_state_dict(proc_state(low), strict=True)
        out16 = low.to(torch.bfloat16)(ids, mask).double()
    return out.detach(), grads, out16


def _grad_scale(grads, k):
    """the largest entry of the tensor's float64 gradient.  One tensor per layer has none: the gradient of attention.self.key.bias is
    identically zero (a shift of every key leaves the softmax unchanged; float64 autograd gives 1e-20, fp32 torch 1e-11), so its error
    is taken relative to the largest entry of the same layer's query.bias gradient -- the same column sums over the same rows."""
    if k.endswith("attention.self.key.bias"):
        k = k.replace("attention.self.key.bias", "attention.self.query.bias")
    return float(grads[k].abs().max().clamp_min(1e-30))


def test_two_layer_model_matches_the_transformers_golden():
    """fp32, eval mode, against transformers' own float64 run (tests/golden/mobilebert_goldens.npz): logits and hidden_states[1] at
    the class tokens within 1e-4 of the largest entry (test_classifier_gpu.py's fp32 bound), the four recorded gradients within 2e-3
    of each tensor's largest entry (the README's fp32 gradient bound)"""
    gold = np.load(GOLDEN)
    ids, mask, dl = golden_inputs()
    m = _model(2, "fp32")
    eng = m.engine
    eng.arena.g.zero_()
    logits = eng.forward(ids.to(DEV), mask.to(DEV), None, save=True, taps=[1])
    eng.backward(dl.to(DEV), train_text=True)
    torch.cuda.synchronize()
    e1, e2 = _rel(logits, torch.from_numpy(gold["logits"])), _rel(eng.last_taps[1], torch.from_numpy(gold["hidden1_cls"]))
    print(f"mobilebert golden: logits {e1:.3e} hidden_states[1] {e2:.3e}")
    assert e1 < 1e-4 and e2 < 1e-4
    for k in GOLDEN_GRADS:
        name = "head." + k[len("classifier."):] if k.startswith("classifier.") else "text_model." + k
        got = eng.arena.view(name, "g").double().cpu()[::GOLDEN_ROW_STRIDE.get(k, 1)]
        err = float((got - torch.from_numpy(gold["grad:" + k])).abs().max() / float(gold["gradmax:" + k]))
        print(f"mobilebert golden: grad {k} {err:.3e}")
        assert err < 2e-3, (k, err)
    eng.release_buffers()


@pytest.mark.parametrize("layers", [2, 24])
def test_fp32_model_matches_the_float64_restatement(layers):
    """eval mode, B = 3, T = 16 (lengths 16, 9, 1), padded and packed: logits within 1e-4 and EVERY parameter gradient within 2e-3 of
    the tensor's largest entry (_grad_scale); packed and padded logits agree to 1e-6 of the largest logit"""
    ids, mask, dl = golden_inputs()
    out, grads, _ = _reference(layers)
    m = _model(layers, "fp32")
    eng = m.engine
    got = {}
    for layout in ("padded", "packed"):
        eng.release_buffers()                  # (the two layouts share buffers sized for B*T rows; padding rows must be zero)
        eng.arena.g.zero_()
        pack = _hand_pack(mask) if layout == "packed" else None
        logits = eng.forward(ids.to(DEV), mask.to(DEV), None, save=True, text_pack=pack)
        eng.backward(dl.to(DEV), train_text=True)
        torch.cuda.synchronize()
        got[layout] = logits.clone()
        err = _rel(logits, out)
        worst, worst_k = 0.0, None
        for k, gref in grads.items():
            name = "head." + k[len("classifier."):] if k.startswith("classifier.") else "text_model." + k
            e = float((eng.arena.view(name, "g").double().cpu() - gref).abs().max() / _grad_scale(grads, k))
            if e > worst:
                worst, worst_k = e, k
        print(f"mobilebert fp32 {layers} layers {layout}: logits {err:.3e}; worst gradient {worst:.3e} ({worst_k})")
        assert err < 1e-4, err
        assert worst < 2e-3, (worst, worst_k)
    gap = float((got["padded"] - got["packed"]).abs().max() / got["padded"].abs().max())
    print(f"mobilebert fp32 {layers} layers: packed vs padded {gap:.3e}")
    assert gap <= 1e-6, gap
    eng.release_buffers()


@pytest.mark.parametrize("layers", [2, 24])
def test_bf16_model_against_the_all_bf16_restatement(layers):
    """bf16 mode, padded and packed: the logits error against float64 must not exceed twice that of the restatement run entirely in
    torch.bfloat16 on the CPU (the factor covers a different rounding order; the engine accumulates in fp32).  Gradients: the project's
    bf16-backward bounds (test_mobilenet_v3_gpu.py): head weight 5e-2; encoder.layer.0.attention.self.value.weight relative L2
    1.5e-1 and cosine above 0.99.  Both error figures are printed."""
    ids, mask, dl = golden_inputs()
    out, grads, out16 = _reference(layers)
    base = float((out16 - out).abs().max() / out.abs().max())
    m = _model(layers, "bf16")
    eng = m.engine
    for layout in ("padded", "packed"):
        eng.release_buffers()
        eng.arena.g.zero_()
        pack = _hand_pack(mask) if layout == "packed" else None
        logits = eng.forward(ids.to(DEV), mask.to(DEV), None, save=True, text_pack=pack)
        eng.backward(dl.to(DEV), train_text=True)
        torch.cuda.synchronize()
        err = _rel(logits, out)
        print(f"mobilebert bf16 {layers} layers {layout}: engine logits error {err:.3e}; all-bf16 restatement {base:.3e}")
        assert err <= 2.0 * base, (err, base)
        gw = _rel(eng.arena.view("head.weight", "g"), grads["classifier.weight"])
        k = "mobilebert.encoder.layer.0.attention.self.value.weight"
        gv, rv = eng.arena.view("text_model." + k, "g").double().cpu(), grads[k]
        l2 = float((gv - rv).norm() / rv.norm())
        cos = float((gv.flatten() / gv.norm()) @ (rv.flatten() / rv.norm()))
        print(f"mobilebert bf16 {layers} layers {layout}: head grad {gw:.3e}; value.weight grad rel L2 {l2:.3e} cos {cos:.5f}")
        assert gw < 5e-2 and l2 < 1.5e-1 and cos > 0.99, (gw, l2, cos)
    eng.release_buffers()


def test_attention_dropout_is_seeded_and_off_in_eval():
    ids, mask, _ = golden_inputs()
    ids, mask = ids.to(DEV), mask.to(DEV)
    m = _model(2, "fp32")
    eng = m.engine
    a = eng.forward(ids, mask, None, seed=5, save=False, enc_drop_p=0.1).clone()
    b = eng.forward(ids, mask, None, seed=5, save=False, enc_drop_p=0.1).clone()
    c = eng.forward(ids, mask, None, seed=6, save=False, enc_drop_p=0.1).clone()
    ev = eng.forward(ids, mask, None, seed=5, save=False, enc_drop_p=0.0).clone()
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, ev)
    with torch.no_grad():
        e1 = m.eval()(ids, mask).clone()
        m.train()
        t1 = m(ids, mask).clone()
        m.enc_dropout = 0.0
        t0 = m(ids, mask).clone()
    assert torch.equal(e1, ev) and torch.equal(t0, e1) and not torch.equal(t1, e1)
    eng.release_buffers()


def test_trains_through_autograd_and_the_flat_optimizer():
    """frozen encoder (the constructor's state): one step changes model.classifier.* only; unfrozen: every tensor changes; the loss on a
    fixed batch falls over a few AdamW steps; a state-dict round trip into a second instance reproduces the logits bit for bit"""
    from garbage_classification_rca_amd.optim import FlatAdamW
    ids, mask, _ = golden_inputs()
    ids, mask = ids.to(DEV), mask.to(DEV)
    labels = torch.tensor([0, 1, 2], device=DEV)
    m = _model(2, "fp32").train()
    m.enc_dropout = 0.0
    opt = FlatAdamW(m, lr=1e-3, weight_decay=0.0)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    F.cross_entropy(m(ids, mask), labels).backward()
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]) == (not k.startswith("model.classifier.")), k
    for p in m.parameters():
        p.requires_grad = True
    losses = []
    for _ in range(5):
        loss = F.cross_entropy(m(ids, mask), labels)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    for k, v in m.state_dict().items():
        assert not torch.equal(v, before[k]), k
    print("mobilebert AdamW losses", losses)
    assert losses[-1] < losses[0]
    m.eval()
    twin = C.MobileBERT(4, dtype="fp32", device=DEV, spec=MobileBertSpec(layers=2), init_seed=9).eval()
    twin.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    with torch.no_grad():
        assert torch.equal(m(ids, mask), twin(ids, mask))
    m.engine.release_buffers()
    twin.engine.release_buffers()


@pytest.mark.parametrize("frozen", [True, False])
def test_graphed_step_reproduces_the_eager_steps(frozen):
    """two layers, B = 4, T = 16, attention dropout on: GraphedTrainStep (2 eager calls, 1 capture, 3 replays) against eager
    hip_train_step on a twin from the same weights.
    Encoder frozen (the state the constructor leaves, the drivers' first phase): every launch of the step reduces in a fixed order,
    and the six losses are the same bit for bit.
    Everything trainable: the embedding backward adds with fp32 atomicAdd (mmrca_trigram_embed_bwd on repeated ids, mmrca_embed_bwd
    on the position rows and the token-type row, which all 64 token rows hit), so two runs of the SAME eager step may differ in the
    order of those sums; measured once: five losses equal, the sixth 2 ulp apart (1.2436373 / 1.2436371).  Reordering a sum of at
    most 64 addends moves it by at most 64 eps relative, and what reaches the next loss goes through lr = 2e-3, so the losses must
    agree to 64 * 2^-24 = 3.8e-6 relative (the project's graph tests allow 2e-3 on top of the eager-vs-eager spread)."""
    from garbage_classification_rca_amd.optim import FlatSGD
    from garbage_classification_rca_amd.procedural import synth_captions
    from garbage_classification_rca_amd.training import FusedCrossEntropy, GraphedTrainStep, hip_train_step
    B, T, n = 4, 16, 6
    data = []
    for k in range(n):
        ids, mask = (torch.from_numpy(a).to(DEV) for a in synth_captions(B, T, seed=40 + k, min_len=3))
        data.append((ids, mask, torch.zeros(B, 0, device=DEV), torch.tensor([k % 4, 1, 2, 3], device=DEV)))
    ms = [_model(2, "fp32") for _ in range(2)]
    for m in ms:
        m.train()
        if not frozen:
            for p in m.parameters():
                p.requires_grad = True
    oa, ob = (FlatSGD(m, lr=2e-3, weight_decay=1e-2) for m in ms)
    crit = FusedCrossEntropy(None, 0.0)
    graphed = GraphedTrainStep(ms[1], crit, ob, warmup=2)
    la, lb = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(n):
            la.append(float(hip_train_step(ms[0], *data[k], crit, oa)))
            lb.append(float(graphed(*data[k])))
    torch.cuda.synchronize()
    print("frozen" if frozen else "trainable", "eager  ", la, "\ngraphed", lb)
    assert graphed.replays == n - 2 and len(graphed._graphs) == 1
    assert len(set(la)) == n                       # the steps differ (the optimizer moves the head / the model, the batches change)
    if frozen:
        assert la == lb
    else:
        assert max(abs(a - b) / abs(a) for a, b in zip(la, lb)) <= 64 * 2.0 ** -24, (la, lb)
    for m in ms:
        m.engine.release_buffers()


# ---------------------------------------------------------------------------------------------------- drivers end to end
# One caption per class (the file-name stems).  The drivers save a checkpoint only when the validation accuracy rises above 0, and an
# untrained model maps each caption to a fixed class: with 'pizza_box' for Blue it happens to get all four wrong (0 % in both phases,
# nothing saved).  The freshly initialised model (init_seed 0) puts 'milk carton' in Blue with its widest margin (0.0086 between the two
# largest logits, float64 restatement), so the first epoch scores 25 %.
CAPTIONS = ['chip_bag', 'milk_carton', 'banana_peel', 'aa_batteries']


def _tiny_folder(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    for split in ("Train", "Val"):
        for ci, c in enumerate(["Black", "Blue", "Green", "TTR"]):
            d = tmp_path / f"Tiny_{split}" / c
            d.mkdir(parents=True)
            for k in range(2 if split == "Train" else 3):
                arr = (rng.random((40, 40, 3)) * 255).astype(np.uint8)
                Image.fromarray(arr).save(d / f"{CAPTIONS[ci]}_{k}.png")


def test_main_text_and_evaluator_run_mobile_bert_on_a_tiny_folder(tmp_path):
    """main_text.py --text_model=mobile_bert: one epoch of each phase, a best-val checkpoint with the reference's file name and
    transformers' key names; calculate_test_accuracy_text.py then evaluates it and writes the report CSV"""
    _tiny_folder(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--text_model=mobile_bert", "--num_workers", "0", "--tokens_max_len", "16"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main_text.py"), "--dataset_folder_name=Tiny", "--epochs", "1", "--ft_epochs", "1",
                        "--seed", "1", *common], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "using fp32" in r.stdout and "Grad Acc steps: 12" in r.stdout and "Batch Size FT: 4" in r.stdout
    assert "Num total parameters of the model: 24583940" in r.stdout
    assert "Starting Fine tuning!!" in r.stdout and "Fine Tuning: Val set accuracy" in r.stdout
    names = (r"BEST_model_mobile_bert_epoch_\d+_LR_0\.001_Reg_0\.01_VAL_ACC_\d+\.\d{5}_",
             r"BEST_model_mobile_bert_FT_EPOCH_\d+_LR_0\.001_Reg_0\.01_FractionLR_5(\.0)?_OPT_sgd_VAL_ACC_\d+\.\d{5}_")
    ckpts = sorted(glob.glob(str(tmp_path / "model_weights" / "mobile_bert" / "BEST_model_*.pth")), key=os.path.getmtime)
    assert ckpts, r.stdout[-3000:]
    for c in ckpts:
        assert any(re.fullmatch(n + r"\d{4}(_\d\d){5}\.pth", os.path.basename(c)) for n in names), c
    sd = torch.load(ckpts[0], map_location="cpu")
    assert len(sd) == 1113 and tuple(sd["model.classifier.weight"].shape) == (4, 512)
    assert "model.mobilebert.encoder.layer.23.ffn.2.output.LayerNorm.bias" in sd
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "calculate_test_accuracy_text.py"), "--model_path", ckpts[0],
                         "--dataset_folder_name", str(tmp_path / "Tiny_Val"), *common], cwd=tmp_path, env=env, capture_output=True, text=True,
                        timeout=600)
    assert r2.returncode == 0, r2.stdout[-1500:] + r2.stderr[-3000:]
    assert "Test accuracy:" in r2.stdout
    assert glob.glob(str(tmp_path / "test_set_reports" / "mobile_bert" / "text_model_mobile_bert_report_test_set_acc_*.csv"))
