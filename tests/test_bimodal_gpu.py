"""The bimodal GRU late-fusion model on the GPU: every kernel of csrc/gru.hip against float64 on the same inputs, the forward chain against
the golden recorded from the reference's own class, the whole model against the float64 restatement (tests/bimodal_ref.py) in the four
dtype modes, its gradients, the dependence on the batch order, a train step (eager and captured) and the drivers.

Tolerances.  GRU and Hadamard kernels: 2e-5 of the tensor's largest float64 entry.  On the same inputs (unit-scale x, weights
U(+-1/sqrt(H)), |h| up to 0.7-0.9) torch's own fp32 CPU GRU sits at <= 9e-7 on every one of these tensors for T <= 256; the factor of
about 20 covers another summation order over 400-500 terms and the device's exp.  Golden chain: 1e-5 of each tensor's scale.  Whole-model
logits: the project's 1e-3 in fp32 / bf16x3 / bf16x3f, 3e-2 in bf16 (the hierarchical suite's bounds).  Gradients: 2e-3 of
max(|ref|max, 1e-3 * gmax), the criterion of test_whole_model_gradients_match_float64_autograd there."""
import contextlib
import functools
import glob
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import lib as L                                          # noqa: E402
from garbage_classification_rca_amd.bimodal_engine import BimodalEngine                       # noqa: E402
from garbage_classification_rca_amd.procedural import proc_input, synth_captions, counter_uniform  # noqa: E402
from tests import bimodal_ref as BR                                                            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bimodal_goldens.npz")
DEV = "cuda:0"
TOL = 2e-5
LEAVES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _err(a, ref):
    """largest absolute error over the largest float64 entry (an all-zero reference must be met exactly)"""
    ref = torch.as_tensor(ref).double().cpu()
    d = float((torch.as_tensor(a).double().cpu() - ref).abs().max())
    return d / float(ref.abs().max()) if float(ref.abs().max()) > 0 else (0.0 if d == 0 else float("inf"))


# ------------------------------------------------------------------------------------------------------------------ GRU kernels
@functools.lru_cache(maxsize=None)
def _gru_case(n_in, hid, T, seed=0):
    """inputs (fp32, as the kernels get them) and the float64 outputs / gradients of the written-out GRU, computed once"""
    g = torch.Generator().manual_seed(1000 * hid + 10 * T + seed)
    bound = hid ** -0.5
    x = torch.randn(T, n_in, generator=g)
    P = [(torch.rand(s, generator=g) * 2 - 1) * bound for s in ((3 * hid, n_in), (3 * hid, hid), (3 * hid,), (3 * hid,))]
    d = torch.randn(T, hid, generator=g)
    xd = x.double().requires_grad_(True)
    Pd = [p.double().requires_grad_(True) for p in P]
    out = BR.gru_sequence(xd, *Pd)
    (out * d.double()).sum().backward()
    with torch.no_grad():
        flat = BR.gru_sequence(x.double(), P[0].double(), torch.zeros_like(P[1]).double(), P[2].double(), P[3].double())
    ref = dict(out=out.detach(), dx=xd.grad, flat=flat, **{k: p.grad for k, p in zip(LEAVES, Pd)})
    return x, P, d, ref


def _gru_gpu(cases, hid, zero_whh=False):
    """len(cases) GRUs (x, P, d) of the same T and width in ONE chain, forward and backward; per GRU dict(out, dx, weight_ih, ...)"""
    T, n_in = cases[0][0].shape
    st = []
    for x, P, d in cases:
        wih, whh, bih, bhh = (p.to(DEV).contiguous() for p in P)
        if zero_whh:
            whh = torch.zeros_like(whh)
        s = dict(x=x.to(DEV), d=d.to(DEV), wih=wih, whh=whh, bih=bih, bhh=bhh, gi=torch.empty(T, 3 * hid, device=DEV),
                 hseq=torch.zeros(T + 1, hid, device=DEV), gates=torch.empty(T, 3 * hid, device=DEV), hn=torch.empty(T, hid, device=DEV),
                 carry=torch.empty(T, hid, device=DEV), dgi=torch.empty(T, 3 * hid, device=DEV), dgh=torch.empty(T, 3 * hid, device=DEV))
        L.gru_linear_fwd(s["x"], n_in, wih, bih, s["gi"], 3 * hid, T, 3 * hid, n_in)
        st.append(s)
    col = lambda k: [s[k] for s in st]
    L.gru_fwd(col("gi"), col("whh"), col("bhh"), col("hseq"), col("gates"), col("hn"), T, hid)
    L.gru_bwd(col("whh"), col("hseq"), col("gates"), col("hn"), col("d"), [hid] * len(st), col("carry"), col("dgi"), col("dgh"), T, hid)
    res = []
    for s in st:
        g = dict(weight_ih=torch.zeros_like(s["wih"]), weight_hh=torch.zeros_like(s["whh"]), bias_ih=torch.zeros_like(s["bih"]),
                 bias_hh=torch.zeros_like(s["bhh"]), dx=torch.empty(T, n_in, device=DEV))
        L.gru_linear_bwd(s["dgi"], 3 * hid, None, 0, s["x"], n_in, s["wih"], g["weight_ih"], g["bias_ih"], g["dx"], n_in, T, 3 * hid, n_in)
        L.gru_linear_bwd(s["dgh"], 3 * hid, None, 0, s["hseq"], hid, s["whh"], g["weight_hh"], g["bias_hh"], None, 0, T, 3 * hid, hid)
        g["out"] = s["hseq"][1:].clone()
        assert float(s["hseq"][0].abs().max()) == 0.0          # h_{-1} is the caller's row: never written
        res.append(g)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("T", [1, 2, 3, 33])
@pytest.mark.parametrize("n_in,hid", [(400, 400), (400, 500)])
def test_gru_forward_and_backward_match_float64(n_in, hid, T):
    """outputs, dx and the four parameter gradients within 2e-5 of the tensor's largest float64 entry; and the recurrence is really
    there: with weight_hh = 0 the kernel's output differs from the full one by more than 0.1 of its scale at T >= 2"""
    x, P, d, ref = _gru_case(n_in, hid, T)
    got = _gru_gpu([(x, P, d)], hid)[0]
    errs = {k: _err(got[k], ref[k]) for k in ("out", "dx") + LEAVES}
    print(f"GRU I={n_in} H={hid} T={T}: |h|max {float(ref['out'].abs().max()):.3f}; errors {errs}")
    assert all(e <= TOL for e in errs.values()), errs
    flat = _gru_gpu([(x, P, d)], hid, zero_whh=True)[0]["out"]
    assert _err(flat, ref["flat"]) <= TOL
    if T >= 2:
        move = float((flat - got["out"]).abs().max() / got["out"].abs().max())
        print(f"  weight_hh = 0 moves the output by {move:.3f} of its scale")
        assert move > 0.1, move
    else:
        assert torch.equal(flat, got["out"])                   # h_{-1} = 0: step 0 does not see weight_hh


@pytest.mark.parametrize("T", [1, 3, 33])
def test_two_grus_in_one_chain_equal_each_run_alone(T):
    a, b = _gru_case(400, 400, T)[:3], _gru_case(400, 400, T, seed=1)[:3]
    both = _gru_gpu([a, b], 400)
    for pair, alone in zip(both, (_gru_gpu([a], 400)[0], _gru_gpu([b], 400)[0])):
        for k in alone:
            assert torch.equal(pair[k], alone[k]), k
    assert not torch.equal(both[0]["out"], both[1]["out"])


@pytest.mark.parametrize("hid", [400, 500])
def test_weight_gradients_are_bitwise_reproducible(hid):
    case = _gru_case(400, hid, 33)[:3]
    r1, r2 = _gru_gpu([case], hid)[0], _gru_gpu([case], hid)[0]
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k


@pytest.mark.parametrize("B,N,K,relu", [(1, 400, 768, False), (3, 450, 900, True), (33, 4, 450, False), (9, 1500, 400, False), (5, 7, 13, True)])
def test_small_linear_forward_and_backward_match_float64(B, N, K, relu):
    """every path of the Linear: 16-byte and single-float loads (K = 450, 13), tails behind the last 256 columns, more batch rows than a
    tile, row pitches wider than the matrix, ReLU masks in the backward, accumulation into non-zero gradients"""
    g = torch.Generator().manual_seed(B + N + K)
    pad = 4
    X, W, b = torch.randn(B, K + pad, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g) * 0.1
    dY, dW0, db0 = torch.randn(B, N + 3, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    Xd, Wd, bd, dYd = X.to(DEV), W.to(DEV), b.to(DEV), dY.to(DEV)
    Y = torch.full((B, N + 3), -7.0, device=DEV)
    L.gru_linear_fwd(Xd, K + pad, Wd, bd, Y, N + 3, B, N, K, relu=relu)
    pre = X[:, :K].double() @ W.double().T + b.double()
    ref = pre.clamp_min(0) if relu else pre
    assert _err(Y[:, :N], ref) <= TOL and bool((Y[:, N:] == -7.0).all())
    dZ = dY[:, :N].double() * ((ref > 0) if relu else 1.0)
    dW, db, dX = dW0.to(DEV), db0.to(DEV), torch.full((B, K + pad), -7.0, device=DEV)
    L.gru_linear_bwd(dYd, N + 3, Y if relu else None, N + 3, Xd, K + pad, Wd, dW, db, dX, K + pad, B, N, K)
    torch.cuda.synchronize()
    assert _err(dW.cpu().double() - dW0.double(), dZ.T @ X[:, :K].double()) <= TOL
    assert _err(db.cpu().double() - db0.double(), dZ.sum(0)) <= TOL
    assert _err(dX[:, :K], dZ @ W.double()) <= TOL and bool((dX[:, K:] == -7.0).all())


# ------------------------------------------------------------------------------------------------------------------ fusion, dropout
@pytest.mark.parametrize("B", [1, 3, 33])
def test_hadamard_fusion_forward_and_backward_match_float64(B):
    C = 400
    g = torch.Generator().manual_seed(B)
    a, x2, d1, d2 = (torch.randn(B, C, generator=g) for _ in range(4))
    k1, k2, bias = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.1
    ad, xd, k1d, k2d, bd = (t.double().requires_grad_(True) for t in (a, x2, k1, k2, bias))
    ref = BR.hadamard(ad, xd, k1d, k2d, bd)
    (ref * (d1 + d2).double()).sum().backward()
    out = torch.full((B, 900), -7.0, device=DEV)
    dev = [t.to(DEV) for t in (a, x2, k1, k2, bias)]
    L.hadamard_fwd(dev[0], C, dev[1], C, dev[2], dev[3], dev[4], out, 900, B, C)
    assert _err(out[:, :C], ref.detach()) <= TOL and bool((out[:, C:] == -7.0).all())
    dab = torch.empty(B, 2 * C, device=DEV)
    g0 = [torch.randn(C, generator=g) for _ in range(3)]
    gk = [t.to(DEV) for t in g0]
    L.hadamard_bwd(d1.to(DEV), C, d2.to(DEV), C, dev[0], C, dev[1], C, out, 900, dev[2], dev[3], dab, 2 * C, dab[:, C:], 2 * C, gk[0], gk[1], gk[2], B, C)
    torch.cuda.synchronize()
    assert _err(dab[:, :C], ad.grad) <= TOL and _err(dab[:, C:], xd.grad) <= TOL
    for got, start, want in zip(gk, g0, (k1d.grad, k2d.grad, bd.grad)):
        assert _err(got.cpu().double() - start.double(), want) <= TOL          # accumulated into a non-zero gradient
    # a single incoming gradient: d2 = None
    dab2 = torch.empty(B, 2 * C, device=DEV)
    L.hadamard_bwd(d1.to(DEV), C, None, 0, dev[0], C, dev[1], C, out, 900, dev[2], dev[3], dab2, 2 * C, dab2[:, C:], 2 * C, gk[0], gk[1], gk[2], B, C)
    want = d1.double() * (1 - ref.detach() ** 2) * k1.double()
    assert _err(dab2[:, :C], want) <= TOL


def _keep(seed, B, width, p):
    u = counter_uniform(seed, np.arange(B * width, dtype=np.uint64))
    return torch.from_numpy(np.asarray(u, dtype=np.float64).reshape(B, width) >= p)


def test_dropout_sites_keep_rate_scale_independence_and_backward():
    B, C, p = 256, 500, 0.86
    s1, s2 = BimodalEngine._site_seed(5, 255, 0), BimodalEngine._site_seed(5, 255, 1)
    x = (torch.randn(B, C, generator=torch.Generator().manual_seed(0)).abs() + 0.1).to(DEV)
    y1, y2 = torch.empty(B, 900, device=DEV), torch.empty(B, C, device=DEV)
    L.dropout_f32(x, C, y1[:, 400:], 900, B, C, p, s1)
    L.dropout_f32(x, C, y2, C, B, C, p, s2)
    torch.cuda.synchronize()
    m1, m2 = (y1[:, 400:] != 0).cpu(), (y2 != 0).cpu()
    assert torch.equal(m1, _keep(s1, B, C, p)) and torch.equal(m2, _keep(s2, B, C, p))
    sd = (p * (1 - p) / (B * C)) ** 0.5
    for m in (m1, m2):
        rate = float(m.double().mean())
        assert abs(rate - (1 - p)) <= 4 * sd, (rate, sd)
    assert not torch.equal(m1, m2) and 0.05 < float((m1 & m2).double().mean() / m1.double().mean()) < 0.25     # independent: overlap ~ 0.14
    keep = m1.to(DEV)
    assert torch.allclose(y1[:, 400:][keep], x[keep] / (1 - p), rtol=1e-6, atol=0)
    # the backward is the same call on the gradient: it zeroes exactly the forward's zeros (in place)
    dy = torch.randn(B, C, device=DEV).abs() + 0.1
    d0 = dy.clone()
    L.dropout_f32(dy, C, dy, C, B, C, p, s1)
    torch.cuda.synchronize()
    assert torch.equal((dy != 0).cpu(), m1) and torch.allclose(dy[keep], d0[keep] / (1 - p), rtol=1e-6, atol=0)
    # p = 0: the identity
    L.dropout_f32(x, C, y2, C, B, C, 0.0, s2)
    assert torch.equal(y2, x)


def test_dropout_masks_follow_the_mask_epoch():
    """the mask epoch (lib.seed_epoch_set, what a HIP-graph replay refreshes) reaches this translation unit's copy: at epoch r a launch
    draws the mask of eager seed + r * MMRCA_SEED_EPOCH_STRIDE"""
    B, C, p, seed, stride = 16, 450, 0.86, 0x1234567, 1000003
    x = torch.ones(B, C, device=DEV)
    y = torch.empty(B, C, device=DEV)
    try:
        for r in (0, 2):
            L.seed_epoch_set(r)
            L.dropout_f32(x, C, y, C, B, C, p, seed)
            torch.cuda.synchronize()
            assert torch.equal(y.cpu() != 0, _keep(seed + r * stride, B, C, p)), r
    finally:
        L.seed_epoch_set(0)
        torch.cuda.synchronize()
    assert not torch.equal(_keep(seed, B, C, p), _keep(seed + 2 * stride, B, C, p))


# ------------------------------------------------------------------------------------------------------------------ golden chain
def _head_engine(dtype="fp32"):
    eng = BimodalEngine("distilbert", "eff_v2_medium", 4, dtype, image_size=64)
    return eng


def test_kernel_chain_reproduces_the_reference_classes_golden():
    """the engine's head, fed the golden's class-token rows and pooled feature: ctx_*, fused, ctx_fused and the logits to 1e-5 of each
    tensor's scale"""
    g = np.load(GOLDEN)
    eng = _head_engine()
    eng.init_parameters(0)
    eng.load_arrays({k: torch.from_numpy(v) for k, v in BR.golden_weights().items()}, strict=False)
    B = g["t"].shape[0]
    logits, sv = eng._head_forward(torch.from_numpy(g["t"]).to(DEV), torch.from_numpy(BR.golden_pooled()).to(DEV), B, 0.0, (0, 0))
    torch.cuda.synchronize()
    st = sv["st"]
    got = dict(ctx_text=st["gru_text"]["hseq"][1:B + 1], ctx_audio=st["gru_audio"]["hseq"][1:B + 1], fused=sv["comb"][:B, :400],
               ctx_fused=st["gru_bimodal"]["hseq"][1:B + 1], logits=logits)
    errs = {k: _err(v, g[k]) for k, v in got.items()}
    print("kernel chain vs the reference's HierarchicalBimodalFusion:", errs)
    eng.release_buffers()
    assert all(e < 1e-5 for e in errs.values()), errs


# ------------------------------------------------------------------------------------------------------------------ whole model
SIZE, B_MODEL = 224, 3
_ORC = {}


def _inputs(B=B_MODEL, size=SIZE, T=32):
    ids_np, mask_np = synth_captions(B, T, seed=21)
    images = torch.from_numpy(proc_input(f"bimodal.images.{size}", (B, 3, size, size)))
    return torch.from_numpy(ids_np), torch.from_numpy(mask_np), images


def _oracle():
    """the float64 restatement with the parameters of BimodalEngine.init_parameters(0), eval mode, run ONCE with its autograd graph:
    dict(orc, t, f, logits (attached), W)"""
    if not _ORC:
        eng = BimodalEngine("distilbert", "eff_v2_medium", 4, "fp32", image_size=SIZE)
        eng.init_parameters(0)
        orc = BR.OracleBimodal().eval()
        orc.load_engine(eng)
        orc = orc.double()
        eng.release_buffers()
        del eng
        for p in orc.parameters():
            p.requires_grad_(True)
        ids, mask, images = _inputs()
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        t = orc.text_model(ids, mask)[:, 0]
        f = orc.image_model(images.double())
        out = BR.bimodal_head(t, f, orc.head_weights())
        _ORC.update(orc=orc, t=t, f=f, logits=out["logits"], out=out)
        print(f"oracle: |t| {t.detach().norm(dim=1).tolist()}, |f| {f.detach().norm(dim=1).tolist()}, |h|max {float(out['ctx_fused'].detach().abs().max()):.3f}, "
              f"logits scale {float(out['logits'].detach().abs().max()):.3e}")
    return _ORC


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16x3", 1e-3), ("bf16x3f", 1e-3), ("bf16", 3e-2)])
def test_whole_model_logits_match_the_float64_restatement(dtype, tol):
    """eval mode, B = 3, EfficientNetV2-M at 224 + DistilBERT"""
    ref = _oracle()["logits"].detach()
    eng = BimodalEngine("distilbert", "eff_v2_medium", 4, dtype, image_size=SIZE)
    eng.init_parameters(0)
    ids, mask, images = _inputs()
    logits = eng.forward(ids.cuda(), mask.cuda(), images.cuda(), save=False, bn_train=False)
    torch.cuda.synchronize()
    e = _err(logits, ref)
    print(f"HierarchicalBimodalFusion @ {SIZE} {dtype}: logits vs float64 restatement {e:.3e}")
    eng.release_buffers()
    assert tuple(logits.shape) == (B_MODEL, 4) and torch.isfinite(logits).all() and e < tol, e


def test_swapping_two_rows_changes_the_other_rows_logits():
    """the GRUs run over the batch: with rows 0 and 1 swapped, row 2's logits move, and the engine matches the restatement on the swapped
    batch.  An implementation that treats the rows independently fails both."""
    o = _oracle()
    perm = [1, 0, 2]
    with torch.no_grad():
        ref = BR.bimodal_head(o["t"][perm], o["f"][perm], o["orc"].head_weights())["logits"]      # (the encoders treat rows independently)
    base = o["logits"].detach()
    assert _err(ref[2], base[2]) > 1e-3
    eng = BimodalEngine("distilbert", "eff_v2_medium", 4, "fp32", image_size=SIZE)
    eng.init_parameters(0)
    ids, mask, images = _inputs()
    l0 = eng.forward(ids.cuda(), mask.cuda(), images.cuda(), save=False).clone()
    l1 = eng.forward(ids[perm].cuda(), mask[perm].cuda(), images[perm].cuda(), save=False).clone()
    torch.cuda.synchronize()
    eng.release_buffers()
    move = float((l1[2] - l0[2]).abs().max() / l0.abs().max())
    print(f"swapping rows 0 and 1 moves row 2's logits by {move:.3e} of their scale; swapped batch vs restatement {_err(l1, ref):.3e}")
    assert move > 1e-3
    assert _err(l0, base) < 1e-3 and _err(l1, ref) < 1e-3
    assert not torch.equal(l0[0], l1[1])       # the same sample as step 0 and as step 1


def test_whole_model_gradients_match_float64_autograd():
    """fp32, B = 3, every parameter trainable, BatchNorm on running statistics, dropout off: each gradient within 2e-3 of
    max(|ref|max, 1e-3 * gmax) against float64 autograd of tests/bimodal_ref.py"""
    o = _oracle()
    orc = o["orc"]
    dl = torch.randn(B_MODEL, 4, generator=torch.Generator().manual_seed(3)) * 0.1
    (o["logits"] * dl.double()).sum().backward()
    eng = BimodalEngine("distilbert", "eff_v2_medium", 4, "fp32", image_size=SIZE)
    eng.init_parameters(0)
    ids, mask, images = _inputs()
    logits = eng.forward(ids.cuda(), mask.cuda(), images.cuda(), save=True, bn_train=False)
    assert _err(logits, o["logits"].detach()) < 1e-3
    eng.arena.g.zero_()
    eng.backward(dl.to(DEV))
    torch.cuda.synchronize()
    named = {"text_model." + k.replace("/", "."): p for k, p in orc.text_model.params.items()}
    named.update({"image_model." + k: p for k, p in orc.image_model.named_parameters()})
    named.update(orc.head_weights())
    gmax = max(float(p.grad.abs().max()) for p in named.values() if p.grad is not None)
    worst, worst_k, bad = 0.0, None, []
    for k in eng.param_keys:
        got, gr = eng.arena.view(k, "g").cpu().double(), named[k].grad
        if gr is None:
            assert float(got.abs().max()) == 0.0, k
            continue
        err, scale = (got - gr.view_as(got)).abs().max().item(), max(gr.abs().max().item(), 1e-3 * gmax)
        if err / scale > worst:
            worst, worst_k = err / scale, k
        if err > 2e-3 * scale:
            bad.append((k, err / scale))
    print("HierarchicalBimodalFusion fp32 vs float64 autograd: worst relative gradient error", worst, worst_k)
    eng.release_buffers()
    assert float(named["gru_bimodal.weight_hh_l0"].grad.abs().max()) > 0
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------------------------ train step
def _model(dtype="bf16x3f", size=SIZE, image_model="eff_v2_medium", batch=4):
    from garbage_classification_rca_amd.multimodal_model import HierarchicalBimodalFusion
    with contextlib.redirect_stdout(io.StringIO()):
        return HierarchicalBimodalFusion(4, 0.6, 0.0, 0.7, 256, "distilbert", batch, True, image_model_name=image_model, dtype=dtype,
                                         image_size=size, init_seed=1, build_unused_parameters=False)


def test_train_step_frozen_then_fine_tuning_and_other_batch_sizes():
    """hip_train_step drives the model unchanged: finite loss, the frozen phase moves only the head span, fine-tuning reaches image_emb
    and text_emb; loss.backward() through the module reaches the arena; B = 1 and a batch size other than the previous call's work"""
    from garbage_classification_rca_amd.optim import FlatAdamW
    from garbage_classification_rca_amd.training import FusedCrossEntropy, hip_train_step
    m = _model()
    m.train()
    eng = m.engine
    opt = FlatAdamW(m, lr=1e-3, weight_decay=1e-2)
    ids, mask, images = _inputs(4)
    labels = torch.tensor([0, 1, 2, 3], device=DEV)
    crit = FusedCrossEntropy(torch.tensor([0.7, 1.3, 0.9, 1.1], device=DEV), 0.1)
    p0 = eng.arena.p.clone()
    loss = hip_train_step(m, ids.cuda(), mask.cuda(), images.cuda(), labels, crit, opt)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    h0 = eng.groups["head"][0]
    assert torch.equal(eng.arena.p[:h0], p0[:h0]) and not torch.equal(eng.arena.p[h0:], p0[h0:])
    for k in ("gru_text.weight_hh_l0", "gru_audio.weight_ih_l0", "gru_bimodal.bias_hh_l0", "fusion.kernel1", "fusion.bias", "classifier.weight"):
        lo, _, n = eng.arena.offsets[k]
        assert not torch.equal(eng.arena.p[lo:lo + n], p0[lo:lo + n]), k
    for p in m.parameters():
        p.requires_grad = True
    p1 = eng.arena.p.clone()
    loss = hip_train_step(m, ids.cuda(), mask.cuda(), images.cuda(), labels, crit, opt)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(eng.arena.p).all()
    for grp in ("image_emb", "text_emb", "text_layer_3", "head"):
        lo, hi = eng.groups[grp]
        assert not torch.equal(eng.arena.p[lo:hi], p1[lo:hi]), grp
    # other batch sizes: the last, short batch of an epoch (B = 1) and back
    for B in (1, 3, 4):
        loss = hip_train_step(m, ids[:B].cuda(), mask[:B].cuda(), images[:B].cuda(), labels[:B], crit, opt)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all() and torch.isfinite(eng.arena.p).all(), B
    # autograd glue of the module: loss.backward() reaches the arena gradients
    eng.arena.g.zero_()
    out = m(ids.cuda(), mask.cuda(), images.cuda())
    assert tuple(out.shape) == (4, 4)
    out.sum().backward()
    torch.cuda.synchronize()
    assert float(m.gru_bimodal.weight_hh_l0.grad.abs().max()) > 0
    assert m.gru_bimodal.weight_hh_l0.grad.data_ptr() == eng.arena.view("gru_bimodal.weight_hh_l0", "g").data_ptr()
    # train mode drops with p = 0.86 whatever drop_ratio the constructor got; eval mode does not drop
    m.eval()
    with torch.no_grad():
        e1, e2 = m(ids.cuda(), mask.cuda(), images.cuda(), eval=True).clone(), m(ids.cuda(), mask.cuda(), images.cuda(), eval=True).clone()
    assert torch.equal(e1, e2)
    eng.release_buffers()


def test_graphed_step_computes_the_eager_step():
    """B = 4, EfficientNetV2-M at 128, bf16x3f: GraphedTrainStep (2 eager calls, 1 capture, 3 replays) against eager hip_train_step on twins
    from the same seed -- the same losses step by step, which requires every replay to draw the p = 0.86 masks of ITS step -- within the
    run-to-run noise of two eager runs (the criterion of tests/test_graph_gpu.py)"""
    from garbage_classification_rca_amd.optim import FlatSGD
    from garbage_classification_rca_amd.training import FusedCrossEntropy, GraphedTrainStep, hip_train_step
    B, n, size = 4, 5, 128
    data = []
    for k in range(n + 1):
        ids_np, mask_np = synth_captions(B, 16, seed=100 + k)
        g = torch.Generator(device="cuda").manual_seed(200 + k)
        data.append((torch.from_numpy(ids_np).cuda(), torch.from_numpy(mask_np).cuda(), torch.randn(B, 3, size, size, device="cuda", generator=g),
                     (torch.arange(B, device="cuda") % 4).to(torch.int32)))
    ma, mb, mc = (_model(size=size).train() for _ in range(3))
    oa, ob, oc = (FlatSGD(m, lr=2e-3, weight_decay=1e-2) for m in (ma, mb, mc))
    crit = FusedCrossEntropy(None, 0.0)
    graphed = GraphedTrainStep(mb, crit, ob, warmup=2)
    la, lb, lc = [], [], []
    with contextlib.redirect_stdout(io.StringIO()) as captured:
        for k in range(n):
            la.append(hip_train_step(ma, *data[k], crit, oa, None, text_pack=None))
            lb.append(graphed(*data[k]))
            lc.append(hip_train_step(mc, *data[k], crit, oc, None, text_pack=None))
        la.append(hip_train_step(ma, *data[n], crit, oa, None, text_pack=None))
        lb.append(hip_train_step(mb, *data[n], crit, ob, None, text_pack=None))
        lc.append(hip_train_step(mc, *data[n], crit, oc, None, text_pack=None))
    torch.cuda.synchronize()
    la, lb, lc = [float(x) for x in la], [float(x) for x in lb], [float(x) for x in lc]
    print("eager  ", [round(x, 4) for x in la])
    print("graphed", [round(x, 4) for x in lb])
    print("eager 2", [round(x, 4) for x in lc])
    assert graphed.replays == n - 2 and len(graphed._graphs) == 1, captured.getvalue()[-500:]
    assert L.seed_epoch_host() == 0
    dev, noise = max(abs(a - b) for a, b in zip(la, lb)), max(abs(a - c) for a, c in zip(la, lc))
    print("largest loss difference: graphed vs eager", dev, " eager vs eager", noise)
    assert dev <= 3.0 * noise + 2e-3, (la, lb, lc)
    assert len({round(x, 3) for x in lb}) > 3                      # (the losses do move from step to step)
    pa, pb, pc = ma.engine.arena.p, mb.engine.arena.p, mc.engine.arena.p
    rel, noise = float((pa - pb).norm() / pa.norm()), float((pa - pc).norm() / pa.norm())
    print("relative distance of the parameters after", n + 1, "steps: graphed vs eager", rel, " eager vs eager", noise)
    assert rel <= 3.0 * noise + 2e-5
    for m in (ma, mb, mc):
        m.engine.release_buffers()


# ------------------------------------------------------------------------------------------------------------------ drivers
def test_drivers_end_to_end(tmp_path):
    """main_both.py --late_fusion=bimodal on synthetic pairs writes a checkpoint with the reference's file-name pattern that holds the GRU
    weights and the unused RCA blocks; calculate_test_accuracy_both.py loads it and writes its report; MM_RCA loads it strictly"""
    from PIL import Image
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--late_fusion=bimodal", "--reverse", "--text_model=distilbert", "--image_model=eff_v2_medium", "--image_size", "224", "--tokens_max_len", "16", "--num_workers", "0"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main_both.py"), *common, "--synthetic", "8", "--epochs", "1", "--ft_epochs", "1", "--seed", "1"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "Starting Fine tuning!!" in r.stdout
    assert "Per-process batch size: 32" in r.stdout               # the reference's override (main_both.py:329-330), whatever --batch_size says
    ckpts = glob.glob(str(tmp_path / "model_weights" / "*" / "BEST_model_*_bimodal_*.pth"))
    assert ckpts, r.stdout[-2000:]
    sd = torch.load(ckpts[0], map_location="cpu")
    assert tuple(sd["gru_text.weight_hh_l0"].shape) == (1200, 400) and "cross_attention_1.W_query.weight" in sd
    rng = np.random.default_rng(0)
    for ci, c in enumerate(["Black", "Blue", "Green", "TTR"]):
        d = tmp_path / "Val" / c
        d.mkdir(parents=True)
        arr = (rng.random((48, 60, 3)) * 255).astype(np.uint8)
        Image.fromarray(arr).save(d / f"{['chip_bag', 'pizza_box', 'banana_peel', 'aa_batteries'][ci]}_0.png")
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "calculate_test_accuracy_both.py"), *common, "--dataset_folder_name", str(tmp_path / "Val"),
                         "--model_path", ckpts[0]], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout[-1500:] + r2.stderr[-3000:]
    assert "Test accuracy random both" in r2.stdout
    assert glob.glob(str(tmp_path / "multimodal_model_report_test_set_acc_*_always_both.csv"))
    from garbage_classification_rca_amd.multimodal_model import MM_RCA
    with contextlib.redirect_stdout(io.StringIO()):
        mm = MM_RCA(4, 0.6, 0.0, 0.7, 256, "distilbert", 32, True, False, False, image_model_name="eff_v2_medium", dtype="bf16x3f", image_size=224)
    mm.load_state_dict(sd, strict=True)
    mm.engine.release_buffers()

