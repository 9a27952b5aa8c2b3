"""The hierarchical late-fusion model on the GPU: every kernel of csrc/hier_head.hip against float64 on the same inputs, the forward chain
against the golden recorded from the reference's own class, the encoder taps (values, gradients, launch sequence), the whole model
against the float64 restatement (tests/hierarchical_ref.py) in the four dtype modes, a train step and the drivers.

Tolerances: the kernels are fp32 products with fp32 sums, compared with float64 on identical (bf16-rounded where applicable) inputs:
1e-5 of the largest entry, what tests/test_classifier_gpu.py applies to mmrca_linear_cls_fwd / _bwd.  Whole-model logits: the project's
north-star 1e-3 in fp32 / bf16x3 / bf16x3f and this suite's bf16 bound 3e-2 (tests/test_conv_gpu.py).  Gradients: the bounds of the tests
they extend (1e-3 conv taps, 2e-3 text taps and whole model, of max(|ref|max, 1e-3 * gmax))."""
import contextlib
import glob
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import lib as L                                          # noqa: E402
from garbage_classification_rca_amd import engine as E                                        # noqa: E402
from garbage_classification_rca_amd.hierarchical_engine import HierarchicalEngine              # noqa: E402
from garbage_classification_rca_amd.procedural import proc_input, proc_state, synth_captions, counter_uniform  # noqa: E402
from oracle import arch as OS                                                                  # noqa: E402
from tests import hierarchical_ref as HR                                                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hierarchical_goldens.npz")
DEV = "cuda:0"
SEG = [0, 1280, 3840, 5888, 6656, 7424, 8192]
LINEARS = {"final_hierarchical_image.weight": (512, 5888), "final_hierarchical_image.bias": (512,),
           "final_hierarchical_text.weight": (512, 2304), "final_hierarchical_text.bias": (512,),
           "final_hierarchical_all.weight": (4, 1024), "final_hierarchical_all.bias": (4,)}


def _rel(a, ref):
    ref = torch.as_tensor(ref).double().cpu()
    return float((torch.as_tensor(a).double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _same(a, b):       # equal up to the summation order of the fp32 atomics in the encoders' weight-gradient / BatchNorm sums
    return float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())


def _differs(a, b):
    return float((a - b).abs().max()) > 1e-2 * float(b.abs().max())


def _rows(t):          # NCHW -> [B*H*W, C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,k,C", [(28, 7, 160), (30, 7, 160), (14, 6, 512), (15, 6, 512)])
@pytest.mark.parametrize("B", [1, 3, 16, 64])
def test_window_average_pool_forward_and_backward_match_float64(B, H, k, C, dtype):
    """forward: NCHW-ordered fp32 vector in a column window of a wider buffer, sums in fp32 (bf16 maps: float64 on the rounded values);
    backward: adds d / k^2 into a NON-ZERO gradient buffer and leaves the uncovered pixels (30 -> rows / columns 28, 29; 15 -> 12..14)
    bit-identical"""
    g = torch.Generator().manual_seed(B * 1000 + H)
    x = torch.randn(B, C, H, H, generator=g).to(dtype)
    oh = H // k
    n, ld, off = C * oh * oh, C * oh * oh + 24, 8
    out = torch.full((B, ld), 7.0, device=DEV)
    L.hier_pool_fwd(_rows(x).to(DEV), out[:, off:], ld, B, H, H, C, k, L.dtype_code(dtype))
    ref = F.avg_pool2d(x.double(), k, k).flatten(1)
    assert ref.shape[1] == n
    e = _rel(out[:, off:off + n], ref)
    assert e < 1e-5, e
    assert bool((out[:, :off] == 7.0).all()) and bool((out[:, off + n:] == 7.0).all())       # nothing outside the window
    d = torch.randn(B, ld, generator=g)
    dx0 = torch.randn(B, C, H, H, generator=g).to(dtype)
    dx = _rows(dx0).to(DEV)
    L.hier_pool_bwd(d.to(DEV)[:, off:], ld, dx, B, H, H, C, k, L.dtype_code(dtype))
    torch.cuda.synchronize()
    up = d[:, off:off + n].double().view(B, C, oh, oh).repeat_interleave(k, 2).repeat_interleave(k, 3) / (k * k)
    want = dx0.double().clone()
    want[:, :, :oh * k, :oh * k] += up
    got = dx.view(B, H, H, C).permute(0, 3, 1, 2).cpu()
    tol = 1e-5 if dtype == torch.float32 else 2 ** -8           # the sum is STORED in the map's dtype: one bf16 rounding
    assert _rel(got, want) < tol, _rel(got, want)
    assert torch.equal(got[:, :, oh * k:, :], dx0[:, :, oh * k:, :]) and torch.equal(got[:, :, :, oh * k:], dx0[:, :, :, oh * k:])


def _keep(seed, B, width, p):
    u = counter_uniform(seed, np.arange(B * width, dtype=np.uint64))
    return torch.from_numpy(np.asarray(u, dtype=np.float64).reshape(B, width) >= p)


def _norm_ref(raw, keep_scale=None):
    x = torch.cat([HR.l2n(raw[:, a:b]) for a, b in zip(SEG, SEG[1:])], 1)
    return x if keep_scale is None else x * keep_scale


@pytest.mark.parametrize("B", [1, 3, 16, 64])
def test_normalise_concatenate_matches_float64_forward_and_backward(B):
    g = torch.Generator().manual_seed(B)
    raw = torch.randn(B, 8192, generator=g) * torch.rand(1, 8192, generator=g)
    raw[:, :1280] *= 1e-5                           # (the pooled feature of a freshly initialised backbone is this small)
    rd = raw.to(DEV)
    x, inv, draw = torch.empty(B, 8192, device=DEV), torch.empty(B, 6, device=DEV), torch.empty(B, 8192, device=DEV)
    L.hier_norm_fwd(rd, x, inv, B, 8192, SEG, 3, 0.0, 1, 2)
    r64 = raw.double().requires_grad_(True)
    ref = _norm_ref(r64)
    assert _rel(x, ref.detach()) < 1e-5
    ref_inv = torch.stack([1 / r64[:, a:b].norm(dim=1) for a, b in zip(SEG, SEG[1:])], 1).detach()
    assert float(((inv.double().cpu() - ref_inv).abs() / ref_inv).max()) < 1e-5
    dx = torch.randn(B, 8192, generator=g)
    ref.backward(dx.double())
    L.hier_norm_bwd(dx.to(DEV), rd, inv, draw, B, 8192, SEG, 3, 0.0, 1, 2)
    torch.cuda.synchronize()
    for a, b in zip(SEG, SEG[1:]):                  # per segment: their gradient scales differ by 1e5
        e = _rel(draw[:, a:b], r64.grad[:, a:b])
        assert e < 1e-5, (a, e)


def test_zero_segment_neither_hangs_nor_faults_and_gives_the_references_nan():
    raw = torch.randn(2, 8192)
    raw[1, 3840:5888] = 0
    x, inv = torch.empty(2, 8192, device=DEV), torch.empty(2, 6, device=DEV)
    L.hier_norm_fwd(raw.to(DEV), x, inv, 2, 8192, SEG, 3, 0.0, 1, 2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x[1, 3840:5888]).all()) and bool(torch.isfinite(x[0]).all()) and bool(torch.isfinite(x[1, :3840]).all())


def test_dropout_masks_of_the_image_and_text_vectors():
    """p = 0.6: both masks recovered from the saved xi | xt; keep counts binomial within 5 sigma; survivors scaled by 1 / (1 - p); the
    two masks differ; same seed same mask, other seed another; the backward uses the forward's mask"""
    B, p, si, st = 64, 0.6, 0x1234567, 0x7654321
    g = torch.Generator().manual_seed(0)
    raw = (torch.randn(B, 8192, generator=g).abs() + 0.1)           # no zeros: a zero output is a dropped one
    rd = raw.to(DEV)
    x, inv = torch.empty(B, 8192, device=DEV), torch.empty(B, 6, device=DEV)
    L.hier_norm_fwd(rd, x, inv, B, 8192, SEG, 3, p, si, st)
    x2 = torch.empty_like(x)
    L.hier_norm_fwd(rd, x2, inv, B, 8192, SEG, 3, p, si, st)
    x3 = torch.empty_like(x)
    L.hier_norm_fwd(rd, x3, inv, B, 8192, SEG, 3, p, si + 1, st + 1)
    torch.cuda.synchronize()
    xc = x.cpu()
    mi, mt = xc[:, :5888] != 0, xc[:, 5888:] != 0
    for m, w, seed in ((mi, 5888, si), (mt, 2304, st)):
        n = B * w
        assert abs(int(m.sum()) - n * (1 - p)) < 5 * (n * p * (1 - p)) ** 0.5
        assert torch.equal(m, _keep(seed, B, w, p))
    assert not torch.equal(mi[:, :2304], mt)
    keep = torch.cat((mi, mt), 1)
    assert _rel(x, _norm_ref(raw.double(), keep.double() / (1 - p))) < 1e-5
    assert torch.equal(x, x2) and not torch.equal(x3 != 0, x != 0)
    dx = torch.randn(B, 8192, generator=g)
    draw = torch.empty(B, 8192, device=DEV)
    L.hier_norm_bwd(dx.to(DEV), rd, inv, draw, B, 8192, SEG, 3, p, si, st)
    torch.cuda.synchronize()
    r64 = raw.double().requires_grad_(True)
    _norm_ref(r64, keep.double() / (1 - p)).backward(dx.double())
    for a, b in zip(SEG, SEG[1:]):
        assert _rel(draw[:, a:b], r64.grad[:, a:b]) < 1e-5


def test_dropout_masks_follow_the_mask_epoch():
    """the mask epoch (lib.seed_epoch_set, what a HIP-graph replay refreshes) reaches this translation unit's copy: at epoch r a launch
    draws the masks of eager seeds + r * MMRCA_SEED_EPOCH_STRIDE"""
    B, p, si, st, stride = 16, 0.6, 0x1234567, 0x7654321, 1000003
    raw = (torch.randn(B, 8192, generator=torch.Generator().manual_seed(0)).abs() + 0.1).to(DEV)
    x, inv = torch.empty(B, 8192, device=DEV), torch.empty(B, 6, device=DEV)
    try:
        for r in (0, 2):
            L.seed_epoch_set(r)
            L.hier_norm_fwd(raw, x, inv, B, 8192, SEG, 3, p, si, st)
            torch.cuda.synchronize()
            xc = x.cpu()
            assert torch.equal(xc[:, :5888] != 0, _keep(si + r * stride, B, 5888, p)), r
            assert torch.equal(xc[:, 5888:] != 0, _keep(st + r * stride, B, 2304, p)), r
    finally:
        L.seed_epoch_set(0)
        torch.cuda.synchronize()


def _linear_operands(B, K, seed=0):
    g = torch.Generator().manual_seed(seed + B + K)
    X = torch.randn(B, K + 64, generator=g) * K ** -0.5
    W = torch.randn(512, K, generator=g)
    b = torch.randn(512, generator=g) * 0.1
    dY = torch.randn(B, 1024, generator=g)
    return X, W, b, dY


def _linear_run(X, W, b, dY, B, K, with_dx=True):
    Xd, Wd, bd, dYd = X.to(DEV), W.to(DEV), b.to(DEV), dY.to(DEV)
    Y = torch.full((B, 1024), -3.0, device=DEV)
    ws = torch.empty(L.hier_linear_workspace_bytes(B, 512, K), dtype=torch.uint8, device=DEV)
    L.hier_linear_relu_fwd(Xd, K + 64, Wd, bd, Y[:, 512:], 1024, ws, B, 512, K)
    dW, db = torch.ones(512, K, device=DEV), torch.ones(512, device=DEV)          # accumulate: start from ones
    dX = torch.full((B, K + 64), 5.0, device=DEV) if with_dx else None
    L.hier_linear_relu_bwd(dYd[:, 512:], 1024, Y[:, 512:], 1024, Xd, K + 64, Wd, dW, db, dX, K + 64, ws if with_dx else None, B, 512, K)
    torch.cuda.synchronize()
    return Y, dW, db, dX


@pytest.mark.parametrize("K", [5888, 2304])
@pytest.mark.parametrize("B", [1, 3, 16, 64, 256])
def test_wide_linear_relu_matches_float64(B, K):
    """Y, dW (+=), db (+=), dX within 1e-5 of the largest entry; operands read out of wider buffers (row pitches K + 64 / 1024)"""
    X, W, b, dY = _linear_operands(B, K)
    Y, dW, db, dX = _linear_run(X, W, b, dY, B, K)
    x64, W64 = X[:, :K].double(), W.double()
    ref = torch.relu(x64 @ W64.T + b.double())
    assert _rel(Y[:, 512:], ref) < 1e-5, _rel(Y[:, 512:], ref)
    assert bool((Y[:, :512] == -3.0).all())
    dZ = dY[:, 512:].double() * (Y[:, 512:].cpu().double() > 0)             # (the kernel's own gate: a pre-activation within 1e-7 of 0 may fall either side)
    assert _rel(dW - 1, dZ.T @ x64) < 1e-5, _rel(dW - 1, dZ.T @ x64)
    assert _rel(db - 1, dZ.sum(0)) < 1e-5
    assert _rel(dX[:, :K], dZ @ W64) < 1e-5
    assert bool((dX[:, K:] == 5.0).all())


def test_weight_gradients_are_bitwise_reproducible_and_dx_is_optional():
    X, W, b, dY = _linear_operands(16, 5888)
    a = _linear_run(X, W, b, dY, 16, 5888)
    c = _linear_run(X, W, b, dY, 16, 5888, with_dx=False)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(a[2], c[2]) and c[3] is None


def test_kernels_reject_shapes_they_do_not_cover():
    t = torch.zeros(4, 8192, device=DEV)
    with pytest.raises(L.MmrcaError):
        L.hier_pool_fwd(torch.zeros(16, 6, device=DEV), t, 8192, 1, 4, 4, 6, 2, L.F32)          # C % 4
    with pytest.raises(L.MmrcaError):
        L.hier_pool_fwd(torch.zeros(16, 8, device=DEV), t, 8192, 1, 4, 4, 8, 5, L.F32)          # window larger than the map
    with pytest.raises(L.MmrcaError):
        L.hier_norm_fwd(t, t.clone(), torch.zeros(4, 6, device=DEV), 4, 8192, [0, 10, 5], 1, 0.0, 0, 0)
    with pytest.raises(L.MmrcaError):
        L.hier_linear_relu_fwd(t, 8192, torch.zeros(512, 1000, device=DEV), torch.zeros(512, device=DEV), torch.zeros(4, 512, device=DEV), 512,
                               torch.zeros(1 << 20, device=DEV), 4, 512, 1000)                   # K % 256
    with pytest.raises(L.MmrcaError):
        L.hier_linear_relu_fwd(t, 8192, torch.zeros(512, 2304, device=DEV), torch.zeros(512, device=DEV), torch.zeros(4, 512, device=DEV), 512,
                               torch.zeros(16, device=DEV), 4, 512, 2304)                        # workspace too small


def test_forward_kernel_chain_reproduces_the_reference_classes_logits():
    """pool -> normalise -> linears on the golden's stage maps, class-token rows and procedural weights: the logits (and xi | xt, hi | ht)
    the reference's own Hierarchical produced, within 1e-5"""
    g = np.load(GOLDEN)
    B, ld = 2, 8192
    s3, s6 = torch.from_numpy(proc_input("hier.stage3", (2, 160, 30, 30))), torch.from_numpy(proc_input("hier.stage6", (2, 512, 15, 15)))
    pooled = torch.from_numpy(proc_input("hier.pooled", (2, 1280)))
    W = {k: torch.from_numpy(v).to(DEV) for k, v in proc_state(LINEARS).items()}
    raw = torch.zeros(B, ld, device=DEV)
    L.hier_pool_fwd(pooled.to(DEV), raw, ld, B, 1, 1, 1280, 1, L.F32)
    L.hier_pool_fwd(_rows(s3).to(DEV), raw[:, 1280:], ld, B, 30, 30, 160, 7, L.F32)
    L.hier_pool_fwd(_rows(s6).to(DEV), raw[:, 3840:], ld, B, 15, 15, 512, 6, L.F32)
    for j, k in enumerate(("t0", "t2", "t4")):
        L.hier_pool_fwd(torch.from_numpy(g[k]).to(DEV), raw[:, SEG[3 + j]:], ld, B, 1, 1, 768, 1, L.F32)
    x, inv, h = torch.empty(B, ld, device=DEV), torch.empty(B, 6, device=DEV), torch.empty(B, 1024, device=DEV)
    L.hier_norm_fwd(raw, x, inv, B, ld, SEG, 3, 0.0, 0, 0)
    ws = torch.empty(L.hier_linear_workspace_bytes(B, 512, 5888), dtype=torch.uint8, device=DEV)
    L.hier_linear_relu_fwd(x, ld, W["final_hierarchical_image.weight"], W["final_hierarchical_image.bias"], h, 1024, ws, B, 512, 5888)
    L.hier_linear_relu_fwd(x[:, 5888:], ld, W["final_hierarchical_text.weight"], W["final_hierarchical_text.bias"], h[:, 512:], 1024, ws, B, 512, 2304)
    logits = torch.empty(B, 4, device=DEV)
    L.linear_cls_fwd(h, 1024, W["final_hierarchical_all.weight"], W["final_hierarchical_all.bias"], logits, B, 1024, 4, 0.0, 0, L.F32)
    torch.cuda.synchronize()
    errs = {k: _rel(v, g[k]) for k, v in (("x", x), ("h", h), ("logits", logits))}
    print("HIP forward chain vs the reference's Hierarchical:", errs)
    assert all(e < 1e-5 for e in errs.values()), errs


# ------------------------------------------------------------------------------------------------------------------ encoder taps
@contextlib.contextmanager
def _call_log():
    """names of the libmmrca wrappers called, in order"""
    log, saved = [], {}
    for name, fn in list(vars(L).items()):
        if callable(fn) and not name.startswith("_") and getattr(fn, "__module__", None) == L.__name__ and isinstance(fn, type(_call_log)):
            saved[name] = fn
            setattr(L, name, (lambda f, n: (lambda *a, **kw: (log.append(n), f(*a, **kw))[1]))(fn, name))
    try:
        yield log
    finally:
        for name, fn in saved.items():
            setattr(L, name, fn)


LAUNCHERS = ("gemm", "conv", "bn_", "dwconv", "se_", "rowpool", "residual", "hier_", "add_layernorm", "mha", "embed", "nchw", "im2row", "split", "cast")


def _launches(log):
    return [n for n in log if n.startswith(LAUNCHERS)]


def _text_engine():
    from garbage_classification_rca_amd.classifier_engine import ClassifierEngine
    eng = ClassifierEngine("distilbert", 4, dtype="fp32")
    eng.init_parameters(5)
    with torch.no_grad():                   # biases and LayerNorm parameters off their (0, 1) initialisation
        gen = torch.Generator().manual_seed(6)
        for k in eng.param_keys:
            v = eng.arena.view(k)
            if v.dim() == 1:
                v.add_((torch.randn(v.shape, generator=gen) * 0.05).to(DEV))
    orc = HR.TappedTextEncoder(OS.TEXT_SPECS["distilbert"], 0.0).double().eval()
    orc.load_flat({k: eng.arena.view(k).detach().cpu().double() for k in eng.param_keys if k.startswith("text_model.")}, "text_model.")
    return eng, orc


@pytest.mark.parametrize("packed", [False, True])
def test_text_taps_and_their_gradients_match_the_float64_oracle(packed):
    """DistilBERT fp32: the class-token rows of hidden_states[2] / [4] equal the oracle's (1e-3, the bound of
    test_text_encoder_cls_matches_transformers_golden), and with a loss on all three outputs every parameter gradient is within 2e-3 of
    max(|ref|max, 1e-3 * gmax); the gradients differ from the run without tap gradients; the launch sequence does not change"""
    eng, orc = _text_engine()
    B, T = 4, 32
    ids_np, mask_np = synth_captions(B, T, seed=11)
    ids, mask = torch.from_numpy(ids_np), torch.from_numpy(mask_np)
    pack = E.make_text_pack(mask_np, "cuda") if packed else None
    assert (pack is not None) == packed
    eng.refresh_working_copy(force=True)
    with _call_log() as log0:
        cls0, sv0 = eng._text_forward(ids.cuda(), mask.cuda(), True, 0.0, 0, pack)
    with _call_log() as log1:
        cls, sv = eng._text_forward(ids.cuda(), mask.cuda(), True, 0.0, 0, pack, taps=(2, 4))
    assert _launches(log0) == _launches(log1) and len(_launches(log0)) > 20 and sv0["taps"] == {}
    assert torch.equal(cls0, cls)
    for p in orc.parameters():
        p.requires_grad_(True)
    last, (t2, t4) = orc(ids, mask)
    for got, ref in ((cls, last[:, 0]), (sv["taps"][2], t2), (sv["taps"][4], t4)):
        assert tuple(got.shape) == (B, 768) and _rel(got, ref.detach()) < 1e-3, _rel(got, ref.detach())
    gen = torch.Generator().manual_seed(1)
    a0, a2, a4 = (torch.randn(B, 768, generator=gen) for _ in range(3))
    ((last[:, 0] * a0.double()).sum() + (t2 * a2.double()).sum() + (t4 * a4.double()).sum()).backward()
    eng.arena.g.zero_()
    eng._text_backward(a0.to(DEV), sv)                 # no tap gradients
    g_plain = eng.arena.g.clone()
    eng.arena.g.zero_()
    cls, sv = eng._text_forward(ids.cuda(), mask.cuda(), True, 0.0, 0, pack, taps=(2, 4))
    eng._text_backward(a0.to(DEV), sv, dtaps={2: a2.to(DEV), 4: a4.to(DEV)})
    torch.cuda.synchronize()
    named = {"text_model." + k.replace("/", "."): p for k, p in orc.params.items()}
    gmax = max(float(p.grad.abs().max()) for p in named.values() if p.grad is not None)
    worst = 0.0
    for k in eng.param_keys:
        if not k.startswith("text_model."):
            continue
        got, gr = eng.arena.view(k, "g").cpu().double(), named[k].grad
        if gr is None:
            assert float(got.abs().max()) == 0.0, k
            continue
        err, scale = (got - gr.view_as(got)).abs().max().item(), max(gr.abs().max().item(), 1e-3 * gmax)
        worst = max(worst, err / scale)
        assert err <= 2e-3 * scale, (k, err, scale)
    print(f"text taps packed={packed}: worst relative gradient error {worst:.2e}")
    lo, hi = eng.groups["text_layer_0"]
    assert _differs(g_plain[lo:hi], eng.arena.g[lo:hi])                   # layers 0-3 see the tap gradients
    lo, hi = eng.groups["text_layer_5"]
    assert _same(g_plain[lo:hi], eng.arena.g[lo:hi])                      # the layers above the taps do not
    eng.release_buffers()


@pytest.mark.parametrize("train", [True, False])
def test_conv_taps_and_their_gradients_match_the_fp32_oracle(train):
    """ConvEncoder fp32 at 64 x 64 (stage maps 4 x 4 and 2 x 2; windows k = 2 and k = 1), injected stochastic-depth masks, against the fp32
    oracle with the same tap loss added -- test_backbone_features_gradients_and_running_stats_match_oracle_fp32 with taps, its bound:
    every tensor within 1e-3 of max(|ref|max, 1e-3 * gmax)"""
    from tests.test_conv_gpu import _conv_pair, _sd_blocks
    enc, own, orc = _conv_pair("eff_v2_medium", torch.float32)
    B, size = 3, 64
    g = torch.Generator().manual_seed(9)
    images = torch.randn(B, 3, size, size, generator=g)
    orc.train(train)
    blocks = _sd_blocks(orc)
    if train and blocks:
        keep = (torch.rand(len(blocks), B, generator=g) > 0.3).float()
        for m, kk in zip(blocks, keep):
            m.stochastic_depth.keep = kk
        enc.injected_keep = keep
    for p in orc.parameters():
        p.requires_grad_(True)
    s3, s6, feat_ref = orc(images)
    assert tuple(s3.shape) == (B, 160, 4, 4) and tuple(s6.shape) == (B, 512, 2, 2)
    p3_ref, p6_ref = F.avg_pool2d(s3, 2, 2).flatten(1), F.avg_pool2d(s6, 1, 1).flatten(1)
    n3, n6 = p3_ref.shape[1], p6_ref.shape[1]
    ld = n3 + n6
    out = torch.zeros(B, ld, device=DEV)
    with _call_log() as log1:
        feat = enc.forward(images.cuda(), save=True, train=train, taps={"stage3": (2, out, ld), "stage6": (1, out[:, n3:], ld)})
    assert _rel(feat, feat_ref.detach()) < 1e-3 and _rel(out[:, :n3], p3_ref.detach()) < 1e-3 and _rel(out[:, n3:], p6_ref.detach()) < 1e-3
    dfeat, d3, d6 = torch.randn(feat_ref.shape, generator=g), torch.randn(B, n3, generator=g), torch.randn(B, n6, generator=g)
    ((feat_ref * dfeat).sum() + (p3_ref * d3).sum() + (p6_ref * d6).sum()).backward()
    d = torch.cat((d3, d6), 1).to(DEV)
    with _call_log() as blog1:
        enc.backward(dfeat.cuda(), dtaps={"stage3": (d, ld), "stage6": (d[:, n3:], ld)})
    torch.cuda.synchronize()
    named = dict(orc.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in named.values() if p.grad is not None)
    worst = 0.0
    tapped = {k: own.g["image_model." + k].clone() for k, _ in enc.param_entries()}
    for k, _ in enc.param_entries():
        got, ref = tapped[k].cpu(), named[k].grad
        err, scale = (got - ref.view_as(got)).abs().max().item(), max(ref.abs().max().item(), 1e-3 * gmax)
        worst = max(worst, err / scale)
        assert err <= 1e-3 * scale, (k, err, scale)
    print(f"conv taps train={train}: worst relative gradient error {worst:.2e}")
    # the same forward / backward without the arguments: the same launches minus the pools, and other gradients in stages 1-3
    if not train:                              # (a second train-mode forward would move the running statistics again)
        for t in own.g.values():
            t.zero_()
        with _call_log() as log0:
            enc.forward(images.cuda(), save=True, train=False)
        with _call_log() as blog0:
            enc.backward(dfeat.cuda())
        torch.cuda.synchronize()
        assert [n for n in _launches(log1) if n != "hier_pool_fwd"] == _launches(log0) and _launches(log1).count("hier_pool_fwd") == 2
        assert [n for n in _launches(blog1) if n != "hier_pool_bwd"] == _launches(blog0) and _launches(blog1).count("hier_pool_bwd") == 2
        assert "hier_pool_fwd" not in log0 and "hier_pool_bwd" not in blog0
        for stage in ("stage1", "stage2", "stage3"):
            k = next(k for k, _ in enc.param_entries() if k.startswith(stage + ".") and k.endswith("0.weight"))
            assert _differs(tapped[k], own.g["image_model." + k]), k
        k = "final_conv.0.weight"
        assert _same(tapped[k], own.g["image_model." + k])                # above both taps: unchanged
    enc.release()


# ------------------------------------------------------------------------------------------------------------------ whole model
_ORACLE = {}


def _inputs(B, size, T=32):
    ids_np, mask_np = synth_captions(B, T, seed=21)
    images = torch.from_numpy(proc_input(f"hier.images.{size}", (B, 3, size, size)))
    return torch.from_numpy(ids_np), torch.from_numpy(mask_np), images


def _oracle_logits(size):
    """float64 logits of tests/hierarchical_ref.py with the parameters of HierarchicalEngine.init_parameters(0), eval mode"""
    if size not in _ORACLE:
        eng = HierarchicalEngine("distilbert", "eff_v2_medium", 4, "fp32", image_size=size)
        eng.init_parameters(0)
        orc = HR.OracleHierarchical().eval()
        orc.load_engine(eng)
        orc = orc.double()
        ids, mask, images = _inputs(2, size)
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        with torch.no_grad():
            s3, s6, pooled = orc.image_model(images.double())
            print(f"oracle @ {size}: |pooled| {pooled.norm(dim=1).tolist()}, |p3| {F.avg_pool2d(s3, 7, 7).flatten(1).norm(dim=1).tolist()}, "
                  f"|p6| {F.avg_pool2d(s6, 6, 6).flatten(1).norm(dim=1).tolist()}")
            _ORACLE[size] = orc(ids, mask, images.double())
        eng.release_buffers()
        del eng
    return _ORACLE[size]


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16x3", 1e-3), ("bf16x3f", 1e-3), ("bf16", 3e-2)])
@pytest.mark.parametrize("size", [448, 480])
def test_whole_model_logits_match_the_float64_restatement(size, dtype, tol):
    """eval mode, B = 2: the project's north-star 1e-3 in fp32 / bf16x3 / bf16x3f, this suite's bf16 bound 3e-2 in bf16"""
    ref = _oracle_logits(size)
    eng = HierarchicalEngine("distilbert", "eff_v2_medium", 4, dtype, image_size=size)
    eng.init_parameters(0)
    ids, mask, images = _inputs(2, size)
    logits = eng.forward(ids.cuda(), mask.cuda(), images.cuda(), save=False, bn_train=False)
    torch.cuda.synchronize()
    e = _rel(logits, ref)
    print(f"Hierarchical @ {size} {dtype}: logits vs float64 restatement {e:.3e}")
    eng.release_buffers()
    assert torch.isfinite(logits).all() and e < tol, e


def test_whole_model_gradients_match_float64_autograd():
    """fp32, B = 2 at 448, every parameter trainable, BatchNorm on running statistics, dropout off: each gradient within 2e-3 of
    max(|ref|max, 1e-3 * gmax) against float64 autograd of tests/hierarchical_ref.py"""
    size, B = 448, 2
    eng = HierarchicalEngine("distilbert", "eff_v2_medium", 4, "fp32", image_size=size)
    eng.init_parameters(0)
    orc = HR.OracleHierarchical().eval()
    orc.load_engine(eng)
    orc = orc.double()
    for p in orc.parameters():
        p.requires_grad_(True)
    ids, mask, images = _inputs(B, size)
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    ref = orc(ids, mask, images.double())
    dl = torch.randn(B, 4, generator=torch.Generator().manual_seed(3)) * 0.1
    (ref * dl.double()).sum().backward()
    logits = eng.forward(ids.cuda(), mask.cuda(), images.cuda(), save=True, bn_train=False)
    assert _rel(logits, ref.detach()) < 1e-3
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
    print("Hierarchical fp32 vs float64 autograd: worst relative gradient error", worst, worst_k)
    eng.release_buffers()
    assert not bad, bad[:10]


def _model(dtype="bf16x3f", size=448, drop=0.6):
    from garbage_classification_rca_amd.multimodal_model import Hierarchical
    with contextlib.redirect_stdout(io.StringIO()):
        return Hierarchical(4, drop, 0.0, 0.7, 256, "distilbert", 4, True, dtype=dtype, image_size=size, init_seed=1)


def test_train_step_frozen_then_fine_tuning():
    """hip_train_step drives the model unchanged: finite loss, the frozen phase moves only the head span, fine-tuning reaches image_emb
    and text_emb"""
    from garbage_classification_rca_amd.optim import FlatAdamW
    from garbage_classification_rca_amd.training import FusedCrossEntropy, hip_train_step
    m = _model()
    m.train()
    eng = m.engine
    opt = FlatAdamW(m, lr=1e-3, weight_decay=1e-2)
    ids, mask, images = _inputs(4, 448)
    labels = torch.tensor([0, 1, 2, 3], device=DEV)
    crit = FusedCrossEntropy(torch.tensor([0.7, 1.3, 0.9, 1.1], device=DEV), 0.1)
    p0 = eng.arena.p.clone()
    loss = hip_train_step(m, ids.cuda(), mask.cuda(), images.cuda(), labels, crit, opt)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    h0 = eng.groups["head"][0]
    assert torch.equal(eng.arena.p[:h0], p0[:h0]) and not torch.equal(eng.arena.p[h0:], p0[h0:])
    for p in m.parameters():
        p.requires_grad = True
    p1 = eng.arena.p.clone()
    loss = hip_train_step(m, ids.cuda(), mask.cuda(), images.cuda(), labels, crit, opt, text_pack=E.make_text_pack(mask.numpy(), "cuda"))
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(eng.arena.p).all()
    for grp in ("image_emb", "text_emb", "text_layer_1", "text_layer_3", "image_stage_stage3", "head"):
        lo, hi = eng.groups[grp]
        assert not torch.equal(eng.arena.p[lo:hi], p1[lo:hi]), grp
    # autograd glue of the module: loss.backward() reaches the arena gradients
    eng.arena.g.zero_()
    out = m(ids.cuda(), mask.cuda(), images.cuda())
    out.sum().backward()
    torch.cuda.synchronize()
    assert float(eng.arena.view("final_hierarchical_image.weight", "g").abs().max()) > 0
    eng.release_buffers()


def test_drivers_end_to_end(tmp_path):
    """main_both.py --late_fusion=hierarchical on synthetic pairs writes a checkpoint with the reference's file-name pattern,
    calculate_test_accuracy_both.py loads it and writes its report; any other fusion name still exits 1"""
    from PIL import Image
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--late_fusion=hierarchical", "--reverse", "--text_model=distilbert", "--image_size", "448", "--tokens_max_len", "16", "--num_workers", "0"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main_both.py"), *common, "--synthetic", "8", "--epochs", "1", "--ft_epochs", "1",
                        "--batch_size", "4", "--batch_size_FT", "4", "--seed", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "Starting Fine tuning!!" in r.stdout and "HIP graph captured" not in r.stdout
    ckpts = glob.glob(str(tmp_path / "model_weights" / "*" / "BEST_model_*_hierarchical_*.pth"))
    assert ckpts, r.stdout[-2000:]
    sd = torch.load(ckpts[0], map_location="cpu")
    assert tuple(sd["final_hierarchical_image.weight"].shape) == (512, 5888) and "cross_attention_1.W_query.weight" in sd
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
    r3 = subprocess.run([sys.executable, os.path.join(ROOT, "main_both.py"), "--late_fusion=gated", "--synthetic", "8"], cwd=tmp_path, env=env,
                        capture_output=True, text=True, timeout=300)
    assert r3.returncode == 1 and "Wrong late fusion strategy" in r3.stdout
