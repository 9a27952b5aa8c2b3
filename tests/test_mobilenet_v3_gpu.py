"""MobileNetV3-Large on the MI355X: the depthwise 5x5 kernels and the hard-swish / hard-sigmoid activation codes against float64,
the whole classifier against the float64 restatement of torchvision's mobilenet_v3_large (tests/mobilenet_v3_ref.py), training through
autograd, the flat optimizer and a captured HIP graph, and the image driver / evaluator end to end."""
import contextlib
import glob
import io
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import classifiers as C     # noqa: E402
from garbage_classification_rca_amd import lib as L             # noqa: E402
from garbage_classification_rca_amd.procedural import proc_input  # noqa: E402
from tests.mobilenet_v3_ref import MobileNetV3Large              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _rel(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _rows(t):                      # NCHW -> NHWC rows [B*H*W, C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ---------------------------------------------------------------------------------------------------- depthwise 5x5
DW5_SHAPES = [(2, 7, 9, 8), (2, 7, 9, 72), (1, 40, 40, 72), (2, 9, 7, 120), (1, 10, 12, 672), (1, 7, 9, 960), (2, 11, 6, 20)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B,H,W,C", DW5_SHAPES)
def test_dwconv5x5_matches_float64(B, H, W, C, stride, dtype):
    """forward, input gradient and weight gradient against F.conv2d(groups=C) in float64 on the same (rounded) operands.  fp32: 1e-5
    (25 fp32 products, measured < 1e-6); bf16: the output / dx are stored in bf16 -> one rounding, 2^-8 relative to the largest entry;
    dw is fp32 (sums over the pixels of bf16 products, fp32 accumulation): 1e-4"""
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C + stride)
    dt = L.dtype_code(dtype)
    x = torch.randn(B, C, H, W, generator=g).to(dtype)
    w = (torch.randn(C, 1, 5, 5, generator=g) * 0.2).to(dtype)
    y64 = F.conv2d(x.double(), w.double(), stride=stride, padding=2, groups=C)
    Ho, Wo = y64.shape[2], y64.shape[3]
    assert (Ho, Wo) == ((H - 1) // stride + 1, (W - 1) // stride + 1)
    dy = torch.randn(B, C, Ho, Wo, generator=g).to(dtype)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    (F.conv2d(xd, wd, stride=stride, padding=2, groups=C) * dy.double()).sum().backward()
    xr, wr, dyr = _rows(x).contiguous().to(DEV), w.view(C, 25).contiguous().to(DEV), _rows(dy).contiguous().to(DEV)
    y = torch.empty(B * Ho * Wo, C, dtype=dtype, device=DEV)
    L.dwconv5x5_fwd(xr, wr, y, B, H, W, C, stride, dt)
    ws = torch.empty(24 << 20, dtype=torch.uint8, device=DEV)
    dx = torch.empty(B * H * W, C, dtype=dtype, device=DEV)
    dw = torch.full((C, 25), 0.5, device=DEV)                      # accumulates: += onto 0.5
    L.dwconv5x5_bwd(dyr, xr, wr, dx, dw, B, H, W, C, stride, dt, ws=ws)
    torch.cuda.synchronize()
    tol = 1e-5 if dtype == torch.float32 else 2 ** -8
    assert _rel(y, _rows(y64)) < tol
    assert _rel(dx, _rows(xd.grad)) < tol
    dw_ref = wd.grad.view(C, 25)
    assert _rel(dw - 0.5, dw_ref) < 1e-4
    # dx = None and dw = None forms, the atomic weight gradient (no workspace), and bitwise reproducibility with a workspace
    dx2 = torch.zeros_like(dx)
    L.dwconv5x5_bwd(dyr, xr, wr, dx2, None, B, H, W, C, stride, dt)
    dw_atomic = torch.zeros(C, 25, device=DEV)
    L.dwconv5x5_bwd(dyr, xr, wr, None, dw_atomic, B, H, W, C, stride, dt)
    dw_a, dw_b = torch.zeros(C, 25, device=DEV), torch.zeros(C, 25, device=DEV)
    L.dwconv5x5_bwd(dyr, xr, wr, None, dw_a, B, H, W, C, stride, dt, ws=ws)
    L.dwconv5x5_bwd(dyr, xr, wr, None, dw_b, B, H, W, C, stride, dt, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx)
    assert _rel(dw_atomic, dw_ref) < 1e-4
    assert torch.equal(dw_a, dw_b) and _rel(dw_a, dw_ref) < 1e-4


# ---------------------------------------------------------------------------------------------------- hard-swish / hard-sigmoid
ACTS = {L.CONV_HSWISH: F.hardswish, L.CONV_HSIGMOID: F.hardsigmoid}


def _act_inputs(rows, C, g):
    u = torch.randn(rows, C, generator=g, dtype=torch.float64) * 3.0
    u.view(-1)[:6] = torch.tensor([-3.0, 0.0, 3.0, -3.0, 3.0, 0.0], dtype=torch.float64)    # aten's kinks, exactly representable
    return u


def _act_ref(u, act):
    ud = u.clone().requires_grad_(True)
    y = ACTS[act](ud)
    y.backward(torch.ones_like(y))
    return y.detach(), ud.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("act", [L.CONV_HSWISH, L.CONV_HSIGMOID])
def test_bias_act_hard_activations_match_float64(act, dtype):
    """mmrca_bias_act_fwd / _bwd: y = act(x + bias), dx = dy * act'(x + bias) (aten's boundary conventions at -3 / +3), dbias += sum.
    The first six columns carry bias 0.5 and x = kink - 0.5 (exact in bf16), so the sum x + bias lands exactly on -3 / 0 / +3.
    fp32 1e-6; bf16 output storage 2^-8"""
    g = torch.Generator().manual_seed(act)
    rows, Cn = 70, 24
    bias = (0.5 * torch.randn(Cn, generator=g, dtype=torch.float64)).to(dtype).double()
    bias[:6] = 0.5
    u = _act_inputs(rows, Cn, g)
    u.view(-1)[:6] -= 0.5
    u = u.to(dtype).double()
    y_ref, d_ref = _act_ref(u + bias, act)
    assert torch.equal((u + bias).view(-1)[:6], torch.tensor([-3.0, 0.0, 3.0, -3.0, 3.0, 0.0], dtype=torch.float64))
    dt = L.dtype_code(dtype)
    xd, bd = u.to(dtype).to(DEV), bias.to(dtype).to(DEV)
    y = torch.empty_like(xd)
    L.bias_act_fwd(xd, bd, y, rows, Cn, act, dt)
    dy = torch.ones_like(xd)
    dx, db = torch.empty_like(xd), torch.zeros(Cn, device=DEV)
    L.bias_act_bwd(dy, xd, bd, dx, db, rows, Cn, act, dt)
    torch.cuda.synchronize()
    tol = 1e-6 if dtype == torch.float32 else 2 ** -8
    assert _rel(y, y_ref) < tol
    assert torch.equal(dx.double().cpu().view(-1)[:6], d_ref.view(-1)[:6].to(dtype).double())       # the kinks: exactly aten's values
    assert _rel(dx, d_ref) < tol
    assert _rel(db, d_ref.sum(0)) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("act", [L.CONV_HSWISH, L.CONV_HSIGMOID])
def test_batchnorm_with_hard_activations_matches_float64(act, dtype):
    """BatchNorm (batch statistics) + act forward -- the plain / bf16 x8 apply pass, the fused residual form and the folded forward
    with the finish inside -- and the backward (reduce + apply, and the sums that mmrca_se_dx accumulates), against float64 autograd of
    act(batch_norm(z)) on the same rounded operands (the kinks themselves are pinned by the bias_act test above).  Bounds: fp32 1e-5
    (forward) / 1e-4 (backward: sums over rows); bf16 output storage 2^-7, gradients 2^-6"""
    g = torch.Generator().manual_seed(10 + act)
    rows, Cn = 512, 32
    z = torch.randn(rows, Cn, generator=g, dtype=torch.float64).to(dtype).double()
    gamma = (1.0 + 0.5 * torch.randn(Cn, generator=g, dtype=torch.float64)).to(dtype).double()
    beta = (0.5 * torch.randn(Cn, generator=g, dtype=torch.float64)).to(dtype).double()
    dy = torch.randn(rows, Cn, generator=g, dtype=torch.float64).to(dtype).double()
    zd, gd, bd = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    mean, var = zd.mean(0), zd.var(0, unbiased=False)
    u = (zd - mean) / torch.sqrt(var + 1e-3) * gd + bd
    y_ref = ACTS[act](u)
    (y_ref * dy).sum().backward()
    dt = L.dtype_code(dtype)
    Z, G, Bt = z.to(dtype).to(DEV), gamma.to(dtype).to(DEV), beta.to(dtype).to(DEV)
    st = torch.zeros(2, Cn, device=DEV)
    rm, rv = torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV)
    L.bn_stats(Z, st[0], st[1], rm, rv, rows, Cn, Cn, 1e-3, 0.01, True, dt)
    y = torch.empty_like(Z)
    L.bn_act_fwd(Z, st[0], st[1], G, Bt, y, rows, Cn, act, dt)
    tol_f = 1e-5 if dtype == torch.float32 else 2 ** -7
    tol_b = 1e-4 if dtype == torch.float32 else 2 ** -6
    torch.cuda.synchronize()
    assert _rel(y, y_ref.detach()) < tol_f
    # running statistics with momentum 0.01 (unbiased variance)
    assert _rel(rm, 0.01 * z.mean(0)) < 1e-5 and _rel(rv, 0.99 + 0.01 * z.var(0, unbiased=True)) < 1e-5
    dx, dgam, dbet, scratch = torch.empty_like(Z), torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV), torch.zeros(2 * Cn, device=DEV)
    L.bn_act_bwd(dy.to(dtype).to(DEV), Z, st[0], st[1], G, Bt, dx, dgam, dbet, scratch, rows, Cn, act, True, dt)
    torch.cuda.synchronize()
    assert _rel(dx, zd.grad) < tol_b and _rel(dgam, gd.grad) < tol_b and _rel(dbet, bd.grad) < tol_b
    if dtype != torch.bfloat16:
        return
    # bf16 x8 forms: residual fused into the apply pass, the folded forward, and the BatchNorm sums of mmrca_se_dx (s = 1, dpool = 0:
    # dx = dy, the sums those of dy)
    res = torch.randn(rows, Cn, generator=g).to(dtype).to(DEV)
    out = torch.empty_like(Z)
    L.bn_act_fwd_res(Z, st[0], st[1], G, Bt, res, None, out, rows, Cn, act, rows // 2, dt)
    s1, s2, shift = torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    L.bn_moments(Z, s1, s2, shift, rows, Cn, Cn, dt)
    yf, mf, rf = torch.empty_like(Z), torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    rm2, rv2 = torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV)
    L.bn_act_fwd_fin(Z, s1, s2, shift, G, Bt, None, None, yf, mf, rf, rm2, rv2, rows, Cn, act, rows // 2, 1e-3, 0.01, dt)
    B2, HW = 2, rows // 2
    sums = torch.zeros(2 * Cn, device=DEV)
    s_ones = torch.ones(B2, Cn, dtype=dtype, device=DEV)
    dpool = torch.zeros(B2, Cn, dtype=dtype, device=DEV)
    dx_se = torch.empty_like(Z)
    dyd = dy.to(dtype).to(DEV)
    L.se_dx(dyd, s_ones, dpool, dx_se, B2, HW, Cn, dt, bn=(Z, st[0], st[1], G, Bt, act, sums))
    dx3, dg3, db3 = torch.empty_like(Z), torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    L.bn_act_bwd(dx_se, Z, st[0], st[1], G, Bt, dx3, dg3, db3, sums, rows, Cn, act, True, dt, sums_ready=True)
    torch.cuda.synchronize()
    assert _rel(out.double().cpu() - res.double().cpu(), y_ref.detach()) < 2 ** -6
    assert _rel(yf, y_ref.detach()) < tol_f
    assert torch.equal(dx_se, dyd)
    assert _rel(dx3, zd.grad) < tol_b and _rel(dg3, gd.grad) < tol_b and _rel(db3, bd.grad) < tol_b


@pytest.mark.parametrize("act", [L.CONV_HSWISH, L.CONV_HSIGMOID])
def test_flat_batchnorm_backward_reduction_with_hard_activations(act):
    """the opt-in flat BatchNorm-backward reduction (bn_act_bwd_reduce_flat_k: a workspace, bf16, C % 8 == 0, enough rows) with the new
    codes, against float64 autograd of act(batch_norm(z)).  Bounds as the two-pass form above: bf16 gradients 2^-6"""
    g = torch.Generator().manual_seed(20 + act)
    rows, Cn = 16384, 32
    z = torch.randn(rows, Cn, generator=g, dtype=torch.float64).to(torch.bfloat16).double()
    gamma = (1.0 + 0.5 * torch.randn(Cn, generator=g, dtype=torch.float64)).to(torch.bfloat16).double()
    beta = (0.5 * torch.randn(Cn, generator=g, dtype=torch.float64)).to(torch.bfloat16).double()
    dy = torch.randn(rows, Cn, generator=g, dtype=torch.float64).to(torch.bfloat16).double()
    zd, gd, bd = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    u = (zd - zd.mean(0)) / torch.sqrt(zd.var(0, unbiased=False) + 1e-3) * gd + bd
    (ACTS[act](u) * dy).sum().backward()
    dt = L.BF16
    Z, G, Bt, DY = (t.to(torch.bfloat16).to(DEV) for t in (z, gamma, beta, dy))
    st = torch.zeros(2, Cn, device=DEV)
    L.bn_stats(Z, st[0], st[1], torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV), rows, Cn, Cn, 1e-3, 0.01, True, dt)
    ws = torch.empty(4 << 20, dtype=torch.float32, device=DEV)
    dx, dgam, dbet, scratch = torch.empty_like(Z), torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV), torch.zeros(2 * Cn, device=DEV)
    L.load().mmrca_bn_flat_set(3)
    try:
        L.bn_act_bwd(DY, Z, st[0], st[1], G, Bt, dx, dgam, dbet, scratch, rows, Cn, act, True, dt, ws=ws)
        torch.cuda.synchronize()
    finally:
        L.load().mmrca_bn_flat_set(0)
    assert _rel(dx, zd.grad) < 2 ** -6 and _rel(dgam, gd.grad) < 2 ** -6 and _rel(dbet, bd.grad) < 2 ** -6


# ---------------------------------------------------------------------------------------------------- the whole classifier
def _reference_of(m):
    ref = MobileNetV3Large(m.n_classes).double()
    ref.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.cpu() for k, v in m.state_dict().items()}, strict=True)
    return ref


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3f"])
@pytest.mark.parametrize("side", [64, 320])
def test_mbnetlarge_matches_the_float64_restatement(side, dtype):
    """eval mode (running statistics): logits, the head weight gradient and the stem weight gradient of sum(logits * dl) against the
    float64 restatement + Linear.  Bounds as test_classifier_gpu.py's for the conv backbones, except the bf16x3f logits at 64 x 64:
    measured 1.7e-3 (a 2 x 2 final feature map: the 1280 features average fewer bf16 roundings; 7.4e-4 at 320 x 320) -> 3e-3.
    The stem gradient of this randomly initialised network is ~1e-9 of the head's (it vanishes through the 15 blocks), so the direction
    is compared on the normalised vectors"""
    torch.manual_seed(0)
    B = 2
    m = C.MBNetLarge(4, False, dtype=dtype, device=DEV, image_size=side)
    eng = m.engine
    # non-trivial running statistics (fresh ones are 0 / 1): the eval path normalises with them
    g = torch.Generator().manual_seed(5)
    for k, t in eng.conv.buffers.items():
        if k.endswith("running_mean"):
            t.copy_(0.1 * torch.randn(t.shape, generator=g))
        elif k.endswith("running_var"):
            t.copy_(1.0 + 0.2 * torch.rand(t.shape, generator=g))
    ref = _reference_of(m).eval()
    images = torch.from_numpy(proc_input(f"mb.{side}", (B, 3, side, side)))
    out = ref(images.double())
    dl = torch.randn(B, 4, dtype=torch.float64)
    (out * dl).sum().backward()
    eng.arena.g.zero_()
    logits = eng.forward(None, None, images.to(DEV), drop_p=0.0, seed=1, save=True, bn_train=False)
    eng.backward(dl.float().to(DEV), train_text=False, train_image=True)
    torch.cuda.synchronize()
    err = _rel(logits, out.detach())
    print(f"mb {side} {dtype}: logits {err:.3e}")
    assert err < (1e-4 if dtype == "fp32" else (1e-3 if side == 320 else 3e-3)), err
    gdw = eng.arena.view("head.weight", "g")
    gw = _rel(gdw, ref.classifier[3].weight.grad)
    stem = eng.arena.view("image_model.features.0.0.weight", "g").double().cpu()
    og = ref.features[0][0].weight.grad
    print(f"mb {side} {dtype}: head grad {gw:.3e}")
    if dtype == "fp32":
        g1 = _rel(stem, og)
        print(f"mb {side} {dtype}: stem grad {g1:.3e}")
        assert gw < 1e-4 and g1 < 1e-3, (gw, g1)
    else:
        g1 = float((stem - og).norm() / og.norm())
        cos = float((stem.flatten() / stem.norm()) @ (og.flatten() / og.norm()))
        print(f"mb {side} {dtype}: stem grad rel L2 {g1:.3e} cos {cos:.5f}")
        assert gw < 5e-2 and g1 < 1.5e-1 and cos > 0.99, (gw, g1, cos)
    eng.release_buffers()


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3f"])
def test_mbnetlarge_train_mode_batch_statistics_and_state_dict_round_trip(dtype):
    """train mode: logits on batch statistics; after the step every running_mean / running_var is the momentum-0.01 update (unbiased
    variance) and num_batches_tracked is 1.  Then a strict state_dict round trip in both directions.  Bounds: logits fp32 1e-3, bf16x3f
    1e-1 (measured 5.2e-2: batch statistics over B = 4 samples of a 2 x 2 map -- 16 values per channel -- magnify the bf16 roundings).
    The running-statistics error is taken relative to the layer's batch standard deviation (many batch means are exactly 0 in float64
    -- a 1x1 convolution of a freshly normalised input -- and ~1e-9 in fp32)."""
    B, side = 4, 64
    m = C.MBNetLarge(4, False, dtype=dtype, device=DEV, image_size=side)
    ref = _reference_of(m).train()
    for mod in ref.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    images = torch.from_numpy(proc_input("mb.train", (B, 3, side, side)))
    out = ref(images.double())
    logits = m.engine.forward(None, None, images.to(DEV), drop_p=0.0, seed=1, save=True, bn_train=True)
    torch.cuda.synchronize()
    err = _rel(logits, out.detach())
    print(f"mb train {dtype}: logits {err:.3e}")
    assert err < (1e-3 if dtype == "fp32" else 1e-1), err
    sd = m.state_dict()
    rsd = ref.state_dict()
    worst = 0.0
    for k, v in rsd.items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == 1, k
        elif k.endswith("running_var"):
            worst = max(worst, _rel(sd[k], v))
        elif k.endswith("running_mean"):
            std = ((rsd[k[: -len("mean")] + "var"] - 0.99) / 0.01).clamp_min(0).sqrt().max()
            worst = max(worst, float((sd[k].double().cpu() - v).abs().max() / (0.01 * std)))
    print(f"mb train {dtype}: running statistics {worst:.3e}")
    assert worst < (1e-4 if dtype == "fp32" else 1e-1), worst          # measured 1.0e-6 / 3.3e-2 (the bf16 forward's error, as the logits)
    # strict round trips: ours -> the restatement (done above) and the restatement -> ours
    g = torch.Generator().manual_seed(3)
    new = {k: (torch.randn(v.shape, generator=g, dtype=torch.float64) * 0.01 if v.is_floating_point() else v + 4) for k, v in rsd.items()}
    m2 = C.MBNetLarge(4, False, dtype=dtype, device=DEV, image_size=side)
    m2.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in new.items()}, strict=True)
    back = m2.state_dict()
    assert list(back) == list(rsd)
    for k, v in new.items():
        assert torch.equal(back[k].cpu(), v.float() if v.is_floating_point() else v), k
    m.engine.release_buffers()


def test_mbnetlarge_trains_through_autograd_and_flat_optimizer():
    """loss.backward() through the one autograd node; the frozen phase steps the head only: features.* and classifier.0.* stay
    bit-identical"""
    from garbage_classification_rca_amd.optim import FlatSGD
    m = C.MBNetLarge(4, True, device=DEV, dtype="bf16", image_size=64)
    m.train()
    opt = FlatSGD(m, 1e-2, 0.0)
    images = torch.from_numpy(proc_input("mb.autograd", (4, 3, 64, 64))).to(DEV)
    labels = torch.tensor([0, 1, 2, 3], device=DEV)
    h0 = m.engine.groups["head"][0]
    enc0 = m.engine.arena.p[:h0].clone()
    cls0 = m.classifier._modules["0"].weight.detach().clone()
    head0 = m.classifier._modules["3"].weight.detach().clone()
    F.cross_entropy(m(images), labels).backward()
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    assert torch.equal(m.engine.arena.p[:h0], enc0) and torch.equal(m.classifier._modules["0"].weight.detach(), cls0)
    assert not torch.equal(m.classifier._modules["3"].weight.detach(), head0)
    for p in m.parameters():
        p.requires_grad = True
    F.cross_entropy(m(images), labels).backward()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(m.engine.arena.p[:h0], enc0) and not torch.equal(m.classifier._modules["0"].weight.detach(), cls0)
    m.engine.release_buffers()


def test_mbnetlarge_graphed_step_reproduces_the_eager_steps():
    """B = 4, 64 x 64, bf16x3f: GraphedTrainStep (2 eager calls, 1 capture, 3 replays) against eager hip_train_step on a twin from the
    same seed, within the eager-vs-eager spread (test_graph_gpu.py's rule)"""
    from garbage_classification_rca_amd.optim import FlatSGD
    from garbage_classification_rca_amd.training import FusedCrossEntropy, GraphedTrainStep, hip_train_step
    B, n, side = 4, 6, 64
    data = []
    for k in range(n):
        images = torch.from_numpy(proc_input(f"mb.graph.{k}", (B, 3, side, side))).to(DEV)
        ids, mask = torch.zeros(B, 1, dtype=torch.int64, device=DEV), torch.ones(B, 1, dtype=torch.int64, device=DEV)
        data.append((ids, mask, images, torch.tensor([k % 4, 1, 2, 3], device=DEV)))
    ms = [C.MBNetLarge(4, False, device=DEV, image_size=side) for _ in range(3)]
    for m in ms:
        m.train()
        for p in m.parameters():
            p.requires_grad = True
    oa, ob, oc = (FlatSGD(m, lr=2e-3, weight_decay=1e-2) for m in ms)
    crit = FusedCrossEntropy(None, 0.0)
    graphed = GraphedTrainStep(ms[1], crit, ob, warmup=2)
    la, lb, lc = [], [], []
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(n):
            la.append(float(hip_train_step(ms[0], *data[k], crit, oa)))
            lb.append(float(graphed(*data[k])))
            lc.append(float(hip_train_step(ms[2], *data[k], crit, oc)))
    torch.cuda.synchronize()
    print("eager  ", la, "\ngraphed", lb, "\neager 2", lc)
    assert graphed.replays == n - 2 and len(graphed._graphs) == 1
    dev, noise = max(abs(a - b) for a, b in zip(la, lb)), max(abs(a - c) for a, c in zip(la, lc))
    assert dev <= 3.0 * noise + 2e-3, (la, lb, lc)
    pa, pb, pc = (m.engine.arena.p for m in ms)
    rel, noise = float((pa - pb).norm() / pa.norm()), float((pa - pc).norm() / pa.norm())
    assert rel <= 3.0 * noise + 2e-5, (rel, noise)
    for m in ms:
        m.engine.release_buffers()


def _tiny_folder(tmp_path):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    for split in ("Train", "Val"):
        for ci, c in enumerate(["Black", "Blue", "Green", "TTR"]):
            d = tmp_path / f"Tiny_{split}" / c
            d.mkdir(parents=True)
            for k in range(2 if split == "Train" else 3):
                arr = (rng.random((int(rng.integers(36, 72)), int(rng.integers(36, 72)), 3)) * 255).astype(np.uint8)
                arr[:, :, ci % 3] = 255 - 40 * ci
                Image.fromarray(arr).save(d / f"{['chip_bag', 'pizza_box', 'banana_peel', 'aa_batteries'][ci]}_{k}.png")


def test_main_image_and_evaluator_run_mb_on_a_tiny_folder(tmp_path):
    """main_image.py --image_model=mb --image_size 64: both phases and a best-val checkpoint with torchvision's key names; then
    calculate_test_accuracy_image.py on it writes the report CSV"""
    _tiny_folder(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--image_model=mb", "--num_workers", "0", "--image_size", "64"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main_image.py"), "--dataset_folder_name=Tiny", "--epochs", "2", "--ft_epochs", "1",
                        "--seed", "1", *common], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "Starting Fine tuning!!" in r.stdout and "Fine Tuning: Val set accuracy" in r.stdout
    ckpts = sorted(glob.glob(str(tmp_path / "model_weights" / "mb" / "BEST_model_mb_*.pth")), key=os.path.getmtime)
    assert ckpts, r.stdout[-3000:]
    sd = torch.load(ckpts[0], map_location="cpu")
    for k in ("features.0.0.weight", "features.16.1.running_var", "classifier.0.weight"):
        assert k in sd, k
    assert tuple(sd["classifier.3.weight"].shape) == (4, 1280)
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "calculate_test_accuracy_image.py"), "--model_path", ckpts[0],
                         "--dataset_folder_name", str(tmp_path / "Tiny_Val"), *common], cwd=tmp_path, env=env, capture_output=True, text=True,
                        timeout=600)
    assert r2.returncode == 0, r2.stdout[-1500:] + r2.stderr[-3000:]
    assert "Test accuracy:" in r2.stdout
    assert glob.glob(str(tmp_path / "test_set_reports" / "mb" / "image_model_mb_report_test_set_acc_*.csv"))
