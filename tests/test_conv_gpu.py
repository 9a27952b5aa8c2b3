"""Conv image backbones (EfficientNetV2-M/L, ShuffleNetV2 x2.0) on the HIP path: every csrc/conv.hip kernel against the
torch op it replaces, and the whole backbones (forward features, every parameter gradient, BatchNorm running statistics)
against the oracle (oracle/conv_models.py: torchvision architectures restated, "torchvision-unpinned").  Needs an MI355X."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import lib as L                     # noqa: E402
from garbage_classification_rca_amd.engine import MMRCAEngine           # noqa: E402
from garbage_classification_rca_amd.conv_engine import ConvEncoder       # noqa: E402
from oracle import conv_models as CM                                     # noqa: E402
from oracle import model as O                                            # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    L.load()
    torch.manual_seed(0)


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def rows(t):      # NCHW -> [B*H*W, C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def nchw(r, B, H, W):
    return r.view(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


TOL = {torch.float32: 1e-5, torch.bfloat16: 2e-2}


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("stride", [1, 2])
def test_im2row_gemm_is_conv3x3_and_col2im_is_its_input_gradient(dt, stride):
    B, C, H, W, Co = 2, 10, 9, 7, 6
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, H, W, generator=g).to(dt).float()
    w = (torch.randn(Co, C, 3, 3, generator=g) * 0.2).to(dt).float()
    xr = rows(x).cuda().to(dt)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    K = 9 * C
    col = torch.empty(B * Ho * Wo, K, device="cuda", dtype=dt)
    L.im2row3x3(xr, col, B, H, W, C, stride, K, L.dtype_code(dt))
    y = col.float().cpu() @ w.view(Co, -1).t()
    ref = F.conv2d(x, w, None, stride, 1)
    assert rel(nchw(y, B, Ho, Wo), ref) < TOL[dt]
    dcol = torch.randn(B * Ho * Wo, K, generator=g).to(dt)
    dx = torch.empty(B * H * W, C, device="cuda", dtype=dt)
    L.col2im3x3(dcol.cuda(), dx, B, H, W, C, stride, K, L.dtype_code(dt))
    # reference: fold the patch gradient back with autograd of unfold
    xr2 = x.clone().requires_grad_(True)
    u = F.unfold(xr2, 3, padding=1, stride=stride)                      # [B, C*9, L] channel-major like the kernel
    (u.transpose(1, 2).reshape(-1, K) * dcol.float()).sum().backward()
    assert rel(nchw(dx.float().cpu(), B, H, W), xr2.grad) < TOL[dt]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", [70, 72])      # 72: the 8-channel kernels (stride 1: two rows x four output pixels per thread)
@pytest.mark.parametrize("H,W", [(8, 11), (15, 15), (7, 4), (1, 9)])      # odd heights: the second row of the last strip is masked
def test_depthwise_conv_fwd_bwd(dt, stride, C, H, W):
    B = 3
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, C, H, W, generator=g).to(dt).float().requires_grad_(True)
    w = (torch.randn(C, 1, 3, 3, generator=g) * 0.3).to(dt).float().requires_grad_(True)
    ref = F.conv2d(x, w, None, stride, 1, groups=C)
    Ho, Wo = ref.shape[2:]
    xd, wd = rows(x.detach()).cuda().to(dt), w.detach().view(C, 9).cuda().to(dt)
    y = torch.empty(B * Ho * Wo, C, device="cuda", dtype=dt)
    L.dwconv3x3_fwd(xd, wd, y, B, H, W, C, stride, L.dtype_code(dt))
    assert rel(nchw(y.float().cpu(), B, Ho, Wo), ref.detach()) < TOL[dt]
    dy = torch.randn(ref.shape, generator=g).to(dt).float()
    ref.backward(dy)
    dx = torch.empty(B * H * W, C, device="cuda", dtype=dt)
    dw = torch.zeros(C, 9, device="cuda")
    L.dwconv3x3_bwd(rows(dy).cuda().to(dt), xd, wd, dx, dw, B, H, W, C, stride, L.dtype_code(dt))
    assert rel(nchw(dx.float().cpu(), B, H, W), x.grad) < TOL[dt]
    assert rel(dw.cpu().view(C, 1, 3, 3), w.grad) < (1e-4 if dt == torch.float32 else 2e-2)
    # the same through the workspace forms (streaming kernel with per-thread sums, or -- small workspace -- per-block partial sums;
    # a second kernel adds them up instead of atomics); dw accumulates
    for ws_floats in (1 << 20, 40000):
        dw2 = torch.full((C, 9), 0.25, device="cuda")
        L.dwconv3x3_bwd(rows(dy).cuda().to(dt), xd, wd, None, dw2, B, H, W, C, stride, L.dtype_code(dt), ws=torch.empty(ws_floats, device="cuda"))
        assert rel(dw2.cpu().view(C, 1, 3, 3) - 0.25, w.grad) < (1e-4 if dt == torch.float32 else 2e-2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("act", [L.CONV_NONE, L.CONV_SILU, L.CONV_RELU])
@pytest.mark.parametrize("train", [True, False])
def test_batchnorm_act_fwd_bwd_and_running_stats(dt, act, train):
    R, C, eps = 1000, 70, 1e-3
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(R, C, generator=g) * 2 + 0.5).to(dt).float().requires_grad_(True)
    gam = (torch.rand(C, generator=g) + 0.5).to(dt).float().requires_grad_(True)
    bet = (torch.randn(C, generator=g) * 0.3).to(dt).float().requires_grad_(True)
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    bn = torch.nn.BatchNorm1d(C, eps=eps)
    with torch.no_grad():
        bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
    bn.train(train)
    u = F.batch_norm(x, bn.running_mean, bn.running_var, gam, bet, train, 0.1, eps)
    ref = {L.CONV_NONE: u, L.CONV_SILU: F.silu(u), L.CONV_RELU: F.relu(u)}[act]
    xd = x.detach().cuda().to(dt)
    mean, rstd = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    rm, rv = rm0.clone().cuda(), rv0.clone().cuda()
    L.bn_stats(xd, mean, rstd, rm, rv, R, C, C, eps, 0.1 if train else 0.0, train, L.dtype_code(dt))
    y = torch.empty(R, C, device="cuda", dtype=dt)
    gd, bd = gam.detach().cuda().to(dt), bet.detach().cuda().to(dt)
    L.bn_act_fwd(xd, mean, rstd, gd, bd, y, R, C, act, L.dtype_code(dt))
    assert rel(y, ref.detach()) < TOL[dt]
    if train:
        assert rel(rm, bn.running_mean) < 1e-5 and rel(rv, bn.running_var) < 1e-5
    dy = torch.randn(R, C, generator=g).to(dt).float()
    ref.backward(dy)
    dx = torch.empty(R, C, device="cuda", dtype=dt)
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    scratch = torch.empty(2 * C, device="cuda")
    L.bn_act_bwd(dy.cuda().to(dt), xd, mean, rstd, gd, bd, dx, dg, db, scratch, R, C, act, train, L.dtype_code(dt))
    tol = 2e-4 if dt == torch.float32 else 3e-2
    assert rel(dx, x.grad) < tol and rel(dg, gam.grad) < tol and rel(db, bet.grad) < tol


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,c,sq", [(5, 320, 20), (64, 1824, 76), (3, 3840, 160), (2, 48, 12)])
def test_fused_squeeze_excitation_mlp_fwd_bwd(dt, B, c, sq):
    """mmrca_se_mlp_fwd / _bwd (one launch forward, two backward) against torch autograd of torchvision's SqueezeExcitation MLP
    (fc1 + SiLU + fc2 + sigmoid; multimodal_model.py:113-126 builds it inside efficientnet_v2_m): the scale, the saved
    pre-activations, dpool and the four parameter gradients (accumulated onto a non-zero start).  EfficientNetV2-M's squeeze widths
    20 / 76 are not multiples of 8 (these were general-kernel GEMMs); 3,840 / 160 is EfficientNetV2-L's widest block."""
    g = torch.Generator().manual_seed(B * c + sq)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(dt).float()
    pooled, w1, b1 = r(B, c, scale=0.5), r(sq, c, scale=c ** -0.5), r(sq, scale=0.2)
    w2, b2, ds = r(c, sq, scale=sq ** -0.5), r(c, scale=0.2), r(B, c, scale=0.3)
    P, W1, B1, W2, B2 = (t.clone().requires_grad_(True) for t in (pooled, w1, b1, w2, b2))
    h_pre_ref = P @ W1.t()
    h_ref = F.silu(h_pre_ref + B1)
    s_pre_ref = h_ref @ W2.t()
    s_ref = torch.sigmoid(s_pre_ref + B2)
    s_ref.backward(ds)
    d = lambda t: t.cuda().to(dt)
    h_pre, h = torch.empty(B, sq, device="cuda", dtype=dt), torch.empty(B, sq, device="cuda", dtype=dt)
    s_pre, s = torch.empty(B, c, device="cuda", dtype=dt), torch.empty(B, c, device="cuda", dtype=dt)
    dc = L.dtype_code(dt)
    L.se_mlp_fwd(d(pooled), d(w1), d(b1), d(w2), d(b2), h_pre, h, s_pre, s, B, c, sq, dc)
    tol = 1e-5 if dt == torch.float32 else 2e-2
    assert rel(h_pre, h_pre_ref.detach()) < tol and rel(h, h_ref.detach()) < tol
    assert rel(s_pre, s_pre_ref.detach()) < tol and rel(s, s_ref.detach()) < tol
    ds_pre, dh_pre, dpool = torch.empty(B, c, device="cuda", dtype=dt), torch.empty(B, sq, device="cuda", dtype=dt), torch.empty(B, c, device="cuda", dtype=dt)
    gw1, gb1 = torch.full((sq, c), 0.5, device="cuda"), torch.full((sq,), 0.5, device="cuda")
    gw2, gb2 = torch.full((c, sq), 0.5, device="cuda"), torch.full((c,), 0.5, device="cuda")
    L.se_mlp_bwd(d(ds), d(pooled), h_pre, h, s_pre, d(w1), d(b1), d(w2), d(b2), ds_pre, dh_pre, dpool, gw1, gb1, gw2, gb2, B, c, sq, dc)
    torch.cuda.synchronize()
    gt = 2e-4 if dt == torch.float32 else 3e-2
    assert rel(dpool, P.grad) < gt
    assert rel(gw1 - 0.5, W1.grad) < gt and rel(gb1 - 0.5, B1.grad) < gt
    assert rel(gw2 - 0.5, W2.grad) < gt and rel(gb2 - 0.5, B2.grad) < gt


@pytest.mark.parametrize("R,C", [(20000, 72), (300, 8), (9001, 384), (64 * 57600 // 64, 1056), (50, 3840)])
def test_batchnorm_statistics_with_the_finish_inside_the_reduction_launch(R, C):
    """mmrca_bn_stats_fused (the last workgroup of a 64-channel block turns the sums into mean / rstd and updates the running statistics)
    against the two-launch form it replaces: same sums, same finish arithmetic -- mean / rstd / running statistics equal to fp32 rounding,
    with caller-zeroed buffers (the conv engine's arena) and with the fills done inside; the tickets come back equal to the number of row
    ranges.  Small and large tensors: one row range, and many."""
    g = torch.Generator().manual_seed(R + C)
    x = (torch.randn(R, C, generator=g) * 1.3 + 0.4).bfloat16().cuda()
    ref = {}
    for name in ("two launches", "fused, caller-zeroed", "fused, fills inside"):
        pz = name == "fused, caller-zeroed"
        stats = torch.zeros(2, C, device="cuda") if pz else torch.full((2, C), 5.0, device="cuda")
        rm, rv = torch.full((C,), 0.2, device="cuda"), torch.full((C,), 0.8, device="cuda")
        tickets = None
        if name != "two launches":
            tickets = torch.zeros((C + 63) // 64, dtype=torch.int32, device="cuda") if pz else torch.full(((C + 63) // 64,), 9, dtype=torch.int32, device="cuda")
        L.bn_stats(x, stats[0], stats[1], rm, rv, R, C, C, 1e-3, 0.1, True, L.BF16, prezeroed=pz, tickets=tickets)
        torch.cuda.synchronize()
        ref[name] = (stats.clone(), rm.clone(), rv.clone())
        if tickets is not None:
            assert int(tickets.min()) == int(tickets.max()) >= 1
    # every form against the fp64 column moments of x (the claim that matters): 1e-5 = ~40 fp32 ulps of the largest entry, the bound the
    # two-launch form has always been held to.  The self-comparison is NOT bit-tight: the row ranges add into the sums through fp32 atomics
    # in whatever order the workgroups retire, so two runs of the SAME kernel differ by a few ulps of a sum (worst seen on any box:
    # 2.05e-6, and that was with the two sides on different row partitions); its bound is 1e-5 as well (>= 4x the worst observed).
    xd = x.double().cpu()
    mean64, var64 = xd.mean(0), xd.var(0, unbiased=False)
    rstd64, rm64, rv64 = (var64 + 1e-3).rsqrt(), 0.9 * 0.2 + 0.1 * mean64, 0.9 * 0.8 + 0.1 * xd.var(0, unbiased=True)
    for name, (stats, rm, rv) in ref.items():
        assert rel(stats[0], mean64) < 1e-5 and rel(stats[1], rstd64) < 1e-5, name
        assert rel(rm, rm64) < 1e-5 and rel(rv, rv64) < 1e-5, name
    for name in ("fused, caller-zeroed", "fused, fills inside"):
        for a, b in zip(ref["two launches"], ref[name]):
            assert rel(b, a) < 1e-5, name


@pytest.fixture
def bn_flat_on():
    """both flat forms are opt-in (faster in isolation, no gain in the conv step): switched on for one test through the library's
    run-time switch (the environment is read once at load)"""
    L.load().mmrca_bn_flat_set(3)
    yield
    L.load().mmrca_bn_flat_set(0)


@pytest.mark.parametrize("R,C", [(20000, 72), (9001, 384), (3000, 3840), (70000, 8)])
@pytest.mark.parametrize("act", [L.CONV_NONE, L.CONV_SILU])
def test_flat_streaming_batchnorm_reductions(R, C, act, bn_flat_on):
    """mmrca_bn_stats_ws / mmrca_bn_act_bwd_ws: the flat form of the two column reductions (thread = fixed channel group, chunks t,
    t + T, ...; per-thread records in a workspace, second launch adds them) against torch.nn.functional.batch_norm and -- tightly --
    against the slice-per-workgroup kernels it replaces on large tensors (same fp32 sums in another order).  Odd row counts, the
    narrowest (8) and widest (3,840: EfficientNetV2-L's last expand) channel counts, a workspace too small for the default thread count."""
    eps, dt = 1e-3, torch.bfloat16
    g = torch.Generator().manual_seed(R + C)
    x = (torch.randn(R, C, generator=g) * 1.5 + 0.7).to(dt).float().requires_grad_(True)
    gam = (torch.rand(C, generator=g) + 0.5).to(dt).float().requires_grad_(True)
    bet = (torch.randn(C, generator=g) * 0.3).to(dt).float().requires_grad_(True)
    u = F.batch_norm(x, torch.zeros(C), torch.ones(C), gam, bet, True, 0.1, eps)
    ref = F.silu(u) if act == L.CONV_SILU else u
    dy = torch.randn(R, C, generator=g).to(dt).float()
    ref.backward(dy)
    xd, dyd, gd, bd = x.detach().cuda().to(dt), dy.cuda().to(dt), gam.detach().cuda().to(dt), bet.detach().cuda().to(dt)
    out = {}
    for name, ws in (("slices", None), ("flat", torch.empty(4 << 20, device="cuda")), ("flat, small workspace", torch.empty(72 * 1024, device="cuda")),
                     ("caller-zeroed buffers", None)):
        pz = name == "caller-zeroed buffers"           # flag bit 0 of the _ws entry points: no fill launch inside (conv_engine's per-step arena)
        stats = torch.zeros(2, C, device="cuda") if pz else torch.full((2, C), 7.0, device="cuda")
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        L.bn_stats(xd, stats[0], stats[1], rm, rv, R, C, C, eps, 0.1, True, L.BF16, ws=ws, prezeroed=pz)
        dx = torch.empty(R, C, device="cuda", dtype=dt)
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        scratch = torch.zeros(2 * C, device="cuda") if pz else torch.full((2 * C,), 7.0, device="cuda")
        L.bn_act_bwd(dyd, xd, stats[0], stats[1], gd, bd, dx, dg, db, scratch, R, C, act, True, L.BF16, ws=ws, prezeroed=pz)
        torch.cuda.synchronize()
        out[name] = (stats.clone(), rm, rv, dx, dg, db)
        mean_ref, var_ref = x.detach().mean(0), x.detach().var(0, unbiased=False)
        assert rel(stats[0], mean_ref) < 1e-5 and rel(stats[1], (var_ref + eps).rsqrt()) < 1e-5, name
        assert rel(rv, 0.9 + 0.1 * x.detach().var(0, unbiased=True)) < 1e-5, name
        assert rel(dx, x.grad) < 3e-2 and rel(dg, gam.grad) < 3e-2 and rel(db, bet.grad) < 3e-2, name
    # self-comparison of two fp32 summation orders (and of the bf16 dx computed from them): NOT bit-tight.  fp32 statistics: each side is
    # within 1e-5 of the fp64 moments (asserted above), so 1e-4 holds by a wide margin whatever order the atomics land in.  bf16 dx: sums
    # that differ in their last bits flip the rounding of a few elements by one bf16 ulp, which is up to 2^-7 = 7.8e-3 of the element;
    # the bound is two ulps of the largest entry.
    for name in ("flat", "flat, small workspace", "caller-zeroed buffers"):
        for a, b in zip(out["slices"], out[name]):
            assert rel(a, b) < (1e-4 if a.dtype == torch.float32 else 1.6e-2), name


@pytest.mark.parametrize("M,N,K", [(1000, 72, 64), (300, 256, 224), (4096, 768, 192), (777, 200, 96), (128, 128, 64)])
def test_gemm_with_batchnorm_moments_in_the_epilogue(M, N, K):
    """mmrca_gemm_bnstats + mmrca_bn_finish_sums == mmrca_gemm + mmrca_bn_stats (the 1x1 convolutions of the conv backbones): same z bit
    for bit, mean / rstd / running statistics to fp32 rounding; both 128x128 kernels (K % 64 == 0 and the 32-deep one), ragged M and N,
    a shift far from the channel means included."""
    g = torch.Generator().manual_seed(M + N)
    A = torch.randn(M, K, generator=g).bfloat16().cuda()
    Bw = (torch.randn(N, K, generator=g) * 0.2 + 0.05).bfloat16().cuda()
    z_ref = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    L.gemm(A, Bw, z_ref, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, dtype=L.BF16)
    mean_r, rstd_r = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    rm_r, rv_r = torch.full((N,), 0.3, device="cuda"), torch.ones(N, device="cuda")
    L.bn_stats(z_ref, mean_r, rstd_r, rm_r, rv_r, M, N, N, 1e-3, 0.1, True, L.BF16)
    for shift_kind in ("running", "none", "far"):
        z = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
        ns = (M + 127) // 128
        s1, s2 = torch.full((ns, N), float("nan"), device="cuda"), torch.full((ns, N), float("nan"), device="cuda")
        rm, rv = torch.full((N,), 0.3, device="cuda"), torch.ones(N, device="cuda")
        shift = {"running": rm, "none": None, "far": torch.full((N,), 25.0, device="cuda")}[shift_kind]
        L.gemm_bnstats(A, Bw, z, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, dtype=L.BF16, shift=shift, s1=s1, s2=s2)
        assert torch.equal(z, z_ref)
        mean, rstd = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
        L.bn_finish_sums(s1, s2, shift, ns, M, mean, rstd, rm, rv, N, 1e-3, 0.1)
        # two different fp32 summation orders (128-row slabs added in a fixed order vs row ranges through atomics) of near-zero-mean
        # columns, relative to the largest channel mean: 1e-4, several times the 2e-5 these were first sized at (not a bit-tight claim)
        tol = 1e-4 if shift_kind != "far" else 4e-3           # (a shift 25 sigma off costs digits, as it must; the engine passes the running mean)
        assert rel(mean, mean_r) < tol and rel(rstd, rstd_r) < tol, shift_kind
        assert rel(rm, rm_r) < tol and rel(rv, rv_r) < tol


@pytest.mark.parametrize("HW", [35, 64, 100])        # odd / even row counts of the two-rows-in-flight loop
@pytest.mark.parametrize("act", [L.CONV_SILU, L.CONV_NONE])
def test_se_backward_second_half_with_the_batchnorm_sums_in_one_pass(HW, act):
    """mmrca_se_dx: dx = dy * s + dpool / HW, and -- for the BatchNorm + activation whose output gradient dx is -- the sums that
    mmrca_bn_act_bwd's first pass would compute from dx and z; mmrca_bn_act_bwd_sums then gives the same dz / dgamma / dbeta."""
    B, C = 3, 72
    g = torch.Generator().manual_seed(HW)
    dy = torch.randn(B * HW, C, generator=g).bfloat16().cuda()
    s = torch.rand(B, C, generator=g).bfloat16().cuda()
    dpool = torch.randn(B, C, generator=g).bfloat16().cuda()
    z = (torch.randn(B * HW, C, generator=g) * 1.5 + 0.3).bfloat16().cuda()
    gam, bet = (1 + 0.2 * torch.randn(C, generator=g)).bfloat16().cuda(), (0.1 * torch.randn(C, generator=g)).bfloat16().cuda()
    mean, rstd = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    L.bn_stats(z, mean, rstd, None, None, B * HW, C, C, 1e-3, 0.0, True, L.BF16)
    # two-kernel reference path
    dx_ref, ds = torch.empty(B * HW, C, device="cuda", dtype=torch.bfloat16), torch.empty(B, C, device="cuda", dtype=torch.bfloat16)
    L.se_scale_bwd(dy, z, s, dx_ref, ds, B, HW, C, L.BF16)                 # (x only feeds ds here)
    L.rowpool_mean_bwd(dpool, dx_ref, B, HW, C, True, L.BF16)
    ds2 = torch.empty_like(ds)
    L.se_scale_bwd(dy, z, s, None, ds2, B, HW, C, L.BF16)                   # ds only
    assert torch.equal(ds, ds2)
    dx = torch.full_like(dx_ref, float("nan"))
    sums = torch.zeros(2 * C, device="cuda")
    L.se_dx(dy, s, dpool, dx, B, HW, C, L.BF16, bn=(z, mean, rstd, gam, bet, act, sums))
    exact = dy.float().view(B, HW, C) * s.float()[:, None] + dpool.float()[:, None] / HW
    assert rel(dx.view(B, HW, C), exact) < 6e-3 and rel(dx, dx_ref) < 1.2e-2          # (the one-pass form rounds once, the old one twice)
    dx2 = torch.empty_like(dx)
    L.se_dx(dy, s, dpool, dx2, B, HW, C, L.BF16)
    assert torch.equal(dx, dx2)
    # BatchNorm backward from the accumulated sums == the two-pass backward on the same dx
    dz_a, dz_b = torch.empty_like(dx), torch.empty_like(dx)
    dg_a, db_a, dg_b, db_b = (torch.zeros(C, device="cuda") for _ in range(4))
    scratch = torch.empty(2 * C, device="cuda")
    L.bn_act_bwd(dx, z, mean, rstd, gam, bet, dz_a, dg_a, db_a, scratch, B * HW, C, act, True, L.BF16)
    assert rel(sums, scratch) < 5e-5                  # two fp32 atomic orders of the same addends (not bit-tight by construction)
    L.bn_act_bwd(dx, z, mean, rstd, gam, bet, dz_b, dg_b, db_b, sums, B * HW, C, act, True, L.BF16, sums_ready=True)
    assert rel(dz_b, dz_a) < 1.6e-2 and rel(dg_b, dg_a) < 5e-5 and rel(db_b, db_a) < 5e-5     # (bf16 dz: two ulps of the largest entry)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [70, 72])      # 72: the 8-channel kernels
def test_pool_se_residual_maxpool_gather(dt, C):
    B, HW = 3, 35
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, HW, C, generator=g).to(dt).float()
    s = torch.rand(B, C, generator=g).to(dt).float()
    xd, sd = x.view(-1, C).cuda().to(dt), s.cuda().to(dt)
    code = L.dtype_code(dt)
    out = torch.empty(B, C, device="cuda", dtype=dt)
    L.rowpool_mean(xd, out, B, HW, C, code)
    assert rel(out, x.mean(1)) < TOL[dt]
    y = torch.empty(B * HW, C, device="cuda", dtype=dt)
    L.se_scale_fwd(xd, sd, y, B, HW, C, code)
    assert rel(y.view(B, HW, C), x * s[:, None]) < TOL[dt]
    dy = torch.randn(B, HW, C, generator=g).to(dt).float()
    dx, ds = torch.empty(B * HW, C, device="cuda", dtype=dt), torch.empty(B, C, device="cuda", dtype=dt)
    L.se_scale_bwd(dy.view(-1, C).cuda().to(dt), xd, sd, dx, ds, B, HW, C, code)
    assert rel(dx.view(B, HW, C), dy * s[:, None]) < TOL[dt] and rel(ds, (dy * x).sum(1)) < TOL[dt]
    dp = torch.randn(B, C, generator=g).to(dt).float()
    acc = dx.clone()
    L.rowpool_mean_bwd(dp.cuda().to(dt), acc, B, HW, C, True, code)
    assert rel(acc.view(B, HW, C), dx.float().cpu().view(B, HW, C) + dp[:, None] / HW) < TOL[dt]
    rs = torch.tensor([0.0, 1.25, 1.25], device="cuda")
    o = torch.empty(B * HW, C, device="cuda", dtype=dt)
    L.residual_add(xd, y, rs, o, B, HW * C, code)
    assert rel(o.view(B, HW, C), x + (x * s[:, None]).to(dt).float() * rs.cpu()[:, None, None]) < TOL[dt]
    # biased activation of the squeeze-excitation 1x1 convolutions
    bias = torch.randn(C, generator=g).to(dt).float()
    pre = x[:, 0].clone().requires_grad_(True)
    ref = torch.sigmoid(pre + bias)
    yb = torch.empty(B, C, device="cuda", dtype=dt)
    L.bias_act_fwd(pre.detach().cuda().to(dt), bias.cuda().to(dt), yb, B, C, L.CONV_SIGMOID, code)
    assert rel(yb, ref.detach()) < TOL[dt]
    go = torch.randn(B, C, generator=g).to(dt).float()
    ref.backward(go)
    dpre, dbias = torch.empty(B, C, device="cuda", dtype=dt), torch.zeros(C, device="cuda")
    L.bias_act_bwd(go.cuda().to(dt), pre.detach().cuda().to(dt), bias.cuda().to(dt), dpre, dbias, B, C, L.CONV_SIGMOID, code)
    assert rel(dpre, pre.grad) < TOL[dt] and rel(dbias, pre.grad.sum(0)) < 2e-2
    # max pooling 3x3 / 2 / 1
    H, W = 9, 6
    xi = torch.randn(B, C, H, W, generator=g).to(dt).float().requires_grad_(True)
    ref = F.max_pool2d(xi, 3, 2, 1)
    Ho, Wo = ref.shape[2:]
    yo = torch.empty(B * Ho * Wo, C, device="cuda", dtype=dt)
    arg = torch.empty(B * Ho * Wo, C, device="cuda", dtype=torch.uint8)
    L.maxpool3x3s2_fwd(rows(xi.detach()).cuda().to(dt), yo, arg, B, H, W, C, code)
    assert rel(nchw(yo.float().cpu(), B, Ho, Wo), ref.detach()) < 1e-6
    gy = torch.randn(ref.shape, generator=g).to(dt).float()
    ref.backward(gy)
    dxi = torch.empty(B * H * W, C, device="cuda", dtype=dt)
    L.maxpool3x3s2_bwd(rows(gy).cuda().to(dt), arg, dxi, B, H, W, C, code)
    assert rel(nchw(dxi.float().cpu(), B, H, W), xi.grad) < TOL[dt]
    # channel gather
    cmap = torch.randperm(C, generator=g)[:40].int().cuda()
    og = torch.zeros(B * HW, 64, device="cuda", dtype=dt)
    L.channel_gather(xd, cmap, og, B * HW, C, 40, 64, 8, code)
    assert torch.equal(og[:, 8:48].float().cpu(), x.view(-1, C)[:, cmap.cpu().long()].to(dt).float())


class _Owner:
    """Minimal parameter owner for a bare ConvEncoder (what MMRCAEngine provides): fp32 tensors per key."""

    def __init__(self, dtype):
        self.dtype, self.device, self.dt, self.gemm_impl = dtype, torch.device("cuda"), L.dtype_code(dtype), L.IMPL_AUTO
        self.p, self.g, self.lp = {}, {}, {}

    def W(self, k):
        return self.lp[k] if self.dtype == torch.bfloat16 else self.p[k]

    def G(self, k):
        return self.g[k]


def _conv_pair(name, dtype, seed=0):
    """Product ConvEncoder and oracle with the same (seeded, non-trivial) parameters and running statistics."""
    torch.manual_seed(seed)
    orc = CM.build_conv_oracle(name)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, t in orc.state_dict().items():
            if k.endswith("running_mean"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
            elif k.endswith("running_var"):
                t.copy_(torch.rand(t.shape, generator=g) * 0.5 + 0.75)
            elif k.endswith(".1.weight") or (t.dim() == 1 and k.endswith("weight")):
                t.copy_(torch.rand(t.shape, generator=g) * 0.5 + 0.75)
            elif t.dim() == 1 and k.endswith("bias"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
    own = _Owner(dtype)
    enc = ConvEncoder(name, own)
    sd = orc.state_dict()
    for k, shp in enc.param_entries():
        assert tuple(sd[k].shape) == tuple(shp), k
        own.p["image_model." + k] = sd[k].detach().clone().float().cuda().contiguous()
        own.g["image_model." + k] = torch.zeros_like(own.p["image_model." + k])
        own.lp["image_model." + k] = own.p["image_model." + k].bfloat16()
    enc.init_buffers(own.device)
    enc.load_buffers(sd)
    return enc, own, orc


def _sd_blocks(orc):
    return [m for m in orc.modules() if isinstance(m, CM.MBConv) and m.use_res_connect and m.stochastic_depth.p > 0]


@pytest.mark.parametrize("name,B,size", [("eff_v2_medium", 3, 64), ("shuffle_net", 4, 64), ("eff_v2_large", 3, 64)])
@pytest.mark.parametrize("train", [True, False])
def test_backbone_features_gradients_and_running_stats_match_oracle_fp32(name, B, size, train):
    enc, own, orc = _conv_pair(name, torch.float32)
    g = torch.Generator().manual_seed(9)
    images = torch.randn(B, 3, size, size, generator=g)
    orc.train(train)
    blocks = _sd_blocks(orc)
    if train and blocks:                      # drive both sides with the same stochastic-depth keep masks
        keep = (torch.rand(len(blocks), B, generator=g) > 0.3).float()
        for m, k in zip(blocks, keep):
            m.stochastic_depth.keep = k
        enc.injected_keep = keep
    for p in orc.parameters():
        p.requires_grad_(True)
    feat_ref = CM.conv_features(orc, images)
    feat = enc.forward(images.cuda(), save=True, train=train)
    assert rel(feat, feat_ref.detach()) < 1e-3, rel(feat, feat_ref.detach())
    dfeat = torch.randn(feat_ref.shape, generator=g)
    feat_ref.backward(dfeat)
    enc.backward(dfeat.cuda())
    torch.cuda.synchronize()
    named = dict(orc.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in named.values() if p.grad is not None)
    worst = 0.0
    for k, _ in enc.param_entries():
        got, ref = own.g["image_model." + k].cpu(), named[k].grad
        if name == "shuffle_net":
            # ShuffleNetV2 gates with ReLU behind BatchNorm over 64..1024 rows: the forwards agree to 2e-5, so about one
            # pre-activation per layer (|u| < 1e-5 of ~1e5 values) takes the other side of the gate, and that single flip
            # moves its channel's BatchNorm-backward sums -- entries of a few tensors differ by per cent, differently in every
            # run (atomic summation order decides the flips).  The oracle in fp64 vs fp32 (no flips at 1e-7) agrees to 7e-5,
            # every kernel is checked exactly against torch above, and EfficientNetV2 (smooth SiLU) matches to 1e-4; here the
            # whole-network check is therefore in the flip-tolerant L2 / cosine sense.
            num, den = (got - ref.view_as(got)).double().norm().item(), ref.double().norm().item()
            cos = torch.nn.functional.cosine_similarity(got.double().flatten(), ref.double().flatten(), dim=0).item() if den > 0 else 1.0
            worst = max(worst, num / max(den, 1e-30))
            assert num <= 5e-2 * max(den, 1e-3 * gmax) and (cos > 0.998 or den < 1e-3 * gmax), (k, num / den, cos)   # (a BatchNorm bias in front of conv + BatchNorm has a ~0 gradient)
            continue
        err = (got - ref.view_as(got)).abs().max().item()
        scale = max(ref.abs().max().item(), 1e-3 * gmax)
        worst = max(worst, err / scale)
        assert err <= 1e-3 * scale, (k, err, scale)        # measured 9e-5
    print(f"{name} train={train}: features rel {rel(feat, feat_ref.detach()):.2e}, worst gradient rel {worst:.2e}")
    if train:
        enc.sync_buffers()
        sd = orc.state_dict()
        for k, t in enc.buffers.items():
            assert rel(t, sd[k]) < 1e-4, k
    enc.release()


def test_backbone_bf16_close_to_oracle():
    enc, own, orc = _conv_pair("eff_v2_medium", torch.bfloat16)
    images = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    orc.eval()
    with torch.no_grad():
        ref = CM.conv_features(orc, images)
    feat = enc.forward(images.cuda(), save=False, train=False)
    e = rel(feat, ref)
    print("EfficientNetV2-M bf16 features relative error:", e)
    assert torch.isfinite(feat.float()).all() and e < 6e-2
    enc.release()


def test_one_pass_batchnorm_statistics_survive_outlier_rows():
    """The bf16 one-pass BatchNorm moments subtract a shift before squaring.  With a single row as the shift (round 2: row 0 --
    the top-left pixel of image 0, a zero-padded border) a channel whose first row sits hundreds of sigma from its mean cancels
    in fp32 over many rows; the shift is now a trimmed mean of 16 hashed rows.  Channel mean 50, sigma 0.25, every image's
    corner pixel (rows 0, HW, 2 HW, ...: what evenly spaced samples would hit) zero."""
    B, HW, C, eps = 64, 6400, 64, 1e-5
    R = B * HW
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(R, C, generator=g) * 0.25 + 50.0)
    x[::HW] = 0.0
    xd = x.cuda().to(torch.bfloat16)
    mean, rstd = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    L.bn_stats(xd, mean, rstd, rm, rv, R, C, C, eps, 0.1, True, L.BF16)
    x64 = xd.double()
    mu, var = x64.mean(0), x64.var(0, unbiased=False)
    assert rel(mean, mu) < 1e-5          # fp32 sums over 409,600 rows
    got_var = 1.0 / rstd.double() ** 2 - eps
    e = float(((got_var - var).abs() / var).max())
    print("one-pass BatchNorm variance, relative error with outlier corner rows:", e)
    assert e < 2e-3, e


@pytest.mark.parametrize("text_model,image_model,size", [("distilbert", "eff_v2_medium", 64), ("distilbert", "shuffle_net", 64),
                                                         ("roberta", "eff_v2_large", 64)])
def test_mm_rca_with_conv_backbone_fp32_logits_and_train_step(text_model, image_model, size):
    """MM_RCA over a conv image backbone end to end: fp32 logits within the north-star 1e-3 of the oracle (eval mode), and a
    train-mode forward/backward that reaches every trainable parameter.  ("roberta", "eff_v2_large") is BASELINE.json
    configs[2]'s pairing (multimodal_model.py:113-126 with the RoBERTa CLS-pooling convention of text_models.py:43-72) as ONE
    model; for it a bf16 train step (the benchmarked precision of configs[2]) runs as well."""
    eng = MMRCAEngine(text_model, image_model, 4, True, 0, torch.float32, image_size=size)
    eng.init_parameters(0)
    orc = O.build_oracle(text_model, image_model, True, False, False, drop_ratio=0.0, enc_dropout=0.0).eval()
    sd = {k: eng.arena.view(k).detach().cpu().clone() for k in eng.param_keys}
    orc.text_model.load_flat(sd, "text_model.")
    isd = {k[len("image_model."):]: v for k, v in sd.items() if k.startswith("image_model.")}
    missing = orc.image_model.load_state_dict(isd, strict=False)
    assert not missing.unexpected_keys and all(("running" in k or "num_batches" in k) for k in missing.missing_keys)
    orc.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("text_model.", "image_model."))}, strict=False)
    from garbage_classification_rca_amd.procedural import synth_captions
    B = 3
    ids, mask = (torch.from_numpy(a) for a in synth_captions(B, 24, seed=1))
    if text_model == "roberta":
        ids = ids.clone(); ids[mask == 0] = 1          # RoBERTa pads with id 1
    images = torch.randn(B, 3, size, size, generator=torch.Generator().manual_seed(3))
    logits = eng.forward(ids.cuda(), mask.cuda(), images.cuda(), save=False, bn_train=False)
    with torch.no_grad():
        ref = orc(ids, mask, images, eval=True)
    assert rel(logits, ref) < 1e-3, rel(logits, ref)
    logits = eng.forward(ids.cuda(), mask.cuda(), images.cuda(), drop_p=0.0, seed=5, save=True, bn_train=True)
    eng.arena.g.zero_()
    eng.backward(torch.randn(B, 4, device="cuda") * 0.1)
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all() and torch.isfinite(eng.arena.g).all()
    lo, hi = eng.groups["image_emb"]
    assert float(eng.arena.g[lo:hi].abs().max()) > 0
    eng.release_buffers()
    if text_model == "roberta":
        e16 = MMRCAEngine(text_model, image_model, 4, True, 0, torch.bfloat16, image_size=size)
        e16.load_arrays(sd)
        l16 = e16.forward(ids.cuda(), mask.cuda(), images.cuda(), save=False, bn_train=False)
        assert rel(l16, ref) < 3e-2, rel(l16, ref)         # bf16 bound of this suite
        l16 = e16.forward(ids.cuda(), mask.cuda(), images.cuda(), drop_p=0.6, seed=5, save=True, enc_drop_p=0.1, bn_train=True)
        e16.arena.g.zero_()
        e16.backward(torch.randn(B, 4, device="cuda") * 0.1)
        torch.cuda.synchronize()
        assert torch.isfinite(l16).all() and torch.isfinite(e16.arena.g).all()
        for grp in ("image_emb", "text_emb", "head"):
            lo, hi = e16.groups[grp]
            assert float(e16.arena.g[lo:hi].abs().max()) > 0, grp
        e16.release_buffers()


def test_facade_state_dict_of_the_default_image_model_has_the_reference_layout_and_loads_it():
    """SURVEY.md section 8 row a4 for the reference's default image model (EfficientNetV2-M, multimodal_model.py:113-126,
    wrapped by EfficientNetV2MFullFeatureExtractor :11-36): ``MM_RCA(...).state_dict()`` carries exactly the image_model.* keys
    (parameters AND BatchNorm buffers, incl. num_batches_tracked) and shapes that the reference module tree produces, and a
    checkpoint shaped like the reference's loads and reproduces the oracle's logits."""
    from garbage_classification_rca_amd.multimodal_model import MM_RCA
    from garbage_classification_rca_amd.procedural import synth_captions
    size, B = 64, 2
    m = MM_RCA(4, 0.0, 0.0, 0.0, 256, "distilbert", B, True, False, False, image_model_name="eff_v2_medium", dtype=torch.float32,
               device=torch.device("cuda:0"), image_size=size)
    orc = O.build_oracle("distilbert", "eff_v2_medium", True, False, False, drop_ratio=0.0, enc_dropout=0.0).eval()
    ref_img = {("image_model." + k): tuple(v.shape) for k, v in orc.image_model.state_dict().items()}
    own = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("image_model.")}
    assert own == ref_img, (sorted(set(own) ^ set(ref_img))[:10])
    assert sum(k.endswith("num_batches_tracked") for k in own) == sum(k.endswith("running_mean") for k in own) > 100
    # a reference-shaped checkpoint: the oracle's image tree with non-trivial BatchNorm statistics
    g = torch.Generator().manual_seed(4)
    ck = dict(m.state_dict())
    for k, v in orc.image_model.state_dict().items():
        if k.endswith("running_var"):
            v = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith("running_mean"):
            v = 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith("num_batches_tracked"):
            v = torch.tensor(7)
        ck["image_model." + k] = v.clone()
    orc.image_model.load_state_dict({k[len("image_model."):]: v for k, v in ck.items() if k.startswith("image_model.")})
    res = m.load_state_dict(ck)
    assert not res.missing_keys and not res.unexpected_keys
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert int(sd["image_model.stem.0.1.num_batches_tracked"]) == 7
    orc.text_model.load_flat(sd, "text_model.")
    orc.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("text_model.", "image_model."))}, strict=False)
    ids, mask = (torch.from_numpy(a) for a in synth_captions(B, 24, seed=2))
    images = torch.randn(B, 3, size, size, generator=g)
    m.eval()
    with torch.no_grad():
        out = m(_input_ids=ids.cuda(), _attention_mask=mask.cuda(), _images=images.cuda(), eval=True)
        ref = orc(ids, mask, images, eval=True)
    assert rel(out, ref) < 1e-3, rel(out, ref)
    m.engine.release_buffers()


def test_the_references_own_ten_argument_call_builds_the_references_model_within_tolerance():
    """the reference constructs its model with ten positionals and nothing else (main_both.py:306-317).
    That exact call must land on the reference's model -- EfficientNetV2-M at 480 x 480 (multimodal_model.py:113-126, 188,
    257-258, 407-408; main_both.py:259) + DistilBERT -- carry the ``image_model.*`` key set of the reference's
    ``EfficientNetV2MFullFeatureExtractor`` (:11-36), and compute logits within north_star's 1e-3 of the fp32 oracle in its
    DEFAULT compute mode."""
    from garbage_classification_rca_amd.multimodal_model import MM_RCA
    from garbage_classification_rca_amd.procedural import synth_captions
    m = MM_RCA(4, .6, 0., .7, 256, "distilbert", 16, True, False, False)
    assert m.get_image_size() == (480, 480)
    assert m.get_max_token_size() == 512
    assert m.image_model_name == "eff_v2_medium" and m.engine.x3f and m.engine.d_img == 1280 and m.engine.d_txt == 768
    assert (m.img_patch_size, m.txt_patch_size) == (80, 48)                       # multimodal_model.py:257-261
    orc = O.build_oracle("distilbert", "eff_v2_medium", True, False, False, drop_ratio=0.6, enc_dropout=0.1).eval()
    ref_img = {("image_model." + k): tuple(v.shape) for k, v in orc.image_model.state_dict().items()}
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    own = {k: tuple(v.shape) for k, v in sd.items() if k.startswith("image_model.")}
    assert own == ref_img, (sorted(set(own) ^ set(ref_img))[:10])
    # frozen at construction, like the reference's backbones (:117-118, 132-133)
    assert not any(p.requires_grad for p in m.text_model.parameters()) and not any(p.requires_grad for p in m.image_model.parameters())
    orc.text_model.load_flat(sd, "text_model.")
    orc.image_model.load_state_dict({k[len("image_model."):]: v for k, v in sd.items() if k.startswith("image_model.")})
    orc.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("text_model.", "image_model."))}, strict=False)
    B = 4
    ids, mask = (torch.from_numpy(a) for a in synth_captions(B, 64, seed=11))
    images = torch.randn(B, 3, 480, 480, generator=torch.Generator().manual_seed(12))
    m.eval()
    with torch.no_grad():
        out = m(ids.cuda(), mask.cuda(), images.cuda(), eval=True)
        ref = orc(ids, mask, images, eval=True)
    e = rel(out, ref)
    print("ten-argument MM_RCA call, default mode: logits vs fp32 oracle", e)
    assert out.shape == (B, 4) and e < 1e-3, e
    # and the reference's training call on it (main_both.py:106-112): the head trains, the frozen backbones get no gradient
    m.train()
    loss = torch.nn.CrossEntropyLoss()(m(ids.cuda(), mask.cuda(), images.cuda()), torch.tensor([0, 1, 2, 3]).cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and float(m.final_with_everything.weight.grad.abs().max()) > 0
    m.engine.release_buffers()


@pytest.mark.parametrize("stride", [1, 2])
def test_tap_major_patch_kernels_are_the_channel_major_ones_permuted(stride):
    """mmrca_im2row3x3_tap / col2im3x3_tap (k = tap*C + c) against the channel-major pair (k = c*9 + tap): same patches, same
    folded gradient"""
    B, C, H, W = 2, 24, 9, 7
    g = torch.Generator().manual_seed(3)
    xr = torch.randn(B * H * W, C, generator=g).bfloat16().cuda()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    K, n = 9 * C, B * Ho * Wo
    col_c, col_t = torch.empty(n, K, device="cuda", dtype=torch.bfloat16), torch.empty(n, K, device="cuda", dtype=torch.bfloat16)
    L.im2row3x3(xr, col_c, B, H, W, C, stride, K, L.BF16)
    L.im2row3x3_tap(xr, col_t, B, H, W, C, stride, K, L.BF16)
    assert torch.equal(col_t.view(n, 9, C), col_c.view(n, C, 9).transpose(1, 2))
    dcol_t = torch.randn(n, K, generator=g).bfloat16().cuda()
    dcol_c = dcol_t.view(n, 9, C).transpose(1, 2).contiguous().view(n, K)
    dx_c, dx_t = torch.empty(B * H * W, C, device="cuda", dtype=torch.bfloat16), torch.empty(B * H * W, C, device="cuda", dtype=torch.bfloat16)
    L.col2im3x3(dcol_c, dx_c, B, H, W, C, stride, K, L.BF16)
    L.col2im3x3_tap(dcol_t, dx_t, B, H, W, C, stride, K, L.BF16)
    assert torch.equal(dx_c, dx_t)
    with pytest.raises(L.MmrcaError):          # the 3-channel stem cannot use it
        L.im2row3x3_tap(xr, col_t, B, H, W, 3, stride, 27, L.BF16)


def test_backbone_bf16_tap_major_equals_channel_major_forward_and_backward():
    """EfficientNetV2-M in bf16: features and every parameter gradient with the dense 3x3 convolutions on tap-major patches
    (default) against the channel-major path (conv_engine.TAP_MAJOR = False).  BatchNorm on running statistics: with batch statistics
    over the 12..48 rows this small input leaves in the late stages, bf16 rounding differences between two summation orders are
    amplified to tens of per cent by the normalisation itself (either order is equally far from the fp32 oracle)."""
    from garbage_classification_rca_amd import conv_engine as CE
    images = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    out = {}
    for tap in (True, False):
        CE.TAP_MAJOR = tap
        try:
            enc, own, _ = _conv_pair("eff_v2_medium", torch.bfloat16, seed=4)
            feat = enc.forward(images, save=True, train=False, seed=9)
            dfeat = (torch.randn(feat.shape, generator=torch.Generator().manual_seed(6)) * 0.1).to(feat.dtype).cuda()
            enc.backward(dfeat)
            torch.cuda.synchronize()
            out[tap] = (feat.float().cpu(), {k: v.float().cpu().clone() for k, v in own.g.items()})
            enc.release()
        finally:
            CE.TAP_MAJOR = True
    print("tap-major vs channel-major features:", rel(out[True][0], out[False][0]))
    assert rel(out[True][0], out[False][0]) < 2e-2
    errs = {k: rel(out[True][1][k], out[False][1][k]) for k in out[True][1] if out[False][1][k].abs().max() > 0}
    worst = max(errs, key=errs.get)
    # the 3x3 weight gradients themselves (the tensors the permuted accumulation writes)
    k3 = [k for k, v in out[True][1].items() if v.dim() == 4 and v.shape[-1] == 3 and v.shape[1] % 8 == 0 and v.shape[1] > 1]
    print("worst gradient:", worst, errs[worst], "; worst 3x3 weight gradient:", max(errs[k] for k in k3))
    # two bf16 runs of a 57-layer backward that differ in the summation order of 19 GEMMs: per-cent level on the worst tensor
    assert errs[worst] < 1e-1, (worst, errs[worst])
    assert k3 and all(errs[k] < 6e-2 for k in k3)
    cos = min(torch.nn.functional.cosine_similarity(out[True][1][k].double().flatten(), out[False][1][k].double().flatten(), dim=0).item() for k in k3)
    print("smallest cosine between the two 3x3 weight gradients:", cos)
    assert cos > 0.998          # (0.9990-0.9997 on im2row + GEMM for both; 0.9990 since the default path is the implicit GEMM, whose
                                # input gradient is a different kernel with a different rounding point)


@pytest.mark.parametrize("maxrows", [1 << 40, 200])
def test_weight_gradients_on_the_side_stream_equal_the_one_stream_backward(maxrows):
    """conv_engine.SIDE_WGRAD: the 1x1 / implicit-GEMM 3x3 weight gradients launched on a second stream beside the input-gradient chain
    (ConvEncoder._wgrad_stream) -- the same kernels on the same operands, so features are bit-identical and every parameter gradient
    differs from the one-stream backward only by the order in which fp32 atomics land (bound: 1e-4 of the tensor's largest entry; the
    one-stream backward run twice differs by up to ~2e-6).  Three backwards in a row over the same buffers: the second and third find
    the dz buffers of the first still registered with their side-stream readers.  maxrows = 200: only the late stages (at this image
    size) use the stream, the rest stays on the main one."""
    from garbage_classification_rca_amd import conv_engine as CE
    images = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    out = {}
    for side in (False, True):
        CE.SIDE_WGRAD, CE.SIDE_MAXROWS = side, maxrows
        try:
            enc, own, _ = _conv_pair("eff_v2_medium", torch.bfloat16, seed=4)
            grads = []
            for rep in range(3):
                for v in own.g.values():
                    v.zero_()
                feat = enc.forward(images, save=True, train=False, seed=9)
                dfeat = (torch.randn(feat.shape, generator=torch.Generator().manual_seed(6)) * 0.1).to(feat.dtype).cuda()
                enc.backward(dfeat)
                torch.cuda.synchronize()
                grads.append({k: v.float().cpu().clone() for k, v in own.g.items()})
            assert (enc._side is not None) == side and not enc._side_busy
            # workspaces are exact-size (a 64 MiB workspace asked for through buf() is 256 padded rows = 16 GiB, and inside a graph
            # capture a 16 GiB fill in every replay: 2.6 ms per step, found in the configs[0] line)
            assert max(t.numel() * t.element_size() for t in enc._bufs.values()) <= 64 << 20 and sum(t.numel() * t.element_size() for t in enc._bufs.values()) < 1 << 30
            out[side] = (feat.float().cpu(), grads)
            enc.release()
        finally:
            CE.SIDE_WGRAD, CE.SIDE_MAXROWS = "auto", 1 << 40
    assert torch.equal(out[True][0], out[False][0])
    worst = 0.0
    for rep in range(3):
        for k, ref in out[False][1][0].items():
            if ref.abs().max() > 0:
                worst = max(worst, rel(out[True][1][rep][k], ref))
    print("side-stream vs one-stream weight gradients, worst tensor:", worst)
    assert worst < 1e-4, worst


@pytest.mark.parametrize("R,C", [(9001, 384), (300, 8), (20000, 72), (3600, 1824), (50, 3840)])
@pytest.mark.parametrize("with_res", [False, True])
def test_batchnorm_forward_with_the_finish_inside_the_apply_pass(R, C, with_res):
    """mmrca_bn_moments + mmrca_bn_act_fwd_fin (two launches: the apply pass turns the sums into mean / rstd itself) against torch's
    train-mode batch_norm in fp64 and against the three-launch form (mmrca_bn_stats + mmrca_bn_act_fwd / _res).  The two forms run the
    same arithmetic on sums whose fp32 atomics land in another order: mean / rstd / running statistics within 2e-6 (8x the largest
    difference seen between two runs of ONE form), outputs within one bf16 rounding of each other."""
    eps, act = 1e-3, L.CONV_SILU
    g = torch.Generator().manual_seed(R + C)
    x = (torch.randn(R, C, generator=g) * 2 + torch.randn(C, generator=g) * 3).bfloat16()
    gam, bet = (torch.rand(C, generator=g) + 0.5).bfloat16(), (torch.randn(C, generator=g) * 0.3).bfloat16()
    res = torch.randn(R, C, generator=g).bfloat16() if with_res else None
    rps = 25 if R % 25 == 0 else R
    rowscale = (torch.rand(R // rps, generator=g) > 0.3).float().cuda() / 0.7 if with_res else None
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    u = F.batch_norm(x.double(), rm0.double().clone(), rv0.double().clone(), gam.double(), bet.double(), True, 0.1, eps)
    ref = F.silu(u)
    if with_res:
        ref = res.double() + rowscale.cpu().double().repeat_interleave(rps)[:, None] * ref
    xd, gd, bd = x.cuda(), gam.cuda(), bet.cuda()
    resd = res.cuda() if with_res else None
    # three launches
    mean_a, rstd_a = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    rm_a, rv_a = rm0.clone().cuda(), rv0.clone().cuda()
    L.bn_stats(xd, mean_a, rstd_a, rm_a, rv_a, R, C, C, eps, 0.1, True, L.BF16)
    y_a = torch.empty(R, C, device="cuda", dtype=torch.bfloat16)
    if with_res:
        L.bn_act_fwd_res(xd, mean_a, rstd_a, gd, bd, resd, rowscale, y_a, R, C, act, rps, L.BF16)
    else:
        L.bn_act_fwd(xd, mean_a, rstd_a, gd, bd, y_a, R, C, act, L.BF16)
    # two launches
    assert L.bn_fold_ok(C, C, L.BF16)
    sums = torch.zeros(3, C, device="cuda")
    mean_b, rstd_b = torch.full((C,), 7.0, device="cuda"), torch.full((C,), 7.0, device="cuda")
    rm_b, rv_b = rm0.clone().cuda(), rv0.clone().cuda()
    y_b = torch.empty(R, C, device="cuda", dtype=torch.bfloat16)
    L.bn_moments(xd, sums[0], sums[1], sums[2], R, C, C, L.BF16)
    L.bn_act_fwd_fin(xd, sums[0], sums[1], sums[2], gd, bd, resd, rowscale, y_b, mean_b, rstd_b, rm_b, rv_b, R, C, act, rps, eps, 0.1, L.BF16)
    torch.cuda.synchronize()
    assert rel(y_b, ref) < TOL[torch.bfloat16], rel(y_b, ref)
    for a, b in ((mean_a, mean_b), (rstd_a, rstd_b), (rm_a, rm_b), (rv_a, rv_b)):
        assert rel(b, a) < 2e-6, rel(b, a)
    # outputs: equal up to the bf16 rounding of a value that moved by ~1e-7
    d = (y_a.float() - y_b.float()).abs()
    assert float((d > 0).float().mean()) < 2e-2 and float((d / y_a.float().abs().clamp_min(1e-3)).max()) < 2 ** -6


def test_backbone_with_the_folded_batchnorm_forward_matches_the_three_launch_form():
    """EfficientNetV2-M, bf16, TRAIN-mode BatchNorm at 96 x 96 (B = 6: the late stages normalise over 54 rows): features, running
    statistics and every parameter gradient with conv_engine.BN_FOLD on against off.  Two runs of EITHER form already differ (the sums'
    fp32 atomics land in another order, a bf16 activation flips by one rounding, train-mode BatchNorm over few rows amplifies it), so the
    bound is the distance between two runs of the three-launch form, times three."""
    from garbage_classification_rca_amd import conv_engine as CE
    images = torch.randn(6, 3, 96, 96, generator=torch.Generator().manual_seed(5)).cuda()

    def run(fold):
        CE.BN_FOLD = fold
        try:
            enc, own, _ = _conv_pair("eff_v2_medium", torch.bfloat16, seed=4)
            enc.injected_keep = torch.ones(sum(1 for blk in enc.blocks if blk.get("res") and blk.get("sd", 0.0) > 0.0), 6)     # (no stochastic depth)
            feat = enc.forward(images, save=True, train=True, seed=9)
            dfeat = (torch.randn(feat.shape, generator=torch.Generator().manual_seed(6)) * 0.1).to(feat.dtype).cuda()
            enc.backward(dfeat)
            enc.sync_buffers()
            torch.cuda.synchronize()
            out = (feat.float().cpu(), torch.cat([v.float().flatten().cpu() for k, v in sorted(own.g.items())]),
                   torch.cat([t.float().flatten().cpu() for k, t in sorted(enc.buffers.items()) if k.endswith(("running_mean", "running_var"))]))
            enc.release()
            return out
        finally:
            CE.BN_FOLD = False
    a, a2, b = run(False), run(False), run(True)
    dist = lambda p, q: float((p - q).norm() / q.norm())
    for i, name in enumerate(("features", "gradients", "running statistics")):
        noise, dev_ = dist(a2[i], a[i]), dist(b[i], a[i])
        print(f"{name}: folded vs three-launch {dev_:.3e}, three-launch vs itself {noise:.3e}")
        assert dev_ <= 3.0 * noise + 1e-5, (name, dev_, noise)
