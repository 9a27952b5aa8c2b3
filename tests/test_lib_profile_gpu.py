"""What lib.py files in GEMM_PROFILE / KERNEL_PROFILE / CONV_PROFILE / GEMM_SHAPES while bench.py has them switched on: one launch
per wrapper family at its smallest qualifying shape, every record written out literally (derived by hand from the wrappers'
formulas: 2MNK or 6MNK FLOPs, algorithmic bytes, layouts), and nothing at all while the lists are off."""
import pytest
import torch

from garbage_classification_rca_amd import lib as L

pytestmark = pytest.mark.gpu

GEMM_FAMILY = "GEMM (1x1 conv / patch matrix / text encoder)"


def _launches():
    dev, b16 = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(3)

    def rnd(*shape, dtype=torch.float32):
        return torch.randn(*shape, device=dev, generator=g).to(dtype)

    A, B, Cb = rnd(128, 64, dtype=b16), rnd(128, 64, dtype=b16), torch.empty(128, 128, device=dev, dtype=b16)
    Af, Bf, Cf = rnd(128, 64), rnd(128, 64), torch.empty(128, 128, device=dev)
    planes = []
    for src in (Af, Bf):
        hi, lo = torch.empty_like(src, dtype=b16), torch.empty_like(src, dtype=b16)
        L.split_f32(src, hi, lo, src.numel())           # not a profiled launch
        planes.append((hi, lo))
    Ak, Bk, Ck = rnd(128, 256, dtype=b16), rnd(128, 256, dtype=b16), torch.zeros(256, 256, device=dev)
    ws = torch.empty(L.SPLITK_WS_BYTES, dtype=torch.uint8, device=dev)
    x, y = rnd(64, 8, dtype=b16), torch.empty(64, 8, device=dev, dtype=b16)
    mean, rstd, gamma, beta = torch.zeros(8, device=dev), torch.ones(8, device=dev), rnd(8, dtype=b16), rnd(8, dtype=b16)
    xd, wd, yd = rnd(16, 8, dtype=b16), rnd(8, 9, dtype=b16), torch.empty(16, 8, device=dev, dtype=b16)
    qkv, out, lse = rnd(16, 192, dtype=b16), torch.empty(16, 64, device=dev, dtype=b16), torch.empty(1, 1, 16, device=dev)
    shapes = {}
    for pre, din in (("sai", 48), ("sat", 48), ("c1", 96), ("c2", 96)):
        hid, o = (128, 96) if pre.startswith("sa") else (64, 48)
        shapes.update({f"{pre}_wq": (hid, din), f"{pre}_bq": (hid,), f"{pre}_wk": (hid, din), f"{pre}_bk": (hid,),
                       f"{pre}_wv": (o, din), f"{pre}_bv": (o,), f"{pre}_g": (o,), f"{pre}_b": (o,)})
    shapes["fin_w"], shapes["fin_b"] = (4, 1536 + 768 + 768), (4,)
    W, keep = L.HeadPtrs(), []
    for f in L.HEAD_FIELDS:
        keep.append(torch.ones(*shapes[f], device=dev) if f.endswith("_g") else rnd(*shapes[f]) * 0.05)
        setattr(W, f, keep[-1].data_ptr())
    img, txt, logits = rnd(1, 768), rnd(1, 768), torch.empty(1, 4, device=dev)
    keep += [A, B, Cb, Cf, planes, Ak, Bk, Ck, ws, x, y, mean, rstd, gamma, beta, xd, wd, yd, qkv, out, lse, img, txt, logits]
    return keep, [
        lambda: L.gemm(A, B, Cb, M=128, N=128, K=64, lda=64, ldb=64, ldc=128, dtype=L.BF16),
        lambda: L.gemm_x3(planes[0], planes[1], Cf, M=128, N=128, K=64, lda=64, ldb=64, ldc=128),
        lambda: L.gemm_splitk(Ak, Bk, Ck, ws, M=256, N=256, K=128, lda=256, ldb=256, ldc=256),
        lambda: L.bn_act_fwd(x, mean, rstd, gamma, beta, y, 64, 8, L.CONV_SILU, L.BF16),
        lambda: L.dwconv3x3_fwd(xd, wd, yd, 1, 4, 4, 8, 1, L.BF16),
        lambda: L.mha_fwd(qkv, None, out, lse, 1, 1, 16, 64, 0.125, L.BF16),
        lambda: L.head_fwd(img, txt, W, logits, 1, 768, 768, 4, True, 0, 0.0, 0, L.F32),
    ]


def _is_event(e):
    return isinstance(e, torch.cuda.Event)


def test_profile_records_are_exactly_those_of_the_wrappers_formulas(monkeypatch):
    keep, launches = _launches()
    saved = (L.GEMM_PROFILE, L.KERNEL_PROFILE, L.CONV_PROFILE, L.GEMM_SHAPES)
    gp, kp, cp, gs = [], [], [], []
    try:
        L.GEMM_PROFILE, L.KERNEL_PROFILE, L.CONV_PROFILE, L.GEMM_SHAPES = gp, kp, cp, gs
        for launch in launches:
            launch()
        torch.cuda.synchronize()
    finally:
        L.GEMM_PROFILE, L.KERNEL_PROFILE, L.CONV_PROFILE, L.GEMM_SHAPES = saved

    # GEMM_PROFILE: (executed matrix-core FLOPs, (a_layout, b_layout, accumulate), e0, e1, (M, N, K, act))
    assert [(r[0], r[1], r[4]) for r in gp] == [
        (2097152.0, (0, 0, 0), (128, 128, 64, 0)),          # gemm: 2 * 128 * 128 * 64
        (6291456.0, (0, 0, 0), (128, 128, 64, 0)),          # gemm_x3: three bf16 passes, 6 * 128 * 128 * 64
        (16777216.0, (1, 1, 1), (256, 256, 128, 0)),        # gemm_splitk: 2 * 256 * 256 * 128, K-major operands, accumulates
    ]
    assert all(type(r[0]) is float and len(r) == 5 for r in gp)
    # CONV_PROFILE: (kernel family, algorithmic HBM bytes, e0, e1)
    assert [r[:2] for r in cp] == [
        (GEMM_FAMILY, 65536),                               # gemm: (128*64 + 128*64) * 2 + 128*128 * 2
        (GEMM_FAMILY, 393216),                              # gemm_splitk: (256*128 + 256*128) * 2 + 256*256 * 4
        ("BatchNorm", 2048),                                # bn_act_fwd: read + write of 64 x 8 bf16
        ("depthwise", 512),                                 # dwconv3x3_fwd: 1 * 8 * (4*4 + 4*4) * 2
    ]
    assert all(type(r[1]) is int and len(r) == 4 for r in cp)
    assert cp[1][2] is None and cp[1][3] is None            # the split-K record carries no events (its time is in GEMM_PROFILE)
    # GEMM_SHAPES: only mmrca_gemm launches, only inside the CONV_PROFILE branch
    assert [r[:7] for r in gs] == [(128, 128, 64, 0, 0, 0, 65536)] and len(gs[0]) == 9
    # KERNEL_PROFILE: (kind, meta, e0, e1)
    assert [r[:2] for r in kp] == [("mha_fwd", (1, 1, 16, 64, False)), ("head_fwd", (1, 768, 768))]
    assert all(len(r) == 4 for r in kp)
    # one pair of events per launch, shared by the lists the launch is filed in
    assert gp[0][2] is cp[0][2] is gs[0][7] and gp[0][3] is cp[0][3] is gs[0][8]
    pairs = [(r[2], r[3]) for r in gp] + [(r[2], r[3]) for r in cp if r[2] is not None] + [(r[2], r[3]) for r in kp]
    assert len(pairs) == 3 + 3 + 2 and len({id(e) for p in pairs for e in p}) == 2 * 7
    for e0, e1 in pairs:
        assert _is_event(e0) and _is_event(e1) and e0.elapsed_time(e1) >= 0

    # the same launches with every list off: nothing is appended anywhere and no event is made
    def no_events():
        raise AssertionError("timing events created with every profile list off")
    monkeypatch.setattr(L, "_events", no_events)
    assert (L.GEMM_PROFILE, L.KERNEL_PROFILE, L.CONV_PROFILE, L.GEMM_SHAPES) == (None, None, None, None)
    for launch in launches:
        launch()
    torch.cuda.synchronize()
    assert (len(gp), len(kp), len(cp), len(gs)) == (3, 2, 4, 1)
    assert (L.GEMM_PROFILE, L.KERNEL_PROFILE, L.CONV_PROFILE, L.GEMM_SHAPES) == (None, None, None, None)
