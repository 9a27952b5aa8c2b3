"""tests/conv_cells_ref.py checked on the CPU: the restated dispatch against conv.hip's source and the case list against its cells,
the float64 references against torch.nn.functional in double (forward and through autograd), the exact-integer operands, the share
of elements inside a kink band, and the K table against the error of the same formulas in float32."""
import os
import re

import torch
import torch.nn.functional as F

from tests import conv_cells_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "garbage_classification_rca_amd", "csrc")
DEV = "cpu"
BIG = 1 << 21          # elements: larger shapes have the same code path in the references; they are compared once per family


def test_the_case_list_reaches_every_dispatch_cell():
    cells = R.all_cells()
    assert len(cells) == 175, sorted(cells)
    reached = set()
    for c in R.ALL_CASES:
        reached.update(R.cell(c)[0])
    assert not cells - reached, f"cells no case reaches: {sorted(cells - reached)}"
    assert not reached - cells, f"all_cells() misses {sorted(reached - cells)}"
    # the grid edges
    for C in R.STAT_C:
        for fam, cases in (("stats", R.STATS_CASES), ("bwd", R.BWD_CASES)):
            qs = [R.cell(c)[1] for c in cases if c.C == C]
            if fam == "stats" or C in (8, 72):
                assert any(q["branch"] == 256 and q["per"] > 256 and q["per"] % 32 for q in qs), f"{fam} C={C}: no ragged 256-row block"
            if fam == "stats":
                assert any(q["branch"] == 32 and q["nblk"] > 1 and q["per"] % 32 for q in qs), f"C={C}: no ragged 32-row block"
    assert any(R.cell(c)[1]["per"] >= 480 and R.cell(c)[1]["branch"] == 256 for c in R.STATS_CASES if c.C == 8)
    # the weight-gradient forms: each is selected by a workspace size computed from the restated dispatch
    for c in R.DW_CASES:
        if c.op != "bwd" or c.form == "dx" or c.mis in ("dy", "x"):
            continue
        names, q = R.cell(c)
        if c.k == 3 and c.dtype == "bf16" and c.C % 8 == 0 and c.stride == 1:
            assert q["form"] == (c.ws or "none"), (c, q)
        if c.k == 5:
            assert q["use_ws"] == (c.ws in ("full", "low")), (c, q)
    k3 = [R.cell(c)[1] for c in R.DW_CASES if c.k == 3 and "slices" in R.cell(c)[1]]
    assert {1, 2, 3} <= {q["slices"] for q in k3} and any(q["form"] == "flat" and q["lanes"] >= 64 for q in k3)
    assert any(q["form"] == "strip" and q["nranges"] > 8 for q in k3) and any(q["form"] == "none" and q["nranges"] > 1 for q in k3)
    k5 = [(c, R.cell(c)[1]) for c in R.DW_CASES if c.k == 5 and c.op == "bwd" and c.form != "dx"]
    assert any(c.ws == "small" and q["lanes"] == 64 and R.dw5_plan(c, 1 << 40, True)[1] > 64 for c, q in k5 if c.dtype == "bf16" and c.C % 8 == 0)
    assert any(c.ws == "low" and 1 <= q["lanes"] < R.dw5_plan(c, 1 << 40, R._v8(c, "dy", "x"))[1] for c, q in k5)
    for k in (3, 5):
        capped = [R.cell(c)[0] for c in R.DW_CASES if c.k == k and R.cell(c)[1].get("capped")]
        assert any("v8" in n[-1] for n in capped) and any("v8" not in n[-1] for n in capped), f"{k}x{k}: no capped pixel ranges"


def test_the_restated_dispatch_matches_conv_source():
    src = _strip_comments()          # (whitespace-normalised, // comments dropped: several conditions carry one at the end of a line)
    for s in R.SOURCE_PINS:
        assert s in src, f"conv.hip no longer contains `{s}`: restate cell() for the new dispatch"


def _strip_comments():
    with open(os.path.join(CSRC, "conv.hip")) as fh:
        text = fh.read()
    text = re.sub(r"//[^\n]*", "", text)
    return " ".join(text.split())


def _nchw(v):
    return v.permute(0, 3, 1, 2).contiguous()


def _nhwc(v):
    return v.permute(0, 2, 3, 1).contiguous()


def _uniq(cases, key):
    seen, out = set(), []
    for c in cases:
        k = key(c)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def test_depthwise_references_agree_with_conv2d_in_double():
    cases = _uniq([c for c in R.DW_CASES if not c.ints], lambda c: (c.k, c.B, c.H, c.W, c.C, c.stride))
    nbig = 0
    for c in cases:
        if c.B * c.H * c.W * c.C > BIG:
            nbig += 1
            if nbig > 2:
                continue
        g = R.gen(c, DEV)
        Ho, Wo = R.dw_out(c)
        x = R.randn(g, c.B, c.H, c.W, c.C).requires_grad_(True)
        w = R.randn(g, c.C, c.k * c.k).requires_grad_(True)
        dy = R.randn(g, c.B, Ho, Wo, c.C)
        y = F.conv2d(_nchw(x), w.view(c.C, 1, c.k, c.k), stride=c.stride, padding=c.k // 2, groups=c.C)
        y.backward(_nchw(dy))
        xd, wd = x.detach(), w.detach()
        for got, ref in ((R.dw_fwd(xd, wd, c.k, c.stride), _nhwc(y.detach())), (R.dw_bwd_data(dy, wd, c.k, c.stride, c.H, c.W), x.grad),
                         (R.dw_bwd_weight(dy, xd, c.k, c.stride), w.grad)):
            assert got.shape == ref.shape
            assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), repr(c)


def _torch_act(u, a):
    return {R.NONE: lambda v: v, R.SILU: F.silu, R.RELU: F.relu, R.SIGMOID: torch.sigmoid, R.HSWISH: F.hardswish, R.HSIGMOID: F.hardsigmoid}[a](u)


def test_batchnorm_references_agree_with_batch_norm_in_double():
    cases = _uniq([c for c in R.BWD_CASES if c.rows * c.C <= BIG or c.C == 72], lambda c: (c.rows, c.C, c.act, c.train))
    for c in cases:
        if c.rows == 1 and c.train:
            continue                        # (torch refuses one value per channel in training mode)
        g = R.gen(c, DEV)
        x = (R.randn(g, c.rows, c.C) * 2 + 1).requires_grad_(True)
        gamma, beta = (R.randn(g, c.C)).requires_grad_(True), R.randn(g, c.C).requires_grad_(True)
        dy = R.randn(g, c.rows, c.C)
        rm, rv = R.randn(g, c.C), 0.5 + R.rand(g, c.C)
        rm0, rv0 = rm.clone(), rv.clone()
        y = _torch_act(F.batch_norm(x, rm, rv, gamma, beta, training=bool(c.train), momentum=0.1, eps=R.EPS), c.act)
        y.backward(dy)
        xd = x.detach()
        if c.train:
            mu, var = xd.mean(0), xd.var(0, unbiased=False)
            n = c.rows
            assert torch.allclose(rm, 0.9 * rm0 + 0.1 * mu, rtol=1e-12, atol=1e-12)
            assert torch.allclose(rv, 0.9 * rv0 + 0.1 * var * n / (n - 1), rtol=1e-12, atol=1e-12)
        else:
            mu, var = rm0, rv0
        rs = (var + R.EPS).rsqrt()
        xh = (xd - mu) * rs
        u = xh * gamma.detach() + beta.detach()
        assert torch.allclose(R.act(u, c.act), y.detach(), rtol=1e-12, atol=1e-12), repr(c)
        du = dy * R.act_grad(u, c.act)
        sd, sx = du.sum(0), (du * xh).sum(0)
        dx = gamma.detach() * rs * (du - ((sd + xh * sx) / c.rows if c.train else 0))
        # (aten's hardswish / hardsigmoid backward hold 1/3 and 1/6 as float constants, in double too: 3e-8 relative)
        tol = 1e-7 if c.act in (R.HSWISH, R.HSIGMOID) else 1e-10
        for got, ref in ((dx, x.grad), (sx, gamma.grad), (sd, beta.grad)):
            assert float((got - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max())), repr(c)


def test_the_reference_statistics_are_the_batch_statistics():
    for c in _uniq([c for c in R.STATS_CASES if c.train and c.rows * c.C <= BIG and not R.rejected(c)], lambda c: (c.rows, c.C, c.dtype, c.mis, c.op == "moments")):
        i = R.build(c, DEV)
        ref = R.stats_ref(c, i)
        if c.op == "moments":
            d = i.x64 - i.shift
            assert torch.allclose(ref["s1"] - i.pre1, d.sum(0), rtol=1e-12, atol=1e-9) and torch.allclose(ref["s2"] - i.pre2, (d * d).sum(0), rtol=1e-12, atol=1e-9)
            continue
        mu, var = i.x64.mean(0), i.x64.var(0, unbiased=False)
        assert float((ref["mean"] - mu).abs().max()) <= 1e-11 * float(i.x64.abs().max()), repr(c)
        assert float((ref["var"] - var).abs().max()) <= 1e-9 * max(1.0, float(var.max())), repr(c)


def test_pooling_references_agree_with_torch_in_double():
    for c in R.LAYOUT_CASES:
        if c.op != "maxpool3x3s2" or c.dtype != "f32":
            continue
        g = R.gen(c, DEV)
        for ties in (True, False):
            x = (R.randint(g, -3, 3, c.B, c.H, c.W, c.C) if ties else R.randn(g, c.B, c.H, c.W, c.C)).requires_grad_(True)
            y, idx = F.max_pool2d(_nchw(x), 3, 2, 1, return_indices=True)
            ry, arg = R.maxpool_ref(x.detach())
            assert torch.equal(ry, _nhwc(y.detach())), repr(c)
            Ho, Wo = ry.shape[1:3]
            oy, ox = torch.arange(Ho).view(1, Ho, 1, 1), torch.arange(Wo).view(1, 1, Wo, 1)
            flat = (2 * oy + arg.long() // 3 - 1) * c.W + 2 * ox + arg.long() % 3 - 1
            assert torch.equal(flat, _nhwc(idx)), f"{c!r}: the first-maximum rule is not max_pool2d's"
            dy = R.randn(g, *ry.shape)
            y.backward(_nchw(dy))
            assert torch.allclose(R.maxpool_bwd_ref(dy, arg, c.H, c.W)[0], x.grad, rtol=1e-13, atol=1e-13), repr(c)
    for c in _uniq([c for c in R.POOL_CASES if c.op == "rowpool_mean"], lambda c: (c.B, c.HW, c.C)):
        i = R.build(c, DEV)
        x = i.x64.view(c.B, c.HW, c.C).clone().requires_grad_(True)
        y = F.adaptive_avg_pool1d(x.permute(0, 2, 1), 1)[:, :, 0]
        assert torch.allclose(R.pool_ref(c, i)["out"], y.detach(), rtol=1e-13, atol=1e-13)
        y.backward(i.dpool64)
        cb = R.Case("pool", "rowpool_mean_bwd", c.dtype, B=c.B, HW=c.HW, C=c.C)
        assert torch.allclose(R.pool_ref(cb, i)["dx"], x.grad.view(-1, c.C), rtol=1e-13, atol=1e-13)


def test_the_exact_integer_operands_are_exact():
    n = 0
    for c in R.ALL_CASES:
        if not c.ints:
            continue
        n += 1
        i = R.build(c, DEV)
        ref = R.FAMILIES[c.fam][1](c, i)
        t = R.tdt(c.dtype)
        for k, v in ref.items():
            if k.endswith("_mag") or k.endswith("_x") or k.startswith("_"):
                continue
            assert torch.equal(v, v.float().double()), f"{c!r}: {k} is not exact in fp32"
            if k in R.T_TYPED:
                assert torch.equal(v, v.to(t).double()), f"{c!r}: {k} is not exact in {c.dtype}"
            # every partial sum in any order: the sum of the |terms| stays below 2^24 (2^8 for what bf16 stores)
            m = ref.get(k + "_mag")
            if m is not None:
                assert float(m.max()) < 2.0 ** 24 and (k not in R.T_TYPED or c.dtype == "f32" or float(m.max()) <= 256.0), f"{c!r}: {k}"
        got = R.emulate(c, i)
        for k, v in got.items():
            assert torch.equal(v, ref[k]), f"{c!r}: {k} differs in float32"
    assert n >= 40


def test_the_kink_band_holds_at_most_half_a_percent_of_every_case():
    worst = 0.0
    for c in R.BWD_CASES + [c for c in R.POOL_CASES if c.op == "bias_act_bwd" or (c.op == "se_dx" and c.bn)]:
        if c.rows is not None and c.rows * c.C > BIG or R.rejected(c):
            continue
        i = R.build(c, DEV)
        share = float(i.near.double().mean())
        worst = max(worst, share)
        assert share <= 0.005, f"{c!r}: {share:.4f} of the elements are inside a kink band"
        if c.fam == "bwd" and c.C > 3 and c.act in R.KINKS and c.rows >= 8:
            on = sum(int((i.u == k).sum()) for k, _ in R.KINKS[c.act])
            assert on >= 1, f"{c!r}: no element exactly on a kink"
    print("worst share", worst)


def test_the_K_table_covers_the_float32_reference_error():
    worst = {}
    for c in R.ALL_CASES:
        if c.fam == "layout" or c.ints or R.rejected(c):
            continue
        i = R.build(c, DEV)
        got = R.emulate(c, i)
        ref = R.reference(c, i, got)
        for name, key, r in R.ratios(c, i, ref, got):
            if r.numel():
                w = float(r.max())
                assert w == w, f"{c!r}: {name} NaN"
                if w > worst.get(key, (0.0, None))[0]:
                    worst[key] = (w, repr(c) + ":" + name)
    print()
    bad = []
    for key in sorted(R.BOUND):
        w, where = worst.get(key, (0.0, None))
        need = max(4.0, 4.0 * w)
        print(f"  {key}: float32 reference {w:.3g} at {where} -> K >= {need:.3g} (table {R.BOUND[key]})")
        if R.BOUND[key] < need:
            bad.append((key, need))
    assert not bad, f"BOUND is below 4x the float32 reference error: {bad}"
    assert set(worst) <= set(R.BOUND)
