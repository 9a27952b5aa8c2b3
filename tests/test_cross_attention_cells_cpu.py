"""tests/cross_attention_ref.py checked on the CPU: the float64 statement of the cross-attention forward against the oracle, the
restated dispatch against attention_cross.hip's source text, the case list against the cells it must reach, the inputs against the
properties the GPU test relies on (a dominant key at every tile and chunk boundary, leading by MIN_LEAD), the list of calls the
library must refuse, and the rounding models that the GPU test's bounds are taken from."""
import os
import re

import numpy as np
import pytest
import torch

from garbage_classification_rca_amd import lib as L
from garbage_classification_rca_amd.procedural import counter_uniform
from tests import cross_attention_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "garbage_classification_rca_amd", "csrc")


# ---- the reference against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,Sq,Skv,dh,p", [(2, 3, 33, 50, 40, 0.0), (2, 3, 33, 50, 40, 0.1), (1, 4, 17, 257, 88, 0.5), (3, 2, 70, 70, 64, 0.0)])
def test_cross_ref_equals_the_oracle_in_double(B, H, Sq, Skv, dh, p):
    from oracle import qformer as OQ
    g = torch.Generator().manual_seed(Sq + Skv)
    q = torch.randn(B, Sq, H * dh, generator=g, dtype=torch.float64)
    k = 2.0 * torch.randn(B, Skv, H * dh, generator=g, dtype=torch.float64)
    v = torch.randn(B, Skv, H * dh, generator=g, dtype=torch.float64)
    mask = R.drop_multiplier(77, B * H, Sq, Skv, p)
    got = R.cross_ref(q, k, v, H, dh ** -0.5, mask)
    exp = OQ.attention(q, k, v, H, mask)
    assert exp.dtype == torch.float64 and got.shape == exp.shape
    assert float((got - exp).abs().max()) <= 1e-12 * float(exp.abs().max())
    if p > 0:       # the oracle's own mask: the same bits, and its float32 (1 / (1 - p)) within an ulp of the kernels' fp32 quotient
        theirs = OQ.keep_mask(77, (B * H, Sq, Skv), p)
        assert torch.equal(theirs > 0, mask > 0) and 0 < int((mask > 0).sum()) < mask.numel()
        assert float((theirs.double() - mask).abs().max()) <= 2.0 ** -22 / (1.0 - p)
    # bf16 inputs are widened, not re-rounded
    qb = q.bfloat16()
    assert torch.equal(R.cross_ref(qb, k, v, H, 0.125), R.cross_ref(qb.double(), k, v, H, 0.125))


def test_the_mask_is_the_counter_uniform_of_block_row_key():
    BH, Sq, Skv, p = 6, 33, 50, 0.5
    keep = R.keep_bits(R.DROP_SEED, BH, Sq, Skv, p)
    for bh, i, j in ((0, 0, 0), (5, 32, 49), (2, 7, 16), (1, 0, 49)):
        u = counter_uniform(R.DROP_SEED, np.array([(bh * Sq + i) * Skv + j], dtype=np.uint64))[0]
        assert bool(keep[bh, i, j]) == bool(u >= np.float32(p))
    assert 0.45 < float(keep.double().mean()) < 0.55
    assert R.drop_scale(0.1) == float(np.float32(1) / (np.float32(1) - np.float32(0.1))) and R.drop_scale(0.5) == 2.0
    m = R.drop_multiplier(R.DROP_SEED, BH, Sq, Skv, p)
    assert set(m.unique().tolist()) == {0.0, 2.0} and R.drop_multiplier(1, BH, Sq, Skv, 0.0) is None


# ---- the restated dispatch against the source --------------------------------------------------------------------------------
def _source():
    with open(os.path.join(CSRC, "attention_cross.hip")) as fh:
        text = fh.read()
    return " ".join(re.sub(r"//[^\n]*", "", text).replace("\\\n", "\n").split())


SOURCE_PINS = (
    "static bool ax_aligned(const void* p, int64_t ld, int a) { return (((uintptr_t)p) % a) == 0 && (ld * 2) % a == 0; }",
    "ax_aligned(q, ldq, 16) && ax_aligned(k, ldk, 16) && ax_aligned(v, ldv, 16) && ax_aligned(out, ldo, 8);",
    "if (impl == MMRCA_GEMM_MFMA && !ok)", "if (ok && impl != MMRCA_GEMM_REF) {",
    "if (nkt <= N_) {", "return ax_launch<N_, 4>(",
    "if (drop_p > 0.f) return ax_launch_d<NKT, DHS, true>(",
    "const int nqt = (Sq + 15) / 16;", "const int tpw = (nqt + nw - 1) / nw;",
    "constexpr int DHP = 32 * DHS, PITCH = DHP * 2 + 16, CROWS = NKTC * 16, IMG = CROWS * PITCH;",
    "for (int k0 = 0; k0 < Skv; k0 += CROWS) {",
    "if (dhs <= 2) { if (nkt <= 2) AX3_CASE(2, 2);", "if (dhs == 3) { if (nkt <= 2) AX3_CASE(2, 3);",
    "MMRCA_REQUIRE(drop_p >= 0.f && drop_p < 1.f, \"mha_cross_fwd_x3: dropout p must be in [0,1)\");",
    "(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0 && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && "
    "(((uintptr_t)out_hi | (uintptr_t)out_lo) & 7) == 0 && ldo % 4 == 0",
    # the mask index of the three kernels and the fp32 scale
    "p[j] *= mmrca_uniform(drop_seed, ((uint64_t)blockIdx.y * Sq + i) * Skv + j) >= drop_p ? drop_sc : 0.f;",
    "const uint64_t idx0 = ((uint64_t)blockIdx.x * Sq + (q0 + l16)) * Skv + 4 * g;",
    "const uint64_t idx0 = ((uint64_t)blockIdx.x * Sq + (q0 + l16)) * Skv + k0 + 4 * g;",
    "s[kt][r] *= mmrca_uniform(drop_seed, idx0 + (kt * 16 + r)) >= drop_p ? drop_sc : 0.f;",
    "const float drop_sc = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;", "const float drop_sc = DROP ? 1.f / (1.f - drop_p) : 1.f;",
)


def test_the_restated_dispatch_matches_the_source():
    src = _source()
    for s in SOURCE_PINS:
        assert s in src, f"attention_cross.hip no longer contains `{s}`: restate dispatch() for the new source"
    assert (R.IMPL_AUTO, R.IMPL_REF, R.IMPL_MFMA) == (L.IMPL_AUTO, L.IMPL_REF, L.IMPL_MFMA)
    # mmrca_mha_cross_fwd: the AX_CASE ladder and its head-dim branches
    assert tuple(int(n) for n in re.findall(r"AX_CASE\((\d+)\)", src)) == R.NKT_LADDER
    assert re.findall(r"if \(dhs (<=|==) (\d)\) return ax_launch<N_, (\d)>", src) == [("<=", "2", "2"), ("==", "3", "3")]
    assert src.count("const int dhs = (dh + 31) / 32, nkt = (Skv + 15) / 16;") == 2
    ok = re.search(r"return dtype == MMRCA_BF16 && dh % 8 == 0 && dh <= (\d+) && Skv <= (\d+) &&", src)
    assert ok and (int(ok.group(1)), int(ok.group(2))) == (R.MAX_DH, R.MFMA_MAX_SKV)
    assert max(R.NKT_LADDER) * 16 == R.MFMA_MAX_SKV
    w = re.findall(r"const int nw = Sq > (\d+) \? (\d) : (\d);", src)
    assert w == [(str(R.MFMA_W8_ABOVE_SQ), "8", "4")]
    assert re.search(r"#define AX_MAX_DH (\d+)", src).group(1) == str(R.MAX_DH) and "#define AX_MAX_S 1024" in src
    # mmrca_mha_cross_fwd_x3: waves, query tiles per wave, the S_q rule and the AX3_CASE table
    w = re.findall(r"const int nw = nqt > (\d+) \? (\d) : (\d);", src)
    assert w == [(str(R.X3_W8_ABOVE_NQT), "8", "4")]
    tp = re.findall(r"if \(tpw (<=|==) (\d)\) return ax3_launch_t<NKTC, DHS, (true|false), (\d)>", src)
    assert tp == [(op, str(t), d, str(t)) for d in ("true", "false") for op, t in (("<=", 1), ("==", 2), ("==", 3))]
    rule = re.search(r"MMRCA_REQUIRE\(dh % 8 == 0 && dh <= (\d+) && Sq <= (\d+),", src)
    assert rule and (int(rule.group(1)), int(rule.group(2))) == (R.MAX_DH, R.X3_MAX_SQ)
    assert R.X3_MAX_SQ == 16 * 8 * R.X3_MAX_TPW
    table = {}
    for upto, n, d in re.findall(r"(?:if \(nkt <= (\d+)\) )?AX3_CASE\((\d+), (\d)\);", src):
        table.setdefault(int(d), []).append((int(upto), int(n)) if upto else int(n))
    assert {d: tuple(v) for d, v in table.items()} == R.X3_LADDER
    # the four images of a chunk fit 160 KiB
    for dhs, (*_, last) in R.X3_LADDER.items():
        assert 4 * last * 16 * (32 * dhs * 2 + 16) <= 160 * 1024
    # dispatch() at the thresholds
    d = R.dispatch
    assert d("fwd", "bf16", 0, 64, 64, 64, True, 0.0) == ("mfma", 4, 2, False, 4)
    assert d("fwd", "bf16", 0, 65, 65, 65 + 7, True, 0.1) == ("mfma", 8, 3, True, 8)
    assert d("fwd", "bf16", 2, 1, 288, 128, True, 0.0) == ("mfma", 18, 4, False, 4)
    assert d("fwd", "bf16", 0, 1, 289, 128, True, 0.0) == ("ref", "bf16", "skv>288") and d("fwd", "bf16", 2, 1, 289, 128, True, 0.0)[0] == "reject"
    assert d("fwd", "bf16", 0, 1, 129, 8, True, 0.0) == ("mfma", 14, 2, False, 4) and d("fwd", "bf16", 0, 1, 225, 8, True, 0.0)[1] == 18
    assert d("fwd", "f32", 1, 9, 9, 12, False, 0.0) == ("ref", "f32", "impl_ref") and d("fwd", "f32", 0, 9, 9, 64, True, 0.0) == ("ref", "f32", "fp32")
    assert d("x3", "f32", 0, 64, 32, 64, True, 0.0) == ("x3", 2, 2, False, 4, 1, "one chunk")
    assert d("x3", "f32", 0, 65, 33, 96, True, 0.5) == ("x3", 4, 3, True, 8, 1, "one chunk")
    assert d("x3", "f32", 0, 129, 65, 97 + 7, True, 0.0) == ("x3", 6, 4, False, 8, 2, "one chunk")
    assert d("x3", "f32", 0, 384, 161, 96, True, 0.0) == ("x3", 10, 3, False, 8, 3, "last chunk of <= 16 keys")
    assert d("x3", "f32", 0, 385, 161, 96, True, 0.0)[0] == "reject"
    assert [R.chunk_form(s, 6) for s in (96, 97, 112, 113, 192, 193)] == ["one chunk", "last chunk of <= 16 keys", "last chunk of <= 16 keys",
                                                                          "ragged last chunk", "whole chunks", "last chunk of <= 16 keys"]


# ---- the case list -----------------------------------------------------------------------------------------------------------
def test_the_case_list_reaches_every_cell():
    ids = [repr(c) for c in R.CASES]
    assert len(set(ids)) == len(ids)
    mfma, ref, x3, forms = R.all_cells()
    assert (len(mfma), len(ref), len(x3), len(forms)) == (48, 6, 72, 12)
    assert mfma - {c.cell for c in R.MFMA_CASES} == set()
    assert ref - {c.cell for c in R.REF_CASES} == set()
    assert {c.cell[2] for c in R.REF_CASES} == set(R.REF_REASONS) and {c.cell[6] for c in R.X3_CASES} == set(R.CHUNK_FORMS)
    assert x3 - {c.cell[1:6] for c in R.X3_CASES} == set()
    assert forms - {(c.cell[1], c.cell[2], c.cell[6]) for c in R.X3_CASES} == set()
    # ... and nothing the restated dispatch does not know
    assert {c.cell for c in R.MFMA_CASES} <= mfma and {c.cell for c in R.REF_CASES} <= ref and {c.cell[1:6] for c in R.X3_CASES} <= x3
    # every matrix-core cell has a case with a ragged last key tile and enough padded keys (a flat row gives each about 1 / (1.4 S_kv)
    # of its weight if it counts them as live: 3% of the keys move it by twice the bf16 bound)
    padded = lambda c: c.Skv % 16 and c.pad_keys >= 9 and c.pad_keys >= 0.03 * c.Skv      # noqa: E731
    assert mfma <= {c.cell for c in R.MFMA_CASES if padded(c)} and x3 <= {c.cell[1:6] for c in R.X3_CASES if padded(c)}
    assert any(c.pad_keys == 0 for c in R.MFMA_CASES) and any(c.pad_keys == 0 for c in R.X3_CASES)
    # every cell shows in a test id: an item's id spells its cells as a product, and the item's cases reach the whole product
    gids = [g[1] for g in R.GROUPS]
    assert len(set(gids)) == len(gids) == 14 and sorted(repr(c) for g in R.GROUPS for c in g[2]) == sorted(ids)
    named = set()
    for kernel, gid, cs in R.GROUPS:
        assert all(c.kernel == kernel for c in cs)
        f = gid.split("-")
        if kernel == "mfma":
            n, ds, drops, ws = int(f[1][1:]), f[2][1:].split("."), f[3].split("."), f[4][1:].split(".")
            want = {("mfma", n, int(d), dr == "drop", int(w)) for d in ds for dr in drops for w in ws}
            assert want == {c.cell for c in cs}, gid
        elif kernel == "x3":
            n, d, drops, wts, fms = int(f[1][1:]), int(f[2][1:]), f[3].split("."), f[4].split("."), f[5].split(".")
            want = {("x3", n, d, dr == "drop", int(wt[1]), int(wt[3])) for dr in drops for wt in wts}
            assert want == {c.cell[:6] for c in cs} and {x.replace("_", " ") for x in fms} == {c.cell[6] for c in cs}, gid
            named |= {(n, d, x.replace("_", " ")) for x in fms}
        else:
            want = {("ref",) + tuple(x.split(":")) for x in gid[4:].split(".")}
            assert want == {c.cell for c in cs}, gid
        named |= want
    assert named >= mfma | ref | {("x3",) + c for c in x3} | forms
    # both ways into the mfma kernel, both dropout rates with a seed above 2^32, every layout, B = 1
    for cs in (R.MFMA_CASES, R.REF_CASES, R.X3_CASES):
        assert {c.drop_p for c in cs} == {0.0, 0.1, 0.5} and all(c.seed > 2 ** 32 for c in cs if c.drop_p)
        assert {c.layout for c in cs} >= {"sep", "kv", "qkv"} and {c.B for c in cs} == {1, 2}
        assert any(c.peak == R.PEAK_OVERFLOW for c in cs)
        assert {1} <= {c.Sq for c in cs} and {1} <= {c.Skv for c in cs} and {8, 128} <= {c.dh for c in cs}
        assert any(c.Skv % 16 == 0 for c in cs) and any(c.Sq % 16 for c in cs) and any(c.Skv % 16 for c in cs)
    assert {c.impl for c in R.MFMA_CASES} == {R.IMPL_AUTO, R.IMPL_MFMA}
    assert any(c.Skv == 288 for c in R.MFMA_CASES) and any(c.Skv == 289 and c.impl == R.IMPL_AUTO and c.dtype == "bf16" for c in R.REF_CASES)
    assert any(c.Sq == R.X3_MAX_SQ for c in R.X3_CASES)
    assert {c.dh for c in R.MFMA_CASES if c.cell[2] == 3} >= {72, 88, 96}       # head-dim padding of 24, 8 and 0 columns
    # the smallest shapes suffice
    assert all(c.B * c.H <= 6 and c.Sq <= 384 and c.Skv <= 336 for c in R.CASES)


@pytest.fixture(scope="module")
def evaluated():
    out = []
    for c in R.CASES:
        inp = R.build(c)
        mask = R.case_mask(c)
        ref = R.cross_ref(inp.q, inp.k, inp.v, c.H, c.scale, mask)
        emu = R.emulate(c.cell, inp.q, inp.k, inp.v, c.H, c.scale, mask)
        out.append((c, inp, ref, emu))
    return out


def test_the_inputs_put_a_dominant_key_on_every_boundary(evaluated):
    worst = (float("inf"), None)
    full = set()
    for c, inp, ref, _ in evaluated:
        lead, missing = R.dominance(c, inp)
        assert not missing, f"{c!r}: boundary keys that dominate no row of (b, h): {missing}"
        assert lead >= R.MIN_LEAD, f"{c!r}: a dominant key leads its runner-up by {lead:.2f} only"
        worst = min(worst, (lead, repr(c)))
        T = inp.boundary
        S = c.Skv
        assert T == c.boundary_keys() and {j for j in (0, 15, 16, S // 16 * 16 - 1, S - 1) if 0 <= j < S} <= set(T)
        if c.kernel == "x3" and c.cell[6] != "one chunk":
            crows = 16 * c.cell[1]
            assert {crows - 1, crows} <= set(T) and any(j >= (R._cdiv(S, crows) - 1) * crows for j in T)
        pk = inp.dominant[0, 0] >= 0
        if int(pk.sum()) >= len(T):
            full.add(c.cell[:6] if c.kernel == "x3" else c.cell)
        # a third of the rows are flat; both kinds exist once there are three rows
        if c.Sq >= 3:
            assert abs(int((~pk).sum()) - c.Sq / 3) <= 1 and bool(pk.any())
        # the dominant key of a peaky row is the row's largest probability, and the row's output is close to that key's V row
        assert bool(torch.isfinite(ref).all())
    print(f"\nsmallest lead of a dominant key: {worst[0]:.2f} at {worst[1]}")
    # every cell has a case in which every boundary key dominates a row of every block
    mfma, ref_cells, x3, _ = R.all_cells()
    assert mfma <= full and ref_cells <= full and {("x3",) + c for c in x3} <= full
    # the overflow cases would overflow: exp of their largest score is not a float32
    for c, inp, _, _ in evaluated:
        if c.peak == R.PEAK_OVERFLOW:
            assert float(R.scores(inp.q, inp.k, c.H, c.scale).max()) > 89.0, repr(c)


def test_the_buffers_are_loud_around_the_live_values():
    seen = set()
    for c in R.CASES[::7] + [c for c in R.CASES if c.layout == "misaligned"][:1]:
        inp = R.build(c)
        D = c.H * c.dh
        lds = [inp.where[x][2] for x in "qkv"] + [inp.ldo]
        assert all(ld > D for ld in lds)
        if c.layout in ("sep", "misaligned"):
            assert len(set(lds)) == 4
        for name, buf in inp.bufs.items():
            live = torch.zeros(buf.shape, dtype=torch.bool)
            for x in "qkv":
                b, col, ld = inp.where[x]
                if b == name:
                    assert ld == buf.shape[1]
                    n = getattr(inp, x).shape[0] * getattr(inp, x).shape[1]
                    live[:n, col:col + D] = True
                    assert buf.shape[0] == n + R.SLACK
            assert bool((buf[~live].float().abs() == R.LOUD).all()) and float(buf[live].float().abs().max()) < 64.0
            assert bool((buf[~live].float() > 0).any()) and bool((buf[~live].float() < 0).any())
        seen.add(c.layout)
        aligned = all((ld * (2 if c.dtype == "bf16" else 4)) % 16 == 0 for ld in lds[:3])
        assert aligned == (c.layout != "misaligned") or c.dh % 8
    assert seen == {"sep", "kv", "qkv", "misaligned"}
    assert torch.tensor(R.SENT).bfloat16().item() == R.SENT and torch.tensor(R.LOUD).bfloat16().item() == R.LOUD


# ---- the calls the library must refuse ---------------------------------------------------------------------------------------
def test_the_list_of_refused_calls():
    names = [n for n, _, _ in R.REJECTED]
    assert len(set(names)) == len(names) == 22
    x3 = [o for _, e, o in R.REJECTED if e == "x3"]
    fwd = [o for _, e, o in R.REJECTED if e == "fwd"]
    assert len(x3) == 16 and len(fwd) == 6
    # x3: head dim, S_q, each stride below H dh, each pointer, a stride off, p = 1, the operand type
    assert {"dh", "Sq", "drop_p", "dtype", "offq", "offk", "offv", "offo", "ldq", "ldk", "ldv", "ldo"} == {k for o in x3 for k in o}
    assert sorted(o["dh"] for o in x3 if "dh" in o) == [12, 136] and [o["Sq"] for o in x3 if "Sq" in o] == [R.X3_MAX_SQ + 1]
    assert sum(1 for o in x3 if any(k.startswith("ld") and v < 0 for k, v in o.items())) == 4
    # fwd: what test_qformer_gpu.py's rejection test leaves out
    assert sorted(o["Skv"] for o in fwd if "Skv" in o) == [R.MFMA_MAX_SKV + 1, 300] and [o["dh"] for o in fwd if "dh" in o] == [12]
    assert R.BASE["fwd"]["impl"] == R.IMPL_MFMA
    for name, entry, over in R.REJECTED:
        a = dict(R.BASE[entry], **over)
        # the base call is valid, and the restated dispatch refuses what it models of the changed one
        b = R.BASE[entry]
        assert R.dispatch(entry, b["dtype"], b["impl"], b["Sq"], b["Skv"], b["dh"], True, b["drop_p"])[0] in ("mfma", "x3")
        size = 2 if a["dtype"] == "bf16" else 4
        aligned = True
        for k, val in over.items():
            if k.startswith("off"):
                aligned &= (val * (2 if k == "offo" and entry == "x3" else size)) % (8 if k == "offo" else 16) == 0
            if k.startswith("ld") and val > 0:
                aligned &= (val * size) % (8 if k == "ldo" and entry == "fwd" else 16) == 0 if entry == "fwd" else val % 4 == 0
        if any(k.startswith("ld") and val < 0 for k, val in over.items()):
            continue
        assert R.dispatch(entry, a["dtype"], a["impl"], a["Sq"], a["Skv"], a["dh"], aligned, a["drop_p"])[0] == "reject", name


# ---- the rounding models: where the GPU test's bounds come from --------------------------------------------------------------
def test_the_rounding_models_set_the_bounds(evaluated):
    worst = {}
    for c, inp, ref, emu in evaluated:
        blk, row = R.errors(emu, ref, c.H)
        b, r = float(blk.max()), float(row.max())
        assert b == b and r == r, repr(c)
        key = R.bound_key(c)
        wb, wr = worst.get(key, ((0.0, None), (0.0, None)))
        worst[key] = (max(wb, (b, repr(c))), max(wr, (r, repr(c))))
        if c.Skv == 1:          # one key: the output is the V row in the output format
            v = inp.v.double().expand(c.B, c.Sq, -1)
            want = v.bfloat16().double() if c.out_dtype == "bf16" and c.entry != "x3" else v
            if c.entry == "x3":
                want = v.bfloat16().double() + (v - v.bfloat16().double()).bfloat16().double()
            assert torch.equal(emu, want), repr(c)
    print()
    for key, (wb, wr) in sorted(worst.items()):
        print(f"  {key}: rounding model against float64, per block {wb[0]:.3g} at {wb[1]}, per row {wr[0]:.3g} at {wr[1]}")
    # bf16 matrix-core cells: the cap of test_attention_cells_gpu.py, with the model 1.5x under it
    assert max(worst["mfma"][0][0], worst["mfma"][1][0]) <= R.MFMA_CAP / R.MFMA_HEADROOM, worst["mfma"]
    # the committed figures are the measured ones
    for key in ("mfma", "x3", "ref_f32"):
        for i in (0, 1):
            assert worst[key][i][0] <= R.EMULATED[key][i] <= 1.25 * worst[key][i][0], (key, i, worst[key][i], R.EMULATED[key])
    # x3 and fp32 ref: 4x the model, under the caps; bf16 ref: one output rounding on top of the fp32 bound
    assert R.MARGIN == 4.0 and R.X3_CAP == 1e-4 and R.REF_F32_CAP == 2e-5 and R.MFMA_CAP == 1e-2
    for cs, key, cap in ((R.X3_CASES, "x3", R.X3_CAP), (R.REF_CASES, "ref_f32", R.REF_F32_CAP)):
        c = next(c for c in cs if c.dtype == "f32")
        assert R.bound(c) == tuple(R.MARGIN * e for e in R.EMULATED[key]) and max(R.bound(c)) <= cap
    c16, c32 = (next(c for c in R.REF_CASES if c.dtype == d) for d in ("bf16", "f32"))
    assert R.bound(c16) == tuple(2.0 ** -8 + e for e in R.bound(c32))
    assert worst["ref_bf16"][0][0] <= R.bound(c16)[0] and worst["ref_bf16"][1][0] <= R.bound(c16)[1]
    assert R.bound(R.MFMA_CASES[0]) == (R.MFMA_CAP, R.MFMA_CAP)
