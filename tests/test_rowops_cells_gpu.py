"""Every dispatch cell of the LayerNorm kernels in csrc/rowops.hip (add_ln_fwd_bf16_k, add_ln_fwd_k with and without the bf16x3
planes, ln_bwd_bf16_k with an fp32 or bf16 saved sum, ln_bwd_k) against a float64 statement of the same operation on the kernel's
exact inputs, and the rest of rowops.hip (GELU backward, column sums, embeddings, patchify, ViT assembly, loss, optimizers, casts,
stochastic-depth scales) against float64 or bitwise.  Needs an MI355X; every call goes through the C ABI.

Inputs are built to expose what randn hides: rows with a large common offset (|mean| >> std: a one-pass variance or a dropped
centring shows), rows of near-constant values (rstd near 1/sqrt(eps)), gamma and beta of mixed signs, and loud finite values in
every input column and row the kernel must not read.  Outputs start as NaN inside the owned region and as a sentinel outside it
(guard columns [D, ld), guard rows, guard elements); every owned element must be written and no sentinel touched.  Every case runs
twice: the non-atomic outputs must repeat bitwise, the atomic column sums within their bound.

Bounds are elementwise, in units of the natural error scale of each output (each is >= 4x the worst value
observed over the case list, written next to it):
  y, ds, dbranch ..... |err| <= K * (ulp_T(|ref|) + 2^-24 * size of the terms) [+ the forward's statistics term, below]
  mean ............... |err| <= K * 2^-24 * mean_row |s|
  rstd ............... |err| <= K * 2^-24 * rstd
  column sums ........ |err| <= K * 2^-24 * (|prefill| + sum_rows |term|)   (never relative to the sum itself: it cancels)
The forward's y is compared with the float64 normalisation of the exact sum; the kernel's own fp32 mean / rstd errors (bounded
tightly above) enter its bound to first order: |gamma| * (|d mean| * rstd + |xhat| * |d rstd| / rstd)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import lib as L                 # noqa: E402
from garbage_classification_rca_amd.procedural import counter_uniform  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "garbage_classification_rca_amd", "csrc")
U = 2.0 ** -24                 # fp32 unit roundoff
SENT = -3072.0                 # guard sentinel (exact in bf16)
LOUD = 8192.0                  # magnitude of the unread input slack
GUARD = 8                      # guard rows behind every row-major buffer, guard elements behind every vector
P_DROP = 0.1
IN_SEED, OUT_SEED, DY_SEED, BR_SEED = 11, 22, 33, 44
EPOCH = 3                      # the nonzero mask epoch of the epoch cases
STRIDE = L.SEED_EPOCH_STRIDE

# K per (output, dtype): observed worst over the case list next to each (seeded inputs; every kernel repeats bitwise)
BOUND = {
    ("y", "bf16"): 4.0,          # observed 0.99 (the bf16 rounding of y: half an ulp of the kernel's fp32 value)
    ("y", "f32"): 5.0,           # observed 1.2
    ("planes", "f32"): 4.0,      # observed 0.99 (y_hi + y_lo, in units of 2^-16 |y|)
    ("mean", "bf16"): 26.0,      # observed 6.46
    ("mean", "f32"): 13.0,       # observed 3.01
    ("rstd", "bf16"): 16.0,      # observed 3.93
    ("rstd", "f32"): 12.0,       # observed 2.85
    ("ds", "bf16"): 3.0,         # observed 0.72
    ("ds", "f32"): 8.0,          # observed 1.93
    ("dbranch", "bf16"): 2.0,    # observed 0.50
    ("dbranch", "f32"): 8.0,     # observed 1.74
    ("colsum", "bf16"): 12.0,    # observed 2.77-2.84 (dgamma, dbeta, dcol, dcol_branch; atomic order varies)
    ("colsum", "f32"): 16.0,     # observed 2.89-3.51
}
OBSERVED = {}


def _note(key, v):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need a GPU"
    L.load()
    L.seed_epoch_set(0)            # test_graph_gpu.py moves the mask epoch
    torch.cuda.synchronize()
    yield
    print("\nrowops cells: worst observed error / bound unit")
    for k in sorted(OBSERVED, key=str):
        b = BOUND.get(k, MISC_BOUND.get(k))
        print(f"  {k}: {OBSERVED[k]:.3g}  (bound {b})")


# ------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _tf(b):
    return "true" if b else "false"


class Case:
    """one LayerNorm call.  op 'fwd' | 'x3' (mmrca_add_layernorm_fwd_x3) | 'bwd' | 'mixed'; lds: (ld_x, ld_y) forward, (ld_dy, ld_s,
    ld_ds) backward; mis: the first operand (x, dy) starts 8 bytes past a 16-byte boundary; planes (x3) 'y' = y and the planes,
    'only' = planes only"""

    def __init__(self, op, dtype, D, rows, lds=None, mis=False, res=False, sum_out=False, in_p=0.0, out_p=0.0, planes="y",
                 dres=False, dbranch=False, dcol=False, dcol_branch=False, dy_p=0.0, br_p=0.0, eps=1e-6, epoch=0, tag=""):
        self.op, self.dtype, self.D, self.rows, self.mis = op, dtype, D, rows, mis
        n = 2 if op in ("fwd", "x3") else 3
        self.lds = tuple(lds) if lds is not None else (D,) * n
        self.res, self.sum_out, self.in_p, self.out_p, self.planes = res, sum_out, in_p, out_p, planes
        self.dres, self.dbranch, self.dcol, self.dcol_branch, self.dy_p, self.br_p = dres, dbranch, dcol, dcol_branch, dy_p, br_p
        self.eps, self.epoch, self.tag = eps, epoch, tag

    def __repr__(self):
        o = [self.op, self.dtype, f"D{self.D}", f"r{self.rows}"]
        if any(ld != self.D for ld in self.lds):
            o.append("ld" + "_".join(map(str, self.lds)))
        for k in ("mis", "res", "sum_out", "dres", "dbranch", "dcol", "dcol_branch"):
            if getattr(self, k):
                o.append(k)
        for k in ("in_p", "out_p", "dy_p", "br_p"):
            if getattr(self, k):
                o.append(k)
        if self.op == "x3":
            o.append("planes-" + self.planes)
        if self.epoch:
            o.append(f"epoch{self.epoch}")
        if self.tag:
            o.append(self.tag)
        return "-".join(o)


def cell(c):
    """(template, rows per grid round) of the launch the call `c` reaches (rowops.hip line numbers)"""
    D, R, bf = c.D, max(c.rows, 0), c.dtype == "bf16"
    t = "bf16" if bf else "float"
    if c.op in ("fwd", "x3"):
        fast = (c.op == "fwd" and bf and D % 8 == 0 and D <= 1536 and all(ld % 8 == 0 for ld in c.lds)   # :213-214
                and not c.mis)
        if fast:
            nv2 = _cdiv(D, 512)                                            # :225
            rp = 2 if nv2 <= 2 else 1                                      # :229
            pack = c.sum_out or (not c.res and c.in_p == 0)                # :227
            drop = c.in_p > 0 or c.out_p > 0                               # :228
            return f"add_ln_fwd_bf16_k<{nv2},{rp},{_tf(pack)},{_tf(drop)}>", 4 * min(_cdiv(R, 8), 1024) * rp   # :215, :125
        nv = _cdiv(D, 256)                                                 # :240
        nv = nv if nv <= 4 else 8                                          # :242-243
        planes = "[y_hi,y_lo]" if c.op == "x3" else ""                     # :260-266 (fp32 only, :209)
        return f"add_ln_fwd_k<{t},{nv}>{planes}", 4 * min(_cdiv(R, 4), 4096)                                 # :235
    if c.op == "bwd":
        fast = (bf and D % 8 == 0 and D <= 1024 and all(ld % 8 == 0 for ld in c.lds) and not c.mis)         # :518-520
        if fast:
            nv2 = 1 if _cdiv(D, 512) <= 1 else 2                           # :529-530
            return f"ln_bwd_bf16_k<{nv2},{_tf(c.dcol)},{_tf(c.dbranch)}>", 8 * min(_cdiv(R, 8), 256)          # :515-516, :527
        nv = _cdiv(D, 256)                                                 # :540
        nv = nv if nv <= 4 else 8                                          # :542-543
        return f"ln_bwd_k<{t},{nv}>", 4 * min(_cdiv(R, 4), 1024)                                            # :512-514
    nv2 = 1 if D <= 512 else 2                                             # :574
    return f"ln_bwd_bf16_k<{nv2},{_tf(c.dcol)},{_tf(c.dbranch)},true>", 8 * min(_cdiv(R, 8), 256)            # :564-565, :572


def all_cells():
    """every template cell() can return over the arguments the entry points accept"""
    out = set()
    for D in range(4, 2049, 4):
        for dtype in ("bf16", "f32"):
            for odd_ld in (False, True):
                for mis in (False, True):
                    for res, sum_out, in_p, out_p in ((a, b, p, q) for a in (0, 1) for b in (0, 1) for p in (0, .1) for q in (0, .1)):
                        c = Case("fwd", dtype, D, 1, lds=(D + 4 * odd_ld, D), mis=mis, res=res, sum_out=sum_out, in_p=in_p, out_p=out_p)
                        out.add(cell(c)[0])
                        if dtype == "f32":
                            c.op = "x3"
                            out.add(cell(c)[0])
                    for dbranch, dcol in ((a, b) for a in (0, 1) for b in (0, 1)):
                        c = Case("bwd", dtype, D, 1, lds=(D, D, D + 4 * odd_ld), mis=mis, dbranch=dbranch, dcol=dcol)
                        out.add(cell(c)[0])
                        if dtype == "bf16" and D % 8 == 0 and D <= 1024 and not odd_ld and not mis:
                            c.op = "mixed"
                            out.add(cell(c)[0])
    return out


# ------------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------------
P = P_DROP
FWD_OPTS = (  # (res, sum_out, in_p, out_p)
    (True, True, 0, 0),        # residual add with the stored sum (ViT LN2, the text encoder's post-LN)
    (False, False, 0, 0),      # plain x (ViT LN1)
    (True, True, P, 0),        # branch dropout before the residual add, stored sum
    (False, False, 0, P),      # embedding LayerNorm with output dropout
    (True, False, 0, 0),       # residual without a stored sum: the fp32-row form
    (True, False, P, 0),       # ... with branch dropout
    (False, False, P, 0),      # dropout on x alone: the fp32-row form
    (False, True, 0, P),       # stored sum without a residual
)
BWD_OPTS = (  # (dres, dbranch, dcol, dcol_branch, dy_p, br_p)
    (True, False, True, False, 0, 0),      # ViT: residual gradient + bias gradient
    (False, True, False, True, 0, P),      # text encoder: dropped branch + its bias gradient
    (False, False, True, False, 0, 0),     # text encoder without dropout
    (True, True, True, True, P, P),        # everything
    (False, False, False, False, 0, 0),    # plain
    (True, True, False, False, P, 0),      # dbranch without its column sums
    (False, False, False, False, P, 0),    # dropout on dy alone
    (True, True, True, False, 0, P),       # dbranch and dcol, no dcol_branch
)


def _two_rounds(op, D, dtype, fast):
    """rows = two full grid rounds and a ragged remainder of the cell"""
    if op in ("fwd", "x3"):
        if fast:
            rnd = 4 * 1024 * (2 if _cdiv(D, 512) <= 2 else 1)
        else:
            rnd = 4 * 4096
    else:
        rnd = 8 * 256 if fast else 4 * 1024
    return 2 * rnd + 37


def _fwd(op, dtype, D, rows, k, **kw):
    res, sum_out, in_p, out_p = FWD_OPTS[k % len(FWD_OPTS)]
    return Case(op, dtype, D, rows, res=res, sum_out=sum_out, in_p=in_p, out_p=out_p, eps=(1e-6, 1e-12)[k % 2], **kw)


def _bwd(op, dtype, D, rows, k, **kw):
    dres, dbranch, dcol, dcol_branch, dy_p, br_p = BWD_OPTS[k % len(BWD_OPTS)]
    return Case(op, dtype, D, rows, dres=dres, dbranch=dbranch, dcol=dcol, dcol_branch=dcol_branch, dy_p=dy_p, br_p=br_p, **kw)


def _cases():
    cs = []
    # the bf16 forward fast path: every option set at the slab edges of each NV2, a few rows; two rounds at the widest D of each NV2
    for i, D in enumerate((8, 504, 512, 520, 768, 1024, 1032, 1408, 1536)):
        for k in range(len(FWD_OPTS)):
            cs.append(_fwd("fwd", "bf16", D, (1, 7, 37)[(i + k) % 3], k, lds=(D + 8 * (k % 3 == 2), D + 8 * (k % 4 == 1))))
            if D in (512, 1024, 1536) and k in (0, 2, 4, 5):         # PACK x DROP
                cs.append(_fwd("fwd", "bf16", D, _two_rounds("fwd", D, "bf16", True), k))
    # the generic forward: fp32, and bf16 by each fallback route (D % 8, D > 1536, ld % 8, a misaligned operand)
    gen = [("f32", D, {}) for D in (4, 252, 256, 260, 768, 1020, 1024, 1028, 1408, 1540, 2048)]
    gen += [("bf16", D, {}) for D in (4, 252, 260, 1020, 1028, 1540, 2048)]
    gen += [("bf16", 768, {"lds": (772, 768)}), ("bf16", 768, {"lds": (768, 772)}), ("bf16", 256, {"mis": True}),
            ("bf16", 1024, {"mis": True}), ("bf16", 1408, {"mis": True})]
    for i, (dt, D, kw) in enumerate(gen):
        for j, k in enumerate((i % 8, (i + 3) % 8, (i + 5) % 8)):
            cs.append(_fwd("fwd", dt, D, (1, 7, 37)[j], k, **kw))
    for i, (dt, D) in enumerate((("f32", 256), ("f32", 260), ("f32", 768), ("f32", 1024), ("f32", 1028), ("bf16", 252),
                                 ("bf16", 260), ("bf16", 1020), ("bf16", 1540))):
        cs.append(_fwd("fwd", dt, D, _two_rounds("fwd", D, dt, False), (0, 5, 2, 4)[i % 4]))
    cs.append(_fwd("fwd", "bf16", 768, _two_rounds("fwd", 768, "bf16", False), 2, mis=True))
    cs.append(_fwd("fwd", "bf16", 520, 0, 0))
    cs.append(_fwd("fwd", "f32", 260, 0, 0))
    # the bf16x3 planes
    for i, D in enumerate((4, 256, 260, 768, 1024, 1028, 1408, 2048)):
        for j, (k, pl) in enumerate(((i % 8, "y"), ((i + 3) % 8, "only"), ((i + 6) % 8, "y"))):
            cs.append(_fwd("x3", "f32", D, (1, 7, 37)[j], k, planes=pl, lds=(D + 4 * (k % 2), D + 4 * (k % 3 == 0))))
        if D in (256, 260, 768, 1024, 1408):
            cs.append(_fwd("x3", "f32", D, _two_rounds("x3", D, "f32", False), i, planes=("y", "only")[i % 2]))
    cs.append(_fwd("x3", "f32", 768, 0, 0))
    # the bf16 backward fast path and the mixed backward: every option set, two rounds at the widest D of each NV2
    for op in ("bwd", "mixed"):
        for i, D in enumerate((8, 504, 512, 520, 768, 1024)):
            for k in range(len(BWD_OPTS)):
                cs.append(_bwd(op, "bf16", D, (1, 7, 37)[(i + k) % 3], k, lds=(D + 8 * (k % 3 == 1), D + 8 * (k % 4 == 2), D + 8 * (k % 2))))
                if D in (512, 1024):
                    cs.append(_bwd(op, "bf16", D, _two_rounds(op, D, "bf16", True), k))
        cs.append(_bwd(op, "bf16", 768, 0, 3))
    # the generic backward: fp32, and bf16 by each fallback route (D % 8, D > 1024, ld % 8, a misaligned operand)
    gen = [("f32", D, {}) for D in (4, 252, 256, 260, 768, 1020, 1024, 1028, 1408, 2048)]
    gen += [("bf16", D, {}) for D in (4, 252, 260, 1020, 1028, 1032, 1408, 2048)]
    gen += [("bf16", 768, {"lds": (772, 768, 768)}), ("bf16", 768, {"lds": (768, 768, 772)}), ("bf16", 512, {"mis": True}),
            ("bf16", 1024, {"mis": True})]
    for i, (dt, D, kw) in enumerate(gen):
        for j, k in enumerate((i % 8, (i + 3) % 8, (i + 5) % 8)):
            cs.append(_bwd("bwd", dt, D, (1, 7, 37)[j], k, **kw))
    for i, (dt, D) in enumerate((("f32", 256), ("f32", 260), ("f32", 768), ("f32", 1024), ("f32", 2048), ("bf16", 252),
                                 ("bf16", 260), ("bf16", 1020), ("bf16", 1408))):
        cs.append(_bwd("bwd", dt, D, _two_rounds("bwd", D, dt, False), (0, 3, 1, 5)[i % 4]))
    cs.append(_bwd("bwd", "bf16", 768, _two_rounds("bwd", 768, "bf16", False), 1, mis=True))
    cs.append(_bwd("bwd", "f32", 260, 0, 0))
    # strided class-token rows (engine.py: the ViT's final LayerNorm over rows b * Tn, forward and backward)
    for dt in ("bf16", "f32"):
        for B in (37, 300):
            tnd = 197 * 768
            cs.append(Case("fwd", dt, 768, B, lds=(tnd, 768), tag="cls-rows"))
            cs.append(Case("fwd", dt, 768, B, lds=(tnd, 768), res=True, sum_out=True, tag="cls-rows"))
            cs.append(Case("bwd", dt, 768, B, lds=(768, tnd, tnd), dcol=True, tag="cls-rows"))
            cs.append(Case("bwd", dt, 768, B, lds=(768, tnd, tnd), dres=True, dbranch=True, dcol=True, dcol_branch=True,
                           br_p=P, tag="cls-rows"))
    # a nonzero mask epoch: rowops' own copy of the epoch is honoured
    cs.append(_fwd("fwd", "bf16", 768, 4133, 2, epoch=EPOCH))
    cs.append(_fwd("fwd", "bf16", 768, 37, 3, epoch=EPOCH))
    cs.append(_fwd("fwd", "f32", 260, 37, 5, epoch=EPOCH))
    cs.append(_bwd("bwd", "bf16", 1024, 4133, 3, epoch=EPOCH))
    cs.append(_bwd("bwd", "f32", 260, 37, 3, epoch=EPOCH))
    cs.append(_bwd("mixed", "bf16", 512, 4133, 3, epoch=EPOCH))
    return cs


CASES = _cases()
# the real ViT-B/16 shape at batch 256 (50,432 token rows of 768): LN1, LN2 and the backward of LN2
VIT_CASES = [Case("fwd", "bf16", 768, 50432, tag="vit"), Case("fwd", "bf16", 768, 50432, res=True, sum_out=True, tag="vit"),
             Case("bwd", "bf16", 768, 50432, dres=True, dcol=True, tag="vit")]


# ------------------------------------------------------------------------------------------------------
# inputs, masks, buffers
# ------------------------------------------------------------------------------------------------------
def _tdt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _s64(c):
    c &= (1 << 64) - 1
    return c - (1 << 64) if c >= (1 << 63) else c


def _lsr(z, k):
    return (z >> k) & ((1 << (64 - k)) - 1)


def uniform(seed, idx):
    """csrc/common.h::mmrca_uniform on the GPU (int64 arithmetic wraps like uint64); `seed` already includes the epoch term"""
    z = idx.add(1).mul(_s64(0x9E3779B97F4A7C15)).add(_s64(seed))
    z = (z ^ _lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _s64(0x94D049BB133111EB)
    z = z ^ _lsr(z, 31)
    return _lsr(z, 40).to(torch.float32) * (1.0 / 16777216.0)


def _keep_scale(p, seed, epoch, rows, D):
    """float64 [rows, D]: keep / (1 - p) of counter r * D + c, with the scale the kernel uses (fp32 1 / (1 - p)); None if p == 0"""
    if p == 0:
        return None
    idx = torch.arange(rows * D, device="cuda", dtype=torch.int64)
    keep = uniform(seed + epoch * STRIDE, idx) >= float(np.float32(p))
    sc = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return (keep.double() * sc).view(rows, D)


def _rows(rows, D, g, offset=40.0):
    """float64 rows of three kinds: randn; randn + a large common offset; near-constant"""
    v = torch.randn(rows, D, generator=g, device="cuda", dtype=torch.float64)
    kind = torch.arange(rows, device="cuda") % 3
    off = offset * torch.randn(rows, 1, generator=g, device="cuda", dtype=torch.float64).sign()
    v = torch.where((kind == 1)[:, None], v + off, v)
    c = torch.randn(rows, 1, generator=g, device="cuda", dtype=torch.float64)
    return torch.where((kind == 2)[:, None], c + 1e-3 * v, v)


def _operand(vals, ld, tdt, g, mis=0):
    """a kernel operand holding vals [rows, D] at row stride ld, loud values in every other element; (tensor to pass, exact float64)"""
    rows, D = vals.shape
    flat = (LOUD * torch.randn(mis + (rows + GUARD) * ld, generator=g, device="cuda").sign()).to(tdt)
    body = flat[mis:mis + rows * ld].view(rows, ld)
    body[:, :D] = vals.to(tdt)
    return flat[mis:], body[:, :D].double()


def _vec_operand(vals, tdt):
    flat = torch.full((vals.numel() + GUARD,), LOUD, dtype=tdt, device="cuda")
    flat[:vals.numel()] = vals.to(tdt)
    return flat, flat[:vals.numel()].double()


class Out:
    """an output: owned [rows, D] at stride ld starts NaN (or `fill`), everything else the sentinel"""

    def __init__(self, rows, D, ld, tdt, fill=None, mis=0, grows=GUARD):
        self.rows, self.D, self.ld, self.mis = rows, D, ld, mis
        self.flat = torch.full((mis + (rows + grows) * ld,), SENT, dtype=tdt, device="cuda")
        self.body = self.flat[mis:mis + rows * ld].view(rows, ld)
        self.body[:, :D] = float("nan") if fill is None else fill.to(tdt)
        self.t = self.flat[mis:]

    @property
    def owned(self):
        return self.body[:, :self.D]

    def untouched(self):
        s = torch.tensor(SENT, dtype=self.flat.dtype, device="cuda")
        return (bool((self.flat[:self.mis] == s).all()) and bool((self.flat[self.mis + self.rows * self.ld:] == s).all())
                and bool((self.body[:, self.D:] == s).all()))


def _vout(n, tdt=torch.float32, fill=None):
    """a vector output of n elements (NaN, or `fill`) and GUARD sentinel elements behind it"""
    return Out(1, n, n + GUARD, tdt, fill=None if fill is None else fill.view(1, n), grows=0)


def _ulp(v, tdt):
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - (7 if tdt == torch.bfloat16 else 23))


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _first_bad(bad):
    idx = torch.nonzero(bad)
    return tuple(int(i) for i in idx[0]) if idx.numel() else None


class Fail(list):
    def check(self, case, key, ratio, what):
        """ratio: error / bound unit, per element; records the worst and fails above the bound"""
        if ratio.numel() == 0:
            return
        worst = float(ratio.max())
        _note(key, worst)
        if not worst <= BOUND[key]:
            where = _first_bad(~(ratio <= BOUND[key]))
            self.append(f"{what}: error {worst:.3g} > {BOUND[key]} units at (row, col) {where}")


# ------------------------------------------------------------------------------------------------------
# LayerNorm forward
# ------------------------------------------------------------------------------------------------------
class FwdIn:
    def __init__(self, c, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        tdt, R, D = _tdt(c.dtype), c.rows, c.D
        ld_x, ld_y = c.lds
        mis = 4 if c.mis else 0                      # 8 bytes of bf16: an 8-byte-aligned x off its 16-byte boundary
        self.x, self.x64 = _operand(_rows(R, D, g), ld_x, tdt, g, mis)
        self.r, self.r64 = _operand(0.5 * torch.randn(R, D, generator=g, device="cuda", dtype=torch.float64), ld_x, tdt, g)
        self.gm, self.gm64 = _vec_operand(torch.randn(D, generator=g, device="cuda", dtype=torch.float64), tdt)
        self.bt, self.bt64 = _vec_operand(0.5 * torch.randn(D, generator=g, device="cuda", dtype=torch.float64), tdt)
        self.kin = _keep_scale(c.in_p, IN_SEED, c.epoch, R, D)
        self.kout = _keep_scale(c.out_p, OUT_SEED, c.epoch, R, D)


def _fwd_run(c, inp):
    tdt, R, D = _tdt(c.dtype), c.rows, c.D
    ld_x, ld_y = c.lds
    o = {"y": Out(R, D, ld_y, tdt) if (c.op == "fwd" or c.planes == "y") else None,
         "sum": Out(R, D, ld_x, tdt) if c.sum_out else None,
         "mean": _vout(R), "rstd": _vout(R)}
    if c.op == "x3":
        o["hi"], o["lo"] = Out(R, D, ld_y, torch.bfloat16), Out(R, D, ld_y, torch.bfloat16)
    t = lambda k: None if o.get(k) is None else o[k].t      # noqa: E731
    if c.epoch:
        L.seed_epoch_set(c.epoch)
    try:
        L.add_layernorm_fwd(inp.x, inp.r if c.res else None, inp.gm, inp.bt, t("sum"), t("y"), t("mean"), t("rstd"), R, D, ld_x,
                            ld_y, c.eps, L.dtype_code(tdt), in_drop=(c.in_p, IN_SEED), out_drop=(c.out_p, OUT_SEED),
                            y_planes=(t("hi"), t("lo")) if c.op == "x3" else None)
        torch.cuda.synchronize()
    finally:
        if c.epoch:
            L.seed_epoch_set(0)
    return o


def _fwd_check(c, inp, o):
    tdt, R, D = _tdt(c.dtype), c.rows, c.D
    fails = Fail()
    for k, b in o.items():
        if b is not None:
            assert b.untouched(), f"{c!r}: a guard element of {k} was written"
            bad = ~torch.isfinite(b.owned.float())
            assert not bool(bad.any()), f"{c!r}: {k} not written / not finite at {_first_bad(bad)}"
    if R == 0:
        return fails
    # the fp32 host statement of the sum: (x * keep * float32(1 / (1 - p))) + res
    a = inp.x64.float()
    if inp.kin is not None:
        a = a * inp.kin.float()                      # keep * sc is 0 or exactly the fp32 scale: one fp32 product
    if c.res:
        a = a + inp.r64.float()
    # the stored sum is rounded once and normalised as rounded; otherwise the fp32 sum is normalised
    s = a.to(tdt).float() if c.sum_out else a
    if c.sum_out:
        got = o["sum"].owned
        bad = _bits(got) != _bits(a.to(tdt))
        assert not bool(bad.any()), f"{c!r} [{cell(c)[0]}]: stored sum differs from the fp32 host sum at {_first_bad(bad)}"
    s = s.double()
    eps = float(np.float32(c.eps))
    mu = s.mean(1)
    rs = ((s - mu[:, None]).square().mean(1) + eps).rsqrt()
    mk, rk = o["mean"].owned[0].double(), o["rstd"].owned[0].double()
    key = c.dtype
    fails.check(c, ("mean", key), (mk - mu).abs() / (U * s.abs().mean(1)).clamp(min=1e-30), "mean")
    fails.check(c, ("rstd", key), (rk - rs).abs() / (U * rs), "rstd")
    xh = (s - mu[:, None]) * rs[:, None]
    y = xh * inp.gm64 + inp.bt64
    arith = (xh * inp.gm64).abs() + inp.bt64.abs()
    # first order in the kernel's own statistics errors: gamma * (d mean * rstd + xhat * d rstd / rstd)
    stats = inp.gm64.abs() * ((mk - mu).abs()[:, None] * rs[:, None] + xh.abs() * ((rk - rs).abs() / rs)[:, None])
    if inp.kout is not None:
        y, arith, stats = y * inp.kout, arith * inp.kout, stats * inp.kout
    stats = 1.01 * stats
    if o["y"] is not None:
        err = (o["y"].owned.double() - y).abs()
        fails.check(c, ("y", key), err / (_ulp(y, tdt) + U * arith + stats), "y")
    if c.op == "x3":
        hi, lo = o["hi"].owned, o["lo"].owned
        if o["y"] is not None:                      # the planes are the split of the fp32 y: bitwise
            yk = o["y"].owned
            bad = (_bits(hi) != _bits(yk.bfloat16())) | (_bits(lo) != _bits((yk - yk.bfloat16().float()).bfloat16()))
            assert not bool(bad.any()), f"{c!r}: y_hi / y_lo are not the bf16 split of y at {_first_bad(bad)}"
        err = (hi.double() + lo.double() - y).abs()
        fails.check(c, ("planes", key), err / (2.0 ** -16 * y.abs() + U * arith + stats + 2.0 ** -133), "y_hi + y_lo")
    return fails


# ------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ------------------------------------------------------------------------------------------------------
class BwdIn:
    def __init__(self, c, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        tdt, R, D = _tdt(c.dtype), c.rows, c.D
        sdt = torch.float32 if c.op == "mixed" else tdt
        ld_dy, ld_s, ld_ds = c.lds
        mis = 4 if c.mis else 0
        self.dy, self.dy64 = _operand(torch.randn(R, D, generator=g, device="cuda", dtype=torch.float64), ld_dy, tdt, g, mis)
        self.s, self.s64 = _operand(_rows(R, D, g), ld_s, sdt, g)
        self.dres, self.dres64 = _operand(torch.randn(R, D, generator=g, device="cuda", dtype=torch.float64), ld_ds, tdt, g)
        self.gm, self.gm64 = _vec_operand(torch.randn(D, generator=g, device="cuda", dtype=torch.float64), tdt)
        mu = self.s64.mean(1) if R else torch.zeros(0, device="cuda", dtype=torch.float64)
        rs = ((self.s64 - mu[:, None]).square().mean(1) + 1e-6).rsqrt() if R else mu
        self.mean, self.mean64 = _vec_operand(mu, torch.float32)
        self.rstd, self.rstd64 = _vec_operand(rs, torch.float32)
        self.pre = {k: 8.0 * torch.randn(D, generator=g, device="cuda", dtype=torch.float64).float().double()
                    for k in ("dgamma", "dbeta", "dcol", "dcol_branch")}
        self.kdy = _keep_scale(c.dy_p, DY_SEED, c.epoch, R, D)
        self.kbr = _keep_scale(c.br_p, BR_SEED, c.epoch, R, D)


def _bwd_run(c, inp):
    tdt, R, D = _tdt(c.dtype), c.rows, c.D
    ld_dy, ld_s, ld_ds = c.lds
    o = {"ds": Out(R, D, ld_ds, tdt), "dbranch": Out(R, D, ld_ds, tdt) if c.dbranch else None}
    for k, on in (("dgamma", True), ("dbeta", True), ("dcol", c.dcol), ("dcol_branch", c.dcol_branch)):
        o[k] = _vout(D, fill=inp.pre[k]) if on else None
    t = lambda k: None if o.get(k) is None else o[k].t      # noqa: E731
    if c.epoch:
        L.seed_epoch_set(c.epoch)
    try:
        args = (inp.dy, inp.s, inp.gm, inp.mean, inp.rstd, inp.dres if c.dres else None, t("ds"), t("dgamma"), t("dbeta"), R, D,
                ld_dy, ld_s, ld_ds)
        kw = dict(dy_drop=(c.dy_p, DY_SEED), branch_drop=(c.br_p, BR_SEED), dbranch=t("dbranch"), dcol=t("dcol"),
                  dcol_branch=t("dcol_branch"))
        if c.op == "mixed":
            L.layernorm_bwd_mixed(*args, **kw)
        else:
            L.layernorm_bwd(*args, L.dtype_code(tdt), **kw)
        torch.cuda.synchronize()
    finally:
        if c.epoch:
            L.seed_epoch_set(0)
    return o


def _bwd_ref(c, inp):
    """float64: ds = rstd (g - mean(g) - xhat mean(g xhat)) (+ dres), g = dy keep sc gamma, with the given fp32 mean / rstd"""
    mu, rs = inp.mean64[:, None], inp.rstd64[:, None]
    d = inp.dy64 if inp.kdy is None else inp.dy64 * inp.kdy
    xh = (inp.s64 - mu) * rs
    g = d * inp.gm64
    o = rs * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    mag = rs * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True))
    ref = {"dgamma": ((d * xh).sum(0), (d * xh).abs().sum(0)), "dbeta": (d.sum(0), d.abs().sum(0))}
    if c.dbranch:
        br = o if inp.kbr is None else o * inp.kbr
        mbr = mag if inp.kbr is None else mag * inp.kbr
        ref["dbranch"] = (br, mbr)
        ref["dcol_branch"] = (br.sum(0), mbr.sum(0))
    ds, mds = (o + inp.dres64, mag + inp.dres64.abs()) if c.dres else (o, mag)
    ref["ds"] = (ds, mds)
    ref["dcol"] = (ds.sum(0), mds.sum(0))
    return ref


def _bwd_check(c, inp, o, ref):
    tdt, R = _tdt(c.dtype), c.rows
    fails = Fail()
    for k, b in o.items():
        if b is not None:
            assert b.untouched(), f"{c!r}: a guard element of {k} was written"
            bad = ~torch.isfinite(b.owned.float())
            assert not bool(bad.any()), f"{c!r}: {k} not written / not finite at {_first_bad(bad)}"
    for k in ("ds", "dbranch"):
        if o.get(k) is not None and R:
            r, m = ref[k]
            err = (o[k].owned.double() - r).abs()
            fails.check(c, (k, c.dtype), err / (_ulp(r, tdt) + U * m), k)
    for k in ("dgamma", "dbeta", "dcol", "dcol_branch"):
        if o.get(k) is not None:
            pre = inp.pre[k]
            r, m = ref[k] if R else (torch.zeros_like(pre), torch.zeros_like(pre))
            err = (o[k].owned[0].double() - (pre + r)).abs()
            fails.check(c, ("colsum", c.dtype), (err / (U * (pre.abs() + m)))[None], k)
    return fails


# ------------------------------------------------------------------------------------------------------
# one case
# ------------------------------------------------------------------------------------------------------
def _case_test(c):
    seed = sum(map(ord, repr(c))) * 31 + c.D
    if c.op in ("fwd", "x3"):
        inp = FwdIn(c, seed)
        o = _fwd_run(c, inp)
        fails = _fwd_check(c, inp, o)
        again = _fwd_run(c, inp)
        atomic = ()
    else:
        inp = BwdIn(c, seed)
        o = _bwd_run(c, inp)
        ref = _bwd_ref(c, inp) if c.rows else None
        fails = _bwd_check(c, inp, o, ref)
        again = _bwd_run(c, inp)
        fails += _bwd_check(c, inp, again, ref)
        atomic = ("dgamma", "dbeta", "dcol", "dcol_branch")
    for k, b in o.items():
        if b is not None and k not in atomic:
            assert torch.equal(_bits(b.flat), _bits(again[k].flat)), f"{c!r}: {k} differs bitwise between two identical runs"
    assert not fails, f"{c!r} [{cell(c)[0]}]: " + "; ".join(fails)


# ------------------------------------------------------------------------------------------------------
# the LayerNorm tests
# ------------------------------------------------------------------------------------------------------
def test_the_case_list_reaches_every_dispatch_cell():
    cells = all_cells()
    assert len(cells) == 53, sorted(cells)
    reached = {cell(c)[0] for c in CASES + VIT_CASES if c.rows > 0}
    assert not cells - reached, f"cells no case reaches: {sorted(cells - reached)}"
    # and every cell runs past two whole grid rounds, and at 1 and 7 rows
    for name in cells:
        cs = [c for c in CASES if cell(c)[0] == name]
        assert any(c.rows > 2 * cell(c)[1] for c in cs), f"{name}: no case runs two full grid rounds"
        assert {1, 7} <= {c.rows for c in cs}, f"{name}: no case at 1 and 7 rows"
    assert [cell(c)[1] for c in VIT_CASES] == [8192, 8192, 2048]


def test_the_restated_dispatch_matches_rowops_source():
    with open(os.path.join(CSRC, "rowops.hip")) as fh:
        src = " ".join(fh.read().split())
    for s in ("#define LN_MAXV 8", "#define LNB_WAVES 8",
              "if (dtype == MMRCA_BF16 && D % 8 == 0 && D <= 1536 && ld_x % 8 == 0 && ld_y % 8 == 0 && aligned16p(x) && aligned16p(y)",
              "const int g2 = (int)((rows + 7) / 8 < 1024 ? (rows + 7) / 8 : 1024);",
              "const int nv2 = (D + 511) / 512;",
              "const bool pack = sum_out || (!res && in_drop_p == 0.f);",
              "const bool drop = in_drop_p > 0.f || out_drop_p > 0.f;",
              "if (nv2 <= 1) LN_FWD16_PD(1, 2); else if (nv2 == 2) LN_FWD16_PD(2, 2); else LN_FWD16_PD(3, 1);",
              "const int grid = (int)((rows + 3) / 4 < 4096 ? (rows + 3) / 4 : 4096);",
              "const int nv = (D + 255) / 256;",
              "if (nv <= 1) LN_FWD_LAUNCH(1); else if (nv <= 2) LN_FWD_LAUNCH(2); else if (nv <= 3) LN_FWD_LAUNCH(3); "
              "else if (nv <= 4) LN_FWD_LAUNCH(4); else LN_FWD_LAUNCH(8);",
              "constexpr int ln_bwd_grid = 256;",
              "const int grid16 = (int)(want16 < ln_bwd_grid ? want16 : ln_bwd_grid);",
              "const int grid = (int)(want < 1024 ? want : 1024);",
              "const int64_t want16 = (rows + LNB_WAVES - 1) / LNB_WAVES;",
              "if (dtype == MMRCA_BF16 && D % 8 == 0 && D <= 1024 && ld_dy % 8 == 0 && ld_s % 8 == 0 && ld_ds % 8 == 0 && dgamma && dbeta",
              "if (nv2 <= 1) LN_BWD16_NV(1); else LN_BWD16_NV(2);",
              "if (nv <= 1) LN_BWD_LAUNCH(1); else if (nv <= 2) LN_BWD_LAUNCH(2); else if (nv <= 3) LN_BWD_LAUNCH(3); "
              "else if (nv <= 4) LN_BWD_LAUNCH(4); else LN_BWD_LAUNCH(8);",
              "const int grid = (int)(want < 256 ? want : 256);",
              "if (D <= 512) LN_BWDM_NV(1); else LN_BWDM_NV(2);"):
        assert s in src, f"rowops.hip no longer contains `{s}`: restate cell() for the new dispatch"


def test_the_gpu_mask_hash_equals_the_host_mirror():
    idx = np.concatenate([np.arange(5000), np.array([2 ** 31 - 1, 2 ** 32 + 7, 50432 * 768 - 1])]).astype(np.uint64)
    for seed in (0, IN_SEED, BR_SEED + EPOCH * STRIDE, 2 ** 63 + 5):
        got = uniform(seed, torch.from_numpy(idx.astype(np.int64)).cuda()).cpu().numpy()
        assert np.array_equal(got, counter_uniform(seed, idx))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_layernorm_cells_match_float64(case):
    _case_test(case)


@pytest.mark.parametrize("case", VIT_CASES, ids=repr)
def test_layernorm_at_the_vit_shape_matches_float64(case):
    _case_test(case)


def test_layernorm_rejects_bad_arguments():
    D, R = 768, 8
    bf = torch.zeros(R * 2064 + 64, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(4096, device="cuda")
    v = torch.zeros(2064, dtype=torch.bfloat16, device="cuda")
    cv = torch.zeros(2064, device="cuda")

    def fwd(D=D, ld=D, in_p=0.0, out_p=0.0):
        L.add_layernorm_fwd(bf, None, v, v, None, bf, f, f, R, D, ld, ld, 1e-6, L.BF16, in_drop=(in_p, 1), out_drop=(out_p, 2))

    def bwd(D=D, ld=D, dy_p=0.0, br_p=0.0, dbranch=None, dcol_branch=None, mixed=False, x=bf):
        if mixed:
            L.layernorm_bwd_mixed(x, f, v, f, f, None, bf, cv, cv, R, D, ld, ld, ld, dy_drop=(dy_p, 1), branch_drop=(br_p, 2),
                                  dbranch=dbranch, dcol_branch=dcol_branch)
        else:
            L.layernorm_bwd(x, bf, v, f, f, None, bf, cv, cv, R, D, ld, ld, ld, L.BF16, dy_drop=(dy_p, 1), branch_drop=(br_p, 2),
                            dbranch=dbranch, dcol_branch=dcol_branch)
    bad = [lambda: fwd(D=766), lambda: fwd(D=2052, ld=2052), lambda: fwd(ld=764), lambda: fwd(in_p=1.0), lambda: fwd(out_p=1.0),
           lambda: bwd(D=766), lambda: bwd(D=2052, ld=2052), lambda: bwd(ld=764), lambda: bwd(dy_p=1.0), lambda: bwd(br_p=1.0),
           lambda: bwd(dcol_branch=cv), lambda: bwd(mixed=True, D=772, ld=776), lambda: bwd(mixed=True, x=bf[4:]),
           lambda: bwd(mixed=True, dcol_branch=cv)]
    for call in bad:
        with pytest.raises(L.MmrcaError):
            call()
    torch.cuda.synchronize()
    assert float(bf.float().abs().max()) == 0.0 and float(f.abs().max()) == 0.0, "a rejected call wrote"


# ------------------------------------------------------------------------------------------------------
# the rest of rowops.hip
# ------------------------------------------------------------------------------------------------------
def _gelu_grad(h):
    phi = torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)
    erf = torch.erf(h / math.sqrt(2))
    return 0.5 * (1 + erf) + h * phi, 0.5 * (1 + erf.abs()) + h.abs() * phi * (2 + 0.5 * h * h)


def _colsum_ratio(got, pre, terms):
    """|got - (pre + sum terms)| / (2^-24 (|pre| + sum |terms|)), per column"""
    return (got.double() - (pre + terms.sum(0))).abs() / (U * (pre.abs() + terms.abs().sum(0)))


def _assert_bound(key, ratio, bound, what):
    w = float(ratio.max()) if ratio.numel() else 0.0
    _note(key, w)
    assert w <= bound, f"{what}: error {w:.3g} > {bound} units at {_first_bad(~(ratio <= bound))}"


# bound units: ulp_T(|ref|) + 2^-24 * size of the terms (elementwise) / 2^-24 * (|prefill| + sum |terms|) (sums)
MISC_BOUND = {"gelu": 5.0,         # observed 1.21
              "colsum": 140.0,     # observed 27-34.7 (1.1 M rows: long per-thread sums)
              "embed": 24.0,       # observed 4.95-5.31 (atomic order varies)
              "assemble": 12.0,    # observed 2.89
              "xent_loss": 5.0,    # observed 1.05
              "xent_grad": 150.0,  # observed 37 (C = 1000: the fp32 sum of the exponentials)
              "optim": 15.0}       # observed 3.69


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gelu_bwd_past_one_grid_round_matches_float64(dt):
    tdt = _tdt(dt)
    n = 2 * 8192 * 256 * 4 + 4 * 37
    g = torch.Generator(device="cuda").manual_seed(5)
    h = (3 * torch.randn(n, generator=g, device="cuda")).to(tdt)
    dg = torch.randn(n, generator=g, device="cuda").to(tdt)
    dh = _vout(n, tdt)
    L.gelu_bwd(dg, h, dh.t, n, L.dtype_code(tdt))
    torch.cuda.synchronize()
    assert dh.untouched() and bool(torch.isfinite(dh.owned.float()).all())
    gg, gm = _gelu_grad(h.double())
    ref = dg.double() * gg
    _assert_bound("gelu", (dh.owned[0].double() - ref).abs() / (_ulp(ref, tdt) + U * dg.double().abs() * gm), MISC_BOUND["gelu"], "dH")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,N,ld", [(1003, 1028, 1036), (600003, 36, 40), (7, 4, 4)])
def test_gelu_bwd_colsum_sums_the_stored_values(dt, M, N, ld):
    """M % 4 != 0 (the four-row loop's tail), ld > N, rows_per_block doubling (600,003 rows), accumulation onto a nonzero db; the
    column sums are those of the stored (rounded) dH"""
    tdt = _tdt(dt)
    g = torch.Generator(device="cuda").manual_seed(M + N)
    h, h64 = _operand(3 * torch.randn(M, N, generator=g, device="cuda", dtype=torch.float64), ld, tdt, g)
    dg, dg64 = _operand(torch.randn(M, N, generator=g, device="cuda", dtype=torch.float64), ld, tdt, g)
    pre = 8.0 * torch.randn(N, generator=g, device="cuda", dtype=torch.float64).float().double()
    dh, db = Out(M, N, ld, tdt), _vout(N, fill=pre)
    L.gelu_bwd_colsum(dg, h, dh.t, db.t, M, N, ld, L.dtype_code(tdt))
    torch.cuda.synchronize()
    assert dh.untouched() and db.untouched() and bool(torch.isfinite(dh.owned.float()).all())
    gg, gm = _gelu_grad(h64)
    ref = dg64 * gg
    _assert_bound("gelu", (dh.owned.double() - ref).abs() / (_ulp(ref, tdt) + U * dg64.abs() * gm), MISC_BOUND["gelu"], "dH")
    _assert_bound("colsum", _colsum_ratio(db.owned[0], pre, dh.owned.double()), MISC_BOUND["colsum"], "db")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,N,ld", [(5, 260, 268), (13, 1028, 1028), (1100003, 36, 40)])
def test_colsum_accum_matches_float64(dt, M, N, ld):
    """M < 16 (no four-row iteration), N % 256 != 0, ld > N, rows_per_block doubling (1,100,003 rows)"""
    tdt = _tdt(dt)
    g = torch.Generator(device="cuda").manual_seed(M * 3 + N)
    dy, dy64 = _operand(torch.randn(M, N, generator=g, device="cuda", dtype=torch.float64) + 2.0, ld, tdt, g)
    pre = 8.0 * torch.randn(N, generator=g, device="cuda", dtype=torch.float64).float().double()
    db = _vout(N, fill=pre)
    L.colsum_accum(dy, db.t, M, N, ld, L.dtype_code(tdt))
    torch.cuda.synchronize()
    assert db.untouched()
    _assert_bound("colsum", _colsum_ratio(db.owned[0], pre, dy64), MISC_BOUND["colsum"], "db")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("D,rows", [(768, 4100), (1280, 37), (1280, 2 * 16384 + 5)])
def test_embed_fwd_bwd_match_float64(dt, D, rows):
    """embed_bwd_acc_k (D <= 1024, rows past its 1,024-row grid round) and embed_bwd_k (D > 1024, rows past its 16,384); word and
    position padding rows; position ids that change inside a wave's rows; all-zero gradient rows; nonzero prefills"""
    tdt = _tdt(dt)
    V, Pn = 1000, 66
    g = torch.Generator(device="cuda").manual_seed(D + rows)
    word, pos, typ = (torch.randn(n, D, generator=g, device="cuda").to(tdt) for n in (V, Pn, 1))
    ids = torch.randint(0, V, (rows,), generator=g, device="cuda", dtype=torch.int32)
    ids[::5] = 7
    pid = (torch.arange(rows, device="cuda") % 64).int()
    pid[rows // 2:] = torch.randint(0, Pn, (rows - rows // 2,), generator=g, device="cuda", dtype=torch.int32)
    out = Out(rows, D, D, tdt)
    L.embed_fwd(ids, pid, word, pos, typ[0], out.t, rows, D, L.dtype_code(tdt))
    torch.cuda.synchronize()
    ref = ((word.float()[ids.long()] + pos.float()[pid.long()]) + typ.float()).to(tdt)
    assert out.untouched() and torch.equal(_bits(out.owned), _bits(ref)), "embed_fwd differs from the fp32 host sum"
    dout = torch.randn(rows, D, generator=g, device="cuda").to(tdt)
    dout[3::7] = 0
    d64 = dout.double()
    pre = {k: (4.0 * torch.randn(n * D, generator=g, device="cuda")).double() for k, n in (("w", V), ("p", Pn), ("t", 1))}
    for with_all in (True, False):
        dw, dp, dty = (_vout(n * D, fill=pre[k]) for k, n in (("w", V), ("p", Pn), ("t", 1)))
        L.embed_bwd(dout, ids, pid, dw.t, dp.t if with_all else None, dty.t if with_all else None, rows, D, L.dtype_code(tdt),
                    pad_id=7, pos_pad_id=1)
        torch.cuda.synchronize()
        assert dw.untouched() and dp.untouched() and dty.untouched()
        keep_w = (ids != 7).double()[:, None]
        tw = torch.zeros(V, D, device="cuda", dtype=torch.float64).index_add_(0, ids.long(), d64 * keep_w)
        mw = torch.zeros(V, D, device="cuda", dtype=torch.float64).index_add_(0, ids.long(), d64.abs() * keep_w)
        gw = dw.owned.view(V, D).double()
        assert torch.equal(gw[7], pre["w"].view(V, D)[7]), "the word padding row took a gradient"
        pw = pre["w"].view(V, D)
        _assert_bound("embed", (gw - pw - tw).abs() / (U * (pw.abs() + mw)), MISC_BOUND["embed"], "dword")
        if with_all:
            keep_p = (pid != 1).double()[:, None]
            tp = torch.zeros(Pn, D, device="cuda", dtype=torch.float64).index_add_(0, pid.long(), d64 * keep_p)
            mp = torch.zeros(Pn, D, device="cuda", dtype=torch.float64).index_add_(0, pid.long(), d64.abs() * keep_p)
            gp, pp = dp.owned.view(Pn, D).double(), pre["p"].view(Pn, D)
            assert torch.equal(gp[1], pp[1]), "the position padding row took a gradient"
            _assert_bound("embed", (gp - pp - tp).abs() / (U * (pp.abs() + mp)), MISC_BOUND["embed"], "dpos")
            _assert_bound("embed", _colsum_ratio(dty.owned[0], pre["t"], d64), MISC_BOUND["embed"], "dtype_row")
        else:
            assert torch.equal(dp.owned[0].double(), pre["p"]) and torch.equal(dty.owned[0].double(), pre["t"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,C,H,W,P", [(2, 3, 224, 224, 14), (3, 3, 28, 42, 14), (2, 3, 64, 96, 16)])
def test_patchify_is_the_host_gather(dt, B, C, H, W, P):
    """P = 14: patchify_any_k (BLIP-2's ViT-g), P = 16: the four-wide kernel; bit-equal to the host gather and cast"""
    tdt = _tdt(dt)
    img = torch.randn(B, C, H, W, device="cuda") * 3
    n = B * (H // P) * (W // P)
    out = Out(n, C * P * P, C * P * P, tdt)
    L.patchify_fwd(img, out.t, B, C, H, W, P, L.dtype_code(tdt))
    torch.cuda.synchronize()
    ref = img.view(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(n, C * P * P).to(tdt)
    assert out.untouched() and torch.equal(_bits(out.owned), _bits(ref))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 11])
def test_vit_assemble_fwd_bwd(dt, B):
    """B % 8 != 0 (the eight-sample loop's tail); dcls and dpos accumulate onto nonzero values; dproj is an exact copy"""
    tdt, nP, D = _tdt(dt), 196, 768
    Tn = nP + 1
    g = torch.Generator(device="cuda").manual_seed(B)
    proj, cls, pos = (torch.randn(n, D, generator=g, device="cuda").to(tdt) for n in (B * nP, 1, Tn))
    x = Out(B * Tn, D, D, tdt)
    L.vit_assemble_fwd(proj, cls[0], pos, x.t, B, nP, D, L.dtype_code(tdt))
    torch.cuda.synchronize()
    ref = (torch.cat([cls.float().expand(B, 1, D), proj.float().view(B, nP, D)], 1) + pos.float()).to(tdt).view(B * Tn, D)
    assert x.untouched() and torch.equal(_bits(x.owned), _bits(ref))
    dx = torch.randn(B * Tn, D, generator=g, device="cuda").to(tdt)
    pc, pp = ((4.0 * torch.randn(n, generator=g, device="cuda")).double() for n in (D, Tn * D))
    dproj, dcls, dpos = Out(B * nP, D, D, tdt), _vout(D, fill=pc), _vout(Tn * D, fill=pp)
    L.vit_assemble_bwd(dx, dproj.t, dcls.t, dpos.t, B, nP, D, L.dtype_code(tdt))
    torch.cuda.synchronize()
    assert dproj.untouched() and dcls.untouched() and dpos.untouched()
    d3 = dx.view(B, Tn, D)
    assert torch.equal(_bits(dproj.owned), _bits(d3[:, 1:].reshape(B * nP, D)))
    d64 = d3.double()
    _assert_bound("assemble", _colsum_ratio(dcls.owned[0], pc, d64[:, 0]), MISC_BOUND["assemble"], "dcls")
    _assert_bound("assemble", _colsum_ratio(dpos.owned[0], pp, d64.reshape(B, Tn * D)), MISC_BOUND["assemble"], "dpos")


def _xent_ref(z, y, w, eps, gs):
    """float64 CrossEntropyLoss(weight, label_smoothing) (mean over sum_i w[y_i]) and its gradient, with the size of their terms"""
    B, C = z.shape
    m = z.amax(1, keepdim=True)
    lse = m + torch.log(torch.exp(z - m).sum(1, keepdim=True))
    p = torch.exp(z - lse)
    wv = torch.ones(C, dtype=torch.float64, device=z.device) if w is None else w
    wy = wv[y][:, None]
    den = float(wy.sum())
    num = (1 - eps) * wy[:, 0] * (lse[:, 0] - z[torch.arange(B), y]) + eps / C * (wv * (lse - z)).sum(1)
    nmag = (1 - eps) * wy[:, 0] * (lse.abs()[:, 0] + z[torch.arange(B), y].abs() + 1) + eps / C * (wv * (lse.abs() + z.abs() + 1)).sum(1)
    onehot = torch.nn.functional.one_hot(y, C).double()
    gr = ((1 - eps) * wy * (p - onehot) + eps / C * (wv.sum() * p - wv)) / den * gs
    gmag = ((1 - eps) * wy * (p + onehot) + eps / C * (wv.sum() * p + wv)) / den * abs(gs)
    return float(num.sum()) / den, float(nmag.sum()) / den, gr, gmag


@pytest.mark.parametrize("C", [1, 4, 1000])
@pytest.mark.parametrize("weighted,eps,gs", [(False, 0.0, 1.0), (True, 0.1, 0.25), (True, 0.0, 3.0), (False, 0.1, 1.0)])
def test_xent_matches_float64(C, weighted, eps, gs):
    """B = 300 (past one 256-thread pass); logits of +-80 and +-100 (exp without the max subtraction overflows fp32 at 88.7);
    loss or dlogits passed alone"""
    B = 300
    g = torch.Generator(device="cuda").manual_seed(C + int(100 * eps))
    z = torch.randn(B, C, generator=g, device="cuda") * 2
    z[::3] = 80 * torch.randn(B, C, generator=g, device="cuda")[::3].sign()
    z[1::3] = 100 * torch.randn(B, C, generator=g, device="cuda")[1::3].sign() + torch.randn(B, C, generator=g, device="cuda")[1::3]
    y = torch.randint(0, C, (B,), generator=g, device="cuda")
    w = (0.25 + 2 * torch.rand(C, generator=g, device="cuda")) if weighted else None
    lref, lmag, gref, gmag = _xent_ref(z.double(), y, None if w is None else w.double(), float(np.float32(eps)), gs)
    for want_loss, want_grad in ((True, True), (True, False), (False, True)):
        loss, dz = _vout(1), Out(B, C, C, torch.float32)
        L.xent_fwd_bwd(z, y.int(), w, eps, loss.t if want_loss else None, dz.t if want_grad else None, B, C, gs)
        torch.cuda.synchronize()
        if want_loss:
            assert loss.untouched()
            _assert_bound("xent_loss", torch.tensor([abs(float(loss.owned[0, 0]) - lref) / (U * lmag)]), MISC_BOUND["xent_loss"], "loss")
        else:
            assert torch.isnan(loss.owned).all() and loss.untouched()
        if want_grad:
            assert dz.untouched() and bool(torch.isfinite(dz.owned).all())
            _assert_bound("xent_grad", (dz.owned.double() - gref).abs() / (U * gmag + 2.0 ** -140), MISC_BOUND["xent_grad"], "dlogits")
        else:
            assert bool(torch.isnan(dz.owned).all()) and dz.untouched()


N_OPT = 8192 * 256 * 4 + 4 * 1001          # past one grid round of the elementwise kernels


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("planes", ["none", "hi", "hi+lo"])
def test_optimizers_match_float64_and_refresh_the_bf16_planes(kind, planes):
    """three steps on an arena longer than one grid round, grad_scale != 1; each step against the float64 statement of the kernel's
    update from the state it was given; lp == bf16(p) and lp_lo == bf16(p - bf16(p)) bitwise"""
    n = N_OPT
    g = torch.Generator(device="cuda").manual_seed(len(kind) * 7 + len(planes))
    p = _vout(n, fill=torch.randn(n, generator=g, device="cuda"))
    m, v = _vout(n, fill=torch.zeros(n, device="cuda")), _vout(n, fill=torch.zeros(n, device="cuda"))
    lp = _vout(n, torch.bfloat16) if planes != "none" else None
    lo = _vout(n, torch.bfloat16) if planes == "hi+lo" else None
    lr, wd, b1, b2, eps, gs = (float(np.float32(a)) for a in (0.01, 0.05, 0.9, 0.999, 1e-8, 0.5))   # what the kernel is given
    for step in range(1, 4):
        grad = torch.randn(n, generator=g, device="cuda") * step
        grad[::97] = 0
        p0, m0, v0, g0 = (t.double() for t in (p.owned[0], m.owned[0], v.owned[0], grad))
        if kind == "sgd":
            L.sgd_step(p.t, grad, None if lp is None else lp.t, n, lr, wd, grad_scale=gs, lp_lo=None if lo is None else lo.t)
            gg = g0 * gs
            pr = p0 - lr * (gg + wd * p0)
            units = {"p": U * (p0.abs() + lr * (gg.abs() + wd * p0.abs()))}
            refs = {"p": pr}
        else:
            L.adamw_step(p.t, grad, m.t, v.t, None if lp is None else lp.t, n, lr, b1, b2, eps, wd, step, grad_scale=gs,
                         lp_lo=None if lo is None else lo.t)
            gg = g0 * gs
            # the bias corrections as the host computes them: 1.f - powf(beta, step) in fp32 (powf within an ulp)
            bc1, bc2 = (float(np.float32(1) - np.power(np.float32(b), np.float32(step))) for b in (b1, b2))
            mr = b1 * m0 + (1 - b1) * gg
            vr = b2 * v0 + (1 - b2) * gg * gg
            den = vr.sqrt() / math.sqrt(bc2) + eps
            upd = lr / bc1 * mr / den
            pr = p0 * (1 - lr * wd) - upd
            refs = {"p": pr, "m": mr, "v": vr}
            ubc = 2 * U * (b1 ** step / bc1 + 0.5 * b2 ** step / bc2)       # one ulp of powf in either correction
            units = {"p": U * (p0.abs() + upd.abs() * 8) + ubc * upd.abs(), "m": U * (b1 * m0.abs() + (1 - b1) * gg.abs()),
                     "v": U * (b2 * v0 + (1 - b2) * gg * gg * 3)}
        torch.cuda.synchronize()
        outs = {"p": p, "m": m, "v": v}
        for k, r in refs.items():
            assert outs[k].untouched()
            _assert_bound("optim", (outs[k].owned[0].double() - r).abs() / (units[k] + 2.0 ** -149), MISC_BOUND["optim"],
                          f"{kind} step {step} {k}")
        pk = p.owned[0]
        if lp is not None:
            assert lp.untouched() and torch.equal(_bits(lp.owned[0]), _bits(pk.bfloat16())), f"step {step}: lp != bf16(p)"
        if lo is not None:
            want = (pk - pk.bfloat16().float()).bfloat16()
            assert lo.untouched() and torch.equal(_bits(lo.owned[0]), _bits(want)), f"step {step}: lp_lo != bf16(p - bf16(p))"


def _special_f32(n, g):
    """random values, exact ties (both parities), one off a tie, denormals, +-0, +-inf, NaN, the largest finite floats"""
    r = torch.randint(0, 2 ** 32, (n,), generator=g, dtype=torch.int64).numpy().astype(np.uint32)
    k = np.arange(n) % 8
    b = r.copy()
    b[k == 1] = (r[k == 1] & 0xFFFF0000) | 0x8000                       # exact ties
    b[k == 2] = (r[k == 2] & 0xFFFF0000) | 0x7FFF                       # just below a tie
    b[k == 3] = (r[k == 3] & 0xFFFF0000) | 0x8001                       # just above a tie
    b[k == 4] = r[k == 4] & 0x807FFFFF                                  # denormals
    b[k == 5] = (r[k == 5] & 0x807F0000) | 0x8000                       # denormal ties
    sp = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0, 0x80000000, 1,
                   0x80008000, 0x00018000, 0x3F808000, 0x3F818000], dtype=np.uint32)
    b[6:6 + 8 * sp.size:8] = sp
    return b


def _rne_bf16(bits):
    """round-to-nearest-even float32 -> bf16 on the bit patterns (no flush of denormals); NaN stays NaN"""
    b = bits.astype(np.uint64)
    out = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = ((bits & 0x7F800000) == 0x7F800000) & ((bits & 0x7FFFFF) != 0)
    out[nan] = 0x7FC0
    return out


def _same_bf16(got, want):
    """bitwise (numpy uint16 patterns), NaN matching any NaN"""
    nan_g = ((got & 0x7F80) == 0x7F80) & ((got & 0x7F) != 0)
    nan_w = ((want & 0x7F80) == 0x7F80) & ((want & 0x7F) != 0)
    bad = (nan_g != nan_w) | (~nan_w & (got != want))
    return not bad.any(), np.nonzero(bad)[0][:4]


def test_cast_and_split_round_to_nearest_even_bitwise():
    n = 8192 * 256 * 4 + 4 * 257                                        # past one grid round
    g = torch.Generator().manual_seed(17)
    bits = _special_f32(n, g)
    hi_ref = _rne_bf16(bits)
    x_np = bits.view(np.float32)
    hi_f = (hi_ref.astype(np.uint32) << 16).view(np.float32)
    with np.errstate(invalid="ignore"):
        lo_ref = _rne_bf16((x_np - hi_f).astype(np.float32).view(np.uint32))   # exact in fp32 (inf - inf = NaN, as on the GPU)
    x = torch.from_numpy(x_np.copy()).cuda()
    d, hi, lo = _vout(n, torch.bfloat16), _vout(n, torch.bfloat16), _vout(n, torch.bfloat16)
    L.cast_f32_to_bf16(x, d.t, n)
    L.split_f32(x, hi.t, lo.t, n)
    torch.cuda.synchronize()
    assert d.untouched() and hi.untouched() and lo.untouched()
    for name, o, want in (("cast_f32_to_bf16", d, hi_ref), ("split_f32 hi", hi, hi_ref), ("split_f32 lo", lo, lo_ref)):
        got = o.owned[0].cpu().view(torch.int16).numpy().view(np.uint16)
        ok, where = _same_bf16(got, want)
        assert ok, f"{name} differs from round-to-nearest-even at {where.tolist()}: x bits {[hex(int(bits[i])) for i in where]}"


@pytest.mark.parametrize("epoch", [0, EPOCH])
def test_sd_rowscale_is_the_counter_hash_bitwise(epoch):
    n, B = 40, 13
    p = torch.tensor([0.0, 0.1, 0.5, 0.9, 0.25] * 8, device="cuda")
    out = _vout(n * B)
    if epoch:
        L.seed_epoch_set(epoch)
    try:
        L.sd_rowscale(p, out.t, n, B, 99)
        torch.cuda.synchronize()
    finally:
        if epoch:
            L.seed_epoch_set(0)
    u = torch.from_numpy(counter_uniform(99 + epoch * STRIDE, np.arange(n * B, dtype=np.uint64))).cuda().view(n, B)
    pc = p.cpu().numpy()
    sc = torch.from_numpy(np.float32(1.0) / (np.float32(1.0) - pc)).cuda()[:, None]
    ref = torch.where(u >= p[:, None], sc.expand(n, B), torch.zeros((), device="cuda"))
    assert out.untouched()
    assert torch.equal(_bits(out.owned.view(n, B)), _bits(ref))
    assert bool((out.owned.view(n, B)[0] == 1.0).all()), "p = 0 must give exactly 1.0"
