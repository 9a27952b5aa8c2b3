"""Every dispatch cell of the fused MM-RCA head (csrc/head.hip: head_fwd_k, head_bwd_k in both dtypes, the four proj_self
instantiations with full and ragged 16-chunks, head_wgrad_k over one, two and three K splits with full and ragged 64-wide k blocks, the
classifier-gradient chunks) against the float64 statement of tests/head_ref.py on the kernel's exact inputs, element by element.
Needs an MI355X; every call goes through the C ABI (L.head_fwd / L.head_bwd).

Inputs (head_ref.case_inputs): feature rows with a common offset of four times their spread, one sample scaled by 1e3 and one by
1e-3, LayerNorm gains and biases of mixed sign, dlogits of mixed sign with one all-zero row.  Logits, dimg and dtxt start as NaN with
sentinel guards behind them; all 34 gradient tensors start from a nonzero seeded pattern (the kernel accumulates: the check is on
got - prefill) with sentinel guards between them; the workspace is exactly head_bwd_workspace_bytes long, NaN inside, a sentinel
guard behind.  Every case runs twice: what has no atomics (logits, dimg, dtxt) or one atomic per address (Q/K/V weight and bias
gradients when there is one K split) must repeat bitwise, the rest within its bound.

Bounds are elementwise in the units of head_ref.ratios (U = 2^-24; never relative to a cancelling sum -- the key-bias gradients are
exactly zero mathematically and are bounded by the sum of their |terms|).  BOUND holds one K per (output kind, dtype), each >= 4x
the worst value observed over the case list, with the float32-on-the-CPU figure of the same graph
(head_ref.CPU_F32_OBSERVED) beside it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import lib as L          # noqa: E402
from tests import head_ref as R                               # noqa: E402

SENT = -3072.0                 # guard sentinel (exact in bf16)
LOUD = 8192.0                  # what stands in the input slack the kernel must not read
GUARD = 8                      # guard elements behind every vector, guard rows behind every matrix
PRE_SEED = 77
WS_GUARD = 256                 # bytes

# K per (output kind, dtype); observed worst over the case list | float32 on the CPU (head_ref.CPU_F32_OBSERVED)
BOUND = {
    ("logits", "f32"): 4.0,       # observed 0.88 | 1.92
    ("logits", "bf16"): 4.0,      # observed 0.72 | 1.92
    ("dx", "f32"): 1300.0,        # observed 269 | 337 (the error of dy itself: the softmax and LayerNorm backwards cancel)
    ("dx", "bf16"): 120.0,        # observed 24.7 | 337 (the unit holds half a bf16 ulp as well)
    ("w_qkv", "f32"): 2400.0,     # observed 477 | 2.9e5
    ("w_qkv", "bf16"): 4000.0,    # observed 797 | 2.9e5
    ("b_qkv", "f32"): 2200.0,     # observed 432 | 5.45e3
    ("b_qkv", "bf16"): 3600.0,    # observed 717 | 5.45e3
    ("ln", "f32"): 3000.0,        # observed 605 | 1.32e3
    ("ln", "bf16"): 5600.0,       # observed 1148 | 1.32e3
    ("fin_w", "f32"): 6800.0,     # observed 1358 | 2.34e3 (columns whose ReLU is almost always shut)
    ("fin_w", "bf16"): 5400.0,    # observed 1063 | 2.34e3
    ("fin_b", "f32"): 12.0,       # observed 1.57-1.77 | 1.0 (one atomic per sample: the order, and with it the figure, varies)
    ("fin_b", "bf16"): 12.0,      # observed 1.52-1.81 | 1.0
}
OBSERVED = {}
QKV = [f"{b}_{l}" for b in R.BLOCKS for l in ("wq", "bq", "wk", "bk", "wv", "bv")]
ATTENTION = [f for f in R.FIELDS if f not in ("fin_w", "fin_b")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need a GPU"
    L.load()
    L.seed_epoch_set(0)            # test_graph_gpu.py moves the mask epoch
    torch.cuda.synchronize()
    yield
    print("\nhead cells: worst observed error / bound unit")
    for k in sorted(OBSERVED):
        print(f"  {k}: {OBSERVED[k]:.3g}  (bound {BOUND[k]}, float32 on the CPU {R.CPU_F32_OBSERVED.get(k[0])})")


# ------------------------------------------------------------------------------------------------------
# buffers
# ------------------------------------------------------------------------------------------------------
class Pack:
    """the 34 tensors of a HeadPtrs in one flat fp32 buffer, `gap` in the GUARD elements behind each"""

    def __init__(self, tensors, gap):
        self.off, n = {}, 0
        for f in R.FIELDS:
            self.off[f] = (n, tuple(tensors[f].shape))
            n += (tensors[f].numel() + 3) // 4 * 4 + GUARD
        host = torch.full((n,), gap, dtype=torch.float32)
        for f in R.FIELDS:
            o, shape = self.off[f]
            host[o:o + tensors[f].numel()] = tensors[f].reshape(-1)
        self.host0 = host
        self.flat = host.cuda()
        self.ptrs = L.HeadPtrs()
        for f in R.FIELDS:
            setattr(self.ptrs, f, self.flat.data_ptr() + 4 * self.off[f][0])

    def split(self, flat):
        """({field: tensor}, gaps intact) of a host copy of the buffer"""
        out, mask = {}, torch.ones(flat.numel(), dtype=torch.bool)
        for f in R.FIELDS:
            o, shape = self.off[f]
            n = int(np.prod(shape))
            out[f] = flat[o:o + n].view(shape)
            mask[o:o + n] = False
        return out, torch.equal(flat[mask], self.host0[mask])


class Rows:
    """an output [rows, D] of dtype t: NaN inside, GUARD sentinel rows behind"""

    def __init__(self, rows, D, t):
        self.rows, self.D = rows, D
        self.flat = torch.full(((rows + GUARD) * D,), SENT, dtype=t, device="cuda")
        self.flat[:rows * D] = float("nan")

    def host(self):
        h = self.flat.cpu()
        assert bool((h[self.rows * self.D:] == SENT).all()), "a guard element was written"
        return h[:self.rows * self.D].view(self.rows, self.D)


def _feature(x):
    """[B, d] features on the GPU with GUARD loud rows behind"""
    flat = torch.full(((x.shape[0] + GUARD) * x.shape[1],), LOUD, dtype=x.dtype)
    flat[:x.numel()] = x.reshape(-1)
    return flat.cuda()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Inputs:
    def __init__(self, c):
        self.c = c
        self.w = R.case_weights(c)
        self.img, self.txt, self.dl = R.case_inputs(c)
        self.W = Pack(self.w, LOUD)
        self.imgd, self.txtd, self.dld = _feature(self.img), _feature(self.txt), _feature(self.dl)
        self.wide = (_feature(self.img.float()), _feature(self.txt.float())) if c.dtype == "bf16" else None
        g = torch.Generator().manual_seed(PRE_SEED)
        self.pre = {f: 2.0 ** -6 * torch.randn(self.w[f].shape, generator=g) for f in R.FIELDS}
        self.ref = R.head_ref(self.w, self.img.double(), self.txt.double(), c.mode, c.reverse, c.n_classes, keep=R.case_keep(c),
                              drop_p=c.drop_p, dlogits=self.dl.double())
        self.terms = R.term_sums(self.ref)
        self.code = L.dtype_code(R.tdt(c.dtype))


class Epoch:
    def __init__(self, e):
        self.e = e

    def __enter__(self):
        if self.e:
            L.seed_epoch_set(self.e)

    def __exit__(self, *a):
        if self.e:
            torch.cuda.synchronize()
            L.seed_epoch_set(0)


def _fwd(i, W=None):
    c = i.c
    out = Rows(1, c.B * c.n_classes, torch.float32)
    with Epoch(c.epoch):
        L.head_fwd(i.imgd, i.txtd, (W or i.W).ptrs, out.flat, c.B, c.d_img, c.d_txt, c.n_classes, c.reverse, c.mode, c.drop_p, c.seed, i.code)
    return out.host().view(c.B, c.n_classes)


def _bwd(i, dimg=True, dtxt=True, wide=False):
    """one backward on fresh prefills: {field: got, 'dimg', 'dtxt'} on the host (gradients WITH their prefill); wide: the fp32
    instantiation on the bf16 case's features widened to fp32"""
    c = i.c
    t = torch.float32 if wide else R.tdt(c.dtype)
    imgd, txtd, code = (*i.wide, L.F32) if wide else (i.imgd, i.txtd, i.code)
    G = Pack(i.pre, SENT)
    di, dt = (Rows(c.B, c.d_img, t) if dimg else None), (Rows(c.B, c.d_txt, t) if dtxt else None)
    need = L.head_bwd_workspace_bytes(c.B, c.d_img, c.d_txt)
    ws = torch.full((need + WS_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")       # NaN inside
    ws[need:] = 0xA5
    with Epoch(c.epoch):
        L.head_bwd(i.dld, imgd, txtd, i.W.ptrs, G.ptrs, di and di.flat, dt and dt.flat, c.B, c.d_img, c.d_txt, c.n_classes,
                   c.reverse, c.mode, c.drop_p, c.seed, code, workspace=ws[:need])
    got, intact = G.split(G.flat.cpu())
    assert intact, f"{c!r}: a guard element between the gradient tensors was written"
    assert bool((ws[need:] == 0xA5).all()), f"{c!r}: the backward wrote past head_bwd_workspace_bytes"
    got["dimg"], got["dtxt"] = (di.host() if dimg else None), (dt.host() if dtxt else None)
    return got


def _judge(i, got, fails, tag=""):
    """every output of `got` against the float64 reference, elementwise, in bound units"""
    c, cell = i.c, i.c.cell
    net = {}
    for k, v in got.items():
        if v is None:
            continue
        bad = ~torch.isfinite(v.float())
        assert not bool(bad.any()), f"{c!r}{tag}: {k} not written / not finite at {tuple(int(j) for j in torch.nonzero(bad)[0])}"
        net[k] = v.double() - i.pre[k].double() if k in i.pre else v.double()
    for k, ratio in R.ratios(c, net, i.ref, i.terms, prefill=i.pre).items():
        key = (R.kind_of(k), c.dtype)
        worst = float(ratio.max())
        OBSERVED[key] = max(OBSERVED.get(key, 0.0), worst)
        if not worst <= BOUND[key]:
            idx = tuple(int(j) for j in torch.nonzero(~(ratio <= BOUND[key]))[0])
            fails.append(f"{k}{tag}: error {worst:.3g} > {BOUND[key]} units, first at {idx} [{R.locate(c, cell, k, idx)}]")


def _same(a, b, keys, what, fails):
    for k in keys:
        if a[k] is not None and b[k] is not None and not torch.equal(_bits(a[k]), _bits(b[k])):
            fails.append(f"{k}: {what}")


# ------------------------------------------------------------------------------------------------------
# the cells
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_head_cells_match_float64(case):
    c = case
    i = Inputs(c)
    if c.mode != 1:
        for name, b in i.ref.blk.items():
            pos = float((b.y.detach() > 0).double().mean())
            assert 0.2 < pos < 0.8, f"{c!r}: block {name} has {pos:.2f} of its ReLU inputs positive"
    fails = []
    # forward
    lg = _fwd(i)
    _judge(i, {"logits": lg}, fails)
    if not torch.equal(_bits(lg), _bits(_fwd(i))):
        fails.append("logits differ bitwise between two identical runs")
    # backward, twice on fresh prefills
    a = _bwd(i)
    _judge(i, a, fails)
    b = _bwd(i)
    _judge(i, b, fails, " (second run)")
    once = ["dimg", "dtxt"] + (QKV if c.cell["ksplit"] == 1 else [])
    _same(a, b, once, "differs bitwise between two identical runs", fails)
    if c.dtype == "bf16":
        # the bf16 instantiation differs from the fp32 one in its loads and its final conversion only: its dimg / dtxt are the fp32
        # kernel's values on the same (widened) features rounded to nearest -- half a bf16 ulp, and four fp32 ulps for a product
        # that one instantiation fuses into an FMA and the other does not
        w = _bwd(i, wide=True)
        for k in ("dimg", "dtxt"):
            f32 = w[k].double()
            off = (a[k].double() - f32).abs() / (0.5 * R.ulp(f32, "bf16") + 4.0 * R.ulp(f32, "f32"))
            if not float(off.max()) <= 1.0:
                idx = tuple(int(j) for j in torch.nonzero(~(off <= 1.0))[0])
                fails.append(f"{k}: {float(off.max()):.3g} x half a bf16 ulp from the fp32 kernel's value at {idx}: not rounded to nearest "
                             f"[{R.locate(c, c.cell, k, idx)}]")
    if c.mode == 1:
        for f in ATTENTION:
            if not torch.equal(_bits(a[f]), _bits(i.pre[f])):
                fails.append(f"{f}: features_only changed an attention gradient")
    if c.nulls:
        for di, dt in ((False, True), (True, False), (False, False)):
            n = _bwd(i, di, dt)
            tag = f" (dimg={'set' if di else 'None'}, dtxt={'set' if dt else 'None'})"
            _judge(i, n, fails, tag)
            _same(a, n, once, "changes when the other input gradient is not asked for" + tag, fails)
    assert not fails, f"{c!r} {c.cell}:\n  " + "\n  ".join(fails)


def test_every_bound_is_at_least_four_times_what_was_observed():
    """runs after the cases (collection order inside a file is kept) and judges what they observed"""
    for k, v in OBSERVED.items():
        assert BOUND[k] >= 4.0 * v, f"{k}: bound {BOUND[k]} < 4 x observed {v:.3g}"


# ------------------------------------------------------------------------------------------------------
# the mask, bit by bit
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,widths,p,epoch", [(0, (832, 1088), 0.6, R.EPOCH), (1, (64, 64), 0.1, 0), (1, (1280, 768), 0.6, 0),
                                                 (2, (1280, 768), 0.1, 0)])
def test_single_mask_bits_show_in_the_logits(mode, widths, p, epoch):
    """fin_w = the indicator of one column per class, fin_b = 0: logit [b][k] is v[b][col_k] keep / (1 - p), so a dropped column is an
    exact zero and a kept one is not: 16 mask bits per sample per launch, at the first and last active column and 14 between"""
    c = R.Case(17, *widths, mode, True, "f32", n_classes=16, drop_p=p, epoch=epoch)
    i = Inputs(c)
    keep = R.case_keep(c)
    v = i.ref.cat.detach()                                   # before the mask
    live = torch.nonzero(v.abs().min(0).values > 1e-3).flatten()      # columns no sample has a ReLU zero in
    assert live.numel() >= 64
    rng = np.random.default_rng(5)
    for rnd in range(2):
        cols = torch.cat((live[:1], live[torch.from_numpy(np.sort(rng.choice(live.numel() - 2, 14, replace=False)) + 1)], live[-1:]))
        w = dict(i.w)
        w["fin_w"] = torch.zeros_like(i.w["fin_w"])
        w["fin_w"][torch.arange(16), cols] = 1.0
        w["fin_b"] = torch.zeros(16)
        lg = _fwd(i, Pack(w, LOUD))
        k = keep[:, cols]
        assert 0 < int(k.sum()) < k.numel()
        assert torch.equal(lg != 0, k), f"mode {mode}: the kernel's mask differs from sample * wact + column at {torch.nonzero((lg != 0) != k)[:4].tolist()}"
        want = v[:, cols] * k / (1.0 - float(np.float32(p)))
        assert float(((lg.double() - want).abs() / (want.abs() + 1e-30))[k].max()) < 1e-3


# ------------------------------------------------------------------------------------------------------
# arguments and the LDS boundary
# ------------------------------------------------------------------------------------------------------
def test_head_rejects_bad_arguments_without_launching():
    c = R.Case(4, 832, 1088, 0, True, "f32")
    i = Inputs(c)
    G = Pack(i.pre, SENT)
    lg = Rows(1, 4 * 16, torch.float32)
    di, dt = Rows(4, 2112, torch.float32), Rows(4, 2112, torch.float32)
    need = L.head_bwd_workspace_bytes(4, 832, 1088)
    ws = torch.full((need + 16,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(B=4, d_img=832, d_txt=1088, n=4, mode=0, p=0.0, code=L.F32, W=i.W.ptrs, Gp=G.ptrs, w=ws[:need], fwd=True, bwd=True):
        if fwd:
            with pytest.raises(L.MmrcaError):
                L.head_fwd(i.imgd, i.txtd, W, lg.flat, B, d_img, d_txt, n, True, mode, p, 7, code)
        if bwd:
            with pytest.raises(L.MmrcaError):
                L.head_bwd(i.dld, i.imgd, i.txtd, W, Gp, di.flat, dt.flat, B, d_img, d_txt, n, True, mode, p, 7, code, workspace=w)

    def without(ptrs, field):
        q = L.HeadPtrs()
        for f in R.FIELDS:
            setattr(q, f, None if f == field else getattr(ptrs, f))
        return q
    call(B=0)
    call(d_img=96)
    call(d_txt=2112)
    call(n=0)
    call(n=17)
    call(mode=3)
    call(p=1.0)
    call(code=7)
    call(W=without(i.W.ptrs, "c2_wv"))
    call(Gp=without(G.ptrs, "sat_bk"), fwd=False)
    call(w=ws[:need - 1], fwd=False)
    call(w=ws[4:4 + need], fwd=False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(lg.host()).all()) and bool(torch.isnan(di.host()).all()) and bool(torch.isnan(dt.host()).all()), "a rejected call wrote"
    got, intact = G.split(G.flat.cpu())
    assert intact and all(torch.equal(got[f], i.pre[f]) for f in R.FIELDS), "a rejected call wrote a gradient"
    assert bool((ws == 0xA5).all()), "a rejected call wrote the workspace"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_backward_refuses_what_its_lds_plan_cannot_hold_and_the_forward_still_runs(dtype):
    """d_img + d_txt = 3520: the forward needs 95 KiB of LDS and runs; the backward would need 160.25 KiB and says so"""
    c = R.Case(3, *R.LDS_OVER_WIDTHS, 0, True, dtype)
    i = Inputs(c)
    fails = []
    _judge(i, {"logits": _fwd(i)}, fails)
    assert not fails, fails
    with pytest.raises(L.MmrcaError, match="LDS budget exceeded"):
        _bwd(i)
