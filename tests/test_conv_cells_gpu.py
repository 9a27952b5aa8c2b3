"""Every dispatch cell of the depthwise-conv, BatchNorm, pooling / squeeze-excitation and layout kernels of csrc/conv.hip against the
float64 statement of the same operation on the kernel's exact inputs (tests/conv_cells_ref.py: the references, the restated dispatch,
the case lists, the input builders, the error model and what is out of scope).  Needs an MI355X; every call goes through the C ABI.

Every input buffer is followed by guard rows and guard elements of loud finite values; every output starts as NaN inside the owned
region and as a sentinel outside it, and after the call every owned element is written and every sentinel bit-identical.  Every case
runs twice: outputs written without atomics repeat bitwise, outputs that are (or depend on) fp32 atomic sums repeat within their
bound.  Those are the 3x3 weight gradient in all its forms (dw_wg_reduce_k adds its eight row chunks atomically), the 5x5 weight
gradient without a workspace, the statistics, the backward's sums and parameter gradients, and -- with batch statistics -- the dx
that is computed from those sums."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import lib as L          # noqa: E402
from tests import conv_cells_ref as R                         # noqa: E402

DEV = "cuda"
F32T = torch.float32
OBSERVED = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need a GPU"
    L.load()
    torch.cuda.synchronize()
    yield
    print("\nconv cells: worst observed error / bound unit")
    for k in sorted(OBSERVED, key=str):
        print(f"  {k}: {OBSERVED[k]:.3g}  (bound {R.BOUND[k]})")


def _vec(v, t=F32T, mis=False):
    return R.operand(v.reshape(1, -1), t, mis)[0]


def _ws(nbytes):
    """a 16-byte aligned workspace of exactly nbytes (NaN: a row read before it is written shows), sentinels behind it"""
    o = R.Out(1, nbytes // 4, F32T, DEV)
    return o, o.flat[:nbytes // 4]


# ------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------
def _run_dw(c, i):
    t = R.tdt(c.dtype)
    code, (Ho, Wo), kk = L.dtype_code(t), R.dw_out(c), c.k * c.k
    if c.op == "fwd":
        y = R.Out(c.B * Ho * Wo, c.C, t, DEV, mis=c.mis == "y")
        (L.dwconv3x3_fwd if c.k == 3 else L.dwconv5x5_fwd)(i.x, i.w, y.t, c.B, c.H, c.W, c.C, c.stride, code)
        return {"y": y}
    o = {}
    if c.form in ("dx", "both"):
        o["dx"] = R.Out(c.B * c.H * c.W, c.C, t, DEV, mis=c.mis == "dx")
    if c.form in ("dw", "both"):
        o["dw"] = R.Out(1, c.C * kk, F32T, DEV, fill=i.pre)
    nbytes = R.dw_ws_bytes(c)
    ws = None
    if nbytes is not None:
        o["_ws"], ws = _ws(nbytes)
    (L.dwconv3x3_bwd if c.k == 3 else L.dwconv5x5_bwd)(i.dy, i.x, i.w, o["dx"].t if "dx" in o else None, o["dw"].t if "dw" in o else None,
                                                      c.B, c.H, c.W, c.C, c.stride, code, ws=ws)
    return o


def _run_stats(c, i):
    t, C = R.tdt(c.dtype), c.C
    code = L.dtype_code(t)
    o = {}
    if c.op == "moments":
        o["s1"], o["s2"], o["shift"] = R.Out(1, C, F32T, DEV, fill=i.pre1), R.Out(1, C, F32T, DEV, fill=i.pre2), R.Out(1, C, F32T, DEV)
        L.bn_moments(i.x, o["s1"].t, o["s2"].t, o["shift"].t, c.rows, C, c.ld, code)
        return o
    zero = torch.zeros(2 * C, device=DEV)
    fill = zero if c.prezeroed else torch.full((2 * C,), 123.0, device=DEV)      # not prezeroed: garbage the entry point must clear
    if c.ld != C:            # one [2, C] buffer: the adjacent form (one fill instead of two)
        o["_ms"] = R.Out(2, C, F32T, DEV, fill=fill)
        mean, rstd = o["_ms"].t, o["_ms"].t[C:]
    else:
        o["mean"], o["rstd"] = R.Out(1, C, F32T, DEV, fill=fill[:C]), R.Out(1, C, F32T, DEV, fill=fill[C:])
        mean, rstd = o["mean"].t, o["rstd"].t
    if not c.norun:
        o["rm"], o["rv"] = R.Out(1, C, F32T, DEV, fill=i.rm), R.Out(1, C, F32T, DEV, fill=i.rv)
    tickets = None
    if c.op == "fused":
        n = R.cdiv(C, 64)
        o["_tickets"] = R.Out(1, n, torch.int32, DEV, fill=torch.zeros(n, device=DEV) if c.prezeroed else torch.full((n,), 5.0, device=DEV))
        tickets = o["_tickets"].t[:n]
    L.bn_stats(i.x, mean, rstd, o["rm"].t if "rm" in o else None, o["rv"].t if "rv" in o else None, c.rows, C, c.ld, R.EPS, c.momentum or 0.0,
               c.train, code, prezeroed=bool(c.prezeroed), tickets=tickets)
    return o


def _run_fwd(c, i):
    t, C, Rw = R.tdt(c.dtype), c.C, c.rows
    code = L.dtype_code(t)
    o = {"y": R.Out(Rw, C, t, DEV, mis=c.mis == "y")}
    res = i.res if c.res else None
    sc = _vec(i.sc) if c.res and c.rowscale else None
    if c.op == "fin":
        o["mean"], o["rstd"] = R.Out(1, C, F32T, DEV), R.Out(1, C, F32T, DEV)
        o["rm"], o["rv"] = R.Out(1, C, F32T, DEV, fill=i.rm), R.Out(1, C, F32T, DEV, fill=i.rv)
        L.bn_act_fwd_fin(i.x, _vec(i.s1), _vec(i.s2), _vec(i.sh), i.gamma, i.beta, res, sc, o["y"].t, o["mean"].t, o["rstd"].t, o["rm"].t,
                         o["rv"].t, Rw, C, c.act, c.rps, R.EPS, c.momentum or 0.0, code)
    elif c.op == "res":
        L.bn_act_fwd_res(i.x, _vec(i.mu), _vec(i.rs), i.gamma, i.beta, res, sc, o["y"].t, Rw, C, c.act, c.rps, code)
    else:
        L.bn_act_fwd(i.x, _vec(i.mu), _vec(i.rs), i.gamma, i.beta, o["y"].t, Rw, C, c.act, code)
    return o


def _run_bwd(c, i):
    t, C, Rw = R.tdt(c.dtype), c.C, c.rows
    o = {}
    if c.op == "sums":
        o["_sums"] = R.Out(1, 2 * C, F32T, DEV, fill=torch.cat([i.sd, i.sx]))
    else:
        o["_sums"] = R.Out(1, 2 * C, F32T, DEV, fill=torch.full((2 * C,), 123.0, device=DEV))
    if not c.nodx:
        o["dx"] = R.Out(Rw, C, t, DEV, mis=c.mis == "dx")
    if not c.noparam:
        o["dgamma"], o["dbeta"] = R.Out(1, C, F32T, DEV, fill=i.pre_g), R.Out(1, C, F32T, DEV, fill=i.pre_b)
    g = lambda k: o[k].t if k in o else None      # noqa: E731
    L.bn_act_bwd(i.dy, i.x, _vec(i.mu), _vec(i.rs), i.gamma, i.beta, g("dx"), g("dgamma"), g("dbeta"), o["_sums"].t, Rw, C, c.act,
                 int(bool(c.train)), L.dtype_code(t), sums_ready=c.op == "sums")
    return o


def _run_pool(c, i):
    t = R.tdt(c.dtype)
    code, op, mis = L.dtype_code(t), c.op, c.mis
    if op == "residual_add":
        o = {"out": R.Out(c.B, c.per_sample, t, DEV, mis=mis == "out")}
        L.residual_add(None if c.noa else i.a, i.br, _vec(i.sc) if c.rowscale else None, o["out"].t, c.B, c.per_sample, code)
        return o
    B, HW, C = c.B, c.HW, c.C
    Rw = B * HW
    if op == "rowpool_mean":
        o = {"out": R.Out(B, C, t, DEV)}
        L.rowpool_mean(i.x, o["out"].t, B, HW, C, code)
    elif op == "rowpool_mean_bwd":
        o = {"dx": R.Out(Rw, C, t, DEV, mis=mis == "dx", fill=i.dx0 if c.acc else None)}
        L.rowpool_mean_bwd(i.dpool, o["dx"].t, B, HW, C, bool(c.acc), code)
    elif op == "se_scale_fwd":
        o = {"y": R.Out(Rw, C, t, DEV, mis=mis == "y")}
        L.se_scale_fwd(i.x, i.s, o["y"].t, B, HW, C, code)
    elif op == "se_scale_bwd":
        o = {"ds": R.Out(B, C, t, DEV)}
        if not c.nodx:
            o["dx"] = R.Out(Rw, C, t, DEV, mis=mis == "dx")
        L.se_scale_bwd(i.dy, i.x, i.s, o["dx"].t if "dx" in o else None, o["ds"].t, B, HW, C, code)
    elif op == "se_dx":
        o = {"dx": R.Out(Rw, C, t, DEV, mis=mis == "dx")}
        bn = None
        if c.bn:
            o["sums"] = R.Out(2, C, F32T, DEV, fill=i.pre)
            bn = (i.z, _vec(i.mu), _vec(i.rs), i.gamma, i.beta, c.act, o["sums"].t)
        L.se_dx(i.dy, i.s, i.dpool, o["dx"].t, B, HW, C, code, bn=bn)
    elif op == "bias_act_fwd":
        o = {"y": R.Out(Rw, C, t, DEV)}
        L.bias_act_fwd(i.x, None if c.nobias else i.bias, o["y"].t, Rw, C, c.act, code)
    elif op == "bias_act_bwd":
        o = {"dx": R.Out(Rw, C, t, DEV)}
        if not c.nodb:
            o["dbias"] = R.Out(1, C, F32T, DEV, fill=i.pre)
        L.bias_act_bwd(i.dy, i.x, None if c.nobias else i.bias, o["dx"].t, o["dbias"].t if "dbias" in o else None, Rw, C, c.act, code)
    return o


RUN = {"dw": _run_dw, "stats": _run_stats, "fwd": _run_fwd, "bwd": _run_bwd, "pool": _run_pool}


def _atomic(c):
    """the outputs that are, or are computed from, fp32 atomic sums"""
    if c.fam == "dw":
        return {"dw"} if (c.k == 3 or c.ws in (None, "none", "small")) else set()
    if c.fam == "stats":
        return {"mean", "rstd", "_ms", "rm", "rv", "s1", "s2"}
    if c.fam == "bwd" and c.op == "bwd":
        return {"_sums", "dgamma", "dbeta"} | ({"dx"} if c.train else set())
    if c.fam == "pool" and c.op == "se_dx":
        return {"sums"}
    return set()


# ------------------------------------------------------------------------------------------------------
# one case
# ------------------------------------------------------------------------------------------------------
def _first_bad(bad):
    idx = torch.nonzero(bad)
    return tuple(int(k) for k in idx[0]) if idx.numel() else None


def _collect(c, i, o, tag):
    """guards, every owned element written; the outputs as float64 under the reference's names"""
    got = {}
    for k, b in o.items():
        assert b.untouched(), f"{tag}: a guard element of {k} was written"
        if k in ("_ws", "_tickets"):
            continue
        bad = ~torch.isfinite(b.owned.float())
        assert not bool(bad.any()), f"{tag}: {k} not written / not finite at {_first_bad(bad)}"
        if not k.startswith("_"):
            got[k] = b.owned.double()
    if "_ms" in o:
        got["mean"], got["rstd"] = o["_ms"].owned[0].double(), o["_ms"].owned[1].double()
    if "_sums" in o:
        s = o["_sums"].owned[0]
        if c.op == "sums":
            assert torch.equal(s.double(), torch.cat([i.sd, i.sx])), f"{tag}: the given sums were changed"
        else:
            got["sd"], got["sx"] = s[:c.C].double(), s[c.C:].double()
    return got


def _check(c, i, ref, got, tag):
    fails = []
    got = {k: v.reshape(ref[k].shape) for k, v in got.items() if k in ref}
    if c.ints:
        for k, v in got.items():
            if not torch.equal(v, ref[k]):
                fails.append(f"{k} differs from the exact integer result at {_first_bad(v != ref[k])}")
        return fails
    for name, key, r in R.ratios(c, i, ref, got):
        if not r.numel():
            continue
        w = float(r.max())
        OBSERVED[key] = max(OBSERVED.get(key, 0.0), w)
        if not w <= R.BOUND[key]:
            fails.append(f"{name}: error {w:.3g} > {R.BOUND[key]} units at {_first_bad(~(r <= R.BOUND[key]))}")
    return fails


def _case_test(c):
    tag = f"{c!r} [{' + '.join(R.cell(c)[0])}]"
    i = R.build(c, DEV)
    if R.rejected(c):
        with pytest.raises(L.MmrcaError):
            RUN[c.fam](c, i)
        return
    o = RUN[c.fam](c, i)
    torch.cuda.synchronize()
    got = _collect(c, i, o, tag)
    if c.fam == "stats" and c.op == "moments":
        assert torch.equal(got.pop("shift")[0], i.shift), f"{tag}: the shift is not the trimmed mean of the 16 sampled rows"
    if c.fam == "stats" and c.op == "stats" and not c.train:
        assert torch.equal(got["rm"][0], i.rm) and torch.equal(got["rv"][0], i.rv), f"{tag}: eval mode changed the running statistics"
    if c.fam in ("stats", "fwd") and "rm" in got and not (c.momentum or 0.0) > 0:
        assert torch.equal(got["rm"][0], i.rm) and torch.equal(got["rv"][0], i.rv), f"{tag}: momentum 0 changed the running statistics"
    ref = R.reference(c, i, got)
    if c.fam in ("bwd", "pool") and hasattr(i, "near"):
        share = float(i.near.double().mean())
        assert share <= 0.005, f"{tag}: {share:.4f} of the elements are inside a kink band"
    fails = _check(c, i, ref, got, tag)
    o2 = RUN[c.fam](c, i)
    torch.cuda.synchronize()
    got2 = _collect(c, i, o2, tag)
    got2.pop("shift", None)
    atomic = _atomic(c)
    for k, b in o.items():
        if k in ("_ws", "_tickets") or k in atomic:
            continue
        assert torch.equal(R.bits(b.flat), R.bits(o2[k].flat)), f"{tag}: {k} differs bitwise between two identical runs"
    if atomic:
        ref2 = R.reference(c, i, got2)
        fails += ["second run: " + f for f in _check(c, i, ref2, got2, tag)]
    assert not fails, f"{tag}: " + "; ".join(fails)


def _rejected_writes_nothing(c):
    """the -3 returns: MmrcaError, and no output element written"""
    i = R.build(c, DEV)
    t, C, Rw = R.tdt(c.dtype), c.C, (c.rows or (c.B or 0) * (c.HW or 0))
    outs = [R.Out(max(Rw, 1), C, t, DEV, mis=c.mis in ("y", "dx")) for _ in range(1)] + [R.Out(1, 2 * C, F32T, DEV) for _ in range(4)]
    y, a, b, s3, s4 = outs
    code = L.dtype_code(t)
    with pytest.raises(L.MmrcaError):
        if c.fam == "stats":
            L.bn_moments(i.x, a.t, b.t, s3.t, c.rows, C, c.ld, code)
        elif c.op == "res":
            L.bn_act_fwd_res(i.x, _vec(i.mu), _vec(i.rs), i.gamma, i.beta, i.res, _vec(i.sc) if c.rowscale else None, y.t, Rw, C, c.act, c.rps, code)
        elif c.op == "fin":
            L.bn_act_fwd_fin(i.x, _vec(i.s1), _vec(i.s2), _vec(i.sh), i.gamma, i.beta, i.res if c.res else None, None, y.t, a.t, b.t, s3.t, s4.t,
                             Rw, C, c.act, c.rps, R.EPS, 0.1, code)
        else:
            bn = (i.z, _vec(i.mu), _vec(i.rs), i.gamma, i.beta, c.act, a.t) if c.bn else None
            L.se_dx(i.dy, i.s, i.dpool, y.t, c.B, c.HW, C, code, bn=bn)
    torch.cuda.synchronize()
    for o in outs:
        assert o.untouched() and bool(torch.isnan(o.owned.float()).all()), f"{c!r}: a rejected call wrote"


def _split(cases):
    return [c for c in cases if not R.rejected(c)], [c for c in cases if R.rejected(c)]


DW_RUN, _ = _split(R.DW_CASES)
STATS_RUN, STATS_REJ = _split(R.STATS_CASES)
FWD_RUN, FWD_REJ = _split(R.FWD_CASES)
BWD_RUN, _ = _split(R.BWD_CASES)
POOL_RUN, POOL_REJ = _split(R.POOL_CASES)


@pytest.mark.parametrize("case", DW_RUN, ids=repr)
def test_depthwise_cells_match_float64(case):
    _case_test(case)


@pytest.mark.parametrize("case", STATS_RUN, ids=repr)
def test_batchnorm_statistics_cells_match_float64(case):
    _case_test(case)


@pytest.mark.parametrize("case", FWD_RUN, ids=repr)
def test_batchnorm_apply_cells_match_float64(case):
    _case_test(case)


@pytest.mark.parametrize("case", BWD_RUN, ids=repr)
def test_batchnorm_backward_cells_match_float64(case):
    _case_test(case)


@pytest.mark.parametrize("case", POOL_RUN, ids=repr)
def test_pool_se_elementwise_cells_match_float64(case):
    _case_test(case)


@pytest.mark.parametrize("case", STATS_REJ + FWD_REJ + POOL_REJ, ids=repr)
def test_unbuilt_cases_are_rejected_and_write_nothing(case):
    _rejected_writes_nothing(case)


# ------------------------------------------------------------------------------------------------------
# max pooling and the layout kernels
# ------------------------------------------------------------------------------------------------------
LAYOUT = {op: [c for c in R.LAYOUT_CASES if c.op == op] for op in {c.op for c in R.LAYOUT_CASES}}


@pytest.mark.parametrize("case", LAYOUT["maxpool3x3s2"], ids=repr)
def test_maxpool_takes_the_first_maximum_and_routes_the_gradient_there(case):
    c, t = case, R.tdt(case.dtype)
    g, code = R.gen(c, DEV), L.dtype_code(t)
    Ho, Wo = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
    x, x64 = R.operand(R.randint(g, -3, 3, c.B * c.H * c.W, c.C), t)              # small integers: ties in nearly every window
    dy, dy64 = R.operand(R.randn(g, c.B * Ho * Wo, c.C), t)
    ry, rarg = R.maxpool_ref(x64.view(c.B, c.H, c.W, c.C))
    rdx, rmag = R.maxpool_bwd_ref(dy64.view(c.B, Ho, Wo, c.C), rarg, c.H, c.W)
    prev = None
    for _ in range(2):
        y, arg, dx = R.Out(c.B * Ho * Wo, c.C, t, DEV), R.Out(c.B * Ho * Wo, c.C, torch.uint8, DEV), R.Out(c.B * c.H * c.W, c.C, t, DEV)
        L.maxpool3x3s2_fwd(x, y.t, arg.t, c.B, c.H, c.W, c.C, code)
        L.maxpool3x3s2_bwd(dy, arg.t, dx.t, c.B, c.H, c.W, c.C, code)
        torch.cuda.synchronize()
        assert y.untouched() and arg.untouched() and dx.untouched(), f"{c!r}: a guard element was written"
        assert torch.equal(y.owned.double(), ry.view(-1, c.C)), f"{c!r}: y is not the window maximum"
        assert torch.equal(arg.owned, rarg.view(-1, c.C)), f"{c!r}: the argmax is not the first maximum in (ky, kx) order"
        r = R.pointwise(dx.owned.double(), rdx.view(-1, c.C), rmag.view(-1, c.C), t)
        OBSERVED[("ew", c.dtype)] = max(OBSERVED.get(("ew", c.dtype), 0.0), float(r.max()))
        assert float(r.max()) <= R.BOUND[("ew", c.dtype)], f"{c!r}: dx error {float(r.max()):.3g} units at {_first_bad(r > R.BOUND[('ew', c.dtype)])}"
        cur = (R.bits(y.flat), R.bits(arg.flat), R.bits(dx.flat))
        assert prev is None or all(torch.equal(a, b) for a, b in zip(prev, cur)), f"{c!r}: two identical runs differ"
        prev = cur


@pytest.mark.parametrize("case", LAYOUT["channel_gather"], ids=repr)
def test_channel_gather_writes_its_columns_only(case):
    c, t = case, R.tdt(case.dtype)
    g = R.gen(c, DEV)
    x, x64 = R.operand(R.randn(g, c.rows, c.Cin), t)
    cmap = torch.randint(0, c.Cin, (c.Cout,), generator=g, device=DEV, dtype=torch.int32)
    out = R.Out(c.rows, c.ld_out, t, DEV)
    out.body[:] = R.SENT
    L.channel_gather(x, cmap, out.t, c.rows, c.Cin, c.Cout, c.ld_out, c.col0, L.dtype_code(t))
    torch.cuda.synchronize()
    want = torch.full((c.rows, c.ld_out), R.SENT, dtype=torch.float64, device=DEV)
    want[:, c.col0:c.col0 + c.Cout] = x64[:, cmap.long()]
    assert out.untouched() and torch.equal(out.body.double(), want), f"{c!r}"


@pytest.mark.parametrize("case", LAYOUT["channel_interleave2"] + LAYOUT["channel_deinterleave2"], ids=repr)
def test_channel_interleave_and_its_inverse_are_the_host_permutation(case):
    c, t = case, R.tdt(case.dtype)
    g, code = R.gen(c, DEV), L.dtype_code(t)
    if c.op == "channel_interleave2":
        a, a64 = R.operand(R.randn(g, c.rows, c.bf), t, ld=c.lda)
        b, b64 = R.operand(R.randn(g, c.rows, c.bf), t)
        out = R.Out(c.rows, 2 * c.bf, t, DEV)
        L.channel_interleave2(a, c.lda, b, out.t, c.rows, c.bf, code)
        torch.cuda.synchronize()
        want = torch.stack([a64, b64], 2).reshape(c.rows, 2 * c.bf)
        assert out.untouched() and torch.equal(out.owned.double(), want), f"{c!r}"
        return
    d, d64 = R.operand(R.randn(g, c.rows, 2 * c.bf), t)
    even, odd = R.Out(c.rows, c.bf, t, DEV, ld=c.lda), R.Out(c.rows, c.bf, t, DEV)
    L.channel_deinterleave2(d, even.t, c.lda, odd.t, c.rows, c.bf, code)
    torch.cuda.synchronize()
    assert even.untouched() and odd.untouched(), f"{c!r}: a guard element was written"
    assert torch.equal(even.owned.double(), d64[:, 0::2]) and torch.equal(odd.owned.double(), d64[:, 1::2]), f"{c!r}"


@pytest.mark.parametrize("case", LAYOUT["nchw_to_rows"], ids=repr)
def test_nchw_to_rows_is_permute_and_round_to_nearest_even(case):
    c, t = case, R.tdt(case.dtype)
    g = R.gen(c, DEV)
    img = (3.0 * R.randn(g, c.B, c.C, c.H, c.W)).float()
    img.view(-1)[::7] = 1.00390625                # 1 + 2^-8: a tie between two bf16 values (rounds to the even one, 1.0)
    flat, _ = R.operand(img.double().reshape(1, -1), F32T)
    out = R.Out(c.B * c.H * c.W, c.C, t, DEV)
    L.nchw_to_rows(flat, out.t, c.B, c.C, c.H, c.W, L.dtype_code(t))
    torch.cuda.synchronize()
    want = img.permute(0, 2, 3, 1).reshape(-1, c.C).to(t)
    assert out.untouched() and torch.equal(R.bits(out.owned.contiguous()), R.bits(want.contiguous())), f"{c!r}"
