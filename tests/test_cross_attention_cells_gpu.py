"""Every dispatch cell of the cross-attention forward (csrc/attention_cross.hip: the 48 instantiations of mha_cross_mfma_k, every way
mmrca_mha_cross_fwd falls to mha_cross_ref_k in both dtypes, the 72 instantiations of mha_cross_x3_k over one chunk, whole chunks, a
ragged last chunk and a last chunk of at most one tile) against the float64 statement of tests/cross_attention_ref.py on the kernel's
exact inputs, per (batch, head) block and per query row.  Needs an MI355X; every call goes through the C ABI (L.mha_cross_fwd,
L.mha_cross_fwd_x3).

Inputs (cross_attention_ref.build): a third of the query rows flat, the rest with one key about 12 (or 100) above the others, that
key cycling through the tile and chunk boundaries; four different row strides; +-8192 in the gap columns and in 128 slack rows behind
every input.  Outputs start as NaN where the kernel owns an element and as a sentinel in the gap columns and in 16 guard rows behind:
afterwards every owned element is finite and every sentinel is bit-identical.  Every case runs twice and repeats bitwise (no kernel
here has an atomic).

The 193 cases run as 14 test items (cross_attention_ref.GROUPS): one per key-tile count of the mfma kernel, one per (chunk, head dim)
pair of the x3 kernel, one for the reference kernel.  An item's id spells its cells as a product, it runs all of its cases whatever
the earlier ones did, and its failure message names each failing case (the cell and the shape), the block, the row and the row's
dominant key.

Bounds (cross_attention_ref.bound) come from the rounding model of each kernel on the CPU (cross_attention_ref.EMULATED), never from
what a GPU returned; the worst errors observed on an MI355X stand beside them below and are printed again at teardown."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import lib as L          # noqa: E402
from tests import cross_attention_ref as R                    # noqa: E402

# kernel: (per block, per row) bound <- rounding model on the CPU (cross_attention_ref.EMULATED) | observed on an MI355X over the cases
#   mfma     : 1e-2, 1e-2 (the forward cap of test_attention_cells_gpu.py)  <- 5.3e-3, 6.4e-3 | 5.3e-3, 6.4e-3
#   x3       : 7.6e-5, 8.0e-5 (4x the model, cap 1e-4)                      <- 1.9e-5, 2.0e-5 | 1.9e-5, 2.7e-5
#   ref f32  : 4.8e-6, 5.2e-6 (4x the model, cap 2e-5)                      <- 1.1e-6, 1.2e-6 | 1.3e-6, 1.3e-6
#   ref bf16 : 3.91e-3 (2^-8 for the output rounding + the fp32 bound)      <- 3.7e-3, 3.7e-3 | 3.7e-3, 3.7e-3
# (the bf16 kernels agree with their models to the printed digits: inputs are seeded and the error is the output rounding's)
OBSERVED = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need a GPU"
    L.load()
    L.seed_epoch_set(0)            # test_graph_gpu.py moves the mask epoch
    torch.cuda.synchronize()
    yield
    print("\ncross-attention cells: worst observed error, per block / per row")
    for k in sorted(OBSERVED):
        print(f"  {k}: {OBSERVED[k][0]:.3g} / {OBSERVED[k][1]:.3g}")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _operand(dev, inp, x, off=0):
    """(a view that starts at the operand's first element, its row stride)"""
    buf, col, ld = inp.where[x]
    return dev[buf].view(-1)[col + off:], ld


class Out:
    """an output [B * Sq, D] with row stride ldo: NaN where the kernel owns an element, SENT in the gap columns and GUARD rows"""

    def __init__(self, rows, D, ldo, t):
        self.rows, self.D = rows, D
        self.init = torch.full((rows + R.GUARD, ldo), R.SENT, dtype=t)
        self.init[:rows, :D] = float("nan")
        self.dev = self.init.cuda()

    def host(self, tag):
        h = self.dev.cpu()
        own = torch.zeros(h.shape, dtype=torch.bool)
        own[:self.rows, :self.D] = True
        assert torch.equal(_bits(h)[~own], _bits(self.init)[~own]), f"{tag}: a gap column or a guard row of the output was written"
        bad = ~torch.isfinite(h[:self.rows, :self.D].float())
        assert not bool(bad.any()), f"{tag}: output not written / not finite at (row, column) {tuple(int(j) for j in torch.nonzero(bad)[0])}"
        return h[:self.rows, :self.D]


def _run(c, inp, dev):
    """one call on fresh outputs: the owned part of the output on the host (the x3 kernel: its two planes)"""
    D, rows = c.H * c.dh, c.B * c.Sq
    (q, ldq), (k, ldk), (v, ldv) = (_operand(dev, inp, x) for x in "qkv")
    if c.entry == "x3":
        hi, lo = Out(rows, D, inp.ldo, torch.bfloat16), Out(rows, D, inp.ldo, torch.bfloat16)
        L.mha_cross_fwd_x3(q, ldq, k, ldk, v, ldv, (hi.dev, lo.dev), inp.ldo, c.B, c.H, c.Sq, c.Skv, c.dh, c.scale, drop_p=c.drop_p, drop_seed=c.seed)
        torch.cuda.synchronize()
        return [hi.host(f"{c!r} (hi plane)"), lo.host(f"{c!r} (lo plane)")]
    out = Out(rows, D, inp.ldo, R.tdt(c.dtype))
    L.mha_cross_fwd(q, ldq, k, ldk, v, ldv, out.dev, inp.ldo, c.B, c.H, c.Sq, c.Skv, c.dh, c.scale, L.dtype_code(R.tdt(c.dtype)), c.impl,
                    drop_p=c.drop_p, drop_seed=c.seed)
    torch.cuda.synchronize()
    return [out.host(repr(c))]


def _cell(c):
    inp = R.build(c)
    dev = {name: buf.cuda() for name, buf in inp.bufs.items()}
    mask = R.case_mask(c)
    ref = R.cross_ref(inp.q, inp.k, inp.v, c.H, c.scale, mask)
    a = _run(c, inp, dev)
    b = _run(c, inp, dev)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y)), f"{c!r}: two identical calls differ bitwise"
    for name, buf in inp.bufs.items():
        assert torch.equal(_bits(dev[name].cpu()), _bits(buf)), f"{c!r}: input buffer {name} was written"
    got = sum(x.double() for x in a).view(c.B, c.Sq, c.H * c.dh)
    blk, row = R.errors(got, ref, c.H)
    wb, wr = float(blk.max()), float(row.max())
    key = R.bound_key(c)
    ob, orow = OBSERVED.get(key, (0.0, 0.0))
    OBSERVED[key] = (max(ob, wb), max(orow, wr))
    bb, br = R.bound(c)
    print(f"{c!r}: per block {wb:.3g} (bound {bb:.3g}), per row {wr:.3g} (bound {br:.3g})")
    fails = []
    if not wb <= bb:
        bi, hi = (int(j) for j in torch.nonzero(~(blk <= bb))[0])
        fails.append(f"block b={bi} h={hi}: max |err| / max |ref| = {float(blk[bi, hi]):.3g} > {bb:.3g}")
    if not wr <= br:
        bad = torch.nonzero(~(row <= br))
        bi, hi, i = (int(j) for j in bad[0])
        dom = int(inp.dominant[bi, hi, i])
        fails.append(f"row b={bi} h={hi} i={i} ({'flat' if dom < 0 else f'dominant key {dom}'}): max |err| / row scale = "
                     f"{float(row[bi, hi, i]):.3g} > {br:.3g}; {bad.shape[0]} rows of {row.numel()} over the bound, dominant keys "
                     f"{sorted({int(inp.dominant[tuple(j)]) for j in bad})} (boundary keys {inp.boundary})")
    if c.Skv == 1:              # one key: the probability is exactly 1 and the output is the V row in the output format
        emu = R.emulate(c.cell, inp.q, inp.k, inp.v, c.H, c.scale, mask)
        if not torch.equal(got, emu):
            fails.append("S_kv = 1: the output is not the V row in the output format")
    assert not fails, f"{c!r} cell {c.cell}:\n  " + "\n  ".join(fails)


def _cells(cases):
    """every case of an item (cross_attention_ref.GROUPS); a case that fails does not hide the cases behind it"""
    fails = []
    for c in cases:
        try:
            _cell(c)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, f"{len(fails)} of {len(cases)} cases:\n" + "\n".join(fails)


def _items(kernel):
    g = [x for x in R.GROUPS if x[0] == kernel]
    return dict(argnames="cases", argvalues=[x[2] for x in g], ids=[x[1] for x in g])


@pytest.mark.parametrize(**_items("mfma"))
def test_mfma_cells_match_float64(cases):
    _cells(cases)


@pytest.mark.parametrize(**_items("ref"))
def test_ref_cells_match_float64(cases):
    _cells(cases)


@pytest.mark.parametrize(**_items("x3"))
def test_x3_cells_match_float64(cases):
    _cells(cases)


def _one_per_head_dim(cases):
    seen, out = set(), []
    for c in cases:
        if c.dh % 32 and c.dh % 8 == 0 and (c.kernel, c.dh) not in seen:
            seen.add((c.kernel, c.dh))
            out.append(c)
    return out


def test_nothing_outside_a_heads_columns_is_read():
    """head dims that are no multiple of 32: the matrix-core kernels pad them, and the padding of the last head lies in the gap
    columns.  With NaN instead of +-8192 in every gap column and slack row, the output is bit-identical: a padded column that was
    read and multiplied by a zero would turn its row into NaN.  One case per (kernel, head dim)."""
    cases = _one_per_head_dim(R.CASES)
    assert {(c.kernel, R.DHS_OF(c.dh)) for c in cases} >= {(k, d) for k in ("mfma", "x3") for d in (2, 3, 4)}
    fails = []
    for c in cases:
        outs = []
        try:
            for poison in (False, True):
                inp = R.build(c, poison=poison)
                outs.append(_run(c, inp, {name: buf.cuda() for name, buf in inp.bufs.items()}))
            if not all(torch.equal(_bits(x), _bits(y)) for x, y in zip(*outs)):
                fails.append(f"{c!r}: the two outputs differ")
        except AssertionError as e:             # a NaN that reached the output fails _run's own check
            fails.append(str(e).splitlines()[0])
    assert not fails, "the output depends on what stands outside the operands' H x dh columns:\n  " + "\n  ".join(fails)


# ------------------------------------------------------------------------------------------------------
# the mask, bit by bit
# ------------------------------------------------------------------------------------------------------
def test_single_mask_bits_show_in_the_output_of_all_three_kernels():
    """V = the first S_kv rows of the identity in every head (S_kv <= dh): out[b, i, h, j] is P_ij x the mask's multiplier, so a
    dropped key is an exact zero and a kept one is not.  S_kv is no multiple of 16 (a kernel that strides its counter by the padded
    key count reads other bits from the second row on); S_kv = 100 at head dim 104 takes the x3 kernel over two chunks of 96 keys."""
    for Sq, Skv, dh, p in ((33, 50, 56, 0.5), (20, 100, 104, 0.5), (70, 17, 24, 0.1)):
        _mask_bits(Sq, Skv, dh, p)


def _mask_bits(Sq, Skv, dh, p):
    B, H = 2, 3
    D, seed = H * dh, R.DROP_SEED + 1
    assert Skv <= dh and Skv % 16
    g = torch.Generator().manual_seed(Sq + Skv)
    q = (0.3 * torch.randn(B * Sq, D, generator=g)).bfloat16()
    k = (0.3 * torch.randn(B * Skv, D, generator=g)).bfloat16()
    v = torch.zeros(B, Skv, H, dh)
    v[:, torch.arange(Skv), :, torch.arange(Skv)] = 1.0
    v = v.view(B * Skv, D).bfloat16()
    keep = R.keep_bits(seed, B * H, Sq, Skv, p).view(B, H, Sq, Skv).transpose(1, 2)          # [B, Sq, H, Skv]
    assert 0 < int(keep.sum()) < keep.numel()
    prob = torch.softmax(R.scores(q.view(B, Sq, D), k.view(B, Skv, D), H, dh ** -0.5), -1).transpose(1, 2)
    want = prob * keep * R.drop_scale(p)
    scale = float(np.float32(dh ** -0.5))
    outs = {}
    for name, t, impl in (("mfma", torch.bfloat16, L.IMPL_MFMA), ("ref-bf16", torch.bfloat16, L.IMPL_REF), ("ref-f32", torch.float32, L.IMPL_AUTO)):
        out = torch.full((B * Sq, D), float("nan"), dtype=t, device="cuda")
        qd, kd, vd = (x.to(t).cuda() for x in (q, k, v))
        L.mha_cross_fwd(qd, D, kd, D, vd, D, out, D, B, H, Sq, Skv, dh, scale, L.dtype_code(t), impl, drop_p=p, drop_seed=seed)
        outs[name] = out.double().cpu()
    hi = torch.full((B * Sq, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    lo = torch.full_like(hi, float("nan"))
    qd, kd, vd = (x.float().cuda() for x in (q, k, v))
    L.mha_cross_fwd_x3(qd, D, kd, D, vd, D, (hi, lo), D, B, H, Sq, Skv, dh, scale, drop_p=p, drop_seed=seed)
    torch.cuda.synchronize()
    outs["x3"] = hi.double().cpu() + lo.double().cpu()
    for name, o in outs.items():
        o = o.view(B, Sq, H, dh)
        name = f"{name}, S_q {Sq}, S_kv {Skv}, head dim {dh}, p {p}"
        assert bool(torch.isfinite(o).all()), name
        assert bool((o[..., Skv:] == 0).all()), f"{name}: a column no key maps to is not zero"
        live = o[..., :Skv] != 0
        if not torch.equal(live, keep):
            b, i, h, j = (int(x) for x in torch.nonzero(live != keep)[0])
            raise AssertionError(f"{name}: the mask differs from counter ((b*H+h)*Sq+i)*Skv+j at {int((live != keep).sum())} places, first at "
                                 f"b={b} h={h} i={i} j={j}")
        rel = ((o[..., :Skv] - want).abs() / want.clamp(min=1e-30))[keep]
        assert float(rel.max()) < (1e-2 if name.startswith(("mfma", "ref-bf16")) else 1e-4), (name, float(rel.max()))


# ------------------------------------------------------------------------------------------------------
# calls that must be refused before any launch
# ------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_launch():
    """the valid base calls are taken; each of the 22 changed ones (cross_attention_ref.REJECTED) is refused and writes nothing"""
    for entry in ("x3", "fwd"):
        _base_call_is_taken(entry)
    wrong = []
    for name, entry, over in R.REJECTED:
        try:
            _refused(name, entry, over)
        except (AssertionError, pytest.fail.Exception) as e:          # pytest.raises fails with its own exception type
            wrong.append(f"{name}: {e}")
    assert not wrong, "\n".join(wrong)


def _refused(name, entry, over):
    a = dict(R.BASE[entry], **over)
    B, H, Sq, Skv, dh = a["B"], a["H"], a["Sq"], a["Skv"], a["dh"]
    D = H * dh
    t = R.tdt(a["dtype"])
    ld = {x: D + over.get("ld" + x, 16) for x in "qkvo"}
    off = {x: over.get("off" + x, 0) for x in "qkvo"}
    # large enough for the call as asked, whatever it would have launched
    n = (B * max(Sq, Skv) + 8) * (D + 64)
    ins = {x: torch.ones(n, dtype=t, device="cuda") for x in "qkv"}
    to = torch.bfloat16 if entry == "x3" else t
    outs = [torch.full((n,), float("nan"), dtype=to, device="cuda") for _ in range(2)]
    scale = float(np.float32(dh ** -0.5))
    with pytest.raises(L.MmrcaError):
        if entry == "x3":
            L.mha_cross_fwd_x3(ins["q"][off["q"]:], ld["q"], ins["k"][off["k"]:], ld["k"], ins["v"][off["v"]:], ld["v"],
                               (outs[0][off["o"]:], outs[1][off["o"]:]), ld["o"], B, H, Sq, Skv, dh, scale, drop_p=a["drop_p"], drop_seed=7)
        else:
            L.mha_cross_fwd(ins["q"][off["q"]:], ld["q"], ins["k"][off["k"]:], ld["k"], ins["v"][off["v"]:], ld["v"], outs[0][off["o"]:], ld["o"],
                            B, H, Sq, Skv, dh, scale, L.dtype_code(t), a["impl"], drop_p=a["drop_p"], drop_seed=7)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs), f"{name}: a refused call wrote its output"


def _base_call_is_taken(entry):
    """what the refused calls change is the only thing wrong with them"""
    a = R.BASE[entry]
    B, H, Sq, Skv, dh = a["B"], a["H"], a["Sq"], a["Skv"], a["dh"]
    D = H * dh
    t = R.tdt(a["dtype"])
    ins = [torch.ones((B * max(Sq, Skv), D + 16), dtype=t, device="cuda") for _ in range(3)]
    outs = [torch.full((B * Sq, D + 16), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    if entry == "x3":
        L.mha_cross_fwd_x3(ins[0], D + 16, ins[1], D + 16, ins[2], D + 16, outs, D + 16, B, H, Sq, Skv, dh, 0.125, drop_p=a["drop_p"], drop_seed=7)
    else:
        L.mha_cross_fwd(ins[0], D + 16, ins[1], D + 16, ins[2], D + 16, outs[0], D + 16, B, H, Sq, Skv, dh, 0.125, L.dtype_code(t), a["impl"],
                        drop_p=a["drop_p"], drop_seed=7)
    torch.cuda.synchronize()
    got = outs[0].float() + (outs[1].float() if entry == "x3" else 0.0)         # V is all ones: every output is 1
    assert float((got[:, :D] - 1.0).abs().max()) < 1e-6 and bool(torch.isnan(got[:, D:]).all())
