"""The cross-attention forward (csrc/attention_cross.hip) stated plainly in float64, the host-side dispatch of its
three kernels restated as a cell map, a rounding model of each kernel, the dropout multiplier rebuilt on the host, and the committed
case list, input builder, error norm and bounds of tests/test_cross_attention_cells_gpu.py.  Nothing here touches a GPU or loads the
library; tests/test_cross_attention_cells_cpu.py checks this file against the oracle and against attention_cross.hip's source.

Inputs (build()).  Every (batch, head) block has a set of BOUNDARY KEYS: key 0, keys 15 and 16, the last key of the last whole 16-key
tile, key S_kv - 1 and, for the chunked x3 kernel, the last key of chunk 0, the first key of chunk 1 and one key inside the last
chunk.  Query row i is FLAT when i % 3 == 2 (0.8 randn: an average over all keys) and PEAKY otherwise:
    q_i = 0.5 randn + k_j peak sqrt(dh) / |k_j|^2          (peak = 12; 100 in the cases that would overflow without the max-subtraction)
so that key j scores about `peak` above every other key; j cycles through the boundary keys, starting at a different one in every
block.  A head of dh columns cannot hold S_kv nearly orthogonal keys, so the keys are built for it: the boundary keys of a block are
orthogonal to one another with norm sqrt(dh), and every other key is randn with its component inside the boundary keys' span scaled
by OTHER_IN_SPAN.  That is what makes the lead of the dominant key a property of the construction (dominance(), asserted for every
case on the CPU) instead of a property of the seed.  V = randn + 0.5 ((key mod 7) - 3) tells the keys apart.

Buffers.  Four different row strides, each larger than H dh, in the 'sep' layout; 'kv' holds k | v in one [rows, 2D + gap] buffer and
'qkv' q | k | v in one [rows, 3D + gap] buffer, as the engine does.  The gap columns and SLACK rows behind every input hold +-LOUD.
Outputs are NaN where the kernel owns an element and SENT everywhere else (gap columns, GUARD rows behind).

Errors (errors()) are per (batch, head) block, max |err| / max |ref|, and per query row, max |err| / max(row max |ref|, 1e-2 x block
max |ref|): the norm of tests/test_attention_cells_gpu.py.  Bounds (bound()) come from the rounding models below, never from a GPU."""
import zlib

import numpy as np
import torch

from garbage_classification_rca_amd.procedural import counter_uniform

# ---- constants of attention_cross.hip and lib.py, restated (test_cross_attention_cells_cpu.py reads them back out of the source) ----
IMPL_AUTO, IMPL_REF, IMPL_MFMA = 0, 1, 2
NKT_LADDER = (4, 8, 14, 18)                    # mmrca_mha_cross_fwd: the first N with ceil(S_kv / 16) <= N
MFMA_MAX_SKV = 288
MFMA_W8_ABOVE_SQ = 64                          # 8 waves when S_q > 64, else 4
DHS_OF = lambda dh: max(2, -(-dh // 32))       # noqa: E731   head dim padded to 32 * DHS columns
X3_LADDER = {2: ((2, 2), (4, 4), 10), 3: ((2, 2), (4, 4), 10), 4: ((2, 2), (4, 4), 6)}     # DHS -> ((nkt <=, NKTC), ..., else NKTC)
X3_MAX_SQ = 384
X3_W8_ABOVE_NQT = 4                            # 8 waves when ceil(S_q / 16) > 4, else 4
X3_MAX_TPW = 3
MAX_DH = 128
REF_REASONS = ("impl_ref", "fp32", "skv>288", "dh%8", "misaligned")
CHUNK_FORMS = ("one chunk", "whole chunks", "ragged last chunk", "last chunk of <= 16 keys")

SLACK, GUARD = 128, 16
LOUD, SENT = 8192.0, -3072.0                   # both exact in bf16
DROP_SEED = (1 << 33) + 12345                  # above 2^32: the counter arithmetic is 64-bit
PEAK, PEAK_OVERFLOW = 12.0, 100.0
OTHER_IN_SPAN = 0.1
MIN_LEAD = 6.0


def _cdiv(a, b):
    return -(-a // b)


def tdt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


# ---- the dispatch, restated -------------------------------------------------------------------------------------------------
def chunk_form(Skv, nktc):
    crows = 16 * nktc
    n = _cdiv(Skv, crows)
    if n == 1:
        return CHUNK_FORMS[0]
    rem = Skv - (n - 1) * crows
    return CHUNK_FORMS[1] if rem == crows else (CHUNK_FORMS[3] if rem <= 16 else CHUNK_FORMS[2])


def dispatch(entry, dtype, impl, Sq, Skv, dh, aligned, drop_p):
    """the cell the library takes: ("mfma", NKT, DHS, DROP, waves) | ("ref", dtype, reason) | ("x3", NKTC, DHS, DROP, waves, TPW,
    chunk_form) | ("reject", why).  entry 'fwd' = mmrca_mha_cross_fwd, 'x3' = mmrca_mha_cross_fwd_x3; dtype 'bf16' | 'f32'."""
    drop = drop_p > 0
    if not 0 <= drop_p < 1:
        return ("reject", "drop_p")
    nkt = _cdiv(Skv, 16)
    if entry == "x3":
        if dtype != "f32":
            return ("reject", "dtype")
        if dh % 8 or dh > MAX_DH or Sq > X3_MAX_SQ:
            return ("reject", "dh / S_q")
        if not aligned:
            return ("reject", "alignment")
        *steps, last = X3_LADDER[DHS_OF(dh)]
        nktc = next((n for upto, n in steps if nkt <= upto), last)
        nqt = _cdiv(Sq, 16)
        nw = 8 if nqt > X3_W8_ABOVE_NQT else 4
        tpw = max(1, _cdiv(nqt, nw))
        assert tpw <= X3_MAX_TPW
        return ("x3", nktc, DHS_OF(dh), drop, nw, tpw, chunk_form(Skv, nktc))
    assert entry == "fwd"
    why = None
    if dtype != "bf16":
        why = "fp32"
    elif Skv > MFMA_MAX_SKV:
        why = "skv>288"
    elif dh % 8 or dh > MAX_DH:
        why = "dh%8"
    elif not aligned:
        why = "misaligned"
    if impl == IMPL_MFMA and why:
        return ("reject", why)
    if why is None and impl != IMPL_REF:
        return ("mfma", next(n for n in NKT_LADDER if nkt <= n), DHS_OF(dh), drop, 8 if Sq > MFMA_W8_ABOVE_SQ else 4)
    if dh > MAX_DH or Skv > 1024:
        return ("reject", "ref limits")
    return ("ref", dtype, "impl_ref" if impl == IMPL_REF else why)


def all_cells():
    """every cell the two entry points can reach"""
    mfma = {("mfma", n, d, dr, w) for n in NKT_LADDER for d in (2, 3, 4) for dr in (False, True) for w in (4, 8)}
    ref = {("ref", "f32", "fp32"), ("ref", "f32", "impl_ref"), ("ref", "bf16", "impl_ref"), ("ref", "bf16", "skv>288"),
           ("ref", "bf16", "dh%8"), ("ref", "bf16", "misaligned")}
    pairs = [(n, d) for d in (2, 3) for n in (2, 4, 10)] + [(n, 4) for n in (2, 4, 6)]
    x3 = {(n, d, dr, w, t) for n, d in pairs for dr in (False, True) for w, t in ((4, 1), (8, 1), (8, 2), (8, 3))}
    forms = {(n, d, f) for n, d in ((10, 2), (10, 3), (6, 4)) for f in CHUNK_FORMS}
    return mfma, ref, x3, forms


# ---- the float64 statement and the dropout multiplier -----------------------------------------------------------------------
def drop_scale(p):
    """the kernels' fp32 1 / (1 - p)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_bits(seed, BH, Sq, Skv, p):
    """[BH, Sq, Skv] bool: counter ((b * H + h) * S_q + i) * S_kv + j, keep iff u >= float32(p)"""
    u = counter_uniform(seed, np.arange(BH * Sq * Skv, dtype=np.uint64))
    return torch.from_numpy((u >= np.float32(p)).reshape(BH, Sq, Skv))


def drop_multiplier(seed, BH, Sq, Skv, p):
    """[BH, Sq, Skv] float64 of 0 or 1 / (1 - p); None when p == 0"""
    return keep_bits(seed, BH, Sq, Skv, p).double() * drop_scale(p) if p > 0 else None


def _heads(x, H):
    B, S, D = x.shape
    return x.reshape(B, S, H, D // H).transpose(1, 2)            # [B, H, S, dh]


def _merge(o):
    B, H, S, dh = o.shape
    return o.transpose(1, 2).reshape(B, S, H * dh)


def scores(q, k, H, scale):
    """float64 [B, H, Sq, Skv] of the inputs as given (bf16 widened exactly)"""
    return _heads(q.double(), H) @ _heads(k.double(), H).transpose(-1, -2) * float(scale)


def cross_ref(q, k, v, H, scale, mask=None):
    """softmax(q k^T scale) (x mask) v per head in float64: q [B, Sq, D], k / v [B, Skv, D], mask [B*H, Sq, Skv] or None"""
    a = torch.softmax(scores(q, k, H, scale), dim=-1)
    if mask is not None:
        a = a * mask.double().view(a.shape)
    return _merge(a @ _heads(v.double(), H))


# ---- a rounding model of each kernel: the roundings the source states, and nothing else -------------------------------------
def _f32(x):
    return x.float().double()


def _bf(x):
    return x.float().bfloat16().double()


def emulate(cell, q, k, v, H, scale, mask=None):
    """float64 [B, Sq, D] of what the kernel of `cell` stores (the x3 kernel: the sum of its two planes)"""
    kind = cell[0]
    if kind == "ref":                       # fp32 math throughout, one rounding to the output type
        qh, kh, vh = (_heads(t.float(), H) for t in (q, k, v))
        s = qh @ kh.transpose(-1, -2) * np.float32(scale)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        inv = 1.0 / e.sum(-1, keepdim=True)
        if mask is not None:
            e = e * mask.float().view(e.shape)
        return _merge(((e @ vh) * inv).to(tdt(cell[1])).double())
    s = scores(q, k, H, scale)              # exact products of the inputs
    e = _f32(torch.exp(s - s.amax(-1, keepdim=True)))
    inv = _f32(1.0 / _f32(e.sum(-1, keepdim=True)))
    if mask is not None:
        e = _f32(e * mask.double().view(e.shape))
    vh = _heads(v.double(), H)
    if kind == "mfma":
        return _merge(_bf(_f32(_f32(_bf(e) @ vh) * inv)))
    assert kind == "x3"
    p_hi = _bf(e)
    p_lo = _bf(_f32(e - p_hi))
    v_hi = _bf(vh)
    v_lo = _bf(_f32(vh - v_hi))
    x = _f32(_f32(p_hi @ v_lo + p_lo @ v_hi + p_hi @ v_hi) * inv)
    hi = _bf(x)
    return _merge(hi + _bf(_f32(x - hi)))


# ---- the error norm ---------------------------------------------------------------------------------------------------------
def errors(got, ref, H):
    """(block [B, H], row [B, H, Sq]) of float64 got / ref [B, Sq, D]"""
    g, r = _heads(got, H), _heads(ref, H)
    er, rr = (g - r).abs().amax(-1), r.abs().amax(-1)            # [B, H, Sq]
    eb, rb = er.amax(-1), rr.amax(-1)                            # [B, H]
    tiny = 1e-300
    return eb / (rb + tiny), er / (torch.maximum(rr, 1e-2 * rb[..., None]) + tiny)


# ---- the cases --------------------------------------------------------------------------------------------------------------
class Case:
    """one call: entry 'fwd' | 'x3', dtype 'bf16' | 'f32', layout 'sep' | 'kv' | 'qkv' | 'misaligned' (sep with a K stride that is
    no multiple of 16 bytes)"""

    def __init__(self, entry, dtype, impl, Sq, Skv, dh, B=2, H=3, layout="sep", drop_p=0.0, peak=PEAK):
        self.entry, self.dtype, self.impl, self.Sq, self.Skv, self.dh = entry, dtype, impl, Sq, Skv, dh
        self.B, self.H, self.layout, self.drop_p, self.peak = B, H, layout, drop_p, peak
        self.seed = DROP_SEED + Sq if drop_p > 0 else 0
        assert layout != "qkv" or Sq == Skv
        self.cell = dispatch(entry, dtype, impl, Sq, Skv, dh, layout != "misaligned", drop_p)
        assert self.cell[0] != "reject", (self.shape, self.cell)

    @property
    def kernel(self):
        return self.cell[0]

    @property
    def out_dtype(self):
        return "bf16" if self.entry == "x3" else self.dtype

    @property
    def scale(self):
        return float(np.float32(self.dh ** -0.5))

    @property
    def shape(self):
        s = f"B{self.B}H{self.H}-q{self.Sq}-k{self.Skv}-d{self.dh}-{self.layout}"
        if self.drop_p:
            s += f"-p{self.drop_p}"
        if self.peak != PEAK:
            s += f"-peak{self.peak:g}"
        return s

    def __repr__(self):
        c = self.cell
        if c[0] == "mfma":
            name = f"mfma-N{c[1]}-D{c[2]}-{'drop' if c[3] else 'plain'}-w{c[4]}"
        elif c[0] == "ref":
            name = f"ref-{c[1]}-{c[2]}"
        else:
            name = f"x3-N{c[1]}-D{c[2]}-{'drop' if c[3] else 'plain'}-w{c[4]}-t{c[5]}-{c[6].replace(' ', '_')}"
        return name + "__" + self.shape

    @property
    def pad_keys(self):
        """zero-filled key rows the matrix-core kernels stage behind key S_kv - 1"""
        if self.kernel == "ref":
            return 0
        per = 16 * self.cell[1]
        return (_cdiv(self.Skv, per) * per if self.kernel == "x3" else per) - self.Skv

    def boundary_keys(self):
        """the boundary keys of this case, in key order"""
        S = self.Skv
        t = {0, 15, 16, S // 16 * 16 - 1, S - 1}
        if self.kernel == "x3":
            crows = 16 * self.cell[1]
            n = _cdiv(S, crows)
            if n > 1:
                t |= {crows - 1, crows, (n - 1) * crows + (S - (n - 1) * crows) // 2}
        return sorted(j for j in t if 0 <= j < S)


def _pick(seq, i):
    return seq[i % len(seq)]


# shapes per dispatch coordinate; a cell takes them in rotation so that no two cells of a family share a whole shape
# (S_kv of the sweeps leaves at least 9 padded keys, 3% of the keys or more, in the last tile or behind it: a kernel that counts them
# as live shows in every cell; the whole-tile shapes follow as cases of their own)
_SKV_OF_NKT = {4: (50, 55, 17, 33), 8: (100, 119, 65, 113), 14: (215, 200, 129, 209), 18: (257, 279, 225, 241)}
_DH_OF_DHS = {2: (64, 40, 48, 56), 3: (88, 72, 96), 4: (128, 104, 120)}
_SQ_OF_WAVES = {4: (32, 17, 64, 33), 8: (65, 100, 70, 129)}
_SKV_OF_NKTC = {2: (23, 17, 20, 22), 4: (50, 55, 33, 49), 10: (257, 161, 100, 217, 300), 6: (97, 153, 200, 257, 300, 81)}
_SQ_OF_TPW = {(4, 1): (32, 8, 64, 33), (8, 1): (65, 100, 128), (8, 2): (129, 200, 256), (8, 3): (257, 300, 384)}
_BH = ((2, 3), (2, 3), (1, 6), (2, 3), (1, 3))
_P = (0.1, 0.5)


def _cases():
    cs, n = [], 0
    # every mfma cell
    for nkt in NKT_LADDER:
        for dhs in (2, 3, 4):
            for drop in (False, True):
                for waves in (4, 8):
                    Skv, dh, Sq = _pick(_SKV_OF_NKT[nkt], n), _pick(_DH_OF_DHS[dhs], n + n // 4), _pick(_SQ_OF_WAVES[waves], n // 3)
                    layout = _pick(("sep", "kv", "qkv"), n)
                    if layout == "qkv":
                        if (Skv > MFMA_W8_ABOVE_SQ) == (waves == 8):
                            Sq = Skv
                        else:
                            layout = "kv"
                    B, H = _pick(_BH, n)
                    cs.append(Case("fwd", "bf16", _pick((IMPL_AUTO, IMPL_MFMA), n), Sq, Skv, dh, B, H, layout, _pick(_P, n) if drop else 0.0))
                    n += 1
    # every way to the reference kernel
    for dtype, impl, Sq, Skv, dh, layout, p in (
            ("f32", IMPL_AUTO, 33, 50, 40, "kv", 0.0), ("f32", IMPL_AUTO, 70, 257, 88, "sep", 0.1), ("f32", IMPL_AUTO, 17, 289, 12, "sep", 0.5),
            ("f32", IMPL_REF, 32, 100, 64, "sep", 0.0), ("bf16", IMPL_REF, 65, 257, 64, "kv", 0.1), ("bf16", IMPL_REF, 33, 33, 24, "qkv", 0.0),
            ("bf16", IMPL_AUTO, 32, 289, 64, "kv", 0.0), ("bf16", IMPL_AUTO, 17, 300, 96, "sep", 0.5),
            ("bf16", IMPL_AUTO, 33, 50, 12, "sep", 0.0), ("bf16", IMPL_AUTO, 20, 65, 36, "kv", 0.1),
            ("bf16", IMPL_AUTO, 33, 100, 64, "misaligned", 0.0), ("bf16", IMPL_AUTO, 65, 257, 88, "misaligned", 0.5)):
        B, H = _pick(_BH, n)
        cs.append(Case("fwd", dtype, impl, Sq, Skv, dh, B, H, layout, p))
        n += 1
    # every x3 cell
    for dhs in (2, 3, 4):
        *steps, last = X3_LADDER[dhs]
        for nktc in [s[1] for s in steps] + [last]:
            for drop in (False, True):
                for wt in ((4, 1), (8, 1), (8, 2), (8, 3)):
                    Skv, dh, Sq = _pick(_SKV_OF_NKTC[nktc], n), _pick(_DH_OF_DHS[dhs], n + n // 4), _pick(_SQ_OF_TPW[wt], n // 3)
                    layout = _pick(("sep", "kv"), n)
                    B, H = _pick(_BH, n)
                    cs.append(Case("x3", "f32", IMPL_AUTO, Sq, Skv, dh, B, H, layout, _pick(_P, n) if drop else 0.0))
                    n += 1
    # every chunk form of the pairs that can take more than one chunk, plain and dropped
    for nktc, dh in ((10, 64), (10, 88), (6, 128)):
        c = 16 * nktc
        for i, Skv in enumerate((c - 7, 2 * c, c + 57, c + 1, 2 * c + 16, c + 16)):
            cs.append(Case("x3", "f32", IMPL_AUTO, (33, 70)[i % 2], Skv, dh, layout=("kv", "sep")[i % 2], drop_p=(0.0, 0.1, 0.5)[i % 3]))
    cs.append(Case("x3", "f32", IMPL_AUTO, 257, 257, 88, layout="qkv"))            # the vision tower's form: q | k | v fused
    # key counts that are whole tiles: nothing is padded, and a chunk or an image is exactly full
    for i, Skv in enumerate((16, 32, 64, 128, 224)):
        cs.append(Case("fwd", "bf16", IMPL_AUTO, (33, 70)[i % 2], Skv, (64, 88, 128)[i % 3], layout=("sep", "kv")[i % 2], drop_p=(0.0, 0.1)[i % 2]))
    for i, (Skv, dh) in enumerate(((16, 64), (32, 88), (64, 128), (96, 128), (160, 88), (160, 64))):
        cs.append(Case("x3", "f32", IMPL_AUTO, (33, 70)[i % 2], Skv, dh, layout=("sep", "kv")[i % 2], drop_p=(0.0, 0.1)[i % 2]))
    # edge shapes of each kernel
    for entry, dtype, impl in (("fwd", "bf16", IMPL_AUTO), ("fwd", "f32", IMPL_AUTO), ("fwd", "bf16", IMPL_REF), ("x3", "f32", IMPL_AUTO)):
        cs.append(Case(entry, dtype, impl, 1, 50, 64, layout="kv"))                # one query
        cs.append(Case(entry, dtype, impl, 1, 1, 64, B=1, H=6))
        cs.append(Case(entry, dtype, impl, 33, 1, 88))                             # one key: the output is the V row
        cs.append(Case(entry, dtype, impl, 17, 20, 8, drop_p=0.1))                 # the smallest head
        cs.append(Case(entry, dtype, impl, 48, 48, 128, B=1, H=3, layout="qkv"))   # whole tiles on both sides, the largest head
        cs.append(Case(entry, dtype, impl, 33, 257, 64, layout="kv", peak=PEAK_OVERFLOW))
        cs.append(Case(entry, dtype, impl, 65, 100, 88, drop_p=0.1, peak=PEAK_OVERFLOW))
    cs.append(Case("fwd", "bf16", IMPL_AUTO, 16, 288, 128, B=1, H=3, layout="kv"))                        # the mfma limit at the largest head
    cs.append(Case("fwd", "bf16", IMPL_AUTO, 16, 289, 128, B=1, H=3, layout="kv"))                        # one key more: AUTO falls to ref
    cs.append(Case("x3", "f32", IMPL_AUTO, 384, 161, 96, B=1, H=3, drop_p=0.1))                           # the x3 limit of S_q
    return cs


CASES = _cases()
MFMA_CASES = [c for c in CASES if c.kernel == "mfma"]
REF_CASES = [c for c in CASES if c.kernel == "ref"]
X3_CASES = [c for c in CASES if c.kernel == "x3"]


def _groups():
    """The GPU test's items: (kernel, id, cases).  One item per key-tile count of the mfma kernel, per (chunk, head-dim) pair of the
    x3 kernel, and one for the reference kernel, so that the suite grows by a handful of items and not by one per case.  An id spells
    the cells of its item as a product: 'mfma-N4-D2.3.4-plain.drop-w4.w8' holds the 12 cells N4 x {D2, D3, D4} x {plain, drop} x
    {w4, w8}, and test_cross_attention_cells_cpu.py asserts that the item's cases reach every member of that product."""
    out = []
    dots = lambda xs: ".".join(str(x) for x in sorted(set(xs)))                    # noqa: E731
    drops = lambda cs, i: ".".join(n for n, d in (("plain", False), ("drop", True)) if any(c.cell[i] == d for c in cs))   # noqa: E731
    for n in NKT_LADDER:
        cs = [c for c in MFMA_CASES if c.cell[1] == n]
        out.append(("mfma", f"mfma-N{n}-D{dots(c.cell[2] for c in cs)}-{drops(cs, 3)}-w{dots(c.cell[4] for c in cs)}", cs))
    out.append(("ref", "ref-" + ".".join(f"{d}:{r}" for d, r in sorted({c.cell[1:] for c in REF_CASES})), REF_CASES))
    for n, d in sorted({c.cell[1:3] for c in X3_CASES}, key=lambda k: (k[1], k[0])):
        cs = [c for c in X3_CASES if c.cell[1:3] == (n, d)]
        wt = ".".join(f"w{w}t{t}" for w, t in sorted({c.cell[4:6] for c in cs}))
        forms = ".".join(f.replace(" ", "_") for f in CHUNK_FORMS if any(c.cell[6] == f for c in cs))
        out.append(("x3", f"x3-N{n}-D{d}-{drops(cs, 3)}-{wt}-{forms}", cs))
    return out


GROUPS = _groups()


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _loud(rows, cols):
    r, c = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    return torch.where((r + c) % 2 == 0, LOUD, -LOUD).double()


class Inputs:
    """host buffers of a case.  bufs: {name: 2-D tensor in the case's dtype}; operand x in 'qkv': (buffer name, first column, row
    stride); q / k / v: the live values [B, S, D] in the case's dtype; dominant [B, H, Sq]: the dominant key of a peaky row, -1 for a
    flat row; ldo: the output's row stride"""


def build(c, poison=False):
    """poison: NaN instead of +-LOUD around the live values (the live values are the same)"""
    B, H, Sq, Skv, dh = c.B, c.H, c.Sq, c.Skv, c.dh
    D = H * dh
    g = torch.Generator().manual_seed(zlib.crc32(c.shape.encode()))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    T = c.boundary_keys()
    nT = len(T)
    assert nT < dh, "the boundary keys need a span of their own inside the head"
    # keys: boundary keys orthogonal with norm sqrt(dh); the others randn with OTHER_IN_SPAN of their component inside that span
    basis, _ = torch.linalg.qr(rnd(B, H, dh, nT))                           # [B, H, dh, nT], orthonormal columns
    k = rnd(B, H, Skv, dh)
    inside = (k @ basis) @ basis.transpose(-1, -2)
    k = k - (1.0 - OTHER_IN_SPAN) * inside
    k[:, :, T, :] = basis.transpose(-1, -2) * dh ** 0.5
    v = rnd(B, H, Skv, dh) + 0.5 * ((torch.arange(Skv) % 7) - 3.0)[None, None, :, None]
    # queries
    i = torch.arange(Sq)
    flat = i % 3 == 2
    nth = torch.cumsum((~flat).long(), 0) - 1                               # the how-many-th peaky row
    bh = torch.arange(B * H).view(B, H, 1)
    which = (nth.view(1, 1, Sq) + bh) % nT
    dom = torch.tensor(T)[which]                                            # [B, H, Sq]
    dom = torch.where(flat.view(1, 1, Sq), -1, dom)
    kd = torch.gather(k, 2, dom.clamp(min=0)[..., None].expand(B, H, Sq, dh))
    peaky = 0.5 * rnd(B, H, Sq, dh) + kd * (c.peak * dh ** 0.5) / (kd * kd).sum(-1, keepdim=True)
    q = torch.where(flat.view(1, 1, Sq, 1), 0.8 * rnd(B, H, Sq, dh), peaky)
    t = tdt(c.dtype)
    r = Inputs()
    r.q, r.k, r.v = (_merge(x).to(t) for x in (q, k, v))
    r.dominant, r.boundary = dom, T
    # buffers
    lay = c.layout
    r.ldo = D + 8
    if lay == "qkv":
        ld = 3 * D + 24
        where = {"q": ("qkv", 0, ld), "k": ("qkv", D, ld), "v": ("qkv", 2 * D, ld)}
        rows = {"qkv": B * Sq}
    elif lay == "kv":
        ld = 2 * D + 24
        where = {"q": ("q", 0, D + 16), "k": ("kv", 0, ld), "v": ("kv", D, ld)}
        rows = {"q": B * Sq, "kv": B * Skv}
    else:
        where = {"q": ("q", 0, D + 16), "k": ("k", 0, D + (20 if lay == "misaligned" else 24)), "v": ("v", 0, D + 40)}
        rows = {"q": B * Sq, "k": B * Skv, "v": B * Skv}
    r.where, r.bufs = where, {}
    for name, (buf, col, ld) in where.items():
        if buf not in r.bufs:
            r.bufs[buf] = (_loud(rows[buf] + SLACK, ld) * (float("nan") if poison else 1.0)).to(t)
        live = getattr(r, name)
        r.bufs[buf][:live.shape[0] * live.shape[1], col:col + D] = live.reshape(-1, D)
    return r


def dominance(c, inp):
    """(the smallest lead of a dominant key over its row's runner-up, in score; the boundary keys no row of some block has as its
    dominant key) on the inputs as the kernel gets them"""
    s = scores(inp.q, inp.k, c.H, c.scale)
    dom = inp.dominant
    pk = dom >= 0
    if not bool(pk.any()):
        return float("inf"), []
    top = torch.gather(s, 3, dom.clamp(min=0)[..., None])[..., 0]
    rest = s.scatter(3, dom.clamp(min=0)[..., None], float("-inf")).amax(-1) if c.Skv > 1 else torch.full_like(top, float("-inf"))
    lead = float((top - rest)[pk].min())
    missing = []
    want = min(len(inp.boundary), int(pk[0, 0].sum()))
    for b in range(c.B):
        for h in range(c.H):
            have = set(dom[b, h][pk[b, h]].tolist())
            if len(have) < want:
                missing.append((b, h, sorted(set(inp.boundary) - have)))
    return lead, missing


def case_mask(c):
    return drop_multiplier(c.seed, c.B * c.H, c.Sq, c.Skv, c.drop_p)


# ---- bounds -------------------------------------------------------------------------------------------------------------------
# worst error of emulate() against cross_ref() over the case list, (per block, per row), measured by test_cross_attention_cells_cpu.py,
# which asserts that each figure here is at or above what it measures and within 1.25x of it
EMULATED = {
    "mfma": (5.3e-3, 6.5e-3),          # observed on an MI355X: 5.3e-3, 6.4e-3
    "x3": (1.9e-5, 2.0e-5),            # observed 1.9e-5, 2.7e-5
    "ref_f32": (1.2e-6, 1.3e-6),       # observed 1.3e-6, 1.3e-6 (bf16: 3.7e-3, 3.7e-3, the output rounding)
}
MFMA_CAP = 1e-2            # the forward cap of tests/test_attention_cells_gpu.py
MFMA_HEADROOM = 1.5        # the rounding model must stay this far under the cap
X3_CAP = 1e-4
REF_F32_CAP = 2e-5         # the fp32 forward bound of tests/test_attention_cells_gpu.py
MARGIN = 4.0


def bound(c):
    """(per block, per row) bound of a case's kernel"""
    if c.kernel == "mfma":
        return MFMA_CAP, MFMA_CAP
    if c.kernel == "x3":
        return tuple(min(MARGIN * e, X3_CAP) for e in EMULATED["x3"])
    f32 = tuple(min(MARGIN * e, REF_F32_CAP) for e in EMULATED["ref_f32"])
    return f32 if c.dtype == "f32" else tuple(2.0 ** -8 + e for e in f32)


def bound_key(c):
    return c.kernel if c.kernel != "ref" else "ref_" + c.dtype


# ---- calls that must be refused before any launch ---------------------------------------------------------------------------
# (name, entry, overrides of the valid base call BASE[entry]).  Overrides: a shape / p / impl / dtype value, ld<x> = a row stride as
# an offset from H dh, off<x> = elements the operand's pointer is moved by
BASE = {"x3": dict(dtype="f32", impl=IMPL_AUTO, B=2, H=3, Sq=33, Skv=50, dh=64, drop_p=0.0),
        "fwd": dict(dtype="bf16", impl=IMPL_MFMA, B=2, H=3, Sq=33, Skv=50, dh=64, drop_p=0.0)}
REJECTED = (
    ("x3: dh % 8 != 0", "x3", dict(dh=12)),
    ("x3: dh > 128", "x3", dict(dh=136)),
    ("x3: S_q > 384", "x3", dict(Sq=385)),
    ("x3: q stride below H dh", "x3", dict(ldq=-8)),
    ("x3: k stride below H dh", "x3", dict(ldk=-8)),
    ("x3: v stride below H dh", "x3", dict(ldv=-8)),
    ("x3: out stride below H dh", "x3", dict(ldo=-8)),
    ("x3: q pointer off 16 bytes", "x3", dict(offq=1)),
    ("x3: k pointer off 16 bytes", "x3", dict(offk=2)),
    ("x3: v pointer off 16 bytes", "x3", dict(offv=3)),
    ("x3: plane pointer off 8 bytes", "x3", dict(offo=1)),
    ("x3: q stride no multiple of 4", "x3", dict(ldq=2)),
    ("x3: k stride no multiple of 4", "x3", dict(ldk=6)),
    ("x3: out stride no multiple of 4", "x3", dict(ldo=2)),
    ("x3: drop_p = 1", "x3", dict(drop_p=1.0)),
    ("x3: bf16 operands", "x3", dict(dtype="bf16")),
    ("fwd: forced MFMA, S_kv = 289", "fwd", dict(Skv=289)),
    ("fwd: forced MFMA, S_kv = 300", "fwd", dict(Skv=300)),
    ("fwd: forced MFMA, dh % 8 != 0", "fwd", dict(dh=12)),
    ("fwd: forced MFMA, k pointer off 16 bytes", "fwd", dict(offk=4)),
    ("fwd: forced MFMA, v stride no multiple of 16 bytes", "fwd", dict(ldv=12)),
    ("fwd: forced MFMA, out pointer off 8 bytes", "fwd", dict(offo=2)),
)
