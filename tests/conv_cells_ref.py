"""Float64 references, the restated host dispatch, the case lists, the input builders and the error model for the depthwise-conv,
BatchNorm, pooling / squeeze-excitation and layout kernels of csrc/conv.hip.  Plain torch: nothing of the GPU library is imported
but its constants.  tests/test_conv_cells_cpu.py checks this module on the CPU; tests/test_conv_cells_gpu.py drives every case
through the C ABI.

Out of scope:
  * the 64-bit-index instantiations (`uint64_t` variants, `small32 == false`): they need tensors of 2^31 elements;
  * the opt-in flat BatchNorm forms behind mmrca_bn_flat_set: off in the product, and test_conv_gpu.py / test_mobilenet_v3_gpu.py
    already hold them tightly against the slice forms;
  * mmrca_se_mlp_*, im2row / col2im and conv_igemm.hip: they have shape-swept tests of their own;
  * the existing tests: they stay as they are.
A workspace pointer that is not 16-byte aligned (it then counts as absent) is not run either: every workspace here is aligned.

cell(case) names the kernel instantiation(s) the host code launches for the call, one per launch, and the grid quantities that
decide the edges (col_grid's branch / nblk / per, the depthwise slices / nranges / lanes, BN_R, the activation code); SOURCE_PINS
are the host lines it restates, as they stand in conv.hip.

Inputs expose what randn hides.  BatchNorm x: a per-channel mean of several sigma with mixed signs, channel 1 nearly constant
(variance << eps), channel 2 with three rows 300 sigma out; dy with a per-channel offset, so the train-mode terms sum_du / rows
and sum_duxh / rows are of the order of du; gamma of mixed signs with an exact zero (channel 4), beta of mixed signs.  Channel 3
of the apply / backward cases is normalised with mean 0, rstd 1, gamma 1, beta 0, so u == x exactly, and x walks over the kinks
(-3, 0, 3): the reference uses the conventions of act_grad_f there (relu' (0) = 0, hardswish' (-3) = 0, hardswish' (3) = 1,
hardsigmoid' (+-3) = 0).  Everywhere else the builder moves x off the kinks (|u - kink| >= 2^-7 max(1, |u|) in bf16, 2^-20 in
fp32); elements still inside that band are left out of the elementwise comparison and enter the sums' bounds with their whole
jump, and their share is asserted to be at most 0.5 % per case.

Tie rule of the max pooling: maxpool3x3s2_fwd_k scans the window row by row with `v > best`, so the FIRST maximum in (ky, kx) order
takes the gradient -- the rule of torch's max_pool2d; the reference scans in the same order and the inputs are small integers, so
nearly every window has ties.

Bounds (elementwise, in units; K per key in BOUND):
  T-typed outputs (y, dx, pooled, ds, out) ... |err| <= K * (ulp_T(|ref|) / 2 + 2^-24 * M) + X
  fp32 sums (+= outputs, statistics) ......... |err| <= K * 2^-24 * (|prefill| + sum |addend|) + X
M = the sum of the absolute values of the terms of the expression; X = explicit terms outside K:
  * the approximate intrinsics (sigmoid_f = rcp(1 + __expf(-u)), rsqrtf): |y| * (EXPF_ULP + RCP_ULP + 1.5 |u|) * 2^-23 for SiLU /
    sigmoid and their derivatives, 2 * RSQRT_ULP * 2^-23 * (var + eps) for the rstd-implied variance.  The ulp figures are those of
    the HIP math API tables (__expf 1, rsqrtf 1, hardware reciprocal 1: also the claim in conv.hip:22), doubled; the HIP
    documentation is not shipped with the toolchain this was written against, so they are an ASSUMPTION.  The |u| term is the
    rounding of the exponent u * log2(e), which no ulp figure of the result covers;
  * first order in the kernel's own fp32 statistics (mean / rstd of bn_act_fwd_fin, the two sums of the backward), which are
    bounded themselves: |gamma| (|d mean| rstd + |xhat| |d rstd| / rstd), |gamma rstd| (|d sum_du| + |xhat| |d sum_duxh|) / rows;
  * for the sums of the backward, the jump of act' at every element inside the kink band;
  * for the column sums that col_grid lays out (statistics, moments, the backward's two sums), the worst case of the kernels'
    chains of dependent additions -- ceil(per / lanes) per thread, then nblk atomics on one address: chain_x() below.  The first
    run on the MI355X exceeded the K-only bound exactly there (a mean over 983,077 rows in 2,048 blocks: 377 units on the
    near-constant channel, 2.2e-5 relative): same-signed near-equal addends round the same way at every step, which the float32
    reference in chunks of 256 rows does not do.  It is a property of fp32 accumulation in this order, not an indexing error, and the
    variance it feeds is centred on the same mean (the bound carries that error as dm^2, or 2 |d1| dm + dm^2 for the one-pass form).
The one-pass bf16 moments sum d = x - shift and d^2, shift = the trimmed mean of 16 sampled rows (bn_shift_row / bn_trimmed,
restated here and compared bitwise with the shift mmrca_bn_moments returns).

K = max(4, 4 * worst error of the same formula evaluated in plain torch float32 on the CPU over the whole case list), in the
bound's unit (four times the reference's own error).  Measured by test_conv_cells_cpu.py, which asserts
that BOUND covers what it measures; the values observed on the MI355X stand next to them.

Row counts of the BatchNorm statistics on col_grid's 256-row branch: `per >= 480` needs rows >= cap * 480, i.e. > 100 MB of
input for every C >= 70 (C = 72: 737,280 rows), against the 16 MB limit of this suite.  C = 8 runs it (983,077 rows, 15.7 MB in
bf16); the other C run the 256-row branch with a ragged `per` in (256, 480): the eight-rows-in-flight loop (r + 224 < r1) runs
once for every row lane and the 32-row tail after it for some.
"""
import math

import torch
import torch.nn.functional as F

from garbage_classification_rca_amd.lib import BF16, F32  # noqa: F401  (constants only)

U = 2.0 ** -24
SENT = -3072.0
LOUD = 8192.0
GUARD = 8
EPS = 1e-3
NONE, SILU, RELU, SIGMOID, HSWISH, HSIGMOID = range(6)
ACTS = (NONE, SILU, RELU, SIGMOID, HSWISH, HSIGMOID)
EXPF_ULP, RCP_ULP, RSQRT_ULP = 2.0, 2.0, 2.0
# host constants of conv.hip (pinned by SOURCE_PINS)
DW_FLAT_THREADS, DW_WG_BLOCKS, DW5_WG_THREADS, DW5_WG_MIN_GROUPS, DW5_RED_CHUNKS, BN_R, BN_SHIFT_ROWS = 65536, 768, 256 * 4 * 4 * 64, 32, 16, 4, 16

# K per (output kind, dtype) = max(4, 4 x the float32 reference's worst error over the case list, rounded up to a half); both
# measured values next to it
BOUND = {
    ("bn_dx", "bf16"): 4.5,   # float32 reference 1; observed on the MI355X 1
    ("bn_dx", "f32"): 11.0,  # float32 reference 2.63; observed on the MI355X 2.43
    ("bn_mean", "bf16"): 4.5,   # float32 reference 1.08; observed on the MI355X 1.21
    ("bn_mean", "f32"): 4.0,   # float32 reference 0; observed on the MI355X 0
    ("bn_run", "bf16"): 8.0,   # float32 reference 1.84; observed on the MI355X 1.75
    ("bn_run", "f32"): 8.5,   # float32 reference 2.04; observed on the MI355X 1.69
    ("bn_s", "bf16"): 4.0,   # float32 reference 0; observed on the MI355X 0
    ("bn_sums", "bf16"): 4.5,   # float32 reference 1; observed on the MI355X 1
    ("bn_sums", "f32"): 4.5,   # float32 reference 0.999; observed on the MI355X 0.994
    ("bn_var", "bf16"): 4.0,   # float32 reference 0.553; observed on the MI355X 0.62
    ("bn_var", "f32"): 4.0,   # float32 reference 0; observed on the MI355X 0
    ("bn_y", "bf16"): 4.5,   # float32 reference 1; observed on the MI355X 1
    ("bn_y", "f32"): 8.0,   # float32 reference 1.95; observed on the MI355X 1.77
    ("colsum", "bf16"): 10.0,  # float32 reference 2.42; observed on the MI355X 2.25
    ("colsum", "f32"): 8.0,   # float32 reference 1.93; observed on the MI355X 2.46
    ("dw_dw", "bf16"): 7.0,   # float32 reference 1.65; observed on the MI355X 1.78
    ("dw_dw", "f32"): 16.0,  # float32 reference 3.87; observed on the MI355X 2.38
    ("dw_dx", "bf16"): 4.5,   # float32 reference 1; observed on the MI355X 1
    ("dw_dx", "f32"): 13.5,  # float32 reference 3.28; observed on the MI355X 3.24
    ("dw_y", "bf16"): 4.5,   # float32 reference 1; observed on the MI355X 1
    ("dw_y", "f32"): 14.0,  # float32 reference 3.35; observed on the MI355X 3.31
    ("ew", "bf16"): 4.5,   # float32 reference 1; observed on the MI355X 1
    ("ew", "f32"): 6.0,   # float32 reference 1.41; observed on the MI355X 1.35
    ("pool", "bf16"): 4.5,   # float32 reference 1; observed on the MI355X 1
    ("pool", "f32"): 9.0,   # float32 reference 2.14; observed on the MI355X 2.39
}


def cdiv(a, b):
    return -(-a // b)


def tdt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def ulp(v, t):
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - (7 if t == torch.bfloat16 else 23))


class Case:
    """one call: fam 'dw' | 'stats' | 'fwd' | 'bwd' | 'pool' | 'layout'; absent options read as None"""

    def __init__(self, fam, op, dtype, **kw):
        self.__dict__.update(fam=fam, op=op, dtype=dtype, **kw)
        self._keys = tuple(kw)

    def __getattr__(self, k):
        if k.startswith("_"):
            raise AttributeError(k)
        return None

    def __repr__(self):
        o = [self.op, self.dtype]
        for k in self._keys:
            v = getattr(self, k)
            if v is None or v is False:
                continue
            o.append(k if v is True else f"{k}{v}")
        return "-".join(o)


# ------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ------------------------------------------------------------------------------------------------------
SOURCE_PINS = (
    "static bool dw_v8_ok(int C, int dtype, const void* a, const void* b, const void* c) { return dtype == MMRCA_BF16 && C % 8 == 0 && "
    "((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0; }",
    "static bool bn_v8_ok(int C, int dtype, const void* a, const void* b, const void* c, const void* d) { return dtype == MMRCA_BF16 && "
    "C % 8 == 0 && ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0; }",
    "static bool pool_v8_ok(int C, int dtype, const void* a, const void* b, const void* c, const void* d) { return dtype == MMRCA_BF16 && "
    "C % 8 == 0 && ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0; }",
    "static bool se_v8_ok(int C, int dtype, const void* a, const void* b, const void* c) { return dtype == MMRCA_BF16 && C % 8 == 0 && "
    "((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0; }",
    "static const int DW_FLAT_THREADS = 65536;", "static const int DW_WG_BLOCKS = 768;",
    "static const int64_t DW5_WG_THREADS = 256 * 4 * 4 * 64;", "constexpr int64_t DW5_WG_MIN_GROUPS = 32;",
    "constexpr int DW5_RED_CHUNKS = 16;", "#define BN_R 4", "#define BN_SHIFT_ROWS 16",
    # depthwise 3x3
    "const bool small32 = (int64_t)B * H * W * C * 2 < (1ll << 32);",
    "if (dw_v8_ok(C, dtype, x, w, y) && stride == 1 && small32) {",
    "if (dx && dw_v8_ok(C, dtype, dy, w, dx) && stride == 1 && small32) {", "} else if (dx && dw_v8_ok(C, dtype, dy, w, dx)) {",
    "const int64_t cslices = (C + 63) / 64; int64_t nblk = npix / 32 > 0 ? npix / 32 : 1; "
    "if (nblk > 2048 / cslices) nblk = 2048 / cslices > 0 ? 2048 / cslices : 1; const int64_t per = (npix + nblk - 1) / nblk;",
    "if (dw_v8_ok(C, dtype, dy, x, dw) && stride == 1 && small32) {",
    "const int64_t ngrp = (int64_t)B * H * ((W + 3) / 4); const int slices = (C / 8 + 63) / 64;",
    "const int64_t row_bytes = (int64_t)slices * 4608 * 4;",
    "const bool use_ws = ws && (((uintptr_t)ws) & 15) == 0 && ws_bytes >= 8 * row_bytes; int64_t nb = DW_WG_BLOCKS / slices; "
    "if (use_ws && nb > ws_bytes / row_bytes) nb = ws_bytes / row_bytes; if (nb > ngrp / 8) nb = ngrp / 8 > 0 ? ngrp / 8 : 1; "
    "const int64_t gper = (ngrp + nb - 1) / nb; const unsigned nranges = (unsigned)((ngrp + gper - 1) / gper);",
    "int64_t lanes = (int64_t)DW_FLAT_THREADS / C8; const int64_t ngrp_f = (int64_t)B * ((H + 1) / 2) * ((W + 3) / 4);",
    "if (lanes > ngrp_f) lanes = ngrp_f; if (ws && lanes * C8 * 72 * 4 > ws_bytes) lanes = ws_bytes / (C8 * 72 * 4); "
    "if (ws && (((uintptr_t)ws) & 15) == 0 && lanes >= 64) {",
    "} else if (use_ws) {",
    # depthwise 5x5
    "static bool dw5_small32(int B, int H, int W, int C) { return (int64_t)B * H * W * C < (1ll << 31); }",
    "const int n = C * 25; const int64_t part_bytes = (int64_t)DW5_RED_CHUNKS * n * 4; const bool ws_ok = ws && (((uintptr_t)ws) & 15) == 0;",
    "const int64_t C8 = C / 8, ngrp = (int64_t)B * Ho * ((Wo + 3) / 4); int64_t lanes = DW5_WG_THREADS / (5 * C8); "
    "if (lanes > ngrp / DW5_WG_MIN_GROUPS) lanes = ngrp / DW5_WG_MIN_GROUPS; if (lanes < 1) lanes = 1; "
    "const bool use_ws = ws_ok && ws_bytes >= part_bytes + (int64_t)n * 4; "
    "if (use_ws && lanes * n * 4 > ws_bytes - part_bytes) lanes = (ws_bytes - part_bytes) / ((int64_t)n * 4); "
    "if (!use_ws && lanes > 64) lanes = 64;",
    "const int64_t npix = (int64_t)B * Ho * Wo, cslices = (C + 63) / 64; int64_t nblk = npix / 32 > 0 ? npix / 32 : 1; "
    "if (nblk > 2048 / cslices) nblk = 2048 / cslices > 0 ? 2048 / cslices : 1; "
    "const bool use_ws = ws_ok && ws_bytes >= part_bytes + (int64_t)n * 4; "
    "if (use_ws && nblk * n * 4 > ws_bytes - part_bytes) nblk = (ws_bytes - part_bytes) / ((int64_t)n * 4); "
    "const int64_t per = (npix + nblk - 1) / nblk; nblk = (npix + per - 1) / per;",
    # col_grid
    "const int64_t slices = (C + 63) / 64; int64_t cap = 3072 / slices; if (cap < 8) cap = 8; if (cap > 2048) cap = 2048; "
    "int64_t nblk = rows / 256 > 0 ? rows / 256 : 1; if (nblk > cap) nblk = cap; if (nblk * slices < 512) {",
    "nblk = rows / 32 > 0 ? rows / 32 : 1;", "if (nblk * slices > 1024) nblk = 1024 / slices > 0 ? 1024 / slices : 1; } "
    "*per = (rows + nblk - 1) / nblk;",
    # the statistics
    "if (dtype == MMRCA_BF16 && C % 8 == 0 && ld % 8 == 0 && (((uintptr_t)x) & 15) == 0) {",
    "if (!(dtype == MMRCA_BF16 && C % 8 == 0 && ld % 8 == 0 && (((uintptr_t)x) & 15) == 0))",
    "const int64_t seg = rows / BN_SHIFT_ROWS; if (seg <= 0) return k < rows ? k : rows - 1; "
    "return (int64_t)k * seg + (int64_t)((2654435761u * (unsigned)(k + 1)) % (unsigned long long)seg);",
    "__device__ __forceinline__ float bn_trimmed(float sum, float lo, float hi) { return (sum - lo - hi) * (1.0f / (BN_SHIFT_ROWS - 2)); }",
    "for (; r + 224 < r1; r += 256) {",
    # apply / backward
    "if (bn_v8_ok(C, dtype, x, y, gamma, beta) && ((((uintptr_t)mean) | ((uintptr_t)rstd)) & 15) == 0) {",
    "if (!(bn_v8_ok(C, dtype, x, out, gamma, beta) && ((((uintptr_t)mean) | ((uintptr_t)rstd) | ((uintptr_t)res)) & 15) == 0))",
    "if (!(bn_v8_ok(C, dtype, x, y, gamma, beta) && ((((uintptr_t)s1) | ((uintptr_t)s2) | ((uintptr_t)shift) | ((uintptr_t)res)) & 15) == 0))",
    "else if (sizeof(T) == 2 && C % 8 == 0 && ((((uintptr_t)dy) | ((uintptr_t)x)) & 15) == 0)",
    "const bool v8 = dx && bn_v8_ok(C, dtype, dy, x, dx, gamma) && "
    "((((uintptr_t)mean) | ((uintptr_t)rstd) | ((uintptr_t)scratch) | ((uintptr_t)beta)) & 15) == 0;",
    "if (dgamma && dbeta && !dx) hipLaunchKernelGGL(bn_param_grads_k,",
    # pooling / squeeze-excitation / residual
    "if (pool_v8_ok(C, dtype, x, x, x, x)) {", "if (se_v8_ok(C, dtype, dpool, dx, dx)) {", "if (se_v8_ok(C, dtype, x, s, y)) {",
    "if (pool_v8_ok(C, dtype, dy, x, s, dx)) {", "if (!(pool_v8_ok(C, dtype, dy, s, dpool, dx) && (!z || ((((uintptr_t)z) & 15) == 0))))",
    "if (dtype == MMRCA_BF16 && per_sample % 8 == 0 && ((((uintptr_t)a) | ((uintptr_t)branch) | ((uintptr_t)out)) & 15) == 0) {",
    "if (v > best) { best = v; bt = ky * 3 + kx; }",
)


def col_grid(rows, C):
    """(branch, nblk, per) of conv.hip::col_grid; branch = the row count a block was sized for (256 | 32)"""
    slices = cdiv(C, 64)
    cap = min(max(3072 // slices, 8), 2048)
    nblk = min(max(rows // 256, 1), cap)
    branch = 256
    if nblk * slices < 512:
        branch = 32
        nblk = max(rows // 32, 1)
        if nblk * slices > 1024:
            nblk = max(1024 // slices, 1)
    per = cdiv(rows, nblk)
    return branch, cdiv(rows, per), per


def _T(c):
    return "bf16_t" if c.dtype == "bf16" else "float"


def _v8(c, *operands):
    """the v8 predicates: bf16, C % 8 == 0 and none of the named operands misaligned"""
    return c.dtype == "bf16" and c.C % 8 == 0 and c.mis not in operands


def dw_out(c):
    return (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1


def _dw_pix(c):
    Ho, Wo = dw_out(c)
    npix = c.B * Ho * Wo
    cslices = cdiv(c.C, 64)
    nblk = max(npix // 32, 1)
    if nblk > 2048 // cslices:
        nblk = max(2048 // cslices, 1)
    return npix, cslices, nblk


def dw3_plan(c, ws_bytes):
    """the stride-1 bf16 weight gradient of the 3x3: (form, slices, nranges, lanes)"""
    ngrp = c.B * c.H * cdiv(c.W, 4)
    slices = cdiv(c.C // 8, 64)
    row_bytes = slices * 4608 * 4
    use_ws = ws_bytes is not None and ws_bytes >= 8 * row_bytes
    nb = DW_WG_BLOCKS // slices
    if use_ws and nb > ws_bytes // row_bytes:
        nb = ws_bytes // row_bytes
    if nb > ngrp // 8:
        nb = max(ngrp // 8, 1)
    gper = cdiv(ngrp, nb)
    nranges = cdiv(ngrp, gper)
    C8 = c.C // 8
    lanes = min(DW_FLAT_THREADS // C8, c.B * cdiv(c.H, 2) * cdiv(c.W, 4))
    if ws_bytes is not None and lanes * C8 * 288 > ws_bytes:
        lanes = ws_bytes // (C8 * 288)
    form = "flat" if ws_bytes is not None and lanes >= 64 else ("strip" if use_ws else "none")
    return form, slices, nranges, lanes


def dw5_plan(c, ws_bytes, v8):
    """the 5x5 weight gradient: (workspace used, lanes or pixel ranges)"""
    Ho, Wo = dw_out(c)
    n = c.C * 25
    part = DW5_RED_CHUNKS * n * 4
    use_ws = ws_bytes is not None and ws_bytes >= part + n * 4
    if v8:
        ngrp = c.B * Ho * cdiv(Wo, 4)
        lanes = max(min(DW5_WG_THREADS // (5 * (c.C // 8)), ngrp // DW5_WG_MIN_GROUPS), 1)
        if use_ws and lanes * n * 4 > ws_bytes - part:
            lanes = (ws_bytes - part) // (n * 4)
        if not use_ws and lanes > 64:
            lanes = 64
        return use_ws, lanes
    npix, _, nblk = _dw_pix(c)
    if use_ws and nblk * n * 4 > ws_bytes - part:
        nblk = (ws_bytes - part) // (n * 4)
    per = cdiv(npix, nblk)
    return use_ws, cdiv(npix, per)


def dw_ws_bytes(c):
    """the workspace size that selects the form c.ws asks for (None: no workspace; -1: the form cannot be selected at this shape)"""
    if c.ws in (None, "none"):
        return None
    if c.k == 3:
        if not (_v8(c, "dy", "x") and c.stride == 1):
            return 1 << 16                                   # ignored by the kernels that run
        C8, slices = c.C // 8, cdiv(c.C // 8, 64)
        lanes0 = min(DW_FLAT_THREADS // C8, c.B * cdiv(c.H, 2) * cdiv(c.W, 4))
        if c.ws == "flat":
            return lanes0 * C8 * 288 if lanes0 >= 64 else -1
        # as many rows as keep the streaming form out (lanes < 64), at least the 8 that use_ws asks for
        b = max(8 * slices * 18432, 64 * C8 * 288 - 16) if lanes0 >= 64 else 16 * slices * 18432
        return b if dw3_plan(c, b)[0] == "strip" else -1
    n = c.C * 25
    part = DW5_RED_CHUNKS * n * 4
    full = dw5_plan(c, 1 << 40, _v8(c, "dy", "x"))[1]
    return {"full": part + full * n * 4, "low": part + max(full // 2, 1) * n * 4, "small": part + n * 4 - 16}[c.ws]


def cell(c, ws_bytes="auto"):
    """(kernel names, one per launch; grid quantities)"""
    T, f = _T(c), c.fam
    if f == "dw":
        if ws_bytes == "auto":
            ws_bytes = dw_ws_bytes(c)
        k, s = c.k, c.stride
        if c.op == "fwd":
            if k == 3:
                if _v8(c, "x", "w", "y"):
                    return ("dw3x3_s1_strip2_v8_k<false>" if s == 1 else "dwconv3x3_fwd_v8_k",), {}
                return (f"dwconv3x3_fwd_k<{T}>",), {}
            return ((f"dw5x5_fwd_v8_k<{s},false,unsigned>" if _v8(c, "x", "w", "y") else f"dwconv5x5_fwd_k<{T}>"),), {}
        names, q = [], {}
        if c.form in ("dx", "both"):
            v8 = _v8(c, "dy", "w", "dx")
            if k == 3:
                names.append(("dw3x3_s1_strip2_v8_k<true>" if s == 1 else "dwconv3x3_bwd_data_v8_k") if v8 else f"dwconv3x3_bwd_data_k<{T}>")
            else:
                names.append(("dw5x5_fwd_v8_k<1,true,unsigned>" if s == 1 else "dw5x5_s2_data_v8_k<unsigned>") if v8 else f"dwconv5x5_bwd_data_k<{T}>")
        if c.form in ("dw", "both"):
            v8 = _v8(c, "dy", "x")
            npix, cslices, nblk = _dw_pix(c)
            if k == 3:
                if v8 and s == 1:
                    form, slices, nranges, lanes = dw3_plan(c, ws_bytes)
                    q.update(form=form, slices=slices, nranges=nranges, lanes=lanes)
                    names += {"flat": ["dwconv3x3_bwd_weight_s1_flat_v8_k<2>", "dw_wg_reduce_k"],
                              "strip": ["dwconv3x3_bwd_weight_s1_strip2_v8_k<1,true>", "dw_wg_reduce_k"],
                              "none": ["dwconv3x3_bwd_weight_s1_strip2_v8_k<1,false>"]}[form]
                else:
                    q.update(nblk=nblk, per=cdiv(npix, nblk), capped=npix // 32 > 2048 // cslices)
                    names.append("dwconv3x3_bwd_weight_v8_k" if v8 else f"dwconv3x3_bwd_weight_k<{T}>")
            else:
                use_ws, lanes = dw5_plan(c, ws_bytes, v8)
                q.update(use_ws=use_ws, lanes=lanes, capped=npix // 32 > 2048 // cslices)
                w = "true" if use_ws else "false"
                names.append(f"dw5x5_wgrad_v8_k<{s},{w},unsigned>" if v8 else f"dwconv5x5_bwd_weight_k<{T},{w}>")
                if use_ws:
                    names += ["dw5_reduce_part_k", "dw5_reduce_fin_k"]
        return tuple(names), q
    if f == "stats":
        branch, nblk, per = col_grid(c.rows, c.C)
        q = dict(branch=branch, nblk=nblk, per=per)
        if c.op == "stats" and not c.train:
            return ("bn_eval_stats_k",), q
        one = c.dtype == "bf16" and c.C % 8 == 0 and c.ld % 8 == 0 and c.mis != "x"
        if c.op == "moments":
            return (("col_moment2_v8_k[shift_out]",) if one else ("REJECT",)), q
        if one:
            return (("col_moment2_v8_k[fin]",) if c.op == "fused" else ("col_moment2_v8_k", "bn_finish_shifted_k")), q
        return (f"col_moment_k<{T},false>", f"col_moment_k<{T},true>", "bn_finish_var_k"), q
    if f == "fwd":
        q = dict(BN_R=BN_R, act=c.act)
        if c.op == "fwd":
            return ((f"bn_act_fwd_v8_k<{c.act}>" if _v8(c, "x", "y", "gamma") else f"bn_act_fwd_k<{T},{c.act}>"),), q
        if not _v8(c, "x", "y", "gamma") or (c.res and c.mis == "res"):
            return ("REJECT",), q
        if c.op == "res":
            return (f"bn_act_fwd_res_v8_k<{c.act}>",), q
        return (f"bn_act_fwd_fin_v8_k<{'true' if c.res else 'false'},{c.act}>",), q
    if f == "bwd":
        branch, nblk, per = col_grid(c.rows, c.C)
        q = dict(branch=branch, nblk=nblk, per=per, BN_R=BN_R, act=c.act)
        names = []
        if c.op == "bwd":
            names.append(f"bn_act_bwd_reduce_v8_k<{c.act}>" if _v8(c, "dy", "x") else f"bn_act_bwd_reduce_k<{T},{c.act}>")
        if not c.nodx:
            names.append(f"bn_act_bwd_apply_v8_k<{c.act}>" if _v8(c, "dy", "x", "dx", "gamma") else f"bn_act_bwd_apply_k<{T},{c.act}>")
        elif not c.noparam:
            names.append("bn_param_grads_k")
        return tuple(names), q
    if f == "pool":
        op = c.op
        if op == "rowpool_mean":
            return (("rowpool_mean_v8_k" if _v8(c, "x") else f"rowpool_mean_k<{T}>"),), {}
        if op == "rowpool_mean_bwd":
            return (("rowpool_mean_bwd_v8_k" if _v8(c, "dpool", "dx") else f"rowpool_mean_bwd_k<{T}>"),), {}
        if op == "se_scale_fwd":
            return (("se_scale_fwd_v8_k" if _v8(c, "x", "s", "y") else f"se_scale_fwd_k<{T}>"),), {}
        if op == "se_scale_bwd":
            return (("se_scale_bwd_v8_k" if _v8(c, "dy", "x", "s", "dx") else f"se_scale_bwd_k<{T}>"),), {}
        if op == "se_dx":
            if not _v8(c, "dy", "s", "dpool", "dx", "z"):
                return ("REJECT",), {}
            return ((f"se_dx_v8_k<true,{c.act}>" if c.bn else "se_dx_v8_k<false,-1>"),), {}
        if op == "bias_act_fwd":
            return (f"bias_act_fwd_k<{T},{c.act}>",), dict(act=c.act)
        if op == "bias_act_bwd":
            return (f"bias_act_bwd_k<{T},{c.act}>",), dict(act=c.act)
        if op == "residual_add":
            v8 = c.dtype == "bf16" and c.per_sample % 8 == 0 and c.mis not in ("a", "branch", "out")
            return (("residual_add_v8_k" if v8 else f"residual_add_k<{T}>"),), {}
    if f == "layout":
        if c.op == "maxpool3x3s2":
            return (f"maxpool3x3s2_fwd_k<{T}>", f"maxpool3x3s2_bwd_k<{T}>"), {}
        return (f"{c.op}_k<{T}>",), {}
    raise ValueError(repr(c))


def all_cells():
    """every kernel name cell() can return over the arguments the entry points accept (32-bit index forms, flat forms off)"""
    out = set()
    for dtype in ("bf16", "f32"):
        for C in (8, 20):
            for mis in (None, "x", "dy", "w", "y", "dx", "gamma", "res", "z", "dpool", "s", "a"):
                for k in (3, 5):
                    for s in (1, 2):
                        out.update(cell(Case("dw", "fwd", dtype, k=k, B=1, H=64, W=64, C=C, stride=s, mis=mis))[0])
                        for ws in ((None, 1 << 30, 147456) if k == 3 else (None, 1 << 30)):
                            out.update(cell(Case("dw", "bwd", dtype, k=k, B=1, H=64, W=64, C=C, stride=s, form="both", mis=mis), ws)[0])
                            out.update(cell(Case("dw", "bwd", dtype, k=k, B=1, H=4, W=4, C=C, stride=s, form="both", mis=mis), ws)[0])
                for op in ("stats", "fused", "moments"):
                    for train in (0, 1):
                        out.update(cell(Case("stats", op, dtype, rows=64, C=C, ld=C, train=train, mis=mis))[0])
                for act in ACTS:
                    for op in ("fwd", "res", "fin"):
                        for res in (False, True):
                            out.update(cell(Case("fwd", op, dtype, rows=64, C=C, act=act, res=res, mis=mis))[0])
                    for op in ("bwd", "sums"):
                        for nodx in (False, True):
                            out.update(cell(Case("bwd", op, dtype, rows=64, C=C, act=act, nodx=nodx, mis=mis))[0])
                    for op in ("bias_act_fwd", "bias_act_bwd"):
                        out.update(cell(Case("pool", op, dtype, B=1, HW=1, C=C, act=act))[0])
                    out.update(cell(Case("pool", "se_dx", dtype, B=1, HW=4, C=C, act=act, bn=True, mis=mis))[0])
                for op in ("rowpool_mean", "rowpool_mean_bwd", "se_scale_fwd", "se_scale_bwd", "se_dx"):
                    out.update(cell(Case("pool", op, dtype, B=1, HW=4, C=C, mis=mis))[0])
                for ps in (8, 20):
                    out.update(cell(Case("pool", "residual_add", dtype, B=1, per_sample=ps, mis=mis))[0])
        for op in ("maxpool3x3s2", "channel_gather", "channel_interleave2", "channel_deinterleave2", "nchw_to_rows"):
            out.update(cell(Case("layout", op, dtype))[0])
    return out


# ------------------------------------------------------------------------------------------------------
# the case lists
# ------------------------------------------------------------------------------------------------------
DW_C = (8, 20, 72, 520, 1032)
DW_HW = ((1, 1), (1, 9), (2, 2), (7, 3), (7, 5), (8, 11), (15, 15))


def _dw_cases():
    cs, i = [], 0
    for k in (3, 5):
        forms_ws = ("none", "flat", "strip") if k == 3 else ("none", "full", "low", "small")
        for dtype in ("bf16", "f32"):
            for stride in (1, 2):
                for C in DW_C:
                    for (H, W) in DW_HW:
                        i += 1
                        B = (1, 3)[i % 2]
                        cs.append(Case("dw", "fwd", dtype, k=k, B=B, H=H, W=W, C=C, stride=stride))
                        c = Case("dw", "bwd", dtype, k=k, B=(3, 1)[i % 2], H=H, W=W, C=C, stride=stride, form=("both", "dx", "dw")[i % 3],
                                 ws=forms_ws[(i // 3) % len(forms_ws)])
                        if dw_ws_bytes(c) == -1:
                            c.ws = "none"
                        cs.append(c)
        # every workspace form of the weight gradient at sizes with more groups than lanes, and the capped pixel ranges
        for C in (8, 72, 520, 1032):
            for ws in forms_ws:
                for stride in (1, 2):
                    c = Case("dw", "bwd", "bf16", k=k, B=3, H=31, W=(37 if C <= 72 else 13), C=C, stride=stride, form="dw", ws=ws)
                    if dw_ws_bytes(c) != -1:
                        cs.append(c)
        cs.append(Case("dw", "bwd", "f32", k=k, B=3, H=15, W=15, C=20, stride=1, form="dw", ws=forms_ws[1]))
        cs.append(Case("dw", "bwd", "f32", k=k, B=3, H=15, W=15, C=20, stride=2, form="dw", ws=forms_ws[-1]))
        # npix / 32 > 2048 / cslices: the capped pixel ranges of the generic and the v8 weight kernels
        cs.append(Case("dw", "bwd", "f32", k=k, B=1, H=257, W=257, C=20, stride=1, form="dw", ws="none"))
        cs.append(Case("dw", "bwd", "bf16", k=k, B=3, H=209, W=209, C=72, stride=2, form="both", ws="none"))
        if k == 5:
            cs.append(Case("dw", "bwd", "bf16", k=k, B=3, H=105, W=105, C=72, stride=1, form="dw", ws="small"))   # lanes capped at 64
            cs.append(Case("dw", "bwd", "bf16", k=k, B=3, H=105, W=105, C=72, stride=1, form="dw", ws="low"))
        # a misaligned operand: bf16, C % 8 == 0, the generic kernels
        for C, (H, W) in ((72, (7, 5)), (520, (8, 11))):
            for stride in (1, 2):
                for mis in ("x", "w", "y"):
                    cs.append(Case("dw", "fwd", "bf16", k=k, B=3, H=H, W=W, C=C, stride=stride, mis=mis))
                for mis in ("dy", "x", "w", "dx"):
                    cs.append(Case("dw", "bwd", "bf16", k=k, B=3, H=H, W=W, C=C, stride=stride, form="both", ws="none", mis=mis))
        # exact integers
        for dtype, C in (("bf16", 72), ("bf16", 520), ("bf16", 20), ("f32", 20)):
            for stride in (1, 2):
                cs.append(Case("dw", "fwd", dtype, k=k, B=3, H=7, W=5, C=C, stride=stride, ints=True))
                for ws in forms_ws:
                    c = Case("dw", "bwd", dtype, k=k, B=3, H=9, W=(37 if C == 72 else 6), C=C, stride=stride, form="both", ws=ws, ints=True)
                    if dw_ws_bytes(c) != -1:
                        cs.append(c)
    return cs


def _rows_for(C, branch):
    """a row count on the given col_grid branch with a ragged last block (256: per > 256, so the eight-in-flight loop runs for every
    row lane and the 32-row tail for some; per >= 480 where that fits 16 MB: C = 8)"""
    slices = cdiv(C, 64)
    if branch == 32:
        rows = 32 * 5 + 13
        assert col_grid(rows, C)[0] == 32
        return rows
    if C == 8:
        return 2048 * 480 + 37
    return 256 * cdiv(512, slices) + max(cdiv(512, slices), 40) + 3


STAT_C = (8, 70, 72, 520, 3840)


def _stats_cases():
    cs, i = [], 0
    for dtype in ("bf16", "f32"):
        for C in STAT_C:
            rows_list = [1, 2, 31, 33, 255, 257, _rows_for(C, 32), _rows_for(C, 256)]
            for rows in rows_list:
                big = rows > 1000
                if big and dtype == "f32" and C == 3840:
                    continue                       # 35 MB in fp32; the generic kernels run this branch at C = 520 and in bf16 at C = 70
                for ld in (C, C + 8):
                    if big and ld != C and C != 72:
                        continue
                    i += 1
                    mode = i % 4               # 0: plain; 1: momentum 0; 2: no running statistics; 3: prezeroed
                    kw = dict(rows=rows, C=C, ld=ld, train=1, momentum=(0.1, 0.0, 0.0, 0.1)[mode], norun=mode == 2, prezeroed=mode == 3)
                    cs.append(Case("stats", "stats", dtype, **kw))
                    cs.append(Case("stats", "fused", dtype, **dict(kw, prezeroed=i % 2 == 1)))
                    cs.append(Case("stats", "moments", dtype, rows=rows, C=C, ld=ld, train=1))
            cs.append(Case("stats", "stats", dtype, rows=33, C=C, ld=C, train=0, momentum=0.1))
        for C in (8, 72, 520):
            for rows in (33, 257, _rows_for(72, 32)):
                cs.append(Case("stats", "stats", dtype, rows=rows, C=C, ld=C, train=1, momentum=0.1, mis="x"))
                cs.append(Case("stats", "fused", dtype, rows=rows, C=C, ld=C + 8, train=1, momentum=0.1, mis="x"))
                cs.append(Case("stats", "moments", dtype, rows=rows, C=C, ld=C, train=1, mis="x"))
    return cs


APPLY_C = (8, 70, 72, 520)
APPLY_ROWS = (1, 7, BN_R - 1, BN_R + 1, 301, 2085)


def _fwd_cases():
    cs, i = [], 0
    for dtype in ("bf16", "f32"):
        for C in APPLY_C:
            for rows in APPLY_ROWS:
                for act in ACTS:
                    i += 1
                    cs.append(Case("fwd", "fwd", dtype, rows=rows, C=C, act=act))
                    rps = rows if i % 2 or rows % 7 else rows // 7
                    cs.append(Case("fwd", "res", dtype, rows=rows, C=C, act=act, res=True, rowscale=i % 3 != 0, rps=rps))
                    cs.append(Case("fwd", "fin", dtype, rows=rows, C=C, act=act, res=(i + i // 6) % 2 == 0, rowscale=i % 4 == 0, rps=rps,
                                   momentum=(0.1, 0.0)[i % 5 == 0]))
    for C in (8, 72, 520):
        for j, mis in enumerate(("x", "y", "gamma", "res")):
            act = ACTS[(j + C) % 6]
            cs.append(Case("fwd", "fwd", "bf16", rows=37, C=C, act=act, mis=mis))
            cs.append(Case("fwd", "res", "bf16", rows=37, C=C, act=act, res=True, rowscale=True, rps=37, mis=mis))
            cs.append(Case("fwd", "fin", "bf16", rows=37, C=C, act=act, res=True, rowscale=True, rps=37, momentum=0.1, mis=mis))
    return cs


def _bwd_cases():
    cs, i = [], 0
    for dtype in ("bf16", "f32"):
        for C in APPLY_C:
            for rows in APPLY_ROWS:
                for act in ACTS:
                    for train in (0, 1):
                        i += 1
                        kw = dict(rows=rows, C=C, act=act, train=train, nodx=i % 5 == 0, noparam=i % 7 == 0)
                        cs.append(Case("bwd", ("bwd", "sums")[i % 3 == 0], dtype, **kw))
        # the eight-rows-in-flight loop of the reduce pass (col_grid's 256-row branch, per > 256) and its 32-row tail
        for C in (8, 72):
            cs.append(Case("bwd", "bwd", dtype, rows=_rows_for(C, 256) if C != 8 else 256 * 512 + 560, C=C, act=(SILU, RELU)[C == 8], train=1))
    for C in (8, 72, 520):
        for j, mis in enumerate(("gamma", "dy", "x", "dx")):
            for train in (0, 1):
                cs.append(Case("bwd", "bwd", "bf16", rows=(37, 301)[train], C=C, act=ACTS[(j + C + train) % 6], train=train, mis=mis))
        for act in (RELU, SIGMOID):      # ShuffleNetV2's activation and the one only its backbone test reached, train 0 / NULL forms, aligned
            cs.append(Case("bwd", "bwd", "bf16", rows=301, C=C, act=act, train=0))
            cs.append(Case("bwd", "bwd", "bf16", rows=301, C=C, act=act, train=1, nodx=True))
            cs.append(Case("bwd", "bwd", "bf16", rows=301, C=C, act=act, train=1, noparam=True))
    return cs


POOL_HW = (1, 2, 35, 64, 257)


def _pool_cases():
    cs, i = [], 0
    for dtype in ("bf16", "f32"):
        for C in APPLY_C:
            for HW in POOL_HW:
                i += 1
                B = (1, 3)[i % 2]
                kw = dict(B=B, HW=HW, C=C)
                cs.append(Case("pool", "rowpool_mean", dtype, **kw))
                cs.append(Case("pool", "rowpool_mean_bwd", dtype, acc=i % 2 == 0, **kw))
                cs.append(Case("pool", "rowpool_mean_bwd", dtype, acc=i % 2 == 1, **dict(kw, B=4 - B)))
                cs.append(Case("pool", "se_scale_fwd", dtype, **kw))
                cs.append(Case("pool", "se_scale_bwd", dtype, nodx=dtype == "bf16" and C % 8 == 0 and i % 2 == 0, **kw))
                cs.append(Case("pool", "se_dx", dtype, **kw))
                cs.append(Case("pool", "se_dx", dtype, bn=True, act=ACTS[i % 6], **kw))
                cs.append(Case("pool", "residual_add", dtype, B=B, per_sample=HW * C, rowscale=i % 3 != 0, noa=i % 4 == 0))
        for act in ACTS:
            for rows, C in ((1, 8), (17, 70), (131, 72), (64, 520)):       # (the [B, C] matrices of squeeze-excitation)
                cs.append(Case("pool", "bias_act_fwd", dtype, B=rows, HW=1, C=C, act=act, nobias=act == NONE))
                cs.append(Case("pool", "bias_act_bwd", dtype, B=rows, HW=1, C=C, act=act, nobias=act == NONE, nodb=rows == 17))
        cs.append(Case("pool", "residual_add", dtype, B=3, per_sample=20, rowscale=True))
    for C in (8, 72):
        for HW in (35, 257):
            kw = dict(B=3, HW=HW, C=C)
            cs.append(Case("pool", "rowpool_mean", "bf16", mis="x", **kw))
            for mis in ("dpool", "dx"):
                cs.append(Case("pool", "rowpool_mean_bwd", "bf16", acc=True, mis=mis, **kw))
            for mis in ("x", "s", "y"):
                cs.append(Case("pool", "se_scale_fwd", "bf16", mis=mis, **kw))
            for mis in ("dy", "x", "s", "dx"):
                cs.append(Case("pool", "se_scale_bwd", "bf16", mis=mis, **kw))
            for mis in ("dy", "s", "dpool", "dx", "z"):
                cs.append(Case("pool", "se_dx", "bf16", bn=mis == "z", act=SILU, mis=mis, **kw))
            for mis in ("a", "branch", "out"):
                cs.append(Case("pool", "residual_add", "bf16", B=3, per_sample=HW * C, rowscale=True, mis=mis))
    # exact integers
    for dtype in ("bf16", "f32"):
        for C in (20, 72):
            kw = dict(B=3, HW=64, C=C, ints=True)
            cs += [Case("pool", "rowpool_mean", dtype, **kw), Case("pool", "se_scale_fwd", dtype, **kw), Case("pool", "se_scale_bwd", dtype, **kw),
                   Case("pool", "bias_act_bwd", dtype, B=64, HW=1, C=C, act=NONE, ints=True),
                   Case("pool", "residual_add", dtype, B=3, per_sample=64 * C, rowscale=True, ints=True)]
    return cs


def _layout_cases():
    cs = []
    for dtype in ("bf16", "f32"):
        for (H, W) in ((1, 1), (2, 3), (9, 6), (7, 7)):
            for B, C in ((1, 8), (3, 70)):
                cs.append(Case("layout", "maxpool3x3s2", dtype, B=B, H=H, W=W, C=C))          # (forward, then the backward on its argmax)
        for rows, Cin, Cout, ld_out, col0 in ((1, 8, 8, 8, 0), (37, 70, 24, 48, 5), (300, 72, 72, 150, 3), (5, 16, 7, 20, 13)):
            cs.append(Case("layout", "channel_gather", dtype, rows=rows, Cin=Cin, Cout=Cout, ld_out=ld_out, col0=col0))
        for rows, bf, lda in ((1, 4, 4), (37, 61, 122), (300, 122, 244), (5, 8, 20)):
            cs.append(Case("layout", "channel_interleave2", dtype, rows=rows, bf=bf, lda=lda))
            cs.append(Case("layout", "channel_deinterleave2", dtype, rows=rows, bf=bf, lda=bf))
            cs.append(Case("layout", "channel_deinterleave2", dtype, rows=rows, bf=bf, lda=2 * bf))
        for B, C, H, W in ((1, 3, 1, 1), (3, 3, 7, 5), (2, 5, 16, 9)):
            cs.append(Case("layout", "nchw_to_rows", dtype, B=B, C=C, H=H, W=W))
    return cs


DW_CASES, STATS_CASES, FWD_CASES, BWD_CASES, POOL_CASES, LAYOUT_CASES = (_dw_cases(), _stats_cases(), _fwd_cases(), _bwd_cases(),
                                                                         _pool_cases(), _layout_cases())
ALL_CASES = DW_CASES + STATS_CASES + FWD_CASES + BWD_CASES + POOL_CASES + LAYOUT_CASES


# ------------------------------------------------------------------------------------------------------
# buffers
# ------------------------------------------------------------------------------------------------------
def gen(c, dev):
    return torch.Generator(device=dev).manual_seed(sum(map(ord, repr(c))) * 31 + 7)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, device=g.device, dtype=torch.float64)


def rand(g, *shape):
    return torch.rand(*shape, generator=g, device=g.device, dtype=torch.float64)


def randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g, device=g.device).double()


def signs(g, *shape):
    return torch.where(rand(g, *shape) < 0.5, -1.0, 1.0).double()


def operand(vals, t, mis=False, ld=None):
    """a kernel operand holding vals [rows, D] at row stride ld, loud values in every other element, GUARD loud rows behind it, starting
    8 bytes past a 16-byte boundary if mis; (tensor to pass, its exact float64 values)"""
    vals = vals.reshape(vals.shape[0], -1) if vals.dim() > 1 else vals.reshape(1, -1)
    rows, D = vals.shape
    ld = D if ld is None else ld
    m = (8 // t.itemsize) if mis else 0
    n = m + (rows + GUARD) * ld + GUARD
    flat = torch.full((n,), LOUD, dtype=t, device=vals.device)
    flat[1::2] = -LOUD
    body = flat[m:m + rows * ld].view(rows, ld)
    body[:, :D] = vals.to(t)
    return flat[m:], body[:, :D].double()


class Out:
    """an output: owned [rows, D] at stride ld starts NaN (or `fill`), everything else the sentinel"""

    def __init__(self, rows, D, t, dev, ld=None, fill=None, mis=False):
        ld = D if ld is None else ld
        self.rows, self.D, self.ld = rows, D, ld
        self.m = (8 // torch.empty(0, dtype=t).element_size()) if mis else 0
        sent = SENT if t.is_floating_point else 77
        self.sent = sent
        self.flat = torch.full((self.m + (rows + GUARD) * ld + GUARD,), sent, dtype=t, device=dev)
        self.body = self.flat[self.m:self.m + rows * ld].view(rows, ld)
        if fill is not None:
            self.body[:, :D] = fill.reshape(rows, D).to(t)
        elif t.is_floating_point:
            self.body[:, :D] = float("nan")
        self.t = self.flat[self.m:]

    @property
    def owned(self):
        return self.body[:, :self.D]

    def untouched(self):
        s = self.sent
        return bool((self.flat[:self.m] == s).all()) and bool((self.flat[self.m + self.rows * self.ld:] == s).all()) and \
            bool((self.body[:, self.D:] == s).all())


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


# ------------------------------------------------------------------------------------------------------
# activations (float64 or float32 statements of act_f / act_grad_f, with act_grad_f's conventions at the kinks)
# ------------------------------------------------------------------------------------------------------
def act(u, a):
    if a == SILU:
        return u * torch.sigmoid(u)
    if a == RELU:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if a == SIGMOID:
        return torch.sigmoid(u)
    if a == HSWISH:
        return u * (u + 3).clamp(0, 6) / 6
    if a == HSIGMOID:
        return (u + 3).clamp(0, 6) / 6
    return u


def act_grad(u, a):
    one, zero = torch.ones_like(u), torch.zeros_like(u)
    if a == SILU:
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    if a == RELU:
        return torch.where(u > 0, one, zero)
    if a == SIGMOID:
        s = torch.sigmoid(u)
        return s * (1 - s)
    if a == HSWISH:
        return torch.where(u <= -3, zero, torch.where(u < 3, u / 3 + 0.5, one))
    if a == HSIGMOID:
        return torch.where((u > -3) & (u < 3), one / 6, zero)
    return one


def act_mag(u, a):
    """(sum of the |terms| of act(u) including the Lipschitz-weighted size of u's own terms `m`, intrinsic relative error)"""
    lip = {NONE: 1.0, SILU: 1.1, RELU: 1.0, SIGMOID: 0.25, HSWISH: 1.5, HSIGMOID: 1.0 / 6}[a]
    intr = (EXPF_ULP + RCP_ULP + 1.5 * u.abs()) * 2.0 ** -23 if a in (SILU, SIGMOID) else torch.zeros_like(u)
    return lip, intr


def act_grad_mag(u, a):
    """sum of the |terms| of act'(u)"""
    if a == SILU:
        return torch.sigmoid(u) * (1 + 2 * u.abs())
    if a == SIGMOID:
        return 2 * torch.sigmoid(u)
    if a == HSWISH:
        return torch.where(u <= -3, torch.zeros_like(u), torch.where(u < 3, u.abs() / 3 + 0.5, torch.ones_like(u)))
    return act_grad(u, a)


KINKS = {RELU: ((0.0, 1.0),), HSWISH: ((-3.0, 0.5), (3.0, 0.5)), HSIGMOID: ((-3.0, 1.0 / 6), (3.0, 1.0 / 6))}     # (kink, jump of act')


def kink_band(u, a, t):
    """(elements inside the band of a kink but not exactly on it, the jump of act' there)"""
    thr = (2.0 ** -7 if t == torch.bfloat16 else 2.0 ** -20) * u.abs().clamp(min=1.0)
    near, jump = torch.zeros_like(u, dtype=torch.bool), torch.zeros_like(u)
    for kpos, j in KINKS.get(a, ()):
        nk = ((u - kpos).abs() < thr) & (u != kpos)
        near |= nk
        jump = torch.where(nk, torch.full_like(u, 1.1 * j), jump)        # (1.1: the slope inside the band)
    return near, jump


# ------------------------------------------------------------------------------------------------------
# depthwise convolutions
# ------------------------------------------------------------------------------------------------------
def _taps(k):
    return [(ky, kx) for ky in range(k) for kx in range(k)]


def dw_fwd(x, w, k, s):
    """x [B, H, W, C], w [C, k*k] -> y [B, Ho, Wo, C] (padding k // 2)"""
    p = k // 2
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    xp = F.pad(x, (0, 0, p, p, p, p))
    y = torch.zeros(B, Ho, Wo, C, dtype=x.dtype, device=x.device)
    for ky, kx in _taps(k):
        y = y + xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s, :] * w[:, ky * k + kx]
    return y


def dw_bwd_data(dy, w, k, s, H, W):
    p = k // 2
    B, Ho, Wo, C = dy.shape
    dxp = torch.zeros(B, H + 2 * p, W + 2 * p, C, dtype=dy.dtype, device=dy.device)
    for ky, kx in _taps(k):
        dxp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s, :] += dy * w[:, ky * k + kx]
    return dxp[:, p:p + H, p:p + W, :].contiguous()


def dw_bwd_weight(dy, x, k, s):
    p = k // 2
    B, Ho, Wo, C = dy.shape
    xp = F.pad(x, (0, 0, p, p, p, p))
    return torch.stack([(dy * xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s, :]).sum((0, 1, 2)) for ky, kx in _taps(k)], 1)


class DwIn:
    def __init__(self, c, dev):
        g, t = gen(c, dev), tdt(c.dtype)
        Ho, Wo = dw_out(c)
        kk = c.k * c.k
        if c.ints:      # |y|, |dx| <= kk * 2 * 2 <= 100, |dw| <= 4 * npix + 64 < 2^24: every product and partial sum is exact in fp32
            x, dy, w = randint(g, -2, 2, c.B * c.H * c.W, c.C), randint(g, -2, 2, c.B * Ho * Wo, c.C), randint(g, -2, 2, c.C, kk)
            pre = randint(g, -64, 64, c.C, kk)
        else:
            x, dy, w = randn(g, c.B * c.H * c.W, c.C), randn(g, c.B * Ho * Wo, c.C), 0.5 * randn(g, c.C, kk)
            pre = (8.0 * randn(g, c.C, kk)).float().double()
        mis = c.mis
        self.x, x64 = operand(x, t, mis == "x")
        self.x64 = x64.view(c.B, c.H, c.W, c.C)
        self.w, w64 = operand(w.reshape(1, -1), t, mis == "w")
        self.w64 = w64.view(c.C, kk)
        if c.op == "bwd":
            self.dy, dy64 = operand(dy, t, mis == "dy")
            self.dy64 = dy64.view(c.B, Ho, Wo, c.C)
        self.pre = pre


def dw_ref(c, i, dt=torch.float64):
    """name -> value in dt; with dt = float64 also name + '_mag' -> the sum of the |terms|"""
    o = {}
    x, w = i.x64.to(dt), i.w64.to(dt)
    mag = dt == torch.float64
    if c.op == "fwd":
        o["y"] = dw_fwd(x, w, c.k, c.stride)
        if mag:
            o["y_mag"] = dw_fwd(x.abs(), w.abs(), c.k, c.stride)
        return o
    dy = i.dy64.to(dt)
    if c.form in ("dx", "both"):
        o["dx"] = dw_bwd_data(dy, w, c.k, c.stride, c.H, c.W)
        if mag:
            o["dx_mag"] = dw_bwd_data(dy.abs(), w.abs(), c.k, c.stride, c.H, c.W)
    if c.form in ("dw", "both"):
        o["dw"] = i.pre.to(dt) + dw_bwd_weight(dy, x, c.k, c.stride)
        if mag:
            o["dw_mag"] = i.pre.abs() + dw_bwd_weight(dy.abs(), x.abs(), c.k, c.stride)
    return o


def pointwise(got, ref, mag, t, extra=None):
    """|err| in units of ulp_T(|ref|) / 2 + 2^-24 * mag, after the explicit terms `extra`"""
    err = (got - ref).abs()
    if extra is not None:
        err = (err - extra).clamp(min=0)
    return err / (ulp(ref, t) / 2 + U * mag + 2.0 ** -140)


def sumwise(got, ref, mag, extra=None):
    err = (got - ref).abs()
    if extra is not None:
        err = (err - extra).clamp(min=0)
    return err / (U * mag + 2.0 ** -140)


def dw_ratios(c, i, ref, got):
    """[(name, key, ratio tensor)] of the outputs in `got` (float64 tensors shaped like the reference)"""
    t, out = tdt(c.dtype), []
    for name, key in (("y", "dw_y"), ("dx", "dw_dx")):
        if name in got:
            out.append((name, (key, c.dtype), pointwise(got[name], ref[name], ref[name + "_mag"], t)))
    if "dw" in got:
        out.append(("dw", ("dw_dw", c.dtype), sumwise(got["dw"], ref["dw"], ref["dw_mag"])))
    return out


# ------------------------------------------------------------------------------------------------------
# BatchNorm inputs
# ------------------------------------------------------------------------------------------------------
PLANT = torch.tensor([-3.0, 0.0, 3.0, 1.0, -1.0, 2.5, -4.0, 5.0], dtype=torch.float64)


def bn_x(rows, C, g):
    """float64 [rows, C]: per-channel mean of 3-6 sigma with mixed signs; channel 1 nearly constant; channel 2 with three rows 300
    sigma out; channel 3 walks over the kinks (for the apply / backward cases, which normalise it with mean 0, rstd 1)"""
    mean = signs(g, C) * (3.0 + 3.0 * rand(g, C))
    x = randn(g, rows, C) + mean
    if C > 1:
        x[:, 1] = mean[1] + 1e-4 * randn(g, rows)
    if C > 2:
        x[torch.arange(min(rows, 3), device=x.device) * max(rows // 3, 1), 2] += 300.0
    if C > 3:
        x[:, 3] = PLANT.to(x.device)[torch.arange(rows, device=x.device) % 8]
    return x


def bn_params(C, g, t):
    gamma = signs(g, C) * (1.5 + rand(g, C))
    beta = signs(g, C) * (0.25 + 0.5 * rand(g, C))
    if C > 4:
        gamma[4] = 0.0
    if C > 3:
        gamma[3], beta[3] = 1.0, 0.0
    return gamma.to(t).double(), beta.to(t).double()


def bn_given_stats(x64, C):
    """fp32 mean / rstd vectors handed to the apply / backward kernels: the batch statistics of x (channel 3: mean 0, rstd 1)"""
    mu = x64.mean(0)
    rs = ((x64 - mu).square().mean(0) + EPS).rsqrt()
    if C > 3:
        mu[3], rs[3] = 0.0, 1.0
    return mu.float().double(), rs.float().double()


def off_kinks(x64, mu, rs, gamma, beta, a, t):
    """x with every element inside a kink band (but not on the kink) moved out of it: by an ulp of x's type or by four band widths of u,
    whichever is larger; rounded to the type"""
    for _ in range(3):
        u = (x64 - mu) * rs * gamma + beta
        near, _j = kink_band(u, a, t)
        if not bool(near.any()):
            break
        thr = (2.0 ** -7 if t == torch.bfloat16 else 2.0 ** -20) * u.abs().clamp(min=1.0)
        step = torch.maximum(2 * ulp(x64, t), 4 * thr / (gamma.abs() * rs).clamp(min=1e-6))
        x64 = torch.where(near, x64 + step, x64).to(t).double()
    return x64


# ------------------------------------------------------------------------------------------------------
# BatchNorm statistics
# ------------------------------------------------------------------------------------------------------
def bn_shift_row(k, rows):
    seg = rows // BN_SHIFT_ROWS
    if seg <= 0:
        return k if k < rows else rows - 1
    return k * seg + ((2654435761 * (k + 1)) % (1 << 32)) % seg


def bn_shift(x64, rows):
    """the shift of the one-pass moments, operation for operation in fp32: the sum of the 16 sampled rows in order, minus their
    minimum and maximum, times float32(1 / 14)"""
    v = torch.stack([x64[bn_shift_row(k, rows)] for k in range(BN_SHIFT_ROWS)]).float()
    s = torch.zeros_like(v[0])
    for k in range(BN_SHIFT_ROWS):
        s = s + v[k]
    return ((s - v.min(0).values - v.max(0).values) * torch.tensor(1.0 / (BN_SHIFT_ROWS - 2), dtype=torch.float32, device=v.device)).double()


class StatsIn:
    def __init__(self, c, dev):
        g, t = gen(c, dev), tdt(c.dtype)
        self.x, self.x64 = operand(bn_x(c.rows, c.C, g), t, c.mis == "x", ld=c.ld)
        self.rm = (signs(g, c.C) * (1 + rand(g, c.C))).float().double()
        self.rv = (0.5 + rand(g, c.C)).float().double()
        self.pre1, self.pre2 = (4.0 * randn(g, c.C)).float().double(), (4.0 * rand(g, c.C)).float().double()
        self.one_pass = cell(c)[0][0].startswith("col_moment2")
        self.shift = bn_shift(self.x64, c.rows) if self.one_pass else torch.zeros(c.C, dtype=torch.float64, device=dev)


def _blocked_sum(v, chunk=256):
    """column sums in chunks of `chunk` rows, then over the chunks (an order independent of the kernels')"""
    n = v.shape[0]
    parts = [v[k:k + chunk].sum(0) for k in range(0, n, chunk)]
    return torch.stack(parts).sum(0)


def chain_x(v, pre, rows, C, lanes):
    """First-order worst case of the DEPENDENT fp32 additions behind a column sum of v [rows, C] as col_grid lays it out: a thread adds
    ceil(per / lanes) rows one after the other (+ 5 for the shuffle / LDS tree), and the nblk blocks of a channel add their sums to ONE
    address with atomics, i.e. one after the other in some order.  Each addition errs by at most 2^-24 of the partial sum it produces:
    a thread's partials are bounded by the sum of its |addends|, the running total of the atomics by |prefill| + the sum of the |block
    sums| (blocks = `per` consecutive rows).  K does not cover this: it is measured against a float32 sum in chunks of 256 rows,
    whose depth does not grow with nblk, and same-signed near-equal addends (the near-constant channel) round the same way at every
    step, so the error grows with the chain's length, not with its square root (observed: 377 units = 2.2e-5 of a mean over
    983,077 rows in 2,048 blocks)."""
    _, nblk, per = col_grid(rows, C)
    blocks = F.pad(v, (0, 0, 0, nblk * per - rows)).view(nblk, per, -1).sum(1).abs().sum(0)
    return U * ((cdiv(per, lanes) + 5) * v.abs().sum(0) + nblk * (blocks + (pre.abs() if pre is not None else 0.0)))


def stats_ref(c, i, dt=torch.float64):
    """the statistics as the cell forms them, in dt: one pass of shifted sums (bf16 fast path) or two passes"""
    o, n = {}, c.rows
    mom = c.momentum or 0.0
    if c.op == "stats" and not c.train:
        o["mean"], o["var"] = i.rm.to(dt), i.rv.to(dt)
        o["rstd"] = (o["var"] + torch.tensor(EPS, dtype=torch.float32).to(dt)).rsqrt()
        return o
    x = i.x64.to(dt)
    if i.one_pass:
        d = x - i.shift.to(dt)
        s1, s2 = _blocked_sum(d), _blocked_sum(d * d)
        if c.op == "moments":
            o["s1"], o["s2"] = i.pre1.to(dt) + s1, i.pre2.to(dt) + s2
            if dt == torch.float64:
                o["s1_mag"], o["s2_mag"] = i.pre1.abs() + d.abs().sum(0), i.pre2.abs() + (d * d).sum(0)
                o["s1_x"], o["s2_x"] = chain_x(d, i.pre1, n, c.C, 32), chain_x(d * d, i.pre2, n, c.C, 32)
            return o
        d1 = s1 / n
        o["mean"], o["var"] = i.shift.to(dt) + d1, (s2 / n - d1 * d1).clamp(min=0)
        if dt == torch.float64:
            o["mean_mag"] = i.shift.abs() + d.abs().mean(0)
            o["var_mag"] = (d * d).mean(0) + 2 * d1.abs() * d.abs().mean(0) + o["var"] + EPS
            o["mean_x"], o["var_x"], o["_d1"] = chain_x(d, None, n, c.C, 32) / n, chain_x(d * d, None, n, c.C, 32) / n, d1.abs()
    else:
        mu = _blocked_sum(x) / n
        d = x - mu
        o["mean"], o["var"] = mu, _blocked_sum(d * d) / n
        if dt == torch.float64:
            o["mean_mag"] = x.abs().mean(0)
            o["var_mag"] = (d * d).mean(0) + o["var"] + EPS
            o["mean_x"], o["var_x"], o["_d1"] = chain_x(x, None, n, c.C, 4) / n, chain_x(d * d, None, n, c.C, 4) / n, torch.zeros_like(mu)
    eps = torch.tensor(EPS, dtype=torch.float32).to(dt)
    o["rstd"] = (o["var"] + eps).rsqrt()
    if not c.norun and mom > 0:
        m = torch.tensor(mom, dtype=torch.float32).to(dt)
        unb = o["var"] * n / (n - 1) if n > 1 else o["var"]
        o["rm"], o["rv"] = (1 - m) * i.rm.to(dt) + m * o["mean"], (1 - m) * i.rv.to(dt) + m * unb
        if dt == torch.float64:
            f = n / (n - 1) if n > 1 else 1.0
            o["rm_mag"], o["rv_mag"] = i.rm.abs() + m * o["mean"].abs(), i.rv.abs() + m * unb.abs()
            o["rm_stat"], o["rv_stat"] = m, m * f                  # d running / d (mean | var)
    return o


def stats_ratios(c, i, ref, got):
    out, dk = [], c.dtype
    if "s1" in got:
        return [("s1", ("bn_s", dk), sumwise(got["s1"], ref["s1"], ref["s1_mag"], ref["s1_x"])),
                ("s2", ("bn_s", dk), sumwise(got["s2"], ref["s2"], ref["s2_mag"], ref["s2_x"]))]
    eps = float(torch.tensor(EPS, dtype=torch.float32))
    var_got = got["rstd"] ** -2 - eps
    rs_x = 2 * RSQRT_ULP * 2.0 ** -23 * (ref["var"] + eps)
    if c.op == "stats" and not c.train:
        assert torch.equal(got["mean"], ref["mean"]), "eval-mode mean is not the running mean"
        return [("rstd", ("bn_var", dk), sumwise(var_got, ref["var"], ref["var"] + eps, rs_x))]
    # the variance is centred on the kernel's own mean (two passes), or q - d1^2 with its own d1 (one pass): an error dm of the mean
    # adds dm^2, or 2 |d1| dm + dm^2
    dm = (got["mean"] - ref["mean"]).abs()
    var_x = ref["var_x"] + 2 * ref["_d1"] * dm + dm * dm
    out.append(("mean", ("bn_mean", dk), sumwise(got["mean"], ref["mean"], ref["mean_mag"], ref["mean_x"])))
    out.append(("rstd", ("bn_var", dk), sumwise(var_got, ref["var"], ref["var_mag"], rs_x + var_x)))
    if "rm" in got and "rm" in ref:
        # the running statistics follow the kernel's own mean / variance; the variance it used is not an output: bounded as above
        dv = BOUND[("bn_var", dk)] * U * ref["var_mag"] + var_x
        out.append(("running_mean", ("bn_run", dk), sumwise(got["rm"], ref["rm"], ref["rm_mag"], 1.001 * ref["rm_stat"] * dm)))
        out.append(("running_var", ("bn_run", dk), sumwise(got["rv"], ref["rv"], ref["rv_mag"], 1.001 * ref["rv_stat"] * dv)))
    return out


# ------------------------------------------------------------------------------------------------------
# BatchNorm apply
# ------------------------------------------------------------------------------------------------------
class FwdIn:
    def __init__(self, c, dev):
        g, t = gen(c, dev), tdt(c.dtype)
        R, C = c.rows, c.C
        x = bn_x(R, C, g).to(t).double()
        gamma, beta = bn_params(C, g, t)
        mu, rs = bn_given_stats(x, C)
        if c.op == "fin":       # the sums a moments launch leaves: shift near the mean, s1 = sum d, s2 = sum d^2 (fp32)
            sh = (mu + 0.25 * randn(g, C)).float().double()
            d = x - sh
            self.sh, self.s1, self.s2 = sh, d.sum(0).float().double(), (d * d).sum(0).float().double()
            d1 = self.s1 / R
            mu, rs = sh + d1, ((self.s2 / R - d1 * d1).clamp(min=0) + float(torch.tensor(EPS, dtype=torch.float32))).rsqrt()
            self.rm, self.rv = (signs(g, C) * (1 + rand(g, C))).float().double(), (0.5 + rand(g, C)).float().double()
        self.mu, self.rs = mu, rs
        self.x, self.x64 = operand(x, t, c.mis == "x")
        self.gamma, self.g64 = operand(gamma.reshape(1, -1), t, c.mis == "gamma")
        self.beta, self.b64 = operand(beta.reshape(1, -1), t)
        self.g64, self.b64 = self.g64[0], self.b64[0]
        if c.res:
            self.res, self.res64 = operand(randn(g, R, C), t, c.mis == "res")
            nsamp = cdiv(R, c.rps)
            sc = torch.where(rand(g, nsamp) < 0.3, 0.0, 1.0 / 0.8).float().double() if c.rowscale else None
            self.sc = sc
            self.sc_rows = sc[torch.arange(R, device=dev) // c.rps][:, None] if c.rowscale else torch.ones(R, 1, dtype=torch.float64, device=dev)


def fwd_ref(c, i, dt=torch.float64):
    o = {}
    x, g, b = i.x64.to(dt), i.g64.to(dt), i.b64.to(dt)
    mu, rs = i.mu.to(dt), i.rs.to(dt)
    if c.op == "fin":
        n = c.rows
        eps = torch.tensor(EPS, dtype=torch.float32).to(dt)
        d1 = i.s1.to(dt) / n
        q = i.s2.to(dt) / n
        var = (q - d1 * d1).clamp(min=0)
        mu, rs = i.sh.to(dt) + d1, (var + eps).rsqrt()
        o["mean"], o["rstd"], o["var"] = mu, rs, var
        mom = c.momentum or 0.0
        if mom > 0:
            m = torch.tensor(mom, dtype=torch.float32).to(dt)
            unb = var * n / (n - 1) if n > 1 else var
            o["rm"], o["rv"] = (1 - m) * i.rm.to(dt) + m * mu, (1 - m) * i.rv.to(dt) + m * unb
        if dt == torch.float64:
            o["mean_mag"] = i.sh.abs() + d1.abs()
            o["var_mag"] = q.abs() + 2 * d1 * d1 + var + EPS
            if mom > 0:
                f = n / (n - 1) if n > 1 else 1.0
                o["rm_mag"], o["rv_mag"] = i.rm.abs() + m * mu.abs(), i.rv.abs() + m * unb.abs()
                o["rm_stat"], o["rv_stat"] = m, m * f
    xh = (x - mu) * rs
    u = xh * g + b
    v = act(u, c.act)
    y = i.res64.to(dt) + i.sc_rows.to(dt) * v if c.res else v
    o["y"] = y
    if dt == torch.float64:
        lip, intr = act_mag(u, c.act)
        m = lip * ((xh * g).abs() + b.abs()) + v.abs()
        x_ = intr * v.abs()
        if c.res:
            m, x_ = i.res64.abs() + i.sc_rows * m, i.sc_rows * x_
        o["y_mag"], o["y_x"] = m, x_
        o["_xh"], o["_lip"] = xh, lip * (i.sc_rows if c.res else 1.0)
    return o


def fwd_ratios(c, i, ref, got):
    t, dk, out = tdt(c.dtype), c.dtype, []
    extra = ref["y_x"]
    if c.op == "fin" and "mean" in got:
        eps = float(torch.tensor(EPS, dtype=torch.float32))
        var_got = got["rstd"] ** -2 - eps
        out.append(("mean", ("bn_mean", dk), sumwise(got["mean"], ref["mean"], ref["mean_mag"])))
        out.append(("rstd", ("bn_var", dk), sumwise(var_got, ref["var"], ref["var_mag"], 2 * RSQRT_ULP * 2.0 ** -23 * (ref["var"] + eps))))
        dm, dr = (got["mean"] - ref["mean"]).abs(), (got["rstd"] - ref["rstd"]).abs()
        extra = extra + 1.01 * ref["_lip"] * i.g64.abs() * (dm * ref["rstd"] + ref["_xh"].abs() * dr / ref["rstd"])
        if "rm" in ref:
            dv = BOUND[("bn_var", dk)] * U * ref["var_mag"]
            out.append(("running_mean", ("bn_run", dk), sumwise(got["rm"], ref["rm"], ref["rm_mag"], 1.001 * ref["rm_stat"] * dm)))
            out.append(("running_var", ("bn_run", dk), sumwise(got["rv"], ref["rv"], ref["rv_mag"], 1.001 * ref["rv_stat"] * dv)))
    out.append(("y", ("bn_y", dk), pointwise(got["y"], ref["y"], ref["y_mag"], t, extra)))
    return out


# ------------------------------------------------------------------------------------------------------
# BatchNorm backward
# ------------------------------------------------------------------------------------------------------
class BwdIn:
    def __init__(self, c, dev):
        g, t = gen(c, dev), tdt(c.dtype)
        R, C = c.rows, c.C
        x = bn_x(R, C, g).to(t).double()
        gamma, beta = bn_params(C, g, t)
        self.mu, self.rs = bn_given_stats(x, C)
        x = off_kinks(x, self.mu, self.rs, gamma, beta, c.act, t)
        dy = randn(g, R, C) + signs(g, C) * (0.5 + rand(g, C))
        self.x, self.x64 = operand(x, t, c.mis == "x")
        self.dy, self.dy64 = operand(dy, t, c.mis == "dy")
        self.gamma, g64 = operand(gamma.reshape(1, -1), t, c.mis == "gamma")
        self.beta, b64 = operand(beta.reshape(1, -1), t)
        self.g64, self.b64 = g64[0], b64[0]
        self.pre_g, self.pre_b = (8.0 * randn(g, C)).float().double(), (8.0 * randn(g, C)).float().double()
        self.xh = (self.x64 - self.mu) * self.rs
        self.u = self.xh * self.g64 + self.b64
        self.near, self.jump = kink_band(self.u, c.act, t)
        if c.op == "sums":      # the sums se_dx left: the exact sums rounded to fp32
            du = self.dy64 * act_grad(self.u, c.act)
            self.sd, self.sx = du.sum(0).float().double(), (du * self.xh).sum(0).float().double()


def bwd_ref(c, i, dt=torch.float64):
    o, n = {}, c.rows
    xh = (i.x64.to(dt) - i.mu.to(dt)) * i.rs.to(dt)
    g, b, dy = i.g64.to(dt), i.b64.to(dt), i.dy64.to(dt)
    u = xh * g + b
    du = dy * act_grad(u, c.act)
    if c.op == "sums":
        sd, sx = i.sd.to(dt), i.sx.to(dt)
    else:
        sd, sx = _blocked_sum(du), _blocked_sum(du * xh)
        o["sd"], o["sx"] = sd, sx
    if not c.noparam:
        o["dgamma"], o["dbeta"] = i.pre_g.to(dt) + sx, i.pre_b.to(dt) + sd
    gr = g * i.rs.to(dt)
    corr = (sd + xh * sx) / n if c.train else torch.zeros_like(du)
    if not c.nodx:
        o["dx"] = gr * (du - corr)
    if dt == torch.float64:
        gm = act_grad_mag(u, c.act)
        _lip, intr = act_mag(u, c.act)
        dum = dy.abs() * gm
        o["du_x"] = dum * intr
        o["sd_mag"], o["sx_mag"] = dum.sum(0), (dum * xh.abs()).sum(0)
        # elements inside a kink band may take the other branch of act': their whole jump enters the sums' bounds
        jm = torch.where(i.near, dy.abs() * i.jump, torch.zeros_like(dy))
        o["sd_x"], o["sx_x"] = jm.sum(0) + o["du_x"].sum(0), (jm * xh.abs()).sum(0) + (o["du_x"] * xh.abs()).sum(0)
        if c.op == "bwd":
            lanes = 32 if _v8(c, "dy", "x") else 4
            o["sd_x"], o["sx_x"] = o["sd_x"] + chain_x(du, None, n, c.C, lanes), o["sx_x"] + chain_x(du * xh, None, n, c.C, lanes)
        o["dx_mag"] = gr.abs() * (dum + ((sd.abs() + (xh * sx).abs()) / n if c.train else 0.0))
        o["_gr"], o["_xh"] = gr, xh
    return o


def bwd_ratios(c, i, ref, got):
    t, dk, out = tdt(c.dtype), c.dtype, []
    dsd = dsx = torch.zeros_like(i.mu)
    if "sd" in got:
        out.append(("sum_du", ("bn_sums", dk), sumwise(got["sd"], ref["sd"], ref["sd_mag"], ref["sd_x"])))
        out.append(("sum_duxh", ("bn_sums", dk), sumwise(got["sx"], ref["sx"], ref["sx_mag"], ref["sx_x"])))
        dsd, dsx = (got["sd"] - ref["sd"]).abs(), (got["sx"] - ref["sx"]).abs()
    if "dgamma" in got:
        x_g, x_b = (ref["sx_x"], ref["sd_x"]) if c.op == "bwd" else (None, None)
        out.append(("dgamma", ("bn_sums", dk), sumwise(got["dgamma"], ref["dgamma"], i.pre_g.abs() + ref["sx_mag"], x_g)))
        out.append(("dbeta", ("bn_sums", dk), sumwise(got["dbeta"], ref["dbeta"], i.pre_b.abs() + ref["sd_mag"], x_b)))
    if "dx" in got:
        extra = ref["_gr"].abs() * ref["du_x"]
        if c.train:
            extra = extra + 1.01 * ref["_gr"].abs() * (dsd + ref["_xh"].abs() * dsx) / c.rows
        r = pointwise(got["dx"], ref["dx"], ref["dx_mag"], t, extra)
        out.append(("dx", ("bn_dx", dk), torch.where(i.near, torch.zeros_like(r), r)))
    return out


# ------------------------------------------------------------------------------------------------------
# pooling, squeeze-excitation, elementwise
# ------------------------------------------------------------------------------------------------------
class PoolIn:
    def __init__(self, c, dev):
        g, t = gen(c, dev), tdt(c.dtype)
        op, mis = c.op, c.mis
        if op == "residual_add":
            B, n = c.B, c.per_sample
            if c.ints:
                a, br, sc = randint(g, -100, 100, B, n), randint(g, -50, 50, B, n), torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64, device=dev)[:B]
            else:
                a, br = randn(g, B, n), randn(g, B, n)
                sc = torch.where(rand(g, B) < 0.4, 0.0, 1.25).double()
                sc[0] = 0.0
            self.a, self.a64 = operand(a, t, mis == "a")
            self.br, self.br64 = operand(br, t, mis == "branch")
            self.sc = sc.float().double()
            return
        B, HW, C = c.B, c.HW, c.C
        R = B * HW
        if c.ints:      # |x|, |dy| <= 2, |s| <= 2: products <= 4, sums over 64 rows <= 256: exact in fp32 and in bf16
            x, dy, s = randint(g, -2, 2, R, C), randint(g, -2, 2, R, C), randint(g, -2, 2, B, C)
        else:
            x, dy, s = randn(g, R, C) + signs(g, C), randn(g, R, C) + 0.5 * signs(g, C), rand(g, B, C)
        self.x, self.x64 = operand(x, t, mis == "x")
        self.dy, self.dy64 = operand(dy, t, mis == "dy")
        self.s, self.s64 = operand(s, t, mis == "s")
        self.dpool, self.dpool64 = operand(8.0 * randn(g, B, C), t, mis == "dpool")
        self.dx0 = randn(g, R, C).to(t).double()
        if op in ("bias_act_fwd", "bias_act_bwd"):
            bias = (signs(g, C) * (0.25 + 0.5 * rand(g, C))).to(t).double()
            if c.ints:
                bias = randint(g, -2, 2, C)
            if c.nobias:
                bias = torch.zeros_like(bias)
            xx = 3.0 * randn(g, R, C).to(t).double() if not c.ints else x
            if C > 3 and not c.ints:
                xx[:, 3] = PLANT.to(dev)[torch.arange(R, device=dev) % 8]
                bias[3] = 0.0
            one = torch.ones(C, dtype=torch.float64, device=dev)
            xx = off_kinks(xx, 0 * one, one, one, bias, c.act, t)
            self.x, self.x64 = operand(xx, t)
            self.bias, b64 = operand(bias.reshape(1, -1), t)
            self.b64 = b64[0]
            self.u = self.x64 + self.b64
            self.near, self.jump = kink_band(self.u, c.act, t)
            self.pre = (8.0 * randn(g, C)).float().double() if not c.ints else randint(g, -64, 64, C)
        if op == "se_dx" and c.bn:
            z = bn_x(R, C, g).to(t).double()
            gamma, beta = bn_params(C, g, t)
            self.mu, self.rs = bn_given_stats(z, C)
            z = off_kinks(z, self.mu, self.rs, gamma, beta, c.act, t)
            self.z, self.z64 = operand(z, t, mis == "z")
            self.gamma, g64 = operand(gamma.reshape(1, -1), t)
            self.beta, b64 = operand(beta.reshape(1, -1), t)
            self.g64, self.b64 = g64[0], b64[0]
            self.pre = (8.0 * randn(g, 2, C)).float().double()
            self.xh = (self.z64 - self.mu) * self.rs
            self.u = self.xh * self.g64 + self.b64
            self.near, self.jump = kink_band(self.u, c.act, t)


def _per_sample(v, HW):
    return v.repeat_interleave(HW, 0)


def pool_ref(c, i, dt=torch.float64, dx_stored=None):
    """dx_stored (se_dx with the BatchNorm sums): the dx the kernel stored -- the sums are those of the stored values"""
    o, op, mag = {}, c.op, dt == torch.float64
    if op == "residual_add":
        a, br, sc = i.a64.to(dt), i.br64.to(dt), (i.sc.to(dt)[:, None] if c.rowscale else 1.0)
        o["out"] = br * sc + (0 if c.noa else a)
        if mag:
            o["out_mag"] = (br * sc).abs() + (0 if c.noa else a.abs())
        return o
    B, HW, C = c.B, c.HW, c.C
    x, dy, s = i.x64.to(dt), i.dy64.to(dt), i.s64.to(dt)
    if op == "rowpool_mean":
        o["out"] = x.view(B, HW, C).sum(1) / HW
        if mag:
            o["out_mag"] = x.abs().view(B, HW, C).sum(1) / HW
    elif op == "rowpool_mean_bwd":
        gpart = _per_sample(i.dpool64.to(dt), HW) / HW
        o["dx"] = (i.dx0.to(dt) if c.acc else 0) + gpart
        if mag:
            o["dx_mag"] = (i.dx0.abs() if c.acc else 0) + gpart.abs()
    elif op == "se_scale_fwd":
        o["y"] = x * _per_sample(s, HW)
        if mag:
            o["y_mag"] = o["y"].abs()
    elif op == "se_scale_bwd":
        if not c.nodx:
            o["dx"] = dy * _per_sample(s, HW)
        o["ds"] = (dy * x).view(B, HW, C).sum(1)
        if mag:
            o["dx_mag"], o["ds_mag"] = (dy * _per_sample(s, HW)).abs(), (dy * x).abs().view(B, HW, C).sum(1)
    elif op == "se_dx":
        a, p = dy * _per_sample(s, HW), _per_sample(i.dpool64.to(dt), HW) / HW
        o["dx"] = a + p
        if mag:
            o["dx_mag"] = a.abs() + p.abs()
        if c.bn:
            dxs = (o["dx"].to(tdt(c.dtype)).to(dt) if dx_stored is None else dx_stored.to(dt))
            xh = (i.z64.to(dt) - i.mu.to(dt)) * i.rs.to(dt)
            u = xh * i.g64.to(dt) + i.b64.to(dt)
            du = dxs * act_grad(u, c.act)
            o["sums"] = i.pre.to(dt) + torch.stack([du.sum(0), (du * xh).sum(0)])
            if mag:
                dum = dxs.abs() * act_grad_mag(u, c.act)
                _l, intr = act_mag(u, c.act)
                jm = torch.where(i.near, dxs.abs() * i.jump, torch.zeros_like(dxs))
                o["sums_mag"] = i.pre.abs() + torch.stack([dum.sum(0), (dum * xh.abs()).sum(0)])
                o["sums_x"] = torch.stack([(jm + dum * intr).sum(0), ((jm + dum * intr) * xh.abs()).sum(0)])
    elif op == "bias_act_fwd":
        u = x + i.b64.to(dt)
        o["y"] = act(u, c.act)
        if mag:
            lip, intr = act_mag(u, c.act)
            o["y_mag"], o["y_x"] = lip * (x.abs() + i.b64.abs()) + o["y"].abs(), intr * o["y"].abs()
    elif op == "bias_act_bwd":
        u = x + i.b64.to(dt)
        o["dx"] = dy * act_grad(u, c.act)
        if not c.nodb:
            o["dbias"] = i.pre.to(dt) + o["dx"].sum(0)
        if mag:
            dum = dy.abs() * act_grad_mag(u, c.act)
            _l, intr = act_mag(u, c.act)
            jm = torch.where(i.near, dy.abs() * i.jump, torch.zeros_like(dy))
            o["dx_mag"], o["dx_x"] = dum, dum * intr
            o["dbias_mag"], o["dbias_x"] = i.pre.abs() + dum.sum(0), (jm + dum * intr).sum(0)
    return o


def pool_ratios(c, i, ref, got):
    t, dk, out = tdt(c.dtype), c.dtype, []
    for name in ("out", "y", "dx", "ds"):
        if name in got:
            key = "pool" if (c.op, name) in (("rowpool_mean", "out"), ("se_scale_bwd", "ds")) else "ew"
            r = pointwise(got[name], ref[name], ref[name + "_mag"], t, ref.get(name + "_x"))
            if c.op == "bias_act_bwd" and name == "dx":
                r = torch.where(i.near, torch.zeros_like(r), r)
            out.append((name, (key, dk), r))
    for name in ("sums", "dbias"):
        if name in got:
            out.append((name, ("colsum", dk), sumwise(got[name], ref[name], ref[name + "_mag"], ref.get(name + "_x"))))
    return out


# ------------------------------------------------------------------------------------------------------
# max pooling and the layout kernels (bitwise)
# ------------------------------------------------------------------------------------------------------
def maxpool_ref(x):
    """x [B, H, W, C] -> (y, argmax tap): the first maximum in (ky, kx) order wins (`v > best` in maxpool3x3s2_fwd_k)"""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    best = torch.full((B, Ho, Wo, C), float("-inf"), dtype=x.dtype, device=x.device)
    arg = torch.zeros(B, Ho, Wo, C, dtype=torch.uint8, device=x.device)
    for ky, kx in _taps(3):
        v = xp[:, ky:ky + (Ho - 1) * 2 + 1:2, kx:kx + (Wo - 1) * 2 + 1:2, :]
        better = v > best
        best = torch.where(better, v, best)
        arg = torch.where(better, torch.full_like(arg, ky * 3 + kx), arg)
    return best, arg


def maxpool_bwd_ref(dy, arg, H, W):
    """dx [B, H, W, C] and the sum of |terms|: every output pixel's gradient goes to its argmax tap"""
    B, Ho, Wo, C = dy.shape
    dxp = torch.zeros(B, H + 2, W + 2, C, dtype=dy.dtype, device=dy.device)
    mg = torch.zeros_like(dxp)
    for ky, kx in _taps(3):
        sel = (arg == ky * 3 + kx).to(dy.dtype)
        dxp[:, ky:ky + (Ho - 1) * 2 + 1:2, kx:kx + (Wo - 1) * 2 + 1:2, :] += dy * sel
        mg[:, ky:ky + (Ho - 1) * 2 + 1:2, kx:kx + (Wo - 1) * 2 + 1:2, :] += dy.abs() * sel
    return dxp[:, 1:1 + H, 1:1 + W, :].contiguous(), mg[:, 1:1 + H, 1:1 + W, :].contiguous()


# ------------------------------------------------------------------------------------------------------
# one driver for both test files
# ------------------------------------------------------------------------------------------------------
FAMILIES = {"dw": (DwIn, dw_ref, dw_ratios), "stats": (StatsIn, stats_ref, stats_ratios), "fwd": (FwdIn, fwd_ref, fwd_ratios),
            "bwd": (BwdIn, bwd_ref, bwd_ratios), "pool": (PoolIn, pool_ref, pool_ratios)}
T_TYPED = ("y", "dx", "out", "ds")          # outputs stored in the activation type; every other output is fp32


def build(c, dev):
    return FAMILIES[c.fam][0](c, dev)


def reference(c, i, got):
    """the float64 reference of the outputs in `got` (se_dx with the BatchNorm sums: the sums of the dx the kernel stored)"""
    if c.fam == "pool" and c.op == "se_dx" and c.bn:
        return pool_ref(c, i, dx_stored=got["dx"].view(-1, c.C))
    return FAMILIES[c.fam][1](c, i)


def ratios(c, i, ref, got):
    return FAMILIES[c.fam][2](c, i, ref, got)


def emulate(c, i):
    """the same formulas in plain torch float32 (blocked sums of 256 rows: an order of its own), stored like the kernel stores them"""
    r32 = FAMILIES[c.fam][1](c, i, torch.float32)
    t = tdt(c.dtype)
    return {k: (v.to(t) if k in T_TYPED else v).double() for k, v in r32.items() if not k.startswith("_")}


def rejected(c):
    return cell(c)[0] == ("REJECT",)
