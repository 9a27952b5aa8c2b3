"""Every dispatch cell of the attention kernels (attention_mfma.hip bf16, attention_f32.hip fp32, the reference kernels the fp32
path falls to above S = 208, and the class-token kernels of attention_cls.hip) against a float64 statement of the same
operation on the kernel's exact inputs -- forward AND backward, checked per (sequence, head) block and per row of each of
out, dQ, dK and dV, so that a failure names the cell, the head and the segment that broke.  Needs an MI355X; every call
goes through the C ABI.

Inputs are built to expose what randn hides: peaky scores (one dominant key per row), masked keys whose scores sit ~100
above every valid score and whose V rows are large (a masked key that enters the row maximum or P.V shows at once), and
large finite values in the slack rows behind every input (tile padding is filled with copies of valid rows and multiplied
by an exact zero, so nothing behind the last row may reach an output).  Outputs start as NaN with sentinel guard rows
behind them; every owned row must be written and no guard row touched.  Every case runs twice and must repeat bitwise."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import lib as L                 # noqa: E402
from garbage_classification_rca_amd.procedural import counter_uniform  # noqa: E402

DH = 64
SCALE = DH ** -0.5
SEED = 4242          # dropout seed
P_DROP = 0.1
SLACK = 128          # loud rows behind every input buffer
GUARD = 16           # sentinel rows behind every output buffer
LOUD = 8192.0        # magnitude of the slack rows (finite: padding is multiplied by an exact zero, and 0 * NaN would not be)
SENT = -3072.0       # guard-row sentinel (exact in bf16)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "garbage_classification_rca_amd", "csrc")

# Bounds on max |err| / max |ref| per (sequence, head) block, and per row with a floor of 1e-2 x the block max (DESIGN section 0
# #1: >= 4x the worst value observed over the case list below).  Observed worst over the cases, block / row, next to each bound.
# bf16: storing an output in bf16 alone costs up to 2^-8 = 3.9e-3 of its block's largest entry (8 significant bits), so no bound
# within the issue's caps (1e-2 forward, 1.5e-2 backward) can be 4x the observed; these are the caps, 1.5x above the observed
# (inputs are seeded and every kernel repeats bitwise, so the values below are exactly what each run sees).
BOUND = {
    ("bf16", "out"): 1e-2,     # observed 5.2e-3 / 6.7e-3 (persistent forward, S = 224, peaky, B*H = 3072)
    ("bf16", "dq"): 1.5e-2,    # observed 8.6e-3 / 9.4e-3 (fused backward, S = 224, peaky, B*H = 3072)
    ("bf16", "dk"): 1.5e-2,    # observed 7.7e-3 / 8.9e-3 (persistent backward, S = 193, peaky, B*H = 3072)
    ("bf16", "dv"): 1.5e-2,    # observed 6.8e-3 / 9.5e-3 (persistent backward, S = 197, peaky, B*H = 3072)
    ("f32", "out"): 2e-5,      # observed 1.7e-6 / 3.7e-6
    ("f32", "dq"): 4e-5,       # observed 7.7e-6 / 8.0e-6
    ("f32", "dk"): 4e-5,       # observed 4.4e-6 / 5.0e-6
    ("f32", "dv"): 4e-5,       # observed 1.6e-6 / 5.3e-6
}
# |err| <= bound * max(1, |lse|); observed: bf16 3.3e-7 (generic and class-token kernels), fp32 6.0e-7
LSE_BOUND = {"bf16": 2e-6, "f32": 3e-6}
# mha_fwd_mfma_p_k takes the row sum from the bf16-rounded probabilities (the all-ones MFMA over the P operand of P.V), not from
# the fp32 ones: its log-sum-exp carries their rounding, ~2^-9 / sqrt(keys) relative per row.  observed 1.7e-4 (S = 208, peaky,
# B*H = 3072)
LSE_BOUND_PERSISTENT = 7e-4


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ------------------------------------------------------------------------------------------------------
def _walk(nbh, ncu):
    """how a persistent kernel's grid of min(nbh, ncu) workgroups walks heads bh, bh + grid, ..."""
    if nbh <= ncu:
        return "one head per workgroup"
    return "whole rounds" if nbh % ncu == 0 else "ragged last round"


def cell(S, dtype, masked, packed, drop, nbh, cls=False, ncu=None):
    """The kernel templates one forward + backward call reaches: (forward kernels..., backward kernels...).
    dtype 'bf16' | 'f32'; masked = a key_mask is passed; packed = cu_seqlens is passed; drop = dropout p > 0; nbh = B * H."""
    ncu = _ncu() if ncu is None else ncu
    tn = "bf16" if dtype == "bf16" else "float"
    if cls:                                                     # attention_cls.hip:176, 189 (any dtype, S <= 1024)
        return (f"mha_cls_fwd_k<{tn}>", f"mha_cls_bwd_k<{tn}>")
    if dtype == "bf16":                                         # attention_api.hip:23, 77: bf16, head dim 64, S <= 512 -> MFMA
        nkt = next(o for o in (2, 4, 8, 14, 16, 32) if o >= (S + 31) // 32 * 2)        # attention_mfma.hip pick_nkt
        vit = nkt == 14 and not drop and not masked and not packed and S > 16 * 12      # mmrca_mha_fwd_mfma, mmrca_mha_bwd_mfma
        if vit:
            fwd = f"mha_fwd_mfma_p_k<14,16>[{_walk(nbh, ncu)}]"                         # mmrca_mha_fwd_mfma
            if S <= 16 * 13:                                                            # mmrca_mha_bwd_mfma
                return (fwd, f"mha_bwd_p_mfma_v_k<14,8,2>[{_walk(nbh, ncu)}]")
            return (fwd, "mha_bwd_fused_mfma_v_k<14,8>")                              # mmrca_mha_bwd_mfma
        # AT_SWITCH (attention_mfma.hip): nkt 2/4/8 run 4 waves; 14/16 run 8 where the call passes W8_PLAIN / W8_DROP,
        # 32 only where it also passes W8_32.  The forward passes (true, false, false) (mmrca_mha_fwd_mfma), dQ (true, true, true)
        # and dK/dV (true, false, true) (mmrca_mha_bwd_mfma).
        def waves(w8_plain, w8_drop, w8_32):
            if nkt <= 8:
                return 4
            w8 = w8_drop if drop else w8_plain
            return 8 if (w8 and (nkt != 32 or w8_32)) else 4
        d = "true" if drop else "false"
        return (f"mha_fwd_mfma_k<{nkt},{d},{waves(True, False, False)}>",
                f"mha_bwd_dq_mfma_k<{nkt},{d},{waves(True, True, True)}>",
                f"mha_bwd_dkv_mfma_k<{nkt},{d},{waves(True, False, True)}>")
    d = "true" if drop else "false"
    if S <= 208:                                                # attention_f32.hip mmrca_mha_f32m_ok; attention_api.hip:25, 79
        nkt = 4 if S <= 64 else (8 if S <= 128 else 13)         # attention_f32.hip nkt_for, mmrca_mha_fwd_f32m
        return (f"mha_fwd_f32m_k<{nkt},{d}>", f"mha_bwd_dq_f32m_k<{d}>", f"mha_bwd_dkv_f32m_k<{d}>")   # mmrca_mha_bwd_f32m (ceil(S/16) tiles)
    # attention_api.hip:26, 81 -> attention_ref.hip: the LDS-staged kernels while their images fit 160 KiB (mmrca_mha_fwd_ref,
    # mmrca_mha_bwd_ref), else the row-per-wave kernels.  Sizes as atl_bytes with ATT_MAX_DH = 128, ATL_WAVES = 16.
    def atl(per_wave, extra):
        return (2 * S * (DH + 1) + extra + 16 * per_wave) * 4
    fwd = "mha_fwd_lds_k<float>" if atl(128 + S, 0) <= 160 * 1024 else "mha_fwd_ref_k<float>"
    if atl(2 * 128 + S, 0) <= 160 * 1024 and atl(2 * 128 + 2 * S, S) <= 160 * 1024:
        return (fwd, "mha_bwd_dq_lds_k<float>", "mha_bwd_dkv_lds_k<float>")
    return (fwd, "mha_bwd_dq_ref_k<float>", "mha_bwd_dkv_ref_k<float>")


def all_cells(ncu):
    """every value cell() can return over the shapes the kernels take (S <= 512, the layouts a call can pass)"""
    out = set()
    for S in range(1, 513):
        for dtype in ("bf16", "f32"):
            for masked, packed in ((False, False), (True, False), (False, True)):
                for drop in (False, True):
                    for nbh in (1, ncu, ncu + 1, 2 * ncu):
                        for cls in (False, True):
                            out.add(cell(S, dtype, masked, packed, drop, nbh, cls, ncu))
    return out


# ------------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, dtype, S, layout, regime, B=None, H=2, lens=None, drop=False, cls=False):
        self.dtype, self.S, self.layout, self.regime, self.drop, self.cls = dtype, S, layout, regime, drop, cls
        self.lens = lens
        self.B = B if B is not None else (len(lens) if lens is not None else 2)
        self.H = H

    @property
    def masked(self):
        return self.layout in ("prefix", "holes")

    @property
    def packed(self):
        return self.layout == "packed"

    def cell(self, ncu):
        return cell(self.S, self.dtype, self.masked, self.packed, self.drop, self.B * self.H, self.cls, ncu)

    def __repr__(self):
        d = "-drop" if self.drop else ""
        c = "cls-" if self.cls else ""
        return f"{c}{self.dtype}-S{self.S}-{self.layout}{d}-{self.regime}-B{self.B}H{self.H}"


def _edge_lens(S, with_empty=True):
    """sequence lengths on the 16-row tile edges (and a fully masked sequence)"""
    ls = [0] if with_empty else []
    for n in (1, 15, 16, 17, 31, 32, 33, S - 1, S):
        if 1 <= n <= S and n not in ls:
            ls.append(n)
    return ls


def _drop_lens(S):
    """edge lengths trimmed so that B * S^2 stays about 2 M (the keep matrix is built on the host)"""
    ls = _edge_lens(S)
    if len(ls) * S * S > 2_200_000:
        ls = [n for n in ls if n in (0, 1, 16, 17, 33, S - 1, S)]
    return ls


def _bh_split(nbh):
    """(B, H) with B * H = nbh: H = 12 where it divides, else the largest divisor <= 16"""
    if nbh % 12 == 0:
        return nbh // 12, 12
    h = max(d for d in range(1, 17) if nbh % d == 0)
    return nbh // h, h


BF16_S = (1, 17, 32, 33, 64, 65, 100, 128, 129, 192, 200, 224, 225, 256, 257, 300, 512)
BF16_ONCE = (17, 64, 100, 192, 225, 300)          # one S per key-tile count 2 / 4 / 8 / 14 / 16 / 32 for the extra variants
F32_S = (1, 17, 64, 65, 128, 129, 197, 208)
CLS_S = (1, 17, 65, 197, 224, 300, 512)


def _cases():
    cs = []
    for S in BF16_S:
        cs.append(Case("bf16", S, "none", "unit"))
        cs.append(Case("bf16", S, "prefix", "loudkeys", lens=_edge_lens(S)))
        cs.append(Case("bf16", S, "packed", "unit", lens=_edge_lens(S)))
    for S in BF16_ONCE:
        cs.append(Case("bf16", S, "none", "peaky", B=3))
        cs.append(Case("bf16", S, "prefix", "peaky", lens=_edge_lens(S)))
        cs.append(Case("bf16", S, "holes", "loudkeys", B=3))
        cs.append(Case("bf16", S, "prefix", "loudkeys", lens=_drop_lens(S), H=1, drop=True))
        cs.append(Case("bf16", S, "packed", "unit", lens=_drop_lens(S), H=1, drop=True))
    return cs


# head counts of the persistent cases, as functions of the CU count (resolved when the test runs, not at collection)
VIT_NBH = {"12": lambda n: 12, "ncu-1": lambda n: n - 1, "ncu": lambda n: n, "ncu+1": lambda n: n + 1, "2ncu": lambda n: 2 * n,
           "2ncu+5": lambda n: 2 * n + 5, "3072": lambda n: 3072}
VIT_S = (193, 197, 208, 209, 224)


def _persistent_case(S, nbh_name, ncu):
    B, H = _bh_split(VIT_NBH[nbh_name](ncu))
    return Case("bf16", S, "none", "peaky" if nbh_name in ("ncu+1", "3072") else "unit", B=B, H=H)


def _f32_cases():
    cs = []
    for S in F32_S:
        cs.append(Case("f32", S, "none", "peaky" if S in (64, 197) else "unit"))
        cs.append(Case("f32", S, "prefix", "loudkeys", lens=_edge_lens(S)))
        cs.append(Case("f32", S, "packed", "unit", lens=_edge_lens(S)))
        cs.append(Case("f32", S, "prefix", "loudkeys", lens=_drop_lens(S), H=1, drop=True))
    cs.append(Case("f32", 209, "none", "peaky"))                           # the LDS-staged reference kernels
    cs.append(Case("f32", 256, "holes", "loudkeys", B=3))                  # LDS-staged forward, row-per-wave backward
    cs.append(Case("f32", 300, "prefix", "loudkeys", lens=_edge_lens(300)))  # the row-per-wave reference kernels
    cs.append(Case("f32", 512, "packed", "unit", lens=_edge_lens(512)))
    return cs


def _cls_cases():
    cs = []
    for dtype in ("bf16", "f32"):
        for S in CLS_S:
            cs.append(Case(dtype, S, "prefix", "loudkeys", lens=_edge_lens(S), cls=True))
            cs.append(Case(dtype, S, "packed", "unit", lens=_edge_lens(S, with_empty=False), cls=True))
    return cs


CASES, F32_CASES, CLS_CASES = _cases(), _f32_cases(), _cls_cases()


# ------------------------------------------------------------------------------------------------------
# inputs, the float64 reference, the kernel calls
# ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need a GPU"
    L.load()
    L.seed_epoch_set(0)           # test_graph_gpu.py moves the mask epoch; the keep matrices below are those of epoch 0
    torch.cuda.synchronize()


def _tdt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _keep(B, H, S):
    """the dropout keep-scale of element (b, h, q, key): counter ((b*H+h)*S+q)*S+key of SEED (include/mmrca.h), float64"""
    idx = np.arange(B * H * S * S, dtype=np.uint64)
    k = (counter_uniform(SEED, idx) >= np.float32(P_DROP)).astype(np.float64) / (1.0 - np.float32(P_DROP))
    return torch.from_numpy(k).view(B, H, S, S).cuda()


class Inputs:
    """one case's kernel buffers and their padded float64 images"""

    def __init__(self, case, seed):
        B, H, S, dev = case.B, case.H, case.S, "cuda"
        g = torch.Generator(device=dev).manual_seed(seed)
        x = torch.randn(B, S, 3, H, DH, generator=g, device=dev, dtype=torch.float64)
        kval = torch.ones(B, S, dtype=torch.bool, device=dev)
        if case.lens is not None:
            kval = torch.arange(S, device=dev)[None, :] < torch.tensor(case.lens, device=dev)[:, None]
        elif case.layout == "holes":
            kval = torch.rand(B, S, generator=g, device=dev) > 0.3
            kval[-1] = False                                   # and one fully masked sequence
        if case.regime == "peaky":
            x[:, :, 0] *= 4.0                                  # scores with sd ~ 4
        if case.regime == "loudkeys" and not case.packed:
            u = torch.randn(DH, generator=g, device=dev, dtype=torch.float64)
            u /= u.norm()
            q, k = x[:, :, 0], x[:, :, 1]
            q -= (q @ u)[..., None] * u
            q += 4.0 * u                                       # every query: 4 along u
            k -= (k @ u)[..., None] * u                        # valid keys: orthogonal to u
            dead = ~kval
            k[dead] = 200.0 * u                                # masked keys: scores 4 * 200 / 8 = 100 above the valid ones
            x[:, :, 2][dead] = 4096.0 * torch.randn(x[:, :, 2][dead].shape, generator=g, device=dev, dtype=torch.float64).sign()
        tdt = _tdt(case.dtype)
        x = x.to(tdt)
        dout = torch.randn(B, S, H, DH, generator=g, device=dev, dtype=torch.float64).to(tdt)
        # token rows of the kernel layout -> padded position b * S + i
        if case.packed:
            lens = torch.tensor(case.lens, device=dev)
            self.pos = torch.cat([b * S + torch.arange(int(n), device=dev) for b, n in enumerate(case.lens)]).long()
            self.cu = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lens.cumsum(0)]).int()
            self.mask = None
        else:
            self.pos = torch.arange(B * S, device=dev)
            self.cu = None
            self.mask = kval.int().contiguous().view(-1) if case.masked else None
        rows = self.rows = self.pos.numel()
        self.qkv = self._loud((rows, 3 * H * DH), tdt, g)
        self.qkv[:rows] = x.view(B * S, 3 * H * DH)[self.pos]
        self.dout = self._loud((rows, H * DH), tdt, g)
        owned = torch.zeros(B * S, dtype=torch.bool, device=dev)
        owned[self.pos] = True
        self.owned = owned.view(B, S)                          # query rows the layout holds
        if case.cls:                                           # the class-token kernels: dout of row 0 only
            self.dout_c = torch.randn(B, H * DH, generator=g, device=dev, dtype=torch.float64).to(tdt)
            d = torch.zeros(B, S, H, DH, dtype=torch.float64, device=dev)
            d[:, 0] = self.dout_c.double().view(B, H, DH)
            self.dout_ref = d * self.owned[:, :, None, None]
        else:
            self.dout[:rows] = dout.view(B * S, H * DH)[self.pos]
            self.dout_ref = dout.double() * self.owned[:, :, None, None]   # no gradient enters at rows the layout lacks
        self.x = x.double()
        self.kval = kval
        self.keep = _keep(B, H, S) if case.drop else None

    @staticmethod
    def _loud(shape, tdt, g):
        """a buffer with SLACK rows of large finite values behind the `shape[0]` rows the caller fills"""
        rows, cols = shape
        t = torch.empty(rows + SLACK, cols, dtype=tdt, device="cuda")
        t[rows:] = (LOUD * torch.randn(SLACK, cols, generator=g, device="cuda").sign()).to(tdt)
        return t


def reference(x, kval, dout, keep, o_in=None):
    """float64 attention forward and backward in the padded layout.  x [B, S, 3, H, dh] (the kernel's q | k | v), kval [B, S]
    (valid keys), dout [B, S, H, dh], keep [B, H, S, S] (dropout keep-scales) or None, o_in [B, S, H, dh]: the out the backward
    is given (D below uses it, as the backward's contract does; None: the exact O).  Returns out, dq, dk, dv [B, S, H, dh],
    lse [B, H, S] (natural log; +inf for a query whose keys are all masked, whose out is exactly 0) and, per output, the same
    products taken over absolute values (the size of the terms a cancelling sum is made of: the floor of the error norms):
      P = softmax(Q K^T scale) over the valid keys, O = (P o keep) V, dV = (P o keep)^T dO, dP = dO V^T, D = rowsum(dO o O),
      dS = P o (dP o keep - D), dQ = dS K scale, dK = dS^T Q scale."""
    B, S, _, H, dh = x.shape
    heads = lambda t: t.permute(0, 2, 1, 3).reshape(B * H, S, dh)   # noqa: E731
    q, k, v = (heads(x[:, :, i]) for i in range(3))
    do = heads(dout)
    oi = heads(o_in) if o_in is not None else None
    km = kval.repeat_interleave(H, 0)                          # [B*H, S]
    kp = keep.reshape(B * H, S, S) if keep is not None else None
    res = {n: torch.zeros(B * H, S, dh, dtype=torch.float64, device=x.device) for n in ("out", "dq", "dk", "dv")}
    mag = {n: torch.zeros(B * H, S, dh, dtype=torch.float64, device=x.device) for n in ("out", "dq", "dk", "dv")}
    lse = torch.empty(B * H, S, dtype=torch.float64, device=x.device)
    ch = max(1, (1 << 24) // (S * S))                          # heads per chunk: 128 MiB per [ch, S, S] float64 temporary
    for i in range(0, B * H, ch):
        j = min(B * H, i + ch)
        s = (q[i:j] @ k[i:j].transpose(1, 2)) * SCALE
        s = s.masked_fill(~km[i:j, None, :], float("-inf"))
        m = s.amax(-1, keepdim=True)
        live = m > float("-inf")
        p = torch.exp(s - torch.where(live, m, torch.zeros_like(m)))
        lsum = p.sum(-1, keepdim=True)
        lse[i:j] = torch.where(live, m + torch.log(lsum), torch.full_like(m, float("inf")))[..., 0]
        p = p / torch.where(live, lsum, torch.ones_like(lsum))
        pk = p * kp[i:j] if kp is not None else p
        o = pk @ v[i:j]
        dP = do[i:j] @ v[i:j].transpose(1, 2)
        dPm = do[i:j].abs() @ v[i:j].abs().transpose(1, 2)    # the size of dP's terms
        if kp is not None:
            dP, dPm = dP * kp[i:j], dPm * kp[i:j]
        ob = oi[i:j] if oi is not None else o
        D, Dm = (do[i:j] * ob).sum(-1, keepdim=True), (do[i:j] * ob).abs().sum(-1, keepdim=True)
        dS = p * (dP - D)
        res["out"][i:j] = o
        res["dq"][i:j] = (dS @ k[i:j]) * SCALE
        res["dk"][i:j] = (dS.transpose(1, 2) @ q[i:j]) * SCALE
        res["dv"][i:j] = pk.transpose(1, 2) @ do[i:j]
        a = p * (dPm + Dm)
        mag["out"][i:j] = pk @ v[i:j].abs()
        mag["dq"][i:j] = (a @ k[i:j].abs()) * SCALE
        mag["dk"][i:j] = (a.transpose(1, 2) @ q[i:j].abs()) * SCALE
        mag["dv"][i:j] = pk.transpose(1, 2) @ do[i:j].abs()
    back = lambda t: t.view(B, H, S, dh).permute(0, 2, 1, 3)   # noqa: E731
    return {n: back(t) for n, t in res.items()}, {n: back(t) for n, t in mag.items()}, lse.view(B, H, S)


def _out_buf(rows, cols, tdt):
    t = torch.full((rows + GUARD, cols), float("nan"), dtype=tdt, device="cuda")
    t[rows:] = SENT
    return t


def _lse_buf(n):
    t = torch.full((n + GUARD,), float("nan"), device="cuda")
    t[n:] = SENT
    return t


def _run(case, inp):
    """forward then backward through the C ABI (the backward fed the forward's own out and lse, as in the product)"""
    B, H, S = case.B, case.H, case.S
    tdt, code = _tdt(case.dtype), L.dtype_code(_tdt(case.dtype))
    p = P_DROP if case.drop else 0.0
    if case.cls:
        out, lse = _out_buf(B, H * DH, tdt), _lse_buf(B * H)
        L.mha_cls_fwd(inp.qkv, inp.mask, out, lse, B, H, S, DH, SCALE, code, drop_p=p, drop_seed=SEED, cu=inp.cu)
        dqkv = _out_buf(inp.rows, 3 * H * DH, tdt)
        L.mha_cls_bwd(inp.qkv, inp.mask, out, inp.dout_c, lse, dqkv, B, H, S, DH, SCALE, code, drop_p=p, drop_seed=SEED, cu=inp.cu)
    else:
        out, lse = _out_buf(inp.rows, H * DH, tdt), _lse_buf(B * H * S)
        L.mha_fwd(inp.qkv, inp.mask, out, lse, B, H, S, DH, SCALE, code, L.IMPL_AUTO, drop_p=p, drop_seed=SEED, cu=inp.cu)
        dqkv = _out_buf(inp.rows, 3 * H * DH, tdt)
        L.mha_bwd(inp.qkv, inp.mask, out, inp.dout, lse, dqkv, B, H, S, DH, SCALE, code, L.IMPL_AUTO, drop_p=p, drop_seed=SEED,
                  cu=inp.cu)
    torch.cuda.synchronize()
    return out, lse, dqkv


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _block_errors(got, ref, mag, seq, B):
    """got / ref / mag [rows, H, dh] (float64), seq [rows] = the sequence of each row.  Per (sequence, head) block:
    max |err| / max |ref|; per row: max |err| / max(max |ref| of the row, 1e-2 x the block's).  Both denominators are floored at
    1e-2 x the size of the terms (mag): where the exact result cancels to nothing (dQ / dK of a query with a single valid key is
    exactly 0) only rounding noise of that size is left.  A block (row) whose reference and terms are all 0 must be exactly 0."""
    H = got.shape[1]
    er, rr, mr = (got - ref).abs().amax(-1), ref.abs().amax(-1), mag.abs().amax(-1)               # [rows, H]
    amax = lambda t: torch.zeros(B, H, dtype=torch.float64, device=got.device).index_reduce_(0, seq, t, "amax")   # noqa: E731
    eb, rb, mb = amax(er), amax(rr), amax(mr)

    def ratio(e, r):
        return torch.where(r > 0, e / torch.where(r > 0, r, torch.ones_like(r)),
                           torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
    return ratio(eb, torch.maximum(rb, 1e-2 * mb)), ratio(er, torch.maximum(torch.maximum(rr, 1e-2 * rb[seq]), 1e-2 * mr))


OBSERVED = {}     # (dtype, segment) -> worst (block, row) error over the cases run


def _check(case, inp, res, tag):
    out, lse, dqkv = res
    B, H, S, rows = case.B, case.H, case.S, inp.rows
    # (class-token kernels: the sequences that have a row 0)
    has = torch.tensor([n > 0 for n in case.lens] if case.packed else [True] * B, device="cuda")
    # the reference backward takes D from the out the kernel's backward was given
    o_in = torch.zeros(B * S, H, DH, dtype=torch.float64, device="cuda")
    if case.cls:
        o_in.view(B, S, H, DH)[:, 0] = out[:B].double().view(B, H, DH) * has[:, None, None]
    else:
        o_in[inp.pos] = out[:rows].double().view(rows, H, DH)
    ref, mag, r_lse = reference(inp.x, inp.kval, inp.dout_ref, inp.keep, o_in.view(B, S, H, DH))
    r_out = ref["out"]
    # nothing written past the end
    for name, buf, n in (("out", out, B if case.cls else rows), ("dqkv", dqkv, rows)):
        assert torch.equal(buf[n:], torch.full_like(buf[n:], SENT)), f"{tag}: {name} guard rows were written"
    nl = B * H if case.cls else B * H * S
    assert torch.equal(lse[nl:], torch.full_like(lse[nl:], SENT)), f"{tag}: lse guard was written"
    # which rows the layout owns, and the reference rows they correspond to
    seq = inp.pos // S
    if case.cls:
        o_rows = torch.nonzero(has)[:, 0]
        got_out = out[:B][o_rows].double().view(-1, H, DH)
        ref_out, mag_out = r_out[:, 0][o_rows], mag["out"][:, 0][o_rows]
        o_seq = o_rows
        got_lse, ref_lse = lse[:B * H].view(B, H)[o_rows].double(), r_lse[:, :, 0][o_rows]
    else:
        got_out = out[:rows].double().view(rows, H, DH)
        ref_out, mag_out = r_out.reshape(B * S, H, DH)[inp.pos], mag["out"].reshape(B * S, H, DH)[inp.pos]
        o_seq = seq
        own = inp.owned[:, None, :].expand(B, H, S)
        got_lse, ref_lse = lse[:B * H * S].view(B, H, S)[own].double(), r_lse[own]
    g3 = dqkv[:rows].double().view(rows, 3, H, DH)
    segs = {"out": (got_out, ref_out, mag_out, o_seq)}
    for i, name in enumerate(("dq", "dk", "dv")):
        segs[name] = (g3[:, i], ref[name].reshape(B * S, H, DH)[inp.pos], mag[name].reshape(B * S, H, DH)[inp.pos], seq)
    # every owned row written
    for name, (g, _, _, _) in segs.items():
        bad = ~torch.isfinite(g).all(-1).all(-1)
        assert not bool(bad.any()), f"{tag}: {name} rows not written / not finite: {torch.nonzero(bad)[:8, 0].tolist()}"
    # lse: finite exactly where the reference is, +inf elsewhere, within bound x max(1, |lse|)
    fin = torch.isfinite(ref_lse)
    assert torch.equal(torch.isfinite(got_lse), fin), f"{tag}: lse finite where the reference is not (or the reverse)"
    assert bool((got_lse[~fin] == float("inf")).all()), f"{tag}: lse of a query without valid keys is not +inf"
    lerr = float(((got_lse[fin] - ref_lse[fin]).abs() / ref_lse[fin].abs().clamp(min=1.0)).max()) if bool(fin.any()) else 0.0
    # exact zeros: the dK / dV rows of every masked key, everything of a fully masked sequence
    if case.masked:
        dead = ~inp.kval.view(-1)[inp.pos]
        for i, name in ((1, "dk"), (2, "dv")):
            nz = g3[dead, i].abs().amax(-1).amax(-1) != 0
            assert not bool(nz.any()), f"{tag}: {name} of masked keys not exactly 0 (rows {torch.nonzero(dead)[:, 0][nz][:8].tolist()})"
        for b in range(B):
            if not bool(inp.kval[b].any()):
                rows_b = seq == b
                assert float(g3[rows_b].abs().max()) == 0.0, f"{tag}: gradients of fully masked sequence {b} not exactly 0"
                ob = o_seq == b
                if bool(ob.any()):
                    assert float(got_out[ob].abs().max()) == 0.0, f"{tag}: out of fully masked sequence {b} not exactly 0"
    if case.cls:                                               # the class-token backward zeroes dQ outside row 0
        first = torch.ones(rows, dtype=torch.bool, device="cuda")
        first[inp.pos % S == 0] = False
        if bool(first.any()):
            assert float(g3[first, 0].abs().max()) == 0.0, f"{tag}: dQ rows >= 1 not exactly 0"
    # per block and per row
    dt = case.dtype
    msg = [f"{tag} [{' '.join(case.cell(_ncu()))}]:"]
    fails = []
    for name, (g, r, mg, sq) in segs.items():
        blk, row = _block_errors(g, r, mg, sq, B)
        wb, wr = float(blk.max()), float(row.max())
        bound = BOUND[(dt, name)]
        msg.append(f"{name} {wb:.2e}/{wr:.2e}")
        prev = OBSERVED.get((dt, name), (0.0, 0.0))
        OBSERVED[(dt, name)] = (max(prev[0], wb), max(prev[1], wr))
        if wb > bound:
            b, h = divmod(int(blk.argmax()), H)
            fails.append(f"{name}: block (b={b}, h={h}) error {wb:.3e} > {bound:.1e}")
        if wr > bound:
            rr, h = divmod(int(row.argmax()), H)
            fails.append(f"{name}: row {rr} (b={int(sq[rr])}, h={h}) error {wr:.3e} > {bound:.1e}")
    msg.append(f"lse {lerr:.2e}")
    OBSERVED[(dt, "lse")] = (max(OBSERVED.get((dt, "lse"), (0.0, 0.0))[0], lerr), 0.0)
    print(" ".join(msg))
    lb = LSE_BOUND_PERSISTENT if case.cell(_ncu())[0].startswith("mha_fwd_mfma_p_k") else LSE_BOUND[dt]
    if lerr > lb:
        fails.append(f"lse error {lerr:.3e} > {lb:.0e}")
    assert not fails, f"{tag} [{' '.join(case.cell(_ncu()))}]: " + "; ".join(fails)


def _case_test(case, seed):
    inp = Inputs(case, seed)
    res = _run(case, inp)
    _check(case, inp, res, repr(case))
    again = _run(case, inp)
    for name, a, b in zip(("out", "lse", "dqkv"), res, again):
        assert torch.equal(_bits(a), _bits(b)), f"{case!r}: {name} differs bitwise between two identical runs"


# ------------------------------------------------------------------------------------------------------
# the tests
# ------------------------------------------------------------------------------------------------------
def test_the_case_list_reaches_every_dispatch_cell():
    ncu = _ncu()
    vit = [_persistent_case(S, n, ncu) for S in VIT_S for n in VIT_NBH]
    reached = {c.cell(ncu) for c in CASES + F32_CASES + CLS_CASES + vit}
    missing = all_cells(ncu) - reached
    assert not missing, f"cells no case reaches: {sorted(missing)}"


def test_attention_sources_have_no_float_atomics():
    """bitwise reproducibility rests on fixed summation orders: no atomic read-modify-write in the attention kernels
    (the optional bias column sums of mmrca_mha_bwd_colsum run in a separate pass outside these files)"""
    pat = re.compile(r"\batomic\w*\s*\(|__hip_atomic|global_atomic|ds_add_|buffer_atomic|unsafeAtomic")
    for f in sorted(os.listdir(CSRC)):
        if f.startswith("attention_") and f.endswith(".hip"):
            with open(os.path.join(CSRC, f)) as fh:
                for n, line in enumerate(fh, 1):
                    code = line.split("//")[0]
                    assert not pat.search(code), f"{f}:{n}: {line.strip()}"


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_bf16_generic_kernels_match_float64(case):
    _case_test(case, seed=case.S * 7 + len(repr(case)))


@pytest.mark.parametrize("nbh", list(VIT_NBH))
@pytest.mark.parametrize("S", VIT_S)
def test_bf16_vit_kernels_walking_heads_match_float64(S, nbh):
    """the persistent forward / backward (S 193..208) and the fused backward (209..224): B*H from one head per workgroup to twelve
    rounds, the ragged last round included"""
    case = _persistent_case(S, nbh, _ncu())
    _case_test(case, seed=S * 13 + case.B)


@pytest.mark.parametrize("case", F32_CASES, ids=repr)
def test_f32_kernels_match_float64(case):
    _case_test(case, seed=case.S * 11 + len(repr(case)))


@pytest.mark.parametrize("case", CLS_CASES, ids=repr)
def test_class_token_kernels_match_row0_of_float64(case):
    _case_test(case, seed=case.S * 17 + len(repr(case)))
