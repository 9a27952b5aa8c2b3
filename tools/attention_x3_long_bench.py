#!/usr/bin/env python
"""The bf16x3f attention forward at T = 512 (12 heads x 64): what the text encoder ran before mmrca_mha_fwd_x3 took S > 224 --
the fp32 forward (mmrca_mha_fwd, which lands on attention_ref.hip there) plus the cast_f32_to_bf16 pass over q|k|v that gave the
bf16 backward its operands -- against mmrca_mha_fwd_x3 on the hi / lo planes.  Both run from this library (the fp32 route is
unchanged), alternating, HIP events around each group of launches after a warm-up; per shape the median over the rounds and every
round's value.  The two contexts are compared first (faster and different is not faster).

    python tools/attention_x3_long_bench.py --rounds 5 --out profiles/attention_x3_long.json
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from garbage_classification_rca_amd import lib as L  # noqa: E402

H, DH = 12, 64
D = H * DH


def shapes():
    g = torch.Generator().manual_seed(0)
    T = 512
    full = torch.full((16,), T)
    one_dead = full.clone()
    one_dead[5] = 0
    short = torch.randint(6, 15, (16,), generator=g)
    long_ = torch.randint(100, 401, (128,), generator=g)
    return [("B16_S512_padded_all_live", 16, T, full, False), ("B16_S512_padded_one_caption_masked", 16, T, one_dead, False),
            ("B16_T512_packed_len_6_14", 16, T, short, True), ("B128_T512_packed_len_100_400", 128, T, long_, True)]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    L.load()
    sc = 1 / math.sqrt(DH)
    res = []
    for name, B, T, lens, packed in shapes():
        kval = torch.arange(T)[None, :] < lens[:, None]
        if packed:
            pos = torch.nonzero(kval.reshape(-1))[:, 0].cuda()
            rows = int(lens.sum())
            cu = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).int().cuda()
            mask = torch.ones(rows, dtype=torch.int32, device="cuda")
        else:
            rows, cu, mask = B * T, None, kval.int().contiguous().view(-1).cuda()
        g = torch.Generator(device="cuda").manual_seed(B)
        x = torch.randn(rows, 3 * D, device="cuda", generator=g)
        hi = x.bfloat16()
        lo = (x - hi.float()).bfloat16()
        qkv32 = hi.float() + lo.float()
        qkv16 = torch.empty(rows, 3 * D, dtype=torch.bfloat16, device="cuda")
        ctx32 = torch.zeros(rows, D, device="cuda")
        pl = (torch.zeros(rows, D, dtype=torch.bfloat16, device="cuda"), torch.zeros(rows, D, dtype=torch.bfloat16, device="cuda"))
        lse_p, lse_c = torch.zeros(B * H * T, device="cuda"), torch.zeros(B * H * T, device="cuda")

        def parent():
            L.mha_fwd(qkv32, mask, ctx32, lse_p, B, H, T, DH, sc, L.F32, cu=cu)
            L.cast_f32_to_bf16(qkv32, qkv16, rows * 3 * D)

        def change():
            L.mha_fwd_x3((hi, lo), mask, pl, lse_c, B, H, T, DH, sc, cu=cu)

        parent(); change()
        torch.cuda.synchronize()
        diff = float((pl[0].float() + pl[1].float() - ctx32).abs().max()) / float(ctx32.abs().max())
        t1 = timed(parent, 2)
        ip, ic = max(3, min(200, int(2e5 / t1))), 200           # ~0.2 s of parent work per round
        for _ in range(3):
            change()
        rp, rc = [], []
        for _ in range(a.rounds):
            rp.append(round(timed(parent, ip), 1))
            rc.append(round(timed(change, ic), 1))
        mp, mc = sorted(rp)[len(rp) // 2], sorted(rc)[len(rc) // 2]
        row = dict(shape=name, B=B, H=H, T=T, dh=DH, rows=rows, live_tokens=int(lens.sum()), packed=packed,
                   parent_us=mp, change_us=mc, speedup=round(mp / mc, 2), parent_rounds_us=rp, change_rounds_us=rc,
                   launches_per_parent_round=ip, launches_per_change_round=ic, context_max_diff_rel=diff)
        print(json.dumps(row), flush=True)
        res.append(row)
    doc = dict(what="tools/attention_x3_long_bench.py on one MI355X: bf16x3f attention forward at T = 512, 12 heads x 64; parent = mmrca_mha_fwd (fp32) + "
                    "mmrca_cast_f32_to_bf16 over q|k|v, change = mmrca_mha_fwd_x3 on the planes; HIP events, rounds alternate parent and change, "
                    "median of the rounds in *_us",
               device=torch.cuda.get_device_name(0), shapes=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
