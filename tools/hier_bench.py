#!/usr/bin/env python
"""Timing of the hierarchical late-fusion head (csrc/hier_head.hip) and of the model it belongs to, on the GPU:

    python tools/hier_bench.py kernels     # per-launch time of every new kernel at B = 16 / 64 / 256, and the wide Linear + ReLU against
                                           # mmrca_gemm in fp32 mode on the same shapes (the isolation table of DESIGN.md)
    python tools/hier_bench.py steps       # train-step rate of Hierarchical against MM_RCA on the same backbones
                                           # (EfficientNetV2-M @ 480 + DistilBERT, bf16x3f, B = 16 / 64, frozen and fine-tuning)

Device events around `reps` back-to-back calls after a warm-up; one JSON line per measurement."""
import contextlib
import io
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from garbage_classification_rca_amd import lib as L  # noqa: E402

DEV = "cuda:0"
SEG = [0, 1280, 3840, 5888, 6656, 7424, 8192]


def timed(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def ru(x, m):
    return (x + m - 1) // m * m


def kernels():
    for B in (16, 64, 256):
        out = {}
        for name, H, C, k in (("stage3", 30, 160, 7), ("stage6", 15, 512, 6)):
            for dt, code in ((torch.bfloat16, L.BF16), (torch.float32, L.F32)):
                x = torch.randn(B * H * H, C, device=DEV).to(dt)
                raw = torch.zeros(B, 8192, device=DEV)
                tag = f"pool_{name}_{'bf16' if code == L.BF16 else 'fp32'}"
                out[tag + "_fwd"] = timed(lambda: L.hier_pool_fwd(x, raw, 8192, B, H, H, C, k, code))
                out[tag + "_bwd"] = timed(lambda: L.hier_pool_bwd(raw, 8192, x, B, H, H, C, k, code))
        raw = torch.randn(B, 8192, device=DEV)
        x, inv, draw = torch.empty_like(raw), torch.empty(B, 6, device=DEV), torch.empty_like(raw)
        out["norm_fwd_p0.6"] = timed(lambda: L.hier_norm_fwd(raw, x, inv, B, 8192, SEG, 3, 0.6, 1, 2))
        out["norm_bwd_p0.6"] = timed(lambda: L.hier_norm_bwd(raw, raw, inv, draw, B, 8192, SEG, 3, 0.6, 1, 2))
        print(json.dumps({"what": "per-call us", "B": B, **{k: round(v, 2) for k, v in out.items()}}))
        for K in (5888, 2304):
            N, Bp = 512, ru(B, 64)
            X = torch.zeros(Bp, K, device=DEV)
            X[:B] = torch.randn(B, K, device=DEV) * K ** -0.5
            W, b = torch.randn(N, K, device=DEV), torch.randn(N, device=DEV)
            Y, dY = torch.zeros(Bp, N, device=DEV), torch.zeros(Bp, N, device=DEV)
            dY[:B] = torch.randn(B, N, device=DEV)
            dW, db, dX = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV), torch.zeros(Bp, K, device=DEV)
            ws = torch.empty(L.hier_linear_workspace_bytes(B, N, K), dtype=torch.uint8, device=DEV)
            r = {"what": "linear us", "B": B, "N": N, "K": K}
            r["hier_fwd"] = timed(lambda: L.hier_linear_relu_fwd(X, K, W, b, Y, N, ws, B, N, K))
            r["gemm_fwd"] = timed(lambda: L.gemm(X, W, Y, bias=b, M=B, N=N, K=K, lda=K, ldb=K, ldc=N, dtype=L.F32))      # (without the ReLU)
            r["hier_bwd_wgrad_only"] = timed(lambda: L.hier_linear_relu_bwd(dY, N, Y, N, X, K, W, dW, db, None, K, None, B, N, K))
            r["hier_bwd"] = timed(lambda: L.hier_linear_relu_bwd(dY, N, Y, N, X, K, W, dW, db, dX, K, ws, B, N, K))
            r["gemm_wgrad"] = timed(lambda: L.gemm(dY, X, dW, M=N, N=K, K=Bp, lda=N, ldb=K, ldc=K, a_layout=L.KROW, b_layout=L.KROW, accum=True,
                                                   dtype=L.F32))
            r["gemm_dgrad"] = timed(lambda: L.gemm(dY, W, dX, M=B, N=K, K=N, lda=N, ldb=K, ldc=K, a_layout=L.ROWK, b_layout=L.KROW, dtype=L.F32))
            r["gemm_bwd"] = r["gemm_wgrad"] + r["gemm_dgrad"]            # (without the ReLU gate and the bias gradient)
            print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()}))


def steps():
    from garbage_classification_rca_amd import engine as E
    from garbage_classification_rca_amd.multimodal_model import MM_RCA, Hierarchical
    from garbage_classification_rca_amd.optim import FlatAdamW
    from garbage_classification_rca_amd.procedural import synth_captions
    from garbage_classification_rca_amd.training import FusedCrossEntropy, hip_train_step
    for B in (16, 64):
        ids_np, mask_np = synth_captions(B, 64, seed=1)
        ids, mask = torch.from_numpy(ids_np).to(DEV), torch.from_numpy(mask_np).to(DEV)
        images = torch.randn(B, 3, 480, 480, device=DEV)
        labels = (torch.arange(B, device=DEV) % 4)
        pack = E.make_text_pack(mask_np, DEV)
        for name in ("MM_RCA", "Hierarchical"):
            with contextlib.redirect_stdout(io.StringIO()):
                m = (MM_RCA(4, 0.6, 0.0, 0.7, 256, "distilbert", B, True, False, False) if name == "MM_RCA"
                     else Hierarchical(4, 0.6, 0.0, 0.7, 256, "distilbert", B, True))
            m.train()
            opt, crit = FlatAdamW(m, lr=1e-4, weight_decay=1e-2), FusedCrossEntropy(None, 0.0)
            for phase in ("frozen", "fine-tuning"):
                if phase == "fine-tuning":
                    for p in m.parameters():
                        p.requires_grad = True
                us = timed(lambda: hip_train_step(m, ids, mask, images, labels, crit, opt, text_pack=pack), reps=12, warm=3)
                print(json.dumps({"what": "train step", "model": name, "B": B, "phase": phase, "ms_per_step": round(us / 1e3, 2),
                                  "samples_per_s": round(B / (us / 1e6), 1)}))
            m.engine.release_buffers()
            del m, opt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    {"kernels": kernels, "steps": steps}[sys.argv[1] if len(sys.argv) > 1 else "kernels"]()
