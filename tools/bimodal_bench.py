#!/usr/bin/env python
"""Timing of the bimodal GRU late-fusion head (csrc/gru.hip) and of the model it belongs to, on the GPU:

    python tools/bimodal_bench.py chains    # the forward and backward recurrent chains alone at T = 4 / 32 / 64: gru_text + gru_audio in
                                            # one chain (H = 400, two GRUs per launch) and gru_bimodal (H = 500); total and per step
    python tools/bimodal_bench.py head      # the whole head, forward and backward, at B = 4 / 32 / 64 (every launch between the encoders'
                                            # features and the logits)
    python tools/bimodal_bench.py steps     # train-step rate of HierarchicalBimodalFusion against MM_RCA on the same backbones
                                            # (EfficientNetV2-M @ 480 + DistilBERT, bf16x3f, B = 4 / 32, frozen and fine-tuning), the two
                                            # models alternating
    python tools/bimodal_bench.py logits    # logits error of the four dtype modes against the float64 restatement at 224 and 480

Device events around `reps` back-to-back calls after a warm-up; one JSON line per measurement."""
import contextlib
import io
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from garbage_classification_rca_amd import lib as L  # noqa: E402

DEV = "cuda:0"


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


def chains():
    for T in (4, 32, 64):
        for name, n, hid in (("gru_text+gru_audio", 2, 400), ("gru_bimodal", 1, 500)):
            mk = lambda *s: [torch.randn(*s, device=DEV) * hid ** -0.5 for _ in range(n)]
            gi, whh, bhh, d = mk(T, 3 * hid), mk(3 * hid, hid), mk(3 * hid), mk(T, hid)
            hseq = [torch.zeros(T + 1, hid, device=DEV) for _ in range(n)]
            gates, hn, carry, dgi, dgh = mk(T, 3 * hid), mk(T, hid), mk(T, hid), mk(T, 3 * hid), mk(T, 3 * hid)
            fwd = timed(lambda: L.gru_fwd(gi, whh, bhh, hseq, gates, hn, T, hid))
            bwd = timed(lambda: L.gru_bwd(whh, hseq, gates, hn, d, [hid] * n, carry, dgi, dgh, T, hid))
            print(json.dumps({"what": "recurrent chain us", "chain": name, "T": T, "H": hid, "fwd": round(fwd, 1), "fwd_per_step": round(fwd / T, 2),
                              "bwd": round(bwd, 1), "bwd_per_step": round(bwd / T, 2)}))


def head():
    from garbage_classification_rca_amd.bimodal_engine import BimodalEngine
    eng = BimodalEngine("distilbert", "eff_v2_medium", 4, "fp32", image_size=64)
    eng.init_parameters(0)
    for B in (4, 32, 64):
        cls, feat = torch.randn(B, 768, device=DEV), torch.randn(B, 1280, device=DEV)
        dl = torch.randn(B, 4, device=DEV)
        sv = {}

        def fwd():
            _, s = eng._head_forward(cls, feat, B, 0.86, (1, 2))
            sv.update(s, drop_p=0.86, seeds=(1, 2))
        f = timed(fwd)
        b = timed(lambda: eng._head_backward(dl, sv, B, True))
        print(json.dumps({"what": "whole head us", "B": B, "fwd": round(f, 1), "bwd": round(b, 1)}))
    eng.release_buffers()


def steps():
    from garbage_classification_rca_amd import engine as E
    from garbage_classification_rca_amd.multimodal_model import MM_RCA, HierarchicalBimodalFusion
    from garbage_classification_rca_amd.optim import FlatAdamW
    from garbage_classification_rca_amd.procedural import synth_captions
    from garbage_classification_rca_amd.training import FusedCrossEntropy, hip_train_step
    for B in (4, 32):
        ids_np, mask_np = synth_captions(B, 64, seed=1)
        ids, mask = torch.from_numpy(ids_np).to(DEV), torch.from_numpy(mask_np).to(DEV)
        images = torch.randn(B, 3, 480, 480, device=DEV)
        labels = (torch.arange(B, device=DEV) % 4)
        pack = E.make_text_pack(mask_np, DEV)
        ms = {}
        with contextlib.redirect_stdout(io.StringIO()):
            ms["MM_RCA"] = MM_RCA(4, 0.6, 0.0, 0.7, 256, "distilbert", B, True, False, False)
            ms["HierarchicalBimodalFusion"] = HierarchicalBimodalFusion(4, 0.6, 0.0, 0.7, 256, "distilbert", B, True)
        run = {}
        for name, m in ms.items():
            m.train()
            run[name] = (m, FlatAdamW(m, lr=1e-4, weight_decay=1e-2), FusedCrossEntropy(None, 0.0))
        for phase in ("frozen", "fine-tuning"):
            if phase == "fine-tuning":
                for m in ms.values():
                    for p in m.parameters():
                        p.requires_grad = True
            for rnd in range(2):                         # alternating: MM_RCA, bimodal, MM_RCA, bimodal
                for name, (m, opt, crit) in run.items():
                    us = timed(lambda: hip_train_step(m, ids, mask, images, labels, crit, opt, text_pack=pack), reps=10, warm=3)
                    print(json.dumps({"what": "train step", "model": name, "B": B, "phase": phase, "round": rnd, "ms_per_step": round(us / 1e3, 2),
                                      "samples_per_s": round(B / (us / 1e6), 1)}))
        for m in ms.values():
            m.engine.release_buffers()
        del ms, run
        torch.cuda.empty_cache()


def logits():
    from garbage_classification_rca_amd.bimodal_engine import BimodalEngine
    from garbage_classification_rca_amd.procedural import proc_input, synth_captions
    from tests import bimodal_ref as BR
    B = 3
    ids_np, mask_np = synth_captions(B, 32, seed=21)
    ids, mask = torch.from_numpy(ids_np), torch.from_numpy(mask_np)
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    for size in (224, 480):
        images = torch.from_numpy(proc_input(f"bimodal.images.{size}", (B, 3, size, size)))
        eng = BimodalEngine("distilbert", "eff_v2_medium", 4, "fp32", image_size=size)
        eng.init_parameters(0)
        orc = BR.OracleBimodal().eval()
        orc.load_engine(eng)
        orc = orc.double()
        eng.release_buffers()
        with torch.no_grad():
            ref = orc(ids, mask, images.double())
        out = {"what": "logits error vs float64", "size": size, "scale": float(ref.abs().max())}
        for dtype in ("fp32", "bf16x3", "bf16x3f", "bf16"):
            eng = BimodalEngine("distilbert", "eff_v2_medium", 4, dtype, image_size=size)
            eng.init_parameters(0)
            got = eng.forward(ids.cuda(), mask.cuda(), images.cuda(), save=False, bn_train=False).double().cpu()
            out[dtype] = float((got - ref).abs().max() / ref.abs().max())
            eng.release_buffers()
        print(json.dumps(out))


if __name__ == "__main__":
    {"chains": chains, "head": head, "steps": steps, "logits": logits}[sys.argv[1] if len(sys.argv) > 1 else "chains"]()
