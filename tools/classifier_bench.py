#!/usr/bin/env python
"""Train-step throughput of the single-modality classifiers (classifiers.py) on one GPU: samples/s of the fine-tuning step (every
parameter trainable: forward, cross entropy, backward, SGD step, gradient zeroing) on synthetic inputs resident in HBM.

    python tools/classifier_bench.py [--steps 10] [--warmup 3] [--only vit_b16_bf16,...]

Configurations: ViT-B/16 image-only at B = 128 in bf16 and bf16x3f, DistilBERT text-only at B = 128 (captions of 64 tokens, as bench.py),
EfficientNetV2-M at 480 x 480, B = 64 (bf16x3f), MobileNetV3-Large at 320 x 320, B = 256 (bf16 and bf16x3f), and, for comparison, the MM_RCA ViT-B/16 + DistilBERT step at B = 128 in bf16.
MobileBERT text-only (fp32) at the reference's two launch shapes -- B = 18 with the encoder frozen and B = 4 fine-tuning, captions of
10-20 live tokens padded to 512 -- launched from Python (live tokens packed, as the driver's eager step does) and as a captured HIP
graph (padded layout, as --hip_graph on does).
One JSON line per configuration.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from garbage_classification_rca_amd import classifiers as C                      # noqa: E402
from garbage_classification_rca_amd.optim import FlatSGD                         # noqa: E402
from garbage_classification_rca_amd.procedural import proc_input, synth_captions  # noqa: E402
from garbage_classification_rca_amd.engine import make_text_pack                 # noqa: E402
from garbage_classification_rca_amd.training import FusedCrossEntropy, GraphedTrainStep, hip_train_step  # noqa: E402

CONFIGS = {
    "vit_b16_bf16": ("image", "transformer_B16", "bf16", 128),
    "vit_b16_bf16x3f": ("image", "transformer_B16", "bf16x3f", 128),
    "distilbert_bf16x3f": ("text", "distilbert", "bf16x3f", 128),
    "effv2m_480_bf16x3f": ("image", "eff_v2_medium", "bf16x3f", 64),
    "mb_320_bf16": ("image", "mb", "bf16", 256),
    "mb_320_bf16x3f": ("image", "mb", "bf16x3f", 256),
    "mm_rca_vit_b16_distilbert_bf16": ("both", "transformer_B16", "bf16", 128),
    # (kind, model, dtype, batch, options: frozen encoder / caption length T with 10-20 live tokens / captured HIP graph)
    "mobile_bert_b18_frozen": ("text", "mobile_bert", "fp32", 18, dict(frozen=True, T=512)),
    "mobile_bert_b18_frozen_graph": ("text", "mobile_bert", "fp32", 18, dict(frozen=True, T=512, graph=True)),
    "mobile_bert_b4_ft": ("text", "mobile_bert", "fp32", 4, dict(T=512)),
    "mobile_bert_b4_ft_graph": ("text", "mobile_bert", "fp32", 4, dict(T=512, graph=True)),
    "mobile_bert_b4_ft_bf16": ("text", "mobile_bert", "bf16", 4, dict(T=512)),
}


def build(kind, name, dtype):
    if kind == "image":
        return C.IMAGE_FACTORIES[name](4, False, dtype=dtype, device="cuda")
    if kind == "text":
        m = C.build_text_classifier(name, 4, 0.1, dtype, "cuda")
    else:
        from garbage_classification_rca_amd.multimodal_model import MM_RCA
        m = MM_RCA(4, 0.6, 0.0, 0.7, 256, "distilbert", 128, True, False, False, image_model_name=name,
                   dtype=torch.bfloat16 if dtype == "bf16" else dtype, build_unused_parameters=False)
    return m


def run(tag, kind, name, dtype, B, steps, warmup, frozen=False, T=64, graph=False):
    m = build(kind, name, dtype)
    for p in m.parameters():
        p.requires_grad = p.requires_grad if frozen else True
    m.train()
    side = m.get_image_size()[0] if kind != "text" else 1
    images = torch.from_numpy(proc_input("cls_bench", (B, 3, side, side))).cuda() if kind != "text" else torch.zeros(B, 0, device="cuda")
    if T == 64:
        ids_h, mask_h = (torch.from_numpy(a) for a in synth_captions(B, 64, seed=3))
    else:                       # 10-20 live tokens, padded to T
        ids_h, mask_h = (torch.nn.functional.pad(torch.from_numpy(a), (0, T - 20)) for a in synth_captions(B, 20, seed=3, min_len=10))
    ids, mask = ids_h.cuda(), mask_h.cuda()
    labels = (torch.arange(B, device="cuda") % 4)
    opt, crit = FlatSGD(m, 1e-3, 1e-2), FusedCrossEntropy()
    if graph:
        graphed = GraphedTrainStep(m, crit, opt, warmup=2)
        step = lambda: graphed(ids, mask, images, labels)                                                   # noqa: E731
        warmup = max(warmup, 4)
    else:
        pack = make_text_pack(mask_h, "cuda") if T != 64 else None
        step = lambda: hip_train_step(m, ids, mask, images, labels, crit, opt, text_pack=pack)            # noqa: E731
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    print(json.dumps(dict(config=tag, model=name, dtype=dtype, batch=B, step_ms=round(dt * 1e3, 3), samples_per_s=round(B / dt, 1),
                          loss=round(float(loss), 5))), flush=True)
    m.engine.release_buffers()
    del m, opt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("classifier_bench.py needs a GPU")
    for tag, cfg in CONFIGS.items():
        if a.only and tag not in a.only.split(","):
            continue
        run(tag, *cfg[:4], a.steps, a.warmup, **(cfg[4] if len(cfg) > 4 else {}))


if __name__ == "__main__":
    main()
