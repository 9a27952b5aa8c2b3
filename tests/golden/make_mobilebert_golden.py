"""Writes tests/golden/mobilebert_goldens.npz from transformers' own ``MobileBertForSequenceClassification`` in float64: two layers,
everything else the configuration of google/mobilebert-uncased with ``classifier_activation=False``, the procedural weights and
inputs of tests/mobilebert_ref.py (B = 3, T = 16, live lengths 16, 9, 1).  Records the inputs, dlogits, the logits,
``hidden_states[1]`` at the three class-token rows and four parameter gradients of sum(logits * dlogits); no weights.  To keep the file
to tens of kilobytes the two large gradient matrices are recorded as every GOLDEN_ROW_STRIDE-th row plus the largest entry of the whole
matrix (``gradmax:``), which the tolerances are relative to; the GPU tests check every full gradient against the float64 restatement.

    python tests/golden/make_mobilebert_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.mobilebert_ref import GOLDEN, GOLDEN_GRADS, GOLDEN_ROW_STRIDE, golden_inputs, proc_state  # noqa: E402


def main():
    from transformers import MobileBertConfig, MobileBertForSequenceClassification
    cfg = MobileBertConfig(classifier_activation=False, num_labels=4, num_hidden_layers=2)
    model = MobileBertForSequenceClassification(cfg).double().eval()
    model.load_state_dict({k: v.double() for k, v in proc_state(model).items()}, strict=True)
    ids, mask, dlogits = golden_inputs()
    out = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    (out.logits * dlogits.double()).sum().backward()
    params = dict(model.named_parameters())
    rec = dict(ids=ids.numpy(), mask=mask.numpy(), dlogits=dlogits.numpy(), logits=out.logits.detach().numpy(),
               hidden1_cls=out.hidden_states[1][:, 0].detach().numpy())
    for k in GOLDEN_GRADS:
        g = params[k].grad
        rec["gradmax:" + k] = g.abs().max().numpy()
        rec["grad:" + k] = g[::GOLDEN_ROW_STRIDE.get(k, 1)].numpy()
    np.savez_compressed(GOLDEN, **rec)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes; max |logit|", float(out.logits.detach().abs().max()))


if __name__ == "__main__":
    main()
