"""Restatement of the hierarchical late-fusion model (the reference's ``Hierarchical.forward``, CVPR_code/multimodal_model.py:729-818)
composed from the oracle's parts, in whatever dtype it is cast to (the tests use float64):

    text:   t0 = last_hidden_state[:, 0], t2 = hidden_states[2][:, 0], t4 = hidden_states[4][:, 0]
            (hidden_states[0] is the embedding output, so hidden_states[n] is the output of encoder layer n - 1)
    image:  (out_stage3, out_stage6, pooled) of EfficientNetV2-M; p3 = AvgPool2d(7, 7)(out_stage3), p6 = AvgPool2d(6, 6)(out_stage6),
            flattened in NCHW order
    head:   every one of the six vectors divided by its L2 norm; xi = cat(f, p3, p6), xt = cat(t0, t2, t4); dropout on each;
            hi = relu(Li(xi)), ht = relu(Lt(xt)); logits = La(cat(hi, ht))
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import arch as S          # (the checker's own tables, as oracle/model.py)
from oracle import conv_models as CM
from oracle import model as O


class _RecordingF:
    """torch.nn.functional with layer_norm outputs recorded: the n-th LayerNorm of OracleTextEncoder.forward is the embedding
    LayerNorm (n = 0), then sa_layer_norm / output_layer_norm of each layer, so hidden_states[k] = record[2 k] for k >= 1"""

    def __init__(self):
        self.record = []

    def __getattr__(self, name):
        return getattr(F, name)

    def layer_norm(self, *a, **kw):
        y = F.layer_norm(*a, **kw)
        self.record.append(y)
        return y


class TappedTextEncoder(O.OracleTextEncoder):
    """OracleTextEncoder that also returns the class-token rows of ``hidden_states[n]`` for n in ``taps``"""

    taps = (2, 4)

    def forward(self, input_ids, attention_mask):
        rec = _RecordingF()
        with _swap(O, "F", rec):
            last = super().forward(input_ids, attention_mask)
        assert len(rec.record) == 2 * self.spec.layers + 1
        return last, [rec.record[2 * n][:, 0] for n in self.taps]


@contextlib.contextmanager
def _swap(mod, name, value):
    old = getattr(mod, name)
    setattr(mod, name, value)
    try:
        yield
    finally:
        setattr(mod, name, old)


def l2n(v):
    return v / v.norm(dim=1, keepdim=True)


def hierarchical_head(pooled, stage3, stage6, t0, t2, t4, W, drop=None):
    """W: {"final_hierarchical_image.weight": ..., ...}; stage maps NCHW; drop: optional (mask_i [B,5888], mask_t [B,2304]) of
    inverted-dropout factors.  Returns (x = xi | xt after dropout, h = hi | ht, logits)."""
    p3 = F.avg_pool2d(stage3, 7, 7).flatten(1)
    p6 = F.avg_pool2d(stage6, 6, 6).flatten(1)
    xi = torch.cat((l2n(pooled), l2n(p3), l2n(p6)), 1)
    xt = torch.cat((l2n(t0), l2n(t2), l2n(t4)), 1)
    if drop is not None:
        xi, xt = xi * drop[0], xt * drop[1]
    hi = torch.relu(F.linear(xi, W["final_hierarchical_image.weight"], W["final_hierarchical_image.bias"]))
    ht = torch.relu(F.linear(xt, W["final_hierarchical_text.weight"], W["final_hierarchical_text.bias"]))
    h = torch.cat((hi, ht), 1)
    return torch.cat((xi, xt), 1), h, F.linear(h, W["final_hierarchical_all.weight"], W["final_hierarchical_all.bias"])


class OracleHierarchical(torch.nn.Module):
    def __init__(self, text_model="distilbert", n_classes=4, enc_dropout=0.0):
        super().__init__()
        self.text_model = TappedTextEncoder(S.TEXT_SPECS[text_model], enc_dropout)
        self.image_model = CM.OracleEffNetV2Extractor("eff_v2_medium")
        self.image_model.pooled_only = False
        self.final_hierarchical_image = torch.nn.Linear(5888, 512)
        self.final_hierarchical_text = torch.nn.Linear(2304, 512)
        self.final_hierarchical_all = torch.nn.Linear(1024, n_classes)

    def load_engine(self, eng):
        """the parameters of a HierarchicalEngine (engine.init_parameters(seed)), as the conv tests load theirs"""
        sd = {k: eng.arena.view(k).detach().cpu().clone() for k in eng.param_keys}
        self.text_model.load_flat(sd, "text_model.")
        isd = {k[len("image_model."):]: v for k, v in sd.items() if k.startswith("image_model.")}
        missing = self.image_model.load_state_dict(isd, strict=False)
        assert not missing.unexpected_keys and all(("running" in k or "num_batches" in k) for k in missing.missing_keys)
        own = {k: v for k, v in sd.items() if k.startswith("final_hierarchical")}
        assert len(own) == 6
        self.load_state_dict(own, strict=False)
        return sd

    def head_weights(self):
        return {k: v for k, v in self.named_parameters() if k.startswith("final_hierarchical")}

    def forward(self, ids, mask, images):
        t0, (t2, t4) = self.text_model(ids, mask)
        s3, s6, pooled = self.image_model(images)
        return hierarchical_head(pooled, s3, s6, t0[:, 0], t2, t4, self.head_weights())[2]
