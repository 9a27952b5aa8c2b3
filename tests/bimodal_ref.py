"""Restatement of the bimodal GRU late-fusion model (the reference's ``HierarchicalBimodalFusion.forward``,
CVPR_code/multimodal_model.py:835-888) composed from the oracle's encoders, in whatever dtype it is cast to (the tests use float64):

    t = last_hidden_state[:, 0] / its L2 norm      f = pooled image feature / its L2 norm
    x_text = Lt(t)   x_image = Li(f)                                            [B, 400]
    ctx_text = GRU_text(x_text)   ctx_audio = GRU_audio(x_image)                [B, 400]   the batch is the sequence: T = B, h_{-1} = 0
    fused = tanh(ctx_text * kernel1 + ctx_audio * kernel2 + bias)               [B, 400]
    ctx_fused = GRU_bimodal(fused)                                              [B, 500]
    proj = drop2(relu(concat_fc(cat(fused, drop1(ctx_fused)))))                 [B, 450]
    logits = classifier(proj)                                                   [B, 4]

The GRU is written out from torch's documented cell equations (gate rows r | z | n of weight_ih_l0 / weight_hh_l0), not ``nn.GRU``:

    r = s(W_ir x + b_ir + W_hr h + b_hr)    z = s(W_iz x + b_iz + W_hz h + b_hz)
    n = tanh(W_in x + b_in + r * (W_hn h + b_hn))        h' = (1 - z) * n + z * h
"""
import torch
import torch.nn.functional as F

from oracle import model as O

DIM, HIDDEN, PROJ, CLASSES = 400, 500, 450, 4
GRUS = (("gru_text", DIM, DIM), ("gru_audio", DIM, DIM), ("gru_bimodal", DIM, HIDDEN))


def head_shapes(d_img=1280, d_txt=768):
    """(key, shape) of the head's parameters, in the engine's arena order"""
    P = [("modality_text_to_dim.weight", (DIM, d_txt)), ("modality_text_to_dim.bias", (DIM,)),
         ("modality_image_to_dim.weight", (DIM, d_img)), ("modality_image_to_dim.bias", (DIM,))]

    def gru(name, n_in, hid):
        return [(f"{name}.weight_ih_l0", (3 * hid, n_in)), (f"{name}.weight_hh_l0", (3 * hid, hid)),
                (f"{name}.bias_ih_l0", (3 * hid,)), (f"{name}.bias_hh_l0", (3 * hid,))]
    P += gru(*GRUS[0]) + gru(*GRUS[1])
    P += [("fusion.kernel1", (DIM,)), ("fusion.kernel2", (DIM,)), ("fusion.bias", (DIM,))]
    P += gru(*GRUS[2])
    P += [("concat_fc.weight", (PROJ, DIM + HIDDEN)), ("concat_fc.bias", (PROJ,)), ("classifier.weight", (CLASSES, PROJ)), ("classifier.bias", (CLASSES,))]
    return P


GOLDEN_B = 3
GOLDEN_GRU_SCALE = 4.0       # proc_state draws N(0, 0.02); times 4 (torch's default is U(+-0.05)) the gates leave their linear range: |ctx| 0.5-0.7


def golden_weights():
    """the head weights tests/golden/make_bimodal_golden.py loaded into the reference's class, regenerated from their names (numpy fp32):
    proc_state over head_shapes(), every GRU entry scaled by GOLDEN_GRU_SCALE"""
    from garbage_classification_rca_amd.procedural import proc_state
    W = proc_state(dict(head_shapes()))
    return {k: (v * W[k].dtype.type(GOLDEN_GRU_SCALE) if k.startswith("gru_") else v) for k, v in W.items()}


def golden_pooled():
    from garbage_classification_rca_amd.procedural import proc_input
    return proc_input("bimodal.pooled", (GOLDEN_B, 1280))


def gru_sequence(x, w_ih, w_hh, b_ih, b_hh, h0=None):
    """x [T, I] -> [T, H]: one unbatched sequence through one GRU layer, step by step"""
    H = w_hh.shape[1]
    h = x.new_zeros(H) if h0 is None else h0
    out = []
    for t in range(x.shape[0]):
        gi = w_ih @ x[t] + b_ih
        gh = w_hh @ h + b_hh
        r = torch.sigmoid(gi[:H] + gh[:H])
        z = torch.sigmoid(gi[H:2 * H] + gh[H:2 * H])
        n = torch.tanh(gi[2 * H:] + r * gh[2 * H:])
        h = (1 - z) * n + z * h
        out.append(h)
    return torch.stack(out)


def _gru(W, name, x):
    return gru_sequence(x, W[name + ".weight_ih_l0"], W[name + ".weight_hh_l0"], W[name + ".bias_ih_l0"], W[name + ".bias_hh_l0"])


def l2n(v):
    return v / v.norm(dim=1, keepdim=True)


def hadamard(a, b, k1, k2, bias):
    return torch.tanh(a * k1 + b * k2 + bias)


def bimodal_head(t, f, W, drop=None):
    """t [B, d_txt] class-token rows, f [B, d_img] pooled feature, W {key: tensor}; drop: optional (mask1 [B, 500], mask2 [B, 450]) of
    inverted-dropout factors.  Returns dict(ctx_text, ctx_audio, fused, ctx_fused, proj, logits)."""
    x_text = F.linear(l2n(t), W["modality_text_to_dim.weight"], W["modality_text_to_dim.bias"])
    x_image = F.linear(l2n(f), W["modality_image_to_dim.weight"], W["modality_image_to_dim.bias"])
    ctx_text, ctx_audio = _gru(W, "gru_text", x_text), _gru(W, "gru_audio", x_image)
    fused = hadamard(ctx_text, ctx_audio, W["fusion.kernel1"], W["fusion.kernel2"], W["fusion.bias"])
    ctx_fused = _gru(W, "gru_bimodal", fused)
    c = ctx_fused if drop is None else ctx_fused * drop[0]
    proj = torch.relu(F.linear(torch.cat((fused, c), 1), W["concat_fc.weight"], W["concat_fc.bias"]))
    if drop is not None:
        proj = proj * drop[1]
    return dict(ctx_text=ctx_text, ctx_audio=ctx_audio, fused=fused, ctx_fused=ctx_fused, proj=proj,
                logits=F.linear(proj, W["classifier.weight"], W["classifier.bias"]))


class OracleBimodal(torch.nn.Module):
    """the oracle's encoders (oracle.model.build_oracle) under the restated head"""

    def __init__(self, text_model="distilbert", image_model="eff_v2_medium"):
        super().__init__()
        base = O.build_oracle(text_model, image_model, True, drop_ratio=0.0, enc_dropout=0.0)
        self.text_model, self.image_model = base.text_model, base.image_model
        self.head = torch.nn.ParameterDict()
        self._names = {}

    def load_engine(self, eng):
        """the parameters of a BimodalEngine (engine.init_parameters(seed))"""
        sd = {k: eng.arena.view(k).detach().cpu().clone() for k in eng.param_keys}
        self.text_model.load_flat(sd, "text_model.")
        if hasattr(self.image_model, "load_flat"):
            self.image_model.load_flat(sd, "image_model.")
        else:
            isd = {k[len("image_model."):]: v for k, v in sd.items() if k.startswith("image_model.")}
            missing = self.image_model.load_state_dict(isd, strict=False)
            assert not missing.unexpected_keys and all(("running" in k or "num_batches" in k) for k in missing.missing_keys)
        for k, shp in head_shapes(eng.d_img, eng.d_txt):
            assert tuple(sd[k].shape) == tuple(shp), k
            self._names[k] = k.replace(".", "/")
            self.head[self._names[k]] = torch.nn.Parameter(sd[k].clone())
        return sd

    def head_weights(self):
        return {k: self.head[n] for k, n in self._names.items()}

    def forward(self, ids, mask, images):
        t = self.text_model(ids, mask)[:, 0]
        f = self.image_model(images)
        return bimodal_head(t, f, self.head_weights())["logits"]
