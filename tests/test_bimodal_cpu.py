"""The bimodal GRU late-fusion model (multimodal_model.HierarchicalBimodalFusion, --late_fusion=bimodal): what holds without a GPU -- the
written-out GRU against torch.nn.GRU, the restatement against the golden recorded from the reference's own class, the checkpoint
layout, the arena, the eight-positional constructor, the new library symbols and the command line."""
import contextlib
import ctypes
import io
import json
import os

import numpy as np
import pytest
import torch

from garbage_classification_rca_amd import abi
from garbage_classification_rca_amd import lib as L
from garbage_classification_rca_amd.multimodal_model import MM_RCA, HierarchicalBimodalFusion, EffV2MediumAndDistilbertGated
from tests import bimodal_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bimodal_goldens.npz")
NEW_EXPORTS = ["mmrca_gru_linear_fwd", "mmrca_gru_linear_bwd", "mmrca_gru_fwd", "mmrca_gru_bwd", "mmrca_hadamard_fwd", "mmrca_hadamard_bwd",
               "mmrca_dropout_f32"]
GOLDEN_TENSORS = ("ctx_text", "ctx_audio", "fused", "ctx_fused", "logits")


def relmax(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))       # (T = 1: the weight_hh gradient is exactly zero)


@pytest.mark.parametrize("n_in,hid,T", [(400, 400, 1), (400, 500, 3), (7, 5, 33)])
def test_written_out_gru_equals_torch_gru_on_an_unbatched_sequence(n_in, hid, T):
    """float64, an unbatched [T, I] input (what the reference's 2-D tensors are to torch): outputs and all gradients to 1e-12"""
    torch.manual_seed(T)
    gru = torch.nn.GRU(n_in, hid, batch_first=True).double()
    x = torch.randn(T, n_in, dtype=torch.float64, requires_grad=True)
    ref, hT = gru(x)
    assert tuple(ref.shape) == (T, hid) and tuple(hT.shape) == (1, hid)
    x2 = x.detach().clone().requires_grad_(True)
    P = [p.detach().clone().requires_grad_(True) for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
    out = BR.gru_sequence(x2, *P)
    assert relmax(out.detach(), ref.detach()) < 1e-12
    d = torch.randn(T, hid, dtype=torch.float64)
    (ref * d).sum().backward()
    (out * d).sum().backward()
    assert relmax(x2.grad, x.grad) < 1e-12
    for mine, theirs in zip(P, (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)):
        assert relmax(mine.grad, theirs.grad) < 1e-12


def test_restatement_reproduces_the_reference_classes_golden():
    """float32, 1e-5 of each tensor's largest entry (the issue's bound), on the recorded class-token rows and the procedural pooled feature"""
    g = np.load(GOLDEN)
    W = {k: torch.from_numpy(v) for k, v in BR.golden_weights().items()}
    out = BR.bimodal_head(torch.from_numpy(g["t"]), torch.from_numpy(BR.golden_pooled()), W)
    errs = {k: relmax(out[k], g[k]) for k in GOLDEN_TENSORS}
    print("float32 restatement vs the reference's HierarchicalBimodalFusion:", errs)
    assert g["logits"].shape == (3, 4) and g["ctx_fused"].shape == (3, 500)
    assert all(e < 1e-5 for e in errs.values()), errs


def test_the_golden_depends_on_the_recurrence_and_on_the_batch_order():
    """zeroing every weight_hh moves ctx_fused by more than 1e-2 of its scale, and swapping rows 0 and 1 changes row 2's logits"""
    g = np.load(GOLDEN)
    W = {k: torch.from_numpy(v).double() for k, v in BR.golden_weights().items()}
    t, f = torch.from_numpy(g["t"]).double(), torch.from_numpy(BR.golden_pooled()).double()
    full = BR.bimodal_head(t, f, W)
    W0 = {k: (torch.zeros_like(v) if k.endswith("weight_hh_l0") else v) for k, v in W.items()}
    assert relmax(BR.bimodal_head(t, f, W0)["ctx_fused"], full["ctx_fused"]) > 1e-2
    perm = [1, 0, 2]
    swapped = BR.bimodal_head(t[perm], f[perm], W)
    assert relmax(swapped["logits"][2], full["logits"][2]) > 1e-3


@pytest.fixture(scope="module")
def model():
    with contextlib.redirect_stdout(io.StringIO()):
        return HierarchicalBimodalFusion(4, 0.6, 0.0, 0.7, 256, "distilbert", 16, True, device="cpu", dtype="fp32")


def test_the_eight_positional_call_constructs(model):
    assert isinstance(model, EffV2MediumAndDistilbertGated)
    assert model.get_image_size() == (480, 480) and model.get_max_token_size() == 512
    # --model_dropout does nothing in this forward: the two dropouts are fixed at 0.86
    assert model.model_dropout == 0.6 and model.drop_ratio == 0.86 and model.img_dropout_prob == 0.7
    head = [k for k, _ in BR.head_shapes()]
    trainable = sorted(k for k, p in model.named_parameters() if p.requires_grad and k in model._arena_params)
    assert trainable == sorted(head)            # backbones frozen at construction, the head trainable


def test_state_dict_keys_and_shapes_are_mm_rcas(model):
    """against the MM_RCA entry of tests/golden/state_dict_layout.json (recorded from the reference's constructor; image_model.* is not
    in it) and against this build's MM_RCA"""
    layout = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_layout.json")))["distilbert|features_only=0|cross_attention_only=0|batch_size=16|fc=256"]
    a = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    mine = {k: list(s) for k, s in a.items() if not k.startswith("image_model.")}
    assert mine == layout, (sorted(set(mine) ^ set(layout))[:8], [k for k in mine if k in layout and mine[k] != layout[k]][:8])
    with contextlib.redirect_stdout(io.StringIO()):
        ref = MM_RCA(4, 0.6, 0.0, 0.7, 256, "distilbert", 16, True, False, False, device="cpu", dtype="fp32")
    b = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert a == b
    for k, shp in BR.head_shapes():
        assert a[k] == tuple(shp), k
        assert k in model._arena_params and k not in ref._arena_params       # arena parameters here, present-but-unused there
    assert a["gru_text.weight_hh_l0"] == (1200, 400) and a["gru_bimodal.weight_hh_l0"] == (1500, 500) and a["classifier.weight"] == (4, 450)
    for k in ("cross_attention_1.W_query.weight", "final_with_everything.weight", "final_hierarchical_image.weight"):
        assert k in a and k not in model._arena_params
    # checkpoints interchange in both directions
    ref.load_state_dict(model.state_dict(), strict=True)
    model.load_state_dict(ref.state_dict(), strict=True)


def test_arena_order_groups_and_initialisation(model):
    eng = model.engine
    spans = sorted(eng.groups.values())
    assert spans[0][0] == 0 and spans[-1][1] == eng.arena.total
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    lo, hi = eng.groups["head"]
    assert eng.trainable_spans(False, False) == [(lo, eng.arena.total)] and hi == eng.arena.total
    assert eng.trainable_spans(True, True) == [(0, eng.arena.total)]
    assert [k for k in eng.param_keys if eng._group_of(k) == "head"] == [k for k, _ in BR.head_shapes()]
    assert eng.arena.offsets["modality_text_to_dim.weight"][0] == lo
    # torch's defaults: GRU U(-1/sqrt(H), 1/sqrt(H)), kernels standard normal, fusion bias zero
    for name, _, hid in BR.GRUS:
        for leaf in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            v = eng.arena.view(f"{name}.{leaf}")
            assert float(v.abs().max()) <= hid ** -0.5 and float(v.abs().max()) > 0.9 * hid ** -0.5, (name, leaf)
            assert abs(float(v.mean())) < 0.1 * hid ** -0.5
    for leaf in ("kernel1", "kernel2"):
        v = eng.arena.view("fusion." + leaf)
        assert 0.8 < float(v.std()) < 1.2 and abs(float(v.mean())) < 0.2
    assert float(eng.arena.view("fusion.bias").abs().max()) == 0.0


@pytest.mark.parametrize("kw", [dict(image_model_name="transformer_B16"), dict(image_model_name="shuffle_net", image_size=224),
                                dict(image_model_name="eff_v2_medium", image_size=224)])
def test_every_backbone_and_image_size_of_mm_rca_is_accepted(kw):
    with contextlib.redirect_stdout(io.StringIO()):
        m = HierarchicalBimodalFusion(4, 0.6, 0.0, 0.7, 256, "distilbert", 16, True, device="cpu", dtype="fp32", build_unused_parameters=False, **kw)
    assert tuple(m.engine.arena.view("modality_image_to_dim.weight").shape) == (400, m.engine.d_img)
    assert m.get_image_size() == (224, 224)


def test_new_exports_exist_in_the_library_the_binding_and_the_header():
    lib = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "mmrca.h")).read()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in abi.prototypes() and getattr(L.load(), name).argtypes is not None, name
        assert name + "(" in header, name


def test_launch_validation_names_the_offending_value():
    """shapes the kernels do not cover are rejected before any launch (no GPU is touched: the checks come first)"""
    lib = L.load()
    one = (ctypes.c_void_p * 1)(16)
    ld = (ctypes.c_int * 1)(600)
    for H, word in ((516, "H=516"), (402, "H=402"), (0, "H=0")):
        assert lib.mmrca_gru_fwd(1, one, one, one, one, one, one, 3, H, None) != 0
        assert word in lib.mmrca_last_error().decode()
        assert lib.mmrca_gru_bwd(1, one, one, one, one, one, ld, one, one, one, 3, H, None) != 0
        assert word in lib.mmrca_last_error().decode()
    assert lib.mmrca_gru_fwd(3, one, one, one, one, one, one, 3, 400, None) != 0 and "3 GRUs" in lib.mmrca_last_error().decode()
    assert lib.mmrca_gru_fwd(1, one, one, one, one, one, one, 0, 400, None) != 0 and "T=0" in lib.mmrca_last_error().decode()
    assert lib.mmrca_gru_linear_fwd(16, 300, 16, 16, 16, 4, 3, 4, 400, 0, None) != 0 and "300" in lib.mmrca_last_error().decode()
    assert lib.mmrca_dropout_f32(16, 8, 16, 8, 2, 8, 1.0, 0, None) != 0 and "drop_p" in lib.mmrca_last_error().decode()


def test_late_fusion_bimodal_parses_and_the_default_is_unchanged():
    from garbage_classification_rca_amd.options import args_parser
    assert vars(args_parser(["--late_fusion=bimodal"]))["late_fusion"] == "bimodal"
    assert vars(args_parser([]))["late_fusion"] == "gated"           # the reference's default, which still exits as a wrong strategy
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        args_parser(["--help"])
    assert "bimodal" in buf.getvalue()
    import CVPR_code.multimodal_model as shim
    assert shim.HierarchicalBimodalFusion is HierarchicalBimodalFusion
