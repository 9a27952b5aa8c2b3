"""The hierarchical late-fusion model (multimodal_model.Hierarchical, --late_fusion=hierarchical): what holds without a GPU -- the float64
restatement against the golden recorded from the reference's own class, the checkpoint layout, the arena groups, the eight-positional
constructor, the configuration guard and the new library symbols."""
import ctypes
import os

import numpy as np
import pytest
import torch

from garbage_classification_rca_amd import abi
from garbage_classification_rca_amd import lib as L
from garbage_classification_rca_amd.multimodal_model import MM_RCA, Hierarchical, EffV2MediumAndDistilbertGated
from garbage_classification_rca_amd.procedural import proc_input, proc_state
from tests import hierarchical_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hierarchical_goldens.npz")
LINEARS = {"final_hierarchical_image.weight": (512, 5888), "final_hierarchical_image.bias": (512,),
           "final_hierarchical_text.weight": (512, 2304), "final_hierarchical_text.bias": (512,),
           "final_hierarchical_all.weight": (4, 1024), "final_hierarchical_all.bias": (4,)}
NEW_EXPORTS = ["mmrca_hier_pool_fwd", "mmrca_hier_pool_bwd", "mmrca_hier_norm_fwd", "mmrca_hier_norm_bwd", "mmrca_hier_linear_relu_fwd",
               "mmrca_hier_linear_relu_bwd", "mmrca_hier_linear_workspace_bytes"]


def golden_inputs(dtype=torch.float64):
    """the procedural inputs tests/golden/make_hierarchical_golden.py fed to the reference's class, regenerated from their names"""
    t = lambda a: torch.from_numpy(a).to(dtype)
    return dict(stage3=t(proc_input("hier.stage3", (2, 160, 30, 30))), stage6=t(proc_input("hier.stage6", (2, 512, 15, 15))),
                pooled=t(proc_input("hier.pooled", (2, 1280))), weights={k: t(v) for k, v in proc_state(LINEARS).items()})


def relmax(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


def test_float64_restatement_reproduces_the_reference_classes_golden():
    """1e-6 relative: the golden itself is fp32 arithmetic (the issue's bound)"""
    g = np.load(GOLDEN)
    gi = golden_inputs()
    t = lambda k: torch.from_numpy(g[k]).double()
    x, h, logits = HR.hierarchical_head(gi["pooled"], gi["stage3"], gi["stage6"], t("t0"), t("t2"), t("t4"), gi["weights"])
    errs = {k: relmax(v, g[k]) for k, v in (("x", x), ("h", h), ("logits", logits))}
    print("float64 restatement vs the reference's Hierarchical (fp32):", errs)
    assert x.shape == (2, 8192) and h.shape == (2, 1024)
    assert all(e < 1e-6 for e in errs.values()), errs


@pytest.fixture(scope="module")
def model():
    return Hierarchical(4, 0.6, 0.0, 0.7, 256, "distilbert", 16, True, device="cpu", dtype="fp32")


def test_the_eight_positional_call_constructs(model):
    assert isinstance(model, EffV2MediumAndDistilbertGated)
    assert model.get_image_size() == (480, 480) and model.get_max_token_size() == 512
    assert model.drop_ratio == 0.6 and model.img_dropout_prob == 0.7
    # backbones frozen at construction, the three linears trainable
    trainable = sorted(k for k, p in model.named_parameters() if p.requires_grad and k.startswith(("text_model.", "image_model.", "final_hierarchical")))
    assert trainable == sorted(LINEARS)


def test_state_dict_keys_and_shapes_are_mm_rcas(model):
    ref = MM_RCA(4, 0.6, 0.0, 0.7, 256, "distilbert", 16, True, False, False, device="cpu", dtype="fp32")
    a = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    b = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert set(a) == set(b), (sorted(set(a) - set(b))[:5], sorted(set(b) - set(a))[:5])
    assert a == b
    for k, shp in LINEARS.items():
        assert a[k] == shp, k
        assert k in model._arena_params and k not in ref._arena_params       # arena parameters here, present-but-unused there
    assert "cross_attention_1.W_query.weight" in a and "cross_attention_1.W_query.weight" not in model._arena_params


def test_arena_groups_tile_the_arena_and_frozen_spans_are_the_head(model):
    eng = model.engine
    spans = sorted(eng.groups.values())
    assert spans[0][0] == 0 and spans[-1][1] == eng.arena.total
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    lo, hi = eng.groups["head"]
    assert eng.trainable_spans(False, False) == [(lo, eng.arena.total)]
    assert eng.arena.offsets["final_hierarchical_image.weight"][0] == lo and hi == eng.arena.total
    assert eng.trainable_spans(True, True) == [(0, eng.arena.total)]
    assert [k for k in eng.param_keys if eng._group_of(k) == "head"] == list(LINEARS)
    assert eng.seg_off == [0, 1280, 3840, 5888, 6656, 7424, 8192]


@pytest.mark.parametrize("kw,word", [(dict(image_model_name="shuffle_net"), "shuffle_net"), (dict(image_model_name="transformer_B16"), "transformer_B16"),
                                     (dict(image_size=416), "416"), (dict(image_size=224), "224")])
def test_configurations_the_linears_do_not_fit_fail_loudly(kw, word):
    with pytest.raises((ValueError, SystemExit)) as e:
        Hierarchical(4, 0.6, 0.0, 0.7, 256, "distilbert", 16, True, device="cpu", dtype="fp32", **kw)
    assert word in str(e.value), str(e.value)


def test_a_text_width_other_than_768_fails_loudly(monkeypatch):
    from garbage_classification_rca_amd import spec as S
    import dataclasses
    wide = dataclasses.replace(S.TEXT_SPECS["distilbert"], dim=1024)
    monkeypatch.setitem(S.TEXT_SPECS, "wide_text", wide)
    with pytest.raises((ValueError, SystemExit)) as e:
        Hierarchical(4, 0.6, 0.0, 0.7, 256, "wide_text", 16, True, device="cpu", dtype="fp32")
    assert "wide_text" in str(e.value) and "1024" in str(e.value)


@pytest.mark.parametrize("size", [448, 480, 512])
def test_sizes_that_pool_to_4x4_and_2x2_are_accepted(size):
    from garbage_classification_rca_amd.hierarchical_engine import check_hierarchical_config, stage_map_sizes
    check_hierarchical_config("distilbert", "eff_v2_medium", size)
    h3, h6 = stage_map_sizes(size)
    assert (h3 // 7, h6 // 6) == (4, 2)


def test_new_exports_exist_in_the_library_the_binding_and_the_header():
    lib = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "mmrca.h")).read()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in abi.prototypes() and getattr(L.load(), name).argtypes is not None, name
        assert name + "(" in header, name


def test_only_the_help_text_of_late_fusion_changed():
    from garbage_classification_rca_amd.options import args_parser
    import contextlib, io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        args_parser(["--help"])
    assert "hierarchical" in buf.getvalue()
    assert vars(args_parser([]))["late_fusion"] == "gated"           # the reference's default, which still exits as a wrong strategy
