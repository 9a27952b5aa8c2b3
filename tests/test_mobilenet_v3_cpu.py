"""MobileNetV3-Large classifier (classifiers.MBNetLarge, the reference's ``--image_model=mb``): what holds without a GPU -- the
state_dict against the float64 restatement of torchvision's mobilenet_v3_large, the parameter count the reference quotes, the gradient
groups, the driver's batch table, and that MM_RCA still treats ``mb`` as an unknown image model."""
import pytest
import torch

from garbage_classification_rca_amd import classifiers as C
from garbage_classification_rca_amd import conv_engine as CE
from garbage_classification_rca_amd import lib as L
from garbage_classification_rca_amd import main_image as MI
from tests.mobilenet_v3_ref import MobileNetV3Large


def test_restatement_has_the_reference_parameter_count():
    """main_image.py:328: 4,207,156 parameters with the 4-class head"""
    assert sum(p.numel() for p in MobileNetV3Large(4).parameters()) == 4_207_156


def test_mbnetlarge_state_dict_matches_torchvisions_module_tree():
    m = C.MBNetLarge(4, True, device="cpu")
    ref = MobileNetV3Large(4)
    ours = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    theirs = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    assert ours == theirs                                          # keys, shapes and module order, BatchNorm buffers included
    assert sum(p.numel() for p in m.parameters()) == 4_207_156
    sd = m.state_dict()
    assert tuple(sd["classifier.0.weight"].shape) == (1280, 960) and tuple(sd["classifier.3.weight"].shape) == (4, 1280)
    dw5 = [k for k, v in sd.items() if v.dim() == 4 and v.shape[1:] == (1, 5, 5)]
    assert [tuple(sd[k].shape)[0] for k in dw5] == [72, 120, 120, 672, 960, 960]
    se = [tuple(sd[k].shape)[0] for k in sd if k.endswith("fc1.weight")]
    assert se == [24, 32, 32, 120, 168, 168, 240, 240]
    assert m.get_image_size() == (320, 320)
    assert C.MBNetLarge(4, device="cpu", image_size=64).get_image_size() == (64, 64)
    # transfer learning freezes the backbone (features.* and classifier.0.*); the head classifier.3 stays trainable
    assert sorted(k for k, p in m.named_parameters() if p.requires_grad) == ["classifier.3.bias", "classifier.3.weight"]


def test_mbnetlarge_plan_batchnorm_and_activations():
    enc = C.MBNetLarge(4, device="cpu").engine.conv
    units = list(enc._all_units())
    assert all(u.eps == 1e-3 and u.momentum == 0.01 for u in units)
    assert enc.stem.act == L.CONV_HSWISH and enc.final.act == L.CONV_HSWISH and enc.tail[3] == L.CONV_HSWISH
    assert [b["res"] for b in enc.blocks] == [True, False, True, False, True, True, False, True, True, True, False, True, False, True, True]
    for b in enc.blocks:
        assert b["units"][-1].act == L.CONV_NONE
        if b["se"] is not None:
            assert (b["se"].act1, b["se"].act2) == (L.CONV_RELU, L.CONV_HSIGMOID)
            assert not CE.ConvEncoder._se_fused(b["se"], 1 << 40)     # the fused MLP is SiLU / sigmoid only
    # the other backbones keep momentum 0.1
    effnet = C.EffNetV2_M(4, device="cpu", image_size=64).engine.conv
    assert all(u.momentum == 0.1 for u in effnet._all_units())


def test_mbnetlarge_arena_groups_tile_and_frozen_span_is_the_head():
    m = C.MBNetLarge(4, True, device="cpu", dtype="bf16x3f")
    eng = m.engine
    spans = sorted(eng.groups.values())
    assert spans[0][0] == 0 and spans[-1][1] == eng.arena.total
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert set(eng.groups) == {"image_emb", "image_stage_mb_s2", "image_stage_mb_s4", "image_stage_mb_s8", "image_stage_mb_s16",
                               "image_stage_mb_s32", "image_stage_final_conv", "head"}
    assert eng.arena.offsets["image_model.classifier.0.weight"][0] >= eng.groups["image_stage_final_conv"][0]
    h0 = eng.groups["head"][0]
    assert eng.trainable_spans(*m._train_flags()) == [(h0, eng.arena.total)]
    for p in m.parameters():
        p.requires_grad = True
    assert eng.trainable_spans(*m._train_flags()) == [(0, eng.arena.total)]
    assert eng.conv_dtype == torch.bfloat16


def test_main_image_runs_mb_with_the_reference_batch_row():
    assert "mb" in set(MI.BATCHES) and MI.BATCHES["mb"] == (256, 256, None)
    from garbage_classification_rca_amd import calculate_test_accuracy_image as CT
    assert CT.BATCHES["mb"] == 256


def test_mm_rca_still_treats_mb_as_an_unknown_image_model():
    from garbage_classification_rca_amd.engine import MMRCAEngine
    assert "mb" not in CE.CONV_MODELS
    with pytest.raises(ValueError, match="Wrong image model"):
        MMRCAEngine("distilbert", "mb", 4, True, 0, torch.float32, device="cpu")
