"""MobileBERT without a GPU: the float64 restatement against the golden file and against transformers' own class, the parameter
count, the module's state-dict layout / frozen set / arena groups, the compute modes, the driver tables and the library's exports."""
import ctypes
import os

import numpy as np
import pytest
import torch

from garbage_classification_rca_amd import calculate_test_accuracy_text as CT
from garbage_classification_rca_amd import classifiers as C
from garbage_classification_rca_amd import abi
from garbage_classification_rca_amd import lib as L
from garbage_classification_rca_amd import main_text as MT
from garbage_classification_rca_amd import spec as S
from garbage_classification_rca_amd.engine import MMRCAEngine
from garbage_classification_rca_amd.mobilebert_engine import MOBILEBERT, MobileBertSpec, mobilebert_params
from tests.mobilebert_ref import GOLDEN, GOLDEN_GRADS, GOLDEN_ROW_STRIDE, MobileBertRef, golden_inputs, proc_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["mmrca_nonorm_fwd", "mmrca_nonorm_bwd", "mmrca_nonorm_bwd_workspace_bytes", "mmrca_trigram_embed_fwd", "mmrca_trigram_embed_bwd"]
N_PARAMS, N_TENSORS = 24583940, 1113


def _proc_ref(layers):
    m = MobileBertRef(4, layers).double().eval()
    m.load_state_dict({k: v.double() for k, v in proc_state(m).items()}, strict=True)
    return m


def test_restatement_reproduces_the_golden_file():
    """logits, hidden_states[1] at the class tokens and the four recorded gradients of transformers' float64 run, to 1e-10"""
    g = np.load(GOLDEN)
    ids, mask, dl = golden_inputs()
    assert np.array_equal(g["ids"], ids.numpy()) and np.array_equal(g["mask"], mask.numpy()) and np.array_equal(g["dlogits"], dl.numpy())
    assert list(mask.sum(1)) == [16, 9, 1]
    m = _proc_ref(2)
    logits, hs = m(ids, mask, hidden_states=True)
    (logits * dl.double()).sum().backward()
    assert np.abs(logits.detach().numpy() - g["logits"]).max() < 1e-10
    assert np.abs(hs[1][:, 0].detach().numpy() - g["hidden1_cls"]).max() < 1e-10
    params = dict(m.named_parameters())
    for k in GOLDEN_GRADS:
        grad = params[k].grad
        assert abs(float(grad.abs().max()) - float(g["gradmax:" + k])) < 1e-10
        assert np.abs(grad[::GOLDEN_ROW_STRIDE.get(k, 1)].numpy() - g["grad:" + k]).max() < 1e-10, k
    assert os.path.getsize(GOLDEN) < 100 << 10


@pytest.mark.parametrize("layers", [2, 24])
def test_restatement_matches_the_live_transformers_class(layers):
    """keys, shapes and order of the state dict, and the float64 logits and a gradient, at 2 and 24 layers"""
    tr = pytest.importorskip("transformers")
    cfg = tr.MobileBertConfig(classifier_activation=False, num_labels=4, num_hidden_layers=layers)
    live = tr.MobileBertForSequenceClassification(cfg).double().eval()
    m = _proc_ref(layers)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in live.state_dict().items()]
    live.load_state_dict(m.state_dict(), strict=True)
    ids, mask, dl = golden_inputs()
    a, b = m(ids, mask), live(input_ids=ids, attention_mask=mask).logits
    (a * dl.double()).sum().backward()
    (b * dl.double()).sum().backward()
    a, b = a.detach(), b.detach()
    assert float((a - b).abs().max()) < 1e-10 * max(1.0, float(b.abs().max()))
    k = "mobilebert.encoder.layer.0.attention.self.value.weight"
    ga, gb = dict(m.named_parameters())[k].grad, dict(live.named_parameters())[k].grad
    assert float((ga - gb).abs().max()) < 1e-10 * max(1.0, float(gb.abs().max()))


def test_parameter_count_is_the_checkpoints():
    m = MobileBertRef(4)
    assert sum(p.numel() for p in m.parameters()) == N_PARAMS and len(m.state_dict()) == N_TENSORS
    assert len(mobilebert_params(MOBILEBERT)) == N_TENSORS - 2


def test_module_state_dict_frozen_set_and_groups():
    m = C.MobileBERT(4, device="cpu")
    ref = MobileBertRef(4)
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [("model." + k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    assert sum(v.numel() for v in sd.values()) == N_PARAMS
    ref.load_state_dict({k[len("model."):]: v for k, v in sd.items()}, strict=True)
    trainable = [k for k, p in m.named_parameters() if p.requires_grad]
    assert trainable == ["model.classifier.weight", "model.classifier.bias"]
    assert all(k.startswith("model.mobilebert.") for k, p in m.named_parameters() if not p.requires_grad)
    eng = m.engine
    assert list(eng.groups) == ["text_emb"] + [f"text_layer_{i}" for i in range(24)] + ["head"]
    spans = sorted(eng.groups.values())
    assert spans[0][0] == 0 and spans[-1][1] == eng.arena.total
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert eng.trainable_spans(False, False) == [(eng.groups["head"][0], eng.arena.total)]
    assert eng.trainable_spans(True, False) == [(0, eng.arena.total)]
    assert m._train_flags() == (False, False)
    # transformers' _init_weights: NoNorm (1, 0), zero biases and pad row, N(0, 0.02) matrices
    assert float(sd["model.mobilebert.embeddings.word_embeddings.weight"][0].abs().max()) == 0.0
    assert float(sd["model.mobilebert.encoder.layer.3.ffn.1.output.LayerNorm.weight"].min()) == 1.0
    assert float(sd["model.mobilebert.encoder.layer.3.ffn.1.output.dense.bias"].abs().max()) == 0.0
    assert abs(float(sd["model.mobilebert.encoder.layer.3.attention.self.value.weight"].std()) - 0.02) < 2e-3
    assert m.get_max_token_size() == 512 and m.enc_dropout == 0.1 and m.drop_ratio == 0.0
    assert m.get_tokenizer().vocab_size == 30522


def test_shallow_spec_and_modes():
    m = C.MobileBERT(3, device="cpu", dtype="bf16", spec=MobileBertSpec(layers=2, vocab=100))
    assert len(m.state_dict()) == 7 + 2 * 46 + 2 and m.engine.arena.lp is not None
    assert tuple(m.state_dict()["model.classifier.weight"].shape) == (3, 512)
    for name in ("bf16x3", "bf16x3f"):
        with pytest.raises(ValueError, match="fp32 or bf16"):
            C.MobileBERT(4, device="cpu", dtype=name)


def test_driver_tables_and_the_multimodal_models_still_reject_it():
    assert MT.BATCHES["mobile_bert"] == (18, 4, 12)
    assert CT.BATCHES["mobile_bert"] == 18
    assert C.TEXT_FACTORIES["mobile_bert"] is C.MobileBERT
    assert "mobile_bert" not in S.TEXT_SPECS
    with pytest.raises(ValueError, match="Wrong text model"):
        MMRCAEngine("mobile_bert", "transformer_B16", 4, True, 0, torch.float32, "cpu")
    for name in ("bart", "gpt2"):
        assert name not in MT.BATCHES and name not in CT.BATCHES


def test_scripts_pick_fp32_under_their_default_dtype(capsys):
    m = C.build_text_classifier("mobile_bert", 4, 0.3, "bf16x3f", "cpu")
    assert "using fp32" in capsys.readouterr().out and m.engine.dtype == torch.float32 and m.drop_ratio == 0.0
    assert C.build_text_classifier("mobile_bert", 4, 0.3, torch.bfloat16, "cpu").engine.dtype == torch.bfloat16
    assert capsys.readouterr().out == ""


def test_header_declares_and_library_exports_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "mmrca.h")).read()
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name + "(" in header, name
        assert name in abi.prototypes() and getattr(L.load(), name).argtypes is not None, name
        assert hasattr(lib, name), name
