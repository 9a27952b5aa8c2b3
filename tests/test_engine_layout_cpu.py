"""The engine family without a GPU: every engine's arena layout (size, key count, groups and a fingerprint of key / offset / shape, all
recorded before the constructors were merged into one), the invariants the optimizers and the gradient exchange rely on, and the
compute-mode flags for every accepted ``dtype`` spelling."""
import hashlib
import os

import pytest
import torch

from garbage_classification_rca_amd import lib as L
from garbage_classification_rca_amd.bimodal_engine import BimodalEngine
from garbage_classification_rca_amd.classifier_engine import ClassifierEngine
from garbage_classification_rca_amd.engine import MMRCAEngine
from garbage_classification_rca_amd.hierarchical_engine import HierarchicalEngine
from garbage_classification_rca_amd.mobilebert_engine import MobileBertEngine

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmmrca.so is not built")

# (engine, positional args, keyword args, arena.total, len(param_keys), len(groups), fingerprint)
LAYOUTS = [
    (MMRCAEngine, ("distilbert", "transformer_B16", 4, True, 0, "bf16x3f"), {}, 152243392, 284, 22, "55999c5e4133"),
    (MMRCAEngine, ("bert", "eff_v2_medium", 4, True, 1, torch.bfloat16), dict(image_size=480), 162439744, 880, 24, "270460afeff2"),
    (MMRCAEngine, ("roberta", "shuffle_net", 4, True, 2, "fp32"), {}, 129507392, 399, 19, "567402eccfc9"),
    (ClassifierEngine, ("mb", 4, "bf16x3f"), {}, 4210432, 174, 8, "0d0323916f63"),
    (ClassifierEngine, ("roberta", 4, "fp32"), {}, 124058176, 199, 14, "7b378e4c0628"),
    (ClassifierEngine, ("transformer_L16", 4, "bf16"), {}, 303305792, 296, 27, "5132f0f9784c"),
    (HierarchicalEngine, ("distilbert",), {}, 123430848, 753, 17, "c7f3db8033a3"),
    (BimodalEngine, ("distilbert", "shuffle_net"), dict(image_size=224), 76525440, 291, 13, "e1c1323edd36"),
    (MobileBertEngine, (4, "fp32"), {}, 24584000, 1113, 26, "cd12a790df9d"),
]


def fingerprint(eng):
    text = "\n".join(f"{k} {eng.arena.offsets[k][0]} {eng.arena.offsets[k][1]}" for k in eng.param_keys)
    return hashlib.sha1(text.encode()).hexdigest()[:12]


@pytest.mark.parametrize("cls,args,kw,total,n_keys,n_groups,fp", LAYOUTS, ids=[f"{r[0].__name__}-{r[1][0]}" for r in LAYOUTS])
def test_arena_layout_groups_and_spans(cls, args, kw, total, n_keys, n_groups, fp):
    eng = cls(*args, device="cpu", **kw)
    assert (eng.arena.total, len(eng.param_keys), len(eng.groups), fingerprint(eng)) == (total, n_keys, n_groups, fp)
    spans = list(eng.groups.values())                       # in arena order, no gap, no overlap
    assert spans[0][0] == 0 and spans[-1][1] == eng.arena.total
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert eng._text_stream is None and eng.buffer_generation == 0
    assert eng._side_v is None and eng._side_t is None and eng._side is None
    bounds = {lo for lo, _ in spans} | {eng.arena.total}
    for tt in (False, True):
        for ti in (False, True):
            ts = eng.trainable_spans(tt, ti)
            assert ts and ts[-1][1] == eng.arena.total
            assert all(lo in bounds and hi in bounds and lo < hi for lo, hi in ts), (tt, ti, ts)
    eng.release_buffers()
    assert eng.buffer_generation == 1


BF16, F32 = torch.bfloat16, torch.float32
# spelling -> (dtype, x3, x3f, gdtype, bdt); conv_dtype is bf16 exactly under bf16x3f with a conv image backbone
SPELLINGS = {"bf16": (BF16, False, False, BF16, L.BF16), BF16: (BF16, False, False, BF16, L.BF16),
             "fp32": (F32, False, False, F32, L.F32), "f32": (F32, False, False, F32, L.F32), F32: (F32, False, False, F32, L.F32),
             "bf16x3": (F32, True, False, F32, L.F32), "x3": (F32, True, False, F32, L.F32),
             "bf16x3f": (F32, True, True, BF16, L.BF16), "x3f": (F32, True, True, BF16, L.BF16)}
MODE_ENGINES = [
    ("conv", lambda d: MMRCAEngine("distilbert", "shuffle_net", 4, True, 0, d, "cpu")),
    ("vit", lambda d: MMRCAEngine("distilbert", "transformer_B16", 4, True, 0, d, "cpu")),
    ("conv", lambda d: ClassifierEngine("mb", 4, d, "cpu")),
    ("vit", lambda d: ClassifierEngine("transformer_B16", 4, d, "cpu")),
    ("text", lambda d: ClassifierEngine("distilbert", 4, d, "cpu")),
    ("conv", lambda d: HierarchicalEngine("distilbert", dtype=d, device="cpu")),
    ("conv", lambda d: BimodalEngine("distilbert", "shuffle_net", dtype=d, device="cpu", image_size=224)),
]


@pytest.mark.parametrize("image,make", MODE_ENGINES, ids=["mmrca-conv", "mmrca-vit", "cls-conv", "cls-vit", "cls-text", "hier", "bimodal"])
def test_mode_flags_of_every_dtype_spelling(image, make):
    for spelling, (dtype, x3, x3f, gdtype, bdt) in SPELLINGS.items():
        eng = make(spelling)
        conv_dtype = BF16 if (x3f and image == "conv") else None
        assert (eng.dtype, eng.x3, eng.x3f, eng.gdtype, eng.bdt, eng.conv_dtype) == (dtype, x3, x3f, gdtype, bdt, conv_dtype), spelling
        assert eng.dt == L.dtype_code(dtype) and (eng.arena.lp is not None) == (dtype == BF16 or x3) and (eng.arena.lp_lo is not None) == x3
        assert (eng.conv is not None) == (image == "conv")


def test_mobilebert_mode_flags():
    for spelling, dtype in (("fp32", F32), ("f32", F32), (F32, F32), ("bf16", BF16), (BF16, BF16)):
        eng = MobileBertEngine(4, spelling, "cpu")
        assert (eng.dtype, eng.x3, eng.x3f, eng.gdtype, eng.bdt, eng.conv_dtype) == (dtype, False, False, dtype, L.dtype_code(dtype), None)
        assert (eng.arena.lp is not None) == (dtype == BF16) and eng.arena.lp_lo is None
