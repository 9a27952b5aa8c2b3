"""The bf16x3 attention forward at 225 <= S <= 512 (mha_fwd_x3_c_k, csrc/attention_mfma.hip), the part that needs no GPU: the range
lib.py announces to the engines, and that the C ABI did not grow for it (the same entry point, the same prototype, the same binding)."""
import ctypes as C
import os
import re

import pytest

from garbage_classification_rca_amd import abi
from garbage_classification_rca_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmrca.h")

# mmrca_mha_fwd_x3's parameter list as it stood before the range grew
X3_PARAMS = [("qkv_hi", C.c_void_p), ("qkv_lo", C.c_void_p), ("key_mask", C.c_void_p), ("out_hi", C.c_void_p), ("out_lo", C.c_void_p),
             ("lse", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("S", C.c_int32), ("dh", C.c_int32), ("scale", C.c_float),
             ("drop_p", C.c_float), ("drop_seed", C.c_uint64), ("cu_seqlens", C.c_void_p), ("stream", C.c_void_p)]


@pytest.mark.parametrize("S,dh,ok", [(1, 64, True), (224, 64, True), (225, 64, True), (512, 64, True), (513, 64, False), (300, 32, False)])
def test_the_range_lib_announces(S, dh, ok):
    assert L.mha_fwd_x3_ok(S, dh) is ok


def test_the_entry_point_keeps_its_prototype_and_the_table_its_size():
    text = open(HEADER).read()
    m = re.search(r"\bint\s+mmrca_mha_fwd_x3\s*\(([^)]*)\)\s*;", text)
    assert m, "include/mmrca.h no longer declares mmrca_mha_fwd_x3"
    names = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert names == [n for n, _ in X3_PARAMS]
    restype, params = abi.prototypes(HEADER, {"MmrcaHeadWeights": C.POINTER(L.HeadPtrs), "MmrcaHeadGrads": C.POINTER(L.HeadPtrs)})["mmrca_mha_fwd_x3"]
    assert restype is C.c_int
    assert [ctype for ctype, _ in params] == [t for _, t in X3_PARAMS] == list(L.load().mmrca_mha_fwd_x3.argtypes)
    assert L.load().mmrca_mha_fwd_x3.restype is C.c_int
    assert all(getattr(L.load(), name).argtypes is not None for name in set(re.findall(r"\b(mmrca_[a-z0-9_]+)\s*\(", text)))
    assert "1 <= S <= 512" in text[m.start() - 900:m.start()]          # the comment above the prototype names the new range
