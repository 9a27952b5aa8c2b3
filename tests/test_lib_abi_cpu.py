"""lib.py against include/mmrca.h as garbage_classification_rca_amd/abi.py reads it: the parser against an independent count, the
types lib.load() gives every declared function and the Python constants against the header, every wrapper of lib.py against the
prototype it calls (a recorder stands in for the library: no GPU), and the conv byte table against recorded values.  Needs only the
cross-compiled library."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

from garbage_classification_rca_amd import abi
from garbage_classification_rca_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmrca.h")


# ------------------------------------------------------------------------------------------------ parser
HEAD_PTR = C.POINTER(L.HeadPtrs)
STRUCT_POINTERS = {"MmrcaHeadWeights": HEAD_PTR, "MmrcaHeadGrads": HEAD_PTR}


def test_parser_finds_every_declared_function_and_the_loaded_library_is_typed_as_the_header_says():
    declared = set(re.findall(r"\b(mmrca_[a-z0-9_]+)\s*\(", open(HEADER).read()))      # test_host_cpu.py's independent regex
    protos = abi.prototypes(HEADER, STRUCT_POINTERS)
    assert set(protos) == declared and len(protos) == len(declared)
    assert len(protos) == 117                          # the one count of entry points in the tree
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    lib = L.load()
    # widths, order and count of every argument and the return type, of every declared function
    for name, (restype, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        assert (fn.restype, list(fn.argtypes)) == (restype, [ctype for ctype, _ in params]), name
    # what lib._launch relies on: every entry point that takes a stream takes it last and reports through an int status
    for name, (restype, params) in protos.items():
        if "stream" in [pname for _, pname in params]:
            assert params[-1] == (C.c_void_p, "stream") and restype is C.c_int, name
    assert L.head_bwd_workspace_bytes(2, 1280, 768) > 0         # host arithmetic
    assert lib.mmrca_last_error.restype is protos["mmrca_last_error"][0] is C.c_char_p and protos["mmrca_last_error"][1] == []
    assert lib.mmrca_version.restype is protos["mmrca_version"][0] is C.c_int
    assert protos["mmrca_head_bwd_workspace_bytes"] == (C.c_int64, [(C.c_int, "B"), (C.c_int, "d_img"), (C.c_int, "d_txt")])
    assert protos["mmrca_gemm_bnstats_slots"] == (C.c_int64, [(C.c_int64, "M")])
    assert protos["mmrca_head_fwd"][1][2] == (HEAD_PTR, "w") and [c for c, _ in protos["mmrca_head_bwd"][1][3:5]] == [HEAD_PTR] * 2
    assert [n for _, n in protos["mmrca_bn_act_fwd"][1]] == ["x", "mean", "rstd", "gamma", "beta", "y", "rows", "C", "act", "dtype", "stream"]


@pytest.mark.parametrize("fragment, word", [
    ("int mmrca_bad(const void* x, long n, void* stream);", "long"),                    # unknown scalar type
    ("int mmrca_bad(const void* x, size_t n);", "size_t"),
    ("int mmrca_bad(const void* x, int (*cb)(int), void* stream);", "mmrca_bad"),       # function-pointer parameter
    ("int mmrca_bad(MMRCA_ARGS(x), int n);", "mmrca_bad"),                              # macro inside a prototype
    ("int mmrca_bad(const void* x, int);", "mmrca_bad"),                                # unnamed parameter
    ("int mmrca_bad(const Unknown* x);", "Unknown"),                                    # pointer to an undeclared type
    ("MMRCA_API int mmrca_bad(int n);", "mmrca_bad"),                                   # macro in front of the return type
    ("float mmrca_bad(int n);", "mmrca_bad"),                                           # return type outside the grammar
    ("int mmrca_bad(int n);\nint mmrca_bad(int n);", "twice"),
])
def test_parser_rejects_what_the_grammar_does_not_cover(tmp_path, fragment, word):
    path = tmp_path / "fragment.h"
    path.write_text("/* a comment; with a semicolon */\n#include <stdint.h>\nint mmrca_good(const float* p, int64_t n, void* stream);\n" + fragment + "\n")
    with pytest.raises(abi.MmrcaError, match=word):
        abi.prototypes(str(path))
    path.write_text("int mmrca_good(const float* p, int64_t n, void* stream);\nconst char* mmrca_text(void);\n")
    assert abi.prototypes(str(path)) == {"mmrca_good": (C.c_int, [(C.c_void_p, "p"), (C.c_int64, "n"), (C.c_void_p, "stream")]),
                                         "mmrca_text": (C.c_char_p, [])}


def test_missing_header_is_an_error_that_says_so(tmp_path):
    with pytest.raises(abi.MmrcaError, match="nowhere.h"):
        abi.prototypes(str(tmp_path / "nowhere.h"))


def test_bind_names_a_declared_function_the_library_lacks(tmp_path):
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    path = tmp_path / "ahead.h"
    path.write_text("int mmrca_version(void);\nint mmrca_not_built_yet(const void* x, int64_t n, void* stream);\n")
    cdll = C.CDLL(L.LIB_PATH)                           # a handle of its own: lib.load()'s functions keep their types
    with pytest.raises(abi.MmrcaError, match=r"mmrca_not_built_yet .*rebuild"):
        abi.bind(cdll, abi.prototypes(str(path)))
    abi.bind(cdll, {"mmrca_version": abi.prototypes(str(path))["mmrca_version"]})
    assert (cdll.mmrca_version.restype, list(cdll.mmrca_version.argtypes)) == (C.c_int, []) and cdll.mmrca_version() >= 1


# ------------------------------------------------------------------------------------------------ constants
def test_python_constants_mirror_the_header():
    h = abi.parse(HEADER)
    assert L.HEAD_FIELDS == h.structs["MmrcaHeadWeights"] == h.structs["MmrcaHeadGrads"]
    assert [n for n, _ in L.HeadPtrs._fields_] == L.HEAD_FIELDS
    dtypes, acts, layouts, impls = h.enums
    assert dtypes == {"MMRCA_F32": L.F32, "MMRCA_BF16": L.BF16}
    assert acts == {"MMRCA_ACT_NONE": L.ACT_NONE, "MMRCA_ACT_GELU": L.ACT_GELU, "MMRCA_ACT_GELU_BWD": L.ACT_GELU_BWD,
                    "MMRCA_ACT_GELU_SAVE_GRAD": L.ACT_GELU_SAVE_GRAD, "MMRCA_ACT_MUL": L.ACT_MUL,
                    "MMRCA_ACT_GELU_SAVE_GRAD_BF16": L.ACT_GELU_SAVE_GRAD_BF16}
    assert layouts == {"MMRCA_ROWK": L.ROWK, "MMRCA_KROW": L.KROW}
    assert impls == {"MMRCA_GEMM_AUTO": L.IMPL_AUTO, "MMRCA_GEMM_REF": L.IMPL_REF, "MMRCA_GEMM_MFMA": L.IMPL_MFMA,
                     "MMRCA_GEMM_MFMA256": L.IMPL_MFMA256, "MMRCA_GEMM_MFMA_PERSIST": L.IMPL_MFMA_PERSIST,
                     "MMRCA_GEMM_MFMA_BK32": L.IMPL_MFMA_BK32, "MMRCA_GEMM_MFMA_1STAGE": L.IMPL_MFMA_1STAGE,
                     "MMRCA_GEMM_MFMA_TALL": L.IMPL_MFMA_TALL, "MMRCA_GEMM_MFMA_256W": L.IMPL_MFMA_256W,
                     "MMRCA_GEMM_MFMA_256X4": L.IMPL_MFMA_256X4}
    assert (0, 1, 2, 3, 4, 5) == (L.ACT_NONE, L.ACT_GELU, L.ACT_GELU_BWD, L.ACT_GELU_SAVE_GRAD, L.ACT_MUL, L.ACT_GELU_SAVE_GRAD_BF16)
    assert len(set(impls.values())) == 10


# ------------------------------------------------------------------------------------------------ marshalling
STREAM = 0x7E0000001000
_ESZ = {torch.float32: 4, torch.bfloat16: 2, torch.int32: 4, torch.int64: 8, torch.uint8: 1}
WORKSPACE_BYTES = 64        # what the recorder answers for every *_workspace_bytes / *_slots query


class _Tensor:
    """stands in for a tensor in HBM: what the wrappers read of one, and a handle no scalar argument can be mistaken for"""
    is_cuda = True
    device = SimpleNamespace(index=0)
    handles = set()

    def __init__(self, dtype=torch.float32, numel=1 << 16):
        self.dtype, self._numel = dtype, numel
        self._ptr = 0x7F0000000000 + 0x1000 * (len(_Tensor.handles) + 1)
        _Tensor.handles.add(self._ptr)

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._numel

    def element_size(self):
        return _ESZ[self.dtype]


class _Recorder:
    """stands in for the loaded library: records every mmrca_* call and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mmrca_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return WORKSPACE_BYTES if name.endswith(("_workspace_bytes", "_slots")) else 0
        return fn


# exports that lib.py has no wrapper for: called through L.load() by preprocess.py, the tools and the tests, or not at all
NO_WRAPPER = {
    "mmrca_last_error",                         # read by _check, only after a failed call
    "mmrca_version",
    "mmrca_debug_set", "mmrca_bn_flat_set", "mmrca_debug_attn_stamps",       # development switches (tools, tests)
    "mmrca_gemm_bnstats_slots",                 # callers size s1 / s2 as ceil(M / 128) themselves
    "mmrca_gemm_splitk_workspace_bytes",        # callers allocate the fixed SPLITK_WS_BYTES
    "mmrca_gemm_streamk_config",                # tools and tests only
    "mmrca_image_preprocess", "mmrca_image_rotate_crop", "mmrca_image_resize_u8", "mmrca_image_stats_u8",
    "mmrca_image_augment",                      # preprocess.py calls these five itself
}
# public functions of lib.py that never reach the library: predicates, conversions and bookkeeping
NOT_A_LAUNCH = {"build_library", "load", "dtype_code", "ptr", "stream_ptr", "gemm_is_mfma", "gemm_splitk_ok", "gemm_splitk_ragged_ok",
                "mha_fwd_planes_ok", "mha_fwd_x3_ok", "seed_epoch_host", "seed_epoch_note", "gemm_bnstats_ok", "bn_fold_ok"}


def _wrapper_calls():
    """(wrapper, positional arguments, keyword arguments) through every branch of every wrapper.  Explicit-workspace forms where
    the default would allocate on a device: head_bwd(workspace=...); streamk_workspace runs with torch.zeros stubbed."""
    f32, b16, i32, i64, u8 = torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8
    t = _Tensor
    w, g = L.HeadPtrs(), L.HeadPtrs()
    gk = dict(M=4, N=5, K=6, lda=7, ldb=8, ldc=9)
    mha = (2, 3, 16, 64, 0.125)                                   # B, H, S, dh, scale
    ln = (5, 6, 7, 8)                                             # rows, D, ld_x, ld_y
    lnb = (5, 6, 7, 8, 9)                                         # rows, D, ld_dy, ld_s, ld_ds
    conv = (2, 5, 7, 8, 2, 80, L.BF16)                            # B, H, W, C, stride, ldk, dtype
    dw = (2, 5, 7, 8, 2, L.BF16)                                  # B, H, W, C, stride, dtype
    bnb = (6, 8, 1, True, L.BF16)                                 # rows, C, act, train, dtype
    bns = (6, 8, 8, 1e-5, 0.1)                                    # rows, C, ld, eps, momentum
    return [
        ("streamk_workspace", (4096, 4096, _Tensor.device), dict(force=True)),
        ("gemm", (t(), t(), t()), dict(bias=t(), addend=t(), preact=t(), accum=True, dtype=L.F32, **gk)),
        ("gemm", (t(), t(), t()), dict(dtype=L.BF16, act=L.ACT_GELU, impl=L.IMPL_MFMA, **gk)),
        ("gemm", (t(), t(), t()), dict(dtype=L.BF16, colsum=t(), preact=t(), act=L.ACT_MUL, **gk)),
        ("gemm", (t(), t(), t()), dict(dtype=L.BF16, rows_readable=(4, 256), impl=L.IMPL_MFMA256, **gk)),
        ("gemm", (t(), t(), t()), dict(dtype=L.BF16, rows_readable=(4, 256), colsum=t(), **gk)),
        ("gemm_splitk", (t(), t(), t(), t(u8)), gk),
        ("gemm_x3", ((t(), t()), (t(), t()), t()), dict(C_lo=t(), bias=t(), addend=t(), preact=t(), colsum=t(), **gk)),
        ("gemm_x3", ((t(), t()), (t(), t()), t()), dict(accum=True, a_layout=L.KROW, b_layout=L.KROW, **gk)),
        ("gemm_splitk_x3", ((t(), t()), (t(), t()), t(), t(u8)), gk),
        ("split_f32", (t(), t(), t(), 64), {}),
        ("colsum_accum", (t(), t(), 4, 5, 6, L.BF16), {}),
        ("gelu_bwd", (t(), t(), t(), 64, L.BF16), {}),
        ("gelu_bwd_colsum", (t(), t(), t(), t(), 4, 5, 6, L.BF16), {}),
        ("mha_fwd", (t(), t(i32), t(), t()) + mha + (L.BF16,), dict(impl=L.IMPL_MFMA, drop_p=0.1, drop_seed=2 ** 63 + 5, cu=t(i32))),
        ("mha_fwd", (t(), None, t(), t()) + mha + (L.F32,), {}),
        ("mha_fwd_planes", (t(), t(i32), t(), (t(), t()), t()) + mha, dict(drop_p=0.1, drop_seed=7, cu=t(i32))),
        ("mha_fwd_planes", (t(), None, t(), (t(), t()), t()) + mha, {}),
        ("mha_fwd_planes_in", ((t(), t()), t(i32), t(), (t(), t()), t()) + mha, dict(drop_p=0.1, drop_seed=7, cu=t(i32))),
        ("mha_fwd_planes_in", ((t(), t()), None, None, (t(), t()), t()) + mha, {}),
        ("mha_fwd_x3", ((t(), t()), t(i32), (t(), t()), t()) + mha, dict(drop_p=0.1, drop_seed=7, cu=t(i32))),
        ("mha_fwd_x3", ((t(), t()), None, (t(), t()), t()) + mha, {}),
        ("mha_bwd", (t(), t(i32), t(), t(), t(), t()) + mha + (L.BF16,), dict(impl=L.IMPL_MFMA, drop_p=0.1, drop_seed=7, cu=t(i32))),
        ("mha_bwd", (t(), None, t(), t(), t(), t()) + mha + (L.BF16,), dict(colsum=t())),
        ("mha_bwd", (t(), None, t(), t(), t(), t()) + mha + (L.BF16,), dict(colsum=t(), cu=t(i32), rows=30)),
        ("mha_cross_fwd", (t(), 264, t(), 265, t(), 266, t(), 88, 2, 3, 32, 257, 88, 0.1, L.BF16), dict(impl=L.IMPL_MFMA, drop_p=0.1, drop_seed=7)),
        ("mha_cross_fwd_x3", (t(), 264, t(), 265, t(), 266, (t(b16), t(b16)), 88, 2, 3, 32, 257, 88, 0.1), dict(drop_p=0.1, drop_seed=7)),
        ("mha_cls_fwd", (t(), t(i32), t(), t()) + mha + (L.BF16,), dict(drop_p=0.1, drop_seed=7, cu=t(i32))),
        ("mha_cls_fwd", (t(), None, t(), t()) + mha + (L.F32,), {}),
        ("mha_cls_bwd", (t(), t(i32), t(), t(), t(), t()) + mha + (L.BF16,), dict(drop_p=0.1, drop_seed=7, cu=t(i32))),
        ("mha_cls_bwd", (t(), None, t(), t(), t(), t()) + mha + (L.F32,), {}),
        ("add_layernorm_fwd", (t(), t(), t(), t(), t(), t(), t(), t()) + ln + (1e-6, L.BF16), dict(in_drop=(0.1, 3), out_drop=(0.2, 4))),
        ("add_layernorm_fwd", (t(), None, t(), t(), None, t(), None, None) + ln + (1e-6, L.F32), {}),
        ("add_layernorm_fwd", (t(), t(), t(), t(), t(), None, t(), t()) + ln + (1e-6, L.F32), dict(y_planes=(t(b16), t(b16)), in_drop=(0.1, 3))),
        ("layernorm_bwd", tuple(t() for _ in range(9)) + lnb + (L.BF16,),
         dict(dy_drop=(0.1, 3), branch_drop=(0.2, 4), dbranch=t(), dcol=t(), dcol_branch=t())),
        ("layernorm_bwd", (t(), t(), t(), t(), t(), None, t(), t(), t()) + lnb + (L.F32,), {}),
        ("layernorm_bwd_mixed", tuple(t() for _ in range(9)) + lnb, dict(dy_drop=(0.1, 3), branch_drop=(0.2, 4), dbranch=t(), dcol=t(), dcol_branch=t())),
        ("layernorm_bwd_mixed", (t(), t(), t(), t(), t(), None, t(), t(), t()) + lnb, {}),
        ("embed_fwd", (t(i32), t(i32), t(), t(), t(), t(), 5, 6, L.BF16), {}),
        ("embed_bwd", (t(), t(i32), t(i32), t(), t(), t(), 5, 6, L.BF16), dict(pad_id=0, pos_pad_id=1)),
        ("embed_bwd", (t(), t(i32), t(i32), t(), t(), None, 5, 6, L.F32), {}),
        ("patchify_fwd", (t(), t(), 2, 3, 32, 48, 16, L.BF16), {}),
        ("vit_assemble_fwd", (t(), t(), t(), t(), 2, 6, 8, L.BF16), {}),
        ("vit_assemble_bwd", (t(), t(), t(), t(), 2, 6, 8, L.BF16), {}),
        ("head_fwd", (t(), t(), w, t(), 2, 1280, 768, 4, True, 1, 0.1, 7, L.BF16), {}),
        ("head_bwd_workspace_bytes", (2, 1280, 768), {}),
        ("head_bwd", (t(), t(), t(), w, g, t(), t(), 2, 1280, 768, 4, False, 0, 0.1, 7, L.BF16), dict(workspace=t(u8))),
        ("head_bwd", (t(), t(), t(), w, g, None, None, 2, 1280, 768, 4, True, 2, 0.0, 7, L.F32), dict(workspace=t(u8))),
        ("linear_cls_fwd", (t(), 8, t(), t(), t(), 2, 8, 4, 0.1, -3, L.BF16), {}),
        ("linear_cls_bwd", (t(), t(), 8, t(), t(), t(), t(), 2, 8, 4, 0.1, -3, L.BF16), {}),
        ("linear_cls_bwd", (t(), t(), 8, t(), t(), t(), None, 2, 8, 4, 0, 9, L.F32), {}),
        ("xent_fwd_bwd", (t(), t(i32), t(), 0.1, t(), t(), 2, 4), dict(grad_scale=0.5)),
        ("xent_fwd_bwd", (t(), t(i32), None, 0.0, t(), None, 2, 4), {}),
        ("sgd_step", (t(), t(), t(b16), 64, 1e-3, 1e-2), dict(grad_scale=0.5)),
        ("sgd_step", (t(), t(), None, 64, 1e-3, 1e-2), {}),
        ("sgd_step", (t(), t(), t(b16), 64, 1e-3, 1e-2), dict(lp_lo=t(b16))),
        ("adamw_step", (t(), t(), t(), t(), t(b16), 64, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3), dict(grad_scale=0.5)),
        ("adamw_step", (t(), t(), t(), t(), t(b16), 64, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3), dict(lp_lo=t(b16))),
        ("hier_pool_fwd", (t(), t(), 96, 2, 6, 6, 8, 3, L.BF16), {}),
        ("hier_pool_bwd", (t(), 96, t(), 2, 6, 6, 8, 3, L.BF16), {}),
        ("hier_norm_fwd", (t(), t(), t(), 2, 12, [0, 4, 8, 12], 2, 0.1, -1, 7), {}),
        ("hier_norm_bwd", (t(), t(), t(), t(), 2, 12, [0, 4, 8, 12], 2, 0.1, -1, 7), {}),
        ("hier_linear_workspace_bytes", (2, 64, 256), {}),
        ("hier_linear_relu_fwd", (t(), 256, t(), t(), t(), 64, t(), 2, 64, 256), {}),
        ("hier_linear_relu_bwd", (t(), 64, t(), 68, t(), 256, t(), t(), t(), t(), 260, t(), 2, 64, 256), {}),
        ("hier_linear_relu_bwd", (t(), 64, t(), 68, t(), 256, t(), t(), t(), None, 260, None, 2, 64, 256), {}),
        ("gru_linear_fwd", (t(), 8, t(), t(), t(), 12, 2, 12, 8), dict(relu=True)),
        ("gru_linear_fwd", (t(), 8, t(), None, t(), 12, 2, 12, 8), {}),
        ("gru_linear_bwd", (t(), 12, t(), 13, t(), 8, t(), t(), t(), t(), 9, 2, 12, 8), {}),
        ("gru_linear_bwd", (t(), 12, None, 13, t(), 8, t(), None, None, None, 9, 2, 12, 8), {}),
        ("gru_fwd", tuple([t(), t()] for _ in range(6)) + (3, 4), {}),
        ("gru_bwd", tuple([t()] for _ in range(5)) + ([4],) + tuple([t()] for _ in range(3)) + (3, 4), {}),
        ("hadamard_fwd", (t(), 8, t(), 9, t(), t(), t(), t(), 10, 2, 8), {}),
        ("hadamard_bwd", (t(), 8, t(), 9, t(), 10, t(), 11, t(), 12, t(), t(), t(), 13, t(), 14, t(), t(), t(), 2, 8), {}),
        ("hadamard_bwd", (t(), 8, None, 9, t(), 10, t(), 11, t(), 12, t(), t(), t(), 13, t(), 14, t(), t(), t(), 2, 8), {}),
        ("dropout_f32", (t(), 8, t(), 9, 2, 8, 0.1, -5), {}),
        ("seed_epoch_set", (5,), {}),
        ("seed_epoch_set", (), dict(device_value=t(i64, 1))),
        ("sd_rowscale", (t(f32, 3), t(f32, 6), 3, 2, -9), {}),
        ("cast_f32_to_bf16", (t(), t(b16), 64), {}),
        ("nchw_to_rows", (t(), t(), 2, 3, 5, 7, L.BF16), {}),
        ("im2row3x3", (t(), t()) + conv, {}), ("col2im3x3", (t(), t()) + conv, {}),
        ("im2row3x3_tap", (t(), t()) + conv, {}), ("col2im3x3_tap", (t(), t()) + conv, {}),
        ("dwconv3x3_fwd", (t(), t(), t()) + dw, {}),
        ("dwconv3x3_bwd", (t(), t(), t(), t(), t()) + dw, {}),
        ("dwconv3x3_bwd", (t(), t(), t(), None, None) + dw, dict(ws=t())),
        ("dwconv5x5_fwd", (t(), t(), t()) + dw, {}),
        ("dwconv5x5_bwd", (t(), t(), t(), t(), t()) + dw, {}),
        ("dwconv5x5_bwd", (t(), t(), t(), None, None) + dw, dict(ws=t())),
        ("conv3x3_stat_slots", (2, 5, 7), {}),
        ("conv3x3_fwd", (t(), t(), t(), 2, 5, 7, 8, 16, L.BF16), {}),
        ("conv3x3_fwd", (t(), t(), t(), 2, 5, 7, 8, 16, L.BF16), dict(parts=(t(), t(), t()))),
        ("conv_bn_finish", ((t(), t(), t()), 2, 5, 7, t(), t(), t(), t(), 16, 1e-5, 0.1), {}),
        ("conv_bn_finish", ((t(), t(), t()), 2, 5, 7, t(), t(), None, None, 16, 1e-5, 0.0), {}),
        ("conv3x3_wgrad", (t(), t(), t(), 2, 5, 7, 8, 16, L.BF16), {}),
        ("gemm_bnstats", (t(), t(), t()), dict(dtype=L.BF16, shift=t(), s1=t(), s2=t(), **gk)),
        ("gemm_bnstats", (t(), t(), t()), dict(dtype=L.BF16, shift=None, s1=t(), s2=t(), **gk)),
        ("bn_finish_sums", (t(), t(), t(), 3, 300, t(), t(), t(), t(), 8, 1e-5, 0.1), {}),
        ("bn_moments", (t(), t(), t(), t(), 6, 8, 8, L.BF16), {}),
        ("bn_act_fwd_fin", tuple(t() for _ in range(13)) + (6, 8, 1, 3, 1e-5, 0.1, L.BF16), {}),
        ("bn_act_fwd_fin", tuple(t() for _ in range(6)) + (None, None) + tuple(t() for _ in range(5)) + (6, 8, 1, 3, 1e-5, 0.1, L.BF16), {}),
        ("bn_act_fwd_res", tuple(t() for _ in range(8)) + (6, 8, 1, 3, L.BF16), {}),
        ("bn_act_fwd_res", tuple(t() for _ in range(6)) + (None, t(), 6, 8, 1, 3, L.BF16), {}),
        ("bn_stats", tuple(t() for _ in range(5)) + bns + (True, L.BF16), {}),
        ("bn_stats", tuple(t() for _ in range(5)) + bns + (False, L.F32), {}),
        ("bn_stats", tuple(t() for _ in range(5)) + bns + (True, L.BF16), dict(ws=t())),
        ("bn_stats", tuple(t() for _ in range(5)) + bns + (True, L.BF16), dict(prezeroed=True)),
        ("bn_stats", tuple(t() for _ in range(5)) + bns + (True, L.BF16), dict(ws=t(), prezeroed=True, tickets=t(i32, 1))),
        ("bn_stats", tuple(t() for _ in range(5)) + bns + (True, L.BF16), dict(tickets=t(i32, 1))),
        ("bn_stats", tuple(t() for _ in range(5)) + bns + (True, L.BF16), dict(tickets=t(i32, 1), prezeroed=True)),
        ("bn_stats", tuple(t() for _ in range(5)) + bns + (False, L.BF16), dict(tickets=t(i32, 1))),
        ("bn_act_fwd", tuple(t() for _ in range(6)) + (6, 8, 1, L.BF16), {}),
        ("bn_act_bwd", tuple(t() for _ in range(10)) + bnb, {}),
        ("bn_act_bwd", tuple(t() for _ in range(6)) + (None, None, None) + (t(),) + bnb, {}),
        ("bn_act_bwd", tuple(t() for _ in range(10)) + bnb, dict(sums_ready=True)),
        ("bn_act_bwd", tuple(t() for _ in range(10)) + bnb, dict(sums_ready=True, ws=t(), prezeroed=True)),
        ("bn_act_bwd", tuple(t() for _ in range(10)) + bnb, dict(ws=t())),
        ("bn_act_bwd", tuple(t() for _ in range(10)) + bnb, dict(prezeroed=True)),
        ("rowpool_mean", (t(), t(), 2, 35, 8, L.BF16), {}),
        ("rowpool_mean_bwd", (t(), t(), 2, 35, 8, True, L.BF16), {}),
        ("se_mlp_fwd", tuple(t() for _ in range(9)) + (2, 8, 4, L.BF16), {}),
        ("se_mlp_bwd", tuple(t() for _ in range(16)) + (2, 8, 4, L.BF16), {}),
        ("se_scale_fwd", (t(), t(), t(), 2, 35, 8, L.BF16), {}),
        ("se_scale_bwd", (t(), t(), t(), t(), t(), 2, 35, 8, L.BF16), {}),
        ("se_scale_bwd", (t(), t(), t(), None, t(), 2, 35, 8, L.BF16), {}),
        ("se_dx", (t(), t(), t(), t(), 2, 35, 8, L.BF16), {}),
        ("se_dx", (t(), t(), t(), t(), 2, 35, 8, L.BF16), dict(bn=(t(), t(), t(), t(), t(), 1, t()))),
        ("bias_act_fwd", (t(), t(), t(), 6, 8, 1, L.BF16), {}),
        ("bias_act_bwd", (t(), t(), t(), t(), t(), 6, 8, 1, L.BF16), {}),
        ("residual_add", (t(), t(), t(), t(), 2, 280, L.BF16), {}),
        ("residual_add", (None, t(), None, t(), 2, 280, L.BF16), {}),
        ("maxpool3x3s2_fwd", (t(), t(), t(u8), 2, 5, 7, 8, L.BF16), {}),
        ("maxpool3x3s2_bwd", (t(), t(u8), t(), 2, 5, 7, 8, L.BF16), {}),
        ("channel_interleave2", (t(), 16, t(), t(), 6, 8, L.BF16), {}),
        ("channel_deinterleave2", (t(), t(), 16, t(), 6, 8, L.BF16), {}),
        ("channel_gather", (t(), t(i32), t(), 6, 8, 4, 12, 2, L.BF16), {}),
        ("nonorm_fwd", (t(), t(), t(), t(), t(), t(), 5, 6, 7, 8, 9, 10, L.BF16), {}),
        ("nonorm_fwd", (t(), None, t(), t(), None, t(), 5, 6, 7, 8, 9, 10, L.F32), {}),
        ("nonorm_bwd_workspace_bytes", (5, 6), {}),
        ("nonorm_bwd", tuple(t() for _ in range(9)) + (5, 6, 7, 8, 9, 10, L.BF16), {}),
        ("nonorm_bwd", (t(), t(), t(), None, t(), t(), t(), None, t()) + (5, 6, 7, 8, 9, 10, L.F32), {}),
        ("trigram_embed_fwd", (t(i32), t(i32), t(), t(), 10, 2, 8, 4, 100, L.BF16), {}),
        ("trigram_embed_fwd", (t(i32), None, t(), t(), 16, 2, 8, 4, 100, L.F32), {}),
        ("trigram_embed_bwd", (t(), t(i32), t(i32), t(), 10, 2, 8, 4, 100, 0, L.BF16), {}),
    ]


_INT_RANGE = {C.c_int: (-2 ** 31, 2 ** 31), C.c_int64: (-2 ** 63, 2 ** 63), C.c_uint64: (0, 2 ** 64)}


def _check_call(name, args, protos):
    restype, params = protos[name]
    assert len(args) == len(params), f"{name}: {len(args)} arguments for {len(params)} parameters"
    for v, (ctype, pname) in zip(args, params):
        where = f"{name}({pname}) <- {v!r}"
        ctype.from_param(v)                                       # what ctypes itself does with the typed function
        is_handle = v is None or (isinstance(v, int) and not isinstance(v, bool) and (v in _Tensor.handles or v == STREAM))
        if ctype is C.c_void_p or ctype is C.POINTER(L.HeadPtrs):
            assert is_handle or isinstance(v, C.Array) or type(v).__name__ == "CArgObject", where      # a handle, a host table or byref()
        else:
            assert not is_handle and isinstance(v, (int, float)), where
            if ctype in _INT_RANGE:
                lo, hi = _INT_RANGE[ctype]
                assert isinstance(v, int) and lo <= v < hi, where
    if params and params[-1][1] == "stream":
        assert args[-1] == STREAM, name


def test_every_wrapper_marshals_what_the_header_declares(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(L, "_lib", rec)
    monkeypatch.setattr(L, "stream_ptr", lambda: STREAM)
    monkeypatch.setattr(L, "_STREAMK_WS", {})
    monkeypatch.setattr(L, "_seed_epoch", L._seed_epoch)
    monkeypatch.setattr(torch, "zeros", lambda n, dtype, device: _Tensor(dtype, n))          # streamk_workspace's allocation

    def no_events():
        raise AssertionError("a wrapper created timing events with every profile list off")
    monkeypatch.setattr(L, "_events", no_events)
    assert L.GEMM_PROFILE is None and L.KERNEL_PROFILE is None and L.CONV_PROFILE is None and L.GEMM_SHAPES is None
    protos = abi.prototypes(HEADER, STRUCT_POINTERS)
    called = set()
    for wrapper, args, kwargs in _wrapper_calls():
        before = len(rec.calls)
        getattr(L, wrapper)(*args, **kwargs)
        assert len(rec.calls) > before, f"{wrapper} did not reach the library"
        called.add(wrapper)
    for name, args in rec.calls:
        _check_call(name, args, protos)
    public = {n for n, f in vars(L).items() if inspect.isfunction(f) and f.__module__ == L.__name__ and not n.startswith("_")}
    assert public - NOT_A_LAUNCH == called, (public - NOT_A_LAUNCH) ^ called
    assert len(called) == 92
    reached = {name for name, _ in rec.calls}
    assert reached == set(protos) - NO_WRAPPER, reached ^ (set(protos) - NO_WRAPPER)
    assert NO_WRAPPER <= set(protos)
    assert len(L._STREAMK_WS) == 1                                 # the registration went through


def test_check_call_catches_a_handle_in_a_scalar_slot_and_a_missing_argument():
    """the checker of the test above, on three wrong calls"""
    protos = abi.prototypes(HEADER)
    h = _Tensor().data_ptr()
    _check_call("mmrca_split_f32", (h, h, h, 64, STREAM), protos)
    with pytest.raises(AssertionError):
        _check_call("mmrca_split_f32", (h, h, 64, h, STREAM), protos)          # swapped pointer / count
    with pytest.raises(AssertionError):
        _check_call("mmrca_split_f32", (h, h, h, 64), protos)                  # the stream is missing
    with pytest.raises((AssertionError, TypeError)):
        _check_call("mmrca_split_f32", (h, h, h, 64.0, STREAM), protos)        # a float where the header says int64_t


# ------------------------------------------------------------------------------------------------ byte table
# (entry point, launch arguments without the stream, family, algorithmic bytes): the bytes are what the positional table this one
# replaced gave for these tuples -- one per key and per arm of a conditional (train, accumulate, res / dx / dw / z / a given or not),
# pairwise distinct sizes so that two swapped names change the product
BYTE_CASES = [
    ("mmrca_nchw_to_rows", (9001, 9002, 3, 5, 7, 11, 1), "layout", 6930),
    ("mmrca_nchw_to_rows", (9001, 9002, 3, 5, 7, 11, 0), "layout", 9240),
    ("mmrca_im2row3x3", (9001, 9002, 3, 5, 7, 11, 2, 13, 1), "patches", 3246),
    ("mmrca_col2im3x3", (9001, 9002, 3, 5, 7, 11, 2, 13, 1), "patches", 3246),
    ("mmrca_im2row3x3_tap", (9001, 9002, 3, 5, 7, 11, 2, 13, 1), "patches", 3246),
    ("mmrca_col2im3x3_tap", (9001, 9002, 3, 5, 7, 11, 2, 13, 1), "patches", 3246),
    ("mmrca_dwconv3x3_fwd", (9001, 9002, 9003, 3, 5, 7, 11, 2, 1), "depthwise", 3102),
    ("mmrca_dwconv3x3_bwd", (9001, 9002, 9003, 9004, 9005, 3, 5, 7, 11, 2, 1), "depthwise", 5412),
    ("mmrca_dwconv3x3_bwd_ws", (9001, 9002, 9003, 9004, 9005, 3, 5, 7, 11, 2, 1, 9012, 13), "depthwise", 5412),
    ("mmrca_dwconv5x5_fwd", (9001, 9002, 9003, 3, 5, 7, 11, 2, 1), "depthwise 5x5", 3102),
    ("mmrca_dwconv5x5_bwd_ws", (9001, 9002, 9003, 9004, 9005, 3, 5, 7, 11, 2, 1, 9012, 13), "depthwise 5x5", 5412),
    ("mmrca_dwconv5x5_bwd_ws", (9001, 9002, 9003, None, 9005, 3, 5, 7, 11, 2, 1, 9012, 13), "depthwise 5x5", 3102),
    ("mmrca_dwconv5x5_bwd_ws", (9001, 9002, 9003, 9004, None, 3, 5, 7, 11, 2, 1, 9012, 13), "depthwise 5x5", 3102),
    ("mmrca_dwconv5x5_bwd_ws", (9001, 9002, 9003, None, None, 3, 5, 7, 11, 2, 1, 9012, 13), "depthwise 5x5", 792),
    ("mmrca_conv3x3_fwd", (9001, 9002, 9003, 9004, 9005, 9006, 3, 5, 7, 11, 13, 1), "conv3x3 implicit GEMM", 7614),
    ("mmrca_conv3x3_wgrad", (9001, 9002, 9003, 3, 5, 7, 11, 13, 1), "conv3x3 implicit GEMM", 10188),
    ("mmrca_gemm_bnstats", (9001, 9002, 9003, 3, 5, 7, 11, 13, 17, 1, 9011, 9012, 9013), "GEMM (1x1 / patch)", 142),
    ("mmrca_channel_interleave2", (9001, 3, 9003, 9004, 5, 7, 1), "layout", 280),
    ("mmrca_channel_deinterleave2", (9001, 9002, 3, 9004, 5, 7, 1), "layout", 280),
    ("mmrca_bn_stats", (9001, 9002, 9003, 9004, 9005, 3, 5, 7, 0.5, 0.5, 1, 1), "BatchNorm", 30),
    ("mmrca_bn_stats", (9001, 9002, 9003, 9004, 9005, 3, 5, 7, 0.5, 0.5, 0, 1), "BatchNorm", 0),
    ("mmrca_bn_stats_ws", (9001, 9002, 9003, 9004, 9005, 3, 5, 7, 0.5, 0.5, 1, 1, 9013, 11, 1), "BatchNorm", 30),
    ("mmrca_bn_stats_ws", (9001, 9002, 9003, 9004, 9005, 3, 5, 7, 0.5, 0.5, 0, 1, 9013, 11, 1), "BatchNorm", 0),
    ("mmrca_bn_stats_fused", (9001, 9002, 9003, 9004, 9005, 3, 5, 7, 0.5, 0.5, 1, 9012, 1), "BatchNorm", 30),
    ("mmrca_bn_act_fwd", (9001, 9002, 9003, 9004, 9005, 9006, 3, 5, 7, 1), "BatchNorm", 60),
    ("mmrca_bn_act_fwd_res", (9001, 9002, 9003, 9004, 9005, 9006, 9007, 9008, 3, 5, 7, 11, 1), "BatchNorm", 90),
    ("mmrca_bn_moments", (9001, 9002, 9003, 9004, 3, 5, 7, 1), "BatchNorm", 30),
    ("mmrca_bn_act_fwd_fin", (9001, 9002, 9003, 9004, 9005, 9006, 9007, 9008, 9009, 9010, 9011, 9012, 9013, 3, 5, 7, 11, 0.5, 0.5, 1), "BatchNorm", 90),
    ("mmrca_bn_act_fwd_fin", (9001, 9002, 9003, 9004, 9005, 9006, None, 9008, 9009, 9010, 9011, 9012, 9013, 3, 5, 7, 11, 0.5, 0.5, 1), "BatchNorm", 60),
    ("mmrca_bn_act_bwd", (9001, 9002, 9003, 9004, 9005, 9006, 9007, 9008, 9009, 9010, 3, 5, 7, 1, 1), "BatchNorm", 150),
    ("mmrca_bn_act_bwd", (9001, 9002, 9003, 9004, 9005, 9006, 9007, 9008, 9009, 9010, 3, 5, 7, 0, 1), "BatchNorm", 90),
    ("mmrca_bn_act_bwd_ws", (9001, 9002, 9003, 9004, 9005, 9006, 9007, 9008, 9009, 9010, 3, 5, 7, 1, 1, 9016, 11, 1), "BatchNorm", 150),
    ("mmrca_bn_act_bwd_ws", (9001, 9002, 9003, 9004, 9005, 9006, 9007, 9008, 9009, 9010, 3, 5, 7, 0, 1, 9016, 11, 1), "BatchNorm", 90),
    ("mmrca_bn_act_bwd_sums", (9001, 9002, 9003, 9004, 9005, 9006, 9007, 9008, 9009, 9010, 3, 5, 7, 1, 1), "BatchNorm", 90),
    ("mmrca_rowpool_mean", (9001, 9002, 3, 5, 7, 1), "pool / squeeze-excitation", 210),
    ("mmrca_rowpool_mean_bwd", (9001, 9002, 3, 5, 7, 1, 1), "pool / squeeze-excitation", 420),
    ("mmrca_rowpool_mean_bwd", (9001, 9002, 3, 5, 7, 0, 1), "pool / squeeze-excitation", 210),
    ("mmrca_se_scale_fwd", (9001, 9002, 9003, 3, 5, 7, 1), "pool / squeeze-excitation", 420),
    ("mmrca_se_mlp_fwd", (9001, 9002, 9003, 9004, 9005, 9006, 9007, 9008, 9009, 3, 5, 7, 1), "pool / squeeze-excitation", 356),
    ("mmrca_se_mlp_bwd", (9001, 9002, 9003, 9004, 9005, 9006, 9007, 9008, 9009, 9010, 9011, 9012, 9013, 9014, 9015, 9016, 3, 5, 7, 1), "pool / squeeze-excitation", 852),
    ("mmrca_se_scale_bwd", (9001, 9002, 9003, 9004, 9005, 3, 5, 7, 1), "pool / squeeze-excitation", 630),
    ("mmrca_se_scale_bwd", (9001, 9002, 9003, None, 9005, 3, 5, 7, 1), "pool / squeeze-excitation", 420),
    ("mmrca_se_dx", (9001, 9002, 9003, 9004, 3, 5, 7, 1, 9009, 9010, 9011, 9012, 9013, 11, 9015), "pool / squeeze-excitation", 630),
    ("mmrca_se_dx", (9001, 9002, 9003, 9004, 3, 5, 7, 1, None, 9010, 9011, 9012, 9013, 11, 9015), "pool / squeeze-excitation", 420),
    ("mmrca_residual_add", (9001, 9002, 9003, 9004, 3, 5, 1), "residual", 90),
    ("mmrca_residual_add", (None, 9002, 9003, 9004, 3, 5, 1), "residual", 60),
    ("mmrca_maxpool3x3s2_fwd", (9001, 9002, 9003, 3, 5, 7, 11, 1), "pool / squeeze-excitation", 3498),
    ("mmrca_maxpool3x3s2_bwd", (9001, 9002, 9003, 3, 5, 7, 11, 1), "pool / squeeze-excitation", 3498),
    ("mmrca_channel_gather", (9001, 9002, 9003, 3, 5, 7, 11, 13, 1), "layout", 84),
]


class _Event:
    def record(self):
        pass


def test_conv_byte_table_is_unchanged(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(L, "_lib", rec)
    monkeypatch.setattr(L, "stream_ptr", lambda: STREAM)
    monkeypatch.setattr(L, "_events", lambda: (_Event(), _Event()))
    monkeypatch.setattr(L, "CONV_PROFILE", [])
    for name, args, family, nbytes in BYTE_CASES:
        L._c(name, *args)
        fam, got, e0, e1 = L.CONV_PROFILE[-1]
        assert (fam, got) == (family, nbytes) and type(got) is int, (name, args, fam, got)
        assert isinstance(e0, _Event) and isinstance(e1, _Event) and e0 is not e1
        assert rec.calls[-1] == (name, args + (STREAM,))
    assert len(L.CONV_PROFILE) == len(BYTE_CASES)
    assert {name for name, *_ in BYTE_CASES} == set(L._CONV_BYTES)
    L._c("mmrca_bias_act_fwd", 1, 2, 3, 6, 8, 1, L.BF16)           # not in the table: counted under "other" with 0 bytes
    assert L.CONV_PROFILE[-1][:2] == ("other", 0)
    monkeypatch.setattr(L, "CONV_PROFILE", None)
    monkeypatch.setattr(L, "_events", None)                        # the unprofiled path makes no events
    L._c(*BYTE_CASES[0][:1], *BYTE_CASES[0][1])
    assert rec.calls[-1] == (BYTE_CASES[0][0], BYTE_CASES[0][1] + (STREAM,))
