"""Launch traces: the ordered list of libmmrca calls one ``forward`` (+ ``backward``) of an engine makes, in a canonical text form.

No GPU and no libmmrca.so: a recorder stands in for the loaded library (as in tests/test_lib_abi_cpu.py) and the engines run on
``device="cpu"``, where every buffer is an ordinary tensor nobody computes on.  ``install`` patches what ties the engines to a
GPU; ``lib.ptr`` is patched to hand the recorder the tensor itself, so every pointer a wrapper passes resolves to (storage,
offset) exactly; integers taken with ``.data_ptr()`` directly (the head's pointer struct, the GRU pointer tables) resolve by address range.

Canonical form of one call:  ``name(arg, arg, ...)`` with the arguments in the order of the prototype in include/mmrca.h --
non-pointer arguments as passed (floats by repr), pointer arguments as symbols:

    <plane>+<element offset>            a pointer into a named plane (the arenas ``p`` / ``g`` / ``lp`` / ``lp_lo``; the BLIP-2 engine's
                                        ``store`` / ``w_hi`` / ``w_lo`` / ``cls_p`` / ``cls_g`` / ``cls_m`` / ``cls_v``)
    ids | mask | images | dlogits +off  a pointer into an input, by its role
    #k:<dtype>:<numel>+<offset>         any other allocation; k numbers the distinct allocations in order of first appearance in the trace
    None                                a null pointer

so buffer NAMES do not enter a trace, while which launches share a buffer, its size and its dtype do.  The configurations of
tests/golden/launch_traces.json are listed in ``CONFIGS``; tests/golden/make_launch_traces.py wrote that file ONCE, from the engine code as
it stood before the per-layer forwards were folded, and tests/test_launch_trace_cpu.py holds the engines to it.
"""
import ctypes as C
import hashlib
from types import SimpleNamespace

import torch

from garbage_classification_rca_amd import abi
from garbage_classification_rca_amd import engine as E
from garbage_classification_rca_amd import lib as L
from garbage_classification_rca_amd import q_former as QF

DIGEST_HEX = 6          # 24 bits per call: a changed launch goes unnoticed with probability 6e-8
WORKSPACE_BYTES = 64    # what the recorder answers for every *_workspace_bytes / *_slots query


class TraceError(AssertionError):
    pass


class Recorder:
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


def install(mp) -> Recorder:
    """mp: pytest's monkeypatch (or a pytest.MonkeyPatch()).  Everything is undone with it."""
    rec = Recorder()
    mp.setattr(L, "_lib", rec)
    mp.setattr(L, "load", lambda *a, **k: rec)
    mp.setattr(L, "ptr", lambda t: t)
    mp.setattr(L, "_dev", lambda t, name: None)
    mp.setattr(L, "stream_ptr", lambda: 0)
    mp.setattr(L, "_HEAD_WS", {})
    mp.setattr(E.MMRCAEngine, "_check_resident", lambda self, *named: None)
    mp.setattr(torch.cuda, "current_stream", lambda *a, **k: SimpleNamespace(cuda_stream=0))
    return rec


# ------------------------------------------------------------------------------------------------ canonical form
_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.int64: "i64", torch.uint8: "u8", torch.float64: "f64",
       torch.int8: "i8", torch.bool: "bool", torch.float16: "f16"}
_PROTOS = {}


def _protos():
    if not _PROTOS:
        _PROTOS.update(abi.prototypes())
    return _PROTOS


class _Resolver:
    def __init__(self, named, calls, extra=()):
        """named: [(symbol, tensor)] planes and inputs; extra: tensors that may be reached by address only"""
        self.named = [(nm, t.data_ptr(), t.numel() * t.element_size(), t.element_size()) for nm, t in named if t is not None and t.numel()]
        self.allocs = {}        # storage address -> [nbytes, dtype, number or None]
        self.count = 0
        for _, args in calls:
            for a in args:
                if isinstance(a, torch.Tensor):
                    self._note(a)
        for t in extra:
            self._note(t)

    def _note(self, t):
        st = t.untyped_storage()
        self.allocs.setdefault(st.data_ptr(), [st.nbytes(), t.dtype, None])

    def addr(self, p, what):
        for nm, base, nbytes, esz in self.named:
            if base <= p < base + nbytes:
                if (p - base) % esz:
                    raise TraceError(f"{what}: pointer into {nm} off its element grid")
                return f"{nm}+{(p - base) // esz}"
        for base, rec in self.allocs.items():
            if base <= p < base + max(rec[0], 1):
                if rec[2] is None:
                    rec[2] = self.count
                    self.count += 1
                esz = torch.empty(0, dtype=rec[1]).element_size()
                if (p - base) % esz:
                    raise TraceError(f"{what}: pointer off the element grid of its allocation")
                return f"#{rec[2]}:{_DT[rec[1]]}:{rec[0] // esz}+{(p - base) // esz}"
        raise TraceError(f"{what}: pointer {p:#x} resolves to no known allocation")

    def pointer(self, a, what):
        if a is None:
            return "None"
        if isinstance(a, torch.Tensor):
            return self.addr(a.data_ptr(), what)
        if isinstance(a, int):
            return self.addr(a, what)
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:              # the pointer tables of gru_fwd / gru_bwd, entry by entry
                return "[" + ", ".join("None" if v is None else self.addr(v, what) for v in a) + "]"
            return "[" + ", ".join(repr(v) for v in a) + "]"
        obj = getattr(a, "_obj", None)              # ctypes.byref(HeadPtrs)
        if isinstance(obj, L.HeadPtrs):
            return "{" + ", ".join(f"{f}=" + ("None" if getattr(obj, f) is None else self.addr(getattr(obj, f), f"{what}.{f}"))
                                   for f in L.HEAD_FIELDS) + "}"
        raise TraceError(f"{what}: cannot write a pointer argument of type {type(a).__name__}")


def canonical(calls, named, extra=()):
    """-> one canonical line per call"""
    protos, res, lines = _protos(), _Resolver(named, calls, extra), []
    for idx, (name, args) in enumerate(calls):
        if name not in protos:
            raise TraceError(f"call {idx}: {name} is not declared in include/mmrca.h")
        params = protos[name][1]
        if len(params) != len(args):
            raise TraceError(f"call {idx}: {name} takes {len(params)} arguments, got {len(args)}")
        out = []
        for (ctype, pname), a in zip(params, args):
            what = f"call {idx} {name}({pname})"
            if ctype is C.c_void_p and pname != "stream":
                out.append(res.pointer(a, what))
            elif isinstance(a, (torch.Tensor, C.Array)):
                raise TraceError(f"{what}: a {type(a).__name__} where the header declares a scalar")
            elif isinstance(a, (bool, int, float)):
                out.append(repr(a))
            else:                                   # numpy / torch scalars would print differently from one version to the next
                raise TraceError(f"{what}: scalar of type {type(a).__name__}; the wrappers pass Python numbers")
        lines.append(f"{name}({', '.join(out)})")
    return lines


def digest(line):
    return hashlib.sha1(line.encode()).hexdigest()[:DIGEST_HEX]


def entry(line):
    """what the fixture stores of one call: the entry point without its prefix, and a short digest of the whole canonical line"""
    return line.split("(", 1)[0][len("mmrca_"):] + " " + digest(line)


# ------------------------------------------------------------------------------------------------ configurations
B, T, LIVE = 2, 32, 20
TINY_BLIP2 = dict(v_dim=64, v_heads=2, v_layers=2, v_mlp=128, image_size=56, q_dim=48, q_heads=2, q_layers=3, q_mlp=96, n_query=4, cross_freq=2)


def _text_inputs():
    ids = (5 + torch.arange(B * T, dtype=torch.int64) % 89).view(B, T)
    mask = torch.ones(B, T, dtype=torch.int64)
    mask[1, LIVE:] = 0
    return ids, mask


def _flat(v):
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, (tuple, list)):
        for x in v:
            yield from _flat(x)
    elif isinstance(v, dict):
        for x in v.values():
            yield from _flat(x)


def _main(make, size=224, pack=False, fwd=None, bwd=None, backward=True, cls_tail=True, images=True):
    """a configuration of the arena engines: make() -> engine; fwd / bwd: keyword arguments of forward / backward"""
    def run(mp, rec):
        mp.setattr(E, "CLS_TAIL", cls_tail)
        eng = make()
        ids, mask = _text_inputs()
        img = torch.zeros(B, 3, size, size) if images else None
        kw = dict(fwd or {})
        if pack:
            kw["text_pack"] = E.make_text_pack(mask, "cpu")
            assert kw["text_pack"] is not None
        del rec.calls[:]
        logits = eng.forward(ids, mask, img, **kw)
        dl = torch.zeros(B, logits.shape[1])
        if backward:
            eng.backward(dl, **(bwd or {}))
        a = eng.arena
        named = [("p", a.p), ("g", a.g), ("lp", a.lp), ("lp_lo", a.lp_lo), ("ids", ids), ("mask", mask), ("images", img), ("dlogits", dl)]
        extra = list(_flat(eng._bufs)) + (list(_flat(eng.conv._bufs)) if getattr(eng, "conv", None) is not None else [])
        return canonical(rec.calls, named, extra)
    return run


def _blip2(dtype, training, **ctor):
    def run(mp, rec):
        eng = QF.Blip2QFormerEngine(QF.Blip2Spec(**TINY_BLIP2), dtype=dtype, device="cpu", **ctor)
        eng.init_parameters(0)
        eng.train(training)
        px = torch.zeros(3, 3, 56, 56)
        del rec.calls[:]
        logits = eng.forward(px, drop_seed=5)
        dl = torch.zeros_like(logits)
        eng.backward(dl)
        named = [("store", eng.store.w), ("w_hi", eng.w_hi), ("w_lo", eng.w_lo), ("cls_p", eng.cls_p), ("cls_g", eng.cls_g),
                 ("cls_m", eng.cls_m), ("cls_v", eng.cls_v), ("images", px), ("dlogits", dl)]
        return canonical(rec.calls, named, list(_flat(eng._bufs)))
    return run


def _mmrca(text, image, dtype, **kw):
    return lambda: E.MMRCAEngine(text, image, 4, True, 0, dtype, "cpu", **kw)


def _configs():
    from garbage_classification_rca_amd.bimodal_engine import BimodalEngine
    from garbage_classification_rca_amd.classifier_engine import ClassifierEngine
    from garbage_classification_rca_amd.hierarchical_engine import HierarchicalEngine
    from garbage_classification_rca_amd.mobilebert_engine import MobileBertEngine
    drop = dict(drop_p=0.1, enc_drop_p=0.1, seed=3)
    c = {}
    for dt in ("bf16", "fp32", "bf16x3", "bf16x3f"):                                           # 1
        c[f"mmrca-distilbert-vitb16-{dt}"] = _main(_mmrca("distilbert", "transformer_B16", dt), fwd=drop)
    for dt in ("bf16", "bf16x3f"):
        for text in ("roberta", "bert"):                                                       # 2: position offset / token types, packed rows
            c[f"mmrca-{text}-vitb16-{dt}-packed"] = _main(_mmrca(text, "transformer_B16", dt), fwd=drop, pack=True)
        c[f"mmrca-distilbert-vitb16-{dt}-notail"] = _main(_mmrca("distilbert", "transformer_B16", dt), fwd=drop, cls_tail=False)        # 3
        c[f"mmrca-distilbert-vitb16-{dt}-eval"] = _main(_mmrca("distilbert", "transformer_B16", dt), fwd=dict(save=False), backward=False)   # 4
    c["mmrca-distilbert-vitb16-bf16-frozen-text"] = _main(_mmrca("distilbert", "transformer_B16", "bf16"), fwd=drop, bwd=dict(train_text=False))   # 5
    c["mmrca-distilbert-vitb16-bf16-frozen-image"] = _main(_mmrca("distilbert", "transformer_B16", "bf16"), fwd=drop, bwd=dict(train_image=False))
    c["hierarchical-distilbert-effv2m-bf16x3f"] = _main(lambda: HierarchicalEngine("distilbert", "eff_v2_medium", 4, "bf16x3f", "cpu", 448),          # 6
                                                        size=448, fwd=dict(bn_train=True, **drop))
    c["bimodal-distilbert-vitb16-bf16x3f"] = _main(lambda: BimodalEngine("distilbert", "transformer_B16", 4, "bf16x3f", "cpu", 224), fwd=drop)
    c["classifier-distilbert-bf16x3f"] = _main(lambda: ClassifierEngine("distilbert", 4, "bf16x3f", "cpu"), fwd=drop, images=False)
    c["classifier-vitb16-bf16x3f"] = _main(lambda: ClassifierEngine("transformer_B16", 4, "bf16x3f", "cpu"), fwd=drop)
    c["mobilebert-fp32"] = _main(lambda: MobileBertEngine(4, "fp32", "cpu"), fwd=drop, images=False)
    c["mmrca-bert-shufflenet-bf16-bn-train"] = _main(_mmrca("bert", "shuffle_net", "bf16", image_size=32), size=32, fwd=dict(bn_train=True, **drop))
    for dt in ("bf16", "fp32", "bf16x3f"):                                                     # 7
        for training in (False, True):
            c[f"blip2-tiny-{dt}-{'train' if training else 'eval'}"] = _blip2(dt, training)
    c["blip2-tiny-bf16x3f-eval-gemm-ref"] = _blip2("bf16x3f", False, gemm_impl=L.IMPL_REF)
    return c


CONFIGS = _configs()


def trace(name, mp):
    """canonical lines of configuration `name`, recorded under the patches of `mp`"""
    rec = install(mp)
    with torch.no_grad():
        return CONFIGS[name](mp, rec)
