"""Host-side logic on CPU: CLI, dataset, training-loop semantics, sharding, gradient sync (gloo, world_size 2), and
that the C-ABI library loads and exports every symbol include/mmrca.h declares.  No GPU compute here."""
import ast
import ctypes
import json
import os
import re
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")

from garbage_classification_rca_amd import lib as L                                   # noqa: E402
from garbage_classification_rca_amd import spec as S                                  # noqa: E402
from garbage_classification_rca_amd.options import args_parser                        # noqa: E402
from garbage_classification_rca_amd import CustomImageTextFolder as DS                # noqa: E402
from garbage_classification_rca_amd import distributed as D                           # noqa: E402
from garbage_classification_rca_amd.training import run_one_epoch, get_class_weights_from_counts, calculate_set_accuracy, mode_config_dict  # noqa: E402


# ------------------------------------------------------------------------------------------------ C ABI
def test_library_builds_loads_and_exports_every_declared_symbol():
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    lib = ctypes.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "mmrca.h")).read()
    declared = set(re.findall(r"\b(mmrca_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mmrca.h but not exported"
    bound = L.load()
    for name in declared:
        assert getattr(bound, name).argtypes is not None, f"{name} declared in include/mmrca.h but not typed by lib.load()"
    assert bound.mmrca_version() >= 1


def test_oracle_architecture_tables_are_independent_and_agree_with_transformers_and_the_product():
    """The oracle builds its modules from oracle/arch.py (restated from the third-party sources, cross-checked against the
    installed transformers classes key by key), never from the product's spec.py; the product's tables must say the same."""
    from oracle import arch as A
    from garbage_classification_rca_amd import spec as S
    src = open(os.path.join(ROOT, "oracle", "model.py")).read() + open(os.path.join(ROOT, "oracle", "arch.py")).read()
    assert not re.search(r"^\s*(from|import)\s+garbage_classification_rca_amd", src, re.M)       # no import of the product package
    seen = A.verify_against_transformers()
    assert seen["distilbert"] > 90 and seen["bert"] > 190 and seen["roberta"] > 190
    for name in A.TEXT_SPECS:
        assert dict(S.text_params(S.TEXT_SPECS[name])) == dict(A.text_params(A.TEXT_SPECS[name])), name
        a, b = A.TEXT_SPECS[name], S.TEXT_SPECS[name]
        assert (a.vocab, a.max_pos, a.dim, a.heads, a.ffn, a.layers, a.type_vocab, a.pad_id, a.pos_offset, a.ln_eps) == \
               (b.vocab, b.max_pos, b.dim, b.heads, b.ffn, b.layers, b.type_vocab, b.pad_id, b.pos_offset, b.ln_eps)
        for i in range(a.layers):
            assert A.text_layer_keys(a, i) == S.text_layer_keys(b, i)
    for name in A.VISION_SPECS:
        assert dict(S.vision_params(S.VISION_SPECS[name])) == dict(A.vision_params(A.VISION_SPECS[name])), name
    assert (A.NUM_PATCHES, A.SA_HID, A.SA_OUT, A.CA_HID, A.CA_OUT) == (S.NUM_PATCHES, S.SA_HID, S.SA_OUT, S.CA_HID, S.CA_OUT)


def test_product_path_fails_loudly_without_gpu_tensors():
    L.load()
    a = torch.zeros(4, 4)
    with pytest.raises(L.MmrcaError):
        L.gemm(a, a, a, M=4, N=4, K=4, lda=4, ldb=4, ldc=4, dtype=L.F32)
    with pytest.raises(L.MmrcaError):
        L.add_layernorm_fwd(a, None, a, a, None, a, None, None, 4, 4, 4, 4, 1e-5, L.F32)
    if not torch.cuda.is_available():
        from garbage_classification_rca_amd.engine import MMRCAEngine
        with pytest.raises(Exception):
            MMRCAEngine("distilbert", "transformer_B16")        # no device, no fallback


def test_no_product_module_imports_the_oracle():
    pkg = os.path.join(ROOT, "garbage_classification_rca_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            tree = ast.parse(open(os.path.join(pkg, fn)).read())
            for node in ast.walk(tree):
                names = []
                if isinstance(node, ast.Import):
                    names = [a.name for a in node.names]
                elif isinstance(node, ast.ImportFrom):
                    names = [node.module or ""]
                assert not any(n == "oracle" or n.startswith("oracle.") for n in names), fn


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_defaults_match_reference_parser():
    gold = json.load(open(os.path.join(G, "options_goldens.json")))
    mine = vars(args_parser([]))
    for k, v in gold["defaults"].items():
        assert k in mine, k
        assert mine[k] == v, (k, mine[k], v)
    ex = vars(args_parser(["--late_fusion=MM_RCA", "--reverse", "--no-tl", "--features_only", "--acc_steps", "3"]))
    for k, v in gold["example"].items():
        assert ex[k] == v
    extra = set(mine) - set(gold["defaults"])
    assert extra == {"tokens_max_len", "dtype", "synthetic", "num_workers", "seed", "image_size", "gpu_preprocess", "blip2_checkpoint", "hip_graph"}     # additive flags only
    # the reference's launch line (slurm_files/multimodal/MM_RCA.sh:15-30) must compute within the 1e-3 bound: the default compute
    # mode is the fastest one that does (bf16 is opt-in)
    assert mine["dtype"] == "bf16x3f"


def test_facade_defaults_are_the_references_model():
    """``MM_RCA`` called with the reference's ten positionals (main_both.py:306-317) must build what the
    reference builds -- EfficientNetV2-M (multimodal_model.py:113-126, 188) -- in a mode inside the tolerance; the additive
    keyword arguments may not change that.  (The construction itself needs HBM: tests/test_conv_gpu.py makes the call.)"""
    import inspect
    from garbage_classification_rca_amd.multimodal_model import MM_RCA, EffV2MediumAndDistilbertGated
    sig = inspect.signature(MM_RCA.__init__)
    names = list(sig.parameters)[1:]
    assert names[:10] == ["n_classes", "drop_ratio", "image_or_text_dropout_chance", "img_prob_dropout", "num_neurons_fc",
                          "text_model_name", "batch_size", "reverse", "features_only", "cross_attention_only"]
    assert all(sig.parameters[n].default is inspect.Parameter.empty for n in names[:10])          # :158-168: all required
    assert all(sig.parameters[n].default is not inspect.Parameter.empty for n in names[10:])      # additive ones all optional
    assert sig.parameters["image_model_name"].default == "eff_v2_medium"
    assert sig.parameters["dtype"].default == "bf16x3f"
    assert sig.parameters["image_size"].default is None             # -> 480 for EfficientNetV2-M (:407-408)
    assert issubclass(MM_RCA, EffV2MediumAndDistilbertGated)
    fwd = list(inspect.signature(MM_RCA.forward).parameters)[1:]
    assert fwd == ["_input_ids", "_attention_mask", "_images", "eval", "remove_image", "remove_text"]       # :638-644


# ------------------------------------------------------------------------------------------------ dataset
def _golden_lines():
    out = {}
    for ln in open(os.path.join(G, "dataset_goldens.txt")).read().splitlines():
        parts = ln.split("\t")
        out.setdefault(parts[0], []).append(parts[1:])
    return out


def _make_tree(td):
    from PIL import Image
    files = {"Black": ["chip_bag_12.png", "styrofoam cup.jpg", "notes.txt"], "Blue": ["Pizza_Box_3.png"],
             "Green": ["banana-peel_001.jpeg", "sub/coffee_grounds.png"], "TTR": ["AA batteries_7.bmp"]}
    for c, fs in files.items():
        for f in fs:
            p = os.path.join(td, c, f)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            if f.endswith(".txt"):
                open(p, "w").write("x")
            else:
                Image.new("RGB", (5, 4), (10, 20, 30)).save(p)
    csvp = os.path.join(td, "desc.csv")
    open(csvp, "w").write("filename,description\nBlack/chip_bag_12.png,an empty bag of chips\nsub/coffee_grounds.png,used coffee grounds\n")
    return csvp


def test_pre_process_text_known_answers():
    for src, want in _golden_lines()["KAT"]:
        assert repr(DS.pre_process_text(ast.literal_eval(src))) == want


def test_dataset_listing_matches_reference():
    gold = _golden_lines()
    with tempfile.TemporaryDirectory() as td:
        csvp = _make_tree(td)
        d = DS.CustomImageTextFolder(td)
        assert repr(d.classes) == gold["CLASSES"][0][0]
        assert repr(d.targets) == gold["TARGETS"][0][0]
        assert repr([len(x) for x in d.per_class]) == gold["PER_CLASS"][0][0]
        assert len(d) == int(gold["LEN"][0][0]) and d.imgs is d.samples
        for (s, t), g in zip(d.samples, gold["SAMPLE"]):
            assert [os.path.relpath(s["image"], td), repr(s["text"]), repr(s["long_text"]), str(t)] == g
        item, tgt = d[0]
        assert [repr(sorted(item.keys())), repr(sorted(item["image"].keys())), repr(sorted(item["text"].keys())), str(tgt)] == gold["ITEM0"][0]
        d2 = DS.CustomImageTextFolder(td, extended_desc=csvp)
        for (s, t), g in zip(d2.samples, gold["SAMPLE_EXT"]):
            assert [os.path.relpath(s["image"], td), repr(s["long_text"])] == g
        assert repr(d2[0][0]["text"]["original_text"]) == gold["ITEM0_EXT"][0][0]
        # tokenised items and collation
        from garbage_classification_rca_amd.multimodal_model import HashingTokenizer
        d3 = DS.CustomImageTextFolder(td, tokens_max_len=12, tokenizer_text=HashingTokenizer(),
                                      transform=lambda im: torch.zeros(3, 8, 8))
        batch, labels = next(iter(torch.utils.data.DataLoader(d3, batch_size=3)))
        assert batch["text"]["tokens"].shape == (3, 12) and batch["text"]["tokens"].dtype == torch.int64
        assert batch["text"]["attention_mask"].sum(1).tolist() == [4, 4, 4]      # [CLS] w w [SEP]
        assert batch["image"]["raw_image"].shape == (3, 3, 8, 8) and labels.tolist() == [0, 0, 1]
        ids, mask = d3.get_tokens("pizza box")
        assert ids[0] == 101 and ids[3] == 102 and mask.sum() == 4


def test_dataset_errors_like_reference():
    with tempfile.TemporaryDirectory() as td:
        with pytest.raises(FileNotFoundError):
            DS.CustomImageTextFolder(td)                      # no class folders
        os.makedirs(os.path.join(td, "Black"))
        with pytest.raises(FileNotFoundError):
            DS.CustomImageTextFolder(td)                      # class without a valid file


def test_class_weights_and_synthetic_dataset():
    assert get_class_weights_from_counts([2, 1, 2, 1]) == [6 / 8, 6 / 4, 6 / 8, 6 / 4]
    ds = DS.SyntheticImageTextDataset(10, 32, 16)
    item, t = ds[3]
    assert item["image"]["raw_image"].shape == (3, 32, 32) and t == 3
    assert item["text"]["tokens"][0] == 101 and int(item["text"]["attention_mask"].sum()) >= 8
    assert torch.equal(ds[3][0]["image"]["raw_image"], item["image"]["raw_image"])


# ------------------------------------------------------------------------------------------------ training loop
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(6, 4)

    def forward(self, _input_ids, _attention_mask, _images, eval=False, remove_image=False, remove_text=False):
        x = _images.flatten(1)[:, :6]
        if remove_image:
            x = torch.zeros_like(x)
        return self.fc(x)


def _loader(n, bs):
    g = torch.Generator().manual_seed(0)
    xs, ys = torch.randn(n, 3, 2, 1, generator=g), torch.arange(n) % 4
    items = [({"image": {"raw_image": xs[i], "image_path": str(i)},
               "text": {"original_text": "", "tokens": torch.zeros(4, dtype=torch.int64), "attention_mask": torch.ones(4, dtype=torch.int64)}}, int(ys[i]))
             for i in range(n)]
    return torch.utils.data.DataLoader(items, batch_size=bs), xs, ys


def test_trim_caption_columns_keeps_every_live_token():
    """graphed steps run padded rows: the dataset's 512-column captions (CustomImageTextFolder.py:305-333, padding='max_length') are cut to
    the columns the batch uses, rounded up to 16; nothing live is dropped, short or empty batches keep at least one block"""
    from garbage_classification_rca_amd.training import trim_caption_columns
    tok = torch.arange(4 * 512).view(4, 512)
    mask = torch.zeros(4, 512, dtype=torch.int64)
    for b, n in enumerate((7, 19, 1, 12)):
        mask[b, :n] = 1
    t, m = trim_caption_columns(tok, mask)
    assert t.shape == m.shape == (4, 32) and torch.equal(t, tok[:, :32]) and int(m.sum()) == int(mask.sum()) and t.is_contiguous()
    mask[1, 19:] = 0; mask[1, :16] = 1; mask[1, 16:] = 0
    assert trim_caption_columns(tok, mask)[0].shape == (4, 16)
    assert trim_caption_columns(tok, torch.zeros_like(mask))[0].shape == (4, 16)            # a caption batch zeroed by modality dropout
    full = torch.ones(4, 512, dtype=torch.int64)
    t, m = trim_caption_columns(tok, full)
    assert t is tok and m is full                                                              # nothing to trim: the inputs themselves
    assert trim_caption_columns(tok[:, :10], mask[:, :10])[0].shape == (4, 10)                # already shorter than a block


@pytest.mark.parametrize("acc_steps", [0, 2, 3])
def test_run_one_epoch_accumulation_semantics(acc_steps):
    """Gradients of the micro-batches are SUMMED (backward before the /acc_steps), the step happens every acc_steps
    batches or on the last one; the logged loss is scaled (main_both.py:112-124)."""
    torch.manual_seed(0)
    m, ref = _Tiny(), _Tiny()
    ref.load_state_dict(m.state_dict())
    dl, xs, ys = _loader(10, 2)          # 5 batches
    opt = torch.optim.SGD(m.parameters(), lr=0.1, weight_decay=0.01)
    nb, losses = run_one_epoch(0, m, dl, 10, "cpu", 2, opt, [1, 1, 1, 1], False, acc_steps, 0.1, verbose=False)
    assert nb == 5 and len(losses) == 5
    ropt = torch.optim.SGD(ref.parameters(), lr=0.1, weight_decay=0.01)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    logged = []
    for b in range(5):
        out = ref(None, None, xs[2 * b:2 * b + 2])
        loss = crit(out, ys[2 * b:2 * b + 2])
        loss.backward()
        step = True if acc_steps == 0 else ((b + 1) % acc_steps == 0 or b == 4)
        logged.append(loss.item() / (acc_steps if acc_steps else 1))
        if step:
            ropt.step(); ropt.zero_grad()
    for a, b in zip(m.parameters(), ref.parameters()):
        assert torch.allclose(a, b, atol=1e-6)
    assert np.allclose([float(l) for l in losses], logged, atol=1e-6)


def test_run_one_epoch_class_weights_and_accuracy():
    torch.manual_seed(1)
    m = _Tiny()
    dl, xs, ys = _loader(8, 4)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    _, losses = run_one_epoch(0, m, dl, 8, "cpu", 4, opt, [0.5, 2.0, 1.0, 1.5], True, 0, 0.0, verbose=False)
    want = torch.nn.CrossEntropyLoss(weight=torch.tensor([0.5, 2.0, 1.0, 1.5]))(m(None, None, xs[:4]), ys[:4])
    assert abs(float(losses[0]) - want.item()) < 1e-6
    acc, rep = calculate_set_accuracy(m, dl, 8, "cpu", 4, mode_config_dict["both"], True, verbose=False)
    pred = m(None, None, xs).argmax(1)
    assert abs(acc - 100.0 * float((pred == ys).float().mean())) < 1e-9
    acc0, _ = calculate_set_accuracy(m, dl, 8, "cpu", 4, mode_config_dict["text_only"], True, verbose=False)
    assert 0.0 <= acc0 <= 100.0


# ------------------------------------------------------------------------------------------------ sharding + gradient sync
def test_sharded_sampler_partitions_every_index_once():
    for n, world in [(10, 2), (17, 4), (8, 8), (5, 8)]:
        seen = []
        for r in range(world):
            s = D.ShardedSampler(n, r, world, shuffle=True, seed=3)
            s.set_epoch(2)
            idx = s.indices()
            assert len(idx) == len(s) == -(-n // world)
            seen += idx
        assert set(seen) == set(range(n))                     # every sample visited
        assert len(seen) - n < world                          # padding only to equalise ranks
    a, b = D.ShardedSampler(10, 0, 2, seed=1), D.ShardedSampler(10, 0, 2, seed=1)
    a.set_epoch(0); b.set_epoch(1)
    assert a.indices() != b.indices()


def _ddp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    r, _, w = D.init_from_env("gloo")
    torch.manual_seed(0)
    W = torch.randn(4, 6)
    X, Y = torch.randn(8, 6), torch.arange(8) % 4
    sampler = D.ShardedSampler(8, r, w, shuffle=False)
    idx = sampler.indices()
    Wp = W.clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(X[idx] @ Wp.t(), Y[idx]).backward()
    flat = torch.zeros(64)
    flat[8:32] = Wp.grad.flatten()
    flat[40:44] = float(r + 1)
    sync = D.GradSync(flat, w, bucket_bytes=64)
    # spans become ready from high to low addresses, as during backward; adjacent ones merge into one all-reduce
    sync.span_ready(40, 64)
    sync.span_ready(32, 40)
    sync.span_ready(0, 32, flush=True)
    sync.finish()
    # (plain numpy through the queue: a torch tensor travels as a file descriptor the parent must fetch from THIS process while it is
    # still alive -- a race that showed up as ConnectionResetError in the parent)
    q.put((r, flat.float().numpy().copy(), len(sync.pending), sync.bytes_reduced))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    """a TCP port nobody is listening on right now (a pid-derived constant collided with a lingering rendezvous once)"""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


_RENDEZVOUS_ERRORS = ("address already in use", "eaddrinuse", "errno 98", "rendezvous", "connection refused", "failed to connect",
                      "the server socket has failed", "could not connect", "connection reset by peer")


def _guarded_rank(worker, rank, world, port, q):
    """runs in the spawned process: a failure travels to the parent as text, so that it can tell a rendezvous problem (retry on a
    fresh port) from a real failure of the code under test (no retry)"""
    try:
        worker(rank, world, port, q)
    except BaseException as e:          # noqa: BLE001 -- reported, then re-raised
        import traceback
        q.put(("__error__", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


def _run_world2(worker, attempts=3):
    """start two spawned ranks of `worker(rank, world, port, queue)` and collect their two results.  ONLY a rendezvous that does not
    come up (the probed port was taken in the meantime: address-in-use / connection errors from the store) is retried, on a fresh
    port; any other exception, a non-zero exit without such a message, or a timeout fails the test at once -- an intermittent
    failure of the code under test (stream ordering, bucket merging in GradSync) must not be retried away."""
    import queue as _queue
    import torch.multiprocessing as mp
    last = None
    for _ in range(attempts):
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_guarded_rank, args=(worker, r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res, errors = [], []
        try:
            while len(res) + len(errors) < 2:
                item = q.get(timeout=120)
                (errors if isinstance(item, tuple) and len(item) == 3 and item[0] == "__error__" else res).append(item)
        except _queue.Empty:
            for p in procs:
                if p.is_alive():
                    p.terminate()
                p.join(10)
            if not errors:
                raise AssertionError(f"world-2 workers timed out (exit codes {[p.exitcode for p in procs]}): not retried")
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.terminate()
                p.join(10)
        if not errors and all(p.exitcode == 0 for p in procs):
            return res
        text = "\n".join(e[2] for e in errors)
        if errors and any(pat in text.lower() for pat in _RENDEZVOUS_ERRORS):
            last = text
            continue                    # the only retried case
        raise AssertionError(f"world-2 worker failed (exit codes {[p.exitcode for p in procs]}), not a rendezvous error, not retried:\n{text}")
    raise AssertionError(f"world-2 rendezvous did not come up in {attempts} attempts: {last}")


def _always_fails_worker(rank, world, port, q):
    raise ValueError("a real failure of the code under test")


def test_run_world2_does_not_retry_a_real_failure():
    import time
    t0 = time.time()
    with pytest.raises(AssertionError, match="not a rendezvous error"):
        _run_world2(_always_fails_worker)
    assert time.time() - t0 < 100      # one attempt, not three


def test_gradient_sync_world2_equals_full_batch_gradient():
    res = sorted(_run_world2(_ddp_worker), key=lambda t: t[0])
    torch.manual_seed(0)
    W = torch.randn(4, 6)
    X, Y = torch.randn(8, 6), torch.arange(8) % 4
    Wp = W.clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(X @ Wp.t(), Y).backward()        # gradient of the mean loss over the global batch
    for r, flat, pending, nbytes in res:
        flat = torch.from_numpy(flat)
        assert torch.allclose(flat[8:32], Wp.grad.flatten(), atol=1e-6)
        assert torch.allclose(flat[40:44], torch.full((4,), 1.5))
        assert pending == 0 and nbytes == 64 * 4


# ------------------------------------------------------------------------------------------------ inventories
def test_parameter_inventories():
    used = S.head_used_params(1280, 768, 4, False, False)
    assert sum(int(np.prod(s)) for _, s in used) == 94820
    n_txt = sum(int(np.prod(s)) for _, s in S.text_params(S.TEXT_SPECS["distilbert"]))
    assert n_txt == 66362880                                               # DistilBertModel parameters
    n_vit = sum(int(np.prod(s)) for _, s in S.vision_params(S.VISION_SPECS["transformer_B16"]))
    assert n_vit == 85798656                                               # vit_b_16 without the classification head
    keys = [k for k, _ in S.head_unused_params(1280, 768, 4, 256, 16, False, False)]
    for k in ("clip_fc_layer.weight", "logit_scale", "gru_text.weight_ih_l0", "fusion.kernel1", "classifier.bias", "final.weight"):
        assert k in keys


def test_test_split_evaluator_logic_on_cpu():
    """calculate_test_accuracy (reference calculate_test_accuracy_both.py:52-117) with a stand-in model: accuracy,
    confusion matrix, sklearn report, CSV / image file names."""
    from garbage_classification_rca_amd import calculate_test_accuracy_both as E
    m = _Tiny()
    dl, xs, ys = _loader(12, 4)
    acc, report, rd, cm = E.calculate_test_accuracy(m, dl, 12, "cpu", 4, mode_config_dict["both"], True, verbose=False)
    pred = m(None, None, xs).argmax(1)
    assert abs(acc - 100.0 * int((pred == ys).sum()) / 12) < 1e-9
    assert cm.shape == (4, 4) and cm.sum() == 12 and int(np.trace(cm)) == int((pred == ys).sum())
    assert set(rd.keys()) >= {"Black", "Blue", "Green", "TTR", "accuracy"}
    with tempfile.TemporaryDirectory() as td:
        csvp, pngp = E.generate_report_and_image(rd, acc, cm, "always_both", out_dir=td)
        assert os.path.basename(csvp) == "multimodal_model_report_test_set_acc_{:.2f}_always_both.csv".format(acc)
        assert os.path.exists(csvp)


def test_make_text_pack_layout_and_fallbacks():
    """engine.make_text_pack: live tokens back to back, total rounded up to 64 with padding rows of captions that have
    room, class-token rows first in each caption; None when packing does not apply."""
    from garbage_classification_rca_amd.engine import make_text_pack
    B, T = 8, 32
    lens = np.array([32, 5, 17, 1, 32, 9, 20, 3])
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.int64)
    p = make_text_pack(mask, "cpu")
    assert p is not None and p.M == 128 and p.M % 64 == 0 and p.M >= lens.sum()
    cu, perm, km, first = p.cu.numpy(), p.perm.numpy(), p.mask.numpy(), p.first.numpy()
    assert cu[0] == 0 and cu[-1] == p.M and (np.diff(cu) >= lens).all() and (np.diff(cu) <= T).all()
    assert (first == cu[:-1]).all() and (perm[first] == np.arange(B) * T).all()
    for b in range(B):
        rows = perm[cu[b]:cu[b + 1]]
        assert (rows == b * T + np.arange(len(rows))).all()              # a prefix of caption b, in order
        assert km[cu[b]:cu[b + 1]].sum() == lens[b]                      # the padding rows taken in are masked keys
    assert km.sum() == lens.sum()
    assert make_text_pack(torch.from_numpy(mask), "cpu").M == p.M       # tensors work too
    holes = mask.copy(); holes[2, 3] = 0
    assert make_text_pack(holes, "cpu") is None                           # not a prefix mask
    dropped = mask.copy(); dropped[4] = 0
    assert make_text_pack(dropped, "cpu") is None                         # a caption zeroed by modality dropout
    assert make_text_pack(mask[:3, :24], "cpu") is None                   # B*T not a multiple of 64
    full = np.ones((2, 32), dtype=np.int64)
    assert make_text_pack(full, "cpu").M == 64                            # nothing to skip: identity layout


# ------------------------------------------------------------------------------------------------ a4 / a5 goldens
def test_state_dict_layout_equals_the_reference_constructor():
    """a4: key -> shape of the reference's ``MM_RCA(...).state_dict()`` (multimodal_model.py:158-328), dumped by
    tests/golden/make_goldens.py from the reference class for 2 text models x 4 flag combinations, against the product's
    parameter inventories (what the module facade registers).  image_model.* is excluded there (torchvision absent)."""
    import json
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_layout.json")))
    assert len(d) == 8
    for cfg, ref in d.items():
        text, fo, cao, bs, fc = cfg.split("|")
        fo, cao = bool(int(fo.split("=")[1])), bool(int(cao.split("=")[1]))
        bs, fc = int(bs.split("=")[1]), int(fc.split("=")[1])
        mine = {"text_model." + k: list(s) for k, s in S.text_params(S.TEXT_SPECS[text])}
        used = S.head_used_params(1280, 768, 4, fo, cao)
        mine.update({k: list(s) for k, s in used})
        mine.update({k: list(s) for k, s in S.head_unused_params(1280, 768, 4, fc, bs, fo, cao) if k not in dict(used)})
        assert mine == ref, (cfg, sorted(set(mine) ^ set(ref))[:8], [k for k in mine if k in ref and mine[k] != ref[k]][:8])


def test_product_drop_modalities_follows_the_reference_truth_table():
    """a5: the PRODUCT's ``drop_modalities`` (not the oracle's copy) against the table recorded from the reference's
    method (multimodal_model.py:420-455): which inputs are zeroed, int64 ids stay int64, and how many draws of the
    global numpy RNG each call consumes."""
    import types
    from garbage_classification_rca_amd.multimodal_model import MM_RCA
    g = np.load(os.path.join(ROOT, "tests", "golden", "head_goldens.npz"))
    for row in g["dropmod_table"]:
        ev, ri, rt, p_any, p_img, seed, z_img, z_ids, z_mask, draws, _ = row
        m = types.SimpleNamespace(image_or_text_dropout_chance=p_any, img_dropout_prob=p_img,
                                  _images=torch.ones(3, 3, 4, 4), _input_ids=torch.full((3, 8), 7, dtype=torch.int64),
                                  _attention_mask=torch.ones(3, 8, dtype=torch.int64))
        np.random.seed(int(seed))
        MM_RCA.drop_modalities(m, bool(ev), bool(ri), bool(rt))
        assert float(m._images.abs().sum() == 0) == z_img, row
        assert float(m._input_ids.abs().sum() == 0) == z_ids and float(m._attention_mask.abs().sum() == 0) == z_mask, row
        assert m._input_ids.dtype == torch.int64
        nxt = np.random.rand()
        fresh = np.random.RandomState(int(seed)).rand(6)
        assert int(np.argmin(np.abs(fresh - nxt))) == int(draws), row


def test_conv_backbone_inventories_match_the_reference_counts_and_the_oracle_layout():
    """a7 / f3: the restated torchvision architectures carry exactly the parameter counts the reference quotes for its
    4-class classifiers (main_image.py:295 eff_v2_medium 52 863 480, :302 eff_v2_large 117 239 396), and the product's
    parameter / buffer inventory (names, shapes, order) is the oracle module tree's state_dict."""
    from oracle import conv_models as CM
    from garbage_classification_rca_amd.conv_engine import ConvEncoder
    want = {"eff_v2_medium": 52863480, "eff_v2_large": 117239396}
    for name in ("eff_v2_medium", "eff_v2_large", "shuffle_net"):
        orc = CM.build_conv_oracle(name)
        n = sum(p.numel() for p in orc.parameters())
        if name in want:
            assert n + 1280 * 4 + 4 == want[name]
        enc = ConvEncoder(name, owner=None)
        sd = orc.state_dict()
        pk = [k for k, _ in enc.param_entries()]
        assert pk == [k for k, _ in orc.named_parameters()], name
        assert all(tuple(sd[k].shape) == tuple(s) for k, s in enc.param_entries())
        bk = [k for k, _ in enc.buffer_entries()]
        assert bk == [k for k, _ in orc.named_buffers()], name
        assert sorted(pk + bk) == sorted(sd.keys())


# ------------------------------------------------------------------------------------------------ (e) readiness
def _ddp_worker2(rank, world, port, q):
    """GradSync under the engine's real call pattern: spans of TWO producers (vision layers and text layers) arrive
    interleaved, gradient accumulation syncs only on the stepping micro-batch, bf16 on the wire is optional."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for wire in (None, torch.bfloat16):
        flat = torch.zeros(96)
        sync = D.GradSync(flat, world, bucket_bytes=16 * 4, wire_dtype=wire)
        # micro-batch 1 of 2 (acc_steps = 2): accumulate only, nothing may be reduced
        flat += (rank + 1.0)
        sync.enabled = False
        for lo, hi in ((80, 96), (64, 80), (16, 32), (48, 64), (0, 16), (32, 48)):
            sync.span_ready(lo, hi)
        sync.finish()
        assert sync.bytes_reduced == 0 and torch.all(flat == rank + 1.0)
        # micro-batch 2: the stepping one.  Arena order: text [0,48) | vision [48,80) | head [80,96); the head finishes first,
        # then vision and text layers alternate (two streams), each descending within its own encoder
        flat += 10.0 * (rank + 1.0)
        sync.enabled = True
        for lo, hi in ((80, 96), (64, 80), (32, 48), (48, 64), (16, 32), (0, 16)):
            sync.span_ready(lo, hi, flush=(lo in (48, 0)))
        sync.finish()
        out["bf16" if wire else "fp32"] = (flat.float().numpy().copy(), sync.bytes_reduced)      # numpy: see _ddp_worker
    # evaluation counts: 10 samples over 2 ranks of 5, then 7 samples over 2 ranks (rank 1 draws one wrapped duplicate)
    s = D.ShardedSampler(7, rank, world, shuffle=False)
    out["num_real"] = (len(s), s.num_real, D.all_reduce_counts(s.num_real, s.num_real, "cpu"))
    out["seed"] = D.broadcast_seed(None)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_gradient_sync_two_producers_accumulation_and_bf16_wire_world2():
    res = dict(_run_world2(_ddp_worker2))
    want = torch.full((96,), (11.0 + 22.0) / 2)            # mean over the two ranks of the ACCUMULATED gradient
    for r in (0, 1):
        flat, nbytes = res[r]["fp32"]
        assert torch.equal(torch.from_numpy(flat), want) and nbytes == 96 * 4
        flat16, nbytes16 = res[r]["bf16"]
        assert torch.allclose(torch.from_numpy(flat16), want, rtol=1e-2) and nbytes16 == 96 * 2      # half the bytes on the wire
    assert res[0]["num_real"][:2] == (4, 4) and res[1]["num_real"][:2] == (4, 3)
    assert res[0]["num_real"][2] == (7, 7) and res[0]["seed"] == res[1]["seed"]


def test_train_augmentation_planning_matches_the_oracle_and_the_c_structs():
    """Host side of row f1's training path: the per-image descriptors (preprocess.py::plan_*) against the oracle's
    restatement of albumentations' geometry, the descriptor dtypes against the C structs, and the sampler's firing rates."""
    from oracle import transforms as T
    from garbage_classification_rca_amd import preprocess as P
    assert P.ROT_DTYPE.itemsize == 72 and P.AUG_DTYPE.itemsize == 160
    hdr = open(os.path.join(ROOT, "include", "mmrca.h")).read()
    for f in P.AUG_DTYPE.names:
        assert re.search(r"\b%s\b" % f, hdr), f
    rng = np.random.default_rng(3)
    for _ in range(50):
        h, w, ang = int(rng.integers(20, 500)), int(rng.integers(20, 500)), float(rng.uniform(-90, 90))
        inv, x_min, y_min, dh, dw = P.plan_rotation(h, w, ang)
        x0, x1, y0, y1 = T.rotated_rect_with_max_area(h, w, ang)
        assert (x_min, y_min, dh, dw) == (x0, y0, y1 - y0, x1 - x0)
        assert 0 <= x_min and x_min + dw <= w and 0 <= y_min and y_min + dh <= h
        j = np.mod(np.abs(rng.normal(0, 0.08, (4, 2))), 1.0)
        assert np.allclose(P.plan_perspective(h, w, j), T.perspective_matrix(h, w, j).reshape(9), rtol=2e-5, atol=1e-6)    # closed form vs the oracle's 8x8 solve
        a, l = float(rng.uniform(0.2, 0.5)), float(rng.uniform(0.5, 1.0))
        assert np.allclose(P.sharpen_kernel(a, l), T.sharpen_matrix(a, l).reshape(9), rtol=0, atol=1e-7)
        assert abs(P.sharpen_kernel(a, l).sum() - (1.0 - a + a * l)) < 1e-5     # (1 - alpha) * 1 + alpha * lightness
    # rotating by 0 keeps the whole image; the crop of a 45-degree rotation of a square is about 1/sqrt 2 of its side... /2
    assert P.plan_rotation(100, 100, 0.0)[1:] == (0, 0, 100, 100)
    _, _, _, dh, dw = P.plan_rotation(100, 100, 45.0)
    assert 68 <= dh <= 72 and dh == dw
    ps = P.sample_train_params(np.random.default_rng(0), 4000, 0.3)
    for key in ("angle", "blur_k", "bc", "sharpen", "persp", "scale"):
        rate = np.mean([p.get(key) is not None for p in ps])
        assert abs(rate - 0.3) < 0.03, (key, rate)
    assert abs(np.mean([p["flip_v"] for p in ps]) - 0.3) < 0.03
    angles = np.array([p["angle"] for p in ps if "angle" in p]); scales = np.array([p["scale"] for p in ps if "scale" in p])
    assert -90 <= angles.min() and angles.max() <= 90 and abs(angles.mean()) < 6
    assert 0.5 <= scales.min() and scales.max() <= 1.5 and abs(scales.mean() - 1.0) < 0.03
    assert set(p["blur_k"] for p in ps if "blur_k" in p) == {3, 5, 7}
    assert P.sample_train_params(np.random.default_rng(0), 10, 0.0) == [dict(flip_v=False, flip_h=False)] * 10


def test_oracle_train_pipeline_stage_properties():
    """Size-independent properties of the restated augmentations (no golden vectors exist for them: parity unpinned)."""
    from oracle import transforms as T
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (60, 44, 3), dtype=np.uint8)
    const = np.full((40, 50, 3), 93, dtype=np.uint8)
    assert np.array_equal(T.rotate_crop_u8(img, 0.0), img) and np.array_equal(T.scale_u8(img, 1.0), img)
    sq = rng.integers(0, 256, (48, 48, 3), dtype=np.uint8)
    x0, x1, y0, y1 = T.rotated_rect_with_max_area(48, 48, 90.0)
    assert x1 - x0 >= 47 and y1 - y0 >= 47
    assert np.array_equal(T.rotate_crop_u8(sq, 90.0), np.rot90(sq, 1)[y0:y1, x0:x1])      # +angle = counter-clockwise on the screen
    for k in (3, 5, 7):
        assert np.array_equal(T.gaussian_blur_u8(const, k), const) and abs(sum(T.BLUR_TAPS[k]) - 1.0) < 1e-12
    assert np.array_equal(T.sharpen_u8(const, 0.4, 1.0), const)                     # lightness 1: the weights sum to 1
    assert np.array_equal(T.brightness_contrast_u8(img, 1.0, 0.0), img)
    assert T.brightness_contrast_u8(img, 1.2, 0.2).min() >= 51 and T.brightness_contrast_u8(img, 0.8, -0.2).max() <= 153
    r = T.rotate_crop_u8(const, 37.0)
    assert r.size > 0 and np.all(r[1:-1, 1:-1] == 93)           # crop_border: at most the outermost ring blends with the border
    p = T.perspective_u8(const, np.full((4, 2), 0.08))
    assert np.all(p == 93)                                                          # the jittered quadrilateral lies inside
    z = T.scale_u8(const, 0.5)
    assert z[0, 0, 0] == 0 and z[20, 25, 0] == 93 and abs(int((z[..., 0] == 93).sum()) - 20 * 25) <= 50


# ------------------------------------------------------------------------------------------------ --balanced_sampler
def test_balanced_sampler_weights_draws_and_rank_striding():
    """main_both.py:478-526 -> imbalanced_sampler/imbalanced.py: weight_i = 1 / count[label_i], len(dataset) draws with
    replacement; under data parallelism the ranks' draws interleave to the single-process draw"""
    from garbage_classification_rca_amd.distributed import BalancedShardedSampler
    targets = [0] * 600 + [1] * 300 + [2] * 90 + [3] * 10
    s = BalancedShardedSampler(targets, 0, 1, seed=5)
    w = s.weights.numpy()
    assert np.allclose(w[0], 1 / 600) and np.allclose(w[650], 1 / 300) and np.allclose(w[995], 1 / 10) and len(s) == 1000
    idx = list(iter(s))
    assert len(idx) == 1000 and all(0 <= i < 1000 for i in idx)
    cls = np.bincount(np.asarray(targets)[idx], minlength=4)
    assert (np.abs(cls - 250) < 60).all(), cls                       # each class ~ a quarter of the draws (sigma ~ 14)
    assert len(set(i for i in idx if targets[i] == 3)) <= 10 and cls[3] > 150          # the rare class is drawn WITH replacement
    assert list(iter(s)) != idx                                        # the next pass re-draws
    # two ranks: same seed, same pass -> interleaved halves of one draw of ceil(n / 2) * 2
    a, b = BalancedShardedSampler(targets, 0, 2, seed=5), BalancedShardedSampler(targets, 1, 2, seed=5)
    one = BalancedShardedSampler(targets, 0, 1, seed=5)
    ia, ib, io = list(iter(a)), list(iter(b)), list(iter(one))
    assert len(ia) == len(ib) == 500 and [x for p in zip(ia, ib) for x in p] == io
    a.set_epoch(3); one.set_epoch(3)
    assert list(iter(a)) == list(iter(one))[0::2]
    assert len(BalancedShardedSampler([], 0, 1)) == 0 and list(iter(BalancedShardedSampler([], 0, 1))) == []


def _smt_two_socket_topology():
    """2 sockets x 32 cores x 2 threads as Linux numbers them: 0-31 socket 0, 32-63 socket 1, 64-95 the siblings of 0-31, 96-127 of 32-63"""
    return {c: ((c % 64) // 32, ((c % 64) // 32, c % 32)) for c in range(128)}


def test_rank_to_cpu_binding_slices_and_worker_cap(monkeypatch, tmp_path):
    """one process per GPU (replacing nn.DataParallel, main_both.py:386-388) with 16 loader workers each (:476-492) oversubscribes a
    node unless every rank keeps to its own cores.  ADVICE r5: the slices come from the TOPOLOGY (NUMA node of the rank's GPU, physical
    cores with their SMT siblings), not from the order of the CPU ids; an unreadable topology or an unknown LOCAL_WORLD_SIZE binds nothing."""
    topo = _smt_two_socket_topology()
    cpus = list(range(128))
    # GPU NUMA nodes known (0-3 on node 0, 4-7 on node 1): every rank on its GPU's socket, whole cores, disjoint, all CPUs used
    gn = [0, 0, 0, 0, 1, 1, 1, 1]
    sl = [D.cpu_slice(r, 8, cpus, topo, gn) for r in range(8)]
    assert sl[0] == list(range(0, 8)) + list(range(64, 72)) and sl[3] == list(range(24, 32)) + list(range(88, 96))
    assert sl[4] == list(range(32, 40)) + list(range(96, 104))
    assert all(len(x) == 16 for x in sl) and sorted(sum(sl, [])) == cpus
    for r in range(8):
        assert {topo[c][0] for c in sl[r]} == {gn[r]}                           # ranks 2, 3 stay on socket 0 (id-order eighths: socket 1)
        assert all((c + 64) % 128 in sl[r] for c in sl[r])                      # SMT siblings stay together
    # an odd wiring (GPUs alternate between the sockets) is followed, not assumed away
    alt = [D.cpu_slice(r, 4, cpus, topo, [0, 1, 0, 1]) for r in range(4)]
    assert alt[0] == list(range(0, 16)) + list(range(64, 80)) and alt[2] == list(range(16, 32)) + list(range(80, 96))
    assert {topo[c][0] for c in alt[1] + alt[3]} == {1}
    # GPU nodes unknown: equal runs of cores in (node, package, core) order
    un = [D.cpu_slice(r, 8, cpus, topo, None) for r in range(8)]
    assert un == sl
    # a restricted CPU set (container cpuset), fewer cores than ranks, one rank, no topology
    few = D.cpu_slice(1, 2, [4, 5, 6, 7, 68, 69, 70, 71], topo, None)
    assert few == [6, 7, 70, 71]
    assert D.cpu_slice(5, 8, [0, 1, 2], topo, None) == [2]                    # wrap, never empty
    assert D.cpu_slice(0, 1, cpus, topo, None) == cpus
    assert D.cpu_slice(0, 2, [0, 1, 500], topo, None) == []                   # a CPU the topology does not know: no slice, no binding
    assert D.cpu_slice(3, 8, cpus, topo, [0, 0, 0, 2, 1, 1, 1, 1]) == []      # GPU on a node with no allowed CPU
    # sysfs reader on a fabricated tree (node cpulists with ranges, per-cpu package / core ids); a missing file -> None
    for n, lst in ((0, "0-1,4-5"), (1, "2-3,6-7")):
        (tmp_path / "node" / f"node{n}").mkdir(parents=True)
        (tmp_path / "node" / f"node{n}" / "cpulist").write_text(lst + "\n")
    (tmp_path / "node" / "possible").write_text("0-1\n")
    for c in range(8):
        d = tmp_path / "cpu" / f"cpu{c}" / "topology"
        d.mkdir(parents=True)
        (d / "physical_package_id").write_text(f"{(c % 4) // 2}\n")
        (d / "core_id").write_text(f"{c % 2}\n")
    got = D.read_cpu_topology(range(8), str(tmp_path))
    assert got[0] == (0, (0, 0)) and got[5] == (0, (0, 1)) and got[6] == (1, (1, 0)) and len(got) == 8
    assert D.cpu_slice(1, 2, list(range(8)), got, None) == [2, 3, 6, 7]
    assert D.read_cpu_topology([0, 9], str(tmp_path)) is None
    assert D.gpu_numa_nodes(2, str(tmp_path)) is None                           # (no such PCI devices / no GPU here)
    before = os.sched_getaffinity(0)
    try:
        assert D.bind_rank_to_cpus(0, 1) is None               # one rank per node: untouched
        assert D.bind_rank_to_cpus(0, 0) is None               # LOCAL_WORLD_SIZE unset: untouched
        monkeypatch.setenv("MMRCA_CPU_BIND", "0")
        assert D.bind_rank_to_cpus(1, 2) is None and os.sched_getaffinity(0) == before
        monkeypatch.setenv("MMRCA_CPU_BIND", "1")
        want = D.cpu_slice(1, 2)
        if len(want) < D.MIN_CPUS_PER_RANK:
            assert D.bind_rank_to_cpus(1, 2) is None and os.sched_getaffinity(0) == before      # too few cores per rank: left alone
        else:
            got = D.bind_rank_to_cpus(1, 2)
            assert got == want and os.sched_getaffinity(0) == set(got) and set(got) < before
            assert not set(got) & set(D.cpu_slice(0, 2, sorted(before)))
            assert D.loader_workers(16) == max(1, min(16, len(got) - 1))
    finally:
        os.sched_setaffinity(0, before)
    assert D.loader_workers(0) == 0 and D.loader_workers(3) == max(1, min(3, len(before) - 1))


def _inflight_checker():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("check_inflight_regs", os.path.join(root, "tools", "check_inflight_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return root, mod


def test_inflight_register_checker_catches_what_it_is_for():
    """the checker itself, on hand-written ISA: a copy of an asm load's destination before the wait is flagged (global and LDS loads,
    counted waits, an SMEM load making lgkmcnt(N > 0) unordered), the same sequences with the wait in front are not, and loads the
    compiler emitted itself (outside #ASMSTART / #ASMEND) are not tracked"""
    _, mod = _inflight_checker()

    def run(body):
        text = "\t.type\tk,@function\nk:\n" + "\n".join("\t" + l for l in body) + "\n.Lfunc_end0:\n"
        n, res = mod.scan(text, "")
        assert n == 1
        return [r for r in res if r[0] != "loads"], sum(r[2] for r in res if r[0] == "loads")

    A, E = "#ASMSTART", "#ASMEND"
    bad, n = run([A, "global_load_dwordx4 v[10:13], v[2:3], off", E, "v_mov_b32_e32 v40, v11", A, "s_waitcnt vmcnt(0)", E])
    assert n == 1 and len(bad) == 1 and bad[0][3] == [("v", 11)]
    bad, _ = run([A, "global_load_dwordx4 v[10:13], v[2:3], off", E, A, "s_waitcnt vmcnt(0)", E, "v_mov_b32_e32 v40, v11"])
    assert not bad
    bad, _ = run(["global_load_dwordx4 v[10:13], v[2:3], off", "v_mov_b32_e32 v40, v11"])                # the compiler's own load
    assert not bad
    # counted vmcnt: two loads then a store; vmcnt(1) retires the two loads, vmcnt(2) only the first
    seq = [A, "global_load_dword v10, v[2:3], off", "global_load_dword v11, v[2:3], off", E, "global_store_dword v[4:5], v6, off"]
    bad, _ = run(seq + [A, "s_waitcnt vmcnt(1)", E, "v_add_f32_e32 v1, v10, v11"])
    assert not bad
    bad, _ = run(seq + [A, "s_waitcnt vmcnt(2)", E, "v_add_f32_e32 v1, v10, v11"])
    assert len(bad) == 1 and bad[0][3] == [("v", 11)]
    # LDS-DMA has no register destination; an overwritten destination counts as a touch
    bad, n = run([A, "global_load_lds_dwordx4 v[2:3], off", E, "v_mov_b32_e32 v2, v9"])
    assert not bad and n == 0
    bad, _ = run([A, "ds_read_b128 v[20:23], v5 offset:64", E, "v_mov_b32_e32 v22, 0", A, "s_waitcnt lgkmcnt(0)", E])
    assert len(bad) == 1
    # lgkmcnt(N > 0) is ordered only while no scalar load is outstanding
    two = [A, "ds_read_b32 v20, v5", "ds_read_b32 v21, v5", E]
    bad, _ = run(two + ["s_waitcnt lgkmcnt(1)", "v_mov_b32_e32 v1, v20"])
    assert not bad
    bad, _ = run(["s_load_dwordx2 s[0:1], s[4:5], 0x0"] + two + ["s_waitcnt lgkmcnt(1)", "v_mov_b32_e32 v1, v20"])
    assert len(bad) == 1
    bad, _ = run([A, "ds_read_b64_tr_b16 v[30:31], v5 offset:128", E, "v_accvgpr_write_b32 a3, v30"])       # a spill to an AGPR
    assert len(bad) == 1


def test_split_phase_asm_loads_are_not_touched_before_their_wait():
    """Every kernel that issues inline-asm loads whose destination registers the COMPILER picks and that are awaited by a later asm
    s_waitcnt: the attention backward's row constants (csrc/attention_mfma.hip, rc_issue / rc_finish) and every LDS fragment read of
    the GEMM, implicit-GEMM and attention main loops (csrc/lds_asm.h).  hipcc believes such an output is valid the moment the asm
    statement ends; under register pressure it may copy it before the wait -- seen once (round 4, GEMM side-operand experiment, DESIGN
    K2): right on a warm cache, garbage on a cold one.  This compiles every such file to gfx950 ISA (no GPU needed) and checks that
    nothing reads or writes an in-flight destination register in ANY of their kernels."""
    from concurrent.futures import ThreadPoolExecutor
    root, mod = _inflight_checker()
    files = {"attention_mfma.hip": 1000, "gemm256.hip": 1000, "gemm.hip": 100, "conv_igemm.hip": 50, "attention_cross.hip": 0, "attention_f32.hip": 0}
    csrc = os.path.join(root, "garbage_classification_rca_amd", "csrc")
    # (every file with inline asm is listed: a new one must be added here)
    with_asm = {f for f in os.listdir(csrc) if f.endswith(".hip") and ("asm volatile" in open(os.path.join(csrc, f)).read() or "lds_asm.h" in open(os.path.join(csrc, f)).read())}
    assert with_asm <= set(files), with_asm - set(files)
    with ThreadPoolExecutor(4) as ex:
        texts = dict(zip(files, ex.map(lambda f: mod.compile_to_asm(os.path.join(csrc, f)), files)))
    for f, text in texts.items():
        kernels, res = mod.scan(text, "")
        bad = [r for r in res if r[0] != "loads"]
        loads = sum(r[2] for r in res if r[0] == "loads")
        print(f, kernels, "kernels,", loads, "asm loads tracked")
        assert kernels > 0 and loads >= files[f], (f, kernels, loads)
        assert not bad, (f, bad[:5])
    # the one place where asm loads stay in flight ACROSS compiled code (the persistent attention backward's row constants): they land
    # in fixed registers above the range the kernel is compiled for (amdgpu_num_vgpr), so no compiler-emitted instruction may name one
    lines = texts["attention_mfma.hip"].split("\n")
    i = next(k for k, l in enumerate(lines) if re.match(r"_Z18mha_bwd_p_mfma_v_k\w*:", l))
    inasm, n_asm, outside = False, 0, []
    for l in lines[i + 1:]:
        if l.lstrip().startswith(".Lfunc_end"):
            break
        if "#ASMSTART" in l:
            inasm = True
        elif "#ASMEND" in l:
            inasm = False
        elif not l.strip().startswith(";"):
            regs = [int(x) for x in re.findall(r"\bv(\d+)\b", l)] + [k for a, b in re.findall(r"v\[(\d+):(\d+)\]", l) for k in range(int(a), int(b) + 1)]
            if any(r >= 216 for r in regs):
                if inasm:
                    n_asm += 1
                else:
                    outside.append(l.strip())
    assert n_asm == 48 and not outside, (n_asm, outside[:3])          # 4 x 3 loads + 36 v_movs behind the wait
    # ... and the kernel descriptor must ALLOCATE those registers (v216..v251 -> 252 per lane): the compiler counts the asm clobber
    # list into the allocation today; a toolchain that stopped doing so would hand the wave 216 registers and the loads would land
    # out of range
    alloc = mod.allocated_vgprs(texts["attention_mfma.hip"], "_Z18mha_bwd_p_mfma_v_k")
    assert alloc and all(v >= 252 for v in alloc.values()), alloc


def test_no_kernel_source_reads_the_environment():
    """the kernel sources carry no A/B switches: nothing under csrc/ calls getenv, and the only MMRCA_* variable lib.py reads is
    MMRCA_SK (include/mmrca.h documents it)"""
    pkg = os.path.join(ROOT, "garbage_classification_rca_amd")
    for f in sorted(os.listdir(os.path.join(pkg, "csrc"))):
        if f.endswith((".hip", ".cpp", ".h")):
            with open(os.path.join(pkg, "csrc", f)) as fh:
                for n, line in enumerate(fh, 1):
                    assert "getenv" not in line, f"csrc/{f}:{n}: {line.strip()}"
    with open(os.path.join(pkg, "lib.py")) as fh:
        reads = re.findall(r"os\.environ\s*(?:\.get\s*\(|\[)\s*[\"'](MMRCA_[A-Z0-9_]+)", fh.read())
    assert set(reads) == {"MMRCA_SK"}, reads


def test_bench_launches_its_own_ranks_and_reports_a_failed_one(tmp_path, capfd):
    """bench.launch_ranks (python bench.py --gpus N with no torchrun around it; main_both.py:386-388's multi-GPU entry): every child gets
    torchrun's environment, rank 0's stdout is the parent's, and one failing rank ends the others and sets the exit code.  The children
    here are a probe script -- the parent never touches a GPU, so this runs on the CPU box."""
    import time
    sys.path.insert(0, ROOT)
    import bench
    probe = tmp_path / "probe.py"
    probe.write_text(
        "import json, os, sys, time\n"
        "r = int(os.environ['RANK'])\n"
        "print(json.dumps({k: os.environ.get(k) for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}), flush=True)\n"
        "if sys.argv[1] == 'fail':\n"
        "    if r == 1: sys.exit(3)\n"
        "    time.sleep(120)\n")
    capfd.readouterr()
    assert bench.launch_ranks(3, [sys.executable, str(probe), "ok"]) == 0
    out = [json.loads(l) for l in capfd.readouterr().out.splitlines() if l.startswith("{")]
    assert len(out) == 1                          # only rank 0's line reaches stdout
    assert out[0]["RANK"] == "0" and out[0]["LOCAL_RANK"] == "0" and out[0]["WORLD_SIZE"] == "3" and out[0]["LOCAL_WORLD_SIZE"] == "3"
    assert out[0]["MASTER_ADDR"] == "127.0.0.1" and int(out[0]["MASTER_PORT"]) > 0
    t0 = time.time()
    assert bench.launch_ranks(2, [sys.executable, str(probe), "fail"]) == 3
    assert time.time() - t0 < 60                  # rank 0 (sleeping) was ended, not waited for


def test_bench_output_dump_samples_parameters_in_state_dict_order(tmp_path):
    """bench.py --dump-outputs: the parameter values are the arena's entries in key order without its alignment padding, or a
    fixed, seeded sample of them; the files are float32 (float64 kept) and stay under the size limit"""
    sys.path.insert(0, ROOT)
    import bench
    from garbage_classification_rca_amd.engine import Arena
    ents = [("a", (3, 5)), ("b", (7,)), ("c", (2, 2, 2))]
    ar = Arena(ents, "cpu", with_lp=False)
    for k, _ in ents:
        ar.view(k).copy_(torch.randn(ar.view(k).shape))
    flat = torch.cat([ar.view(k).reshape(-1) for k, _ in ents])
    assert ar.total > flat.numel()                                     # (there is padding to leave out)
    assert torch.equal(bench.param_sample(ar, [k for k, _ in ents]), flat)
    s1, s2 = (bench.param_sample(ar, [k for k, _ in ents], n=16, seed=3) for _ in range(2))
    assert torch.equal(s1, s2) and s1.numel() == 16
    assert torch.equal(s1, flat[torch.from_numpy(bench.flat_sample(flat.numel(), 16, 3))])
    bench.dump_outputs(str(tmp_path / "d"), {"x": flat.bfloat16(), "y": flat.double(), "loss": torch.ones(1)})
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in ("x", "y", "loss")}
    assert got["x"].dtype == np.float32 and got["y"].dtype == np.float64 and got["loss"].dtype == np.float32
    assert np.array_equal(got["y"], flat.double().numpy())
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "big"), {"x": torch.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1)})


def _width_worker(rank, world, port, q):
    """two ranks whose batches use different caption widths end up on the SAME trimmed width (the graph key of a captured train step)"""
    import torch.distributed as dist
    from garbage_classification_rca_amd import training as TR
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = []
    for lens in ([5, 9], [20, 3], [3, 40], [64, 64]):
        n = lens[rank]
        mask = torch.zeros(4, 64, dtype=torch.int64)
        mask[:, :n] = 1
        tok = torch.arange(4 * 64).view(4, 64)
        own = TR.caption_width(mask)
        w = D.agree_caption_width(own)
        t, m = TR.trim_caption_columns(tok, mask, width=w)
        out.append((own, w, tuple(t.shape), int(m.sum()), bool(torch.equal(t, tok[:, :w]))))
    sync = D.GradSync(torch.zeros(8), world)
    out.append(sync.capturable())
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_ranks_agree_on_the_caption_width_of_a_graphed_step_world2():
    """run_one_epoch trims captions per rank and the trimmed width is part of the HIP-graph key -- the ranks now take the
    maximum over the ranks (host-side gloo all-reduce), so they key alike; and the captured RCCL exchange is opt-in on > 1 rank."""
    res = dict(_run_world2(_width_worker))
    for r in (0, 1):
        own = [x[0] for x in res[r][:4]]
        assert own == ([16, 32, 16, 64] if r == 0 else [16, 16, 48, 64])
        assert [x[1] for x in res[r][:4]] == [16, 32, 48, 64]                  # the maximum of the two
        assert [x[2] for x in res[r][:4]] == [(4, 16), (4, 32), (4, 48), (4, 64)]
        assert all(x[4] for x in res[r][:4])
        assert res[r][4] is False                                               # gloo: never capturable
    assert [x[3] for x in res[0][:4]] == [4 * 5, 4 * 20, 4 * 3, 4 * 64]         # no live token cut off
