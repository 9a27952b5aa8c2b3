"""The bf16x3 attention forward at 225 <= S <= 512 (mha_fwd_x3_c_k, csrc/attention_mfma.hip): keys walked in chunks of 128 with a
running maximum / sum per query row, behind the unchanged entry point mmrca_mha_fwd_x3 -- what the bf16x3f mode runs when the text
encoder sees captions padded to the text model's maximum.  Needs an MI355X; every call goes through the C ABI.

Bounds are test_x3f_gpu.py's for S <= 224: context within 3e-5 of the largest entry and log-sum-exp within 1e-5 * max(1, max |lse|)
against a float64 softmax(QK^T scale)V on the values the planes encode; under dropout, context within 2e-5 of the largest entry
against the fp32 reference kernel drawing the same counter masks.  Shapes: B = 2 .. 4, H = 2; S = 225 is the first length past the
resident kernel, 257 and 385 leave ONE key in the last chunk, 300 has a ragged last query tile and a ragged last 32-key pair, 449 is
one key past two of the resident kernel's 224-key images, 256 and 512 are whole chunks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import lib as L            # noqa: E402
from tests.test_x3f_gpu import _planes                         # noqa: E402

DH, H = 64, 2
D = H * DH
SCALE = DH ** -0.5


def _setup():
    assert torch.cuda.is_available(), "these tests need a GPU"
    L.load()
    L.seed_epoch_set(0)          # (test_graph_gpu.py moves the dropout-mask epoch)


def _qkv(rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    hi, lo = _planes(torch.randn(rows, 3 * D, device="cuda", generator=g))
    return hi, lo, hi.float() + lo.float()            # the planes and exactly what they encode


def _x3(hi, lo, mask, B, S, rows, drop=0.0, seed=0, cu=None):
    pl = (torch.full((rows, D), float("nan"), dtype=torch.bfloat16, device="cuda"), torch.full((rows, D), float("nan"), dtype=torch.bfloat16, device="cuda"))
    lse = torch.full((B * H * S,), float("nan"), device="cuda")
    L.mha_fwd_x3((hi, lo), mask, pl, lse, B, H, S, DH, SCALE, drop_p=drop, drop_seed=seed, cu=cu)
    torch.cuda.synchronize()
    return pl, lse


def _ref_kernel(qkv, mask, B, S, rows, drop=0.0, seed=0, cu=None):
    """the fp32 reference kernels (attention_ref.hip) on the fp32 values"""
    o, lse = torch.zeros(rows, D, device="cuda"), torch.zeros(B * H * S, device="cuda")
    L.mha_fwd(qkv, mask, o, lse, B, H, S, DH, SCALE, L.F32, impl=L.IMPL_REF, drop_p=drop, drop_seed=seed, cu=cu)
    torch.cuda.synchronize()
    return o, lse


def _f64(qkv, kval, B, S):
    """float64 softmax(QK^T scale)V over the valid keys kval [B, S]: context [B*S, D] (0 for a query without a valid key) and lse
    [B*H*S] (+inf there)"""
    x = qkv.double().view(B, S, 3, H, DH)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    sc = ((q @ k.transpose(2, 3)) * SCALE).masked_fill(~kval.view(B, 1, 1, S), float("-inf"))
    live = kval.any(1).view(B, 1, 1, 1)
    p = torch.softmax(torch.where(live, sc, torch.zeros_like(sc)), -1) * live
    lse = torch.where(live[..., 0], torch.logsumexp(torch.where(live, sc, torch.zeros_like(sc)), -1), torch.full((B, H, S), float("inf"), dtype=torch.float64, device=qkv.device))
    return (p @ v).transpose(1, 2).reshape(B * S, D), lse.reshape(-1)


def _check_f64(tag, pl, lse, ref, lref):
    got = pl[0].double() + pl[1].double()
    assert bool(torch.isfinite(got).all()), f"{tag}: context rows not written"
    fin = torch.isfinite(lref)
    assert torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == float("inf")).all()), f"{tag}: +inf log-sum-exp entries differ"
    e = float((got - ref).abs().max()) / float(ref.abs().max())
    el, lmax = float((lse[fin].double() - lref[fin]).abs().max()), float(lref[fin].abs().max())
    print(f"{tag}: context error {e:.2e} of the largest entry (bound 3e-5), lse error {el:.2e} (bound {1e-5 * max(1.0, lmax):.2e})")
    assert e < 3e-5
    assert el <= 1e-5 * max(1.0, lmax)


@pytest.mark.parametrize("S", [225, 256, 257, 300, 385, 449, 512])
def test_unmasked_shapes_match_float64_and_repeat_bitwise(S):
    """observed on the MI355X (seeded inputs, no atomics: repeatable): context 5.4e-6 .. 7.3e-6, log-sum-exp 1.2e-6 .. 1.7e-6"""
    _setup()
    B = 2
    hi, lo, qkv = _qkv(B * S, S)
    pl, lse = _x3(hi, lo, None, B, S, B * S)
    ref, lref = _f64(qkv, torch.ones(B, S, dtype=torch.bool, device="cuda"), B, S)
    _check_f64(f"bf16x3 chunked forward S={S}", pl, lse, ref, lref)
    pl2, lse2 = _x3(hi, lo, None, B, S, B * S)
    assert torch.equal(pl2[0], pl[0]) and torch.equal(pl2[1], pl[1]) and torch.equal(lse2, lse)


@pytest.mark.parametrize("S", [300, 512])
def test_key_masks_whole_masked_chunks_and_a_fully_masked_sequence(S):
    """sequence 0: a random mask; 1: the whole first chunk (keys 0..127) masked, so the running maximum is still -inf when the second
    chunk arrives; 2: every key masked (zero context, lse = +inf); 3: everything from key 128 on masked (all later chunks must leave
    maximum, sum and O as they are).  observed: context 6.1e-6 / 4.7e-6, log-sum-exp 1.7e-6 / 2.3e-6"""
    _setup()
    B = 4
    hi, lo, qkv = _qkv(B * S, 1000 + S)
    g = torch.Generator(device="cuda").manual_seed(S)
    kval = torch.rand(B, S, device="cuda", generator=g) > 0.3
    kval[1, :128] = False
    kval[2] = False
    kval[3, 128:] = False
    mask = kval.int().contiguous().view(-1)
    pl, lse = _x3(hi, lo, mask, B, S, B * S)
    ref, lref = _f64(qkv, kval, B, S)
    _check_f64(f"bf16x3 chunked forward, masked, S={S}", pl, lse, ref, lref)
    got = pl[0].float() + pl[1].float()
    assert float(got.view(B, S, D)[2].abs().max()) == 0.0 and bool((lse.view(B, H, S)[2] == float("inf")).all())
    _, lk = _ref_kernel(qkv, mask, B, S, B * S)
    assert torch.equal(torch.isfinite(lse), torch.isfinite(lk))          # the same set of live rows as the reference kernel
    pl2, lse2 = _x3(hi, lo, mask, B, S, B * S)
    assert torch.equal(pl2[0], pl[0]) and torch.equal(pl2[1], pl[1]) and torch.equal(lse2, lse)


@pytest.mark.parametrize("S", [300, 512])
def test_packed_layout_equals_the_padded_run_bit_for_bit(S):
    """captions of [S, 9, 230, 1] tokens stored back to back: only the live keys are walked (3 or 4, 1, 2 and 1 chunks), chunk
    boundaries at the same key indices as in the padded run with the tail keys masked"""
    _setup()
    B = 4
    lens = torch.tensor([S, 9, 230, 1])
    hi, lo, _ = _qkv(B * S, 2000 + S)
    kval = torch.arange(S)[None, :] < lens[:, None]
    pos = torch.nonzero(kval.reshape(-1))[:, 0].cuda()                 # padded row of every packed row
    rows = int(lens.sum())
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).int().cuda()
    plp, lsep = _x3(hi, lo, kval.int().contiguous().view(-1).cuda(), B, S, B * S)
    plk, lsek = _x3(hi[pos].contiguous(), lo[pos].contiguous(), torch.ones(rows, dtype=torch.int32, device="cuda"), B, S, rows, cu=cu)
    assert torch.equal(plk[0], plp[0][pos]) and torch.equal(plk[1], plp[1][pos])
    live = kval.cuda()[:, None, :].expand(B, H, S).reshape(-1)          # lse keeps the padded [B, H, S] index space
    assert torch.equal(lsek[live], lsep[live]) and bool(torch.isfinite(lsek[live]).all())


@pytest.mark.parametrize("S", [256, 512])
def test_dropout_draws_the_masks_of_the_fp32_reference_kernel(S):
    """attention-probability dropout 0.1 from the counter (seed, ((b*H+h)*S+q)*S+key): the same masks as attention_ref.hip with the
    same seed, or the contexts would differ by whole probabilities.  observed: 6.1e-6 / 9.4e-6 of the largest entry"""
    _setup()
    B = 3
    hi, lo, qkv = _qkv(B * S, 3000 + S)
    g = torch.Generator(device="cuda").manual_seed(S)
    mask = (torch.rand(B * S, device="cuda", generator=g) > 0.2).int()
    mask.view(B, S)[:, 0] = 1
    pl, lse = _x3(hi, lo, mask, B, S, B * S, drop=0.1, seed=77)
    ref, lk = _ref_kernel(qkv, mask, B, S, B * S, drop=0.1, seed=77)
    got = pl[0].float() + pl[1].float()
    e = float((got - ref).abs().max()) / float(ref.abs().max())
    el = float((lse - lk).abs().max())
    print(f"bf16x3 chunked forward, dropout 0.1, S={S}: context error {e:.2e} of the largest entry (bound 2e-5), lse vs the reference kernel {el:.2e}")
    assert e < 2e-5
    assert el <= 1e-5 * max(1.0, float(lk.abs().max()))
    pl2, lse2 = _x3(hi, lo, mask, B, S, B * S, drop=0.1, seed=77)
    assert torch.equal(pl2[0], pl[0]) and torch.equal(pl2[1], pl[1]) and torch.equal(lse2, lse)


def test_bf16_backward_pairs_with_the_chunked_forward_under_dropout():
    """What the bf16x3f mode does at S = 300: the bf16 backward (mmrca_mha_bwd) reads the hi planes of q|k|v and of the chunked forward's
    context, its log-sum-exp and the same dropout seed, and must rebuild the forward's masks.  Against float64 autograd of
    ((softmax(QK^T scale) o keep) V) on the hi-plane values with keep from the counter function (tests/test_attention_cells_gpu._keep);
    bound: that file's bf16 backward cells, max |err| <= 1.5e-2 x max |ref| per (sequence, head) block of dQ, dK and dV.
    observed: dQ 3.9e-3, dK 3.8e-3, dV 3.8e-3"""
    from tests.test_attention_cells_gpu import BOUND, P_DROP, SEED, _keep
    _setup()
    B, S = 2, 300
    hi, lo, _ = _qkv(B * S, 4000)
    g = torch.Generator(device="cuda").manual_seed(5)
    dout = torch.randn(B * S, D, device="cuda", generator=g).bfloat16()
    pl, lse = _x3(hi, lo, None, B, S, B * S, drop=P_DROP, seed=SEED)
    dqkv = torch.full((B * S, 3 * D), float("nan"), dtype=torch.bfloat16, device="cuda")
    L.mha_bwd(hi, None, pl[0], dout, lse, dqkv, B, H, S, DH, SCALE, L.BF16, L.IMPL_AUTO, drop_p=P_DROP, drop_seed=SEED)
    torch.cuda.synchronize()
    x = hi.double().view(B, S, 3, H, DH).requires_grad_(True)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    o = (torch.softmax((q @ k.transpose(2, 3)) * SCALE, -1) * _keep(B, H, S)) @ v             # [B, H, S, dh]
    o.backward(dout.double().view(B, S, H, DH).transpose(1, 2))
    got = dqkv.double().view(B, S, 3, H, DH)
    assert bool(torch.isfinite(got).all())
    for i, name in enumerate(("dq", "dk", "dv")):
        err = (got[:, :, i] - x.grad[:, :, i]).abs().amax((1, 3))                              # [B, H]
        mag = x.grad[:, :, i].abs().amax((1, 3))
        worst = float((err / mag).max())
        print(f"bf16 backward behind the chunked forward, S={S}, dropout {P_DROP}: {name} worst block error {worst:.2e} (bound {BOUND[('bf16', name)]:.1e})")
        assert worst <= BOUND[("bf16", name)]


# ------------------------------------------------------------------------------------------------ engine level
_ORC = {}


def _batch():
    from garbage_classification_rca_amd.procedural import proc_input, synth_captions
    B, T = 2, 256
    ids, mask = synth_captions(B, T, seed=4321)
    ids, mask = ids.copy(), mask.copy()
    mask[0, :] = 1                               # one caption fully live,
    mask[1, :17], mask[1, 17:] = 1, 0            # one of 17 tokens
    ids[1, 17:] = 0
    ids[:, 0] = 101
    images = proc_input("e2e.images", (B, 3, 224, 224))
    return torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(images), mask


def _oracle():
    """float64 logits and parameter gradients of the oracle on the initialisation the model trains from, computed once"""
    if not _ORC:
        import os
        from oracle import model as O
        from tests.test_x3_gpu import _pair_init_weights
        eng, orc, sd = _pair_init_weights(0)
        eng.release_buffers()
        del eng
        torch.cuda.empty_cache()
        ids, mask, images, _ = _batch()
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        orc = orc.double()
        for p in orc.parameters():
            p.requires_grad_(True)
        ref = orc(ids, mask, images.double(), eval=True)
        labels, cw = torch.tensor([0, 1]), torch.tensor([0.7, 1.3, 0.9, 1.1])
        O.cross_entropy(ref, labels, cw.double(), 0.1).backward()
        named = {"text_model." + k.replace("/", "."): p for k, p in orc.text_model.params.items()}
        named.update({"image_model." + k.replace("/", "."): p for k, p in orc.image_model.params.items()})
        named.update({k: p for k, p in orc.named_parameters() if not k.startswith(("text_model.", "image_model."))})
        _ORC.update(sd=sd, ref=ref.detach(), named=named, labels=labels, cw=cw)
    return _ORC


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_x3f_engine_at_256_positions_keeps_q_k_v_as_planes(layout, monkeypatch):
    """DistilBERT + ViT-B/16 in bf16x3f, B = 2, captions of 256 positions (one fully live, one of 17 tokens): the QKV GEMM writes planes,
    the forward is the chunked three-pass kernel, the bf16 backward reads the hi planes.  Logits < 1e-3 against the float64 oracle and
    test_x3f_gpu.py's gradient bounds (cosine >= 0.999, worst entry <= 6e-2).  The padded run switches the class-token tail off so
    that EVERY text layer, the last included, goes through mmrca_mha_fwd_x3 and mmrca_mha_bwd -- then no q|k|v buffer in fp32 and no
    *_qkv16 cast scratch may exist; the packed run keeps the default (the last layer's class-token attention reads fp32 q|k|v).
    observed: padded logits 1.5e-6, worst gradient entry 2.1e-2, min cosine 0.99991; packed 1.6e-6, 2.1e-2, 0.99991"""
    from garbage_classification_rca_amd import engine as E
    from tests.test_engine_gpu import rel
    _setup()
    o = _oracle()
    if layout == "padded":
        monkeypatch.setattr(E, "CLS_TAIL", False)
    ids, mask, images, mask_np = _batch()
    B, T = ids.shape
    eng = E.MMRCAEngine("distilbert", "transformer_B16", 4, True, 0, "bf16x3f")
    eng.load_arrays(o["sd"])
    assert eng.x3f and eng._qkv_planes_ok(T, DH)
    pack = E.make_text_pack(mask_np, "cuda") if layout == "packed" else None
    assert (pack is not None) == (layout == "packed")
    logits = eng.forward(ids.cuda(), mask.cuda(), images.cuda(), text_pack=pack)
    loss, dl = torch.empty(1, device="cuda"), torch.empty(B, 4, device="cuda")
    L.xent_fwd_bwd(logits, o["labels"].int().cuda(), o["cw"].cuda(), 0.1, loss, dl, B, 4)
    layers = eng._saved["text"]["layers"]
    planes = [isinstance(a["qkv"], E.Planes) for a in layers]
    eng.arena.g.zero_()
    eng.backward(dl)
    torch.cuda.synchronize()
    names = [k[0] for k in eng._bufs if isinstance(k, tuple) and isinstance(k[0], str)]
    if layout == "padded":
        assert all(planes)
        assert not [n for n in names if n.endswith("_qkv16")] and "t_qkv" not in names, sorted(set(names))
    else:
        assert all(planes[:-1])
    gmax = max(float(p.grad.abs().max()) for p in o["named"].values() if p.grad is not None)
    worst, cos_min = 0.0, 1.0
    for k in eng.param_keys:
        gr = o["named"][k].grad
        got = eng.arena.view(k, "g").cpu().double()
        if gr is None:
            assert float(got.abs().max()) == 0.0, k
            continue
        gr = gr.view_as(got)
        worst = max(worst, float((got - gr).abs().max()) / max(float(gr.abs().max()), 1e-3 * gmax))
        if float(gr.abs().max()) > 1e-3 * gmax and gr.numel() >= 64:
            cos_min = min(cos_min, float(torch.nn.functional.cosine_similarity(got.flatten(), gr.flatten(), dim=0)))
    e = rel(logits, o["ref"])
    print(f"bf16x3f engine, T=256, {layout}: logits {e:.2e}, worst gradient entry {worst:.2e}, min cosine {cos_min:.5f}")
    eng.release_buffers()
    assert e < 1e-3
    assert cos_min >= 0.999 and worst <= 6e-2
