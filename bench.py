#!/usr/bin/env python
"""Headline benchmark: train samples/s (image+text pairs) of MM-RCA, ViT-B/16 + DistilBERT, bf16, per-GPU batch 256
(BASELINE.json configs[1]), on N GPUs of one node (weak scaling, one process per GPU over RCCL).

    python bench.py --gpus 1 --steps 10 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
    python bench.py --gpus N ...          # no launcher: bench.py starts its own N ranks (launch_ranks below) and relays rank 0's line

A step = one pass of the hot path over one batch of synthetic pairs already resident in HBM: forward (text encoder,
vision encoder, fused RCA head), weighted/smoothed cross entropy, full backward (fine-tuning phase: every parameter
trainable, main_both.py:690-697), gradient all-reduce (N>1), SGD step (lr 1e-3, weight decay 1e-2: the reference
defaults, options.py) and gradient zeroing.  Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md, chip-level parameters)
PEAK_F32_TFLOPS = 157.3        # fp32-in MFMA (v_mfma_f32_32x32x2_f32), same guide
# forward matmul FLOPs per sample: DistilBERT S=64 5.51 G + ViT-B/16 35.1 G + head 2.9 M
FWD_GFLOP_PER_SAMPLE = 40.6


def gemm_sources_sha256() -> str:
    """hash of the GEMM kernel sources: roofline.traffic quotes a committed PMC summary only if it was measured on these"""
    import hashlib
    h = hashlib.sha256()
    for f in ("gemm.hip", "gemm256.hip", "gemm_x3.hip", "lds_asm.h", "common.h"):
        with open(os.path.join(ROOT, "garbage_classification_rca_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def effective_cores() -> int:
    """Cores this process may actually use: min(affinity, cgroup CPU quota).  (On the GPU boxes os.cpu_count() is 256
    while the container's quota is 16 CPUs; 256 threads under that quota run ~10x slower than 16.)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


DUMP_LIMIT_BYTES = 64 << 20    # --dump-outputs: all files together
DUMP_SAMPLE = 4 << 20          # larger outputs are dumped as a fixed, seeded sample of this many values (16 MB in float32)


def flat_sample(total: int, n: int = DUMP_SAMPLE, seed: int = 0):
    """indices 0 .. total-1, or a fixed, seeded, sorted sample of n of them (numpy int64)"""
    import numpy as np
    if total <= n:
        return np.arange(total, dtype=np.int64)
    return np.sort(np.random.default_rng(seed).integers(0, total, n, dtype=np.int64))


def param_sample(arena, keys, n: int = DUMP_SAMPLE, seed: int = 0) -> torch.Tensor:
    """the parameters `keys` of a flat arena (engine.Arena) concatenated in that order, the arena's alignment padding left out --
    or a fixed, seeded sample of n of those values; the sample does not depend on the arena layout"""
    import numpy as np
    starts = np.array([arena.offsets[k][0] for k in keys], dtype=np.int64)
    sizes = np.array([arena.offsets[k][2] for k in keys], dtype=np.int64)
    ends = np.cumsum(sizes)
    logical = flat_sample(int(ends[-1]), n, seed)
    which = np.searchsorted(ends, logical, side="right")
    idx = starts[which] + logical - (ends[which] - sizes[which])
    return arena.p[torch.from_numpy(idx).to(arena.p.device)]


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """--dump-outputs: each array as <out_dir>/<name>.npy, float64 kept, everything else as float32"""
    import numpy as np
    host = {}
    for name, a in arrays.items():
        a = a.detach()
        host[name] = a.double().cpu().numpy() if a.dtype == torch.float64 else a.float().cpu().numpy()
    nbytes = sum(a.nbytes for a in host.values())
    assert nbytes <= DUMP_LIMIT_BYTES, f"--dump-outputs: {nbytes} bytes > {DUMP_LIMIT_BYTES}"
    os.makedirs(out_dir, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    print(f"[bench] outputs of the last timed step: {', '.join(f'{k}{list(a.shape)}' for k, a in host.items())} -> {out_dir}",
          file=sys.stderr, flush=True)


class LogitsKeepingCrossEntropy:
    """--dump-outputs: training.FusedCrossEntropy that also keeps a reference to the logits it is given (no copy, no sync), so the
    logits of the last timed step can be read after the timed region.  Under a HIP graph that is the captured logits buffer, which
    every replay rewrites."""

    def __init__(self, crit):
        self.crit, self.weight, self.logits = crit, crit.weight, None

    def __call__(self, logits, labels):
        self.logits = logits
        return self.crit(logits, labels)


def cpu_baseline(batches=(4, 32), steps=3, seq_len=64, text_model="distilbert", image_model="transformer_B16", image_size=224):
    """The oracle (CPU restatement of the reference's model + run_one_epoch step) on this box's host cores, same synthetic
    tensors, fp32 eager, fine-tuning phase, as SURVEY.md section 8(d) states it: batch 4 (configs[0]'s batch) and batch 32,
    `steps` timed steps after one warm-up each, torch threads = the cores this process may use (stated).  `value` is the
    batch-32 figure.  A reported baseline, not the optimisation target."""
    from oracle import model as O
    from garbage_classification_rca_amd.procedural import synth_captions
    n = effective_cores()
    torch.set_num_threads(n)
    m = O.build_oracle(text_model, image_model, True, drop_ratio=0.6, enc_dropout=0.1).train()
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("image_model.") and image_model not in ("transformer_B16", "transformer_L16"):
                continue              # conv backbone: torchvision's own init
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif name.endswith("weight"):
                p.fill_(1.0)          # every 1-D "weight" on this path is a LayerNorm scale
            else:
                p.zero_()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3, weight_decay=1e-2)
    by_batch = {}
    for batch in batches:
        print(f"[bench] cpu_baseline: oracle train step on {n} host threads, batch {batch} ...", file=sys.stderr, flush=True)
        ids, mask = (torch.from_numpy(a) for a in synth_captions(batch, seq_len, seed=4321))
        images = torch.randn(batch, 3, image_size, image_size, generator=torch.Generator().manual_seed(1234))
        labels = torch.arange(batch) % 4

        def step():
            out = m(ids, mask, images)
            loss = O.cross_entropy(out, labels)
            loss.backward()
            opt.step()
            opt.zero_grad()
        step()
        t0 = time.time()
        for _ in range(steps):
            step()
            print("[bench] cpu_baseline: step done", file=sys.stderr, flush=True)
        by_batch[batch] = round(batch * steps / (time.time() - t0), 3)
    return {"value": by_batch[batches[-1]], "unit": "samples/s", "cores": n, "threads": n, "kind": "port",
            "by_batch": {str(k): v for k, v in by_batch.items()},
            "sample": f"oracle (PyTorch CPU fp32 eager restatement of MM_RCA + run_one_epoch step), {image_model} + {text_model}, "
                      f"S={seq_len}, batch {' and '.join(str(b_) for b_ in batches)} (value = batch {batches[-1]}), {steps} timed steps after 1 warm-up each, "
                      f"torch.set_num_threads({n}) = min(affinity, cgroup quota) of this box"}


def parity_check(model, ids, mask, images, n=8, others=True):
    """Logits of all three precision modes of the engine against the oracle (CPU fp32) on the first `n` synthetic pairs, with
    the benchmarked model's CURRENT weights (eval mode: no dropout).  Runs after the timed region; the oracle is the checker
    here, never the thing measured."""
    from oracle import model as O
    from garbage_classification_rca_amd.engine import MMRCAEngine, make_text_pack
    eng = model.engine
    sd = {k: eng.arena.view(k).detach().cpu().clone() for k in eng.param_keys}
    img_name = eng.vs.name if eng.vs is not None else eng.conv.name
    orc = O.build_oracle(eng.ts.name, img_name, eng.reverse, eng.mode == 1, eng.mode == 2, drop_ratio=0.0, enc_dropout=0.0).eval()
    orc.text_model.load_flat(sd, "text_model.")
    if eng.vs is not None:
        orc.image_model.load_flat(sd, "image_model.")
    else:       # conv backbone: parameters and BatchNorm running statistics by their torchvision names
        eng.conv.sync_buffers()
        isd = {k[len("image_model."):]: v for k, v in sd.items() if k.startswith("image_model.")}
        isd.update({k: v.detach().cpu() for k, v in eng.conv.buffers.items()})
        orc.image_model.load_state_dict(isd)
    orc.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("text_model.", "image_model."))}, strict=False)
    i_h, m_h, x_h = ids[:n].cpu(), mask[:n].cpu(), images[:n].float().cpu()
    torch.set_num_threads(effective_cores())
    with torch.no_grad():
        ref = orc(i_h, m_h, x_h, eval=True)
    rel = lambda a: float(((a.float().cpu() - ref).abs().max() / ref.abs().max()).item())
    pack = make_text_pack(m_h.numpy(), ids.device)
    own = "bf16x3f" if eng.x3f else ("bf16x3" if eng.x3 else ("bf16" if eng.dtype == torch.bfloat16 else "fp32"))
    eng.refresh_working_copy(force=True)
    out = {own + "_logits_rel": round(rel(eng.forward(ids[:n], mask[:n], images[:n], save=False, text_pack=pack)), 8), "samples": n,
           "benchmarked_mode": own,
           "reference": "oracle (CPU fp32 restatement pinned by the reference's goldens), same weights, eval mode"}
    # with transformer encoders bf16x3f's forward IS the bf16x3 forward (same kernels, same logits); with a conv image backbone it is
    # not (bf16 conv kernels next to the bf16x3 text encoder) and is measured on its own
    modes = [("bf16", torch.bfloat16), ("bf16x3", "bf16x3"), ("fp32", torch.float32)] + ([("bf16x3f", "bf16x3f")] if eng.conv is not None else [])
    for name, dt in modes if others else ():
        if name == own or (name == "bf16x3" and own == "bf16x3f" and eng.conv is None):
            continue
        e2 = MMRCAEngine(eng.ts.name, img_name, eng.n_classes, eng.reverse, eng.mode, dt, eng.device)
        e2.load_arrays(sd)
        if eng.conv is not None:
            e2.conv.load_buffers({k: v for k, v in eng.conv.buffers.items()})
        out[name + "_logits_rel"] = round(rel(e2.forward(ids[:n], mask[:n], images[:n], save=False)), 8)
        e2.release_buffers()
        del e2
    out["north_star_bound"] = 1e-3
    out["modes_meeting_the_bound"] = [k[:-len("_logits_rel")] for k, v in out.items() if k.endswith("_logits_rel") and v <= 1e-3]
    if eng.conv is None and "bf16x3" in out["modes_meeting_the_bound"] and "bf16x3f" not in out["modes_meeting_the_bound"]:
        out["modes_meeting_the_bound"].append("bf16x3f")          # its forward IS the bf16x3 forward (same kernels, same logits)
    return out


def compliant_leg(args, dev, parity, steps=12, warmup=3):
    """A second, short timed leg of the SAME workload (same batch, shapes, optimizer, synthetic tensors, packed captions) in the
    fastest precision mode whose forward logits meet north_star's bound (<= 1e-3 relative to the fp32 reference,
    CVPR_code/multimodal_model.py:651-726), so that the driver's own line carries a timed number for a compliant mode next to the
    bf16 headline.  Candidates in order of speed: bf16x3f (the bf16x3 forward with the bf16 backward), bf16x3, fp32; the choice is
    made on the parity object measured on the headline's weights.  The leg trains its own replica from the same seed; its
    `logits_rel` is measured on ITS weights after ITS steps (8 pairs against the oracle), and the figure on the headline's
    post-run weights is repeated next to it."""
    from garbage_classification_rca_amd.engine import make_text_pack
    from garbage_classification_rca_amd.multimodal_model import MM_RCA
    from garbage_classification_rca_amd.optim import FlatSGD
    from garbage_classification_rca_amd.procedural import synth_captions
    from garbage_classification_rca_amd.training import FusedCrossEntropy, hip_train_step, PACK_TEXT
    import contextlib
    import io
    fwd_of = {"bf16x3f": "bf16x3f" if "bf16x3f_logits_rel" in parity else "bf16x3", "bf16x3": "bf16x3", "fp32": "fp32"}
    mode = next((m for m in ("bf16x3f", "bf16x3", "fp32") if parity.get(fwd_of[m] + "_logits_rel", 1.0) <= 1e-3), None)
    if mode is None:
        return {"dtype": None, "note": "no mode met the bound on the headline's weights"}
    B, S = args.batch, args.seq_len
    print(f"[bench] compliant leg: {mode}, {warmup} + {steps} steps at batch {B} ...", file=sys.stderr, flush=True)
    with contextlib.redirect_stdout(io.StringIO()):
        model = MM_RCA(4, 0.6, 0.0, 0.7, 256, args.text_model, B, True, False, args.cross_attention_only, image_model_name=args.image_model,
                       dtype={"fp32": torch.float32}.get(mode, mode), device=dev, init_seed=0, image_size=args.image_size)
    model.train()
    for p in model.parameters():
        p.requires_grad = True
    opt, crit = FlatSGD(model, lr=1e-3, weight_decay=1e-2), FusedCrossEntropy(None, 0.0)
    nb = 2
    ids, mask_host = synth_captions(B * nb, S, seed=4321)
    if args.text_model == "roberta":
        ids[mask_host == 0] = 1
    ids, mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask_host).to(dev)
    images = torch.randn(B * nb, 3, args.image_size, args.image_size, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    labels = (torch.arange(B * nb, device=dev) % 4).to(torch.int32)

    def step(i):
        j = (i % nb) * B
        return hip_train_step(model, ids[j:j + B], mask[j:j + B], images[j:j + B], labels[j:j + B], crit, opt, None,
                              text_pack=(make_text_pack(mask_host[j:j + B], dev) if PACK_TEXT else None))
    with contextlib.redirect_stdout(io.StringIO()):
        for i in range(warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            loss = step(i)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        own = parity_check(model, ids, mask, images, others=False)
        # roofline of THIS leg's GEMMs, measured like the headline's: the same steps replayed on one stream with HIP events around every
        # matrix-core GEMM launch.  Executed work counts the three passes of a bf16x3 product (3 x 2MNK); useful work is the fp32
        # product it stands for (2MNK).  The backward of bf16x3f is single-pass bf16: executed = useful there.
        from garbage_classification_rca_amd import lib as L
        eng = model.engine
        saved_streams = (eng._side_v, eng._side_t, eng._side, eng._text_stream)
        eng._side_v = eng._side_t = eng._side = eng._text_stream = None
        step(0)
        torch.cuda.synchronize()
        L.GEMM_PROFILE = []
        replay = 2
        for i in range(replay):
            step(i)
        torch.cuda.synchronize()
        prof, L.GEMM_PROFILE = L.GEMM_PROFILE, None
        eng._side_v, eng._side_t, eng._side, eng._text_stream = saved_streams
    g_exec = sum(p[0] for p in prof)
    g_useful = sum(2.0 * p[4][0] * p[4][1] * p[4][2] for p in prof)
    g_ms = sum(p[2].elapsed_time(p[3]) for p in prof)
    x3_ms = sum(p[2].elapsed_time(p[3]) for p in prof if p[0] > 2.5 * p[4][0] * p[4][1] * p[4][2])
    traffic, traffic_src = None, "no PMC pass of this mode is committed"
    import glob as _glob
    pmc_files = sorted(_glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_hbm_traffic_bf16x3f.json")), reverse=True)     # newest round first
    if pmc_files:
        pmc_json, pmc_name = pmc_files[0], os.path.basename(pmc_files[0])
        with open(pmc_json) as fh:
            pj = json.load(fh)
        if pj.get("gemm_sources_sha256") == gemm_sources_sha256():
            traffic, traffic_src = pj.get("gemm_hbm_bytes_per_launch_mean"), f"profiles/{pmc_name} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, x2 gfx950 fetch correction; this build's GEMM sources)"
        else:
            traffic_src = f"profiles/{pmc_name} is STALE (measured on other GEMM sources); not quoted"
    roof = {"bound": "mfma", "achieved": round(g_exec / (g_ms * 1e-3) / 1e12, 2) if g_ms > 0 else 0.0, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(g_exec / (g_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4) if g_ms > 0 else 0.0,
            "fp32_equivalent_useful_TFLOPs": round(g_useful / (g_ms * 1e-3) / 1e12, 2) if g_ms > 0 else 0.0,
            "useful_frac": round(g_useful / (g_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4) if g_ms > 0 else 0.0,
            "gemm_ms_per_step": round(g_ms / replay, 3), "three_pass_gemm_ms_per_step": round(x3_ms / replay, 3), "launches_per_step": len(prof) // replay,
            "traffic": traffic, "traffic_source": traffic_src,
            "flops_counted": "achieved = executed matrix-core work (3 x 2MNK for the forward's three-pass products, 2MNK for the bf16 backward) / GEMM "
                             "HIP-event time; fp32_equivalent_useful = 2MNK of every product / the same time",
            "measured_in": f"single-stream replay of {replay} steps after this leg's timed region"}
    model.engine.release_buffers()
    key = mode + "_logits_rel"
    out = {"dtype": mode, "value": round(B * steps / elapsed, 2), "unit": "samples/s", "ms_per_step": round(elapsed / steps * 1e3, 3), "steps": steps,
           "warmup": warmup, "per_gpu_batch": B, "logits_rel": own[key], "logits_rel_measured_on": f"this leg's weights after its {warmup + steps} steps, 8 pairs vs the oracle",
           "logits_rel_on_headline_weights": parity.get(fwd_of[mode] + "_logits_rel"), "north_star_bound": 1e-3, "final_loss": round(float(loss.item()), 4),
           "roofline": roof,
           "what": {"bf16x3f": "forward: fp32 residual stream / LayerNorm / attention (fp32 matrix cores), every nn.Linear as a three-pass split-bf16 product "
                               "(the bf16x3 forward, same logits); backward: the bf16 mode's (single-pass bf16 products and bf16 attention backward on the hi planes "
                               "of the saved activations, bf16 gradient buffers, fp32 gradient accumulation and optimizer); a conv image backbone runs its bf16 "
                               "kernels (measured: the bf16 mode's logits error on these models is its TEXT encoder's)",
                    "bf16x3": "fp32 storage, every nn.Linear (forward and backward) as a three-pass split-bf16 product, fp32 attention",
                    "fp32": "every GEMM and the attention on the fp32 matrix cores"}[mode]}
    return out


def bench_qformer(args):
    """BASELINE.json configs[4]: one iteration of q_former_training.py:279-302 per step -- frozen ViT-g/14 + Q-Former forward
    (train mode: Q-Former dropouts active), Linear(768,4) classifier, CE / 8, classifier backward, AdamW every 8th step.
    The OPT-2.7B forward the reference also runs feeds neither the loss nor the metrics and is not computed (q_former.py)."""
    from garbage_classification_rca_amd import lib as L
    from garbage_classification_rca_amd import distributed as D
    from garbage_classification_rca_amd import q_former as QF
    import torch.distributed as dist
    rank, local, world = D.init_from_env("nccl")
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs a GPU: the product path has no CPU fallback"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    L.load()
    B = args.batch
    x3 = args.dtype in ("bf16x3", "bf16x3f")
    dtype = torch.bfloat16 if args.dtype == "bf16" else ("bf16x3f" if x3 else torch.float32)
    spec = QF.BLIP2_OPT_2_7B
    eng = QF.Blip2QFormerEngine(spec, dtype=dtype, device=dev)
    eng.init_parameters(seed=0)
    opt = QF.ClassifierAdamW(eng)
    nb = 2
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    images = torch.randn(B * nb, 3, spec.image_size, spec.image_size, device=dev, generator=gen)
    labels = (torch.arange(B * nb, device=dev) % 4).view(-1, 1)

    def step(i):
        j = (i % nb) * B
        return QF.train_step(eng, opt, images[j:j + B], labels[j:j + B], i, world=world)

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"loss": loss, "classifier": eng.cls_p})
    # roofline of the dominant kernel family (the bf16 MFMA GEMMs): HIP events around every GEMM launch of a replay
    replay = max(1, min(2, args.steps))
    L.GEMM_PROFILE = []
    for i in range(replay):
        step(i)
    torch.cuda.synchronize()
    prof, L.GEMM_PROFILE = L.GEMM_PROFILE, None
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        if os.environ.get("MMRCA_CHECK_REPLICAS") == "1":
            # data-parallel invariant: every rank applied the same averaged classifier gradient
            chk = eng.cls_p.double().sum().view(1)
            lo, hi = chk.clone(), chk.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            assert float(hi - lo) == 0.0, f"replicas diverged: {float(lo)} vs {float(hi)}"
            if rank == 0:
                print(f"[bench] classifier replicas identical after {opt.t} optimizer steps (checksum {float(chk):.8f})", file=sys.stderr, flush=True)
    if rank != 0:
        return
    flops = sum(p[0] for p in prof)
    ms = sum(p[2].elapsed_time(p[3]) for p in prof)
    achieved = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    alg = [(2.0 if args.dtype == "bf16" else 4.0) * (Mg * Kg + Ng * Kg + Mg * Ng) for _f, _k, _e0, _e1, (Mg, Ng, Kg, _a) in prof]
    peak = PEAK_BF16_TFLOPS if (args.dtype == "bf16" or x3) else PEAK_F32_TFLOPS
    # logits of the timed mode against the oracle (full depth, 2 images, eval mode): the number north_star bounds by 1e-3
    parity = None
    if not args.no_cpu_baseline or args.parity:
        parity = qformer_parity(eng, spec, dev)
    T, D_, NQ = spec.v_tokens, spec.v_dim, spec.n_query
    attn_flop = B * (spec.v_layers * 4.0 * T * T * D_ + spec.q_layers * 4.0 * NQ * NQ * spec.q_dim
                     + (spec.q_layers // spec.cross_freq) * 4.0 * NQ * T * spec.q_dim)
    out = {"metric": "train samples/sec (images), BLIP-2 Q-Former classifier (q_former_training.py)", "value": round(B * world * args.steps / elapsed, 2),
           "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "bf16" if args.dtype == "bf16" else ("bf16x3f (fp32 values as two bf16 planes, three MFMA passes per product)" if x3 else "f32"),
           "data": "synthetic",
           "config": {"workload": "BASELINE configs[4]: q_former_training.py iteration -- frozen BLIP-2 ViT-g/14 (39 layers, 257x1408) + Q-Former "
                                  "(12 layers, 32 queries, cross-attention to the image tokens) forward in train mode, Linear(768,4) classifier fwd/bwd, "
                                  "CE/8, AdamW(5e-4, eps 1e-5) every 8th iteration; 224x224 images",
                      "per_gpu_batch": B, "global_batch": B * world, "parallelism": f"dp{world}", "random_init": True,
                      "dtype_note": "BASELINE configs[4] says fp16; the reference script itself runs fp32 (from_pretrained default, no autocast). "
                                    "This build stores the frozen towers in bf16 with fp32 accumulation -- the same byte width and MFMA rate as fp16 "
                                    "(the C ABI has no fp16 type) -- and keeps the classifier, loss and AdamW in fp32; --dtype fp32 runs everything in fp32",
                      "not_computed": "OPT-2.7B language-model forward (feeds neither the loss nor the metrics; its LoRA factors never get a gradient)",
                      "fwd_gemm_gflop_per_sample": round(flops / replay / B / 1e9, 1), "attention_gflop_per_sample": round(attn_flop / B / 1e9, 1),
                      "final_loss_over_8": round(float(loss.item()), 5)},
           "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                        "traffic": None, "algorithmic_bytes_per_launch": round(sum(alg) / max(len(alg), 1)),
                        "kernel": "bf16 16x16x32 MFMA GEMMs (every nn.Linear of the vision tower and the Q-Former, forward only)",
                        "launches_per_step": len(prof) // replay, "gemm_ms_per_step": round(ms / replay, 3),
                        "measured_in": f"replay of {replay} steps after the timed region, HIP events around each GEMM launch"}}
    if x3:
        out["roofline"]["flops_counted"] = ("achieved = EXECUTED bf16 matrix-core work (3 x 2MNK per product) / GEMM time; "
                                            "fp32_equivalent_useful = 2MNK / GEMM time")
        out["roofline"]["fp32_equivalent_useful_TFLOPs"] = round(achieved / 3.0, 2)
    if parity is not None:
        out["parity"] = parity
    if not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_qformer(spec)
    print(json.dumps(out), flush=True)


def qformer_parity(eng, spec, dev, batch=2):
    """logits of `eng`'s compute mode at FULL depth against oracle/qformer.py on procedural weights and inputs (eval mode), like
    tests/test_fullsize_gpu.py; the engine's own (random) weights are put back afterwards"""
    import numpy as np
    from oracle import qformer as OQ
    from garbage_classification_rca_amd import q_former as QF
    from garbage_classification_rca_amd.procedural import proc_tensor, proc_input
    torch.set_num_threads(effective_cores())
    print("[bench] parity: Q-Former oracle at full depth on the host ...", file=sys.stderr, flush=True)
    sd = {k: proc_tensor(k, shp) for k, shp in QF.blip2_params(spec)}
    sd["query_tokens"] = sd["query_tokens"] * np.float32(20.0)
    cls = {"classifier.weight": proc_tensor("classifier.weight", (spec.n_classes, spec.q_dim)) * np.float32(4.0),
           "classifier.bias": proc_tensor("classifier.bias", (spec.n_classes,))}
    cfg = dict(v_layers=spec.v_layers, v_heads=spec.v_heads, patch=spec.patch, q_layers=spec.q_layers, q_heads=spec.q_heads,
               cross_freq=spec.cross_freq, hidden_drop=spec.hidden_drop, attn_drop=spec.attn_drop)
    px = torch.from_numpy(proc_input("qf_px_full", (batch, 3, spec.image_size, spec.image_size)))
    with torch.no_grad():
        exp, _ = OQ.forward_logits(sd, cls, px, cfg, train=False)
    keep_w, keep_c, was_training = eng.store.w.clone(), eng.cls_p.clone(), eng.training
    eng.load_state_dict(sd, cls)
    got = eng.eval().forward(px.to(dev)).float().cpu()
    eng.store.w.copy_(keep_w); eng.cls_p.copy_(keep_c); eng._refresh_planes(); eng.train(was_training)
    e = float((got - exp).abs().max() / exp.abs().max())
    return {"logits_rel": float(f"{e:.3e}"), "mode": eng.mode, "samples": batch, "north_star_bound": 1e-3, "within_bound": bool(e <= 1e-3),
            "reference": "oracle/qformer.py (CPU fp32 restatement pinned to transformers 5.15.0's Blip2 classes), full depth 39 + 12 layers, "
                         "procedural weights, eval mode"}


def cpu_baseline_qformer(spec, batch=2, steps=2):
    """oracle/qformer.py (CPU fp32 restatement pinned to transformers' Blip2 classes) at the full blip2-opt-2.7b widths on this
    box's host cores: forward in train mode + classifier step, `steps` iterations of `batch` images."""
    from oracle import qformer as OQ
    from garbage_classification_rca_amd import q_former as QF
    n = effective_cores()
    torch.set_num_threads(n)
    print(f"[bench] cpu_baseline: Q-Former oracle on {n} host threads, batch {batch} ...", file=sys.stderr, flush=True)
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k, shp in QF.blip2_params(spec):
        if "LayerNorm" in k or "layer_norm" in k or "layernorm" in k:
            sd[k] = torch.ones(shp) if k.endswith("weight") else torch.zeros(shp)
        elif k.endswith("bias"):
            sd[k] = torch.zeros(shp)
        else:
            sd[k] = torch.randn(shp, generator=g) * 0.02
    lin = torch.nn.Linear(spec.q_dim, spec.n_classes)
    cfg = dict(v_layers=spec.v_layers, v_heads=spec.v_heads, patch=spec.patch, q_layers=spec.q_layers, q_heads=spec.q_heads,
               cross_freq=spec.cross_freq, hidden_drop=spec.hidden_drop, attn_drop=spec.attn_drop)
    cls = {"classifier.weight": lin.weight.detach(), "classifier.bias": lin.bias.detach()}
    batches = [(torch.randn(batch, 3, spec.image_size, spec.image_size, generator=g), torch.arange(batch).view(-1, 1) % 4) for _ in range(steps + 1)]
    count = [0]

    def feats(px):
        count[0] += 1
        return OQ.forward_logits(sd, cls, px, cfg, train=True, drop_seed=count[0])[1][:, 0, :]
    OQ.reference_loop(feats, lin, batches[:1])
    print("[bench] cpu_baseline: warm-up iteration done", file=sys.stderr, flush=True)
    t0 = time.time()
    OQ.reference_loop(feats, lin, batches[1:])
    dt = time.time() - t0
    return {"value": round(batch * steps / dt, 3), "unit": "samples/s", "cores": n, "kind": "port",
            "sample": f"oracle/qformer.py (PyTorch CPU fp32 restatement of the Blip2 vision tower + Q-Former + the q_former_training.py loop), "
                      f"full widths, batch {batch}, {steps} timed iterations after 1 warm-up, {n} threads"}


def launch_ranks(n: int, cmd=None) -> int:
    """`python bench.py --gpus N` with no launcher around it (WORLD_SIZE unset): start the N ranks ourselves -- the one-process-per-GPU
    replacement of the reference's single-process nn.DataParallel (main_both.py:386-388).  This parent has NOT touched the GPU (no HIP
    call, no torch.cuda call: it must not, a process that has initialised the GPU may neither exec nor be forked from on this pool); it
    starts N fresh children of this same script with RANK / LOCAL_RANK / WORLD_SIZE / LOCAL_WORLD_SIZE / MASTER_ADDR / MASTER_PORT set
    (what torch.distributed.run would set), relays rank 0's stdout (the ONE JSON line) and every rank's stderr, and returns non-zero if
    any child does -- ending the others first, by their PIDs, so that a rank that died before the rendezvous cannot leave the rest waiting."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:      # a free port for the rendezvous
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    base = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    base.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")               # dmabuf IPC: RCCL across processes needs it on this image
    cmd = cmd or [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    procs = []
    for r in range(n):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=(r == 0)))
    # rank 0's stdout is relayed: the JSON line to our stdout, anything else a library printed there (gloo's "[Gloo] Rank 0 is
    # connected ...") to stderr -- the contract is ONE line on stdout
    import threading

    def relay(pipe):
        for line in pipe:
            (sys.stdout if line.lstrip().startswith("{") else sys.stderr).write(line)
            sys.stdout.flush()
    relay_thread = threading.Thread(target=relay, args=(procs[0].stdout,), daemon=True)
    relay_thread.start()
    rc, alive = 0, set(range(n))
    while alive:
        for r in sorted(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"[bench] rank {r} exited with {code}: stopping the other ranks", file=sys.stderr, flush=True)
                for o in alive:
                    procs[o].terminate()
        time.sleep(0.05)
    relay_thread.join(timeout=10)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256, help="per-GPU batch (BASELINE config: 256)")
    ap.add_argument("--seq_len", type=int, default=64)
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--parity", action="store_true", help="measure the logits parity object even with --no_cpu_baseline (secondary lines)")
    ap.add_argument("--no_compliant", action="store_true", help="skip the second timed leg in the fastest mode that meets the 1e-3 logits bound")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32", "bf16x3", "bf16x3f"),
                    help="bf16 (the benchmarked configuration) | bf16x3: the fast <= 1e-3 mode -- fp32 storage / residual stream / LayerNorm / "
                         "attention, every nn.Linear as a three-pass split-bf16 product on the bf16 matrix cores | fp32: every GEMM on the fp32 matrix cores")
    ap.add_argument("--graph", default="auto", choices=("auto", "on", "off"),
                    help="replay the step's forward/backward launches from a HIP graph (training.GraphedTrainStep); auto = per-GPU batch <= 16 on one GPU "
                         "(the launch-bound regime: configs[0])")
    ap.add_argument("--frozen", action="store_true", help="time the frozen-backbone phase instead (reported separately)")
    ap.add_argument("--text_model", default="distilbert", help="distilbert (BASELINE configs[1]) | bert | roberta")
    ap.add_argument("--image_model", default="transformer_B16", help="transformer_B16 (configs[1]) | transformer_L16 | eff_v2_medium | eff_v2_large (configs[2]) | shuffle_net")
    ap.add_argument("--image_size", type=int, default=224)
    ap.add_argument("--cross_attention_only", action="store_true", help="configs[3]: ViT-L/16 + BERT-base, --seq_len 128")
    ap.add_argument("--workload", default="mmrca", choices=("mmrca", "qformer"),
                    help="mmrca: the headline MM-RCA train step | qformer: BASELINE configs[4], the BLIP-2 Q-Former classifier iteration")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32): mmrca -- loss, logits [batch, 4], "
                         "params (the parameters after the optimizer step, in state_dict order; a fixed, seeded sample of 4 Mi values when there "
                         "are more), bn_buffers (conv backbones: BatchNorm running statistics, likewise); qformer -- loss, classifier")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:       # no launcher: be one (before anything below touches the GPU)
        sys.exit(launch_ranks(args.gpus))
    if args.workload == "qformer":
        return bench_qformer(args)

    from garbage_classification_rca_amd import lib as L
    from garbage_classification_rca_amd import distributed as D
    from garbage_classification_rca_amd import engine as ENG
    from garbage_classification_rca_amd.multimodal_model import MM_RCA
    from garbage_classification_rca_amd.optim import FlatSGD
    from garbage_classification_rca_amd.procedural import synth_captions
    from garbage_classification_rca_amd.training import FusedCrossEntropy, hip_train_step
    import torch.distributed as dist

    rank, local, world = D.init_from_env("nccl")
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs a GPU: the MM-RCA product path has no CPU fallback"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    L.load()
    B, S = args.batch, args.seq_len

    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        model = MM_RCA(4, 0.6, 0.0, 0.7, 256, args.text_model, B, True, False, args.cross_attention_only,
                       image_model_name=args.image_model, dtype={"bf16": torch.bfloat16, "fp32": torch.float32}.get(args.dtype, args.dtype), device=dev, init_seed=0,
                       image_size=args.image_size)
    model.train()
    if not args.frozen:
        for p in model.parameters():
            p.requires_grad = True
    opt = FlatSGD(model, lr=1e-3, weight_decay=1e-2)
    crit = FusedCrossEntropy(None, 0.0)
    if args.dump_outputs:
        crit = LogitsKeepingCrossEntropy(crit)
    sync = D.GradSync(model.engine.arena.g, world) if world > 1 else None
    comm = None
    if world > 1:
        # self-diagnosis of the data-parallel exchange (the one collective of the path: gradient average before the optimizer)
        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones)
        ranks_seen = int(ones.item())
        assert ranks_seen == world, f"collective saw {ranks_seen} ranks, WORLD_SIZE={world}"
        comm = {"backend": dist.get_backend() + (" (RCCL)" if dist.get_backend() == "nccl" else ""), "ranks_seen": ranks_seen,
                "wire_dtype": "bf16" if sync.wire_dtype == torch.bfloat16 else "fp32", "bucket_bytes": sync.bucket_elems * 4}

    # synthetic pairs, resident in HBM before the timed region; a few distinct batches
    nb = 2
    ids, mask_host = synth_captions(B * nb, S, seed=4321 + rank)
    if args.text_model == "roberta":
        ids[mask_host == 0] = 1               # RoBERTa pads with id 1
    ids, mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask_host).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    images = torch.randn(B * nb, 3, args.image_size, args.image_size, device=dev, generator=gen)
    labels = (torch.arange(B * nb, device=dev) % 4).to(torch.int32)

    # packed token layouts of the batches, built from the HOST masks before the timed region (what a DataLoader-fed loop
    # does per batch without a device sync): the text encoder skips the padding rows (engine.TextPack)
    from garbage_classification_rca_amd.engine import make_text_pack
    from garbage_classification_rca_amd.training import PACK_TEXT
    from garbage_classification_rca_amd.engine import CLS_TAIL as E_CLS_TAIL
    packs = [make_text_pack(mask_host[k * B:(k + 1) * B], dev) if PACK_TEXT else None for k in range(nb)]
    live = sum(p.M for p in packs) / (nb * B * S) if all(p is not None for p in packs) else 1.0

    pack_in_loop = os.environ.get("MMRCA_BENCH_PACK_IN_LOOP", "1") == "1" and PACK_TEXT

    # auto = main_both.py's rule (--hip_graph auto): one GPU, batch <= 16 and images up to 224 x 224 -- where the step is launch-bound.  The
    # reference's own launch shape (EfficientNetV2-M @ 480, B = 16) is NOT: a replay runs it at the eager step's speed (488 vs 492
    # samples/s), and eager it can put its weight gradients on a side stream (509; conv_engine.SIDE_WGRAD) -- `--graph on` still captures it
    use_graph = args.graph == "on" or (args.graph == "auto" and B <= 16 and world == 1 and args.dtype in ("bf16", "bf16x3f")
                                       and B * args.image_size * args.image_size <= 16 * 224 * 224)
    graphed = None
    if use_graph:
        from garbage_classification_rca_amd.training import GraphedTrainStep
        graphed = GraphedTrainStep(model, crit, opt, sync, warmup=2)
        live = 1.0                             # the captured launches run the padded caption layout
    graph_on = [graphed is not None]

    def step(i):
        j = (i % nb) * B
        if graph_on[0]:
            return graphed(ids[j:j + B], mask[j:j + B], images[j:j + B], labels[j:j + B])
        # the packed layout is rebuilt from the host mask INSIDE the timed step, as a DataLoader-fed loop does per batch
        # (numpy + two small pinned async copies; MMRCA_BENCH_PACK_IN_LOOP=0 reuses the ones built above)
        pack = make_text_pack(mask_host[j:j + B], dev) if pack_in_loop else packs[i % nb]
        return hip_train_step(model, ids[j:j + B], mask[j:j + B], images[j:j + B], labels[j:j + B], crit, opt, sync,
                              text_pack=pack)

    with contextlib.redirect_stdout(io.StringIO()):
        for i in range(max(args.warmup, 4) if graphed is not None else args.warmup):    # (2 eager calls + the capture happen untimed)
            step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
        sync.bytes_reduced, sync.launches, sync.wait_events, sync.timing = 0, 0, [], True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        for i in range(args.steps):
            loss = step(i)
    host_enqueue = time.perf_counter() - t0          # host time to enqueue the steps (the GPU runs behind it)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:        # before the untimed steps below move the parameters on
        eng = model.engine
        outs = {"loss": loss, "logits": crit.logits, "params": param_sample(eng.arena, eng.param_keys)}
        if eng.conv is not None:
            stats = [t.reshape(-1) for k, t in sorted(eng.conv.buffers.items()) if not k.endswith("num_batches_tracked")]
            stats = torch.cat(stats)
            outs["bn_buffers"] = stats[torch.from_numpy(flat_sample(stats.numel())).to(dev)]
        dump_outputs(args.dump_outputs, outs)
    if world > 1:
        sync.timing = False
        wait_ms = sum(e0.elapsed_time(e1) for e0, e1 in sync.wait_events)
        comm.update({"bytes_per_step": int(sync.bytes_reduced // args.steps), "allreduce_launches_per_step": sync.launches // args.steps,
                     "allreduce_wait_ms_per_step": round(wait_ms / args.steps, 3),
                     "wait_definition": "time the compute stream spends blocked in GradSync.finish() (HIP events around its waits): the part of the "
                                        "exchange NOT hidden behind the backward"})

    # What one step costs the HOST: `host_enqueue` above includes the time launch calls block on a full hardware queue (the host runs
    # ahead of the GPU), so it tracks the step time.  The cost proper is the time to enqueue ONE step onto an EMPTY queue (device
    # synchronised first; a step's ~500 packets fit the queue, so nothing blocks): measured here, outside the timed region.
    host_idle = []
    with contextlib.redirect_stdout(io.StringIO()):
        for i in range(3):
            torch.cuda.synchronize()
            th = time.perf_counter()
            step(i)
            host_idle.append(time.perf_counter() - th)
    torch.cuda.synchronize()
    host_idle_ms = sorted(host_idle)[len(host_idle) // 2] * 1e3

    # Roofline of the dominant kernel (the MFMA GEMM).  The timed region above overlaps kernels on several HIP streams
    # (weight-gradient GEMMs beside the input-gradient chain, text beside vision encoder), so per-launch durations there
    # are not separable.  The same steps are therefore replayed on ONE stream right after the timed region, with every
    # MFMA GEMM launch bracketed by HIP events on its launch stream; `achieved` = sum(2MNK) / sum(durations).
    eng = model.engine
    graph_on[0] = False                        # the per-launch measurements below bracket eager launches with HIP events
    saved_streams = (eng._side_v, eng._side_t, eng._side, eng._text_stream)
    eng._side_v = eng._side_t = eng._side = eng._text_stream = None
    from garbage_classification_rca_amd import conv_engine as CE
    saved_conv_side, CE.SIDE_WGRAD = CE.SIDE_WGRAD, False      # (the conv backbones' weight gradients too: ONE stream for the per-launch timings)
    replay = max(2, min(4, args.steps))
    with contextlib.redirect_stdout(io.StringIO()):
        step(0)
        torch.cuda.synchronize()
        L.GEMM_PROFILE = []
        L.KERNEL_PROFILE = []
        ts0 = time.perf_counter()
        for i in range(replay):
            step(i)
        torch.cuda.synchronize()
        serial_ms = (time.perf_counter() - ts0) / replay * 1e3
        cprof = None
        if eng.conv is not None:       # conv image encoder: a third replay with every launch's ALGORITHMIC bytes and HIP-event time
            L.CONV_PROFILE = []
            if os.environ.get("MMRCA_BENCH_SHAPES") == "1":
                L.GEMM_SHAPES = []
            for i in range(replay):
                step(i)
            torch.cuda.synchronize()
            cprof, L.CONV_PROFILE = L.CONV_PROFILE, None
            if L.GEMM_SHAPES is not None:      # per-shape table of every GEMM of the conv step (stderr), for kernel tuning
                tab = {}
                for (Mg, Ng, Kg, al, bl, ac, nb_, e0, e1) in L.GEMM_SHAPES:
                    d_ = tab.setdefault((Mg, Ng, Kg, al, bl, ac), [0, 0.0, nb_])
                    d_[0] += 1; d_[1] += e0.elapsed_time(e1)
                L.GEMM_SHAPES = None
                print("[bench] GEMMs of the conv step by shape (M, N, K, a_layout, b_layout, accum): calls/step, us/call, ms/step, TB/s, TFLOP/s", file=sys.stderr)
                for k_, (n_, ms_, nb_) in sorted(tab.items(), key=lambda kv: -kv[1][1])[:60]:
                    us = ms_ / n_ * 1e3
                    print(f"[bench]   {k_}: {n_ // replay} x {us:7.1f} us = {ms_ / replay:6.2f} ms   {nb_ / (us * 1e-6) / 1e12:5.2f} TB/s   "
                          f"{2.0 * k_[0] * k_[1] * k_[2] / (us * 1e-6) / 1e12:6.1f} TFLOP/s", file=sys.stderr)
    prof, L.GEMM_PROFILE = L.GEMM_PROFILE, None
    kprof, L.KERNEL_PROFILE = L.KERNEL_PROFILE, None
    eng._side_v, eng._side_t, eng._side, eng._text_stream = saved_streams
    CE.SIDE_WGRAD = saved_conv_side
    if world > 1 and os.environ.get("MMRCA_CHECK_REPLICAS") == "1":
        # data-parallel invariant: every rank applied the same averaged gradient, so the replicas are bit-identical
        chk = eng.arena.p.double().sum().view(1)
        lo, hi = chk.clone(), chk.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        assert float(hi - lo) == 0.0, f"replicas diverged: {float(lo)} vs {float(hi)}"
        if rank == 0:
            print(f"[bench] replicas identical after {args.warmup + args.steps + replay + 1} steps (param checksum {float(chk):.6f}); "
                  f"all-reduced {sync.bytes_reduced / 1e6:.1f} MB in total", file=sys.stderr, flush=True)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    final_loss = float(loss.item())

    if rank == 0:
        print(f"[bench] timed region done: {elapsed / args.steps * 1e3:.2f} ms/step", file=sys.stderr, flush=True)
        flops = sum(p[0] for p in prof)
        ms = sum(p[2].elapsed_time(p[3]) for p in prof)
        by_kind = {}
        for f, kind, e0, e1, _shape in prof:
            d = by_kind.setdefault(kind, [0.0, 0.0, 0])
            d[0] += f; d[1] += e0.elapsed_time(e1); d[2] += 1
        achieved = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        # HBM-side bytes per GEMM launch: PMC counters cannot be read in-process, so the committed summary of the two
        # rocprofv3 --pmc passes over THIS command (tools/pmc_traffic.py) is quoted, next to the algorithmic bytes
        # (operands once + outputs once, from the launch shapes of this run)
        traffic, traffic_src = None, None
        import glob as _glob
        for pmc_json in sorted(_glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r[0-9][0-9]_pmc_hbm_traffic.json")), reverse=True):
            pmc_name = os.path.basename(pmc_json)         # newest round first
            if os.path.exists(pmc_json):
                with open(pmc_json) as fh:
                    pj = json.load(fh)
                # the summary names the GEMM sources it was measured on (tools/pmc_traffic.py); a kernel edit since then makes it stale
                if pj.get("gemm_sources_sha256") != gemm_sources_sha256():
                    traffic_src = (f"profiles/{pmc_name} is STALE (measured on other GEMM sources: {str(pj.get('gemm_sources_sha256'))[:12]} vs "
                                   f"{gemm_sources_sha256()[:12]} now); not quoted -- re-run tools/r06_artifacts.sh")
                    break
                traffic = pj.get("gemm_hbm_bytes_per_launch_mean")
                traffic_src = (f"profiles/{pmc_name} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, x2 gfx950 fetch correction; "
                               f"GEMM sources sha256 {pj['gemm_sources_sha256'][:12]} = this build)")
                break
        alg = []
        for f, kind, e0, e1, shp in prof:
            Mg, Ng, Kg, actg = shp
            out_b = 4 if kind[2] else 2
            alg.append(2.0 * (Mg * Kg + Ng * Kg) + out_b * Mg * Ng * (2 if actg in (L.ACT_GELU, L.ACT_GELU_SAVE_GRAD, L.ACT_MUL) else 1))
        alg_mean = sum(alg) / max(len(alg), 1)
        if os.environ.get("MMRCA_BENCH_SHAPES") == "1":       # in-situ per-shape table (stderr), for kernel tuning
            by_shape = {}
            for f, kind, e0, e1, shp in prof:
                d = by_shape.setdefault((kind, shp), [0.0, 0.0, 0])
                d[0] += f; d[1] += e0.elapsed_time(e1); d[2] += 1
            for (kind, shp), v in sorted(by_shape.items(), key=lambda kv: -kv[1][1]):
                print(f"[bench] gemm a{kind[0]}b{kind[1]}acc{kind[2]} M={shp[0]} N={shp[1]} K={shp[2]} act={shp[3]}: {v[2] // replay}/step, "
                      f"{v[1] / v[2] * 1e3:.0f} us, {v[0] / (v[1] * 1e-3) / 1e12:.0f} TF, {v[1] / replay:.2f} ms/step", file=sys.stderr, flush=True)
        value = B * world * args.steps / elapsed
        gemm_peak = PEAK_BF16_TFLOPS if args.dtype in ("bf16", "bf16x3", "bf16x3f") else PEAK_F32_TFLOPS
        fwd_gflop = FWD_GFLOP_PER_SAMPLE if (args.text_model, args.image_model, S) == ("distilbert", "transformer_B16", 64) else (
            145.5 if (args.text_model, args.image_model, S) == ("bert", "transformer_L16", 128) else float("nan"))
        train_flop_per_sample = (fwd_gflop * (1.0 if args.frozen else 3.0)) * 1e9

        # attention kernels (K3): algorithmic QK^T + PV FLOPs (forward 4 S^2 d per (b,h); backward 2.5x that: five products,
        # recomputation not counted) over the HIP-event time of the mha_* launches of the replay
        lens = mask_host.reshape(nb, B, S).sum(-1).astype("float64")             # live caption lengths per batch
        def attn_flops(kind, meta, batch_idx):
            Bm, Hm, Sm, dm, packed = meta
            s2 = float((lens[batch_idx] ** 2).sum()) if packed else float(Bm) * Sm * Sm
            return 4.0 * Hm * dm * s2 * (1.0 if kind == "mha_fwd" else 2.5)
        esz = 2 if args.dtype == "bf16" else 4
        def attn_bytes(kind, meta, batch_idx):
            # algorithmic HBM bytes of one launch: forward reads Q, K, V and writes O (+ the fp32 log-sum-exp); backward reads
            # Q, K, V, O, dO and writes dQ, dK, dV -- 4 resp. 8 tensors of tokens x H x d elements
            Bm, Hm, Sm, dm, packed = meta
            tokens = float(lens[batch_idx].sum()) if packed else float(Bm) * Sm
            return tokens * Hm * (dm * esz * (4.0 if kind == "mha_fwd" else 8.0) + 4.0)
        abytes = {"mha_fwd": 0.0, "mha_bwd": 0.0}
        akind = {"mha_fwd": [0.0, 0.0, 0], "mha_bwd": [0.0, 0.0, 0]}
        hk = {"head_fwd": [0.0, 0], "head_bwd": [0.0, 0]}
        per_step = max(1, len(kprof) // replay)
        for idx, (kind, meta, e0, e1) in enumerate(kprof):
            dt_ms = e0.elapsed_time(e1)
            if kind in akind:
                akind[kind][0] += attn_flops(kind, meta, (idx // per_step) % nb); akind[kind][1] += dt_ms; akind[kind][2] += 1
                abytes[kind] += attn_bytes(kind, meta, (idx // per_step) % nb)
            elif kind in hk:
                hk[kind][0] += dt_ms; hk[kind][1] += 1
        a_fl, a_ms = akind["mha_fwd"][0] + akind["mha_bwd"][0], akind["mha_fwd"][1] + akind["mha_bwd"][1]
        tf = lambda fl, ms_: round(fl / (ms_ * 1e-3) / 1e12, 1) if ms_ > 0 else None
        attention = {"what": "fused attention kernels (QK^T, softmax, PV and their backward) of both encoders; algorithmic "
                             "FLOPs = 4 S^2 d per (b,h) forward, 10 S^2 d backward (recomputation not counted)",
                     "achieved": tf(a_fl, a_ms), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(a_fl / (a_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4) if a_ms > 0 else None,
                     "fwd_TFLOPs": tf(*akind["mha_fwd"][:2]), "bwd_TFLOPs": tf(*akind["mha_bwd"][:2]),
                     "ms_per_step": round(a_ms / replay, 3), "launches_per_step": (akind["mha_fwd"][2] + akind["mha_bwd"][2]) // replay,
                     "north_star_target_frac": 0.40,
                     # the roofline that binds at these sizes (S = 197 / 64, d = 64): one pass over Q, K, V, O is 98 FLOP per byte
                     # forward -- at the 8 TB/s HBM peak the kernels cannot exceed hbm_ceiling_frac of the MFMA peak
                     "hbm": {"bytes_per_step": int((abytes["mha_fwd"] + abytes["mha_bwd"]) / replay),
                             "fwd_TBps": round(abytes["mha_fwd"] / (akind["mha_fwd"][1] * 1e-3) / 1e12, 2) if akind["mha_fwd"][1] > 0 else None,
                             "bwd_TBps": round(abytes["mha_bwd"] / (akind["mha_bwd"][1] * 1e-3) / 1e12, 2) if akind["mha_bwd"][1] > 0 else None,
                             "peak_TBps": 8.0,
                             "frac_of_hbm_peak": round((abytes["mha_fwd"] + abytes["mha_bwd"]) / (a_ms * 1e-3) / 8e12, 4) if a_ms > 0 else None,
                             "hbm_ceiling_frac_of_mfma_peak": round(a_fl / ((abytes["mha_fwd"] + abytes["mha_bwd"]) / 8e12) / 1e12 / PEAK_BF16_TFLOPS, 4)
                             if abytes["mha_fwd"] + abytes["mha_bwd"] > 0 else None}}
        # fused RCA head (K1): latency and HBM rate (4,112 B per sample + 190 KB of weights per launch)
        d_i, d_t = eng.d_img, eng.d_txt
        head_bytes = B * ((d_i + d_t) * 2 + 16) + 94820 * 2
        hf = hk["head_fwd"][0] / max(hk["head_fwd"][1], 1) * 1e3
        hb = hk["head_bwd"][0] / max(hk["head_bwd"][1], 1) * 1e3
        head = {"what": "fused MM-RCA head (L2 norm, 2 self-attention + 2 reverse cross-attention blocks of 16x16, LN+ReLU, concat, "
                        "dropout, classifier), one launch per direction", "fwd_us": round(hf, 1), "bwd_us": round(hb, 1),
                "algorithmic_bytes_fwd": head_bytes, "fwd_GBps": round(head_bytes / (hf * 1e-6) / 1e9, 2) if hf > 0 else None,
                "peak_GBps": 8000.0, "frac_of_hbm_peak": round(head_bytes / (hf * 1e-6) / 8e12, 6) if hf > 0 else None,
                "bound": "launch latency (2.9 MFLOP and 4.1 KB per sample)"}
        # whole step on EXECUTED FLOPs: GEMM launches (2MNK) + attention (algorithmic) per step; the nominal 3x-forward
        # figure (which also counts rows the dead-row elimination never computes) is kept under its own key
        exec_flop_per_step = flops / replay + a_fl / replay
        step_s = elapsed / args.steps
        out = {
            "metric": "train samples/sec (image+text pairs), MM-RCA ViT-B16+DistilBERT", "value": round(value, 2),
            "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": {"bf16": "bf16", "fp32": "f32", "bf16x3": "bf16x3 (fp32 values as two bf16 planes, three MFMA passes per product)",
                                                "bf16x3f": "bf16x3f (forward: fp32 values as two bf16 planes, three MFMA passes per product; backward: bf16)"}[args.dtype], "data": "synthetic",
            "config": {"workload": "MM_RCA --reverse" + (" --cross_attention_only " if args.cross_attention_only else " ")
                       + {"transformer_B16": "ViT-B/16", "transformer_L16": "ViT-L/16", "eff_v2_medium": "EfficientNetV2-M", "eff_v2_large": "EfficientNetV2-L",
                          "shuffle_net": "ShuffleNetV2-x2.0"}[args.image_model] + " + "
                       + {"distilbert": "DistilBERT", "bert": "BERT-base", "roberta": "RoBERTa-base"}[args.text_model] + ", "
                       + ("frozen-backbone" if args.frozen else "fine-tune")
                       + f" train step (fwd+loss+bwd+allreduce+SGD), {args.image_size}x{args.image_size} images, {S}-token captions",
                       "per_gpu_batch": B, "global_batch": B * world, "seq_len": S, "image": args.image_size, "parallelism": f"dp{world}",
                       "optimizer": "sgd lr=1e-3 wd=1e-2", "random_init": True, "caption_rows_processed": round(live, 3),
                       "dead_row_elimination": {"class_token_tail": bool(E_CLS_TAIL), "packed_captions": bool(PACK_TEXT) and graphed is None,
                                                "note": "identical logits and gradients; MMRCA_CLS_TAIL=0 MMRCA_PACK_TEXT=0 runs every row"}, "final_loss": round(final_loss, 4),
                       # schema 2 (round 6): `host_enqueue_ms_per_step` has its rounds-1..4 meaning again -- host wall time inside
                       # the timed loop; round 5 had reused the name for the empty-queue measurement, which now has a name of its own
                       "host_schema": 2,
                       "host_enqueue_ms_per_step": round(host_enqueue / args.steps * 1e3, 2),
                       "host_enqueue_idle_queue_ms_per_step": round(host_idle_ms, 2),
                       "host_enqueue_note": "host_enqueue_idle_queue_ms_per_step: host time to enqueue one step onto an EMPTY queue (median of 3, each "
                                            "after a device sync) = what the Python + ctypes + hipLaunchKernel calls cost.  host_enqueue_ms_per_step: "
                                            "host wall time per step inside the timed loop (rounds 1-4's meaning; BENCH_r05 carried the idle-queue "
                                            "number under this key), which also counts launch calls blocking on a full queue, i.e. it follows the "
                                            "step time while the host is ahead",
                       "hip_graph": (None if graphed is None else {"replays_in_timed_region": args.steps, "graphs": len(graphed._graphs),
                                                                   "outside_the_graph": "input copies, mask-epoch word, loss copy, SGD step, gradient memset"}),
                       **({"x3_backward_passes": {"weight_gradient": ENG.X3_WGRAD_PASSES, "input_gradient": ENG.X3_DGRAD_PASSES,
                                                  "note": "3 / 3 = every product with all three plane pairs (default: gradients 3e-5 from float64); fewer "
                                                          "= opt-in cheaper backward (MMRCA_X3_*_PASSES), forward logits unchanged, gradients at 5e-3 .. 1e-2"}}
                          if args.dtype == "bf16x3" else {})},
            "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": gemm_peak, "unit": "TFLOP/s",
                         "frac": round(achieved / gemm_peak, 4), "traffic": traffic if args.dtype == "bf16" else None,
                         "traffic_unit": "bytes per GEMM KERNEL launch (mean; a call that AUTO splits into whole persistent rounds + a 128x128 tail is two "
                                         "kernel launches there and one in launches_per_step / algorithmic_bytes_per_launch)", "traffic_source": traffic_src,
                         "algorithmic_bytes_per_launch": round(alg_mean),
                         "kernel": ("bf16 16x16x32 MFMA GEMMs: gemm_p256_k (persistent 256x256 tiles) and gemm_mfma_k1s (128x128 tiles) for the "
                                    "forward / input gradient, gemm_mfma256_k + splitk_reduce256_k (256x256 split-K) for the weight gradient; "
                                    "every nn.Linear fwd/dgrad/wgrad") if args.dtype == "bf16" else
                                   ("the same bf16 MFMA kernels in their bf16x3 form (gemm_x3.hip): three plane-pair passes per product into one fp32 "
                                    "accumulator; achieved / flops count the EXECUTED bf16 matrix-core work = 3 x 2MNK") if args.dtype in ("bf16x3", "bf16x3f") else
                                   "fp32 32x32x2 MFMA GEMM gemm_gen_k (128x64 tiles, three-level fp32 summation); every nn.Linear fwd/dgrad/wgrad",
                         "launches_per_step": len(prof) // replay, "gemm_ms_per_step": round(ms / replay, 3),
                         "measured_in": f"single-stream replay of {replay} steps after the timed region ({round(serial_ms, 2)} ms/step serialized)",
                         "by_layout_TFLOPs": {f"a{k[0]}b{k[1]}acc{k[2]}": round(v[0] / (v[1] * 1e-3) / 1e12, 1) for k, v in by_kind.items() if v[1] > 0},
                         "flops_counted": "achieved = executed 2MNK of the GEMM launches / their HIP-event time; whole_step_* = executed "
                                          "GEMM + attention FLOPs per step / wall time of the timed region",
                         "whole_step_executed_TFLOPs": round(exec_flop_per_step / step_s / 1e12, 2),
                         "whole_step_frac": round(exec_flop_per_step / step_s / 1e12 / gemm_peak, 4),
                         "whole_step_nominal_model_TFLOPs": round(value / world * train_flop_per_sample / 1e12, 2),
                         "attention": attention, "head": head},
        }
        if cprof is not None:
            # The conv step is HBM-shaped (BatchNorm / depthwise / squeeze-excitation passes, wide-output 1x1 GEMMs): its binding
            # roofline is bytes, not FLOPs.  Algorithmic bytes = every operand an op must read once + every result it must write once,
            # from the launch arguments (lib._CONV_BYTES), summed over the step as it is decomposed into kernels today.
            fam = {}
            for name, nbytes, e0, e1 in cprof:
                d = fam.setdefault(name, [0, 0.0, 0])
                d[0] += nbytes; d[2] += 1
                if e0 is not None:
                    d[1] += e0.elapsed_time(e1)
            gemm_ms = sum(p[2].elapsed_time(p[3]) for p in prof) / replay
            tot_b = sum(v[0] for v in fam.values()) / replay
            table = {}
            for name, (nb, ms_, n) in sorted(fam.items(), key=lambda kv: -kv[1][0]):
                ms1 = (ms_ / replay) if ms_ > 0 else (gemm_ms if name.startswith("GEMM") else None)
                table[name] = {"GB_per_step": round(nb / replay / 1e9, 2), "launches_per_step": n // replay, "ms_per_step": None if ms1 is None else round(ms1, 2),
                               "TBps": None if not ms1 else round(nb / replay / (ms1 * 1e-3) / 1e12, 2)}
            floor_ms = tot_b / 8e12 * 1e3
            out["roofline"]["hbm"] = {
                "bound": "hbm", "what": "whole train step of the conv image encoder + text encoder: algorithmic HBM bytes of every launch (operands read once + results "
                                        "written once, per launch arguments; every launch of every family -- all GEMMs included since round 5 -- timed by HIP events) against the 8 TB/s peak",
                "algorithmic_GB_per_step": round(tot_b / 1e9, 2), "floor_ms_at_8TBps": round(floor_ms, 2), "floor_ms_at_6.3TBps_achievable": round(tot_b / 6.3e12 * 1e3, 2),
                "step_ms": round(elapsed / args.steps * 1e3, 2), "achieved_TBps": round(tot_b / (elapsed / args.steps) / 1e12, 3), "peak_TBps": 8.0,
                "frac": round(floor_ms / (elapsed / args.steps * 1e3), 4), "families": table,
                "note": "frac = byte floor / measured step: how far the step is from the roofline that binds it; the MFMA frac above covers the GEMM launches only"}
        if comm is not None:
            out["comm"] = comm
        if (not args.no_cpu_baseline or args.parity) and world == 1:
            with contextlib.redirect_stdout(io.StringIO()):
                out["parity"] = parity_check(model, ids, mask, images)
        if not args.no_cpu_baseline and world == 1:
            if args.dtype == "bf16" and not args.frozen and not args.no_compliant:
                eng.release_buffers()
                out["compliant"] = compliant_leg(args, dev, out["parity"])
            out["cpu_baseline"] = cpu_baseline(seq_len=S, text_model=args.text_model, image_model=args.image_model, image_size=args.image_size)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
