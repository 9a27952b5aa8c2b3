"""bench.py --gpus N without a launcher around it: the script starts its own N ranks (bench.launch_ranks), one process per GPU -- the
replacement of the reference's single-process nn.DataParallel (main_both.py:386-388).  On this one-GPU box the two ranks share the card
and gloo stands in for RCCL (MMRCA_DIST_BACKEND), as in the torchrun rehearsal of test_engine_gpu.py."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_starts_its_own_two_ranks_and_prints_one_line():
    env = dict(os.environ, MMRCA_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--no_cpu_baseline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]       # ONE line on stdout: library chatter is relayed to stderr
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["warmup"] == 2 and d["scaling"] == "weak"
    assert d["comm"]["ranks_seen"] == 2 and d["comm"]["bytes_per_step"] > 0
    assert d["config"]["global_batch"] == 512


@pytest.mark.gpu
def test_bench_dumps_the_outputs_of_its_last_timed_step(tmp_path):
    """--dump-outputs DIR: loss, logits and (a seeded sample of) the parameters after the last timed step, float32, at most 64 MB.
    Batch 8 replays a HIP graph under --graph auto, where the logits are the captured buffer every replay rewrites; --graph off launches
    every step from Python.  Either way the dumped logits must give the dumped loss of the same step."""
    import numpy as np
    for graph in ("auto", "off"):
        out = tmp_path / graph
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8", "--steps", "3", "--warmup", "2",
               "--no_cpu_baseline", "--graph", graph, "--dump-outputs", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        assert (d["config"]["hip_graph"] is not None) == (graph == "auto")
        files = sorted(p.name for p in out.iterdir())
        assert files == ["logits.npy", "loss.npy", "params.npy"], files
        assert sum(p.stat().st_size for p in out.iterdir()) <= 64 << 20
        a = {f[:-4]: np.load(out / f) for f in files}
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
        assert a["logits"].shape == (8, 4) and a["loss"].shape == (1,) and a["params"].shape == (4 << 20,)
        assert abs(float(a["loss"][0]) - d["config"]["final_loss"]) < 1e-4
        z = a["logits"].astype(np.float64)                 # mean cross entropy against bench.py's labels (arange % 4)
        ce = np.mean(np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1) - z[np.arange(8), np.arange(8) % 4])
        assert abs(ce - float(a["loss"][0])) < 1e-5, (ce, a["loss"])
