"""GPU: bench.py's N > 1 code path on one GPU, so that it cannot rot while no 8-GPU node runs it: a process group over RCCL
with a world of one, the all-gather of 96-byte partials inside vdf_msm_sharded (the host's collective ordered on the
library's stream), the local point sum, the strong-scaling sub-record with its exactness check and the JSON contract; and the
plain run (no --full) with the output it dumps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_rehearses_the_collective_path():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29571", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    # a fresh child process (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--rehearse-collective", "--strong", "--strong-log2n", "20",
                        "--no-prove", "--no-cpu", "--steps", "3", "--warmup", "2"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, "stdout carries exactly one JSON line"
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline"):
        assert key in line, key
    assert line["n_gpus"] == 1 and line["scaling"] == "weak" and line["value"] > 0 and "workload" in line["config"]
    s = line["strong_2_20"]
    assert s["exact"] is True                       # [sum s_i k_i] G, through partial -> RCCL all-gather -> point sum
    assert s["n_gpus"] == 1 and s["scaling"] == "strong" and s["points_per_gpu"] == 1 << 20 and s["total_points"] == 1 << 20
    assert "vdf_msm_sharded" in s["path"] and s["value"] > 0
    assert line["self_check"]["ok"] is True


def test_plain_run_times_its_steps_and_dumps_the_exact_point(tmp_path):
    """A run without --full: one timed region of exactly --steps steps, the contract's headline keys, and --dump-outputs writing
    the last step's point.  Over [k_i]G generators that point must be [sum s_i k_i] G for the seeded scalars."""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    import torch
    log2n, steps = 16, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--bases", "dlog", "--log2n", str(log2n), "--steps", str(steps),
                        "--warmup", "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, "stdout carries exactly one JSON line"
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "GPoints/s" and line["dtype"] == "u32" and "prove_step" not in line and "cpu_baseline" not in line
    got = np.load(tmp_path / "msm_result.npy")
    assert got.dtype == np.float64 and got.shape == (2, 8)
    xy = tuple(sum(int(got[r_, k]) << (32 * k) for k in range(8)) for r_ in range(2))
    # the scalars bench.py draws for rank 0, drawn again
    n = 1 << log2n
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    sc = torch.randint(-(2**63), 2**63 - 1, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    sc[:, 3] &= 0x3FFFFFFFFFFFFFFF
    k = bench._sum_s_k(sc.cpu().numpy().view("<u8"), bench._dlogs(7, 0, n)) % bench._Q
    assert xy == bench._scalar_mul_generator(k, bench._P)
