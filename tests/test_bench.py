"""bench.py's plain run and --dump-outputs: the sampling rule on the CPU, and on the GPU one
short plain run whose dumped arrays must be bitwise what the same calls give here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_indices_fixed_sample():
    """whole arrays up to DUMP_MAX_ELEMS; above it a sorted, in-range sample that depends on
    the name and size alone (so two runs, or two builds, store the same elements)"""
    cap = bench.DUMP_MAX_ELEMS
    assert bench.dump_indices("o", cap) is None
    n = 4 * 16 * 2048 * 64
    a, b = bench.dump_indices("dq", n), bench.dump_indices("dq", n)
    assert a.dtype == np.int64 and a.shape == (cap,)
    assert np.array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and a[0] >= 0 and a[-1] < n
    assert not np.array_equal(a, bench.dump_indices("dk", n))
    # five arrays of a dump stay below 64 MB
    assert 5 * cap * 4 < 64 * 1024 * 1024


def test_dump_outputs_files(tmp_path):
    """float32 <name>.npy per array: whole (with its shape) when small, the sampled flat
    elements when large, rank-suffixed on ranks > 0"""
    small = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    n = bench.DUMP_MAX_ELEMS + 1000
    big = torch.arange(n, dtype=torch.float32) * 0.5
    bench.dump_outputs(torch, str(tmp_path / "d"), 0, {"small": small, "big": big})
    s = np.load(tmp_path / "d" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (2, 3, 4)
    assert np.array_equal(s, small.numpy().astype(np.float32))
    b = np.load(tmp_path / "d" / "big.npy")
    assert b.dtype == np.float32 and b.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.array_equal(b, big.numpy()[bench.dump_indices("big", n)])
    bench.dump_outputs(torch, str(tmp_path / "d"), 1, {"small": small})
    assert (tmp_path / "d" / "small.rank1.npy").exists()


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    """`bench.py --steps 2 --warmup 1 --dump-outputs DIR` on C1: the line is the plain one
    (nothing behind --full ran), and DIR holds O, LSE, dQ, dK, dV of the step, bitwise what
    fa2amd gives for the bench's seeded inputs (every path is deterministic)."""
    import fa2amd

    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--warmup-ms", "0", "--workload", "c1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["steps"] == 2 and line["full"] is False
    assert line["metric"] == bench.METRIC and line["unit"] == "TFLOPS" and line["dtype"] == "fp16"
    assert line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["extra_configs"] is None

    B, H, S, D, _ = bench.WORKLOADS["c1"]
    gen = torch.Generator().manual_seed(42)
    q, k, v = (torch.rand(B, H, S, D, generator=gen).cuda() for _ in range(3))
    do = torch.ones_like(q)
    o, lse = fa2amd.forward(q, k, v, "fp16")
    dq, dk, dv = fa2amd.backward(q, k, v, o, do, lse, "fp16")
    torch.cuda.synchronize()
    assert sorted(os.listdir(out)) == ["dk.npy", "dq.npy", "dv.npy", "lse.npy", "o.npy"]
    for name, want in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == tuple(want.shape)
        assert np.array_equal(got, want.cpu().numpy()), name
