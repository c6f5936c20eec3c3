#!/usr/bin/env python3
"""bench.py -- FA2 forward+backward on MI355X, BASELINE.json's headline metric.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c3|c5|c1]
                    [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes the last step's outputs when
--dump-outputs is given and prints the result line (metric, value, unit, ms_per_step,
...).  Everything else this file measures -- the per-launch roofline region, the other
configs (extra_configs), the CPU baselines -- takes runs of its own and is behind
--full; without it those entries of the line are null.

--dump-outputs DIR writes what the timed path computed in its last timed step, the
arrays its caller receives (O, LSE, dQ, dK, dV of this rank), as DIR/<name>.npy in
float32 (DIR/<name>.rank<r>.npy on ranks r > 0).  An array above DUMP_MAX_ELEMS
elements is stored as a fixed sample of its flattened elements (dump_indices: seeded,
the same for every run and build), so a dump stays below 64 MB.  The inputs are seeded,
so two builds run with the same arguments are compared output for output.

One *step* = the FA2 forward (O, LSE) + backward (dQ, dK, dV; fa2_backward's launch
plan) over one batch of synthetic fp32 inputs already resident in HBM (harness
distribution: torch.manual_seed(42 + rank), torch.rand for Q, K, V; dO = ones as
the reference harness uses, test_flash_attention2.py:220-232), fp16 tiles on MFMA.

Workloads (BASELINE.json configs):
  * N = 1 (default c3): B4_H16_S2048_D64, the config the metric is quoted on
    ("... at S=2048 D=64", the headline roofline config);
  * N > 1 (default c5): B64_H16_S2048_D64 strong-scaled over the ranks, the
    north star's 1/2/4/8-GPU curve: every rank takes the contiguous B*H slice
    fa2_shard_range gives it (one process per GPU, no data-path collective;
    RCCL only carries the timing barrier and the max over ranks).  The N = 1 line
    of a --full run also times C5 on one GPU (extra_configs.c5_1gpu) as the curve's
    anchor.
`--gpus N` without a launcher starts N ranks itself (torch.distributed.run, before
any GPU call in this process) and exits with their status.

value = algorithmic fwd+bwd FLOPs of the job (14*B*H*S^2*D) / the max over ranks of
the K-step wall time (barrier + synchronize on both sides).
With --full:
roofline = the dominant kernel launch's algorithmic FLOPs / its mean duration, timed
live with HIP events on the launch's own stream around every launch of a second
K-step region, against the dense fp16 MFMA peak; step_frac = the whole step's
algorithmic rate (value) against the same peak; traffic = the dominant launch's HBM
bytes from the committed rocprofv3 PMC summary (profiles/pmc_summary.json), null
unless that profile was taken of this very build (fa2_build_id).
cpu_baseline (rank 0, N = 1) = PyTorch-CPU SDPA fwd+bwd (north_star's baseline) on
the host's usable cores, 2 warm-ups then the median of >= 3 runs, on whole heads of
the workload; the harness's compute_reference and the C restatement of the oracle
(oracle/fa2_oracle.c) are timed beside it, and C1 (config #1, the reference's
"CPU reference path") as well.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "cuda-flash-attention_amd"))

MFMA_F16_PEAK_TFLOPS = 2500.0   # MI355X dense fp16/bf16 MFMA (MI355X_MICROARCH.md)
MFMA_F32_PEAK_TFLOPS = 157.3    # fp32 MFMA = fp32 vector peak
HBM_PEAK_GBPS = 8000.0

WORKLOADS = {
    # name: (B, H, S, D, per_rank)
    "c3": (4, 16, 2048, 64, True),
    "c5": (64, 16, 2048, 64, False),
    "c1": (2, 8, 512, 64, True),
}
METRIC = "FA2 fwd+bwd TFLOPS & HBM GB/s (% of gfx950 roofline) at S=2048 D=64"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# --dump-outputs: at most this many elements of one array (5 arrays x 8 MB of float32)
DUMP_MAX_ELEMS = 2 * 1024 * 1024


def dump_indices(name: str, n: int):
    """The flattened elements of an n-element output `name` that a dump holds: all of them
    (None) up to DUMP_MAX_ELEMS, else DUMP_MAX_ELEMS sorted indices drawn (with
    replacement) from a generator seeded by the name and n alone."""
    if n <= DUMP_MAX_ELEMS:
        return None
    seed = [n] + [ord(c) for c in name]
    return np.sort(np.random.default_rng(seed).integers(0, n, size=DUMP_MAX_ELEMS, dtype=np.int64))


def dump_outputs(torch, out_dir: str, rank: int, arrays: dict):
    """Write the device tensors `arrays` as float32 out_dir/<name>.npy (see the module
    docstring); the caller has synchronised the device."""
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        idx = dump_indices(name, flat.numel())
        if idx is not None:
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        a = flat.to(torch.float32).cpu().numpy()
        a = a if idx is not None else a.reshape(tuple(t.shape))
        np.save(os.path.join(out_dir, f"{name}.npy" if rank == 0 else f"{name}.rank{rank}.npy"), a)


# kernel-name prefixes in the rocprofv3 PMC summary
PMC_PREFIX = {"fwd": ("fa2_fwd_f16", "fa2_fwd_hs"), "dq": ("fa2_bwd_dq_f16", "fa2_bwd_dq_hs"),
              "dkdv": ("fa2_bwd_dkdv_f16", "fa2_bwd_dkdv_hs"), "bwd32": ("fa2_bwd_f32",)}


def traffic_from_profile(kernel: str, D: int, S: int, heads: int, build_id: str, path: str | None = None):
    """HBM bytes per launch of `kernel` (FETCH_SIZE x 2 + WRITE_SIZE, gfx950-corrected)
    from the committed rocprofv3 PMC summary profiles/pmc_summary.json (tools/pmc.sh ->
    tools/pmc_summary.py), or None when it does not cover this kernel and shape, or was
    taken of another build than the loaded library (its _meta.build_id against
    fa2_build_id(): a rebuilt kernel never inherits an old traffic figure)."""
    path = path or os.path.join(ROOT, "profiles", "pmc_summary.json")
    try:
        with open(path) as f:
            summ = json.load(f)
    except (OSError, ValueError):
        return None
    meta = summ.get("_meta", {})
    if meta.get("S") != S or meta.get("D") != D or meta.get("heads") != heads:
        return None
    if meta.get("build_id") != build_id:
        log(f"profiles/pmc_summary.json is of build {meta.get('build_id')}, the library is {build_id}: traffic null")
        return None
    for name, ent in summ.items():
        if name.startswith(PMC_PREFIX.get(kernel, ("?",))) and (f"<{D}," in name or f"<{D}>" in name):
            try:
                return float(ent["hbm_bytes_per_launch"])
            except (KeyError, TypeError):
                return None
    return None


# ---------------------------------------------------------------------------
# CPU baseline
# ---------------------------------------------------------------------------
def usable_cpus():
    """(cpus this process may run on: affinity capped by the cgroup CPU quota, affinity
    count, quota or None)"""
    aff = len(os.sched_getaffinity(0))
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
        if q != "max":
            quota = max(1, -(-int(q) // int(p)))
    except (OSError, ValueError):
        pass
    return (min(aff, quota) if quota else aff), aff, quota


def cpu_model():
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for line in out.splitlines():
            if line.startswith("Model name:"):
                return line.split(":", 1)[1].strip()
    except (OSError, subprocess.SubprocessError):
        pass
    return "unknown"


def _median_runs(fn, warm=2, runs=3, budget_s=8.0):
    """2 warm-ups, then >= `runs` timed runs (more while within budget); median s"""
    for _ in range(warm):
        fn()
    ts = []
    t_all = time.perf_counter()
    while len(ts) < runs or (time.perf_counter() - t_all < budget_s and len(ts) < 10):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), len(ts)


def cpu_baseline(S, D, heads):
    """PyTorch-CPU SDPA fwd+bwd on `heads` heads of (S, D) -- the north star's
    baseline -- with the harness's compute_reference (matmul, /sqrt(D), softmax,
    matmul; autograd with dO = ones: test_flash_attention2.py:197-232) and the
    oracle's C port beside it; plus the C1 (B2_H8_S512_D64) fwd+bwd entry."""
    import torch

    threads, aff, quota = usable_cpus()
    torch.set_num_threads(threads)
    flops = 14.0 * heads * S * S * D
    gen = torch.Generator().manual_seed(42)
    q, k, v = (torch.rand(1, heads, S, D, generator=gen) for _ in range(3))

    def sdpa(q=q, k=k, v=v):
        qq, kk, vv = (x.clone().requires_grad_() for x in (q, k, v))
        o = torch.nn.functional.scaled_dot_product_attention(qq, kk, vv)
        o.backward(torch.ones_like(o))

    def compute_reference(q=q, k=k, v=v):
        qq, kk, vv = (x.clone().requires_grad_() for x in (q, k, v))
        s = torch.matmul(qq, kk.transpose(-2, -1)) / (D ** 0.5)
        o = torch.matmul(torch.softmax(s, dim=-1), vv)
        o.backward(torch.ones_like(o))

    t_sdpa, n_sdpa = _median_runs(sdpa)
    t_ref, n_ref = _median_runs(compute_reference)
    out = {"value": round(flops / t_sdpa / 1e12, 5), "unit": "TFLOPS", "cores": threads, "kind": "reference",
           "sample": f"{heads} heads x (S={S}, D={D}) fp32 torch SDPA fwd+bwd (autograd, dO = ones), "
                     f"median of {n_sdpa} after 2 warm-ups: {t_sdpa:.3f} s; {threads} threads",
           "cpu_model": cpu_model(), "affinity_cpus": aff, "cgroup_cpu_quota": quota,
           "compute_reference": {"value": round(flops / t_ref / 1e12, 5), "unit": "TFLOPS", "median_s": round(t_ref, 4),
                                 "runs": n_ref}}
    try:
        from oracle import c_oracle, fa2_oracle as fo

        qn, kn, vn = fo.harness_inputs(1, heads, S, D, seed=42)
        don = np.ones_like(qn)
        c_oracle.forward(qn[:, :1, :64], kn[:, :1, :64], vn[:, :1, :64], 1)  # load / build outside the timing

        def port():
            o, lse = c_oracle.forward(qn, kn, vn, nthreads=threads)
            c_oracle.backward(qn, kn, vn, o, don, lse, nthreads=threads)

        t_port, n_port = _median_runs(port, warm=1, runs=3, budget_s=4.0)
        out["oracle_port"] = {"value": round(flops / t_port / 1e12, 5), "unit": "TFLOPS", "kind": "port",
                              "median_s": round(t_port, 4), "runs": n_port, "source": "oracle/fa2_oracle.c"}
    except Exception as e:  # reported, never required
        log("oracle port baseline failed:", e)
    # C1 = B2_H8_S512_D64: the reference's CPU-runnable config (#1), fwd+bwd
    B1, H1, S1, D1 = 2, 8, 512, 64
    q1, k1, v1 = (torch.rand(B1, H1, S1, D1, generator=gen) for _ in range(3))
    t1, n1 = _median_runs(lambda: sdpa(q1, k1, v1))
    out["c1_B2_H8_S512_D64"] = {"value": round(14.0 * B1 * H1 * S1 * S1 * D1 / t1 / 1e12, 5), "unit": "TFLOPS",
                                "median_s": round(t1, 5), "runs": n1, "what": "torch SDPA fwd+bwd"}
    return out


# ---------------------------------------------------------------------------
# GPU timing helpers
# ---------------------------------------------------------------------------
def time_config(fa2amd, torch, dev, B, H, S, D, prec, fwd_only, iters=50, warmup=3, warmup_ms=250.0, dist=None,
                total_heads=None, do_randn=False):
    """Mean ms of fwd (+ bwd) on one synthetic config (harness distribution), events on
    the current stream; returns (ms, tflops, gbps) with the algorithmic counts.  With
    `dist` each rank runs its own B x H slice, the region is bracketed by barriers, ms
    is the max over ranks and the rates count `total_heads` heads.  do_randn: dO ~ N(0, 1)
    (seed 43) instead of the harness's ones."""
    gen = torch.Generator().manual_seed(7)
    q, k, v = (torch.rand(B, H, S, D, generator=gen).to(dev) for _ in range(3))
    do = (torch.randn(B, H, S, D, generator=torch.Generator().manual_seed(43)).to(dev) if do_randn
          else torch.ones_like(q))
    o, lse = torch.empty_like(q), torch.empty(B, H, S, device=dev)
    dq, dk, dv, dl = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q), torch.empty(B, H, S, device=dev)

    def once():
        fa2amd.forward(q, k, v, prec, out=o, lse=lse)
        if not fwd_only:
            fa2amd.backward(q, k, v, o, do, lse, prec, dq=dq, dk=dk, dv=dv, delta_buf=dl)

    n, tw = 0, time.perf_counter()  # untimed: W runs and >= warmup_ms of load (clock ramp)
    while n < warmup or (time.perf_counter() - tw) * 1e3 < warmup_ms:
        once()
        n += 1
        if n >= warmup and n % 8 == 0:
            torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    if dist is not None:
        dist.barrier()
        torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / iters
    if dist is not None:
        ms = all_max(torch, dist, dev, ms)
    heads = total_heads or B * H
    flops = (4.0 if fwd_only else 14.0) * heads * S * S * D
    nbytes = (16.0 * S * D + 4.0 * S if fwd_only else 48.0 * S * D + 8.0 * S) * heads
    return ms, flops / ms / 1e9, nbytes / ms / 1e6


def all_max(torch, dist, dev, x):
    """max over ranks of a host float (RCCL needs a device tensor, gloo a host one)"""
    t = torch.tensor([x], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def roof_entry(ms, tf, gbps, S, fwd_only):
    """A point against its binding roofline: algorithmic intensity (fwd S/4, fwd+bwd
    14 S / 48 FLOP/B at fp32 I/O) below the fp16 MFMA ridge (peak FLOP/s over HBM B/s)
    means HBM-bound."""
    intensity = (S / 4.0) if fwd_only else (14.0 * S / 48.0)
    ridge = MFMA_F16_PEAK_TFLOPS * 1e3 / HBM_PEAK_GBPS
    fm, fh = tf / MFMA_F16_PEAK_TFLOPS, gbps / HBM_PEAK_GBPS
    bound = "hbm" if intensity < ridge else "mfma"
    return {"ms": round(ms, 4), "tflops": round(tf, 2), "hbm_gbps": round(gbps, 1), "frac_mfma": round(fm, 4),
            "frac_hbm": round(fh, 4), "bound": bound, "frac": round(fh if bound == "hbm" else fm, 4)}


SWEEP_S = (512, 1024, 2048, 4096)


def sweep_sharded(fa2amd, torch, dev, dist, world, rank):
    """north_star's sweep, B2_H8_S{512..4096}_D64 fwd+bwd, with its 16 heads sharded
    over the ranks (contiguous B x H slices, no collective on the data path)."""
    first, heads = fa2amd.shard_range(16, world, rank)
    out = {}
    for S in SWEEP_S:
        ms, tf, gbps = time_config(fa2amd, torch, dev, 1, heads, S, 64, "fp16", False, dist=dist, total_heads=16)
        out[str(S)] = roof_entry(ms, tf, gbps, S, False)
    return out


def extras(fa2amd, torch, dev):
    """north_star's sweep, BASELINE.json's other GPU configs (C2, C4, bf16 C3) and the
    one-GPU anchor of the C5 scaling curve, each against its roofline."""
    out = {"sweep_B2_H8_D64_fp16_fwdbwd": {}}
    for S in SWEEP_S:
        ms, tf, gbps = time_config(fa2amd, torch, dev, 2, 8, S, 64, "fp16", False)
        out["sweep_B2_H8_D64_fp16_fwdbwd"][str(S)] = roof_entry(ms, tf, gbps, S, False)
    ms, tf, gbps = time_config(fa2amd, torch, dev, 8, 16, 4096, 128, "fp16", True, iters=20)
    out["c4_B8_H16_S4096_D128_fp16_fwd"] = roof_entry(ms, tf, gbps, 4096, True)
    ms, tf, gbps = time_config(fa2amd, torch, dev, 4, 16, 2048, 64, "bf16", False)
    out["c3_B4_H16_S2048_D64_bf16_fwdbwd"] = roof_entry(ms, tf, gbps, 2048, False)
    # the headline's step with a realistic upstream gradient: dO ~ N(0, 1) (seed 43) instead
    # of the harness's dO = ones (test_flash_attention2.py:220-232); at the power cap the
    # operand bits set the clock, so the data dependence is reported beside the headline
    ms, tf, gbps = time_config(fa2amd, torch, dev, 4, 16, 2048, 64, "fp16", False, do_randn=True)
    out["c3_dO_randn"] = roof_entry(ms, tf, gbps, 2048, False)
    ms, tf, gbps = time_config(fa2amd, torch, dev, 2, 8, 512, 64, "fp32", False)
    out["c2_B2_H8_S512_D64_fp32_fwdbwd"] = {"ms": round(ms, 4), "tflops": round(tf, 2),
                                            "frac_mfma_f32": round(tf / MFMA_F32_PEAK_TFLOPS, 4)}
    ms, tf, gbps = time_config(fa2amd, torch, dev, 64, 16, 2048, 64, "fp16", False, iters=10)
    out["c5_1gpu_B64_H16_S2048_D64_fp16_fwdbwd"] = roof_entry(ms, tf, gbps, 2048, False)
    try:
        out["c3_host_api_pcie_inclusive"] = host_api_entry(fa2amd, 4, 16, 2048, 64)
    except Exception as e:  # reported, never required
        log("c3 host-API entry failed:", e)
        out["c3_host_api_pcie_inclusive"] = None
    return out


def host_api_entry(fa2amd, B, H, S, D, runs=3, num_devices=1):
    """The reference's host-buffer boundary (host_flash_attention2_{forward,backward}_fp16
    semantics through fa2_{forward,backward}_host): H2D, kernels, D2H per call, the
    heads sharded over `num_devices` GPUs.  Wall time of fwd + bwd from host arrays
    (PCIe-inclusive; reported beside the HBM-resident `value`, never as it) and the
    kernel-only ms the calls report.  The result arrays are allocated once and reused,
    as a caller looping over batches does (fresh ones add the page faults of their
    first touch to every call)."""
    gen = np.random.default_rng(3)
    q, k, v = (gen.random((B, H, S, D), dtype=np.float32) for _ in range(3))
    do = np.ones_like(q)
    o, lse = np.empty_like(q), np.empty((B, H, S), np.float32)
    dq, dk, dv = np.empty_like(q), np.empty_like(q), np.empty_like(q)
    walls, kms = [], []
    for i in range(runs + 1):
        t0 = time.perf_counter()
        _, _, kf = fa2amd.forward_host(q, k, v, "fp16", num_devices=num_devices, out=o, lse=lse)
        _, _, _, kb = fa2amd.backward_host(q, k, v, o, do, lse, "fp16", num_devices=num_devices, dq=dq, dk=dk, dv=dv)
        if i:  # the first call pays the device scratch allocation and the first touch
            walls.append(time.perf_counter() - t0)
            kms.append(kf + kb)
    fa2amd.host_release()
    wall, km = statistics.median(walls), statistics.median(kms)
    flops = 14.0 * B * H * S * S * D
    nbytes = 4 * B * H * S * D * (3 + 1 + 5 + 3) + 4 * B * H * S * 2
    return {"wall_ms": round(wall * 1e3, 3), "tflops_wall": round(flops / wall / 1e12, 2), "kernel_ms": round(km, 4),
            "tflops_kernels": round(flops / (km * 1e-3) / 1e12, 2), "h2d_d2h_bytes": nbytes,
            "pcie_gbps": round(nbytes / wall / 1e9, 1), "num_devices": num_devices,
            "what": f"fa2_forward_host + fa2_backward_host from host numpy buffers, B*H over {num_devices} device(s) "
                    f"(H2D, kernels, D2H per call; result arrays reused), median of {runs}"}


# ---------------------------------------------------------------------------
# launcher
# ---------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n):
    """`--gpus N` with no launcher: start N ranks under torch.distributed.run (as the
    driver does) from this process, which touches no GPU, and return their status."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--warmup-ms", type=float, default=400.0,
                    help="keep warming (untimed) until at least this much wall time has passed: the "
                         "power-capped MI355X needs ~0.2 s of load to reach its steady clock")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=None,
                    help="default: c3 on one GPU, c5 (strong-scaled) on more")
    ap.add_argument("--precision", choices=["fp16", "fp32", "bf16"], default="fp16")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's O, LSE, dQ, dK, dV as DIR/<name>.npy "
                         "(float32; a fixed seeded sample of arrays above DUMP_MAX_ELEMS elements)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline figure: the per-launch roofline region, "
                         "the extra configs and the CPU baselines")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the S sweep / C2 / C4 / C5 extra configs")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher and rank plumbing only (gloo, no GPU work): the JSON line without numbers")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "0"))
    if world == 0:
        if args.gpus > 1:
            return spawn_ranks(args.gpus)
        world = 1
    elif args.gpus != world:
        log(f"--gpus {args.gpus} but WORLD_SIZE {world}: measuring the {world} launched ranks")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    workload = args.workload or ("c3" if world == 1 else "c5")
    B, H, S, D, per_rank = WORKLOADS[workload]

    import torch
    import torch.distributed as dist

    # FA2_BENCH_REHEARSE=1: every rank on cuda:0 over gloo -- rehearses the N > 1 path
    # (barriers, max over ranks, sharded sweep) on a one-GPU box; never used for numbers
    rehearse = os.environ.get("FA2_BENCH_REHEARSE") == "1" or args.dry_run
    if world > 1:
        if rehearse:
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    if per_rank:
        heads, Bl, Hl = B * H, B, H
    else:
        import fa2amd

        _, heads = fa2amd.shard_range(B * H, world, rank)
        Bl, Hl = 1, heads
    total_heads = B * H * world if per_rank else B * H
    parallelism = f"bh-shard{world}" if world > 1 else "single"
    workload_name = f"B{B}_H{H}_S{S}_D{D} {args.precision}-tile fwd+bwd" + (
        " per rank" if per_rank else (f", B*H split over {world} ranks" if world > 1 else ""))

    if args.dry_run:
        if world > 1:
            t = all_max(torch, dist, None, float(rank))
            dist.barrier()
        if rank == 0:
            print(json.dumps({"metric": METRIC, "value": None, "unit": "TFLOPS", "n_gpus": world, "dry_run": True,
                              "scaling": "weak" if per_rank else "strong", "heads_rank0": heads,
                              "config": {"workload": workload_name, "parallelism": parallelism}}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return 0

    import fa2amd

    local_dev = 0 if rehearse else local
    dev = torch.device("cuda", local_dev)
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(42 + rank)
    q = torch.rand(Bl, Hl, S, D, generator=gen).to(dev)
    k = torch.rand(Bl, Hl, S, D, generator=gen).to(dev)
    v = torch.rand(Bl, Hl, S, D, generator=gen).to(dev)
    do = torch.ones_like(q)
    o = torch.empty_like(q)
    lse = torch.empty(Bl, Hl, S, device=dev)
    dl = torch.empty(Bl, Hl, S, device=dev)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    stream = torch.cuda.current_stream(dev)
    prec = args.precision
    # fa2_backward's plan on full grids at fp16 (>= 8 blocks of 32 rows per CU, D <= 64
    # as at C3 / C5): the dQ kernel (Δ fused) then the dK/dV kernel.  The roofline region
    # times those two launches separately through their split entry points (the same
    # kernel instances fa2_backward launches); otherwise the backward as one unit.
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    split_bwd = prec == "fp16" and D <= 64 and heads * ((S + 31) // 32) >= 8 * ncu
    kernels = ["fwd", "dq", "dkdv"] if split_bwd else ["fwd", "bwd"]

    def step(ev=None):
        def mark(i):
            if ev is not None:
                ev[i].record(stream)
        mark(0)
        fa2amd.forward(q, k, v, prec, out=o, lse=lse, stream=stream)
        mark(1)
        if ev is not None and split_bwd:
            fa2amd.backward_dq_delta(q, k, v, o, do, lse, dl, dq, stream=stream)
            mark(2)
            fa2amd.backward_dkdv(q, k, v, do, lse, dl, dk, dv, stream=stream)
            mark(3)
            return
        fa2amd.backward(q, k, v, o, do, lse, prec, dq=dq, dk=dk, dv=dv, delta_buf=dl, stream=stream)
        mark(2)

    # Untimed warmup: at least W steps AND at least --warmup-ms of load.  With 5 warmup
    # steps (~2 ms) the clock is still ramping when the timed region starts and a 20-step
    # region reads ~16 % slow (r01: 0.408 ms/step vs 0.343 at steady clock).
    warm_steps = 0
    tw = time.perf_counter()
    while warm_steps < args.warmup or (time.perf_counter() - tw) * 1e3 < args.warmup_ms:
        for _ in range(10 if warm_steps >= args.warmup else 1):
            step()
            warm_steps += 1
        if warm_steps >= args.warmup:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)

    # timed region 1 -> value: K steps exactly as a caller issues them (no event between
    # kernels: a timing event serialises the stream)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    if world > 1:
        dist.barrier()
        elapsed = all_max(torch, dist, dev, elapsed)

    # what the last timed step left in the caller's buffers, before anything else runs
    if args.dump_outputs:
        dump_outputs(torch, args.dump_outputs, rank, {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv})

    per_head = S * S * D
    flops = 14.0 * per_head * total_heads * args.steps
    tflops = flops / elapsed / 1e12
    hbm_bytes = (48.0 * S * D + 8.0 * S) * total_heads * args.steps  # fwd 16SD+4S, bwd 32SD+4S per head
    ms_per_step = elapsed / args.steps * 1e3

    roof = None
    if args.full:
        # timed region 2 -> roofline: the same K steps with HIP events around every launch
        # on its stream (the isolated per-launch durations rocprofv3's kernel trace reports)
        events = [[torch.cuda.Event(enable_timing=True) for _ in range(len(kernels) + 1)] for _ in range(args.steps)]
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for s in range(args.steps):
            step(events[s])
        torch.cuda.synchronize(dev)
        elapsed_ev = time.perf_counter() - t1
        kms = {name: float(np.mean([events[s][i].elapsed_time(events[s][i + 1]) for s in range(args.steps)]))
               for i, name in enumerate(kernels)}

        # dominant launch and its algorithmic FLOPs per head: fwd 4 S^2 D; dK/dV 8 S^2 D (S,
        # dP, dV, dK: four of the backward's five GEMMs); dQ 2 S^2 D (its S and dP recompute
        # earns nothing); a whole backward 10 S^2 D
        alg = {"fwd": 4.0, "dq": 2.0, "dkdv": 8.0, "bwd": 10.0}
        dom = max(kms, key=kms.get)
        dom_flops = alg[dom] * per_head * heads
        peak = MFMA_F16_PEAK_TFLOPS if prec in ("fp16", "bf16") else MFMA_F32_PEAK_TFLOPS
        achieved = dom_flops / (kms[dom] * 1e-3) / 1e12
        traffic = traffic_from_profile(dom if prec != "fp32" else "bwd32", D, S, heads, fa2amd.build_id())
        roof = {"bound": "mfma", "kernel": dom, "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                "frac": round(achieved / peak, 4), "traffic": traffic,
                # the whole step against the same peak: 14 S^2 D per head per step / ms_per_step
                "step_frac": round(tflops / peak, 4),
                "kernel_ms": {n: round(x, 4) for n, x in kms.items()},
                "bwd_tflops": round(10.0 * per_head * heads / (sum(kms[n] for n in kms if n != "fwd") * 1e-3) / 1e12,
                                    2),
                "ms_per_step_with_events": round(elapsed_ev / args.steps * 1e3, 4)}

    cpu = None
    extra = None
    if args.full and rank == 0 and world == 1 and not args.no_extras:
        extra = extras(fa2amd, torch, dev)
    elif args.full and world > 1 and not args.no_extras:
        extra = {f"sweep_B2_H8_D64_fp16_fwdbwd_sharded{world}": sweep_sharded(fa2amd, torch, dev, dist, world, rank)}
        # the reference's host-buffer semantics at the N-GPU point: rank 0 shards C5 over
        # all N devices through fa2_*_host (one host thread per device) while the other
        # ranks wait at the barrier (rehearsals on one GPU skip it)
        torch.cuda.synchronize(dev)
        dist.barrier()
        if rank == 0 and not rehearse:
            Bc, Hc, Sc, Dc, _ = WORKLOADS["c5"]
            # reported, never required: a failure (fewer visible devices, memory beside the
            # other ranks' buffers) is logged and recorded as null, and rank 0 still reaches
            # the barrier the other ranks wait at
            try:
                extra["c5_host_api_pcie_inclusive"] = host_api_entry(fa2amd, Bc, Hc, Sc, Dc, runs=2,
                                                                     num_devices=world)
            except Exception as e:
                log("c5 host-API entry failed:", e)
                extra["c5_host_api_pcie_inclusive"] = None
        dist.barrier()
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            cpu = cpu_baseline(S, D, 16)
        except Exception as e:  # the baseline is reported, never required
            log("cpu baseline failed:", e)

    if rank == 0:
        line = {
            "metric": METRIC,
            "value": round(tflops, 3),
            "unit": "TFLOPS",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "warmup_steps_run": warm_steps,
            "ms_per_step": round(ms_per_step, 4),
            "full": args.full,
            "higher_is_better": True,
            "scaling": "weak" if per_rank else "strong",
            "vs_baseline": None,
            "dtype": prec,
            "data": "synthetic (torch.rand U[0,1) Q/K/V as the reference harness draws them, dO = ones)",
            "config": {"workload": workload_name, "batch": B, "heads": H, "seq_len": S, "head_dim": D,
                       "parallelism": parallelism},
            "hbm_gbps": round(hbm_bytes / elapsed / 1e9, 2),
            "roofline": roof,
            "cpu_baseline": cpu,
            "extra_configs": extra,
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
