#!/usr/bin/env python
"""bench.py — headline benchmark of the SfM dense-compute path on MI355X.

Primary line (BASELINE.json metric, config C3/C4): image-pairs matched/sec —
all 32,896 pairs of 257 synthetic images x 4096 SuperPoint-like 256-d
descriptors (int8-quantised, resident in HBM), BF-L2 + ratio test 0.75 on the
MFMA kernel, through the product API ``dist.match_all_pairs_sharded``.  With N
ranks (one process per GPU) the pairs are split over the ranks (strong scaling
over the fixed dataset) and the int16 match graph is all-gathered by the
C-ABI's RCCL collective (``sfmhip_allgather``), chunk by chunk, overlapped with
the match launches.

A plain run (``bench.py --gpus N --steps K --warmup W``) does only that: it sets
up, warms up, times the K steps, writes the last step's outputs with
``--dump-outputs DIR`` and prints the result line.  Everything below runs only
with ``--full``.

Secondary lines (``--full``; ``secondary`` list of the same JSON object):
  * TSDF Mvoxel/sec (C5), z-slab sharded over ranks;
  * BA obs/sec: DLT + residual + FD Jacobian (C3 BA workload), DLT and FD-J
    kernels timed apart, with the numpy/scipy CPU baseline;
  * N = 1 only: C2 (64 x 2048 SIFT-128), the exact float matching mode on C3,
    the north-star composite (C3 match + C3 DLT/BA evaluation + C5 TSDF vs the
    summed CPU wall-clock), DDA traversal, plenoxel render, vq, geometric
    verification, PnP and the plenoxel training step.
CPU baselines (``--full``) follow BASELINE.md §2: 1 warm-up + median of 3 timed
runs, with every host thread the box gives us and again with 1 thread
(``value_1thread``).

Usage:  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
        python bench.py --full [--steps K] [--warmup W] [--no-cpu-baseline] [--skip-secondary]
        python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import contextlib
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_IMG, M_KPT, DIM = 257, 4096, 256
C2_IMG, C2_KPT, C2_DIM = 64, 2048, 128
TSDF_R, TSDF_F = 256, 257
BA_PAIRS, BA_OBS = 256, 4096
PEAK_INT8_TOPS = 5000.0       # MI355X dense int8 MFMA (MI355X_MICROARCH.md: 2x bf16 2.5 PF)
PEAK_HBM_GBS = 8000.0         # HBM3E spec
MATCH_CHUNKS = 4              # N>1: match launches per step, each overlapped with the previous all-gather
PEAK_FP32_TFLOPS = 157.3      # vector fp32
PEAK_FP64_TFLOPS = 78.6       # fp64 (vector and v_mfma_f64 matrix peaks are the same on MI355X)
DLT_FLOP_PER_OBS = 1200.0     # 6x4 f64 DLT null vector, ~1.2 kflop per observation
FDJ_BYTES_PER_OBS = 200.0     # 40 B in + 16 B residual + 144 B Jacobian values
DLT_BYTES_PER_OBS = 64.0      # 2 x 2 f64 pixels in, 4 f64 out
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "r6", "traffic.json")
VERIFY_WORK_FILE = os.path.join(ROOT, "profiles", "r3", "verify_work.json")
# Algorithmic fp64 flop counts of the secondary lines (DESIGN.md §5 derives each):
F_5PT = 18_000.0        # one 5-point solve: 5x9 null space, 10x20 constraint matrix, 10x10 solve, degree-10 roots
F_SAMPSON = 38.0        # one Sampson error (E x1, E^T x2, x2^T E x1, 4 squares, quotient) per model and point
F_TRI_POSE = 1_250.0    # recoverPose: one DLT point (1.2 kflop) + two depth tests, per candidate pose
F_EPNP = 90_000.0       # one EPnP hypothesis on 5 points (12x12 M^T M, Jacobi eigenvectors, 3 beta sets + GN, Procrustes)
F_PNP_SCORE = 30.0      # one reprojection + squared error per hypothesis and point
F_LM_OBS = 290.0        # one CvLevMarq pass per inlier: projection + analytic 2x6 Jacobian + J^T J / J^T e
F_BA_J_OBS = 500.0      # one scipy 2-point FD Jacobian row pair per observation: 10 projections
F_BA_STEP_OBS = 650.0   # the damped GN direction, the 2-D subspace products and one trial residual, per observation
BA_BYTES_OBS = 64.0     # compulsory per solve: X (24 B) + pixel (16 B) read, X (24 B) written


def pmc_traffic(kind: str, frac: float = 1.0, src: str = TRAFFIC_FILE):
    """HBM bytes per step of the dominant kernel from the committed PMC passes
    (counters need their own rocprofv3 runs), scaled to this rank's share."""
    try:
        with open(src) as f:
            t = json.load(f)
        return t[kind]["bytes_per_step"] * frac
    except (OSError, KeyError, ValueError):
        return None


def verify_work():
    """Data-dependent work terms measured on the bench scenes by
    tools/count_verify_work.py (mean 5-point models per RANSAC sample, LM
    projection passes per PnP refinement)."""
    try:
        with open(VERIFY_WORK_FILE) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, steps, warmup, barrier):
    """W untimed steps, then K steps bracketed by barrier + synchronize; returns
    (wall seconds over K steps, per-step kernel ms from HIP events)."""
    for _ in range(warmup):
        fn(None)
    torch.cuda.synchronize()
    barrier()
    ev = []
    t0 = time.perf_counter()
    for _ in range(steps):
        ev.append(fn(True))
    torch.cuda.synchronize()
    barrier()
    wall = time.perf_counter() - t0
    kms = [a.elapsed_time(b) for a, b in ev if a is not None]
    return wall, kms


def max_over_ranks(x: float, world: int, device) -> float:
    if world == 1:
        return x
    t = torch.tensor([x], dtype=torch.float64,
                     device=device if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


# ---------------------------------------------------------------------------
# CPU baseline methodology: host threads, 1 warm-up + median of 3
def host_threads() -> int:
    """Threads this process may use on the host: OMP_NUM_THREADS when the
    environment sets it (the GPU box sets 16, this job's share of the host: its
    rules size worker pools to that share), else the whole affinity mask."""
    try:
        return max(1, int(os.environ["OMP_NUM_THREADS"]))
    except (KeyError, ValueError):
        return max(1, len(os.sched_getaffinity(0)))


def host_info() -> dict:
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"cpu_count": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)),
            "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "threads_used": host_threads(), "model": model,
            "numpy": np.__version__, "torch_threads": torch.get_num_threads()}


@contextlib.contextmanager
def blas_limit(n: int):
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        yield
        return
    with threadpool_limits(limits=int(n)):
        yield


def cpu_median(fn, reps: int = 3):
    fn()                                     # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def cpu_leg(run, n_all: int, n_one: int, unit: str, kind: str, sample: str, scale: float = 1.0) -> dict:
    """``run(k, threads)`` does k units of the CPU path with that many threads
    (BLAS pool and/or a thread pool over independent pieces).  Timed with every
    host thread on k = n_all units and with 1 thread on k = n_one units; the
    rates are units/s times ``scale`` (units -> metric unit)."""
    nt = host_threads()
    with blas_limit(nt):
        t_all, ts_all = cpu_median(lambda: run(n_all, nt))
    with blas_limit(1):
        t_one, ts_one = cpu_median(lambda: run(n_one, 1))
    return {"value": n_all / t_all * scale, "unit": unit, "cores": nt, "kind": kind,
            "value_1thread": n_one / t_one * scale, "sample": sample,
            "timing": f"median of 3 after 1 warm-up: {nt} threads on {n_all} units "
                      f"({', '.join(f'{t:.3f}' for t in ts_all)} s), 1 thread on {n_one} units "
                      f"({', '.join(f'{t:.3f}' for t in ts_one)} s)"}


def pool_map(fn, items, threads: int):
    if threads <= 1:
        return [fn(i) for i in items]
    with cf.ThreadPoolExecutor(threads) as ex:
        return list(ex.map(fn, items))


# ---------------------------------------------------------------------------
def match_cpu_leg(qcpu, pairs, sample, n_one=3):
    """Oracle (numpy GEMM form on exact int8 values + top-2 + exact ratio) on a
    spread sample of the same pairs.  All threads: pairs over a thread pool,
    one BLAS thread per worker (numpy drops the GIL in the GEMM and the
    reductions; one pair at a time on a 16-thread BLAS leaves the top-2
    passes single-threaded: 83 vs 108 ms per pair for 16 vs 1 threads in
    profiles/r2/bench.json)."""
    from oracle import match as om

    def one(i):
        a, b = (int(v) for v in pairs[i])
        om.bf_match_q(qcpu[a], qcpu[b], (3, 4))

    def run(k, nt):
        with blas_limit(1):
            pool_map(one, sample[:k], nt)
    return cpu_leg(run, len(sample), n_one, "pairs/s", "port",
                   f"oracle.match.bf_match_q on {len(sample)} pairs over a thread pool (all threads) / {n_one} "
                   f"pairs (1 thread), spread over the pair list")


def match_cpu_leg_gemm(xcpu, pairs, sample, n_one=3):
    """The headline's CPU baseline ("matching: numpy oracle GEMM-form"):
    oracle.match.bf_match_gemm_f32 — f32 A @ B.T + norms, argpartition top two, ratio
    test — on a spread sample of the same float descriptors, pairs over a thread pool
    with one BLAS thread per worker (all threads) and on one thread."""
    from oracle import match as om

    def one(i):
        a, b = (int(v) for v in pairs[i])
        om.bf_match_gemm_f32(xcpu[a], xcpu[b], (3, 4))

    def run(k, nt):
        with blas_limit(1):
            pool_map(one, sample[:k], nt)
    return cpu_leg(run, len(sample), n_one, "pairs/s", "port",
                   f"numpy f32 GEMM form (oracle.match.bf_match_gemm_f32: A @ B.T + norms, argpartition top-2, "
                   f"ratio 0.75) on {len(sample)} pairs over a thread pool (all threads) / {n_one} pairs (1 thread), "
                   f"spread over the pair list")


def match_cpu_leg_exact(xcpu, pairs, sample, n_one=2):
    """The exact-float oracle (oracle.match.bf_match_exact: f32 descriptors, squared L2
    summed in f64 in k order, top-2, exact ratio) on a spread sample of the same pairs,
    pairs over a thread pool with one BLAS thread per worker."""
    from oracle import match as om

    def one(i):
        a, b = (int(v) for v in pairs[i])
        om.bf_match_exact(xcpu[a], xcpu[b], (3, 4))

    def run(k, nt):
        with blas_limit(1):
            pool_map(one, sample[:k], nt)
    return cpu_leg(run, len(sample), n_one, "pairs/s", "port",
                   f"oracle.match.bf_match_exact on {len(sample)} pairs over a thread pool (all threads) / {n_one} "
                   f"pairs (1 thread), spread over the pair list")


def spread(n_total: int, n: int):
    return [(i * 997) % n_total for i in range(n)]


def c2_line(sfm, syn, device, args, barrier, cpu=True):
    """Config C2: 64 images x 2048 SIFT-128 (integer 0..255 values), all 2016
    pairs, MODE_SIFT quantisation, ratio 0.75; roofline 2.165 T int8-ops."""
    sdist = importlib.import_module("3d_reconstruction_amd.dist")
    x = syn.sift_like(C2_IMG, C2_KPT, C2_DIM, seed=0, device=device)
    bank = sfm.DescriptorBank.from_float(x, mode=sfm.MODE_SIFT)
    del x
    pairs = sfm.all_pairs(C2_IMG)
    pdev = torch.from_numpy(pairs).to(device)
    P = len(pairs)

    def step(record):
        e0, e1 = events() if record else (None, None)
        if record:
            e0.record()
        sdist.match_all_pairs_sharded(bank, pdev, chunks=1, after_compute=(e1.record if record else None))
        return (e0, e1)

    wall, kms = timed(step, max(args.steps, 10), 2, barrier)
    ms = wall / max(args.steps, 10) * 1e3
    k_ms = float(np.mean(kms))
    ops = 2.0 * C2_KPT * C2_KPT * C2_DIM * P
    line = {"metric": "C2 image-pairs matched/sec", "value": P / (ms * 1e-3), "unit": "pairs/s", "ms_per_step": ms,
            "dtype": "int8",
            "config": {"workload": f"C2: {C2_IMG} imgs x {C2_KPT} SIFT-128 (0..255), all {P} pairs, MODE_SIFT "
                                   f"(q = x - 128), ratio 0.75", "operand_shift": bank.shift},
            "roofline": {"bound": "mfma", "kernel": "match_kernel<128>", "kernel_ms": k_ms, "unit": "TOPS",
                         "achieved": ops / (k_ms * 1e-3) / 1e12, "peak": PEAK_INT8_TOPS,
                         "frac": ops / (k_ms * 1e-3) / 1e12 / PEAK_INT8_TOPS,
                         "note": "kernel_ms spans the match launch, which writes the int16 graph itself"}}
    if cpu:
        sample = spread(P, 16)
        qcpu = {int(k): bank.q[int(k)].cpu().numpy() for i in sample for k in pairs[i]}
        line["cpu_baseline"] = match_cpu_leg(qcpu, pairs, sample)
    del bank
    torch.cuda.empty_cache()
    return line


def int8_line(sfm, syn, device, args, barrier, cpu=True, exact_ms=None):
    """The quantised mode (DescriptorBank.from_float(..., exact=False)): exact integer
    squared L2 of the int8 quantisation q = rint(127 x), the int8 MFMA kernel alone, on
    all C3 pairs.  Reported with its speed relative to the exact-float headline."""
    sdist = importlib.import_module("3d_reconstruction_amd.dist")
    x = syn.superpoint_like(N_IMG, M_KPT, DIM, seed=1, device=device)
    bank = sfm.DescriptorBank.from_float(x, mode=sfm.MODE_FLOAT, exact=False)
    del x
    pairs = sfm.all_pairs(N_IMG)
    pdev = torch.from_numpy(pairs).to(device)
    P = pdev.shape[0]

    def step(record):
        e0, e1 = events() if record else (None, None)
        if record:
            e0.record()
        sdist.match_all_pairs_sharded(bank, pdev, exact=False, chunks=1,
                                      after_compute=(e1.record if record else None))
        return (e0, e1)

    wall, kms = timed(step, args.steps, 1, barrier)
    ms = wall / args.steps * 1e3
    k_ms = float(np.mean(kms))
    ops = 2.0 * M_KPT * M_KPT * DIM * P
    line = {"metric": "quantised-int8 image-pairs matched/sec", "value": P / (ms * 1e-3), "unit": "pairs/s",
            "ms_per_step": ms, "dtype": "int8",
            "config": {"workload": f"C3 float descriptors quantised q = rint(127 x), exact int8 BF-L2 + ratio 0.75 "
                                   f"(DescriptorBank.from_float(exact=False)): {N_IMG} imgs x {M_KPT} x {DIM}, "
                                   f"all {P} pairs"},
            "roofline": {"bound": "mfma", "kernel": "match_kernel<256>", "kernel_ms": k_ms, "unit": "TOPS",
                         "achieved": ops / (k_ms * 1e-3) / 1e12, "peak": PEAK_INT8_TOPS,
                         "frac": ops / (k_ms * 1e-3) / 1e12 / PEAK_INT8_TOPS,
                         "traffic": pmc_traffic("match_int8"),
                         "traffic_unit": "bytes per launch (FETCH_SIZE*2 + WRITE_SIZE, profiles/r6/traffic.json: "
                                         "the int8-mode launch writing the int16 graph)",
                         "algorithmic": "2*M*N*d int8 ops per pair"},
            "speed_vs_exact": (exact_ms / ms) if exact_ms else None}
    if cpu:
        sample = spread(P, 16)
        qcpu = {int(k): bank.q[int(k)].cpu().numpy() for i in sample for k in pairs[i]}
        line["cpu_baseline"] = match_cpu_leg(qcpu, pairs, sample)
    del bank
    torch.cuda.empty_cache()
    return line


def render_compulsory_bytes(vg, ro, rd, z) -> int:
    """Exact compulsory HBM bytes of one render launch: every distinct 128-B
    voxel line (voxel-major, 32 f32 channels) the trilinear corners of the
    in-bounds samples touch (plenoxel mask |p| < scale, align_corners), plus
    the rays, sample depths and colours read/written once."""
    D, H, W = vg.D, vg.H, vg.W
    lo = torch.tensor(vg.bmin, device=ro.device)
    hi = torch.tensor(vg.bmax, device=ro.device)
    size = torch.tensor([W - 1, H - 1, D - 1], dtype=torch.float32, device=ro.device)
    seen = torch.zeros(D * H * W, dtype=torch.bool, device=ro.device)
    for s in range(0, ro.shape[0], 2048):
        p = ro[s:s + 2048, None, :] + rd[s:s + 2048, None, :] * z[s:s + 2048, :, None]
        inb = ((p.abs() < hi) if vg.mask_mode == 1 else ((p >= lo) & (p <= hi))).all(-1)
        q = ((p - lo) / (hi - lo) * 2 - 1).clamp(-1, 1)
        f = ((q + 1) / 2 * size)[inb]
        i0 = f.floor().long()
        for c in range(8):
            ix = (i0[:, 0] + (c & 1)).clamp(0, W - 1)
            iy = (i0[:, 1] + ((c >> 1) & 1)).clamp(0, H - 1)
            iz = (i0[:, 2] + ((c >> 2) & 1)).clamp(0, D - 1)
            seen[(iz * H + iy) * W + ix] = True
    n_lines = int(seen.sum().item())
    B, S = z.shape
    return n_lines * 128 + B * (24 + 4 * S + 12)


def voxel_and_vq_lines(sfm, syn, device, args, barrier, cpu=True):
    """V1 DDA traversal, V2+V4 fused sample/SH/composite at the plenoxel config
    (28 x 256^3 grid, 16 x 2048 rays x 192 bins per launch) and M2 vq (C3
    descriptors as f64 vs a 200-word codebook), each with a CPU baseline."""
    out = []
    g = torch.Generator(device=device)
    g.manual_seed(7)
    # V1: the survey's probe geometry (4096 rays, bin 1, far <= 64).  The output is
    # the reference's (N, S_max, 3) NaN-padded tensor, so its size grows with the
    # longest ray; at 1M rays it is ~89 GB of mostly padding (tools/dda_probe.py).
    nr = 4096
    o = torch.rand((nr, 3), generator=g, device=device) * 64 - 32
    dvec = torch.randn((nr, 3), generator=g, device=device)
    far = torch.rand((nr, 1), generator=g, device=device) * 64
    rays = torch.cat([o, dvec / dvec.norm(dim=1, keepdim=True), torch.zeros_like(far), far], 1).contiguous()

    def dda_step(record):
        e0, e1 = events() if record else (None, None)
        if record:
            e0.record()
        sfm.voxel_traversal(rays, 1.0)
        if record:
            e1.record()
        return (e0, e1)

    wall, _ = timed(dda_step, args.steps, 1, barrier)
    ms = wall / args.steps * 1e3
    vt = sfm.voxel_traversal(rays, 1.0)
    # algorithmic bytes of one call: the rays read once + the (N, S_max, 3) array written once
    dda_bytes = rays.numel() * rays.element_size() + vt.numel() * vt.element_size()
    line = {"metric": "voxel_traversal rays/sec", "value": nr / (ms * 1e-3), "unit": "rays/s", "ms_per_step": ms,
            "config": {"workload": "V1 DDA (voxel_travesal.py semantics): 4096 rays, bin 1, far U(0,64) "
                                   "(walk into capped rows + host S_max + row-building pass)",
                       "s_max": int(vt.shape[1])},
            "roofline": {"bound": "hbm", "kernel": "dda_walk + dda_rows", "unit": "GB/s",
                         "algorithmic_bytes": dda_bytes, "achieved": dda_bytes / (ms * 1e-3) / 1e9,
                         "peak": PEAK_HBM_GBS, "frac": dda_bytes / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                         "note": "whole call (two launches + the one S_max read-back) per step: a 4096-ray call "
                                 "is launch / sync bound, not HBM bound"}}
    del vt
    if cpu:
        from oracle import voxel as ov
        rr = rays.cpu().numpy()
        line["cpu_baseline"] = cpu_leg(lambda k, nt: ov.voxel_traversal(rr[:k], 1.0), nr, nr, "rays/s", "port",
                                       f"the same {nr} rays through oracle.voxel.voxel_traversal (numpy; the "
                                       f"reference loop is single-threaded, so threads only reach numpy)")
    out.append(line)
    # V2+V4: plenoxel N=256 grid, 16 batches of 2048 rays x 192 bins
    N, B, S, NB = 256, 2048, 192, 16
    grid = (torch.randn((28, N, N, N), generator=g, device=device) * 0.1)
    vg = sfm.VoxelGrid.plenoxel(grid, 1.5)
    vg.voxel_major()
    del grid
    ro = torch.randn((NB * B, 3), generator=g, device=device) * 0.2 + torch.tensor([0.0, 0.0, -3.0], device=device)
    rd = torch.randn((NB * B, 3), generator=g, device=device) * 0.2 + torch.tensor([0.0, 0.0, 1.0], device=device)
    rd = rd / rd.norm(dim=1, keepdim=True)
    t = torch.linspace(2.0, 6.0, S, device=device).expand(NB * B, S)
    mid = (t[:, :-1] + t[:, 1:]) / 2
    u = torch.rand((NB * B, S), generator=g, device=device)
    z = (torch.cat([t[:, :1], mid], 1) + (torch.cat([mid, t[:, -1:]], 1) - torch.cat([t[:, :1], mid], 1)) * u)
    z = z.contiguous()

    def render_step(record):
        e0, e1 = events() if record else (None, None)
        if record:
            e0.record()
        vg.render(ro, rd, z)
        if record:
            e1.record()
        return (e0, e1)

    wall, kms = timed(render_step, args.steps, 1, barrier)
    ms = wall / args.steps * 1e3
    k_ms = float(np.mean(kms))
    comp = render_compulsory_bytes(vg, ro, rd, z)
    line = {"metric": "render_rays rays/sec", "value": NB * B / (ms * 1e-3), "unit": "rays/s", "ms_per_step": ms,
            "config": {"workload": "V2+V4 plenoxel render_rays: 28x256^3 grid, 16 x (2048 rays x 192 bins) "
                                   "in one launch"},
            "roofline": {"bound": "hbm", "kernel": "render_kernel", "kernel_ms": k_ms, "unit": "GB/s",
                         "compulsory_bytes": comp,
                         "achieved": comp / (k_ms * 1e-3) / 1e9, "peak": PEAK_HBM_GBS,
                         "frac": comp / (k_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                         "traffic": pmc_traffic("render"),
                         "traffic_unit": "bytes per launch (FETCH_SIZE*2 + WRITE_SIZE, profiles/r6/traffic.json): "
                                         "voxel lines re-fetched, see DESIGN K5",
                         "note": "compulsory = distinct 128-B voxel lines under the in-bounds samples' trilinear "
                                 "corners (exact count) + rays/z read + colours written; the 8-corner x 28-channel "
                                 "gather volume (896 B/sample) mostly hits in L2"}}
    if cpu:
        from oracle import voxel as ov
        gsmall = vg.grid.cpu().numpy()
        ro_c, rd_c, z_c = ro[:256].cpu().numpy(), rd[:256].cpu().numpy(), z[:256].cpu().numpy()

        def run(k, nt):
            parts = [(s, min(k, s + max(1, k // nt))) for s in range(0, k, max(1, k // nt))]
            pool_map(lambda ab: ov.render(gsmall, (-1.5,) * 3, (1.5,) * 3, 1, ro_c[ab[0]:ab[1]], rd_c[ab[0]:ab[1]],
                                          z_c[ab[0]:ab[1]]), parts, nt)
        line["cpu_baseline"] = cpu_leg(run, 256, 64, "rays/s", "port",
                                       "oracle.voxel.render (numpy f32 restatement of plenoxel.render_rays) on "
                                       "256 rays x 192 bins (all threads: ray blocks over a thread pool) / 64 rays "
                                       "(1 thread)")
        del gsmall
    out.append(line)
    del vg
    torch.cuda.empty_cache()
    # M2: vq of all C3 descriptors (f64) against a 200-word codebook
    obs = syn.superpoint_like(N_IMG, M_KPT, 128, seed=3, device=device).reshape(-1, 128).double().contiguous()
    book = obs[torch.randperm(obs.shape[0], generator=g, device=device)[:200]].contiguous()
    codes = torch.empty(obs.shape[0], dtype=torch.int32, device=device)
    dst = torch.empty(obs.shape[0], dtype=torch.float64, device=device)
    abi = importlib.import_module("3d_reconstruction_amd._abi")

    def vq_step(record):
        e0, e1 = events() if record else (None, None)
        if record:
            e0.record()
        abi.call("sfmhip_vq", obs.data_ptr(), obs.shape[0], book.data_ptr(), 200, 128, codes.data_ptr(),
                 dst.data_ptr(), abi.stream_ptr())
        if record:
            e1.record()
        return (e0, e1)

    wall, kms = timed(vq_step, args.steps, 1, barrier)
    ms = wall / args.steps * 1e3
    fl = 2 * obs.shape[0] * 200 * 128 / (np.mean(kms) * 1e-3) / 1e12
    line = {"metric": "vq obs/sec", "value": obs.shape[0] / (ms * 1e-3), "unit": "obs/s", "ms_per_step": ms,
            "config": {"workload": "M2 vq (matching.py:27): 257x4096 obs x 200 codes x 128-d, f64"},
            # f16-split filter on v_mfma_f32_16x16x32_f16 (3 MFMAs per product, proven error bound;
            # undecided observations settled in f64): the f64 observation stream (n*d*8 B, read once)
            # plus codes + distances written is the bound — 3 x 2nkd f16 flops take 0.07 ms at the
            # dense f16 peak, the stream 0.14 ms at 8 TB/s
            "roofline": {"bound": "hbm", "kernel": "vq_f16s_kernel+vq_exact_kernel", "kernel_ms": float(np.mean(kms)),
                         "unit": "GB/s", "compulsory_bytes": obs.shape[0] * (128 * 8 + 12),
                         "achieved": obs.shape[0] * (128 * 8 + 12) / (np.mean(kms) * 1e-3) / 1e9,
                         "peak": PEAK_HBM_GBS, "frac": obs.shape[0] * (128 * 8 + 12) / (np.mean(kms) * 1e-3) / 1e9
                         / PEAK_HBM_GBS, "gemm_tflops_2nkd": fl, "traffic": pmc_traffic("vq"),
                         "traffic_unit": "bytes per call (FETCH_SIZE*2 + WRITE_SIZE, profiles/r6/traffic.json)"}}
    if cpu:
        from scipy.cluster.vq import vq as scipy_vq
        oo, bb = obs[:65536].cpu().numpy(), book.cpu().numpy()

        def run(k, nt):
            step_ = max(1, k // nt)
            pool_map(lambda s: scipy_vq(oo[s:s + step_], bb), range(0, k, step_), nt)
        line["cpu_baseline"] = cpu_leg(run, 65536, 16384, "obs/s", "reference",
                                       "scipy.cluster.vq.vq (the reference's own call) on 65,536 obs (all threads: "
                                       "row blocks over a thread pool) / 16,384 obs (1 thread)")
    out.append(line)
    return out


def verify_line(sfm, syn, device, args, barrier, cpu=True):
    """§8f row 2: findEssentialMat (RANSAC, prob 0.999, 1 px) + recoverPose for
    256 BFS-candidate pairs x 2048 matches (30 % outliers, 0.5 px noise), one
    batched launch each; CPU baseline = the oracle restatement."""
    v = sfm.verify
    s = syn.two_view_pairs(256, 2048, outlier_frac=0.3, noise_px=0.5, seed=6)
    a, b, of = v.pack_pairs(s["pts0"], s["pts1"])
    cam = torch.tensor(v._cam(s["K"]), dtype=torch.float64, device=device).expand(256, 4).contiguous()
    holder = {}

    def step(record):
        e0, e1 = events() if record else (None, None)
        if record:
            e0.record()
        r = v.find_essential_batched(a, b, of, cam)
        holder["rp"] = v.recover_pose_batched(r["E"], a, b, of, cam, mask=r["mask"])
        holder["r"] = r
        if record:
            e1.record()
        return (e0, e1)

    wall, kms = timed(step, args.steps, 1, barrier)
    ms = wall / args.steps * 1e3
    it_p = holder["r"]["iters"].double().cpu().numpy()
    iters = float(it_p.mean())
    n_p = np.array([len(x) for x in s["pts0"]], np.float64)
    k_ms = float(np.mean(kms))
    line = {"metric": "geometric verification pairs/sec", "value": 256 / (ms * 1e-3), "unit": "pairs/s",
            "ms_per_step": ms,
            "config": {"workload": "findEssentialMat(RANSAC, 0.999, 1px) + recoverPose: 256 pairs x 2048 matches, "
                                   "30% outliers, 0.5 px noise (matching.py:134-139 / sfm.py:108-119)",
                       "mean_ransac_iters": iters},
            "roofline": {"bound": "fp64", "kernel": "ess_init/chunk/replay/final + recover_pose_kernel",
                         "kernel_ms": k_ms}}
    vw = verify_work()
    if vw is not None:
        mps = vw["essential"]["models_per_sample"]
        flops = float(np.sum(it_p * (F_5PT + mps * n_p * F_SAMPSON)) + np.sum(4.0 * n_p * F_TRI_POSE))
        tf = flops / (k_ms * 1e-3) / 1e12
        line["roofline"].update({
            "unit": "TFLOP/s", "algorithmic_flop": flops, "achieved": tf, "peak": PEAK_FP64_TFLOPS,
            "frac": tf / PEAK_FP64_TFLOPS,
            "count": f"sum over pairs of iters x ({F_5PT:.0f} + {mps:.2f} models/sample x n x {F_SAMPSON:.0f}) "
                     f"+ 4 poses x n x {F_TRI_POSE:.0f} (recoverPose); models/sample from "
                     f"profiles/r3/verify_work.json"})
    if cpu:
        from oracle import ransac as orc

        def one(p):
            E, m = orc.find_essential_mat(s["pts0"][p], s["pts1"][p], s["K"])
            keep = m.ravel() > 0
            orc.recover_pose(E, s["pts0"][p][keep], s["pts1"][p][keep], s["K"])
        line["cpu_baseline"] = cpu_leg(lambda k, nt: pool_map(one, range(k), nt), 8, 2, "pairs/s", "port",
                                       "oracle.ransac (numpy restatement of OpenCV's findEssentialMat + "
                                       "recoverPose) on 8 pairs over a thread pool / 2 pairs on 1 thread")
    return line


def train_line(sfm, syn, device, args, barrier, cpu=True):
    """§8f row 4: one plenoxel training step at the reference's config
    (plenoxel.py:124-133: NerfModel(N=256), batch 2048 rays, 192 bins,
    hn=2, hf=6): fused render forward+backward (scatter into the gradient)
    + Adam over all 28 x 256^3 parameters with the gradient reset."""
    tm = importlib.import_module("3d_reconstruction_amd.train")
    N, B, S = 256, 2048, 192
    g = torch.Generator(device=device)
    g.manual_seed(11)
    grid = torch.ones((28, N, N, N), device=device) / 100        # NerfModel init (plenoxel.py:29)
    tr = tm.GridTrainer.plenoxel(grid, 1.5, lr=1e-2)
    del grid
    torch.cuda.empty_cache()
    ro = torch.randn((B, 3), generator=g, device=device) * 0.2 + torch.tensor([0.0, 0.0, -3.0], device=device)
    rd = torch.randn((B, 3), generator=g, device=device) * 0.2 + torch.tensor([0.0, 0.0, 1.0], device=device)
    rd = (rd / rd.norm(dim=1, keepdim=True)).contiguous()
    t = torch.linspace(2.0, 6.0, S, device=device).expand(B, S)
    mid = (t[:, :-1] + t[:, 1:]) / 2
    lower = torch.cat([t[:, :1], mid], 1)
    upper = torch.cat([mid, t[:, -1:]], 1)
    z = (lower + (upper - lower) * torch.rand((B, S), generator=g, device=device)).contiguous()
    gt = torch.rand((B, 3), generator=g, device=device)
    ev = {}

    def step(record):
        e0 = e1 = e2 = None
        if record:
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
        loss, _, nb = tr._backward(ro, rd, gt, z)
        if record:
            e1.record()
        tr.optimizer_step()
        if record:
            e2.record()
            ev.setdefault("a", []).append((e1, e2))
        float(loss.item()) / (3 * nb)              # loss.item() every step, as plenoxel.py:110
        return (e0, e2)

    wall, kms = timed(step, args.steps, 1, barrier)
    ms = wall / args.steps * 1e3
    adam_ms = float(np.mean([a.elapsed_time(b) for a, b in ev["a"]]))
    # this box's streaming rate on the same buffers (a device copy of the parameter lines):
    # Adam's time tracks it from box to box (tools/adam_probe.py)
    tmp = torch.empty_like(tr.param)
    cps = []
    for _ in range(4):
        a, b = events()
        a.record()
        tmp.copy_(tr.param)
        b.record()
        torch.cuda.synchronize()
        cps.append(2 * tr.param.numel() * 4 / (a.elapsed_time(b) * 1e-3) / 1e9)
    del tmp
    copy_gbs = max(cps[1:])
    n_par = 28 * N ** 3
    tr.backward(ro, rd, gt, z)                    # the share of voxel lines one step's scatter touches
    touched = float(tr.touched.float().mean().item())
    tr.optimizer_step()
    moved = 24 + 8 * touched                      # p, m, v read + written; grad only on touched lines
    line = {"metric": "plenoxel training steps/sec", "value": 1e3 / ms, "unit": "steps/s", "ms_per_step": ms,
            "config": {"workload": "plenoxel.py train step: NerfModel(N=256) 28x256^3, 2048 rays x 192 bins, "
                                   "mse + backward + Adam(lr=1e-2)"},
            "roofline": {"bound": "hbm", "kernel": "adam_flagged_kernel", "kernel_ms": adam_ms, "unit": "GB/s",
                         "algorithmic_bytes_per_param": 32,
                         "achieved": n_par * 32 / (adam_ms * 1e-3) / 1e9, "peak": PEAK_HBM_GBS,
                         "frac": n_par * 32 / (adam_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                         "touched_line_frac": touched,
                         "moved_gbs": n_par * 32 / 28 * moved / (adam_ms * 1e-3) / 1e9,
                         "box_copy_gbs": copy_gbs,
                         "moved_vs_copy": (n_par * 32 / 28 * moved / (adam_ms * 1e-3) / 1e9) / copy_gbs,
                         "note": "torch Adam's 32 B/param (p, g, m, v read; p, m, v, g written) is the algorithmic "
                                 "count; the kernel skips grad lines the step's scatter did not touch (known 0), and "
                                 "moves (24 + 8 x touched) B per slot of the voxel-major 32-channel layout "
                                 "(4 pad channels): moved_gbs"}}
    if cpu:
        from oracle import train as ot
        Nc, Bc = 64, 64
        gsmall = np.full((28, Nc, Nc, Nc), 0.01, np.float32)
        zz, roc, rdc, gtc = z[:Bc].cpu().numpy(), ro[:Bc].cpu().numpy(), rd[:Bc].cpu().numpy(), gt[:Bc].cpu().numpy()
        t_r, _ = cpu_median(lambda: ot.render_loss_grad(gsmall, (-1.5,) * 3, (1.5,) * 3, 1, roc, rdc, zz, gtc))
        t_r /= Bc
        _, _, grad = ot.render_loss_grad(gsmall, (-1.5,) * 3, (1.5,) * 3, 1, roc, rdc, zz, gtc)
        t_a, _ = cpu_median(lambda: ot.adam_step(gsmall, grad, np.zeros_like(grad), np.zeros_like(grad), 1))
        t_a /= gsmall.size
        est = t_r * B + t_a * n_par
        line["cpu_baseline"] = {"value": 1.0 / est, "unit": "steps/s", "cores": 1, "kind": "port",
                                "sample": f"oracle.train on {Bc} rays (render+backward, {t_r * 1e3:.2f} ms/ray) "
                                          f"and Adam over 28x{Nc}^3 params ({t_a * 1e9:.1f} ns/param), each the "
                                          f"median of 3 after 1 warm-up, extrapolated to 2048 rays + 28x256^3 "
                                          f"params = {est:.1f} s/step (single-threaded numpy)"}
    del tr
    torch.cuda.empty_cache()
    return line


def sdf_train_line(sfm, syn, device, args, barrier, cpu=True):
    """§8f row 4, sdf.py mode: one iteration of sdf.py's training loop (sdf.py:427-438) at the
    reference's config — SDFGrid(get_grid_resolution(max_resolution=250)) (sdf.py:94-108, 414),
    batches of 2048 rays, GradientBasedSampler's 160 stratified samples (sdf.py:154-180, 220-256),
    forward (SH-2 colour, sdf.py:361-406), mse on the valid rays, backward and Adam(lr=1e-2) over
    all 28 x R^3 parameters: GridTrainer(MASK_SDF).sdf_step.  Synthetic: the point cloud is the C3
    synthetic scene's (uniform in [-1,1]^3, so get_grid_resolution gives 250^3), rays are pixel rays of
    orbit cameras looking at it, colours random."""
    tm = importlib.import_module("3d_reconstruction_amd.train")
    B, S = 2048, 160
    pts = syn.ba_scene(1, 4096, seed=4)["X"]
    # SceneHelper.get_grid_resolution (sdf.py:94-108), restated on the host (bounds x1.5, int-truncated)
    mn = (pts.min(0) * 1.5).astype(int)
    mx = (pts.max(0) * 1.5).astype(int)
    gsz = mx - mn
    box = np.max(gsz) / 250
    res = tuple(int(v) for v in np.ceil(gsz / box).astype(int))   # (x, y, z) order used as (D, H, W): sdf.py quirk
    grid = torch.ones((28,) + res, device=device) / 100           # SDFGrid init (sdf.py:280)
    tr = tm.GridTrainer(grid, tuple(float(v) for v in mn), tuple(float(v) for v in mx), tm.MASK_SDF, lr=1e-2)
    del grid
    torch.cuda.empty_cache()
    g = torch.Generator(device=device)
    g.manual_seed(12)
    Rs, ts = syn.orbit_cameras(64, seed=3)
    Rt = torch.tensor(np.stack(Rs), dtype=torch.float32, device=device)
    tt = torch.tensor(np.stack(ts), dtype=torch.float32, device=device)

    def batch():
        cam = torch.randint(0, 64, (B,), generator=g, device=device)
        u = (torch.rand(B, generator=g, device=device) - 0.5) * syn.IMG_W
        v = (torch.rand(B, generator=g, device=device) - 0.5) * syn.IMG_H
        dc = torch.stack([u / syn.FOCAL, v / syn.FOCAL, torch.ones_like(u)], 1)
        R = Rt[cam]
        d = torch.einsum("bji,bj->bi", R, dc)                      # R^T dc: camera -> world
        o = -torch.einsum("bji,bj->bi", R, tt[cam])                # centre -R^T t
        return o.contiguous(), (d / d.norm(dim=1, keepdim=True)).contiguous(), \
            torch.rand((B, 3), generator=g, device=device)
    batches = [batch() for _ in range(4)]
    ev = {}
    it = {"k": 0}
    nvalid = []

    def step(record):
        ro, rd, gt = batches[it["k"] % len(batches)]
        it["k"] += 1
        e0 = e2 = None
        ea = None
        if record:
            e0, e2 = events()
            ea = events()
            e0.record()
        loss, valid = tr.sdf_step(ro, rd, gt, S, events=ea)   # loss.item() every step (sdf.py:441)
        if record:
            e2.record()
            ev.setdefault("a", []).append(ea)
            nvalid.append(valid)
        return (e0, e2)

    wall, kms = timed(step, args.steps, 1, barrier)
    ms = wall / args.steps * 1e3
    adam_ms = float(np.mean([a.elapsed_time(b) for a, b in ev["a"]]))
    valid_frac = float(torch.stack(nvalid).float().mean().item())
    n_par = 28 * int(np.prod(res))
    line = {"metric": "sdf.py training steps/sec", "value": 1e3 / ms, "unit": "steps/s", "ms_per_step": ms,
            "config": {"workload": f"sdf.py train step: SDFGrid {res[0]}x{res[1]}x{res[2]} x 28 ch "
                                   f"(get_grid_resolution(250) of the synthetic C3 point cloud), {B} rays x {S} "
                                   f"stratified samples, mse on valid rays + backward + Adam(lr=1e-2)",
                       "grid": list(res), "valid_ray_frac": valid_frac},
            "roofline": {"bound": "hbm", "kernel": "adam_flagged_kernel", "kernel_ms": adam_ms, "unit": "GB/s",
                         "algorithmic_bytes_per_param": 32,
                         "achieved": n_par * 32 / (adam_ms * 1e-3) / 1e9, "peak": PEAK_HBM_GBS,
                         "frac": n_par * 32 / (adam_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                         "step_frac": n_par * 32 / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                         "note": "torch Adam's 32 B/param over the 28 x R^3 grid is the compulsory traffic of a step "
                                 "(the sampler + render backward add < 1 %): frac on the Adam kernel's events, "
                                 "step_frac on the whole step's wall time (incl. the valid-ray compaction's host "
                                 "sync, as the reference's boolean mask indexing)"}}
    if cpu:
        from oracle import train as ot
        from oracle import voxel as ov
        Nc, Bc = 64, 32
        gsmall = np.full((28, Nc, Nc, Nc), 0.01, np.float32)
        ro, rd, gt = (t[:Bc].cpu().numpy() for t in batches[0])
        bmn, bmx = tuple(float(v) for v in mn), tuple(float(v) for v in mx)

        def cpu_render():
            tn, tf, vv = ov.ray_aabb(ro, rd, np.array(bmn, np.float32), np.array(bmx, np.float32))
            z = ov.sample_uniform(tn[vv], tf[vv], S, np.random.default_rng(0).random((int(vv.sum()), S),
                                                                                   dtype=np.float32))
            return ot.render_loss_grad(gsmall, bmn, bmx, 0, ro[vv], rd[vv], z, gt[vv])
        t_r, _ = cpu_median(cpu_render)
        t_r /= Bc
        _, _, grad = cpu_render()
        t_a, _ = cpu_median(lambda: ot.adam_step(gsmall, grad, np.zeros_like(grad), np.zeros_like(grad), 1))
        t_a /= gsmall.size
        est = t_r * B + t_a * n_par
        line["cpu_baseline"] = {"value": 1.0 / est, "unit": "steps/s", "cores": 1, "kind": "port",
                                "sample": f"oracle sampler + oracle.train render/backward (SDF mask) on {Bc} rays "
                                          f"({t_r * 1e3:.2f} ms/ray) and Adam over 28x{Nc}^3 params "
                                          f"({t_a * 1e9:.1f} ns/param), each the median of 3 after 1 warm-up, "
                                          f"extrapolated to {B} rays + 28x{res[0]}x{res[1]}x{res[2]} params = "
                                          f"{est:.1f} s/step (single-threaded numpy)"}
    del tr
    torch.cuda.empty_cache()
    return line


def pnp_line(sfm, syn, device, args, barrier, cpu=True):
    """sfm.py:116 solvePnPRansac batched: 256 registrations x 2000 2D-3D
    correspondences (30 % outliers, 0.5 px noise), EPnP RANSAC + LM refine."""
    from oracle import geometry as og
    v = sfm.verify
    rng = np.random.default_rng(12)
    K = np.diag([syn.FOCAL, syn.FOCAL, 1.0])
    P, n = 256, 2000
    Xs, uvs = [], []
    for _ in range(P):
        rv = rng.normal(0, 0.2, 3)
        t = np.array([rng.normal(0, 0.3), rng.normal(0, 0.3), 5.0 + rng.random()])
        X = rng.uniform(-1, 1, (n, 3))
        uv = og.project_points(X, rv, t, K) + rng.normal(0, 0.5, (n, 2))
        bad = rng.random(n) < 0.3
        uv[bad] = rng.uniform(-900, 900, (int(bad.sum()), 2))
        Xs.append(X)
        uvs.append(uv)
    Xd = torch.tensor(np.concatenate(Xs), device=device)
    ud = torch.tensor(np.concatenate(uvs), device=device)
    of = torch.tensor(np.arange(P + 1, dtype=np.int64) * n, device=device)
    cam = torch.tensor(v._cam(K), device=device).expand(P, 4).contiguous()
    holder = {}

    def step(record):
        e0, e1 = events() if record else (None, None)
        if record:
            e0.record()
        holder["r"] = v.pnp_ransac_batched(Xd, ud, of, cam)
        if record:
            e1.record()
        return (e0, e1)

    wall, kms = timed(step, args.steps, 1, barrier)
    ms = wall / args.steps * 1e3
    k_ms = float(np.mean(kms))
    it_p = holder["r"]["iters"].double().cpu().numpy()
    inl_p = holder["r"]["n_inliers"].double().cpu().numpy()
    line = {"metric": "PnP registrations/sec", "value": P / (ms * 1e-3), "unit": "registrations/s",
            "ms_per_step": ms,
            "config": {"workload": "solvePnPRansac (sfm.py:116: 100 iters, 8 px, 0.99) + LM refine: 256 problems x "
                                   "2000 correspondences, 30% outliers",
                       "mean_ransac_iters": float(it_p.mean())},
            "roofline": {"bound": "fp64", "kernel": "pnp_ransac_kernel", "kernel_ms": k_ms}}
    vw = verify_work()
    if vw is not None:
        lm_passes = vw["pnp"]["lm_projection_passes_per_problem"]
        flops = float(np.sum(it_p * (F_EPNP + n * F_PNP_SCORE)) + np.sum(lm_passes * inl_p * F_LM_OBS))
        tf = flops / (k_ms * 1e-3) / 1e12
        line["roofline"].update({
            "unit": "TFLOP/s", "algorithmic_flop": flops, "achieved": tf, "peak": PEAK_FP64_TFLOPS,
            "frac": tf / PEAK_FP64_TFLOPS,
            "count": f"sum over problems of iters x ({F_EPNP:.0f} + n x {F_PNP_SCORE:.0f}) + {lm_passes:.2f} LM "
                     f"passes x inliers x {F_LM_OBS:.0f}; LM passes from profiles/r3/verify_work.json"})
    if cpu:
        from oracle import pnp as opnp
        line["cpu_baseline"] = cpu_leg(lambda k, nt: pool_map(lambda i: opnp.solve_pnp_ransac(Xs[i], uvs[i], K),
                                                              range(k), nt),
                                       16, 4, "registrations/s", "port",
                                       "oracle.pnp (numpy restatement of OpenCV's solvePnPRansac) on 16 problems "
                                       "over a thread pool / 4 problems on 1 thread")
    return line


def ba_cpu_leg(s):
    """The reference's per-pair CPU path for the same work (sfm.py:27-38): numpy
    batched-SVD DLT (cv2.triangulatePoints restatement) + the residual and
    scipy approx_derivative grouped 2-point Jacobian with the ba_sparse
    pattern (what least_squares evaluates per TRF iteration); pairs over a
    thread pool for the all-threads run.  Also the full scipy least_squares
    solve per pair with sfm.py:38's settings (reported, not in the rate)."""
    from oracle import geometry as og

    def one(p):
        sl = slice(p * BA_OBS, (p + 1) * BA_OBS)
        og.triangulate_points(s["P"][p, 0], s["P"][p, 1], s["x0"][:, sl], s["x1"][:, sl])
        xv = np.concatenate([s["cam"][p], s["X"][sl].ravel()])
        og.fd_jacobian(xv, s["K"][p], s["pts2d"][sl])

    sample = spread(BA_PAIRS, 16)
    leg = cpu_leg(lambda k, nt: pool_map(one, sample[:k], nt), 16, 4, "obs/s", "port",
                  "per pair: oracle.geometry.triangulate_points (numpy batched SVD, cv2.triangulatePoints "
                  "restatement) + oracle.geometry.fd_jacobian (residual + scipy approx_derivative with the "
                  "ba_sparse groups) on 16 pairs over a thread pool / 4 pairs on 1 thread", scale=BA_OBS)
    from scipy.optimize import least_squares
    p = sample[0]
    sl = slice(p * BA_OBS, (p + 1) * BA_OBS)
    xv = np.concatenate([s["cam"][p], s["X"][sl].ravel()])
    A = og.ba_sparse(BA_OBS, len(xv), 6)
    holder = {}

    def solve():
        holder["r"] = least_squares(og.reprojection_error, xv, jac_sparsity=A, verbose=0, x_scale="jac",
                                    ftol=1e-8, args=(s["K"][p], s["pts2d"][sl]))
    t_ls, _ = cpu_median(solve)
    leg["least_squares_s_per_pair"] = t_ls
    leg["least_squares_nfev"] = int(holder["r"].nfev)
    return leg


def ba_line(sfm, syn, device, args, barrier, cpu=True):
    """DLT + residual + FD-Jacobian over BA_PAIRS pairs x BA_OBS observations
    (pair ranges per rank); DLT and residual/FD-J kernels timed apart."""
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    sdist = importlib.import_module("3d_reconstruction_amd.dist")
    s = syn.ba_scene(BA_PAIRS, BA_OBS, seed=4)
    n = BA_PAIRS * BA_OBS
    olo, ohi = sdist.shard_range(BA_PAIRS, rank, world)
    sl = slice(olo * BA_OBS, ohi * BA_OBS)
    tt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in s.items()}
    x0l, x1l = tt["x0"][:, sl].contiguous(), tt["x1"][:, sl].contiguous()
    Xl, p2l, pol = tt["X"][sl].contiguous(), tt["pts2d"][sl].contiguous(), tt["pair_of_obs"][sl].contiguous()
    X4 = torch.empty((4, x0l.shape[1]), dtype=torch.float64, device=device)
    rr = torch.empty((Xl.shape[0], 2), dtype=torch.float64, device=device)
    jv = torch.empty((Xl.shape[0], 2, 9), dtype=torch.float64, device=device)
    mids = []

    def ba_step(record):
        e0 = e1 = em = None
        if record:
            e0, e1 = events()
            em = torch.cuda.Event(enable_timing=True)
            e0.record()
        sfm.triangulate_batched(tt["P"], pol, x0l, x1l, out=X4)
        if record:
            em.record()
        sfm.residual_jacobian_batched(tt["cam"], tt["K"], Xl, p2l, pol, r=rr, jv=jv)
        if record:
            e1.record()
            mids.append((e0, em, e1))
        return (e0, e1)

    # a 0.13 ms step: at least 20 timed steps after 5 warm-ups, so one clock-ramp
    # outlier (seen at 137 us vs 26 us in a 4-call rocprof run) cannot carry the mean
    n_ba = max(args.steps, 20)
    wall_b, kms_b = timed(ba_step, n_ba, max(args.warmup, 5), barrier)
    wall_b = max_over_ranks(wall_b, world, device)
    b_ms = wall_b / n_ba * 1e3
    k_ms = max_over_ranks(float(np.mean(kms_b)), world, device)
    # per-kernel durations: 20 back-to-back calls between two events on the launch stream,
    # so the queue stays fed and the host's launch gap in front of a single call (the
    # step's events see the GPU idle while ctypes enqueues) is not counted as kernel time
    def burst(fn, reps=20):
        for _ in range(3):
            fn()
        a, b = events()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    dlt_ms = max_over_ranks(burst(lambda: sfm.triangulate_batched(tt["P"], pol, x0l, x1l, out=X4)), world, device)
    fdj_ms = max_over_ranks(burst(lambda: sfm.residual_jacobian_batched(tt["cam"], tt["K"], Xl, p2l, pol, r=rr,
                                                                         jv=jv)), world, device)
    step_split_ms = (float(np.mean([a.elapsed_time(m) for a, m, _ in mids])),
                     float(np.mean([m.elapsed_time(b) for _, m, b in mids])))
    local = (ohi - olo) * BA_OBS
    dlt_tf = local * DLT_FLOP_PER_OBS / (dlt_ms * 1e-3) / 1e12
    fdj_gbs = local * FDJ_BYTES_PER_OBS / (fdj_ms * 1e-3) / 1e9
    line = {
        "metric": "BA obs/sec (DLT + residual + FD-Jacobian)", "value": n / (b_ms * 1e-3), "unit": "obs/s",
        "ms_per_step": b_ms, "scaling": "strong", "dtype": "f64",
        "config": {"workload": f"C3 BA: {BA_PAIRS} pairs x {BA_OBS} obs, f64", "parallelism": f"pairs/{world}"},
        "roofline": {"kernel_ms": k_ms,
                     "timing": "dlt/fdjac kernel_ms: 20 back-to-back calls between HIP events on the launch "
                               "stream (dlt_normal + dlt_list kernels; residual + fdjac kernels); "
                               f"in-step event split {step_split_ms[0]:.4f} / {step_split_ms[1]:.4f} ms includes "
                               "the host launch gap",
                     "dlt": {"bound": "fp64", "kernel": "dlt_kernel", "kernel_ms": dlt_ms, "unit": "TFLOP/s",
                             "algorithmic_flop_per_obs": DLT_FLOP_PER_OBS, "achieved": dlt_tf,
                             "peak": PEAK_FP64_TFLOPS, "frac": dlt_tf / PEAK_FP64_TFLOPS,
                             "achieved_gbs": local * DLT_BYTES_PER_OBS / (dlt_ms * 1e-3) / 1e9},
                     "fdjac": {"bound": "hbm", "kernel": "fdjac_kernel", "kernel_ms": fdj_ms, "unit": "GB/s",
                               "algorithmic_bytes_per_obs": FDJ_BYTES_PER_OBS, "achieved": fdj_gbs,
                               "peak": PEAK_HBM_GBS, "frac": fdj_gbs / PEAK_HBM_GBS}},
    }
    if cpu and rank == 0 and world == 1:
        line["cpu_baseline"] = ba_cpu_leg(s)
    return line


def ba_solve_line(sfm, syn, device, args, barrier, cpu=True):
    """The whole BA solve of sfm.py:37-38 for C3's 256 pairs x 4096 observations
    on the GPU (ba.hip: scipy's TRF/lsmr iteration restated, one workgroup per
    pair); the step re-stages the initial cameras/points (device copies) and
    solves every pair to scipy's termination.  CPU: scipy least_squares with
    sfm.py:38's settings per pair (the reference call)."""
    s = syn.ba_scene(BA_PAIRS, BA_OBS, seed=4)
    tt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in s.items()}
    off = torch.arange(BA_PAIRS + 1, dtype=torch.int64, device=device) * BA_OBS
    cam, X = tt["cam"].clone(), tt["X"].clone()
    holder = {}
    sfm.ba_solve_batched(cam, tt["K"], X, tt["pts2d"], off)     # validates the offsets once (host sync)

    def step(record):
        e0, e1 = events() if record else (None, None)
        cam.copy_(tt["cam"])
        X.copy_(tt["X"])
        if record:
            e0.record()
        holder["r"] = sfm.ba_solve_batched(cam, tt["K"], X, tt["pts2d"], off, validate=False)
        if record:
            e1.record()
        return (e0, e1)

    wall, kms = timed(step, args.steps, 1, barrier)
    ms = wall / args.steps * 1e3
    r = holder["r"]
    k_ms = float(np.mean(kms))
    nfev = r["nfev"].double().cpu().numpy()
    njev = r["njev"].double().cpu().numpy()
    flops = float(np.sum(BA_OBS * (njev * F_BA_J_OBS + nfev * F_BA_STEP_OBS)))
    tf = flops / (k_ms * 1e-3) / 1e12
    line = {"metric": "BA solves/sec (sfm.py:38 least_squares, on device)", "value": BA_PAIRS / (ms * 1e-3),
            "unit": "pairs/s", "ms_per_step": ms, "dtype": "f64",
            "config": {"workload": f"C3 BA: {BA_PAIRS} pairs x {BA_OBS} obs, scipy TRF (x_scale='jac', ftol 1e-8) "
                                   f"restated on the device",
                       "mean_nfev": float(nfev.mean()), "mean_njev": float(njev.mean()),
                       "status_ok": int((r["status"] > 0).sum().item())},
            "kernel_ms": k_ms,
            "roofline": {"bound": "fp64", "kernel": "ba_trf_kernel", "kernel_ms": k_ms, "unit": "TFLOP/s",
                         "algorithmic_flop": flops, "achieved": tf, "peak": PEAK_FP64_TFLOPS,
                         "frac": tf / PEAK_FP64_TFLOPS,
                         "achieved_gbs": BA_PAIRS * BA_OBS * BA_BYTES_OBS / (k_ms * 1e-3) / 1e9,
                         "count": f"sum over pairs of n_obs x (njev x {F_BA_J_OBS:.0f} + nfev x {F_BA_STEP_OBS:.0f}) "
                                  f"fp64 flops; compulsory bytes {BA_BYTES_OBS:.0f} per observation per solve "
                                  f"(achieved_gbs): the fp64 bound is the larger",
                         # the record passes re-read each observation's 26-double scratch record ~20 times
                         # per solve: measured L2-miss traffic, the rate the kernel actually moves
                         "traffic": pmc_traffic("ba"),
                         "traffic_gbs": (pmc_traffic("ba") or 0.0) / (k_ms * 1e-3) / 1e9,
                         "traffic_unit": "bytes per launch (FETCH_SIZE*2 + WRITE_SIZE, profiles/r6/traffic.json, "
                                         "pmc_ba.txt)"}}
    # sfm.py:37-38 left exactly as written (scipy least_squares, jac_sparsity=ba_sparse, 2-point FD) with
    # only `import sfmhip as cv2`: every residual evaluation is one sfmhip.projectPoints call (host <->
    # device round trip); scipy's TRF / LSMR stay on the host.  Wall time per pair on one C3 pair.
    from scipy.optimize import least_squares as _ls
    import sfmhip as cv2_alias
    p0 = 0
    sl0 = slice(p0 * BA_OBS, (p0 + 1) * BA_OBS)
    x0_0 = np.concatenate([s["cam"][p0], s["X"][sl0].ravel()])
    A0 = cv2_alias.ba_sparse(BA_OBS, len(x0_0), 6)

    acc = {"t": 0.0, "calls": 0}

    def sfm_py_residual(x, K, point_2D):
        t0 = time.perf_counter()
        proj, _ = cv2_alias.projectPoints(x[6:].reshape((len(point_2D), 3)), x[:3], x[3:6], K, distCoeffs=None)
        out = (point_2D - proj[:, 0, :]).ravel()
        acc["t"] += time.perf_counter() - t0
        acc["calls"] += 1
        return out
    hold = {}

    def literal():
        acc["t"], acc["calls"] = 0.0, 0
        hold["r"] = _ls(sfm_py_residual, x0_0, jac_sparsity=A0, x_scale="jac", ftol=1e-8,
                        args=(s["K"][p0], s["pts2d"][sl0]))
        hold["t_res"], hold["calls"] = acc["t"], acc["calls"]
    with blas_limit(1):
        t_lit, ts_lit = cpu_median(literal)
    line["unchanged_sfm_py"] = {
        "s_per_pair": t_lit, "nfev": int(hold["r"].nfev), "residual_calls": hold["calls"],
        "s_in_residual": hold["t_res"], "us_per_residual_call": hold["t_res"] / max(1, hold["calls"]) * 1e6,
        "s_scipy_host": t_lit - hold["t_res"],
        "note": "sfm.py:38 unchanged, `import sfmhip as cv2`: scipy least_squares on the host (1 BLAS thread), "
                "each residual evaluation one sfmhip.projectPoints call (sfmhip_reproj_residual_host: one pinned "
                "staging copy each way + a stream sync); one C3 pair (4096 obs), median of 3 after 1 warm-up. "
                "s_scipy_host = the time outside the residual calls (scipy's TRF / LSMR / FD bookkeeping), the "
                "floor any residual backend leaves"}
    # the same call with the restated numpy residual (what sfm.py costs on this host without cv2), split
    # the same way: the residual share is what a faster backend can remove
    from oracle import geometry as og_lit
    acc_c = {"t": 0.0, "calls": 0}

    def cpu_residual(x, K, point_2D):
        t0 = time.perf_counter()
        out = og_lit.reprojection_error(x, K, point_2D)
        acc_c["t"] += time.perf_counter() - t0
        acc_c["calls"] += 1
        return out
    hold_c = {}

    def literal_cpu():
        acc_c["t"], acc_c["calls"] = 0.0, 0
        _ls(cpu_residual, x0_0, jac_sparsity=A0, x_scale="jac", ftol=1e-8, args=(s["K"][p0], s["pts2d"][sl0]))
        hold_c["t_res"] = acc_c["t"]
    with blas_limit(1):
        t_cpu1, _ = cpu_median(literal_cpu)
    line["unchanged_sfm_py"].update({
        "cpu_s_per_pair": t_cpu1, "cpu_s_in_residual": hold_c["t_res"], "cpu_s_scipy_host": t_cpu1 - hold_c["t_res"],
        "ratio_vs_cpu": t_lit / t_cpu1})
    if cpu:
        from scipy.optimize import least_squares
        from oracle import geometry as og
        sample = spread(BA_PAIRS, 8)
        A = og.ba_sparse(BA_OBS, 6 + 3 * BA_OBS, 6)

        def one(p):
            sl = slice(p * BA_OBS, (p + 1) * BA_OBS)
            x0 = np.concatenate([s["cam"][p], s["X"][sl].ravel()])
            least_squares(og.reprojection_error, x0, jac_sparsity=A, x_scale="jac", ftol=1e-8,
                          args=(s["K"][p], s["pts2d"][sl]))
        line["cpu_baseline"] = cpu_leg(lambda k, nt: pool_map(one, sample[:k], nt), 8, 2, "pairs/s", "reference",
                                       "scipy.optimize.least_squares with sfm.py:38's arguments (the reference "
                                       "call) on the restated residual: 8 pairs over a thread pool / 2 pairs on "
                                       "1 thread")
    return line


def tsdf_cpu_leg(syn):
    """numpy per-frame TSDF oracle (oracle.voxel.tsdf_integrate) on frames of
    the same C5 scene; all threads = z-slabs over a thread pool (numpy drops
    the GIL inside its array loops), 1 thread = the whole grid."""
    from oracle import voxel as ov
    dep, ps, Kk = syn.tsdf_scene(4, syn.IMG_H, syn.IMG_W, device="cpu")
    dep, ps, Kk = dep.numpy(), ps.numpy(), Kk.numpy()
    R = TSDF_R
    args = ((-1.2,) * 3, (1.2,) * 3, np.float32(3 * 2.4 / (R - 1)))

    def run(k, nt):
        if nt <= 1:
            ov.tsdf_integrate(np.zeros((R, R, R), np.float32), np.zeros((R, R, R), np.float32), dep[:k], ps[:k],
                              Kk[:k], *args)
            return
        step_ = -(-R // nt)
        pool_map(lambda z0: ov.tsdf_integrate(np.zeros((min(R, z0 + step_) - z0, R, R), np.float32),
                                              np.zeros((min(R, z0 + step_) - z0, R, R), np.float32), dep[:k], ps[:k],
                                              Kk[:k], *args, z0=z0, z1=min(R, z0 + step_), grid_depth=R),
                 range(0, R, step_), nt)
    return cpu_leg(run, 4, 1, "Mvoxel-updates/s", "port",
                   "oracle.voxel.tsdf_integrate (numpy f32) on 4 frames of the C5 scene (all threads: z-slabs "
                   "over a thread pool) / 1 frame (1 thread, whole grid)", scale=R ** 3 / 1e6)


def composite_line(result, match_cpu, ba, tsdf):
    """North-star composite (BASELINE.json): C3 all-pairs match step + C3 DLT/BA
    evaluation (256 pairs x 4096 obs) + C5 TSDF step on 1 MI355X against the
    summed CPU wall-clock of the same three workloads (each extrapolated from
    its timed sample, the faster of its all-threads and 1-thread runs), target
    >= 50x; value_1thread: every CPU part on one thread."""
    P = result["config"]["pairs"]
    gpu_s = (result["ms_per_step"] + ba["ms_per_step"] + tsdf["ms_per_step"]) * 1e-3
    cb, ct = ba.get("cpu_baseline"), tsdf.get("cpu_baseline")
    if not (match_cpu and cb and ct):
        return None
    n_obs = BA_PAIRS * BA_OBS
    upd = TSDF_R ** 3 * TSDF_F / 1e6

    def cpu_s(key):
        return P / match_cpu[key] + n_obs / cb[key] + upd / ct[key]

    def best(leg):   # the faster of the two thread counts (GIL-bound legs run slower on the pool)
        return max(leg["value"], leg["value_1thread"])
    cpu_all = P / best(match_cpu) + n_obs / best(cb) + upd / best(ct)
    cpu_one = cpu_s("value_1thread")
    return {"metric": "north-star composite speedup vs reference CPU path", "value": cpu_all / gpu_s, "unit": "x",
            "target": 50.0, "value_1thread": cpu_one / gpu_s, "gpu_s": gpu_s,
            "cpu_s": cpu_all, "cpu_s_1thread": cpu_one, "cores": match_cpu["cores"],
            "parts_s": {"gpu": {"match": result["ms_per_step"] * 1e-3, "ba": ba["ms_per_step"] * 1e-3,
                                "tsdf": tsdf["ms_per_step"] * 1e-3},
                        "cpu": {"match": P / best(match_cpu), "ba": n_obs / best(cb), "tsdf": upd / best(ct)},
                        "cpu_1thread": {"match": P / match_cpu["value_1thread"], "ba": n_obs / cb["value_1thread"],
                                        "tsdf": upd / ct["value_1thread"]}},
            "config": {"workload": "C3 all-pairs matching (32,896 pairs) + C3 DLT + residual + FD Jacobian "
                                   "(256 x 4096 obs) + C5 TSDF (256^3 x 257 frames), 1 GPU vs host CPU; CPU "
                                   "times are linear extrapolations of the timed samples; matching's CPU part "
                                   "is the numpy f32 GEMM form (SURVEY.md §8d), the headline's cpu_baseline"}}


def free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n: int, argv) -> int:
    """``bench.py --gpus N`` (N > 1) without a torch.distributed launcher: start
    N fresh child processes of this script, one per GPU, with RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_ADDR / MASTER_PORT set, and wait for them.  The parent
    never touches the GPU (it only imported torch) and never exec's: the
    children are new processes.  Rank 0 inherits stdout (the one JSON line);
    the other ranks' stdout goes to stderr.  If any child fails, the others are
    stopped (their exact PIDs) and its exit code is returned."""
    import subprocess
    port = os.environ.get("MASTER_PORT") or str(free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   GROUP_RANK="0", MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"), MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else sys.stderr.fileno()))
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 128 - code
                log(f"[launcher] rank {procs.index(p)} exited with {code}; stopping the other ranks")
                for q in live:
                    q.terminate()
        if live:
            time.sleep(0.2)
    for p in procs:
        p.wait()
    return rc


DUMP_ROWS = 2048              # pair rows of the match graph kept by --dump-outputs (x 4096 f32 = 32 MiB)


def dump_outputs(dirname: str, graph: torch.Tensor) -> dict:
    """--dump-outputs: the match graph the last timed step returned (what a caller of
    ``dist.match_all_pairs_sharded`` receives: (P, m_pad) matches0, -1 = no match), as
    float32 .npy files.  The C3 graph is 135 M entries, so the dump keeps a fixed,
    seeded sample of its pair rows (all rows while P <= DUMP_ROWS), the rows' indices
    and, over every row, the number of matches of each pair."""
    os.makedirs(dirname, exist_ok=True)
    P = int(graph.shape[0])
    if P > DUMP_ROWS:
        rows = np.sort(np.random.default_rng(0).choice(P, DUMP_ROWS, replace=False))
    else:
        rows = np.arange(P)
    sample = graph[torch.from_numpy(rows).to(graph.device)].to(torch.float32).cpu().numpy()
    counts = (graph >= 0).sum(dim=1).to(torch.float32).cpu().numpy()
    files = {"matches0_rows": sample, "matches0_row_index": rows.astype(np.float64), "matches_per_pair": counts}
    for name, a in files.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    return {name: list(a.shape) for name, a in files.items()}


def dry_run(world: int, rank: int, backend: str) -> dict:
    """--dry-run: the rank/world plumbing without any GPU work (CPU tests of
    the launcher): every rank joins the process group and the world is
    all-gathered."""
    if world > 1:
        dist.init_process_group(backend)
        ranks = [None] * world
        dist.all_gather_object(ranks, {"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "0")),
                                       "pid": os.getpid()})
        dist.destroy_process_group()
    else:
        ranks = [{"rank": 0, "local_rank": 0, "pid": os.getpid()}]
    return {"metric": "image-pairs matched/sec", "value": None, "unit": "pairs/s", "n_gpus": world,
            "dry_run": True, "ranks": ranks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true", default=os.environ.get("SFMHIP_BENCH_FULL", "") not in ("", "0"),
                    help="also run the secondary lines, the CPU baselines and the composite (default: the "
                         "headline's set-up, warm-up and timed steps only); SFMHIP_BENCH_FULL=1 in the "
                         "environment does the same, for the session scripts under tools/")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs as DIR/<name>.npy (float32/float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baselines")
    ap.add_argument("--skip-secondary", action="store_true", help="with --full: leave out the secondary lines")
    ap.add_argument("--no-rebalance", action="store_true",
                    help="N > 1: keep equal-thickness TSDF slabs (default: re-cut from measured fusion times)")
    ap.add_argument("--rebalance-rounds", type=int, default=3)
    ap.add_argument("--n-img", type=int, default=N_IMG)
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL on ROCm); gloo only for rehearsal")
    ap.add_argument("--rehearse-overlap", action="store_true",
                    help="N=1 rehearsal of the N>1 path: a one-rank RCCL communicator + the overlapped all-gather")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher/process-group plumbing only (no GPU work; CPU tests)")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit(f"--gpus must be >= 1 (got {args.gpus})")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit(f"--steps must be >= 1 and --warmup >= 0 (got {args.steps}, {args.warmup})")
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        # one process per GPU: this process only launches and waits (no GPU call here)
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} does not match the launcher's WORLD_SIZE {world}")
    if args.dry_run:
        line = dry_run(world, rank, "gloo" if args.dist_backend == "nccl" else args.dist_backend)
        if rank == 0:
            print(json.dumps(line), flush=True)
        return
    # stdout carries exactly one JSON line: RCCL (version banner at communicator
    # init) and other libraries print to fd 1, so fd 1 becomes stderr for the run
    # and the result goes to a private copy of the original stdout
    sys.stdout.flush()
    out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("SFMHIP_BENCH_SAME_DEVICE"):  # rehearsal: every rank on device 0
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(args.dist_backend)
        barrier = lambda: dist.barrier()  # noqa: E731
    else:
        barrier = lambda: None  # noqa: E731

    sfm = importlib.import_module("3d_reconstruction_amd")
    syn = importlib.import_module("3d_reconstruction_amd.synthetic")
    sdist = importlib.import_module("3d_reconstruction_amd.dist")
    cpu = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline

    # the match-graph collective: the C-ABI's RCCL communicator (sfmhip_comm_*),
    # bootstrapped over the torch.distributed group; gloo rehearsals use torch
    comm = None
    if (world > 1 and args.dist_backend == "nccl") or args.rehearse_overlap:
        comm = sdist.RcclComm() if world > 1 else sdist.RcclComm.single()

    # ---------------- C3/C4: all-pairs matching ----------------------------
    n_img = args.n_img
    t0 = time.perf_counter()
    x = syn.superpoint_like(n_img, M_KPT, DIM, seed=1, device=device)
    # the float descriptors' own semantics (exact f32-input BF-L2, Matcher's default): the int8
    # MFMA pass certifies most rows with a proven residual bound, the rest are re-scored in f64
    bank = sfm.DescriptorBank.from_float(x, mode=sfm.MODE_FLOAT, exact=True)
    pairs_all = sfm.all_pairs(n_img)
    if cpu:
        sample = spread(len(pairs_all), 12)
        xcpu = {int(k): x[int(k)].cpu().numpy() for i in sample for k in pairs_all[i]}
    del x
    torch.cuda.synchronize()
    log(f"[rank {rank}] descriptors ready ({time.perf_counter() - t0:.1f}s): "
        f"{n_img}x{M_KPT}x{DIM} int8 = {bank.q.numel() / 1e6:.0f} MB + f32 = {bank.x.numel() * 4 / 1e6:.0f} MB")
    P = len(pairs_all)
    pairs_dev = torch.from_numpy(pairs_all).to(device)
    chunks = MATCH_CHUNKS if (world > 1 or comm is not None) else 1
    holder = {}

    def match_step(record):
        e0, e1 = events() if record else (None, None)
        if record:
            e0.record()
        holder["g"] = sdist.match_all_pairs_sharded(bank, pairs_dev, ratio=(3, 4), exact=True, comm=comm,
                                                    chunks=chunks, after_compute=(e1.record if record else None))
        return (e0, e1)

    wall, kms = timed(match_step, args.steps, args.warmup, barrier)
    wall = max_over_ranks(wall, world, device)
    ms_per_step = wall / args.steps * 1e3
    kern_ms = max_over_ranks(float(np.mean(kms)), world, device)
    pairs_per_launch = sum(max(0, b - a) for a, b in sdist.chunk_rows(P, rank, world, chunks))
    ops_per_launch = 2.0 * M_KPT * M_KPT * DIM * pairs_per_launch
    achieved_tops = ops_per_launch / (kern_ms * 1e-3) / 1e12
    graph = holder["g"]
    rescored = int(bank.last_resolved.item()) if bank.last_resolved is not None else None
    log(f"[rank {rank}] match: {ms_per_step:.2f} ms/step, kernel {kern_ms:.2f} ms, {achieved_tops:.0f} TOPS, "
        f"gathered graph {tuple(graph.shape)} {graph.dtype}"
        + (f", {int((graph >= 0).sum().item())} matches" if args.full else ""))
    dumped = dump_outputs(args.dump_outputs, graph) if (args.dump_outputs and rank == 0) else None

    result = {
        "metric": "image-pairs matched/sec",
        "value": P / (ms_per_step * 1e-3),
        "unit": "pairs/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32 descriptors: int8 MFMA certified filter + f64 re-score",
        "data": "synthetic (SuperPoint-like unit-norm descriptors, 40% cross-view overlap, seed 1)",
        "config": {"workload": f"C3/C4 all-pairs BF-L2 + ratio 0.75: {n_img} imgs x {M_KPT} kpts x {DIM}-d, "
                               "exact f32-input semantics (oracle.match.bf_match_exact, bit for bit)",
                   "pairs": P, "api": "dist.match_all_pairs_sharded(exact=True)", "match_mode": "exact-float",
                   "rows_rescored_per_step": rescored,
                   "parallelism": f"pairs/{world}" + (
                       f" + {chunks} RCCL all-gathers (int16, sfmhip_allgather) overlapped with the match launches"
                       if comm is not None else (" + torch.distributed all-gather (rehearsal)" if world > 1 else ""))},
        "roofline": {"bound": "mfma", "achieved": achieved_tops, "peak": PEAK_INT8_TOPS, "unit": "TOPS",
                     "frac": achieved_tops / PEAK_INT8_TOPS,
                     "traffic": pmc_traffic("match", pairs_per_launch / P) if n_img == N_IMG else None,
                     "traffic_unit": "bytes per launch (FETCH_SIZE*2 + WRITE_SIZE, profiles/r6/traffic.json: match_kernel "
                                     "(certifying epilogue, int16 graph) + the resolve kernels: collect, batched f64 "
                                     "re-score)",
                     "kernel": "match_kernel<256> (exact mode) + resolve kernels", "kernel_ms": kern_ms,
                     "algorithmic": "2*M*N*d int8 ops per pair x pairs per launch (the f64 re-score of the "
                                    "uncertified rows is overhead, not work)"},
    }
    if dumped is not None:
        result["dumped_outputs"] = dumped
    match_cpu = None
    del bank, holder["g"], graph
    torch.cuda.empty_cache()

    if args.full and not args.skip_secondary:
        # ---------------- C5: TSDF ------------------------------------------
        t0 = time.perf_counter()
        depth, poses, K = syn.tsdf_scene(TSDF_F, syn.IMG_H, syn.IMG_W, device=device)
        torch.cuda.synchronize()
        log(f"[rank {rank}] depth maps ready ({time.perf_counter() - t0:.1f}s): {depth.numel() * 4 / 1e9:.2f} GB")
        R = TSDF_R
        slabs = [sdist.shard_range(R, r, world) for r in range(world)]
        z0, z1 = slabs[rank]
        T = torch.zeros((R, R, R), dtype=torch.float32, device=device)
        Wt = torch.zeros_like(T)
        trunc = 3 * 2.4 / (R - 1)
        bmin, bmax = (-1.2, -1.2, -1.2), (1.2, 1.2, 1.2)

        def tsdf_step(record, fusion_events=None):
            T[z0:z1].zero_()
            Wt[z0:z1].zero_()
            e0, e1 = events() if record else (None, None)
            if record:
                e0.record()
            if world > 1:   # each rank builds the block table of 1/N of the frames; one all-gather
                tab = sdist.shared_block_table(depth, comm=comm)
                if fusion_events:
                    fusion_events[0].record()
                sfm.tsdf_integrate(T, Wt, depth, poses, K, bmin, bmax, trunc, z0, z1, block_table=tab)
                if fusion_events:
                    fusion_events[1].record()
            else:
                sfm.tsdf_integrate(T, Wt, depth, poses, K, bmin, bmax, trunc, z0, z1)
            if record:
                e1.record()
            return (e0, e1)

        rebalance = world > 1 and not args.no_rebalance
        if rebalance:
            # feedback balancing (dist.rebalance_slabs): the slab fusions of an orbit scene differ by
            # up to ~35 % at equal thickness (the centre carries more surface), so each rank times its
            # own fusion, the times are all-gathered and the slabs re-cut; the grid is the same for any
            # cut.  Untimed, like the warm-up steps.
            for _ in range(args.rebalance_rounds):
                fe = events()
                tsdf_step(False, fe)
                torch.cuda.synchronize()
                slabs = sdist.rebalance_slabs(slabs, sdist.allgather_times(fe[0].elapsed_time(fe[1])), R)
                z0, z1 = slabs[rank]
        wall_t, kms_t = timed(tsdf_step, args.steps, args.warmup, barrier)
        wall_t = max_over_ranks(wall_t, world, device)
        t_ms = wall_t / args.steps * 1e3
        tk_ms = max_over_ranks(float(np.mean(kms_t)), world, device)
        upd = R ** 3 * TSDF_F
        local_upd = (z1 - z0) * R * R * TSDF_F
        comp_bytes = (z1 - z0) * R * R * 16 + depth.numel() * 4
        tsdf = {
            "metric": "TSDF Mvoxel/sec", "value": upd / (t_ms * 1e-3) / 1e6, "unit": "Mvoxel-updates/s",
            "ms_per_step": t_ms, "scaling": "strong", "dtype": "f32",
            "config": {"workload": f"C5: {R}^3 grid x {TSDF_F} depth maps {syn.IMG_W}x{syn.IMG_H}",
                       "parallelism": f"z-slabs/{world}" + (" + 1 all-gather of the depth block table" if world > 1
                                                             else ""),
                       "slabs": [list(ab) for ab in slabs],
                       "slab_cut": (f"re-cut from measured fusion times ({args.rebalance_rounds} rounds, "
                                    "dist.rebalance_slabs)" if rebalance else "equal thickness")},
            "roofline": {"bound": "valu", "kernel": "tsdf_fuse_kernel + pre-passes", "kernel_ms": tk_ms, "unit": "TFLOP/s",
                         "achieved": 32.0 * local_upd / (tk_ms * 1e-3) / 1e12, "peak": PEAK_FP32_TFLOPS,
                         "frac": (32.0 * local_upd / (tk_ms * 1e-3) / 1e12) / PEAK_FP32_TFLOPS,
                         "achieved_hbm_gbs": comp_bytes / (tk_ms * 1e-3) / 1e9, "peak_hbm_gbs": PEAK_HBM_GBS,
                         "traffic": pmc_traffic("tsdf", (z1 - z0) / R),
                         "traffic_unit": "bytes per step (every pre-pass + the fusion, profiles/r6/traffic.json)"},
            "updated_voxel_frac": float((Wt[z0:z1] > 0).float().mean().item()),
        }
        del depth, T, Wt
        torch.cuda.empty_cache()
        if cpu:
            tsdf["cpu_baseline"] = tsdf_cpu_leg(syn)
        result["secondary"] = [tsdf]
        # BASELINE's metric is "pairs/s + TSDF Mvoxel/s": the TSDF half at the top level too
        result["tsdf_value"] = tsdf["value"]
        result["tsdf_unit"] = tsdf["unit"]
        result["tsdf_ms_per_step"] = tsdf["ms_per_step"]
        result["tsdf_roofline"] = {k: tsdf["roofline"][k] for k in ("bound", "achieved", "peak", "unit", "frac",
                                                                   "kernel_ms", "traffic")}

        # ---------------- BA: DLT + residual + FD Jacobian ------------------
        ba = ba_line(sfm, syn, device, args, barrier, cpu=cpu)
        result["secondary"].append(ba)

        if world == 1:
            result["secondary"].append(ba_solve_line(sfm, syn, device, args, barrier, cpu=cpu))
            result["secondary"].append(c2_line(sfm, syn, device, args, barrier, cpu=cpu))
            result["secondary"].append(int8_line(sfm, syn, device, args, barrier, cpu=cpu, exact_ms=ms_per_step))
            result["secondary"].extend(voxel_and_vq_lines(sfm, syn, device, args, barrier, cpu=cpu))
            result["secondary"].append(verify_line(sfm, syn, device, args, barrier, cpu=cpu))
            result["secondary"].append(pnp_line(sfm, syn, device, args, barrier, cpu=cpu))
            result["secondary"].append(train_line(sfm, syn, device, args, barrier, cpu=cpu))
            result["secondary"].append(sdf_train_line(sfm, syn, device, args, barrier, cpu=cpu))

    # ---------------- CPU baseline (rank 0, N=1 only) ------------------------
    if cpu:
        match_cpu = match_cpu_leg_gemm(xcpu, pairs_all, sample)
        match_cpu["sample"] += f"; linear extrapolation to all {P} pairs = {P / match_cpu['value']:.0f} s"
        result["cpu_baseline"] = match_cpu
        # the exact-float oracle (a deliberately scalar k-loop, the parity checker) timed beside it,
        # NOT the baseline: it is ~30x slower than the GEMM form a host user would run
        ex = match_cpu_leg_exact(xcpu, pairs_all, sample[:8])
        result["cpu_exact_oracle"] = {k: ex[k] for k in ("value", "value_1thread", "unit", "cores", "sample")}
        result["host"] = host_info()
        if "secondary" in result:
            comp = composite_line(result, match_cpu, result["secondary"][1], result["secondary"][0])
            if comp is not None:
                result["secondary"].insert(0, comp)

    if rank == 0:
        if "tsdf_value" in result:   # last key: the end of the line is what a truncated tail keeps
            int8 = next((x for x in result.get("secondary", []) if x.get("metric", "").startswith("quantised")), {})
            result["headline"] = {"match_mode": "exact-float", "pairs_per_s": result["value"],
                                  "match_ms_per_step": result["ms_per_step"],
                                  "int8_mode_ms_per_step": int8.get("ms_per_step"),
                                  "match_frac": result["roofline"]["frac"], "tsdf_mvoxel_per_s": result["tsdf_value"],
                                  "tsdf_ms_per_step": result["tsdf_ms_per_step"],
                                  "tsdf_frac": result["tsdf_roofline"]["frac"], "n_gpus": world}
        print(json.dumps(result), file=out, flush=True)
    if comm is not None:
        comm.close()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
