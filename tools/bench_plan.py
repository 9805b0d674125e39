"""Time the dense-stage planner (plan.py, V13) at V = 257 views and 1 M tracks of lengths 2 to 12
(a track is seen by consecutive views of an orbit; points uniform in the unit box), against the
numpy restatement tests/plan_ref.py timed on the same host.  HIP events around the Python call
for the three kernels (device inputs prepared beforehand), 3 warm-ups, 10 timed runs, median with
min - max:
  obs_depth     sfmhip_obs_depth over all observations,
  pair_counts   sfmhip_view_pair_counts (memsets, the count kernel, the mirror), and once more with
                SFMHIP_PLAN_GLOBAL unset at --lds-views views (default 200, the largest count whose
                triangles fit the LDS) on the same tracks folded onto those views,
  select        sfmhip_segmented_select of two ranks per view over the depths in camera order,
  select_3      the same kernel over three segments of N values (the scene box),
and wall-clock time (host work, uploads and kernels, synchronised) for plan_dense, beside the
wall-clock time of the restatement's plan_dense and of its parts.  The plan of the device and the
restatement's are compared for equal bits.  Prints one JSON line and writes it to --out (default
profiles/plan/bench_plan.json).  There is no pass/fail time or threshold."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
sfm = importlib.import_module("3d_reconstruction_amd")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")
abi = importlib.import_module("3d_reconstruction_amd._abi")
import plan_ref as pr  # noqa: E402


def timed(fn, warmup, runs):
    ts = []
    for i in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return out, {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def wall(fn, runs):
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def scene(V, N, seed):
    rng = np.random.default_rng(seed)
    Rs, ts = syn.orbit_cameras(V, seed=seed)
    poses = np.concatenate([Rs, ts[:, :, None]], 2)
    X = rng.uniform(-1, 1, (N, 3))
    L = rng.integers(2, 13, N)
    start = rng.integers(0, V, N)
    pt = np.repeat(np.arange(N), L)
    within = np.arange(len(pt)) - np.repeat(np.cumsum(L) - L, L)
    cam = (np.repeat(start, L) + within) % V
    K = np.tile(np.array([[syn.FOCAL, syn.FOCAL, syn.IMG_W / 2.0, syn.IMG_H / 2.0]]), (V, 1))
    return poses, K, X, cam.astype(np.int64), pt.astype(np.int64)


def pair_inputs(poses, X, cam, pt, dev):
    V, N = len(poses), len(X)
    cs, _, pt_off = pr.sorted_unique_obs(cam, pt, V, N)
    return dict(V=V, N=N, M=len(cs), c=torch.from_numpy(pr.camera_centres(poses)).to(dev),
                X=torch.from_numpy(X).to(dev), cam=torch.from_numpy(cs.astype(np.int32)).to(dev),
                off=torch.from_numpy(pt_off).to(dev), shared=torch.zeros((V, V), dtype=torch.int32, device=dev),
                good=torch.zeros((V, V), dtype=torch.int32, device=dev))


def pair_call(a, c2):
    abi.call("sfmhip_view_pair_counts", a["c"].data_ptr(), a["V"], a["X"].data_ptr(), a["N"], a["cam"].data_ptr(), a["M"],
             a["off"].data_ptr(), c2[0], c2[1], a["shared"].data_ptr(), a["good"].data_ptr(), abi.stream_ptr())
    return a["shared"], a["good"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=257)
    ap.add_argument("--tracks", type=int, default=1_000_000)
    ap.add_argument("--lds-views", type=int, default=sfm.plan.PAIR_LDS_MAX_VIEWS)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--plan-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan", "bench_plan.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V, N = args.views, args.tracks
    poses, K, X, cam, pt = scene(V, N, 51)
    M = len(cam)
    c2 = pr.angle_thresholds(1.0, 45.0)
    res, ref = {}, {}

    Pd, Xd = torch.from_numpy(poses).to(dev), torch.from_numpy(X).to(dev)
    ocd, opd = torch.from_numpy(cam.astype(np.int32)).to(dev), torch.from_numpy(pt.astype(np.int32)).to(dev)
    z, res["obs_depth"] = timed(lambda: sfm.plan._obs_depth(Pd, Xd, ocd, opd), args.warmup, args.runs)
    a = pair_inputs(poses, X, cam, pt, dev)
    (shared, good), res["pair_counts"] = timed(lambda: pair_call(a, c2), args.warmup, args.runs)
    shared, good = shared.cpu().numpy(), good.cpu().numpy()
    res["pair_counts"]["pairs"] = int(shared.sum()) // 2
    Vl = args.lds_views
    al = pair_inputs(poses[:Vl], X, cam % Vl, pt, dev)
    _, res["pair_counts_lds"] = timed(lambda: pair_call(al, c2), args.warmup, args.runs)
    res["pair_counts_lds"]["views"] = Vl
    res["pair_counts_lds"]["pairs"] = int(al["shared"].sum().item()) // 2
    os.environ["SFMHIP_PLAN_GLOBAL"] = "1"
    sfm.knobs_reload()
    _, res["pair_counts_lds_views_global_path"] = timed(lambda: pair_call(al, c2), args.warmup, args.runs)
    del os.environ["SFMHIP_PLAN_GLOBAL"]
    sfm.knobs_reload()

    order = np.argsort(cam, kind="stable")
    cam_off = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(cam, minlength=V), out=cam_off[1:])
    zc = z[torch.from_numpy(order).to(dev)]
    n = np.diff(cam_off)
    r0, r1 = sfm.plan._quantile_ranks(n, 0.02)
    so, rk = torch.from_numpy(cam_off).to(dev), torch.from_numpy(np.stack([r0, r1], 1)).to(dev)
    _, res["select"] = timed(lambda: sfm.segmented_select(zc, so, rk), args.warmup, args.runs)
    vals = Xd.to(torch.float32).t().contiguous().reshape(-1)
    b0, b1 = sfm.plan._quantile_ranks(np.array([N] * 3), 0.01)
    so3, rk3 = torch.arange(4, device=dev) * N, torch.from_numpy(np.stack([b0, b1], 1)).to(dev)
    _, res["select_3"] = timed(lambda: sfm.segmented_select(vals, so3, rk3), args.warmup, args.runs)

    plan, res["plan_dense_wall"] = wall(lambda: sfm.plan_dense(poses, K, X, cam, pt), args.plan_runs)

    _, ref["obs_depth"] = wall(lambda: pr.obs_depth(poses, X, cam, pt), 1)
    (rs, rg), ref["pair_counts"] = wall(lambda: pr.view_pair_counts(poses, X, cam, pt), 1)
    _, ref["depth_ranges"] = wall(lambda: pr.view_depth_ranges(poses, X, cam, pt), 1)
    _, ref["scene_bounds"] = wall(lambda: pr.scene_bounds(X, pt), 1)
    rplan, ref["plan_dense_wall"] = wall(lambda: pr.plan_dense(poses, K, X, cam, pt), 1)
    u32 = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)   # noqa: E731
    equal = (np.array_equal(shared, rs) and np.array_equal(good, rg) and plan.neighbours == rplan["neighbours"]
             and all(np.array_equal(u32(getattr(plan, k)), u32(rplan[k])) for k in ("near", "far", "bmin", "bmax"))
             and all(np.array_equal(u32(p), u32(q)) for p, q in zip(plan.planes, rplan["planes"]))
             and np.array_equal(plan.shared.cpu().numpy(), rs))
    line = {"metric": "dense-stage planner, ms per call (median of runs); kernels by HIP events, *_wall by the host clock",
            "unit": "ms", "views": V, "tracks": N, "observations": M, "track_lengths": [2, 12], "results": res,
            "numpy_restatement_wall": ref, "bit_equal_with_restatement": bool(equal),
            "planes_per_view_min_max": [int(min(len(p) for p in plan.planes)), int(max(len(p) for p in plan.planes))],
            "runs": args.runs, "warmup": args.warmup, "plan_runs": args.plan_runs,
            "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
