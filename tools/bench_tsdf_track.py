"""Time frame-to-model tracking (sfmhip_icp_track through voxel.icp_track / tsdf_track) on the
fused C5 scene: 256^3 grid fused from 257 depth maps of 1936 x 1296; one input view's depth,
at 1936 x 1296 and sub-sampled to 484 x 324 (K scaled), is tracked from a fixed perturbation of
its pose for 10 iterations against the model ray-cast at that start pose.
HIP events around the Python call, 5 warm-ups, 20 timed runs, median with min - max, for
  icp_track    the device-resident loop on ray-cast maps made beforehand,
  tsdf_track   the product call (ray-cast + icp_track),
  host_loop    the same track driven from the host: per iteration one icp_normal_equations
               call, the sums copied back, a numpy solve and pose update.
Also reports the pairs of the last iteration and the pose errors before and after.  Prints one
JSON line and writes it to --out (default profiles/track/bench_tsdf_track.json).  There is no
pass/fail time.  --only NAME runs one of the three (for a kernel trace of its own) and writes a
file only when --out is given."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sfm = importlib.import_module("3d_reconstruction_amd")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")

TWIST = np.array([0.010, -0.012, 0.008, 0.020, -0.015, 0.025])
TRI = [(i, j) for i in range(6) for j in range(i, 6)]


def rodrigues(w):
    th = math.sqrt(float(w @ w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return math.cos(th) * np.eye(3) + (1 - math.cos(th)) * np.outer(k, k) + math.sin(th) * kx


def update(pose, delta):
    Rn = pose[:, :3] @ rodrigues(delta[:3]).T
    return np.concatenate([Rn, (pose[:, 3] - Rn @ delta[3:])[:, None]], 1)


def errors(pose, truth):
    Rd = pose[:, :3] @ truth[:, :3].T
    ang = math.acos(min(1.0, max(-1.0, (np.trace(Rd) - 1) / 2)))
    return ang, float(np.linalg.norm(pose[:, :3].T @ pose[:, 3] - truth[:, :3].T @ truth[:, 3]))


def host_track(args7, dist_max, cos_min, iters, min_pairs):
    depth, K, pose0, md, mn, mp, mk = args7
    T = pose0[0].double().cpu().numpy()
    for _ in range(iters):
        p32 = torch.from_numpy(T.astype(np.float32))[None]
        s = sfm.icp_normal_equations(depth, K, p32, md, mn, mp, mk, dist_max, cos_min=cos_min)[0].cpu().numpy()
        A = np.zeros((6, 6))
        for k, (i, j) in enumerate(TRI):
            A[i, j] = A[j, i] = s[k]
        if s[28] < min_pairs:
            break
        T = update(T, np.linalg.solve(A, -s[21:27]))
    return T


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--frames", type=int, default=257)
    ap.add_argument("--view", type=int, default=40)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dist-max", type=float, default=0.1)
    ap.add_argument("--cos-min", type=float, default=0.7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--only", choices=("icp_track", "tsdf_track", "host_loop"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    R = args.res
    bmin, bmax, trunc = (-1.2,) * 3, (1.2,) * 3, 3 * 2.4 / (R - 1)
    depth, poses, K = syn.tsdf_scene(args.frames, syn.IMG_H, syn.IMG_W, device=dev)
    T = torch.zeros((R, R, R), dtype=torch.float32, device=dev)
    Wt = torch.zeros_like(T)
    sfm.tsdf_integrate(T, Wt, depth, poses, K, bmin, bmax, trunc)
    v = args.view
    truth = poses[v].double().cpu().numpy()
    # the start pose: the true one with the twist undone
    start = update(truth, -TWIST)
    pose0 = torch.from_numpy(start.astype(np.float32))[None].to(dev)
    full = depth[v:v + 1].contiguous()
    k_full = K[v:v + 1].contiguous()
    del depth
    torch.cuda.synchronize()
    res = {}
    for name, sub in (("1936x1296", 1), ("484x324", 4)):
        dp = full[:, ::sub, ::sub].contiguous()
        kk = (k_full / sub).contiguous()
        md, mn, _ = sfm.tsdf_raycast(T, Wt, pose0, kk, tuple(dp.shape[1:]), bmin, bmax, normals=True)
        a7 = (dp, kk, pose0, md, mn, pose0, kk)
        kw = dict(cos_min=args.cos_min, iters=args.iters)
        arms = {
            "icp_track": lambda: sfm.icp_track(*a7, args.dist_max, log=True, **kw),
            "tsdf_track": lambda: sfm.tsdf_track(T, Wt, dp, kk, pose0, bmin, bmax, args.dist_max, **kw),
            "host_loop": lambda: host_track(a7, args.dist_max, args.cos_min, args.iters, 64),
        }
        r = {"image": list(dp.shape[1:]), "start_error_rad_centre": errors(start, truth)}
        for arm, fn in arms.items():
            if args.only and arm != args.only:
                continue
            out, r[arm] = timed(fn, args.warmup, args.runs)
            if arm == "icp_track":
                r["pairs_last_iteration"] = int(out[2][0, -1, 28])
                r["lost"] = bool(out[1][0])
                r["final_error_rad_centre"] = errors(out[0][0].double().cpu().numpy(), truth)
            elif arm == "host_loop":
                r["host_loop_final_error_rad_centre"] = errors(out, truth)
        res[name] = r
    line = {"metric": "frame-to-model tracking on the fused C5 scene, ms per call (median of runs)", "unit": "ms",
            "results": res, "iters": args.iters, "dist_max": args.dist_max, "cos_min": args.cos_min,
            "twist": TWIST.tolist(), "runs": args.runs, "warmup": args.warmup, "grid": [R, R, R],
            "frames": args.frames, "view": v, "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if args.out is None and not args.only:
        args.out = os.path.join(ROOT, "profiles", "track", "bench_tsdf_track.json")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
