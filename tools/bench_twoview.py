"""Time verify.find_homography_batched beside verify.find_essential_batched on the same packed batch:
256 pairs of 2048 correspondences with 30 % outliers (synthetic.two_view_pairs, the essential
benchmark's scene: a general 3D scene, so no homography explains a pair and its RANSAC runs all of
maxIters).  The essential call is the yardstick; it is the parent commit's, unchanged.  A second
batch of planar pairs (every inlier on one plane) shows the homography kernel where its niters
collapses, and the general scene at 1024, 2048 and 4096 points per pair separates the scoring (the
slope) from the rest of a chunk (the intercept).  HIP events around the Python call (device inputs packed beforehand), 3 warm-ups, 10
timed runs, median with min - max; the outputs of the last run give the hypotheses drawn per pair.
Prints one JSON line and writes it to --out (default profiles/twoview/bench_twoview.json).  There
is no pass/fail time or threshold."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
sfm = importlib.import_module("3d_reconstruction_amd")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")


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


def planar_pairs(P, n, outlier, seed):
    """P pairs of n correspondences under a random homography near the identity, 0.5 px noise."""
    rng = np.random.default_rng(seed)
    p0, p1 = [], []
    for _ in range(P):
        H = np.eye(3) + rng.normal(0, 1, (3, 3)) * np.array([[0.05, 0.05, 20], [0.05, 0.05, 20], [2e-5, 2e-5, 0]])
        a = rng.uniform([-syn.IMG_W / 2, -syn.IMG_H / 2], [syn.IMG_W / 2, syn.IMG_H / 2], (n, 2))
        q = np.column_stack([a, np.ones(n)]) @ H.T
        b = q[:, :2] / q[:, 2:3] + rng.normal(0, 0.5, (n, 2))
        bad = rng.random(n) < outlier
        b[bad] = rng.uniform([-syn.IMG_W / 2, -syn.IMG_H / 2], [syn.IMG_W / 2, syn.IMG_H / 2], (int(bad.sum()), 2))
        p0.append(a.astype(np.float32))
        p1.append(b.astype(np.float32))
    return p0, p1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twoview", "bench_twoview.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    v = sfm.verify
    P = args.pairs
    s = syn.two_view_pairs(P, args.points, outlier_frac=args.outliers, seed=6)
    a, b, of = v.pack_pairs(s["pts0"], s["pts1"])
    cam = v._cam_rows(v._cam(s["K"]), P)
    res = {}
    e, res["find_essential"] = timed(lambda: v.find_essential_batched(a, b, of, cam), args.warmup, args.runs)
    h, res["find_homography"] = timed(lambda: v.find_homography_batched(a, b, of), args.warmup, args.runs)
    pa, pb, pof = v.pack_pairs(*planar_pairs(P, args.points, args.outliers, 7))
    hp, res["find_homography_planar"] = timed(lambda: v.find_homography_batched(pa, pb, pof), args.warmup, args.runs)
    for key, r in (("find_essential", e), ("find_homography", h), ("find_homography_planar", hp)):
        it = r["iters"].cpu().numpy()
        res[key].update(us_per_pair=1e3 * res[key]["median_ms"] / P, iters_mean=float(it.mean()), iters_max=int(it.max()),
                        inliers_mean=float(r["n_inliers"].cpu().numpy().mean()))
    # the same general scene at other sizes: every pair runs all of maxIters, so the slope over the
    # points is the scoring and the intercept is everything else (draws, solves, replay, barriers)
    res["find_homography_by_points"] = {}
    for n in (1024, 2048, 4096):
        sn = syn.two_view_pairs(P, n, outlier_frac=args.outliers, seed=6)
        an, bn, ofn = v.pack_pairs(sn["pts0"], sn["pts1"])
        rn, st = timed(lambda: v.find_homography_batched(an, bn, ofn), args.warmup, args.runs)
        st["iters_mean"] = float(rn["iters"].cpu().numpy().mean())
        res["find_homography_by_points"][str(n)] = st
    line = {"metric": "two-view RANSAC, ms per batched call (median of runs), HIP events", "unit": "ms", "pairs": P,
            "points_per_pair": args.points, "outlier_frac": args.outliers, "results": res,
            "homography_over_essential": res["find_homography"]["median_ms"] / res["find_essential"]["median_ms"],
            "runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
