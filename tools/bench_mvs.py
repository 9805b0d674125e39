"""Time census plane-sweep stereo (mvs.py, V10) on the five-camera scene of tests/mvs_ref.py at
1936 x 1296 (f, cx, cy scaled by 1296 / 192; images generated with torch on the device):
P = 128 planes uniform in inverse depth over [2, 7], view 2 against its S = 4 neighbours.
HIP events around the Python call, 5 warm-ups, 20 timed runs, median with min - max, for
  census      census_transform of the five images,
  sweep       plane_sweep of reference view 2 from the census (also as pixel x plane x source
              evaluations per second),
  filter      depth_consistency of all five swept maps,
  mvs_depth   the product call for all five views (census, three sweeps, filter).
Then closes the loop from images to a model: the five filtered depth maps are fused with
tsdf_integrate into a 128^3 grid over [-1, 1]^3 and view 2 is ray-cast; the median
|ray-cast - analytic| over the in-range pixels the ray-cast covers is reported beside the same
figure for the analytic depth maps fused the same way.  Prints one JSON line and writes it to
--out (default profiles/mvs/bench_mvs.json).  There is no pass/fail time or threshold.
--only NAME runs one of the four arms (for a kernel trace of its own), skips the fusion and
writes a file only when --out is given."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sfm = importlib.import_module("3d_reconstruction_amd")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")

ARMS = ("census", "sweep", "filter", "mvs_depth")


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


def fused_error(depth_maps, poses, K, truth, rng, res):
    """Fuse the maps into a res^3 grid over [-1, 1]^3 (mu = 3 voxels), ray-cast view 2 and
    compare it with the analytic depth over the in-range pixels it covers."""
    dev = depth_maps.device
    T = torch.zeros((res, res, res), dtype=torch.float32, device=dev)
    Wt = torch.zeros_like(T)
    box = ((-1.0,) * 3, (1.0,) * 3)
    sfm.tsdf_integrate(T, Wt, depth_maps, poses, K, box[0], box[1], 3 * 2.0 / (res - 1))
    rc = sfm.tsdf_raycast(T, Wt, poses[2:3], K[2:3], tuple(truth.shape), box[0], box[1])[0][0]
    hit = rng & (rc > 0)
    err = (rc - truth).abs()[hit]
    return {"pixels": int(hit.sum()), "in_range_pixels": int(rng.sum()),
            "median_abs_error": float(err.median()) if err.numel() else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=syn.IMG_H)
    ap.add_argument("--width", type=int, default=syn.IMG_W)
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--only", choices=ARMS, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    H, W, P = args.height, args.width, args.planes
    sc = H / 192.0
    grey, truth, poses, K = syn.mvs_scene(H, W, 220.0 * sc, 128.0 * sc, 96.0 * sc, device=dev)
    planes = sfm.inverse_depth_planes(2.0, 7.0, P)
    lists = [[s for s in range(5) if s != r and abs(s - r) <= 2] for r in range(5)]
    srcs = torch.full((5, 4), -1, dtype=torch.int32)
    for r, nb in enumerate(lists):
        srcs[r, :len(nb)] = torch.tensor(nb, dtype=torch.int32)
    srcs = srcs.to(dev)
    refs = torch.arange(5, dtype=torch.int32, device=dev)
    cen = sfm.census_transform(grey)
    swept = sfm.mvs_depth(grey, poses, K, lists, planes, min_consistent=0)   # min_consistent 0: the swept maps
    torch.cuda.synchronize()
    arms = {
        "census": lambda: sfm.census_transform(grey),
        "sweep": lambda: sfm.plane_sweep(cen, poses, K, [2], [lists[2]], planes),
        "filter": lambda: sfm.depth_consistency(swept, poses, K, refs, srcs),
        "mvs_depth": lambda: sfm.mvs_depth(grey, poses, K, lists, planes),
    }
    res = {}
    for arm, fn in arms.items():
        if args.only and arm != args.only:
            continue
        _, res[arm] = timed(fn, args.warmup, args.runs)
    if "sweep" in res:
        res["sweep"]["evaluations"] = H * W * P * len(lists[2])
        res["sweep"]["evaluations_per_s"] = res["sweep"]["evaluations"] / (res["sweep"]["median_ms"] * 1e-3)
    line = {"metric": "census plane-sweep stereo on the five-camera scene, ms per call (median of runs)", "unit": "ms",
            "image": [H, W], "planes": P, "sources": len(lists[2]), "agg_radius": 2, "results": res,
            "runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    if not args.only:
        depth = sfm.mvs_depth(grey, poses, K, lists, planes)
        t2 = truth[2]
        b = int(round(8 * sc))
        rng = torch.zeros_like(t2, dtype=torch.bool)
        rng[b:H - b, b:W - b] = True
        rng &= (t2 > 2.5) & (t2 < 5.0)
        d2 = depth[2]
        ok = rng & (d2 > 0)
        rel = ((d2 - t2).abs() / t2.clamp_min(1e-6))[ok]
        line["view_2"] = {"filtered_completeness": float(ok.sum() / rng.sum()),
                          "within_2pc": float((rel <= 0.02).float().mean()),
                          "median_abs_error": float((d2 - t2).abs()[ok].median())}
        line["fusion"] = {"grid": [args.grid] * 3, "box": [-1.0, 1.0],
                          "stereo": fused_error(depth, poses, K, t2, rng, args.grid),
                          "analytic": fused_error(truth, poses, K, t2, rng, args.grid)}
    text = json.dumps(line)
    print(text)
    if args.out is None and not args.only:
        args.out = os.path.join(ROOT, "profiles", "mvs", "bench_mvs.json")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
