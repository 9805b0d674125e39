"""Time the semi-global mode of the plane sweep (mvs.py, V10 steps 4a, 4b, 5' - 7') in the setting
of tools/bench_mvs.py: the five-camera scene of tests/mvs_ref.py at 1936 x 1296 (f, cx, cy scaled by
1296 / 192; images generated with torch on the device), P = 128 planes uniform in inverse depth
over [2, 7], a = 2, view 2 against its S = 4 neighbours, p1 = 50, p2 = 400.  HIP events around the
Python call, 5 warm-ups, 20 timed runs, median with min - max, for
  cost_volume     the u16 cost volume of view 2,
  aggregate_8     sgm_aggregate of it along eight paths (with the bytes it moves per second:
                  per direction the volume is read and sm written, and sm also read by every
                  direction but the first),
  aggregate_4     the same along four paths,
  volume_select   the selection on the aggregated volume,
  smoothed        plane_sweep(..., smooth=(50, 400)), the three calls with their allocations,
  unsmoothed      plane_sweep(...) of the same view in the same process: the yardstick,
and reports smoothed / unsmoothed.  Then closes the loop as bench_mvs.py does: the five maps of
mvs_depth, smoothed and not, are fused with tsdf_integrate into a 128^3 grid over [-1, 1]^3 and
view 2 is ray-cast; the median |ray-cast - analytic| over the in-range pixels the ray-cast covers
is reported for both beside the analytic maps fused the same way.  Prints one JSON line and writes
it to --out (default profiles/mvs/bench_mvs_sgm.json).  There is no pass/fail time or threshold.
--only NAME runs one arm (for a kernel trace of its own), skips the fusion and writes a file only
when --out is given."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sfm = importlib.import_module("3d_reconstruction_amd")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")
from bench_mvs import fused_error, timed  # noqa: E402

ARMS = ("cost_volume", "aggregate_8", "aggregate_4", "volume_select", "smoothed", "unsmoothed")
READ_RATE = 6.45e12   # bytes per second: the achievable read rate DESIGN.md section 7 records for this device


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=syn.IMG_H)
    ap.add_argument("--width", type=int, default=syn.IMG_W)
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--p1", type=int, default=50)
    ap.add_argument("--p2", type=int, default=400)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--only", choices=ARMS, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    H, W, P = args.height, args.width, args.planes
    smooth = (args.p1, args.p2)
    sc = H / 192.0
    grey, truth, poses, K = syn.mvs_scene(H, W, 220.0 * sc, 128.0 * sc, 96.0 * sc, device=dev)
    planes = sfm.inverse_depth_planes(2.0, 7.0, P)
    lists = [[s for s in range(5) if s != r and abs(s - r) <= 2] for r in range(5)]
    cen = sfm.census_transform(grey)
    view = ([2], [lists[2]])
    vol = sfm.cost_volume(cen, poses, K, *view, planes)
    sm = sfm.sgm_aggregate(vol, *smooth, 8)
    torch.cuda.synchronize()
    arms = {
        "cost_volume": lambda: sfm.cost_volume(cen, poses, K, *view, planes),
        "aggregate_8": lambda: sfm.sgm_aggregate(vol, *smooth, 8),
        "aggregate_4": lambda: sfm.sgm_aggregate(vol, *smooth, 4),
        "volume_select": lambda: sfm.volume_select(sm, poses, K, *view, planes),
        "smoothed": lambda: sfm.plane_sweep(cen, poses, K, *view, planes, smooth=smooth),
        "unsmoothed": lambda: sfm.plane_sweep(cen, poses, K, *view, planes),
    }
    res = {}
    for arm, fn in arms.items():
        if args.only and arm != args.only:
            continue
        _, res[arm] = timed(fn, args.warmup, args.runs)
    for n in (8, 4):
        r = res.get(f"aggregate_{n}")
        if r:
            r["bytes"] = H * W * P * (6 + 10 * (n - 1))
            r["bytes_per_s"] = r["bytes"] / (r["median_ms"] * 1e-3)
            r["share_of_read_rate"] = r["bytes_per_s"] / READ_RATE
    line = {"metric": "semi-global plane sweep on the five-camera scene, ms per call (median of runs)", "unit": "ms",
            "image": [H, W], "planes": P, "sources": len(lists[2]), "agg_radius": 2, "p1": smooth[0], "p2": smooth[1],
            "results": res, "runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    if "smoothed" in res and "unsmoothed" in res:
        line["smoothed_over_unsmoothed"] = res["smoothed"]["median_ms"] / res["unsmoothed"]["median_ms"]
    if not args.only:
        del vol, sm
        t2 = truth[2]
        b = int(round(8 * sc))
        rng = torch.zeros_like(t2, dtype=torch.bool)
        rng[b:H - b, b:W - b] = True
        rng &= (t2 > 2.5) & (t2 < 5.0)
        line["fusion"] = {"grid": [args.grid] * 3, "box": [-1.0, 1.0],
                          "analytic": fused_error(truth, poses, K, t2, rng, args.grid)}
        for name, mode in (("unsmoothed", None), ("smoothed", smooth)):
            depth = sfm.mvs_depth(grey, poses, K, lists, planes, smooth=mode)
            ok = rng & (depth[2] > 0)
            rel = ((depth[2] - t2).abs() / t2.clamp_min(1e-6))[ok]
            line["fusion"][name] = dict(fused_error(depth, poses, K, t2, rng, args.grid),
                                        filtered_completeness=float(ok.sum() / rng.sum()),
                                        within_2pc=float((rel <= 0.02).float().mean()))
    text = json.dumps(line)
    print(text)
    if args.out is None and not args.only:
        args.out = os.path.join(ROOT, "profiles", "mvs", "bench_mvs_sgm.json")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
