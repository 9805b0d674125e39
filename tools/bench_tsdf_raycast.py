"""Time the TSDF ray-cast (sfmhip_tsdf_raycast through voxel.tsdf_raycast) on the fused C5
scene: 256^3 grid fused from 257 depth maps of 1936 x 1296 with colour, 8 of the input views
rendered at 1936 x 1296 with the default step (half a voxel), normals and colours on.
HIP events around the Python call, 5 warm-ups, 20 timed runs, median with min - max.  The two
arms SFMHIP_RAYCAST_SKIP=1 (box clipping + brick skipping) and =0 (every sample up to the hit)
alternate run by run in one process, with a knob reload between them.  Also reports, per arm,
the samples evaluated (the sum of `steps`), and once the hit fraction and the median
|rendered - input depth| in voxels.  Prints one JSON line and, with --out, writes it to a file
(profiles/raycast/).  There is no pass/fail time."""
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


def set_arm(skip):
    os.environ["SFMHIP_RAYCAST_SKIP"] = str(skip)
    sfm.knobs_reload()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--frames", type=int, default=257)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--height", type=int, default=syn.IMG_H)
    ap.add_argument("--width", type=int, default=syn.IMG_W)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    R = args.res
    bmin, bmax, trunc = (-1.2,) * 3, (1.2,) * 3, 3 * 2.4 / (R - 1)
    depth, poses, K = syn.tsdf_scene(args.frames, args.height, args.width, device=dev)
    colour = syn.tsdf_scene_colour(depth, poses, K)
    T = torch.zeros((R, R, R), dtype=torch.float32, device=dev)
    Wt = torch.zeros_like(T)
    C = torch.zeros((R, R, R, 4), dtype=torch.int32, device=dev)
    sfm.tsdf_integrate(T, Wt, depth, poses, K, bmin, bmax, trunc)
    sfm.tsdf_integrate_colour(C, depth, colour, poses, K, bmin, bmax, trunc)
    del colour
    views = [(i * args.frames) // args.views for i in range(args.views)]
    vp, vk, inp = poses[views].contiguous(), K[views].contiguous(), depth[views]
    size = (args.height, args.width)
    torch.cuda.synchronize()

    def cast(steps=False):
        return sfm.tsdf_raycast(T, Wt, vp, vk, size, bmin, bmax, normals=True, colours=C, steps=steps)

    times = {1: [], 0: []}
    for i in range(args.warmup + args.runs):
        for arm in (1, 0):
            set_arm(arm)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cast()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[arm].append(e0.elapsed_time(e1))
    rays = len(views) * size[0] * size[1]
    res, outs = {}, {}
    for arm in (1, 0):
        set_arm(arm)
        outs[arm] = cast(steps=True)
        med = statistics.median(times[arm])
        res["skip" if arm else "plain"] = {
            "median_ms": med, "min_ms": min(times[arm]), "max_ms": max(times[arm]),
            "mrays_per_s": rays / med / 1e3, "samples_evaluated": int(outs[arm][3].sum(dtype=torch.int64))}
    set_arm(1)
    d1, d0 = outs[1][0], outs[0][0]
    same = all(torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a,
                           b.view(torch.uint8) if b.dtype != torch.uint8 else b)
               for a, b in zip(outs[1][:3], outs[0][:3]))
    hit = d1 > 0
    both = hit & (inp > 0)
    vox = 2.4 / (R - 1)
    step = 0.5 * vox
    far = float((vp[:, 2, :3].abs().sum(1) * 1.2 + vp[:, 2, 3]).max())
    line = {"metric": "tsdf ray-cast of the fused C5 scene, ms per call (median of runs)", "unit": "ms", "results": res,
            "runs": args.runs, "warmup": args.warmup, "grid": [R, R, R], "frames": args.frames, "views": views,
            "image": list(size), "rays": rays, "step": step, "samples_per_ray": int((far - 0.0) // step) + 1,
            "arms_bit_identical": bool(same), "hit_fraction": float(hit.float().mean()),
            "median_abs_depth_error_voxels": float((d1[both] - inp[both]).abs().median() / vox),
            "normals": True, "colours": True, "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
