"""Time the V11 SIFT (features.py, sift.hip) on V = 8 views of the MVS scene at 1296 x 1936
(images generated with torch on the device): HIP events around each Python call, warm-up rounds,
then 12 interleaved rounds (every arm once per round), median with min - max, for
  pyramid       sift_pyramid (7 octaves of 6 levels), also as bytes moved over the time: every
                blur reads its source and writes its level once (the least a level-by-level
                pyramid can move), set against the 6.45 TB/s read rate of DESIGN.md,
  torch_chain   the same blur chain as separable torch.nn.functional.conv2d calls on replicate-
                padded images, same taps, same device, same process: a clock, not a reference
                (cuDNN-style accumulation order, not bit-equal),
  detect        sift_detect on that pyramid,
  orient        sift_orient of the detected records,
  describe      sift_describe of the oriented records (orient + describe also as keypoints/s),
  sift          the product call, all four with its two host read-backs of the counts.
Prints one JSON line and writes it to --out (default profiles/sift/bench_features.json).  There
is no pass/fail time or threshold.  --only NAME runs one arm (for a kernel trace of its own) and
writes a file only when --out is given."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sfm = importlib.import_module("3d_reconstruction_amd")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")
ft = sfm.features

ARMS = ("pyramid", "torch_chain", "detect", "orient", "describe", "sift")


def torch_chain(img, O, taps, radii):
    """The pyramid as separable conv2d calls: (V,1,H,W) f32, replicate padding, rows then columns."""
    out = []
    x = img[:, None].to(torch.float32)
    for o in range(O):
        for s in range(ft.L):
            if s == 0 and o > 0:
                x = out[-ft.L + ft.S][:, :, ::2, ::2].contiguous()
            else:
                r = int(radii[s])
                k = taps[s, :2 * r + 1]
                x = F.conv2d(F.pad(x, (r, r, 0, 0), mode="replicate"), k.view(1, 1, 1, -1))
                x = F.conv2d(F.pad(x, (0, 0, r, r), mode="replicate"), k.view(1, 1, -1, 1))
            out.append(x)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--height", type=int, default=1296)
    ap.add_argument("--width", type=int, default=1936)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--only", choices=ARMS, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V, H, W = args.views, args.height, args.width
    sc = H / 192.0
    grey = syn.mvs_scene(H, W, 220.0 * sc, 128.0 * sc, 96.0 * sc, n_views=V, device=dev)[0]
    O = ft.default_octaves(H, W)
    tb = ft.sift_tables()
    taps = torch.from_numpy(tb["taps"].copy()).to(dev)
    pyr = ft.sift_pyramid(grey, O)
    _, count = ft.sift_detect(pyr, H, W, O, 0)
    cap = int(count.max())
    rec, count = ft.sift_detect(pyr, H, W, O, cap)
    _, ocount = ft.sift_orient(pyr, H, W, O, rec, count, 0)
    cap_o = int(ocount.max())
    orec, ocount = ft.sift_orient(pyr, H, W, O, rec, count, cap_o)
    torch.cuda.synchronize()
    arms = {
        "pyramid": lambda: ft.sift_pyramid(grey, O),
        "torch_chain": lambda: torch_chain(grey, O, taps, tb["radii"]),
        "detect": lambda: ft.sift_detect(pyr, H, W, O, cap),
        "orient": lambda: ft.sift_orient(pyr, H, W, O, rec, count, cap_o),
        "describe": lambda: ft.sift_describe(pyr, H, W, O, orec, ocount),
        "sift": lambda: ft.sift(grey, max_num_keypoints=cap_o, cap=cap),
    }
    if args.only:
        arms = {args.only: arms[args.only]}
    ts = {a: [] for a in arms}
    for i in range(args.warmup + args.rounds):
        for a, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            del out
            if i >= args.warmup:
                ts[a].append(e0.elapsed_time(e1))
    res = {a: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for a, t in ts.items()}
    dims, per = ft.pyramid_layout(H, W, O)
    # per octave: 5 blurs read and write f32, level 0 reads u8 (octave 0) or a quarter of level S of the octave before
    moved = V * sum(h * w * (4 * 5 * 2 + 4 + (1 if o == 0 else 4)) for o, (h, w, _) in enumerate(dims))
    if "pyramid" in res:
        res["pyramid"]["bytes"] = moved
        res["pyramid"]["TB_per_s"] = moved / (res["pyramid"]["median_ms"] * 1e-3) / 1e12
        res["pyramid"]["share_of_6.45_TB_per_s"] = res["pyramid"]["TB_per_s"] / 6.45
    n_kp, n_okp = int(count.sum()), int(ocount.sum())
    if "orient" in res and "describe" in res:
        res["orient_describe_keypoints_per_s"] = n_okp / ((res["orient"]["median_ms"] + res["describe"]["median_ms"]) * 1e-3)
    line = {"metric": "SIFT feature extraction, ms per call (median of interleaved rounds)", "unit": "ms",
            "views": V, "image": [H, W], "octaves": O, "pyramid_floats_per_view": per, "keypoints": n_kp,
            "oriented_keypoints": n_okp, "results": res, "rounds": args.rounds, "warmup": args.warmup,
            "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if args.out is None and not args.only:
        args.out = os.path.join(ROOT, "profiles", "sift", "bench_features.json")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
