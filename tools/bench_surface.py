"""Time the TSDF surface extractor (sfmhip_tsdf_surface_count + _emit) on the fused C5
scene (256^3 grid x 257 depth maps): HIP events around voxel.tsdf_extract_surface, 5
warm-ups, 20 timed runs, median.  Prints one JSON line (ms, V, F, and the fraction of an
HBM roofline built from the bytes the three phases have to move) and, with --out, writes
it to a file (profiles/surface/).  The numpy restatement's time at 64^3 goes beside it as
context only: there is no pass/fail time."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sfm = importlib.import_module("3d_reconstruction_amd")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")

PEAK_HBM_GBS = 8000.0   # HBM3E spec, as in bench.py


def phase_bytes(D, H, W, V, F, normals=True):
    """Bytes each phase has to move at least once (work arrays included)."""
    nv, nc = D * H * W, (D - 1) * (H - 1) * (W - 1)
    classify = 8 * nv + nv + 4 * nc                 # T, Wt in; edge mask, triangle counts out
    scan = 2 * (nv + 4 * nc) + 4 * nv + 4 * nc      # two read passes; vertex / triangle offsets out
    emit = nv + 4 * nc + V * (24 if normals else 12) + F * 12   # mask, offsets in; mesh out (gathers not counted)
    return {"classify": classify, "scan": scan, "emit": emit}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--frames", type=int, default=257)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--ref-res", type=int, default=64, help="grid of the numpy reference timing (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    R = args.res
    bmin, bmax = (-1.2,) * 3, (1.2,) * 3

    def fuse(res, device):
        depth, poses, K = syn.tsdf_scene(args.frames, syn.IMG_H, syn.IMG_W, device=device)
        T = torch.zeros((res, res, res), dtype=torch.float32, device=dev)
        Wt = torch.zeros_like(T)
        sfm.tsdf_integrate(T, Wt, depth, poses, K, bmin, bmax, 3 * 2.4 / (res - 1))
        return T, Wt

    T, Wt = fuse(R, dev)
    torch.cuda.synchronize()
    times = []
    for i in range(args.warmup + args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        v, n, f = sfm.tsdf_extract_surface(T, Wt, bmin, bmax)
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    V, F = v.shape[0], f.shape[0]
    pb = phase_bytes(R, R, R, V, F)
    total = sum(pb.values())
    line = {"metric": "tsdf_extract_surface ms (count + emit, normals)", "value": ms, "unit": "ms",
            "min_ms": min(times), "max_ms": max(times), "runs": args.runs, "warmup": args.warmup,
            "grid": [R, R, R], "frames": args.frames, "vertices": V, "faces": F,
            "observed_frac": float((Wt > 0).float().mean()),
            "roofline": {"bound": "hbm", "bytes": pb, "total_bytes": total,
                         "achieved_gbs": total / (ms * 1e-3) / 1e9, "peak_gbs": PEAK_HBM_GBS,
                         "frac": total / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS},
            "device": torch.cuda.get_device_name(0)}
    if args.ref_res:
        import surface_ref as sr
        Ts, Ws = fuse(args.ref_res, dev)
        Th, Wh = Ts.cpu().numpy(), Ws.cpu().numpy()
        t0 = time.perf_counter()
        rv, _, rf = sr.extract(Th, Wh, bmin, bmax)
        line["numpy_reference"] = {"grid": [args.ref_res] * 3, "seconds": time.perf_counter() - t0,
                                   "vertices": int(rv.shape[0]), "faces": int(rf.shape[0]),
                                   "note": "context only: tests/surface_ref.py on the host, a smaller grid"}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
