"""Time sfmhip_triangulate_tracks (triangulate.hip, S2b) on a reconstruction-sized list: 200 k tracks
over 100 orbit cameras, track lengths drawn like a real reconstruction's (floor(2 (1 + Lomax(1.5)))
clipped to [2, 40]: median 3, a tail to 40; a track is seen by consecutive views), 0.3 px noise and
10 % of the observations displaced by 20 - 100 px.  Device inputs are prepared beforehand; after the
warm-ups every timed call reports the HIP-event times of its two phases (the call's phase_ms
argument: scoring kernel, select-and-fit kernel) and the whole call is timed by events around it
(initialisation, scan and the read-back of the hypothesis total included).  The call is timed with
the tracks handed to the fit kernel in descending order of length and in list order.  The VGPR and
scratch figures come from the kernel resource report in csrc/triangulate.s (make asm-triangulate)
when that file is there.  Prints one JSON line and writes it to --out (default
profiles/triangulate/bench_retriangulate.json).  There is no pass/fail time or threshold."""
import argparse
import ctypes
import importlib
import json
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
sfm = importlib.import_module("3d_reconstruction_amd")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")
abi = importlib.import_module("3d_reconstruction_amd._abi")


def scene(C, N, seed, frac=0.10, noise_px=0.3):
    rng = np.random.default_rng(seed)
    Rs, ts = syn.orbit_cameras(C, seed=seed)
    poses = np.concatenate([Rs, ts[:, :, None]], 2)
    X = rng.uniform(-1, 1, (N, 3))
    L = np.clip(np.floor(2 * (1 + rng.pareto(1.5, N))), 2, min(40, C)).astype(np.int64)
    pt = np.repeat(np.arange(N), L)
    within = np.arange(len(pt)) - np.repeat(np.cumsum(L) - L, L)
    cam = (np.repeat(rng.integers(0, C, N), L) + within) % C
    Xc = np.einsum("mij,mj->mi", Rs[cam], X[pt]) + ts[cam]
    uv = Xc[:, :2] / Xc[:, 2:] * syn.FOCAL + rng.normal(0, noise_px, (len(pt), 2))
    out = rng.random(len(pt)) < frac
    uv[out] += rng.uniform(20, 100, (int(out.sum()), 2)) * rng.choice([-1.0, 1.0], (int(out.sum()), 2))
    return poses, cam, pt, uv, L, out


def resource_report(path):
    if not os.path.exists(path):
        return None
    text = open(path).read()
    rep = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, flags=re.S):
        name = re.search(r"tri_\w+?_kernel", m.group(1))
        if name:
            rep[name.group(0)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(0)).group(1)) for k in
                                  ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count")
                                  if re.search(r"\.%s:\s+(\d+)" % k, m.group(0))}
    return rep


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--tracks", type=int, default=200_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--asm", default=os.path.join(ROOT, "3d_reconstruction_amd", "csrc", "triangulate.s"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate", "bench_retriangulate.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    C, N = args.cameras, args.tracks
    poses, cam, pt, uv, L, out = scene(C, N, 61)
    M = len(cam)
    order, pt_off, _, _ = sfm.ba_global_structure(cam, pt, C, N)
    cam4 = np.tile([syn.FOCAL, syn.FOCAL, 0.0, 0.0], (C, 1))
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)      # noqa: E731
    d = dict(P=t(poses, torch.float64), cam=t(cam4, torch.float64), off=t(pt_off, torch.int64),
             oc=t(cam[order], torch.int32), uv=t(uv[order], torch.float64),
             by_length=t(np.argsort(-L, kind="stable"), torch.int32),
             X=torch.empty((N, 3), dtype=torch.float64, device=dev), st=torch.empty(N, dtype=torch.int32, device=dev),
             ni=torch.empty(N, dtype=torch.int32, device=dev), inl=torch.empty(M, dtype=torch.uint8, device=dev),
             res=torch.empty(M, dtype=torch.float64, device=dev))
    n_hyp = ctypes.c_int64(0)
    phase = (ctypes.c_float * 2)()
    cos_min = float(np.cos(np.radians(1.5)))

    def run(track_order, timed_phases):
        abi.call("sfmhip_triangulate_tracks", d["P"].data_ptr(), d["cam"].data_ptr(), C, d["off"].data_ptr(), N,
                 d["oc"].data_ptr(), d["uv"].data_ptr(), M, None if track_order is None else track_order.data_ptr(),
                 4.0, cos_min, 256, 3, d["X"].data_ptr(), d["st"].data_ptr(), d["ni"].data_ptr(), d["inl"].data_ptr(),
                 d["res"].data_ptr(), ctypes.addressof(n_hyp), ctypes.addressof(phase) if timed_phases else None,
                 abi.stream_ptr())

    def measure(track_order):
        score, fit, whole = [], [], []
        for i in range(args.warmup + args.runs):
            run(track_order, True)
            if i >= args.warmup:
                score.append(phase[0])
                fit.append(phase[1])
        for i in range(args.warmup + args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(track_order, False)
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                whole.append(e0.elapsed_time(e1))
        return {"score_kernel": stats(score), "fit_kernel": stats(fit), "whole_call": stats(whole)}

    res = {"fit_by_descending_length": measure(d["by_length"]), "fit_in_list_order": measure(None)}
    run(d["by_length"], False)
    torch.cuda.synchronize()
    status = d["st"].cpu().numpy()
    inl = np.empty(M, bool)
    inl[order] = d["inl"].cpu().numpy().astype(bool)
    ok_obs = (status == 0)[pt]
    best = res["fit_by_descending_length"]
    kernels_ms = best["score_kernel"]["median_ms"] + best["fit_kernel"]["median_ms"]
    line = {"metric": "robust N-view triangulation of tracks, ms per call (median of runs, HIP events)", "unit": "ms",
            "cameras": C, "tracks": N, "observations": M, "hypotheses": int(n_hyp.value),
            "track_length_median_max": [float(np.median(L)), int(L.max())], "results": res,
            "hypotheses_per_s": n_hyp.value / (best["score_kernel"]["median_ms"] * 1e-3),
            "tracks_per_s_both_kernels": N / (kernels_ms * 1e-3),
            "tracks_per_s_whole_call": N / (best["whole_call"]["median_ms"] * 1e-3),
            "score_share_of_kernels": best["score_kernel"]["median_ms"] / kernels_ms,
            "status_counts": np.bincount(status, minlength=5).tolist(),
            "inlier_is_clean_on_ok_tracks": float((inl[ok_obs] == ~out[ok_obs]).mean()),
            "kernel_resources": resource_report(args.asm), "runs": args.runs, "warmup": args.warmup,
            "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
