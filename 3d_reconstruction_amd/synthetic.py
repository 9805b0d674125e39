"""Synthetic workloads of BASELINE.json's configs (there is no network for the
real dataset's features or depth maps).  Generated with torch on any device
from a seed, so the same call gives the same data on CPU (tests / oracle) and
GPU (bench) up to the generator's device stream.

* C2: 64 images x 2048 SIFT-128 (integer values 0..255 stored as f32)
* C3/C4: 257 images x 4096 SuperPoint-256 (L2-normalised f32)
* BA/DLT scene: cameras on an orbit with the sfm.py camera (f = 2378.98305085,
  principal point 0), noisy observations of random 3D points per pair
* C5: 257 analytic depth maps (plane + spheres) 1936 x 1296 around a 256^3 grid
"""
from __future__ import annotations

import math

import numpy as np
import torch

FOCAL = 2378.98305085   # sfm.py:24
IMG_W, IMG_H = 1936, 1296


def _gen(device, seed):
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return g


def _shared_indices(n_img, m, share, window, g, device):
    """Pool index of every (image, slot): own feature, or with prob ``share`` a
    random feature of an image within +-window (the overlap between views)."""
    k = torch.arange(n_img, device=device)[:, None].expand(n_img, m)
    s = torch.arange(m, device=device)[None, :].expand(n_img, m)
    own = k * m + s
    nb = (k + torch.randint(-window, window + 1, (n_img, m), generator=g, device=device)).clamp(0, n_img - 1)
    other = nb * m + torch.randint(0, m, (n_img, m), generator=g, device=device)
    pick = torch.rand((n_img, m), generator=g, device=device) < share
    return torch.where(pick, other, own)


def sift_like(n_img=64, m=2048, d=128, seed=0, share=0.4, window=3, noise=8.0, device="cpu"):
    """f32 (n_img, m, d) with integer values in 0..255 (config C2)."""
    g = _gen(device, seed)
    pool = torch.randint(0, 256, (n_img * m, d), generator=g, device=device, dtype=torch.int16).float()
    idx = _shared_indices(n_img, m, share, window, g, device)
    x = pool[idx] + noise * torch.randn((n_img, m, d), generator=g, device=device)
    return x.round_().clamp_(0, 255)


def superpoint_like(n_img=257, m=4096, d=256, seed=1, share=0.4, window=3, noise=0.08, device="cpu"):
    """L2-normalised f32 (n_img, m, d) (configs C3/C4)."""
    g = _gen(device, seed)
    pool = torch.randn((n_img * m, d), generator=g, device=device)
    pool = pool / pool.norm(dim=1, keepdim=True)
    idx = _shared_indices(n_img, m, share, window, g, device)
    x = pool[idx]
    x = x + noise * torch.randn(x.shape, generator=g, device=device) / math.sqrt(d)
    return x / x.norm(dim=-1, keepdim=True)


# ---------------------------------------------------------------------------
def _rodrigues_np(r):
    th = float(np.linalg.norm(r))
    if th < 1e-15:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def _look_at(c, target=np.zeros(3), up=np.array([0.0, 1.0, 0.0])):
    """World->camera R, t for a camera at c looking at target (z forward)."""
    z = target - c
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ c


def orbit_cameras(n, radius=4.0, height=0.6, seed=3):
    rng = np.random.default_rng(seed)
    Rs, ts = [], []
    for i in range(n):
        a = 2 * math.pi * i / n
        c = np.array([radius * math.cos(a), height + 0.2 * rng.standard_normal(), radius * math.sin(a)])
        R, t = _look_at(c)
        Rs.append(R)
        ts.append(t)
    return np.stack(Rs), np.stack(ts)


def ba_scene(n_pairs=256, n_obs=4096, seed=4, noise_px=0.5):
    """Per pair (i, i+1): P (n_pairs,2,3,4), x0/x1 (2,n) for DLT; and the BA
    inputs of sfm.py:36-38 for camera j: cam (n_pairs,6)=[rvec,t], K, X (n,3)
    (perturbed initial points), pts2d (n,2) (view j); pair_of_obs (n,)."""
    rng = np.random.default_rng(seed)
    Rs, ts = orbit_cameras(n_pairs + 1, seed=seed)
    K = np.array([[FOCAL, 0, 0], [0, FOCAL, 0], [0, 0, 1.0]])
    P = np.empty((n_pairs, 2, 3, 4))
    cam = np.empty((n_pairs, 6))
    n = n_pairs * n_obs
    X = rng.uniform(-1, 1, (n, 3))
    x0 = np.empty((2, n))
    x1 = np.empty((2, n))
    for p in range(n_pairs):
        sl = slice(p * n_obs, (p + 1) * n_obs)
        for v, cidx in enumerate((p, p + 1)):
            Rt = np.hstack([Rs[cidx], ts[cidx][:, None]])
            P[p, v] = K @ Rt
            Xh = np.hstack([X[sl], np.ones((n_obs, 1))])
            pr = (P[p, v] @ Xh.T)
            uv = pr[:2] / pr[2] + rng.normal(0, noise_px, (2, n_obs))
            (x0 if v == 0 else x1)[:, sl] = uv
        # rvec of R_{j}: inverse Rodrigues via axis-angle
        R = Rs[p + 1]
        ang = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2)))
        if ang < 1e-12:
            rv = np.zeros(3)
        else:
            rv = ang / (2 * math.sin(ang)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        cam[p, :3] = rv
        cam[p, 3:] = ts[p + 1]
    pair_of_obs = np.repeat(np.arange(n_pairs, dtype=np.int32), n_obs)
    Xinit = X + rng.normal(0, 0.01, X.shape)
    Kb = np.broadcast_to(K, (n_pairs, 3, 3)).copy()
    return dict(P=P, x0=x0, x1=x1, cam=cam, K=Kb, X=Xinit, pts2d=x1.T.copy(), pair_of_obs=pair_of_obs)


def two_view_pairs(n_pairs=256, n_pts=2048, outlier_frac=0.3, noise_px=0.5, seed=6, step=1):
    """Matched keypoints for pairs (i, i+step) of an orbit, in the reference's
    centred pixel convention (K = diag(f, f, 1), matching.py:133): pts0/pts1
    lists of (n, 2) f32 (like m_kpts0/1, matching.py:126-127), a fraction
    ``outlier_frac`` replaced by random image points; also the true R, t
    (camera i -> camera i+step) and the inlier flags.  ``n_pts`` may be a
    per-pair sequence."""
    rng = np.random.default_rng(seed)
    Rs, ts = orbit_cameras(n_pairs + step, seed=seed)
    K = np.array([[FOCAL, 0, 0], [0, FOCAL, 0], [0, 0, 1.0]])
    sizes = np.broadcast_to(np.asarray(n_pts), (n_pairs,))
    out = dict(pts0=[], pts1=[], R=[], t=[], inlier=[], K=K)
    for p in range(n_pairs):
        n = int(sizes[p])
        X = rng.uniform(-1, 1, (n, 3))
        uv = []
        for c in (p, p + step):
            Xc = X @ Rs[c].T + ts[c]
            uv.append(Xc[:, :2] / Xc[:, 2:] * FOCAL + rng.normal(0, noise_px, (n, 2)))
        bad = rng.random(n) < outlier_frac
        uv[1][bad] = rng.uniform([-IMG_W / 2, -IMG_H / 2], [IMG_W / 2, IMG_H / 2], (int(bad.sum()), 2))
        out["pts0"].append(uv[0].astype(np.float32))
        out["pts1"].append(uv[1].astype(np.float32))
        R = Rs[p + step] @ Rs[p].T
        out["R"].append(R)
        out["t"].append(ts[p + step] - R @ ts[p])
        out["inlier"].append(~bad)
    return out


def sfm_scene(n_img=6, n_pts=800, noise_px=0.3, wrong_frac=0.08, seed=8):
    """Inputs of sfm.py's loop for a chain of pairs (0,1), (1,2), ...: every
    image sees every point (keypoints in a per-image random order, centred
    pixels, f32), all_matches[p] = [idx0, idx1, track ids] with a fraction of
    wrong correspondences, random colours."""
    rng = np.random.default_rng(seed)
    Rs, ts = orbit_cameras(4 * n_img, seed=seed)
    X = rng.uniform(-1, 1, (n_pts, 3))
    perm, pts = [], []
    for c in range(n_img):
        pm = rng.permutation(n_pts)
        Xc = X @ Rs[c].T + ts[c]
        uv = Xc[:, :2] / Xc[:, 2:] * FOCAL + rng.normal(0, noise_px, (n_pts, 2))
        kp = np.empty((n_pts, 2), np.float32)
        kp[pm] = uv                                   # keypoint pm[g] is point g
        pts.append(kp)
        perm.append(pm)
    img_pairs, all_matches = [], []
    for c in range(n_img - 1):
        g = rng.permutation(n_pts)[: int(0.9 * n_pts)]
        idx0, idx1 = perm[c][g], perm[c + 1][g].copy()
        wrong = rng.random(len(g)) < wrong_frac
        idx1[wrong] = rng.integers(0, n_pts, int(wrong.sum()))
        img_pairs.append((c, c + 1))
        all_matches.append([idx0.astype(np.int64), idx1.astype(np.int64), g.astype(np.int64)])
    colors = [rng.integers(0, 256, (n_pts, 3)).astype(np.uint8) for _ in range(n_img)]
    return dict(img_pairs=img_pairs, all_matches=all_matches, all_points=pts, all_colors=colors, X=X,
                R=Rs[:n_img], t=ts[:n_img])


def _rvec_of(R):
    ang = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2)))
    if ang < 1e-12:
        return np.zeros(3)
    return ang / (2 * math.sin(ang)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def ba_global_scene(C=6, N=200, vis=0.6, noise_px=0.3, seed=11, fixed=(0, 1), cam_rot=0.01, cam_t=0.02,
                    pt_sigma=0.02):
    """A global bundle-adjustment problem (geometry.bundle_adjust): C orbit
    cameras with the sfm.py camera, N points in [-1, 1]^3, each (camera, point)
    observed with probability ``vis`` (every point by at least two cameras)
    with ``noise_px`` pixel noise.  Returns the truth (cam_true (C,6) = rvec, t;
    X_true), the perturbed start (cam, X: free cameras moved by ``cam_rot`` rad /
    ``cam_t``, points by ``pt_sigma``; the cameras in ``fixed`` stay at the
    truth), K (C,3,3), the observation list obs_cam, obs_pt (int32), pts2d and
    cam_fixed (C,) uint8."""
    rng = np.random.default_rng(seed)
    Rs, ts = orbit_cameras(C, seed=seed)
    X = rng.uniform(-1, 1, (N, 3))
    seen = rng.random((N, C)) < vis
    for p in np.nonzero(seen.sum(1) < min(2, C))[0]:
        seen[p, rng.permutation(C)[:min(2, C)]] = True
    obs_pt, obs_cam = (a.astype(np.int32) for a in np.nonzero(seen))
    Xc = np.einsum("mij,mj->mi", Rs[obs_cam], X[obs_pt]) + ts[obs_cam]
    pts2d = Xc[:, :2] / Xc[:, 2:] * FOCAL + rng.normal(0, noise_px, (len(obs_cam), 2))
    cam_true = np.hstack([np.stack([_rvec_of(R) for R in Rs]), ts])
    cam_fixed = np.zeros(C, np.uint8)
    cam_fixed[[c for c in fixed if c < C]] = 1
    free = (cam_fixed == 0)[:, None]
    cam = cam_true + free * np.hstack([rng.normal(0, cam_rot, (C, 3)), rng.normal(0, cam_t, (C, 3))])
    K = np.broadcast_to(np.array([[FOCAL, 0, 0], [0, FOCAL, 0], [0, 0, 1.0]]), (C, 3, 3)).copy()
    return dict(cam_true=cam_true, X_true=X, cam=cam, X=X + rng.normal(0, pt_sigma, X.shape), K=K, obs_cam=obs_cam,
                obs_pt=obs_pt, pts2d=pts2d, cam_fixed=cam_fixed)


# ---------------------------------------------------------------------------
SPHERES = ((0.0, -0.2, 0.0, 0.45), (0.5, 0.1, 0.3, 0.25), (-0.45, 0.0, -0.35, 0.3))
FLOOR_Y = -0.6


def tsdf_scene(n_frames=257, Hd=IMG_H, Wd=IMG_W, focal=FOCAL, radius=4.0, seed=5, device="cpu",
               chunk_rows=256):
    """Analytic depth maps (camera z of the first hit; 0 = miss) of a floor plane
    y = FLOOR_Y plus spheres, seen from an orbit.  Returns depth (F,Hd,Wd) f32,
    poses (F,3,4) f32 world->camera, K (F,4) f32 [fx, fy, cx, cy]."""
    Rs, ts = orbit_cameras(n_frames, radius=radius, seed=seed)
    poses = np.concatenate([Rs, ts[:, :, None]], 2).astype(np.float32)
    K = np.tile(np.array([[focal, focal, Wd / 2.0, Hd / 2.0]], np.float32), (n_frames, 1))
    depth = torch.empty((n_frames, Hd, Wd), dtype=torch.float32, device=device)
    us = torch.arange(Wd, device=device, dtype=torch.float32)
    for f in range(n_frames):
        R = torch.tensor(Rs[f], dtype=torch.float32, device=device)
        c = torch.tensor(-Rs[f].T @ ts[f], dtype=torch.float32, device=device)
        for r0 in range(0, Hd, chunk_rows):
            vs = torch.arange(r0, min(Hd, r0 + chunk_rows), device=device, dtype=torch.float32)
            dc = torch.stack(torch.broadcast_tensors((us[None, :] - Wd / 2.0) / focal,
                                                     (vs[:, None] - Hd / 2.0) / focal,
                                                     torch.ones(1, device=device)), -1)  # camera dir, z = 1
            dw = dc @ R  # world direction (R^T dc), z-component 1 in camera frame
            best = torch.full(dw.shape[:2], float("inf"), device=device)
            for (sx, sy, sz, sr) in SPHERES:
                oc = c - torch.tensor([sx, sy, sz], device=device)
                a = (dw * dw).sum(-1)
                b = 2 * (dw * oc).sum(-1)
                cc = float((oc * oc).sum() - sr * sr)
                disc = b * b - 4 * a * cc
                tt = (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a)
                ok = (disc >= 0) & (tt > 0)
                best = torch.where(ok & (tt < best), tt, best)
            tp = (FLOOR_Y - c[1]) / dw[..., 1]
            okp = (tp > 0) & (dw[..., 1].abs() > 1e-9)
            best = torch.where(okp & (tp < best), tp, best)
            depth[f, r0:r0 + vs.shape[0]] = torch.where(torch.isfinite(best), best, torch.zeros_like(best))
    return depth, torch.from_numpy(poses).to(device), torch.from_numpy(K).to(device)


def tsdf_scene_colour(depth, poses, K):
    """Procedural colour images for depth maps like :func:`tsdf_scene`'s: every valid pixel
    (depth > 0) is back-projected to its world hit point X and coloured
    clip(rint(127.5 + 100 X), 0, 255), x, y, z -> r, g, b; invalid pixels are 0 and the
    fourth byte is 255.  Returns (F,Hd,Wd,4) uint8 on depth's device (frame by frame)."""
    depth = torch.as_tensor(depth)
    device = depth.device
    poses = torch.as_tensor(poses).to(device=device, dtype=torch.float64)
    K = torch.as_tensor(K).to(device=device, dtype=torch.float64)
    F, Hd, Wd = depth.shape
    out = torch.zeros((F, Hd, Wd, 4), dtype=torch.uint8, device=device)
    us = torch.arange(Wd, device=device, dtype=torch.float64)[None, :]
    vs = torch.arange(Hd, device=device, dtype=torch.float64)[:, None]
    for f in range(F):
        d = depth[f].to(torch.float64)
        fx, fy, cx, cy = (float(x) for x in K[f])
        pc = torch.stack(torch.broadcast_tensors((us - cx) / fx * d, (vs - cy) / fy * d, d), -1)   # camera frame
        X = (pc - poses[f, :, 3]) @ poses[f, :, :3]   # R^T (pc - t)
        rgb = torch.clamp(torch.round(127.5 + 100.0 * X), 0, 255).to(torch.uint8)
        out[f, ..., :3] = torch.where((d > 0)[..., None], rgb, torch.zeros_like(rgb))
        out[f, ..., 3] = 255
    return out


# ---------------------------------------------------------------------------
def _value_noise(X, cell):
    """Trilinear value noise over the integer lattice q = floor(X / cell); lattice values
    0..255 from an int64 hash that wraps as numpy's int64 does."""
    g = X / cell
    q = torch.floor(g)
    f = g - q
    q = q.to(torch.int64)
    out = torch.zeros_like(g[..., 0])
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                h = ((q[..., 0] + dx) * 73856093) ^ ((q[..., 1] + dy) * 19349663) ^ ((q[..., 2] + dz) * 83492791)
                h = (h ^ (h >> 13)) * 1274126177
                val = ((h ^ (h >> 16)) & 255).to(g.dtype)
                w = (f[..., 0] if dx else 1 - f[..., 0]) * (f[..., 1] if dy else 1 - f[..., 1]) * \
                    (f[..., 2] if dz else 1 - f[..., 2])
                out = out + w * val
    return out


def mvs_scene(Hd=192, Wd=256, focal=220.0, cx=128.0, cy=96.0, n_views=5, device="cpu", dist=None):
    """Posed grey images of :func:`tsdf_scene`'s floor and spheres for multi-view stereo: camera
    i at (3 cos a, 2.2, 3 sin a), a = 90 + 5 (i - 2) degrees, looking at the origin.  The depth
    is analytic in f64 (the ray maths of :func:`tsdf_scene`) and rounded to f32; the grey value
    of a pixel is clip(rint(0.6 N(X, 0.08) + 0.4 N(X + 17.3, 0.036)), 0, 255) at its world hit
    point X (f64 back-projection as in :func:`tsdf_scene_colour`), N trilinear value noise, so
    the views agree on the texture of a surface point; 0 where a ray hits nothing.
    ``dist=(k1, k2)`` renders through the radial model: a pixel's ray is that of its undistorted
    normalised point (the 20 fixed-point steps of ``undistort_points``), and the depth is the z
    along that ray.
    Returns grey (V,Hd,Wd) u8, depth (V,Hd,Wd) f32, poses (V,3,4) f32, K (V,4) f32."""
    f64 = torch.float64
    us = torch.arange(Wd, device=device, dtype=f64)[None, :]
    vs = torch.arange(Hd, device=device, dtype=f64)[:, None]
    poses = np.empty((n_views, 3, 4), np.float32)
    K = np.tile(np.array([[focal, focal, cx, cy]], np.float32), (n_views, 1))
    depth = torch.empty((n_views, Hd, Wd), dtype=torch.float32, device=device)
    grey = torch.zeros((n_views, Hd, Wd), dtype=torch.uint8, device=device)
    xn, yn = (us - cx) / focal, (vs - cy) / focal
    if dist is not None:
        k1, k2 = (float(k) for k in dist)
        xd, yd = torch.broadcast_tensors(xn, yn)
        xn, yn = xd, yd
        for _ in range(20):
            r2 = xn * xn + yn * yn
            d = (1.0 + k1 * r2) + k2 * (r2 * r2)
            xn, yn = xd / d, yd / d
    for i in range(n_views):
        a = math.radians(90.0 + 5.0 * (i - 2))
        c_np = np.array([3.0 * math.cos(a), 2.2, 3.0 * math.sin(a)])
        R_np, t_np = _look_at(c_np)
        poses[i, :, :3], poses[i, :, 3] = R_np, t_np
        R = torch.tensor(R_np, dtype=f64, device=device)
        c = torch.tensor(c_np, dtype=f64, device=device)
        dc = torch.stack(torch.broadcast_tensors(xn, yn, torch.ones(1, device=device, dtype=f64)), -1)
        dw = dc @ R
        best = torch.full(dw.shape[:2], float("inf"), device=device, dtype=f64)
        for (sx, sy, sz, sr) in SPHERES:
            oc = c - torch.tensor([sx, sy, sz], device=device, dtype=f64)
            qa = (dw * dw).sum(-1)
            qb = 2 * (dw * oc).sum(-1)
            qc = float((oc * oc).sum() - sr * sr)
            disc = qb * qb - 4 * qa * qc
            tt = (-qb - torch.sqrt(disc.clamp_min(0))) / (2 * qa)
            ok = (disc >= 0) & (tt > 0)
            best = torch.where(ok & (tt < best), tt, best)
        tp = (FLOOR_Y - c[1]) / dw[..., 1]
        okp = (tp > 0) & (dw[..., 1].abs() > 1e-9)
        best = torch.where(okp & (tp < best), tp, best)
        depth[i] = torch.where(torch.isfinite(best), best, torch.zeros_like(best)).to(torch.float32)
        # texture at the hit point of the rounded depth, through the rounded pose
        d = depth[i].to(f64)
        P = torch.tensor(poses[i], dtype=f64, device=device)
        fx, fy, cxx, cyy = (float(x) for x in K[i])
        if dist is None:
            pc = torch.stack(torch.broadcast_tensors((us - cxx) / fx * d, (vs - cyy) / fy * d, d), -1)
        else:
            pc = torch.stack(torch.broadcast_tensors(xn * d, yn * d, d), -1)
        X = (pc - P[:, 3]) @ P[:, :3]
        g = torch.clamp(torch.round(0.6 * _value_noise(X, 0.08) + 0.4 * _value_noise(X + 17.3, 0.036)), 0, 255)
        grey[i] = torch.where(d > 0, g, torch.zeros_like(g)).to(torch.uint8)
    return grey, depth, torch.from_numpy(poses).to(device), torch.from_numpy(K).to(device)
