"""V13: planning the dense stage from a sparse reconstruction (build-defined; the semantics are
the V13 block of include/sfmhip.h).  What :func:`~.mvs.mvs_depth` and the TSDF calls leave to the
caller (source views, depth planes, the box of the voxel grid) derived from the cameras, points
and observations that :func:`~.reconstruct.global_refine` returns.

* :func:`view_pair_counts` — per pair of views, the tracks both observe and those among them with
  a usable triangulation angle.
* :func:`select_sources` — the best source views of every reference (host).
* :func:`view_depth_ranges` — a robust near / far depth per view.
* :func:`scene_bounds` — a robust box around the points.
* :func:`obs_depth`, :func:`segmented_select` — the two kernels under the last two.
* :func:`plan_dense` — all of it, with a plane count per view that follows from its range.
* :func:`plan_from_reconstruction` — the same from :func:`~.reconstruct.incremental_sfm` state.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from ._abi import call, dev, ptr, require_gpu, stream_ptr
from .geometry import ba_global_structure
from .mvs import inverse_depth_planes

PAIR_LDS_MAX_VIEWS = 200   # sfmhip_view_pair_counts counts in LDS up to this many views (include/sfmhip.h V13)
MAX_RANKS = 8


def _host(x, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype))


def _poses(poses) -> np.ndarray:
    P = _host(poses, np.float64)
    if P.ndim != 3 or P.shape[1:] != (3, 4):
        raise ValueError(f"poses must be (V,3,4), got {P.shape}")
    return P


def _points(X) -> torch.Tensor:
    Xd = dev(X if isinstance(X, torch.Tensor) else np.array(X, np.float64), torch.float64)   # a copy: X may be read-only
    if Xd.dim() != 2 or Xd.shape[1] != 3:
        raise ValueError(f"X must be (N,3), got {tuple(Xd.shape)}")
    return Xd


def _obs(obs_cam, obs_pt, V: int, N: int):
    """The caller's lists as host int64, every index inside [0, V) x [0, N) (checked here, on the
    host: the kernels are not launched on a list that fails)."""
    oc, op = _host(obs_cam, np.int64).ravel(), _host(obs_pt, np.int64).ravel()
    if oc.shape != op.shape:
        raise ValueError("obs_cam and obs_pt must have one entry per observation")
    if len(oc) and (oc.min() < 0 or oc.max() >= V or op.min() < 0 or op.max() >= N):
        raise ValueError(f"an observation index lies outside [0, {V}) x [0, {N})")
    return oc, op


def camera_centres(poses) -> np.ndarray:
    """(V,3,4) world->camera -> (V,3) f64 centres, on the host in a fixed elementwise order:
    ``c_i = -((R[0,i] t0 + R[1,i] t1) + R[2,i] t2)``."""
    P = _poses(poses)
    R, t = P[:, :, :3], P[:, :, 3]
    return -((R[:, 0, :] * t[:, 0:1] + R[:, 1, :] * t[:, 1:2]) + R[:, 2, :] * t[:, 2:3])


def obs_depth(poses, X, obs_cam, obs_pt) -> torch.Tensor:
    """Camera-frame depth of every observation (sfmhip_obs_depth): ``z`` (M,) f32 on the device,
    ``+inf`` where the depth is not finite and positive.  Indices outside [0, V) x [0, N) raise."""
    require_gpu()
    P = _poses(poses)
    Xd = _points(X)
    oc, op = _obs(obs_cam, obs_pt, len(P), Xd.shape[0])
    return _obs_depth(dev(P, torch.float64), Xd, dev(oc.astype(np.int32), torch.int32),
                      dev(op.astype(np.int32), torch.int32))


def _obs_depth(Pd, Xd, ocd, opd) -> torch.Tensor:
    z = torch.empty(ocd.shape[0], dtype=torch.float32, device=Xd.device)
    call("sfmhip_obs_depth", ptr(Pd), Pd.shape[0], ptr(Xd), Xd.shape[0], ptr(ocd), ptr(opd), ocd.shape[0], ptr(z),
         stream_ptr())
    return z


def segmented_select(values, seg_off, ranks) -> torch.Tensor:
    """Exact order statistics per segment (sfmhip_segmented_select): values (M,) f32, seg_off
    (S+1,) int64, ranks (S,R) int64, R <= 8 -> (S,R) f32 on the device.  The order is that of the
    radix key (-0.0 < +0.0, +inf and positive NaNs last); a rank outside its segment gives NaN."""
    gpu = require_gpu()
    v = dev(values if isinstance(values, torch.Tensor) else np.asarray(values, np.float32), torch.float32).reshape(-1)
    so = dev(seg_off if isinstance(seg_off, torch.Tensor) else np.asarray(seg_off, np.int64), torch.int64).reshape(-1)
    rk = dev(ranks if isinstance(ranks, torch.Tensor) else np.asarray(ranks, np.int64), torch.int64)
    if so.shape[0] < 1 or rk.dim() != 2 or rk.shape[0] != so.shape[0] - 1:
        raise ValueError(f"need seg_off (S+1,) and ranks (S,R), got {tuple(so.shape)} and {tuple(rk.shape)}")
    if rk.shape[1] > MAX_RANKS:
        raise ValueError(f"at most {MAX_RANKS} ranks per segment, got {rk.shape[1]}")
    S, R = rk.shape
    out = torch.empty((S, R), dtype=torch.float32, device=gpu)
    call("sfmhip_segmented_select", ptr(v), v.shape[0], ptr(so), S, ptr(rk), R, ptr(out), stream_ptr())
    return out


def _angle_thresholds(min_angle: float, max_angle: float):
    min_angle, max_angle = float(min_angle), float(max_angle)
    if not 0.0 <= min_angle <= max_angle <= 90.0:
        raise ValueError(f"need 0 <= min_angle <= max_angle <= 90 degrees, got {min_angle} / {max_angle}")
    lo, hi = math.cos(math.radians(max_angle)), math.cos(math.radians(min_angle))
    return lo * lo, hi * hi


def view_pair_counts(poses, X, obs_cam, obs_pt, min_angle: float = 1.0, max_angle: float = 45.0):
    """Covisibility of every pair of views (sfmhip_view_pair_counts).

    poses (V,3,4) world->camera, X (N,3), obs_cam / obs_pt (M,): observation m is point obs_pt[m]
    seen by view obs_cam[m], in any order; a repeated (view, point) row counts once.  Returns the
    device tensors ``shared`` and ``good`` (V,V) int32, symmetric with a zero diagonal:
    ``shared[a,b]`` the points both views observe, ``good[a,b]`` those whose triangulation angle
    at the point lies in [min_angle, max_angle] degrees (at most 90)."""
    gpu = require_gpu()
    P = _poses(poses)
    Xd = _points(X)
    V, N = len(P), Xd.shape[0]
    oc, op = _obs(obs_cam, obs_pt, V, N)
    c2_lo, c2_hi = _angle_thresholds(min_angle, max_angle)
    key = np.unique(op * max(V, 1) + oc)                       # sorted by (point, camera), repeats removed
    pt, cam = key // max(V, 1), key % max(V, 1)
    pt_off = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(pt, minlength=N)[:N], out=pt_off[1:])
    shared = torch.zeros((V, V), dtype=torch.int32, device=gpu)
    good = torch.zeros((V, V), dtype=torch.int32, device=gpu)
    cd, camd, offd = dev(camera_centres(P), torch.float64), dev(cam.astype(np.int32), torch.int32), dev(pt_off, torch.int64)
    call("sfmhip_view_pair_counts", ptr(cd), V, ptr(Xd), N, ptr(camd), len(cam), ptr(offd), c2_lo, c2_hi, ptr(shared),
         ptr(good), stream_ptr())
    return shared, good


def select_sources(shared, good, max_sources: int = 4, min_good: int = 16):
    """Per view a, the views b != a with ``good[a,b] >= min_good``, ordered by ``good`` descending,
    then ``shared`` descending, then index ascending; the first ``max_sources`` (at most 16).
    Runs on the host.  Returns a list of V lists."""
    max_sources = int(max_sources)
    if not 0 <= max_sources <= 16:
        raise ValueError(f"max_sources must be in [0, 16], got {max_sources}")
    sh, gd = _host(shared, np.int64), _host(good, np.int64)
    if gd.ndim != 2 or gd.shape[0] != gd.shape[1] or sh.shape != gd.shape:
        raise ValueError(f"shared and good must be (V,V), got {sh.shape} and {gd.shape}")
    out = []
    for a in range(len(gd)):
        cand = [b for b in np.nonzero(gd[a] >= min_good)[0].tolist() if b != a]
        cand.sort(key=lambda b: (-gd[a, b], -sh[a, b], b))
        out.append(cand[:max_sources])
    return out


def _quantile_ranks(n, q: float):
    """floor(q (n - 1)) and ceil((1 - q)(n - 1)) in f64, elementwise over the int64 array n."""
    m = (np.asarray(n, np.int64) - 1).astype(np.float64)
    return np.floor(q * m).astype(np.int64), np.ceil((1.0 - q) * m).astype(np.int64)


def _check_q(q: float) -> float:
    q = float(q)
    if not 0.0 <= q <= 0.5:
        raise ValueError(f"a quantile must be in [0, 0.5], got {q}")
    return q


def view_depth_ranges(poses, X, obs_cam, obs_pt, q: float = 0.02, margin: float = 0.1, min_points: int = 8):
    """A robust depth range per view.  Over the n valid (finite, positive) depths of a view's
    observations, sorted: ``lo = z[floor(q (n-1))]``, ``hi = z[ceil((1-q)(n-1))]``,
    ``near = f32(f64(lo) (1 - margin))``, ``far = f32(f64(hi) (1 + margin))``; a view with
    n < ``min_points`` gets 0 / 0.  sfmhip_obs_depth, a gather into camera order and
    sfmhip_segmented_select.  Returns ``near``, ``far`` (V,) f32 and ``count`` (V,) int64 (n), on
    the device."""
    gpu = require_gpu()
    q, margin = _check_q(q), float(margin)
    P = _poses(poses)
    Xd = _points(X)
    V, N = len(P), Xd.shape[0]
    oc, op = _obs(obs_cam, obs_pt, V, N)
    ocd = dev(oc.astype(np.int32), torch.int32)
    z = _obs_depth(dev(P, torch.float64), Xd, ocd, dev(op.astype(np.int32), torch.int32))
    order, _, cam_perm, cam_off = ba_global_structure(oc, op, V, N)
    zc = z[dev(order[cam_perm], torch.int64)]                    # camera by camera
    valid = z < float("inf")
    count = torch.bincount(ocd[valid].to(torch.int64), minlength=V)[:V] if V else torch.zeros(0, dtype=torch.int64,
                                                                                               device=gpu)
    n = count.cpu().numpy()
    r0, r1 = _quantile_ranks(n, q)
    sel = segmented_select(zc, cam_off, np.stack([r0, r1], 1)).to(torch.float64)
    ok = dev(n >= max(int(min_points), 1), torch.bool)
    zero = torch.zeros(V, dtype=torch.float32, device=gpu)
    near = torch.where(ok, (sel[:, 0] * (1.0 - margin)).to(torch.float32), zero)
    far = torch.where(ok, (sel[:, 1] * (1.0 + margin)).to(torch.float32), zero)
    return near, far, count


def scene_bounds(X, obs_pt, q: float = 0.01, pad: float = 0.1, min_obs: int = 2):
    """A robust box around the points for the voxel grid.  Of the points whose f32-rounded
    coordinates are finite and that have at least ``min_obs`` rows in ``obs_pt``, per axis the
    order statistics ``lo``, ``hi`` of the f32 coordinates by the rank rule of
    :func:`view_depth_ranges` (one sfmhip_segmented_select over three segments), each side widened
    by ``pad`` times the axis's extent in f64: ``bmin = f32(lo - pad (hi - lo))``,
    ``bmax = f32(hi + pad (hi - lo))``.  Returns ``bmin``, ``bmax`` (3,) f32 on the device; zeros
    when no point qualifies."""
    gpu = require_gpu()
    q, pad = _check_q(q), float(pad)
    Xd = _points(X)
    N = Xd.shape[0]
    op = dev(obs_pt if isinstance(obs_pt, torch.Tensor) else np.asarray(obs_pt, np.int64), torch.int64).reshape(-1)
    if op.numel() and (int(op.min()) < 0 or int(op.max()) >= N):
        raise ValueError(f"an observation index lies outside [0, {N})")
    Xf = Xd.to(torch.float32)
    keep = torch.isfinite(Xf).all(1) & (torch.bincount(op, minlength=N)[:N] >= int(min_obs))
    n = int(keep.sum())
    if n == 0:
        return torch.zeros(3, dtype=torch.float32, device=gpu), torch.zeros(3, dtype=torch.float32, device=gpu)
    vals = Xf[keep].t().contiguous().reshape(-1)                 # x of every kept point, then y, then z
    r0, r1 = _quantile_ranks(np.array([n, n, n]), q)
    sel = segmented_select(vals, np.arange(4, dtype=np.int64) * n, np.stack([r0, r1], 1)).to(torch.float64)
    lo, hi = sel[:, 0], sel[:, 1]
    ext = hi - lo
    return (lo - pad * ext).to(torch.float32), (hi + pad * ext).to(torch.float32)


def plane_count(fx: float, baseline: float, near: float, far: float, step_px: float = 1.0, p_min: int = 8,
                p_max: int = 256) -> int:
    """``clip(ceil(((fx b) (1/near - 1/far)) / step_px) + 1, p_min, p_max)`` in f64: neighbouring
    planes are then about ``step_px`` pixels apart in a source at distance ``baseline``."""
    fx, b, near, far = np.float64(fx), np.float64(baseline), np.float64(near), np.float64(far)
    disp = ((fx * b) * (1.0 / near - 1.0 / far)) / np.float64(step_px)
    return int(min(max(math.ceil(disp) + 1, int(p_min)), int(p_max)))


def cubic_grid(bmin, bmax, longest: int = 96):
    """A voxel grid with cubic voxels over the box: ``longest`` samples along the longest axis
    (the grids of :func:`~.voxel.tsdf_integrate` sample from ``bmin`` to ``bmax`` inclusive), as
    many along the others as cover them at the same step.  f64 on the host.  Returns
    ``(D, H, W)`` (the z, y, x sample counts), ``bmin``, the enlarged ``bmax`` (tuples of 3
    floats) and the step."""
    lo, hi = _host(bmin, np.float64).ravel(), _host(bmax, np.float64).ravel()
    ext = hi - lo
    if int(longest) < 2 or not (np.isfinite(ext).all() and ext.max() > 0 and ext.min() >= 0):
        raise ValueError(f"need a finite box with a positive extent and longest >= 2, got {lo} .. {hi}, {longest}")
    step = ext.max() / (int(longest) - 1)
    n = np.maximum(np.ceil(ext / step).astype(np.int64), 1) + 1
    n[int(np.argmax(ext))] = int(longest)
    top = lo + (n - 1) * step
    return (int(n[2]), int(n[1]), int(n[0])), tuple(float(v) for v in lo), tuple(float(v) for v in top), float(step)


@dataclass
class DensePlan:
    """What :func:`plan_dense` returns: ``neighbours`` (V lists) and ``planes`` (V f32 arrays) for
    :func:`~.mvs.mvs_depth`, ``near`` / ``far`` (V,) f32 and ``count`` (V,) int64, ``bmin`` /
    ``bmax`` (3,) f32 for the TSDF calls (host arrays), and the device matrices ``shared``, ``good``."""
    neighbours: list
    near: np.ndarray
    far: np.ndarray
    count: np.ndarray
    planes: list
    bmin: np.ndarray
    bmax: np.ndarray
    shared: torch.Tensor
    good: torch.Tensor
    poses: np.ndarray | None = field(default=None)
    K: np.ndarray | None = field(default=None)
    tracks: np.ndarray | None = field(default=None)
    X: np.ndarray | None = field(default=None)


def plan_dense(poses, K, X, obs_cam, obs_pt, step_px: float = 1.0, p_min: int = 8, p_max: int = 256,
               min_angle: float = 1.0, max_angle: float = 45.0, max_sources: int = 4, min_good: int = 16,
               q: float = 0.02, margin: float = 0.1, min_points: int = 8, bounds_q: float = 0.01, pad: float = 0.1,
               min_obs: int = 2) -> DensePlan:
    """The inputs of the dense stage from a sparse reconstruction: poses (V,3,4) world->camera, K
    (V,4) [fx, fy, cx, cy], X (N,3), observations as for :func:`view_pair_counts`.

    Sources: :func:`select_sources` of :func:`view_pair_counts`.  Range: :func:`view_depth_ranges`.
    Planes of a view: :func:`~.mvs.inverse_depth_planes` (near, far, P) with
    ``P =`` :func:`plane_count` (its fx, the largest distance from its centre to a selected
    source's centre, its range).  A view without sources or without a range (0 / 0, or
    far <= near) gets an empty source list and an empty plane array: :func:`~.mvs.mvs_depth` leaves
    it all-invalid.  Box: :func:`scene_bounds` (``bounds_q``, ``pad``, ``min_obs``)."""
    P = _poses(poses)
    Kh = _host(K, np.float64)
    if Kh.shape != (len(P), 4):
        raise ValueError(f"K must be ({len(P)},4) to match the views, got {Kh.shape}")
    Xd = _points(X)
    shared, good = view_pair_counts(P, Xd, obs_cam, obs_pt, min_angle, max_angle)
    nb = select_sources(shared, good, max_sources, min_good)
    near, far, count = (t.cpu().numpy() for t in view_depth_ranges(P, Xd, obs_cam, obs_pt, q, margin, min_points))
    bmin, bmax = (t.cpu().numpy() for t in scene_bounds(Xd, obs_pt, bounds_q, pad, min_obs))
    c = camera_centres(P)
    planes = []
    for v in range(len(P)):
        if not nb[v] or not (near[v] > 0 and far[v] > near[v]):
            nb[v] = []
            planes.append(np.zeros(0, np.float32))
            continue
        d = c[nb[v]] - c[v]
        b = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max()
        planes.append(inverse_depth_planes(near[v], far[v], plane_count(Kh[v, 0], b, near[v], far[v], step_px, p_min,
                                                                        p_max)))
    return DensePlan(nb, near, far, count, planes, bmin, bmax, shared, good)


def dense_inputs_from_reconstruction(cameras, all_point3ds, img_pairs, all_matches, focal: float, size) -> dict:
    """The dense path's view of :func:`~.reconstruct.incremental_sfm` / ``global_refine`` state
    (host only).

    Observations are collected as :func:`~.reconstruct.global_refine` collects its candidates:
    for pair (i, j), keypoints idx0[w] of image i and idx1[w] of image j observe track idx3d[w];
    only registered cameras and triangulated tracks count; one observation per (camera, track)
    (of several keypoints, the one with the lowest index).  ``size`` = (W, H) of the images.

    The SfM stages work in keypoint coordinates (x - W/2, -(y - H/2)) with K = diag(f, f, 1); the
    dense kernels work in pixels with y down.  So ``poses[c] = diag(1, -1, 1) [R|t]`` (orthogonal
    with determinant -1: the dense kernels use a pose only as a 3 x 4 map and invert its rotation
    by the transpose) and ``K`` rows are (f, f, W/2, H/2): a track projects onto the
    pixel (x, y) of its keypoint.  An unregistered camera gets a zero pose and no observations.

    Returns a dict: ``poses`` (V,3,4) f64, ``K`` (V,4) f64, ``X`` (N,3) f64 (the triangulated
    tracks that are observed), ``tracks`` (N,) their track ids, and ``obs_cam``, ``obs_pt`` (rows
    of ``X``), ``obs_kp`` (keypoint indices) (M,) int64."""
    Wd, Hd = (float(s) for s in size)
    V = len(cameras)
    flip = np.diag([1.0, -1.0, 1.0])
    poses = np.zeros((V, 3, 4), np.float64)
    for c, cam in enumerate(cameras):
        if cam is not None:
            poses[c] = flip @ np.asarray(cam, np.float64)[:3, :4]
    K = np.tile(np.array([[float(focal), float(focal), Wd / 2.0, Hd / 2.0]]), (V, 1))
    have = np.array([p is not None for p in all_point3ds[0]], bool)
    cand = []
    for index, (i, j) in enumerate(img_pairs):
        idx0, idx1, idx3d = (np.asarray(a, np.int64) for a in all_matches[index])
        for c, kp in ((i, idx0), (j, idx1)):
            if cameras[c] is not None:
                ok = have[idx3d]
                cand.append(np.stack([np.full(int(ok.sum()), c, np.int64), idx3d[ok], kp[ok]], 1))
    cand = np.unique(np.concatenate(cand), axis=0) if cand else np.zeros((0, 3), np.int64)
    if len(cand):   # sorted by (camera, track, keypoint): keep the first row of every (camera, track)
        first = np.ones(len(cand), bool)
        first[1:] = (cand[1:, 0] != cand[:-1, 0]) | (cand[1:, 1] != cand[:-1, 1])
        cand = cand[first]
    tracks, obs_pt = np.unique(cand[:, 1], return_inverse=True)
    X = np.stack([np.asarray(all_point3ds[0][t], np.float64).reshape(3) for t in tracks]) if len(tracks) \
        else np.zeros((0, 3))
    return dict(poses=poses, K=K, X=X, tracks=tracks, obs_cam=cand[:, 0].copy(), obs_pt=obs_pt.ravel().astype(np.int64),
                obs_kp=cand[:, 2].copy())


def plan_from_reconstruction(cameras, all_point3ds, img_pairs, all_matches, focal: float, size, **knobs) -> DensePlan:
    """:func:`plan_dense` of :func:`~.reconstruct.incremental_sfm` / ``global_refine`` state, through
    :func:`dense_inputs_from_reconstruction`: an unregistered camera becomes a view without
    sources.  ``knobs``: the keyword arguments of :func:`plan_dense`.  The result also holds the
    dense-path ``poses`` (V,3,4) f64 and ``K`` (V,4) f64 to hand to :func:`~.mvs.mvs_depth` and the
    TSDF calls, ``X`` (N,3) f64 and ``tracks`` (N,), the track id of every row of ``X``."""
    d = dense_inputs_from_reconstruction(cameras, all_point3ds, img_pairs, all_matches, focal, size)
    plan = plan_dense(d["poses"], d["K"], d["X"], d["obs_cam"], d["obs_pt"], **knobs)
    plan.poses, plan.K, plan.tracks, plan.X = d["poses"], d["K"], d["tracks"], d["X"]
    return plan
