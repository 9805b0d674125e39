"""S1: sfm.py's per-pair ``triangulate`` (sfm.py:26-52) and its incremental
loop (sfm.py:101-131, ``incremental_sfm``) on the sfmhip kernels.

``triangulate`` (sfm.py:26-52):
GPU DLT, then the two-view bundle adjustment of camera j + the new points with
scipy ``least_squares`` driving the GPU residual and the GPU grouped-FD
Jacobian (``jac=fd_jacobian`` gives the values ``jac_sparsity=ba_sparse``
would).  Same arguments and the same in-place updates of the stage's state
(``cameras``, ``all_point3ds``) as the reference, which keeps them global.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import least_squares

from .geometry import (Rodrigues, calculate_reprojection_error, convertPointsFromHomogeneous, fd_jacobian, least_squares_ba,
                       triangulatePoints)
from . import verify as _verify

FOCAL = 2378.98305085   # sfm.py:24


def triangulate(i, j, pts0, pts1, idx0, idx1, idx3d, K, cameras, all_point3ds, all_colors, solver: str = "host"):
    """sfm.py:26-52.  Returns the focal length (K[0][0]) like the reference.

    ``solver`` for the BA of sfm.py:38: "host" = scipy's least_squares driving
    the GPU residual and FD Jacobian (the reference's iteration, one device
    round trip per evaluation); "device" = the whole TRF solve on the GPU
    (geometry.least_squares_ba: one launch, the same algorithm restated)."""
    X4 = triangulatePoints(np.matmul(K, cameras[i]), np.matmul(K, cameras[j]), pts0.T, pts1.T)
    X4 = X4 / X4[3]
    new_pts = convertPointsFromHomogeneous(X4.T)[:, 0, :]
    for w, track in enumerate(idx3d):       # later duplicates overwrite earlier ones, as in the reference
        all_point3ds[0][track] = new_pts[w]
        all_point3ds[1][track] = all_colors[i][idx0[w]]
    rvec = Rodrigues(cameras[j][:3, :3])[0].ravel()
    x0 = np.hstack((rvec, cameras[j][:3, 3].ravel(), np.stack([all_point3ds[0][t] for t in idx3d]).ravel()))
    if solver == "device":
        res = least_squares_ba(x0, K, pts1, ftol=1e-8)
    elif solver == "host":
        res = least_squares(calculate_reprojection_error, x0, jac=fd_jacobian, x_scale="jac", ftol=1e-8,
                            args=(K, pts1))
    else:
        raise ValueError(f"solver must be 'host' or 'device', got {solver!r}")
    R = Rodrigues(res.x[:3])[0]
    t = res.x[3:6]
    refined = res.x[6:].reshape(len(idx3d), 3)
    for w, track in enumerate(idx3d):
        all_point3ds[0][track] = refined[w]
    cameras[j] = np.hstack((R, t.reshape((3, 1))))
    return K[0][0]


class GpuOps:
    """The cv2 / scipy calls of sfm.py:101-131, on the sfmhip kernels."""
    findEssentialMat = staticmethod(_verify.findEssentialMat)
    recoverPose = staticmethod(_verify.recoverPose)
    solvePnPRansac = staticmethod(_verify.solvePnPRansac)
    Rodrigues = staticmethod(Rodrigues)
    triangulate = staticmethod(triangulate)


def incremental_sfm(img_pairs, all_matches, all_points, all_colors, n_images: int, focal: float = FOCAL,
                    ops=GpuOps):
    """sfm.py:101-131 -> (cameras list (None for unregistered), all_point3ds [points, colors]).

    Per pair (i, j) in BFS order: findEssentialMat RANSAC on the matched
    keypoints, keep its inliers; register camera j from recoverPose (first
    pair) or solvePnPRansac on the already-triangulated tracks; triangulate +
    bundle-adjust the new tracks that pass recoverPose's cheirality."""
    n_tracks = int(np.max(np.hstack([m[2] for m in all_matches]))) + 1
    all_point3ds = [[None] * n_tracks, [None] * n_tracks]
    cameras = [None] * n_images
    for index, (i, j) in enumerate(img_pairs):
        idx0, idx1, idx3d = (np.asarray(a) for a in all_matches[index])
        pts0 = np.asarray(all_points[i])[idx0].astype("float64")
        pts1 = np.asarray(all_points[j])[idx1].astype("float64")
        point3ds = np.array(all_point3ds[0], dtype=object)[idx3d]
        K = np.array([[focal, 0, 0], [0, focal, 0], [0, 0, 1]])
        E, mask = ops.findEssentialMat(pts0, pts1, K, _verify.RANSAC, 0.999, 1)
        keep = mask.ravel() == 1
        idx0, idx1, idx3d = idx0[keep], idx1[keep], idx3d[keep]
        pts0, pts1, point3ds = pts0[keep], pts1[keep], point3ds[keep]
        mask_ = np.array([pt is None for pt in point3ds])
        if index != 0:
            _, rvecs, t, _ = ops.solvePnPRansac(np.stack(point3ds[mask_ == 0]), pts1[mask_ == 0], K,
                                                np.zeros((5, 1), dtype=np.float32), 0)
            R, _ = ops.Rodrigues(rvecs)
            _, _, _, mask_inliers = ops.recoverPose(E, pts0, pts1, K)
        else:
            _, R, t, mask_inliers = ops.recoverPose(E, pts0, pts1, K)
        mask_ = mask_ * (mask_inliers.ravel() > 0)
        cameras[j] = np.hstack((R, np.asarray(t).reshape(3, 1)))
        if cameras[i] is None:
            cameras[i] = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])
        if np.sum(mask_) > 0:
            sel = mask_ == 1
            focal = ops.triangulate(i, j, pts0[sel], pts1[sel], idx0[sel], idx1[sel], idx3d[sel], K, cameras,
                                    all_point3ds, all_colors)
    return cameras, all_point3ds


def global_refine(cameras, all_point3ds, img_pairs, all_matches, all_points, focal: float = FOCAL,
                  gate_px: float = 4.0, fixed=None, loss: str = "linear", f_scale: float = 1.0, reject_px=None,
                  polish: bool = False, refine_intrinsics=(), **solver):
    """Global bundle adjustment of an :func:`incremental_sfm` result, in place
    (geometry.bundle_adjust; not part of the reference, whose loop only adjusts
    camera j and the new points of each pair).

    Observations come from the tracks: for pair (i, j), keypoints idx0[w] of image
    i and idx1[w] of image j observe track idx3d[w]; only registered cameras and
    triangulated tracks count, and a keypoint counts once per (camera, track).  The
    loop's RANSAC masks are not kept, so wrong correspondences are gated instead:
    an observation stays only if its reprojection error under the incoming
    reconstruction is at most ``gate_px`` (the GPU residual kernel), and tracks
    left with fewer than two observations are dropped.  ``fixed``: cameras that do
    not move (default: the first registered one, which carries the identity pose).
    ``solver``: keyword arguments of bundle_adjust.

    Free cameras and the adjusted points are written back into ``cameras`` and
    ``all_point3ds[0]`` unless the solver reports an input error.  Returns
    (result, n_obs): bundle_adjust's result object, with ``n_candidates`` (before
    the gate) and the gated list ``obs_cam``, ``obs_track``, ``pts2d`` added, and
    the number of observations adjusted.

    With a robust ``loss`` ("huber", "soft_l1", "cauchy"; scale ``f_scale`` in pixels, see
    bundle_adjust) the gate no longer has to separate right from wrong matches: ``gate_px``
    may be wide or ``np.inf``, candidates with a non-positive depth under the incoming
    reconstruction are dropped as well (one of them would end the solve with status -2), and
    after the solve an observation is an inlier iff its final residual is at most
    ``reject_px`` (default: ``gate_px`` if finite, else 4.0).  ``polish=True`` then runs a
    second, linear bundle_adjust on the inliers of the tracks that keep at least two of them,
    from the robust result.  Tracks with fewer than two inliers are set to ``None`` in
    ``all_point3ds[0]`` and ``all_point3ds[1]``.  The result (of the polish when there is
    one) gains ``inlier`` (bool, over the gated list) and ``robust`` (the first solve's
    result when polished, else ``None``; the polish's own ``residual`` covers only the
    observations it used).

    ``refine_intrinsics`` (a subset of {"f", "pp", "k1", "k2"}, see bundle_adjust) also refines the
    one camera all images share: the focal length starts at ``focal``, the distortion at 0 (so the
    pinhole gate above is right as it stands), and the result carries the refined ``K`` and
    ``dist``; a polish starts from them.  Empty (the default): the pinhole calls, unchanged."""
    from .geometry import _residual, bundle_adjust
    robust = loss != "linear"
    calib = dict(refine_intrinsics=refine_intrinsics) if len(refine_intrinsics) else {}
    if not robust and (polish or reject_px is not None):
        raise ValueError("reject_px and polish need a robust loss")
    K = np.array([[focal, 0, 0], [0, focal, 0], [0, 0, 1.0]])
    have = np.array([p is not None for p in all_point3ds[0]])
    cand = []
    for index, (i, j) in enumerate(img_pairs):
        idx0, idx1, idx3d = (np.asarray(a, np.int64) for a in all_matches[index])
        for c, kp in ((i, idx0), (j, idx1)):
            if cameras[c] is not None:
                ok = have[idx3d]
                cand.append(np.stack([np.full(int(ok.sum()), c, np.int64), idx3d[ok], kp[ok]], 1))
    cand = np.unique(np.concatenate(cand), axis=0) if cand else np.zeros((0, 3), np.int64)
    oc, ot = cand[:, 0], cand[:, 1]
    uv = np.zeros((len(cand), 2))
    keep = np.zeros(len(cand), bool)
    rvec = {}
    for c in np.unique(oc):
        sel = oc == c
        uv[sel] = np.asarray(all_points[c], np.float64)[cand[sel, 2]]
        rvec[c] = Rodrigues(np.asarray(cameras[c], np.float64)[:3, :3])[0].ravel()
        Xc = np.stack([all_point3ds[0][t] for t in ot[sel]]).astype(np.float64)
        cam6 = np.concatenate([rvec[c], np.asarray(cameras[c], np.float64)[:3, 3]])
        r = _residual(cam6, K.reshape(1, 9), Xc, uv[sel])
        keep[sel] = np.hypot(r[:, 0], r[:, 1]) <= gate_px
        if robust:
            P = np.asarray(cameras[c], np.float64)
            keep[sel] &= Xc @ P[2, :3] + P[2, 3] > 0
    n_tr = len(have)
    keep &= (np.bincount(ot[keep], minlength=n_tr) >= 2)[ot]
    oc, ot, uv = oc[keep], ot[keep], uv[keep]
    cams, cam_idx = np.unique(oc, return_inverse=True)
    trs, tr_idx = np.unique(ot, return_inverse=True)
    cam6 = np.stack([np.concatenate([rvec[c], np.asarray(cameras[c], np.float64)[:3, 3]]) for c in cams]) \
        if len(cams) else np.zeros((0, 6))
    X = np.stack([all_point3ds[0][t] for t in trs]).astype(np.float64) if len(trs) else np.zeros((0, 3))
    if fixed is None:
        first = img_pairs[0][0] if len(img_pairs) and img_pairs[0][0] in cams else (cams[0] if len(cams) else None)
        fixed = () if first is None else (first,)
    cam_fixed = np.isin(cams, np.asarray(list(fixed), np.int64)).astype(np.uint8)
    if robust:
        first = bundle_adjust(cam6, K, X, cam_idx, tr_idx, uv, cam_fixed=cam_fixed, loss=loss, f_scale=f_scale, **calib,
                              **solver)
        res, inlier = first, np.zeros(len(oc), bool)
        if first.status >= 0:
            limit = reject_px if reject_px is not None else (gate_px if np.isfinite(gate_px) else 4.0)
            inlier = first.residual <= limit
            alive = np.bincount(tr_idx[inlier], minlength=len(trs)) >= 2
            if polish:
                use = inlier & alive[tr_idx]
                again = dict(calib, dist=first.dist) if calib else {}
                res = bundle_adjust(first.cam, first.K[0] if calib and len(cams) else K, first.X, cam_idx[use],
                                    tr_idx[use], uv[use], cam_fixed=cam_fixed, **again, **solver)
            for k, c in enumerate(cams):
                if not cam_fixed[k]:
                    cameras[c] = np.hstack((Rodrigues(res.cam[k, :3])[0], res.cam[k, 3:].reshape(3, 1)))
            for k, t in enumerate(trs):
                all_point3ds[0][t] = res.X[k] if alive[k] else None
                if not alive[k]:
                    all_point3ds[1][t] = None
        res.inlier, res.robust = inlier, (first if res is not first else None)
        res.n_candidates = len(cand)
        res.obs_cam, res.obs_track, res.pts2d = oc, ot, uv
        return res, len(oc)
    res = bundle_adjust(cam6, K, X, cam_idx, tr_idx, uv, cam_fixed=cam_fixed, **calib, **solver)
    if res.status >= 0:
        for k, c in enumerate(cams):
            if not cam_fixed[k]:
                cameras[c] = np.hstack((Rodrigues(res.cam[k, :3])[0], res.cam[k, 3:].reshape(3, 1)))
        for k, t in enumerate(trs):
            all_point3ds[0][t] = res.X[k]
    res.n_candidates = len(cand)
    res.obs_cam, res.obs_track, res.pts2d = oc, ot, uv
    return res, len(oc)


def track_candidates(cameras, img_pairs, all_matches, all_points, n_tracks: int):
    """The observations the match lists hold of the registered cameras, as :func:`global_refine`
    collects them but with the tracks that have no point included: for pair (i, j), keypoints
    idx0[w] of image i and idx1[w] of image j observe track idx3d[w], once per (camera, track,
    keypoint).  Returns (cand (M,3) int64 = camera, track, keypoint, sorted; pts2d (M,2) f64)."""
    cand = []
    for index, (i, j) in enumerate(img_pairs):
        idx0, idx1, idx3d = (np.asarray(a, np.int64) for a in all_matches[index])
        for c, kp in ((i, idx0), (j, idx1)):
            if cameras[c] is not None:
                ok = (idx3d >= 0) & (idx3d < n_tracks)
                cand.append(np.stack([np.full(int(ok.sum()), c, np.int64), idx3d[ok], kp[ok]], 1))
    cand = np.unique(np.concatenate(cand), axis=0) if cand else np.zeros((0, 3), np.int64)
    uv = np.zeros((len(cand), 2))
    for c in np.unique(cand[:, 0]):
        sel = cand[:, 0] == c
        uv[sel] = np.asarray(all_points[c], np.float64)[cand[sel, 2]]
    return cand, uv


def retriangulate(cameras, all_point3ds, img_pairs, all_matches, all_points, focal: float = FOCAL, all_colors=None,
                  mode: str = "missing", **knobs):
    """Re-estimate the tracks of an :func:`incremental_sfm` / :func:`global_refine` state from all
    of their observations under the current cameras, in place (geometry.triangulate_tracks; not
    part of the reference, which gives a track the point of the pair it is first seen in).

    Candidates are :func:`track_candidates`: every keypoint of a registered camera observes its
    track, tracks without a point included.  ``mode="missing"``: only tracks that are ``None`` in
    ``all_point3ds[0]`` receive a point (tracks the first pair rejected, or that a polish
    dropped); ``mode="all"``: every track whose status is OK is replaced as well (after the
    calibration changed, say).  A track that fails keeps what it had.  A newly created track
    takes the colour of the keypoint of its first inlier observation when ``all_colors`` is
    given.  ``knobs``: dist, reproj_px, min_angle, max_hyp, refine_iters of triangulate_tracks, and
    ``K`` (3,3), which replaces the camera matrix built from ``focal`` (principal point 0) — after
    ``global_refine(..., refine_intrinsics=...)`` pass its result's ``K[0]`` and ``dist``.

    Returns triangulate_tracks' result with ``obs_cam``, ``obs_track``, ``pts2d`` (the candidate
    list its ``inlier`` and ``residual`` refer to), ``obs_kp``, ``n_new`` and ``n_replaced`` added."""
    from .geometry import triangulate_tracks
    if mode not in ("missing", "all"):
        raise ValueError(f"mode must be 'missing' or 'all', got {mode!r}")
    n_tr = len(all_point3ds[0])
    K = knobs.pop("K", None)
    K = np.array([[focal, 0, 0], [0, focal, 0], [0, 0, 1.0]]) if K is None else np.asarray(K, np.float64)
    if K.shape != (3, 3):
        raise ValueError("K must be (3, 3): the one camera all images share")
    cand, uv = track_candidates(cameras, img_pairs, all_matches, all_points, n_tr)
    oc, ot, kp = cand[:, 0], cand[:, 1], cand[:, 2]
    res = triangulate_tracks(cameras, K, oc, ot, uv, n_tracks=n_tr, **knobs)
    had = np.array([p is not None for p in all_point3ds[0]], bool)
    first = np.full(n_tr, -1, np.int64)          # the first inlier observation of every track
    idx = np.nonzero(res.inlier)[0]
    first[ot[idx[::-1]]] = idx[::-1]
    n_new = n_replaced = 0
    for t in np.nonzero(res.ok)[0]:
        if had[t] and mode != "all":
            continue
        all_point3ds[0][t] = res.X[t].copy()
        if had[t]:
            n_replaced += 1
        else:
            n_new += 1
            if all_colors is not None and first[t] >= 0:
                all_point3ds[1][t] = all_colors[oc[first[t]]][kp[first[t]]]
    res.obs_cam, res.obs_track, res.obs_kp, res.pts2d = oc, ot, kp, uv
    res.n_new, res.n_replaced = n_new, n_replaced
    return res


def save_sfm_outputs(out_dir: str, img_list, cameras, all_point3ds) -> None:
    """sfm.py:133-146 formats: reconstructed_img.txt, cameras_extrinsic.npy, points_3d.npy."""
    import os
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "reconstructed_img.txt"), "wt") as fh:
        for name, cam in zip(img_list, cameras):
            if cam is not None:
                fh.write(name + "\n")
    np.save(os.path.join(out_dir, "cameras_extrinsic.npy"), np.array([c for c in cameras if c is not None]))
    pts = np.array(all_point3ds[0], dtype=object)
    have = np.array([p is not None for p in pts])
    np.save(os.path.join(out_dir, "points_3d.npy"), np.stack(pts[have]).astype(float))
