"""S1-S5: DLT triangulation, reprojection residual and the scipy grouped
finite-difference Jacobian, with the numpy signatures ``sfm.py`` calls.

Drop-in surfaces:

* :func:`triangulatePoints` — ``cv2.triangulatePoints`` (``sfm.py:27``)
* :func:`projectPoints` — ``cv2.projectPoints`` without distortion (``sfm.py:89``)
* :func:`calculate_reprojection_error` — ``sfm.py:87-91``
* :func:`ba_sparse` — ``sfm.py:79-85``
* :func:`fd_jacobian` — a ``jac=`` callable numerically identical (to the
  tolerance in tests/) to scipy's grouped 2-point FD that
  ``least_squares(..., jac_sparsity=ba_sparse(...))`` builds (``sfm.py:37-38``)
* batched forms (:func:`triangulate_batched`, :func:`residual_jacobian_batched`)
  over many pairs' observations resident on the GPU — the benchmarked path.

``Rodrigues`` and ``convertPointsFromHomogeneous`` are host helpers for the
3x3 / per-pair bookkeeping around the hot path (``sfm.py:29,36,39``); they are
not kernels.
"""
from __future__ import annotations

import ctypes
import math
from types import SimpleNamespace

import numpy as np
import torch
from scipy.sparse import csr_matrix, lil_matrix

from ._abi import call, dev, ptr, require_gpu, stream_ptr


# ---------------------------------------------------------------------------
# host helpers (not on the hot path)
def Rodrigues(src):
    """cv2.Rodrigues: (3,)/(3,1)/(1,3) vector -> ((3,3), None) or (3,3) -> ((3,1), None)."""
    a = np.asarray(src, dtype=np.float64)
    if a.size == 3:
        rx, ry, rz = (float(v) for v in a.ravel())
        theta = math.sqrt(rx * rx + ry * ry + rz * rz)
        if theta < 2.220446049250313e-16:
            return np.eye(3), None
        c, s = math.cos(theta), math.sin(theta)
        c1 = 1.0 - c
        it = 1.0 / theta
        rx, ry, rz = rx * it, ry * it, rz * it
        rrt = np.array([rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz])
        rxm = np.array([0, -rz, ry, rz, 0, -rx, -ry, rx, 0])
        eye = np.eye(3).ravel()
        return ((c * eye + c1 * rrt) + s * rxm).reshape(3, 3), None
    if a.shape != (3, 3):
        raise ValueError("Rodrigues expects a 3-vector or a 3x3 matrix")
    # matrix -> vector (OpenCV's SVD-projected formula)
    u, _, vt = np.linalg.svd(a)
    R = u @ vt
    rx, ry, rz = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]
    s = math.sqrt((rx * rx + ry * ry + rz * rz) * 0.25)
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) * 0.5
    c = min(max(c, -1.0), 1.0)
    theta = math.acos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros((3, 1)), None
        t = (R[0, 0] + 1) * 0.5
        rx = math.sqrt(max(t, 0.0))
        t = (R[1, 1] + 1) * 0.5
        ry = math.sqrt(max(t, 0.0)) * (-1.0 if R[0, 1] < 0 else 1.0)
        t = (R[2, 2] + 1) * 0.5
        rz = math.sqrt(max(t, 0.0)) * (-1.0 if R[0, 2] < 0 else 1.0)
        if abs(rx) < abs(ry) and abs(rx) < abs(rz) and (R[1, 2] > 0) != (ry * rz > 0):
            rz = -rz
        theta /= math.sqrt(rx * rx + ry * ry + rz * rz)
        return np.array([[rx * theta], [ry * theta], [rz * theta]]), None
    vth = 1.0 / (2 * s) * theta
    return np.array([[rx * vth], [ry * vth], [rz * vth]]), None


def convertPointsFromHomogeneous(src):
    """cv2.convertPointsFromHomogeneous for (n,4) -> (n,1,3)."""
    a = np.asarray(src, dtype=np.float64).reshape(-1, 4)
    w = a[:, 3:4]
    scale = np.where(w != 0, 1.0 / np.where(w != 0, w, 1.0), 1.0)
    return (a[:, :3] * scale)[:, None, :]


def ba_sparse(len_point: int, len_x: int, y: int = 6):
    """sfm.py:79-85 — the (2n, len_x) int sparsity of the BA Jacobian."""
    n = int(len_point)
    A = lil_matrix((2 * n, int(len_x)), dtype=int)
    rows = np.arange(2 * n)
    A[rows, :y] = 1
    for c in range(3):
        cols = y + 3 * np.arange(n) + c
        A[2 * np.arange(n), cols] = 1
        A[2 * np.arange(n) + 1, cols] = 1
    return A


# ---------------------------------------------------------------------------
# GPU-backed drop-ins
def triangulatePoints(projMatr1, projMatr2, projPoints1, projPoints2):
    """cv2.triangulatePoints: P1, P2 (3,4); points (2,n) -> homogeneous (4,n) f64.

    The 4-vector is the unit-norm DLT null vector with w >= 0 (OpenCV's sign is
    arbitrary; ``X / X[3]`` is identical)."""
    P = np.stack([np.asarray(projMatr1, np.float64).reshape(3, 4),
                  np.asarray(projMatr2, np.float64).reshape(3, 4)])[None]
    x0 = np.asarray(projPoints1, np.float64).reshape(2, -1)
    x1 = np.asarray(projPoints2, np.float64).reshape(2, -1)
    n = x0.shape[1]
    if x1.shape[1] != n:
        raise ValueError("projPoints1 and projPoints2 must have the same number of points")
    X4 = triangulate_batched(dev(P, torch.float64), None, dev(x0, torch.float64), dev(x1, torch.float64))
    torch.cuda.synchronize()
    return X4.cpu().numpy()


def triangulate_batched(P: torch.Tensor, pair_of_obs: torch.Tensor | None, x0: torch.Tensor,
                        x1: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Device-resident DLT: P (n_pairs,2,3,4) f64, x0/x1 (2,n) f64 -> (4,n) f64."""
    require_gpu()
    n = x0.shape[1]
    X4 = out if out is not None else torch.empty((4, n), dtype=torch.float64, device=x0.device)
    call("sfmhip_triangulate_dlt", ptr(P), ptr(pair_of_obs), ptr(x0), ptr(x1), n, ptr(X4), stream_ptr())
    return X4


def _K_of(K):
    return np.asarray(K, np.float64).reshape(1, 9)


def projectPoints(objectPoints, rvec, tvec, cameraMatrix, distCoeffs=None):
    """cv2.projectPoints (no distortion): returns ((n,1,2) f64, None).

    The reference discards the analytic jacobian output (``sfm.py:89``)."""
    if distCoeffs is not None and np.any(np.asarray(distCoeffs) != 0):
        raise NotImplementedError("distortion coefficients are not supported (sfm.py passes None)")
    X = np.asarray(objectPoints, np.float64).reshape(-1, 3)
    cam = np.concatenate([np.asarray(rvec, np.float64).ravel(), np.asarray(tvec, np.float64).ravel()])
    r = _residual(cam, _K_of(cameraMatrix), X, None)
    return (-r).reshape(-1, 1, 2), None


def _residual(cam, K, X, pts2d):
    """Host arrays in, host (n,2) out, through sfmhip_reproj_residual_host: one pinned
    staging buffer, one copy each way and a stream synchronisation per call (scipy's
    least_squares calls this ~40 times per pair at sfm.py:38).  pts2d None = zeros."""
    require_gpu()
    n = X.shape[0]
    cam = np.ascontiguousarray(cam, np.float64)
    K = np.ascontiguousarray(K, np.float64)
    X = np.ascontiguousarray(X, np.float64)
    r = np.empty((n, 2), np.float64)
    if pts2d is not None:
        pts2d = np.ascontiguousarray(pts2d, np.float64)
        if pts2d.shape != (n, 2):
            raise ValueError("point_2D must have one (x, y) row per 3D point")
    if cam.size != 6 or K.size != 9 or X.shape != (n, 3):
        raise ValueError("cam (6,), K (3,3) and X (n,3) expected")
    call("sfmhip_reproj_residual_host", cam.ctypes.data, K.ctypes.data, X.ctypes.data,
         None if pts2d is None else pts2d.ctypes.data, n, r.ctypes.data, stream_ptr())
    return r


def calculate_reprojection_error(x, K, point_2D):
    """sfm.py:87-91: x = [rvec(3), t(3), X(3n)] -> (point_2D - proj).ravel() (2n,)."""
    x = np.asarray(x, np.float64)
    p2 = np.asarray(point_2D, np.float64).reshape(-1, 2)
    X = x[6:].reshape(len(p2), 3)
    return _residual(x[:6], _K_of(K), X, p2).ravel()


def _jac_structure(n: int):
    cols = np.empty((n, 2, 9), dtype=np.int32)
    cols[:, :, :6] = np.arange(6, dtype=np.int32)
    cols[:, :, 6:] = (6 + 3 * np.arange(n, dtype=np.int32))[:, None, None] + np.arange(3, dtype=np.int32)
    indptr = np.arange(0, 18 * n + 1, 9, dtype=np.int32)
    return cols.ravel(), indptr


def fd_jacobian(x, K, point_2D, f0=None):
    """``jac=`` callable for ``least_squares``: scipy's 2-point grouped FD of
    :func:`calculate_reprojection_error` as a CSR matrix (2n, 6+3n)."""
    x = np.asarray(x, np.float64)
    p2 = np.asarray(point_2D, np.float64).reshape(-1, 2)
    n = len(p2)
    camt = dev(x[:6].reshape(1, 6), torch.float64)
    Kt = dev(_K_of(K), torch.float64)
    Xt = dev(x[6:].reshape(n, 3), torch.float64)
    pt = dev(p2, torch.float64)
    f0t = dev(np.asarray(f0, np.float64).reshape(n, 2), torch.float64) if f0 is not None else None
    jv = torch.empty((n, 2, 9), dtype=torch.float64, device=Xt.device)
    call("sfmhip_reproj_fd_jacobian", ptr(camt), ptr(Kt), ptr(Xt), ptr(pt), None, 1, n, ptr(f0t), None,
         ptr(jv), stream_ptr())
    torch.cuda.synchronize()
    indices, indptr = _jac_structure(n)
    return csr_matrix((jv.cpu().numpy().ravel(), indices, indptr), shape=(2 * n, 6 + 3 * n))


def residual_jacobian_batched(cam: torch.Tensor, K: torch.Tensor, X: torch.Tensor, pts2d: torch.Tensor,
                              pair_of_obs: torch.Tensor | None, r: torch.Tensor | None = None,
                              jv: torch.Tensor | None = None):
    """Device-resident residual + FD Jacobian over many pairs' observations.

    cam (n_pairs,6), K (n_pairs,3,3), X (n,3), pts2d (n,2) f64; pair_of_obs (n,) int32.
    Returns r (n,2) and jvals (n,2,9) (CSR values, columns rvec, t, X_i)."""
    require_gpu()
    n = X.shape[0]
    dvc = X.device
    r = r if r is not None else torch.empty((n, 2), dtype=torch.float64, device=dvc)
    jv = jv if jv is not None else torch.empty((n, 2, 9), dtype=torch.float64, device=dvc)
    call("sfmhip_reproj_fd_jacobian", ptr(cam), ptr(K), ptr(X), ptr(pts2d), ptr(pair_of_obs),
         int(cam.shape[0]), n, None, ptr(r), ptr(jv), stream_ptr())
    return r, jv


def ba_solve_batched(cam: torch.Tensor, K: torch.Tensor, X: torch.Tensor, pts2d: torch.Tensor,
                     pair_off: torch.Tensor, ftol: float = 1e-8, xtol: float = 1e-8, gtol: float = 1e-8,
                     max_nfev: int | None = None, validate: bool = True) -> dict:
    """The BA solve of sfm.py:37-38 for every pair at once, on the GPU (ba.hip):
    scipy ``least_squares(calculate_reprojection_error, [rvec, t, X], jac_sparsity=
    ba_sparse(...), x_scale='jac', ftol=ftol)`` restated (oracle/ba.py).

    cam (P,6) and X (n,3) f64 device tensors are updated in place; K (P,3,3),
    pts2d (n,2) f64; pair_off (P+1) int64 (pair p owns observations
    [pair_off[p], pair_off[p+1])).  Returns device tensors cost (P,) f64 and
    nfev, njev, status (P,) int32 (scipy's meanings; -1 = malformed offsets).

    ``validate`` checks pair_off on the device (off[0] = 0, non-decreasing,
    off[P] = n) and raises ValueError — one reduction and a host sync; the
    kernel itself never reads or writes outside [0, n) whatever the offsets
    (a pair with bad offsets is skipped with status -1)."""
    require_gpu()
    P = int(cam.shape[0])
    for name, t, dt in (("cam", cam, torch.float64), ("K", K, torch.float64), ("X", X, torch.float64),
                        ("pts2d", pts2d, torch.float64), ("pair_off", pair_off, torch.int64)):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} device tensor")
    n = int(X.shape[0])
    if tuple(cam.shape) != (P, 6) or tuple(K.shape) != (P, 3, 3) or tuple(X.shape) != (n, 3) or \
            tuple(pts2d.shape) != (n, 2) or tuple(pair_off.shape) != (P + 1,):
        raise ValueError("shapes must be cam (P,6), K (P,3,3), X (n,3), pts2d (n,2), pair_off (P+1,)")
    dvc = cam.device
    if validate and P > 0:
        bad = (pair_off[0] != 0) | (pair_off[-1] != n) | (pair_off[1:] < pair_off[:-1]).any()
        if bool(bad.item()):
            raise ValueError("pair_off must start at 0, be non-decreasing and end at X.shape[0]")
    cost = torch.empty(P, dtype=torch.float64, device=dvc)
    nfev = torch.empty(P, dtype=torch.int32, device=dvc)
    njev = torch.empty(P, dtype=torch.int32, device=dvc)
    status = torch.empty(P, dtype=torch.int32, device=dvc)
    call("sfmhip_ba_solve", ptr(cam), ptr(K), ptr(X), ptr(pts2d), ptr(pair_off), P, n, float(ftol), float(xtol),
         float(gtol), int(max_nfev or 0), ptr(cost), ptr(nfev), ptr(njev), ptr(status), stream_ptr())
    return {"cost": cost, "nfev": nfev, "njev": njev, "status": status}


def least_squares_ba(x0, K, point_2D, ftol: float = 1e-8, xtol: float = 1e-8, gtol: float = 1e-8,
                     max_nfev: int | None = None):
    """Drop-in for sfm.py:38 ``least_squares(calculate_reprojection_error, x0,
    jac_sparsity=ba_sparse(...), x_scale='jac', ftol=1e-8, args=(K, point_2D))``
    on one pair: returns an object with scipy's ``x``, ``cost``, ``fun``,
    ``nfev``, ``njev``, ``status`` and ``success``."""
    dv = require_gpu()
    x0 = np.asarray(x0, np.float64)
    p2 = np.asarray(point_2D, np.float64).reshape(-1, 2)
    n = len(p2)
    if x0.shape != (6 + 3 * n,):
        raise ValueError(f"x0 must have 6 + 3 * {n} entries")
    cam = torch.tensor(x0[:6].reshape(1, 6), device=dv)
    X = torch.tensor(x0[6:].reshape(n, 3), device=dv)
    Kt = torch.tensor(np.asarray(K, np.float64).reshape(1, 3, 3), device=dv)
    pt = torch.tensor(p2, device=dv)
    off = torch.tensor([0, n], dtype=torch.int64, device=dv)
    res = ba_solve_batched(cam, Kt, X, pt, off, ftol, xtol, gtol, max_nfev)
    torch.cuda.synchronize()
    x = np.concatenate([cam.cpu().numpy().ravel(), X.cpu().numpy().ravel()])
    status = int(res["status"].item())
    return SimpleNamespace(x=x, cost=float(res["cost"].item()), fun=calculate_reprojection_error(x, K, p2),
                           nfev=int(res["nfev"].item()), njev=int(res["njev"].item()), status=status,
                           success=status > 0)


# ---------------------------------------------------------------------------
# K3''': global bundle adjustment (ba_global.hip; build-defined, DESIGN.md K3''')
def ba_global_structure(obs_cam, obs_pt, C: int, N: int):
    """The sorted layout ``sfmhip_ba_global*`` take, built once per solve on the host.

    Returns int64 arrays ``order`` (M,) — positions in the caller's list, sorted by
    (point, camera), repeated pairs in the caller's order —, ``pt_off`` (N+1,),
    ``cam_perm`` (M,) — positions in the sorted list, camera by camera, ascending
    inside a camera — and ``cam_off`` (C+1,).  An index outside [0, C) x [0, N) is
    not counted, so the offsets then do not end at M and the library reports the
    list as malformed."""
    obs_cam = np.asarray(obs_cam, np.int64).ravel()
    obs_pt = np.asarray(obs_pt, np.int64).ravel()
    if obs_cam.shape != obs_pt.shape:
        raise ValueError("obs_cam and obs_pt must have one entry per observation")
    # one stable sort of the combined key = lexsort((obs_cam, obs_pt)), several times faster; a list
    # that is already sorted (np.nonzero of a visibility matrix) costs a single pass
    order = np.argsort(obs_pt * max(int(C), 1) + obs_cam, kind="stable")
    cam_sorted = obs_cam[order]
    cam_perm = np.argsort(cam_sorted.astype(np.int16) if C <= 32767 else cam_sorted, kind="stable")   # int16: radix sort
    pt_off = np.zeros(N + 1, np.int64)
    cam_off = np.zeros(C + 1, np.int64)
    np.cumsum(np.bincount(obs_pt[(obs_pt >= 0) & (obs_pt < N)], minlength=N)[:N], out=pt_off[1:])
    np.cumsum(np.bincount(obs_cam[(obs_cam >= 0) & (obs_cam < C)], minlength=C)[:C], out=cam_off[1:])
    return order, pt_off, cam_perm, cam_off


def _ba_global_inputs(cam, K, X, obs_cam, obs_pt, pts2d):
    cam = np.ascontiguousarray(np.asarray(cam, np.float64).reshape(-1, 6))
    X = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1, 3))
    C, N = len(cam), len(X)
    K = np.asarray(K, np.float64)
    K = np.ascontiguousarray(np.broadcast_to(K, (C, 3, 3)) if K.shape == (3, 3) else K.reshape(C, 3, 3))
    obs_cam = np.asarray(obs_cam).ravel()
    obs_pt = np.asarray(obs_pt).ravel()
    pts2d = np.asarray(pts2d, np.float64).reshape(-1, 2)
    M = len(obs_cam)
    if len(obs_pt) != M or len(pts2d) != M:
        raise ValueError("obs_cam, obs_pt and pts2d must have one row per observation")
    if M and (np.abs(obs_cam).max() > 2 ** 31 - 1 or np.abs(obs_pt).max() > 2 ** 31 - 1):
        raise ValueError("observation indices must fit int32")
    order, pt_off, cam_perm, cam_off = ba_global_structure(obs_cam, obs_pt, C, N)
    d = dict(C=C, N=N, M=M, order=order,
             cam=dev(cam, torch.float64), K=dev(K, torch.float64), X=dev(X, torch.float64),
             obs_cam=dev(obs_cam[order].astype(np.int32), torch.int32),
             obs_pt=dev(obs_pt[order].astype(np.int32), torch.int32),
             pts2d=dev(np.ascontiguousarray(pts2d[order]), torch.float64),
             pt_off=dev(pt_off, torch.int64), cam_perm=dev(cam_perm, torch.int64), cam_off=dev(cam_off, torch.int64))
    return d


def _fixed_tensor(cam_fixed, C):
    f = np.ascontiguousarray(np.asarray(cam_fixed).astype(np.uint8).ravel())
    if f.shape != (C,):
        raise ValueError("cam_fixed must have one entry per camera")
    return dev(f, torch.uint8)


BA_LOSSES = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3}


def _ba_loss(loss, f_scale):
    if loss not in BA_LOSSES:
        raise ValueError(f"loss must be one of {sorted(BA_LOSSES)}, got {loss!r}")
    return BA_LOSSES[loss], float(f_scale)


def ba_loss_weight(e2, loss: str = "linear", f_scale: float = 1.0) -> np.ndarray:
    """The IRLS weight rho'(z), z = e2 / f_scale^2, of squared residual norms ``e2`` (numpy; the
    solver's own weights are computed on the device, this is for reporting)."""
    z = np.asarray(e2, np.float64) / (float(f_scale) * float(f_scale))
    with np.errstate(divide="ignore", invalid="ignore"):
        if loss == "huber":
            return np.where(z <= 1.0, 1.0, 1.0 / np.sqrt(z))
        if loss == "soft_l1":
            return 1.0 / np.sqrt(1.0 + z)
        if loss == "cauchy":
            return 1.0 / (1.0 + z)
    _ba_loss(loss, f_scale)
    return np.ones_like(z)


def ba_global_linearize(cam, K, X, obs_cam, obs_pt, pts2d, loss: str = "linear", f_scale: float = 1.0) -> dict:
    """Linearise the global problem at (cam, X) (``sfmhip_ba_global_linearize_robust``).

    cam (C,6) = rvec, t; K (3,3) or (C,3,3); X (N,3); one (obs_cam, obs_pt, pts2d) row
    per observation, in any order.  Returns device tensors in the SORTED order
    (``order`` maps it to the caller's list): r (M,2), Jc (M,2,6), Jp (M,2,3), and
    the blocks U (C,6,6), g_c (C,6), V (N,3,3), g_p (N,3); ``cost`` (float), and the
    layout arrays ``sfmhip_ba_global_schur_matvec`` needs.

    With a robust ``loss`` (see :func:`bundle_adjust`) r, Jc, Jp are the weighted sqrt(w) r,
    sqrt(w) Jc, sqrt(w) Jp, the blocks and ``cost`` the robust ones; ``weight`` (M,) is w per
    sorted observation (1 for the linear loss)."""
    require_gpu()
    code, f_scale = _ba_loss(loss, f_scale)
    d = _ba_global_inputs(cam, K, X, obs_cam, obs_pt, pts2d)
    C, N, M = d["C"], d["N"], d["M"]
    dv = d["cam"].device
    for name, shape in (("r", (M, 2)), ("Jc", (M, 2, 6)), ("Jp", (M, 2, 3)), ("U", (C, 6, 6)), ("g_c", (C, 6)),
                        ("V", (N, 3, 3)), ("g_p", (N, 3)), ("weight", (M,))):
        d[name] = torch.empty(shape, dtype=torch.float64, device=dv)
    cost = ctypes.c_double(0.0)
    call("sfmhip_ba_global_linearize_robust", ptr(d["cam"]), ptr(d["K"]), ptr(d["X"]), ptr(d["obs_cam"]),
         ptr(d["obs_pt"]), ptr(d["pts2d"]), ptr(d["pt_off"]), ptr(d["cam_perm"]), ptr(d["cam_off"]), C, N, M, ptr(d["r"]),
         ptr(d["Jc"]), ptr(d["Jp"]), ptr(d["U"]), ptr(d["g_c"]), ptr(d["V"]), ptr(d["g_p"]), ctypes.addressof(cost),
         stream_ptr(), code, f_scale, ptr(d["weight"]))
    d["cost"] = cost.value
    return d


def ba_global_schur_matvec(lin: dict, x, lam: float, cam_fixed=None) -> torch.Tensor:
    """out (C,6) = S(lam) x with S = U* - W V*^-1 W^T of the linearisation ``lin``
    (:func:`ba_global_linearize`), matrix-free; rows of fixed cameras are exactly 0.
    ``lam`` must be positive if a point has fewer than two observations (its V is singular and
    only the damping makes V* invertible); ``lam = 0`` is for problems where every V is regular."""
    require_gpu()
    C, N, M = lin["C"], lin["N"], lin["M"]
    xt = dev(np.asarray(x, np.float64).reshape(C, 6) if not isinstance(x, torch.Tensor) else x, torch.float64)
    if tuple(xt.shape) != (C, 6):
        raise ValueError("x must be (C, 6)")
    fx = None if cam_fixed is None else _fixed_tensor(cam_fixed, C)
    out = torch.empty((C, 6), dtype=torch.float64, device=xt.device)
    call("sfmhip_ba_global_schur_matvec", ptr(lin["Jc"]), ptr(lin["Jp"]), ptr(lin["U"]), ptr(lin["V"]),
         ptr(lin["obs_cam"]), ptr(lin["obs_pt"]), ptr(lin["pt_off"]), ptr(lin["cam_perm"]), ptr(lin["cam_off"]),
         ptr(fx), C, N, M, float(lam), ptr(xt), ptr(out), stream_ptr())
    return out


class _BundleResult(SimpleNamespace):
    """bundle_adjust's result.  ``residual`` and ``weight`` are brought from the device and put into
    the caller's order when first read, so a solve whose caller does not read them pays nothing."""

    def _e2(self):
        if not isinstance(self._res2, np.ndarray):
            e2 = np.empty(len(self._order))
            e2[self._order] = self._res2.cpu().numpy()      # sorted order -> the caller's
            self._res2 = e2
        return self._res2

    @property
    def residual(self):
        return np.sqrt(self._e2())

    @property
    def weight(self):
        return ba_loss_weight(self._e2(), self.loss, self.f_scale)


# K3''' with intrinsics (ba_calib.hip): theta = (f, cx, cy, k1, k2) per intrinsics group
_CALIB_PARTS = {"f": (0,), "pp": (1, 2), "k1": (3,), "k2": (4,)}


def _calib_mask(refine_intrinsics) -> np.ndarray:
    if isinstance(refine_intrinsics, str):
        refine_intrinsics = (refine_intrinsics,)
    mask = np.zeros(5, np.uint8)
    for name in refine_intrinsics:
        if name not in _CALIB_PARTS:
            raise ValueError(f"refine_intrinsics must be a subset of {sorted(_CALIB_PARTS)}, got {name!r}")
        mask[list(_CALIB_PARTS[name])] = 1
    return mask


def _calib_dist(dist) -> np.ndarray:
    """(2,) / (G,2) = k1, k2, or a cv2 vector (k1, k2, p1, p2[, k3]) with p1 = p2 = k3 = 0 -> (1,2) / (G,2)."""
    d = np.zeros((1, 2)) if dist is None else np.asarray(dist, np.float64)
    if d.ndim == 2 and d.shape[1] == 2:
        return np.ascontiguousarray(d)
    d = d.ravel()
    if d.size in (4, 5):
        if np.any(d[2:] != 0):
            raise NotImplementedError("only radial distortion (k1, k2) is modelled: p1, p2 and k3 must be 0")
        d = d[:2]
    if d.size != 2:
        raise ValueError("dist must be (2,), (G, 2) or a cv2 distortion vector of 4 or 5 entries")
    return np.ascontiguousarray(d.reshape(1, 2))


def _calib_inputs(d: dict, dist, refine_intrinsics, cam_group) -> dict:
    """Adds theta (G,5), asp (G,), cam_group (C,), mask (5,) device tensors and G to the inputs."""
    C = d["C"]
    K = d["K"].cpu().numpy()
    mask = _calib_mask(refine_intrinsics)
    dist = _calib_dist(dist)
    grp = np.zeros(C, np.int64) if cam_group is None else np.asarray(cam_group).astype(np.int64).ravel()
    if grp.shape != (C,):
        raise ValueError("cam_group must have one entry per camera")
    if C and grp.min() < 0:
        raise ValueError("cam_group entries must not be negative")
    G = max(int(grp.max()) + 1 if C else 1, len(dist) if len(dist) > 1 else 1)
    if len(dist) == 1:
        dist = np.repeat(dist, G, 0)
    if len(dist) != G:
        raise ValueError(f"dist has {len(dist)} rows for {G} intrinsics groups")
    if C and (np.any(K[:, 0, 1] != 0) or np.any(K[:, 1, 0] != 0)):
        raise ValueError("the camera matrices must have zero skew")
    theta = np.zeros((G, 5))
    theta[:, 0] = 1.0                                    # a group without cameras: never read
    asp = np.ones(G)
    for g in np.unique(grp):
        Kg = K[grp == g]
        if np.any(Kg != Kg[0]):
            raise ValueError(f"the cameras of intrinsics group {g} must share one camera matrix")
        theta[g, :3] = Kg[0, 0, 0], Kg[0, 0, 2], Kg[0, 1, 2]
        asp[g] = Kg[0, 1, 1] / Kg[0, 0, 0]
    theta[:, 3:] = dist
    d.update(G=G, theta=dev(theta, torch.float64), asp=dev(asp, torch.float64),
             cam_group=dev(grp.astype(np.int32), torch.int32), mask=dev(mask, torch.uint8))
    return d


def _calib_K(theta: np.ndarray, asp: np.ndarray, grp: np.ndarray) -> np.ndarray:
    K = np.zeros((len(grp), 3, 3))
    K[:, 0, 0] = theta[grp, 0]
    K[:, 1, 1] = theta[grp, 0] * asp[grp]
    K[:, 0, 2] = theta[grp, 1]
    K[:, 1, 2] = theta[grp, 2]
    K[:, 2, 2] = 1.0
    return K


def ba_calib_linearize(cam, K, X, obs_cam, obs_pt, pts2d, dist=None, refine_intrinsics=(), cam_group=None,
                       loss: str = "linear", f_scale: float = 1.0) -> dict:
    """Linearise the global problem with intrinsics (``sfmhip_ba_calib_linearize``), the arguments
    of :func:`bundle_adjust`.  As :func:`ba_global_linearize`, plus Jk (M,2,5) = d r / d theta
    (columns of components that are not refined are 0), B (C,6,5), H (G,5,5), g_k (G,5) and the
    tensors ``theta`` (G,5), ``asp`` (G,), ``cam_group`` (C,), ``mask`` (5,) the matvec needs."""
    require_gpu()
    code, f_scale = _ba_loss(loss, f_scale)
    d = _calib_inputs(_ba_global_inputs(cam, K, X, obs_cam, obs_pt, pts2d), dist, refine_intrinsics, cam_group)
    C, N, M, G = d["C"], d["N"], d["M"], d["G"]
    dv = d["cam"].device
    for name, shape in (("r", (M, 2)), ("Jc", (M, 2, 6)), ("Jk", (M, 2, 5)), ("Jp", (M, 2, 3)), ("U", (C, 6, 6)),
                        ("g_c", (C, 6)), ("B", (C, 6, 5)), ("H", (G, 5, 5)), ("g_k", (G, 5)), ("V", (N, 3, 3)),
                        ("g_p", (N, 3)), ("weight", (M,))):
        d[name] = torch.empty(shape, dtype=torch.float64, device=dv)
    cost = ctypes.c_double(0.0)
    call("sfmhip_ba_calib_linearize", ptr(d["cam"]), ptr(d["theta"]), ptr(d["asp"]), ptr(d["cam_group"]),
         ptr(d["mask"]), ptr(d["X"]), ptr(d["obs_cam"]), ptr(d["obs_pt"]), ptr(d["pts2d"]), ptr(d["pt_off"]),
         ptr(d["cam_perm"]), ptr(d["cam_off"]), C, N, G, M, ptr(d["r"]), ptr(d["Jc"]), ptr(d["Jk"]), ptr(d["Jp"]),
         ptr(d["U"]), ptr(d["g_c"]), ptr(d["B"]), ptr(d["H"]), ptr(d["g_k"]), ptr(d["V"]), ptr(d["g_p"]),
         ctypes.addressof(cost), stream_ptr(), code, f_scale, ptr(d["weight"]))
    d["cost"] = cost.value
    return d


def ba_calib_matvec(lin: dict, x, lam: float, cam_fixed=None) -> torch.Tensor:
    """out (6C + 5G,) = S~(lam) x~ of the linearisation ``lin`` (:func:`ba_calib_linearize`),
    matrix-free; x~ = (x_c (C,6) flattened, x_k (G,5) flattened).  Rows of fixed cameras and of
    components that are not refined are exactly 0.  ``lam`` as in :func:`ba_global_schur_matvec`."""
    require_gpu()
    C, N, M, G = lin["C"], lin["N"], lin["M"], lin["G"]
    n = 6 * C + 5 * G
    xt = dev(np.asarray(x, np.float64).reshape(n) if not isinstance(x, torch.Tensor) else x, torch.float64)
    if tuple(xt.shape) != (n,):
        raise ValueError("x must be (6 C + 5 G,)")
    fx = None if cam_fixed is None else _fixed_tensor(cam_fixed, C)
    out = torch.empty((n,), dtype=torch.float64, device=xt.device)
    call("sfmhip_ba_calib_matvec", ptr(lin["Jc"]), ptr(lin["Jk"]), ptr(lin["Jp"]), ptr(lin["U"]), ptr(lin["B"]),
         ptr(lin["H"]), ptr(lin["V"]), ptr(lin["cam_group"]), ptr(lin["mask"]), ptr(lin["obs_cam"]),
         ptr(lin["obs_pt"]), ptr(lin["pt_off"]), ptr(lin["cam_perm"]), ptr(lin["cam_off"]), ptr(fx), C, N, G, M,
         float(lam), ptr(xt), ptr(out), stream_ptr())
    return out


def undistort_points(src, K, dist) -> np.ndarray:
    """Pixels (n,2) seen through the radial model (K, dist = k1, k2) -> the pixels (n,2) the same
    K gives without distortion (``sfmhip_undistort_points``: 20 fixed-point steps per point), so
    keypoints can go back through the pinhole stages."""
    require_gpu()
    K = np.asarray(K, np.float64).reshape(3, 3)
    if K[0, 1] != 0:
        raise ValueError("the camera matrix must have zero skew")
    k1, k2 = _calib_dist(dist)[0]
    s = dev(np.ascontiguousarray(np.asarray(src, np.float64).reshape(-1, 2)), torch.float64)
    out = torch.empty_like(s)
    call("sfmhip_undistort_points", ptr(s), int(s.shape[0]), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
         float(K[1, 2]), float(k1), float(k2), ptr(out), stream_ptr())
    return out.cpu().numpy()


def undistortPoints(src, cameraMatrix, distCoeffs):
    """``cv2.undistortPoints(src, cameraMatrix, distCoeffs, P=cameraMatrix)`` for the radial
    model (p1 = p2 = k3 = 0): (n,1,2) pixel coordinates under the same camera matrix."""
    return undistort_points(src, cameraMatrix, distCoeffs).reshape(-1, 1, 2)


def bundle_adjust(cam, K, X, obs_cam, obs_pt, pts2d, cam_fixed=None, gtol: float = 1e-8, ftol: float = 1e-10,
                  eta: float = 1e-2, max_iter: int = 50, max_cg: int = 64, loss: str = "linear", f_scale: float = 1.0,
                  dist=None, refine_intrinsics=(), cam_group=None):
    """Global bundle adjustment of all cameras and points (``sfmhip_ba_global_robust``).

    cam (C,6) = rvec, t (world -> camera); K (3,3) or (C,3,3), held fixed; X (N,3);
    observation m says camera obs_cam[m] saw point obs_pt[m] at pts2d[m], in any
    order.  ``cam_fixed`` (C,) marks cameras that do not move; the default fixes
    camera 0 (fix a second camera to pin the scale as well).  Schur-complement
    Levenberg-Marquardt, the reduced system solved by preconditioned CG to
    ``eta`` in at most ``max_cg`` iterations per trial step.

    Returns an object with ``cam``, ``X`` (numpy, the inputs are not modified),
    ``cost0``, ``cost``, ``status`` (1 gtol, 2 ftol, 0 max_iter, 3 damping overflow,
    -1 malformed observation list, -2 a point behind a camera at the start; for
    the negative ones cam and X are the inputs), ``nit`` (linearisations),
    ``n_accept`` and ``n_cg``; ``residual`` (M,), the final unweighted |r| of every
    observation in pixels, in the caller's order (NaN for a negative status), and
    ``weight`` (M,), the loss's weight at that residual.

    ``loss``: "linear" (plain least squares), "huber", "soft_l1" or "cauchy", with the
    scale ``f_scale`` > 0 in pixels.  The loss is applied per observation, to the
    2-vector of its residual, as Ceres does — not per scalar component as scipy's
    ``least_squares`` does: z = |r|^2 / f_scale^2, cost = 0.5 f_scale^2 sum rho(z) with
    scipy's rho, weights w = rho'(z) (plain IRLS, no second-order correction).
    ``cost0`` and ``cost`` are that robust cost.  Cauchy with f_scale of 1-2 px
    converges on gross outliers; Huber under IRLS creeps.

    Intrinsics (``sfmhip_ba_calib``, DESIGN.md "K3''' with intrinsics"): ``dist`` = (k1, k2), one
    row per intrinsics group or one for all (a cv2 distortion vector is accepted when p1, p2 and
    k3 are 0), puts OpenCV's radial model between the normalised point and the pixel;
    ``refine_intrinsics``, a subset of {"f", "pp", "k1", "k2"}, frees the focal length (the
    aspect fy / fx of the input K stays), the principal point and the two coefficients;
    ``cam_group`` (C,) maps every camera to its intrinsics group (default: one shared camera; the
    K of a group's cameras must be equal and have zero skew).  With ``dist`` None and nothing to
    refine the call is the pinhole solve above, unchanged.  Otherwise the result also carries
    ``K`` (C,3,3), ``dist`` (G,2) and ``theta`` (G,5) = f, cx, cy, k1, k2, and ``residual`` /
    ``weight`` are those of the distorted model."""
    require_gpu()
    code, f_scale = _ba_loss(loss, f_scale)
    calib = dist is not None or bool(_calib_mask(refine_intrinsics).any())
    d = _ba_global_inputs(cam, K, X, obs_cam, obs_pt, pts2d)
    C, N, M = d["C"], d["N"], d["M"]
    if cam_fixed is None:
        cam_fixed = np.zeros(C, np.uint8)
        cam_fixed[:1] = 1
    fx = _fixed_tensor(cam_fixed, C)
    camt, Xt = d["cam"].clone(), d["X"].clone()
    cost = (ctypes.c_double * 2)()
    info = (ctypes.c_int32 * 4)()
    res2 = torch.full((M,), float("nan"), dtype=torch.float64, device=camt.device)
    if calib:
        d = _calib_inputs(d, dist, refine_intrinsics, cam_group)
        tht = d["theta"].clone()
        call("sfmhip_ba_calib", ptr(camt), ptr(tht), ptr(d["asp"]), ptr(d["cam_group"]), ptr(d["mask"]), ptr(Xt),
             ptr(d["obs_cam"]), ptr(d["obs_pt"]), ptr(d["pts2d"]), ptr(d["pt_off"]), ptr(d["cam_perm"]),
             ptr(d["cam_off"]), ptr(fx), C, N, d["G"], M, float(gtol), float(ftol), float(eta), int(max_iter),
             int(max_cg), ctypes.addressof(cost), ctypes.addressof(info), stream_ptr(), code, f_scale, ptr(res2))
        theta = tht.cpu().numpy()
        return _BundleResult(cam=camt.cpu().numpy(), X=Xt.cpu().numpy(), cost0=cost[0], cost=cost[1],
                             status=int(info[0]), nit=int(info[1]), n_accept=int(info[2]), n_cg=int(info[3]),
                             loss=loss, f_scale=f_scale, _res2=res2, _order=d["order"], theta=theta,
                             dist=theta[:, 3:].copy(),
                             K=_calib_K(theta, d["asp"].cpu().numpy(), d["cam_group"].cpu().numpy()))
    call("sfmhip_ba_global_robust", ptr(camt), ptr(d["K"]), ptr(Xt), ptr(d["obs_cam"]), ptr(d["obs_pt"]),
         ptr(d["pts2d"]), ptr(d["pt_off"]), ptr(d["cam_perm"]), ptr(d["cam_off"]), ptr(fx), C, N, M, float(gtol),
         float(ftol), float(eta), int(max_iter), int(max_cg), ctypes.addressof(cost), ctypes.addressof(info),
         stream_ptr(), code, f_scale, ptr(res2))
    return _BundleResult(cam=camt.cpu().numpy(), X=Xt.cpu().numpy(), cost0=cost[0], cost=cost[1],
                         status=int(info[0]), nit=int(info[1]), n_accept=int(info[2]), n_cg=int(info[3]),
                         loss=loss, f_scale=f_scale, _res2=res2, _order=d["order"])


# ---------------------------------------------------------------------------
# S2b: robust N-view triangulation of tracks (triangulate.hip; build-defined)
TRI_STATUS = {0: "ok", 1: "fewer than two distinct cameras", 2: "no hypothesis survived",
              3: "final angle too small", 4: "fit failed"}


def triangulate_tracks(poses, K, obs_cam, obs_pt, pts2d, n_tracks=None, dist=None, reproj_px: float = 4.0,
                       min_angle: float = 1.5, max_hyp: int = 256, refine_iters: int = 3, cam_group=None):
    """Every track's 3D point from all of its observations, some of which may be wrong matches
    (``sfmhip_triangulate_tracks``, include/sfmhip.h S2b: two-view hypotheses scored against the
    whole track, a Gauss-Newton fit to the winner's inliers, one re-classification and a refit).

    ``poses`` (C,3,4) world -> camera, or a list with ``None`` for an unregistered camera, whose
    observations are dropped; ``K`` (3,3) or (C,3,3) with zero skew; observation m says camera
    obs_cam[m] saw track obs_pt[m] at pts2d[m], in any order (the sort is
    :func:`ba_global_structure`'s; a repeated (track, camera) pair is legal).  ``n_tracks``
    defaults to the largest track index + 1.  ``dist`` = (k1, k2), or one row per intrinsics
    group as :func:`bundle_adjust` reports it with ``cam_group`` (C,) as there (one row per
    camera without it): the observations first pass through :func:`undistort_points`, and
    residuals are then in undistorted pixels.  An observation is an inlier within ``reproj_px``
    pixels; ``min_angle`` (degrees) is the smallest triangulation angle, ``max_hyp`` the most
    hypotheses per track, ``refine_iters`` the Gauss-Newton steps per fit.

    Returns an object with ``X`` (N,3; NaN unless OK), ``status`` (N,; TRI_STATUS), ``ok`` (N,) bool,
    ``n_inliers`` (N,), and ``inlier`` (M,) bool and ``residual`` (M,; pixels under X, NaN where the
    track is not OK or the observation was dropped) in the caller's order, and ``n_hyp``, the
    hypotheses scored.  Index and shape errors raise ValueError before any launch."""
    poses = list(poses)
    C = len(poses)
    registered = np.array([p is not None for p in poses], bool)
    P = np.zeros((C, 3, 4))
    for c in np.nonzero(registered)[0]:
        Pc = np.asarray(poses[c], np.float64)
        if Pc.shape != (3, 4):
            raise ValueError(f"pose {c} must be (3, 4), got {Pc.shape}")
        P[c] = Pc
    K = np.asarray(K, np.float64)
    if K.shape == (3, 3):
        K = np.broadcast_to(K, (C, 3, 3))
    if K.shape != (C, 3, 3):
        raise ValueError("K must be (3, 3) or (C, 3, 3)")
    if C and np.any(K[:, 0, 1] != 0):
        raise ValueError("the camera matrices must have zero skew")
    obs_cam = np.asarray(obs_cam).ravel()
    obs_pt = np.asarray(obs_pt).ravel()
    pts2d = np.asarray(pts2d, np.float64)
    M = len(obs_cam)
    if len(obs_pt) != M or pts2d.size != 2 * M:
        raise ValueError("obs_cam, obs_pt and pts2d must have one row per observation")
    pts2d = pts2d.reshape(M, 2)
    if M and not (np.issubdtype(obs_cam.dtype, np.integer) and np.issubdtype(obs_pt.dtype, np.integer)):
        raise ValueError("obs_cam and obs_pt must be integers")
    obs_cam, obs_pt = obs_cam.astype(np.int64), obs_pt.astype(np.int64)
    if n_tracks is None:
        n_tracks = int(obs_pt.max()) + 1 if M else 0
    N = int(n_tracks)
    if N < 0 or N > 2 ** 31 - 1:
        raise ValueError("n_tracks must be in [0, 2^31)")
    if M and (obs_cam.min() < 0 or obs_cam.max() >= C):
        raise ValueError("obs_cam entries must lie in [0, C)")
    if M and (obs_pt.min() < 0 or obs_pt.max() >= N):
        raise ValueError("obs_pt entries must lie in [0, n_tracks)")
    if not (np.isfinite(reproj_px) and reproj_px > 0):
        raise ValueError("reproj_px must be finite and positive")
    if not (np.isfinite(min_angle) and 0 <= min_angle < 90):
        raise ValueError("min_angle must be in [0, 90) degrees")
    if int(max_hyp) < 1 or int(max_hyp) > 1 << 20:
        raise ValueError("max_hyp must be in [1, 2^20]")
    if int(refine_iters) < 0:
        raise ValueError("refine_iters must not be negative")
    grp = None
    if dist is not None:
        dist = _calib_dist(dist)
        grp = np.zeros(C, np.int64) if len(dist) == 1 else (np.arange(C) if cam_group is None
                                                            else np.asarray(cam_group).astype(np.int64).ravel())
        if grp.shape != (C,) or (C and (grp.min() < 0 or grp.max() >= len(dist))):
            raise ValueError(f"dist has {len(dist)} rows; cam_group must map every camera to one of them")
    d = require_gpu()
    use = np.nonzero(registered[obs_cam])[0] if M else np.zeros(0, np.int64)
    oc, ot, uv = obs_cam[use], obs_pt[use], np.ascontiguousarray(pts2d[use])
    if dist is not None and len(oc):
        for c in np.unique(oc):
            sel = oc == c
            uv[sel] = undistort_points(uv[sel], K[c], dist[grp[c]])
    order, pt_off, _, _ = ba_global_structure(oc, ot, C, N)
    Mu = len(oc)
    cos_min = math.cos(math.radians(float(min_angle)))           # on the host: the device uses no transcendentals
    cam4 = np.ascontiguousarray(np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1)) if C else np.zeros((0, 4))
    track_order = np.argsort(-np.diff(pt_off), kind="stable").astype(np.int32)   # long tracks first: like trip counts
    Xt = torch.empty((N, 3), dtype=torch.float64, device=d)
    st = torch.empty((N,), dtype=torch.int32, device=d)
    ni = torch.empty((N,), dtype=torch.int32, device=d)
    inl = torch.empty((Mu,), dtype=torch.uint8, device=d)
    res = torch.empty((Mu,), dtype=torch.float64, device=d)
    n_hyp = ctypes.c_int64(0)
    # the inputs stay referenced until the call returns
    Pt, camt = (dev(P, torch.float64), dev(cam4, torch.float64)) if C else (None, None)
    offt = dev(pt_off, torch.int64)
    oct_, uvt = (dev(oc[order].astype(np.int32), torch.int32),
                 dev(np.ascontiguousarray(uv[order]), torch.float64)) if Mu else (None, None)
    ordt = dev(track_order, torch.int32) if N else None
    call("sfmhip_triangulate_tracks", ptr(Pt), ptr(camt), C, ptr(offt), N, ptr(oct_), ptr(uvt), Mu, ptr(ordt),
         float(reproj_px), cos_min, int(max_hyp), int(refine_iters), ptr(Xt) if N else None, ptr(st) if N else None,
         ptr(ni) if N else None, ptr(inl) if Mu else None, ptr(res) if Mu else None, ctypes.addressof(n_hyp), None,
         stream_ptr())
    inlier = np.zeros(M, bool)
    residual = np.full(M, np.nan)
    inlier[use[order]] = inl.cpu().numpy().astype(bool)
    residual[use[order]] = res.cpu().numpy()
    status = st.cpu().numpy()
    return SimpleNamespace(X=Xt.cpu().numpy(), status=status, ok=status == 0, n_inliers=ni.cpu().numpy(),
                           inlier=inlier, residual=residual, n_hyp=int(n_hyp.value))
