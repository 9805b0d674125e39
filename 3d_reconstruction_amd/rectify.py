"""V12: images and depth maps of a radially distorted camera resampled to a pinhole camera, so
that the calibration :func:`~.geometry.bundle_adjust` estimates reaches the dense path
(build-defined; the semantics are the V12 block of include/sfmhip.h).

* :func:`undistort_images` — u8 images, bilinear with an integer blend, and a validity mask.
* :func:`undistort_depth` — f32 depth maps, nearest source pixel, bits copied.
* :func:`undistort_map` — the map itself, in 1/256 source pixels.
* :func:`optimal_new_K` — the pinhole camera that keeps only valid pixels (alpha 0) or the whole
  source frame (alpha 1).
"""
from __future__ import annotations

import numpy as np
import torch

from ._abi import call, dev, ptr, require_gpu, stream_ptr
from .geometry import _calib_dist, undistort_points

_MAX_SIDE = 32768


def _host(x) -> np.ndarray:
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float64)


def _K4(K, name: str) -> np.ndarray:
    """(3,3), (n,3,3), (4,) or (n,4) -> (n,4) f64 = fx, fy, cx, cy; zero skew required."""
    K = _host(K)
    if K.ndim in (2, 3) and K.shape[-2:] == (3, 3):
        K = K.reshape(-1, 3, 3)
        if np.any(K[:, 0, 1] != 0) or np.any(K[:, 1, 0] != 0):
            raise ValueError(f"{name}: the camera matrices must have zero skew")
        return np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1)
    if K.shape == (4,) or (K.ndim == 2 and K.shape[1] == 4):
        return K.reshape(-1, 4)
    raise ValueError(f"{name} must be (3,3), (V,3,3), (4,) or (V,4), got {K.shape}")


def _spread(rows: np.ndarray, V: int, name: str) -> np.ndarray:
    """One row serves every view; otherwise one row per view."""
    if len(rows) == 1:
        rows = np.repeat(rows, V, 0)
    if len(rows) != V:
        raise ValueError(f"{name} holds {len(rows)} cameras for {V} views")
    return rows


def _cameras(K, dist, new_K, V=None):
    """cam_src (V,6) and cam_dst (V,4) f64 on the host, checked; V None: the most rows given."""
    Ks, d = _K4(K, "K"), _calib_dist(_host(dist))
    Kd = Ks if new_K is None else _K4(new_K, "new_K")
    if V is None:
        V = max(len(Ks), len(d), len(Kd))
    Ks, d, Kd = _spread(Ks, V, "K"), _spread(d, V, "dist"), _spread(Kd, V, "new_K")
    return np.ascontiguousarray(np.concatenate([Ks, d], 1)), np.ascontiguousarray(Kd)


def _size(size, default):
    """(W', H') -> (Ho, Wo), checked."""
    if size is None:
        return default
    Wo, Ho = (int(s) for s in size)
    if not (0 <= Wo <= _MAX_SIDE and 0 <= Ho <= _MAX_SIDE):
        raise ValueError(f"size must be (W, H) with both in [0, {_MAX_SIDE}], got {tuple(size)}")
    return Ho, Wo


def _tensor(x, dtype: torch.dtype, name: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    if x.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {x.dtype}")
    return x


def undistort_images(images, K, dist, new_K=None, size=None):
    """V images seen through the radial model (K, dist) resampled to the pinhole camera
    ``new_K`` (``sfmhip_undistort_u8``): bilinear between the four source pixels around the
    mapped point, in integers with weights of 1/256.

    images (V,H,W) or (V,H,W,3|4) u8, numpy or torch; K (3,3), (V,3,3), (4,) or (V,4) = fx, fy,
    cx, cy with zero skew; dist (2,) or (V,2) = k1, k2, or a cv2 vector with p1 = p2 = k3 = 0;
    ``new_K`` like K (default: K); ``size=(W', H')`` of the output (default: the input's).

    Returns ``out`` (V,H',W'[,C]) u8 and ``mask`` (V,H',W') u8 on the device: 1 where the pixel
    maps into the source frame, else 0 with ``out`` 0 (also for a whole view whose cameras hold a
    non-finite number, one of magnitude >= 2^60 or a focal length of 0)."""
    gpu = require_gpu()
    images = _tensor(images, torch.uint8, "images")
    if images.dim() not in (3, 4) or (images.dim() == 4 and images.shape[3] not in (3, 4)):
        raise ValueError(f"images must be (V,H,W) or (V,H,W,3|4), got {tuple(images.shape)}")
    V, H, W = (int(s) for s in images.shape[:3])
    C = 1 if images.dim() == 3 else int(images.shape[3])
    if H > _MAX_SIDE or W > _MAX_SIDE:
        raise ValueError(f"an image has at most {_MAX_SIDE} pixels per side, got {H} x {W}")
    cs, cd = _cameras(K, dist, new_K, V)
    Ho, Wo = _size(size, (H, W))
    img = dev(images, torch.uint8)
    shape = (V, Ho, Wo) if images.dim() == 3 else (V, Ho, Wo, C)
    if V == 0 or H == 0 or W == 0 or Ho == 0 or Wo == 0:    # nothing to read or nothing to write
        return (torch.zeros(shape, dtype=torch.uint8, device=gpu),
                torch.zeros((V, Ho, Wo), dtype=torch.uint8, device=gpu))
    out = torch.empty(shape, dtype=torch.uint8, device=gpu)
    mask = torch.empty((V, Ho, Wo), dtype=torch.uint8, device=gpu)
    cs, cd = dev(cs, torch.float64), dev(cd, torch.float64)
    call("sfmhip_undistort_u8", ptr(img), V, H, W, C, ptr(cs), ptr(cd), Ho, Wo, ptr(out), ptr(mask), stream_ptr())
    return out, mask


def undistort_depth(depth, K, dist, new_K=None, size=None) -> torch.Tensor:
    """V depth maps (V,H,W) f32 (0 = invalid) of the distorted camera resampled to the pinhole
    camera ``new_K`` (``sfmhip_undistort_f32``): every output pixel copies the 32 bits of the
    source pixel nearest to its mapped point (depth along z is unchanged by a radial model, and
    nothing is blended across an edge); 0 where the point falls outside the source frame.
    Arguments as for :func:`undistort_images`.  Returns (V,H',W') f32 on the device."""
    gpu = require_gpu()
    depth = _tensor(depth, torch.float32, "depth")
    if depth.dim() != 3:
        raise ValueError(f"depth must be (V,H,W), got {tuple(depth.shape)}")
    V, H, W = (int(s) for s in depth.shape)
    if H > _MAX_SIDE or W > _MAX_SIDE:
        raise ValueError(f"a map has at most {_MAX_SIDE} pixels per side, got {H} x {W}")
    cs, cd = _cameras(K, dist, new_K, V)
    Ho, Wo = _size(size, (H, W))
    dp = dev(depth, torch.float32)
    if V == 0 or H == 0 or W == 0 or Ho == 0 or Wo == 0:
        return torch.zeros((V, Ho, Wo), dtype=torch.float32, device=gpu)
    out = torch.empty((V, Ho, Wo), dtype=torch.float32, device=gpu)
    cs, cd = dev(cs, torch.float64), dev(cd, torch.float64)
    call("sfmhip_undistort_f32", ptr(dp), V, H, W, ptr(cs), ptr(cd), Ho, Wo, ptr(out), stream_ptr())
    return out


def undistort_map(K, dist, size, new_K=None, new_size=None) -> torch.Tensor:
    """The map of :func:`undistort_images` for source frames of ``size=(W, H)``
    (``sfmhip_undistort_map``): (V,H',W',2) int32 on the device, the source point X, Y of every
    output pixel in units of 1/256 px, (-1, -1) where it is invalid.  V is the number of cameras
    in K, dist and ``new_K`` (those given once are shared)."""
    gpu = require_gpu()
    H, W = _size(size, None)
    cs, cd = _cameras(K, dist, new_K)
    V = len(cs)
    Ho, Wo = _size(new_size, (H, W))
    out = torch.empty((V, Ho, Wo, 2), dtype=torch.int32, device=gpu)
    if V and Ho and Wo:
        cs, cd = dev(cs, torch.float64), dev(cd, torch.float64)
        call("sfmhip_undistort_map", ptr(cs), ptr(cd), V, H, W, Ho, Wo, ptr(out), stream_ptr())
    return out


def optimal_new_K(K, dist, size, alpha: float = 0.0, new_size=None) -> np.ndarray:
    """The pinhole camera (gx, gy, ox, oy) (4,) f64 for :func:`undistort_images` of one camera
    K, dist with frames of ``size=(W, H)``, the package's ``getOptimalNewCameraMatrix``.

    Every pixel of the four edges of the source frame goes through :func:`undistort_points`; in
    normalised coordinates (p - c) / f the inner rectangle is [max over the left edge of x, min
    over the right edge] x [max over the top of y, min over the bottom], the outer rectangle the
    same with min and max swapped; ``alpha`` interpolates linearly from the inner (0: every
    output pixel is valid) to the outer (1: the whole source frame is kept), and the camera
    maps the rectangle onto [0, W'-1] x [0, H'-1] of ``new_size=(W', H')`` (default: ``size``)."""
    Ks, d = _K4(K, "K"), _calib_dist(_host(dist))
    fx, fy, cx, cy = Ks[0]
    if len(Ks) != 1 or len(d) != 1:
        raise ValueError("optimal_new_K takes one camera")
    W, H = (int(s) for s in size)
    Wn, Hn = (W, H) if new_size is None else (int(s) for s in new_size)
    if min(W, H, Wn, Hn) < 2:
        raise ValueError("optimal_new_K needs frames of at least 2 x 2 pixels")
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], got {alpha}")
    us, vs = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    edges = np.concatenate([np.stack([np.zeros(H), vs], 1), np.stack([np.full(H, W - 1.0), vs], 1),
                            np.stack([us, np.zeros(W)], 1), np.stack([us, np.full(W, H - 1.0)], 1)])
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    q = undistort_points(edges, Km, d[0])
    xl, xr = (q[:H, 0] - cx) / fx, (q[H:2 * H, 0] - cx) / fx
    yt, yb = (q[2 * H:2 * H + W, 1] - cy) / fy, (q[2 * H + W:, 1] - cy) / fy
    x_lo = xl.max() + alpha * (xl.min() - xl.max())
    x_hi = xr.min() + alpha * (xr.max() - xr.min())
    y_lo = yt.max() + alpha * (yt.min() - yt.max())
    y_hi = yb.min() + alpha * (yb.max() - yb.min())
    if not (x_hi > x_lo and y_hi > y_lo):
        raise ValueError("the undistorted frame is empty: the model folds over inside the source frame")
    gx = np.float64(Wn - 1) / (x_hi - x_lo)
    gy = np.float64(Hn - 1) / (y_hi - y_lo)
    return np.array([gx, gy, -x_lo * gx, -y_lo * gy], np.float64)
