"""V10: dense depth from posed images by census plane-sweep stereo (build-defined; the
semantics are the V10 block of include/sfmhip.h).

* :func:`census_transform` — the 7 x 7 census signature of every pixel.
* :func:`plane_sweep` — the Hamming cost of a reference view against its sources over a set of
  fronto-parallel planes, box aggregation, winner-take-all with a sub-plane depth.
* :func:`depth_consistency` — keeps a depth where enough source depth maps agree with it.
* :func:`cost_volume`, :func:`sgm_aggregate`, :func:`volume_select` — the sweep in three steps with
  semi-global path aggregation of the cost volume between them (``smooth=`` of the two calls below).
* :func:`mvs_depth` — the three together: images and poses in, depth maps for
  :func:`~.voxel.tsdf_integrate` out.
"""
from __future__ import annotations

import numpy as np
import torch

from ._abi import call, dev, ptr, require_gpu, stream_ptr
from .rectify import undistort_images


def inverse_depth_planes(near: float, far: float, P: int) -> np.ndarray:
    """P plane depths from ``near`` to ``far``, uniform in inverse depth: in f64,
    ``1/((1 - j)/near + j/far)`` with ``j = k/(P - 1)``, rounded to f32."""
    near, far, P = float(near), float(far), int(P)
    if P < 1:
        raise ValueError(f"P must be at least 1, got {P}")
    if not (near > 0.0 and far > 0.0 and np.isfinite(near) and np.isfinite(far)):
        raise ValueError(f"near and far must be finite and > 0, got {near} / {far}")
    if P == 1:
        return np.array([near], np.float32)
    j = np.arange(P, dtype=np.float64) / (P - 1)
    return (1.0 / ((1.0 - j) / near + j / far)).astype(np.float32)


def _grey(images) -> torch.Tensor:
    """(V,H,W) u8, or (V,H,W,3|4) u8 reduced by (77 r + 150 g + 29 b + 128) >> 8 (torch, not
    the hot path) -> contiguous (V,H,W) u8 on the device."""
    if not isinstance(images, torch.Tensor):
        images = torch.as_tensor(np.asarray(images))
    if images.dtype != torch.uint8:
        raise ValueError(f"images must be uint8, got {images.dtype}")
    img = dev(images, torch.uint8)
    if img.dim() == 4 and img.shape[3] in (3, 4):
        c = img.to(torch.int32)
        img = ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).to(torch.uint8).contiguous()
    if img.dim() != 3:
        raise ValueError(f"images must be (V,H,W) or (V,H,W,3|4), got {tuple(images.shape)}")
    return img


def _cameras(poses, K, V: int):
    ps = dev(poses, torch.float32)
    kk = dev(K, torch.float32)
    if tuple(ps.shape) != (V, 3, 4):
        raise ValueError(f"poses must be ({V},3,4) to match the views, got {tuple(ps.shape)}")
    if tuple(kk.shape) != (V, 4):
        raise ValueError(f"K must be ({V},4) to match the views, got {tuple(kk.shape)}")
    return ps, kk


def _lists(refs, srcs):
    rf = dev(np.asarray(refs, np.int32) if not isinstance(refs, torch.Tensor) else refs, torch.int32).reshape(-1)
    sr = dev(np.asarray(srcs, np.int32) if not isinstance(srcs, torch.Tensor) else srcs, torch.int32)
    R = rf.shape[0]
    if sr.dim() != 2 or sr.shape[0] != R or not 1 <= sr.shape[1] <= 16:
        raise ValueError(f"srcs must be ({R},S) with 1 <= S <= 16 to match refs, got {tuple(sr.shape)}")
    return rf, sr


def census_transform(images) -> torch.Tensor:
    """7 x 7 census transform of V grey images (V,H,W) u8 (RGB(A) images (V,H,W,3|4) are
    reduced to grey first) -> (V,H,W) int64 on the device: bit i, i = 0..47 over the
    neighbourhood in row-major order without the centre, is set iff the neighbour lies inside
    the image and is brighter than the centre; the upper 16 bits are 0."""
    gpu = require_gpu()
    img = _grey(images)
    V, H, W = img.shape
    cen = torch.empty((V, H, W), dtype=torch.int64, device=gpu)
    call("sfmhip_census", ptr(img), V, H, W, ptr(cen), stream_ptr())
    return cen


def plane_sweep(images_or_census, poses, K, refs, srcs, planes, agg_radius: int = 2, penalty: int = 24,
                uniq: int = 243, min_views: int = 2, diagnostics: bool = False, smooth=None):
    """Plane-sweep stereo of R reference views against S sources each (steps 2 - 7 of the V10
    block of include/sfmhip.h).

    images_or_census: the (V,H,W) int64 result of :func:`census_transform`, or uint8 images it
    is computed from; poses (V,3,4) world->camera and K (V,4) [fx, fy, cx, cy] as for
    :func:`~.voxel.tsdf_integrate`; refs (R,) view indices; srcs (R,S) view indices, -1 for
    "none" (S <= 16); planes (P,) depths, finite, positive and strictly monotonic in either
    direction (P <= 65535).  A pixel's cost at a plane is the sum over the sources of the
    Hamming distance of the two census signatures (``penalty``, 0..48, where the pixel does not
    project into the source), summed over the (2 agg_radius + 1)^2 window (agg_radius 0..3).
    The winning plane's depth, refined between its neighbours in inverse depth, is kept when
    the winner is not the first or last plane, at least ``min_views`` sources saw the pixel
    there, and ``256 best <= uniq second`` (``second`` the lowest cost at least two planes
    away; uniq 0..256, 256 disables the test).  Every -1 in a row of srcs adds ``penalty`` to
    all of its costs, which blunts that test: sweep views with different numbers of sources in
    separate calls (as :func:`mvs_depth` does).

    Returns depth (R,H,W) f32 on the device, 0 = invalid; ``diagnostics=True`` appends
    ``k`` (R,H,W) int32 (the winning plane), ``best`` and ``second`` (int32) and ``nv``
    (uint8, the sources that saw the pixel at the winner).  An invalid reference (non-finite
    or >= 2^60 pose or intrinsic entry, fx or fy of 0) gives all-zero maps; an invalid source
    counts as out of view.

    ``smooth=(p1, p2)`` or ``(p1, p2, paths)`` (``paths`` as for :func:`sgm_aggregate`, 8 by
    default) smooths the costs along scan lines before the winner is taken: :func:`cost_volume`,
    :func:`sgm_aggregate` and :func:`volume_select` in turn, with P <= 256 and
    (R,H,W,P) volumes of 2 and 4 bytes per entry in memory.  ``None`` is the single-kernel
    sweep."""
    if smooth is not None:
        p1, p2, mask = _smooth(smooth)
        a = _sweep_inputs(images_or_census, poses, K, refs, srcs, planes, p_max=256)
        agg_radius, penalty, uniq, min_views = _sweep_ints(agg_radius, penalty, uniq, min_views)
        vol = _volume(a, agg_radius, penalty)
        sm = _aggregate(vol, p1, p2, mask)
        del vol
        out = _select(sm, a, uniq, min_views, diagnostics)
        return out if diagnostics else out[0]
    gpu = require_gpu()
    if isinstance(images_or_census, torch.Tensor) and images_or_census.dtype == torch.int64:
        cen = dev(images_or_census, torch.int64)
        if cen.dim() != 3:
            raise ValueError(f"a census must be (V,H,W), got {tuple(cen.shape)}")
    else:
        cen = census_transform(images_or_census)
    V, H, W = cen.shape
    ps, kk = _cameras(poses, K, V)
    rf, sr = _lists(refs, srcs)
    R, S = sr.shape
    pl_host = np.asarray(planes.detach().cpu().numpy() if isinstance(planes, torch.Tensor) else planes,
                         np.float32).reshape(-1)
    P = pl_host.shape[0]
    if not 1 <= P <= 65535:
        raise ValueError(f"planes must hold 1 to 65535 depths, got {P}")
    if not (np.isfinite(pl_host).all() and (pl_host > 0).all()):
        raise ValueError("planes must be finite and > 0")
    step = np.diff(pl_host)
    if not ((step > 0).all() or (step < 0).all()):
        raise ValueError("planes must be strictly monotonic")
    agg_radius, penalty, uniq, min_views = int(agg_radius), int(penalty), int(uniq), int(min_views)
    if not 0 <= agg_radius <= 3:
        raise ValueError(f"agg_radius must be in [0, 3], got {agg_radius}")
    if not 0 <= penalty <= 48:
        raise ValueError(f"penalty must be in [0, 48], got {penalty}")
    if not 0 <= uniq <= 256:
        raise ValueError(f"uniq must be in [0, 256], got {uniq}")
    if min_views < 0:
        raise ValueError(f"min_views must be >= 0, got {min_views}")
    pl = dev(pl_host, torch.float32)
    depth = torch.empty((R, H, W), dtype=torch.float32, device=gpu)
    ks = torch.empty((R, H, W), dtype=torch.int32, device=gpu) if diagnostics else None
    best = torch.empty_like(ks) if diagnostics else None
    second = torch.empty_like(ks) if diagnostics else None
    nv = torch.empty((R, H, W), dtype=torch.uint8, device=gpu) if diagnostics else None
    call("sfmhip_plane_sweep", ptr(cen), ptr(ps), ptr(kk), V, H, W, ptr(rf), ptr(sr), R, S, ptr(pl), P, agg_radius,
         penalty, uniq, min_views, ptr(depth), ptr(ks), ptr(best), ptr(second), ptr(nv), stream_ptr())
    return (depth, ks, best, second, nv) if diagnostics else depth


def _smooth(smooth):
    """(p1, p2) or (p1, p2, paths) -> p1, p2, path mask, checked."""
    if not isinstance(smooth, (tuple, list)) or len(smooth) not in (2, 3):
        raise ValueError(f"smooth must be (p1, p2) or (p1, p2, paths), got {smooth!r}")
    p1, p2 = int(smooth[0]), int(smooth[1])
    if not 0 <= p1 <= p2 <= 16383:
        raise ValueError(f"need 0 <= p1 <= p2 <= 16383, got p1 {p1}, p2 {p2}")
    return p1, p2, _path_mask(smooth[2] if len(smooth) == 3 else 8)


def _path_mask(paths) -> int:
    """8 -> 0xFF (all eight directions), 4 -> 0x0F (along rows and columns), ("mask", m) -> m."""
    if isinstance(paths, (tuple, list)) and len(paths) == 2 and paths[0] == "mask":
        mask = int(paths[1])
        if not 1 <= mask <= 0xFF:
            raise ValueError(f"a path mask must be in [1, 255], got {mask}")
        return mask
    if isinstance(paths, (tuple, list)) or int(paths) not in (4, 8):
        raise ValueError(f'paths must be 8, 4 or ("mask", m), got {paths!r}')
    return 0xFF if int(paths) == 8 else 0x0F


def _sweep_ints(agg_radius, penalty, uniq, min_views):
    agg_radius, penalty, uniq, min_views = int(agg_radius), int(penalty), int(uniq), int(min_views)
    if not 0 <= agg_radius <= 3:
        raise ValueError(f"agg_radius must be in [0, 3], got {agg_radius}")
    if not 0 <= penalty <= 48:
        raise ValueError(f"penalty must be in [0, 48], got {penalty}")
    if not 0 <= uniq <= 256:
        raise ValueError(f"uniq must be in [0, 256], got {uniq}")
    if min_views < 0:
        raise ValueError(f"min_views must be >= 0, got {min_views}")
    return agg_radius, penalty, uniq, min_views


def _planes(planes, p_max: int) -> torch.Tensor:
    pl_host = np.asarray(planes.detach().cpu().numpy() if isinstance(planes, torch.Tensor) else planes,
                         np.float32).reshape(-1)
    P = pl_host.shape[0]
    if not 1 <= P <= p_max:
        raise ValueError(f"planes must hold 1 to {p_max} depths, got {P}")
    if not (np.isfinite(pl_host).all() and (pl_host > 0).all()):
        raise ValueError("planes must be finite and > 0")
    step = np.diff(pl_host)
    if not ((step > 0).all() or (step < 0).all()):
        raise ValueError("planes must be strictly monotonic")
    return dev(pl_host, torch.float32)


def _sweep_inputs(images_or_census, poses, K, refs, srcs, planes, p_max: int, cameras_only=None,
                  already_checked: bool = False) -> dict:
    """The device arguments the three calls share: cen (None for a selection, whose (H, W) is
    ``cameras_only``), poses, K, refs, srcs, planes (``already_checked``: the result of
    :func:`_planes`) and the sizes."""
    if cameras_only is not None:
        cen = None
        H, W = cameras_only
        V = int(poses.shape[0]) if hasattr(poses, "shape") else len(poses)
    else:
        if isinstance(images_or_census, torch.Tensor) and images_or_census.dtype == torch.int64:
            cen = dev(images_or_census, torch.int64)
            if cen.dim() != 3:
                raise ValueError(f"a census must be (V,H,W), got {tuple(cen.shape)}")
        else:
            cen = census_transform(images_or_census)
        V, H, W = cen.shape
    ps, kk = _cameras(poses, K, V)
    rf, sr = _lists(refs, srcs)
    R, S = sr.shape
    pl = planes if already_checked else _planes(planes, p_max)
    return dict(cen=cen, ps=ps, kk=kk, rf=rf, sr=sr, pl=pl, V=V, H=H, W=W, R=R, S=S, P=pl.shape[0])


def _volume(a: dict, agg_radius: int, penalty: int, out=None) -> torch.Tensor:
    vol = torch.empty((a["R"], a["H"], a["W"], a["P"]), dtype=torch.uint16,
                      device=a["ps"].device) if out is None else out
    call("sfmhip_cost_volume", ptr(a["cen"]), ptr(a["ps"]), ptr(a["kk"]), a["V"], a["H"], a["W"], ptr(a["rf"]),
         ptr(a["sr"]), a["R"], a["S"], ptr(a["pl"]), a["P"], agg_radius, penalty, ptr(vol), stream_ptr())
    return vol


def _aggregate(vol: torch.Tensor, p1: int, p2: int, mask: int, out=None) -> torch.Tensor:
    R, H, W, P = vol.shape
    if not 1 <= P <= 256:
        raise ValueError(f"a volume to aggregate holds 1 to 256 planes, got {P}")
    sm = torch.empty((R, H, W, P), dtype=torch.int32, device=vol.device) if out is None else out
    call("sfmhip_sgm_aggregate", ptr(vol), R, H, W, P, p1, p2, mask, ptr(sm), stream_ptr())
    return sm


def _select(sm: torch.Tensor, a: dict, uniq: int, min_views: int, diagnostics: bool):
    gpu, shape = sm.device, (a["R"], a["H"], a["W"])
    depth = torch.empty(shape, dtype=torch.float32, device=gpu)
    ks = torch.empty(shape, dtype=torch.int32, device=gpu) if diagnostics else None
    best = torch.empty_like(ks) if diagnostics else None
    second = torch.empty_like(ks) if diagnostics else None
    nv = torch.empty(shape, dtype=torch.uint8, device=gpu) if diagnostics else None
    call("sfmhip_volume_select", ptr(sm), ptr(a["ps"]), ptr(a["kk"]), a["V"], a["H"], a["W"], ptr(a["rf"]), ptr(a["sr"]),
         a["R"], a["S"], ptr(a["pl"]), a["P"], uniq, min_views, ptr(depth), ptr(ks), ptr(best), ptr(second), ptr(nv),
         stream_ptr())
    return depth, ks, best, second, nv


def cost_volume(images_or_census, poses, K, refs, srcs, planes, agg_radius: int = 2, penalty: int = 24) -> torch.Tensor:
    """The box-aggregated costs of :func:`plane_sweep` (steps 2 - 4 and 4a of the V10 block of
    include/sfmhip.h) as a volume: (R,H,W,P) uint16 on the device, the plane index innermost
    (at most 37632).  Arguments as for :func:`plane_sweep`.  An invalid reference gives an
    all-zero slice."""
    a = _sweep_inputs(images_or_census, poses, K, refs, srcs, planes, p_max=65535)
    agg_radius, penalty, _, _ = _sweep_ints(agg_radius, penalty, 0, 0)
    return _volume(a, agg_radius, penalty)


def sgm_aggregate(vol, p1: int, p2: int, paths=8) -> torch.Tensor:
    """Semi-global path aggregation (step 4b) of a cost volume (R,H,W,P) uint16 (an int16
    tensor is read as the same bits), P <= 256.  Along each selected direction a pixel's
    cost at plane k takes over the cheapest of its predecessor's costs at k (free), at k - 1 or
    k + 1 (``p1``) or anywhere (``p2``), less the predecessor's minimum; the directions are
    summed.  ``0 <= p1 <= p2 <= 16383``.  ``paths``: 8 for all eight directions, 4 for the two
    along rows and the two along columns, or ``("mask", m)`` with bit i of m selecting
    (dv, du) = (0,+1), (0,-1), (+1,0), (-1,0), (+1,+1), (+1,-1), (-1,+1), (-1,-1).

    Returns (R,H,W,P) int32 on the device holding the sums (below 2^19)."""
    require_gpu()
    if not isinstance(vol, torch.Tensor):
        vol = torch.as_tensor(np.asarray(vol))
    if vol.dtype not in (torch.int16, torch.uint16):
        raise ValueError(f"a cost volume has 16-bit entries, got {vol.dtype}")
    vol = dev(vol, vol.dtype)
    if vol.dim() != 4:
        raise ValueError(f"a cost volume must be (R,H,W,P), got {tuple(vol.shape)}")
    p1, p2, mask = _smooth((p1, p2, paths))
    return _aggregate(vol, p1, p2, mask)


def volume_select(sm, poses, K, refs, srcs, planes, uniq: int = 243, min_views: int = 2, diagnostics: bool = False):
    """Steps 5 - 7 of :func:`plane_sweep` on an aggregated volume ``sm`` (R,H,W,P) int32 (entries
    in [0, 2^24), P <= 256): winner, sub-plane depth, validity.  The cameras, lists and planes are
    those the volume was made with: the count of sources that see a pixel at the winning plane
    is recomputed from them.  Returns what :func:`plane_sweep` returns."""
    require_gpu()
    sm = dev(sm, torch.int32)
    if sm.dim() != 4:
        raise ValueError(f"an aggregated volume must be (R,H,W,P), got {tuple(sm.shape)}")
    a = _sweep_inputs(None, poses, K, refs, srcs, planes, p_max=256, cameras_only=tuple(sm.shape[1:3]))
    if (a["R"], a["P"]) != (sm.shape[0], sm.shape[3]):
        raise ValueError(f"the volume {tuple(sm.shape)} does not match {a['R']} references and {a['P']} planes")
    _, _, uniq, min_views = _sweep_ints(0, 0, uniq, min_views)
    out = _select(sm, a, uniq, min_views, diagnostics)
    return out if diagnostics else out[0]


def depth_consistency(depth, poses, K, refs, srcs, eps: float = 0.01, min_consistent: int = 2):
    """Cross-view check of depth maps (step 8 of the V10 block of include/sfmhip.h).

    depth (V,H,W) f32 with poses (V,3,4) and K (V,4); refs (R,) and srcs (R,S) as for
    :func:`plane_sweep`.  A pixel of reference r with depth d > 0 is projected into every
    source of its row; the source agrees when the pixel lands inside it on a depth ds > 0 with
    ``|ds - zc| <= eps zc``, zc the pixel's depth in the source camera.

    Returns ``count`` (R,H,W) uint8, the agreeing sources, and ``filtered`` (R,H,W) f32: the
    reference depth where ``count >= min_consistent``, else 0 (new tensors on the device)."""
    gpu = require_gpu()
    dp = dev(depth, torch.float32)
    if dp.dim() != 3:
        raise ValueError(f"depth must be (V,H,W), got {tuple(dp.shape)}")
    V, H, W = dp.shape
    ps, kk = _cameras(poses, K, V)
    rf, sr = _lists(refs, srcs)
    R, S = sr.shape
    eps, min_consistent = float(eps), int(min_consistent)
    if not (eps >= 0.0 and np.isfinite(eps)):
        raise ValueError(f"eps must be finite and >= 0, got {eps}")
    if min_consistent < 0:
        raise ValueError(f"min_consistent must be >= 0, got {min_consistent}")
    count = torch.empty((R, H, W), dtype=torch.uint8, device=gpu)
    filtered = torch.empty((R, H, W), dtype=torch.float32, device=gpu)
    call("sfmhip_depth_consistency", ptr(dp), ptr(ps), ptr(kk), V, H, W, ptr(rf), ptr(sr), R, S, eps, min_consistent,
         ptr(count), ptr(filtered), stream_ptr())
    return count, filtered


def mvs_depth(images, poses, K, neighbours, planes, agg_radius: int = 2, penalty: int = 24, uniq: int = 243,
              min_views: int = 2, eps: float = 0.01, min_consistent: int = 2, smooth=None, *,
              dist=None) -> torch.Tensor:
    """Depth maps of V posed images: one census, a plane sweep of every view against its own
    sources, and the cross-view consistency filter.

    images (V,H,W) u8 grey or (V,H,W,3|4) u8; poses (V,3,4) world->camera; K (V,4);
    ``neighbours``: per view, the list of the views it is matched against (at most 16; the
    caller's choice, e.g. the views next to it in the match graph, or
    :func:`~.plan.plan_dense`'s); planes as for :func:`plane_sweep`, or a sequence of V such
    arrays, one per view (``plan_dense``'s ``planes``): view r is then swept with ``planes[r]``,
    one :func:`plane_sweep` call per view.  With one array for all, views with equally long lists
    are swept in one call, so no list is padded; a view with an empty list stays all-invalid
    (and its plane array may be empty).  ``smooth=(p1, p2[, paths])`` sweeps
    with semi-global smoothing as :func:`plane_sweep` does, one view at a time through one
    cost volume and one aggregated volume, so the memory is that of one view.
    ``dist`` (as for :func:`~.rectify.undistort_images`): the images were taken through the
    radial model (K, dist); they are first resampled to the pinhole camera of the same K and
    size, and the depth maps are that camera's.

    Returns depth (V,H,W) f32 on the device with 0 = invalid:
    :func:`~.voxel.tsdf_integrate` takes it as it is, with the same poses and K."""
    gpu = require_gpu()
    if dist is not None:
        images = undistort_images(images, K, dist)[0]
    cen = census_transform(images)
    V, H, W = cen.shape
    ps, kk = _cameras(poses, K, V)
    lists = [[int(s) for s in nb] for nb in neighbours]
    if len(lists) != V:
        raise ValueError(f"neighbours must hold one list per view ({V}), got {len(lists)}")
    if any(len(nb) > 16 for nb in lists):
        raise ValueError("a view has at most 16 neighbours")
    if any(not 0 <= s < V for nb in lists for s in nb):
        raise ValueError(f"a neighbour index lies outside [0, {V})")
    swept = torch.zeros((V, H, W), dtype=torch.float32, device=gpu)
    per_view = isinstance(planes, (list, tuple)) and len(planes) > 0 and all(hasattr(p, "__len__") for p in planes)
    if per_view and len(planes) != V:
        raise ValueError(f"planes must hold one array per view ({V}), got {len(planes)}")
    if per_view and smooth is not None:
        p1, p2, mask = _smooth(smooth)
        agg_radius, penalty, uniq, min_views = _sweep_ints(agg_radius, penalty, uniq, min_views)
        for r in range(V):
            if lists[r]:
                a = _sweep_inputs(cen, ps, kk, [r], [lists[r]], planes[r], p_max=256)
                sm = _aggregate(_volume(a, agg_radius, penalty), p1, p2, mask)
                swept[r] = _select(sm, a, uniq, min_views, False)[0][0]
                del sm
    elif per_view:
        for r in range(V):
            if lists[r]:
                swept[r] = plane_sweep(cen, ps, kk, [r], [lists[r]], planes[r], agg_radius, penalty, uniq, min_views)[0]
    elif smooth is not None:
        p1, p2, mask = _smooth(smooth)
        agg_radius, penalty, uniq, min_views = _sweep_ints(agg_radius, penalty, uniq, min_views)
        pl = _planes(planes, 256)
        vol = torch.empty((1, H, W, pl.shape[0]), dtype=torch.uint16, device=gpu)   # one view's volumes, reused
        sm = torch.empty((1, H, W, pl.shape[0]), dtype=torch.int32, device=gpu)
        for r in range(V):
            if lists[r]:
                a = _sweep_inputs(cen, ps, kk, [r], [lists[r]], pl, p_max=256, already_checked=True)
                _volume(a, agg_radius, penalty, out=vol)
                _aggregate(vol, p1, p2, mask, out=sm)
                swept[r] = _select(sm, a, uniq, min_views, False)[0][0]
    else:
        for S in sorted({len(nb) for nb in lists} - {0}):
            refs = [r for r in range(V) if len(lists[r]) == S]
            swept[refs] = plane_sweep(cen, ps, kk, refs, [lists[r] for r in refs], planes, agg_radius, penalty, uniq,
                                      min_views)
    srcs = np.full((V, max([len(nb) for nb in lists] + [1])), -1, np.int32)
    for r, nb in enumerate(lists):
        srcs[r, :len(nb)] = nb
    return depth_consistency(swept, ps, kk, np.arange(V), srcs, eps, min_consistent)[1]
