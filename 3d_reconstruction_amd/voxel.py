"""V1-V5: voxel-grid kernels with the reference's torch signatures.

* :func:`voxel_traversal` — ``voxel_travesal.py:1-73`` (quirks included:
  one-cell-late negative-direction boundary, overshoot, NaN padding, a ray that
  starts inactive is emitted twice).
* :class:`VoxelGrid` — ``SDFGrid.get_sdf`` / ``get_sdf_sh`` (``sdf.py:284-342``),
  ``NerfModel.forward`` (``plenoxel.py:31-43``) and the composite of
  ``SDFGrid.forward`` / ``render_rays`` (``sdf.py:391-406``,
  ``plenoxel.py:71-93``) for a given sample set ``z`` (the reference draws it
  with ``torch.rand``; callers pass it explicitly).
* :func:`ray_aabb`, :func:`sample_uniform` and :meth:`VoxelGrid.sdf_forward` —
  ``GradientBasedSampler`` (sdf.py:154-180, 220-256; its importance samples
  are discarded by the reference at 251-252) + ``SDFGrid.forward``.
* :func:`tsdf_integrate` — TSDF fusion of depth maps into a (D,H,W) grid laid
  out like the ``sdf.py`` grid (build-defined).
* :func:`tsdf_extract_surface` — the fused grid's iso-surface as a triangle mesh
  (marching tetrahedra, build-defined; ``mesh.write_ply`` stores it).
* :func:`tsdf_raycast` — the depth, normal and colour maps the fused grid predicts.
* :func:`icp_normal_equations`, :func:`icp_track`, :func:`tsdf_track` — frame-to-model
  camera tracking by point-to-plane ICP against the ray-cast maps (build-defined).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from ._abi import call, dev, ptr, require_gpu, stream_ptr

MASK_SDF = 0       # sdf.py test_points: bmin <= p <= bmax (inclusive)
MASK_PLENOXEL = 1  # plenoxel: |p| < scale (strict), p/scale clipped to [-1, 1]


def _f3(v) -> np.ndarray:
    a = np.asarray(v if not isinstance(v, torch.Tensor) else v.detach().cpu().numpy(), dtype=np.float32)
    return np.ascontiguousarray(np.broadcast_to(a.ravel(), (3,)) if a.size == 1 else a.ravel()[:3])


def _host_ptr(a: np.ndarray) -> int:
    """Address of a host array; the caller must keep `a` referenced until the call returns."""
    return a.ctypes.data


def voxel_traversal(rays: torch.Tensor, _bin_size, max_steps: int = 1 << 20) -> torch.Tensor:
    """(N,8) rays [o, d, near, far] -> (N, S, 3) visited voxel indices (float, NaN padded)."""
    require_gpu()
    r = dev(rays, torch.float32)
    N = r.shape[0]
    b = float(_bin_size)
    steps = torch.empty(N, dtype=torch.int32, device=r.device)
    # one walk into rows of width `cap` when they fit a bounded buffer (DDA_CAP; 0 = always two passes):
    # the prefix of the rows is the two-pass result whenever every ray ends within cap - 1 steps
    cap = min(int(os.environ.get("SFMHIP_DDA_CAP", "1024")), int(max_steps) + 1)
    if N > 0 and cap >= 2 and N * cap * 12 <= (256 << 20):
        buf = torch.empty((N, cap, 3), dtype=torch.float32, device=r.device)
        call("sfmhip_voxel_traversal_capped", ptr(r), N, b, cap, ptr(buf), ptr(steps), stream_ptr())
        longest = int(steps.max().item())
        if longest < cap:
            out = torch.empty((N, 1 + longest, 3), dtype=torch.float32, device=r.device)
            call("sfmhip_voxel_traversal_rows", ptr(buf), cap, ptr(steps), N, 1 + longest, ptr(out), stream_ptr())
            return out
    call("sfmhip_voxel_traversal_count", ptr(r), N, b, int(max_steps), ptr(steps), stream_ptr())
    longest = int(steps.max().item()) if N > 0 else 0
    if longest > max_steps:
        raise RuntimeError(f"voxel_traversal: a ray is still active after max_steps={max_steps} "
                           "(the reference loop would not terminate)")
    S = 1 + longest
    out = torch.empty((N, S, 3), dtype=torch.float32, device=r.device)
    call("sfmhip_voxel_traversal", ptr(r), N, b, S, ptr(out), stream_ptr())
    return out


def ray_aabb(rays_o: torch.Tensor, rays_d: torch.Tensor, min_bound, max_bound):
    """sdf.py:154-165 -> (t_near (B,), t_far (B,), valid (B,) bool) device tensors."""
    require_gpu()
    o = dev(rays_o, torch.float32).reshape(-1, 3)
    d = dev(rays_d, torch.float32).reshape(-1, 3)
    B = o.shape[0]
    tn = torch.empty(B, dtype=torch.float32, device=o.device)
    tf = torch.empty_like(tn)
    valid = torch.empty(B, dtype=torch.uint8, device=o.device)
    bmn, bmx = _f3(min_bound), _f3(max_bound)   # kept alive across the call
    call("sfmhip_ray_aabb", ptr(o), ptr(d), B, _host_ptr(bmn), _host_ptr(bmx), ptr(tn), ptr(tf), ptr(valid),
         stream_ptr())
    return tn, tf, valid.bool()


def sample_uniform(t_near: torch.Tensor, t_far: torch.Tensor, num_samples: int, t_rand=None,
                   perturb: bool = True) -> torch.Tensor:
    """sdf.py:167-180: stratified samples (B, S); ``t_rand`` (B, S) is the jitter
    the reference draws with torch.rand_like (drawn here when omitted)."""
    tn = dev(t_near, torch.float32)
    tf = dev(t_far, torch.float32)
    B = tn.shape[0]
    if perturb and t_rand is None:
        t_rand = torch.rand((B, num_samples), device=tn.device)
    tr = dev(t_rand, torch.float32) if perturb else None
    z = torch.empty((B, num_samples), dtype=torch.float32, device=tn.device)
    call("sfmhip_stratified_samples", ptr(tn), ptr(tf), ptr(tr), B, int(num_samples), 1 if perturb else 0,
         ptr(z), stream_ptr())
    return z


class VoxelGrid:
    """An SDF + SH-2 colour grid (1, 28, D, H, W) in the reference layout.

    ``mask_mode`` MASK_SDF reproduces sdf.py (bounds min_bound/max_bound),
    MASK_PLENOXEL reproduces plenoxel.py (bounds +-scale)."""

    def __init__(self, grid: torch.Tensor, min_bound, max_bound, mask_mode: int = MASK_SDF):
        require_gpu()
        g = grid.detach()
        if g.dim() == 5:
            g = g[0]
        self.grid = dev(g, torch.float32)
        self.C, self.D, self.H, self.W = (int(s) for s in self.grid.shape)
        self.bmin = _f3(min_bound)
        self.bmax = _f3(max_bound)
        self.mask_mode = int(mask_mode)
        self._vm = None
        self._finite = None
        self._ver = None

    def invalidate(self) -> None:
        """Drop the cached voxel-major copy and finiteness flag (they are also dropped
        automatically when ``self.grid`` is modified in place: its version counter)."""
        self._vm = None
        self._finite = None
        self._ver = None

    def _sync_cache(self) -> None:
        # self.grid may alias the caller's tensor (dev() does not copy): an in-place update
        # bumps its version, and the derived copies must follow it
        if self._ver is not None and self._ver != self.grid._version:
            self.invalidate()
        self._ver = self.grid._version

    @classmethod
    def plenoxel(cls, voxel_grid: torch.Tensor, scale: float = 1.5) -> "VoxelGrid":
        return cls(voxel_grid, (-scale,) * 3, (scale,) * 3, MASK_PLENOXEL)

    def sample(self, points: torch.Tensor) -> torch.Tensor:
        """All C channels at the points: (P, C) f32 (zero outside)."""
        p = dev(points, torch.float32).reshape(-1, 3)
        out = torch.empty((p.shape[0], self.C), dtype=torch.float32, device=p.device)
        call("sfmhip_grid_sample", ptr(self.grid), self.C, self.D, self.H, self.W, _host_ptr(self.bmin),
             _host_ptr(self.bmax), self.mask_mode, ptr(p), p.shape[0], ptr(out), stream_ptr())
        return out

    def nerf_forward(self, x: torch.Tensor, d: torch.Tensor):
        """NerfModel.forward (plenoxel.py:31-43): (color (P,3), sigma (P,)) at
        points x (P,3) seen along unit directions d (P,3); zero outside."""
        if self.C != 28:
            raise ValueError("nerf_forward needs the 28-channel SDF+SH grid")
        p = dev(x, torch.float32).reshape(-1, 3)
        dd = dev(d, torch.float32).reshape(-1, 3)
        if dd.shape != p.shape:
            raise ValueError("x and d must both be (P, 3)")
        color = torch.empty((p.shape[0], 3), dtype=torch.float32, device=p.device)
        sigma = torch.empty(p.shape[0], dtype=torch.float32, device=p.device)
        call("sfmhip_nerf_forward", ptr(self.grid), self.D, self.H, self.W, _host_ptr(self.bmin), _host_ptr(self.bmax),
             self.mask_mode, ptr(p), ptr(dd), p.shape[0], ptr(color), ptr(sigma), stream_ptr())
        return color, sigma

    def get_sdf(self, points: torch.Tensor) -> torch.Tensor:
        return self.sample(points)[:, 0]

    def get_sdf_sh(self, points: torch.Tensor):
        s = self.sample(points)
        return s[:, 0], s[:, 1:]

    def voxel_major(self) -> torch.Tensor:
        self._sync_cache()
        if self._vm is None:
            if self.C > 32:
                raise ValueError("voxel-major layout supports C <= 32")
            vm = torch.empty((self.D, self.H, self.W, 32), dtype=torch.float32, device=self.grid.device)
            call("sfmhip_grid_to_voxel_major", ptr(self.grid), self.C, self.D, self.H, self.W, ptr(vm),
                 stream_ptr())
            self._vm = vm
        return self._vm

    def sdf_forward(self, rays_o, rays_d, num_samples: int = 160, t_rand=None, perturb: bool = True):
        """SDFGrid.forward (sdf.py:391-406) with its sampler (sdf.py:220-256):
        -> (rgb (Bv,3), pts (Bv,S,3), valid (B,) bool)."""
        o = dev(rays_o, torch.float32).reshape(-1, 3)
        d = dev(rays_d, torch.float32).reshape(-1, 3)
        tn, tf, valid = ray_aabb(o, d, self.bmin, self.bmax)
        if not bool(valid.any()):
            raise ValueError("No valid rays intersect the grid.")
        idx = torch.nonzero(valid).squeeze(1)
        ov, dv = o[idx].contiguous(), d[idx].contiguous()
        z = sample_uniform(tn[idx].contiguous(), tf[idx].contiguous(), num_samples, t_rand, perturb)
        pts = ov[:, None, :] + dv[:, None, :] * z[:, :, None]
        return self.render(ov, dv, z), pts, valid

    def render(self, rays_o: torch.Tensor, rays_d: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
        """Fused sample + SH colour + composite for sorted sample depths z (B,S): (B,3)."""
        if self.C != 28:
            raise ValueError("render needs the 28-channel SDF+SH grid")
        o = dev(rays_o, torch.float32).reshape(-1, 3)
        d = dev(rays_d, torch.float32).reshape(-1, 3)
        zz = dev(z, torch.float32)
        B, S = zz.shape
        rgb = torch.empty((B, 3), dtype=torch.float32, device=o.device)
        vm = self.voxel_major()
        if self.finite():   # sdf from the compact channel-0 plane, voxel lines only where alpha != 0
            call("sfmhip_render_rays_sdf", ptr(vm), ptr(self.grid[0]), self.D, self.H, self.W, _host_ptr(self.bmin),
                 _host_ptr(self.bmax), self.mask_mode, ptr(o), ptr(d), ptr(zz), B, S, ptr(rgb), stream_ptr())
        else:
            call("sfmhip_render_rays", ptr(vm), self.D, self.H, self.W, _host_ptr(self.bmin),
                 _host_ptr(self.bmax), self.mask_mode, ptr(o), ptr(d), ptr(zz), B, S, ptr(rgb), stream_ptr())
        return rgb

    def finite(self) -> bool:
        """Whether every grid value is finite (cached with the voxel-major copy): the render
        may then skip the colour lines of samples with alpha = 0, bit-identically."""
        self._sync_cache()
        if getattr(self, "_finite", None) is None:
            self._finite = bool(torch.isfinite(self.grid).all().item())
        return self._finite


def tsdf_integrate(T: torch.Tensor, Wt: torch.Tensor, depth: torch.Tensor, poses: torch.Tensor,
                   K: torch.Tensor, bmin, bmax, trunc: float, z0: int = 0, z1: int | None = None,
                   block_table: torch.Tensor | None = None) -> None:
    """In-place TSDF update of z-slices [z0, z1) of T/Wt (D,H,W) from F depth maps.

    depth (F,Hd,Wd) f32 (<=0 invalid), poses (F,3,4) world->camera f32,
    K (F,4) [fx, fy, cx, cy] f32, bounds in world units, trunc = mu.
    block_table: optional (F, ceil(Hd/16), ceil(Wd/16), 2) f32 device table from
    tsdf_block_table (e.g. assembled across ranks by dist.shared_block_table);
    the result is bit-identical, the call's own pass over the depth maps skipped.

    Batching: the frames of ONE call are fused order-free in integration steps of
    at most 512 frames (integer fixed-point sums S = sum rint(tsdf 2^21), n = #updates,
    then one finish per voxel and step: T' = (T W + S 2^-21) / (W + n); include/sfmhip.h
    V5 block).  The result therefore depends on how frames are grouped into calls:
    one call with F <= 512 frames gives different low bits than F calls of one frame
    (each a step of its own), and both differ from a sequential running average
    T <- (T W + tsdf)/(W + 1) by at most ~2^-22 per update.  Any z-slab / rank split
    of one call is bit-identical to the whole call.  A caller that streams frames and
    needs batching-independent bits integrates them one frame per call (each frame
    its own step, which IS the sequential running average up to the 2^-21 quantum).
    There is no TSDF in the reference (build-defined)."""
    gpu = require_gpu()
    if T.dtype != torch.float32 or Wt.dtype != torch.float32 or not T.is_contiguous() or not Wt.is_contiguous():
        raise ValueError("T and Wt must be contiguous float32 device tensors")
    if T.dim() != 3 or tuple(Wt.shape) != tuple(T.shape):
        raise ValueError(f"T and Wt must be (D,H,W) tensors of one shape, got {tuple(T.shape)} and "
                         f"{tuple(Wt.shape)}")
    if T.device != gpu or Wt.device != gpu:
        raise ValueError(f"T and Wt must live on the current HIP device {gpu}, got {T.device} / {Wt.device}")
    D, H, W = T.shape
    z1 = D if z1 is None else int(z1)
    if not 0 <= int(z0) <= z1 <= D:
        raise ValueError(f"z-slab [{z0}, {z1}) outside [0, {D}]")
    dp, ps, kk = _frame_args(depth, poses, K)
    F, Hd, Wd = dp.shape
    bmn, bmx = _f3(bmin), _f3(bmax)
    if block_table is None:
        call("sfmhip_tsdf_integrate", ptr(T), ptr(Wt), D, H, W, int(z0), z1, ptr(dp), F, Hd, Wd, ptr(ps), ptr(kk),
             _host_ptr(bmn), _host_ptr(bmx), float(trunc), stream_ptr())
        return
    _check_block_table(block_table, F, Hd, Wd, T.device)
    call("sfmhip_tsdf_integrate_tab", ptr(T), ptr(Wt), D, H, W, int(z0), z1, ptr(dp), F, Hd, Wd, ptr(ps), ptr(kk),
         _host_ptr(bmn), _host_ptr(bmx), float(trunc), ptr(block_table), stream_ptr())


def _frame_args(depth, poses, K):
    """The frame arrays of a TSDF call as contiguous f32 device tensors, shapes checked."""
    dp = dev(depth, torch.float32)
    ps = dev(poses, torch.float32)
    kk = dev(K, torch.float32)
    if dp.dim() != 3:
        raise ValueError(f"depth must be (F,Hd,Wd), got {tuple(dp.shape)}")
    F = dp.shape[0]
    if tuple(ps.shape) != (F, 3, 4):
        raise ValueError(f"poses must be ({F},3,4) to match depth, got {tuple(ps.shape)}")
    if tuple(kk.shape) != (F, 4):
        raise ValueError(f"K must be ({F},4) to match depth, got {tuple(kk.shape)}")
    return dp, ps, kk


def _check_block_table(block_table, F, Hd, Wd, device) -> None:
    if tuple(block_table.shape) != block_table_shape(F, Hd, Wd) or block_table.dtype != torch.float32 or \
            not block_table.is_contiguous() or block_table.device != device:
        raise ValueError(f"block_table must be a contiguous float32 {block_table_shape(F, Hd, Wd)} tensor on {device}")


def tsdf_integrate_colour(C: torch.Tensor, depth: torch.Tensor, colour: torch.Tensor, poses: torch.Tensor,
                          K: torch.Tensor, bmin, bmax, trunc: float, z0: int = 0, z1: int | None = None,
                          block_table: torch.Tensor | None = None) -> None:
    """In-place colour fusion into z-slices [z0, z1) of C (D,H,W,4) int32: per voxel
    {sum_r, sum_g, sum_b, n}, arithmetic modulo 2^32 (the V7 block of include/sfmhip.h).

    depth, poses, K, bounds, trunc and block_table as for :func:`tsdf_integrate`; colour
    (F,Hd,Wd,3) or (F,Hd,Wd,4) uint8, pixel-aligned with depth (r, g, b and an ignored
    fourth byte).  A voxel takes a frame's colour iff :func:`tsdf_integrate` would update it
    from that frame with tsdf < 1: it adds the r, g, b of the pixel the distance update read
    and 1 to n.  Integer sums: any frame order, z-slab split or grouping of the frames into
    calls gives the same bits, and C does not depend on T or Wt.  A channel sum can pass
    2^31 only after 2^23 updates of one voxel.
    :func:`tsdf_extract_surface` (``colours=C``) turns C into per-vertex colours."""
    gpu = require_gpu()
    if not isinstance(C, torch.Tensor) or C.dtype != torch.int32 or not C.is_contiguous() or C.dim() != 4 or \
            C.shape[3] != 4:
        raise ValueError("C must be a contiguous int32 (D,H,W,4) device tensor")
    if C.device != gpu:
        raise ValueError(f"C must live on the current HIP device {gpu}, got {C.device}")
    D, H, W = C.shape[:3]
    z1 = D if z1 is None else int(z1)
    if not 0 <= int(z0) <= z1 <= D:
        raise ValueError(f"z-slab [{z0}, {z1}) outside [0, {D}]")
    dp, ps, kk = _frame_args(depth, poses, K)
    F, Hd, Wd = dp.shape
    col = dev(colour, torch.uint8)
    if col.dim() != 4 or tuple(col.shape[:3]) != (F, Hd, Wd) or col.shape[3] not in (3, 4):
        raise ValueError(f"colour must be ({F},{Hd},{Wd},3|4) uint8 to match depth, got {tuple(col.shape)}")
    if col.shape[3] == 3:   # one dword per pixel
        col = torch.nn.functional.pad(col, (0, 1))
    bmn, bmx = _f3(bmin), _f3(bmax)
    if block_table is not None:
        _check_block_table(block_table, F, Hd, Wd, C.device)
    call("sfmhip_tsdf_integrate_colour", ptr(C), D, H, W, int(z0), z1, ptr(dp), ptr(col), F, Hd, Wd, ptr(ps), ptr(kk),
         _host_ptr(bmn), _host_ptr(bmx), float(trunc), ptr(block_table), stream_ptr())


def block_table_shape(F: int, Hd: int, Wd: int) -> tuple:
    return (int(F), -(-int(Hd) // 16), -(-int(Wd) // 16), 2)


def tsdf_block_table(depth: torch.Tensor, f0: int = 0, f1: int | None = None,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """{min, max} of every 16x16 block of depth maps [f0, f1) (rows f0..f1 of `out`,
    an (F, ceil(Hd/16), ceil(Wd/16), 2) f32 device table, allocated when None)."""
    require_gpu()
    dp = dev(depth, torch.float32)
    F, Hd, Wd = dp.shape
    f1 = F if f1 is None else int(f1)
    if out is None:
        out = torch.empty(block_table_shape(F, Hd, Wd), dtype=torch.float32, device=dp.device)
    elif tuple(out.shape) != block_table_shape(F, Hd, Wd) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 {block_table_shape(F, Hd, Wd)} tensor")
    call("sfmhip_tsdf_block_table", ptr(dp), F, Hd, Wd, int(f0), f1, ptr(out), stream_ptr())
    return out


def tsdf_layer_stats(shape, depth: torch.Tensor, poses: torch.Tensor, K: torch.Tensor, bmin, bmax,
                     trunc: float) -> np.ndarray:
    """Per 8-voxel z layer of the grid `shape` = (D,H,W): (tested, culled, free)
    counts of (wave sub-tile, frame) pairs -- what :func:`tsdf_integrate`'s
    pre-passes decide.  Feeds dist.plan_slabs (cost-balanced z-slabs)."""
    require_gpu()
    D, H, W = (int(v) for v in shape)
    dp = dev(depth, torch.float32)
    ps = dev(poses, torch.float32)
    kk = dev(K, torch.float32)
    F, Hd, Wd = dp.shape
    out = np.zeros((-(-D // 8), 3), np.int64)
    bmn, bmx = _f3(bmin), _f3(bmax)
    call("sfmhip_tsdf_layer_stats", D, H, W, ptr(dp), F, Hd, Wd, ptr(ps), ptr(kk), _host_ptr(bmn), _host_ptr(bmx),
         float(trunc), out.ctypes.data, stream_ptr())
    return out


def tsdf_layer_cost(stats: np.ndarray, w_proj: float = 1.0, w_free: float = 0.12, w_tested: float = 0.02) -> np.ndarray:
    """Cost model of a tile layer from :func:`tsdf_layer_stats`: projected
    (sub-tile, frame) pairs dominate the fusion, free-space runs cost a
    fraction, every tested pair a little (mask walk, cull test)."""
    st = np.asarray(stats, np.float64)
    proj = st[:, 0] - st[:, 1] - st[:, 2]
    return w_proj * proj + w_free * st[:, 2] + w_tested * st[:, 0]


def tsdf_cull_stats(shape, depth: torch.Tensor, poses: torch.Tensor, K: torch.Tensor, bmin, bmax, trunc: float,
                    z0: int = 0, z1: int | None = None) -> dict:
    """Diagnostics of tsdf_integrate's pre-passes on grid `shape` = (D,H,W):
    how many (8x2x8 wave sub-tile, frame) pairs are culled and how many are
    fused as free space (tsdf = 1, no depth gather)."""
    require_gpu()
    D, H, W = (int(v) for v in shape)
    z1 = D if z1 is None else int(z1)
    dp = dev(depth, torch.float32)
    ps = dev(poses, torch.float32)
    kk = dev(K, torch.float32)
    F, Hd, Wd = dp.shape
    st = np.zeros(3, np.int64)
    bmn, bmx = _f3(bmin), _f3(bmax)   # kept alive across the call
    call("sfmhip_tsdf_cull_stats", D, H, W, int(z0), z1, ptr(dp), F, Hd, Wd, ptr(ps), ptr(kk),
         _host_ptr(bmn), _host_ptr(bmx), float(trunc), st.ctypes.data, stream_ptr())
    n = max(int(st[0]), 1)
    return {"tested": int(st[0]), "culled": int(st[1]), "free": int(st[2]),
            "culled_frac": st[1] / n, "free_frac": st[2] / n, "full_frac": 1 - (st[1] + st[2]) / n}


def tsdf_extract_surface(T: torch.Tensor, Wt: torch.Tensor, bmin, bmax, iso: float = 0.0, min_weight: float = 1.0,
                         z0: int = 0, z1: int | None = None, normals: bool = True,
                         colours: torch.Tensor | None = None):
    """Triangle mesh of the iso-surface of a fused TSDF grid (marching tetrahedra on the
    Kuhn 6-tetrahedron split; the semantics are the V6 block of include/sfmhip.h).

    T, Wt: (D,H,W) contiguous f32 device tensors as :func:`tsdf_integrate` leaves them;
    a voxel counts as observed when ``Wt >= min_weight`` and T is finite, and only cells
    whose 8 corners are observed emit triangles.  [z0, z1) is a range of cell layers
    (default: all D-1); the triangle soups of a partition into ranges concatenate to the
    whole call's soup bit for bit (multi-GPU z-slabs).

    Returns device tensors ``(vertices (V,3) f32, normals (V,3) f32 | None, faces (F,3)
    int32)``: a consistently oriented mesh, normals and face orientation towards free
    space (increasing T).  D, H or W of 1, or z0 == z1, gives empty (0,3) outputs.

    ``colours``: the (D,H,W,4) int32 grid of :func:`tsdf_integrate_colour`; the call then
    returns a fourth tensor ``vertex_colours (V,4) uint8`` (r, g, b, alpha; the V7 block of
    include/sfmhip.h): each vertex the interpolation of its edge's two voxel colours, alpha 0
    where neither endpoint ever took a colour sample."""
    gpu = require_gpu()
    if not isinstance(T, torch.Tensor) or not isinstance(Wt, torch.Tensor):
        raise ValueError("T and Wt must be torch tensors")
    if T.dtype != torch.float32 or Wt.dtype != torch.float32 or not T.is_contiguous() or not Wt.is_contiguous():
        raise ValueError("T and Wt must be contiguous float32 device tensors")
    if T.dim() != 3 or tuple(Wt.shape) != tuple(T.shape):
        raise ValueError(f"T and Wt must be (D,H,W) tensors of one shape, got {tuple(T.shape)} and "
                         f"{tuple(Wt.shape)}")
    if T.device != gpu or Wt.device != gpu:
        raise ValueError(f"T and Wt must live on the current HIP device {gpu}, got {T.device} / {Wt.device}")
    D, H, W = T.shape
    if colours is not None:
        if not isinstance(colours, torch.Tensor) or colours.dtype != torch.int32 or not colours.is_contiguous() or \
                tuple(colours.shape) != (D, H, W, 4):
            raise ValueError(f"colours must be a contiguous int32 {(D, H, W, 4)} device tensor")
        if colours.device != gpu:
            raise ValueError(f"colours must live on the current HIP device {gpu}, got {colours.device}")
    if min(D, H, W) < 1:
        raise ValueError(f"empty grid {tuple(T.shape)}")
    z0 = int(z0)
    z1 = D - 1 if z1 is None else int(z1)
    if not 0 <= z0 <= z1 <= D - 1:
        raise ValueError(f"cell-layer range [{z0}, {z1}) outside [0, {D - 1}]")
    if not float(min_weight) > 0.0:
        raise ValueError(f"min_weight must be > 0, got {min_weight}")
    for name, b in (("bmin", bmin), ("bmax", bmax)):
        if np.size(b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b) not in (1, 3):
            raise ValueError(f"{name} must have 1 or 3 components")
    bmn, bmx = _f3(bmin), _f3(bmax)
    nv = (z1 - z0 + 1) * H * W
    nc = (z1 - z0) * (H - 1) * (W - 1)
    empty = z0 == z1 or H < 2 or W < 2
    edge_mask = torch.empty(0 if empty else nv, dtype=torch.uint8, device=gpu)
    vert_off = torch.empty(0 if empty else nv + 1, dtype=torch.int32, device=gpu)
    tri_off = torch.empty(0 if empty else nc + 1, dtype=torch.int32, device=gpu)
    totals = np.zeros(2, np.int64)
    head = (ptr(T), ptr(Wt), D, H, W, z0, z1, float(iso), float(min_weight))
    call("sfmhip_tsdf_surface_count", *head, ptr(edge_mask), ptr(vert_off), ptr(tri_off), totals.ctypes.data,
         stream_ptr())
    nvert, ntri = int(totals[0]), int(totals[1])
    vertices = torch.empty((nvert, 3), dtype=torch.float32, device=gpu)
    nrm = torch.empty((nvert, 3), dtype=torch.float32, device=gpu) if normals else None
    faces = torch.empty((ntri, 3), dtype=torch.int32, device=gpu)
    call("sfmhip_tsdf_surface_emit", *head, _host_ptr(bmn), _host_ptr(bmx), ptr(edge_mask), ptr(vert_off),
         ptr(tri_off), ptr(vertices), ptr(nrm), ptr(faces), stream_ptr())
    if colours is None:
        return vertices, nrm, faces
    rgba = torch.empty((nvert, 4), dtype=torch.uint8, device=gpu)
    call("sfmhip_tsdf_surface_colours", ptr(T), ptr(Wt), ptr(colours), D, H, W, z0, z1, float(iso), float(min_weight),
         ptr(edge_mask), ptr(vert_off), ptr(rgba), stream_ptr())
    return vertices, nrm, faces, rgba


def tsdf_raycast(T: torch.Tensor, Wt: torch.Tensor, poses: torch.Tensor, K: torch.Tensor, size, bmin, bmax,
                 iso: float = 0.0, min_weight: float = 1.0, near: float = 0.0, far: float | None = None,
                 step: float | None = None, normals: bool = False, colours: torch.Tensor | None = None,
                 steps: bool = False):
    """Ray-cast a fused TSDF grid into the depth, normal and colour maps it predicts for V
    cameras (the semantics are the V8 block of include/sfmhip.h).

    T, Wt: (D,H,W) contiguous f32 device tensors as :func:`tsdf_integrate` leaves them; poses
    (V,3,4) world->camera and K (V,4) [fx, fy, cx, cy] as for :func:`tsdf_integrate`;
    ``size`` = (Hd, Wd), pixel centres at integer coordinates.  Each pixel's ray is marched
    in camera depth: samples at Zc = near + k * step, k = 0 .. n_samples-1 with
    ``n_samples = floor((far - near) / step) + 1`` (at most 65536), trilinear T at each, and
    the first front-face crossing (T >= iso, then T < iso, both samples in cells whose 8
    corners are observed: ``Wt >= min_weight`` and T finite) gives the depth by linear
    interpolation; 0 where there is none, :func:`tsdf_integrate`'s "invalid" value, so the
    depth map can be integrated again as it is.

    ``step`` defaults to half the smallest voxel edge, ``far`` to the largest camera depth
    of a corner of the grid box over the views.  The ray direction is not normalised: the
    spacing of the samples along a ray is ``step * |dc|`` with dc = ((u - cx)/fx,
    (v - cy)/fy, 1), larger towards the image corners.  Keep ``step * |dc|`` under the
    truncation distance of the fusion, or a ray can step over the band around the surface.

    Returns device tensors ``(depth (V,Hd,Wd) f32, normals (V,Hd,Wd,3) f32 | None, rgba
    (V,Hd,Wd,4) uint8 | None)``: unit world-frame normals towards increasing T (free space)
    when ``normals``; r, g, b, alpha from ``colours``, the (D,H,W,4) int32 grid of
    :func:`tsdf_integrate_colour` (alpha 0 where no corner of the hit cell ever took a colour
    sample).  ``steps=True`` appends an int32 (V,Hd,Wd) count of the samples the kernel
    evaluated per pixel (a diagnostic of the empty-space skipping, SFMHIP_RAYCAST_SKIP).
    A view with a non-finite (or >= 2^60) pose or intrinsic entry, or fx or fy of 0, gives
    all-zero maps."""
    gpu = require_gpu()
    if not isinstance(T, torch.Tensor) or not isinstance(Wt, torch.Tensor):
        raise ValueError("T and Wt must be torch tensors")
    if T.dtype != torch.float32 or Wt.dtype != torch.float32 or not T.is_contiguous() or not Wt.is_contiguous():
        raise ValueError("T and Wt must be contiguous float32 device tensors")
    if T.dim() != 3 or tuple(Wt.shape) != tuple(T.shape):
        raise ValueError(f"T and Wt must be (D,H,W) tensors of one shape, got {tuple(T.shape)} and "
                         f"{tuple(Wt.shape)}")
    if T.device != gpu or Wt.device != gpu:
        raise ValueError(f"T and Wt must live on the current HIP device {gpu}, got {T.device} / {Wt.device}")
    D, H, W = T.shape
    if min(D, H, W) < 2:
        raise ValueError(f"the grid needs at least 2 voxels per axis, got {tuple(T.shape)}")
    if colours is not None:
        if not isinstance(colours, torch.Tensor) or colours.dtype != torch.int32 or not colours.is_contiguous() or \
                tuple(colours.shape) != (D, H, W, 4):
            raise ValueError(f"colours must be a contiguous int32 {(D, H, W, 4)} device tensor")
        if colours.device != gpu:
            raise ValueError(f"colours must live on the current HIP device {gpu}, got {colours.device}")
    ps = dev(poses, torch.float32)
    kk = dev(K, torch.float32)
    if ps.dim() != 3 or tuple(ps.shape[1:]) != (3, 4):
        raise ValueError(f"poses must be (V,3,4), got {tuple(ps.shape)}")
    V = ps.shape[0]
    if tuple(kk.shape) != (V, 4):
        raise ValueError(f"K must be ({V},4) to match poses, got {tuple(kk.shape)}")
    if np.size(size) != 2:
        raise ValueError(f"size must be (Hd, Wd), got {size}")
    Hd, Wd = (int(v) for v in size)
    if Hd < 0 or Wd < 0:
        raise ValueError(f"size must be non-negative, got {size}")
    if not float(min_weight) > 0.0:
        raise ValueError(f"min_weight must be > 0, got {min_weight}")
    for name, b in (("bmin", bmin), ("bmax", bmax)):
        if np.size(b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b) not in (1, 3):
            raise ValueError(f"{name} must have 1 or 3 components")
    bmn, bmx = _f3(bmin), _f3(bmax)
    lo, hi = bmn.astype(np.float64), bmx.astype(np.float64)
    if not (hi > lo).all():
        raise ValueError(f"bmax must be above bmin on every axis, got {bmin} / {bmax}")
    if step is None:
        step = 0.5 * float(((hi - lo) / np.array([W - 1, H - 1, D - 1], np.float64)).min())
    near, step = float(near), float(step)
    if not (near >= 0.0 and np.isfinite(near)):
        raise ValueError(f"near must be finite and >= 0, got {near}")
    if not (step > 0.0 and np.isfinite(step)):
        raise ValueError(f"step must be finite and > 0, got {step}")
    if far is None:   # the deepest corner of the grid box over the views (host)
        corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        zc = ps[:, 2, :].detach().cpu().numpy().astype(np.float64) @ corners.T
        zc = zc[np.isfinite(zc)]
        far = float(zc.max()) if zc.size else near
    far = float(far)
    if not np.isfinite(far):
        raise ValueError(f"far must be finite, got {far}")
    n_samples = max(int(np.floor((far - near) / step)) + 1, 1)
    if n_samples > 65536:
        raise ValueError(f"{n_samples} samples per ray (far {far}, near {near}, step {step}); at most 65536")
    depth = torch.empty((V, Hd, Wd), dtype=torch.float32, device=gpu)
    nrm = torch.empty((V, Hd, Wd, 3), dtype=torch.float32, device=gpu) if normals else None
    rgba = torch.empty((V, Hd, Wd, 4), dtype=torch.uint8, device=gpu) if colours is not None else None
    cnt = torch.empty((V, Hd, Wd), dtype=torch.int32, device=gpu) if steps else None
    call("sfmhip_tsdf_raycast", ptr(T), ptr(Wt), ptr(colours), D, H, W, ptr(ps), ptr(kk), V, Hd, Wd,
         _host_ptr(bmn), _host_ptr(bmx), float(iso), float(min_weight), near, step, n_samples, ptr(depth), ptr(nrm),
         ptr(rgba), ptr(cnt), stream_ptr())
    return (depth, nrm, rgba, cnt) if steps else (depth, nrm, rgba)


def _icp_args(depth, K, poses, model_depth, model_normals, model_poses, model_K, dist_max, cos_min):
    """The arrays of an ICP call as contiguous f32 device tensors, shapes and gates checked."""
    dp, ps, kk = _frame_args(depth, poses, K)
    B = dp.shape[0]
    md = dev(model_depth, torch.float32)
    mn = dev(model_normals, torch.float32)
    mp = dev(model_poses, torch.float32)
    mk = dev(model_K, torch.float32)
    if md.dim() != 3 or md.shape[0] != B:
        raise ValueError(f"model_depth must be ({B},Hm,Wm) to match depth, got {tuple(md.shape)}")
    if tuple(mn.shape) != tuple(md.shape) + (3,):
        raise ValueError(f"model_normals must be {tuple(md.shape) + (3,)} to match model_depth, got {tuple(mn.shape)}")
    if tuple(mp.shape) != (B, 3, 4):
        raise ValueError(f"model_poses must be ({B},3,4) to match depth, got {tuple(mp.shape)}")
    if tuple(mk.shape) != (B, 4):
        raise ValueError(f"model_K must be ({B},4) to match depth, got {tuple(mk.shape)}")
    dist_max = float(dist_max)
    if not (dist_max > 0.0 and np.isfinite(dist_max)):
        raise ValueError(f"dist_max must be finite and > 0, got {dist_max}")
    dist2 = float(np.float32(dist_max) * np.float32(dist_max))
    if not dist2 > 0.0:
        raise ValueError(f"dist_max squared underflows in float32, got {dist_max}")
    if cos_min is None:
        cos2 = -1.0
    else:
        cos_min = float(cos_min)
        if not 0.0 <= cos_min < 1.0:
            raise ValueError(f"cos_min must be in [0, 1) or None, got {cos_min}")
        cos2 = float(np.float32(cos_min) * np.float32(cos_min))
    return dp, kk, ps, md, mn, mp, mk, dist2, cos2


def icp_normal_equations(depth, K, poses, model_depth, model_normals, model_poses, model_K, dist_max: float,
                         cos_min: float | None = None, mask: bool = False):
    """One point-to-plane linearisation of B depth frames against model maps (the semantics
    are the V9 block of include/sfmhip.h).

    depth (B,Hf,Wf) f32 with K (B,4) [fx, fy, cx, cy] and the current estimates poses
    (B,3,4) world->camera; model_depth (B,Hm,Wm) and model_normals (B,Hm,Wm,3) as
    :func:`tsdf_raycast` returns them for the cameras model_poses / model_K.  A frame pixel is
    paired with the model pixel it projects to and kept when the two points are within
    ``dist_max`` (the gate is ``|e|^2 <= f32(dist_max)^2``) and, unless ``cos_min`` is None,
    the frame's own normal (from its right and lower neighbours) makes an angle with the model
    normal whose cosine is at least ``cos_min`` (in [0, 1)).

    Returns ``sums`` (B,29) f64 on the device: the upper triangle of A = sum J J^T row-major
    (21), g = sum J r (6), E = sum r^2 and the pair count n, with J = (pw x n, n) and
    r = n . (pw - vmod); bit-reproducible from run to run.  ``mask=True`` appends the (B,Hf,Wf)
    uint8 mask of the accepted pixels."""
    gpu = require_gpu()
    dp, kk, ps, md, mn, mp, mk, dist2, cos2 = _icp_args(depth, K, poses, model_depth, model_normals, model_poses,
                                                         model_K, dist_max, cos_min)
    B, Hf, Wf = dp.shape
    sums = torch.zeros((B, 29), dtype=torch.float64, device=gpu)
    msk = torch.zeros((B, Hf, Wf), dtype=torch.uint8, device=gpu) if mask else None
    call("sfmhip_icp_normal_equations", ptr(dp), ptr(kk), ptr(ps), B, Hf, Wf, ptr(md), ptr(mn), ptr(mp), ptr(mk),
         md.shape[1], md.shape[2], dist2, cos2, ptr(sums), ptr(msk), stream_ptr())
    torch.cuda.current_stream().synchronize()
    return (sums, msk) if mask else sums


def icp_track(depth, K, poses0, model_depth, model_normals, model_poses, model_K, dist_max: float,
              cos_min: float | None = None, iters: int = 10, min_pairs: int = 64, log: bool = False):
    """Frame-to-model tracking: ``iters`` Gauss-Newton iterations of point-to-plane ICP from
    ``poses0``, all on the device (two kernel launches per iteration, no host round trip).
    Arguments as for :func:`icp_normal_equations`.

    A view is lost when an iteration finds fewer than ``min_pairs`` (>= 6) pairs or a singular
    system (an LDL^T pivot <= 1e-12 trace(A)): it keeps the pose it had, bit for bit, and its
    later iterations do nothing.  A view with a non-finite camera is lost at once.  A frame
    with no pixels loses every view.

    Returns ``poses`` (B,3,4) f32 and ``lost`` (B,) bool on the device; ``log=True`` appends
    the (B,iters,36) f64 record of every iteration: the 29 sums at its start, the 6 delta =
    (omega, v) it applied, and its status (0 ok, 1 lost, 2 skipped view)."""
    gpu = require_gpu()
    dp, kk, ps, md, mn, mp, mk, dist2, cos2 = _icp_args(depth, K, poses0, model_depth, model_normals, model_poses,
                                                         model_K, dist_max, cos_min)
    iters, min_pairs = int(iters), int(min_pairs)
    if iters < 0:
        raise ValueError(f"iters must be >= 0, got {iters}")
    if min_pairs < 6:
        raise ValueError(f"min_pairs must be at least 6, got {min_pairs}")
    B, Hf, Wf = dp.shape
    out = ps.clone()
    rec = torch.zeros((B, iters, 36), dtype=torch.float64, device=gpu)
    if Hf * Wf == 0:
        rec[:, :, 35] = 1.0
    call("sfmhip_icp_track", ptr(dp), ptr(kk), B, Hf, Wf, ptr(md), ptr(mn), ptr(mp), ptr(mk), md.shape[1],
         md.shape[2], dist2, cos2, iters, min_pairs, ptr(out), ptr(rec), stream_ptr())
    torch.cuda.current_stream().synchronize()
    if iters > 0:
        lost = rec[:, -1, 35] != 0.0
    else:
        lost = torch.zeros((B,), dtype=torch.bool, device=gpu)
    return (out, lost, rec) if log else (out, lost)


def tsdf_track(T: torch.Tensor, Wt: torch.Tensor, depth, K, poses0, bmin, bmax, dist_max: float,
               cos_min: float | None = None, iters: int = 10, min_pairs: int = 64, iso: float = 0.0,
               min_weight: float = 1.0, near: float = 0.0, far: float | None = None, step: float | None = None,
               log: bool = False):
    """Track B depth frames against the fused grid (T, Wt): the model is ray-cast once, at
    ``poses0`` with the frames' own ``K`` and image size (``tsdf_raycast(T, Wt, poses0, K,
    (Hf, Wf), bmin, bmax, iso, min_weight, near, far, step, normals=True)``, so ``step``
    defaults to half the smallest voxel edge and ``far`` to the deepest corner of the grid
    box), and :func:`icp_track` aligns the frames to those maps.  Returns what
    :func:`icp_track` returns; the poses feed :func:`tsdf_integrate` as they are.

    For a coarse level, ray-cast at a smaller size yourself and call :func:`icp_track` with a
    sub-sampled frame and K scaled to match."""
    dp, ps, kk = _frame_args(depth, poses0, K)
    md, mn, _ = tsdf_raycast(T, Wt, ps, kk, tuple(dp.shape[1:]), bmin, bmax, iso=iso, min_weight=min_weight, near=near,
                             far=far, step=step, normals=True)
    return icp_track(dp, kk, ps, md, mn, ps, kk, dist_max, cos_min=cos_min, iters=iters, min_pairs=min_pairs, log=log)
