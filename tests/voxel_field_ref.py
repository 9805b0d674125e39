"""Scenes and float64 models for the radiance-field kernels of voxel.hip (V2 grid sample, V3
ray/box and stratified sampler, V4 composite, the layout kernels and the fused training step).

Shared by test_voxel_field_cpu.py (the f32 oracles against these models) and
test_gpu_voxel_field.py (the kernels against the oracles).  Everything here is written from the
definition of the operation: trilinear interpolation with corners-aligned indexing and zero
padding, the slab test, spherical harmonics of degree 2, alpha compositing and the mean squared
error.  Scenes are seeded and deterministic; `lru_cache` keeps one copy per process, callers
must not write into the arrays they get.
"""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32
SH_C = tuple(float(F32(c)) for c in (0.282095, 0.488603, 1.092548, 0.315392, 0.546274))
LAST_DELTA = float(F32(1e10))


# ---------------------------------------------------------------------------------------------
# rays against a box (V3 ray/box)
BOX_MIN = np.array([-2.0, -1.0, -3.0], F32)
BOX_MAX = np.array([3.0, 2.0, 1.0], F32)
RAYS_B = 3 * 256 + 37

_NAN, _INF = float("nan"), float("inf")
# name -> (origin, direction, class): "valid", "invalid" (finite or infinite t, t_far <= t_near)
# or "nan" (both t are NaN, the ray is invalid)
EDGE_RAYS = {
    # a zero component, origin strictly between that slab's planes: the slab gives (-inf, +inf)
    "zero_x_off_plane": ((0.5, 0.5, -5.0), (0.0, 0.0, 1.0), "valid"),
    "negzero_x_off_plane": ((0.5, 0.5, -5.0), (-0.0, 0.25, 1.0), "valid"),
    "zero_xy_negzero_y": ((1.0, 0.0, 4.0), (0.0, -0.0, -1.0), "valid"),
    # a zero component, origin outside that slab: (+inf, +inf) or (-inf, -inf), never valid
    "zero_x_outside_slab": ((4.0, 0.5, -5.0), (0.0, 0.0, 1.0), "invalid"),
    "negzero_y_outside_slab": ((0.5, -1.5, -5.0), (0.1, -0.0, 1.0), "invalid"),
    # a zero component with the origin ON the slab plane: 0 * inf = NaN
    "zero_x_on_min_plane": ((-2.0, 0.5, -5.0), (0.0, 0.0, 1.0), "nan"),
    "negzero_x_on_max_plane": ((3.0, 0.5, -5.0), (-0.0, 0.0, 1.0), "nan"),
    "zero_z_on_max_plane": ((0.0, 0.0, 1.0), (1.0, 0.5, 0.0), "nan"),
    # origin inside the box: t_near clamps to 0
    "origin_inside": ((0.5, 0.5, -1.0), (0.3, -0.2, 0.9), "valid"),
    "origin_inside_axis": ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), "valid"),
    # box wholly behind the ray: t_far < 0
    "box_behind": ((0.5, 0.5, 5.0), (0.0, 0.1, 1.0), "invalid"),
    "box_behind_diag": ((6.0, 5.0, 4.0), (1.0, 1.0, 1.0), "invalid"),
    # through a box corner: the three slabs meet in one t (exact in f32, the numbers are integers)
    "through_corner_max": ((4.0, 3.0, 2.0), (-1.0, -1.0, -1.0), "valid"),   # enters at (3, 2, 1), t = 1
    "through_corner_min": ((-3.0, -2.0, -4.0), (1.0, 1.0, 1.0), "valid"),   # enters at (-2, -1, -3)
    "touch_corner": ((2.0, 3.0, 2.0), (1.0, -1.0, -1.0), "invalid"),        # t_near = t_far = 1
    # non-finite input
    "nan_origin": ((_NAN, 0.5, -5.0), (0.0, 0.0, 1.0), "nan"),
    "nan_direction": ((0.5, 0.5, -5.0), (0.0, _NAN, 1.0), "nan"),
    "inf_origin": ((_INF, 0.5, -5.0), (1.0, 0.0, 1.0), "invalid"),
    "neginf_origin_zero_dir": ((-_INF, 0.5, -5.0), (0.0, 0.0, 1.0), "invalid"),
    "inf_direction": ((0.5, 0.5, -5.0), (_INF, 0.1, 1.0), "invalid"),       # 1/inf = 0: t = -+0 on x
    "neginf_direction": ((0.5, 0.5, -5.0), (-_INF, 0.1, 1.0), "invalid"),
    "inf_direction_z": ((0.5, 0.5, -5.0), (0.0, 0.0, _INF), "invalid"),     # t_near = t_far = 0
    "inf_origin_inf_direction": ((_INF, 0.5, -5.0), (_INF, 0.0, 1.0), "nan"),   # inf * 0
    # a huge direction: tiny but non-zero t
    "huge_direction": ((0.5, 0.5, -5.0), (1e28, 2e28, 1e30), "valid"),
    "huge_direction_away": ((0.5, 0.5, -5.0), (1e28, 2e28, -1e30), "invalid"),
}


@functools.lru_cache(maxsize=None)
def ray_scene():
    """-> dict(o (B,3), d (B,3), edge {name: row}, bulk: bool (B,)): B = 3*256 + 37 rays against
    the box BOX_MIN..BOX_MAX: a random bulk (about 0.7 of it hits) and the EDGE_RAYS block, spread
    over the launch so that the edge rays sit in every workgroup, the partial last one included."""
    rng = np.random.default_rng(31)
    B = RAYS_B
    o = (rng.normal(0, 2.5, (B, 3)) + [0.5, 0.5, -1.0]).astype(F32)
    tgt = rng.uniform(BOX_MIN - 1.5, BOX_MAX + 1.5, (B, 3))
    d = (tgt - o).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(F32)
    names = list(EDGE_RAYS)
    rows = np.linspace(3, B - 1, len(names)).astype(int)    # the last edge ray is the last ray
    assert len(set(rows.tolist())) == len(names)
    edge = {}
    for name, r in zip(names, rows):
        o[r] = np.array(EDGE_RAYS[name][0], F32)
        d[r] = np.array(EDGE_RAYS[name][1], F32)
        edge[name] = int(r)
    bulk = np.ones(B, bool)
    bulk[rows] = False
    return dict(o=o, d=d, edge=edge, bulk=bulk)


def slab64(o, d, bmin, bmax):
    """The slab test in float64 for rays with finite origins and finite non-zero directions:
    -> (t_near clamped at 0, t_far, valid)."""
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    t0 = (np.asarray(bmin, np.float64) - o) / d
    t1 = (np.asarray(bmax, np.float64) - o) / d
    tn = np.minimum(t0, t1).max(-1)
    tf = np.maximum(t0, t1).min(-1)
    tn = np.maximum(tn, 0.0)
    return tn, tf, tf > tn


# ---------------------------------------------------------------------------------------------
# points against a grid (V2 grid sample)
POINT_GRIDS = ((1, 2, 2, 2), (5, 3, 17, 2), (28, 9, 10, 11), (33, 4, 5, 6))
POINTS_P = 2 * 256 + 19


def point_bounds(mode):
    """Non-cubic bounds in mode 0 (sdf.py's box), +-1.5 in mode 1 (plenoxel's scale)."""
    if mode == 0:
        return np.array([-1.0, -1.2, -0.9], F32), np.array([1.1, 1.0, 1.2], F32)
    return np.full(3, -1.5, F32), np.full(3, 1.5, F32)


def _mask_planes(mode):
    """Per axis the coordinates where the mask switches: (lo, hi) of mode 0, (-s, s) of mode 1."""
    mn, mx = point_bounds(mode)
    return [(mn[a], mx[a]) for a in range(3)] if mode == 0 else [(F32(-mx[0]), mx[0])] * 3


@functools.lru_cache(maxsize=None)
def point_scene(shape, mode):
    """-> dict(grid (C,D,H,W), pts (P,3), bmin, bmax, mode) with P = 2*256 + 19 points: every
    face, edge and corner of the mask exactly (27 - 1 combinations of {lo, mid, hi} per axis),
    the same with every on-plane coordinate moved one ulp inwards and one ulp outwards, NaN and
    +-inf points, and a random bulk inside and outside.  Rows are shuffled."""
    C, D, H, W = shape
    rng = np.random.default_rng(1000 * mode + 7 * C + D + H + W)
    grid = (rng.standard_normal((C, D, H, W)) * 0.3).astype(F32)
    mn, mx = point_bounds(mode)
    planes = _mask_planes(mode)
    special = []
    for shift in (0, -1, 1):            # exact, one ulp inwards, one ulp outwards
        for code in range(27):
            if code == 13:              # (mid, mid, mid) has no plane coordinate
                continue
            p = np.empty(3, F32)
            for a in range(3):
                sel = (code // 3 ** a) % 3
                lo, hi = planes[a]
                mid = F32(0.3 * (a + 1) * 0.5)
                if sel == 1:
                    p[a] = mid
                else:
                    v = lo if sel == 0 else hi
                    if shift:
                        inward = F32(0) if shift < 0 else (F32(-np.inf) if sel == 0 else F32(np.inf))
                        v = np.nextafter(v, inward, dtype=F32)
                    p[a] = v
            special.append(p)
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            p = np.array([0.1, -0.2, 0.3], F32)
            p[a] = bad
            special.append(p)
    special.append(np.full(3, np.nan, F32))
    special = np.array(special, F32)
    P = POINTS_P
    bulk = rng.uniform(-1.7, 1.7, (P - len(special), 3)).astype(F32)
    pts = np.concatenate([special, bulk])[rng.permutation(P)]
    return dict(grid=grid, pts=np.ascontiguousarray(pts), bmin=mn, bmax=mx, mode=mode)


def _inside_and_index64(pts, bmin, bmax, mode, D, H, W):
    """Mask and the continuous voxel index (x -> W, y -> H, z -> D) in float64."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    mn = np.asarray(bmin, np.float64)
    mx = np.asarray(bmax, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 0:
            inside = np.all(p >= mn, 1) & np.all(p <= mx, 1)
            u = (p - mn) / (mx - mn)
        else:
            inside = np.all(np.abs(p) < mx[0], 1)
            u = (np.clip(p / mx[0], -1.0, 1.0) + 1.0) / 2.0
    idx = np.where(inside[:, None], u, 0.0) * np.array([W - 1, H - 1, D - 1], np.float64)
    return inside, idx


def _corners64(idx, D, H, W):
    """The 8 corners of each index's cell: -> (flat voxel (n,8), weight (n,8), in range (n,8))."""
    f = np.floor(idx)
    t = idx - f
    f = f.astype(np.int64)
    vox, wts, oks = [], [], []
    for k in range(8):
        bit = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])
        c = f + bit
        w = np.prod(np.where(bit == 1, t, 1.0 - t), 1)
        ok = (c[:, 0] >= 0) & (c[:, 0] < W) & (c[:, 1] >= 0) & (c[:, 1] < H) & (c[:, 2] >= 0) & (c[:, 2] < D)
        cc = np.clip(c, 0, [W - 1, H - 1, D - 1])
        vox.append((cc[:, 2] * H + cc[:, 1]) * W + cc[:, 0])
        wts.append(w)
        oks.append(ok)
    return np.stack(vox, 1), np.stack(wts, 1), np.stack(oks, 1)


def trilinear64(grid, pts, bmin, bmax, mode):
    """Trilinear sample of grid (C,D,H,W) in float64, corners-aligned, zero padding, zero
    outside the mask: -> (inside (P,), value (P,C), sum |w v| (P,C))."""
    g = np.asarray(grid, np.float64)
    C, D, H, W = g.shape
    inside, idx = _inside_and_index64(pts, bmin, bmax, mode, D, H, W)
    vox, w, ok = _corners64(idx, D, H, W)
    w = np.where(ok & inside[:, None], w, 0.0)
    v = g.reshape(C, -1)[:, vox]                       # (C, P, 8)
    val = (v * w[None]).sum(-1).T
    mag = (np.abs(v) * w[None]).sum(-1).T
    return inside, val, mag


# ---------------------------------------------------------------------------------------------
# the training scene (V4 composite and the fused training step)
TRAIN_SHAPE = (28, 11, 12, 13)
TRAIN_B = 37
TRAIN_MISS = (5, 36)          # every sample outside the mask; 36 is alone in the last workgroup of 4
TRAIN_DEAD = (10, 11)         # sdf <= 0 at every sample
TRAIN_FACE = (20, 21, 22)     # mode 0: axis-aligned, in the x = max / y = max faces, one sample on z = max
TRAIN_S = (1, 2, 63, 64, 65, 128, 129, 256)


def train_bounds(mode):
    return point_bounds(mode)


@functools.lru_cache(maxsize=None)
def train_scene(mode, S):
    """-> dict(grid (28,11,12,13), bmin, bmax, mode, o, d, z (37,S), gt): random rays through
    the box plus the named rays above.  Depths are sorted; ray 0 repeats its first depth
    (delta = 0) and, past one chunk, ray 1 repeats depth 63 at 64."""
    rng = np.random.default_rng(100 * S + mode)
    C, D, H, W = TRAIN_SHAPE
    B = TRAIN_B
    bmin, bmax = train_bounds(mode)
    grid = (rng.standard_normal(TRAIN_SHAPE) * 0.3).astype(F32)
    grid[0] += F32(0.15)     # sdf > 0 on about two thirds of the voxels: enough live samples
    o = (rng.normal(0, 0.25, (B, 3)) + [0, 0, -2.5]).astype(F32)
    d = (rng.normal(0, 0.25, (B, 3)) + [0, 0, 1]).astype(F32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    # depths from in front of the box to just short of its far side: the first samples miss, the
    # last ones (the far side of every chunk boundary) are inside and still lit
    z = np.sort(rng.uniform(0.8, 3.6, (B, S)), 1).astype(F32)
    gt = rng.random((B, 3)).astype(F32)
    for r in TRAIN_MISS:
        o[r] = [5.0, 5.0, -2.5]
        d[r] = [0.0, 0.0, 1.0]
    # the face rays (mode 0 only: mode 1's mask is strict): z = 2 lands exactly on z = max
    # (o_z = max_z - 2 is exact in f32)
    if mode == 0:
        oz = F32(bmax[2] - F32(2.0))
        assert F32(oz + F32(2.0)) == bmax[2]
        for r, (x, y) in zip(TRAIN_FACE, ((bmax[0], F32(0.2)), (F32(0.3), bmax[1]), (bmax[0], bmax[1]))):
            o[r] = [x, y, oz]
            d[r] = [0.0, 0.0, 1.0]
            z[r] = np.sort(rng.uniform(0.05, 2.6, S)).astype(F32)
            z[r, min(int(np.searchsorted(z[r], 2.0)), S - 1)] = 2.0
            z[r].sort()
    if S >= 2:
        z[0, 1] = z[0, 0]
    if S > 64:
        z[1, 64] = z[1, 63]
    for r, (oo, dd) in zip(TRAIN_DEAD, (((0.2, -0.3, -2.5), (0.1, 0.05, 1.0)), ((-0.4, 0.3, -2.5), (-0.05, 0.1, 1.0)))):
        o[r] = oo
        d[r] = (np.array(dd) / np.linalg.norm(dd)).astype(F32)      # oblique, through the middle of the box
    # the dead rays: channel 0 negative on every voxel their samples can reach (their cells and
    # one voxel around, so that an index that rounds across a cell border changes nothing)
    pts = (o[TRAIN_DEAD, None, :].astype(np.float64) + d[TRAIN_DEAD, None, :] * z[TRAIN_DEAD, :, None]).reshape(-1, 3)
    inside, idx = _inside_and_index64(pts, bmin, bmax, mode, D, H, W)
    base = np.floor(idx[inside]).astype(np.int64)
    for dx in (-1, 0, 1, 2):
        for dy in (-1, 0, 1, 2):
            for dz in (-1, 0, 1, 2):
                x = np.clip(base[:, 0] + dx, 0, W - 1)
                y = np.clip(base[:, 1] + dy, 0, H - 1)
                zz = np.clip(base[:, 2] + dz, 0, D - 1)
                grid[0, zz, y, x] = -np.abs(grid[0, zz, y, x]) - F32(0.01)
    return dict(grid=grid, bmin=bmin, bmax=bmax, mode=mode, o=o, d=d, z=z, gt=gt)


def sh_basis64(d):
    """(B,3) -> (B,9): the degree-2 real spherical harmonics in the reference's sign convention."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    C0, C1, C2, C3, C4 = SH_C
    return np.stack([C0 + 0 * x, -C1 * y, C1 * z, -C1 * x, C2 * x * y, -C2 * y * z,
                     C3 * (2 * z * z - x * x - y * y), -C2 * x * z, C4 * (x * x - y * y)], 1)


def autograd64(sc):
    """The f64 model: torch grid_sample (align_corners, zero padding) -> SH colour -> composite
    -> mse, gradient by autograd.  -> dict(loss, rgb (B,3), grad (C,D,H,W), inside (B,S), sdf (B,S))."""
    import torch
    import torch.nn.functional as Fn
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    g = f64(sc["grid"]).requires_grad_(True)
    o, d, z, gt, mn, mx = (f64(sc[k]) for k in ("o", "d", "z", "gt", "bmin", "bmax"))
    B, S = z.shape
    p = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
    if sc["mode"] == 0:
        inside = ((p >= mn) & (p <= mx)).all(1)
        gg = (p - mn) / (mx - mn) * 2 - 1
    else:
        inside = (p.abs() < mx[0]).all(1)
        gg = (p / mx[0]).clamp(-1, 1)
    smp = Fn.grid_sample(g[None], gg[None, None, None], mode="bilinear", padding_mode="zeros",
                         align_corners=True)[0, :, 0, 0].T
    smp = smp * inside[:, None]
    sdf = smp[:, 0].reshape(B, S)
    k = smp[:, 1:].reshape(B, S, 3, 9)
    col = (k * f64(sh_basis64(np.asarray(sc["d"], np.float64)))[:, None, None, :]).sum(-1)
    sig = sdf.clamp(min=0)
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full((B, 1), LAST_DELTA, dtype=torch.float64)], 1)
    a = 1 - torch.exp(-sig * delta)
    T = torch.cumprod(1 - a, 1)
    T = torch.cat([torch.ones(B, 1, dtype=torch.float64), T[:, :-1]], 1)
    w = T * a
    rgb = (w[:, :, None] * col).sum(1) + 1 - w.sum(1)[:, None]
    loss = ((rgb - gt) ** 2).mean()
    loss.backward()
    return dict(loss=float(loss.detach()), rgb=rgb.detach().numpy(), grad=g.grad.numpy(),
                inside=inside.numpy().reshape(B, S), sdf=sdf.detach().numpy())


MUTATIONS = ("v_restart", "delta_per_chunk", "strict_mask", "carry_dropped")


def analytic64(sc, mutation=None, chunk=64):
    """The same model with the backward written out (the transmittance suffix recurrence
    V_{i-1} = a_i e_i + (1 - a_i) V_i and the trilinear scatter), in float64 numpy.  Unmutated it
    equals :func:`autograd64` to rounding.  `mutation` breaks it the way a chunked kernel can
    be broken (the kernel walks a ray in chunks of 64 samples):
      "v_restart"        V restarts at 0 at every multiple of `chunk` in the reverse pass
      "delta_per_chunk"  the 1e10 last delta at the end of every chunk instead of at S - 1
      "strict_mask"      mode 0's inclusive mask made strict
      "carry_dropped"    the transmittance restarts at 1 at every chunk in the forward
    -> dict(loss, rgb, grad)."""
    assert mutation is None or mutation in MUTATIONS
    grid = np.asarray(sc["grid"], np.float64)
    C, D, H, W = grid.shape
    o, d, z, gt = (np.asarray(sc[k], np.float64) for k in ("o", "d", "z", "gt"))
    B, S = z.shape
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
    inside, idx = _inside_and_index64(pts, sc["bmin"], sc["bmax"], sc["mode"], D, H, W)
    if mutation == "strict_mask" and sc["mode"] == 0:
        inside &= np.all(pts > np.asarray(sc["bmin"], np.float64), 1) & np.all(pts < np.asarray(sc["bmax"], np.float64), 1)
    vox, w8, ok = _corners64(idx, D, H, W)
    w8 = np.where(ok & inside[:, None], w8, 0.0)
    smp = (grid.reshape(C, -1)[:, vox] * w8[None]).sum(-1).T          # (P, C)
    sdf = smp[:, 0].reshape(B, S)
    bas = sh_basis64(d)                                               # (B, 9)
    col = (smp[:, 1:].reshape(B, S, 3, 9) * bas[:, None, None, :]).sum(-1)
    sig = np.maximum(sdf, 0.0)
    delta = np.concatenate([z[:, 1:] - z[:, :-1], np.full((B, 1), LAST_DELTA)], 1)
    if mutation == "delta_per_chunk":
        delta[:, chunk - 1::chunk] = LAST_DELTA
    E = np.exp(-sig * delta)
    a = 1 - E
    T = np.ones((B, S))
    for i in range(1, S):
        T[:, i] = 1.0 if (mutation == "carry_dropped" and i % chunk == 0) else T[:, i - 1] * E[:, i - 1]
    w = T * a
    rgb = (w[:, :, None] * col).sum(1) + 1 - w.sum(1)[:, None]
    diff = rgb - gt
    loss = float((diff ** 2).mean())
    g = 2.0 / (3 * B) * diff
    e = ((col - 1) * g[:, None, :]).sum(-1)
    V = np.zeros((B, S))
    acc = np.zeros(B)
    for i in range(S - 1, -1, -1):
        V[:, i] = acc
        acc = a[:, i] * e[:, i] + (1 - a[:, i]) * acc
        if mutation == "v_restart" and i % chunk == 0:
            acc = np.zeros(B)
    dsig = T * (e - V) * E * delta
    dsdf = np.where(sdf > 0, dsig, 0.0)
    dk = ((w[:, :, None] * g[:, None, :])[:, :, :, None] * bas[:, None, None, :]).reshape(B * S, 27)
    dsmp = np.concatenate([dsdf.reshape(-1, 1), dk], 1)               # (P, 28)
    grad = np.zeros((C, D * H * W))
    for k in range(8):
        np.add.at(grad.T, vox[:, k], w8[:, k, None] * dsmp)
    return dict(loss=loss, rgb=rgb, grad=grad.reshape(C, D, H, W))


def distances(loss, rgb, grad, ref):
    """(max |rgb - ref|, |loss - ref| / ref, max |grad - ref| / max |ref grad|)."""
    sc = np.abs(ref["grad"]).max()
    return (float(np.abs(rgb - ref["rgb"]).max()), abs(loss - ref["loss"]) / ref["loss"],
            float(np.abs(grad - ref["grad"]).max() / sc) if sc > 0 else float(np.abs(grad).max()))


# oracle.train.render_loss_grad against autograd64 on train_scene(mode, S), as measured by
# test_voxel_field_cpu.py::test_train_oracle_vs_f64 (run with -s to print them again):
# (mode, S) -> (max |rgb diff|, relative loss diff, max |grad diff| / max |grad|)
ORACLE_VS_F64 = {
    (0, 1): (5.19e-07, 3.48e-08, 7.25e-07),
    (0, 2): (5.14e-07, 2.42e-08, 1.03e-06),
    (0, 63): (3.39e-07, 1.63e-08, 5.32e-07),
    (0, 64): (4.60e-07, 4.56e-08, 1.44e-06),
    (0, 65): (5.12e-07, 1.67e-08, 1.19e-06),
    (0, 128): (5.93e-07, 3.94e-08, 1.48e-06),
    (0, 129): (6.34e-07, 1.77e-07, 1.48e-06),
    (0, 256): (9.95e-07, 1.05e-07, 1.54e-06),
    (1, 1): (5.38e-07, 4.83e-08, 8.41e-07),
    (1, 2): (8.77e-07, 6.91e-10, 1.07e-06),
    (1, 63): (4.50e-07, 6.49e-08, 1.17e-06),
    (1, 64): (4.04e-07, 6.04e-08, 1.20e-06),
    (1, 65): (4.42e-07, 9.03e-08, 7.24e-07),
    (1, 128): (5.33e-07, 1.53e-07, 6.16e-07),
    (1, 129): (7.57e-07, 1.14e-07, 1.60e-06),
    (1, 256): (6.59e-07, 6.87e-08, 9.39e-07),
}
# the largest of each column: the "measured value" the CPU gates double (the K7 rule).  A single
# case's loss distance can be small by cancellation (6.9e-10 at (1, 2)), which says nothing
# about the next machine's exp(); the column maximum does
ORACLE_VS_F64_MAX = tuple(max(v[i] for v in ORACLE_VS_F64.values()) for i in range(3))
