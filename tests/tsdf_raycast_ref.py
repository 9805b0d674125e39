"""Numpy restatement of the TSDF ray-cast (semantics in include/sfmhip.h, "V8"), a numpy
model of the HIP kernel's skip rule, and the scenes of the ray-cast tests.  A plain helper
module: not a test, not a conftest.

Everything is f32, one IEEE operation per step (numpy never fuses), so depth and rgba of the
HIP kernel are compared bit for bit.  :func:`raycast` is a plain uniform march over every
sample of every ray: no clipping, no skipping.  :func:`raycast_skip_model` follows the
kernel's control flow (box clipping, brick table, verified jumps) lane by lane and must give
the same bits; its `steps` count shows the skipping at work.
"""
from __future__ import annotations

import itertools

import numpy as np

F32 = np.float32
U32 = np.uint32
NAN = F32(np.nan)
BRICK = 8


# ---- the definition ---------------------------------------------------------------
class _Geo:
    def __init__(self, shape, bmin, bmax):
        D, H, W = shape
        self.dim = np.array([W, H, D], np.int64)   # x, y, z
        self.bmin = np.asarray(bmin, F32).reshape(3)
        self.bmax = np.asarray(bmax, F32).reshape(3)
        self.s = (self.bmax - self.bmin) / (self.dim - 1).astype(F32)
        assert self.s.dtype == F32 and (self.s > 0).all()
        self.hi = (self.dim - 2).astype(F32)


def observed_grid(T, Wt, min_weight):
    """G = T where observed (Wt >= min_weight and T finite), else NaN."""
    T = np.ascontiguousarray(T, F32)
    obs = (np.asarray(Wt, F32) >= F32(min_weight)) & np.isfinite(T)
    return np.where(obs, T, NAN).astype(F32)


def rays(poses, K, Hd, Wd):
    """-> good (V,), o (V,3), dw (V,Hd,Wd,3), all f32, op by op as the header writes them."""
    P = np.asarray(poses, F32).reshape(-1, 12)
    K = np.asarray(K, F32).reshape(-1, 4)
    V = P.shape[0]
    with np.errstate(all="ignore"):
        good = (np.abs(np.concatenate([P, K], 1)) < F32(2.0 ** 60)).all(1) & (K[:, 0] != 0) & (K[:, 1] != 0)
        u = np.arange(Wd, dtype=F32)[None, None, :]
        v = np.arange(Hd, dtype=F32)[None, :, None]
        dcx = (u - K[:, 2, None, None]) / K[:, 0, None, None] + np.zeros((V, Hd, Wd), F32)
        dcy = (v - K[:, 3, None, None]) / K[:, 1, None, None] + np.zeros((V, Hd, Wd), F32)
        o = np.empty((V, 3), F32)
        dw = np.empty((V, Hd, Wd, 3), F32)
        for a in range(3):
            o[:, a] = -((P[:, a] * P[:, 3] + P[:, 4 + a] * P[:, 7]) + P[:, 8 + a] * P[:, 11])
            dw[..., a] = (P[:, a, None, None] * dcx + P[:, 4 + a, None, None] * dcy) + P[:, 8 + a, None, None]
    assert o.dtype == F32 and dw.dtype == F32
    return good, o, dw


def cell_at(o, dw, t, geo):
    """Cell of the points o + t dw (o, dw (N,3), t (N,) f32) -> i (N,3) int64 (0 where out),
    f (N,3) f32, oc (N,) out-code: bit 2a below / 2a+1 above the grid on axis a, 64 NaN."""
    with np.errstate(all="ignore"):
        p = o + t[:, None] * dw
        g = (p - geo.bmin) / geo.s
        fl = np.floor(g)
        f = g - fl
        lo = fl < 0
        hi = fl > geo.hi
        nan = ~(fl >= 0) & ~lo
        sh = np.array([0, 2, 4])
        oc = (lo << sh).sum(1) | ((hi & ~lo) << (sh + 1)).sum(1) | (nan.any(1) * 64)
        i = np.where(lo | hi | nan, 0, fl).astype(np.int64)
    assert f.dtype == F32
    return i, f, oc.astype(np.int64)


def lerp(a, b, w):
    return a + w * (b - a)


def corners(G, i):
    """(N,8) f32 corner values of in-range cells, index dx + 2 dy + 4 dz."""
    return np.stack([G[i[:, 2] + (j >> 2), i[:, 1] + ((j >> 1) & 1), i[:, 0] + (j & 1)] for j in range(8)], 1)


def eval_F(G, i, f, oc):
    """Trilinear F (x, then y, then z); NaN where the cell is out of range or a corner is NaN."""
    F = np.full(i.shape[0], NAN, F32)
    ok = np.nonzero(oc == 0)[0]
    if ok.size:
        with np.errstate(all="ignore"):
            t = corners(G, i[ok])
            fx, fy, fz = f[ok, 0], f[ok, 1], f[ok, 2]
            a00, a01 = lerp(t[:, 0], t[:, 1], fx), lerp(t[:, 2], t[:, 3], fx)
            a10, a11 = lerp(t[:, 4], t[:, 5], fx), lerp(t[:, 6], t[:, 7], fx)
            F[ok] = lerp(lerp(a00, a01, fy), lerp(a10, a11, fy), fz)
    return F


def t_of(k, near, step):
    return (F32(near) + np.asarray(k).astype(F32) * F32(step)).astype(F32)


def _finish(G, C, geo, o, dw, hit, km1, Fp, Fc, iso, near, step, normals, colours):
    """depth, normals, rgba of N rays from each ray's crossing pair (k-1, k)."""
    N = o.shape[0]
    depth = np.zeros(N, F32)
    nrm = np.zeros((N, 3), F32) if normals else None
    rgba = np.zeros((N, 4), np.uint8) if colours else None
    h = np.nonzero(hit)[0]
    if h.size == 0:
        return depth, nrm, rgba
    with np.errstate(all="ignore"):
        d = t_of(km1[h], near, step) + F32(step) * ((Fp[h] - F32(iso)) / (Fp[h] - Fc[h]))
        depth[h] = d
        if not normals and not colours:
            return depth, nrm, rgba
        i, f, oc = cell_at(o[h], dw[h], d, geo)
        valid = oc == 0
        t = np.full((h.size, 8), NAN, F32)
        t[valid] = corners(G, i[valid])
        valid &= ~np.isnan(t).any(1)
        h, i, f, t = h[valid], i[valid], f[valid], t[valid]
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        if normals and h.size:
            gx = lerp(lerp(t[:, 1] - t[:, 0], t[:, 3] - t[:, 2], fy), lerp(t[:, 5] - t[:, 4], t[:, 7] - t[:, 6], fy),
                      fz) / geo.s[0]
            gy = lerp(lerp(t[:, 2] - t[:, 0], t[:, 3] - t[:, 1], fx), lerp(t[:, 6] - t[:, 4], t[:, 7] - t[:, 5], fx),
                      fz) / geo.s[1]
            gz = lerp(lerp(t[:, 4] - t[:, 0], t[:, 5] - t[:, 1], fx), lerp(t[:, 6] - t[:, 2], t[:, 7] - t[:, 3], fx),
                      fy) / geo.s[2]
            ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
            ok = np.isfinite(ln) & (ln > 0)
            g = np.stack([gx, gy, gz], 1)
            nrm[h] = np.where(ok[:, None], g / ln[:, None], F32(0)).astype(F32)
        if colours and h.size:
            num = np.zeros((h.size, 3), F32)
            den = np.zeros(h.size, F32)
            anyc = np.zeros(h.size, bool)
            one = F32(1)
            for j in range(8):
                q = C[i[:, 2] + (j >> 2), i[:, 1] + ((j >> 1) & 1), i[:, 0] + (j & 1)].astype(U32)
                has = q[:, 3] > 0
                ux = fx if j & 1 else one - fx
                uy = fy if j & 2 else one - fy
                uz = fz if j & 4 else one - fz
                w = (ux * uy) * uz
                col = q[:, :3].astype(F32) / q[:, 3].astype(F32)[:, None]
                num = np.where(has[:, None], num + w[:, None] * col, num).astype(F32)
                den = np.where(has, den + w, den).astype(F32)
                anyc |= has
            m = num / den[:, None]
            byte = np.rint(np.fmin(F32(255), np.fmax(F32(0), m))).astype(np.uint8)
            out = np.concatenate([byte, np.full((h.size, 1), 255, np.uint8)], 1)
            rgba[h] = np.where(anyc[:, None], out, 0)
    return depth, nrm, rgba


def _setup(T, Wt, C, poses, K, size, bmin, bmax, min_weight, near, step, n_samples):
    if not min_weight > 0:
        raise ValueError("min_weight must be > 0")
    if not (near >= 0 and step > 0 and 1 <= n_samples <= 65536):
        raise ValueError("bad near / step / n_samples")
    Hd, Wd = size
    G = observed_grid(T, Wt, min_weight)
    geo = _Geo(G.shape, bmin, bmax)
    good, o, dw = rays(poses, K, Hd, Wd)
    V = o.shape[0]
    o = np.repeat(o, Hd * Wd, 0).reshape(-1, 3)
    dw = dw.reshape(-1, 3)
    good = np.repeat(good, Hd * Wd)
    if C is not None:
        C = np.ascontiguousarray(C).view(U32).reshape(G.shape + (4,))
    return G, C, geo, good, o, dw, (V, Hd, Wd)


def _shape_out(res, shp, steps=None):
    depth, nrm, rgba = res
    out = (depth.reshape(shp), None if nrm is None else nrm.reshape(shp + (3,)),
           None if rgba is None else rgba.reshape(shp + (4,)))
    return out if steps is None else out + (steps.reshape(shp),)


def raycast(T, Wt, poses, K, size, bmin, bmax, iso=0.0, min_weight=1.0, near=0.0, step=None, n_samples=1,
            normals=False, colours=None):
    """The definition: every sample of every ray.  -> depth (V,Hd,Wd) f32, normals
    (V,Hd,Wd,3) f32 | None, rgba (V,Hd,Wd,4) u8 | None."""
    G, C, geo, good, o, dw, shp = _setup(T, Wt, colours, poses, K, size, bmin, bmax, min_weight, near, step, n_samples)
    N = o.shape[0]
    hit = np.zeros(N, bool)
    km1 = np.zeros(N, np.int64)
    Fp_hit = np.zeros(N, F32)
    Fc_hit = np.zeros(N, F32)
    iso32 = F32(iso)
    if N:
        Fp = eval_F(G, *cell_at(o, dw, np.full(N, t_of(0, near, step), F32), geo))
        for k in range(1, n_samples):
            Fc = eval_F(G, *cell_at(o, dw, np.full(N, t_of(k, near, step), F32), geo))
            with np.errstate(invalid="ignore"):
                new = good & ~hit & (Fp >= iso32) & (Fc < iso32)
            km1[new], Fp_hit[new], Fc_hit[new] = k - 1, Fp[new], Fc[new]
            hit |= new
            Fp = Fc
    return _shape_out(_finish(G, C, geo, o, dw, hit, km1, Fp_hit, Fc_hit, iso, near, step, normals,
                              colours is not None), shp)


# ---- the kernel's skip rule ---------------------------------------------------------
def brick_table(G, iso):
    """(nbz, nby, nbx) bool: no sample whose cell origin lies in the brick can have F < iso.
    Over the observed voxels of the brick dilated by one (up): L = min, A = max |.|; ruled
    out when none is observed, or A < 2^126 and L >= iso + (2^-19 A + 2^-126) (in f64)."""
    D, H, W = G.shape
    nb = [-(-n // BRICK) for n in (D, H, W)]
    tab = np.zeros(nb, bool)
    for bz, by, bx in itertools.product(*[range(n) for n in nb]):
        blk = G[bz * 8:bz * 8 + 9, by * 8:by * 8 + 9, bx * 8:bx * 8 + 9]
        v = blk[~np.isnan(blk)].astype(np.float64)
        if v.size == 0:
            tab[bz, by, bx] = True
            continue
        L, A = v.min(), np.abs(v).max()
        tab[bz, by, bx] = A < 2.0 ** 126 and L >= float(F32(iso)) + (A * 2.0 ** -19 + 2.0 ** -126)
    return tab


def _clamp_index(x, n):
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(x, F32(0)), F32(n)).astype(np.int64)


def raycast_skip_model(T, Wt, poses, K, size, bmin, bmax, iso=0.0, min_weight=1.0, near=0.0, step=None, n_samples=1,
                       normals=False, colours=None):
    """The march as the HIP kernel runs it with SFMHIP_RAYCAST_SKIP=1, every lane advanced in
    lock step.  -> depth, normals, rgba, steps (samples evaluated per pixel)."""
    G, C, geo, good, o, dw, shp = _setup(T, Wt, colours, poses, K, size, bmin, bmax, min_weight, near, step, n_samples)
    N, n = o.shape[0], int(n_samples)
    tab = brick_table(G, iso)
    iso32 = F32(iso)
    cell = lambda idx, k: cell_at(o[idx], dw[idx], t_of(k, near, step), geo)   # noqa: E731
    brick = lambda i: (i[:, 2] >> 3, i[:, 1] >> 3, i[:, 0] >> 3)   # noqa: E731
    same_brick = lambda a, b: ((a >> 3) == (b >> 3)).all(1)   # noqa: E731

    with np.errstate(all="ignore"):
        k = np.ones(N, np.int64)
        n_eff = np.where(good & np.isfinite(o).all(1) & np.isfinite(dw).all(1), n, 0)
        inv_step = F32(1) / F32(step)
        inv_dw = F32(1) / dw
        idx = np.nonzero(n_eff > 2)[0]
        if idx.size:   # box clipping
            t0 = (geo.bmin - o[idx]) * inv_dw[idx]
            t1 = (geo.bmax - o[idx]) * inv_dw[idx]
            tin = np.fmax.reduce(np.concatenate([np.full((idx.size, 1), -np.inf, F32), np.fmin(t0, t1)], 1), 1)
            tout = np.fmin.reduce(np.concatenate([np.full((idx.size, 1), np.inf, F32), np.fmax(t0, t1)], 1), 1)
            _, _, oc_last = cell(idx, np.full(idx.size, n - 1))
            kx = _clamp_index(np.ceil((tout - F32(near)) * inv_step) + F32(2), n)
            _, _, oc_x = cell(idx, kx)
            cut = (kx < n - 1) & ((oc_last & oc_x & 63) != 0)
            n_eff[idx[cut]] = kx[cut]
            ki = np.minimum(_clamp_index(np.floor((tin - F32(near)) * inv_step) - F32(2), n), n_eff[idx] - 1)
            _, _, oc_1 = cell(idx, np.ones(idx.size))
            _, _, oc_i = cell(idx, np.maximum(ki, 0))
            ent = (ki > 1) & ((oc_1 & oc_i & 63) != 0)
            k[idx[ent]] = ki[ent] + 1
        have = np.zeros(N, bool)
        jump = np.ones(N, np.int64)
        Fp = np.zeros(N, F32)
        Fc = np.zeros(N, F32)
        hit = np.zeros(N, bool)
        evals = np.zeros(N, np.int64)
        while True:
            idx = np.nonzero(~hit & (k < n_eff))[0]
            if idx.size == 0:
                break
            i, f, oc = cell(idx, k[idx])
            skip = np.zeros(idx.size, bool)
            adv = np.ones(idx.size, np.int64)
            # outside the grid
            a = np.nonzero(oc != 0)[0]
            if a.size:
                skip[a] = True
                kk = np.minimum(k[idx[a]] + jump[idx[a]], n_eff[idx[a]] - 1)
                _, _, oce = cell(idx[a], kk)
                tried = (kk > k[idx[a]]) & ((oc[a] & 63) != 0)
                okj = tried & ((oc[a] & oce & 63) != 0)
                adv[a] = np.where(okj, kk - k[idx[a]] + 1, 1)
                ja = jump[idx[a]]
                jump[idx[a]] = np.where(okj, np.minimum(ja * 2, 1 << 14), np.where(tried, np.maximum(ja >> 1, 1), ja))
            # inside: ruled-out bricks
            b = np.nonzero(oc == 0)[0]
            if b.size:
                out = tab[brick(i[b])]
                b = b[out]
            if b.size:
                skip[b] = True
                ib, lb = i[b], idx[b]
                b0 = (ib >> 3) << 3
                edge = geo.bmin + np.where(dw[lb] > 0, b0 + BRICK, b0).astype(F32) * geo.s
                ta = np.where(dw[lb] != 0, (edge - o[lb]) * inv_dw[lb], F32(np.inf)).astype(F32)
                tex = np.fmin.reduce(np.concatenate([np.full((b.size, 1), np.inf, F32), ta], 1), 1)
                kk = np.minimum(_clamp_index(np.floor((tex - F32(near)) * inv_step) - F32(1), n), n_eff[lb] - 1)
                ie, _, oce = cell(lb, np.maximum(kk, 0))
                okj = (kk > k[lb]) & (oce == 0) & same_brick(ie, ib)
                adv[b] = np.where(okj, kk - k[lb] + 1, 1)
            s = idx[skip]
            k[s] += adv[skip]
            have[s] = False
            e = np.nonzero(~skip)[0]
            if e.size == 0:
                continue
            le = idx[e]
            need = ~have[le]
            if need.any():
                ln = le[need]
                Fp[ln] = eval_F(G, *cell(ln, k[ln] - 1))
                evals[ln] += 1
            Fc[le] = eval_F(G, i[e], f[e], oc[e])
            evals[le] += 1
            h = (Fp[le] >= iso32) & (Fc[le] < iso32)
            hit[le[h]] = True
            go = le[~h]
            Fp[go] = Fc[go]
            have[go] = True
            k[go] += 1
    res = _finish(G, C, geo, o, dw, hit, k - 1, Fp, Fc, iso, near, step, normals, colours is not None)
    return _shape_out(res, shp, evals.astype(np.int32))


def sample_count(near, far, step):
    """n_samples as voxel.tsdf_raycast derives it."""
    return max(int(np.floor((float(far) - float(near)) / float(step))) + 1, 1)


# ---- scenes ---------------------------------------------------------------------------
def look_at(c, target, up=(0.0, 1.0, 0.0)):
    """(3,4) f32 world->camera pose of a camera at c looking at target (camera z forward)."""
    c, target = np.asarray(c, np.float64), np.asarray(target, np.float64)
    z = (target - c) / np.linalg.norm(target - c)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, (-R @ c)[:, None]], 1).astype(F32)


def random_colour_grid(shape, rng):
    n = rng.integers(1, 40, shape).astype(U32)
    n[rng.random(shape) < 0.3] = 0
    C = np.zeros(shape + (4,), U32)
    C[..., :3] = (rng.random(shape + (3,)) * 255 * n[..., None]).astype(U32)
    C[..., 3] = n
    return C


def random_scene(seed=11):
    """Scene 1: 9 x 11 x 70, uniform T in [-1, 1], Wt in {0..3}, a few NaN / +-inf and one
    finite 1e30, min_weight 2, iso 0.25, non-unit non-cubic bounds, 2 views of 45 x 62."""
    rng = np.random.default_rng(seed)
    shape = (9, 11, 70)
    T = rng.uniform(-1, 1, shape).astype(F32)
    Wt = rng.integers(0, 4, shape).astype(F32)
    Wt[rng.random(shape) < 0.5] = 3     # most voxels observed, so that valid cells exist
    bad = rng.integers(0, T.size, 12)
    T.reshape(-1)[bad[:4]] = np.nan
    T.reshape(-1)[bad[4:8]] = np.inf
    T.reshape(-1)[bad[8:11]] = -np.inf
    T.reshape(-1)[bad[11]] = 1e30
    Wt.reshape(-1)[bad] = 3
    bmin, bmax = (-1.0, 0.5, 2.0), (2.5, 1.75, 3.0)
    centre = (0.75, 1.125, 2.5)
    poses = np.stack([look_at((0.5, 1.6, -0.5), centre), look_at((3.6, 0.2, 4.4), centre)])
    K = np.array([[60.0, 55.0, 30.5, 22.25], [48.0, 52.0, 31.0, 22.0]], F32)
    step = 0.5 * 1.0 / 8
    return dict(T=T, Wt=Wt, C=random_colour_grid(shape, rng), poses=poses, K=K, size=(45, 62), bmin=bmin, bmax=bmax,
                iso=0.25, min_weight=2.0, near=0.0, far=6.0, step=step, n_samples=sample_count(0.0, 6.0, step))


def adversarial_scene(layer):
    """Scene 3: 37 x 29 x 21, unobserved except (a) a slab two z-layers thick whose crossing
    lies between z-layers layer | layer + 1 (7: the cell's far corners belong to the next
    brick; 8: the cell starts the brick), (b) a lone 2x2x2 cell at voxels 7..8 on all axes,
    where eight bricks meet, (c) a crossing in the last, partial bricks.  Voxel edge 0.25
    (exact), so camera centres at multiples of 0.25 send rays exactly along brick faces."""
    D, H, W = 37, 29, 21
    T = np.zeros((D, H, W), F32)
    Wt = np.zeros((D, H, W), F32)
    rng = np.random.default_rng(layer)
    Wt[layer:layer + 2, 12:28, :] = 1
    T[layer, 12:28, :] = 0.5 + 0.2 * rng.random((16, W))
    T[layer + 1, 12:28, :] = -0.5 + 0.2 * rng.random((16, W))
    Wt[7:9, 7:9, 7:9] = 1
    T[7, 7:9, 7:9] = 0.6 + 0.1 * rng.random((2, 2))
    T[8, 7:9, 7:9] = -0.4 + 0.1 * rng.random((2, 2))
    Wt[33:37, 1:6, 14:21] = 1
    T[33:37, 1:6, 14:21] = ((34.5 - np.arange(33, 37)) * 0.4)[:, None, None] + 0.05 * rng.random((4, 5, 7))
    s = 0.25
    bmin, bmax = (0.0, 0.0, 0.0), ((W - 1) * s, (H - 1) * s, (D - 1) * s)
    ident = lambda c: np.concatenate([np.eye(3), -np.asarray(c, np.float64)[:, None]], 1).astype(F32)   # noqa: E731
    poses = np.stack([
        ident((2.0, 2.0, -2.0)),     # centre ray along the brick edge x = 8, y = 8 voxels
        ident((4.0, 4.0, -1.0)),     # brick faces x = 16, y = 16
        ident((1.875, 1.875, -2.0)),   # through the lone cell (voxel 7.5)
        look_at((8.0, 7.0, -3.0), (2.5, 3.5, 4.5)),
        look_at((-2.0, 1.0, 12.0), (3.0, 2.0, 6.0)),
    ])
    K = np.array([[40.0, 40.0, 31.0, 22.0]] * 3 + [[50.0, 45.0, 30.5, 22.5]] * 2, F32)
    step = 0.3 * s
    return dict(T=T, Wt=Wt, C=None, poses=poses, K=K, size=(45, 62), bmin=bmin, bmax=bmax, iso=0.0, min_weight=1.0,
                near=0.0, far=14.0, step=step, n_samples=sample_count(0.0, 14.0, step))


def call_args(s, **kw):
    """Keyword arguments of raycast / raycast_skip_model for a scene dict."""
    a = dict(T=s["T"], Wt=s["Wt"], poses=s["poses"], K=s["K"], size=s["size"], bmin=s["bmin"], bmax=s["bmax"],
             iso=s["iso"], min_weight=s["min_weight"], near=s["near"], step=s["step"], n_samples=s["n_samples"],
             colours=s.get("C"))
    a.update(kw)
    return a


# ---- sphere known answer --------------------------------------------------------------
def raycast_sphere_bound(R, r, step, dc_max, **_):
    """Largest distance of a hit point from the sphere, derived like surface_ref.sphere_bound.
    With h the voxel edge and delta = step * dc_max the spacing of samples along a ray, both
    samples of the crossing pair lie within delta of the surface and their cells' corners
    within delta + sqrt(3) h: inside the unclipped band (mu = 3 h) and where the distance
    function's curvature is at most 1/rho, rho = r - (delta + sqrt(3) h).  (1) Trilinear
    interpolation of a function errs by at most sum_a h^2/8 max|d2/da2|; the distance to a
    sphere has Hessian (I - n n^T)/rho' with trace 2/rho': h^2 / (4 rho).  (2) The depth is
    the root of the chord of F between the two samples; along the ray the distance has second
    derivative at most 1/rho, so its chord errs by delta^2 / (8 rho), and the chord of the
    interpolation error by at most (1) again, already counted at the root.  Plus f32 slack."""
    h = 2.0 / (R - 1)
    delta = step * dc_max
    rho = r - (delta + np.sqrt(3.0) * h)
    return h * h / (4.0 * rho) + delta * delta / (8.0 * rho) + 1e-6
