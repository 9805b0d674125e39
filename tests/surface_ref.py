"""Vectorised numpy restatement of the TSDF surface extractor (marching tetrahedra
on the Kuhn 6-tetrahedron split; semantics in include/sfmhip.h, "V6").  A plain
helper module for the surface tests: not a test, not a conftest.

Everything is f32, one IEEE operation per step (numpy never fuses), so vertices
and faces of the HIP extractor are compared bit for bit.
"""
from __future__ import annotations

import itertools

import numpy as np

F32 = np.float32

# edge slot k -> (dx, dy, dz)
SLOT_OFFSETS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)], np.int64)
_SLOT_OF = {tuple(o): k for k, o in enumerate(SLOT_OFFSETS.tolist())}

# tetrahedron t = lexicographic rank of the axis permutation (a, b, c) of (x, y, z);
# corners c0, c0 + e_a, c0 + e_a + e_b, c0 + (1,1,1) as (dx, dy, dz)
TET_CORNERS = np.zeros((6, 4, 3), np.int64)
for _t, (_a, _b, _c) in enumerate(itertools.permutations(range(3))):
    TET_CORNERS[_t, 1, _a] = 1
    TET_CORNERS[_t, 2, _a] = TET_CORNERS[_t, 2, _b] = 1
    TET_CORNERS[_t, 3] = 1


def case_triangles(case: int):
    """Triangles of one tetrahedron case (bit j of `case` = tet corner j inside), before
    the orientation swap: a list of 3-tuples of edges (lo, hi) in tet corner indices."""
    ins = [j for j in range(4) if case >> j & 1]
    out = [j for j in range(4) if not case >> j & 1]
    e = lambda a, b: (min(a, b), max(a, b))   # noqa: E731
    if len(ins) == 1:
        i = ins[0]
        return [(e(i, out[0]), e(i, out[1]), e(i, out[2]))]
    if len(ins) == 3:
        o = out[0]
        return [(e(ins[0], o), e(ins[1], o), e(ins[2], o))]
    if len(ins) == 2:
        (p, q), (r, s) = ins, out
        return [(e(p, r), e(p, s), e(q, s)), (e(p, r), e(q, s), e(q, r))]
    return []


def swap_table() -> np.ndarray:
    """(6, 16) bool: swap the last two vertices of the case's triangles so that
    (v1-v0) x (v2-v0) points towards the outside corners.  Derived by placing the
    vertices of a +-1 field (s = 1/2: edge midpoints) and testing each triangle."""
    tab = np.zeros((6, 16), bool)
    for t in range(6):
        P = TET_CORNERS[t].astype(np.float64)
        for case in range(1, 15):
            ins = [j for j in range(4) if case >> j & 1]
            out = [j for j in range(4) if not case >> j & 1]
            toward = P[out].mean(0) - P[ins].mean(0)
            signs = []
            for tri in case_triangles(case):
                v = [0.5 * (P[a] + P[b]) for a, b in tri]
                signs.append(float(np.dot(np.cross(v[1] - v[0], v[2] - v[0]), toward)))
            assert all(s != 0.0 for s in signs) and len({s > 0 for s in signs}) == 1, (t, case, signs)
            tab[t, case] = signs[0] < 0
    return tab


SWAP = swap_table()


def _shift(a: np.ndarray, axis: int, d: int, fill):
    """b[i] = a[i + d] along `axis`, `fill` where i + d is outside."""
    b = np.full_like(a, fill)
    n = a.shape[axis]
    if n <= abs(d):
        return b
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if d > 0:
        src[axis], dst[axis] = slice(d, n), slice(0, n - d)
    else:
        src[axis], dst[axis] = slice(0, n + d), slice(-d, n)
    b[tuple(dst)] = a[tuple(src)]
    return b


def gradient(T: np.ndarray, obs: np.ndarray, step) -> np.ndarray:
    """(D,H,W,3) f32 gradient (x, y, z components): central difference where both
    neighbours are in the grid and observed, one-sided where one is, else 0."""
    G = np.zeros(T.shape + (3,), F32)
    with np.errstate(all="ignore"):
        for a, axis in enumerate((2, 1, 0)):   # x -> W, y -> H, z -> D
            Tp, Tm = _shift(T, axis, 1, F32(0)), _shift(T, axis, -1, F32(0))
            op, om = _shift(obs, axis, 1, False), _shift(obs, axis, -1, False)
            st = F32(step[a])
            cen = (Tp - Tm) / (F32(2) * st)
            fwd = (Tp - T) / st
            bwd = (T - Tm) / st
            G[..., a] = np.where(op & om, cen, np.where(op, fwd, np.where(om, bwd, F32(0))))
    return G


def extract(T, Wt, bmin, bmax, iso=0.0, min_weight=1.0, z0=0, z1=None, normals=True):
    """-> vertices (V,3) f32, normals (V,3) f32 | None, faces (F,3) int32."""
    T = np.ascontiguousarray(T, F32)
    Wt = np.ascontiguousarray(Wt, F32)
    D, H, W = T.shape
    z1 = D - 1 if z1 is None else int(z1)
    z0 = int(z0)
    if not 0 <= z0 <= z1 <= D - 1:
        raise ValueError("bad z range")
    if not min_weight > 0:
        raise ValueError("min_weight must be > 0")
    empty = (np.zeros((0, 3), F32), np.zeros((0, 3), F32) if normals else None, np.zeros((0, 3), np.int32))
    if D < 2 or H < 2 or W < 2 or z0 == z1:
        return empty
    iso = F32(iso)
    bmin = np.asarray(bmin, F32).reshape(3)
    bmax = np.asarray(bmax, F32).reshape(3)
    step = (bmax - bmin) / np.array([W - 1, H - 1, D - 1], F32)   # x, y, z

    obs = (Wt >= F32(min_weight)) & np.isfinite(T)
    with np.errstate(invalid="ignore"):
        ins = T < iso
    valid = np.ones((D - 1, H - 1, W - 1), bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        valid &= obs[dz:D - 1 + dz, dy:H - 1 + dy, dx:W - 1 + dx]
    valid[:z0] = False
    valid[z1:] = False
    vp = np.pad(valid, 1)   # vp[z+1, y+1, x+1] = valid[z, y, x]; absent cells False

    act = np.zeros((D, H, W, 7), bool)
    for k, (dx, dy, dz) in enumerate(SLOT_OFFSETS.tolist()):
        has = np.zeros((D, H, W), bool)
        for ez, ey, ex in itertools.product(*[((0,) if o else (-1, 0)) for o in (dz, dy, dx)]):
            has |= vp[1 + ez:1 + ez + D, 1 + ey:1 + ey + H, 1 + ex:1 + ex + W]
        cross = np.zeros((D, H, W), bool)
        cross[:D - dz, :H - dy, :W - dx] = ins[:D - dz, :H - dy, :W - dx] != ins[dz:, dy:, dx:]
        act[..., k] = has & cross
    zi, yi, xi, ki = np.nonzero(act)   # C order: (voxel linear id, k)
    V = zi.size
    vidx = np.full((D, H, W, 7), -1, np.int64)
    vidx[zi, yi, xi, ki] = np.arange(V)

    off = SLOT_OFFSETS[ki]
    T0 = T[zi, yi, xi]
    T1 = T[zi + off[:, 2], yi + off[:, 1], xi + off[:, 0]]
    s = (iso - T0) / (T1 - T0)
    verts = np.empty((V, 3), F32)
    for a, idx in enumerate((xi, yi, zi)):
        g = idx.astype(F32) + s * off[:, a].astype(F32)
        verts[:, a] = bmin[a] + g * step[a]

    nrm = None
    if normals:
        G = gradient(T, obs, step)
        g0 = G[zi, yi, xi]
        g1 = G[zi + off[:, 2], yi + off[:, 1], xi + off[:, 0]]
        with np.errstate(all="ignore"):
            n = (F32(1) - s)[:, None] * g0 + s[:, None] * g1
            ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            ok = np.isfinite(ln) & (ln > 0)
            nrm = np.where(ok[:, None], n / ln[:, None], F32(0)).astype(F32)

    cz, cy, cx = np.nonzero(valid)
    cid = (cz * (H - 1) + cy) * (W - 1) + cx
    keys, tris = [], []
    for t in range(6):
        tc = TET_CORNERS[t]
        case = np.zeros(cz.size, np.int64)
        for j in range(4):
            case |= ins[cz + tc[j, 2], cy + tc[j, 1], cx + tc[j, 0]].astype(np.int64) << j
        for c in range(1, 15):
            sel = np.nonzero(case == c)[0]
            if sel.size == 0:
                continue
            for j, tri in enumerate(case_triangles(c)):
                ids = []
                for lo, hi in tri:
                    k = _SLOT_OF[tuple((tc[hi] - tc[lo]).tolist())]
                    ids.append(vidx[cz[sel] + tc[lo, 2], cy[sel] + tc[lo, 1], cx[sel] + tc[lo, 0], k])
                if SWAP[t, c]:
                    ids[1], ids[2] = ids[2], ids[1]
                tris.append(np.stack(ids, 1))
                keys.append(np.stack([cid[sel], np.full(sel.size, t), np.full(sel.size, j)], 1))
    if not tris:
        return verts, nrm, np.zeros((0, 3), np.int32)
    tris = np.concatenate(tris)
    keys = np.concatenate(keys)
    assert tris.min() >= 0
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return verts, nrm, tris[order].astype(np.int32)


# ---- helpers shared by the surface tests ------------------------------------
SPHERE = dict(R=32, r=0.6, centre=(0.03, -0.02, 0.05), mu_vox=3.0)


def sphere_grid(R=32, r=0.6, centre=(0.03, -0.02, 0.05), mu_vox=3.0):
    """Analytic sphere TSDF on [-1,1]^3: T = clip((|p - c| - r) / mu, -1, 1), W = 1."""
    ax = np.linspace(-1.0, 1.0, R)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - r
    mu = mu_vox * 2.0 / (R - 1)
    return np.clip(d / mu, -1.0, 1.0).astype(F32), np.ones((R, R, R), F32)


def sphere_bound(R=32, r=0.6, **_):
    """Largest distance of a vertex from the sphere: linear interpolation over an edge of
    length l <= sqrt(3) h of a distance function whose curvature is <= 1/rho within the
    band (rho = r - sqrt(3) h) errs by at most l^2 / (8 rho); plus f32 slack."""
    h = 2.0 / (R - 1)
    return 3.0 * h * h / (8.0 * (r - np.sqrt(3.0) * h)) + 1e-6


def manifold_report(faces: np.ndarray, n_vertices: int) -> dict:
    """Euler characteristic and directed-edge statistics of a triangle mesh."""
    f = np.asarray(faces, np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code = de[:, 0] * n_vertices + de[:, 1]
    rev = de[:, 1] * n_vertices + de[:, 0]
    uniq, counts = np.unique(code, return_counts=True)
    und = np.unique(np.minimum(code, rev))
    return {"V": int(n_vertices), "F": int(f.shape[0]), "E": int(und.size),
            "euler": int(n_vertices - und.size + f.shape[0]),
            "directed_once": bool((counts == 1).all()),
            "opposite_present": bool(np.isin(rev, uniq).all()),
            "all_referenced": bool(np.unique(f).size == n_vertices)}


def soup(vertices: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """(F,3,3) triangle soup vertices[faces]."""
    return np.asarray(vertices)[np.asarray(faces, np.int64)]
