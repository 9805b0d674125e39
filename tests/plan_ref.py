"""numpy restatement of V13 (include/sfmhip.h) and of plan.py: observation depths, view-pair
counts, segmented order statistics, and the plan built from them (source views, depth ranges,
plane counts, scene box).  Op for op: every f64 step is one numpy operation in the order of the
header text, every count an integer.  Also holds the sparse fixture cut from the MVS scene."""
import math
from functools import lru_cache

import numpy as np

import mvs_ref

F32, F64, I64 = np.float32, np.float64, np.int64
QNAN = np.array([0x7FC00000], np.uint32).view(F32)[0]


# ---- the three kernels ------------------------------------------------------------------------
def camera_centres(poses):
    """(V,3,4) -> (V,3) f64: c_i = -((R[0,i] t0 + R[1,i] t1) + R[2,i] t2)."""
    P = np.asarray(poses, F64).reshape(-1, 3, 4)
    R, t = P[:, :, :3], P[:, :, 3]
    return -((R[:, 0, :] * t[:, 0:1] + R[:, 1, :] * t[:, 1:2]) + R[:, 2, :] * t[:, 2:3])


def obs_depth(poses, X, obs_cam, obs_pt):
    """z (M,) f32: f32(((P20 x0 + P21 x1) + P22 x2) + P23), +inf where that is not finite and > 0."""
    P = np.asarray(poses, F64).reshape(-1, 3, 4)[np.asarray(obs_cam, I64)]
    x = np.asarray(X, F64).reshape(-1, 3)[np.asarray(obs_pt, I64)]
    with np.errstate(all="ignore"):
        d = ((P[:, 2, 0] * x[:, 0] + P[:, 2, 1] * x[:, 1]) + P[:, 2, 2] * x[:, 2]) + P[:, 2, 3]
        z = d.astype(F32)
        return np.where((z > 0) & (z < np.inf), z, F32(np.inf)).astype(F32)


def sorted_unique_obs(obs_cam, obs_pt, V, N):
    """The caller's list without repeats, sorted by (point, camera): cam, pt (int64), pt_off (N+1,)."""
    key = np.unique(np.asarray(obs_pt, I64).ravel() * max(int(V), 1) + np.asarray(obs_cam, I64).ravel())
    pt, cam = key // max(int(V), 1), key % max(int(V), 1)
    pt_off = np.zeros(N + 1, I64)
    np.cumsum(np.bincount(pt, minlength=N)[:N], out=pt_off[1:])
    return cam, pt, pt_off


def angle_thresholds(min_angle, max_angle):
    """degrees -> c2_lo = cos^2(max), c2_hi = cos^2(min), squared in f64."""
    lo, hi = math.cos(math.radians(float(max_angle))), math.cos(math.radians(float(min_angle)))
    return lo * lo, hi * hi


def pair_good(ca, cb, x, c2_lo, c2_hi):
    """The sqrt-free angle test for rows of centres ca, cb and points x (each (n,3) f64)."""
    with np.errstate(all="ignore"):
        ra, rb = ca - x, cb - x
        d = (ra[:, 0] * rb[:, 0] + ra[:, 1] * rb[:, 1]) + ra[:, 2] * rb[:, 2]
        n = ((ra[:, 0] * ra[:, 0] + ra[:, 1] * ra[:, 1]) + ra[:, 2] * ra[:, 2]) * \
            ((rb[:, 0] * rb[:, 0] + rb[:, 1] * rb[:, 1]) + rb[:, 2] * rb[:, 2])
        return (d > 0) & (n < np.inf) & (d * d >= c2_lo * n) & (d * d <= c2_hi * n)


def view_pair_counts(poses, X, obs_cam, obs_pt, min_angle=1.0, max_angle=45.0):
    """shared, good (V,V) int32: tracks grouped by length, all pairs of positions (i < j) of a length at once."""
    poses = np.asarray(poses, F64).reshape(-1, 3, 4)
    X = np.asarray(X, F64).reshape(-1, 3)
    V, N = len(poses), len(X)
    shared, good = np.zeros(V * V, I64), np.zeros(V * V, I64)
    if V == 0 or N == 0 or len(np.asarray(obs_cam).ravel()) == 0:
        return shared.reshape(V, V).astype(np.int32), good.reshape(V, V).astype(np.int32)
    c = camera_centres(poses)
    c2_lo, c2_hi = angle_thresholds(min_angle, max_angle)
    cam, _, pt_off = sorted_unique_obs(obs_cam, obs_pt, V, N)
    length = np.diff(pt_off)
    for L in np.unique(length[length >= 2]):
        tr = np.nonzero(length == L)[0]
        cams = cam[pt_off[tr][:, None] + np.arange(L)[None, :]]          # (n, L), ascending in a row
        for i in range(L - 1):                                           # position i against every later one
            a, b = np.repeat(cams[:, i], L - 1 - i), cams[:, i + 1:].ravel()
            g = pair_good(c[a], c[b], np.repeat(X[tr], L - 1 - i, axis=0), c2_lo, c2_hi)
            shared += np.bincount(a * V + b, minlength=V * V)
            good += np.bincount((a * V + b)[g], minlength=V * V)
    shared, good = shared.reshape(V, V), good.reshape(V, V)
    return (shared + shared.T).astype(np.int32), (good + good.T).astype(np.int32)


def radix_key(values):
    """f32 -> uint32 keys whose unsigned order is the total order of the select."""
    bits = np.ascontiguousarray(np.asarray(values, F32)).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def key_value(key):
    key = np.asarray(key, np.uint32)
    return np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(F32)


def segmented_select(values, seg_off, ranks):
    """out (S,R) f32: four 8-bit most-significant-digit passes per rank, as the kernel makes them."""
    values = np.asarray(values, F32).ravel()
    seg_off = np.asarray(seg_off, I64).ravel()
    ranks = np.asarray(ranks, I64)
    S, R = ranks.shape
    out = np.empty((S, R), F32)
    for s in range(S):
        keys = radix_key(values[seg_off[s]:seg_off[s + 1]])
        for r in range(R):
            left = int(ranks[s, r])
            if not 0 <= left < len(keys):
                out[s, r] = QNAN
                continue
            cand, prefix = keys, 0
            for shift in (24, 16, 8, 0):
                hist = np.bincount((cand >> np.uint32(shift)) & np.uint32(255), minlength=256)
                d = 0
                while d < 255 and left >= hist[d]:
                    left -= int(hist[d])
                    d += 1
                cand = cand[((cand >> np.uint32(shift)) & np.uint32(255)) == d]
                prefix |= d << shift
            out[s, r] = key_value(np.array([prefix], np.uint32))[0]
    return out


# ---- the plan ---------------------------------------------------------------------------------
def quantile_ranks(n, q):
    """The two ranks of the rule: floor(q (n - 1)) and ceil((1 - q)(n - 1)), in f64."""
    return int(math.floor(q * (n - 1))), int(math.ceil((1.0 - q) * (n - 1)))


def select_sources(shared, good, max_sources=4, min_good=16):
    shared, good = np.asarray(shared, I64), np.asarray(good, I64)
    V = len(good)
    out = []
    for a in range(V):
        cand = [b for b in range(V) if b != a and good[a, b] >= min_good]
        cand.sort(key=lambda b: (-good[a, b], -shared[a, b], b))
        out.append([int(b) for b in cand[:max_sources]])
    return out


def view_depth_ranges(poses, X, obs_cam, obs_pt, q=0.02, margin=0.1, min_points=8):
    """near, far (V,) f32 and count (V,) int64 from the sorted valid depths of every view."""
    V = len(np.asarray(poses).reshape(-1, 3, 4))
    obs_cam = np.asarray(obs_cam, I64).ravel()
    z = obs_depth(poses, X, obs_cam, obs_pt)
    near, far, count = np.zeros(V, F32), np.zeros(V, F32), np.zeros(V, I64)
    for v in range(V):
        zv = np.sort(z[obs_cam == v])
        zv = zv[zv < np.inf]
        count[v] = n = len(zv)
        if n >= max(int(min_points), 1):
            r0, r1 = quantile_ranks(n, q)
            near[v] = F32(F64(zv[r0]) * (1.0 - margin))
            far[v] = F32(F64(zv[r1]) * (1.0 + margin))
    return near, far, count


def scene_bounds(X, obs_pt, q=0.01, pad=0.1, min_obs=2):
    """bmin, bmax (3,) f32 from per-axis order statistics of the f32-rounded coordinates."""
    X = np.asarray(X, F64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        Xf = X.astype(F32)
    n_obs = np.bincount(np.asarray(obs_pt, I64).ravel(), minlength=len(X))[:len(X)]
    keep = np.isfinite(Xf).all(1) & (n_obs >= min_obs)
    bmin, bmax = np.zeros(3, F32), np.zeros(3, F32)
    n = int(keep.sum())
    if n == 0:
        return bmin, bmax
    r0, r1 = quantile_ranks(n, q)
    for ax in range(3):
        v = np.sort(Xf[keep, ax])
        lo, hi = F64(v[r0]), F64(v[r1])
        ext = hi - lo
        bmin[ax], bmax[ax] = F32(lo - pad * ext), F32(hi + pad * ext)
    return bmin, bmax


def plane_count(fx, b, near, far, step_px=1.0, p_min=8, p_max=256):
    """P = clip(ceil(((fx b) (1/near - 1/far)) / step_px) + 1, p_min, p_max), f64."""
    fx, b, near, far = F64(fx), F64(b), F64(near), F64(far)
    disp = ((fx * b) * (1.0 / near - 1.0 / far)) / F64(step_px)
    return int(min(max(math.ceil(disp) + 1, int(p_min)), int(p_max)))


def plan_dense(poses, K, X, obs_cam, obs_pt, step_px=1.0, p_min=8, p_max=256, min_angle=1.0, max_angle=45.0,
               max_sources=4, min_good=16, q=0.02, margin=0.1, min_points=8, bounds_q=0.01, pad=0.1, min_obs=2):
    poses = np.asarray(poses, F64).reshape(-1, 3, 4)
    K = np.asarray(K, F64).reshape(-1, 4)
    shared, good = view_pair_counts(poses, X, obs_cam, obs_pt, min_angle, max_angle)
    nb = select_sources(shared, good, max_sources, min_good)
    near, far, count = view_depth_ranges(poses, X, obs_cam, obs_pt, q, margin, min_points)
    bmin, bmax = scene_bounds(X, obs_pt, bounds_q, pad, min_obs)
    c = camera_centres(poses)
    planes = []
    for v in range(len(poses)):
        if not nb[v] or not (near[v] > 0 and far[v] > near[v]):
            nb[v] = []
            planes.append(np.zeros(0, F32))
            continue
        d = c[nb[v]] - c[v]
        b = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max()
        P = plane_count(K[v, 0], b, near[v], far[v], step_px, p_min, p_max)
        planes.append(mvs_ref.inverse_depth_planes(F64(near[v]), F64(far[v]), P))
    return dict(neighbours=nb, near=near, far=far, count=count, planes=planes, bmin=bmin, bmax=bmax, shared=shared,
                good=good)


# ---- the sparse fixture -----------------------------------------------------------------------
@lru_cache(maxsize=None)
def fixture():
    """Sparse points sampled from the MVS scene: from every view the pixels (v, u), v = 8, 24, ..,
    184, u = 8, 24, .., 248 with a depth, back-projected in f64; a view observes a point iff the
    point has a positive depth there and projects (nearest pixel) inside the image onto a true
    depth within 1 % of its own.  poses f64 (V,3,4), K f64 (V,4), X (N,3), obs_cam, obs_pt."""
    sc = mvs_ref.scene()
    poses, K, depth = sc["poses"].astype(F64), sc["K"].astype(F64), sc["depth"].astype(F64)
    V, H, W = depth.shape
    pts = []
    for i in range(V):
        vv, uu = np.meshgrid(np.arange(8, H, 16), np.arange(8, W, 16), indexing="ij")
        vv, uu = vv.ravel(), uu.ravel()
        d = depth[i, vv, uu]
        ok = d > 0
        vv, uu, d = vv[ok], uu[ok], d[ok]
        Xc = np.stack([(uu - K[i, 2]) / K[i, 0] * d, (vv - K[i, 3]) / K[i, 1] * d, d], 1)
        pts.append((Xc - poses[i, :, 3]) @ poses[i, :, :3])
    X = np.concatenate(pts)
    oc, op = [], []
    for i in range(V):
        Xc = X @ poses[i, :, :3].T + poses[i, :, 3]
        z = Xc[:, 2]
        front = z > 0
        zs = np.where(front, z, 1.0)
        pu = np.floor(K[i, 0] * Xc[:, 0] / zs + K[i, 2] + 0.5).astype(I64)
        pv = np.floor(K[i, 1] * Xc[:, 1] / zs + K[i, 3] + 0.5).astype(I64)
        inside = front & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
        ds = depth[i, np.clip(pv, 0, H - 1), np.clip(pu, 0, W - 1)]
        seen = inside & (ds > 0) & (np.abs(ds - z) <= 0.01 * z)
        idx = np.nonzero(seen)[0]
        oc.append(np.full(len(idx), i, I64))
        op.append(idx)
    out = dict(poses=poses, K=K, X=X, obs_cam=np.concatenate(oc), obs_pt=np.concatenate(op))
    for v in out.values():
        v.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def fixture_plan():
    """The restatement's plan of the fixture: all four other views as sources, defaults otherwise."""
    fx = fixture()
    return plan_dense(fx["poses"], fx["K"], fx["X"], fx["obs_cam"], fx["obs_pt"], max_sources=4)
