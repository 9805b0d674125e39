"""numpy restatement of the semi-global steps of V10 (include/sfmhip.h, steps 4a, 4b and 5' - 7'):
the u16 cost volume with the plane index innermost, path aggregation along up to eight
directions, and the selection of steps 5 - 7 on the aggregated volume.  Everything the costs
touch is an integer; the f32 steps are those of mvs_ref, op by op.  The census, the box-summed
costs, the scene and its figures come from mvs_ref."""
from functools import lru_cache

import numpy as np

import mvs_ref as m

F32, I32, I64 = np.float32, np.int32, np.int64
INT32_MAX = m.INT32_MAX
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))   # bit i of path_mask: (dv, du)
P_MAX, PEN_MAX = 256, 16383
SMOOTH = (50, 400, 0xFF)   # the scene's p1, p2 and path mask


def check_limits(P, p1, p2, mask):
    if not (1 <= P <= P_MAX and 0 <= p1 <= p2 <= PEN_MAX and 1 <= mask <= 0xFF):
        raise ValueError((P, p1, p2, mask))


def cost_volume(cen, poses, K, refs, srcs, planes, a=2, penalty=24):
    """4a.  -> vol (R,H,W,P) u16; an invalid reference gives an all-zero slice."""
    cen, poses, K = np.asarray(cen), np.asarray(poses, F32), np.asarray(K, F32)
    refs = np.asarray(refs, I32).reshape(-1)
    planes = np.asarray(planes, F32)
    V, H, W = cen.shape
    R, P = len(refs), len(planes)
    srcs = np.asarray(srcs, I32).reshape(R, -1)
    vol = np.zeros((R, H, W, P), np.uint16)
    for i, r in enumerate(refs):
        r = int(r)
        if not (0 <= r < V and m.view_ok(poses[r], K[r])) or H * W == 0:
            continue
        ag, _ = m.cost_volume(cen, poses, K, r, srcs[i], planes, a, penalty)
        assert ag.min() >= 0 and ag.max() <= 37632
        vol[i] = ag.transpose(1, 2, 0)
    return vol


def _step(prev, here, has_q, p1, p2):
    """One step of a path for a set of pixels: prev (N,P) the predecessors' L (any value where
    has_q is False), here (N,P) the pixels' costs.  int64."""
    big = np.iinfo(I64).max // 4
    mq = prev.min(1, keepdims=True)
    down = np.full_like(prev, big)
    down[:, 1:] = prev[:, :-1] + p1          # L(q, k - 1) + p1, only if k > 0
    up = np.full_like(prev, big)
    up[:, :-1] = prev[:, 1:] + p1            # L(q, k + 1) + p1, only if k < P - 1
    add = np.minimum(np.minimum(prev, down), np.minimum(up, mq + p2)) - mq
    return here + np.where(has_q[:, None], add, 0)


def path(vol, d, p1, p2):
    """4b for one direction d = (dv, du): vol (H,W,P) -> L_d (H,W,P) int64."""
    dv, du = d
    H, W, P = vol.shape
    v = vol.astype(I64)
    L = np.empty_like(v)
    if H * W == 0:
        return L
    if dv == 0:     # along a row: all rows at once, column by column
        cols = range(W) if du > 0 else range(W - 1, -1, -1)
        for u in cols:
            q = u - du
            inside = 0 <= q < W
            L[:, u] = _step(L[:, q] if inside else v[:, u], v[:, u], np.full(H, inside), p1, p2)
        return L
    rows = range(H) if dv > 0 else range(H - 1, -1, -1)
    for r in rows:  # row by row; the predecessor of (r, u) is (r - dv, u - du)
        q = r - dv
        if not 0 <= q < H:
            L[r] = v[r]
            continue
        uq = np.arange(W) - du
        has = (uq >= 0) & (uq < W)
        L[r] = _step(L[q][np.clip(uq, 0, W - 1)], v[r], has, p1, p2)
    return L


def sgm_aggregate(vol, p1, p2, mask=0xFF):
    """4b.  vol (R,H,W,P) u16 -> sm (R,H,W,P) u32, the sum of L_d over the directions of mask."""
    vol = np.asarray(vol)
    check_limits(vol.shape[3], p1, p2, mask)
    sm = np.zeros(vol.shape, I64)
    for i in range(vol.shape[0]):
        for b, d in enumerate(DIRECTIONS):
            if mask >> b & 1:
                sm[i] += path(vol[i], d, p1, p2)
    assert sm.max(initial=0) < 2 ** 19
    return sm.astype(np.uint32)


def visible_count(poses, K, r, src_row, planes, H, W):
    """Step 3's nv (P,H,W) u8 of one reference: it needs no image."""
    dx, dy = m.rays(K[r], H, W)
    nv = np.zeros((len(planes), H, W), np.uint8)
    for s, rel in m._sources(poses, K, r, src_row):
        for k in range(len(planes)):
            nv[k] += m.reproject(rel, K[s], dx, dy, F32(planes[k]), H, W)[0]
    return nv


def volume_select(sm, poses, K, refs, srcs, planes, uniq=243, min_views=2, nv_of=None):
    """5' - 7': steps 5 - 7 of mvs_ref.plane_sweep with sm (R,H,W,P) in place of ag; nv_of: per
    reference, the result of visible_count where the caller has it already.
    -> dict of depth f32, k, best, second int32 and nv u8, each (R,H,W)."""
    sm, poses, K = np.asarray(sm), np.asarray(poses, F32), np.asarray(K, F32)
    refs = np.asarray(refs, I32).reshape(-1)
    planes = np.asarray(planes, F32)
    R, H, W, P = sm.shape
    V = len(poses)
    srcs = np.asarray(srcs, I32).reshape(R, -1)
    out = dict(depth=np.zeros((R, H, W), F32), k=np.zeros((R, H, W), I32), best=np.zeros((R, H, W), I32),
               second=np.zeros((R, H, W), I32), nv=np.zeros((R, H, W), np.uint8))
    inv = F32(1) / planes
    for i, r in enumerate(refs):
        r = int(r)
        if not (0 <= r < V and m.view_ok(poses[r], K[r])) or H * W == 0:
            continue
        ag = sm[i].astype(I64).transpose(2, 0, 1)
        nv = visible_count(poses, K, r, srcs[i], planes, H, W) if nv_of is None else nv_of[i]
        ks = ag.argmin(0)
        best = np.take_along_axis(ag, ks[None], 0)[0]
        far = np.abs(np.arange(P)[:, None, None] - ks[None]) >= 2
        second = np.where(far, ag, INT32_MAX).min(0)
        nvk = np.take_along_axis(nv, ks[None], 0)[0]
        inner = (ks > 0) & (ks < P - 1)
        km, kp = np.clip(ks - 1, 0, P - 1), np.clip(ks + 1, 0, P - 1)
        c0 = best.astype(F32)
        cm = np.take_along_axis(ag, km[None], 0)[0].astype(F32)
        cp = np.take_along_axis(ag, kp[None], 0)[0].astype(F32)
        den = (cm - c0) + (cp - c0)
        with np.errstate(all="ignore"):
            off = np.where(inner & (den > 0), (cm - cp) / (F32(2) * den), F32(0)).astype(F32)
            step = np.where(off >= 0, inv[kp] - inv[ks], inv[ks] - inv[km])
            depth = F32(1) / (inv[ks] + off * step)
        ok = inner & (nvk >= min_views) & (256 * best <= uniq * second)
        out["depth"][i] = np.where(ok, depth, F32(0))
        out["k"][i], out["best"][i], out["second"][i], out["nv"][i] = ks, best, second, nvk
    return out


def plane_sweep(cen, poses, K, refs, srcs, planes, a=2, penalty=24, uniq=243, min_views=2, smooth=SMOOTH):
    """plane_sweep(..., smooth=(p1, p2, mask)): 4a, 4b, 5' - 7'."""
    vol = cost_volume(cen, poses, K, refs, srcs, planes, a, penalty)
    sm = sgm_aggregate(vol, smooth[0], smooth[1], smooth[2])
    return volume_select(sm, poses, K, refs, srcs, planes, uniq, min_views)


def mvs_depth_sweep(cen, poses, K, lists, planes, a=2, penalty=24, uniq=243, min_views=2, smooth=SMOOTH):
    """What mvs_depth(..., smooth=...) sweeps: every view against its own list."""
    V, H, W = cen.shape
    out = dict(depth=np.zeros((V, H, W), F32), k=np.zeros((V, H, W), I32), best=np.zeros((V, H, W), I32),
               second=np.zeros((V, H, W), I32), nv=np.zeros((V, H, W), np.uint8))
    for r, nb in enumerate(lists):
        if len(nb) == 0:
            continue
        one = plane_sweep(cen, poses, K, [r], [list(nb)], planes, a, penalty, uniq, min_views, smooth)
        for name in out:
            out[name][r] = one[name][0]
    return out


def weak_grey(grey):
    """The weak-texture variant of an image: uint8(128 + floor((grey - 128) / 32))."""
    return (128 + np.floor_divide(np.asarray(grey).astype(np.int32) - 128, 32)).astype(np.uint8)


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@lru_cache(maxsize=None)
def scene_sweep(weak=False, smooth=SMOOTH):
    """The scene's five views swept with (smooth = (p1, p2, mask)) or without (None) the path
    aggregation, on the committed or the weak-texture images (shared, read-only)."""
    sc, S = m.scene(), m.SCENE
    if not weak and smooth is None:
        return m.scene_sweep()
    cen = m.census(weak_grey(sc["grey"]) if weak else sc["grey"])
    args = (cen, sc["poses"], sc["K"], sc["lists"], sc["planes"], S["a"], S["penalty"], S["uniq"], S["min_views"])
    return _frozen(m.mvs_depth_sweep(*args) if smooth is None else mvs_depth_sweep(*args, smooth))


@lru_cache(maxsize=None)
def scene_filtered(weak=False, smooth=SMOOTH):
    sc, S = m.scene(), m.SCENE
    count, filt = m.depth_consistency(scene_sweep(weak, smooth)["depth"], sc["poses"], sc["K"], np.arange(5),
                                      sc["srcs"], S["eps"], S["min_consistent"])
    count.setflags(write=False)
    filt.setflags(write=False)
    return count, filt


def scene_figures(weak=False, smooth=SMOOTH, view=2):
    return m.scene_figures(scene_sweep(weak, smooth)["depth"][view], scene_filtered(weak, smooth)[1][view], view)


def check_smoothed_figures(f):
    """The conditions of the smoothed scene as committed."""
    assert f["swept_completeness"] >= 0.975, f
    assert f["swept_within_2pc"] >= 0.98, f
    assert f["filtered_completeness"] >= 0.95, f
    assert f["filtered_off_5pc"] <= 0.003, f
