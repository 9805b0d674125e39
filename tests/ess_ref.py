"""findEssentialMat / recoverPose test scenes, the oracle's trace and its model variants.  CPU only.

The GPU kernels (ransac.hip) and oracle/ransac.py run the same RANSAC on the same cv::RNG samples,
but their five-point solvers differ in the null-space basis and the root finder, so their candidate
models agree only to about 1e-8.  A scene can be a parity scene only if its outcome does not depend
on that: `admissible` runs the oracle as it is, with every candidate model perturbed by a random
matrix of Frobenius norm 1e-8 (three seeds), and with a sample's models visited in descending root
order, and all five runs must agree.  recoverPose has a second freedom, the SVD's choice of
R1 / R2 and of the sign of t, so there a scene is a parity scene only if one candidate wins outright
and no cheirality test of an unmasked point lies within 1e-6 of its boundary.

`FE_SCENES` and `RP_SCENES` are the tables shared by tests/test_ess_scenes_cpu.py (admissibility and
the property each scene is listed for) and tests/test_gpu_verify.py (parity).

Out of scope: scenes with repeated correspondences, and exactly planar or rotation-only geometry.
The 5 x 9 epipolar system's null space then has more than four dimensions; its basis is a
build-defined choice of the SVD, so the oracle and the kernel may differ without either being wrong.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import geometry as og
from oracle import ransac as orc

# ransac.hip: points per scoring block of the chunk kernel (256 threads x kPB), of the monolithic
# kernel (512 threads x kPB) and of recover_pose_kernel (kPThreads)
CHUNK_BLOCK = 1024
MONO_BLOCK = 2048
POSE_BLOCK = 768

# [fx, fy, cx, cy]; every entry is exact in float
CAM_OFF = (1480.0, 1850.0, 963.5, -531.25)      # fy = 1.25 fx, cx = 0.65 fx, cy = -0.29 fy
CAM_WIDE = (300.0, 330.0, 40.5, -25.25)
CAM_TELE = (20000.0, 20500.0, 512.5, 384.25)
CAM_DEEP = (900.0, 1150.0, 640.5, 355.25)
CAM_B = (1210.5, 1190.75, -640.25, 355.5)


def cam_matrix(cam) -> np.ndarray:
    fx, fy, cx, cy = cam
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def scene(n, seed, cam=CAM_OFF, rvec=(0.05, -0.2, 0.03), t=(1.0, 0.1, 0.2), zlo=3.0, zhi=12.0, half=0.4,
          outlier=0.1, noise=0.5):
    """Two views of n points -> dict(pts0, pts1 (n,2) f32 pixels, K, R, t, inlier (n,) bool).
    Points lie in view 0 at normalised coordinates uniform in [-half, half]^2 and at log-uniform
    depths in [zlo, zhi] baselines (|t|); a point is kept if view 1 sees it in front and inside
    [-half, half]^2 too.  Outliers keep their view-0 pixel and get a uniform one in view 1.
    The draws are in a fixed order."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = cam
    R = og.rodrigues(np.asarray(rvec, np.float64))
    t = np.asarray(t, np.float64)
    base = float(np.linalg.norm(t))
    x0 = np.zeros((0, 2))
    x1 = np.zeros((0, 2))
    for _ in range(64):
        if len(x0) >= n:
            break
        xy = rng.uniform(-half, half, (2 * n, 2))
        z = np.exp(rng.uniform(math.log(zlo), math.log(zhi), 2 * n)) * base
        X = np.column_stack([xy * z[:, None], z])
        Y = X @ R.T + t
        ok = Y[:, 2] > 0.05 * base
        yx = Y[:, :2] / np.where(ok, Y[:, 2], 1.0)[:, None]
        ok &= np.abs(yx).max(1) <= half
        x0 = np.concatenate([x0, xy[ok]])
        x1 = np.concatenate([x1, yx[ok]])
    if len(x0) < n:
        raise ValueError("view 1 sees too few of the points: the pose does not fit the field of view")
    x0, x1 = x0[:n], x1[:n]
    f, c = np.array([fx, fy]), np.array([cx, cy])
    p0 = x0 * f + c + rng.normal(0, noise, (n, 2))
    p1 = x1 * f + c + rng.normal(0, noise, (n, 2))
    bad = rng.random(n) < outlier
    p1[bad] = rng.uniform(-half, half, (int(bad.sum()), 2)) * f + c
    return dict(pts0=p0.astype(np.float32), pts1=p1.astype(np.float32), K=cam_matrix(cam), R=R, t=t, inlier=~bad)


# ---------------------------------------------------------------------------------------------
# the oracle's trace, its model variants and its wrong-camera forms

VARIANTS = ("plain", "perturbed-1", "perturbed-2", "perturbed-3", "descending")
FAULTS = ("no-principal-point", "swapped-focals", "threshold-over-fx")
PERTURB = 1e-8


def _models(variant):
    """five_point as the named variant sees it: q1, q2 -> list of E."""
    if variant == "plain":
        return orc.five_point
    if variant == "descending":
        return lambda q1, q2: orc.five_point(q1, q2)[::-1]
    rng = np.random.default_rng(int(variant.rsplit("-", 1)[1]))

    def perturbed(q1, q2):
        out = []
        for E in orc.five_point(q1, q2):
            D = rng.normal(size=(3, 3))
            E = E + PERTURB * D / np.linalg.norm(D)
            out.append(E / np.linalg.norm(E))
        return out
    return perturbed


def oracle_trace(sc, prob=0.999, threshold=1.0, max_iters=1000, variant="plain", fault=None):
    """oracle.ransac.find_essential_mat's loop on a scene, with a recording kernel, score and
    update_num_iters around the oracle's own ransac().
    -> dict(E (3,3) or (3k,3) or None, mask (n,1) u8 or None, iters,
            adoptions [(iteration, model index within the sample, inlier count)],
            quotients [num / denom of update_num_iters at each adoption, None where it is not rounded]).
    `fault` gives the oracle a wrong camera: the principal point dropped, fx and fy swapped in the
    normalisation, or the threshold divided by fx instead of (fx + fy) / 2."""
    K = np.asarray(sc["K"], np.float64)
    Kn = K.copy()
    if fault == "no-principal-point":
        Kn[0, 2] = Kn[1, 2] = 0.0
    elif fault == "swapped-focals":
        Kn[0, 0], Kn[1, 1] = K[1, 1], K[0, 0]
    elif fault is not None and fault != "threshold-over-fx":
        raise ValueError(fault)
    q1, q2 = orc.normalise(sc["pts0"], Kn), orc.normalise(sc["pts1"], Kn)
    thresh = threshold / (K[0, 0] if fault == "threshold-over-fx" else (K[0, 0] + K[1, 1]) / 2)
    tf = np.float32(thresh * thresh)
    models = _models(variant)
    state = dict(it=-1, model=-1, good=0)
    adoptions, quotients = [], []

    def kernel(idx):
        state["it"] += 1
        state["model"] = -1
        return models(q1[idx], q2[idx])

    def score(M):
        state["model"] += 1
        mask = orc.sampson_error(M, q1, q2) <= tf
        state["good"] = int(mask.sum())
        return mask

    real_update = orc.update_num_iters

    def update(p, ep, m, niters):
        adoptions.append((state["it"], state["model"], state["good"]))
        num = max(1.0 - min(max(p, 0.0), 1.0), orc.DBL_MIN)
        denom = 1.0 - math.pow(1.0 - min(max(ep, 0.0), 1.0), m)
        q = None
        if denom >= orc.DBL_MIN:
            num, denom = math.log(num), math.log(denom)
            if not (denom >= 0 or -num >= niters * (-denom)):
                q = num / denom
        quotients.append(q)
        return real_update(p, ep, m, niters)

    orc.update_num_iters = update
    try:
        E, mask, it = orc.ransac(len(q1), 5, kernel, score, thresh, prob, max_iters)
    finally:
        orc.update_num_iters = real_update
    if E is not None:
        E = np.vstack(E) if isinstance(E, list) else E
        mask = mask.astype(np.uint8).reshape(-1, 1)
    return dict(E=E, mask=mask, iters=it, adoptions=adoptions, quotients=quotients)


def half_integer_margin(tr):
    """The smallest distance of a rounded num / denom from a half-integer (inf if none is rounded)."""
    qs = [q for q in tr["quotients"] if q is not None]
    return min((abs(q - math.floor(q) - 0.5) for q in qs), default=math.inf)


def per_iteration(adoptions):
    """{iteration: the inlier count it ends with} of an adoption list.  Within one sample the
    descending-order variant meets the models the other way round, so it adopts other intermediate
    models on its way to the sample's best one; niters depends only on the last of them."""
    return {a[0]: a[2] for a in adoptions}


def compare_variants(sc, params):
    """The oracle and its four variants on one scene -> (admissible, traces by variant)."""
    out = {v: oracle_trace(sc, variant=v, **params) for v in VARIANTS}
    t0 = out["plain"]
    same = half_integer_margin(t0) > 1e-6
    for v in VARIANTS[1:]:
        tr = out[v]
        same &= (tr["E"] is None) == (t0["E"] is None) and tr["iters"] == t0["iters"]
        if v == "descending":
            same &= per_iteration(tr["adoptions"]) == per_iteration(t0["adoptions"])
        else:
            same &= tr["adoptions"] == t0["adoptions"]
        if tr["mask"] is not None and t0["mask"] is not None:
            same &= np.array_equal(tr["mask"], t0["mask"])
    return bool(same), out


def admissible(sc, params):
    """True iff the oracle and its four variants agree on whether a model exists, iters, the adoption
    iterations and counts (and, but for the descending-order variant, the model index within the
    sample) and the final mask, and no rounded num / denom lies within 1e-6 of a half-integer."""
    return compare_variants(sc, params)[0]


# ---------------------------------------------------------------------------------------------
# recoverPose

def true_essential(sc, feed="E"):
    """[t]x R of the scene's pose at unit Frobenius norm; "-E" negates it, "swap" is the essential
    matrix of the swapped views (E^T), to be used with pts1, pts0."""
    t = sc["t"]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])
    E = tx @ sc["R"]
    E = E / np.linalg.norm(E)
    return {"E": E, "-E": -E, "swap": E.T.copy()}[feed]


def _rel(v, b):
    return np.abs(v - b) / np.maximum(np.maximum(np.abs(v), abs(b)), 1.0)


def recover_pose_detail(E, pts0, pts1, K, dist=50.0, mask=None):
    """oracle.ransac.recover_pose's four candidates one by one.
    -> dict(counts [4], k (the oracle's winner, first of the largest counts), cands [(R, t)] x 4,
            masks (4, n) bool, margins (4, n, 5)).
    margins: for the unit DLT vector Q of a point under a candidate, |Q[2] Q[3]| and, with
    rel(v, b) = |v - b| / max(|v|, |b|, 1), rel(Z, 0), rel(Z, dist), rel(z2, 0), rel(z2, dist)."""
    K = np.asarray(K, np.float64)
    q1, q2 = orc.normalise(pts0, K), orc.normalise(pts1, K)
    R1, R2, t = orc.decompose_essential_mat(E)
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    keep = np.ones(len(q1), bool) if mask is None else np.asarray(mask).ravel() > 0
    masks, margins = [], []
    for R, tt in cands:
        P = np.hstack([R, tt])
        Q = og.triangulate_points(np.eye(3, 4), P, q1.T, q2.T)
        m = Q[2] * Q[3] > 0
        Qh = Q / Q[3]
        z2 = (P @ Qh)[2]
        m &= (Qh[2] < dist) & (z2 > 0) & (z2 < dist) & keep
        masks.append(m)
        margins.append(np.stack([np.abs(Q[2] * Q[3]), _rel(Qh[2], 0.0), _rel(Qh[2], dist), _rel(z2, 0.0),
                                 _rel(z2, dist)], 1))
    counts = [int(m.sum()) for m in masks]
    return dict(counts=counts, k=int(np.argmax(counts)), cands=cands, masks=np.array(masks),
                margins=np.array(margins), keep=keep)


def pose_admissible(d):
    """One candidate wins outright, and no tested quantity of an unmasked point lies within 1e-6
    relative of its boundary."""
    c = d["counts"]
    strict = all(c[d["k"]] > c[o] for o in range(4) if o != d["k"])
    return bool(strict and d["margins"][:, d["keep"]].min(initial=np.inf) > 1e-6)


# ---------------------------------------------------------------------------------------------
# the findEssentialMat table: (name, scene kwargs, solver kwargs, property)
#   iters / inliers / adopted (the iterations that adopt a model): exact, read from the oracle's trace;
#   maxq_min / maxq_max: bounds on the largest |normalised coordinate|; faults: the wrong cameras
#   that the scene must tell from the right one
# Replaced seeds.  Off-centre: seed 1 -> 18, the first at which all five (prob, threshold, max_iters)
# forms tell all three wrong cameras apart; with seed 1 the forms prob = 0 (nine inliers after one
# sample) and (3.0, 0.9999) gave the same outcome with the threshold divided by fx.  n = 6: seed 6
# without outliers stops after one sample, and with outliers seeds 16..46 end with the sample's own
# five inliers, which no wrong camera changes -> 56.  n = 8: seed 8 likewise stops after one sample,
# seed 18 is not admissible (a perturbed variant adopts another model of the tying sample) -> 28.

_OFF = dict(n=300, seed=18, outlier=0.3)
_WIDE = dict(n=1500, seed=2, cam=CAM_WIDE, half=5.0, rvec=(0.1, -0.3, 0.05), t=(1.0, -0.2, 0.3), zlo=2.0, zhi=20.0)
_TELE = dict(n=300, seed=3, cam=CAM_TELE, half=0.05, rvec=(0.001, -0.012, 0.004), t=(1.0, 0.1, 0.2), zlo=60.0,
             zhi=200.0, outlier=0.2)
_FWD = dict(n=400, seed=4, rvec=(0.02, 0.03, -0.05), t=(0.03, -0.02, 1.0), zlo=3.0, zhi=30.0, outlier=0.2)
_ROLL = dict(n=400, seed=5, cam=CAM_B, rvec=(0.0, 0.0, 3.0), outlier=0.2)

FE_SCENES = [
    ("off-centre", _OFF, {}, dict(iters=139, inliers=177, adopted=[0, 1, 6, 13, 14, 51, 137, 138], faults=FAULTS)),
    ("off-centre-tight", _OFF, dict(threshold=0.4, prob=0.99), dict(iters=530, inliers=116, faults=FAULTS)),
    ("off-centre-loose", _OFF, dict(threshold=3.0, prob=0.9999), dict(iters=56, inliers=206, faults=FAULTS)),
    ("off-centre-prob-0", _OFF, dict(prob=0.0, max_iters=60), dict(iters=1, inliers=8, faults=FAULTS)),
    ("off-centre-prob-1", _OFF, dict(prob=1.0, max_iters=60), dict(iters=60, inliers=151, faults=FAULTS)),
    ("wide-angle", _WIDE, {}, dict(iters=37, inliers=1126, maxq_min=4.0)),
    ("telephoto", _TELE, {}, dict(iters=58, inliers=194, maxq_max=0.05)),
    ("forward-motion", _FWD, {}, dict(iters=47, inliers=273)),
    ("roll-3-rad", _ROLL, {}, dict(iters=40, inliers=277)),
    ("n-6", dict(n=6, seed=56, outlier=0.25), {}, dict(iters=9, inliers=6, faults=FAULTS[:2])),
    ("n-7", dict(n=7, seed=7, outlier=0.0), {}, dict(iters=4, inliers=7, faults=FAULTS[:2])),
    ("n-8", dict(n=8, seed=28, outlier=0.25), {}, dict(iters=25, inliers=6, faults=FAULTS[:2])),
    ("n-1023", dict(n=1023, seed=9), {}, dict(iters=15, inliers=839)),
    ("n-1024", dict(n=1024, seed=10), {}, dict(iters=23, inliers=784)),
    ("n-1025", dict(n=1025, seed=11), {}, dict(iters=16, inliers=835)),
    ("n-2049", dict(n=2049, seed=12, cam=CAM_B), {}, dict(iters=34, inliers=1458)),
]
FE_NAMES = [s[0] for s in FE_SCENES]
_FE = {s[0]: s for s in FE_SCENES}
FE_DEFAULT = [s[0] for s in FE_SCENES if not s[2]]      # the scenes at (0.999, 1.0, 1000): one ragged batch


@functools.lru_cache(maxsize=None)
def fe_scene(name):
    """The named scene's data (shared, read-only)."""
    sc = scene(**_FE[name][1])
    for a in sc.values():
        a.setflags(write=False)
    return sc


def fe_params(name):
    return dict(_FE[name][2])


@functools.lru_cache(maxsize=None)
def fe_trace(name):
    """The plain oracle's trace of the named scene; computed once."""
    return oracle_trace(fe_scene(name), **fe_params(name))


@functools.lru_cache(maxsize=None)
def fe_variants(name):
    """compare_variants on the named scene; computed once."""
    return compare_variants(fe_scene(name), fe_params(name))


def max_normalised(sc):
    return float(np.abs(np.concatenate([orc.normalise(sc["pts0"], sc["K"]), orc.normalise(sc["pts1"], sc["K"])])).max())


# ---------------------------------------------------------------------------------------------
# the recoverPose table: (name, scene kwargs, dict(dist, feed), property)
#   k: the candidate the oracle's decomposition selects, 0..3 = (R1,t), (R2,t), (R1,-t), (R2,-t)
# Depths of 3 to 300 baselines in a field of +-0.9, so that distanceThresh binds at 50, 20 and 8.
# Every k is reached by the choice of pose (pose C is pose A seen from the other view); one scene
# feeds -E, which the oracle decomposes into the same candidates.  Each scene is run without an input
# mask and with `rp_mask`, and no seed had to be replaced.

_DEEP = dict(cam=CAM_DEEP, zlo=3.0, zhi=300.0, half=0.9, outlier=0.05)
_POSE_A = dict(rvec=(0.02, -0.05, 0.01), t=(1.0, 0.1, 0.05))
_POSE_B = dict(rvec=(0.0, 0.4, 0.0), t=(0.1, -0.1, -1.0))
_POSE_C = dict(rvec=(-0.02, 0.05, -0.01), t=(-1.0, -0.1, -0.05))
_POSE_D = dict(rvec=(0.1, 0.2, -0.3), t=(-1.0, 0.2, 0.1))
_POSES = dict(A=(_POSE_A, 1, 40), B=(_POSE_B, 3, 41), C=(_POSE_C, 2, 44), D=(_POSE_D, 0, 42))

RP_SCENES = [(f"deep-{p}-d{d}", dict(n=300, seed=seed, **pose, **_DEEP), dict(dist=float(d), feed="E"), dict(k=k))
             for p, (pose, k, seed) in _POSES.items() for d in (50, 20, 8)] + [
    ("n-767", dict(n=767, seed=50, **_POSE_A, **_DEEP), dict(dist=50.0, feed="E"), dict(k=1)),
    ("n-768", dict(n=768, seed=51, **_POSE_B, **_DEEP), dict(dist=20.0, feed="E"), dict(k=3)),
    ("n-769", dict(n=769, seed=52, **_POSE_C, **_DEEP), dict(dist=8.0, feed="E"), dict(k=2)),
    ("n-1537", dict(n=1537, seed=53, **_POSE_D, **_DEEP), dict(dist=50.0, feed="-E"), dict(k=0)),
]
RP_NAMES = [s[0] for s in RP_SCENES]
_RP = {s[0]: s for s in RP_SCENES}
NO_GATE = 1e300


@functools.lru_cache(maxsize=None)
def rp_scene(name):
    """-> (E, pts0, pts1, K, dist, input mask (n,) u8 keeping about 70 % of the points, scene)."""
    _, kw, how, _ = _RP[name]
    sc = scene(**kw)
    E = true_essential(sc, how["feed"])
    mask = (np.random.default_rng(kw["seed"]).random(kw["n"]) < 0.7).astype(np.uint8)
    for a in (E, mask) + tuple(sc.values()):
        a.setflags(write=False)
    return E, sc["pts0"], sc["pts1"], sc["K"], how["dist"], mask, sc


@functools.lru_cache(maxsize=None)
def rp_detail(name, masked=False, gate=True):
    """recover_pose_detail of the named scene: with or without its input mask, at its distanceThresh
    or with no gate; computed once."""
    E, a, b, K, dist, mask, _ = rp_scene(name)
    return recover_pose_detail(E, a, b, K, dist if gate else NO_GATE, mask if masked else None)
