"""Two-view geometry for the choice of the first image pair.

The reference leaves the first pair to the user (its README: the first pair "greatly affects the
result"; "choose the first image pair manually"), and an essential matrix alone cannot tell a good
one: a rotation-only or planar pair fits one with many inliers although its baseline is meaningless.
The customary test compares the support of a homography with the essential matrix's on the same
correspondences, then asks for parallax and image coverage:

* :func:`classify_pairs` — per pair the essential inliers, the cheirality survivors, the homography
  inliers, the median parallax angle, the image coverage and a label.  Four batched launches over
  all pairs (verify.find_essential_batched, recover_pose_batched, find_homography_batched,
  pair_stats_batched); no CPU path.
* :func:`select_initial_pair` — classifies every candidate pair of a connection graph and returns
  the GENERAL pair with the largest ``n_good * coverage``; :func:`tracks.with_initial_pair` then
  puts it first for :func:`tracks.bfs_tracks` and ``incremental_sfm``.

The thresholds are arguments with the customary defaults of such a test; they are not tuned.
"""
from __future__ import annotations

import numpy as np

from . import verify

DEGENERATE, PLANAR_OR_ROTATION, LOW_PARALLAX, GENERAL = "DEGENERATE", "PLANAR_OR_ROTATION", "LOW_PARALLAX", "GENERAL"
LABELS = (DEGENERATE, PLANAR_OR_ROTATION, LOW_PARALLAX, GENERAL)


def label_pairs(has_model, n_e, n_h, median_angle_deg, max_h_ratio: float = 0.8, min_angle_deg: float = 4.0,
                min_inliers: int = 30):
    """The label logic on given counts (host arrays, no GPU): -> (h_ratio (P,) f64, labels list).
    DEGENERATE: no essential model or n_e < min_inliers; PLANAR_OR_ROTATION: h_ratio = n_h /
    max(n_e, 1) > max_h_ratio; LOW_PARALLAX: median angle < min_angle_deg; else GENERAL — the first
    that applies."""
    has_model = np.asarray(has_model).astype(bool).ravel()
    n_e = np.asarray(n_e, np.int64).ravel()
    n_h = np.asarray(n_h, np.int64).ravel()
    ang = np.asarray(median_angle_deg, np.float64).ravel()
    h_ratio = n_h / np.maximum(n_e, 1)
    labels = []
    for p in range(len(n_e)):
        if not has_model[p] or n_e[p] < min_inliers:
            labels.append(DEGENERATE)
        elif h_ratio[p] > max_h_ratio:
            labels.append(PLANAR_OR_ROTATION)
        elif ang[p] < min_angle_deg:
            labels.append(LOW_PARALLAX)
        else:
            labels.append(GENERAL)
    return h_ratio, labels


def _popcount64(words: np.ndarray) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(words.shape + (8,)), axis=-1).sum(-1)


def classify_pairs(pts0_list, pts1_list, K, size, prob: float = 0.999, threshold: float = 1.0,
                   h_threshold: float = 3.0, max_h_ratio: float = 0.8, min_angle_deg: float = 4.0,
                   min_inliers: int = 30) -> dict:
    """Lists of (n_p, 2) pixel correspondences, K (3,3), size = (width, height) of the images.
    Returns host arrays over the pairs: n_e (essential inliers), n_good (those that also pass
    recoverPose's cheirality), n_h (homography inliers), h_ratio, median_angle_deg (NaN where no
    correspondence is selected), coverage (the smaller of the two images' occupied cells of an 8x8
    grid, over 64), label (list of str), and R (P,3,3), t (P,3) of recoverPose."""
    P = len(pts0_list)
    if P == 0:
        z = np.zeros(0)
        return dict(n_e=z.astype(np.int64), n_good=z.astype(np.int64), n_h=z.astype(np.int64), h_ratio=z,
                    median_angle_deg=z, coverage=z, label=[], R=np.zeros((0, 3, 3)), t=np.zeros((0, 3)))
    a, b, of = verify.pack_pairs(pts0_list, pts1_list)
    cam = verify._cam(K)
    e = verify.find_essential_batched(a, b, of, cam, prob, threshold)
    rp = verify.recover_pose_batched(e["E"], a, b, of, cam, mask=e["mask"])
    h = verify.find_homography_batched(a, b, of, h_threshold)
    st = verify.pair_stats_batched(a, b, of, e["mask"], rp["R"], cam, size)
    has_model = e["n_models"].cpu().numpy() > 0
    n_e = np.where(has_model, e["n_inliers"].cpu().numpy(), 0).astype(np.int64)
    n_good = np.where(has_model, rp["n_good"].cpu().numpy(), 0).astype(np.int64)
    n_h = h["n_inliers"].cpu().numpy().astype(np.int64)
    n_sel = st["n_sel"].cpu().numpy()
    med = st["median"].cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        ang = np.where(n_sel > 0, np.degrees(np.arccos(np.clip(med, -1.0, 1.0))), np.nan)
    coverage = _popcount64(st["cover"].cpu().numpy()).min(1) / 64.0
    h_ratio, labels = label_pairs(has_model, n_e, n_h, ang, max_h_ratio, min_angle_deg, min_inliers)
    return dict(n_e=n_e, n_good=n_good, n_h=n_h, h_ratio=h_ratio, median_angle_deg=ang, coverage=coverage,
                label=labels, R=rp["R"].cpu().numpy(), t=rp["t"].cpu().numpy())


def candidate_pairs(connection):
    """Every ordered pair bfs_tracks can examine, as verify.EssentialVerifier lists them: (u, v) with
    v in connection[u] or u in connection[v], sorted."""
    cand = sorted({(u, int(v)) for u in range(len(connection)) for v in connection[u]} |
                  {(int(v), u) for u in range(len(connection)) for v in connection[u]})
    return [(u, v) for u, v in cand if u != v]


def choose_pair(pairs, labels, n_good, coverage):
    """The GENERAL pair with the largest n_good * coverage, ties to the smaller (i, j) (host only).
    Raises ValueError naming the label counts when no pair is GENERAL."""
    best, best_score = None, -1.0
    for k in sorted(range(len(pairs)), key=lambda k: pairs[k]):
        if labels[k] != GENERAL:
            continue
        score = float(n_good[k]) * float(coverage[k])
        if score > best_score:
            best, best_score = k, score
    if best is None:
        counts = {l: sum(1 for x in labels if x == l) for l in LABELS}
        raise ValueError(f"no GENERAL pair among {len(pairs)} candidates to start from: {counts}")
    return best


def select_initial_pair(connection, match_fn, all_points, K, size, **kwargs):
    """Classifies every candidate pair of the connection graph (``match_fn(r, i) -> (idx0, idx1)``
    into ``all_points[r]`` / ``all_points[i]``, as for EssentialVerifier) and returns (i, j, table):
    the chosen pair and classify_pairs' result with ``pairs`` (the candidates, in table order)."""
    pairs = candidate_pairs(connection)
    p0, p1 = [], []
    for r, i in pairs:
        idx0, idx1 = match_fn(r, i)
        p0.append(np.asarray(all_points[r])[idx0].astype(np.float32).reshape(-1, 2))
        p1.append(np.asarray(all_points[i])[idx1].astype(np.float32).reshape(-1, 2))
    table = classify_pairs(p0, p1, K, size, **kwargs)
    table["pairs"] = pairs
    k = choose_pair(pairs, table["label"], table["n_good"], table["coverage"])
    return pairs[k][0], pairs[k][1], table
