"""CPU: the findHomography restatement (tests/homog_ref.py), its scene table, and the host-only parts
of the first-pair choice (tracks.with_initial_pair, twoview.label_pairs / choose_pair)."""
import importlib

import numpy as np
import pytest

import homog_ref as hr


@pytest.mark.parametrize("name", hr.H_NAMES)
def test_scene_is_admissible(name):
    ok, runs = hr.h_variants(name)
    assert ok, {v: (r["ok"], r["iters"], r["n_inliers"], r["adoptions"][-2:]) for v, r in runs.items()}


@pytest.mark.parametrize("name", hr.H_NAMES)
def test_scene_has_its_property(name):
    prop, sc = hr.h_property(name), hr.h_scene(name)
    tr = hr.h_run(name, keep_masks=bool(prop.get("tie")))
    assert tr["ok"] == prop["ok"]
    assert tr["mask"].shape == (len(sc["src"]),) and int(tr["mask"].sum()) == tr["n_inliers"]
    if "iters" in prop:
        assert tr["iters"] == prop["iters"]
    if "inliers" in prop:
        assert tr["n_inliers"] == prop["inliers"]
    if "min_inlier_frac" in prop:
        assert tr["n_inliers"] >= prop["min_inlier_frac"] * len(sc["src"])
    if "max_iters_run" in prop:
        assert tr["iters"] <= prop["max_iters_run"]
    if prop.get("late"):
        assert tr["adoptions"][-1][0] >= hr.HOMOG_CHUNK
    if prop.get("tie"):
        assert hr.has_tie(tr)
    if "recovers" in prop:
        assert hr.rel_fro(tr["H"], sc["H"]) <= prop["recovers"]
    if tr["ok"]:
        assert tr["H"][2, 2] == 1.0 and np.all(np.isfinite(tr["H"]))
    else:
        assert tr["H"] is None and not tr["mask"].any()


def test_size_scenes_cover_the_scoring_block_and_the_small_counts():
    sizes = sorted(len(hr.h_scene(n)["src"]) for n in hr.SIZE_NAMES)
    assert sizes == [0, 3, 4, 5, 63, 64, 65, 255, 257, 1023, 1024, 1025, 2500]
    assert hr.HOMOG_BLOCK in sizes and max(sizes) > 2 * hr.HOMOG_BLOCK


def test_restatement_recovers_a_known_homography():
    """Noise-free planar correspondences in f64 with 20 % outliers: H to 1e-6 relative."""
    rng = np.random.default_rng(0)
    H = np.array([[0.9, 0.08, 25.0], [-0.06, 1.05, -14.0], [2e-5, -1e-5, 1.0]])
    src = rng.uniform(0, 1, (200, 2)) * np.array(hr.SIZE)
    q = np.column_stack([src, np.ones(200)]) @ H.T
    dst = q[:, :2] / q[:, 2:3]
    bad = rng.random(200) < 0.2
    dst[bad] = rng.uniform(0, 1, (int(bad.sum()), 2)) * np.array(hr.SIZE)
    for variant in ("plain", "svd"):
        tr = hr.find_homography(src, dst, variant=variant)
        assert tr["ok"] == 1 and np.array_equal(tr["mask"].astype(bool), ~bad)
        assert hr.rel_fro(tr["H"], H) <= 1e-6


def test_check_subset_rejects_collinear_and_flipped_samples():
    sq = np.array([[0.0, 0], [10, 0], [10, 10], [0, 10]])
    assert hr.check_subset(sq, sq + 3.0)
    assert not hr.check_subset(np.array([[0.0, 0], [5, 5], [10, 10], [0, 10]]), sq)      # collinear in the source
    assert not hr.check_subset(sq, np.array([[0.0, 0], [10, 0], [0, 10], [10, 10]]))     # a bow tie: triples flip
    assert not hr.check_subset(sq, sq * np.array([-1.0, 1.0]))                           # mirrored: all four flip


def test_pair_stats_restatement_on_a_known_angle():
    """A camera turned by 10 degrees about y with R given: zero parallax after the rotation is
    removed; with the identity given instead, the median is the ray's own turn."""
    from oracle import geometry as og
    K = hr.TV_K
    cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    R = og.rodrigues(np.array([0.0, np.radians(10.0), 0.0]))
    p0 = np.array([[640.0, 480.0], [100.0, 900.0], [1280.0, 100.0]])
    ray = np.column_stack([p0, np.ones(3)]) @ np.linalg.inv(K).T
    q = ray @ R.T @ K.T
    p1 = q[:, :2] / q[:, 2:3]
    st = hr.pair_stats(p0, p1, np.array([1, 1, 0]), R, cam, *hr.TV_SIZE)
    assert np.allclose(st["cosang"][:2], 1.0, atol=1e-12) and st["cosang"][2] == 2.0 and st["n_sel"] == 2
    st = hr.pair_stats(p0, p1, np.ones(3), np.eye(3), cam, *hr.TV_SIZE)
    assert abs(np.degrees(np.arccos(st["cosang"][0])) - 10.0) < 1e-9
    # the third point lies on x = W: outside, so image 0 has two cells
    assert st["cover"][0] == (1 << (4 * 8 + 4)) | (1 << (7 * 8 + 0))


# ---------------------------------------------------------------------------------------------
# host-only parts of the package

def test_with_initial_pair_and_bfs_order(sfm):
    """bfs_tracks from with_initial_pair's graph examines the chosen pair first; the input graph is
    left alone."""
    tracks = sfm.tracks
    conn = [[1, 2, 3], [0, 2], [0, 1, 3], [2, 0]]
    out = tracks.with_initial_pair(conn, 0, 3)
    assert out == [[3, 1, 2], [0, 2], [0, 1, 3], [2, 0]] and conn[0] == [1, 2, 3]
    assert tracks.with_initial_pair(conn, 1, 3)[1] == [3, 0, 2]            # an absent j is put in front
    for bad in ((0, 0), (0, 4), (-1, 2)):
        with pytest.raises(ValueError):
            tracks.with_initial_pair(conn, *bad)
    seen = []

    def match_fn(r, i):            # every pair shares keypoints 0..19, one to one
        seen.append((r, i))
        idx = np.arange(20, dtype=np.int64)
        return idx, idx

    n_kpts = [20] * 4
    pairs, matches = tracks.bfs_tracks(out, 0, n_kpts, match_fn, min_matches=10)
    assert seen[0] == (0, 3) and pairs[0] == (0, 3) and len(pairs) == 3
    seen.clear()
    pairs, _ = tracks.bfs_tracks(conn, 0, n_kpts, match_fn, min_matches=10)
    assert seen[0] == (0, 1) and pairs[0] == (0, 1)


def test_label_logic_on_given_counts(sfm):
    tv = sfm.twoview
    has = [0, 1, 1, 1, 1, 1]
    n_e = [500, 29, 400, 400, 400, 30]
    n_h = [450, 29, 321, 320, 100, 10]
    ang = [9.0, 9.0, 9.0, 3.999, 4.0, np.nan]
    h_ratio, labels = tv.label_pairs(has, n_e, n_h, ang)
    assert labels == [tv.DEGENERATE, tv.DEGENERATE, tv.PLANAR_OR_ROTATION, tv.LOW_PARALLAX, tv.GENERAL, tv.GENERAL]
    assert h_ratio[2] == 321 / 400 and h_ratio[3] == 0.8
    # the thresholds are arguments
    _, labels = tv.label_pairs(has, n_e, n_h, ang, max_h_ratio=0.9, min_angle_deg=10.0, min_inliers=10)
    assert labels == [tv.DEGENERATE, tv.PLANAR_OR_ROTATION, tv.LOW_PARALLAX, tv.LOW_PARALLAX, tv.LOW_PARALLAX,
                      tv.GENERAL]
    # the restatement's label function agrees
    for p in range(6):
        assert hr.label(has[p], n_e[p], n_h[p] / max(n_e[p], 1), ang[p]) == tv.label_pairs(has, n_e, n_h, ang)[1][p]


def test_choose_pair_prefers_score_then_the_smaller_pair(sfm):
    tv = sfm.twoview
    pairs = [(2, 1), (0, 3), (0, 2), (1, 3)]
    labels = [tv.GENERAL, tv.GENERAL, tv.PLANAR_OR_ROTATION, tv.GENERAL]
    assert tv.choose_pair(pairs, labels, [100, 100, 900, 80], [0.5, 0.5, 1.0, 0.5]) == 1      # a tie: (0, 3) < (2, 1)
    assert tv.choose_pair(pairs, labels, [100, 100, 900, 200], [0.5, 0.5, 1.0, 0.5]) == 3
    with pytest.raises(ValueError, match="PLANAR_OR_ROTATION.*2"):
        tv.choose_pair(pairs[:2], [tv.PLANAR_OR_ROTATION] * 2, [1, 1], [1, 1])
    assert tv.candidate_pairs([[1], [2], []]) == [(0, 1), (1, 0), (1, 2), (2, 1)]


def test_new_names_are_exported(sfm):
    for name in ("findHomography", "classify_pairs", "select_initial_pair", "with_initial_pair"):
        assert callable(getattr(sfm, name)), name
    assert callable(sfm.verify.find_homography_batched) and callable(sfm.verify.pair_stats_batched)
    assert sfm.lib.sfmhip_find_homography and sfm.lib.sfmhip_pair_stats
