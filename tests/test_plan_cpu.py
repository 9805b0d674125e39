"""CPU: the numpy restatement of V13 (tests/plan_ref.py) against brute force, np.sort and the MVS
scene's known answer, and the host-side pieces of plan.py (source selection, plane counts, the
adapter from SfM state).  No GPU."""
from importlib import import_module

import numpy as np
import pytest

import mvs_ref
import plan_ref as pr

F32, F64 = np.float32, np.float64


def random_scene(V, N, seed, vis=0.6):
    rng = np.random.default_rng(seed)
    syn = import_module("3d_reconstruction_amd.synthetic")
    Rs, ts = syn.orbit_cameras(4 * V, seed=seed)       # neighbours 360 / (4 V) degrees apart
    poses = np.concatenate([Rs[:V], ts[:V, :, None]], 2)
    X = rng.uniform(-1, 1, (N, 3))
    cam, pt = np.nonzero(rng.random((V, N)) < vis)
    return poses, X, cam, pt


def test_pair_counts_equal_brute_force():
    poses, X, cam, pt = random_scene(6, 40, 31)
    cam, pt = np.concatenate([cam, cam[:7]]), np.concatenate([pt, pt[:7]])      # repeated rows count once
    c2_lo, c2_hi = pr.angle_thresholds(5.0, 40.0)
    centres = np.stack([-poses[i, :, :3].T @ poses[i, :, 3] for i in range(6)])
    np.testing.assert_allclose(pr.camera_centres(poses), centres, atol=1e-14)
    centres = pr.camera_centres(poses)
    seen = np.zeros((6, 40), bool)
    seen[cam, pt] = True
    shared, good = np.zeros((6, 6), np.int32), np.zeros((6, 6), np.int32)
    for a in range(6):
        for b in range(6):
            for p in range(40):
                if a != b and seen[a, p] and seen[b, p]:
                    shared[a, b] += 1
                    ra, rb = centres[a] - X[p], centres[b] - X[p]
                    cos2 = float(ra @ rb) ** 2 / float((ra @ ra) * (rb @ rb))
                    good[a, b] += bool(ra @ rb > 0 and c2_lo <= cos2 <= c2_hi)
    s, g = pr.view_pair_counts(poses, X, cam, pt, 5.0, 40.0)
    assert np.array_equal(s, shared) and np.array_equal(g, good)
    assert 0 < good.sum() < shared.sum()
    assert np.array_equal(s, s.T) and not np.diag(s).any()


def test_pair_counts_degenerate_points():
    poses, X, cam, pt = random_scene(4, 12, 32, vis=1.0)
    X[0] = pr.camera_centres(poses)[1]            # on a camera centre
    X[1, 2], X[2, 0], X[3] = np.nan, np.inf, -np.inf
    s, g = pr.view_pair_counts(poses, X, cam, pt, 0.0, 90.0)
    assert (s[~np.eye(4, dtype=bool)] == 12).all()
    only = pr.view_pair_counts(poses, X[4:], cam[pt >= 4], pt[pt >= 4] - 4, 0.0, 90.0)[1]
    extra = g - only                              # what the four special points add
    assert not extra[1].any()                     # none of them is good with view 1
    assert extra.min() >= 0 and extra.max() <= 1  # the NaN and the infinite points nowhere; the point on centre 1 at most


def test_select_equals_sorted_keys():
    rng = np.random.default_rng(33)
    special = np.array([-0.0, 0.0, np.inf, -np.inf, 1.0, 1.0, 1.0, -1.0, -1.0, 1e-45, -1e-45], F32)
    vals = np.concatenate([special, rng.normal(0, 10, 500).astype(F32), rng.integers(-3, 3, 200).astype(F32)])
    rng.shuffle(vals)
    off = np.array([0, 0, 1, 300, len(vals)])
    for s in range(4):
        seg = vals[off[s]:off[s + 1]]
        n = len(seg)
        ranks = np.arange(-1, n + 1)
        out = pr.segmented_select(vals, off[s:s + 2], ranks[None, :])[0]
        keys = np.sort(pr.radix_key(seg))
        assert np.array_equal(out[1:-1].view(np.uint32), pr.key_value(keys).view(np.uint32))
        assert out[[0, -1]].view(np.uint32).tolist() == [0x7FC00000] * 2
    order = pr.key_value(np.sort(pr.radix_key(special)))
    assert np.signbit(order[4]) and order[4] == 0 and not np.signbit(order[5]) and order[5] == 0   # -0.0 < +0.0
    assert order[0] == -np.inf and order[-1] == np.inf
    with np.errstate(invalid="ignore"):
        assert (np.diff(order.astype(F64)) >= 0).all()


def test_select_sources_order_and_ties(sfm):
    good = np.array([[0, 20, 20, 20, 15, 40],
                     [20, 0, 0, 0, 0, 0],
                     [20, 0, 0, 0, 0, 0],
                     [20, 0, 0, 0, 0, 0],
                     [15, 0, 0, 0, 0, 16],
                     [40, 0, 0, 0, 16, 0]])
    shared = np.array([[0, 50, 60, 50, 90, 41],
                       [50, 0, 0, 0, 0, 0],
                       [60, 0, 0, 0, 0, 0],
                       [50, 0, 0, 0, 0, 0],
                       [90, 0, 0, 0, 0, 30],
                       [41, 0, 0, 0, 30, 0]])
    for fn in (pr.select_sources, sfm.select_sources):
        assert fn(shared, good, max_sources=4, min_good=16) == [[5, 2, 1, 3], [0], [0], [0], [5], [0, 4]]
        assert fn(shared, good, max_sources=2, min_good=16)[0] == [5, 2]
        assert fn(shared, good, max_sources=4, min_good=41) == [[]] * 6
        assert fn(shared, good, max_sources=16, min_good=1)[0] == [5, 2, 1, 3, 4]
    with pytest.raises(ValueError):
        sfm.select_sources(shared, good, max_sources=17)


def test_plane_count_rule_and_clipping(sfm):
    for fn in (pr.plane_count, sfm.plan.plane_count):
        # 220 * 0.5 * (1/2 - 1/10) = 44 px of disparity: 45 planes one pixel apart, 89 half a pixel apart
        assert fn(220.0, 0.5, 2.0, 10.0) == 45
        assert fn(220.0, 0.5, 2.0, 10.0, step_px=0.5) == 89
        assert fn(220.0, 0.5, 2.0, 10.0, step_px=1.0, p_max=32) == 32
        assert fn(220.0, 0.01, 2.0, 10.0) == 8 and fn(220.0, 0.01, 2.0, 10.0, p_min=2) == 2
        assert fn(220.0, 0.5, 2.0, 2.0 + 1e-9, p_min=1) == 2       # ceil of a tiny positive disparity, plus one
        assert fn(1000.0, 3.0, 0.5, 50.0) == 256
    P = pr.plane_count(220.0, 0.5, 2.0, 10.0)
    planes = mvs_ref.inverse_depth_planes(2.0, 10.0, P).astype(F64)
    step = 220.0 * 0.5 * np.abs(np.diff(1.0 / planes))
    assert step.max() <= 1.0 + 1e-5 and step.min() >= 0.97


def test_scene_bounds_hold_their_share():
    rng = np.random.default_rng(34)
    X = rng.normal(0, 1, (4000, 3)) * [1.0, 3.0, 0.2] + [5.0, -2.0, 0.0]
    X[:20] *= 1e4                                        # far outliers, fewer than q of the points
    X[40] = np.nan
    obs_pt = np.concatenate([np.arange(4000), np.arange(3000)])     # the last 1000 seen once: not counted
    for q in (0.01, 0.05):
        bmin, bmax = pr.scene_bounds(X, obs_pt, q=q, pad=0.0, min_obs=2)
        kept = X[:3000][np.isfinite(X[:3000]).all(1)].astype(F32)
        for ax in range(3):
            share = ((kept[:, ax] >= bmin[ax]) & (kept[:, ax] <= bmax[ax])).mean()
            assert share >= 1 - 2 * q, (q, ax, share)
        assert (bmax - bmin < [8, 24, 1.6]).all()        # the outliers did not set the box
    lo, hi = pr.scene_bounds(X, obs_pt, q=0.01, pad=0.0)
    bmin, bmax = pr.scene_bounds(X, obs_pt, q=0.01, pad=0.1)
    np.testing.assert_allclose(bmax - bmin, 1.2 * (hi.astype(F64) - lo), rtol=1e-6)
    assert not np.any(pr.scene_bounds(X, obs_pt[:0])[0]) and not np.any(pr.scene_bounds(X, obs_pt[:0])[1])


def test_depth_ranges_rank_rule():
    poses = np.eye(3, 4)[None].repeat(2, 0)
    z = np.arange(1, 102, dtype=F64)                     # depths 1 .. 101 in view 0
    X = np.concatenate([np.stack([0 * z, 0 * z, z], 1), [[0, 0, -1.0], [0, 0, np.nan]]])
    cam = np.concatenate([np.zeros(103, int), np.ones(5, int)])
    pt = np.concatenate([np.arange(103), np.arange(5)])
    near, far, count = pr.view_depth_ranges(poses, X, cam, pt, q=0.02, margin=0.1, min_points=8)
    assert count.tolist() == [101, 5]                    # the point behind and the NaN are not counted
    assert near[0] == F32(3.0 * 0.9) and far[0] == F32(99.0 * 1.1)      # ranks floor(2) and ceil(98)
    assert near[1] == 0 and far[1] == 0                  # fewer than min_points
    assert pr.quantile_ranks(11, 0.02) == (0, 10) and pr.quantile_ranks(1, 0.02) == (0, 0)


def test_adapter_maps_tracks_onto_keypoint_pixels(sfm):
    syn = import_module("3d_reconstruction_amd.synthetic")
    W, H, n_img = 1200.0, 900.0, 6
    sc = syn.sfm_scene(n_img=n_img, n_pts=300, seed=35)
    cameras = [np.hstack([sc["R"][c], sc["t"][c][:, None]]) for c in range(n_img)]
    cameras[4] = None                                    # an unregistered camera
    pts = [list(sc["X"]), [None] * 300]
    for t in (3, 17):
        pts[0][t] = None                                 # tracks that were never triangulated
    d = sfm.dense_inputs_from_reconstruction(cameras, pts, sc["img_pairs"], sc["all_matches"], syn.FOCAL, (W, H))
    assert 4 not in d["obs_cam"] and not d["poses"][4].any() and not np.isin([3, 17], d["tracks"]).any()
    pair = d["obs_cam"] * 300 + d["obs_pt"]
    assert len(np.unique(pair)) == len(pair) > 1000      # one observation per (camera, track)
    assert np.array_equal(d["X"], sc["X"][d["tracks"]])
    worst, near_kp = 0.0, []
    for c in set(d["obs_cam"].tolist()):
        sel = d["obs_cam"] == c
        Xw = d["X"][d["obs_pt"][sel]]
        Xc = Xw @ d["poses"][c, :, :3].T + d["poses"][c, :, 3]
        assert (Xc[:, 2] > 0).all()
        fx, fy, cx, cy = d["K"][c]
        uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
        Xs = Xw @ cameras[c][:, :3].T + cameras[c][:, 3]                 # the scene's own reprojection ...
        kp = syn.FOCAL * Xs[:, :2] / Xs[:, 2:]                           # ... in keypoint coordinates
        worst = max(worst, np.abs(uv - np.stack([kp[:, 0] + W / 2, H / 2 - kp[:, 1]], 1)).max())
        seen = np.asarray(sc["all_points"][c], F64)[d["obs_kp"][sel]]    # the keypoints themselves, as pixels
        near_kp.append(np.abs(uv - np.stack([seen[:, 0] + W / 2, H / 2 - seen[:, 1]], 1)).max(1))
    assert worst <= 1e-6, worst
    assert np.median(np.concatenate(near_kp)) < 1.0      # all but the wrong matches land on their keypoint
    R = d["poses"][0, :, :3]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
    assert np.linalg.det(R) < 0


def test_fixture_is_what_the_plan_was_measured_on():
    fx, plan = pr.fixture(), pr.fixture_plan()
    N = len(fx["X"])
    assert N == 960 and int((np.bincount(fx["obs_pt"], minlength=N) >= 2).sum()) == 944
    assert [len(p) for p in plan["planes"]] == [66, 50, 34, 50, 66]
    assert all(sorted(nb) == [s for s in range(5) if s != v] for v, nb in enumerate(plan["neighbours"]))
    assert plan["near"].min() > 2.7 and plan["far"].max() < 11.8
    off = ~np.eye(5, dtype=bool)
    assert plan["shared"][off].min() >= 700 and np.array_equal(plan["shared"], plan["good"])


def test_planned_fixture_passes_the_scene_figures():
    """The plan of the fixture (all four other views as sources, defaults otherwise) sweeps every
    view with its own planes and passes the five conditions of the MVS scene for view 2."""
    sc, plan = mvs_ref.scene(), pr.fixture_plan()
    cen = mvs_ref.census(sc["grey"])
    swept = np.zeros(sc["depth"].shape, F32)
    for r in range(5):
        swept[r] = mvs_ref.plane_sweep(cen, sc["poses"], sc["K"], [r], [plan["neighbours"][r]], plan["planes"][r],
                                       mvs_ref.SCENE["a"], mvs_ref.SCENE["penalty"], mvs_ref.SCENE["uniq"],
                                       mvs_ref.SCENE["min_views"])["depth"][0]
    _, filt = mvs_ref.depth_consistency(swept, sc["poses"], sc["K"], np.arange(5), mvs_ref.pad_sources(plan["neighbours"]),
                                        mvs_ref.SCENE["eps"], mvs_ref.SCENE["min_consistent"])
    f = mvs_ref.scene_figures(swept[2], filt[2], view=2)
    print(f)
    mvs_ref.check_scene_figures(f)
