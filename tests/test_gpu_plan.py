"""GPU: V13 — sfmhip_obs_depth, sfmhip_view_pair_counts, sfmhip_segmented_select and the plan
built on them (plan.py) against the numpy restatement tests/plan_ref.py.  Everything is an
integer count or an op-for-op f64 / f32 value: every comparison is for equal bits."""
from importlib import import_module

import numpy as np
import pytest
import torch

import mvs_ref
import mvs_sgm_ref
import plan_ref as pr

pytestmark = pytest.mark.gpu
F32, F64, I64 = np.float32, np.float64, np.int64


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def orbit(V, spread=4):
    """V cameras 360 / (spread V) degrees apart on a circle around the origin, (V,3,4) f64."""
    syn = import_module("3d_reconstruction_amd.synthetic")
    Rs, ts = syn.orbit_cameras(spread * V, seed=41)
    return np.concatenate([Rs[:V], ts[:V, :, None]], 2)


def random_obs(V, N, seed, lo=0, hi=None):
    """N tracks of random lengths in [lo, hi], uniform points in the unit box."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (N, 3))
    cam, pt = [], []
    for p in range(N):
        seen = rng.choice(V, int(rng.integers(lo, (hi or V) + 1)), replace=False)
        cam.append(seen)
        pt.append(np.full(len(seen), p))
    return X, np.concatenate(cam).astype(I64), np.concatenate(pt).astype(I64)


def check_counts(sfm, poses, X, cam, pt, **kw):
    """The device matrices equal the restatement's; returns them (numpy)."""
    s, g = sfm.view_pair_counts(poses, X, cam, pt, **kw)
    assert s.dtype == torch.int32 and g.dtype == torch.int32 and s.shape == g.shape == (len(poses), len(poses))
    s, g = s.cpu().numpy(), g.cpu().numpy()
    rs, rg = pr.view_pair_counts(poses, X, cam, pt, **kw)
    assert np.array_equal(s, rs) and np.array_equal(g, rg)
    return s, g


# ---- pair counts ------------------------------------------------------------------------------
def test_pair_counts_small_shapes(sfm, gpu):
    poses = orbit(4)
    X = np.array([[0.1, 0.2, 0.3], [-0.4, 0.1, 0.0], [0.3, -0.3, 0.2]])
    s, g = check_counts(sfm, poses[:1], X, [0, 0, 0], [0, 1, 2])                       # V = 1
    assert s.tolist() == [[0]] and g.tolist() == [[0]]
    s, g = check_counts(sfm, poses[:2], X, [0, 1, 0, 1], [0, 1, 2, 2], min_angle=0.5)   # V = 2, one shared track
    assert s.tolist() == [[0, 1], [1, 0]] and g.tolist() == [[0, 1], [1, 0]]
    s, g = check_counts(sfm, poses, X, [3, 1, 0], [0, 1, 2])                          # tracks of length 1
    assert not s.any() and not g.any()


def test_pair_counts_one_track_seen_by_every_view(sfm, gpu):
    V = 64
    poses = orbit(V, spread=2)
    X, cam, pt = random_obs(V, 30, 42, lo=0, hi=3)
    cam, pt = np.concatenate([cam, np.arange(V)]), np.concatenate([pt, np.full(V, 7)])
    s, g = check_counts(sfm, poses, X, cam, pt)
    assert (s[~np.eye(V, dtype=bool)] >= 1).all() and 0 < g.sum() < s.sum()


def test_pair_counts_fixture_both_paths_and_any_order(sfm, gpu, knob):
    fx = pr.fixture()
    args = (fx["poses"], fx["X"])
    s, g = check_counts(sfm, *args, fx["obs_cam"], fx["obs_pt"])
    assert np.array_equal(s, pr.fixture_plan()["shared"])
    s2, g2 = check_counts(sfm, *args, fx["obs_cam"], fx["obs_pt"], min_angle=2.0, max_angle=4.0)
    assert np.array_equal(s2, s) and 0 < g2.sum() < g.sum()
    perm = np.random.default_rng(43).permutation(len(fx["obs_cam"]))
    dup = np.concatenate([perm, perm[:100], perm[50:60]])                              # shuffled, rows repeated
    for order in (perm, dup):
        s3, g3 = sfm.view_pair_counts(*args, fx["obs_cam"][order], fx["obs_pt"][order], min_angle=2.0, max_angle=4.0)
        assert np.array_equal(s3.cpu().numpy(), s2) and np.array_equal(g3.cpu().numpy(), g2)
    knob("PLAN_GLOBAL", 1)                                                             # straight to global memory
    s4, g4 = check_counts(sfm, *args, fx["obs_cam"], fx["obs_pt"], min_angle=2.0, max_angle=4.0)
    assert np.array_equal(s4, s2) and np.array_equal(g4, g2)


def test_pair_counts_twin_camera_is_no_source(sfm, gpu):
    """A camera with the centre of view 2, turned 10 degrees about its own y axis (the
    reference README's view pairs of types 1 and 2: same location, useless for triangulation)."""
    poses = orbit(6, spread=8)
    a = np.radians(10.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    poses[5] = Ry @ poses[2]                                                           # same centre: c = -R^T t
    rng = np.random.default_rng(44)
    N = 400
    X = rng.uniform(-1, 1, (N, 3))
    seen = rng.random((6, N)) < 0.25
    seen[2, :150] = seen[5, :150] = True                                               # the twins share many tracks
    cam, pt = np.nonzero(seen)
    s, g = check_counts(sfm, poses, X, cam, pt)
    assert g[2, 5] == 0 and g[5, 2] == 0 and s[2, 5] >= 100
    nb = sfm.select_sources(s, g, max_sources=4, min_good=16)
    assert nb == pr.select_sources(s, g, 4, 16)
    assert 5 not in nb[2] and 2 not in nb[5] and len(nb[2]) == 4
    assert all(s[2, b] < s[2, 5] for b in nb[2])                                       # kept with fewer shared tracks


def test_pair_counts_degenerate_points(sfm, gpu):
    poses = orbit(5)
    X, cam, pt = random_obs(5, 40, 45, lo=2)
    X[0] = pr.camera_centres(poses)[1]                                                 # exactly on a centre
    X[1, 1], X[2, 0], X[3] = np.nan, np.inf, -np.inf
    cam, pt = np.concatenate([cam, np.tile(np.arange(5), 4)]), np.concatenate([pt, np.repeat(np.arange(4), 5)])
    s, g = check_counts(sfm, poses, X, cam, pt, min_angle=0.0, max_angle=90.0)
    special = pt < 4
    _, g_rest = pr.view_pair_counts(poses, X, cam[~special], pt[~special], 0.0, 90.0)
    assert not (g - g_rest)[1].any() and (g - g_rest).max() <= 1 and s.min() >= 0     # shared, not good


@pytest.mark.parametrize("V", [200, 201])
def test_pair_counts_at_the_lds_limit(sfm, gpu, V):
    """The largest V whose triangles fit the LDS, and the first that adds to global memory."""
    assert sfm.plan.PAIR_LDS_MAX_VIEWS == 200
    poses = orbit(V, spread=1)
    X, cam, pt = random_obs(V, 500, 46, lo=0, hi=12)
    cam, pt = np.concatenate([cam, np.arange(V)]), np.concatenate([pt, np.full(V, 3)])      # and one seen by all
    s, g = check_counts(sfm, poses, X, cam, pt, max_angle=60.0)
    assert s[0, V - 1] >= 1 and s[V - 2, V - 1] >= 1 and 0 < g.sum() < s.sum()


def test_pair_counts_many_chunks(sfm, gpu):
    """More tracks than one chunk of 256 and more chunks than one workgroup walks in turn."""
    V = 12
    poses = orbit(V)
    X, cam, pt = random_obs(V, 3000, 47, lo=0, hi=V)
    check_counts(sfm, poses, X, cam, pt, max_angle=30.0)


def test_pair_counts_empty_inputs_and_errors(sfm, gpu):
    poses, none = orbit(3), np.zeros(0, I64)
    for X, cam, pt in ((np.zeros((0, 3)), none, none), (np.ones((4, 3)), none, none)):   # N = 0; M = 0
        s, g = sfm.view_pair_counts(poses, X, cam, pt)
        assert s.shape == (3, 3) and not s.any() and not g.any()
    s, g = sfm.view_pair_counts(np.zeros((0, 3, 4)), np.ones((4, 3)), none, none)
    assert s.shape == (0, 0) and g.shape == (0, 0)
    with pytest.raises(ValueError):
        sfm.view_pair_counts(poses, np.ones((4, 3)), [0, 3], [0, 1])
    with pytest.raises(ValueError):
        sfm.view_pair_counts(poses, np.ones((4, 3)), [0, 1], [0, 4])
    with pytest.raises(ValueError):
        sfm.view_pair_counts(poses, np.ones((4, 3)), [0, 1], [0, 1], max_angle=91.0)
    bad = sfm.lib.sfmhip_view_pair_counts(None, 3, None, 4, None, 2, None, 0.9, 0.5, None, None, None)
    assert bad == -1 and b"c2_lo" in sfm.lib.sfmhip_last_error()


# ---- observation depths -----------------------------------------------------------------------
def test_obs_depth(sfm, gpu):
    fx = pr.fixture()
    z = sfm.obs_depth(fx["poses"], fx["X"], fx["obs_cam"], fx["obs_pt"])
    assert z.dtype == torch.float32 and np.array_equal(bits(z.cpu().numpy()),
                                                       bits(pr.obs_depth(fx["poses"], fx["X"], fx["obs_cam"], fx["obs_pt"])))
    poses = np.eye(3, 4)[None].repeat(2, 0)
    poses[1, 2, 3] = 1e39                                                              # f32 overflow in view 1
    X = np.array([[0, 0, 2.5], [0, 0, -1.0], [0, 0, 0.0], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, np.inf], [0, 0, 1e-50]])
    cam, pt = np.repeat([0, 1], 7), np.tile(np.arange(7), 2)
    z = sfm.obs_depth(poses, X, cam, pt).cpu().numpy()
    assert np.array_equal(bits(z), bits(pr.obs_depth(poses, X, cam, pt)))
    # view 0: behind, at zero, NaN, an infinite depth and an underflow give +inf; 0 * inf is a NaN
    assert z[0] == F32(2.5) and np.isposinf(z[1:]).all()
    assert sfm.obs_depth(poses, X, [], []).shape == (0,)
    for cam, pt in (([2], [0]), ([-1], [0]), ([0], [7]), ([0], [-1])):
        with pytest.raises(ValueError):
            sfm.obs_depth(poses, X, cam, pt)
    assert sfm.lib.sfmhip_obs_depth(None, 2, None, 7, None, None, -1, None, None) == -1


# ---- segmented select -------------------------------------------------------------------------
def check_select(sfm, values, seg_off, ranks):
    out = sfm.segmented_select(values, seg_off, ranks).cpu().numpy()
    assert np.array_equal(bits(out), bits(pr.segmented_select(values, seg_off, ranks)))
    return out


def test_select_edge_segments(sfm, gpu):
    rng = np.random.default_rng(48)
    big = rng.normal(0, 100, 5000).astype(F32)
    big[:6] = [-0.0, 0.0, np.inf, -np.inf, np.inf, 0.0]
    low = (np.full(5000, 0x40490F00, np.uint32) + rng.integers(0, 256, 5000).astype(np.uint32)).view(F32)
    values = np.concatenate([np.array([3.5], F32), np.full(5000, 7.25, F32), big, low])
    seg_off = np.array([0, 0, 1, 5001, 10001, 15001])                    # empty, one, equal, random, low bits
    n = np.diff(seg_off)
    ranks = np.stack([np.zeros(5, I64), n - 1, n // 2], 1)               # R = 3
    out = check_select(sfm, values, seg_off, ranks)
    assert bits(out[0]).tolist() == [0x7FC00000] * 3 and out[1].tolist() == [3.5] * 3 and (out[2] == 7.25).all()
    assert out[3, 0] == -np.inf and out[3, 1] == np.inf
    keys = np.sort(pr.radix_key(big))
    assert bits(out[3, 2]) == bits(pr.key_value(keys[2500:2501]))[0]
    zeros = np.nonzero(keys == pr.radix_key(np.array([-0.0], F32))[0])[0]
    both = check_select(sfm, big, [0, 5000], [[zeros[0], zeros[0] + 1]])  # -0.0 directly below +0.0
    assert bits(both[0]).tolist() == [0x80000000, 0]
    edge = check_select(sfm, values, seg_off, np.stack([np.full(5, -1), n], 1))       # ranks -1 and n
    assert (bits(edge) == 0x7FC00000).all()
    every = np.arange(5000)[None, :]
    for lo in range(0, 5000, 1000):                                      # every rank of the random segment, R = 8
        for r0 in range(lo, lo + 1000, 500):
            sel = every[:, r0:r0 + 500:63]
            check_select(sfm, big, [0, 5000], sel)


def test_select_many_mixed_segments(sfm, gpu):
    rng = np.random.default_rng(49)
    n = rng.integers(0, 41, 300)
    n[:3] = [0, 1, 40]
    seg_off = np.concatenate([[0], np.cumsum(n)])
    values = rng.normal(0, 1, int(n.sum())).astype(F32)
    values[rng.random(len(values)) < 0.2] = 1.0                          # ties
    one = rng.integers(-1, 42, (300, 1))
    check_select(sfm, values, seg_off, one)                              # R = 1
    check_select(sfm, values, seg_off, np.stack([np.zeros(300, I64), n - 1, n // 2], 1))   # R = 3
    assert sfm.segmented_select(values, [0], np.zeros((0, 2), I64)).shape == (0, 2)
    assert sfm.segmented_select(values, seg_off, np.zeros((300, 0), I64)).shape == (300, 0)
    with pytest.raises(ValueError):
        sfm.segmented_select(values, seg_off, np.zeros((300, 9), I64))
    with pytest.raises(ValueError):
        sfm.segmented_select(values, seg_off, np.zeros((299, 1), I64))


# ---- the plan ---------------------------------------------------------------------------------
def assert_plan_equal(plan, ref):
    assert plan.neighbours == ref["neighbours"]
    for name in ("near", "far", "bmin", "bmax"):
        assert np.array_equal(bits(getattr(plan, name)), bits(ref[name])), name
    assert np.array_equal(plan.count, ref["count"])
    assert len(plan.planes) == len(ref["planes"])
    for a, b in zip(plan.planes, ref["planes"]):
        assert a.dtype == F32 and np.array_equal(bits(a), bits(b))
    assert np.array_equal(plan.shared.cpu().numpy(), ref["shared"]) and np.array_equal(plan.good.cpu().numpy(), ref["good"])


def test_ranges_bounds_and_plan_on_the_fixture(sfm, gpu):
    fx, ref = pr.fixture(), pr.fixture_plan()
    args = (fx["poses"], fx["X"], fx["obs_cam"], fx["obs_pt"])
    near, far, count = sfm.view_depth_ranges(*args)
    assert np.array_equal(bits(near.cpu().numpy()), bits(ref["near"]))
    assert np.array_equal(bits(far.cpu().numpy()), bits(ref["far"]))
    assert np.array_equal(count.cpu().numpy(), ref["count"])
    for kw in (dict(q=0.0, margin=0.0), dict(q=0.25, margin=0.5, min_points=900)):
        got, want = sfm.view_depth_ranges(*args, **kw), pr.view_depth_ranges(*args, **kw)
        assert all(np.array_equal(bits(g.cpu().numpy()), bits(w)) for g, w in zip(got[:2], want[:2]))
    bmin, bmax = sfm.scene_bounds(fx["X"], fx["obs_pt"])
    assert np.array_equal(bits(bmin.cpu().numpy()), bits(ref["bmin"]))
    assert np.array_equal(bits(bmax.cpu().numpy()), bits(ref["bmax"]))
    for kw in (dict(q=0.0, pad=0.0, min_obs=1), dict(q=0.1, pad=0.25, min_obs=5), dict(min_obs=6)):
        got, want = sfm.scene_bounds(fx["X"], fx["obs_pt"], **kw), pr.scene_bounds(fx["X"], fx["obs_pt"], **kw)
        assert all(np.array_equal(bits(g.cpu().numpy()), bits(w)) for g, w in zip(got, want)), kw
    plan = sfm.plan_dense(fx["poses"], fx["K"], *args[1:], max_sources=4)
    assert_plan_equal(plan, ref)
    assert [len(p) for p in plan.planes] == [len(p) for p in ref["planes"]]


def test_plan_with_a_thin_view_and_a_view_without_sources(sfm, gpu):
    """View 5 has 5 observations (fewer than min_points); view 6 sees many points that no other
    view sees well enough (every pair below min_good): both end without sources and planes."""
    fx = pr.fixture()
    poses = np.concatenate([fx["poses"], fx["poses"][[0, 4]]])
    poses[5, 0, 3] += 0.3
    poses[6, 0, 3] -= 0.3
    K = np.concatenate([fx["K"], fx["K"][:2]])
    X = np.concatenate([fx["X"], fx["X"][:50] + [0.0, 0.01, 0.0]])
    N0 = len(fx["X"])
    cam = np.concatenate([fx["obs_cam"], np.full(5, 5), np.full(50, 6), np.full(10, 6)])
    pt = np.concatenate([fx["obs_pt"], np.arange(5), N0 + np.arange(50), np.arange(10)])
    kw = dict(max_sources=3, min_good=16, step_px=0.75, p_max=60)
    plan, ref = sfm.plan_dense(poses, K, X, cam, pt, **kw), pr.plan_dense(poses, K, X, cam, pt, **kw)
    assert_plan_equal(plan, ref)
    assert plan.count[5] == 5 and plan.near[5] == 0 and plan.far[5] == 0 and plan.neighbours[5] == []
    assert plan.count[6] == 60 and plan.near[6] > 0 and plan.neighbours[6] == [] and len(plan.planes[6]) == 0
    assert all(len(nb) == 3 for nb in plan.neighbours[:5]) and max(len(p) for p in plan.planes) == 60


# ---- per-view planes in mvs_depth, and the whole dense path -----------------------------------
@pytest.fixture(scope="module")
def planned(sfm, gpu):
    fx, sc = pr.fixture(), mvs_ref.scene()
    plan = sfm.plan_dense(fx["poses"], fx["K"], fx["X"], fx["obs_cam"], fx["obs_pt"], max_sources=4)
    grey = torch.from_numpy(np.array(sc["grey"])).to(gpu)
    return plan, grey, sc


def test_mvs_depth_with_per_view_planes(sfm, gpu, planned):
    plan, grey, sc = planned
    depth = sfm.mvs_depth(grey, sc["poses"], sc["K"], plan.neighbours, plan.planes)
    swept = torch.stack([sfm.plane_sweep(grey, sc["poses"], sc["K"], [r], [plan.neighbours[r]], plan.planes[r])[0]
                         for r in range(5)])
    srcs = mvs_ref.pad_sources(plan.neighbours)
    filt = sfm.depth_consistency(swept, sc["poses"], sc["K"], np.arange(5), srcs)[1]
    assert torch.equal(depth.view(torch.int32), filt.view(torch.int32))
    cen = mvs_ref.census(sc["grey"])
    ref = np.stack([mvs_ref.plane_sweep(cen, sc["poses"], sc["K"], [r], [plan.neighbours[r]], plan.planes[r])["depth"][0]
                    for r in (0, 2)])
    assert np.array_equal(bits(swept[[0, 2]].cpu().numpy()), bits(ref))
    ref_filt = mvs_ref.depth_consistency(swept.cpu().numpy(), sc["poses"], sc["K"], np.arange(5), srcs)[1]
    assert np.array_equal(bits(depth.cpu().numpy()), bits(ref_filt))
    # a view without sources and planes stays invalid, and the others do not change but for its votes
    nb, pl = [list(x) for x in plan.neighbours], list(plan.planes)
    nb[4], pl[4] = [], np.zeros(0, F32)
    part = sfm.mvs_depth(grey, sc["poses"], sc["K"], nb, pl)
    assert not part[4].any() and bool((part[2] > 0).any())
    one = sfm.mvs_depth(grey, sc["poses"], sc["K"], plan.neighbours, [plan.planes[2]] * 5)
    assert torch.equal(one.view(torch.int32), sfm.mvs_depth(grey, sc["poses"], sc["K"], plan.neighbours,
                                                            plan.planes[2]).view(torch.int32))
    with pytest.raises(ValueError):
        sfm.mvs_depth(grey, sc["poses"], sc["K"], plan.neighbours, plan.planes[:4])


def test_mvs_depth_with_per_view_planes_smoothed(sfm, gpu, planned):
    plan, grey, sc = planned
    smooth = (4, 32)
    depth = sfm.mvs_depth(grey, sc["poses"], sc["K"], plan.neighbours, plan.planes, smooth=smooth)
    swept = torch.stack([sfm.plane_sweep(grey, sc["poses"], sc["K"], [r], [plan.neighbours[r]], plan.planes[r],
                                         smooth=smooth)[0] for r in range(5)])
    srcs = mvs_ref.pad_sources(plan.neighbours)
    filt = sfm.depth_consistency(swept, sc["poses"], sc["K"], np.arange(5), srcs)[1]
    assert torch.equal(depth.view(torch.int32), filt.view(torch.int32))
    r = 2                                                                # the view with the fewest planes
    ref = mvs_sgm_ref.plane_sweep(mvs_ref.census(sc["grey"]), sc["poses"], sc["K"], [r], [plan.neighbours[r]],
                                  plan.planes[r], smooth=(smooth[0], smooth[1], 0xFF))
    assert np.array_equal(bits(swept[r].cpu().numpy()), bits(ref["depth"][0]))
    ref_filt = mvs_ref.depth_consistency(swept.cpu().numpy(), sc["poses"], sc["K"], np.arange(5), srcs)[1]
    assert np.array_equal(bits(depth.cpu().numpy()), bits(ref_filt))


def test_planned_dense_path_end_to_end(sfm, gpu, planned):
    """Sparse observations -> plan -> depth maps -> the scene's figures -> TSDF over the planned
    box -> a mesh; a second run gives the same bytes."""
    plan, grey, sc = planned
    fx = pr.fixture()
    poses, K = torch.from_numpy(sc["poses"]).to(gpu), torch.from_numpy(sc["K"]).to(gpu)
    depth = sfm.mvs_depth(grey, poses, K, plan.neighbours, plan.planes)
    swept = sfm.plane_sweep(grey, poses, K, [2], [plan.neighbours[2]], plan.planes[2])
    f = mvs_ref.scene_figures(swept[0].cpu().numpy(), depth[2].cpu().numpy())
    print(f)
    mvs_ref.check_scene_figures(f)
    dims, bmin, bmax, step = sfm.cubic_grid(plan.bmin, plan.bmax, longest=96)
    assert max(dims) == 96 and all(b >= a for a, b in zip(plan.bmax.tolist(), bmax))
    T = torch.zeros(dims, dtype=torch.float32, device=gpu)
    Wt = torch.zeros_like(T)
    sfm.tsdf_integrate(T, Wt, depth, poses, K, bmin, bmax, 3 * step)
    verts, _, faces = sfm.tsdf_extract_surface(T, Wt, bmin, bmax)
    assert verts.shape[0] > 0 and faces.shape[0] > 0
    again = sfm.plan_dense(fx["poses"], fx["K"], fx["X"], fx["obs_cam"], fx["obs_pt"], max_sources=4)
    assert again.neighbours == plan.neighbours and all(a.tobytes() == b.tobytes() for a, b in zip(again.planes, plan.planes))
    for name in ("near", "far", "count", "bmin", "bmax"):
        assert getattr(again, name).tobytes() == getattr(plan, name).tobytes()
    assert torch.equal(again.shared, plan.shared) and torch.equal(again.good, plan.good)
    depth2 = sfm.mvs_depth(grey, poses, K, again.neighbours, again.planes)
    assert torch.equal(depth.view(torch.int32), depth2.view(torch.int32))
