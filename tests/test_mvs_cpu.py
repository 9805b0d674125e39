"""CPU: the V10 multi-view stereo definition (tests/mvs_ref.py) against known answers.  These
check the restatement and the test scene themselves; the HIP kernels are compared with the same
restatement in test_gpu_mvs.py."""
import ctypes

import numpy as np

import mvs_ref as m

F32, I32 = np.float32, np.int32
IDENT = np.eye(3, 4, dtype=F32)


def test_census_bits_by_hand():
    """A 7 x 7 image whose centre is 100: exactly the neighbours written brighter set their bit,
    in row-major order without the centre."""
    img = np.full((7, 7), 50, np.uint8)
    img[3, 3] = 100
    bright = {(0, 0): 0, (0, 6): 6, (2, 3): 17, (3, 2): 23, (3, 4): 24, (4, 3): 30, (6, 0): 41, (6, 6): 47}
    for (y, x) in bright:
        img[y, x] = 101
    img[1, 1] = 100   # equal is not brighter
    cen = m.census(img[None])
    assert int(cen[0, 3, 3]) == sum(1 << i for i in bright.values())
    assert int(cen[0, 3, 3]) >> 48 == 0
    # the corner (0, 0) holds 101: nothing inside the image is brighter, nothing outside counts
    assert int(cen[0, 0, 0]) == 0
    # pixel (0, 1) holds 50: its inside neighbours (dy >= 0, dx >= -1) brighter than 50
    want = 0
    i = 0
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            if dy == 0 and dx == 0:
                continue
            y, x = dy, 1 + dx
            if 0 <= y < 7 and 0 <= x < 7 and img[y, x] > 50:
                want |= 1 << i
            i += 1
    assert want != 0 and int(cen[0, 0, 1]) == want


def test_grey_weights():
    rgb = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]], np.uint8)
    assert m.grey(rgb).tolist() == [255, 77, 149, 29, (770 + 3000 + 870 + 128) >> 8]


def plane_case(order=1):
    """A fronto-parallel textured plane at depth 8 seen by two cameras with f = 64 that differ by
    a translation of 0.5 along x: the disparity at plane depth 32 / d is d pixels, so the planes
    16, 32/3, 8, 6.4, 16/3 have disparities 2..6 and the truth is plane 2 (disparity 4)."""
    H, W, d = 40, 72, 4
    rng = np.random.default_rng(3)
    tex = rng.integers(0, 256, (H, W + 16), dtype=np.uint8)
    img = np.stack([tex[:, 8:8 + W], tex[:, 8 + d:8 + d + W]])   # I1[v, u - d] = I0[v, u]
    poses = np.stack([IDENT, IDENT]).copy()
    poses[1, 0, 3] = -0.5
    K = np.tile(F32([[64, 64, W / 2, H / 2]]), (2, 1))
    planes = (F32(32) / np.arange(2, 7, dtype=F32))[::order]
    return m.census(img), poses, K, planes


def test_frontal_plane_is_recovered_with_zero_cost():
    cen, poses, K, planes = plane_case()
    out = m.plane_sweep(cen, poses, K, [0], [[1]], planes, a=2, penalty=24, uniq=243, min_views=1)
    inner = (slice(0, 1), slice(8, -8), slice(16, -16))   # census and aggregation windows inside both views
    assert (out["k"][inner] == 2).all() and (out["best"][inner] == 0).all() and (out["nv"][inner] == 1).all()
    assert (out["second"][inner] > 0).all()
    d = out["depth"][inner]
    # the sub-plane offset stays within half a plane step in inverse depth
    inv = 1.0 / planes.astype(np.float64)
    assert (d > 0).all() and (np.abs(1.0 / d - inv[2]) <= 0.5 * (inv[3] - inv[2]) * (1 + 1e-6)).all()
    print("depth range on the plane", d.min(), d.max())


def test_both_plane_orders_give_the_same_depth():
    """Near-to-far and far-to-near planes: k* mirrors, off and step change sign together, so the
    depth has the same bits wherever the minimum is attained once (a tie goes to the smaller k
    in either order, which is another plane)."""
    cen, poses, K, planes = plane_case()
    a = m.plane_sweep(cen, poses, K, [0], [[1]], planes, min_views=1)
    b = m.plane_sweep(cen, poses, K, [0], [[1]], planes[::-1].copy(), min_views=1)
    ag, _ = m.cost_volume(cen, poses, K, 0, [1], planes, 2, 24)
    once = (ag == ag.min(0)).sum(0) == 1
    assert once.mean() > 0.9
    assert np.array_equal(a["k"][0][once], len(planes) - 1 - b["k"][0][once])
    assert np.array_equal(a["depth"][0][once].view(np.uint32), b["depth"][0][once].view(np.uint32))
    assert (a["depth"][0][once] > 0).mean() > 0.5


def test_constant_images_are_all_invalid():
    cen, poses, K, planes = plane_case()
    cen = m.census(np.full((2, 40, 72), 9, np.uint8))
    assert not cen.any()
    out = m.plane_sweep(cen, poses, K, [0, 1], [[1], [0]], planes, min_views=0, uniq=256)
    assert not out["k"].any() and not out["depth"].any()   # every cost ties: k* = 0, not inside


def test_skip_rule():
    cen, poses, K, planes = plane_case()
    bad_pose = poses.copy()
    bad_pose[1, 2, 1] = np.inf
    bad_K = K.copy()
    bad_K[1, 1] = 0
    none = m.plane_sweep(cen, poses, K, [0], [[-1]], planes, min_views=0)
    assert (none["nv"] == 0).all() and (none["best"] == 24 * 25).all() and not none["depth"].any()
    for P, KK in ((bad_pose, K), (poses, bad_K)):
        # an invalid source is out of view everywhere: what a -1 entry gives
        out = m.plane_sweep(cen, P, KK, [0], [[1]], planes, min_views=0)
        assert all(np.array_equal(out[n], none[n]) for n in out)
        # an invalid reference gives all-zero outputs
        out = m.plane_sweep(cen, P, KK, [1], [[0]], planes, min_views=0)
        assert not any(out[n].any() for n in out)
        count, filt = m.depth_consistency(np.full((2, 40, 72), 8, F32), P, KK, [0, 1], [[1], [0]], 0.01, 0)
        assert not count.any() and (filt[0] == 8).all() and not filt[1].any()
    # 2^60 is out, the largest float below it is in
    edge = poses.copy()
    edge[1, 0, 3] = 2.0 ** 60
    assert not m.view_ok(edge[1], K[1])
    edge[1, 0, 3] = np.nextafter(F32(2.0 ** 60), F32(0))
    assert m.view_ok(edge[1], K[1])


def test_consistency_on_the_plane():
    """Both views see the plane z = 8 at depth 8: every pixel that lands inside the other view
    is consistent; a 2 % error in the source is not, at eps = 1 %."""
    _, poses, K, _ = plane_case()
    d = np.full((2, 40, 72), 8, F32)
    count, filt = m.depth_consistency(d, poses, K, [0], [[1]], 0.01, 1)
    assert (count[0, :, 4:] == 1).all() and (count[0, :, :4] == 0).all()
    assert (filt[0, :, 4:] == 8).all() and not filt[0, :, :4].any()
    d[1] = F32(8.16)
    assert not m.depth_consistency(d, poses, K, [0], [[1]], 0.01, 1)[0].any()
    assert m.depth_consistency(d, poses, K, [0], [[1]], 0.03, 1)[0][0, :, 4:].all()


def test_inverse_depth_planes(sfm):
    p = m.inverse_depth_planes(2, 7, 96)
    assert p.dtype == F32 and p[0] == 2 and p[-1] == 7 and (np.diff(p) > 0).all()
    inv = 1.0 / p.astype(np.float64)
    assert np.abs(np.diff(inv) - np.diff(inv).mean()).max() < 1e-6
    assert np.array_equal(sfm.mvs.inverse_depth_planes(2, 7, 96), p)
    assert np.array_equal(sfm.inverse_depth_planes(7, 2, 5), m.inverse_depth_planes(7, 2, 5))


def test_scene_known_answer():
    """The five-camera scene, view 2: the conditions of the definition's known answer.  The
    restatement gives completeness 0.958, 0.994 of the valid in-range pixels within 2 %,
    filtered completeness 0.920, 0.057 % of the filtered and 1.08 % of the unfiltered valid
    pixels off by more than 5 %."""
    swept = m.scene_sweep()["depth"]
    _, filt = m.scene_filtered()
    f = m.scene_figures(swept[2], filt[2])
    print(f)
    m.check_scene_figures(f)


def test_c_argument_checks_without_gpu(sfm):
    """The entry points report argument errors, and a no-op, without touching the GPU."""
    fl = ctypes.c_float
    err = sfm.lib.sfmhip_last_error
    f = sfm.lib.sfmhip_plane_sweep

    def sweep(S=4, P=12, a=2, penalty=24, uniq=243, min_views=2, R=1, H=4, W=4, p=1):
        return f(p, p, p, 5, H, W, p, p, R, S, p, P, a, penalty, uniq, min_views, p, None, None, None, None, None)

    for kw, word in ((dict(S=0), b"S must"), (dict(S=17), b"S must"), (dict(P=0), b"P must"),
                     (dict(P=65536), b"P must"), (dict(a=4), b"agg_radius"), (dict(a=-1), b"agg_radius"), (dict(penalty=49), b"penalty"),
                     (dict(uniq=257), b"uniq"), (dict(min_views=-1), b"min_views"), (dict(R=65536), b"reference views"),
                     (dict(H=-1), b"bad shape"), (dict(p=None), b"null pointer")):
        assert sweep(**kw) == -1, kw
        assert word in err(), (kw, err())
    assert sweep(R=0, p=None) == 0 and sweep(H=0, p=None) == 0 and sweep(W=0, p=None) == 0
    g = sfm.lib.sfmhip_depth_consistency
    assert g(1, 1, 1, 5, 4, 4, 1, 1, 1, 4, fl(float("nan")), 2, 1, 2, None) == -1 and b"eps" in err()
    assert g(1, 1, 1, 5, 4, 4, 1, 1, 1, 4, fl(-0.5), 2, 1, 2, None) == -1 and b"eps" in err()
    assert g(1, 1, 1, 5, 4, 4, 1, 1, 1, 0, fl(0.01), 2, 1, 2, None) == -1 and b"S must" in err()
    assert g(1, 1, 1, 5, 4, 4, 1, 1, 1, 4, fl(0.01), -1, 1, 2, None) == -1 and b"min_consistent" in err()
    assert g(1, 1, 1, 5, 4, 4, 1, 1, 1, 4, fl(0.01), 2, 1, 1, None) == -1 and b"alias" in err()
    assert g(None, 1, 1, 5, 4, 4, 1, 1, 1, 4, fl(0.01), 2, 1, 2, None) == -1 and b"null pointer" in err()
    assert g(None, None, None, 5, 4, 4, None, None, 0, 4, fl(0.01), 2, None, None, None) == 0
    c = sfm.lib.sfmhip_census
    assert c(None, 2, 4, 4, None, None) == -1 and b"null pointer" in err()
    assert c(1, -1, 4, 4, 1, None) == -1 and b"bad shape" in err()
    assert c(None, 0, 4, 4, None, None) == 0 and c(None, 2, 0, 4, None, None) == 0
