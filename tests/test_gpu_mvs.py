"""GPU: sfmhip_census / sfmhip_plane_sweep / sfmhip_depth_consistency (through mvs.py) against
the numpy restatement tests/mvs_ref.py (V10 of include/sfmhip.h).  The costs are integers and
the f32 steps are single IEEE operations on both sides, so every output is compared bit for bit."""
import numpy as np
import pytest
import torch

import mvs_ref as m

pytestmark = pytest.mark.gpu

F32, I32, U32 = np.float32, np.int32, np.uint32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U32) if a.dtype == F32 else a


def rodrigues(r):
    th = float(np.linalg.norm(r))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(r, np.float64) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def random_views(V, H, W, seed):
    """Random images under random nearby cameras around the origin looking along +z, each with
    its own intrinsics: at depths around 2 most pixels of one view land inside the others."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (V, H, W), dtype=np.uint8)
    poses = np.empty((V, 3, 4), F32)
    for v in range(V):
        poses[v, :, :3] = rodrigues(0.03 * rng.standard_normal(3))
        poses[v, :, 3] = 0.05 * rng.standard_normal(3)
    K = np.stack([F32([1.2 * W + v, 1.1 * W + 0.5 * v, W / 2 - 0.3 + 0.1 * v, H / 2 + 0.2 - 0.1 * v])
                  for v in range(V)])
    return img, poses, K


def planes_of(P):
    return m.inverse_depth_planes(1.5, 3.0, P)


def check_sweep(sfm, img, poses, K, refs, srcs, planes, **kw):
    """All five outputs of the sweep bit-equal to the restatement."""
    cen = m.census(img)
    ref = m.plane_sweep(cen, poses, K, refs, srcs, planes, kw.get("agg_radius", 2), kw.get("penalty", 24),
                        kw.get("uniq", 243), kw.get("min_views", 2))
    got = sfm.plane_sweep(torch.from_numpy(img), poses, K, refs, srcs, planes, diagnostics=True, **kw)
    got = dict(zip(("depth", "k", "best", "second", "nv"), (g.cpu().numpy() for g in got)))
    for name in ("k", "best", "second", "nv", "depth"):
        assert got[name].dtype == ref[name].dtype and got[name].shape == ref[name].shape, name
        assert np.array_equal(bits(got[name]), bits(ref[name])), name
    only = sfm.plane_sweep(torch.from_numpy(cen.view(np.int64)), poses, K, refs, srcs, planes, **kw)
    assert np.array_equal(bits(only.cpu().numpy()), bits(ref["depth"]))
    return ref


@pytest.fixture(scope="module")
def views():
    return random_views(5, 45, 62, 11)


@pytest.mark.parametrize("shape", [(45, 62), (1, 1), (3, 5)])
def test_census_bit_equal(sfm, gpu, shape):
    img, _, _ = random_views(3, shape[0], shape[1], 5)
    got = sfm.census_transform(torch.from_numpy(img))
    assert got.dtype == torch.int64 and tuple(got.shape) == img.shape
    assert np.array_equal(got.cpu().numpy().view(np.uint64), m.census(img))


def test_census_of_colour_images(sfm, gpu):
    rng = np.random.default_rng(2)
    for ch in (3, 4):
        rgb = rng.integers(0, 256, (2, 20, 33, ch), dtype=np.uint8)
        got = sfm.census_transform(torch.from_numpy(rgb))
        assert np.array_equal(got.cpu().numpy().view(np.uint64), m.census(m.grey(rgb)))


@pytest.mark.parametrize("S", [1, 4])
def test_sweep_odd_shape(sfm, gpu, views, S):
    """45 x 62 is no multiple of the tile; with the uniqueness test off most winners inside the
    plane range carry a depth, and with the default it is exercised on either side."""
    img, poses, K = views
    srcs = [[1, 2, 3, 4][:S]]
    ref = check_sweep(sfm, img, poses, K, [0], srcs, planes_of(12), uniq=256, min_views=1)
    # the data exercises what it should: many pixels with a depth, fully and partly seen ones
    assert (ref["depth"] > 0).mean() > 0.25 and (ref["nv"] == S).mean() > 0.5 and (ref["nv"] < S).any()
    ref = check_sweep(sfm, img, poses, K, [0], srcs, planes_of(12), uniq=250, min_views=S)
    valid = (ref["depth"] > 0).mean()
    print("valid share at uniq 250", valid)


@pytest.mark.parametrize("shape", [(16, 16), (17, 33), (1, 1), (3, 5)])
def test_sweep_edge_shapes(sfm, gpu, shape):
    """One exact tile; one pixel row and column more than a tile; tiles smaller than the halo."""
    img, poses, K = random_views(3, shape[0], shape[1], 7)
    check_sweep(sfm, img, poses, K, [1], [[0, 2]], planes_of(12), uniq=256, min_views=1)


@pytest.mark.parametrize("P", [1, 2, 3])
def test_sweep_few_planes(sfm, gpu, views, P):
    img, poses, K = views
    ref = check_sweep(sfm, img, poses, K, [0], [[1, 2]], planes_of(P), uniq=256, min_views=0)
    assert (ref["second"] == m.INT32_MAX).mean() > (0.0 if P == 3 else 0.99)
    if P < 3:
        assert not ref["depth"].any()


@pytest.mark.parametrize("a", [0, 3])
def test_sweep_window_radius(sfm, gpu, views, a):
    img, poses, K = views
    check_sweep(sfm, img, poses, K, [2], [[1, 3]], planes_of(12), agg_radius=a, uniq=256, min_views=1)


def test_sweep_penalty_and_plane_order(sfm, gpu, views):
    img, poses, K = views
    check_sweep(sfm, img, poses, K, [2], [[1, 3]], planes_of(12)[::-1].copy(), penalty=0, uniq=256, min_views=1)
    check_sweep(sfm, img, poses, K, [2], [[1, 3]], planes_of(12), penalty=48, uniq=256, min_views=2)


def test_sweep_sources_that_do_not_count(sfm, gpu, views):
    """A source that looks the other way, a -1 entry, a source the skip rule takes out, and an
    invalid reference."""
    img, poses, K = views
    poses = poses.copy()
    poses[3, :, :3] = np.diag([-1.0, 1.0, -1.0]) @ poses[3, :, :3]   # turned by 180 degrees about y
    ref = check_sweep(sfm, img, poses, K, [0], [[1, 3]], planes_of(12), uniq=256, min_views=1)
    assert ref["nv"].max() == 1
    away = ref
    ref = check_sweep(sfm, img, poses, K, [0], [[1, -1]], planes_of(12), uniq=256, min_views=1)
    assert all(np.array_equal(bits(ref[n]), bits(away[n])) for n in ref)
    bad = poses.copy()
    bad[4, 1, 2] = np.nan
    Kbad = K.copy()
    Kbad[4, 0] = 0
    for P_, K_ in ((bad, K), (poses, Kbad)):
        ref = check_sweep(sfm, img, P_, K_, [0], [[1, 4]], planes_of(12), uniq=256, min_views=1)
        assert all(np.array_equal(bits(ref[n]), bits(away[n])) for n in ref)
        ref = check_sweep(sfm, img, P_, K_, [4, 0], [[1, 2], [1, 2]], planes_of(12), uniq=256, min_views=1)
        assert not any(ref[n][0].any() for n in ref) and ref["depth"][1].any()


def test_sweep_two_references_with_their_own_lists(sfm, gpu, views):
    img, poses, K = views
    ref = check_sweep(sfm, img, poses, K, [3, 1], [[4, 2, -1], [0, 2, 3]], planes_of(12), uniq=256, min_views=2)
    assert ref["depth"][0].any() and ref["depth"][1].any()


def depth_maps(V, H, W, seed):
    """Depth maps around 2 that agree with a smooth surface within a few per cent, with holes
    and planted NaN, negative and infinite values."""
    rng = np.random.default_rng(seed)
    d = (2.0 + 0.03 * rng.standard_normal((V, H, W))).astype(F32)
    d[rng.random(d.shape) < 0.15] = 0
    flat = d.reshape(-1)
    for val in (np.nan, -1.5, np.inf, -np.inf):
        flat[rng.integers(0, flat.size, max(1, flat.size // 100))] = val
    return d


@pytest.mark.parametrize("shape", [(45, 62), (16, 16), (17, 33), (1, 1), (3, 5)])
def test_consistency_bit_equal(sfm, gpu, shape):
    _, poses, K = random_views(5, shape[0], shape[1], 11)
    d = depth_maps(5, shape[0], shape[1], 4)
    if shape == (1, 1):
        d[:] = 2.0
    refs, srcs = [0, 3, 4], [[1, 2, 3, 4], [4, 2, -1, -1], [0, 1, 2, 3]]
    bad = poses.copy()
    bad[4, 0, 0] = np.inf   # reference 4 is invalid, and so is a source of the others
    for P_, eps, mc in ((poses, 0.02, 2), (poses, 0.0, 0), (bad, 0.05, 1)):
        rc, rf = m.depth_consistency(d, P_, K, refs, srcs, eps, mc)
        count, filt = sfm.depth_consistency(torch.from_numpy(d), P_, K, refs, srcs, eps=eps, min_consistent=mc)
        assert count.dtype == torch.uint8 and filt.dtype == torch.float32
        assert np.array_equal(count.cpu().numpy(), rc)
        assert np.array_equal(bits(filt.cpu().numpy()), bits(rf))
        if shape == (45, 62) and mc == 2:
            hist = np.bincount(rc[0].ravel(), minlength=5)
            print("count histogram of reference 0", hist)
            assert (hist[:4] > 0).all() and (rf[0] > 0).any() and ((rf[0] == 0) & (d[0] > 0)).any()
    if shape == (45, 62):
        assert not rc[2].any() and not rf[2].any()


@pytest.fixture(scope="module")
def scene_gpu(sfm, gpu):
    sc = m.scene()
    grey = torch.from_numpy(sc["grey"]).to(gpu)
    swept = sfm.plane_sweep(grey, sc["poses"], sc["K"], [2], [sc["lists"][2]], sc["planes"], diagnostics=True)
    depth = sfm.mvs_depth(grey, sc["poses"], sc["K"], sc["lists"], sc["planes"])
    return grey, [t.cpu().numpy() for t in swept], depth


def test_scene_view_2_bit_equal(sfm, gpu, scene_gpu):
    _, swept, depth = scene_gpu
    ref = m.scene_sweep()
    for got, name in zip(swept, ("depth", "k", "best", "second", "nv")):
        assert np.array_equal(bits(got[0]), bits(ref[name][2])), name
    assert depth.dtype == torch.float32 and depth.is_cuda
    assert np.array_equal(bits(depth.cpu().numpy()), bits(m.scene_filtered()[1]))


def test_scene_known_answer_on_the_device(sfm, gpu, scene_gpu):
    _, swept, depth = scene_gpu
    f = m.scene_figures(swept[0][0], depth[2].cpu().numpy())
    print(f)
    m.check_scene_figures(f)


def test_scene_two_runs_give_the_same_bits(sfm, gpu, scene_gpu):
    grey, _, depth = scene_gpu
    sc = m.scene()
    again = sfm.mvs_depth(grey, sc["poses"], sc["K"], sc["lists"], sc["planes"])
    assert torch.equal(again.view(torch.int32), depth.view(torch.int32))


def test_empty_inputs_launch_nothing(sfm, gpu, views):
    img, poses, K = views
    none = np.zeros((0, 2), I32)
    out = sfm.plane_sweep(torch.from_numpy(img), poses, K, [], none, planes_of(12), diagnostics=True)
    assert [tuple(t.shape) for t in out] == [(0, 45, 62)] * 5
    count, filt = sfm.depth_consistency(np.zeros((5, 45, 62), F32), poses, K, [], none)
    assert tuple(count.shape) == (0, 45, 62) and tuple(filt.shape) == (0, 45, 62)
    flat = np.zeros((5, 0, 62), np.uint8)
    assert tuple(sfm.census_transform(torch.from_numpy(flat)).shape) == (5, 0, 62)
    assert tuple(sfm.plane_sweep(torch.from_numpy(flat), poses, K, [0], [[1]], planes_of(12)).shape) == (1, 0, 62)
    assert tuple(sfm.census_transform(torch.zeros((0, 4, 4), dtype=torch.uint8)).shape) == (0, 4, 4)
    assert tuple(sfm.mvs_depth(torch.from_numpy(flat), poses, K, m.neighbours(5), planes_of(12)).shape) == (5, 0, 62)
    torch.cuda.synchronize()


def test_non_default_stream(sfm, gpu, views):
    img, poses, K = views
    args = (torch.from_numpy(img).to(gpu), poses, K, m.neighbours(5), planes_of(12))
    kw = dict(uniq=256, min_views=1, eps=0.05, min_consistent=1)
    want = sfm.mvs_depth(*args, **kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = sfm.mvs_depth(*args, **kw)
    stream.synchronize()
    assert want.any() and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_wrapper_argument_checks(sfm, gpu, views):
    img, poses, K = views
    t = torch.from_numpy(img)
    with pytest.raises(ValueError, match="monotonic"):
        sfm.plane_sweep(t, poses, K, [0], [[1]], F32([2, 3, 3, 4]))
    with pytest.raises(ValueError, match="finite"):
        sfm.plane_sweep(t, poses, K, [0], [[1]], F32([2, -3]))
    with pytest.raises(ValueError, match="srcs"):
        sfm.plane_sweep(t, poses, K, [0], [list(range(17))], planes_of(4))
    with pytest.raises(ValueError, match="agg_radius"):
        sfm.plane_sweep(t, poses, K, [0], [[1]], planes_of(4), agg_radius=4)
    with pytest.raises(ValueError, match="poses"):
        sfm.plane_sweep(t, poses[:4], K, [0], [[1]], planes_of(4))
    with pytest.raises(ValueError, match="uint8"):
        sfm.census_transform(torch.zeros((1, 4, 4), dtype=torch.float32))
    with pytest.raises(ValueError, match="eps"):
        sfm.depth_consistency(np.zeros((5, 45, 62), F32), poses, K, [0], [[1]], eps=-1.0)
    with pytest.raises(ValueError, match="neighbours"):
        sfm.mvs_depth(t, poses, K, [[1]], planes_of(4))
