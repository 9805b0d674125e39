"""GPU: sfmhip_cost_volume / sfmhip_sgm_aggregate / sfmhip_volume_select and the smooth= mode of
plane_sweep and mvs_depth (through mvs.py) against the numpy restatement tests/mvs_sgm_ref.py
(steps 4a, 4b and 5' - 7' of the V10 block of include/sfmhip.h).  The costs are integers and the
f32 steps single IEEE operations on both sides: every output is compared bit for bit."""
import numpy as np
import pytest
import torch

import mvs_ref as m
import mvs_sgm_ref as g
from test_gpu_mvs import bits, planes_of, random_views

pytestmark = pytest.mark.gpu

F32, I32, U32 = np.float32, np.int32, np.uint32
NAMES = ("depth", "k", "best", "second", "nv")


def equal_maps(got, ref):
    got = dict(zip(NAMES, (t.cpu().numpy() for t in got)))
    for name in NAMES:
        assert got[name].dtype == ref[name].dtype and got[name].shape == ref[name].shape, name
        assert np.array_equal(bits(got[name]), bits(ref[name])), name
    return got


@pytest.fixture(scope="module")
def views():
    return random_views(5, 45, 62, 11)


# ---- cost_volume ----------------------------------------------------------------------------------
def check_volume(sfm, img, poses, K, refs, srcs, planes, **kw):
    want = g.cost_volume(m.census(img), poses, K, refs, srcs, planes, kw.get("agg_radius", 2), kw.get("penalty", 24))
    got = sfm.cost_volume(torch.from_numpy(img), poses, K, refs, srcs, planes, **kw)
    assert got.dtype == torch.uint16 and tuple(got.shape) == want.shape and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    return want


@pytest.mark.parametrize("shape,S", [((45, 62), 1), ((45, 62), 4), ((17, 33), 2), ((16, 16), 2), ((3, 5), 2), ((1, 1), 2)])
def test_volume_shapes(sfm, gpu, shape, S):
    """No multiple of the tile; one pixel row and column more than a tile; one exact tile; tiles
    smaller than the halo.  12 planes take the plane-by-plane stores, 8 the packed one."""
    img, poses, K = random_views(5, shape[0], shape[1], 11)
    for P in (12, 8):
        vol = check_volume(sfm, img, poses, K, [0], [[1, 2, 3, 4][:S]], planes_of(P))
        assert vol.any() and vol.max() <= 37632


@pytest.mark.parametrize("P", [1, 2, 3, 7, 8, 9, 65, 96])
def test_volume_plane_counts(sfm, gpu, P):
    """The eight-plane packing, its tail, and planes that are no multiple of eight, on 2 x 2 tiles."""
    img, poses, K = random_views(3, 17, 33, 7)
    check_volume(sfm, img, poses, K, [1], [[0, 2]], planes_of(P))


def test_volume_window_penalty_and_plane_order(sfm, gpu, views):
    img, poses, K = views
    for a in (0, 3):
        check_volume(sfm, img, poses, K, [2], [[1, 3]], planes_of(16), agg_radius=a)
    check_volume(sfm, img, poses, K, [2], [[1, 3]], planes_of(12)[::-1].copy(), penalty=0)
    top = check_volume(sfm, img, poses, K, [2], [[1, 3]], planes_of(16), penalty=48, agg_radius=3)
    print("largest cost at penalty 48, a = 3, S = 2:", top.max())


def test_volume_sources_that_do_not_count(sfm, gpu, views):
    """A source that looks away equals a -1 entry; a reference the skip rule removes gives an
    all-zero slice; two references with their own lists."""
    img, poses, K = views
    poses = poses.copy()
    poses[3, :, :3] = np.diag([-1.0, 1.0, -1.0]) @ poses[3, :, :3]
    away = check_volume(sfm, img, poses, K, [0], [[1, 3]], planes_of(8))
    assert np.array_equal(check_volume(sfm, img, poses, K, [0], [[1, -1]], planes_of(8)), away)
    bad = poses.copy()
    bad[4, 1, 2] = np.nan
    for P in (8, 12):
        vol = check_volume(sfm, img, bad, K, [4, 0, 7], [[1, 2], [1, 4], [1, 2]], planes_of(P))
        assert not vol[0].any() and vol[1].any() and not vol[2].any()
    vol = check_volume(sfm, img, poses, K, [3, 1], [[4, 2, -1], [0, 2, 3]], planes_of(8))
    assert vol[0].any() and vol[1].any() and not np.array_equal(vol[0], vol[1])


# ---- sgm_aggregate --------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (9, 5), (33, 17)]
PENALTIES = [(0, 0), (0, 5), (3, 3), (50, 400), (16383, 16383)]


def check_aggregate(sfm, vol, p1, p2, mask):
    want = g.sgm_aggregate(vol, p1, p2, mask)
    got = sfm.sgm_aggregate(torch.from_numpy(vol), p1, p2, ("mask", mask))
    assert got.dtype == torch.int32 and tuple(got.shape) == vol.shape and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(U32), want), (vol.shape, p1, p2, hex(mask))


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 96, 255, 256])
def test_aggregate_random_volumes(sfm, gpu, P):
    """R = 2, every shape, both value ranges ([0, 3] is tie-heavy and takes all four branches of the
    minimum) and every pair of penalties; 8 and 4 paths alternate so that each meets every one."""
    rng = np.random.default_rng(100 + P)
    for si, (H, W) in enumerate(SHAPES):
        for ri, hi in enumerate((37633, 4)):
            vol = rng.integers(0, hi, (2, H, W, P)).astype(np.uint16)
            for pi, (p1, p2) in enumerate(PENALTIES):
                check_aggregate(sfm, vol, p1, p2, (0xFF, 0x0F)[(si + ri + pi) % 2])


def test_aggregate_spellings_of_paths(sfm, gpu):
    vol = np.random.default_rng(1).integers(0, 4, (2, 5, 9, 6)).astype(np.uint16)
    for paths, mask in ((8, 0xFF), (4, 0x0F)):
        got = sfm.sgm_aggregate(torch.from_numpy(vol).view(torch.int16), 1, 2, paths)   # int16: the same bits
        assert np.array_equal(got.cpu().numpy().view(U32), g.sgm_aggregate(vol, 1, 2, mask))
    assert not np.array_equal(g.sgm_aggregate(vol, 1, 2, 0xFF), 2 * g.sgm_aggregate(vol, 1, 2, 0x0F))


@pytest.mark.parametrize("bit", range(8))
def test_aggregate_single_directions(sfm, gpu, bit):
    """One direction at a time, so that no two directions' errors can cancel."""
    rng = np.random.default_rng(bit)
    for H, W in ((5, 9), (9, 5)):
        for P, hi, (p1, p2) in ((5, 4, (1, 2)), (96, 37633, (50, 400)), (7, 37633, (0, 5)), (64, 4, (3, 3))):
            check_aggregate(sfm, rng.integers(0, hi, (2, H, W, P)).astype(np.uint16), p1, p2, 1 << bit)


# ---- volume_select --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(45, 62), (3, 5), (1, 1)])
def test_select_of_the_unsmoothed_volume_is_the_shipped_sweep(sfm, gpu, shape):
    """cost_volume widened to 32 bits and selected gives all five outputs of plane_sweep."""
    img, poses, K = random_views(5, shape[0], shape[1], 11)
    cen = sfm.census_transform(torch.from_numpy(img))
    for P, refs, srcs, kw in ((12, [0], [[1, 2, 3, 4]], dict(uniq=256, min_views=1)),
                              (9, [3, 1], [[4, 2, -1], [0, 2, 3]], dict(uniq=250, min_views=2))):
        planes = planes_of(P)
        want = sfm.plane_sweep(cen, poses, K, refs, srcs, planes, diagnostics=True, **kw)
        vol = sfm.cost_volume(cen, poses, K, refs, srcs, planes)
        wide = vol.view(torch.int16).to(torch.int32) & 0xFFFF
        got = sfm.volume_select(wide, poses, K, refs, srcs, planes, diagnostics=True, **kw)
        for a, b, name in zip(got, want, NAMES):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
        only = sfm.volume_select(wide, poses, K, refs, srcs, planes, **kw)
        assert torch.equal(only.view(torch.int32), want[0].view(torch.int32))
        if shape == (45, 62) and kw["uniq"] == 256:
            assert (want[0] > 0).any()


@pytest.mark.parametrize("P", [1, 2, 3, 7, 12, 256])
def test_select_random_volumes(sfm, gpu, views, P):
    """Tie-heavy volumes in [0, 3] and full-range ones in [0, 2^19); P = 1 and 2 are all-invalid;
    the uniqueness test off and at its strictest, min_views 0 and one more than the sources."""
    _, poses, K = views
    rng = np.random.default_rng(P)
    refs, srcs, planes = [0, 3], [[1, 2, 3, 4], [4, 2, -1, 9]], planes_of(P)
    nv_of = [g.visible_count(poses, K, r, s, planes, 45, 62) for r, s in zip(refs, srcs)]   # once: it needs no volume
    for hi in (4, 2 ** 19):
        sm = rng.integers(0, hi, (2, 45, 62, P)).astype(I32)
        for uniq, min_views in ((243, 2), (0, 0), (256, 0), (256, 5)):
            ref = g.volume_select(sm, poses, K, refs, srcs, planes, uniq, min_views, nv_of)
            got = sfm.volume_select(torch.from_numpy(sm), poses, K, refs, srcs, planes, uniq=uniq, min_views=min_views,
                                    diagnostics=True)
            equal_maps(got, ref)
            if P < 3 or min_views == 5:
                assert not ref["depth"].any()
            elif uniq == 256:
                assert (ref["depth"] > 0).any()
    bad = poses.copy()
    bad[0, 0, 0] = np.inf   # reference 0 is invalid
    ref = equal_maps(sfm.volume_select(torch.from_numpy(sm), bad, K, refs, srcs, planes, uniq=256, min_views=0,
                                       diagnostics=True), g.volume_select(sm, bad, K, refs, srcs, planes, 256, 0))
    assert not any(ref[n][0].any() for n in NAMES)


# ---- the smoothed sweep and mvs_depth -----------------------------------------------------------
@pytest.mark.parametrize("paths,mask", [(8, 0xFF), (4, 0x0F)])
def test_smoothed_sweep_bit_equal(sfm, gpu, views, paths, mask):
    img, poses, K = views
    refs, srcs, planes = [0, 2], [[1, 2, 3, 4], [0, 1, 3, 4]], planes_of(12)
    ref = g.plane_sweep(m.census(img), poses, K, refs, srcs, planes, 2, 24, 256, 2, (3, 40, mask))
    got = sfm.plane_sweep(torch.from_numpy(img), poses, K, refs, srcs, planes, uniq=256, min_views=2, diagnostics=True,
                          smooth=(3, 40, paths))
    equal_maps(got, ref)
    assert (ref["depth"] > 0).any() and (ref["depth"] == 0).any()
    only = sfm.plane_sweep(torch.from_numpy(img), poses, K, refs, srcs, planes, uniq=256, min_views=2,
                           smooth=(3, 40) if paths == 8 else (3, 40, ("mask", mask)))
    assert np.array_equal(bits(only.cpu().numpy()), bits(ref["depth"]))


@pytest.fixture(scope="module")
def scene_gpu(sfm, gpu):
    sc = m.scene()
    grey = torch.from_numpy(sc["grey"]).to(gpu)
    swept = sfm.plane_sweep(grey, sc["poses"], sc["K"], [2], [sc["lists"][2]], sc["planes"], diagnostics=True,
                            smooth=g.SMOOTH[:2])
    depth = sfm.mvs_depth(grey, sc["poses"], sc["K"], sc["lists"], sc["planes"], smooth=g.SMOOTH[:2])
    return grey, [t.cpu().numpy() for t in swept], depth


def test_scene_bit_equal(sfm, gpu, scene_gpu):
    _, swept, depth = scene_gpu
    ref = g.scene_sweep()
    for got, name in zip(swept, NAMES):
        assert np.array_equal(bits(got[0]), bits(ref[name][2])), name
    assert depth.dtype == torch.float32 and depth.is_cuda
    assert np.array_equal(bits(depth.cpu().numpy()), bits(g.scene_filtered()[1]))   # all five views


def test_scene_conditions_on_the_device(sfm, gpu, scene_gpu):
    _, swept, depth = scene_gpu
    f = m.scene_figures(swept[0][0], depth[2].cpu().numpy())
    print(f)
    g.check_smoothed_figures(f)


def test_scene_two_runs_give_the_same_bits(sfm, gpu, scene_gpu):
    grey, _, depth = scene_gpu
    sc = m.scene()
    again = sfm.mvs_depth(grey, sc["poses"], sc["K"], sc["lists"], sc["planes"], smooth=g.SMOOTH[:2])
    assert torch.equal(again.view(torch.int32), depth.view(torch.int32))


def test_non_default_stream(sfm, gpu, views):
    img, poses, K = views
    args = (torch.from_numpy(img).to(gpu), poses, K, m.neighbours(5), planes_of(12))
    kw = dict(uniq=256, min_views=1, eps=0.05, min_consistent=1, smooth=(3, 40))
    want = sfm.mvs_depth(*args, **kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = sfm.mvs_depth(*args, **kw)
    stream.synchronize()
    assert want.any() and torch.equal(got.view(torch.int32), want.view(torch.int32))
    plain = sfm.mvs_depth(*args, **{**kw, "smooth": None})
    assert not torch.equal(plain.view(torch.int32), want.view(torch.int32))   # the smoothing took part


def test_empty_inputs_launch_nothing(sfm, gpu, views):
    img, poses, K = views
    none = np.zeros((0, 2), I32)
    t = torch.from_numpy(img)
    assert tuple(sfm.cost_volume(t, poses, K, [], none, planes_of(12)).shape) == (0, 45, 62, 12)
    assert tuple(sfm.sgm_aggregate(torch.zeros((0, 45, 62, 12), dtype=torch.uint16), 1, 2).shape) == (0, 45, 62, 12)
    assert tuple(sfm.sgm_aggregate(torch.zeros((2, 0, 62, 12), dtype=torch.uint16), 1, 2).shape) == (2, 0, 62, 12)
    out = sfm.volume_select(torch.zeros((0, 45, 62, 12), dtype=torch.int32), poses, K, [], none, planes_of(12),
                            diagnostics=True)
    assert [tuple(x.shape) for x in out] == [(0, 45, 62)] * 5
    out = sfm.plane_sweep(t, poses, K, [], none, planes_of(12), diagnostics=True, smooth=(1, 2))
    assert [tuple(x.shape) for x in out] == [(0, 45, 62)] * 5
    flat = torch.zeros((5, 0, 62), dtype=torch.uint8)
    assert tuple(sfm.plane_sweep(flat, poses, K, [0], [[1]], planes_of(12), smooth=(1, 2)).shape) == (1, 0, 62)
    assert tuple(sfm.mvs_depth(flat, poses, K, m.neighbours(5), planes_of(12), smooth=(1, 2)).shape) == (5, 0, 62)
    torch.cuda.synchronize()


def test_wrapper_argument_checks(sfm, gpu, views):
    img, poses, K = views
    t = torch.from_numpy(img)
    with pytest.raises(ValueError, match="p1 <= p2"):
        sfm.plane_sweep(t, poses, K, [0], [[1]], planes_of(4), smooth=(5, 4))
    with pytest.raises(ValueError, match="16383"):
        sfm.mvs_depth(t, poses, K, m.neighbours(5), planes_of(4), smooth=(5, 16384))
    with pytest.raises(ValueError, match="paths"):
        sfm.plane_sweep(t, poses, K, [0], [[1]], planes_of(4), smooth=(1, 2, 5))
    with pytest.raises(ValueError, match="mask"):
        sfm.sgm_aggregate(torch.zeros((1, 2, 2, 3), dtype=torch.uint16), 1, 2, ("mask", 0))
    with pytest.raises(ValueError, match="256"):
        sfm.plane_sweep(t, poses, K, [0], [[1]], planes_of(257), smooth=(1, 2))
    with pytest.raises(ValueError, match="256"):
        sfm.sgm_aggregate(torch.zeros((1, 2, 2, 257), dtype=torch.uint16), 1, 2)
    with pytest.raises(ValueError, match="256"):
        sfm.volume_select(torch.zeros((1, 45, 62, 257), dtype=torch.int32), poses, K, [0], [[1]], planes_of(257))
    with pytest.raises(ValueError, match="16-bit|uint16"):
        sfm.sgm_aggregate(torch.zeros((1, 2, 2, 3), dtype=torch.int32), 1, 2)
    with pytest.raises(ValueError, match="does not match"):
        sfm.volume_select(torch.zeros((1, 45, 62, 5), dtype=torch.int32), poses, K, [0], [[1]], planes_of(4))
    with pytest.raises(ValueError, match="agg_radius"):
        sfm.cost_volume(t, poses, K, [0], [[1]], planes_of(4), agg_radius=4)
