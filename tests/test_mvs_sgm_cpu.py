"""CPU: the semi-global steps of V10 (tests/mvs_sgm_ref.py: 4a, 4b, 5' - 7' of include/sfmhip.h)
against known answers, and the argument errors of the three entry points without a GPU.  The HIP
kernels are compared with the same restatement in test_gpu_mvs_sgm.py."""
import numpy as np
import pytest

import mvs_ref as m
import mvs_sgm_ref as g

F32, I32, U32 = np.float32, np.int32, np.uint32


def path_by_definition(vol, d, p1, p2):
    """L_d pixel by pixel and plane by plane, as the header text reads."""
    H, W, P = vol.shape
    dv, du = d
    L = np.zeros((H, W, P), np.int64)
    vs = range(H) if dv >= 0 else range(H - 1, -1, -1)
    us = range(W) if du >= 0 else range(W - 1, -1, -1)
    for v in vs:
        for u in us:
            qv, qu = v - dv, u - du
            for k in range(P):
                if not (0 <= qv < H and 0 <= qu < W):
                    L[v, u, k] = vol[v, u, k]
                    continue
                q = L[qv, qu]
                mq = int(q.min())
                c = [int(q[k]), mq + p2]
                if k > 0:
                    c.append(int(q[k - 1]) + p1)
                if k < P - 1:
                    c.append(int(q[k + 1]) + p1)
                L[v, u, k] = int(vol[v, u, k]) + min(c) - mq
    return L


def test_identity_without_penalties():
    """p1 = p2 = 0: every L_d is vol, so sm = n vol and the selection is that of the unsmoothed sweep:
    k* and nv equal, best and second n times as large (INT32_MAX stays), the depth bit-equal (the
    costs scale by a power of two and stay below 2^24)."""
    img, poses, K = (np.random.default_rng(3).integers(0, 256, (3, 20, 27), dtype=np.uint8),
                     np.stack([np.eye(3, 4, dtype=F32)] * 3), np.tile(F32([[30, 30, 13.5, 10]]), (3, 1)))
    poses[1, 0, 3], poses[2, 0, 3] = -0.1, 0.1
    cen = m.census(img)
    planes = m.inverse_depth_planes(1.5, 6.0, 9)
    ref = m.plane_sweep(cen, poses, K, [0], [[1, 2]], planes, 2, 24, 256, 1)
    vol = g.cost_volume(cen, poses, K, [0], [[1, 2]], planes, 2, 24)
    assert vol.dtype == np.uint16 and np.array_equal(vol[0].transpose(2, 0, 1), m.cost_volume(
        cen, poses, K, 0, [1, 2], planes, 2, 24)[0])
    for mask, n in ((0xFF, 8), (0x0F, 4)):
        sm = g.sgm_aggregate(vol, 0, 0, mask)
        assert sm.dtype == U32 and np.array_equal(sm, n * vol.astype(U32))
        out = g.volume_select(sm, poses, K, [0], [[1, 2]], planes, 256, 1)
        assert np.array_equal(out["k"], ref["k"]) and np.array_equal(out["nv"], ref["nv"])
        assert np.array_equal(out["best"], n * ref["best"])
        assert np.array_equal(out["second"], np.where(ref["second"] == m.INT32_MAX, m.INT32_MAX, n * ref["second"]))
        assert np.array_equal(out["depth"].view(U32), ref["depth"].view(U32)) and (out["depth"] > 0).any()


def test_single_direction_by_hand():
    """1 x 4, P = 3, p1 = 1, p2 = 2, direction 0 (the predecessor is the pixel to the left):
      u = 0: L = vol = [3, 0, 5], m = 0
      u = 1: k0 min(3, 0+1, 0+2) = 1 -> 1+1 = 2; k1 min(0, 3+1, 5+1, 2) = 0 -> 4; k2 min(5, 0+1, 2) = 1 -> 2+1 = 3; m = 2
      u = 2: k0 min(2, 4+1, 2+2) - 2 = 0 -> 6; k1 min(4, 2+1, 3+1, 4) - 2 = 1 -> 2; k2 min(3, 4+1, 4) - 2 = 1 -> 1; m = 1
      u = 3: k0 min(6, 2+1, 1+2) - 1 = 2 -> 2; k1 min(2, 6+1, 1+1, 3) - 1 = 1 -> 8; k2 min(1, 2+1, 3) - 1 = 0 -> 3."""
    vol = np.array([[[3, 0, 5], [1, 4, 2], [6, 1, 0], [0, 7, 3]]], np.uint16)
    want = np.array([[[3, 0, 5], [2, 4, 3], [6, 2, 1], [2, 8, 3]]], U32)
    assert np.array_equal(g.sgm_aggregate(vol[None], 1, 2, 1 << 0)[0], want)
    # direction 1 on the mirrored image gives the mirror image
    assert np.array_equal(g.sgm_aggregate(vol[None, :, ::-1], 1, 2, 1 << 1)[0], want[:, ::-1])
    # on a single row every direction with dv != 0 has its predecessor outside: L = vol
    for b in range(2, 8):
        assert np.array_equal(g.sgm_aggregate(vol[None], 1, 2, 1 << b)[0], vol)
    # a larger p2 than any difference: the jump is never taken; p1 = 0 makes a step to a neighbour free
    assert np.array_equal(g.sgm_aggregate(vol[None], 0, 16383, 1)[0, 0, 1], [1 + 0, 4 + 0, 2 + 0])


@pytest.mark.parametrize("shape", [(4, 6, 5), (6, 4, 1), (1, 5, 2), (5, 1, 3)])
def test_paths_against_the_definition_read_literally(shape):
    rng = np.random.default_rng(sum(shape))
    for hi, p1, p2 in ((4, 1, 2), (37633, 50, 400), (37633, 0, 0), (10, 3, 3)):
        vol = rng.integers(0, hi, shape).astype(np.uint16)
        total = np.zeros(shape, np.int64)
        for b, d in enumerate(g.DIRECTIONS):
            L = g.path(vol, d, p1, p2)
            assert np.array_equal(L, path_by_definition(vol, d, p1, p2)), (d, p1, p2)
            total += L
        assert np.array_equal(g.sgm_aggregate(vol[None], p1, p2, 0xFF)[0], total)


def test_bounds_on_a_random_volume():
    rng = np.random.default_rng(8)
    vol = rng.integers(0, 37633, (9, 11, 17)).astype(np.uint16)
    for p1, p2 in ((50, 400), (0, 7), (16383, 16383)):
        for d in g.DIRECTIONS:
            L = g.path(vol, d, p1, p2)
            assert (L >= vol).all() and (L <= vol.astype(np.int64) + p2).all()
            assert (L > vol).any() or p2 == 0
    assert g.sgm_aggregate(vol[None], 16383, 16383, 0xFF).max() < 2 ** 19


def test_selection_ties_and_few_planes():
    """The smallest k of the minimum; second only from two planes away; P < 3 is all-invalid."""
    poses, K = np.eye(3, 4, dtype=F32)[None], F32([[10, 10, 1, 1]])
    sm = np.zeros((1, 1, 2, 5), U32)
    sm[0, 0, 0] = [7, 3, 3, 9, 4]
    sm[0, 0, 1] = [5, 5, 5, 5, 5]
    out = g.volume_select(sm, poses, K, [0], [[-1]], F32([1, 2, 3, 4, 5]), 256, 0)
    assert out["k"].tolist() == [[[1, 0]]] and out["best"].tolist() == [[[3, 5]]]
    assert out["second"].tolist() == [[[4, 5]]] and out["depth"][0, 0, 0] > 0 and out["depth"][0, 0, 1] == 0
    for P in (1, 2):
        out = g.volume_select(sm[..., :P], poses, K, [0], [[-1]], F32([1, 2][:P]), 256, 0)
        assert not out["depth"].any() and (out["second"] == m.INT32_MAX).all()
    bad = poses.copy()
    bad[0, 0, 0] = np.nan
    assert not any(v.any() for v in g.volume_select(sm, bad, K, [0], [[-1]], F32([1, 2, 3, 4, 5]), 256, 0).values())


def test_scene_conditions_as_committed():
    """View 2, a = 2, penalty 24, uniq 243, min_views 2, smooth (50, 400, 8 paths) for every view,
    filter eps 0.01, min_consistent 2.  The restatement gives swept completeness 0.98699, 0.99324 of
    the valid in-range pixels within 2 %, filtered completeness 0.96932 (box only: 0.92050, below
    the bound of 0.95) and 0.144 % of the filtered pixels off by more than 5 %."""
    f = g.scene_figures()
    print(f)
    g.check_smoothed_figures(f)
    box = g.scene_figures(smooth=None)
    assert box["filtered_completeness"] < 0.95, box
    with pytest.raises(AssertionError):
        g.check_smoothed_figures(box)


def test_scene_conditions_weak_texture():
    """grey' = uint8(128 + floor((grey - 128) / 32)): the restatement gives a filtered completeness
    of 0.91941 smoothed and 0.80089 box only."""
    assert g.weak_grey(np.array([0, 127, 128, 159, 160, 255], np.uint8)).tolist() == [124, 127, 128, 128, 129, 131]
    smooth, box = g.scene_figures(weak=True), g.scene_figures(weak=True, smooth=None)
    print(smooth, box)
    assert smooth["filtered_completeness"] >= 0.90, smooth
    assert box["filtered_completeness"] < 0.85, box


def test_exports_and_wrapper_spellings(sfm):
    for name in ("cost_volume", "sgm_aggregate", "volume_select"):
        assert getattr(sfm, name) is getattr(sfm.mvs, name)
    assert sfm.mvs._path_mask(8) == 0xFF and sfm.mvs._path_mask(4) == 0x0F and sfm.mvs._path_mask(("mask", 0x21)) == 0x21
    assert sfm.mvs._smooth((50, 400)) == (50, 400, 0xFF) and sfm.mvs._smooth((0, 0, 4)) == (0, 0, 0x0F)
    for bad in ((5, 4), (-1, 4), (1, 16384), (1, 2, 3), (1, 2, ("mask", 0)), (1, 2, ("mask", 256)), (1,), 7):
        with pytest.raises(ValueError):
            sfm.mvs._smooth(bad)
    assert sfm.lib.sfmhip_version() == 0x000300


def test_c_argument_checks_without_gpu(sfm):
    """Each limit is SFMHIP_E_ARG, and an empty call a no-op, without touching the GPU."""
    err = sfm.lib.sfmhip_last_error

    def volume(S=4, P=12, a=2, penalty=24, R=1, H=4, W=4, p=1):
        return sfm.lib.sfmhip_cost_volume(p, p, p, 5, H, W, p, p, R, S, p, P, a, penalty, p, None)

    for kw, word in ((dict(S=0), b"S must"), (dict(S=17), b"S must"), (dict(P=0), b"P must"), (dict(P=65536), b"P must"),
                     (dict(a=4), b"agg_radius"), (dict(penalty=49), b"penalty"), (dict(R=65536), b"reference views"),
                     (dict(H=-1), b"bad shape"), (dict(p=None), b"null pointer")):
        assert volume(**kw) == -1, kw
        assert word in err(), (kw, err())
    assert volume(R=0, p=None) == 0 and volume(H=0, p=None) == 0 and volume(W=0, p=None) == 0

    def aggregate(R=1, H=4, W=4, P=12, p1=50, p2=400, mask=0xFF, p=1):
        return sfm.lib.sfmhip_sgm_aggregate(p, R, H, W, P, p1, p2, mask, p, None)

    for kw, word in ((dict(P=257), b"P must"), (dict(P=0), b"P must"), (dict(p1=401), b"p1 <= p2"),
                     (dict(p1=-1), b"p1 <= p2"), (dict(p1=16384, p2=16384), b"p1 <= p2"), (dict(p2=16384), b"p1 <= p2"),
                     (dict(mask=0), b"path_mask"), (dict(mask=256), b"path_mask"), (dict(R=65536), b"reference views"),
                     (dict(W=-1), b"bad shape"), (dict(p=None), b"null pointer")):
        assert aggregate(**kw) == -1, kw
        assert word in err(), (kw, err())
    assert aggregate(R=0, p=None) == 0 and aggregate(H=0, p=None) == 0 and aggregate(W=0, p=None) == 0

    def select(S=4, P=12, uniq=243, min_views=2, R=1, H=4, W=4, p=1):
        return sfm.lib.sfmhip_volume_select(p, p, p, 5, H, W, p, p, R, S, p, P, uniq, min_views, p, None, None, None,
                                            None, None)

    for kw, word in ((dict(P=257), b"P must"), (dict(P=0), b"P must"), (dict(S=0), b"S must"), (dict(uniq=257), b"uniq"),
                     (dict(min_views=-1), b"min_views"), (dict(R=65536), b"reference views"),
                     (dict(H=1 << 20), b"2^31"), (dict(p=None), b"null pointer")):
        assert select(**kw) == -1, kw
        assert word in err(), (kw, err())
    assert select(R=0, p=None) == 0 and select(H=0, p=None) == 0 and select(W=0, p=None) == 0
