"""GPU: V12 (undistort.hip through rectify.py) bit for bit against its numpy restatement
(tests/undistort_ref.py), and the distorted MVS scene from images to a mesh."""
import numpy as np
import pytest
import torch

import mvs_ref
import undistort_ref as ur

pytestmark = pytest.mark.gpu

H0, W0 = 37, 53
# barrel, pincushion and no distortion in one call, three different cameras
KS = np.array([[60.0, 61.8, 25.3, 19.1], [58.0, 57.0, 27.9, 17.2], [64.5, 63.0, 26.0, 18.5]])
DS = np.array([[-0.12, 0.03], [0.25, -0.05], [0.0, 0.0]])
CS = np.concatenate([KS, DS], 1)
# output sizes (W', H'): the input's, a smaller one, and one pixel more and one less than the
# kernel's tile, which is 256 consecutive pixels of one output row
SIZES = [None, (41, 29), (257, 5), (255, 3)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def images(C, V=3, H=H0, W=W0, seed=0):
    rng = np.random.default_rng(seed + C)
    return rng.integers(0, 256, (V, H, W) if C == 1 else (V, H, W, C), dtype=np.uint8)


def new_cams(size):
    """The output cameras of a size: the source K scaled to the output frame."""
    if size is None:
        return KS.copy()
    sx, sy = (size[0] - 1) / (W0 - 1), (size[1] - 1) / (H0 - 1)
    return KS * np.array([sx, sy, sx, sy])


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_images_and_masks_bit_equal(sfm, gpu, C, size):
    img = images(C)
    Wo, Ho = size or (W0, H0)
    nk = new_cams(size)
    out, mask = sfm.undistort_images(torch.from_numpy(img).to(gpu), KS, DS, nk, size)
    want, wmask = ur.undistort_u8(img, CS, nk, Ho, Wo)
    assert out.dtype == torch.uint8 and out.is_cuda and mask.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(mask.cpu().numpy(), wmask)
    assert 0 < wmask[1].mean() < 1 and wmask[0].all()            # the pincushion view has both kinds of pixel


@pytest.mark.parametrize("size", SIZES)
def test_map_and_depth_bit_equal(sfm, gpu, size):
    Wo, Ho = size or (W0, H0)
    nk = new_cams(size)
    got = sfm.undistort_map(KS, DS, (W0, H0), nk, size)
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, Ho, Wo, 2)
    assert np.array_equal(got.cpu().numpy(), ur.undistort_map(CS, nk, H0, W0, Ho, Wo))
    rng = np.random.default_rng(5)
    depth = (rng.random((3, H0, W0), dtype=np.float32) * 4 + 0.5).astype(np.float32)
    depth[rng.random((3, H0, W0)) < 0.2] = 0
    depth[0, 18, 26] = np.float32(np.nan)
    out = sfm.undistort_depth(depth, KS, DS, nk, size)
    want = ur.undistort_f32(depth, CS, nk, Ho, Wo)
    assert np.isnan(want).any()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


@pytest.mark.parametrize("shape", [(1, 1), (1, 53), (37, 1)])
def test_degenerate_sources(sfm, gpu, shape):
    """One row or column: x1 / y1 clamp to the only one there is."""
    H, W = shape
    # a side of one pixel is hit only within 1/512 px of its centre: the principal point sits
    # 0.001 px off it, and the output's central row or column looks straight at it
    K = np.array([[9.0, 9.0, 0.001 if W == 1 else (W - 1) / 2 + 0.3, 0.001 if H == 1 else (H - 1) / 2 - 0.2]] * 3)
    cs = np.concatenate([K, DS], 1)
    for size in ((W, H), (7, 5)):
        nk = K.copy()
        nk[:, 2:] = [(size[0] - 1) / 2, (size[1] - 1) / 2]
        for C in (1, 3):
            img = images(C, H=H, W=W)
            out, mask = sfm.undistort_images(img, K, DS, nk, size)
            want, wmask = ur.undistort_u8(img, cs, nk, size[1], size[0])
            assert wmask.any()
            assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(mask.cpu().numpy(), wmask)
        depth = np.random.default_rng(2).random((3, H, W), dtype=np.float32) + 1
        got = sfm.undistort_depth(depth, K, DS, nk, size)
        want = ur.undistort_f32(depth, cs, nk, size[1], size[0])
        assert want.any() and np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_empty_calls(sfm, gpu):
    out, mask = sfm.undistort_images(np.zeros((0, H0, W0, 3), np.uint8), np.zeros((0, 4)), np.zeros((0, 2)))
    assert tuple(out.shape) == (0, H0, W0, 3) and tuple(mask.shape) == (0, H0, W0)
    out, mask = sfm.undistort_images(np.zeros((3, 0, W0), np.uint8), KS, DS, size=(4, 5))
    assert tuple(out.shape) == (3, 5, 4) and not out.any() and not mask.any()
    out, mask = sfm.undistort_images(images(3), KS, DS, size=(0, 5))
    assert tuple(out.shape) == (3, 5, 0, 3) and tuple(mask.shape) == (3, 5, 0)
    assert tuple(sfm.undistort_depth(np.zeros((3, H0, 0), np.float32), KS, DS).shape) == (3, H0, 0)
    assert tuple(sfm.undistort_depth(np.zeros((3, H0, W0), np.float32), KS, DS, size=(6, 0)).shape) == (3, 0, 6)
    assert tuple(sfm.undistort_map(KS, DS, (W0, H0), new_size=(0, 3)).shape) == (3, 3, 0, 2)
    assert tuple(sfm.undistort_map(np.zeros((0, 4)), np.zeros((0, 2)), (W0, H0)).shape) == (0, H0, W0, 2)
    torch.cuda.synchronize()


def test_fold_over(sfm, gpu):
    """k1 = -0.6 under a wide new_K: r d(r) turns back inside the output frame; the mask is 0
    wherever mono <= 0, although such points map into the source frame again."""
    K, dist, wide = KS[0], (-0.6, 0.0), (12.0, 12.0, 25.3, 19.1)
    cs = np.array(list(K) + list(dist))
    _, _, mono = ur.source_coords(cs, wide, H0, W0)
    assert (mono <= 0).any() and (mono > 0).any()
    img = images(1, V=1)
    out, mask = sfm.undistort_images(img, K, dist, wide)
    want, wmask = ur.undistort_u8(img, cs[None], np.array([wide]), H0, W0)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(mask.cpu().numpy(), wmask)
    assert not mask.cpu().numpy()[0][mono <= 0].any() and wmask.any()


@pytest.mark.parametrize("row,col,val", [(0, 3, np.nan), (1, 1, 2.0 ** 60), (2, 0, 0.0)])
def test_skip_rule(sfm, gpu, row, col, val):
    img = images(3)
    good, gmask = sfm.undistort_images(img, KS, DS)
    K = KS.copy()
    K[row, col] = val
    depth = np.random.default_rng(3).random((3, H0, W0), dtype=np.float32) + 1
    for kw in (dict(K=K, new_K=KS), dict(K=KS, new_K=K)):          # in the source camera, in the output camera
        out, mask = sfm.undistort_images(img, kw["K"], DS, kw["new_K"])
        keep = [i for i in range(3) if i != row]
        assert not out[row].any() and not mask[row].any()
        assert torch.equal(out[keep], good[keep]) and torch.equal(mask[keep], gmask[keep])
        cs = np.concatenate([kw["K"], DS], 1)
        assert np.array_equal(out.cpu().numpy(), ur.undistort_u8(img, cs, kw["new_K"], H0, W0)[0])
        d = sfm.undistort_depth(depth, kw["K"], DS, kw["new_K"])
        assert not d[row].any()
        assert np.array_equal(bits(d.cpu().numpy()), bits(ur.undistort_f32(depth, cs, kw["new_K"], H0, W0)))
        assert (sfm.undistort_map(kw["K"], DS, (W0, H0), kw["new_K"])[row] == -1).all()


def test_two_runs_give_the_same_bytes(sfm, gpu):
    img = torch.from_numpy(images(3)).to(gpu)
    a, b = sfm.undistort_images(img, KS, DS, size=(257, 5)), sfm.undistort_images(img, KS, DS, size=(257, 5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_input_handling(sfm, gpu):
    img = images(3)
    want, wmask = sfm.undistort_images(torch.from_numpy(img).to(gpu), KS, DS)
    wide = np.zeros((3, H0, 2 * W0, 3), np.uint8)
    wide[:, :, ::2] = img
    strided = torch.from_numpy(wide).to(gpu)[:, :, ::2]
    assert not strided.is_contiguous()
    for x in (strided, img, torch.from_numpy(img)):                # non-contiguous, numpy, CPU tensor
        out, mask = sfm.undistort_images(x, KS, DS)
        assert torch.equal(out, want) and torch.equal(mask, wmask)
    K33 = np.zeros((3, 3, 3))
    K33[:, 0, 0], K33[:, 1, 1], K33[:, 0, 2], K33[:, 1, 2], K33[:, 2, 2] = KS[:, 0], KS[:, 1], KS[:, 2], KS[:, 3], 1
    assert torch.equal(sfm.undistort_images(img, K33, DS)[0], want)
    one = sfm.undistort_images(img, KS[0], [0.25, -0.05, 0, 0, 0])[0]   # one camera and a cv2 vector for all views
    assert torch.equal(one, sfm.undistort_images(img, np.tile(KS[0], (3, 1)), np.tile([0.25, -0.05], (3, 1)))[0])
    skew = K33.copy()
    skew[1, 0, 1] = 0.1
    with pytest.raises(ValueError):
        sfm.undistort_images(img.astype(np.float32), KS, DS)
    with pytest.raises(ValueError):
        sfm.undistort_depth(np.zeros((3, H0, W0), np.float64), KS, DS)
    with pytest.raises(ValueError):
        sfm.undistort_images(img, skew, DS)
    with pytest.raises(NotImplementedError):
        sfm.undistort_images(img, KS, [0.1, 0.0, 1e-3, 0.0])
    with pytest.raises(ValueError):
        sfm.undistort_images(img, KS[:2], DS)
    with pytest.raises(ValueError):
        sfm.undistort_images(img, KS, DS[:2])
    with pytest.raises(ValueError):
        sfm.undistort_images(img[..., :2], KS, DS)
    with pytest.raises(ValueError):
        sfm.optimal_new_K(KS, DS[0], (W0, H0))


@pytest.mark.parametrize("cam,size,co", [(cam, size, co) for cam, size in ur.CAMERAS for co in ur.COEFFS])
def test_optimal_new_K_on_the_device(sfm, gpu, cam, size, co):
    W, H = size
    nk = sfm.optimal_new_K(cam, co, size, 0.0)
    assert nk.dtype == np.float64 and nk.shape == (4,)
    assert np.array_equal(nk, ur.optimal_new_K(cam, co, size, 0.0))
    img = images(1, V=1, H=H, W=W)
    out, mask = sfm.undistort_images(img, cam, co, nk)
    assert bool((mask == 1).all())
    assert np.array_equal(out.cpu().numpy(), ur.undistort_u8(img, np.array([list(cam) + list(co)]), nk[None], H, W)[0])
    outer = sfm.optimal_new_K(cam, co, size, 1.0, new_size=(W + 6, H + 4))
    assert np.array_equal(outer, ur.optimal_new_K(cam, co, size, 1.0, new_size=(W + 6, H + 4)))


def test_distorted_scene_end_to_end(sfm, gpu):
    """Distorted images -> mvs_depth(dist=) -> TSDF -> mesh."""
    sc, und = ur.scene_distorted(), ur.scene_undistorted()
    grey = torch.from_numpy(np.array(sc["grey"])).to(gpu)
    args = (sc["poses"], sc["K"], sc["lists"], sc["planes"])
    depth = sfm.mvs_depth(grey, *args, dist=ur.DIST)
    img, mask = sfm.undistort_images(grey, sc["K"], ur.DIST)
    assert np.array_equal(img.cpu().numpy(), und["grey"]) and np.array_equal(mask.cpu().numpy(), und["mask"])
    assert torch.equal(depth.view(torch.int32), sfm.mvs_depth(img, *args).view(torch.int32))
    assert np.array_equal(bits(depth.cpu().numpy()), bits(und["filtered"]))
    swept = sfm.plane_sweep(img, sc["poses"], sc["K"], [2], [sc["lists"][2]], sc["planes"])
    assert np.array_equal(bits(swept[0].cpu().numpy()), bits(und["swept"]["depth"][2]))
    f = mvs_ref.scene_figures(swept[0].cpu().numpy(), depth[2].cpu().numpy())
    print(f)
    mvs_ref.check_scene_figures(f)
    raw = sfm.mvs_depth(grey, *args)                                # the same images taken as pinhole images
    raw_swept = sfm.plane_sweep(grey, sc["poses"], sc["K"], [2], [sc["lists"][2]], sc["planes"])
    with pytest.raises(AssertionError):
        mvs_ref.check_scene_figures(mvs_ref.scene_figures(raw_swept[0].cpu().numpy(), raw[2].cpu().numpy()))
    res = 64
    T = torch.zeros((res, res, res), dtype=torch.float32, device=gpu)
    Wt = torch.zeros_like(T)
    box = ((-1.0,) * 3, (1.0,) * 3)
    sfm.tsdf_integrate(T, Wt, depth, torch.from_numpy(sc["poses"]).to(gpu), torch.from_numpy(sc["K"]).to(gpu), box[0],
                       box[1], 3 * 2.0 / (res - 1))
    verts, _, faces = sfm.tsdf_extract_surface(T, Wt, box[0], box[1])
    assert verts.shape[0] > 0 and faces.shape[0] > 0
