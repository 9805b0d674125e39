"""CPU: the numpy restatement of V12 (tests/undistort_ref.py) against known answers: exact copies
and shifts, the map against a longdouble evaluation, optimal_new_K, and the MVS test scene
rendered through the radial model, with and without the resampling."""
from importlib import import_module

import numpy as np
import pytest

import ba_calib_ref
import mvs_ref
import undistort_ref as ur

K0 = (60.0, 61.8, 25.3, 19.1)
H0, W0 = 37, 53
CASES = [(cam, size, co) for cam, size in ur.CAMERAS for co in ur.COEFFS]


def images(C, seed=0, V=2, H=H0, W=W0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (V, H, W) if C == 1 else (V, H, W, C), dtype=np.uint8)


def cams(V, K=K0, dist=(0.0, 0.0), new_K=None):
    cs = np.tile(np.array(list(K) + list(dist), np.float64), (V, 1))
    cd = np.tile(np.array(K if new_K is None else new_K, np.float64), (V, 1))
    return cs, cd


@pytest.mark.parametrize("C", [1, 3, 4])
def test_identity(C):
    img = images(C)
    out, mask = ur.undistort_u8(img, *cams(2), H0, W0)
    assert np.array_equal(out, img) and (mask == 1).all()
    depth = np.random.default_rng(1).random((2, H0, W0), dtype=np.float32)
    assert np.array_equal(ur.undistort_f32(depth, *cams(2), H0, W0), depth)


@pytest.mark.parametrize("C", [1, 3])
def test_integer_shift(C):
    """ox = cx - 3, oy = cy + 2: output (u, v) reads source (u + 3, v - 2)."""
    img = images(C)
    fx, fy, cx, cy = K0
    out, mask = ur.undistort_u8(img, *cams(2, new_K=(fx, fy, cx - 3, cy + 2)), H0, W0)
    want = np.zeros_like(img)
    want[:, 2:, :W0 - 3] = img[:, :H0 - 2, 3:]
    covered = np.zeros((2, H0, W0), np.uint8)
    covered[:, 2:, :W0 - 3] = 1
    assert np.array_equal(out, want) and np.array_equal(mask, covered)


def test_half_pixel_shift():
    """ox = cx - 0.5: (p[x] + p[x + 1] + 1) >> 1, exactly; the last column falls outside."""
    img = images(1)
    fx, fy, cx, cy = K0
    out, mask = ur.undistort_u8(img, *cams(2, new_K=(fx, fy, cx - 0.5, cy)), H0, W0)
    p = img.astype(np.int32)
    assert np.array_equal(out[:, :, :-1], ((p[:, :, :-1] + p[:, :, 1:] + 1) >> 1).astype(np.uint8))
    assert (mask[:, :, :-1] == 1).all() and (mask[:, :, -1] == 0).all() and (out[:, :, -1] == 0).all()


def test_zero_distortion_scene_is_the_pinhole_scene():
    syn = import_module("3d_reconstruction_amd.synthetic")
    a = syn.mvs_scene(24, 32, 27.5, 16.0, 12.0, n_views=2)
    b = syn.mvs_scene(24, 32, 27.5, 16.0, 12.0, n_views=2, dist=(0.0, 0.0))
    for x, y in zip(a, b):
        assert np.array_equal(x.numpy(), y.numpy())


def test_map_accuracy():
    """The f64 chain of the map against ba_calib_ref.distort_points in longdouble, new_K = K, over
    the two cameras and four coefficient pairs.  The chain has 10 roundings on the way to a
    coordinate of at most max(W, H) in magnitude, each a relative 2^-53 of an intermediate of at
    most that size: bound 16 * 2^-53 * max(W, H) (4.5e-13 px at 256).
    Measured worst |error|: 7.6e-14 px (0.17 of the bound); X, Y differ from the rounded
    longdouble map by at most 1 unit (measured: 1, where sx 256 + 0.5 sits on an integer)."""
    worst = worst_rel = worst_unit = 0.0
    for cam, (W, H), co in CASES:
        sx, sy, _ = ur.source_coords(list(cam) + list(co), cam, H, W)
        u, v = np.meshgrid(np.arange(W), np.arange(H))
        ref = ba_calib_ref.distort_points(np.stack([u.ravel(), v.ravel()], 1), ur.K3(cam), co, dt=np.longdouble)
        rx, ry = ref[:, 0].reshape(H, W), ref[:, 1].reshape(H, W)
        err = float(max(np.abs(sx - rx).max(), np.abs(sy - ry).max()))
        bound = 16 * 2.0 ** -53 * max(W, H)
        worst, worst_rel = max(worst, err), max(worst_rel, err / bound)
        assert err <= bound, (cam, co, err, bound)
        X, Y, valid = ur.view_map(list(cam) + list(co), cam, H, W, H, W)
        RX, RY = np.floor(rx * 256 + np.longdouble(0.5)), np.floor(ry * 256 + np.longdouble(0.5))
        unit = float(max(np.abs(X - RX)[valid].max(), np.abs(Y - RY)[valid].max()))
        worst_unit = max(worst_unit, unit)
        assert unit <= 1
    print(f"map accuracy: worst |error| {worst:.3g} px, {worst_rel:.3g} of the bound; worst unit difference "
          f"{worst_unit}")


@pytest.mark.parametrize("cam,size,co", CASES)
def test_optimal_new_K(cam, size, co):
    W, H = size
    cs = list(cam) + list(co)
    inner = ur.optimal_new_K(cam, co, size, 0.0)
    assert ur.view_map(cs, inner, H, W, H, W)[2].all()                   # alpha 0: every output pixel is valid
    outer = ur.optimal_new_K(cam, co, size, 1.0)
    pts = np.array([(u, v) for u in (0, (W - 1) / 2, W - 1) for v in (0, (H - 1) / 2, H - 1)
                    if (u, v) != ((W - 1) / 2, (H - 1) / 2)], np.float64)
    q = ba_calib_ref.undistort_points(pts, ur.K3(cam), co)
    un = (q[:, 0] - cam[2]) / cam[0] * outer[0] + outer[2]
    vn = (q[:, 1] - cam[3]) / cam[1] * outer[1] + outer[3]
    tol = 1e-9                                                            # f64 rounding at <= 256 px is 1e-13
    assert (un >= -tol).all() and (un <= W - 1 + tol).all() and (vn >= -tol).all() and (vn <= H - 1 + tol).all()
    # with the same K: pincushion leaves part of the frame invalid, barrel none
    invalid = 1.0 - ur.view_map(cs, cam, H, W, H, W)[2].mean()
    if co[0] > 0:
        assert 0.07 <= invalid <= 0.14, invalid
    else:
        assert invalid == 0.0
    # another output size keeps the property
    small = ur.optimal_new_K(cam, co, size, 0.0, new_size=(W - 12, H - 8))
    assert ur.view_map(cs, small, H, W, H - 8, W - 12)[2].all()


def test_skip_rule_and_fold_over():
    cs, cd = cams(3, dist=(-0.12, 0.03))
    img = images(1, V=3)
    good = ur.undistort_u8(img, cs, cd, H0, W0)
    for row, col, val in ((0, 4, np.nan), (1, 2, 2.0 ** 60), (2, 0, 0.0)):
        bad = cs.copy()
        bad[row, col] = val
        out, mask = ur.undistort_u8(img, bad, cd, H0, W0)
        keep = [i for i in range(3) if i != row]
        assert not out[row].any() and not mask[row].any()
        assert np.array_equal(out[keep], good[0][keep]) and np.array_equal(mask[keep], good[1][keep])
    wide = (12.0, 12.0, 25.3, 19.1)
    cs, cd = cams(1, dist=(-0.6, 0.0), new_K=wide)
    sx, sy, mono = ur.source_coords(cs[0], cd[0], H0, W0)
    m = ur.undistort_map(cs, cd, H0, W0, H0, W0)[0]
    assert (mono <= 0).any() and (mono > 0).any()
    assert (m[mono <= 0] == -1).all()


def test_distorted_scene_needs_the_resampling():
    """The MVS test scene rendered through (-0.12, 0.03): taken as pinhole images it misses the
    scene's known answer; resampled by the restatement it meets every condition of it.  Truth is
    the pinhole depth of mvs_ref.scene()."""
    raw = ur.scene_distorted()["grey"]
    sw, filt = ur.scene_depths(raw)
    with pytest.raises(AssertionError):
        mvs_ref.check_scene_figures(mvs_ref.scene_figures(sw["depth"][2], filt[2]))
    und = ur.scene_undistorted()
    assert (und["mask"] == 1).all()                                      # barrel: the same K covers the frame
    f = mvs_ref.scene_figures(und["swept"]["depth"][2], und["filtered"][2])
    print(f)
    mvs_ref.check_scene_figures(f)
