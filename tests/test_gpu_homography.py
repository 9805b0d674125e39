"""GPU parity: sfmhip_find_homography and sfmhip_pair_stats (homography.hip) against the restatement
in tests/homog_ref.py, on its table of admissible scenes.

The bar per scene: the mask byte-equal, n_inliers and iters equal, H within 1e-7 relative Frobenius
norm (admissibility pins the outcome up to 1e-8 model differences; the margin of ten covers the
refit's conditioning), and two runs the same bytes.  The restatement of each scene is computed once
(homog_ref.h_run) and shared."""
import ctypes

import numpy as np
import pytest
import torch

import homog_ref as hr

H_TOL = 1e-7
# P = 70: every scene of the table in turn, with an empty and a three-point pair in the middle
BATCH_70 = [hr.H_NAMES[k % len(hr.H_NAMES)] for k in range(70)]
BATCH_70[34], BATCH_70[35] = "n-0", "n-3"


def _run(sfm, names, **kw):
    v = sfm.verify
    a, b, of = v.pack_pairs([hr.h_scene(n)["src"] for n in names], [hr.h_scene(n)["dst"] for n in names])
    r = v.find_homography_batched(a, b, of, **kw)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in r.items()}, of.cpu().numpy()


def _check(names, r, offs):
    for p, name in enumerate(names):
        tr = hr.h_run(name)
        mask = r["mask"][offs[p]:offs[p + 1]]
        print(name, "ok", r["ok"][p], tr["ok"], "iters", r["iters"][p], tr["iters"], "inliers", r["n_inliers"][p],
              tr["n_inliers"], "mask diff", int((mask != tr["mask"]).sum()),
              "H", hr.rel_fro(r["H"][p], tr["H"]) if tr["ok"] and r["ok"][p] else None)
        assert int(r["ok"][p]) == tr["ok"], name
        assert int(r["iters"][p]) == tr["iters"], name
        assert int(r["n_inliers"][p]) == tr["n_inliers"], name
        assert mask.dtype == np.uint8 and np.array_equal(mask, tr["mask"]), name
        if tr["ok"]:
            assert r["H"][p][2, 2] == 1.0
            assert hr.rel_fro(r["H"][p], tr["H"]) <= H_TOL, name
        else:
            assert not r["H"][p].any(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", hr.H_NAMES)
def test_scene_matches_restatement_alone(sfm, gpu, name):
    """P = 1."""
    r, offs = _run(sfm, [name])
    _check([name], r, offs)


@pytest.mark.gpu
def test_pairs_of_two(sfm, gpu):
    """P = 2: a pair after an empty one, and two pairs past one scoring block."""
    for names in (["n-0", "planar"], ["n-2500", "n-1025"]):
        r, offs = _run(sfm, names)
        _check(names, r, offs)


@pytest.mark.gpu
def test_ragged_batch_of_70_and_same_bytes_twice(sfm, gpu):
    r, offs = _run(sfm, BATCH_70)
    assert np.diff(offs)[34] == 0 and np.diff(offs)[35] == 3 and len(set(np.diff(offs))) > 10
    _check(BATCH_70, r, offs)
    r2, _ = _run(sfm, BATCH_70)
    for k in r:
        assert r[k].tobytes() == r2[k].tobytes(), k


@pytest.mark.gpu
def test_cv2_signature(sfm, gpu):
    sc, tr = hr.h_scene("planar"), hr.h_run("planar")
    H, mask = sfm.findHomography(sc["src"], sc["dst"], sfm.RANSAC, 3.0)
    assert H.shape == (3, 3) and mask.shape == (len(sc["src"]), 1) and mask.dtype == np.uint8
    assert np.array_equal(mask.ravel(), tr["mask"]) and hr.rel_fro(H, tr["H"]) <= H_TOL
    sc = hr.h_scene("collinear")
    assert sfm.findHomography(sc["src"], sc["dst"]) == (None, None)
    with pytest.raises(NotImplementedError):
        sfm.findHomography(sc["src"], sc["dst"], method=4)
    # other parameters reach the kernel: a tight threshold and few iterations, against the restatement
    sc = hr.h_scene("dominant-plane")
    tr = hr.find_homography(sc["src"], sc["dst"], threshold=1.5, max_iters=40, confidence=0.9)
    H, mask = sfm.findHomography(sc["src"], sc["dst"], sfm.RANSAC, 1.5, maxIters=40, confidence=0.9)
    assert np.array_equal(mask.ravel(), tr["mask"]) and hr.rel_fro(H, tr["H"]) <= H_TOL


# ---------------------------------------------------------------------------------------------
# sfmhip_pair_stats

def _stats_case(n, seed, all_masked=False):
    rng = np.random.default_rng(seed)
    W, H = hr.TV_SIZE
    p0 = rng.uniform(-100, 1400, (n, 2))
    p1 = rng.uniform(-100, 1100, (n, 2))
    p0[0] = (W, 10.0)                       # exactly on the edge x = W: ignored
    p1[0] = (W - 0.5, H - 0.5)              # the last cell
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    mask[0] = 1
    if all_masked:
        mask[:] = 0
    from oracle import geometry as og
    return p0, p1, mask, og.rodrigues(rng.normal(0, 0.1, 3))


@pytest.mark.gpu
def test_pair_stats_matches_numpy(sfm, gpu):
    v = sfm.verify
    cases = [_stats_case(1, 1), _stats_case(64, 2), _stats_case(65, 3), _stats_case(300, 4, all_masked=True),
             _stats_case(1000, 5)]
    K = hr.TV_K
    cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    a, b, of = v.pack_pairs([c[0] for c in cases], [c[1] for c in cases])
    mask = np.concatenate([c[2] for c in cases])
    R = np.stack([c[3] for c in cases])
    r = v.pair_stats_batched(a, b, of, mask, R, v._cam(K), hr.TV_SIZE)
    torch.cuda.synchronize()
    offs = of.cpu().numpy()
    cos = r["cosang"].cpu().numpy()
    cover = r["cover"].cpu().numpy().view(np.uint64)
    med = r["median"].cpu().numpy()
    for p, (p0, p1, m, Rp) in enumerate(cases):
        st = hr.pair_stats(p0, p1, m, Rp, cam, *hr.TV_SIZE)
        c = cos[offs[p]:offs[p + 1]]
        assert np.abs(c - st["cosang"]).max() <= 1e-12, p
        assert np.array_equal(c == 2.0, m == 0)
        assert (int(cover[p, 0]), int(cover[p, 1])) == st["cover"], p
        assert int(r["n_sel"][p]) == st["n_sel"]
        # an exact order statistic of the device's own values: np.partition of them, bit for bit
        k = (st["n_sel"] - 1) // 2 if st["n_sel"] else 0
        want = np.float32(np.partition(c, k)[k])
        assert med[p].tobytes() == want.tobytes(), (p, med[p], want)
    assert int(cover[0, 0]) == 0 and int(cover[0, 1]) == 1 << 63       # the edge point, the last cell
    assert int(cover[3, 0]) == 0 and int(cover[3, 1]) == 0 and med[3] == np.float32(2.0)


# ---------------------------------------------------------------------------------------------
# argument errors, reported without touching the GPU

def test_argument_errors_without_gpu(sfm):
    lib = sfm.lib
    d = ctypes.c_double
    assert lib.sfmhip_find_homography(None, None, None, 1, d(3.0), d(0.995), 2000, None, None, None, None, None,
                                      None) == -1
    assert b"null pointer" in lib.sfmhip_last_error()
    assert lib.sfmhip_find_homography(None, None, None, -1, d(3.0), d(0.995), 2000, None, None, None, None, None,
                                      None) == -1
    assert b"n_pairs < 0" in lib.sfmhip_last_error()
    assert lib.sfmhip_find_homography(None, None, None, 0, d(3.0), d(0.995), 2000, None, None, None, None, None,
                                      None) == 0
    assert lib.sfmhip_pair_stats(None, None, None, 1, 0, None, None, None, d(640.0), d(480.0), None, None, None, None,
                                 None, None, None) == -1
    assert b"null pointer" in lib.sfmhip_last_error()
    assert lib.sfmhip_pair_stats(None, None, None, -1, 0, None, None, None, d(640.0), d(480.0), None, None, None,
                                 None, None, None, None) == -1
    assert lib.sfmhip_pair_stats(None, None, None, 0, 0, None, None, None, d(640.0), d(480.0), None, None, None, None,
                                 None, None, None) == 0
