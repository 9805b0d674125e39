"""GPU parity: §8f row 2 geometric verification (findEssentialMat RANSAC +
recoverPose, HIP f64) vs the OpenCV restatement in oracle/ransac.py.

Parity is unpinned against OpenCV itself (cv2 absent); against the oracle the
bar is: identical iteration count, inlier count and inlier mask (integer
work), E equal up to sign to 1e-8 (the two sides use different root finders
and null-space bases for the 5-point polynomial: Sturm-free derivative
isolation + Newton on the GPU, LAPACK eigenvalues in numpy), R/t to 1e-8."""
import importlib

import numpy as np
import pytest
import torch

from oracle import ransac as orc

pytestmark = pytest.mark.gpu
syn = importlib.import_module("3d_reconstruction_amd.synthetic")
E_TOL = 1e-8


def _same_up_to_sign(a, b, tol):
    return min(np.abs(a - b).max(), np.abs(a + b).max()) <= tol


@pytest.fixture(scope="module")
def scene():
    return syn.two_view_pairs(6, [300, 1000, 64, 2048, 9, 500], outlier_frac=0.3, seed=6)


def test_find_essential_matches_oracle(sfm, gpu, scene):
    for p in range(len(scene["pts0"])):
        a, b = scene["pts0"][p], scene["pts1"][p]
        E, mask = sfm.verify.findEssentialMat(a, b, scene["K"], sfm.verify.RANSAC, 0.999, 1.0)
        Eo, mo, ito = orc.find_essential_mat(a, b, scene["K"], 0.999, 1.0, return_iters=True)
        assert E.shape == (3, 3) and mask.shape == (len(a), 1) and mask.dtype == np.uint8
        assert np.array_equal(mask, mo), p
        assert _same_up_to_sign(E, Eo, E_TOL), (p, E, Eo)


def test_batched_equals_single_and_iters(sfm, gpu, scene):
    v = sfm.verify
    a, b, of = v.pack_pairs(scene["pts0"], scene["pts1"])
    r = v.find_essential_batched(a, b, of, v._cam(scene["K"]))
    offs = of.cpu().numpy()
    mask = r["mask"].cpu().numpy()
    for p in range(len(scene["pts0"])):
        Eo, mo, ito = orc.find_essential_mat(scene["pts0"][p], scene["pts1"][p], scene["K"], return_iters=True)
        assert int(r["iters"][p]) == ito
        assert int(r["n_inliers"][p]) == int(mo.sum())
        assert np.array_equal(mask[offs[p]:offs[p + 1]], mo.ravel())
        assert _same_up_to_sign(r["E"][p, 0].cpu().numpy().reshape(3, 3), Eo, E_TOL)


def test_recover_pose_matches_oracle_and_truth(sfm, gpu, scene):
    for p in (0, 1, 3, 5):
        a, b = scene["pts0"][p], scene["pts1"][p]
        Eo, mo = orc.find_essential_mat(a, b, scene["K"])
        keep = mo.ravel() > 0
        ng, R, t, m = sfm.verify.recoverPose(Eo, a[keep], b[keep], scene["K"])
        ngo, Ro, to, mko = orc.recover_pose(Eo, a[keep], b[keep], scene["K"])
        assert ng == ngo and np.array_equal(m, mko)
        np.testing.assert_allclose(R, Ro, atol=1e-8)
        np.testing.assert_allclose(t, to, atol=1e-8)
        # vs ground truth: rotation within noise, translation direction
        assert np.abs(R - scene["R"][p]).max() < 0.02
        tt = scene["t"][p] / np.linalg.norm(scene["t"][p])
        assert np.abs(t.ravel() - tt).max() < 0.02
        # the masked form == the compacted call (what matching.py does)
        ng2, R2, t2, m2 = sfm.verify.recoverPose(Eo, a, b, scene["K"], mask=mo)
        assert ng2 == ng and np.array_equal(m2[keep], m) and not m2[~keep].any()


def test_noise_free_recovers_exact_pose(sfm, gpu):
    s = syn.two_view_pairs(2, 400, outlier_frac=0.25, noise_px=0.0, seed=9)
    for p in range(2):
        a = s["pts0"][p].astype(np.float64)
        b = s["pts1"][p].astype(np.float64)
        E, mask = sfm.verify.findEssentialMat(a, b, s["K"])
        inl = s["inlier"][p]
        assert (mask.ravel()[inl] == 1).all()          # every true inlier kept (f32 rounding << 1 px)
        assert mask.sum() <= inl.sum() + 3              # outliers landing within 1 px of their epipolar line
        ng, R, t, _ = sfm.verify.recoverPose(E, a[mask.ravel() > 0], b[mask.ravel() > 0], s["K"])
        assert np.abs(R - s["R"][p]).max() < 1e-4
        tt = s["t"][p] / np.linalg.norm(s["t"][p])
        assert np.abs(t.ravel() - tt).max() < 1e-4


def test_edge_cases(sfm, gpu, scene):
    v = sfm.verify
    a, b = scene["pts0"][1], scene["pts1"][1]
    assert v.findEssentialMat(a[:4], b[:4], scene["K"]) == (None, None)     # count < 5
    E5, m5 = v.findEssentialMat(a[:5], b[:5], scene["K"])                   # count == 5: all models
    Eo5, mo5 = orc.find_essential_mat(a[:5], b[:5], scene["K"])
    assert E5.shape == Eo5.shape and (m5 == 1).all() and np.array_equal(m5, mo5)
    for k in range(E5.shape[0] // 3):
        assert _same_up_to_sign(E5[3 * k:3 * k + 3], Eo5[3 * k:3 * k + 3], E_TOL)
    # pure outliers: either no model or one that agrees with the oracle
    rng = np.random.default_rng(3)
    ra = rng.uniform(-900, 900, (200, 2)).astype(np.float32)
    rb = rng.uniform(-900, 900, (200, 2)).astype(np.float32)
    E, m = v.findEssentialMat(ra, rb, scene["K"])
    Eo, mo = orc.find_essential_mat(ra, rb, scene["K"])
    assert (E is None) == (Eo is None)
    if E is not None:
        assert np.array_equal(m, mo)
    with pytest.raises(NotImplementedError):
        v.findEssentialMat(a, b, scene["K"], method=4)


def test_essential_inliers_is_matching_py_count(sfm, gpu, scene):
    """matching.py:134-144: len(m_kpts0[mask][mask_inliers]) for each pair."""
    got = sfm.verify.essential_inliers_batched(scene["pts0"], scene["pts1"], scene["K"])
    for p in range(len(scene["pts0"])):
        Eo, mo = orc.find_essential_mat(scene["pts0"][p], scene["pts1"][p], scene["K"])
        if Eo is None:
            assert got[p] == -1
            continue
        keep = mo.ravel() > 0
        ngo, _, _, _ = orc.recover_pose(Eo[:3], scene["pts0"][p][keep], scene["pts1"][p][keep], scene["K"])
        assert got[p] == ngo, p


def _ess_run(sfm, pts0, pts1, K, max_iters=1000, prob=0.999, threshold=1.0, **env):
    import os
    keys = ("SFMHIP_ESS_MONO", "SFMHIP_ESS_RECE")
    old = {k: os.environ.pop(k, None) for k in keys}
    try:
        for k, v in env.items():
            os.environ["SFMHIP_ESS_" + k] = str(v)
        sfm.knobs_reload()
        v = sfm.verify
        a, b, of = v.pack_pairs(pts0, pts1)
        r = v.find_essential_batched(a, b, of, v._cam(K), prob=prob, threshold=threshold, max_iters=max_iters)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in r.items()}
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
        sfm.knobs_reload()


def _ess_mixed_scene():
    """Ragged pairs: n < 5, n == 5, tiny n, high outlier fractions (many chunks, a round-1
    work list), all-inlier pairs (niters collapses), and bench-sized pairs."""
    sizes = [3, 5, 6, 9, 40, 300, 2048, 1000, 0, 700, 2048, 5, 120, 64]
    out_fr = [0.3, 0.0, 0.0, 0.2, 0.6, 0.7, 0.3, 0.0, 0.3, 0.55, 0.45, 0.3, 0.8, 0.5]
    pts0, pts1 = [], []
    K = None
    for i, (n, f) in enumerate(zip(sizes, out_fr)):
        s = syn.two_view_pairs(1, max(n, 1), outlier_frac=f, noise_px=0.5, seed=100 + i)
        K = s["K"]
        pts0.append(s["pts0"][0][:n])
        pts1.append(s["pts1"][0][:n])
    return pts0, pts1, K


@pytest.mark.parametrize("max_iters", [1000, 1, 40, 77, 100000])
def test_balanced_equals_monolithic(sfm, gpu, max_iters):
    """The load-balanced form (chunks as work items, records replayed per pair) gives the same
    bits as the one-workgroup-per-pair kernel: E, model counts, masks, inlier and iteration
    counts; also with every chosen E re-solved from its sample (SFMHIP_ESS_RECE=0).  At
    max_iters = 100000 the per-pair scratch (~17 MB) splits the 14 pairs into two batches that
    reuse one scratch block, the pre-drawn samples and the side stream."""
    pts0, pts1, K = _ess_mixed_scene()
    mono = _ess_run(sfm, pts0, pts1, K, max_iters, MONO=1)
    for env in ({}, {"RECE": 0}, {"RECE": 1}):
        bal = _ess_run(sfm, pts0, pts1, K, max_iters, **env)
        for k in ("n_models", "n_inliers", "iters", "mask"):
            assert np.array_equal(bal[k], mono[k]), (env, k, bal[k], mono[k])
        nm = mono["n_models"]
        for p in range(len(nm)):
            assert np.array_equal(bal["E"][p, :nm[p]], mono["E"][p, :nm[p]]), (env, p)


def test_balanced_bench_scene_matches_monolithic(sfm, gpu):
    """The bench workload's first 64 pairs (2-7 chunks each, oracle-counted): same bits."""
    s = syn.two_view_pairs(64, 2048, outlier_frac=0.3, noise_px=0.5, seed=6)
    mono = _ess_run(sfm, s["pts0"], s["pts1"], s["K"], MONO=1)
    for env in ({}, {"RECE": 0}):
        bal = _ess_run(sfm, s["pts0"], s["pts1"], s["K"], **env)
        for k in ("E", "n_models", "n_inliers", "iters", "mask"):
            assert np.array_equal(bal[k], mono[k]), (env, k)
    assert mono["iters"].max() > 64 and mono["iters"].min() >= 1   # round 1 exercised



# ---------------------------------------------------------------------------------------------
# Beyond the centred square camera: the scenes of tests/ess_ref.py.  Every scene there is admissible
# (tests/test_ess_scenes_cpu.py): the oracle's outcome does not depend on a 1e-8 change of the
# candidate models or on the order of a sample's models, and recoverPose's winner is strict with no
# cheirality test near its boundary, so any disagreement is the kernel's.
import ess_ref as er   # noqa: E402


def _sign_dev(a, b):
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))


def _fe_launch(sfm, names, cams=None, **params):
    """One sfmhip_find_essential launch over the named scenes -> numpy outputs and the offsets."""
    v = sfm.verify
    scs = [er.fe_scene(n) for n in names]
    a, b, of = v.pack_pairs([s["pts0"] for s in scs], [s["pts1"] for s in scs])
    if cams is None:
        cams = np.stack([v._cam(s["K"]) for s in scs])
    r = v.find_essential_batched(a, b, of, cams, **params)
    return {k: t.cpu().numpy() for k, t in r.items()}, of.cpu().numpy()


def _fe_same(x, y, i, j, ox, oy):
    """Pair i of launch x and pair j of launch y carry the same bits."""
    for k in ("n_models", "n_inliers", "iters"):
        assert x[k][i] == y[k][j], k
    assert np.array_equal(x["mask"][ox[i]:ox[i + 1]], y["mask"][oy[j]:oy[j + 1]])
    nm = x["n_models"][i]
    assert np.array_equal(x["E"][i, :nm], y["E"][j, :nm])


@pytest.mark.parametrize("name", er.FE_NAMES)
def test_fe_scene_matches_oracle(sfm, gpu, name):
    sc, params, tr = er.fe_scene(name), er.fe_params(name), er.fe_trace(name)
    n = len(sc["pts0"])
    g, _ = _fe_launch(sfm, [name], **params)
    print(f"{name}: n {n} models {g['n_models'][0]} iters {g['iters'][0]}/{tr['iters']} "
          f"inliers {g['n_inliers'][0]}/{int(tr['mask'].sum())} oracle adoptions {tr['adoptions']}")
    assert g["n_models"][0] == 1
    assert g["iters"][0] == tr["iters"]
    assert g["n_inliers"][0] == int(tr["mask"].sum()) == int(g["mask"].sum())
    assert np.array_equal(g["mask"], tr["mask"].ravel())
    Eg = g["E"][0, 0].reshape(3, 3)
    print(f"{name}: max |E gpu -+ E oracle| {_sign_dev(Eg, tr['E']):.3e}")
    assert _same_up_to_sign(Eg, tr["E"], E_TOL), (Eg, tr["E"])
    # the cv2 call form: the same results
    E, mask = sfm.verify.findEssentialMat(sc["pts0"], sc["pts1"], sc["K"], sfm.verify.RANSAC,
                                          params.get("prob", 0.999), params.get("threshold", 1.0),
                                          params.get("max_iters", 1000))
    assert E.shape == (3, 3) and mask.shape == (n, 1) and mask.dtype == np.uint8
    assert np.array_equal(mask, tr["mask"]) and np.array_equal(E, Eg)


@pytest.mark.parametrize("name", er.FE_NAMES)
def test_fe_scene_balanced_equals_monolithic(sfm, gpu, name):
    sc, p = er.fe_scene(name), er.fe_params(name)
    args = ([sc["pts0"]], [sc["pts1"]], sc["K"], p.get("max_iters", 1000), p.get("prob", 0.999), p.get("threshold", 1.0))
    mono = _ess_run(sfm, *args, MONO=1)
    assert mono["n_models"][0] == 1 and mono["iters"][0] == er.fe_trace(name)["iters"]
    for env in ({}, {"RECE": 0}):
        bal = _ess_run(sfm, *args, **env)
        for k in ("E", "n_models", "n_inliers", "iters", "mask"):
            assert np.array_equal(bal[k], mono[k]), (env, k)


def test_fe_ragged_batch_with_a_camera_per_pair(sfm, gpu):
    names = er.FE_DEFAULT
    cams = np.stack([sfm.verify._cam(er.fe_scene(n)["K"]) for n in names])
    assert cams.shape == (len(names), 4) and len({tuple(c) for c in cams}) >= 4
    b, ob = _fe_launch(sfm, names, cams)
    b2, _ = _fe_launch(sfm, names, cams)
    bd, _ = _fe_launch(sfm, names, torch.tensor(cams, device=gpu))
    for i, name in enumerate(names):
        s, os_ = _fe_launch(sfm, [name])
        _fe_same(b, s, i, 0, ob, os_)
        _fe_same(b, b2, i, i, ob, ob)
        _fe_same(b, bd, i, i, ob, ob)
        assert b["iters"][i] == er.fe_trace(name)["iters"]
        assert np.array_equal(b["mask"][ob[i]:ob[i + 1]], er.fe_trace(name)["mask"].ravel())
    # one row is broadcast; any other row count is refused
    same = [n for n in names if tuple(sfm.verify._cam(er.fe_scene(n)["K"])) == er.CAM_OFF]
    assert len(same) >= 3
    rows, orows = _fe_launch(sfm, same)
    row = np.array([er.CAM_OFF])
    for one in (row, torch.tensor(row, device=gpu)):
        got, _ = _fe_launch(sfm, same, one)
        for i in range(len(same)):
            _fe_same(got, rows, i, i, orows, orows)
    two = np.array([er.CAM_OFF, er.CAM_B])
    for bad in (two, torch.tensor(two, device=gpu), torch.tensor(two)):
        with pytest.raises(ValueError):
            _fe_launch(sfm, same, bad)


def _rp_check(got, d, n_keep=None):
    """(n_good, R, t, mask) of the device against recover_pose_detail -> the largest R and t deviations."""
    ng, R, t, m = got
    k = d["k"]
    want = d["masks"][k] if n_keep is None else d["masks"][k][n_keep]
    assert ng == d["counts"][k] == int((m > 0).sum())
    assert m.dtype == np.uint8 and set(np.unique(m)) <= {0, 255}
    assert np.array_equal(m.ravel() > 0, want)
    Ro, to = d["cands"][k]
    np.testing.assert_allclose(R, Ro, rtol=0, atol=1e-8)
    np.testing.assert_allclose(t, to, rtol=0, atol=1e-8)
    return float(np.abs(R - Ro).max()), float(np.abs(t - to).max())


@pytest.mark.parametrize("name", er.RP_NAMES)
def test_rp_scene_matches_oracle(sfm, gpu, name):
    E, a, b, K, dist, mask, _ = er.rp_scene(name)
    E = np.array(E)             # the shared scene is read-only; the call gets its own copy
    v = sfm.verify
    d, dm = er.rp_detail(name), er.rp_detail(name, masked=True)
    dev = [_rp_check(v.recoverPose(E, a, b, K, distanceThresh=dist), d)]
    keep = mask > 0
    full = v.recoverPose(E, a, b, K, mask=mask.reshape(-1, 1), distanceThresh=dist)       # the mask= form
    dev.append(_rp_check(full, dm))
    assert not full[3][~keep].any()
    comp = v.recoverPose(E, a[keep], b[keep], K, distanceThresh=dist)                      # the compacted call
    dev.append(_rp_check(comp, dm, keep))
    assert np.array_equal(comp[1], full[1]) and np.array_equal(comp[2], full[2])
    print(f"{name}: n {len(a)} dist {dist} counts {d['counts']} masked {dm['counts']} oracle k {d['k']}; "
          f"max |R gpu - R oracle| {max(x[0] for x in dev):.3e} max |t gpu - t oracle| {max(x[1] for x in dev):.3e}")


def test_rp_batched_equals_singles(sfm, gpu):
    """recover_pose_batched with a camera row per pair, with and without an input mask: the bits of
    the single calls.  Two find-essential scenes join the first batch with the oracle's E, so that
    the rows differ."""
    v = sfm.verify
    groups = {}
    for name in er.RP_NAMES:
        E, a, b, K, dist, mask, _ = er.rp_scene(name)
        groups.setdefault(dist, []).append((np.array(E), a, b, K, mask))
    for name in ("off-centre", "n-2049"):
        sc, tr = er.fe_scene(name), er.fe_trace(name)
        groups[50.0].append((tr["E"], sc["pts0"], sc["pts1"], sc["K"], tr["mask"].ravel()))
    assert sorted(groups) == [8.0, 20.0, 50.0]
    for dist, probs in groups.items():
        a, b, of = v.pack_pairs([p[1] for p in probs], [p[2] for p in probs])
        Es = np.stack([p[0].ravel() for p in probs])
        cams = np.stack([v._cam(p[3]) for p in probs])
        offs = of.cpu().numpy()
        for masked in (False, True):
            mk = np.concatenate([p[4] for p in probs]).astype(np.uint8) if masked else None
            r = {k: t.cpu().numpy() for k, t in v.recover_pose_batched(Es, a, b, of, cams, mk, dist).items()}
            for i, p in enumerate(probs):
                ng, R, t, m = v.recoverPose(p[0], p[1], p[2], p[3], mask=p[4] if masked else None, distanceThresh=dist)
                assert r["n_good"][i] == ng, (dist, masked, i)
                assert np.array_equal(r["R"][i], R) and np.array_equal(r["t"][i], t.ravel())
                assert np.array_equal(r["mask"][offs[i]:offs[i + 1]], m.ravel())
    assert len({tuple(v._cam(p[3])) for p in groups[50.0]}) == 3


def test_rp_all_zero_mask_is_a_tie(sfm, gpu):
    """Nothing may be counted, so all four candidates tie at 0 and which one is returned is the
    decomposition's choice: asserted as properties, not as parity."""
    E, a, b, K, dist, mask, _ = er.rp_scene("n-769")
    ng, R, t, m = sfm.verify.recoverPose(np.array(E), a, b, K, mask=np.zeros((len(a), 1), np.uint8), distanceThresh=dist)
    assert ng == 0 and m.shape == (len(a), 1) and not m.any()
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
    assert abs(np.linalg.norm(t) - 1) < 1e-12
    cands = er.rp_detail("n-769")["cands"]
    assert min(max(np.abs(R - Rc).max(), np.abs(t - tc).max()) for Rc, tc in cands) <= 1e-8
