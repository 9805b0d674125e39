"""GPU parity: the batched on-device BA solve (sfm.py:37-38) vs the restated
scipy TRF iteration (oracle/ba.py, itself pinned to scipy by
tests/test_oracle_ba.py) and vs scipy's least_squares.

Tolerance: identical nfev / njev / status class, parameters within 1e-6 of
max |x|.  The FD Jacobian values differ from the host's by the FD quantum
(a one-ulp difference of a perturbed residual, device vs glibc sin/cos inside
Rodrigues, moves J by ulp/h ~ 2e-4 absolute: tests/test_gpu_geometry.py), and
the BA problem is rank-deficient (2n residuals, 3n + 6 unknowns: every point
can slide along its ray), so those J differences move the converged point
along the solution manifold by ~1e-7 (observed 7e-8 .. 7e-7 absolute)."""
import importlib

import numpy as np
import pytest
import torch
from scipy.optimize import least_squares

import geom_ref as gr
from oracle import ba as oba
from oracle import geometry as og

pytestmark = pytest.mark.gpu
syn = importlib.import_module("3d_reconstruction_amd.synthetic")


def _ragged_problem(sizes, seed, far=False):
    """Per-pair (cam, K, X, pts) problems of the given sizes (0 = an empty pair)."""
    rng = np.random.default_rng(seed)
    cams, Ks, Xs, ps = [], [], [], []
    for p, n in enumerate(sizes):
        s = syn.ba_scene(1, max(n, 1), seed=seed + p)
        cam = s["cam"][0].copy()
        X = s["X"][:n].copy()
        if far:
            cam += np.r_[rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)]
            X += rng.normal(0, 0.05, X.shape)
        cams.append(cam)
        Ks.append(s["K"][0])
        Xs.append(X)
        ps.append(s["pts2d"][:n])
    return cams, Ks, Xs, ps


def _solve_gpu(sfm, gpu, cams, Ks, Xs, ps, **kw):
    off = np.concatenate([[0], np.cumsum([len(x) for x in Xs])]).astype(np.int64)
    cam = torch.tensor(np.stack(cams), device=gpu)
    K = torch.tensor(np.stack(Ks), device=gpu)
    X = torch.tensor(np.concatenate(Xs).reshape(-1, 3), device=gpu)
    P = torch.tensor(np.concatenate(ps).reshape(-1, 2), device=gpu)
    res = sfm.ba_solve_batched(cam, K, X, P, torch.tensor(off, device=gpu), **kw)
    torch.cuda.synchronize()
    return cam.cpu().numpy(), X.cpu().numpy(), {k: v.cpu().numpy() for k, v in res.items()}, off


@pytest.mark.parametrize("far", [False, True])
def test_ba_solve_batched_vs_oracle(sfm, gpu, far):
    """The batched device TRF meets the oracle's iteration (nfev, njev, x, cost) on ragged
    pairs, including an empty one."""
    sizes = [300, 0, 1000, 37, 700, 2048]
    cams, Ks, Xs, ps = _ragged_problem(sizes, seed=40 + far, far=far)
    cam, X, res, off = _solve_gpu(sfm, gpu, cams, Ks, Xs, ps)
    for p, n in enumerate(sizes):
        if n == 0:
            assert res["nfev"][p] == 0 and res["status"][p] == 1
            continue
        o = oba.trf_ba(cams[p], Xs[p], Ks[p], ps[p])
        assert (res["nfev"][p], res["njev"][p]) == (o["nfev"], o["njev"]), p
        assert res["status"][p] > 0
        xo = np.concatenate([o["cam"], o["X"].ravel()])
        xg = np.concatenate([cam[p], X[off[p]:off[p + 1]].ravel()])
        assert np.abs(xg - xo).max() <= 1e-6 * np.abs(xo).max(), p
        # the cost is flat along the solution manifold the point slides on: 1e-6 relative
        assert abs(res["cost"][p] - o["cost"]) <= 1e-6 * o["cost"] + 1e-12, p


@pytest.mark.parametrize("far", [0, 1])
def test_ba_fused_trial_jacobian_form_bit_identical(sfm, gpu, knob, far):
    """The fused form (SFMHIP_AB=9: the Jacobian at the trial point formed inside the trial
    pass into a second record set, taken on acceptance — VERDICT r5 item 3) against the shipped
    two-pass form: the same cam, X, cost, nfev, njev and status bits on ragged pairs (near and
    far starts), an empty pair, and the bench scene's first 32 pairs (the digest over all 256
    bench pairs, rejected steps included, matched too: DESIGN §6f item 3)."""
    sizes = [300, 0, 1000, 37, 700, 2048]
    cams, Ks, Xs, ps = _ragged_problem(sizes, seed=60 + far, far=far)
    out = []
    for ab in (0, 9):
        knob("AB", ab)
        out.append(_solve_gpu(sfm, gpu, cams, Ks, Xs, ps))
    (c0, x0, r0, _), (c1, x1, r1, _) = out
    assert np.array_equal(c0, c1) and np.array_equal(x0, x1)
    for key in ("cost", "nfev", "njev", "status"):
        assert np.array_equal(r0[key], r1[key]), key
    s = syn.ba_scene(32, 4096, seed=4)
    tt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in s.items()}
    off = torch.arange(33, dtype=torch.int64, device=gpu) * 4096
    res = []
    for ab in (0, 9):
        knob("AB", ab)
        cam, X = tt["cam"].clone(), tt["X"].clone()
        r = sfm.ba_solve_batched(cam, tt["K"], X, tt["pts2d"], off, validate=False)
        res.append((cam.cpu(), X.cpu(), {k: v.cpu() for k, v in r.items() if isinstance(v, torch.Tensor)}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for key in res[0][2]:
        assert torch.equal(res[0][2][key], res[1][2][key]), key


@pytest.mark.parametrize("far", [0, 1])
def test_ba_lds_records_bit_identical(sfm, gpu, knob, far):
    """The records of each pair's first 768 observations kept in LDS (the default) against all
    records in scratch (SFMHIP_AB=7): the same bits on pairs wholly in LDS (<= 768 observations),
    split across LDS and scratch (769, 1500, 2048), an empty pair, and a batch of 300 pairs
    (more workgroups than CUs: the launch runs in rounds)."""
    sizes = [300, 0, 768, 769, 37, 1500, 2048]
    cams, Ks, Xs, ps = _ragged_problem(sizes, seed=70 + far, far=far)
    out = []
    for ab in (0, 7):
        knob("AB", ab)
        out.append(_solve_gpu(sfm, gpu, cams, Ks, Xs, ps))
    (c0, x0, r0, _), (c1, x1, r1, _) = out
    assert np.array_equal(c0, c1) and np.array_equal(x0, x1)
    for key in ("cost", "nfev", "njev", "status"):
        assert np.array_equal(r0[key], r1[key]), key
    sizes = [int(v) for v in np.random.default_rng(far).integers(20, 120, 300)]
    cams, Ks, Xs, ps = _ragged_problem(sizes, seed=80 + far, far=far)
    out = []
    for ab in (0, 7):
        knob("AB", ab)
        out.append(_solve_gpu(sfm, gpu, cams, Ks, Xs, ps))
    (c0, x0, r0, _), (c1, x1, r1, _) = out
    assert np.array_equal(c0, c1) and np.array_equal(x0, x1)
    for key in ("cost", "nfev", "njev", "status"):
        assert np.array_equal(r0[key], r1[key]), key


def test_least_squares_ba_drop_in_vs_scipy(sfm, gpu):
    """sfm.py:38 with the on-device solve: scipy's nfev and solution."""
    cams, Ks, Xs, ps = _ragged_problem([500], seed=50, far=True)
    x0 = np.concatenate([cams[0], Xs[0].ravel()])
    A = og.ba_sparse(500, len(x0), 6)
    r = least_squares(og.reprojection_error, x0, jac_sparsity=A, x_scale="jac", ftol=1e-8, args=(Ks[0], ps[0]))
    g = sfm.least_squares_ba(x0, Ks[0], ps[0])
    assert g.success and r.success
    assert abs(g.nfev - r.nfev) <= 1
    assert np.abs(g.x - r.x).max() <= 1e-6 * np.abs(r.x).max()
    assert abs(g.cost - r.cost) <= 1e-6 * r.cost + 1e-12
    np.testing.assert_allclose(g.fun, og.reprojection_error(g.x, Ks[0], ps[0]), rtol=1e-9, atol=1e-9)


def test_ba_solve_rejects_bad_shapes(sfm, gpu):
    cam = torch.zeros((2, 6), dtype=torch.float64, device=gpu)
    K = torch.zeros((2, 3, 3), dtype=torch.float64, device=gpu)
    X = torch.zeros((5, 3), dtype=torch.float64, device=gpu)
    P = torch.zeros((5, 2), dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError):
        sfm.ba_solve_batched(cam, K, X, P, torch.zeros(2, dtype=torch.int64, device=gpu))
    with pytest.raises(ValueError):
        sfm.ba_solve_batched(cam, K, X.float(), P, torch.zeros(3, dtype=torch.int64, device=gpu))


def test_ba_solve_malformed_offsets(sfm, gpu):
    """Offsets that are not 0 <= off[p] <= off[p+1] <= n: the wrapper raises, and
    with validation off the kernel skips those pairs (status -1) without
    touching X outside any valid range."""
    cams, Ks, Xs, ps = _ragged_problem([40, 40, 40], seed=61)
    cam = torch.tensor(np.stack(cams), device=gpu)
    K = torch.tensor(np.stack(Ks), device=gpu)
    X = torch.tensor(np.concatenate(Xs), device=gpu)
    P = torch.tensor(np.concatenate(ps), device=gpu)
    for off in ([0, 40, 30, 120], [0, 40, 80, 121], [5, 40, 80, 120], [0, 40, 200, 120]):
        with pytest.raises(ValueError):
            sfm.ba_solve_batched(cam, K, X, P, torch.tensor(off, dtype=torch.int64, device=gpu))
    X0 = X.clone()
    res = sfm.ba_solve_batched(cam, K, X, P, torch.tensor([0, 40, 200, 120], dtype=torch.int64, device=gpu),
                               validate=False)
    torch.cuda.synchronize()
    st = res["status"].cpu().numpy()
    assert st[0] > 0 and st[1] == -1 and st[2] == -1
    assert torch.equal(X[40:], X0[40:])               # the skipped pairs' points are untouched


def _sfm_py_residual(cv2):
    """The residual sfm.py:87-91 hands to least_squares, written against a cv2
    module: x = [rvec, t, X...] -> point_2D - projectPoints(X, rvec, t, K)."""
    def residual(x, K, point_2D):
        pts3d = x[6:].reshape((len(point_2D), 3))
        proj, _ = cv2.projectPoints(pts3d, x[:3], x[3:6], K, distCoeffs=None)
        return (point_2D - proj[:, 0, :]).ravel()
    return residual


def test_unchanged_sfm_py_least_squares_through_sfmhip(sfm, gpu):
    """sfm.py:37-38 left exactly as written — scipy least_squares with
    jac_sparsity=ba_sparse(...), x_scale='jac', ftol=1e-8 and the default
    2-point FD — with only ``import sfmhip as cv2`` swapped in: every residual
    evaluation goes through sfmhip.projectPoints on the device.  Same solution
    as the oracle-driven run (the FD quantum of device vs glibc sin/cos is the
    only difference in the Jacobian)."""
    import sfmhip as cv2
    cams, Ks, Xs, ps = _ragged_problem([500], seed=52, far=True)
    x0 = np.concatenate([cams[0], Xs[0].ravel()])
    A = cv2.ba_sparse(500, len(x0), 6)
    got = least_squares(_sfm_py_residual(cv2), x0, jac_sparsity=A, x_scale="jac", ftol=1e-8, args=(Ks[0], ps[0]))
    ref = least_squares(og.reprojection_error, x0, jac_sparsity=og.ba_sparse(500, len(x0), 6), x_scale="jac",
                        ftol=1e-8, args=(Ks[0], ps[0]))
    assert got.success and ref.success
    assert abs(got.nfev - ref.nfev) <= 1
    assert np.abs(got.x - ref.x).max() <= 1e-6 * np.abs(ref.x).max()
    assert abs(got.cost - ref.cost) <= 1e-6 * ref.cost + 1e-12


# ---------------------------------------------------------------------------------------------
# off the centred camera: a camera row per pair, admissible scenes only (tests/geom_ref.py)
def _solve_batch(sfm, gpu, b, **kw):
    scs = b["scenes"]
    return _solve_gpu(sfm, gpu, [s["cam"] for s in scs], [s["K"] for s in scs], [s["X"] for s in scs],
                      [s["pts"] for s in scs], **kw)


def test_ba_solve_batched_per_pair_cameras_vs_oracle(sfm, gpu):
    """One ragged batch, pairs of 1, 2, 3, 5, 0, 37, 300, 768 and 769 observations (fewer residuals
    than camera parameters up to one more than the LDS holds), every pair with its own K row
    (cameras A, B, C jittered), near and far starts, scene scale 1 and 2.5; each scene admissible
    (test_geom_scenes_cpu.py).  The assertions of test_ba_solve_batched_vs_oracle, with the status
    compared for equality."""
    b = gr.ba_batch()
    cam, X, res, off = _solve_batch(sfm, gpu, b)
    for p, adm in enumerate(gr.ba_batch_oracle()):
        if adm is None:
            assert res["nfev"][p] == 0 and res["status"][p] == 1
            continue
        o, xo = adm[1]["oracle"], adm[1]["x"]
        xg = np.concatenate([cam[p], X[off[p]:off[p + 1]].ravel()])
        print(f"pair {p} n {off[p + 1] - off[p]}: gpu (nfev, njev, status) {(res['nfev'][p], res['njev'][p], res['status'][p])} "
              f"oracle {(o['nfev'], o['njev'], o['status'])} |dx| / max |x| {np.abs(xg - xo).max() / np.abs(xo).max():.3e} "
              f"cost {res['cost'][p]:.3e} oracle {o['cost']:.3e}")
    for p, adm in enumerate(gr.ba_batch_oracle()):
        if adm is None:
            continue
        o, xo = adm[1]["oracle"], adm[1]["x"]
        assert (res["nfev"][p], res["njev"][p]) == (o["nfev"], o["njev"]), p
        assert res["status"][p] == o["status"], p
        xg = np.concatenate([cam[p], X[off[p]:off[p + 1]].ravel()])
        assert np.abs(xg - xo).max() <= 1e-6 * np.abs(xo).max(), p
        assert abs(res["cost"][p] - o["cost"]) <= 1e-6 * o["cost"] + 1e-12, p


@pytest.mark.parametrize("ab", [7, 9])
def test_ba_per_pair_cameras_forms_bit_identical(sfm, gpu, knob, ab):
    """The same batch with all records in scratch (SFMHIP_AB=7) and in the fused form (SFMHIP_AB=9):
    the bits of the default."""
    b = gr.ba_batch()
    out = []
    for v in (0, ab):
        knob("AB", v)
        out.append(_solve_batch(sfm, gpu, b))
    (c0, x0, r0, _), (c1, x1, r1, _) = out
    assert np.array_equal(c0, c1) and np.array_equal(x0, x1)
    for key in ("cost", "nfev", "njev", "status"):
        assert np.array_equal(r0[key], r1[key]), key


@pytest.mark.parametrize("kind", ["A", "B", "C"])
def test_ba_stopping_table(sfm, gpu, kind):
    """One admissible 300-point far scene per camera, stopped everywhere but at convergence:
    max_nfev = 1, 2, 3 (status 0, nfev = njev = max_nfev), a gtol above the first |g| (status 1 at
    nfev = 1, X and cam untouched bit for bit) and xtol = 1e-3 (status 3).  After the single step of
    max_nfev = 2, x meets the oracle's at geom_ref.single_step_tol, 10x what Jacobian noise of
    one FD quantum does to the oracle's own step."""
    sc = gr.stop_scene(kind)
    for name in gr.STOPS:
        ok, info = gr.stop_oracle(kind, name)
        o, xo = info["oracle"], info["x"]
        cam, X, res, _ = _solve_gpu(sfm, gpu, [sc["cam"]], [sc["K"]], [sc["X"]], [sc["pts"]], **gr.stop_args(sc, name))
        xg = np.concatenate([cam[0], X.ravel()])
        dx = np.abs(xg - xo).max() / np.abs(xo).max()
        print(f"camera {kind} {name}: gpu {(res['nfev'][0], res['njev'][0], res['status'][0])} oracle "
              f"{(o['nfev'], o['njev'], o['status'])} |dx| / max |x| {dx:.3e}")
        status, nfev = gr.STOP_EXPECT[name]
        assert res["status"][0] == status == o["status"], name
        assert (res["nfev"][0], res["njev"][0]) == (o["nfev"], o["njev"]), name
        if nfev is not None:
            assert (res["nfev"][0], res["njev"][0]) == (nfev, nfev), name
        if name in ("gtol", "max_nfev-1"):
            assert np.array_equal(cam[0], sc["cam"]) and np.array_equal(X, sc["X"]), name
        elif name == "max_nfev-2":
            print(f"camera {kind}: single-step tolerance {gr.single_step_tol(kind):.3e}")
            assert dx <= gr.single_step_tol(kind), name
        else:
            assert dx <= 1e-6, name


def test_least_squares_ba_drop_in_vs_scipy_camera_a(sfm, gpu):
    """test_least_squares_ba_drop_in_vs_scipy on camera A (fx != fy, cx != cy != 0)."""
    s = gr.dropin_scene(0)
    x0 = gr.x_of(s)
    A = og.ba_sparse(500, len(x0), 6)
    r = least_squares(og.reprojection_error, x0, jac_sparsity=A, x_scale="jac", ftol=1e-8, args=(s["K"], s["pts"]))
    g = sfm.least_squares_ba(x0, s["K"], s["pts"])
    print("camera A drop-in: nfev", g.nfev, r.nfev, "|dx| / max |x|", np.abs(g.x - r.x).max() / np.abs(r.x).max())
    assert g.success and r.success
    assert abs(g.nfev - r.nfev) <= 1
    assert np.abs(g.x - r.x).max() <= 1e-6 * np.abs(r.x).max()
    assert abs(g.cost - r.cost) <= 1e-6 * r.cost + 1e-12
    np.testing.assert_allclose(g.fun, og.reprojection_error(g.x, s["K"], s["pts"]), rtol=1e-9, atol=1e-9)


def test_unchanged_sfm_py_least_squares_through_sfmhip_camera_a(sfm, gpu):
    """test_unchanged_sfm_py_least_squares_through_sfmhip on camera A."""
    import sfmhip as cv2
    s = gr.dropin_scene(1)
    x0 = gr.x_of(s)
    A = cv2.ba_sparse(500, len(x0), 6)
    got = least_squares(_sfm_py_residual(cv2), x0, jac_sparsity=A, x_scale="jac", ftol=1e-8, args=(s["K"], s["pts"]))
    ref = least_squares(og.reprojection_error, x0, jac_sparsity=og.ba_sparse(500, len(x0), 6), x_scale="jac",
                        ftol=1e-8, args=(s["K"], s["pts"]))
    print("camera A sfm.py: nfev", got.nfev, ref.nfev, "|dx| / max |x|", np.abs(got.x - ref.x).max() / np.abs(ref.x).max())
    assert got.success and ref.success
    assert abs(got.nfev - ref.nfev) <= 1
    assert np.abs(got.x - ref.x).max() <= 1e-6 * np.abs(ref.x).max()
    assert abs(got.cost - ref.cost) <= 1e-6 * ref.cost + 1e-12
