"""The scene tables of tests/geom_ref.py do what they are listed for.  No GPU.

* every BA scene is admissible: the oracle agrees with its three Jacobian-noise variants;
* every residual / Jacobian scene tells the right camera from each of the five wrong ones by more
  than 100x the GPU test's tolerance, every BA-solve and global-BA scene through its result by more
  than 10x the GPU tolerance (the zero-cost fit hides a wrong camera in the cost);
* the oracle's DLT null vector meets the optimality criterion on every DLT scene, and every lane of
  the full-list scene fails the fast pass's lambda3 floor;
* the FD step's, Rodrigues' and the projection's branches are really reached."""
import numpy as np
import pytest

import ba_global_ref as ref
import geom_ref as gr
from oracle import ba as oba
from oracle import geometry as og

RES_RTOL, RES_ATOL = 1e-12, 1e-9          # test_gpu_geometry.py's residual tolerance


def test_cameras_and_batch_rows():
    for kind in "ABC":
        K = gr.camera(kind)
        assert K[0, 1] == 37 and K[1, 0] == -5 and K[0, 0] != K[1, 1] and K[0, 2] != K[1, 2] and K[0, 2] * K[1, 2] != 0
    A = gr.camera("A")
    f = gr.syn.FOCAL
    assert (A[0, 0], A[1, 1], A[0, 2], A[1, 2]) == (f, 1.25 * f, 0.65 * f, -0.29 * 1.25 * f)
    K = gr.batch_K(70, seed=52)
    assert len({tuple(k.ravel()) for k in K}) == 70
    base = np.stack([gr.camera("ABC"[i % 3]) for i in range(70)])
    rel = np.abs(K[:, [0, 1, 0, 1], [0, 1, 2, 2]] / base[:, [0, 1, 0, 1], [0, 1, 2, 2]] - 1)
    assert rel.max() <= 0.03 and (rel > 0).all()
    # the entries cv2 ignores are ignored by the oracle
    s = gr.residual_batch()["scenes"][0]
    assert np.array_equal(og.reprojection_error(gr.x_of(s), s["K"], s["pts"]),
                          og.reprojection_error(gr.x_of(s), gr.pinhole(s["K"]), s["pts"]))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["residual_batch", "residual_edges", "fd_batch"])
def test_residual_scenes_tell_the_cameras_apart(name):
    b = getattr(gr, name)()
    right = [og.reprojection_error(gr.x_of(s), s["K"], s["pts"]) for s in b["scenes"]]
    tol = [100 * (RES_ATOL + RES_RTOL * np.abs(r)) for r in right]
    for fault, (Kw, skew) in gr.wrong_cameras(b["K"]).items():
        told = 0
        for p, s in enumerate(b["scenes"]):
            with gr.oracle_with(skew=skew[p]):
                wrong = og.reprojection_error(gr.x_of(s), Kw[p], s["pts"])
            told += int((np.abs(wrong - right[p]) > tol[p]).any())
            if fault == "skew":
                assert (gr.normalised_y(s["X"], s["cam"][:3], s["cam"][3:]) != 0).any()
        # row-0 cannot change pair 0; every other fault must show in every pair
        assert told >= len(b["scenes"]) - (fault == "row-0"), (name, fault, told)


def test_fd_and_residual_edges_are_hit():
    c = gr.fd_edge_counts(gr.fd_batch())
    print("fd_batch", c)
    for k in ("zero_rvec", "zero_t", "zero_X", "negative", "big_X", "big_cam", "theta_0", "theta_near_pi"):
        assert c[k] > 0, k
    assert [len(s["X"]) for s in gr.fd_batch()["scenes"]] == [1, 63, 64, 65, 257, 300]
    c = gr.fd_edge_counts(gr.residual_edges())
    print("residual_edges", c)
    for k in ("theta_0", "theta_below", "theta_above", "theta_near_pi", "z_zero", "z_behind"):
        assert c[k] > 0, k
    c = gr.fd_edge_counts(gr.residual_batch())
    assert c["big_X"] > 0 and [len(s["X"]) for s in gr.residual_batch()["scenes"]] == [100, 300, 1, 255, 257, 64]


# ---------------------------------------------------------------------------------------------
def test_ba_batch_is_admissible():
    assert [r[0] for r in gr.BA_ROWS] == [1, 2, 3, 5, 0, 37, 300, 768, 769]
    assert {r[1] for r in gr.BA_ROWS} == {1.0, 2.5} and {r[2] for r in gr.BA_ROWS} == {False, True}
    for p, adm in enumerate(gr.ba_batch_oracle()):
        if adm is None:
            continue
        ok, info = adm
        o = info["oracle"]
        print(f"pair {p} n {gr.BA_ROWS[p][0]}: (nfev, njev, status) {(o['nfev'], o['njev'], o['status'])} cost {o['cost']:.2e} "
              f"Q {info['Q']:.2e} worst {info['worst']:.2e}")
        assert ok, (p, info["reason"])


@pytest.mark.parametrize("kind", ["A", "B", "C"])
def test_stopping_table_is_admissible_and_stops_where_listed(kind):
    for name in gr.STOPS:
        ok, info = gr.stop_oracle(kind, name)
        o = info["oracle"]
        status, nfev = gr.STOP_EXPECT[name]
        print(f"camera {kind} {name}: (nfev, njev, status) {(o['nfev'], o['njev'], o['status'])} worst {info['worst']:.2e}")
        assert ok, (name, info["reason"])
        assert o["status"] == status
        if nfev is not None:
            assert (o["nfev"], o["njev"]) == (nfev, nfev)
    sc = gr.stop_scene(kind)
    ok, info = gr.stop_oracle(kind, "gtol")
    assert np.array_equal(info["x"], gr.x_of(sc))          # the first gradient test: nothing moves
    tol = gr.single_step_tol(kind)
    print(f"camera {kind}: single-step tolerance {tol:.3e}")
    assert 0 < tol <= 10 * gr.ADMIT_X


def test_drop_in_scenes_are_admissible():
    for which in (0, 1):
        ok, info = gr.ba_admissible(gr.dropin_scene(which))
        assert ok, info["reason"]


def _solve_wrong(s, Kw, skew, **stop):
    with gr.oracle_with(skew=skew):
        return oba.trf_ba(s["cam"], s["X"], Kw, s["pts"], **stop)


def _told_by_result(o, w) -> bool:
    xo, xw = gr.oracle_x(o), gr.oracle_x(w)
    return (o["nfev"], o["njev"]) != (w["nfev"], w["njev"]) or \
        bool(np.abs(xw - xo).max() > 10 * gr.GPU_X * np.abs(xo).max())


def test_ba_batch_tells_the_cameras_apart_through_x():
    b = gr.ba_batch()
    for fault, (Kw, skew) in gr.wrong_cameras(b["K"]).items():
        for p, (s, adm) in enumerate(zip(b["scenes"], gr.ba_batch_oracle())):
            if adm is None or (fault == "row-0" and p == 0):
                continue
            assert _told_by_result(adm[1]["oracle"], _solve_wrong(s, Kw[p], skew[p])), (fault, p)


@pytest.mark.parametrize("kind", ["A", "B", "C"])
def test_stopping_table_tells_the_cameras_apart_through_x(kind):
    """A single-pair launch has only row 0, so the row-0 fault does not apply.  max_nfev = 1 and the
    gtol stop leave x where it was, so the step-taking stops must tell."""
    s = gr.stop_scene(kind)
    for fault, (Kw, skew) in gr.wrong_cameras(s["K"]).items():
        if fault == "row-0":
            continue
        for name in ("max_nfev-2", "max_nfev-3", "xtol"):
            args = gr.stop_args(s, name)
            assert _told_by_result(gr.stop_oracle(kind, name)[1]["oracle"], _solve_wrong(s, Kw[0], skew[0], **args)), (fault, name)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [gr.scene_a_k, gr.scene_b_k])
def test_global_scenes_tell_the_cameras_apart_through_the_result(make):
    """test_whole_solve asserts max |g| <= 2 gtol at the GPU's result with the right cameras: the
    restatement's result under each wrong camera misses that by more than 10x."""
    s = make()
    assert len({tuple(k.ravel()) for k in s["K"]}) == len(s["K"])
    gtol = 1e-6
    for fault, (Kw, skew) in gr.wrong_cameras(s["K"]).items():
        with gr.global_ref_with(ref, skew):
            w = ref.solve(s["cam"], Kw, s["X"], s["obs_cam"], s["obs_pt"], s["pts2d"], s["cam_fixed"], gtol=gtol,
                          ftol=0.0, max_iter=6)
        _, gc, gp = ref.gradient(w["cam"], s["K"], w["X"], s["obs_cam"], s["obs_pt"], s["pts2d"], s["cam_fixed"])
        gmax = float(max(np.abs(gc).max(), np.abs(gp).max()))
        print(make.__name__, fault, "max |g| with the right cameras", gmax)
        assert gmax > 10 * 2 * gtol, fault


# ---------------------------------------------------------------------------------------------
def _dlt_scenes():
    for n in gr.DLT_NS:
        P, single, (poo, _, x0, x1) = gr.dlt_noise_free(n)
        for p, (_, a, b) in enumerate(single):
            yield f"noise-free n={n} pair {p}", P[p, 0], P[p, 1], a, b
        for p in np.unique(poo):
            yield f"noise-free batched n={n} pair {p}", P[p, 0], P[p, 1], x0[:, poo == p], x1[:, poo == p]
    P, launches = gr.dlt_waterfall()
    for poo, x0, x1 in launches:
        for p in np.unique(poo):
            yield f"waterfall {len(poo)} pair {p}", P[p, 0], P[p, 1], x0[:, poo == p], x1[:, poo == p]
    for p, d in enumerate(gr.dlt_degenerate()):
        yield f"P1 = P0 pair {p}", d["P1"], d["P1"], d["x0"], d["x1"]
        yield f"P1 = P0, x1 = x0 pair {p}", d["P1"], d["P1"], d["x0"], d["x0"]
        yield f"parallel rays pair {p}", d["Pa"], d["Pb"], d["x"], d["x"]
    P, poo, x0, x1, _ = gr.dlt_nan_batch()
    for p in np.unique(poo):
        yield f"nan batch pair {p}", P[p, 0], P[p, 1], x0[:, poo == p], x1[:, poo == p]
    f = gr.dlt_full_list()
    yield "full list", f["P"][0, 0], f["P"][0, 1], f["x0"], f["x1"]


def test_dlt_oracle_meets_the_optimality_criterion():
    """(|A X| - sigma_min) / sigma_max of numpy's SVD null vector: a few ulp (measured 4e-16 at the
    most); 1e-14 = 45 ulp is two decades under the GPU tests' 1e-12."""
    worst = 0.0
    for name, P0, P1, x0, x1 in _dlt_scenes():
        X4 = og.triangulate_points(P0, P1, x0, x1)
        crit, _ = gr.dlt_criterion(P0, P1, x0, x1, X4)
        worst = max(worst, float(crit.max()))
        assert crit.max() <= 1e-14, name
    print("DLT criterion of the oracle, worst", worst)


def test_dlt_known_answers():
    for d in gr.dlt_degenerate():
        got = og.triangulate_points(d["P1"], d["P1"], d["x0"], d["x1"])
        assert np.abs(got - d["centre"][:, None]).max() <= 1e-9 and d["centre"][3] > 0
        assert (np.abs(og.triangulate_points(d["Pa"], d["Pb"], d["x"], d["x"])[3]) < 1e-9).all()
    P, launches = gr.dlt_waterfall()
    assert sorted(launches[0][0].tolist()) == list(range(64))
    assert not np.array_equal(launches[1][0], np.sort(launches[1][0]))


def test_dlt_full_list_scene_lists_every_lane():
    f = gr.dlt_full_list()
    ratio = gr.dlt_listed(f["P"][0, 0], f["P"][0, 1], f["x0"], f["x1"])
    _, gap = gr.dlt_criterion(f["P"][0, 0], f["P"][0, 1], f["x0"], f["x1"],
                              og.triangulate_points(f["P"][0, 0], f["P"][0, 1], f["x0"], f["x1"]))
    print("lambda3 test: min ratio", ratio.min(), "; sigma4 / sigma3 <= 1e-2 on", int((gap <= 1e-2).sum()), "of", len(gap))
    assert len(ratio) == 65 * 64
    assert ratio.min() > 2.0                     # > 1 lists the lane; 2 leaves the device's rounding far behind
    assert 0 < (gap <= 1e-2).sum() < len(gap)    # both sides of the oracle-agreement rule occur
