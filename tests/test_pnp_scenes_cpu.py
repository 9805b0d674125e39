"""The solvePnPRansac parity scenes (tests/pnp_ref.py SCENES), checked on the CPU before the GPU
sees them:

* every scene is admissible: the oracle with LAPACK, with EPnP's null eigenvector pair rotated by
  three angles, and with pnp.hip's eigen-solver restated in numpy agree on ok, iters, the adoption
  list, the inlier set and the pose to 1e-7 -- so a GPU disagreement is a finding, not the
  eigen-solvers' legitimate freedom inside the null space;
* every scene has the property it is listed for, read from the oracle's trace, and the table as a
  whole covers the kernel's paths (adoptions in the second half of chunk 0, in chunk 1, in later
  chunks, in two different chunks, a partial last chunk, the LM's staging cap on both sides).
"""
import re
from pathlib import Path

import numpy as np
import pytest

import pnp_ref as pr
from oracle import geometry as og


@pytest.mark.parametrize("name", pr.SCENE_NAMES)
def test_scene_is_admissible(name):
    same, spread, out = pr.variants(name)
    print(f"{name}: variant spread {spread:.3e}, iters {out['lapack'][2]}, adoptions {out['lapack'][0]}")
    assert same, {v: (o[0], o[1][0], o[2]) for v, o in out.items()}


@pytest.mark.parametrize("name,kw,params,prop", pr.SCENES, ids=pr.SCENE_NAMES)
def test_scene_has_its_property(name, kw, params, prop):
    adopted, (ok, rv, t, idx), iters = pr.oracle_trace(name)
    assert ok == prop.get("ok", True)
    if not ok:
        assert adopted == []
    else:
        assert adopted and len(idx) == adopted[-1][1]
    if "iters" in prop:
        assert iters == prop["iters"]
    if "inliers" in prop:
        assert len(idx) == prop["inliers"]
    if "true_inliers" in prop:
        assert int(pr.get_scene(name)[5].sum()) == prop["true_inliers"]
    if "last_adopted" in prop:
        assert adopted[-1][0] == prop["last_adopted"]
    if "adopted" in prop:
        assert [a[0] for a in adopted] == prop["adopted"]
    if "counts" in prop:
        assert [a[1] for a in adopted] == prop["counts"]
    if "ties" in prop:
        sc = pr.get_scene(name)
        assert pr.later_ties(sc[0], sc[1], sc[2], **params) == prop["ties"]
    assert len(pr.get_scene(name)[0]) == kw["n"]


def test_table_covers_the_kernel_paths():
    tr = {name: pr.oracle_trace(name) for name in pr.SCENE_NAMES}
    final = [a[-1][0] for a, r, it in tr.values() if a]
    C = pr.CHUNK
    assert any(C // 2 <= k < C for k in final)             # second half of chunk 0
    assert any(C <= k < 2 * C for k in final)              # chunk 1
    assert any(k >= 2 * C for k in final)                  # later chunks
    assert any(len({k // C for k, _ in a}) >= 2 for a, r, it in tr.values())    # two chunks adopt
    assert any(1 <= it % C <= C // 2 - 1 for a, r, it in tr.values())           # partial last chunk, first half
    assert any(k % C == C - 1 for k in final)              # the last slot of a chunk
    assert any(k >= C and k % C >= C // 2 for k in final)  # the second half of a later chunk
    assert any("ties" in prop for _, _, _, prop in pr.SCENES)   # a later tie with another inlier set
    ns = [kw["n"] for _, kw, _, _ in pr.SCENES]
    assert pr.STAGE_CAP in ns and pr.STAGE_CAP + 1 in ns and any(n > pr.STAGE_CAP + 1 for n in ns)
    # fx != fy and a principal point in every scene of the table
    for name in pr.SCENE_NAMES:
        K = pr.get_scene(name)[2]
        assert K[0, 0] != K[1, 1] and K[0, 2] != 0 and K[1, 2] != 0


def test_stage_cap_is_the_kernels():
    src = (Path(__file__).resolve().parent.parent / "3d_reconstruction_amd" / "csrc" / "pnp.hip").read_text()
    c = {k: int(v) for k, v in re.findall(r"constexpr int (kPnThreads|kPnGL|kPnGS) = (\d+);", src)}
    assert "kPnStageCap = kPnH * kPnGS * 8 / 21;" in src and "kPnH = kPnThreads / kPnGL;" in src
    kPnH = c["kPnThreads"] // c["kPnGL"]
    assert kPnH == pr.CHUNK
    assert kPnH * c["kPnGS"] * 8 // 21 == pr.STAGE_CAP


def test_scene_generator_is_exact_in_float():
    # cx, cy of both test cameras survive the kernel's float scoring path unrounded
    for K in (pr.KO, pr.K3):
        assert np.all(K.astype(np.float32).astype(np.float64) == K)
    X, uv, K, rv, t, inl = pr.scene(50, 3, c0=(40.0, -25.0, 60.0), noise=0.0, outlier=0.0)
    np.testing.assert_allclose(og.project_points(X, rv, t, K), uv, rtol=0, atol=1e-9)
    assert np.abs(X.mean(0) - [40.0, -25.0, 60.0]).max() < 0.5


def test_eig_variants_restore_the_oracle():
    from oracle import pnp as opnp
    from oracle import ransac as oransac
    real = (opnp.eig_desc, opnp.ransac, oransac.update_num_iters)
    for v in pr.VARIANTS:
        with pytest.raises(RuntimeError):
            with pr.eig_variant(v):
                raise RuntimeError
    pr.oracle_trace("tiny-6")
    assert (opnp.eig_desc, opnp.ransac, oransac.update_num_iters) == real
    # the variants are real: same invariant subspace, another basis inside the null pair
    X, uv, K = pr.sweep_scene(0)[:3]
    E = opnp.EPnP(K, X.astype(np.float32).astype(np.float64), uv.astype(np.float32).astype(np.float64))
    M = E.M(E.alphas(E.control_points()))
    A = M.T @ M
    _, V0 = opnp.eig_desc(A)
    P0 = V0[10:].T @ V0[10:]
    for v in pr.VARIANTS[1:]:
        with pr.eig_variant(v):
            w, V = opnp.eig_desc(A)
            w3, V3 = opnp.eig_desc(np.diag([3.0, 1.0, 2.0]))
        assert np.array_equal(w3, [3.0, 2.0, 1.0])                       # 3x3: untouched
        assert np.abs(V[10:].T @ V[10:] - P0).max() < 1e-7              # the same null plane
        assert np.abs(np.abs(V[10:] @ V0[10:].T) - np.eye(2)).max() > 1e-3 or v == "device"
        for k in (8, 9):
            assert min(np.abs(V[k] - V0[k]).max(), np.abs(V[k] + V0[k]).max()) < 1e-6


def test_five_point_sweep_cap():
    """The raw-EPnP sweep leaves out the problems whose five eigen-solver variants differ by more
    than 1e-8; at most 5 % may be left out, and the rest must recover the true pose to 1e-5."""
    poses, spread = pr.sweep_reference()
    out = spread > pr.SWEEP_SPREAD
    worst = 0.0
    for s in np.nonzero(~out)[0]:
        rv, t = pr.sweep_scene(s)[3:5]
        worst = max(worst, float(np.abs(og.rodrigues(poses[s, :3]) - og.rodrigues(rv)).max()),
                    float(np.abs(poses[s, 3:] - t).max()))
    print(f"5-point sweep: {int(out.sum())} of {pr.SWEEP} left out (largest spread {spread.max():.3e}), "
          f"largest truth error of the rest {worst:.3e}")
    assert int(out.sum()) <= pr.SWEEP_MAX_EXCLUDED
    assert worst <= 1e-5
