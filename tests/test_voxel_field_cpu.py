"""The f32 oracles of the radiance-field kernels against float64 models written from the
operations' definitions (voxel_field_ref.py).  No GPU: test_gpu_voxel_field.py holds the kernels
to these oracles bit for bit, this file holds the oracles to the mathematics, at the shapes
where a chunked kernel can go wrong (S = 64 / 65 / 128 / 129 / 256, mask faces, edge rays).
"""
import numpy as np
import pytest
import torch

import voxel_field_ref as vf
from oracle import train as ot
from oracle import voxel as ov

U = 2.0 ** -24    # unit roundoff of float32


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", vf.POINT_GRIDS + ((28, 1, 5, 6),), ids=lambda s: "x".join(map(str, s)))
def test_grid_sample_oracle_vs_f64(shape, mode):
    """oracle.voxel.grid_sample vs the f64 trilinear on every point scene: identical mask
    decisions (faces, edges, corners, nextafter either side, NaN, inf), values within a
    derived bound.  (28, 1, 5, 6) adds a one-voxel axis: its index is 0 for every point."""
    sc = vf.point_scene(shape, mode)
    C, D, H, W = shape
    with np.errstate(invalid="ignore", over="ignore"):
        inside_o, _ = ov.normalise(sc["pts"], sc["bmin"], sc["bmax"], mode)
        got = ov.grid_sample(sc["grid"], sc["pts"], sc["bmin"], sc["bmax"], mode)
    inside, val, mag = vf.trilinear64(sc["grid"], sc["pts"], sc["bmin"], sc["bmax"], mode)
    assert np.array_equal(inside_o, inside)
    assert 0.2 < inside.mean() < 0.9 and (~np.isfinite(sc["pts"])).any(1).sum() >= 10
    assert (got[~inside] == 0).all() and np.isfinite(got).all()
    # Derivation of the bound, per point and channel (U = 2^-24, the f32 unit roundoff):
    # (1) arithmetic on the oracle's own index: a weight is a product of three factors, each a
    #     difference of f32 numbers (<= 3 roundings) times two multiplications (2 roundings),
    #     times the voxel value (1), summed over 8 corners in f32 (7): <= 13 roundings on any
    #     term, so 13 U sum |w v|; 16 is used.
    # (2) the index itself: mode 0 computes ((p - mn) / (mx - mn)) * 2 - 1, then (g + 1) / 2 * (N - 1);
    #     (p - mn), (mx - mn) and the quotient q in [0, 1] carry 3 U, the doubling is exact, "- 1"
    #     and "+ 1" add U each on values <= 2 (8 U on g + 1, 4 U after the halving), the product
    #     with N - 1 one more: |d idx| <= 5 U (N - 1).  Mode 1 (p / s, clip) stays below that.
    #     A trilinear interpolant is continuous and piecewise linear in each index with slope at
    #     most L_a, the largest step between voxels adjacent along axis a (also across a cell
    #     border, so an index that rounds into the next cell is covered):
    #     sum_a 5 U (N_a - 1) L_a.
    # The f64 model's own rounding (2^-53) is negligible against both.
    g = sc["grid"].astype(np.float64)
    lip = [np.abs(np.diff(g, axis=ax)).reshape(C, -1).max(1, initial=0.0) for ax in (3, 2, 1)]     # x, y, z
    idx_term = 5 * U * ((W - 1) * lip[0] + (H - 1) * lip[1] + (D - 1) * lip[2])        # (C,)
    bound = 16 * U * mag + idx_term[None, :]
    err = np.abs(got.astype(np.float64) - val)
    print(f"grid {shape} mode {mode}: max err {err.max():.3g}, max err/bound {(err / bound).max():.3g}")
    assert (err <= bound).all()
    # a wrong corner or weight moves a value by a large share of |v|, far above the bound
    assert bound.max() < 0.02 * np.abs(g).max()


def test_ray_aabb_oracle_vs_f64_and_edge_classes():
    """oracle.voxel.ray_aabb vs the f64 slab test on the finite, well-separated rays (`valid`
    identical, t within 4 ulp: a bound difference, a reciprocal and a product), and every named
    edge ray in its hand-written class."""
    rs = vf.ray_scene()
    tn, tf, valid = ov.ray_aabb(rs["o"], rs["d"], vf.BOX_MIN, vf.BOX_MAX)
    assert tn.dtype == np.float32 and tf.dtype == np.float32
    b = rs["bulk"]
    tn64, tf64, v64 = vf.slab64(rs["o"][b], rs["d"][b], vf.BOX_MIN, vf.BOX_MAX)
    sep = np.abs(tf64 - tn64) > 1e-4 * np.maximum(1.0, np.abs(tf64))
    assert sep.mean() > 0.95 and 0.3 < v64[sep].mean() < 0.9
    assert np.array_equal(valid[b][sep], v64[sep])
    for got, ref in ((tn[b][sep], tn64[sep]), (tf[b][sep], tf64[sep])):
        assert (np.abs(got - ref) <= 4 * 2.0 ** -23 * np.abs(ref)).all()
    assert (np.isnan(tn) == np.isnan(tf)).all()
    for name, row in rs["edge"].items():
        cls = "nan" if np.isnan(tn[row]) else ("valid" if valid[row] else "invalid")
        assert cls == vf.EDGE_RAYS[name][2], name
        assert not (np.isnan(tn[row]) and valid[row])
    e = rs["edge"]
    assert tn[e["origin_inside"]] == 0 and tn[e["origin_inside_axis"]] == 0 and tf[e["origin_inside_axis"]] == 3
    assert tf[e["box_behind"]] < 0 and tf[e["box_behind_diag"]] < 0
    assert tn[e["through_corner_max"]] == 1 and tn[e["touch_corner"]] == 1 and tf[e["touch_corner"]] == 1
    assert 0 < tn[e["huge_direction"]] < 1e-29
    # signed zeros are defined (IEEE 754-2019 minimum / maximum), whatever the operand order
    for name in ("inf_direction", "neginf_direction", "inf_direction_z"):
        assert tf[e[name]] == 0 and not np.signbit(tf[e[name]]) and not np.signbit(tn[e[name]])


@pytest.mark.parametrize("S", [2, 3, 64, 65, 161])
def test_linspace_oracle_equals_torch(S):
    assert np.array_equal(ov.torch_linspace01(S), torch.linspace(0, 1, S).numpy())


# ---------------------------------------------------------------------------------------------
def _oracle(sc):
    return ot.render_loss_grad(sc["grid"], sc["bmin"], sc["bmax"], sc["mode"], sc["o"], sc["d"], sc["z"], sc["gt"])


@pytest.mark.parametrize("S", vf.TRAIN_S)
@pytest.mark.parametrize("mode", [0, 1])
def test_train_oracle_vs_f64(mode, S):
    """oracle.train.render_loss_grad vs the f64 autograd model (torch grid_sample -> SH ->
    composite -> mse, backward()) on train_scene(mode, S).

    Measured (max |rgb diff|, relative loss diff, max |grad diff| / max |grad|):
        S      mode 0                          mode 1
        1      5.2e-07  3.5e-08  7.3e-07       5.4e-07  4.8e-08  8.4e-07
        2      5.1e-07  2.4e-08  1.0e-06       8.8e-07  6.9e-10  1.1e-06
        63     3.4e-07  1.6e-08  5.3e-07       4.5e-07  6.5e-08  1.2e-06
        64     4.6e-07  4.6e-08  1.4e-06       4.0e-07  6.0e-08  1.2e-06
        65     5.1e-07  1.7e-08  1.2e-06       4.4e-07  9.0e-08  7.2e-07
        128    5.9e-07  3.9e-08  1.5e-06       5.3e-07  1.5e-07  6.2e-07
        129    6.3e-07  1.8e-07  1.5e-06       7.6e-07  1.1e-07  1.6e-06
        256    1.0e-06  1.1e-07  1.5e-06       6.6e-07  6.9e-08  9.4e-07
    (voxel_field_ref.ORACLE_VS_F64).  Gates, twice the largest of each column (the K7 rule):
    rgb 2.0e-6, loss 3.5e-7, gradient 3.2e-6 of its largest entry.  The non-zero pattern of the
    gradient is identical."""
    sc = vf.train_scene(mode, S)
    loss, rgb, grad = _oracle(sc)
    ref = vf.autograd64(sc)
    d_rgb, d_loss, d_grad = vf.distances(loss, rgb, grad, ref)
    print(f"    ({mode}, {S}): ({d_rgb:.2e}, {d_loss:.2e}, {d_grad:.2e}),")
    g_rgb, g_loss, g_grad = (2 * m for m in vf.ORACLE_VS_F64_MAX)
    assert d_rgb <= g_rgb and d_loss <= g_loss and d_grad <= g_grad
    assert np.array_equal(grad != 0, ref["grad"] != 0)
    # the written-out backward the mutations below are applied to is the same model
    an = vf.analytic64(sc)
    assert max(vf.distances(an["loss"], an["rgb"], an["grad"], ref)) < 1e-12
    assert np.array_equal(an["grad"] != 0, ref["grad"] != 0)


@pytest.mark.parametrize("mode", [0, 1])
def test_mutations_bite_past_one_chunk_only(mode):
    """The scenes see what the S = 24 fixture could not.  Each mutation of the f64 model
    (voxel_field_ref.analytic64, never the kernel) must move rgb or the gradient by more than
    100x the oracle gate at S = 65 and 129; the chunk mutations leave S = 1 and S = 64 alone,
    bit for bit; the strict mask changes the face rays only (and nothing in mode 1).

    Measured (max |rgb diff|, max |grad diff| / max |grad|, share of non-zero gradient entries
    that change), mode 0 / mode 1:
        v_restart        S=65  0     1.12  0.018 / 0     2.43  0.023   S=129  0     0.75  0.023 / 0     1.20  0.027
        delta_per_chunk  S=65  0.19  0.59  0.51  / 0.89  0.39  0.68    S=129  1.16  1.51  0.82  / 1.11  1.34  0.89
        carry_dropped    S=65  0.37  0.63  0.51  / 0.57  0.41  0.67    S=129  0.42  0.60  0.82  / 0.49  1.04  0.97
        strict_mask      S=65  0.38  0.64  0.033 / 0     0     0       S=129  0.41  0.68  0.039 / 0     0     0
    against gates of 2.0e-6 (rgb) and 3.2e-6 (gradient)."""
    g_rgb, _, g_grad = (2 * m for m in vf.ORACLE_VS_F64_MAX)
    for S in (1, 64, 65, 129):
        sc = vf.train_scene(mode, S)
        base = vf.analytic64(sc)
        for mu in vf.MUTATIONS:
            m = vf.analytic64(sc, mu)
            d_rgb, _, d_grad = vf.distances(m["loss"], m["rgb"], m["grad"], base)
            share = (m["grad"] != base["grad"]).sum() / (base["grad"] != 0).sum()
            print(f"mode {mode} S {S} {mu}: rgb {d_rgb:.3g} grad {d_grad:.3g} share {share:.3g}")
            rows = np.flatnonzero(np.abs(m["rgb"] - base["rgb"]).max(1) > 0)
            if mu == "strict_mask":
                if mode == 1:
                    assert d_rgb == 0 and d_grad == 0
                    continue
                assert set(rows.tolist()) <= set(vf.TRAIN_FACE) and len(rows) >= 2
                assert d_rgb > 100 * g_rgb and d_grad > 100 * g_grad
                # and the gradient of every other ray is untouched: drop the face rays, nothing moves
                keep = np.setdiff1d(np.arange(vf.TRAIN_B), vf.TRAIN_FACE)
                sub = {k: (v[keep] if k in ("o", "d", "z", "gt") else v) for k, v in sc.items()}
                a, b = vf.analytic64(sub), vf.analytic64(sub, mu)
                assert np.array_equal(a["grad"], b["grad"]) and np.array_equal(a["rgb"], b["rgb"])
            elif S <= 64:
                assert np.array_equal(m["rgb"], base["rgb"]) and np.array_equal(m["grad"], base["grad"])
                assert m["loss"] == base["loss"]
            else:
                assert d_grad > 100 * g_grad
                if mu != "v_restart":    # the reverse pass does not feed the colour
                    assert d_rgb > 100 * g_rgb


@pytest.mark.parametrize("S", vf.TRAIN_S)
@pytest.mark.parametrize("mode", [0, 1])
def test_train_scene_is_not_vacuous(mode, S):
    """Asserted on the oracle alone.  Share of samples inside the mask >= 0.25 (observed
    0.46-0.85), share with sdf > 0 >= 0.10 (observed 0.17-0.57), the missing and the dead rays
    give rgb = 1 exactly and a zero gradient (4 rays), depths sorted with a repeat, and in
    mode 0 a sample exactly on each upper face."""
    sc = vf.train_scene(mode, S)
    o, d, z = sc["o"], sc["d"], sc["z"]
    assert o.shape == (vf.TRAIN_B, 3) and z.shape == (vf.TRAIN_B, S) and vf.TRAIN_B % 4 == 1
    assert (np.diff(z, axis=1) >= 0).all()
    if S >= 2:
        assert (np.diff(z, axis=1) == 0).any()
    if S > 64:
        assert z[1, 64] == z[1, 63]
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
    inside, _ = ov.normalise(pts, sc["bmin"], sc["bmax"], mode)
    sdf = ov.grid_sample(sc["grid"], pts, sc["bmin"], sc["bmax"], mode)[:, 0]
    inside, sdf = inside.reshape(-1, S), sdf.reshape(-1, S)
    print(f"mode {mode} S {S}: inside {inside.mean():.2f}, sdf > 0 {(sdf > 0).mean():.2f}")
    assert inside.mean() >= 0.25 and (sdf > 0).mean() >= 0.10
    assert not inside[list(vf.TRAIN_MISS)].any()
    dead = list(vf.TRAIN_DEAD)
    assert (sdf[dead] <= 0).all() and (S < 63 or inside[dead].mean(1).min() > 0.25)
    quiet = list(vf.TRAIN_MISS) + dead
    _, rgb, grad = ot.render_loss_grad(sc["grid"], sc["bmin"], sc["bmax"], mode, o[quiet], d[quiet], z[quiet],
                                       sc["gt"][quiet])
    assert (rgb == 1).all() and not grad.any()
    if mode == 0:
        p = pts.reshape(-1, S, 3)
        for axis, rays in ((0, (20, 22)), (1, (21, 22)), (2, vf.TRAIN_FACE)):
            for r in rays:
                on = p[r, :, axis] == sc["bmax"][axis]
                assert (on & inside[r]).any()
        for r in vf.TRAIN_FACE:     # every sample of a face ray up to z = max is inside: the inclusive mask
            assert inside[r].sum() == (p[r, :, 2] <= sc["bmax"][2]).sum() >= 1
