"""GPU parity of the radiance-field kernels of voxel.hip against their f32 oracles, on the scenes
of voxel_field_ref.py: V2 grid sample and nerf_forward, V3 ray/box and stratified sampler, the
two layout kernels, V4 render and the fused training step.  test_voxel_field_cpu.py holds the
same oracles to float64 models on the same scenes.

Bit-equal means: the same NaN positions and the same int32 bit patterns everywhere else.
"""
import importlib

import numpy as np
import pytest
import torch

import voxel_field_ref as vf
from oracle import train as ot
from oracle import voxel as ov

pytestmark = pytest.mark.gpu
abi = importlib.import_module("3d_reconstruction_amd._abi")
vox = importlib.import_module("3d_reconstruction_amd.voxel")
trainmod = importlib.import_module("3d_reconstruction_amd.train")

CANARY = -1.2345678e9


def bits(a):
    """float32 array -> int32 view with every NaN mapped to one pattern."""
    a = np.array(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32)
    a[np.isnan(a)] = np.float32(np.nan)
    return a.view(np.int32)


def assert_bit_equal(got, ref):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape
    bad = np.argwhere(g != r)
    assert bad.size == 0, f"{len(bad)} of {g.size} differ, first at {bad[0].tolist()}: " \
                          f"{g[tuple(bad[0])]:#x} vs {r[tuple(bad[0])]:#x}"


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------
def test_ray_aabb_bit_equal_all_rays(sfm, gpu):
    """t_near, t_far and valid of all 3*256 + 37 rays, invalid rays included: zero and -0.0
    direction components off and on the slab plane (NaN), origin inside, box behind, corner
    rays, NaN / +-inf / 1e30 input."""
    rs = vf.ray_scene()
    tn, tf, va = vox.ray_aabb(torch.tensor(rs["o"]), torch.tensor(rs["d"]), vf.BOX_MIN, vf.BOX_MAX)
    tno, tfo, vao = ov.ray_aabb(rs["o"], rs["d"], vf.BOX_MIN, vf.BOX_MAX)
    assert va.dtype == torch.bool and np.array_equal(va.cpu().numpy(), vao)
    assert_bit_equal(tn, tno)
    assert_bit_equal(tf, tfo)
    assert np.isnan(tno).sum() >= 6 and 0.3 < vao.mean() < 0.9


@pytest.mark.parametrize("perturb", [True, False])
@pytest.mark.parametrize("S", [2, 3, 64, 65, 161])
def test_stratified_bit_equal(sfm, gpu, S, perturb):
    """torch_linspace01 splits at S / 2: even and odd S, the smallest S, one sample past a
    power of two; jitter of exactly 0 and nextafter(1, 0); t_near == t_far; a NaN bound;
    perturb off.  B * S is ragged against the 256-thread workgroup."""
    rng = np.random.default_rng(S)
    B = 300
    tn = rng.uniform(0.0, 3.0, B).astype(np.float32)
    tf = (tn + rng.uniform(0.1, 4.0, B)).astype(np.float32)
    tf[7] = tn[7]
    tn[11], tf[12] = np.nan, np.nan
    tf[13] = np.inf
    t_rand = rng.random((B, S)).astype(np.float32)
    t_rand[:, 0] = 0.0
    t_rand[::3, S - 1] = np.nextafter(np.float32(1), np.float32(0))
    t_rand[5] = 0.0
    t_rand[6] = np.nextafter(np.float32(1), np.float32(0))
    assert (B * S) % 256 != 0 or S == 64      # 300 x 64 is 75 whole workgroups, every other S is ragged
    z = vox.sample_uniform(torch.tensor(tn), torch.tensor(tf), S, torch.tensor(t_rand) if perturb else None,
                           perturb=perturb)
    with np.errstate(invalid="ignore"):
        ref = ov.sample_uniform(tn, tf, S, t_rand if perturb else None)
    assert_bit_equal(z, ref)
    assert np.isnan(ref[11]).all() and np.isnan(ref[12]).any() and np.ptp(ref[7]) <= 1e-6


def test_stratified_rejects_one_sample_without_writing(sfm, gpu):
    B = 5
    tn = torch.zeros(B, device=gpu)
    tf = torch.ones(B, device=gpu)
    tr = torch.rand((B, 1), device=gpu)
    z = torch.full((B, 4), CANARY, device=gpu)
    with pytest.raises(abi.SfmHipError, match="sfmhip_stratified_samples"):
        abi.call("sfmhip_stratified_samples", abi.ptr(tn), abi.ptr(tf), abi.ptr(tr), B, 1, 1, abi.ptr(z), stream())
    torch.cuda.synchronize()
    assert (z == CANARY).all()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", vf.POINT_GRIDS + ((28, 1, 5, 6),), ids=lambda s: "x".join(map(str, s)))
def test_grid_sample_bit_equal(sfm, gpu, shape, mode):
    """VoxelGrid.sample on every point scene: C = 1 / 5 / 28 / 33, the 2x2x2 grid, a one-voxel
    axis, P = 2*256 + 19, mask faces / edges / corners exactly and nextafter either side
    (mode 0 inclusive, mode 1 strict), NaN and inf points."""
    sc = vf.point_scene(shape, mode)
    vg = sfm.VoxelGrid(torch.tensor(sc["grid"]), sc["bmin"], sc["bmax"], mode)
    got = vg.sample(torch.tensor(sc["pts"]))
    with np.errstate(invalid="ignore", over="ignore"):
        ref = ov.grid_sample(sc["grid"], sc["pts"], sc["bmin"], sc["bmax"], mode)
        inside, _ = ov.normalise(sc["pts"], sc["bmin"], sc["bmax"], mode)
    assert got.shape == (vf.POINTS_P, shape[0])
    assert_bit_equal(got, ref)
    assert (bits(got)[~inside] == 0).all() and (~inside).sum() > 50       # +0.0 in all C channels


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(28, 9, 10, 11), (28, 1, 5, 6)], ids=lambda s: "x".join(map(str, s)))
def test_nerf_forward_bit_equal(sfm, gpu, shape, mode):
    """nerf_forward = grid_sample + SH colour + relu on channel 0, in both mask modes and on a
    grid with a one-voxel axis (which sfmhip_grid_sample accepts as well: the two entry points
    take the same grids)."""
    sc = vf.point_scene(shape, mode)
    rng = np.random.default_rng(3)
    d = rng.standard_normal((vf.POINTS_P, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    vg = sfm.VoxelGrid(torch.tensor(sc["grid"]), sc["bmin"], sc["bmax"], mode)
    color, sigma = vg.nerf_forward(torch.tensor(sc["pts"]), torch.tensor(d))
    with np.errstate(invalid="ignore", over="ignore"):
        s = ov.grid_sample(sc["grid"], sc["pts"], sc["bmin"], sc["bmax"], mode)
        inside, _ = ov.normalise(sc["pts"], sc["bmin"], sc["bmax"], mode)
    col = np.where(inside[:, None], ov.sh_colour(s[:, 1:], d), np.float32(0)).astype(np.float32)
    assert_bit_equal(sigma, np.maximum(s[:, 0], np.float32(0)))
    assert_bit_equal(color, col)
    assert (bits(color)[~inside] == 0).all() and (bits(sigma)[~inside] == 0).all()
    assert_bit_equal(vg.sample(torch.tensor(sc["pts"])), s)


@pytest.mark.parametrize("C", [1, 5, 28, 32])
def test_layout_round_trip(sfm, gpu, C):
    """grid -> voxel-major -> grid on a 3x5x7 grid (105 voxels, no multiple of 8): the right
    value in channel c < C, exact 0.0 in channels C..31 (the output starts as a canary), the round
    trip bit for bit."""
    D, H, W = 3, 5, 7
    rng = np.random.default_rng(C)
    grid = rng.standard_normal((C, D, H, W)).astype(np.float32)
    grid[0, 0, 0, 0], grid[C - 1, 2, 4, 6] = -0.0, np.nan
    g = torch.tensor(grid, device=gpu)
    vm = torch.full((D, H, W, 32), CANARY, device=gpu)
    abi.call("sfmhip_grid_to_voxel_major", abi.ptr(g), C, D, H, W, abi.ptr(vm), stream())
    assert_bit_equal(vm[..., :C], np.moveaxis(grid, 0, -1))
    assert (bits(vm[..., C:]) == 0).all()
    back = torch.full((C, D, H, W), CANARY, device=gpu)
    abi.call("sfmhip_grid_from_voxel_major", abi.ptr(vm), C, D, H, W, abi.ptr(back), stream())
    assert_bit_equal(back, grid)


def test_layout_rejects_33_channels_without_writing(sfm, gpu):
    g = torch.zeros((33, 3, 5, 7), device=gpu)
    vm = torch.full((3, 5, 7, 32), CANARY, device=gpu)
    with pytest.raises(abi.SfmHipError, match="sfmhip_grid_to_voxel_major"):
        abi.call("sfmhip_grid_to_voxel_major", abi.ptr(g), 33, 3, 5, 7, abi.ptr(vm), stream())
    out = torch.full((33, 3, 5, 7), CANARY, device=gpu)
    with pytest.raises(abi.SfmHipError, match="sfmhip_grid_from_voxel_major"):
        abi.call("sfmhip_grid_from_voxel_major", abi.ptr(vm), 33, 3, 5, 7, abi.ptr(out), stream())
    torch.cuda.synchronize()
    assert (vm == CANARY).all() and (out == CANARY).all()
    with pytest.raises(ValueError):
        sfm.VoxelGrid(g, -1, 1).voxel_major()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 64, 65, 129])
@pytest.mark.parametrize("mode", [0, 1])
def test_render_train_scene_vs_oracle(sfm, gpu, mode, S):
    """VoxelGrid.render across the 64-sample chunk boundary in both mask modes vs
    oracle.voxel.render (rtol = atol = 1e-5, the existing render tests' tolerance); rays that
    miss the grid are white, exactly 1.0; the sdf-plane entry and the full entry give the same
    bits (mode 0's face rays have +1 corners out of range).  Measured on the MI355X: at most
    1.1e-6 (mode 1, S = 129); S = 1 in mode 1 is bit-equal."""
    sc = vf.train_scene(mode, S)
    D, H, W = vf.TRAIN_SHAPE[1:]
    vg = sfm.VoxelGrid(torch.tensor(sc["grid"]), sc["bmin"], sc["bmax"], mode)
    o, d, z = (torch.tensor(sc[k], device=gpu) for k in ("o", "d", "z"))
    rgb = vg.render(o, d, z)
    ref = ov.render(sc["grid"], sc["bmin"], sc["bmax"], mode, sc["o"], sc["d"], sc["z"])
    got = rgb.cpu().numpy()
    print(f"render mode {mode} S {S}: max |diff| {np.abs(got - ref).max():.3g}")
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)
    quiet = list(vf.TRAIN_MISS + vf.TRAIN_DEAD)
    assert (got[quiet] == 1.0).all() and (ref[quiet] == 1.0).all()
    assert (np.abs(got - 1.0).max(1) > 1e-3).sum() >= 10          # the others are not white
    outs = []
    for name, extra in (("sfmhip_render_rays", ()), ("sfmhip_render_rays_sdf", (vg.grid[0].data_ptr(),))):
        out = torch.full((vf.TRAIN_B, 3), CANARY, device=gpu)
        abi.call(name, vg.voxel_major().data_ptr(), *extra, D, H, W, sc["bmin"].ctypes.data, sc["bmax"].ctypes.data,
                 mode, o.data_ptr(), d.data_ptr(), z.data_ptr(), vf.TRAIN_B, S, out.data_ptr(), stream())
        outs.append(out)
    assert vg.finite() and torch.equal(outs[0], outs[1]) and torch.equal(outs[1], rgb)


# the gradient's tolerance: the project's 160-sample one.  S = 256 sums more terms per voxel; its
# atol is the larger of that and twice the oracle's own distance from float64 on the same case
GRAD_RTOL, GRAD_ATOL = 2e-5, 1e-6


def _grad_atol(mode, S):
    return max(GRAD_ATOL, 2 * vf.ORACLE_VS_F64[(mode, S)][2]) if S == 256 else GRAD_ATOL


def _reached(sc):
    """The voxels the scatter may add to: the in-range corners of every sample inside the mask
    (the oracle's f32 index arithmetic), zero weights included."""
    C, D, H, W = vf.TRAIN_SHAPE
    pts = (sc["o"][:, None, :] + sc["d"][:, None, :] * sc["z"][:, :, None]).reshape(-1, 3)
    inside, g = ov.normalise(pts, sc["bmin"], sc["bmax"], sc["mode"])
    bx, by, bz, _ = ot._corners(g[inside], D, H, W)
    hit = np.zeros((D, H, W), bool)
    for k in range(8):
        x, y, z = bx + (k & 1), by + ((k >> 1) & 1), bz + ((k >> 2) & 1)
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H) & (z >= 0) & (z < D)
        hit[z[ok], y[ok], x[ok]] = True
    return hit


@pytest.mark.parametrize("S", [1, 64, 65, 128, 256])
@pytest.mark.parametrize("mode", [0, 1])
def test_render_train_vs_oracle(sfm, gpu, mode, S):
    """GridTrainer.backward on the train scene: one chunk exactly, one sample into the second,
    two chunks, the 256-sample cap; 37 rays, so the last workgroup of 4 holds one ray, a miss.

    rgb at 2e-6, loss at 1e-6 relative (test_gpu_train.py's), gradient at rtol 2e-5 + atol 1e-6
    max|grad| (S = 256: see _grad_atol), every line with a non-zero oracle gradient flagged,
    every unflagged line exactly zero, the quiet rays (2 misses, 2 with sdf <= 0 throughout) add
    nothing, then one Adam step bit-equal to oracle.train.adam_step on the GPU's own gradient.

    Measured on the MI355X (max |rgb diff|, relative loss diff, max |grad diff| / max |grad|,
    largest share of the gradient tolerance any entry uses; the atomics' order moves the last
    digits from run to run):
        S      mode 0                                mode 1
        1      0        3.9e-09  8.8e-09  0.003      0        3.7e-10  6.4e-08  0.005
        64     5.4e-07  1.8e-08  9.3e-07  0.15       4.8e-07  1.7e-07  1.1e-06  0.40
        65     5.4e-07  5.0e-08  5.8e-07  0.15       3.6e-07  4.5e-08  7.6e-07  0.18
        128    7.8e-07  1.8e-07  1.0e-06  0.30       7.2e-07  4.8e-08  1.9e-06  0.21
        256    1.3e-06  5.8e-07  1.8e-06  0.38       1.2e-06  3.1e-07  2.4e-06  0.34
    (S = 256: atol 3.1e-6 in mode 0 and 1.9e-6 in mode 1, from voxel_field_ref.ORACLE_VS_F64.)"""
    sc = vf.train_scene(mode, S)
    C, D, H, W = vf.TRAIN_SHAPE
    tr = trainmod.GridTrainer(torch.tensor(sc["grid"]), sc["bmin"], sc["bmax"], mode)
    loss, rgb = tr.backward(sc["o"], sc["d"], sc["gt"], sc["z"])
    lo, rgbo, grado = ot.render_loss_grad(sc["grid"], sc["bmin"], sc["bmax"], mode, sc["o"], sc["d"], sc["z"],
                                          sc["gt"])
    rgb = rgb.cpu().numpy()
    gg = tr._export(tr.grad)[0].cpu().numpy()
    scale = np.abs(grado).max()
    print(f"train mode {mode} S {S}: rgb {np.abs(rgb - rgbo).max():.3g} loss {abs(loss - lo) / lo:.3g} "
          f"grad {np.abs(gg - grado).max() / scale:.3g} of max, atol {_grad_atol(mode, S):.3g}, largest share of "
          f"the tolerance {(np.abs(gg - grado) / (_grad_atol(mode, S) * scale + GRAD_RTOL * np.abs(grado))).max():.3g}")
    np.testing.assert_allclose(rgb, rgbo, rtol=0, atol=2e-6)
    assert abs(loss - lo) <= 1e-6 * lo
    np.testing.assert_allclose(gg, grado, rtol=GRAD_RTOL, atol=_grad_atol(mode, S) * scale)
    quiet = list(vf.TRAIN_MISS + vf.TRAIN_DEAD)
    assert (rgb[quiet] == 1.0).all()
    # the zero pattern
    touched = tr.touched.cpu().numpy().astype(bool)
    vm = tr.grad.cpu().numpy()
    assert touched[np.abs(grado).max(0) > 0].all()
    assert np.array_equal(touched, _reached(sc)) and 0.02 < touched.mean() < 1
    assert (bits(vm[~touched]) == 0).all() and not vm[..., C:].any()
    # the quiet rays on their own: nothing in channel 0 (nor anywhere else)
    tq = trainmod.GridTrainer(torch.tensor(sc["grid"]), sc["bmin"], sc["bmax"], mode)
    _, rgbq = tq.backward(sc["o"][quiet], sc["d"][quiet], sc["gt"][quiet], sc["z"][quiet])
    assert (rgbq == 1.0).all() and not tq.grad.any()
    assert not tq.touched[torch.tensor(~touched, device=gpu)].any()
    # Adam on the GPU's own gradient
    tr.optimizer_step()
    assert not tr.touched.any() and not tr.grad.any()
    p1, m1, v1 = ot.adam_step(sc["grid"], gg, np.zeros_like(gg), np.zeros_like(gg), 1)
    assert_bit_equal(tr.grid[0], p1)
    st = tr.state()
    assert_bit_equal(st["exp_avg"][0], m1)
    assert_bit_equal(st["exp_avg_sq"][0], v1)


@pytest.mark.parametrize("mode", [0, 1])
def test_render_train_rejects_257_samples_and_no_rays_is_a_no_op(sfm, gpu, mode):
    sc = vf.train_scene(mode, 256)
    C, D, H, W = vf.TRAIN_SHAPE
    B = vf.TRAIN_B
    tr = trainmod.GridTrainer(torch.tensor(sc["grid"]), sc["bmin"], sc["bmax"], mode)
    o, d, gt = (torch.tensor(sc[k], device=gpu) for k in ("o", "d", "gt"))
    z = torch.tensor(np.concatenate([sc["z"], sc["z"][:, -1:] + 0.01], 1), device=gpu)        # (B, 257)
    rgb = torch.full((B, 3), CANARY, device=gpu)
    sq = torch.full((B,), CANARY, device=gpu)
    grad = torch.full((D, H, W, 32), CANARY, device=gpu)
    touched = torch.full((D, H, W), 7, dtype=torch.uint8, device=gpu)

    def run(nrays, S):
        abi.call("sfmhip_render_train", abi.ptr(tr.param), D, H, W, sc["bmin"].ctypes.data, sc["bmax"].ctypes.data,
                 mode, abi.ptr(o), abi.ptr(d), abi.ptr(z), abi.ptr(gt), nrays, S, abi.ptr(rgb), abi.ptr(sq),
                 abi.ptr(grad), abi.ptr(touched), stream())
    with pytest.raises(abi.SfmHipError, match="S must be <= 256"):
        run(B, 257)
    run(0, 257 - 1)                   # no rays: nothing launched, nothing written
    run(0, 1)
    torch.cuda.synchronize()
    assert (rgb == CANARY).all() and (sq == CANARY).all() and (grad == CANARY).all() and (touched == 7).all()
    with pytest.raises(abi.SfmHipError, match="S must be <= 256"):
        tr.backward(o, d, gt, z)
    empty = np.zeros((0, 3), np.float32)
    loss, rgb0 = tr.backward(empty, empty, empty, np.zeros((0, 5), np.float32))
    assert np.isnan(loss) and rgb0.shape == (0, 3)
    assert not tr.grad.any() and not tr.touched.any()
