"""GPU: TSDF depth and colour fusion (tsdf.hip: block table, brick / cull / refine passes, the
fused persistent pre-pass, tsdf_fuse_kernel / tsdf_colour_kernel) off the centred square-pixel
camera, bit for bit against oracle.voxel.tsdf_integrate and tests/tsdf_colour_ref.py on the
scenes of tests/tsdf_cam_scenes.py: anisotropic and off-centre (A), a camera and a roll per
frame (B), crops with the principal point outside the image and mirrored frames (C),
telephoto on large frames (D).  tests/test_tsdf_cameras_cpu.py shows on the CPU that these
scenes tell fx from fy, frame f's record from frame 0's and a focal length from its absolute
value, which the one camera of the other fusion tests cannot."""
import numpy as np
import pytest
import torch

import tsdf_cam_scenes as cs
import tsdf_colour_ref as cr
import tsdf_raycast_ref as rr
from oracle import voxel as ov

pytestmark = pytest.mark.gpu

# the launch modes of test_gpu_voxel.py: the library's choice, whole-grid / latency mode, and the
# whole-grid form with separate (w1) or fused (w3, w31: no lag, no patience) pre-passes
LAT_MODES = ["auto", "0", "1", "w1", "w3", "w31"]
COLOUR_MODES = ["auto", "0", "1", "w1"]
SCENES = ["A", "B", "C", "D"]
BND = (cs.BMIN, cs.BMAX)
TRUNC = float(cs.MU)
SLABS = ((0, 7), (7, 21), (21, 48))


def _set_lat(knob, lat):
    if lat in ("0", "1"):
        knob("TSDF_LATENCY", lat)
    elif lat.startswith("w"):
        knob("TSDF_LATENCY", 0)
        knob("AB", lat[1:])


def prior():
    rng = np.random.default_rng(5)
    return (rng.uniform(-1, 1, cs.SHAPE).astype(np.float32), rng.integers(0, 3, cs.SHAPE).astype(np.float32))


class Case:
    """A scene, a random prior grid state and the oracle's result from it, computed once."""

    def __init__(self, depth, poses, K):
        self.depth, self.poses, self.K = depth, poses, K
        self.T0, self.W0 = prior()
        self.T, self.W = self.oracle(self.T0, self.W0)
        self.frames = tuple(torch.from_numpy(a.copy()) for a in (depth, poses, K))
        for a in (self.depth, self.poses, self.K, self.T0, self.W0, self.T, self.W):
            a.setflags(write=False)

    def oracle(self, T, W, frames=slice(None), **kw):
        return ov.tsdf_integrate(T, W, self.depth[frames], self.poses[frames], self.K[frames], *BND, cs.MU, **kw)

    def gpu(self, sfm, gpu, T=None, W=None, frames=slice(None), **kw):
        """One tsdf_integrate call from (T, W) (default: the prior) -> numpy (T, W)."""
        T = torch.from_numpy((self.T0 if T is None else T).copy()).to(gpu)
        W = torch.from_numpy((self.W0 if W is None else W).copy()).to(gpu)
        sfm.tsdf_integrate(T, W, *(a[frames] for a in self.frames), *BND, TRUNC, **kw)
        torch.cuda.synchronize()
        return T.cpu().numpy(), W.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(*cs.SCENES[name]())
        return cache[name]
    return get


def same(got, ref):
    np.testing.assert_array_equal(got[1], ref[1])
    np.testing.assert_array_equal(got[0], ref[0])


@pytest.mark.parametrize("lat", LAT_MODES)
@pytest.mark.parametrize("name", SCENES)
def test_fusion_bitexact(sfm, gpu, knob, cases, name, lat):
    _set_lat(knob, lat)
    c = cases(name)
    same(c.gpu(sfm, gpu), (c.T, c.W))
    assert (c.W > c.W0).mean() >= 0.3


@pytest.fixture(scope="module")
def colour_refs(cases):
    cache = {}

    def get(name):
        if name not in cache:
            c = cases(name)
            colour = cr.random_colour(c.depth, 7)
            ref = cr.integrate_colour(np.zeros(cs.SHAPE + (4,), np.int32), c.depth, colour, c.poses, c.K, *BND,
                                      cs.MU).view(np.uint32)
            ref.setflags(write=False)
            cache[name] = (colour, ref)
        return cache[name]
    return get


@pytest.mark.parametrize("lat", COLOUR_MODES)
@pytest.mark.parametrize("name", SCENES)
def test_colour_bitexact(sfm, gpu, knob, cases, colour_refs, name, lat):
    _set_lat(knob, lat)
    c = cases(name)
    colour, ref = colour_refs(name)
    C = torch.zeros(cs.SHAPE + (4,), dtype=torch.int32, device=gpu)
    sfm.tsdf_integrate_colour(C, c.frames[0], torch.from_numpy(colour), c.frames[1], c.frames[2], *BND, TRUNC)
    torch.cuda.synchronize()
    share = (ref[..., 3] > 0).mean()
    print(f"scene {name}: coloured share {share:.3f}")
    assert np.array_equal(C.cpu().numpy().view(np.uint32), ref)
    assert share >= 0.05


@pytest.mark.parametrize("name", SCENES)
def test_prepasses_decide_something(sfm, gpu, cases, name):
    """The bit-exact runs above went through the culling and free-space proofs, not the
    keep-everything fallback: both decide some (wave sub-tile, frame) pairs of every scene."""
    c = cases(name)
    st = sfm.tsdf_cull_stats(cs.SHAPE, *c.frames, *BND, TRUNC)
    tested, culled, free = st["tested"], st["culled"], st["free"]
    print(f"scene {name}: tested {tested}, culled {culled / tested:.3f}, free {free / tested:.3f}, "
          f"projected {(tested - culled - free) / tested:.3f}")
    assert culled > 0 and free > 0 and culled + free <= tested
    layers = sfm.tsdf_layer_stats(cs.SHAPE, *c.frames, *BND, TRUNC)
    assert layers.shape == (cs.R // 8, 3)
    assert tuple(int(x) for x in layers.sum(0)) == (tested, culled, free)


@pytest.mark.parametrize("name", ["B", "C"])
def test_slabs_frames_and_shared_table(sfm, gpu, cases, name):
    """A camera and a roll per frame move the block range of each frame that a z-slab needs:
    slabs fused one by one with a caller-built table give the single call's grid and, each,
    the oracle's slab; a call split by frames equals the oracle applied twice."""
    c = cases(name)
    whole = c.gpu(sfm, gpu)
    same(whole, (c.T, c.W))
    d = c.frames[0].to(gpu)
    tab = sfm.tsdf_block_table(d, 0, 5)
    sfm.tsdf_block_table(d, 5, d.shape[0], out=tab)
    T, W = c.T0, c.W0
    for z0, z1 in SLABS:
        T, W = c.gpu(sfm, gpu, T, W, z0=z0, z1=z1, block_table=tab)
        Tr, Wr = c.oracle(c.T0, c.W0, z0=z0, z1=z1)
        same((T[z0:z1], W[z0:z1]), (Tr[z0:z1], Wr[z0:z1]))
    same((T, W), whole)
    T, W = c.gpu(sfm, gpu, frames=slice(0, 5))
    T, W = c.gpu(sfm, gpu, T, W, frames=slice(5, None))
    same((T, W), c.oracle(*c.oracle(c.T0, c.W0, slice(0, 5)), slice(5, None)))


ODD_FX0, ODD_FAR, ODD_FLIP = 2, 6, 9


@pytest.fixture(scope="module")
def odd_case():
    """Scene B with fx = 0 in one frame (defined: every voxel in front maps to column
    floor(cx + 0.5)), cx = 2^20 in another (every pixel off the image: the frame adds nothing)
    and a third stored bottom-up (fy -> -fy, cy -> Hd - 1 - cy, rendered again)."""
    depth, poses, K = cs.scene_b()
    Hd, Wd = depth.shape[1:]
    K[ODD_FX0, 0] = 0.0
    K[ODD_FAR, 2] = 2.0 ** 20
    K[ODD_FLIP, 1] = -K[ODD_FLIP, 1]
    K[ODD_FLIP, 3] = Hd - 1 - K[ODD_FLIP, 3]
    depth[ODD_FLIP] = cs.render_depth(poses[ODD_FLIP:ODD_FLIP + 1], K[ODD_FLIP:ODD_FLIP + 1], Hd, Wd)[0]
    c = Case(depth, poses, K)
    keep = [f for f in range(depth.shape[0]) if f != ODD_FAR]
    same(c.oracle(c.T0, c.W0, keep), (c.T, c.W))           # the off-image frame adds nothing
    col = int(np.floor(K[ODD_FX0, 2] + np.float32(0.5)))
    only = c.oracle(c.T0, c.W0, slice(ODD_FX0, ODD_FX0 + 1))[1] > c.W0
    assert 0 <= col < Wd and (depth[ODD_FX0][:, col] > 0).any() and only.any()   # and the fx = 0 frame does add
    return c


@pytest.mark.parametrize("lat", LAT_MODES)
def test_odd_intrinsics_stay_local(sfm, gpu, knob, odd_case, lat):
    _set_lat(knob, lat)
    same(odd_case.gpu(sfm, gpu), (odd_case.T, odd_case.W))


@pytest.mark.parametrize("name", ["A", "C"])
def test_fused_views_raycast_back(sfm, gpu, cases, name):
    """Fused on the GPU, then ray-cast at the input cameras (C view 0 is a mirrored frame):
    the depth equals the ray-cast restatement on the same grid bit for bit, and the input
    depth within half a voxel in the median (the gate of test_gpu_tsdf_raycast.py)."""
    c = cases(name)
    views = [0, 1, 5]
    Hd, Wd = c.depth.shape[1:]
    T = torch.zeros(cs.SHAPE, dtype=torch.float32, device=gpu)
    W = torch.zeros_like(T)
    sfm.tsdf_integrate(T, W, *c.frames, *BND, TRUNC)
    step = 0.5 * cs.VOXEL
    got = sfm.tsdf_raycast(T, W, c.frames[1][views], c.frames[2][views], (Hd, Wd), *BND, iso=0.0, min_weight=1.0,
                           near=0.0, far=6.5, step=step)[0]
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    ref = rr.raycast(T.cpu().numpy(), W.cpu().numpy(), c.poses[views], c.K[views], (Hd, Wd), *BND, iso=0.0,
                     min_weight=1.0, near=0.0, step=step, n_samples=rr.sample_count(0.0, 6.5, step))[0]
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    for i, v in enumerate(views):
        hit = got[i] > 0
        both = hit & (c.depth[v] > 0)
        med = float(np.median(np.abs(got[i][both].astype(np.float64) - c.depth[v][both]))) / cs.VOXEL
        print(f"scene {name} view {v}: hit share {hit.mean():.3f}, median |depth_out - depth_in| {med:.3f} voxels")
        assert hit.mean() > 0.03 and med <= 0.5
