"""Images with known answers for the SIFT tests (test_sift_cpu.py, test_gpu_sift.py)."""
import functools

import numpy as np

# (sigma_b, count): blob sizes chosen inside the scale range of octaves 0, 1 and 2
# (a blob of sigma_b peaks at the scale 2^(-1/6) sigma_b; levels 1..3 of octave o hold the
# scales 2.0 2^o .. 3.2 2^o), away from the seams between levels, where the discrete extremum
# test of any SIFT can lose a blob
BLOB_SIGMAS = [2.3, 2.4, 2.9, 3.0, 3.6, 3.7, 4.7, 5.8, 7.0, 9.4, 10.0]


@functools.lru_cache(maxsize=None)
def blob_image():
    """Isotropic Gaussian blobs, sigma_b from 2.3 to 10, both polarities, at non-integer centres
    on a flat grey background, 12 per octave range.  Returns img (H,W) u8, centres (B,2) f64 (x, y),
    sigmas (B,) f64, signs (B,)."""
    rng = np.random.default_rng(11)
    sig = []
    for s in BLOB_SIGMAS:
        sig += [s] * (2 if s < 4 else (4 if s < 8 else 6))
    sig = np.array(sig)
    # rows of blobs, each cell 9 sigma wide and tall
    W = 560
    cx, cy, x, y, rowh = [], [], 8.0, 8.0, 0.0
    for s in sig:
        cell = 9.0 * s
        if x + cell > W - 8:
            x, y, rowh = 8.0, y + rowh, 0.0
        # non-integer centres, but not within 0.2 of a half pixel of the blob's octave: there the
        # refinement of any SIFT steps to and fro between two samples and gives the candidate up
        step = 1.0 if s < 4 else (2.0 if s < 8 else 4.0)
        cx.append(step * (np.rint((x + cell / 2) / step) + rng.uniform(-0.3, 0.3)))
        cy.append(step * (np.rint((y + cell / 2) / step) + rng.uniform(-0.3, 0.3)))
        x += cell
        rowh = max(rowh, cell)
    H = int(np.ceil(y + rowh + 8))
    sign = np.where(np.arange(sig.size) % 2 == 0, 1.0, -1.0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.full((H, W), 128.0)
    for s, a, b, p in zip(sig, cx, cy, sign):
        img += p * 100.0 * np.exp(-((xx - a) ** 2 + (yy - b) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), np.stack([cx, cy], 1), sig, sign


def step_image(H=96, W=128):
    """A straight step edge (slightly slanted) between two flat halves."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.where(xx + 0.31 * yy > 0.5 * W + 10, 200, 60).astype(np.uint8)


def block_texture(H, W, seed, blocks):
    """Random blocks of each side in `blocks`, averaged and stretched about 128: a few hundred
    keypoints on 233 x 301, more than the 256 one chunk of the orientation emit holds."""
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W), np.float64)
    for b in blocks:
        g = rng.integers(0, 256, (-(-H // b), -(-W // b)))
        img += np.kron(g, np.ones((b, b)))[:H, :W]
    img /= len(blocks)
    return np.clip(np.rint((img - 128) * 1.6 + 128), 0, 255).astype(np.uint8)


def half_flat_texture():
    """The 150 x 203 texture with its right third constant: random records there see no gradient
    (no orientation peak, a descriptor of norm 0)."""
    img = block_texture(150, 203, 1, (3, 7)).copy()
    img[:, 2 * 203 // 3:] = 128
    return img


PLANT = 32          # side of a planted octave
PLANT_BORDER = 5    # the border the planted stencils are placed for


def planted_pyramid(kind):
    """One octave (6, 32, 32) f32 built by hand from its DoG: G[0] = 0, G[k + 1] = G[k] + D[k], all
    values dyadic so that G[k + 1] - G[k] gives D back exactly (asserted).  D is zero but for a
    stencil about a maximum of 64 on DoG level 2: the six axis neighbours 56, the in-level
    diagonals +64 a on (+,+), (-,-) and -64 a on (+,-), (-,+).
      "det0":  a = 0.25: hxx = hyy = hll = -16, hxy = 16: det == 0 exactly.
      "big":   a = 0.25 - 2^-26, x neighbours 60 and 52: det = -2^-11, ox = 2^21 > 1048576.
      "move":  a = 0.125, x neighbours 63 and 49: ox = 0.583, oy = 0.292, ol = 0: one column to the
               right.  Planted on column W - 1 - border (leaves by the column bound) and, on other
               rows, one column inward (moves and goes on).
      "iso":   a = 0: converges at once with hxx = hyy = -16, hxy = 0, so (tr tr) r = 1024 r and
               ((r + 1)(r + 1)) d2 = 256 (r + 1)^2: at edge ratio 1 the two sides are equal, which the
               header rejects (>=); at 10 it is a record.
      "zero":  all zero."""
    n, s = PLANT, 64.0
    D = np.zeros((5, n, n), np.float32)

    def stencil(y, x, a, dxp, dxm):
        D[2, y, x] = s
        D[1, y, x] = D[3, y, x] = D[2, y + 1, x] = D[2, y - 1, x] = 0.875 * s
        D[2, y, x + 1], D[2, y, x - 1] = (0.875 + dxp) * s, (0.875 - dxm) * s
        D[2, y + 1, x + 1] = D[2, y - 1, x - 1] = a * s
        D[2, y + 1, x - 1] = D[2, y - 1, x + 1] = -a * s

    if kind == "det0":
        stencil(14, 15, 0.25, 0.0, 0.0)
    elif kind == "big":
        stencil(14, 15, 0.25 - 2.0 ** -26, 0.0625, 0.0625)
    elif kind == "move":
        stencil(10, n - 1 - PLANT_BORDER, 0.125, 7 / 64, 7 / 64)
        stencil(20, n - 2 - PLANT_BORDER, 0.125, 7 / 64, 7 / 64)
    elif kind == "iso":
        stencil(14, 15, 0.0, 0.0, 0.0)
    elif kind != "zero":
        raise ValueError(kind)
    G = np.zeros((6, n, n), np.float32)
    for k in range(5):
        G[k + 1] = G[k] + D[k]
    assert np.array_equal(G[1:] - G[:-1], D)
    return G


def steep(octs):
    """A pyramid times 2^12 (exact): gradients of order 10^5, so that the integer histogram terms
    of the orientation reach their bound of 4194304."""
    return [g * np.float32(4096.0) for g in octs]


def random_records(octs, n, seed):
    """n records no detector wrote: octave and level uniform, x and y uniform over the level plus
    2 pixels on every side, the scale in [1.8, 3.6]."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 8), np.int32)
    o = rng.integers(0, len(octs), n)
    hw = np.array([g.shape[1:] for g in octs])
    x = rng.uniform(-2.0, hw[o, 1] + 1.0).astype(np.float32)
    y = rng.uniform(-2.0, hw[o, 0] + 1.0).astype(np.float32)
    po = (2.0 ** o).astype(np.float32)
    rec[:, 0], rec[:, 1] = o, rng.integers(1, 4, n)
    fl = np.stack([x, y, rng.uniform(1.8, 3.6, n).astype(np.float32), np.ones(n, np.float32), x * po, y * po], 1)
    rec[:, 2:] = fl.view(np.int32)
    return rec


def reproject(xy, v0, v1, depth, poses, K):
    """Pixels xy (N,2) of view v0 -> their pixels in view v1 through the analytic depth
    (bilinear at xy) and the poses (world -> camera), f64; NaN where the depth is invalid."""
    d = np.asarray(depth[v0], np.float64)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    x0, y0 = np.clip(np.floor(x).astype(int), 0, d.shape[1] - 2), np.clip(np.floor(y).astype(int), 0, d.shape[0] - 2)
    fx, fy = x - x0, y - y0
    c = [d[y0, x0], d[y0, x0 + 1], d[y0 + 1, x0], d[y0 + 1, x0 + 1]]
    z = (c[0] * (1 - fx) + c[1] * fx) * (1 - fy) + (c[2] * (1 - fx) + c[3] * fx) * fy
    z = np.where(np.minimum.reduce(c) > 0, z, np.nan)
    P0, P1 = np.asarray(poses[v0], np.float64), np.asarray(poses[v1], np.float64)
    k0, k1 = np.asarray(K[v0], np.float64), np.asarray(K[v1], np.float64)
    pc = np.stack([(x - k0[2]) / k0[0] * z, (y - k0[3]) / k0[1] * z, z], 1)
    Xw = (pc - P0[:, 3]) @ P0[:, :3]
    q = Xw @ P1[:, :3].T + P1[:, 3]
    return np.stack([k1[0] * q[:, 0] / q[:, 2] + k1[2], k1[1] * q[:, 1] / q[:, 2] + k1[3]], 1)
