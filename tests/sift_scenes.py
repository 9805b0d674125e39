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
