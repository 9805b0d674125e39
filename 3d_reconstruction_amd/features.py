"""V11: SIFT keypoints and descriptors (build-defined; the semantics are the V11 block of
include/sfmhip.h, restated in numpy by tests/sift_ref.py).

* :func:`sift_tables` — the Gaussian taps, window tables, cell weights and the cos/sin table
  the kernels take as inputs (f64 on the host, rounded to f32: no device transcendentals).
* :func:`sift_pyramid`, :func:`sift_detect`, :func:`sift_orient`, :func:`sift_describe` — the
  four stages, thin wrappers returning device tensors.
* :func:`sift` — the four together: images in; counts, positions, scales, orientations,
  responses and uint8 descriptors out (what ``Matcher(features="sift")`` / ``MODE_SIFT`` takes).

The first octave is the image itself (no doubling), and all images of a call have one size.
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import torch

from ._abi import call, dev, ptr, require_gpu, stream_ptr
from .mvs import _grey

S = 3                 # intervals per octave
L = S + 3             # Gaussian levels per octave
SIGMA0 = 1.6
INPUT_BLUR = 0.5
TAP_STRIDE = 27
REC_WORDS = 8
MAX_PEAKS = 4
# record words (int32; the floats by their bits)
R_OCT, R_LEVEL, R_X, R_Y, R_SCALE, R_RESP, R_IMX, R_IMY = range(8)


@functools.lru_cache(maxsize=None)
def _tables_host():
    sig = SIGMA0 * 2.0 ** (np.arange(L, dtype=np.float64) / S)
    inc = np.empty(L)
    inc[0] = math.sqrt(sig[0] ** 2 - INPUT_BLUR ** 2)
    inc[1:] = np.sqrt(sig[1:] ** 2 - sig[:-1] ** 2)
    radii = np.ceil(4.0 * inc).astype(np.int32)
    taps = np.zeros((L, TAP_STRIDE), np.float32)
    for s in range(L):
        k = np.arange(-radii[s], radii[s] + 1, dtype=np.float64)
        g = np.exp(-k * k / (2.0 * inc[s] ** 2))
        taps[s, :g.size] = (g / g.sum()).astype(np.float32)
    i = np.arange(17, dtype=np.float64) - 8.0
    wo = np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2.0 * (8.0 / 3.0) ** 2)).astype(np.float32)
    a = np.arange(16, dtype=np.float64) - 7.5
    wd = np.exp(-(a[:, None] ** 2 + a[None, :] ** 2) / (2.0 * 8.0 ** 2)).astype(np.float32)
    r = (np.arange(16, dtype=np.float64) - 1.5) / 4.0
    cw = np.maximum(0.0, 1.0 - np.abs(r[None, :] - np.arange(4.0)[:, None])).astype(np.float32)
    ang = 2.0 * np.pi * np.arange(1024, dtype=np.float64) / 1024.0
    cs = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    out = dict(sig=sig.astype(np.float32), radii=radii, taps=taps, wo=wo, wd=wd, cw=cw, cs=cs)
    for v in out.values():
        v.setflags(write=False)
    return out


def sift_tables() -> dict:
    """The inputs of the V11 kernels as read-only numpy arrays: ``sig`` (6,) f32 the level
    sigmas 1.6 2^(s/3); ``radii`` (6,) int32 and ``taps`` (6, 27) f32 the blur of each level
    (level 0 from the assumed input blur 0.5, level s from level s - 1; radius ceil(4 sigma),
    normalised in f64); ``wo`` (17, 17) the orientation window; ``wd`` (16, 16) the descriptor
    window; ``cw`` (4, 16) the bilinear weight of sample a in cell k; ``cs`` (1024, 2) cos and
    sin of q/1024 turn."""
    return _tables_host()


@functools.lru_cache(maxsize=8)
def _tables_dev(device_index: int) -> dict:
    t = _tables_host()
    d = torch.device("cuda", device_index)
    return {k: torch.from_numpy(np.array(t[k])).to(d) for k in ("sig", "taps", "wo", "wd", "cw", "cs")}


def _dev_tables() -> dict:
    return _tables_dev(require_gpu().index)


def default_octaves(H: int, W: int) -> int:
    """floor(log2 min(H, W)) - 3, at least 1."""
    return max(1, int(math.floor(math.log2(min(H, W)))) - 3)


def pyramid_layout(H: int, W: int, O: int):
    """[(H_o, W_o, off_o)] per octave and the floats per view of the pyramid buffer."""
    dims, off = [], 0
    for o in range(O):
        h, w = ((H - 1) >> o) + 1, ((W - 1) >> o) + 1
        dims.append((h, w, off))
        off += L * h * w
    return dims, off


def _check_octaves(H: int, W: int, O: int) -> None:
    if not (1 <= O <= 16 and (min(H, W) >> (O - 1)) >= 1):
        raise ValueError(f"{O} octaves do not fit a {H} x {W} image")


def sift_pyramid(images, octaves: int | None = None, taps=None, radii=None) -> torch.Tensor:
    """Gaussian pyramid of V grey images (V,H,W) u8 -> (V, per) f32 on the device, laid out
    as :func:`pyramid_layout` says (step 1 of the V11 block).  ``taps`` (6,27) f32 / ``radii``
    (6,) override the tables of :func:`sift_tables`."""
    gpu = require_gpu()
    img = dev(images, torch.uint8)
    if img.dim() != 3 or img.shape[1] < 1 or img.shape[2] < 1:
        raise ValueError(f"images must be (V,H,W) with H, W >= 1, got {tuple(img.shape)}")
    V, H, W = img.shape
    O = default_octaves(H, W) if octaves is None else int(octaves)
    _check_octaves(H, W, O)
    tp = _dev_tables()["taps"] if taps is None else dev(np.asarray(taps, np.float32), torch.float32)
    rd = np.ascontiguousarray(sift_tables()["radii"] if radii is None else radii, dtype=np.int32)
    if tuple(tp.shape) != (L, TAP_STRIDE) or rd.shape != (L,):
        raise ValueError("taps must be (6, 27) and radii (6,)")
    _, per = pyramid_layout(H, W, O)
    pyr = torch.empty((V, per), dtype=torch.float32, device=gpu)
    call("sfmhip_sift_pyramid", ptr(img), V, H, W, O, ptr(tp), rd.ctypes.data_as(ctypes.c_void_p), ptr(pyr),
         stream_ptr())
    return pyr


def _pyr(pyr, H: int, W: int, O: int) -> torch.Tensor:
    _check_octaves(H, W, O)
    p = dev(pyr, torch.float32)
    if p.dim() != 2 or p.shape[1] != pyramid_layout(H, W, O)[1]:
        raise ValueError(f"a pyramid of {O} octaves of {H} x {W} is (V, {pyramid_layout(H, W, O)[1]}), "
                         f"got {tuple(p.shape)}")
    return p


def sift_detect(pyr, H: int, W: int, O: int, cap: int, contrast: float = 0.04, edge: float = 10.0, border: int = 5):
    """Scale-space extrema of a pyramid with the quadratic refinement and the contrast and edge
    tests (step 2).  Returns ``rec`` (V, cap, 8) int32 — octave, level, then x, y (octave
    pixels), scale (octave pixels), response, x, y (image pixels) as f32 bits — in ascending
    (octave, level, row, column) of the start sample, and ``count`` (V,) int32, the true totals
    (only the first ``cap`` are written; rows beyond stay 0)."""
    gpu = require_gpu()
    p = _pyr(pyr, H, W, O)
    V, cap, border = p.shape[0], int(cap), int(border)
    if cap < 0 or border < 1:
        raise ValueError(f"cap must be >= 0 and border >= 1, got {cap} / {border}")
    rec = torch.zeros((V, cap, REC_WORDS), dtype=torch.int32, device=gpu)
    count = torch.zeros((V,), dtype=torch.int32, device=gpu)
    pre = float(np.float32(0.5 * float(contrast) / S * 255.0))
    thr = float(np.float32(float(contrast) * 255.0))
    call("sfmhip_sift_detect", ptr(p), V, H, W, O, ptr(_dev_tables()["sig"]), border, pre, thr, float(np.float32(edge)),
         cap, ptr(rec), ptr(count), stream_ptr())
    return rec, count


def sift_orient(pyr, H: int, W: int, O: int, rec, count, cap_o: int):
    """Orientation assignment (step 3): every record gives up to 4 oriented records, word 1
    becoming ``level | (q << 8)`` with q the orientation in 1/1024 turn.  Returns ``orec``
    (V, cap_o, 8) int32 and ``ocount`` (V,) int32 (the true totals)."""
    gpu = require_gpu()
    p = _pyr(pyr, H, W, O)
    rc, ct = dev(rec, torch.int32), dev(count, torch.int32)
    V, cap_o = p.shape[0], int(cap_o)
    if rc.dim() != 3 or rc.shape[0] != V or rc.shape[2] != REC_WORDS or tuple(ct.shape) != (V,) or cap_o < 0:
        raise ValueError(f"rec must be ({V}, cap, 8) and count ({V},), got {tuple(rc.shape)} / {tuple(ct.shape)}")
    orec = torch.zeros((V, cap_o, REC_WORDS), dtype=torch.int32, device=gpu)
    ocount = torch.zeros((V,), dtype=torch.int32, device=gpu)
    call("sfmhip_sift_orient", ptr(p), V, H, W, O, ptr(rc), ptr(ct), rc.shape[1], ptr(_dev_tables()["wo"]), cap_o,
         ptr(orec), ptr(ocount), stream_ptr())
    return orec, ocount


def sift_describe(pyr, H: int, W: int, O: int, orec, ocount) -> torch.Tensor:
    """The 4 x 4 x 8 descriptor of every oriented record (step 4): (V, cap_o, 128) uint8 on the
    device, rows beyond the count 0."""
    gpu = require_gpu()
    p = _pyr(pyr, H, W, O)
    rc, ct = dev(orec, torch.int32), dev(ocount, torch.int32)
    V = p.shape[0]
    if rc.dim() != 3 or rc.shape[0] != V or rc.shape[2] != REC_WORDS or tuple(ct.shape) != (V,):
        raise ValueError(f"orec must be ({V}, cap_o, 8) and ocount ({V},), got {tuple(rc.shape)} / {tuple(ct.shape)}")
    t = _dev_tables()
    desc = torch.zeros((V, rc.shape[1], 128), dtype=torch.uint8, device=gpu)
    call("sfmhip_sift_describe", ptr(p), V, H, W, O, ptr(rc), ptr(ct), rc.shape[1], ptr(t["wd"]), ptr(t["cw"]),
         ptr(t["cs"]), ptr(desc), stream_ptr())
    return desc


def sift(images, max_num_keypoints: int = 2048, contrast: float = 0.04, edge: float = 10.0, border: int = 5,
         octaves: int | None = None, bgr: bool = False, cap: int | None = None) -> dict:
    """SIFT features of V images of one size: (V,H,W) u8 grey, or (V,H,W,3|4) u8 reduced by
    :func:`~.mvs.mvs_depth`'s grey rule (``bgr=True``: the channels are b, g, r).

    Runs the four stages; ``cap`` is the first guess of the keypoints per image (default
    ``4 max_num_keypoints``): when an image has more, detection (or orientation) is run once
    more with the reported count, never truncated.  Where an image has more oriented keypoints
    than ``max_num_keypoints`` the strongest by response are kept, in the order of a stable
    descending sort; otherwise the order is that of detection.

    Returns a dict of device tensors padded to K = the largest count: ``count`` (V,) int32,
    ``keypoints`` (V,K,2) f32 (x, y in image pixels), ``scales`` (V,K) f32 (sigma in image
    pixels), ``orientations`` (V,K) f32 (radians, multiples of 2 pi/1024), ``responses`` (V,K)
    f32, ``octaves`` (V,K) int32 and ``descriptors`` (V,K,128) uint8."""
    gpu = require_gpu()
    if not isinstance(images, torch.Tensor):
        images = torch.as_tensor(np.asarray(images))
    if bgr and images.dim() == 4 and images.shape[3] >= 3:
        images = torch.cat([images[..., :3].flip(-1), images[..., 3:]], dim=-1)
    img = _grey(images)
    V, H, W = img.shape
    kmax = int(max_num_keypoints)
    if kmax < 0:
        raise ValueError(f"max_num_keypoints must be >= 0, got {kmax}")
    O = default_octaves(H, W) if octaves is None else int(octaves)
    pyr = sift_pyramid(img, O)
    cap = max(4 * kmax, 256) if cap is None else int(cap)
    rec, count = sift_detect(pyr, H, W, O, cap, contrast, edge, border)
    most = int(count.max()) if V else 0
    if most > cap:
        rec, count = sift_detect(pyr, H, W, O, most, contrast, edge, border)
    cap_o = most + most // 2 + 16
    orec, ocount = sift_orient(pyr, H, W, O, rec, count, cap_o)
    omost = int(ocount.max()) if V else 0
    if omost > cap_o:
        orec, ocount = sift_orient(pyr, H, W, O, rec, count, omost)
    K = min(omost, kmax)
    if omost > kmax:   # plumbing, not the hot path: the strongest kmax per image, ties in input order
        resp = orec[:, :, R_RESP].view(torch.float32).clone()
        resp[torch.arange(orec.shape[1], device=gpu)[None, :] >= ocount[:, None]] = -1.0
        order = torch.sort(resp, dim=1, descending=True, stable=True).indices[:, :K]
        orec = torch.gather(orec, 1, order[:, :, None].expand(-1, -1, REC_WORDS)).contiguous()
        ocount = torch.clamp(ocount, max=K)
    else:
        orec = orec[:, :K].contiguous()
    desc = sift_describe(pyr, H, W, O, orec, ocount)
    f = orec.view(torch.float32)
    valid = torch.arange(K, device=gpu)[None, :] < ocount[:, None]
    octv = torch.where(valid, orec[:, :, R_OCT], 0)
    q = (orec[:, :, R_LEVEL] >> 8) & 1023
    zero = torch.zeros((), dtype=torch.float32, device=gpu)
    return dict(count=ocount,
                keypoints=torch.where(valid[:, :, None], f[:, :, R_IMX:R_IMY + 1], zero),
                scales=torch.where(valid, f[:, :, R_SCALE] * torch.pow(2.0, octv.to(torch.float32)), zero),
                orientations=torch.where(valid, q.to(torch.float32) * float(np.float32(2.0 * np.pi / 1024.0)), zero),
                responses=torch.where(valid, f[:, :, R_RESP], zero),
                octaves=octv,
                descriptors=desc)
