"""numpy model of the FP6 (e2m3) integer grid of the match filter (DESIGN.md K1''; include/sfmhip.h,
sfmhip_desc_quantize_fp6): the quantiser, the 6-bit codes and their 24-of-32-byte packing.  Written
from the definition (nearest grid point by search, ties to the even code), not from the kernel's
arithmetic."""
import numpy as np

# magnitude index n = exponent << 3 | mantissa (bias 1) -> 8 x the e2m3 value
GRID = np.array(list(range(0, 16)) + list(range(16, 32, 2)) + list(range(32, 61, 4)), np.int64)
CLIP = 60


def decode(code):
    """8 x the value of a 6-bit e2m3 code (sign << 5 | exponent << 3 | mantissa), from the format's
    definition: subnormal m / 8 for exponent 0, else (1 + m / 8) 2^(e - 1)."""
    code = np.asarray(code, np.int64)
    s, e, m = code >> 5, (code >> 3) & 3, code & 7
    mag8 = np.where(e == 0, m, (8 + m) * (1 << np.maximum(e - 1, 0)))
    return np.where(s == 1, -mag8, mag8)


def quantize(x):
    """x f32 [...] -> (g int8 [...], code uint8 [...]): the grid point nearest to the f32 product
    127 * x, |.| clipped at 60, ties to the even code; g = 0 has code 0."""
    with np.errstate(over="ignore"):                               # a product past f32's range is inf: clipped
        y = np.float32(127.0) * np.asarray(x, np.float32)
    t = np.minimum(np.abs(y.astype(np.float64)), float(CLIP))
    dist = np.abs(t[..., None] - GRID.astype(np.float64))          # exact in f64
    best = dist.min(axis=-1, keepdims=True)
    tie = dist == best                                             # one or two neighbours
    even = (np.arange(GRID.size) % 2 == 0)
    n_first = tie.argmax(axis=-1)
    n_even = (tie & even).argmax(axis=-1)
    n = np.where(tie.sum(axis=-1) > 1, n_even, n_first)
    neg = (y < 0) & (n > 0)
    g = np.where(neg, -GRID[n], GRID[n]).astype(np.int8)
    code = (n | np.where(neg, 32, 0)).astype(np.uint8)
    return g, code


def pack(code):
    """codes uint8 [..., d] (d % 32 == 0) -> bytes uint8 [..., d]: per 32 codes one 32-byte chunk,
    code e at bits 6 e .. 6 e + 5 of its first 24 bytes (little endian), the last 8 bytes zero."""
    code = np.asarray(code, np.uint8)
    d = code.shape[-1]
    c = code.reshape(code.shape[:-1] + (d // 32, 32)).astype(np.uint8)
    bits = (c[..., None] >> np.arange(6, dtype=np.uint8)) & 1      # [..., 32, 6] little endian
    bits = bits.reshape(c.shape[:-1] + (192,))
    by = np.packbits(bits, axis=-1, bitorder="little")             # [..., 24]
    out = np.zeros(c.shape[:-1] + (32,), np.uint8)
    out[..., :24] = by
    return out.reshape(code.shape)


def unpack(by):
    """Inverse of pack; also returns whether every chunk's last 8 bytes are zero."""
    by = np.asarray(by, np.uint8)
    d = by.shape[-1]
    c = by.reshape(by.shape[:-1] + (d // 32, 32))
    bits = np.unpackbits(c[..., :24], axis=-1, bitorder="little").reshape(c.shape[:-1] + (32, 6))
    code = (bits.astype(np.uint8) << np.arange(6, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)
    return code.reshape(by.shape), bool((c[..., 24:] == 0).all())
