"""numpy model of the dense FP6 operand rows the match kernel reads (DESIGN.md K1'' "Layout";
include/sfmhip.h, sfmhip_desc_pack_fp6).  Written from the layout text, not from the kernel:

  a row of d codes is d / 32 slots; slot s holds codes 32 s .. 32 s + 31 as 24 bytes, code p of the slot
  at bits 6 p .. 6 p + 5 (little endian) — the first 24 bytes of the quantiser's 32-byte chunk s;
  the dense row is 3 d / 4 bytes: the low piece of slot s (bytes 0 .. 15 of the 24) at row byte 16 s,
  the high piece (bytes 16 .. 23) at row byte d / 2 + 8 s.
"""
import numpy as np


def pack_dense(chunks):
    """chunks uint8 [..., d] (fp6_grid_ref.pack: one 32-byte chunk per 32 codes) -> uint8 [..., 3 d / 4]."""
    chunks = np.asarray(chunks, np.uint8)
    d = chunks.shape[-1]
    c = chunks.reshape(chunks.shape[:-1] + (d // 32, 32))
    out = np.zeros(chunks.shape[:-1] + (3 * d // 4,), np.uint8)
    for s in range(d // 32):
        out[..., 16 * s:16 * s + 16] = c[..., s, 0:16]
        out[..., d // 2 + 8 * s:d // 2 + 8 * s + 8] = c[..., s, 16:24]
    return out


def unpack_dense(dense):
    """Inverse of pack_dense: uint8 [..., 3 d / 4] -> the 32-byte chunks uint8 [..., d] (zero tails)."""
    dense = np.asarray(dense, np.uint8)
    d = dense.shape[-1] * 4 // 3
    c = np.zeros(dense.shape[:-1] + (d // 32, 32), np.uint8)
    for s in range(d // 32):
        c[..., s, 0:16] = dense[..., 16 * s:16 * s + 16]
        c[..., s, 16:24] = dense[..., d // 2 + 8 * s:d // 2 + 8 * s + 8]
    return c.reshape(dense.shape[:-1] + (d,))


def slot_codes(row, s):
    """The 32 codes of slot s of one dense row, read bit by bit from the row's bytes."""
    row = np.asarray(row, np.uint8)
    d = row.shape[-1] * 4 // 3
    by = bytes(row[16 * s:16 * s + 16]) + bytes(row[d // 2 + 8 * s:d // 2 + 8 * s + 8])
    v = int.from_bytes(by, "little")
    return [(v >> (6 * p)) & 63 for p in range(32)]
