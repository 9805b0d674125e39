"""CPU: the numpy model of the dense FP6 operand rows (DESIGN.md K1'' "Layout") that
tests/test_gpu_match_fp6_dense.py holds sfmhip_desc_pack_fp6 to."""
import numpy as np
import pytest

import fp6_dense_ref as dense
import fp6_grid_ref as fp6


@pytest.mark.parametrize("d", [128, 256])
def test_pack_then_unpack_is_the_identity(d):
    rng = np.random.default_rng(d)
    codes = rng.integers(0, 64, (3, 7, d)).astype(np.uint8)
    chunks = fp6.pack(codes)
    rows = dense.pack_dense(chunks)
    assert rows.shape == (3, 7, 3 * d // 4) and rows.dtype == np.uint8
    back = dense.unpack_dense(rows)
    assert np.array_equal(back, chunks)
    got, zero_tail = fp6.unpack(back)
    assert zero_tail and np.array_equal(got, codes)


@pytest.mark.parametrize("d", [128, 256])
def test_every_code_at_every_position(d):
    """Row v holds code (v + p + 5 s) % 64 at position p of slot s: over the 64 rows every code value
    sits at every position of every slot, and the row's bytes hold it where the layout says."""
    v, s, p = np.meshgrid(np.arange(64), np.arange(d // 32), np.arange(32), indexing="ij")
    codes = ((v + p + 5 * s) % 64).astype(np.uint8).reshape(64, d)
    for pos in range(32):
        for slot in range(d // 32):
            assert set(codes[:, 32 * slot + pos].tolist()) == set(range(64))
    rows = dense.pack_dense(fp6.pack(codes))
    for r in range(64):
        for slot in range(d // 32):
            assert dense.slot_codes(rows[r], slot) == codes[r, 32 * slot:32 * slot + 32].tolist(), (r, slot)
    got, zero_tail = fp6.unpack(dense.unpack_dense(rows))
    assert zero_tail and np.array_equal(got, codes)


@pytest.mark.parametrize("d", [128, 256])
def test_pieces_are_aligned_and_cover_the_row(d):
    one = np.zeros(d, np.uint8)
    seen = np.zeros(3 * d // 4, np.int64)
    for e in range(d):
        one[:] = 0
        one[e] = 63
        row = dense.pack_dense(fp6.pack(one))
        nz = np.flatnonzero(row)
        s, p = divmod(e, 32)
        byte = (6 * p) // 8                                            # first byte of the code inside its 24
        at = 16 * s + byte if byte < 16 else d // 2 + 8 * s + byte - 16
        assert nz[0] == at and nz.size <= 2, (e, nz)
        seen[nz] += 1
    assert (seen > 0).all()                                            # no padding byte in a dense row
    assert (d // 2) % 8 == 0 and (3 * d // 4) % 16 == 0                # 8-byte high pieces, 16-byte rows
