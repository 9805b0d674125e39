"""GPU parity of the certifying matcher's value-only form (DESIGN.md K1'): the exact float mode
without distance outputs runs the int8 pass on raw values (no index packed into the keys),
certifies on the interval [Du - 1, Du] and recovers the winner's index for accepted rows only.

Reference: oracle.bf_match_exact, bit-exact indices.  Images of 1..500 keypoints (m_pad 512):
query images with na = 257 (a second workgroup of one row) and na = 1, nb no multiple of 128."""
import numpy as np
import pytest
import torch

from oracle import match as om

pytestmark = pytest.mark.gpu

NK = np.array([257, 500, 301, 1], np.int32)
M = 512
PAIRS = np.array([[0, 1], [3, 1], [1, 2], [2, 0], [1, 0]], np.int32)
CASES = [(64, 1), (128, 0), (128, 1), (256, 0), (256, 1)]   # (d, mode): MODE_SIFT = 0, MODE_FLOAT = 1


def _random_images(d, mode, seed):
    """Independent random rows: no image shares structure with another, so an unplanted row's
    two best candidates are nearly equidistant and the certificate rejects it."""
    rng = np.random.default_rng(seed)
    if mode == 1:
        x = rng.standard_normal((len(NK), M, d)).astype(np.float32)
        x /= np.linalg.norm(x, axis=2, keepdims=True)
    else:
        x = rng.integers(0, 81, (len(NK), M, d)).astype(np.float32) + np.float32(0.37)
    for i, n in enumerate(NK):
        x[i, n:] = 0
    return x, rng


def _near_copy(row, mode, rng):
    if mode == 1:
        return row + (1e-3 * rng.standard_normal(row.shape)).astype(np.float32)
    out = row.copy()
    out[rng.choice(row.shape[0], 3, replace=False)] += 1
    return out


def _planted(d, mode):
    """Image 0's rows get a near-copy in image 1: every in-block offset 0..127 in blocks 0..2,
    offsets 0..115 of the last (partial) block with the last valid row 499, and row 256 (the
    second workgroup); image 3's only row copies image 1's last valid row."""
    x, rng = _random_images(d, mode, 100 + d + mode)
    plant = {}
    for r in range(128):
        plant[r] = (r % 3) * 128 + r
    for r in range(128, 244):
        plant[r] = 3 * 128 + (r - 128)
    plant[256] = 2 * 128 + 127
    assert max(plant.values()) == NK[1] - 1 and len(set(plant.values())) == len(plant)
    for r, j in plant.items():
        x[1, j] = _near_copy(x[0, r], mode, rng)
    x[3, 0] = _near_copy(x[1, NK[1] - 1], mode, rng)
    return x, plant


def _oracle(x, nk, pairs):
    out = np.full((len(pairs), x.shape[1]), -1, np.int64)
    for p, (a, b) in enumerate(pairs):
        out[p, :nk[a]] = om.bf_match_exact(x[a, :nk[a]], x[b, :nk[b]], (3, 4))
    return out


_cache = {}


def _planted_case(d, mode):
    if (d, mode) not in _cache:
        x, plant = _planted(d, mode)
        _cache[(d, mode)] = (x, plant, _oracle(x, NK, PAIRS))
    return _cache[(d, mode)]


def _match(sfm, gpu, x, nk, pairs, mode, dtype):
    bank = sfm.DescriptorBank.from_float(torch.from_numpy(x), n_kpts=nk, mode=mode, exact=True)
    out = torch.empty((len(pairs), x.shape[1]), dtype=dtype, device=gpu)
    m0 = bank.match(pairs, ratio=0.75, out=out).cpu().numpy().astype(np.int64)
    return bank, m0


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32])
@pytest.mark.parametrize("d,mode", CASES)
def test_planted_winners_are_index_recovered(sfm, gpu, d, mode, dtype):
    x, plant, ref = _planted_case(d, mode)
    bank, m0 = _match(sfm, gpu, x, NK, PAIRS, mode, dtype)
    for r, j in plant.items():
        assert m0[0, r] == j, (r, j, m0[0, r])
    assert m0[1, 0] == NK[1] - 1
    assert np.array_equal(m0, ref)
    # a row the resolve settles is counted: had the planted rows (245 of pair 0) gone that way
    # the count would be >= 245; independent random rows are rejected by the certificate, so
    # only stray near-boundary rows remain
    assert int(bank.last_resolved.item()) < len(plant) // 8


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32])
@pytest.mark.parametrize("d,mode", [(64, 1), (256, 0), (256, 1)])
def test_duplicated_best_candidate_goes_to_the_resolve(sfm, gpu, d, mode, dtype):
    """Two identical rows of image b as a query row's best: equal values are never accepted by
    the certificate, the resolve settles them as the oracle does (d1 == d2: no match)."""
    x, rng = _random_images(d, mode, 7 * d + mode)
    dup = {5: (4, 20),        # same lane, two tiles of one block
           6: (132, 137),     # two lane groups of one tile
           7: (40, 300),      # two blocks
           256: (498, 499)}   # the last rows of the partial block, second workgroup
    for r, (j1, j2) in dup.items():
        x[1, j1] = _near_copy(x[0, r], mode, rng)
        x[1, j2] = x[1, j1]
    pairs = PAIRS[:1]
    ref = _oracle(x, NK, pairs)
    bank, m0 = _match(sfm, gpu, x, NK, pairs, mode, dtype)
    assert np.array_equal(m0, ref)
    assert all(ref[0, r] == -1 for r in dup)
    assert int(bank.last_resolved.item()) >= len(dup)


# candidates at these squared distances from a query row (integer data: the int8 distances are
# the exact ones).  D and D + 1 share the value v = (na - D - p) / 2 when na - D is odd, so
# with both parities of na every list below has a pair of equal v and different p_j: as the
# best two, behind a clear best, and around the ratio boundary d1 / d2 = 9 / 16.
_STEPS = {1: (1,), 2: (1, 1), 3: (1, 1, 1), 4: (2,), 5: (2, 1), 6: (2, 1, 1), 9: (3,), 16: (4,), 17: (4, 1)}
_SCENARIOS = [(1, 2), (2, 3), (1, 4, 5), (1, 5, 6), (9, 16), (9, 17), (9, 16, 17), (2, 5, 4)]


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32])
@pytest.mark.parametrize("d", [64, 256])
def test_equal_value_different_parity(sfm, gpu, d, dtype):
    rng = np.random.default_rng(d)
    x = rng.integers(118, 139, (2, M, d)).astype(np.float32)   # q = x - 128 in [-10, 10]
    nk = np.array([257, 500], np.int32)
    r, j = 0, 3
    rows = []
    for sc in _SCENARIOS:
        for flip in (0, 1):            # both parities of |q_a|^2
            x[0, r, 5] += flip
            for D in sc:
                x[1, j] = x[0, r]
                for t, step in enumerate(_STEPS[D]):
                    x[1, j, 10 + t] += step
                assert int(((x[1, j] - x[0, r]) ** 2).sum()) == D
                j += 7                 # positions spread over tiles, lane groups and blocks
            rows.append(r)
            r += 15
    r = 256                             # the second workgroup's only row
    x[1, 499] = x[0, r]
    x[1, 499, 10] += 1
    x[1, 498] = x[1, 499]
    x[1, 498, 11] += 1
    assert j < 498 and rows[-1] < 256
    par = {int((x[0, q] - 128).astype(np.int64).dot((x[0, q] - 128).astype(np.int64))) & 1 for q in rows}
    assert par == {0, 1}
    for i, n in enumerate(nk):
        x[i, n:] = 0
    pairs = np.array([[0, 1]], np.int32)
    ref = _oracle(x, nk, pairs)
    assert (ref[0, rows] >= 0).sum() >= 8 and (ref[0, rows] < 0).sum() >= 2
    _, m0 = _match(sfm, gpu, x, nk, pairs, 0, dtype)
    assert np.array_equal(m0, ref)


@pytest.mark.parametrize("d,mode", [(64, 1), (256, 0), (256, 1)])
def test_distances_requested_keep_the_packed_form(sfm, gpu, d, mode):
    x, plant, ref = _planted_case(d, mode)
    bank = sfm.DescriptorBank.from_float(torch.from_numpy(x), n_kpts=NK, mode=mode, exact=True)
    plain = bank.match(PAIRS, ratio=0.75).cpu().numpy()
    m0, d1, d2 = (t.cpu().numpy() for t in bank.match(PAIRS, ratio=0.75, with_dist=True))
    assert np.array_equal(m0, plain) and np.array_equal(m0, ref)
    q = om.quantize(x, mode)
    for p, (a, b) in enumerate(PAIRS):
        _, r1, r2 = om.bf_match_q(q[a, :NK[a]], q[b, :NK[b]], (3, 4), return_dist=True)
        assert np.array_equal(d1[p, :NK[a]], r1) and np.array_equal(d2[p, :NK[a]], r2)
        assert (d1[p, NK[a]:] == -1).all() and (d2[p, NK[a]:] == -1).all()


def test_empty_int16_call_checks_the_shape(sfm, gpu):
    rc = sfm.lib.sfmhip_match_pairs_i16(None, None, None, None, 1, 32768, 128, None, 0, 3, 4, None, None)
    assert rc == -1 and b"m_pad must be <= 32767" in sfm.lib.sfmhip_last_error()
    rc = sfm.lib.sfmhip_match_pairs_i16(None, None, None, None, 1, 32640, 128, None, 0, 3, 4, None, None)
    assert rc == 0
