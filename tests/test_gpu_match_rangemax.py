"""GPU parity of the value-only match kernel's range maxima (DESIGN.md K1'): the loop keeps the
maximum of each 16-candidate group (a lane's 4 rows x 4 candidate tiles) instead of a per-distance
top two, so a row's second-best value is hidden whenever it shares the group of the best, and the
post-loop rescan of that group has to bring it back before the certificate decides.

Reference: oracle.match.bf_match_exact, indices bit for bit.  Integer MODE_SIFT data (the int8
distances are the exact ones) with dictated squared distances: per query row a best at D1 and a
second at D2, every other candidate thousands away, so a kernel that loses the second accepts the
row.  (9, 16) sits on the ratio boundary (strict <: no match), (9, 17) passes."""
import numpy as np
import pytest
import torch

from oracle import match as om

pytestmark = pytest.mark.gpu

M = 512
NK = np.array([257, 500], np.int32)
PAIRS = np.array([[0, 1]], np.int32)
_STEPS = {1: (1,), 2: (1, 1), 3: (1, 1, 1), 4: (2,), 9: (3,), 16: (4,), 17: (4, 1), 400: (20,)}
DIST = [(9, 16), (9, 17), (1, 2), (2, 3), (4, 400)]
# (query row, best j, second j): candidate j = 128 block + 16 tile + 4 lane group + accumulator,
# a range = 4 tiles = 64 candidates; each position also with the best at the higher index
SAME_GROUP = [(0, 3, 19),        # same group, another tile: j + 16
              (7, 340, 324),
              (14, 69, 70),      # same group, same tile: j + 1 within one row quad
              (21, 398, 397),
              (256, 483, 499)]   # the last, partial block's group {483, 499}: its range holds padded rows
ELSEWHERE = [(28, 130, 134),     # another lane group of the same tile: j + 4
             (35, 150, 146),
             (42, 200, 264),     # the next range: j + 64
             (49, 280, 216),
             (56, 40, 300),      # another block
             (63, 430, 45)]
PLANTS = SAME_GROUP + ELSEWHERE
assert len({j for _, a, b in PLANTS for j in (a, b)}) == 2 * len(PLANTS)
assert all(a // 64 == b // 64 and a % 16 // 4 == b % 16 // 4 for _, a, b in SAME_GROUP)

_cache = {}


def _dataset(d, dist, parity):
    """x [2, M, d], the planted rows and the reference graph; every planted query row has
    |q_a|^2 of the given parity."""
    key = (d, dist, parity)
    if key not in _cache:
        rng = np.random.default_rng(d)
        x = rng.integers(118, 139, (2, M, d)).astype(np.float32)   # q = x - 128 in [-10, 10]
        for r, j1, j2 in PLANTS:
            q = (x[0, r] - 128).astype(np.int64)
            if int(q.dot(q)) % 2 != parity:
                x[0, r, 5] += 1
            q = (x[0, r] - 128).astype(np.int64)
            assert int(q.dot(q)) % 2 == parity
            for j, D in zip((j1, j2), dist):
                x[1, j] = x[0, r]
                for t, step in enumerate(_STEPS[D]):
                    x[1, j, 10 + t] += step
                assert int(((x[1, j] - x[0, r]) ** 2).sum()) == D
        for i, n in enumerate(NK):
            x[i, n:] = 0
        ref = np.full((1, M), -1, np.int64)
        ref[0, :NK[0]] = om.bf_match_exact(x[0, :NK[0]], x[1, :NK[1]], (3, 4))
        _cache[key] = (x, ref)
    return _cache[key]


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32])
@pytest.mark.parametrize("d", [64, 256])
def test_hidden_second_is_recovered(sfm, gpu, d, dtype):
    sets = [(dist, parity, *_dataset(d, dist, parity)) for dist in DIST for parity in (0, 1)]
    # from the reference alone: the same-group rows hold both outcomes, matched rows name the best
    matched = unmatched = 0
    for dist, parity, x, ref in sets:
        for r, j1, _ in PLANTS:
            assert ref[0, r] in (j1, -1), (dist, parity, r)
        rows = [r for r, _, _ in SAME_GROUP]
        matched += int((ref[0, rows] >= 0).sum())
        unmatched += int((ref[0, rows] < 0).sum())
    print(f"same-group planted rows: {matched} matched, {unmatched} unmatched in the reference")
    assert matched >= 4 and unmatched >= 4
    for dist, parity, x, ref in sets:
        bank = sfm.DescriptorBank.from_float(torch.from_numpy(x), n_kpts=NK, mode=sfm.MODE_SIFT, exact=True)
        out = torch.empty((len(PAIRS), M), dtype=dtype, device=gpu)
        m0 = bank.match(PAIRS, ratio=0.75, out=out).cpu().numpy().astype(np.int64)
        bad = np.flatnonzero(m0[0] != ref[0])
        assert bad.size == 0, (dist, parity, bad[:8], m0[0, bad[:8]], ref[0, bad[:8]])
        # the packed-key kernel (distance outputs requested) gives the same graph
        p0 = bank.match(PAIRS, ratio=0.75, with_dist=True)[0].cpu().numpy().astype(np.int64)
        assert np.array_equal(m0, p0), (dist, parity)
