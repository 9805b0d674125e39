"""GPU: the seams of the FP6 match filter's software-pipelined block loop (DESIGN.md K1'' "Schedule").

The loop consumes a candidate tile's accumulators under the next tile's MFMAs and folds a finished range
into the top two under the next range, so what can go wrong sits where a tile, a range or a block hands
over: the first tile of the first block, the block boundary (the pending maxima and the carried range
id), ring parity, the drain behind the last block, and ragged last blocks.  The shapes are the smallest
that hold each of these: seven images of 513 .. 1 rows in a bank of m_pad = 640 (one full query block of
512 rows and a ragged second one), every ordered pair, d = 256 and d = 128; as candidate images they give
5, 3, 3, 2, 1 and 1 blocks and the nb_rows < 2 exit.  The graph must equal the oracle's entry for entry,
and the int8 filter's on the same grid values with the same number of rows sent to the f64 pass."""
import importlib

import numpy as np
import pytest
import torch

import fp6_grid_ref as fp6
from oracle import match as om

pytestmark = pytest.mark.gpu

abi = importlib.import_module("3d_reconstruction_amd._abi")

M = 640
NK = np.array([513, 384, 257, 129, 128, 17, 1], np.int32)
PAIRS = np.array([[a, b] for a in range(len(NK)) for b in range(len(NK)) if a != b], np.int32)
# squared grid distances (best, second) and the unit steps that make them (as test_gpu_match_fp6_dense)
_STEPS = {1: (1,), 2: (1, 1), 3: (1, 1, 1), 4: (2,), 9: (3,), 16: (4,), 17: (4, 1), 64: (8,)}
DIST = [(9, 16), (9, 17), (1, 2), (2, 3), (4, 64)]
FAR_DIST = (16, 64)                          # a triple hung on a row that an earlier triple fixed
BIG_DIST = [(144, 256), (144, 272)]          # grid steps of 4 on rows of magnitude 60
BIG_EVERY = 5                                # every 5th free-standing triple is a magnitude-60 row

_cache = {}


def _plan():
    """(query image, query row, candidate image, best, second, kind) for every candidate image with two or
    more rows.  The queries of image 0's candidates are the other images' last valid rows; the others are
    rows of image 0 (0, 511 and 512 among them) or of a neighbour."""
    last = [int(n) - 1 for n in NK]
    plan = []

    def add(b, queries, positions):
        assert len(queries) == len(positions)
        for (a, r), (j1, j2, kind) in zip(queries, positions):
            plan.append((a, r, b, j1, j2, kind))

    def positions(nk, first, group, spare):
        p = [(first, spare[0], "tile0"), (nk - 1, spare[1], "last")]
        if nk > 128:
            p.append((127, 128, "block"))
        if nk > 256:
            p.append((255, 256, "block"))
        if nk > 64:
            p.append((63, 64, "range"))
        p.append((group[0], group[1], "group"))
        return p

    add(0, [(1, last[1]), (2, last[2]), (3, last[3]), (4, last[4]), (5, last[5]), (6, 0)],
        positions(513, 5, (70, 86), (300, 200)))
    add(1, [(0, 0), (0, 511), (0, 512), (0, 100), (0, 301), (0, 505)], positions(384, 3, (200, 216), (150, 10)))
    add(2, [(0, 16), (0, 17), (0, 250), (0, 270), (0, 400), (0, 496)], positions(257, 7, (140, 156), (100, 40)))
    add(3, [(1, 1), (1, 6), (1, 130), (1, 260), (1, 382)], positions(129, 12, (20, 36), (50, 90)))
    add(4, [(2, 0), (2, 1), (2, 129), (2, 254)], positions(128, 15, (100, 116), (30, 70)))
    add(5, [(3, 0), (3, 65), (3, 100)], positions(17, 9, (2, 1), (13, 4)))
    return plan


def _check_coverage(plan):
    """Every seam is planted, read off the plan alone."""
    nblk = [(int(n) + 127) // 128 for n in NK]
    assert nblk[:6] == [5, 3, 3, 2, 1, 1] and NK[6] < 2      # odd and even block counts, one block, the early exit
    assert sorted(int(n) - 128 * (k - 1) for n, k in zip(NK[:6], nblk)) == [1, 1, 1, 17, 128, 128]   # ragged ends
    assert 129 - 128 == 1 and 257 - 256 == 1 and 513 - 512 == 1 and int(NK[5]) == 17
    for b, nk in enumerate(NK):
        mine = [(j1, j2, kind) for _, _, bb, j1, j2, kind in plan if bb == b]
        if nk < 2:
            assert not mine
            continue
        assert any(j1 < 16 for j1, _, _ in mine)                                      # best in tile 0 of block 0
        assert any(j1 == nk - 1 for j1, _, _ in mine)                                 # best in the last valid row
        for lo in (127, 255):                                                          # tile 7 -> tile 0 of the next block
            assert (lo + 1 >= nk) or any(j1 == lo and j2 == lo + 1 for j1, j2, _ in mine)
        assert nk <= 64 or any(j1 == 63 and j2 == 64 for j1, j2, _ in mine)            # across a range boundary
        assert any(j1 // 64 == j2 // 64 and j1 % 16 // 4 == j2 % 16 // 4 and j1 != j2 for j1, j2, _ in mine)
        assert all(0 <= j < nk for j1, j2, _ in mine for j in (j1, j2))
    queries = {(a, r) for a, r, *_ in plan}
    assert len(queries) == len(plan)
    assert {(0, 0), (0, 511), (0, 512)} <= queries                                     # row 512 is image 0's last
    assert {(i, int(NK[i]) - 1) for i in range(1, 6)} <= queries                       # last valid rows
    assert all(0 <= r < NK[a] for a, r in queries)


def _dataset(d):
    """g int [7, M, d] on the grid, x = g / 127 in f32, the reference graph of every pair, the plan."""
    if d in _cache:
        return _cache[d]
    rng = np.random.default_rng(d + 77)
    g = rng.integers(-6, 7, (len(NK), M, d)).astype(np.int64)
    plan = _plan()
    _check_coverage(plan)
    fixed = set()
    n = free_standing = 0

    def step_from(src, D):
        """src plus unit steps that make the squared distance D; coordinates move with n"""
        nonlocal n
        row = src.copy()
        for t, step in enumerate(_STEPS[D]):
            k = (37 * n + 61 * t + (d // 2) * (n % 2)) % d
            row[k] += step if row[k] <= 0 else -step
        n += 1
        assert int(((row - src) ** 2).sum()) == D
        return row

    for a, r, b, j1, j2, _ in plan:
        q, c1, c2 = (a, r), (b, j1), (b, j2)
        assert not (c1 in fixed and c2 in fixed) and not (q in fixed and (c1 in fixed or c2 in fixed))
        if c1 in fixed or c2 in fixed:
            # the row belongs to an earlier triple: hang the query on it, far enough not to disturb that triple
            D1, D2 = FAR_DIST
            if c1 in fixed:
                g[q] = step_from(g[c1], D1)
                g[c2] = step_from(g[q], D2)
            else:
                g[q] = step_from(g[c2], D2)
                g[c1] = step_from(g[q], D1)
        else:
            big = free_standing % BIG_EVERY == 2 and q not in fixed               # a fixed query keeps its value
            if big:
                g[q] = 60 * rng.choice([-1, 1], d)
                D1, D2 = BIG_DIST[free_standing % 2]
                for c, D in ((c1, D1), (c2, D2)):
                    g[c] = g[q]
                    k = rng.choice(d, D // 16, replace=False)
                    g[c][k] -= 4 * np.sign(g[c][k])                                   # 60 -> 56: one grid step of 4
                    assert int(((g[c] - g[q]) ** 2).sum()) == D
            else:
                D1, D2 = DIST[free_standing % len(DIST)]
                g[c1] = step_from(g[q], D1)
                g[c2] = step_from(g[q], D2)
            free_standing += 1
        fixed |= {q, c1, c2}
    for i, nk in enumerate(NK):
        g[i, nk:] = 0
    assert np.isin(np.abs(g), fp6.GRID).all()
    assert (np.abs(g) == 60).any()
    x = (g / 127.0).astype(np.float32)
    ref = np.full((len(PAIRS), M), -1, np.int64)
    for p, (a, b) in enumerate(PAIRS):
        if NK[b] >= 2:
            ref[p, :NK[a]] = om.bf_match_exact(x[a, :NK[a]], x[b, :NK[b]], (3, 4))
    # CPU check before any GPU run: a planted row names its best or nothing, and a quarter of them match
    pair_of = {(int(a), int(b)): p for p, (a, b) in enumerate(PAIRS)}
    got = [int(ref[pair_of[(a, b)], r]) for a, r, b, *_ in plan]
    assert all(m in (j1, -1) for m, (_, _, _, j1, _, _) in zip(got, plan)), list(zip(got, plan))
    assert sum(m >= 0 for m in got) >= len(plan) // 4 + (len(plan) % 4 > 0)
    _cache[d] = (g, x, ref)
    return _cache[d]


def _match(bank, dtype, gpu):
    out = torch.empty((len(PAIRS), bank.m_pad), dtype=dtype, device=gpu)
    m0 = bank.match(PAIRS, ratio=0.75, out=out).cpu().numpy().astype(np.int64)
    return m0, int(bank.last_resolved.item())


@pytest.mark.parametrize("d", [256, 128])
def test_seams_of_the_pipelined_loop(sfm, gpu, knob, d):
    g, x, ref = _dataset(d)
    bank = sfm.DescriptorBank.from_float(torch.from_numpy(x), n_kpts=NK, mode=sfm.MODE_FLOAT, exact=True)
    assert bank.m_pad == M and bank.code is not None
    assert np.array_equal(bank.g.cpu().numpy().astype(np.int64), g)               # the data lies on the grid
    res = {}
    for fp6_on in (1, 0):
        knob("MATCH_FP6", fp6_on)
        for dtype in (torch.int16, torch.int32):
            m0, nres = _match(bank, dtype, gpu)
            bad = np.argwhere(m0 != ref)
            assert bad.size == 0, (fp6_on, dtype, [tuple(PAIRS[p]) + (r,) for p, r in bad[:8]],
                                   m0[tuple(bad[:8].T)], ref[tuple(bad[:8].T)])
            res[(fp6_on, dtype)] = nres
    valid_rows = int(sum(NK[a] for a, _ in PAIRS))
    print(f"d {d}: rows resolved {res} of {valid_rows} valid rows")
    for dtype in (torch.int16, torch.int32):
        assert res[(1, dtype)] == res[(0, dtype)], res                            # the same rows go to the f64 pass
    assert res[(1, torch.int32)] < valid_rows // 4                                # the filter decided most rows
