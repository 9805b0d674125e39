"""The value-only match kernel's top two from range maxima (DESIGN.md K1'), restated in numpy on an
integer value matrix V[row, candidate] (v = <b_j, a_i> + h_j in the kernel).

A lane group g of the kernel sees, per 16-candidate tile, the rows 4g..4g+3; a range is VG tiles
and a group the 4 VG values a lane group sees in one range.  The loop keeps, per lane group, the
top two w1 >= w2 of the group maxima and the range where w1 rose (strictly); the lane groups merge
by a butterfly that keeps the smaller (range, lane group) on equal bests; the recorded group is
rescanned for the value the maxima can hide.  The outcome must be the exact top two of the row as
a multiset, and the winner's index whenever the best is unique."""
import numpy as np
import pytest

MF, NG = 16, 4   # candidate rows per tile, lane groups
INT_MIN = np.iinfo(np.int32).min


def _group_maxima(V, vg):
    """[rows, ranges, NG] maxima in the kernel's candidate order."""
    n = V.shape[1]
    t = V.reshape(V.shape[0], n // (vg * MF), vg, NG, 4)   # range, tile, lane group, accumulator
    return t.max(axis=(2, 4))


def _lane_scan(Mx):
    """Per lane group: top two of its maxima over the ranges and the range of the best."""
    rows, nr, _ = Mx.shape
    w1 = np.full((rows, NG), INT_MIN, np.int64)
    w2 = w1.copy()
    wr = np.zeros((rows, NG), np.int64)
    for rid in range(nr):
        r = Mx[:, rid, :]
        wr = np.where(r > w1, rid, wr)
        w2 = np.sort(np.stack([w1, w2, r]), axis=0)[1]   # med3
        w1 = np.maximum(w1, r)
    return w1, w2, wr


def _merge(w1, w2, wr):
    a1, a2 = w1.copy(), w2.copy()
    al = wr * NG + np.arange(NG)
    for off in (1, 2):   # lane xor 16, 32
        p = np.arange(NG) ^ off
        o1, o2, ol = a1[:, p], a2[:, p], al[:, p]
        mine = (a1 > o1) | ((a1 == o1) & (al < ol))
        a2 = np.maximum(np.maximum(np.minimum(a1, o1), a2), o2)
        al = np.where(mine, al, ol)
        a1 = np.maximum(a1, o1)
    assert (a1 == a1[:, :1]).all() and (a2 == a2[:, :1]).all() and (al == al[:, :1]).all()
    return a1[:, 0], a2[:, 0], al[:, 0]


def _group_candidates(loc, vg):
    """[rows, 4 vg] candidate indices of the group `loc` (the kernel's j0 + (c >> 2) MF + (c & 3))."""
    j0 = (loc // NG) * vg * MF + 4 * (loc % NG)
    c = np.arange(4 * vg)
    return j0[:, None] + (c >> 2) * MF + (c & 3)


def rangemax_top2(V, vg):
    v1, v2p, loc = _merge(*_lane_scan(_group_maxima(V, vg)))
    cand = _group_candidates(loc, vg)
    u = np.take_along_axis(V, cand, axis=1)
    hit = u == v1[:, None]
    nh = hit.sum(axis=1)
    assert (nh >= 1).all()                        # the recorded group attains v1
    x = np.where(hit, INT_MIN, u).max(axis=1)     # the largest of the others
    x = np.where(nh >= 2, v1, x)
    idx = np.where(nh == 1, np.take_along_axis(cand, hit.argmax(axis=1)[:, None], axis=1)[:, 0], -1)
    return v1, np.maximum(v2p, x), v2p, idx


def _exact_top2(V):
    s = np.sort(V, axis=1)
    return s[:, -1], s[:, -2]


def _check(V, vg):
    v1, v2, v2p, idx = rangemax_top2(V, vg)
    e1, e2 = _exact_top2(V)
    assert np.array_equal(v1, e1)
    assert np.array_equal(v2, e2)
    assert (v2p <= e2).all()
    uniq = e1 > e2
    assert np.array_equal(idx[uniq], V.argmax(axis=1)[uniq])   # a unique best is found
    return v2p < e2                                            # rows whose second the maxima hid


@pytest.mark.parametrize("vg", [1, 2, 4, 8])
@pytest.mark.parametrize("n,span", [(128, 3), (384, 6), (512, 40)])
def test_random_values_with_ties(vg, n, span):
    rng = np.random.default_rng(1000 * vg + n)
    V = rng.integers(-span, span + 1, (300, n)).astype(np.int64)
    _check(V, vg)


@pytest.mark.parametrize("vg", [1, 2, 4, 8])
def test_adversarial_rows(vg):
    n = 384
    rng = np.random.default_rng(vg)
    base = rng.integers(-50, 0, (8, n)).astype(np.int64)
    cand = _group_candidates(np.array([2 * NG + 1, 0, NG + 3]), vg)   # three groups' members
    rows = []

    def row(k, vals):
        v = base[k % len(base)].copy()
        for j, x in vals.items():
            v[j] = x
        rows.append(v)

    for g in cand:
        a, b = int(g[0]), int(g[-1])
        other = int((b + 4) % n) if (b + 4) % n not in g else int((b + 8) % n)
        row(0, {a: 90, b: 80})                    # best and second in one group
        row(1, {b: 90, a: 80})                    # ... the best later
        row(2, {a: 90, b: 90})                    # the best twice in one group
        row(3, {a: 90, b: 90, other: 85})
        row(4, {a: 90, other: 90})                # the best in two groups
        row(5, {a: 90, other: 90, b: 89})
        row(6, {a: 90, b: 80, other: 85})         # the hidden one is only the third
        row(7, {a: 90, b: 85, other: 80})         # hidden second above the other groups' best
    rows.append(np.full(n, 7, np.int64))          # everything equal
    rows.append(np.full(n, -2 ** 23, np.int64))   # ... at the padded rows' value
    V = np.stack(rows)
    hidden = _check(V, vg)
    assert hidden.sum() >= 6                      # the rescan was needed


def test_padded_tail_values():
    """The last block's padded rows carry v = -2^23: below every valid value, ties among themselves."""
    rng = np.random.default_rng(5)
    V = rng.integers(-9, 10, (200, 512)).astype(np.int64)
    V[:, 500:] = -2 ** 23
    V[0, :499] = -2 ** 23 + 1                     # one valid value above the padding, at 499
    V[1, 1:500] = -2 ** 23                        # a single candidate that is not padding-valued
    V[2, 483], V[2, 499] = 30, 29                 # the group {483, 499}
    V[3, 499], V[3, 483] = 30, 30
    for vg in (1, 2, 4, 8):
        _check(V, vg)
