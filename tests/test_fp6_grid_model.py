"""CPU: the FP6 integer grid of the match filter (DESIGN.md K1'') — the numpy model that
tests/test_gpu_match_fp6.py holds the GPU quantiser to, checked against the format's definition."""
import numpy as np

import fp6_grid_ref as fp6

# the grid as the design states it
G = sorted(set(range(0, 16)) | set(range(16, 31, 2)) | set(range(32, 61, 4)))


def test_grid_is_the_e2m3_value_set():
    vals = fp6.decode(np.arange(64))
    assert sorted(set(vals.tolist())) == sorted({-g for g in G} | set(G))
    assert fp6.GRID.tolist() == G and len(G) == 32
    # the magnitude index is the code's low 5 bits, monotone in the value
    assert np.array_equal(fp6.decode(np.arange(32)), fp6.GRID)
    assert np.array_equal(fp6.decode(np.arange(32) + 32), -fp6.GRID)


def test_round_trip():
    g = np.array([s * v for v in G for s in (1, -1)], np.int64)
    x = (g / 127.0).astype(np.float32)
    q, code = fp6.quantize(x)
    assert np.array_equal(q.astype(np.int64), g)
    assert np.array_equal(fp6.decode(code), g)
    # up to 15 the grid is the int8 quantiser's rint(127 x)
    xs = np.linspace(-15.4 / 127, 15.4 / 127, 2001).astype(np.float32)
    assert np.array_equal(fp6.quantize(xs)[0], np.rint(np.float32(127) * xs).astype(np.int8))
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 64, (3, 5, 256)).astype(np.uint8)
    by = fp6.pack(codes)
    assert by.shape == codes.shape and by.dtype == np.uint8
    back, zero_tail = fp6.unpack(by)
    assert zero_tail and np.array_equal(back, codes)
    # code e of a chunk sits at bits 6 e .. 6 e + 5
    one = np.zeros(32, np.uint8)
    one[5] = 0x2B
    v = int.from_bytes(fp6.pack(one)[:24].tobytes(), "little")
    assert v == 0x2B << 30


def exact_inputs(targets):
    """f32 x with 127 * x == target exactly in f32 (searched among the neighbours of target / 127)."""
    xs = []
    for t in targets:
        x0 = np.float32(t / 127.0)
        cand = [x0]
        for _ in range(4):
            cand += [np.nextafter(cand[-1], np.float32(np.inf)), np.nextafter(cand[0], np.float32(-np.inf))]
            cand.sort()
        hit = [c for c in cand if np.float32(127.0) * c == np.float32(t)]
        if hit:
            xs.append((t, hit[0]))
    return xs


def test_midpoints_go_to_the_even_code():
    mids = [(a + b) / 2.0 for a, b in zip(G[:-1], G[1:])]
    found = exact_inputs(mids + [-m for m in mids])
    assert len(found) >= len(mids)          # most midpoints are reachable exactly
    for t, x in found:
        g, code = fp6.quantize(np.array([x], np.float32))
        n = int(code[0]) & 31
        lo = max(i for i, v in enumerate(G) if v < abs(t))
        assert n in (lo, lo + 1) and n % 2 == 0, (t, n)
        assert int(g[0]) == int(np.sign(t)) * G[n]
    # just off a midpoint the nearer point wins
    g, _ = fp6.quantize(np.array([30.9 / 127, 31.1 / 127, 15.4 / 127, 15.6 / 127, 57.9 / 127, 58.1 / 127], np.float32))
    assert g.tolist() == [30, 32, 15, 16, 56, 60]


def test_clip_and_zero():
    x = np.array([60.0 / 127, 61.9 / 127, 0.6, 1.0, 3.0e38, -0.6, -3.0e38, 0.0, -0.0, 1e-42, -1e-42, 0.3 / 127,
                  -0.3 / 127], np.float32)
    g, code = fp6.quantize(x)
    assert g.tolist() == [60, 60, 60, 60, 60, -60, -60, 0, 0, 0, 0, 0, 0]
    assert code.tolist() == [31, 31, 31, 31, 31, 63, 63, 0, 0, 0, 0, 0, 0]


def test_partial_sums_stay_below_2_24():
    """Every partial sum of h_j + sum_k g_a g_b is an integer below 2^24: exact in f32 in any order."""
    d = 256
    gmax = int(fp6.GRID.max())
    assert gmax == fp6.CLIP
    dot_max = d * gmax * gmax                     # |sum g_a g_b| over any subset of k
    norm_max = d * gmax * gmax                    # |g_b|^2
    # keys = -norm * 128 + low (low in [0, 127]), h = keys >> 8: valid rows
    h_min = (-norm_max * 128) >> 8
    assert h_min == -460800
    h_pad = (-(1 << 31)) >> 8                     # padded rows: keys = INT_MIN + low
    assert h_pad == -(1 << 23)
    assert dot_max + max(abs(h_min), abs(h_pad)) < 1 << 24
    # and the loop's sentinel lies below every reachable value
    assert min(h_pad, h_min - dot_max) > -(1 << 24)
