"""GPU: the FP6 certified filter of the exact float mode (DESIGN.md K1''): the e2m3 integer-grid
quantiser against its numpy model bit for bit, the scaled-MFMA kernel's integer arithmetic against
the int8 kernel on data that lies on the grid (same graph, same rows sent to the f64 pass), and the
graph against oracle.match.bf_match_exact on off-grid, clipped and degenerate inputs."""
import importlib

import numpy as np
import pytest
import torch

import fp6_grid_ref as fp6
from oracle import match as om

pytestmark = pytest.mark.gpu

abi = importlib.import_module("3d_reconstruction_amd._abi")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")

M = 512
NK = np.array([257, 500], np.int32)
PAIRS = np.array([[0, 1]], np.int32)
# (query row, best j, second j) as in test_gpu_match_rangemax.py: candidate j = 128 block + 16 tile
# + 4 lane group + accumulator, a range = 4 tiles = 64 candidates
SAME_GROUP = [(0, 3, 19), (7, 340, 324), (14, 69, 70), (21, 398, 397), (256, 483, 499)]
ELSEWHERE = [(28, 130, 134), (35, 150, 146), (42, 200, 264), (49, 280, 216), (56, 40, 300), (63, 430, 45)]
PLANTS = SAME_GROUP + ELSEWHERE
# rows of magnitude 60 in every dimension (|dot| near 9e5): same group, another range, another block
BIG_SAME = [(70, 5, 21), (77, 410, 394)]
BIG = BIG_SAME + [(84, 140, 270), (91, 330, 60)]
assert len({j for _, a, b in PLANTS + BIG for j in (a, b)}) == 2 * len(PLANTS + BIG)
assert all(a // 64 == b // 64 and a % 16 // 4 == b % 16 // 4 for _, a, b in SAME_GROUP + BIG_SAME)
# squared grid distances of (best, second): unit steps on the small rows (|g| <= 14: step 1 of the grid)
_STEPS = {1: (1,), 2: (1, 1), 3: (1, 1, 1), 4: (2,), 9: (3,), 16: (4,), 17: (4, 1), 64: (8,)}
DIST = [(9, 16), (9, 17), (1, 2), (2, 3), (4, 64)]
# ... and grid steps of 4 on the magnitude-60 rows: 144 = 9 steps, 256 = 16, 272 = 17
BIG_DIST = [(144, 256), (144, 272)]

_cache = {}


def _grid_dataset(d, dist, big, parity):
    """g int [2, M, d] on the grid, x = g / 127 in f32, the reference graph."""
    key = (d, dist, big, parity)
    if key not in _cache:
        rng = np.random.default_rng(d + 7)
        g = rng.integers(-6, 7, (2, M, d)).astype(np.int64)
        for r, j1, j2 in PLANTS:
            if int(g[0, r].dot(g[0, r])) % 2 != parity:
                g[0, r, 5] += 1
            assert int(g[0, r].dot(g[0, r])) % 2 == parity
            for j, D in zip((j1, j2), dist):
                g[1, j] = g[0, r]
                for t, step in enumerate(_STEPS[D]):
                    g[1, j, 10 + t] += step
                assert int(((g[1, j] - g[0, r]) ** 2).sum()) == D
        for n, (r, j1, j2) in enumerate(BIG):
            g[0, r] = 60 * rng.choice([-1, 1], d)
            for j, D in zip((j1, j2), big):
                g[1, j] = g[0, r]
                k = rng.choice(d, D // 16, replace=False)
                g[1, j, k] -= 4 * np.sign(g[1, j, k])            # 60 -> 56: one grid step of 4
                assert int(((g[1, j] - g[0, r]) ** 2).sum()) == D
            assert abs(int(g[0, r].dot(g[1, j1]))) > 0.97 * d * 3600
        for i, n in enumerate(NK):
            g[i, n:] = 0
        assert np.isin(np.abs(g), fp6.GRID).all()
        x = (g / 127.0).astype(np.float32)
        ref = np.full((1, M), -1, np.int64)
        ref[0, :NK[0]] = om.bf_match_exact(x[0, :NK[0]], x[1, :NK[1]], (3, 4))
        _cache[key] = (g, x, ref)
    return _cache[key]


def _match(sfm, bank, pairs, dtype, gpu):
    out = torch.empty((len(pairs), bank.m_pad), dtype=dtype, device=gpu)
    m0 = bank.match(pairs, ratio=0.75, out=out).cpu().numpy().astype(np.int64)
    return m0, int(bank.last_resolved.item())


def _exact_inputs(targets):
    xs = []
    for t in targets:
        c = np.float32(t / 127.0)
        cand = [c]
        for _ in range(4):
            cand = [np.nextafter(cand[0], np.float32(-np.inf))] + cand + [np.nextafter(cand[-1], np.float32(np.inf))]
        xs += [v for v in cand if np.float32(127.0) * v == np.float32(t)][:1]
    return xs


def test_quantiser_matches_the_model(sfm, gpu):
    d, m_pad = 256, 128
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((2, m_pad, d)) * 0.12).astype(np.float32)
    mids = [(a + b) / 2.0 for a, b in zip(fp6.GRID[:-1], fp6.GRID[1:])]
    mid_x = _exact_inputs(mids + [-m for m in mids])
    assert len(mid_x) >= len(mids)                                # exact midpoints are in the input
    special = np.array(mid_x + [0.0, -0.0, 0.5, -0.5, 1.0, -7.5, 3e38, -3e38, 60.0 / 127, 62.0 / 127, 1e-42, -1e-42,
                                1e-39, -1e-39, 0.49 / 127, -0.51 / 127], np.float32)
    x[0, 0, :special.size] = special
    x[0, 1, -special.size:] = special[::-1]
    x[1, 5] = (rng.integers(-70, 71, d) / 127.0).astype(np.float32)
    nk = np.array([100, 7], np.int32)                             # rows past n_kpts are padding: zero
    xt = torch.from_numpy(x).to(gpu)
    g = torch.full((2, m_pad, d), 99, dtype=torch.int8, device=gpu)
    code = torch.full((2, m_pad, d), 0xAB, dtype=torch.uint8, device=gpu)
    nkt = torch.from_numpy(nk).to(gpu)
    abi.call("sfmhip_desc_quantize_fp6", abi.ptr(xt), 2, m_pad, d, abi.ptr(nkt), abi.ptr(g), abi.ptr(code),
             abi.stream_ptr())
    torch.cuda.synchronize()
    rg, rc = fp6.quantize(x)
    for i, n in enumerate(nk):
        rg[i, n:] = 0
        rc[i, n:] = 0
    assert np.array_equal(g.cpu().numpy(), rg)
    assert np.array_equal(code.cpu().numpy(), fp6.pack(rc))
    back, zero_tail = fp6.unpack(code.cpu().numpy())
    assert zero_tail and np.array_equal(fp6.decode(back), rg.astype(np.int64))


@pytest.mark.parametrize("d", [128, 256])
def test_grid_data_is_summed_exactly(sfm, gpu, knob, d):
    """On grid data g = q, so the FP6 and the int8 filter see the same integers: the same graph (the
    oracle's) and the same rows sent to the f64 pass show that the scaled MFMA sums them exactly."""
    sets = []
    for n, dist in enumerate(DIST):
        for parity in (0, 1):
            big = BIG_DIST[(n + parity) % 2]
            sets.append((dist, big, parity, *_grid_dataset(d, dist, big, parity)))
    # from the reference alone: the planted same-group rows hold both outcomes, matched rows name the best
    matched = unmatched = 0
    for dist, big, parity, g, x, ref in sets:
        for r, j1, _ in PLANTS + BIG:
            assert ref[0, r] in (j1, -1), (dist, big, parity, r)
        for r, j1, _ in BIG:
            if big == (144, 272):
                assert ref[0, r] == j1
        rows = [r for r, _, _ in SAME_GROUP + BIG_SAME]
        matched += int((ref[0, rows] >= 0).sum())
        unmatched += int((ref[0, rows] < 0).sum())
    print(f"same-group planted rows: {matched} matched, {unmatched} unmatched in the reference")
    assert matched >= 4 and unmatched >= 4
    for dist, big, parity, g, x, ref in sets:
        bank = sfm.DescriptorBank.from_float(torch.from_numpy(x), n_kpts=NK, mode=sfm.MODE_FLOAT, exact=True)
        assert bank.code is not None
        assert np.array_equal(bank.g.cpu().numpy().astype(np.int64), g)           # the data lies on the grid
        assert np.array_equal(bank.q.cpu().numpy().astype(np.int64), g)           # and g = q
        res = {}
        for fp6_on in (1, 0):
            knob("MATCH_FP6", fp6_on)
            for dtype in (torch.int16, torch.int32):
                m0, nres = _match(sfm, bank, PAIRS, dtype, gpu)
                bad = np.flatnonzero(m0[0] != ref[0])
                assert bad.size == 0, (fp6_on, dtype, dist, big, parity, bad[:8], m0[0, bad[:8]], ref[0, bad[:8]])
                res[(fp6_on, dtype)] = nres
        print(f"d {d} dist {dist} big {big} parity {parity}: rows resolved {res}")
        for dtype in (torch.int16, torch.int32):
            assert res[(1, dtype)] == res[(0, dtype)], (dist, big, parity, res)
        assert res[(1, torch.int32)] < NK[0] // 4                                 # the filter decided most rows


def _offgrid(gpu):
    if "off" not in _cache:
        x = syn.superpoint_like(3, 512, 256, seed=5).numpy().astype(np.float32)
        x = np.concatenate([x, np.zeros((2, 512, 256), np.float32)])
        rng = np.random.default_rng(11)
        # |127 x| well past 60: clipped, a large residual, resolved.  A bank's certificate adds the largest
        # residual of image b to every row's bound, so these rows sit in image 2 alone and the share of rows
        # the filter decides is measured on the pairs whose image b is 0 or 1 (image 2 as a: its clipped
        # rows are queries there)
        for r in (3, 17, 200, 300, 480):
            x[2, r] *= np.float32(rng.uniform(8.0, 14.0))
        assert (np.abs(127 * x[2, 3]) > 60).any()
        x[4, 0] = x[0, 9]
        nk = np.array([257, 500, 512, 0, 1], np.int32)
        for i, n in enumerate(nk):
            x[i, n:] = 0
        pairs = np.array([[0, 1], [1, 0], [2, 0], [2, 1], [1, 2], [0, 2], [0, 3], [3, 0], [4, 1], [1, 4], [3, 4]],
                         np.int32)
        ref = np.full((len(pairs), 512), -1, np.int64)
        for p, (a, b) in enumerate(pairs):
            if nk[a] and nk[b] >= 2:
                ref[p, :nk[a]] = om.bf_match_exact(x[a, :nk[a]], x[b, :nk[b]], (3, 4))
        _cache["off"] = (x, nk, pairs, ref)
    return _cache["off"]


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32])
def test_offgrid_clipped_and_degenerate_images(sfm, gpu, knob, dtype):
    x, nk, pairs, ref = _offgrid(gpu)
    bank = sfm.DescriptorBank.from_float(torch.from_numpy(x), n_kpts=nk, mode=sfm.MODE_FLOAT, exact=True)
    assert int(bank.g.abs().max()) == 60
    m0, _ = _match(sfm, bank, pairs, dtype, gpu)
    assert np.array_equal(m0, ref)
    full = pairs[:4]                                               # full images, image b without clipped rows
    valid = int(sum(nk[a] for a, _ in full))
    _, nres = _match(sfm, bank, full, dtype, gpu)
    knob("MATCH_FP6", 0)
    m8, nres8 = _match(sfm, bank, full, dtype, gpu)
    print(f"rows resolved of {valid}: fp6 {nres}, int8 on the grid values {nres8}")
    assert np.array_equal(m8, ref[:4])
    assert 0 < nres <= 0.10 * valid                                # the filter is under test, not the resolve


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32])
def test_every_row_through_the_resolve(sfm, gpu, knob, dtype):
    knob("MATCH_CERT", 0)
    x, nk, pairs, ref = _offgrid(gpu)
    bank = sfm.DescriptorBank.from_float(torch.from_numpy(x), n_kpts=nk, mode=sfm.MODE_FLOAT, exact=True)
    m0, nres = _match(sfm, bank, pairs, dtype, gpu)
    assert np.array_equal(m0, ref)
    assert nres == sum(int(nk[a]) for a, b in pairs if nk[b] >= 2)
    assert m0.min() >= -1 and m0.max() < 512                       # no transient mark is left in the graph
    g, xg, refg = _grid_dataset(256, DIST[0], BIG_DIST[0], 0)      # the widest distances: the magnitude-60 rows
    bank = sfm.DescriptorBank.from_float(torch.from_numpy(xg), n_kpts=NK, mode=sfm.MODE_FLOAT, exact=True)
    m0, nres = _match(sfm, bank, PAIRS, dtype, gpu)
    assert np.array_equal(m0, refg) and nres == NK[0]


def test_routing(sfm, gpu, knob):
    sdist = importlib.import_module("3d_reconstruction_amd.dist")
    x64 = syn.superpoint_like(2, 512, 64, seed=2)
    sift = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (2, 512, 128)).astype(np.float32))
    banks = [sfm.DescriptorBank.from_float(x64, n_kpts=NK, mode=sfm.MODE_FLOAT, exact=True),
             sfm.DescriptorBank.from_float(sift, n_kpts=NK, mode=sfm.MODE_SIFT, exact=True)]
    x128 = syn.superpoint_like(3, 384, 128, seed=8).to(gpu)
    b128 = sfm.DescriptorBank.from_float(x128, mode=sfm.MODE_FLOAT, exact=True)
    assert banks[0].code is None and banks[1].code is None and b128.code is not None
    on = [_match(sfm, b, PAIRS, torch.int16, gpu) for b in banks]
    pairs = sfm.all_pairs(3)
    g16 = sdist.match_all_pairs_sharded(b128, torch.from_numpy(pairs).to(gpu), exact=True)
    assert g16.dtype == torch.int16
    out = torch.empty((len(pairs), b128.m_pad), dtype=torch.int32, device=gpu)
    g32 = b128.match(pairs, out=out)
    assert torch.equal(g16.long(), g32.long())
    ref = np.stack([om.bf_match_exact(x128[a].cpu().numpy(), x128[b].cpu().numpy(), (3, 4)) for a, b in pairs])
    assert np.array_equal(g32.cpu().numpy()[:, :384].astype(np.int64), ref)
    knob("MATCH_FP6", 0)
    off = [_match(sfm, b, PAIRS, torch.int16, gpu) for b in banks]
    for (m_on, n_on), (m_off, n_off) in zip(on, off):
        assert np.array_equal(m_on, m_off) and n_on == n_off
    assert torch.equal(b128.match(pairs).long(), g32.long())
