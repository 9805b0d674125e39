"""GPU: the dense operand rows of the FP6 match filter (DESIGN.md K1'' "Layout"): the pack entry
against its numpy model bit for bit, and the kernel on a shape with several query blocks, a ragged
last query block and a ragged last candidate block, against the oracle and against the int8 filter
on the same grid values (same graph, same rows sent to the f64 pass)."""
import importlib

import numpy as np
import pytest
import torch

import fp6_dense_ref as dense
import fp6_grid_ref as fp6
from oracle import match as om

pytestmark = pytest.mark.gpu

abi = importlib.import_module("3d_reconstruction_amd._abi")

M = 1152                                     # 2 * 512 + 128: more than one query block of 512 rows, the last ragged
NK = np.array([1100, 700], np.int32)         # ragged last candidate block in both directions
PAIRS = np.array([[0, 1], [1, 0]], np.int32)
# squared grid distances (best, second) and the unit steps that make them (|g| <= 14: step 1 of the grid)
_STEPS = {1: (1,), 2: (1, 1), 3: (1, 1, 1), 4: (2,), 9: (3,), 16: (4,), 17: (4, 1), 64: (8,)}
DIST = [(9, 16), (9, 17), (1, 2), (2, 3), (4, 64)]
BIG_DIST = [(144, 256), (144, 272)]          # grid steps of 4 on rows of magnitude 60
BIG_EVERY = 7                                # every 7th planted query row is a magnitude-60 row

_cache = {}


def _plan(n_query, n_cand, taken_q, taken_c, rng):
    """One planted query row per 16-row tile of the query image (so every tile of every wave of every
    query block holds one), each with a best and a second candidate; the candidates walk through the
    eight 16-row tile positions of a 128-row block, the four lane groups and the four accumulators.
    Every third pair lies in one group (the same range of 64 candidates and the same lane group: the
    second is hidden behind the best's group maximum and comes back from the rescan)."""
    plan = []
    free = [int(j) for j in rng.permutation(n_cand) if int(j) not in taken_c]

    def take(ok):
        j = next(j for j in free if ok(j))
        free.remove(j)
        return j

    for t in range((n_query + 15) // 16):
        rows = [r for r in range(16 * t, min(16 * t + 16, n_query)) if r not in taken_q]
        r = rows[(5 * t) % len(rows)]
        j1 = take(lambda j: j % 128 // 16 == t % 8)
        if t % 3 == 0:
            j2 = take(lambda j: j // 64 == j1 // 64 and j % 16 // 4 == j1 % 16 // 4)
        else:
            j2 = take(lambda j: j % 128 // 16 == (t // 8 + t) % 8 and j // 64 != j1 // 64)
        plan.append((r, j1, j2))
    return plan


def _dataset(d):
    """g int [2, M, d] on the grid, x = g / 127 in f32, the reference graphs of both pairs."""
    if d not in _cache:
        rng = np.random.default_rng(d + 31)
        g = rng.integers(-6, 7, (2, M, d)).astype(np.int64)
        fwd = _plan(int(NK[0]), int(NK[1]), set(), set(), rng)                     # pair (0, 1)
        q0 = {r for r, _, _ in fwd}
        c1 = {j for _, a, b in fwd for j in (a, b)}
        bwd = _plan(int(NK[1]), int(NK[0]), c1, q0, rng)                           # pair (1, 0)
        assert len(fwd) == 69 and len(bwd) == 44
        n = 0
        for qi, plan in ((0, fwd), (1, bwd)):
            ci = 1 - qi
            for r, j1, j2 in plan:
                big = n % BIG_EVERY == 0
                if big:
                    g[qi, r] = 60 * rng.choice([-1, 1], d)
                elif int(g[qi, r].dot(g[qi, r])) % 2 != n % 2:                    # both parities of the norm
                    g[qi, r, 5] += 1
                dist = BIG_DIST[n % 2] if big else DIST[n % len(DIST)]
                for j, D in zip((j1, j2), dist):
                    g[ci, j] = g[qi, r]
                    if big:
                        k = rng.choice(d, D // 16, replace=False)                  # both k-steps, every slot
                        g[ci, j, k] -= 4 * np.sign(g[ci, j, k])                    # 60 -> 56: one grid step of 4
                    else:
                        for t, step in enumerate(_STEPS[D]):
                            k = (37 * n + 61 * t + (d // 2) * (n % 2)) % d         # odd n: the upper half of k
                            g[ci, j, k] += step
                    assert int(((g[ci, j] - g[qi, r]) ** 2).sum()) == D
                n += 1
        for i, nk in enumerate(NK):
            g[i, nk:] = 0
        assert np.isin(np.abs(g), fp6.GRID).all()
        # coverage, from the plan alone
        for plan, nq in ((fwd, int(NK[0])), (bwd, int(NK[1]))):
            assert {r // 16 for r, _, _ in plan} == set(range((nq + 15) // 16))
            assert {j % 128 // 16 for _, a, b in plan for j in (a, b)} == set(range(8))
            assert {j % 16 for _, a, b in plan for j in (a, b)} == set(range(16))   # lane group x accumulator
            assert sum(a // 64 == b // 64 and a % 16 // 4 == b % 16 // 4 for _, a, b in plan) >= len(plan) // 3
        x = (g / 127.0).astype(np.float32)
        ref = np.full((2, M), -1, np.int64)
        for p, (a, b) in enumerate(PAIRS):
            ref[p, :NK[a]] = om.bf_match_exact(x[a, :NK[a]], x[b, :NK[b]], (3, 4))
        for p, plan in enumerate((fwd, bwd)):
            assert all(ref[p, r] in (j1, -1) for r, j1, _ in plan)
            assert sum(ref[p, r] == j1 for r, j1, _ in plan) >= len(plan) // 4     # matched rows name the best
        _cache[d] = (g, x, ref)
    return _cache[d]


def _match(bank, dtype, gpu):
    out = torch.empty((len(PAIRS), bank.m_pad), dtype=dtype, device=gpu)
    m0 = bank.match(PAIRS, ratio=0.75, out=out).cpu().numpy().astype(np.int64)
    return m0, int(bank.last_resolved.item())


@pytest.mark.parametrize("d", [128, 256])
def test_pack_matches_the_model(sfm, gpu, d):
    m_pad = 128
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((2, m_pad, d)) * 0.15).astype(np.float32)
    x[1, 5] = (rng.integers(-70, 71, d) / 127.0).astype(np.float32)
    nk = np.array([100, 7], np.int32)                             # rows past n_kpts are padding: zero
    xt, nkt = torch.from_numpy(x).to(gpu), torch.from_numpy(nk).to(gpu)
    g = torch.empty((2, m_pad, d), dtype=torch.int8, device=gpu)
    code = torch.empty((2, m_pad, d), dtype=torch.uint8, device=gpu)
    rows = torch.full((2, m_pad, 3 * d // 4), 0xAB, dtype=torch.uint8, device=gpu)
    abi.call("sfmhip_desc_quantize_fp6", abi.ptr(xt), 2, m_pad, d, abi.ptr(nkt), abi.ptr(g), abi.ptr(code),
             abi.stream_ptr())
    abi.call("sfmhip_desc_pack_fp6", abi.ptr(code), 2, m_pad, d, abi.ptr(rows), abi.stream_ptr())
    torch.cuda.synchronize()
    _, rc = fp6.quantize(x)
    for i, n in enumerate(nk):
        rc[i, n:] = 0
    assert rc.max() > 40 and (rc & 31).max() == 31                # both signs, the largest magnitude
    want = dense.pack_dense(fp6.pack(rc))
    got = rows.cpu().numpy()
    assert np.array_equal(got, want)
    for i, n in enumerate(nk):
        assert not got[i, n:].any()
    back, zero_tail = fp6.unpack(dense.unpack_dense(got))
    assert zero_tail and np.array_equal(back, rc)
    # the bank builds the same rows
    bank = sfm.DescriptorBank.from_float(xt, n_kpts=nk, mode=sfm.MODE_FLOAT, exact=True)
    assert bank.code is not None and np.array_equal(bank.dense.cpu().numpy(), want)


@pytest.mark.parametrize("d", [256, 128])
def test_blocks_waves_and_ragged_ends(sfm, gpu, knob, d):
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
            assert bad.size == 0, (fp6_on, dtype, bad[:8], m0[tuple(bad[:8].T)], ref[tuple(bad[:8].T)])
            res[(fp6_on, dtype)] = nres
    print(f"d {d}: rows resolved {res}")
    for dtype in (torch.int16, torch.int32):
        assert res[(1, dtype)] == res[(0, dtype)], res
    assert res[(1, torch.int32)] < int(NK.sum()) // 4                             # the filter decided most rows
