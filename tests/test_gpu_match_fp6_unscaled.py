"""GPU: match_fp6_kernel on the unscaled FP6 MFMA (DESIGN.md K1'', round 12).  The loop runs in units of
2^-6 (products g_a g_b / 64, chains from h / 64) and hands value_only_tail the integers it always saw, so
the graph must stay oracle.match.bf_match_exact's bit for bit and the filter must certify exactly the rows
the scaled form certified: `last_resolved` is held to the counts of the parent commit's build on the same
inputs (tests/golden/fp6_unscaled_parent_counts.json, written by tools/fp6_parent_counts.py from a
library built at the parent commit).

Shapes: 640 rows with n_kpts (640, 600, 513) — one full 512-row workgroup plus a partial one, five
candidate blocks (the ring parity and the owed payments cross an odd boundary), a partial last block, a last
block of one row, padded rows with h = -2^23 — and 128 rows, a single block (first-block payments and the
drain alone).  Data on the grid with rows of magnitude 60 on both sides (|dot| = d * 3600 at both signs:
the top of the exact range), and a random unit-norm bank."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import fp6_grid_ref as fp6
from conftest import GOLDEN
from oracle import match as om

pytestmark = pytest.mark.gpu

abi = importlib.import_module("3d_reconstruction_amd._abi")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")

PAIRS = np.array([[0, 1], [1, 2], [2, 0], [0, 2], [2, 1]], np.int32)
NKPTS = {640: (640, 600, 513), 128: (128, 100, 65)}
# the magnitude-60 family: image 0 row BIG_ROW = 60 s; in images 1 and 2 a copy FAR[img] grid steps of 4 away,
# one 9 steps away and the row -60 s, one of the copies in the last (partial) block where the image has one.
# Squared distances 16 * 9 against 16 * 16 tie in the ratio test (16 * 144 = 9 * 256: the filter cannot
# decide, the f64 pass settles the row), against 16 * 17 they pass it.
BIG_ROW = 70
FAR = {1: 16, 2: 17}
BIG_AT = {640: {1: (5, 530, 140), 2: (512, 21, 300)}, 128: {1: (5, 90, 40), 2: (64, 21, 33)}}
CASES = [(kind, m, d) for kind in ("grid", "unit") for m in (640, 128) for d in (128, 256)]
COUNTS_FILE = os.path.join(GOLDEN, "fp6_unscaled_parent_counts.json")

_cache = {}


def case_name(kind, m, d, dtype):
    return f"{kind}-m{m}-d{d}-{'int16' if dtype == torch.int16 else 'int32'}"


def case_inputs(kind, m, d):
    """-> (x f32 [3, m, d], n_kpts int32 [3], g int64 on the grid or None); no reference here, so that
    tools/fp6_parent_counts.py can build the same banks."""
    nk = np.array(NKPTS[m], np.int32)
    if kind == "unit":
        x = syn.superpoint_like(3, m, d, seed=12).numpy().astype(np.float32)
        g = None
    else:
        rng = np.random.default_rng(1000 * d + m)
        g = rng.integers(-6, 7, (3, m, d)).astype(np.int64)
        s = 60 * rng.choice([-1, 1], d)
        g[0, BIG_ROW] = s
        for img, (jfar, j9, jneg) in BIG_AT[m].items():
            for j, steps in ((jfar, FAR[img]), (j9, 9)):
                g[img, j] = s
                k = rng.choice(d, steps, replace=False)
                g[img, j, k] -= 4 * np.sign(s[k])                  # 60 -> 56: one grid step of 4
                assert int(g[img, j].dot(s)) > 0.97 * d * 3600
            g[img, jneg] = -s
            assert int(g[img, jneg].dot(s)) == -d * 3600
        assert np.isin(np.abs(g), fp6.GRID).all()
        x = (g / 127.0).astype(np.float32)
    for i, n in enumerate(nk):
        x[i, n:] = 0
        if g is not None:
            g[i, n:] = 0
    return x, nk, g


def _case(kind, m, d):
    key = (kind, m, d)
    if key not in _cache:
        x, nk, g = case_inputs(kind, m, d)
        ref = np.full((len(PAIRS), m), -1, np.int64)
        for p, (a, b) in enumerate(PAIRS):
            ref[p, :nk[a]] = om.bf_match_exact(x[a, :nk[a]], x[b, :nk[b]], (3, 4))
        for arr in (x, ref):
            arr.setflags(write=False)
        _cache[key] = (x, nk, g, ref)
    return _cache[key]


def _bank(sfm, x, nk):
    return sfm.DescriptorBank.from_float(torch.from_numpy(x.copy()), n_kpts=nk, mode=sfm.MODE_FLOAT, exact=True)


def _match(bank, dtype, gpu):
    out = torch.empty((len(PAIRS), bank.m_pad), dtype=dtype, device=gpu)
    m0 = bank.match(PAIRS, ratio=0.75, out=out).cpu().numpy().astype(np.int64)
    return m0, int(bank.last_resolved.item())


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32], ids=["int16", "int32"])
@pytest.mark.parametrize("kind,m,d", CASES)
def test_graph_is_the_oracles_and_the_filter_certifies_the_parents_rows(sfm, gpu, kind, m, d, dtype):
    x, nk, g, ref = _case(kind, m, d)
    bank = _bank(sfm, x, nk)
    assert bank.dense is not None and bank.m_pad == m
    if g is not None:
        assert np.array_equal(bank.g.cpu().numpy().astype(np.int64), g)      # the data lies on the grid
        assert int(bank.g.abs().max()) == 60
    m0, nres = _match(bank, dtype, gpu)
    bad = np.argwhere(m0 != ref)
    assert bad.size == 0, (bad[:8], m0[tuple(bad[:8].T)], ref[tuple(bad[:8].T)])
    with open(COUNTS_FILE) as f:
        parent = json.load(f)["counts"]
    valid = int(sum(nk[a] for a, _ in PAIRS))
    print(f"{case_name(kind, m, d, dtype)}: rows resolved {nres} of {valid}, parent build {parent[case_name(kind, m, d, dtype)]}")
    assert nres == parent[case_name(kind, m, d, dtype)]


@pytest.mark.parametrize("kind,m,d", CASES)
def test_every_row_through_the_resolve(sfm, gpu, knob, kind, m, d):
    knob("MATCH_CERT", 0)
    x, nk, g, ref = _case(kind, m, d)
    bank = _bank(sfm, x, nk)
    for dtype in (torch.int16, torch.int32):
        m0, nres = _match(bank, dtype, gpu)
        assert np.array_equal(m0, ref)
        assert nres == sum(int(nk[a]) for a, _ in PAIRS)


def _check_entries_without_key_values(sfm, gpu, kind, m, d):
    x, nk, g, ref = _case(kind, m, d)
    bank = _bank(sfm, x, nk)
    pr = torch.from_numpy(PAIRS).to(gpu)
    for dtype, entry in ((torch.int32, "sfmhip_match_pairs_exact_fp6"), (torch.int16, "sfmhip_match_pairs_exact_fp6_i16")):
        want = torch.empty((len(PAIRS), m), dtype=dtype, device=gpu)
        bank.match(PAIRS, ratio=0.75, out=want)                               # the _kv entry on the same bank
        want_res = int(bank.last_resolved.item())
        got = torch.full_like(want, 7)
        nres = torch.full((1,), 7, dtype=torch.int32, device=gpu)
        abi.call(entry, abi.ptr(bank.dense), abi.ptr(bank.g), abi.ptr(bank.gnorms), abi.ptr(bank.gkeys),
                 abi.ptr(bank.x), abi.ptr(bank.gerow), abi.ptr(bank.geimg), abi.ptr(bank.n_kpts), bank.n_img,
                 bank.m_pad, bank.d, abi.ptr(pr), len(PAIRS), 3, 4, abi.ptr(got), abi.ptr(nres), abi.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(got, want), entry
        assert np.array_equal(got.cpu().numpy().astype(np.int64), ref), entry
        assert int(nres.item()) == want_res, entry


@pytest.mark.parametrize("kind,m,d", CASES)
def test_entries_without_key_values_give_the_kv_graph(sfm, gpu, kind, m, d):
    """sfmhip_match_pairs_exact_fp6 / _fp6_i16 build h and hf in the call's own scratch: the same graph, row
    for row the oracle's, and the same resolved-row count as the _kv entries on the bank's key values."""
    _check_entries_without_key_values(sfm, gpu, kind, m, d)


@pytest.mark.parametrize("kind,m,d", CASES)
def test_entries_without_key_values_on_the_int8_kernel(sfm, gpu, knob, kind, m, d):
    """SFMHIP_MATCH_FP6=0: the int8 value-only kernel on g, h built per call and no hf."""
    knob("MATCH_FP6", 0)
    _check_entries_without_key_values(sfm, gpu, kind, m, d)


@pytest.mark.parametrize("m", [640, 128])
def test_key_values_entry(sfm, gpu, m):
    """sfmhip_match_key_values against key_values_kernel's definition: h = keys >> 8 bit for bit, and
    hf = h / 64 exactly; the bank holds the same arrays."""
    x, nk, g, _ = _case("grid", m, 256)
    bank = _bank(sfm, x, nk)
    h = torch.full_like(bank.gkeys, 7)
    hf = torch.full(bank.gkeys.shape, 7.0, dtype=torch.float32, device=gpu)
    abi.call("sfmhip_match_key_values", abi.ptr(bank.gkeys), bank.n_img, bank.m_pad, abi.ptr(h), abi.ptr(hf),
             abi.stream_ptr())
    torch.cuda.synchronize()
    want = bank.gkeys >> 8                                                    # arithmetic shift on int32
    assert h.dtype == torch.int32 and torch.equal(h, want)
    assert torch.equal(hf.double() * 64, want.double())                       # f64 holds both sides exactly
    assert int(want.min()) == -(1 << 23) and float(hf.min()) == -float(1 << 17)   # the padded rows
    assert torch.equal(bank.gh, h) and torch.equal(bank.ghf, hf)
