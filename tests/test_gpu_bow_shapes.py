"""GPU: sfmhip_vq (all three dispatch forms), sfmhip_kmeans_update, sfmhip_word_histogram and the
bow.kmeans host loop beyond the 200-word, d = 128 golden, against the plain references of
tests/bow_ref.py (held to scipy by tests/test_bow_ref_cpu.py) and scipy.cluster.vq.kmeans.

Integer data: codes, distances, means and bins bit for bit.  Float vq: equal codes on every row
(the scenes' smallest relative top-two gap is >= 1e-9, the f64 decision noise ~1e-13) and
distances within (d + 4) 2^-53: a sum of d non-negative fma terms carries at most (d + 2) u, the
square root halves that and adds u, so about (d / 2 + 2) u, taken twice.
"""
import importlib

import numpy as np
import pytest
import torch

import bow_ref as br

pytestmark = pytest.mark.gpu
bow = importlib.import_module("3d_reconstruction_amd.bow")

E_ARG = -1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _last_error(sfm):
    return sfm.lib.sfmhip_last_error().decode(errors="replace")


# ---------------------------------------------------------------------------
# vq
def _vq_bits(sfm, kind, *shape):
    obs, code = {"int": br.vq_int_scene, "tie": br.vq_tie_scene}[kind](*shape)
    rc, rd, _ = br.vq_reference(kind, *shape)
    codes, dist = sfm.vq(obs.copy(), code.copy())
    bad = np.nonzero((codes != rc) | (dist != rd))[0]
    print(f"vq {kind} {shape}: {len(bad)} of {len(rc)} rows differ", bad[:8].tolist(), codes[bad[:8]].tolist(),
          rc[bad[:8]].tolist())
    assert np.array_equal(codes, rc)
    assert np.array_equal(dist, rd)
    return codes, dist


@pytest.mark.parametrize("n,k,d", br.VQ_DIFF_SHAPES)
def test_vq_difference_form_integer_bits(sfm, gpu, n, k, d):
    """vq_kernel (128 < d <= 256): n around the 16-observation workgroup, k around the 32-codeword
    chunk and the 16-lane argmin, d on both sides of 64 KB of dynamic LDS (170 | 171) up to 256."""
    _vq_bits(sfm, "int", n, k, d)


def test_vq_difference_form_tie_across_lane_pair_and_chunks(sfm, gpu):
    """The nearest codeword of one row stands at indices 3, 19 (the lane's second codeword), 35 (the
    next chunk) and 67 (the ragged last chunk): the code is 3."""
    codes, dist = _vq_bits(sfm, "tie")
    assert codes[br.VQ_TIE_ROW] == br.VQ_TIE_INDICES[0] and dist[br.VQ_TIE_ROW] == 1.0


@pytest.mark.parametrize("n,k,d", br.VQ_MFMA_FULL_SHAPES)
def test_vq_mfma_full_width_multi_pass_integer_bits(sfm, gpu, n, k, d):
    """vq_mfma_kernel<128, true> over more than one code-book pass (d = 128, k > 256)."""
    _vq_bits(sfm, "int", n, k, d)


@pytest.mark.parametrize("n,k,d", br.VQ_MFMA_EDGE_SHAPES)
def test_vq_mfma_template_edges_integer_bits(sfm, gpu, n, k, d):
    """Every d at which the DP = 32 / 64 / 128 template changes or pads, n around the 256-observation
    tile, k at one full pass of 144 codewords and one more."""
    _vq_bits(sfm, "int", n, k, d)


@pytest.mark.parametrize("n,k,d", br.VQ_F16S_SHAPES)
def test_vq_f16_split_small_ends_integer_bits(sfm, gpu, n, k, d):
    """vq_f16s_kernel + vq_exact_kernel (d = 128, k <= 256) at one row, a ragged 16-row unit, an odd
    count of codeword blocks and the full 256."""
    _vq_bits(sfm, "int", n, k, d)


@pytest.mark.parametrize("n,k,d", br.VQ_FLOAT_SHAPES)
def test_vq_float_codes_equal_and_distances_to_rounding(sfm, gpu, n, k, d):
    if not br.LONGDOUBLE_OK:
        pytest.skip("np.longdouble is no wider than f64 here")
    obs, code, rows, words = br.vq_float_scene(n, k, d)
    rc, rd, gap = br.vq_reference("float", n, k, d)
    codes, dist = sfm.vq(obs.copy(), code.copy())
    rtol = (d + 4) * 2.0 ** -53
    live = rd > 0
    err = float(np.max(np.abs(dist[live] - rd[live]) / rd[live]))
    print(f"vq float {(n, k, d)}: gap {gap:.3e}, {np.count_nonzero(codes != rc)} codes differ, "
          f"max relative distance error {err:.3e} (bound {rtol:.3e}), hits {dist[rows].tolist()}")
    assert gap >= 1e-9
    assert np.array_equal(codes, rc)
    assert np.all(np.abs(dist - rd) <= rtol * rd)
    assert np.array_equal(codes[rows], words) and np.all(dist[rows] == 0.0)


def test_vq_rejects_wide_rows_and_empty_books(sfm, gpu):
    n = 4
    obs = torch.ones((n, 257), dtype=torch.float64, device=gpu)
    code = torch.ones((3, 257), dtype=torch.float64, device=gpu)
    codes = torch.full((n,), -77, dtype=torch.int32, device=gpu)
    dist = torch.full((n,), -77.0, dtype=torch.float64, device=gpu)
    rc = sfm.lib.sfmhip_vq(obs.data_ptr(), n, code.data_ptr(), 3, 257, codes.data_ptr(), dist.data_ptr(), _stream())
    assert rc == E_ARG and "d <= 256" in _last_error(sfm)
    rc = sfm.lib.sfmhip_vq(obs.data_ptr(), n, code.data_ptr(), 0, 256, codes.data_ptr(), dist.data_ptr(), _stream())
    assert rc == E_ARG and "sfmhip_vq" in _last_error(sfm)
    torch.cuda.synchronize()
    assert bool((codes == -77).all()) and bool((dist == -77.0).all())      # nothing was launched


# ---------------------------------------------------------------------------
# k-means centroid update
CANARY = -1234.5


def _update(sfm, gpu, obs, codes, k, d):
    n = 0 if obs is None else obs.shape[0]
    o = None if obs is None else torch.from_numpy(np.array(obs)).to(gpu)
    c = None if codes is None else torch.from_numpy(np.array(codes)).to(gpu)
    book = torch.full((k, d), CANARY, dtype=torch.float64, device=gpu)
    counts = torch.full((k,), -9, dtype=torch.int32, device=gpu)
    rc = sfm.lib.sfmhip_kmeans_update(None if o is None else o.data_ptr(), n, d, None if c is None else c.data_ptr(),
                                      k, book.data_ptr(), counts.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, book.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("name", list(br.UPDATE_SCENES))
def test_kmeans_update_bits_counts_and_untouched_rows(sfm, gpu, name):
    """The 64-lane ballot (63 | 64 | 65 rows), the 2048-code chunk (2047 | 2048 | 2049, two chunks and
    one row), each of the four 256-feature accumulator slots (d = 255 .. 1024), k > n, codes outside
    [0, k), a cluster whose members all sit in the second chunk."""
    obs, codes, k = br.update_scene(name)
    means, ref_counts = br.update_reference(name)
    rc, book, counts = _update(sfm, gpu, obs, codes, k, obs.shape[1])
    assert rc == 0, _last_error(sfm)
    has = ref_counts > 0
    print(f"kmeans_update {name} {br.UPDATE_SCENES[name]}: counts {ref_counts.tolist()[:8]}, "
          f"{np.count_nonzero(book[has] != means[has])} entries differ")
    assert np.array_equal(counts, ref_counts)
    assert np.array_equal(book[has], means[has])
    assert np.all(book[~has] == CANARY)


def test_kmeans_update_no_observations(sfm, gpu):
    """n = 0 (an empty tensor's pointer is null): every count 0, the book as it was."""
    rc, book, counts = _update(sfm, gpu, None, None, 5, 300)
    assert rc == 0, _last_error(sfm)
    assert np.all(counts == 0) and np.all(book == CANARY)


def test_kmeans_update_rejects_wide_rows(sfm, gpu):
    rc, book, counts = _update(sfm, gpu, np.ones((3, 1025)), np.zeros(3, np.int32), 2, 1025)
    assert rc == E_ARG and "d <= 1024" in _last_error(sfm)
    assert np.all(book == CANARY) and np.all(counts == -9)


# ---------------------------------------------------------------------------
# word histogram
TAIL = 64


def _histogram(sfm, gpu, codes, offsets, k, cells):
    c = torch.from_numpy(np.array(codes)).to(gpu)
    off = torch.from_numpy(np.array(offsets)).to(gpu)
    hist = torch.full((cells + TAIL,), -7777, dtype=torch.int32, device=gpu)
    rc = sfm.lib.sfmhip_word_histogram(c.data_ptr(), off.data_ptr(), len(offsets) - 1, k, hist.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, hist.cpu().numpy()


@pytest.mark.parametrize("k", br.HIST_KS)
def test_word_histogram_exact(sfm, gpu, k):
    """Images of 257, 0, 1, 3000, 255 and 256 codes in one call; one bin, the k > 256 bin loop and the
    k = 16384 limit (64 KB of LDS); codes -1, k and 2^31 - 1 count for nothing; the words after the
    last row stay."""
    codes, offsets = br.histogram_scene(k)
    ref = br.histogram_ref(codes, offsets, k)
    rc, hist = _histogram(sfm, gpu, codes, offsets, k, ref.size)
    assert rc == 0, _last_error(sfm)
    got = hist[:ref.size].reshape(ref.shape)
    print(f"histogram k = {k}: {np.count_nonzero(got != ref)} bins differ, row sums {got.sum(1).tolist()}")
    assert np.array_equal(got, ref)
    assert np.all(hist[ref.size:] == -7777)
    freq = bow.frequency_vectors(torch.from_numpy(np.array(codes)).to(gpu), offsets.copy(), k)
    assert freq.dtype == np.float64 and np.array_equal(freq, ref)


def test_word_histogram_rejects_more_bins_than_lds(sfm, gpu):
    codes, offsets = br.histogram_scene(200)
    rc, hist = _histogram(sfm, gpu, codes, offsets, 16385, 6 * 16385)
    assert rc == E_ARG and "sfmhip_word_histogram" in _last_error(sfm)
    assert np.all(hist == -7777)


# ---------------------------------------------------------------------------
# bow.kmeans host loop vs scipy.cluster.vq.kmeans
def _same_book(got, ref):
    book, dist = got
    rbook, rdist = ref
    print(f"kmeans: book {book.shape} vs scipy {rbook.shape}, distortion {dist!r} vs {rdist!r}")
    assert book.shape == rbook.shape
    np.testing.assert_allclose(book, rbook, rtol=1e-12, atol=1e-12)
    assert abs(dist - rdist) <= 1e-12 * abs(rdist)


def test_kmeans_explicit_guess_drops_the_empty_cluster(sfm, gpu):
    from scipy.cluster.vq import kmeans
    obs = br.kmeans_scene()[0].copy()
    guess = br.kmeans_guess()
    ref = kmeans(obs, guess)
    assert guess.shape == (7, 8) and ref[0].shape == (6, 8)
    _same_book(bow.kmeans(obs, guess), ref)


def test_kmeans_int_k_best_of_three_seeded(sfm, gpu):
    """k as an int, the best of three seeded runs.  scipy is seeded through np.random.seed, as
    oracle/bow.codebook (and the reference) seed it: from 1.15 on its `rng=` turns a RandomState into a
    Generator over the same bits, whose choice() draws other rows than RandomState.choice(), the
    stream bow.kmeans keeps.  Both spellings of that stream must give scipy's book."""
    from scipy.cluster.vq import kmeans
    obs = br.kmeans_scene()[0].copy()
    state = np.random.get_state()
    try:
        np.random.seed(5)
        ref = kmeans(obs, 6, iter=3)
        np.random.seed(5)
        got = bow.kmeans(obs, 6, iter=3)
    finally:
        np.random.set_state(state)
    _same_book(got, ref)
    _same_book(bow.kmeans(obs, 6, iter=3, rng=np.random.RandomState(5)), ref)


def test_kmeans_one_dimensional_observations(sfm, gpu):
    from scipy.cluster.vq import kmeans
    obs = br.kmeans_scene()[0].copy()
    x = np.ascontiguousarray(obs[:, 0] + 0.125 * obs[:, 1])
    guess = np.array([1.1, 6.3, 12.6])          # no midpoint on the data's 1/8 grid
    ref = kmeans(x, guess)
    assert ref[0].shape == (3,)
    _same_book(bow.kmeans(x, guess), ref)


@pytest.mark.parametrize("kwargs", [dict(k_or_guess=3, iter=0), dict(k_or_guess=0), dict(k_or_guess=2.5),
                                    dict(k_or_guess=3, nan=True)], ids=["iter0", "k0", "k2.5", "nan"])
def test_kmeans_argument_errors(sfm, gpu, kwargs):
    from scipy.cluster.vq import kmeans
    obs = br.kmeans_scene()[0].copy()
    if kwargs.pop("nan", False):
        obs[17, 3] = np.nan
    with pytest.raises(ValueError):
        kmeans(obs, check_finite=True, **kwargs)
    with pytest.raises(ValueError):
        bow.kmeans(obs, check_finite=True, **kwargs)
