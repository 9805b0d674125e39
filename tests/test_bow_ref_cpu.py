"""The references of tests/bow_ref.py held to scipy and numpy, on the scenes the GPU tests of
tests/test_gpu_bow_shapes.py use.  No GPU.

* vq_ref == scipy.cluster.vq.vq bit for bit (codes and distances) on every integer scene, where
  scipy is exact;
* on every float scene the smallest relative gap between the best two squared distances of any
  row is >= 1e-9, four orders above the f64 GEMM-form decision noise d 2^-52 (|x|^2 + |c|^2) / q
  ~ 1e-13: the condition under which the GPU test may demand equal codes of every row;
* cluster_means_ref == scipy's update_cluster_means bit for bit on in-range codes;
* histogram_ref == the np.add.at form of oracle/bow.py.
"""
import numpy as np
import pytest
from scipy.cluster.vq import _vq, vq

import bow_ref as br

FLOAT_GAP = 1e-9


@pytest.mark.parametrize("n,k,d", br.VQ_INT_SHAPES)
def test_vq_ref_equals_scipy_on_integer_scenes(n, k, d):
    obs, code = br.vq_int_scene(n, k, d)
    codes, dist, _ = br.vq_reference("int", n, k, d)
    sc, sd = vq(obs, code)
    assert np.array_equal(codes, sc) and np.array_equal(dist, sd)
    assert dist[n - 1] == 0.0 and codes[n - 1] == min(1, k - 1)     # the planted hit; lowest of the tied pair


def test_vq_ref_tie_scene():
    obs, code = br.vq_tie_scene()
    codes, dist, _ = br.vq_reference("tie")
    sc, sd = vq(obs, code)
    assert np.array_equal(codes, sc) and np.array_equal(dist, sd)
    assert codes[br.VQ_TIE_ROW] == br.VQ_TIE_INDICES[0] and dist[br.VQ_TIE_ROW] == 1.0
    q = ((code - obs[br.VQ_TIE_ROW]) ** 2).sum(1)
    assert sorted(np.nonzero(q == q.min())[0]) == list(br.VQ_TIE_INDICES)


@pytest.mark.skipif(not br.LONGDOUBLE_OK, reason="np.longdouble is no wider than f64 here")
@pytest.mark.parametrize("n,k,d", br.VQ_FLOAT_SHAPES)
def test_float_scenes_have_no_near_ties(n, k, d):
    obs, code, rows, words = br.vq_float_scene(n, k, d)
    codes, dist, gap = br.vq_reference("float", n, k, d)
    print(f"float scene {(n, k, d)}: smallest relative top-two gap {gap:.3e}")
    assert gap >= FLOAT_GAP
    assert np.array_equal(codes[rows], words) and np.all(dist[rows] == 0.0)
    assert np.count_nonzero(dist == 0.0) == br.VQ_FLOAT_HITS
    sc, sd = vq(obs, code)                                          # scipy: same codes, distances to BLAS rounding
    assert np.array_equal(codes, sc)
    np.testing.assert_allclose(sd, dist, rtol=1e-12, atol=1e-6)     # atol: its GEMM-form residue at the exact hits


def test_vq_ref_gap_and_lowest_index():
    code = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, 0.0], [0.0, 5.0]])
    codes, dist, gap = br.vq_ref(np.array([[1.0, 0.0]]), code[[0, 1, 3]])
    assert codes[0] == 0 and dist[0] == 1.0 and gap == 0.75         # q = 1, 4, 26
    codes, dist, gap = br.vq_ref(np.array([[1.0, 0.0], [3.0, 0.0]]), code)
    assert codes.tolist() == [0, 1] and gap == 0.0                  # codewords 0 and 2 tie on row 0
    assert br.vq_ref(np.array([[1.0, 2.0]]), code[:1])[2] == 1.0


@pytest.mark.parametrize("name", list(br.UPDATE_SCENES))
def test_cluster_means_ref_equals_scipy(name):
    obs, codes, k = br.update_scene(name)
    means, counts = br.update_reference(name)
    inside = (codes >= 0) & (codes < k)
    assert name.endswith("outside_codes") == (not inside.all())
    ref, has = _vq.update_cluster_means(np.ascontiguousarray(obs[inside]), codes[inside].astype(np.int32), k)
    assert np.array_equal(has, counts > 0)
    assert np.array_equal(means, ref)                               # zero rows for empty clusters on both sides
    assert np.array_equal(counts, np.bincount(codes[inside], minlength=k))
    if name.endswith("empty_cluster") or name == "more_clusters_than_rows":
        assert not has.all()
    if name.endswith("second_only"):
        members = np.nonzero(codes == 2)[0]
        assert members.min() == 2048 and members.max() == 4095 and len(members) > 600


def test_cluster_means_ref_is_sequential_not_pairwise():
    """The order is the point: on a long cluster the pairwise np.sum gives other bits."""
    obs, codes, k = br.update_scene("two_chunks_second_only")
    means, counts = br.update_reference("two_chunks_second_only")
    # numpy sums pairwise along a contiguous axis only: hence the transposed copy
    pairwise = np.stack([np.ascontiguousarray(obs[codes == c].T).sum(1) / counts[c] for c in range(k)])
    assert not np.array_equal(pairwise, means)
    np.testing.assert_allclose(pairwise, means, rtol=0, atol=1e-13)


@pytest.mark.parametrize("k", br.HIST_KS)
def test_histogram_ref_equals_add_at(k):
    codes, offsets = br.histogram_scene(k)
    assert np.diff(offsets).tolist() == list(br.HIST_SIZES)
    for bad in (-1, k, 2 ** 31 - 1):
        assert np.count_nonzero(codes == bad) >= 9
    ref = br.histogram_ref(codes, offsets, k)
    freq = np.zeros((len(offsets) - 1, k))
    for i in range(len(offsets) - 1):
        w = codes[offsets[i]:offsets[i + 1]]
        np.add.at(freq[i], w[(w >= 0) & (w < k)], 1.0)              # oracle/bow.py's form, in-range words
    assert np.array_equal(ref, freq)
    planted = ((codes < 0) | (codes >= k)).sum()
    assert ref.sum() == len(codes) - planted and ref[1].sum() == 0
