"""Plain references for the BoW front end (vq, k-means centroid update, word
histogram) and the seeded scenes the tests run them on.  numpy only, no GPU.
TEST INFRASTRUCTURE ONLY.

`vq_ref` is the difference form in np.longdouble (64-bit mantissa where the
platform has one): on integer data every value is exact, on floats it is 11 bits
finer than the f64 kernels it judges.  `cluster_means_ref` sums every cluster's
rows in index order with an explicit f64 `s = s + row` (np.sum sums pairwise), the
order scipy's update_cluster_means and `kmeans_update_kernel` use, so the bits can
be demanded.  tests/test_bow_ref_cpu.py holds all three to scipy / numpy.
"""
from __future__ import annotations

import functools

import numpy as np

LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63


class NoLongDouble(RuntimeError):
    """Float data and no 64-bit-mantissa long double: the reference cannot judge f64."""


def _integral(a):
    return bool(np.all(a == np.rint(a))) and float(np.abs(a).max(initial=0.0)) < 2.0 ** 20


def vq_ref(obs, code):
    """(codes int32, sqrt(min) rounded to f64, smallest relative top-two gap (q2 - q1) / q2 over
    the rows).  Lowest index on ties.  One codeword: every gap is 1."""
    obs = np.asarray(obs, np.float64)
    code = np.asarray(code, np.float64)
    n, k = obs.shape[0], code.shape[0]
    if LONGDOUBLE_OK:
        wide = np.longdouble
    elif _integral(obs) and _integral(code):
        wide = np.int64                 # exact: |difference| < 2^21, d < 2^20 terms
    else:
        raise NoLongDouble("np.longdouble has fewer than 63 mantissa bits")
    o_w, c_w = obs.astype(wide), code.astype(wide)
    codes = np.empty(n, np.int32)
    dist = np.empty(n, np.float64)
    gap = 1.0
    for i in range(n):
        df = c_w - o_w[i]
        q = (df * df).sum(axis=1)
        j = int(np.argmin(q))           # first occurrence of the minimum
        codes[i] = j
        q1 = q[j]
        if float(q1) == q1:             # representable (always on integer data): f64 sqrt rounds once
            dist[i] = np.sqrt(np.float64(q1))
        else:
            dist[i] = np.float64(np.sqrt(q1))
        if k > 1:
            q2 = np.delete(q, j).min()
            gap = min(gap, float((q2 - q1) / q2) if q2 > 0 else 0.0)
    return codes, dist, gap


def cluster_means_ref(obs, codes, k):
    """(means (k, d) f64, counts (k,) int64): per cluster the f64 sum of its rows in index order,
    divided by the count; zero rows for empty clusters; codes outside [0, k) count for nothing."""
    obs = np.asarray(obs, np.float64)
    codes = np.asarray(codes)
    sums = np.zeros((k, obs.shape[1]), np.float64)
    counts = np.zeros(k, np.int64)
    for i in range(obs.shape[0]):
        c = int(codes[i])
        if 0 <= c < k:
            sums[c] = sums[c] + obs[i]
            counts[c] += 1
    for c in range(k):
        if counts[c]:
            sums[c] = sums[c] / np.float64(counts[c])
    return sums, counts


def histogram_ref(codes, offsets, k):
    """(n_img, k) int64: np.bincount of every image's in-range codes."""
    codes = np.asarray(codes).astype(np.int64)
    out = np.zeros((len(offsets) - 1, k), np.int64)
    for i in range(len(offsets) - 1):
        c = codes[offsets[i]:offsets[i + 1]]
        out[i] = np.bincount(c[(c >= 0) & (c < k)], minlength=k)
    return out


# ---------------------------------------------------------------------------
# vq scenes.  (n, k, d) per dispatch form of sfmhip_vq.
VQ_DIFF_SHAPES = [(1, 1, 129), (15, 31, 130), (16, 32, 170), (17, 33, 171), (100, 65, 200), (257, 100, 255),
                  (33, 64, 256)]
VQ_MFMA_FULL_SHAPES = [(300, 257, 128), (50, 300, 128)]
VQ_MFMA_EDGE_SHAPES = [(n, k, d) for d in (1, 3, 32, 33, 64, 65, 127) for n in (255, 256, 257) for k in (144, 145)]
VQ_F16S_SHAPES = [(1, 5, 128), (15, 33, 128), (16, 256, 128), (17, 255, 128)]
VQ_INT_SHAPES = VQ_DIFF_SHAPES + VQ_MFMA_FULL_SHAPES + VQ_MFMA_EDGE_SHAPES + VQ_F16S_SHAPES
VQ_FLOAT_SHAPES = [(300, 33, 129), (300, 65, 171), (300, 100, 256), (300, 257, 128), (300, 40, 33)]
VQ_FLOAT_HITS = 5


@functools.lru_cache(maxsize=None)
def vq_int_scene(n, k, d):
    """Integers in [-20, 20]; code[k-1] = code[1] when k > 3 (an exact tie between two indices) and
    the last observation equal to a codeword (code[1], so that tie is raced, when there is one)."""
    rng = np.random.default_rng(1000003 * n + 1009 * k + d)
    obs = rng.integers(-20, 21, (n, d)).astype(np.float64)
    code = rng.integers(-20, 21, (k, d)).astype(np.float64)
    if k > 3:
        code[k - 1] = code[1]
    obs[n - 1] = code[min(1, k - 1)]
    obs.setflags(write=False)
    code.setflags(write=False)
    return obs, code


VQ_TIE_ROW, VQ_TIE_INDICES = 5, (3, 19, 35, 67)


@functools.lru_cache(maxsize=None)
def vq_tie_scene():
    """d = 200, k = 70, n = 20: the codeword nearest to observation 5 (one unit away) sits at indices
    3, 19 (the same lane's second codeword), 35 (the next chunk) and 67 (the last, ragged chunk)."""
    obs, code = (a.copy() for a in vq_int_scene(20, 70, 200))
    w = obs[VQ_TIE_ROW].copy()
    w[17] += 1.0
    code[list(VQ_TIE_INDICES)] = w
    obs.setflags(write=False)
    code.setflags(write=False)
    return obs, code


@functools.lru_cache(maxsize=None)
def vq_float_scene(n, k, d):
    """Standard-normal observations drawn independently of a standard-normal code book (a real
    nearest-codeword race); VQ_FLOAT_HITS observations are set equal to codewords.  Returns
    (obs, code, hit rows, their codewords)."""
    rng = np.random.default_rng(7 + 31 * n + 1009 * k + 1000003 * d)
    obs = rng.standard_normal((n, d))
    code = rng.standard_normal((k, d))
    rows = np.array([0, 16, n // 2, n - 2, n - 1])
    words = np.array([k - 1, 0, k // 2, 17 % k, 1])
    obs[rows] = code[words]
    obs.setflags(write=False)
    code.setflags(write=False)
    return obs, code, rows, words


@functools.lru_cache(maxsize=None)
def vq_reference(kind, *shape):
    """vq_ref of a scene, computed once and shared."""
    obs, code = {"int": vq_int_scene, "float": vq_float_scene, "tie": vq_tie_scene}[kind](*shape)[:2]
    codes, dist, gap = vq_ref(obs, code)
    codes.setflags(write=False)
    dist.setflags(write=False)
    return codes, dist, gap


# ---------------------------------------------------------------------------
# k-means update scenes: name -> (n, d, k).  64-lane ballot, 2048-code chunk, the four 256-feature
# slots, more clusters than observations.
UPDATE_SCENES = {
    "one": (1, 1, 1),
    "ballot_minus": (63, 255, 3),
    "ballot_empty_cluster": (64, 256, 5),
    "ballot_plus_outside_codes": (65, 257, 5),
    "chunk_minus": (2047, 8, 4),
    "chunk": (2048, 8, 4),
    "chunk_plus_outside_codes": (2049, 513, 4),
    "two_chunks_second_only": (4097, 1024, 3),
    "more_clusters_than_rows": (10, 4, 40),
}


@functools.lru_cache(maxsize=None)
def update_scene(name):
    """(obs (n, d) standard normal, codes (n,) int32, k).  `*_empty_cluster` leaves cluster 3 without
    members, `*_outside_codes` carries codes -1 and k among the valid ones, `*_second_only` has every
    member of cluster 2 in [2048, 4096) and the one row of the third chunk in cluster 0."""
    n, d, k = UPDATE_SCENES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 7919 * n)
    obs = rng.standard_normal((n, d))
    codes = rng.integers(0, k, n).astype(np.int32)
    if name.endswith("empty_cluster"):
        codes[codes == 3] = 4
    if name.endswith("outside_codes"):
        codes[rng.choice(n, n // 8, replace=False)] = -1
        codes[rng.choice(n, n // 8, replace=False)] = k
        codes[0], codes[n - 1] = k, -1
    if name.endswith("second_only"):
        codes = rng.integers(0, 2, n).astype(np.int32)
        codes[2048 + rng.choice(2048, 700, replace=False)] = 2
        codes[[2048, 4095]] = 2
        codes[4096] = 0
    obs.setflags(write=False)
    codes.setflags(write=False)
    return obs, codes, k


@functools.lru_cache(maxsize=None)
def update_reference(name):
    obs, codes, k = update_scene(name)
    means, counts = cluster_means_ref(obs, codes, k)
    means.setflags(write=False)
    counts.setflags(write=False)
    return means, counts


# ---------------------------------------------------------------------------
# Histogram scene: images of 257, 0, 1, 3000, 255 and 256 codes in one call.
HIST_SIZES = (257, 0, 1, 3000, 255, 256)
HIST_KS = (1, 200, 257, 1000, 16384)


@functools.lru_cache(maxsize=None)
def histogram_scene(k):
    """(codes int32, offsets int64): codes uniform in [0, k) with -1, k and 2^31 - 1 planted in the
    images of 257, 3000 and 256 codes (first, middle and last positions among them)."""
    rng = np.random.default_rng(40009 + k)
    offsets = np.concatenate([[0], np.cumsum(HIST_SIZES)]).astype(np.int64)
    codes = rng.integers(0, k, int(offsets[-1])).astype(np.int32)
    for img in (0, 3, 5):
        a, b = int(offsets[img]), int(offsets[img + 1])
        codes[a], codes[(a + b) // 2], codes[b - 1] = -1, k, 2 ** 31 - 1
        codes[a + 1 + rng.choice(b - a - 2, 9, replace=False)] = np.tile([-1, k, 2 ** 31 - 1], 3)
    codes.setflags(write=False)
    offsets.setflags(write=False)
    return codes, offsets


# ---------------------------------------------------------------------------
# k-means host loop scene
@functools.lru_cache(maxsize=None)
def kmeans_scene():
    """(obs (600, 8), centres (6, 8)): six centres on a grid of spacing 4, 12 apart in three
    coordinates at the least, 100 observations each with integer noise in [-3, 3], shuffled."""
    rng = np.random.default_rng(606)
    centres = 4.0 * np.array([[0, 0, 0, 0, 0, 0, 0, 0], [3, 3, 0, 0, 3, 0, 0, 3], [0, 3, 3, 0, 0, 3, 3, 0],
                              [3, 0, 3, 3, 0, 0, 3, 3], [0, 0, 0, 3, 3, 3, 0, 3], [3, 3, 3, 3, 3, 3, 3, 0]], np.float64)
    obs = np.repeat(centres, 100, axis=0) + rng.integers(-3, 4, (600, 8))
    obs = obs[rng.permutation(600)]
    obs.setflags(write=False)
    centres.setflags(write=False)
    return obs, centres


def kmeans_guess():
    """Seven rows: the six centres moved by less than 0.4 per coordinate, and one row at 1e4 that
    attracts nothing and is dropped."""
    _, centres = kmeans_scene()
    rng = np.random.default_rng(607)
    near = centres + rng.uniform(-0.4, 0.4, centres.shape)
    return np.vstack([near[:3], np.full((1, 8), 1e4), near[3:]])
