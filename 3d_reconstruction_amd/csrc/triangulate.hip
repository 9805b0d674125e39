// triangulate.hip — S2b: robust N-view triangulation of tracks (semantics: include/sfmhip.h S2b,
// restated in numpy by tests/tri_ref.py).  f64, one IEEE operation per step in the order written
// (-ffp-contract=off), no floating-point atomics, every sum in the order of the sorted observation
// list: two runs give the same bytes and the result does not depend on the launch geometry.
//   init     one lane per track / observation: the outputs' failure values (status 1, NaN, 0) and the
//            track's hypothesis count min(L (L - 1) / 2, max_hyp) into hyp_off[t + 1]; the first C
//            lanes also write the camera centres.
//   scan     one workgroup: in-place inclusive scan of the counts (an integer sum), hyp_off[N] = H.
//            The host reads H (the one read-back of the call, before the two phases) to size the
//            records; nothing returns to the host between the phases.
//   score    the hypotheses of all tracks flattened, one lane per hypothesis: a binary search in
//            hyp_off finds the track, an integer walk maps the pair index to (a, b); the lane solves
//            the two-view point in closed form, scores it against the track's L observations and
//            writes one record (inlier count, cost).  A wave's lanes sit in the same or in
//            neighbouring tracks, so a short track costs no idle wave.
//   fit      one lane per track, tracks in the caller's order (descending length: the lanes of a
//            wave run similar trip counts): scans the track's records in h order for the winner (no
//            atomics, no ties by arrival), re-scores it for the set, then fit, classify, fit and the
//            final tests.  The inlier set lives in the `inlier` output, so a lane's state does not
//            grow with the track.
#include "common.h"
#include "geom_dev.h"

#include <algorithm>
#include <cmath>

namespace sfmhip {
namespace {

constexpr int kWg = 256;
constexpr int kScanWg = 1024;
constexpr int kMaxLen = 1 << 20;   // observations per track; max_hyp has the same bound: h n_pairs < 2^60

struct TriArgs {
    const double* poses;      // [C][3][4]
    const double* cam;        // [C][4] fx fy cx cy
    const double* centres;    // [C][3] (workspace)
    const int64_t* pt_off;    // [N + 1]
    const int32_t* obs_cam;   // [M]
    const double* pts2d;      // [M][2]
    int64_t N, M;
    int C, max_hyp, refine_iters;
    double thr2, c2;          // reproj_px^2, cos_min^2
};

__device__ __forceinline__ bool finite3(const double* X) {
    return fabs(X[0]) < (double)INFINITY && fabs(X[1]) < (double)INFINITY && fabs(X[2]) < (double)INFINITY;
}

// the track's segment; malformed (outside [0, M], reversed, longer than kMaxLen): empty
__device__ __forceinline__ int track_len(const TriArgs& w, int64_t t, int64_t& o0) {
    const int64_t a0 = w.pt_off[t], a1 = w.pt_off[t + 1];
    o0 = 0;
    if (a0 < 0 || a1 < a0 || a1 > w.M || a1 - a0 > (int64_t)kMaxLen) return 0;
    o0 = a0;
    return (int)(a1 - a0);
}

__device__ __forceinline__ int64_t hyp_count(int L, int max_hyp) {
    if (L < 2) return 0;
    const int64_t np = (int64_t)L * (L - 1) / 2;
    return np <= (int64_t)max_hyp ? np : (int64_t)max_hyp;
}

// hypothesis h -> positions (a, b), a < b, of the lexicographic pair list
__device__ __forceinline__ void hyp_pair(int64_t h, int L, int max_hyp, int& a, int& b) {
    const int64_t np = (int64_t)L * (L - 1) / 2;
    int64_t rem = np <= (int64_t)max_hyp ? h : h * np / (int64_t)max_hyp;
    int i = 0;
    while (i < L - 2 && rem >= (int64_t)(L - 1 - i)) {   // rem < n_pairs: the bound on i never binds
        rem -= (int64_t)(L - 1 - i);
        ++i;
    }
    a = i;
    b = i + 1 + (int)rem;
}

// camera-frame depth z and squared pixel error e2 of X against the observation (u, v) of camera c
__device__ __forceinline__ void reproj(const TriArgs& w, int c, const double* X, double u, double v, double& z,
                                       double& e2) {
    const double* P = w.poses + (size_t)c * 12;
    const double* k = w.cam + (size_t)c * 4;
    const double xc = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
    const double yc = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
    z = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
    const double iz = 1.0 / z;
    const double du = ((xc * iz) * k[0] + k[2]) - u;
    const double dv = ((yc * iz) * k[1] + k[3]) - v;
    e2 = du * du + dv * dv;
}

// Step 3 under X.  The list is sorted by (track, camera), so a camera's observations are one run:
// the run's inlier with the smallest e2 stays (the first of equals).  cnt / cost: the kept inliers
// and the sum of their e2 in run order; hit: how many of the positions a, b were kept.
template <bool WRITE>
__device__ inline void classify(const TriArgs& w, int64_t o0, int L, const double* X, int a, int b, uint8_t* inl,
                                int& cnt, double& cost, int& hit) {
    cnt = 0;
    cost = 0.0;
    hit = 0;
    int run_cam = -1, best_k = -1;
    double best_e2 = 0.0;
    for (int k = 0; k <= L; ++k) {
        int c = -1;
        if (k < L) {
            c = w.obs_cam[o0 + k];
            if (WRITE) inl[o0 + k] = 0;
            if (c < 0 || c >= w.C) continue;   // not an observation
        }
        if (c != run_cam) {
            if (best_k >= 0) {
                ++cnt;
                cost += best_e2;
                hit += (best_k == a) + (best_k == b);
                if (WRITE) inl[o0 + best_k] = 1;
            }
            run_cam = c;
            best_k = -1;
        }
        if (k == L) break;
        double z, e2;
        reproj(w, c, X, w.pts2d[2 * (o0 + k)], w.pts2d[2 * (o0 + k) + 1], z, e2);
        if (z > 0.0 && e2 <= w.thr2 && (best_k < 0 || e2 < best_e2)) {   // a NaN fails both
            best_k = k;
            best_e2 = e2;
        }
    }
}

// is the angle at X between the rays to the centres of cameras ca and cb too small (cos > cos_min)?
__device__ __forceinline__ bool angle_small(const TriArgs& w, int ca, int cb, const double* X) {
    const double* A = w.centres + (size_t)ca * 3;
    const double* B = w.centres + (size_t)cb * 3;
    const double ra0 = A[0] - X[0], ra1 = A[1] - X[1], ra2 = A[2] - X[2];
    const double rb0 = B[0] - X[0], rb1 = B[1] - X[1], rb2 = B[2] - X[2];
    const double d = (ra0 * rb0 + ra1 * rb1) + ra2 * rb2;
    const double n = ((ra0 * ra0 + ra1 * ra1) + ra2 * ra2) * ((rb0 * rb0 + rb1 * rb1) + rb2 * rb2);
    return d > 0.0 && d * d > w.c2 * n;
}

// Step 2: the midpoint of the common perpendicular of the two viewing rays (closed form).
__device__ inline bool hyp_point(const TriArgs& w, int64_t o0, int a, int b, double* X) {
    const int ca = w.obs_cam[o0 + a], cb = w.obs_cam[o0 + b];
    if (ca < 0 || ca >= w.C || cb < 0 || cb >= w.C || ca == cb) return false;
    const double* Pa = w.poses + (size_t)ca * 12;
    const double* Pb = w.poses + (size_t)cb * 12;
    const double* ka = w.cam + (size_t)ca * 4;
    const double* kb = w.cam + (size_t)cb * 4;
    const double xa = (w.pts2d[2 * (o0 + a)] - ka[2]) / ka[0], ya = (w.pts2d[2 * (o0 + a) + 1] - ka[3]) / ka[1];
    const double xb = (w.pts2d[2 * (o0 + b)] - kb[2]) / kb[0], yb = (w.pts2d[2 * (o0 + b) + 1] - kb[3]) / kb[1];
    double da[3], db[3], wv[3];
    const double* A = w.centres + (size_t)ca * 3;
    const double* B = w.centres + (size_t)cb * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        da[i] = (Pa[i] * xa + Pa[4 + i] * ya) + Pa[8 + i];   // R^T (x, y, 1)
        db[i] = (Pb[i] * xb + Pb[4 + i] * yb) + Pb[8 + i];
        wv[i] = A[i] - B[i];
    }
    const double aa = (da[0] * da[0] + da[1] * da[1]) + da[2] * da[2];
    const double bb = (da[0] * db[0] + da[1] * db[1]) + da[2] * db[2];
    const double cc = (db[0] * db[0] + db[1] * db[1]) + db[2] * db[2];
    const double dd = (da[0] * wv[0] + da[1] * wv[1]) + da[2] * wv[2];
    const double ee = (db[0] * wv[0] + db[1] * wv[1]) + db[2] * wv[2];
    const double den = aa * cc - bb * bb;
    const double s = (bb * ee - cc * dd) / den;
    const double t = (aa * ee - bb * dd) / den;
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = 0.5 * ((A[i] + s * da[i]) + (B[i] + t * db[i]));
    if (!finite3(X)) return false;
    return !angle_small(w, ca, cb, X);
}

// Step 5's fit to the set flagged in inl: N-view DLT start, then refine_iters Gauss-Newton steps.
__device__ inline void fit_point(const TriArgs& w, int64_t o0, int L, const uint8_t* inl, double* X) {
    double m[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) m[i][j] = 0.0;
    for (int k = 0; k < L; ++k) {
        if (!inl[o0 + k]) continue;
        const int c = w.obs_cam[o0 + k];
        if (c < 0 || c >= w.C) continue;   // flags are this lane's own; never read out of bounds
        const double* P = w.poses + (size_t)c * 12;
        const double* kk = w.cam + (size_t)c * 4;
        const double x = (w.pts2d[2 * (o0 + k)] - kk[2]) / kk[0], y = (w.pts2d[2 * (o0 + k) + 1] - kk[3]) / kk[1];
        double r1[4], r2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r1[j] = x * P[8 + j] - P[j];
            r2[j] = y * P[8 + j] - P[4 + j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j) m[i][j] += r1[i] * r1[j] + r2[i] * r2[j];
    }
#pragma unroll
    for (int i = 1; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) m[i][j] = m[j][i];
    double y4[4];
    null_vector_jacobi4(m, y4);
    X[0] = y4[0] / y4[3];
    X[1] = y4[1] / y4[3];
    X[2] = y4[2] / y4[3];
    for (int it = 0; it < w.refine_iters; ++it) {
        double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, g0 = 0, g1 = 0, g2 = 0;
        for (int k = 0; k < L; ++k) {
            if (!inl[o0 + k]) continue;
            const int c = w.obs_cam[o0 + k];
            if (c < 0 || c >= w.C) continue;
            const double* P = w.poses + (size_t)c * 12;
            const double* kk = w.cam + (size_t)c * 4;
            const double xc = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
            const double yc = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
            const double z = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
            const double iz = 1.0 / z;
            const double px = xc * iz, py = yc * iz;
            const double ru = (px * kk[0] + kk[2]) - w.pts2d[2 * (o0 + k)];
            const double rv = (py * kk[1] + kk[3]) - w.pts2d[2 * (o0 + k) + 1];
            const double su = kk[0] * iz, sv = kk[1] * iz;
            const double ju0 = su * (P[0] - px * P[8]), ju1 = su * (P[1] - px * P[9]), ju2 = su * (P[2] - px * P[10]);
            const double jv0 = sv * (P[4] - py * P[8]), jv1 = sv * (P[5] - py * P[9]), jv2 = sv * (P[6] - py * P[10]);
            a00 += ju0 * ju0 + jv0 * jv0;
            a01 += ju0 * ju1 + jv0 * jv1;
            a02 += ju0 * ju2 + jv0 * jv2;
            a11 += ju1 * ju1 + jv1 * jv1;
            a12 += ju1 * ju2 + jv1 * jv2;
            a22 += ju2 * ju2 + jv2 * jv2;
            g0 += ju0 * ru + jv0 * rv;
            g1 += ju1 * ru + jv1 * rv;
            g2 += ju2 * ru + jv2 * rv;
        }
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = (a00 * c00 + a01 * c01) + a02 * c02;
        X[0] -= ((c00 * g0 + c01 * g1) + c02 * g2) / det;
        X[1] -= ((c01 * g0 + c11 * g1) + c12 * g2) / det;
        X[2] -= ((c02 * g0 + c12 * g1) + c22 * g2) / det;
    }
}

__global__ __launch_bounds__(kWg) void tri_init_kernel(TriArgs w, double* __restrict__ centres,
                                                       int64_t* __restrict__ hyp_off, double* __restrict__ X,
                                                       int32_t* __restrict__ status, int32_t* __restrict__ n_inl,
                                                       uint8_t* __restrict__ inl, double* __restrict__ residual) {
    const int64_t i = (int64_t)blockIdx.x * kWg + threadIdx.x;
    if (i < w.C) {
        const double* P = w.poses + (size_t)i * 12;
#pragma unroll
        for (int q = 0; q < 3; ++q) centres[i * 3 + q] = -((P[q] * P[3] + P[4 + q] * P[7]) + P[8 + q] * P[11]);
    }
    if (i < w.N) {
        int64_t o0;
        const int L = track_len(w, i, o0);
        hyp_off[i + 1] = hyp_count(L, w.max_hyp);
        X[3 * i] = X[3 * i + 1] = X[3 * i + 2] = (double)NAN;
        status[i] = 1;
        n_inl[i] = 0;
    }
    if (i < w.M) {
        inl[i] = 0;
        residual[i] = (double)NAN;
    }
}

__global__ __launch_bounds__(kScanWg) void tri_scan_kernel(int64_t* __restrict__ off, int64_t N) {
    __shared__ int64_t s[kScanWg];
    const int t = threadIdx.x;
    const int64_t per = (N + kScanWg - 1) / kScanWg;
    const int64_t i0 = min(N, (int64_t)t * per), i1 = min(N, i0 + per);
    int64_t sum = 0;
    for (int64_t i = i0; i < i1; ++i) sum += off[1 + i];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanWg; d <<= 1) {
        const int64_t v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int64_t run = s[t] - sum;
    for (int64_t i = i0; i < i1; ++i) {
        run += off[1 + i];
        off[1 + i] = run;
    }
    if (t == 0) off[0] = 0;
}

__global__ __launch_bounds__(kWg) void tri_score_kernel(TriArgs w, const int64_t* __restrict__ hyp_off, int64_t H,
                                                        int32_t* __restrict__ rec_cnt, double* __restrict__ rec_cost) {
    const int64_t g = (int64_t)blockIdx.x * kWg + threadIdx.x;
    if (g >= H) return;
    int64_t lo = 0, hi = w.N - 1;   // the track with hyp_off[t] <= g < hyp_off[t + 1]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (hyp_off[mid + 1] > g) hi = mid; else lo = mid + 1;
    }
    int64_t o0;
    const int L = track_len(w, lo, o0);
    int cnt = 0, hit = 0;
    double cost = 0.0;
    if (L >= 2) {   // holds for every g < H; a guard, not a case
        int a, b;
        hyp_pair(g - hyp_off[lo], L, w.max_hyp, a, b);
        double X[3];
        if (b < L && hyp_point(w, o0, a, b, X)) classify<false>(w, o0, L, X, a, b, nullptr, cnt, cost, hit);
    }
    rec_cnt[g] = hit == 2 ? cnt : 0;   // a or b not an inlier of its own model: dropped
    rec_cost[g] = cost;
}

__global__ __launch_bounds__(kWg) void tri_fit_kernel(TriArgs w, const int64_t* __restrict__ hyp_off,
                                                      const int32_t* __restrict__ rec_cnt,
                                                      const double* __restrict__ rec_cost,
                                                      const int32_t* __restrict__ order, double* __restrict__ Xout,
                                                      int32_t* __restrict__ status, int32_t* __restrict__ n_inl,
                                                      uint8_t* __restrict__ inl, double* __restrict__ residual) {
    const int64_t i = (int64_t)blockIdx.x * kWg + threadIdx.x;
    if (i >= w.N) return;
    const int64_t t = order ? (int64_t)order[i] : i;
    if (t < 0 || t >= w.N) return;
    int64_t o0;
    const int L = track_len(w, t, o0);
    int n_cam = 0, prev = -1;
    for (int k = 0; k < L; ++k) {
        const int c = w.obs_cam[o0 + k];
        if (c < 0 || c >= w.C) continue;
        if (c != prev) ++n_cam;
        prev = c;
    }
    if (n_cam < 2) return;   // status 1, as initialised
    int st = 0, cnt = 0, hit = 0;
    double cost = 0.0, X[3] = {0.0, 0.0, 0.0};
    const int64_t h0 = hyp_off[t], h1 = hyp_off[t + 1];
    int64_t best = -1;
    int best_cnt = 1;   // a surviving hypothesis has its two observations as inliers
    double best_cost = 0.0;
    for (int64_t h = h0; h < h1; ++h) {
        const int n = rec_cnt[h];
        if (n < 2) continue;
        const double cst = rec_cost[h];
        if (best < 0 || n > best_cnt || (n == best_cnt && cst < best_cost)) {
            best = h;
            best_cnt = n;
            best_cost = cst;
        }
    }
    if (best < 0) st = 2;
    if (st == 0) {
        int a, b;
        hyp_pair(best - h0, L, w.max_hyp, a, b);
        if (!(b < L && hyp_point(w, o0, a, b, X))) st = 2;   // cannot happen: the record says it survived
        if (st == 0) {
            classify<true>(w, o0, L, X, a, b, inl, cnt, cost, hit);
            fit_point(w, o0, L, inl, X);
            classify<true>(w, o0, L, X, -1, -1, inl, cnt, cost, hit);   // a non-finite X1 leaves no inlier
            if (cnt < 2) st = 4;
        }
    }
    if (st == 0) {
        fit_point(w, o0, L, inl, X);
        if (!finite3(X)) st = 4;
    }
    if (st == 0) {
        for (int k = 0; k < L; ++k) {
            if (!inl[o0 + k]) continue;
            const int c = w.obs_cam[o0 + k];
            if (c < 0 || c >= w.C) continue;
            const double* P = w.poses + (size_t)c * 12;
            const double z = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
            if (!(z > 0.0)) st = 4;
        }
    }
    if (st == 0) {
        bool wide = false;   // some pair of inlier views whose rays meet at cos <= cos_min
        for (int p = 0; p < L && !wide; ++p) {
            if (!inl[o0 + p]) continue;
            const int ca = w.obs_cam[o0 + p];
            if (ca < 0 || ca >= w.C) continue;
            for (int q = p + 1; q < L && !wide; ++q) {
                if (!inl[o0 + q]) continue;
                const int cb = w.obs_cam[o0 + q];
                if (cb < 0 || cb >= w.C) continue;
                wide = !angle_small(w, ca, cb, X);
            }
        }
        if (!wide) st = 3;
    }
    status[t] = st;
    if (st != 0) {
        for (int k = 0; k < L; ++k) inl[o0 + k] = 0;
        return;   // X, n_inliers and residual keep their failure values
    }
    Xout[3 * t] = X[0];
    Xout[3 * t + 1] = X[1];
    Xout[3 * t + 2] = X[2];
    n_inl[t] = cnt;
    for (int k = 0; k < L; ++k) {
        const int c = w.obs_cam[o0 + k];
        if (c < 0 || c >= w.C) continue;
        double z, e2;
        reproj(w, c, X, w.pts2d[2 * (o0 + k)], w.pts2d[2 * (o0 + k) + 1], z, e2);
        residual[o0 + k] = sqrt(e2);
    }
}

}  // namespace
}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_triangulate_tracks(const double* poses, const double* cam, int C, const int64_t* pt_off, int64_t N,
                                         const int32_t* obs_cam, const double* pts2d, int64_t M,
                                         const int32_t* track_order, double reproj_px, double cos_min, int max_hyp,
                                         int refine_iters, double* X, int32_t* status, int32_t* n_inliers,
                                         uint8_t* inlier, double* residual, int64_t* n_hyp, float* phase_ms,
                                         void* stream) {
    const char* fn = "sfmhip_triangulate_tracks";
    SFMHIP_REQUIRE(C >= 0 && N >= 0 && M >= 0, "%s: bad shape (C %d, N %lld, M %lld)", fn, C, (long long)N, (long long)M);
    SFMHIP_REQUIRE(N <= 0x7FFFFFFF && M <= ((int64_t)1 << 38), "%s: at most 2^31 - 1 tracks and 2^38 observations", fn);
    SFMHIP_REQUIRE(max_hyp >= 1 && max_hyp <= kMaxLen, "%s: max_hyp must be in [1, %d], got %d", fn, kMaxLen, max_hyp);
    SFMHIP_REQUIRE(refine_iters >= 0, "%s: refine_iters must not be negative, got %d", fn, refine_iters);
    SFMHIP_REQUIRE(std::isfinite(reproj_px) && reproj_px > 0.0, "%s: reproj_px must be finite and positive, got %g", fn,
                   reproj_px);
    SFMHIP_REQUIRE(std::isfinite(cos_min) && cos_min > 0.0 && cos_min <= 1.0, "%s: cos_min must be in (0, 1], got %g", fn,
                   cos_min);
    SFMHIP_REQUIRE(std::isfinite(reproj_px * reproj_px), "%s: reproj_px^2 overflows", fn);
    SFMHIP_REQUIRE((N == 0 || (pt_off && X && status && n_inliers)) && (M == 0 || (obs_cam && pts2d && inlier && residual)) &&
                       (C == 0 || (poses && cam)),
                   "%s: null pointer", fn);
    if (n_hyp) *n_hyp = 0;
    if (phase_ms) phase_ms[0] = phase_ms[1] = 0.0f;
    if (N == 0 && M == 0) return SFMHIP_OK;
    hipStream_t st = as_stream(stream);
    TriArgs w;
    w.poses = poses; w.cam = cam; w.pt_off = pt_off; w.obs_cam = obs_cam; w.pts2d = pts2d;
    w.N = N; w.M = M; w.C = C; w.max_hyp = max_hyp; w.refine_iters = refine_iters;
    w.thr2 = reproj_px * reproj_px;
    w.c2 = cos_min * cos_min;
    void* scratch = nullptr;
    const size_t off_bytes = (size_t)(N + 1) * sizeof(int64_t);
    if (scratch_alloc(&scratch, off_bytes + (size_t)std::max(C, 1) * 3 * sizeof(double), st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: scratch allocation failed", fn);
        return SFMHIP_E_HIP;
    }
    int64_t* hyp_off = static_cast<int64_t*>(scratch);
    double* centres = reinterpret_cast<double*>(static_cast<char*>(scratch) + off_bytes);
    w.centres = centres;
    const int64_t n_init = std::max<int64_t>(std::max<int64_t>(N, M), C);
    hipLaunchKernelGGL(tri_init_kernel, dim3((unsigned)((n_init + kWg - 1) / kWg)), dim3(kWg), 0, st, w, centres, hyp_off,
                       X, status, n_inliers, inlier, residual);
    int rc = check_launch("tri_init_kernel");
    if (rc != SFMHIP_OK || N == 0 || M == 0 || C < 2) {   // every track has status 1
        scratch_free(scratch, st);
        return rc;
    }
    hipLaunchKernelGGL(tri_scan_kernel, dim3(1), dim3(kScanWg), 0, st, hyp_off, N);
    rc = check_launch("tri_scan_kernel");
    int64_t H = 0;
    if (rc == SFMHIP_OK && (hipMemcpyAsync(&H, hyp_off + N, sizeof(H), hipMemcpyDeviceToHost, st) != hipSuccess ||
                            hipStreamSynchronize(st) != hipSuccess)) {
        set_error("%s: %s", fn, hipGetErrorString(hipGetLastError()));
        rc = SFMHIP_E_HIP;
    }
    if (rc == SFMHIP_OK && (H < 0 || H > ((int64_t)1 << 38))) {
        set_error("%s: %lld hypotheses, at most 2^38 per call", fn, (long long)H);
        rc = SFMHIP_E_OVERFLOW;
    }
    if (rc != SFMHIP_OK || H == 0) {   // no track has a pair: status 1 everywhere
        scratch_free(scratch, st);
        return rc;
    }
    if (n_hyp) *n_hyp = H;
    void* rec = nullptr;
    if (scratch_alloc(&rec, (size_t)H * (sizeof(double) + sizeof(int32_t)), st) != hipSuccess) {
        (void)hipGetLastError();
        scratch_free(scratch, st);
        set_error("%s: scratch allocation failed (%lld hypotheses)", fn, (long long)H);
        return SFMHIP_E_HIP;
    }
    double* rec_cost = static_cast<double*>(rec);
    int32_t* rec_cnt = reinterpret_cast<int32_t*>(rec_cost + H);
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool timed = phase_ms != nullptr;
    if (timed)
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) timed = false;
    if (timed) (void)hipEventRecord(ev[0], st);
    hipLaunchKernelGGL(tri_score_kernel, dim3((unsigned)((H + kWg - 1) / kWg)), dim3(kWg), 0, st, w, hyp_off, H, rec_cnt,
                       rec_cost);
    rc = check_launch("tri_score_kernel");
    if (timed) (void)hipEventRecord(ev[1], st);
    if (rc == SFMHIP_OK) {
        hipLaunchKernelGGL(tri_fit_kernel, dim3((unsigned)((N + kWg - 1) / kWg)), dim3(kWg), 0, st, w, hyp_off, rec_cnt,
                           rec_cost, track_order, X, status, n_inliers, inlier, residual);
        rc = check_launch("tri_fit_kernel");
    }
    if (timed) {
        (void)hipEventRecord(ev[2], st);
        if (hipEventSynchronize(ev[2]) == hipSuccess) {
            (void)hipEventElapsedTime(&phase_ms[0], ev[0], ev[1]);
            (void)hipEventElapsedTime(&phase_ms[1], ev[1], ev[2]);
        } else {
            (void)hipGetLastError();
        }
    }
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    scratch_free(rec, st);
    scratch_free(scratch, st);
    return rc;
}
