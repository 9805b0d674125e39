// homography.hip — two-view geometry beside the essential matrix, f64:
//   sfmhip_find_homography   cv2.findHomography(src, dst, RANSAC, 3, maxIters 2000, confidence 0.995),
//                            batched over image pairs (OpenCV 4.x calib3d: fundam.cpp
//                            HomographyEstimatorCallback, ptsetreg.cpp RANSACPointSetRegistrator);
//   sfmhip_pair_stats        per-pair parallax (cosine of the angle between the viewing rays of a
//                            correspondence, rotation removed) and 8x8 image coverage words.
// The CPU restatement of both is tests/homog_ref.py.  Parity at the OpenCV boundary is unpinned
// (cv2 absent).
//
// find_homography: one workgroup (4 waves) per pair, hypotheses kHC = 64 at a time:
//   1. lane 0 draws the chunk's four-point samples from cv::RNG(-1) in getSubset's draw order (a
//      sample depends on the draw order only, never on the models);
//   2. one lane per sample: checkSubset (collinear triples, orientation of the four triples), then
//      the model.  Four points in general position fix H exactly, so the sample's model is formed in
//      closed form in the Hartley-normalised frame (H0 = sum_i w_i p_i C_i^T over the projective basis
//      of three of the points, 3x3 cross products only: some 60 live doubles, where a 9x9
//      eigen-solve per lane would hold 126) — the null vector of the 8x9 DLT system up to rounding;
//   3. all 256 lanes score every model of the chunk, kHPB points per lane in registers and the models
//      broadcast from LDS; each wave's ballot counts go to s_cnt[model][wave] (integers, no atomics);
//   4. lane 0 replays the chunk in sample order: a model replaces the best iff count >
//      max(best, 3), niters shrinks by RANSACUpdateNumIters — the sequential loop's outcome for
//      any chunk size, and the same bytes on every run.
// The final H is the normalised DLT over the winning model's inliers: 24 moment sums (fixed
// reduction tree), the 9x9 normal matrix in LDS, cyclic Jacobi with one lane per row.
#include <cfloat>

#include "common.h"
#include "geom_dev.h"

namespace sfmhip {
namespace {

constexpr int kHT = 256;            // threads per pair
constexpr int kHW = kHT / 64;       // waves
constexpr int kHC = 64;             // hypotheses per chunk
constexpr int kHPB = 4;             // points per lane per scoring block (block: kHT * kHPB = 1024 points)
constexpr double kDblEps = 2.220446049250313e-16;
constexpr double kDblMin = 2.2250738585072014e-308;
constexpr double kFltEps = 1.1920928955078125e-07;

// RANSACUpdateNumIters (ptsetreg.cpp).
__device__ int update_num_iters(double p, double ep, int m, int max_iters) {
    p = fmax(p, 0.0);
    p = fmin(p, 1.0);
    ep = fmax(ep, 0.0);
    ep = fmin(ep, 1.0);
    double num = fmax(1.0 - p, kDblMin);
    double denom = 1.0 - pow(1.0 - ep, (double)m);
    if (denom < kDblMin) return 0;
    num = log(num);
    denom = log(denom);
    return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

// haveCollinearPoints' test for the triple (k, j, i), i the last drawn of the three.
__device__ __forceinline__ bool collinear3(const double (&p)[4][2], int k, int j, int i) {
    const double dx1 = p[j][0] - p[i][0], dy1 = p[j][1] - p[i][1];
    const double dx2 = p[k][0] - p[i][0], dy2 = p[k][1] - p[i][1];
    return fabs(dx2 * dy1 - dy2 * dx1) <= kFltEps * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
}

// det [[x0 y0 1] [x1 y1 1] [x2 y2 1]] in cv::determinant's op order for a Matx33.
__device__ __forceinline__ double orient3(const double (&p)[4][2], int a, int b, int c) {
    return (p[a][0] * (p[b][1] - p[c][1]) - p[a][1] * (p[b][0] - p[c][0])) + (p[b][0] * p[c][1] - p[b][1] * p[c][0]);
}

// HomographyEstimatorCallback::checkSubset on a four-point sample: no three points collinear in
// either image, and every triple keeps its orientation.
__device__ bool check_subset(const double (&a)[4][2], const double (&b)[4][2]) {
    constexpr int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    bool ok = true;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        ok = ok && !collinear3(a, tt[t][0], tt[t][1], tt[t][2]) && !collinear3(b, tt[t][0], tt[t][1], tt[t][2]);
        ok = ok && !(orient3(a, tt[t][0], tt[t][1], tt[t][2]) * orient3(b, tt[t][0], tt[t][1], tt[t][2]) < 0);
    }
    return ok;
}

// OpenCV's normalisation of a point set: x' = (x - c) * s, c the centroid, s = count / sum |x - c|.
struct HNorm {
    double cx, cy, sx, sy;
};

// H = invHnorm(dst) * H0 * Hnorm2(src), divided by H[8].  False (no model) when |H[8]| < DBL_EPSILON
// or an entry is not finite.
__device__ bool denormalise(const double* H0, const HNorm& ns, const HNorm& nd, double* H) {
    double T[9];
    const double ix = 1.0 / nd.sx, iy = 1.0 / nd.sy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        T[c] = H0[c] * ix + nd.cx * H0[6 + c];
        T[3 + c] = H0[3 + c] * iy + nd.cy * H0[6 + c];
        T[6 + c] = H0[6 + c];
    }
    const double tx = -ns.cx * ns.sx, ty = -ns.cy * ns.sy;
    double G[9];
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[3 * r] = T[3 * r] * ns.sx;
        G[3 * r + 1] = T[3 * r + 1] * ns.sy;
        G[3 * r + 2] = (T[3 * r] * tx + T[3 * r + 1] * ty) + T[3 * r + 2];
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) fin = fin && isfinite(G[e]);
    if (!fin || !(fabs(G[8]) >= kDblEps)) return false;
    const double inv = 1.0 / G[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        H[e] = G[e] * inv;
        fin = fin && isfinite(H[e]);
    }
    H[8] = 1.0;
    return fin;
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// The model of one four-point sample (a: src, b: dst, pixels).  False: the sample proposes no model.
__device__ bool sample_model(const double (&a)[4][2], const double (&b)[4][2], double* H) {
    if (!check_subset(a, b)) return false;
    HNorm ns, nd;
    ns.cx = (((a[0][0] + a[1][0]) + a[2][0]) + a[3][0]) / 4;
    ns.cy = (((a[0][1] + a[1][1]) + a[2][1]) + a[3][1]) / 4;
    nd.cx = (((b[0][0] + b[1][0]) + b[2][0]) + b[3][0]) / 4;
    nd.cy = (((b[0][1] + b[1][1]) + b[2][1]) + b[3][1]) / 4;
    double sa[2] = {0, 0}, sb[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sa[0] += fabs(a[i][0] - ns.cx);
        sa[1] += fabs(a[i][1] - ns.cy);
        sb[0] += fabs(b[i][0] - nd.cx);
        sb[1] += fabs(b[i][1] - nd.cy);
    }
    if (sa[0] < kDblEps || sa[1] < kDblEps || sb[0] < kDblEps || sb[1] < kDblEps) return false;
    ns.sx = 4 / sa[0]; ns.sy = 4 / sa[1];
    nd.sx = 4 / sb[0]; nd.sy = 4 / sb[1];
    double P[4][3], Q[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        P[i][0] = (a[i][0] - ns.cx) * ns.sx; P[i][1] = (a[i][1] - ns.cy) * ns.sy; P[i][2] = 1.0;
        Q[i][0] = (b[i][0] - nd.cx) * nd.sx; Q[i][1] = (b[i][1] - nd.cy) * nd.sy; Q[i][2] = 1.0;
    }
    // projective bases: P3 = sum_i (lam_i / det) P_i with lam_i = C_i . P3, C_0 = P1 x P2, ...; the same
    // for the destination (mu_i, D_i).  H0 = sum_i (mu_i / lam_i) Q_i C_i^T, scaled by lam_0 lam_1 lam_2.
    double C[3][3], D[3], lam[3], mu[3];
    cross3(P[1], P[2], C[0]);
    cross3(P[2], P[0], C[1]);
    cross3(P[0], P[1], C[2]);
    cross3(Q[1], Q[2], D); mu[0] = dot3(D, Q[3]);
    cross3(Q[2], Q[0], D); mu[1] = dot3(D, Q[3]);
    cross3(Q[0], Q[1], D); mu[2] = dot3(D, Q[3]);
#pragma unroll
    for (int i = 0; i < 3; ++i) lam[i] = dot3(C[i], P[3]);
    const double w[3] = {mu[0] * (lam[1] * lam[2]), mu[1] * (lam[0] * lam[2]), mu[2] * (lam[0] * lam[1])};
    double H0[9], n2 = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = (w[0] * Q[0][r] * C[0][c] + w[1] * Q[1][r] * C[1][c]) + w[2] * Q[2][r] * C[2][c];
            H0[3 * r + c] = v;
            n2 += v * v;
        }
    if (!(n2 > 0) || !isfinite(n2)) return false;
    const double inv = 1.0 / sqrt(n2);
#pragma unroll
    for (int e = 0; e < 9; ++e) H0[e] *= inv;
    return denormalise(H0, ns, nd, H);
}

// HomographyEstimatorCallback::computeError's forward transfer error in f64, stored as float.
__device__ __forceinline__ float transfer_error(const double* H, double x, double y, double X, double Y) {
    const double ww = 1.0 / ((H[6] * x + H[7] * y) + H[8]);
    const double dx = ((H[0] * x + H[1] * y) + H[2]) * ww - X;
    const double dy = ((H[3] * x + H[4] * y) + H[5]) * ww - Y;
    return (float)(dx * dx + dy * dy);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Block sums of K doubles per lane: xor butterfly per wave, the waves added in wave order — one
// fixed tree, so the same bytes on every run.  Every lane gets the sums.  s_red: [kHW][K].
template <int K>
__device__ void block_sums(double (&v)[K], double* s_red, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum_f64(v[k]);
        if (lane == 0) s_red[wave * K + k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = s_red[k];
#pragma unroll
        for (int w = 1; w < kHW; ++w) s += s_red[w * K + k];
        v[k] = s;
    }
    __syncthreads();
}

// Eigenvector of the smallest eigenvalue of the symmetric 9x9 matrix in s_A (destroyed), by cyclic
// Jacobi: lane r < 9 of the calling wave owns row r in the column update (A <- A J, V <- V J) and
// column r in the row update (A <- J^T A).  Every lane of the wave must call it; v gets the vector.
__device__ void jacobi9_min(double (*s_A)[9], double (*s_V)[9], int lane, double* v) {
    if (lane < 9)
#pragma unroll
        for (int c = 0; c < 9; ++c) s_V[lane][c] = (c == lane) ? 1.0 : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    double tr = 0;
    for (int k = 0; k < 9; ++k) tr += fabs(s_A[k][k]);
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double app = s_A[p][p], aqq = s_A[q][q], apq = s_A[p][q];
                if (apq == 0.0 || fabs(apq) <= 1e-20 * tr || fabs(apq) <= 1e-18 * sqrt(fabs(app * aqq))) continue;
                rotated = true;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                if (lane < 9) {
                    const double arp = s_A[lane][p], arq = s_A[lane][q];
                    s_A[lane][p] = c * arp - s * arq;
                    s_A[lane][q] = s * arp + c * arq;
                    const double vrp = s_V[lane][p], vrq = s_V[lane][q];
                    s_V[lane][p] = c * vrp - s * vrq;
                    s_V[lane][q] = s * vrp + c * vrq;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (lane < 9) {
                    const double apc = s_A[p][lane], aqc = s_A[q][lane];
                    s_A[p][lane] = (lane == q) ? 0.0 : c * apc - s * aqc;
                    s_A[q][lane] = (lane == p) ? 0.0 : s * apc + c * aqc;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
        if (!rotated) break;
    }
    int best = 0;
    double bv = s_A[0][0];
    for (int k = 1; k < 9; ++k)
        if (s_A[k][k] < bv) { bv = s_A[k][k]; best = k; }
    for (int r = 0; r < 9; ++r) v[r] = s_V[r][best];
}

__global__ __launch_bounds__(kHT) void homography_ransac_kernel(
    const double* __restrict__ pts0, const double* __restrict__ pts1, const int64_t* __restrict__ offs,
    double threshold, double confidence, int max_iters, double* __restrict__ H_out, int32_t* __restrict__ ok_out,
    uint8_t* __restrict__ mask, int32_t* __restrict__ ninl_out, int32_t* __restrict__ iters_out) {
    __shared__ double s_H[kHC][9];
    __shared__ int s_valid[kHC];
    __shared__ int s_cnt[kHC][kHW];
    __shared__ int s_sub[kHC * 4];
    __shared__ double s_best[9];
    __shared__ double s_red[kHW * 24];
    __shared__ double s_A[9][9], s_V[9][9];
    __shared__ int s_niters, s_maxgood, s_k0, s_last;

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t off = offs[p];
    const int64_t n64 = offs[p + 1] - off;
    const int n = n64 < 0 ? 0 : (int)n64;   // a malformed (decreasing) offset pair is an empty pair
    const float tf = (float)(threshold * threshold);
    const double* A0 = pts0 + 2 * off;
    const double* B0 = pts1 + 2 * off;
    double* Ho = H_out + (int64_t)p * 9;
    for (int i = tid; i < n; i += kHT) mask[off + i] = 0;
    if (tid == 0) {
        s_niters = max(max_iters, 1);
        s_maxgood = 0;
        s_k0 = 0;
        s_last = -1;
    }
    __syncthreads();
    if (n < 4) {
        if (tid == 0) {
            ok_out[p] = 0; ninl_out[p] = 0; iters_out[p] = 0;
            for (int e = 0; e < 9; ++e) Ho[e] = 0.0;
        }
        return;
    }
    uint64_t rng = ~0ULL;   // cv::RNG(-1); lane 0's copy is the stream
    const unsigned mg = (unsigned)(0x100000000ULL / (unsigned)n);
    for (;;) {
        const int k0 = s_k0, niters = s_niters;
        const int nh = (n == 4) ? 1 : min(kHC, niters - k0);
        if (tid == 0) {
            if (n == 4) {   // count == modelPoints: one model from all the points
                for (int i = 0; i < 4; ++i) s_sub[i] = i;
            } else {
                for (int hh = 0; hh < nh; ++hh)
                    for (int i = 0; i < 4; ++i) {
                        int idx;
                        for (;;) {
                            rng = (uint64_t)(unsigned)rng * 4164903690ULL + (unsigned)(rng >> 32);
                            idx = (int)cv_rng_mod((unsigned)rng, (unsigned)n, mg);
                            int j = 0;
                            while (j < i && s_sub[hh * 4 + j] != idx) ++j;
                            if (j == i) break;
                        }
                        s_sub[hh * 4 + i] = idx;
                    }
            }
        }
        for (int i = tid; i < kHC * kHW; i += kHT) (&s_cnt[0][0])[i] = 0;
        __syncthreads();
        if (tid < kHC) {
            bool ok = false;
            if (tid < nh) {
                double a[4][2], b[4][2], Hm[9];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int idx = s_sub[tid * 4 + j];
                    a[j][0] = A0[2 * idx]; a[j][1] = A0[2 * idx + 1];
                    b[j][0] = B0[2 * idx]; b[j][1] = B0[2 * idx + 1];
                }
                ok = sample_model(a, b, Hm);
                if (ok)
#pragma unroll
                    for (int e = 0; e < 9; ++e) s_H[tid][e] = Hm[e];
            }
            s_valid[tid] = ok ? 1 : 0;
        }
        __syncthreads();
        for (int b0 = 0; b0 < n; b0 += kHT * kHPB) {
            double pt[kHPB][4];
            bool val[kHPB];
#pragma unroll
            for (int u = 0; u < kHPB; ++u) {
                const int i = b0 + u * kHT + tid;
                val[u] = i < n;
                pt[u][0] = val[u] ? A0[2 * i] : 0.0;
                pt[u][1] = val[u] ? A0[2 * i + 1] : 0.0;
                pt[u][2] = val[u] ? B0[2 * i] : 0.0;
                pt[u][3] = val[u] ? B0[2 * i + 1] : 0.0;
            }
            for (int j = 0; j < nh; ++j) {
                if (!s_valid[j]) continue;   // uniform
                double Hm[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) Hm[e] = s_H[j][e];
                int c = 0;
#pragma unroll
                for (int u = 0; u < kHPB; ++u)
                    c += __popcll(__ballot(val[u] && transfer_error(Hm, pt[u][0], pt[u][1], pt[u][2], pt[u][3]) <= tf));
                if (lane == 0) s_cnt[j][wave] += c;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int nit = niters, maxgood = s_maxgood, last = s_last;
            for (int hh = 0; hh < nh; ++hh) {
                const int k = k0 + hh;
                if (k >= nit) break;
                if (s_valid[hh]) {
                    int good = 0;
                    for (int w = 0; w < kHW; ++w) good += s_cnt[hh][w];
                    if (n == 4) good = 4;   // count == modelPoints: the mask is all ones
                    if (good > max(maxgood, 3)) {
                        for (int e = 0; e < 9; ++e) s_best[e] = s_H[hh][e];
                        maxgood = good;
                        nit = update_num_iters(confidence, (double)(n - good) / n, 4, nit);
                    }
                }
                last = k;
            }
            if (n == 4) nit = 0;
            s_niters = nit;
            s_maxgood = maxgood;
            s_last = last;
            s_k0 = k0 + kHC;
        }
        __syncthreads();
        if (s_k0 >= s_niters) break;
    }
    const int maxgood = s_maxgood;
    if (maxgood <= 0) {
        if (tid == 0) {
            ok_out[p] = 0; ninl_out[p] = 0; iters_out[p] = s_last + 1;
            for (int e = 0; e < 9; ++e) Ho[e] = 0.0;
        }
        return;
    }
    // the winning sample model's mask, and the refit on its inliers: moments in two passes
    // (centroids, then mean absolute deviations), then the 24 sums that make up the normal matrix
    double Hb[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Hb[e] = s_best[e];
    double m4[4] = {0, 0, 0, 0};
    for (int i = tid; i < n; i += kHT) {
        const double x = A0[2 * i], y = A0[2 * i + 1], X = B0[2 * i], Y = B0[2 * i + 1];
        const bool in = (n == 4) || transfer_error(Hb, x, y, X, Y) <= tf;
        mask[off + i] = in ? 1 : 0;
        if (in) { m4[0] += x; m4[1] += y; m4[2] += X; m4[3] += Y; }
    }
    block_sums<4>(m4, s_red, tid);   // (a lane reads back only the mask rows it wrote itself)
    HNorm ns, nd;
    ns.cx = m4[0] / maxgood; ns.cy = m4[1] / maxgood;
    nd.cx = m4[2] / maxgood; nd.cy = m4[3] / maxgood;
    double d4[4] = {0, 0, 0, 0};
    for (int i = tid; i < n; i += kHT)
        if (mask[off + i]) {
            d4[0] += fabs(A0[2 * i] - ns.cx);
            d4[1] += fabs(A0[2 * i + 1] - ns.cy);
            d4[2] += fabs(B0[2 * i] - nd.cx);
            d4[3] += fabs(B0[2 * i + 1] - nd.cy);
        }
    block_sums<4>(d4, s_red, tid);
    const bool spread = !(d4[0] < kDblEps || d4[1] < kDblEps || d4[2] < kDblEps || d4[3] < kDblEps);
    if (spread) {
        ns.sx = maxgood / d4[0]; ns.sy = maxgood / d4[1];
        nd.sx = maxgood / d4[2]; nd.sy = maxgood / d4[3];
        // rows Lx = [P, 0, -x P], Ly = [0, P, -y P], P = (X, Y, 1) the source, (x, y) the destination:
        // L^T L = [[S, 0, -Sx], [0, S, -Sy], [-Sx, -Sy, Sr]] with S = sum P P^T, Sx = sum x P P^T,
        // Sy = sum y P P^T, Sr = sum (x^2 + y^2) P P^T; six entries each (00 01 02 11 12 22)
        double m[24];
#pragma unroll
        for (int k = 0; k < 24; ++k) m[k] = 0.0;
        for (int i = tid; i < n; i += kHT)
            if (mask[off + i]) {
                const double X = (A0[2 * i] - ns.cx) * ns.sx, Y = (A0[2 * i + 1] - ns.cy) * ns.sy;
                const double x = (B0[2 * i] - nd.cx) * nd.sx, y = (B0[2 * i + 1] - nd.cy) * nd.sy;
                const double pp[6] = {X * X, X * Y, X, Y * Y, Y, 1.0};
                const double r2 = x * x + y * y;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    m[k] += pp[k];
                    m[6 + k] += x * pp[k];
                    m[12 + k] += y * pp[k];
                    m[18 + k] += r2 * pp[k];
                }
            }
        block_sums<24>(m, s_red, tid);
        if (tid == 0) {
            constexpr int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    const int k = sym[r][c];
                    s_A[r][c] = m[k];          s_A[r][3 + c] = 0.0;       s_A[r][6 + c] = -m[6 + k];
                    s_A[3 + r][c] = 0.0;       s_A[3 + r][3 + c] = m[k];  s_A[3 + r][6 + c] = -m[12 + k];
                    s_A[6 + r][c] = -m[6 + k]; s_A[6 + r][3 + c] = -m[12 + k]; s_A[6 + r][6 + c] = m[18 + k];
                }
        }
    }
    __syncthreads();
    if (wave == 0) {
        bool refit = false;
        double Hr[9];
        if (spread) {
            double v[9];
            jacobi9_min(s_A, s_V, lane, v);
            refit = denormalise(v, ns, nd, Hr);
        }
        if (tid == 0) {
            ok_out[p] = 1;
            ninl_out[p] = maxgood;
            iters_out[p] = s_last + 1;
            // a refit that yields no model leaves the sample's model (OpenCV ignores its status)
            for (int e = 0; e < 9; ++e) Ho[e] = refit ? Hr[e] : Hb[e];
        }
    }
}

// Wave OR of a 64-bit word.
__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (unsigned long long)__shfl_xor((long long)v, o);
    return v;
}

// Bit of the 8x8 grid cell of (x, y) over [0, W) x [0, H); 0 for a point outside the image.
__device__ __forceinline__ unsigned long long cover_bit(double x, double y, double W, double H) {
    if (!(x >= 0.0 && x < W && y >= 0.0 && y < H)) return 0ULL;
    const int cx = min((int)floor(8.0 * x / W), 7), cy = min((int)floor(8.0 * y / H), 7);
    return 1ULL << (cy * 8 + cx);
}

__global__ __launch_bounds__(kHT) void pair_stats_kernel(
    const double* __restrict__ pts0, const double* __restrict__ pts1, const int64_t* __restrict__ offs,
    const uint8_t* __restrict__ mask, const double* __restrict__ Rm, const double* __restrict__ cam, double W,
    double H, double* __restrict__ cosang, float* __restrict__ cos32, int64_t* __restrict__ rank,
    unsigned long long* __restrict__ cover, int32_t* __restrict__ n_sel) {
    __shared__ unsigned long long s_c0[kHW], s_c1[kHW];
    __shared__ int s_n[kHW];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t off = offs[p];
    const int64_t n64 = offs[p + 1] - off;
    const int n = n64 < 0 ? 0 : (int)n64;
    double R[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = Rm[9 * (int64_t)p + e];
    const double fx = cam[4 * p], fy = cam[4 * p + 1], cx = cam[4 * p + 2], cy = cam[4 * p + 3];
    unsigned long long c0 = 0, c1 = 0;
    int cnt = 0;
    for (int i = tid; i < n; i += kHT) {
        double c = 2.0;   // the sentinel of a masked-out row: above every cosine
        if (mask[off + i]) {
            const double x0 = pts0[2 * (off + i)], y0 = pts0[2 * (off + i) + 1];
            const double x1 = pts1[2 * (off + i)], y1 = pts1[2 * (off + i) + 1];
            const double a0 = (x0 - cx) / fx, a1 = (y0 - cy) / fy;
            const double b0 = (x1 - cx) / fx, b1 = (y1 - cy) / fy;
            // R^T (b0, b1, 1)
            const double r0 = (R[0] * b0 + R[3] * b1) + R[6];
            const double r1 = (R[1] * b0 + R[4] * b1) + R[7];
            const double r2 = (R[2] * b0 + R[5] * b1) + R[8];
            const double num = (a0 * r0 + a1 * r1) + r2;
            const double den = sqrt(((a0 * a0 + a1 * a1) + 1.0) * ((r0 * r0 + r1 * r1) + r2 * r2));
            c = num / den;
            c0 |= cover_bit(x0, y0, W, H);
            c1 |= cover_bit(x1, y1, W, H);
            ++cnt;
        }
        cosang[off + i] = c;
        cos32[off + i] = (float)c;
    }
    c0 = wave_or_u64(c0);
    c1 = wave_or_u64(c1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) { s_c0[wave] = c0; s_c1[wave] = c1; s_n[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long w0 = 0, w1 = 0;
        int m = 0;
        for (int w = 0; w < kHW; ++w) { w0 |= s_c0[w]; w1 |= s_c1[w]; m += s_n[w]; }
        cover[2 * (int64_t)p] = w0;
        cover[2 * (int64_t)p + 1] = w1;
        n_sel[p] = m;
        rank[p] = m > 0 ? (m - 1) / 2 : 0;   // the lower median of the selected rows (the sentinels sort last)
    }
}

}  // namespace
}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_find_homography(const double* pts0, const double* pts1, const int64_t* offsets, int n_pairs,
                                      double threshold, double confidence, int max_iters, double* H, int32_t* ok,
                                      uint8_t* mask, int32_t* n_inliers, int32_t* iters, void* stream) {
    SFMHIP_REQUIRE(n_pairs >= 0, "find_homography: n_pairs < 0");
    if (n_pairs == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(pts0 && pts1 && offsets && H && ok && mask && n_inliers && iters, "find_homography: null pointer");
    SFMHIP_REQUIRE(confidence >= 0 && confidence <= 1 && threshold > 0,
                   "find_homography: confidence in [0,1], threshold > 0");
    hipLaunchKernelGGL(homography_ransac_kernel, dim3(n_pairs), dim3(kHT), 0, as_stream(stream), pts0, pts1, offsets,
                       threshold, confidence, max_iters, H, ok, mask, n_inliers, iters);
    return check_launch("homography_ransac_kernel");
}

extern "C" int sfmhip_pair_stats(const double* pts0, const double* pts1, const int64_t* offsets, int n_pairs,
                                 int64_t n_points, const uint8_t* mask, const double* R, const double* cam,
                                 double width, double height, double* cosang, float* work, int64_t* rank_work,
                                 uint64_t* cover, int32_t* n_sel, float* median, void* stream) {
    SFMHIP_REQUIRE(n_pairs >= 0 && n_points >= 0, "pair_stats: n_pairs < 0 or n_points < 0");
    if (n_pairs == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(offsets && R && cam && rank_work && cover && n_sel && median, "pair_stats: null pointer");
    SFMHIP_REQUIRE(n_points == 0 || (pts0 && pts1 && mask && cosang && work), "pair_stats: null pointer");
    SFMHIP_REQUIRE(width > 0 && height > 0, "pair_stats: width, height > 0");
    hipLaunchKernelGGL(pair_stats_kernel, dim3(n_pairs), dim3(kHT), 0, as_stream(stream), pts0, pts1, offsets, mask, R,
                       cam, width, height, cosang, work, rank_work, reinterpret_cast<unsigned long long*>(cover), n_sel);
    const int rc = check_launch("pair_stats_kernel");
    if (rc != SFMHIP_OK) return rc;
    // the median as an exact order statistic of the device's own values (the f32 cast is monotone)
    return sfmhip_segmented_select(work, n_points, offsets, n_pairs, rank_work, 1, median, stream);
}
