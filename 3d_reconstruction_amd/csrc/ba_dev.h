// ba_dev.h — pieces shared by the global bundle adjustments (ba_global.hip: pinhole, K fixed;
// ba_calib.hip: shared intrinsics and radial distortion as unknowns).  Every function here is
// the one ba_global.hip held before ba_calib.hip existed, operation for operation.
#pragma once
#include "common.h"
#include <algorithm>
#include <cmath>

namespace sfmhip {
namespace {

constexpr int kWg = 256;
constexpr int kChunk = 256;            // observations per camera chunk (= one per lane)
constexpr double kFloor = 1e-12;       // floor of a damped diagonal entry
constexpr double kLambda0 = 1e-4, kLambdaMin = 1e-12, kLambdaMax = 1e12;
enum { kMatvec = 0, kRhs = 1, kBacksub = 2 };
enum { kLinear = 0, kHuber = 1, kSoftL1 = 2, kCauchy = 3 };   // loss codes of the C ABI

__device__ __forceinline__ bool is_fixed(const uint8_t* f, int c) { return f != nullptr && f[c] != 0; }

// Sum over the workgroup by the pairwise tree (stride 128, ..., 1); every lane gets the sum.
__device__ __forceinline__ double block_sum(double v, double* sm) {
    const int tid = threadIdx.x;
    sm[tid] = v;
    __syncthreads();
    for (int s = kWg / 2; s >= 1; s >>= 1) {
        if (tid < s) sm[tid] = sm[tid] + sm[tid + s];
        __syncthreads();
    }
    const double out = sm[0];
    __syncthreads();
    return out;
}

// Structure check of the sorted observation layout for entry i of the launch: every read is
// guarded by the checks before it.  True: malformed.
__device__ __forceinline__ bool structure_bad(int64_t i, const int32_t* oc, const int32_t* op, const int64_t* pt_off,
                                              const int64_t* cam_perm, const int64_t* cam_off, int C, int N,
                                              int64_t M) {
    bool bad = false;
    if (i <= N) {
        const int64_t o = pt_off[i];
        bad |= o < 0 || o > M || (i == 0 && o != 0) || (i == N && o != M) || (i < N && pt_off[i + 1] < o);
    }
    if (i <= C) {
        const int64_t o = cam_off[i];
        bad |= o < 0 || o > M || (i == 0 && o != 0) || (i == C && o != M) || (i < C && cam_off[i + 1] < o);
    }
    if (i < M) {
        const int c = oc[i], p = op[i];
        if (c < 0 || c >= C || p < 0 || p >= N) {
            bad = true;
        } else {
            bad |= !(pt_off[p] <= i && i < pt_off[p + 1]);
            if (i > 0 && op[i - 1] == p) bad |= oc[i - 1] > c;
        }
        const int64_t j = cam_perm[i];
        if (j < 0 || j >= M) {
            bad = true;
        } else {
            const int cj = oc[j];
            if (cj < 0 || cj >= C) {
                bad = true;
            } else {
                const int64_t lo = cam_off[cj];
                bad |= !(lo <= i && i < cam_off[cj + 1]);
                if (i > 0 && i > lo) bad |= !(cam_perm[i - 1] < j);
            }
        }
    }
    return bad;
}

// chunk_base[c] = first chunk of camera c (chunk_base[C] = number of chunks), chunk_cam = the
// owner of every chunk; one lane walks the cameras in sequence.  W: the workspace of the caller.
template <class W>
__device__ __forceinline__ void chunk_numbering(const W& w) {
    int base = 0;
    for (int c = 0; c < w.C; ++c) {
        w.chunk_base[c] = base;
        const int n = (int)((w.cam_off[c + 1] - w.cam_off[c] + kChunk - 1) / kChunk);
        for (int k = 0; k < n && base + k < w.tmax; ++k) w.chunk_cam[base + k] = c;
        base = min(base + n, w.tmax);
    }
    w.chunk_base[w.C] = base;
}

// One workgroup per camera chunk: NV values per observation from F, summed through the tree.
template <int NV, class W, class F>
__device__ __forceinline__ void chunk_reduce(const W& w, double* part, F f) {
    __shared__ double sm[NV * kWg];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= w.chunk_base[w.C]) return;
    const int c = w.chunk_cam[b];
    const int64_t pos = w.cam_off[c] + (int64_t)(b - w.chunk_base[c]) * kChunk + tid;
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    if (pos < w.cam_off[c + 1]) f(w.cam_perm[pos], v);
#pragma unroll
    for (int k = 0; k < NV; ++k) sm[k * kWg + tid] = v[k];
    __syncthreads();
    for (int s = kWg / 2; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < NV; ++k) sm[k * kWg + tid] = sm[k * kWg + tid] + sm[k * kWg + tid + s];
        }
        __syncthreads();
    }
    if (tid < NV) part[(int64_t)b * NV + tid] = sm[tid * kWg];
}

// Inverse of an SPD NxN block (row-major) by LDL^T and unit-vector solves.
template <int N>
__device__ __forceinline__ void ldl_inverse(const double* A, double* Ai) {
    double L[N][N], d[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double acc = A[j * N + j];
#pragma unroll
        for (int m = 0; m < j; ++m) acc = acc - (L[j][m] * L[j][m]) * d[m];
        d[j] = acc;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double a2 = A[i * N + j];
#pragma unroll
            for (int m = 0; m < j; ++m) a2 = a2 - (L[i][m] * L[j][m]) * d[m];
            L[i][j] = a2 / d[j];
        }
    }
#pragma unroll
    for (int e = 0; e < N; ++e) {
        double z[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double acc = i == e ? 1.0 : 0.0;
#pragma unroll
            for (int m = 0; m < i; ++m) acc = acc - L[i][m] * z[m];
            z[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = z[i] / d[i];
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {
            double acc = z[i];
#pragma unroll
            for (int m = i + 1; m < N; ++m) acc = acc - L[m][i] * z[m];
            z[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) Ai[i * N + e] = z[i];
    }
}

// A + lambda diag(A), each diagonal entry floored, then the inverse.
template <int N>
__device__ __forceinline__ void damp_invert(const double* A, double lam, double* As, double* Ai) {
    double a[N * N];
#pragma unroll
    for (int k = 0; k < N * N; ++k) a[k] = A[k];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double dg = a[i * N + i] + lam * a[i * N + i];
        a[i * N + i] = dg >= kFloor ? dg : kFloor;
    }
    if (As != nullptr) {
#pragma unroll
        for (int k = 0; k < N * N; ++k) As[k] = a[k];
    }
    double inv[N * N];
    ldl_inverse<N>(a, inv);
#pragma unroll
    for (int k = 0; k < N * N; ++k) Ai[k] = inv[k];
}

// rho'(z) and rho(z) of the robust losses (scipy's definitions), z = |r|^2 / f^2 of one observation.
template <int LOSS>
__device__ __forceinline__ double loss_weight(double z) {
    if (LOSS == kHuber) return z <= 1.0 ? 1.0 : 1.0 / sqrt(z);
    if (LOSS == kSoftL1) return 1.0 / sqrt(1.0 + z);
    return 1.0 / (1.0 + z);
}

template <int LOSS>
__device__ __forceinline__ double loss_rho(double z) {
    if (LOSS == kHuber) return z <= 1.0 ? z : 2.0 * sqrt(z) - 1.0;
    if (LOSS == kSoftL1) return 2.0 * (sqrt(1.0 + z) - 1.0);
    return log1p(z);
}

// Matrix -> rotation vector: the axis from the skew part, the angle atan2(s, c).
__device__ inline void rodrigues_inverse(const double* R, double* rv) {
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1.0) * 0.5;
    c = fmin(fmax(c, -1.0), 1.0);
    double theta = atan2(s, c);
    if (s < 1e-5) {
        if (c > 0.0) {
            rv[0] = rx * 0.5; rv[1] = ry * 0.5; rv[2] = rz * 0.5;
            return;
        }
        rx = sqrt(fmax((R[0] + 1.0) * 0.5, 0.0));
        ry = sqrt(fmax((R[4] + 1.0) * 0.5, 0.0)) * (R[1] < 0.0 ? -1.0 : 1.0);
        rz = sqrt(fmax((R[8] + 1.0) * 0.5, 0.0)) * (R[2] < 0.0 ? -1.0 : 1.0);
        if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0.0) != (ry * rz > 0.0)) rz = -rz;
        theta = theta / sqrt(rx * rx + ry * ry + rz * rz);
        rv[0] = rx * theta; rv[1] = ry * theta; rv[2] = rz * theta;
        return;
    }
    const double vth = theta / (2.0 * s);
    rv[0] = rx * vth; rv[1] = ry * vth; rv[2] = rz * vth;
}

// Host side: one scratch allocation carved into the arrays a call needs.
struct Arena {
    char* base = nullptr;
    size_t used = 0;
    template <class T>
    T* take(size_t n) {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~size_t(255);
        return p;
    }
};

inline int grid_of(int64_t n) { return std::max(1, ceil_div(n, kWg)); }

}  // namespace
}  // namespace sfmhip
