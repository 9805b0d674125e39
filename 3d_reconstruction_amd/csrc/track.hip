// track.hip — V9: frame-to-model camera tracking, point-to-plane ICP of a depth frame against
// the maps sfmhip_tsdf_raycast leaves (semantics: include/sfmhip.h V9, restated in numpy by
// tests/tsdf_track_ref.py).  Two kernels per iteration, plain launches on the caller's stream:
//   reduce  one lane per frame pixel, a wave = an 8 x 8 pixel tile, a workgroup = 16 x 16
//           pixels; a workgroup walks `share` consecutive 16 x 16 tiles (a function of the
//           frame's shape only) and keeps the 29 f64 sums per lane in registers, then one wave
//           reduction by shuffles, one cross-wave reduction through LDS in wave order, and
//           one 29-double partial per workgroup in scratch.  No atomics: the order of every
//           addition is fixed by the shapes.
//   solve   one workgroup per view: the view's partials summed in index order, in 32 runs of
//           consecutive partials side by side and then the runs in order (the launch-boundary
//           reduce: combined in the next kernel's prologue; one lane adding all of them paid
//           one load latency per partial, 40 - 60 us), then on one lane the 6 x 6 LDL^T,
//           Rodrigues and the pose composition in f64; writes the f64 pose state, its f32
//           rounding (which the next reduce reads) and the log record.
// The per-pixel arithmetic is f32 with -ffp-contract=off: mask and n are bit-identical to the
// numpy form; every product summed is exact in f64.
#include "common.h"
#include <climits>
#include <cmath>

namespace sfmhip {
namespace {

constexpr int kSums = 29;          // 21 A (upper triangle, row-major), 6 g, E, n
constexpr int kLog = 36;           // 29 sums, 6 delta, status
// 1936 x 1296 / 484 x 324, 10 iterations: (4, 1024) 0.54 / 0.29 ms, (4, 256) 0.94 / 0.29,
// (1, 1024) 0.53 / 0.31, (2, 512) 0.64 / 0.28, (4, 2048) 0.66 / 0.27 (tools/bench_tsdf_track.py)
constexpr int kShareMin = 4;       // 16 x 16 tiles per workgroup at least
constexpr int kPartialsMax = 1024; // workgroups per view at most
constexpr int kRuns = 32;          // the solve sums a view's partials in 32 runs
constexpr int kSolveThreads = 32 * kRuns;

struct IcpArgs {
    const float* depth_f;
    const float* Kf;
    const float* pose;
    const float* depth_m;
    const float* normals_m;
    const float* pose_m;
    const float* Km;
    int Hf, Wf, Hm, Wm;
    int ntx, nt, share;
    float dist2, cos2;
    const int* state;   // nullable: per-view status of the track so far (non-zero: lost)
    double* partials;   // [B][gridDim.x][29]
    uint8_t* mask;      // nullable
};

__device__ __forceinline__ bool depth_ok(float d) { return d > 0.f && d < 0x1p60f; }

// the view's 32 camera values: wave-uniform addresses of read-only memory (scalar loads)
__device__ __forceinline__ bool load_cams(const float* __restrict__ pose, const float* __restrict__ pose_m,
                                          const float* __restrict__ Kf, const float* __restrict__ Km, int view,
                                          float* P, float* M, float* K, float* Km4) {
    bool good = true;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        P[q] = pose[view * 12 + q];
        M[q] = pose_m[view * 12 + q];
        good = good && fabsf(P[q]) < 0x1p60f && fabsf(M[q]) < 0x1p60f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        K[q] = Kf[view * 4 + q];
        Km4[q] = Km[view * 4 + q];
        good = good && fabsf(K[q]) < 0x1p60f && fabsf(Km4[q]) < 0x1p60f;
    }
    return good && K[0] != 0.f && K[1] != 0.f && Km4[0] != 0.f && Km4[1] != 0.f;
}

__global__ __launch_bounds__(256) void icp_reduce_kernel(IcpArgs A) {
    __shared__ double red[4][kSums];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int view = blockIdx.y;
    if (A.state && A.state[view] != 0) return;   // a lost view: its later iterations are no-ops

    float P[12], M[12], K[4], Km[4];
    const bool good = load_cams(A.pose, A.pose_m, A.Kf, A.Km, view, P, M, K, Km);
    const float* __restrict__ depth_f = A.depth_f + (size_t)view * A.Hf * A.Wf;
    const float* __restrict__ depth_m = A.depth_m + (size_t)view * A.Hm * A.Wm;
    const float* __restrict__ normals_m = A.normals_m + (size_t)view * A.Hm * A.Wm * 3;

    double s[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = 0.0;

    const int t0 = blockIdx.x * A.share, t1 = min(t0 + A.share, A.nt);
    for (int t = t0; t < t1; ++t) {
        const int u = (t % A.ntx) * 16 + (wave & 1) * 8 + (lane & 7);
        const int v = (t / A.ntx) * 16 + (wave >> 1) * 8 + (lane >> 3);
        if (u >= A.Wf || v >= A.Hf) continue;
        const size_t pix = (size_t)v * A.Wf + u;
        bool acc = false;
        float J[6], r = 0.f;
        const float d = good ? depth_f[pix] : 0.f;
        if (depth_ok(d)) {
            // 1. back-projection
            const float xn = ((float)u - K[2]) / K[0], yn = ((float)v - K[3]) / K[1];
            const float pc[3] = {xn * d, yn * d, d};
            const float q[3] = {pc[0] - P[3], pc[1] - P[7], pc[2] - P[11]};
            float pw[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) pw[a] = (P[a] * q[0] + P[4 + a] * q[1]) + P[8 + a] * q[2];
            // 2. association
            float c[3];
#pragma unroll
            for (int rr = 0; rr < 3; ++rr)
                c[rr] = ((M[4 * rr] * pw[0] + M[4 * rr + 1] * pw[1]) + M[4 * rr + 2] * pw[2]) + M[4 * rr + 3];
            if (c[2] >= 0x1p-60f && c[2] < 0x1p60f) {
                const float iz = 1.0f / c[2];
                const float fu = floorf((Km[0] * c[0]) * iz + (Km[2] + 0.5f));
                const float fv = floorf((Km[1] * c[1]) * iz + (Km[3] + 0.5f));
                if (fu >= 0.f && fu < (float)A.Wm && fv >= 0.f && fv < (float)A.Hm) {
                    const int um = (int)fu, vm = (int)fv;
                    const size_t pm = (size_t)vm * A.Wm + um;
                    const float dm = depth_m[pm];
                    const float nm[3] = {normals_m[pm * 3], normals_m[pm * 3 + 1], normals_m[pm * 3 + 2]};
                    const bool nfin = isfinite(nm[0]) && isfinite(nm[1]) && isfinite(nm[2]);
                    const bool nzero = nm[0] == 0.f && nm[1] == 0.f && nm[2] == 0.f;
                    if (dm > 0.f && nfin && !nzero) {
                        // 3. model vertex (V8's ray)
                        const float dcx = (fu - Km[2]) / Km[0], dcy = (fv - Km[3]) / Km[1];
                        float e[3];
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            const float o = -((M[a] * M[3] + M[4 + a] * M[7]) + M[8 + a] * M[11]);
                            const float dw = (M[a] * dcx + M[4 + a] * dcy) + M[8 + a];
                            e[a] = pw[a] - (o + dm * dw);
                        }
                        // 4. distance gate
                        acc = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= A.dist2;
                        // 5. normal gate
                        if (acc && A.cos2 >= 0.f) {
                            acc = false;
                            if (u + 1 < A.Wf && v + 1 < A.Hf) {
                                const float dr = depth_f[pix + 1], dd = depth_f[pix + A.Wf];
                                if (depth_ok(dr) && depth_ok(dd)) {
                                    const float xr = ((float)(u + 1) - K[2]) / K[0];
                                    const float yd = ((float)(v + 1) - K[3]) / K[1];
                                    const float a3[3] = {xr * dr - pc[0], yn * dr - pc[1], dr - pc[2]};
                                    const float b3[3] = {xn * dd - pc[0], yd * dd - pc[1], dd - pc[2]};
                                    const float cr[3] = {b3[1] * a3[2] - b3[2] * a3[1], b3[2] * a3[0] - b3[0] * a3[2],
                                                         b3[0] * a3[1] - b3[1] * a3[0]};
                                    float cw[3];
#pragma unroll
                                    for (int a = 0; a < 3; ++a)
                                        cw[a] = (P[a] * cr[0] + P[4 + a] * cr[1]) + P[8 + a] * cr[2];
                                    const float dotr = (cw[0] * nm[0] + cw[1] * nm[1]) + cw[2] * nm[2];
                                    // bv x a points towards the camera iff fx fy > 0: a mirrored
                                    // frame (one focal length negative) turns it round
                                    const bool flip = (K[0] < 0.f) != (K[1] < 0.f);
                                    const float dotv = flip ? -dotr : dotr;
                                    const float cc = (cw[0] * cw[0] + cw[1] * cw[1]) + cw[2] * cw[2];
                                    acc = dotv > 0.f && dotv * dotv >= A.cos2 * cc;
                                }
                            }
                        }
                        // 6. row
                        r = (nm[0] * e[0] + nm[1] * e[1]) + nm[2] * e[2];
                        J[0] = pw[1] * nm[2] - pw[2] * nm[1];
                        J[1] = pw[2] * nm[0] - pw[0] * nm[2];
                        J[2] = pw[0] * nm[1] - pw[1] * nm[0];
                        J[3] = nm[0];
                        J[4] = nm[1];
                        J[5] = nm[2];
                    }
                }
            }
        }
        if (A.mask) A.mask[(size_t)view * A.Hf * A.Wf + pix] = acc ? 1 : 0;
        if (acc) {
            double Jd[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) Jd[i] = (double)J[i];
            const double rd = (double)r;
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) s[k++] += Jd[i] * Jd[j];
#pragma unroll
            for (int i = 0; i < 6; ++i) s[21 + i] += Jd[i] * rd;
            s[27] += rd * rd;
            s[28] += 1.0;
        }
    }

    // lane 0 of each wave: a fixed binary tree over the lanes
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
        double x = s[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0) red[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        const int k = threadIdx.x;
        A.partials[((size_t)view * gridDim.x + blockIdx.x) * kSums + k] =
            ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

struct SolveArgs {
    const double* partials;   // [B][P][29]
    int P;
    int iter, n_iters;        // n_iters 0: sums only (sfmhip_icp_normal_equations)
    double min_pairs;
    float* pose;              // [B][12] f32: read at iter 0, written after every good solve
    const float* pose_m;
    const float* Kf;
    const float* Km;
    double* pose64;           // [B][12] the f64 pose carried across iterations
    int* state;               // [B] 0 tracking, 1 lost, 2 skipped view
    double* sums;             // sums-only output [B][29]
    double* log;              // nullable [B][n_iters][36]
};

// A delta = -g by LDL^T without pivoting; false when a pivot is not above tol
__device__ bool solve6(const double* S, double tol, double* delta) {
    double A[6][6], L[6][6], D[6];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = S[k++];
    for (int j = 0; j < 6; ++j) {
        double dj = A[j][j];
        for (int m = 0; m < j; ++m) dj -= (L[j][m] * L[j][m]) * D[m];
        if (!(dj > tol)) return false;
        D[j] = dj;
        for (int i = j + 1; i < 6; ++i) {
            double x = A[i][j];
            for (int m = 0; m < j; ++m) x -= (L[i][m] * L[j][m]) * D[m];
            L[i][j] = x / dj;
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double x = -S[21 + i];
        for (int m = 0; m < i; ++m) x -= L[i][m] * y[m];
        y[i] = x;
    }
    for (int i = 5; i >= 0; --i) {
        double x = y[i] / D[i];
        for (int m = i + 1; m < 6; ++m) x -= L[m][i] * delta[m];
        delta[i] = x;
    }
    return true;
}

__global__ __launch_bounds__(kSolveThreads) void icp_solve_kernel(SolveArgs S) {
    __shared__ double sm[kSums];
    __shared__ double runs[kRuns][32];
    const int view = blockIdx.x, lane = threadIdx.x;
    const int st0 = S.iter > 0 ? S.state[view] : 0;
    if (st0 != 0) {   // lost earlier: a no-op, the record carries zero sums and the status
        if (S.log && lane < kLog)
            S.log[((size_t)view * S.n_iters + S.iter) * kLog + lane] = lane == kLog - 1 ? (double)st0 : 0.0;
        return;
    }
    {   // the view's partials: kRuns runs of consecutive ones, each in order, then the runs in order
        const int run = lane >> 5, k = lane & 31;
        const int len = (S.P + kRuns - 1) / kRuns;
        const int p0 = run * len, p1 = min(p0 + len, S.P);
        double x = 0.0;
        if (k < kSums) {
            const double* __restrict__ src = S.partials + (size_t)view * S.P * kSums + k;
#pragma unroll 4
            for (int p = p0; p < p1; ++p) x += src[(size_t)p * kSums];
        }
        runs[run][k] = x;
    }
    __syncthreads();
    if (lane < kSums) {
        double x = runs[0][lane];
        for (int r = 1; r < kRuns; ++r) x += runs[r][lane];
        sm[lane] = x;
        if (S.n_iters == 0) S.sums[(size_t)view * kSums + lane] = x;
    }
    if (S.n_iters == 0) return;
    __syncthreads();
    if (lane != 0) return;

    double T[12];
    if (S.iter == 0) {
        for (int q = 0; q < 12; ++q) T[q] = (double)S.pose[view * 12 + q];
    } else {
        for (int q = 0; q < 12; ++q) T[q] = S.pose64[view * 12 + q];
    }
    int status = 0;
    if (S.iter == 0) {
        float P[12], M[12], K[4], Km[4];
        if (!load_cams(S.pose, S.pose_m, S.Kf, S.Km, view, P, M, K, Km)) status = 2;
    }
    double delta[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (status == 0) {
        const double tr = ((((sm[0] + sm[6]) + sm[11]) + sm[15]) + sm[18]) + sm[20];
        if (sm[28] < S.min_pairs || !solve6(sm, 1e-12 * tr, delta)) {
            status = 1;
            for (int i = 0; i < 6; ++i) delta[i] = 0.0;
        }
    }
    if (status == 0) {
        // dR = Rodrigues(omega); R' = R dR^T; t' = t - R' v
        const double w0 = delta[0], w1 = delta[1], w2 = delta[2];
        const double th = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
        double dR[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        if (th > 0.0) {
            const double k[3] = {w0 / th, w1 / th, w2 / th};
            const double c = cos(th), sn = sin(th), C = 1.0 - c;
            const double kx[3][3] = {{0.0, -k[2], k[1]}, {k[2], 0.0, -k[0]}, {-k[1], k[0], 0.0}};
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) dR[i][j] = ((i == j ? c : 0.0) + C * (k[i] * k[j])) + sn * kx[i][j];
        }
        double Rn[3][3];
        for (int r = 0; r < 3; ++r)
            for (int a = 0; a < 3; ++a)
                Rn[r][a] = (T[4 * r] * dR[a][0] + T[4 * r + 1] * dR[a][1]) + T[4 * r + 2] * dR[a][2];
        for (int r = 0; r < 3; ++r) {
            const double tn = T[4 * r + 3] - ((Rn[r][0] * delta[3] + Rn[r][1] * delta[4]) + Rn[r][2] * delta[5]);
            for (int a = 0; a < 3; ++a) T[4 * r + a] = Rn[r][a];
            T[4 * r + 3] = tn;
        }
        for (int q = 0; q < 12; ++q) {
            S.pose64[view * 12 + q] = T[q];
            S.pose[view * 12 + q] = (float)T[q];
        }
    }
    S.state[view] = status;
    if (S.log) {
        double* rec = S.log + ((size_t)view * S.n_iters + S.iter) * kLog;
        for (int k = 0; k < kSums; ++k) rec[k] = sm[k];
        for (int i = 0; i < 6; ++i) rec[kSums + i] = delta[i];
        rec[kLog - 1] = (double)status;
    }
}

struct Plan {
    IcpArgs a;
    int P;
};

int make_plan(const char* fn, const float* depth_f, const float* Kf, const float* pose, int B, int Hf, int Wf,
              const float* depth_m, const float* normals_m, const float* pose_m, const float* Km, int Hm, int Wm,
              float dist2, float cos2, Plan& pl) {
    SFMHIP_REQUIRE(B >= 0 && Hf >= 0 && Wf >= 0 && Hm >= 0 && Wm >= 0, "%s: bad shape (%d; %d,%d; %d,%d)", fn, B, Hf, Wf,
                   Hm, Wm);
    SFMHIP_REQUIRE(B <= 65535 && Hf < (1 << 20) && Wf < (1 << 20) && Hm < (1 << 20) && Wm < (1 << 20),
                   "%s: too many views or pixels", fn);
    SFMHIP_REQUIRE((int64_t)Hf * Wf < (int64_t)INT_MAX && (int64_t)Hm * Wm < (int64_t)INT_MAX,
                   "%s: an image must hold fewer than 2^31 pixels", fn);
    SFMHIP_REQUIRE(dist2 > 0.f, "%s: dist2 must be > 0", fn);   // a NaN fails
    SFMHIP_REQUIRE(!(cos2 >= 1.f) && cos2 == cos2, "%s: cos2 must be below 1 (negative: no normal gate)", fn);
    IcpArgs& a = pl.a;
    a.depth_f = depth_f;
    a.Kf = Kf;
    a.pose = pose;
    a.depth_m = depth_m;
    a.normals_m = normals_m;
    a.pose_m = pose_m;
    a.Km = Km;
    a.Hf = Hf;
    a.Wf = Wf;
    a.Hm = Hm;
    a.Wm = Wm;
    a.ntx = ceil_div(Wf, 16);
    a.nt = a.ntx * ceil_div(Hf, 16);
    a.share = std::max(kShareMin, ceil_div(a.nt, kPartialsMax));
    a.dist2 = dist2;
    a.cos2 = cos2;
    a.state = nullptr;
    a.partials = nullptr;
    a.mask = nullptr;
    pl.P = ceil_div(a.nt, a.share);
    return SFMHIP_OK;
}

int check_pointers(const char* fn, const Plan& pl) {
    const IcpArgs& a = pl.a;
    SFMHIP_REQUIRE(a.depth_f && a.Kf && a.pose && a.pose_m && a.Km, "%s: null pointer", fn);
    SFMHIP_REQUIRE((a.depth_m && a.normals_m) || a.Hm == 0 || a.Wm == 0, "%s: null pointer (model maps)", fn);
    return SFMHIP_OK;
}

}  // namespace
}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_icp_normal_equations(const float* depth_f, const float* Kf, const float* pose, int B, int Hf,
                                           int Wf, const float* depth_m, const float* normals_m, const float* pose_m,
                                           const float* Km, int Hm, int Wm, float dist2, float cos2, double* sums,
                                           uint8_t* mask, void* stream) {
    const char* fn = "sfmhip_icp_normal_equations";
    Plan pl;
    int rc = make_plan(fn, depth_f, Kf, pose, B, Hf, Wf, depth_m, normals_m, pose_m, Km, Hm, Wm, dist2, cos2, pl);
    if (rc != SFMHIP_OK) return rc;
    if (B == 0 || Hf == 0 || Wf == 0) return SFMHIP_OK;
    if ((rc = check_pointers(fn, pl)) != SFMHIP_OK) return rc;
    SFMHIP_REQUIRE(sums, "%s: null pointer (sums)", fn);
    hipStream_t st = as_stream(stream);
    void* sc = nullptr;
    const hipError_t e = scratch_alloc(&sc, (size_t)B * pl.P * kSums * sizeof(double), st);
    if (e != hipSuccess) {
        set_error("%s: scratch: %s", fn, hipGetErrorString(e));
        return SFMHIP_E_HIP;
    }
    pl.a.partials = static_cast<double*>(sc);
    pl.a.mask = mask;
    hipLaunchKernelGGL(icp_reduce_kernel, dim3(pl.P, B), dim3(256), 0, st, pl.a);
    rc = check_launch("icp_reduce_kernel");
    if (rc == SFMHIP_OK) {
        SolveArgs S = {};
        S.partials = pl.a.partials;
        S.P = pl.P;
        S.sums = sums;
        hipLaunchKernelGGL(icp_solve_kernel, dim3(B), dim3(kSolveThreads), 0, st, S);
        rc = check_launch("icp_solve_kernel");
    }
    scratch_free(sc, st);
    return rc;
}

extern "C" int sfmhip_icp_track(const float* depth_f, const float* Kf, int B, int Hf, int Wf, const float* depth_m,
                                const float* normals_m, const float* pose_m, const float* Km, int Hm, int Wm,
                                float dist2, float cos2, int n_iters, int min_pairs, float* pose_inout, double* log,
                                void* stream) {
    const char* fn = "sfmhip_icp_track";
    Plan pl;
    int rc = make_plan(fn, depth_f, Kf, pose_inout, B, Hf, Wf, depth_m, normals_m, pose_m, Km, Hm, Wm, dist2, cos2, pl);
    if (rc != SFMHIP_OK) return rc;
    SFMHIP_REQUIRE(n_iters >= 0 && n_iters <= 65536, "%s: n_iters must be in [0, 65536], got %d", fn, n_iters);
    SFMHIP_REQUIRE(min_pairs >= 6, "%s: min_pairs must be at least 6, got %d", fn, min_pairs);
    if (B == 0 || Hf == 0 || Wf == 0 || n_iters == 0) return SFMHIP_OK;
    if ((rc = check_pointers(fn, pl)) != SFMHIP_OK) return rc;
    hipStream_t st = as_stream(stream);
    // partials [B][P][29] f64, pose64 [B][12] f64, state [B] i32
    const size_t n_part = (size_t)B * pl.P * kSums, n_pose = (size_t)B * 12;
    void* sc = nullptr;
    const hipError_t e = scratch_alloc(&sc, (n_part + n_pose) * sizeof(double) + (size_t)B * sizeof(int), st);
    if (e != hipSuccess) {
        set_error("%s: scratch: %s", fn, hipGetErrorString(e));
        return SFMHIP_E_HIP;
    }
    double* partials = static_cast<double*>(sc);
    double* pose64 = partials + n_part;
    int* state = reinterpret_cast<int*>(pose64 + n_pose);
    pl.a.partials = partials;
    SolveArgs S = {};
    S.partials = partials;
    S.P = pl.P;
    S.n_iters = n_iters;
    S.min_pairs = (double)min_pairs;
    S.pose = pose_inout;
    S.pose_m = pose_m;
    S.Kf = Kf;
    S.Km = Km;
    S.pose64 = pose64;
    S.state = state;
    S.log = log;
    for (int it = 0; it < n_iters && rc == SFMHIP_OK; ++it) {
        pl.a.state = it > 0 ? state : nullptr;   // written by the first solve
        hipLaunchKernelGGL(icp_reduce_kernel, dim3(pl.P, B), dim3(256), 0, st, pl.a);
        rc = check_launch("icp_reduce_kernel");
        if (rc != SFMHIP_OK) break;
        S.iter = it;
        hipLaunchKernelGGL(icp_solve_kernel, dim3(B), dim3(kSolveThreads), 0, st, S);
        rc = check_launch("icp_solve_kernel");
    }
    scratch_free(sc, st);
    return rc;
}
