// plan.hip — V13: planning the dense stage from a sparse reconstruction (semantics: include/sfmhip.h
// V13, restated in numpy by tests/plan_ref.py).  Plain launches on the caller's stream; every sum is
// an integer, every f64 step one IEEE operation in the order written (-ffp-contract=off), so every
// output is defined to the bit and independent of the launch geometry.
//   obs_depth   one lane per observation: row 2 of its camera's pose times its point, four f64
//               steps, rounded to f32; +inf where that is not a finite positive depth.
//   pair counts a workgroup takes chunks of 256 consecutive tracks.  A track of length L has
//               L (L - 1) / 2 camera pairs: the chunk's pair counts are scanned in LDS and the
//               flattened pairs dealt out evenly, lane t walks pairs [t per, (t + 1) per) (one
//               binary search and one decode at its first pair, then a walk), so a track seen by
//               every view is spread over the whole workgroup.  The counts go to the upper
//               triangles of `shared` and `good`: privatised in LDS per workgroup (one workgroup
//               per CU, grid-stride over the chunks, one flush of the non-zero entries at the end)
//               while both triangles fit beside the chunk arrays (V <= 200), else integer atomics
//               straight to global memory.  A last kernel mirrors the upper triangle.
//   select      one workgroup per segment, four most-significant-digit passes of 8 bits over the
//               radix keys: a 256-bin LDS histogram per rank of the elements that match the
//               rank's prefix so far, one lane per rank walks it to the digit that holds the rank.
//               The segment is never sorted and nothing returns to the host between passes.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace sfmhip {
namespace {

constexpr int kChunk = 256;                 // tracks per chunk = lanes per workgroup of the pair kernel
constexpr int kLdsBytes = 160 * 1024;       // LDS of a gfx950 workgroup
constexpr int kPairFixedLds = kChunk * 8 + kChunk * 4 + 64;   // scan, track lengths, slack
constexpr int kMaxViews = 32767;
constexpr int kSelWg = 1024;
constexpr int kMaxRanks = 8;

__global__ __launch_bounds__(256) void obs_depth_kernel(const double* __restrict__ poses, int V,
                                                        const double* __restrict__ X, int64_t N,
                                                        const int32_t* __restrict__ obs_cam,
                                                        const int32_t* __restrict__ obs_pt, int64_t M,
                                                        float* __restrict__ z) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int c = obs_cam[m], p = obs_pt[m];
    float out = INFINITY;
    if (c >= 0 && c < V && p >= 0 && p < N) {   // the entry point's contract; never read out of bounds
        const double* P = poses + (size_t)c * 12 + 8;
        const double* x = X + (size_t)p * 3;
        const double d = ((P[0] * x[0] + P[1] * x[1]) + P[2] * x[2]) + P[3];
        const float f = (float)d;
        if (f > 0.0f && f < INFINITY) out = f;   // a NaN fails both
    }
    z[m] = out;
}

// index of (lo, hi), lo < hi, in the row-major upper triangle without the diagonal
__device__ __forceinline__ int tri_index(int lo, int hi, int V) { return lo * (2 * V - lo - 1) / 2 + (hi - lo - 1); }

template <bool kLds>
__global__ __launch_bounds__(kChunk) void pair_counts_kernel(const double* __restrict__ centres, int V,
                                                             const double* __restrict__ X, int64_t N,
                                                             const int32_t* __restrict__ obs_cam, int64_t M,
                                                             const int64_t* __restrict__ pt_off, double c2_lo,
                                                             double c2_hi, int32_t* __restrict__ shared,
                                                             int32_t* __restrict__ good, int64_t n_chunks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* s_scan = reinterpret_cast<uint64_t*>(smem);                       // [kChunk] inclusive pair counts
    int* s_len = reinterpret_cast<int*>(smem + kChunk * 8);                     // [kChunk] track lengths (0: skipped)
    int* s_shared = reinterpret_cast<int*>(smem + kPairFixedLds);               // [V (V - 1) / 2]
    const int tri = V * (V - 1) / 2;
    int* s_good = s_shared + tri;
    const int t = threadIdx.x;
    if (kLds) {
        for (int e = t; e < 2 * tri; e += kChunk) s_shared[e] = 0;
    }
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        __syncthreads();   // the previous chunk's walk is over (and the zeroing above)
        const int64_t tr = chunk * kChunk + t;
        int L = 0;
        if (tr < N) {
            const int64_t a0 = pt_off[tr], a1 = pt_off[tr + 1];
            if (a0 >= 0 && a1 >= a0 && a1 <= M && a1 - a0 <= (int64_t)V) L = (int)(a1 - a0);   // else malformed: skipped
        }
        s_len[t] = L;
        s_scan[t] = L >= 2 ? (uint64_t)L * (uint64_t)(L - 1) / 2 : 0;
        __syncthreads();
        for (int d = 1; d < kChunk; d <<= 1) {
            const uint64_t v = t >= d ? s_scan[t - d] : 0;
            __syncthreads();
            s_scan[t] += v;
            __syncthreads();
        }
        const uint64_t total = s_scan[kChunk - 1];
        const uint64_t per = (total + kChunk - 1) / kChunk;
        const uint64_t q0 = min(total, (uint64_t)t * per), q1 = min(total, q0 + per);
        if (q0 >= q1) continue;
        int lo = 0, hi = kChunk - 1;   // the first track whose inclusive count exceeds q0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_scan[mid] > q0) hi = mid; else lo = mid + 1;
        }
        int k = lo;
        uint64_t rem = q0 - (k ? s_scan[k - 1] : 0);
        L = s_len[k];
        int i = 0;
        while (rem >= (uint64_t)(L - 1 - i)) {
            rem -= (uint64_t)(L - 1 - i);
            ++i;
        }
        int j = i + 1 + (int)rem;
        int64_t o0 = pt_off[chunk * kChunk + k];
        const double* xp = X + (size_t)(chunk * kChunk + k) * 3;
        double x0 = xp[0], x1 = xp[1], x2 = xp[2];
        int a = -1;
        double ra0 = 0, ra1 = 0, ra2 = 0, na = 0;
        for (uint64_t q = q0; q < q1; ++q) {
            if (a < 0) {   // a new first camera of the pair
                a = obs_cam[o0 + i];
                if (a >= 0 && a < V) {
                    const double* ca = centres + (size_t)a * 3;
                    ra0 = ca[0] - x0; ra1 = ca[1] - x1; ra2 = ca[2] - x2;
                    na = (ra0 * ra0 + ra1 * ra1) + ra2 * ra2;
                }
            }
            const int b = obs_cam[o0 + j];
            if (a >= 0 && a < V && b >= 0 && b < V && a != b) {
                const double* cb = centres + (size_t)b * 3;
                const double rb0 = cb[0] - x0, rb1 = cb[1] - x1, rb2 = cb[2] - x2;
                const double d = (ra0 * rb0 + ra1 * rb1) + ra2 * rb2;
                const double n = na * ((rb0 * rb0 + rb1 * rb1) + rb2 * rb2);
                const double dd = d * d;
                const bool is_good = d > 0.0 && n < (double)INFINITY && dd >= c2_lo * n && dd <= c2_hi * n;
                const int r = min(a, b), c = max(a, b);
                if (kLds) {
                    const int e = tri_index(r, c, V);
                    atomicAdd(&s_shared[e], 1);
                    if (is_good) atomicAdd(&s_good[e], 1);
                } else {
                    const size_t e = (size_t)r * V + c;
                    atomicAdd(&shared[e], 1);
                    if (is_good) atomicAdd(&good[e], 1);
                }
            }
            if (++j == L) {
                ++i;
                j = i + 1;
                a = -1;
                if (i >= L - 1 && q + 1 < q1) {   // the track is done and pairs remain: the next one with a pair
                    do { ++k; } while (s_len[k] < 2);
                    L = s_len[k];
                    i = 0;
                    j = 1;
                    o0 = pt_off[chunk * kChunk + k];
                    xp = X + (size_t)(chunk * kChunk + k) * 3;
                    x0 = xp[0]; x1 = xp[1]; x2 = xp[2];
                }
            }
        }
    }
    if (kLds) {
        __syncthreads();
        for (int e = t; e < V * V; e += kChunk) {
            const int r = e / V, c = e % V;
            if (r < c) {
                const int q = tri_index(r, c, V);
                const int s = s_shared[q], g = s_good[q];
                if (s) atomicAdd(&shared[e], s);
                if (g) atomicAdd(&good[e], g);
            }
        }
    }
}

__global__ __launch_bounds__(256) void mirror_kernel(int32_t* __restrict__ shared, int32_t* __restrict__ good, int V) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)V * V) return;
    const int r = (int)(e / V), c = (int)(e % V);
    if (r > c) {
        shared[e] = shared[(size_t)c * V + r];
        good[e] = good[(size_t)c * V + r];
    }
}

__device__ __forceinline__ uint32_t radix_key(uint32_t bits) { return bits & 0x80000000u ? ~bits : bits ^ 0x80000000u; }

__global__ __launch_bounds__(kSelWg) void segmented_select_kernel(const uint32_t* __restrict__ values, int64_t M,
                                                                  const int64_t* __restrict__ seg_off,
                                                                  const int64_t* __restrict__ ranks, int R,
                                                                  uint32_t* __restrict__ out) {
    __shared__ unsigned hist[kMaxRanks][256];
    __shared__ uint32_t s_prefix[kMaxRanks];   // the key's digits found so far (the bits above the pass's digit)
    __shared__ int64_t s_rank[kMaxRanks];      // the rank among the elements that share the prefix; -1: none
    const int64_t s = blockIdx.x;
    const int t = threadIdx.x;
    int64_t o0 = seg_off[s], o1 = seg_off[s + 1];
    if (o0 < 0 || o1 < o0 || o1 > M) o0 = o1 = 0;   // malformed: an empty segment
    const int64_t n = o1 - o0;
    if (t < R) {
        const int64_t r = ranks[s * R + t];
        s_rank[t] = r >= 0 && r < n ? r : -1;
        s_prefix[t] = 0;
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int e = t; e < R * 256; e += kSelWg) (&hist[0][0])[e] = 0;
        __syncthreads();
        const uint32_t mask = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
        for (int64_t m = o0 + t; m < o1; m += kSelWg) {
            const uint32_t key = radix_key(values[m]);
            for (int r = 0; r < R; ++r)
                if (s_rank[r] >= 0 && (key & mask) == s_prefix[r]) atomicAdd(&hist[r][(key >> shift) & 255], 1u);
        }
        __syncthreads();
        if (t < R && s_rank[t] >= 0) {
            int64_t left = s_rank[t];
            int d = 0;
            while (d < 255 && left >= (int64_t)hist[t][d]) {
                left -= hist[t][d];
                ++d;
            }
            s_rank[t] = left;
            s_prefix[t] |= (uint32_t)d << shift;
        }
        __syncthreads();
    }
    if (t < R) {
        const uint32_t key = s_prefix[t];
        out[s * R + t] = s_rank[t] < 0 ? 0x7FC00000u : (key & 0x80000000u ? key ^ 0x80000000u : ~key);
    }
}

}  // namespace
}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_obs_depth(const double* poses, int V, const double* X, int64_t N, const int32_t* obs_cam,
                                const int32_t* obs_pt, int64_t M, float* z, void* stream) {
    const char* fn = "sfmhip_obs_depth";
    SFMHIP_REQUIRE(V >= 0 && N >= 0 && M >= 0, "%s: bad shape (V %d, N %lld, M %lld)", fn, V, (long long)N, (long long)M);
    SFMHIP_REQUIRE(M <= ((int64_t)1 << 38), "%s: at most 2^38 observations per call", fn);
    if (M == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(obs_cam && obs_pt && z, "%s: null pointer", fn);
    SFMHIP_REQUIRE((V == 0 || poses) && (N == 0 || X), "%s: null pointer", fn);
    hipLaunchKernelGGL(obs_depth_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, as_stream(stream), poses, V, X,
                       N, obs_cam, obs_pt, M, z);
    return check_launch("obs_depth_kernel");
}

extern "C" int sfmhip_view_pair_counts(const double* centres, int V, const double* X, int64_t N, const int32_t* obs_cam,
                                       int64_t M, const int64_t* pt_off, double c2_lo, double c2_hi, int32_t* shared,
                                       int32_t* good, void* stream) {
    const char* fn = "sfmhip_view_pair_counts";
    SFMHIP_REQUIRE(V >= 0 && N >= 0 && M >= 0, "%s: bad shape (V %d, N %lld, M %lld)", fn, V, (long long)N, (long long)M);
    SFMHIP_REQUIRE(V <= kMaxViews, "%s: at most %d views, got %d", fn, kMaxViews, V);
    SFMHIP_REQUIRE(c2_lo >= 0.0 && c2_lo <= c2_hi && c2_hi <= 1.0, "%s: need 0 <= c2_lo <= c2_hi <= 1, got %g / %g", fn,
                   c2_lo, c2_hi);
    if (V == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(shared && good, "%s: null pointer", fn);
    hipStream_t st = as_stream(stream);
    const size_t bytes = (size_t)V * V * sizeof(int32_t);
    if (hipMemsetAsync(shared, 0, bytes, st) != hipSuccess || hipMemsetAsync(good, 0, bytes, st) != hipSuccess) {
        set_error("%s: %s", fn, hipGetErrorString(hipGetLastError()));
        return SFMHIP_E_HIP;
    }
    if (M == 0 || N == 0 || V == 1) return SFMHIP_OK;   // zeros, no launch
    SFMHIP_REQUIRE(centres && X && obs_cam && pt_off, "%s: null pointer", fn);
    const int64_t n_chunks = (N + kChunk - 1) / kChunk;
    const int64_t lds = (int64_t)kPairFixedLds + 4ll * V * (V - 1);
    const int n_cu = cu_count();
    if (lds <= kLdsBytes && knobs().plan_global == 0) {
        auto kern = pair_counts_kernel<true>;
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3((unsigned)std::min<int64_t>(n_chunks, n_cu)), dim3(kChunk), (size_t)lds, st, centres,
                           V, X, N, obs_cam, M, pt_off, c2_lo, c2_hi, shared, good, n_chunks);
    } else {
        hipLaunchKernelGGL(pair_counts_kernel<false>, dim3((unsigned)std::min<int64_t>(n_chunks, 16ll * n_cu)),
                           dim3(kChunk), (size_t)kPairFixedLds, st, centres, V, X, N, obs_cam, M, pt_off, c2_lo, c2_hi,
                           shared, good, n_chunks);
    }
    int rc = check_launch("pair_counts_kernel");
    if (rc != SFMHIP_OK) return rc;
    hipLaunchKernelGGL(mirror_kernel, dim3(ceil_div((int64_t)V * V, 256)), dim3(256), 0, st, shared, good, V);
    return check_launch("mirror_kernel");
}

extern "C" int sfmhip_segmented_select(const float* values, int64_t M, const int64_t* seg_off, int64_t S,
                                       const int64_t* ranks, int R, float* out, void* stream) {
    const char* fn = "sfmhip_segmented_select";
    SFMHIP_REQUIRE(M >= 0 && S >= 0 && R >= 0, "%s: bad shape (M %lld, S %lld, R %d)", fn, (long long)M, (long long)S, R);
    SFMHIP_REQUIRE(R <= kMaxRanks, "%s: at most %d ranks per segment, got %d", fn, kMaxRanks, R);
    SFMHIP_REQUIRE(S <= 0x7FFFFFFF, "%s: at most 2^31 - 1 segments per call", fn);
    if (S == 0 || R == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(seg_off && ranks && out && (M == 0 || values), "%s: null pointer", fn);
    hipLaunchKernelGGL(segmented_select_kernel, dim3((unsigned)S), dim3(kSelWg), 0, as_stream(stream),
                       reinterpret_cast<const uint32_t*>(values), M, seg_off, ranks, R, reinterpret_cast<uint32_t*>(out));
    return check_launch("segmented_select_kernel");
}
