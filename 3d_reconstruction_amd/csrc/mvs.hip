// mvs.hip — V10: dense depth from posed grey images by census plane-sweep stereo (semantics:
// include/sfmhip.h V10, restated in numpy by tests/mvs_ref.py).  Plain launches on the caller's
// stream, no atomics:
//   census   one lane per pixel, a workgroup = a 16 x 16 tile whose 22 x 22 neighbourhood is
//            staged in LDS (0 outside the image: never brighter than a centre).
//   prepare  one lane per (reference, source) of a call: the skip rule, the relative pose in
//            f64 rounded to f32 and the source intrinsics, as one 16-float record that the
//            sweep and the filter read from wave-uniform addresses.
//   sweep    a workgroup takes a 32 x 16 reference tile and loops over the planes: per plane
//            the lanes write the raw cost of the (32 + 2a) x (16 + 2a) tile-plus-halo cells to
//            LDS (the low half of a word; the visible-source count in the high half), box-sum it
//            separably (rows, then columns: both halves at once, neither can carry), and
//            every lane folds its pixel's aggregated cost into registers: the four smallest
//            (cost << 16 | plane) keys, and the costs of the winner's two neighbours (the
//            previous plane's cost is carried, the next one patched).  Two barriers per plane.
//   filter   one lane per pixel: the reprojection of the sweep at the pixel's own depth.
// and, for the semi-global mode (steps 4a, 4b, 5' - 7'; tests/mvs_sgm_ref.py):
//   volume   the sweep's tile and sums, storing every plane's aggregated cost as u16, plane innermost.
//   sgm      one wave per scan line of one direction, four planes per lane, one launch per direction.
//   select   one lane per pixel: the sweep's winner, second and sub-plane depth from the summed paths.
// The projection is f32 with -ffp-contract=off, one IEEE step per operation: every output is
// bit-identical to the numpy form.
#include "common.h"
#include <climits>

namespace sfmhip {
namespace {

constexpr int kRec = 16;       // floats per record: 3 x 4 relative pose, fx, fy, cx + 0.5, cy + 0.5
constexpr int kMaxA = 3;
// the sweep's reference tile.  1936 x 1296, P = 128, S = 4, a = 2, ms per view (tools/bench_mvs.py):
// 16 x 16 (256 lanes, 1.56 cells per pixel) 4.99, 32 x 16 (512, 1.41) 4.65, 32 x 32 (1024, 1.27) 5.63
// (with a projection that branched around the census load, see project())
constexpr int kTileW = 32, kTileH = 16;
constexpr int kMaxS = 16;
constexpr int kMaxPenalty = 48;

__device__ __forceinline__ bool view_ok(const float* __restrict__ pose, const float* __restrict__ K) {
    bool good = true;
    for (int q = 0; q < 12; ++q) good = good && fabsf(pose[q]) < 0x1p60f;
    for (int q = 0; q < 4; ++q) good = good && fabsf(K[q]) < 0x1p60f;
    return good && K[0] != 0.f && K[1] != 0.f;
}

// record 0 of a reference: its fx, fy, cx, cy; record 1 + s: source s seen from the reference.
// meta: the view index of the record, or -1 (a reference or source that does not count).
__global__ __launch_bounds__(64) void mvs_prepare_kernel(const float* __restrict__ poses, const float* __restrict__ K,
                                                         int V, const int* __restrict__ refs,
                                                         const int* __restrict__ srcs, int R, int S,
                                                         float* __restrict__ tab, int* __restrict__ meta) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * (S + 1)) return;
    const int ri = idx / (S + 1), j = idx % (S + 1);
    float rec[kRec];
    for (int q = 0; q < kRec; ++q) rec[q] = 0.f;
    const int ref = refs[ri];
    int view = -1;
    if (ref >= 0 && ref < V && view_ok(poses + (size_t)ref * 12, K + (size_t)ref * 4)) {
        if (j == 0) {
            view = ref;
            for (int q = 0; q < 4; ++q) rec[q] = K[(size_t)ref * 4 + q];
        } else {
            const int s = srcs[(size_t)ri * S + (j - 1)];
            if (s >= 0 && s < V && view_ok(poses + (size_t)s * 12, K + (size_t)s * 4)) {
                view = s;
                const float* __restrict__ pr = poses + (size_t)ref * 12;
                const float* __restrict__ ps = poses + (size_t)s * 12;
                for (int i = 0; i < 3; ++i) {
                    double rr[3];
                    for (int c = 0; c < 3; ++c)
                        rr[c] = ((double)ps[4 * i] * (double)pr[4 * c] +
                                 (double)ps[4 * i + 1] * (double)pr[4 * c + 1]) +
                                (double)ps[4 * i + 2] * (double)pr[4 * c + 2];
                    const double t = (double)ps[4 * i + 3] -
                                     ((rr[0] * (double)pr[3] + rr[1] * (double)pr[7]) + rr[2] * (double)pr[11]);
                    for (int c = 0; c < 3; ++c) rec[4 * i + c] = (float)rr[c];
                    rec[4 * i + 3] = (float)t;
                }
                rec[12] = K[(size_t)s * 4];
                rec[13] = K[(size_t)s * 4 + 1];
                rec[14] = K[(size_t)s * 4 + 2] + 0.5f;
                rec[15] = K[(size_t)s * 4 + 3] + 0.5f;
            }
        }
    }
    for (int q = 0; q < kRec; ++q) tab[(size_t)idx * kRec + q] = rec[q];
    meta[idx] = view;
}

// V5's projection of the reference-camera point (X, Y, z) through a source record: whether it is
// visible, the pixel it lands on (pixel 0 when it is not) and its source-camera depth.  No branch:
// the sweep loads a census from every lane and selects afterwards (1936 x 1296, P = 128, S = 4:
// 4.65 -> 4.25 ms per view against skipping the load of the lanes that see nothing)
__device__ __forceinline__ bool project(const float* __restrict__ rec, float X, float Y, float z, int H, int W,
                                        size_t& pix, float& zc) {
    const float xc = ((rec[0] * X + rec[1] * Y) + rec[2] * z) + rec[3];
    const float yc = ((rec[4] * X + rec[5] * Y) + rec[6] * z) + rec[7];
    zc = ((rec[8] * X + rec[9] * Y) + rec[10] * z) + rec[11];
    const float iz = 1.0f / zc;
    const float fu = floorf((rec[12] * xc) * iz + rec[14]);
    const float fv = floorf((rec[13] * yc) * iz + rec[15]);
    const bool vis = zc >= 0x1p-60f && zc < 0x1p60f && fu >= 0.f && fu < (float)W && fv >= 0.f && fv < (float)H;
    pix = (size_t)(int)(vis ? fv : 0.f) * W + (int)(vis ? fu : 0.f);
    return vis;
}

__global__ __launch_bounds__(256) void mvs_census_kernel(const uint8_t* __restrict__ img, int H, int W, int ntx,
                                                         uint64_t* __restrict__ cen) {
    __shared__ uint8_t t[22 * 22];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int u0 = (blockIdx.x % ntx) * 16, v0 = (blockIdx.x / ntx) * 16;
    const size_t base = (size_t)blockIdx.y * H * W;
    for (int cell = tid; cell < 22 * 22; cell += 256) {
        const int uu = u0 - 3 + cell % 22, vv = v0 - 3 + cell / 22;
        t[cell] = (uu >= 0 && uu < W && vv >= 0 && vv < H) ? img[base + (size_t)vv * W + uu] : 0;
    }
    __syncthreads();
    const int u = u0 + tx, v = v0 + ty;
    if (u >= W || v >= H) return;
    const unsigned c = t[(ty + 3) * 22 + tx + 3];
    uint64_t bits = 0;
    int i = 0;
#pragma unroll
    for (int dy = 0; dy < 7; ++dy)
#pragma unroll
        for (int dx = 0; dx < 7; ++dx) {
            if (dy == 3 && dx == 3) continue;
            bits |= (uint64_t)(t[(ty + dy) * 22 + tx + dx] > c) << i;
            ++i;
        }
    cen[base + (size_t)v * W + u] = bits;
}

struct SweepArgs {
    const uint64_t* cen;
    const float* tab;
    const int* meta;
    const float* planes;
    int H, W, S, P, a, penalty, uniq, min_views, ntx;
    float* depth;
    int* kstar;    // nullable, like best, second and nv
    int* best;
    int* second;
    uint8_t* nv;
};

template <int TW, int TH>
__global__ __launch_bounds__(TW * TH) void mvs_sweep_kernel(SweepArgs A) {
    constexpr int NT = TW * TH;
    static_assert((TW + 2 * kMaxA) * (TH + 2 * kMaxA) <= 2 * NT, "two cells per lane");
    __shared__ int raw[(TW + 2 * kMaxA) * (TH + 2 * kMaxA)];   // per cell: raw cost | visible sources << 16
    __shared__ int hs[(TH + 2 * kMaxA) * TW];                  // row sums of the TW columns of the tile
    const int tid = threadIdx.x, tx = tid % TW, ty = tid / TW;
    const int H = A.H, W = A.W, S = A.S, P = A.P, a = A.a;
    const int u0 = (blockIdx.x % A.ntx) * TW, v0 = (blockIdx.x / A.ntx) * TH;
    const int u = u0 + tx, v = v0 + ty;
    const bool inimg = u < W && v < H;
    const size_t HW = (size_t)H * W;
    const size_t opix = (size_t)blockIdx.y * HW + (size_t)v * W + u;
    const int* __restrict__ meta = A.meta + (size_t)blockIdx.y * (S + 1);
    const float* __restrict__ tab = A.tab + (size_t)blockIdx.y * (S + 1) * kRec;
    const float* __restrict__ planes = A.planes;
    const uint64_t* __restrict__ cen = A.cen;

    const int ref = meta[0];
    if (ref < 0) {   // the skip rule took the reference out: all-zero maps
        if (inimg) {
            A.depth[opix] = 0.f;
            if (A.kstar) A.kstar[opix] = 0;
            if (A.best) A.best[opix] = 0;
            if (A.second) A.second[opix] = 0;
            if (A.nv) A.nv[opix] = 0;
        }
        return;
    }
    const float fx = tab[0], fy = tab[1], cx = tab[2], cy = tab[3];
    const int T = TW + 2 * a, ncell = T * (TH + 2 * a), fill = A.penalty * S;

    // a lane's two cells of the tile-plus-halo: V8's ray and the reference census, once
    float dxr[2], dyr[2];
    uint64_t cr[2];
    bool live[2], inside[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cell = tid + NT * j;
        const int uu = u0 - a + cell % T, vv = v0 - a + cell / T;
        live[j] = cell < ncell;
        inside[j] = live[j] && uu >= 0 && uu < W && vv >= 0 && vv < H;
        dxr[j] = ((float)uu - cx) / fx;
        dyr[j] = ((float)vv - cy) / fy;
        cr[j] = inside[j] ? cen[(size_t)ref * HW + (size_t)vv * W + uu] : 0;
    }

    unsigned b0 = 0xffffffffu, b1 = 0xffffffffu, b2 = 0xffffffffu, b3 = 0xffffffffu;
    int kbest = -2, prev = 0, cm = 0, cp = 0, nvbest = 0;
    for (int k = 0; k < P; ++k) {
        const float z = planes[k];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!live[j]) continue;
            int val = fill;
            if (inside[j]) {
                const float X = dxr[j] * z, Y = dyr[j] * z;
                val = 0;
                for (int s = 0; s < S; ++s) {
                    int c = A.penalty;
                    const int src = meta[1 + s];
                    if (src >= 0) {
                        size_t pix;
                        float zc;
                        const bool vis = project(tab + (size_t)(1 + s) * kRec, X, Y, z, H, W, pix, zc);
                        const int ham = __popcll(cr[j] ^ cen[(size_t)src * HW + pix]) + (1 << 16);
                        c = vis ? ham : c;
                    }
                    val += c;
                }
            }
            raw[tid + NT * j] = val;
        }
        __syncthreads();
        for (int e = tid; e < (TH + 2 * a) * TW; e += NT) {
            const int* row = raw + (e / TW) * T + (e % TW);
            int x = row[0];
            for (int d = 1; d <= 2 * a; ++d) x += row[d];
            hs[e] = x;
        }
        const int nvc = raw[(ty + a) * T + tx + a] >> 16;
        __syncthreads();
        int tot = hs[ty * TW + tx];
        for (int d = 1; d <= 2 * a; ++d) tot += hs[(ty + d) * TW + tx];
        const int ag = tot & 0xffff;

        unsigned key = ((unsigned)ag << 16) | (unsigned)k;
        if (k == kbest + 1) cp = ag;
        if (key < b0) {
            cm = prev;
            cp = 0;
            kbest = k;
            nvbest = nvc;
        }
        prev = ag;
        unsigned t;
        t = min(b0, key); key = max(b0, key); b0 = t;
        t = min(b1, key); key = max(b1, key); b1 = t;
        t = min(b2, key); key = max(b2, key); b2 = t;
        b3 = min(b3, key);
    }
    if (!inimg) return;

    const int ks = kbest, best = (int)(b0 >> 16);
    int second = INT_MAX;
    {
        const unsigned cand[3] = {b3, b2, b1};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int kk = (int)(cand[i] & 0xffffu);
            if (cand[i] != 0xffffffffu && abs(kk - ks) >= 2) second = (int)(cand[i] >> 16);
        }
    }
    float depth = 0.f;
    if (ks > 0 && ks < P - 1 && nvbest >= A.min_views && 256ll * best <= (long long)A.uniq * second) {
        const float i0 = 1.0f / planes[ks], im = 1.0f / planes[ks - 1], ip = 1.0f / planes[ks + 1];
        const float c0 = (float)best, cmf = (float)cm, cpf = (float)cp;
        const float den = (cmf - c0) + (cpf - c0);
        const float off = den > 0.f ? (cmf - cpf) / (2.0f * den) : 0.f;
        const float step = off >= 0.f ? ip - i0 : i0 - im;
        depth = 1.0f / (i0 + off * step);
    }
    A.depth[opix] = depth;
    if (A.kstar) A.kstar[opix] = ks;
    if (A.best) A.best[opix] = best;
    if (A.second) A.second[opix] = second;
    if (A.nv) A.nv[opix] = (uint8_t)nvbest;
}

__global__ __launch_bounds__(256) void mvs_filter_kernel(const float* __restrict__ depth,
                                                         const float* __restrict__ tabs,
                                                         const int* __restrict__ metas, int H, int W, int S, int ntx,
                                                         float eps, int min_consistent, uint8_t* __restrict__ count,
                                                         float* __restrict__ filtered) {
    const int tid = threadIdx.x;
    const int u = (blockIdx.x % ntx) * 16 + (tid & 15), v = (blockIdx.x / ntx) * 16 + (tid >> 4);
    if (u >= W || v >= H) return;
    const size_t HW = (size_t)H * W;
    const size_t opix = (size_t)blockIdx.y * HW + (size_t)v * W + u;
    const int* __restrict__ meta = metas + (size_t)blockIdx.y * (S + 1);
    const float* __restrict__ tab = tabs + (size_t)blockIdx.y * (S + 1) * kRec;
    const int ref = meta[0];
    int cnt = 0;
    float d = 0.f;
    bool pos = false;
    if (ref >= 0) {
        d = depth[(size_t)ref * HW + (size_t)v * W + u];
        pos = d > 0.f;
    }
    if (pos) {
        const float dx = ((float)u - tab[2]) / tab[0], dy = ((float)v - tab[3]) / tab[1];
        const float X = dx * d, Y = dy * d;
        for (int s = 0; s < S; ++s) {
            const int src = meta[1 + s];
            if (src < 0) continue;
            size_t pix;
            float zc;
            if (project(tab + (size_t)(1 + s) * kRec, X, Y, d, H, W, pix, zc)) {
                const float ds = depth[(size_t)src * HW + pix];
                if (ds > 0.f && fabsf(ds - zc) <= eps * zc) ++cnt;
            }
        }
    }
    count[opix] = (uint8_t)cnt;
    filtered[opix] = (pos && cnt >= min_consistent) ? d : 0.f;
}

// ---- steps 4a, 4b and 5' - 7': the cost volume, semi-global path aggregation, selection --------

struct VolumeArgs {
    int H, W, S, P, a, penalty, ntx;
};

// The sweep's tile, halo and LDS row / column sums, with stores in place of the running state.
// VEC (P a multiple of 8 and vol 16-byte aligned, so every pixel's run is): a lane keeps its pixel's
// last eight planes packed in four registers, every eighth plane they go to an LDS stage, and every
// 32 planes four lanes write a pixel's 64 contiguous bytes (1936 x 1296, P = 128, ms per call: a
// 16-byte store per lane per eight planes 7.64, the stage 7.13, both before the change below).
// Any other P goes out plane by plane as u16.
// The pointers are kernel arguments of their own, not members of A: the stores to vol inside the
// plane loop must not be able to alias the records, or their reads stop being scalar loads
// (1936 x 1296, P = 128, S = 4: 7.14 -> 4.31 ms).
template <int TW, int TH, bool VEC>
__global__ __launch_bounds__(TW * TH) void mvs_volume_kernel(VolumeArgs A, const uint64_t* __restrict__ cen,
                                                             const float* __restrict__ tabs,
                                                             const int* __restrict__ metas,
                                                             const float* __restrict__ planes,
                                                             uint16_t* __restrict__ vol) {
    constexpr int NT = TW * TH;
    static_assert((TW + 2 * kMaxA) * (TH + 2 * kMaxA) <= 2 * NT, "two cells per lane");
    __shared__ int raw[(TW + 2 * kMaxA) * (TH + 2 * kMaxA)];
    __shared__ int hs[(TH + 2 * kMaxA) * TW];
    __shared__ uint4 stage[VEC ? NT * 4 : 1];   // VEC: 32 planes of every pixel of the tile, [pixel][group of 8]
    const int tid = threadIdx.x, tx = tid % TW, ty = tid / TW;
    const int H = A.H, W = A.W, S = A.S, P = A.P, a = A.a;
    const int u0 = (blockIdx.x % A.ntx) * TW, v0 = (blockIdx.x / A.ntx) * TH;
    const int u = u0 + tx, v = v0 + ty;
    const bool inimg = u < W && v < H;
    const size_t HW = (size_t)H * W;
    vol += (size_t)blockIdx.y * HW * P;   // the reference's slice
    uint16_t* __restrict__ out = vol + ((size_t)v * W + u) * P;   // used if inimg
    const int* __restrict__ meta = metas + (size_t)blockIdx.y * (S + 1);
    const float* __restrict__ tab = tabs + (size_t)blockIdx.y * (S + 1) * kRec;

    const int ref = meta[0];
    if (ref < 0) {   // the skip rule took the reference out: an all-zero slice
        if (inimg)
            for (int k = 0; k < P; ++k) out[k] = 0;
        return;
    }
    const float fx = tab[0], fy = tab[1], cx = tab[2], cy = tab[3];
    const int T = TW + 2 * a, ncell = T * (TH + 2 * a), fill = A.penalty * S;

    float dxr[2], dyr[2];
    uint64_t cr[2];
    bool live[2], inside[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cell = tid + NT * j;
        const int uu = u0 - a + cell % T, vv = v0 - a + cell / T;
        live[j] = cell < ncell;
        inside[j] = live[j] && uu >= 0 && uu < W && vv >= 0 && vv < H;
        dxr[j] = ((float)uu - cx) / fx;
        dyr[j] = ((float)vv - cy) / fy;
        cr[j] = inside[j] ? cen[(size_t)ref * HW + (size_t)vv * W + uu] : 0;
    }

    unsigned pk0 = 0u, pk1 = 0u, pk2 = 0u, pk3 = 0u;   // the last eight planes, the oldest in the low half of pk0
    for (int k = 0; k < P; ++k) {
        const float z = planes[k];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!live[j]) continue;
            int val = fill;
            if (inside[j]) {
                const float X = dxr[j] * z, Y = dyr[j] * z;
                val = 0;
                for (int s = 0; s < S; ++s) {
                    int c = A.penalty;
                    const int src = meta[1 + s];
                    if (src >= 0) {
                        size_t pix;
                        float zc;
                        const bool vis = project(tab + (size_t)(1 + s) * kRec, X, Y, z, H, W, pix, zc);
                        const int ham = __popcll(cr[j] ^ cen[(size_t)src * HW + pix]);
                        c = vis ? ham : c;
                    }
                    val += c;
                }
            }
            raw[tid + NT * j] = val;
        }
        __syncthreads();
        for (int e = tid; e < (TH + 2 * a) * TW; e += NT) {
            const int* row = raw + (e / TW) * T + (e % TW);
            int x = row[0];
            for (int d = 1; d <= 2 * a; ++d) x += row[d];
            hs[e] = x;
        }
        __syncthreads();
        int tot = hs[ty * TW + tx];
        for (int d = 1; d <= 2 * a; ++d) tot += hs[(ty + d) * TW + tx];
        if (!VEC) {
            if (inimg) out[k] = (uint16_t)tot;
            continue;
        }
        pk0 = (pk0 >> 16) | (pk1 << 16);
        pk1 = (pk1 >> 16) | (pk2 << 16);
        pk2 = (pk2 >> 16) | (pk3 << 16);
        pk3 = (pk3 >> 16) | ((unsigned)tot << 16);
        if (VEC && (k & 7) == 7) {
            // four groups of 8 planes are collected per pixel, then four lanes write a pixel's 64 bytes
            const int g = (k >> 3) & 3;
            stage[tid * 4 + g] = make_uint4(pk0, pk1, pk2, pk3);
            if (g == 3 || k == P - 1) {
                __syncthreads();   // the next write of stage comes after the next plane's barriers
                const int kb = k - 7 - 8 * g;
                for (int i = tid; i < NT * 4; i += NT) {
                    const int p = i >> 2, q = i & 3;
                    const int uu = u0 + p % TW, vv = v0 + p / TW;
                    if (q <= g && uu < W && vv < H)
                        *reinterpret_cast<uint4*>(vol + ((size_t)vv * W + uu) * P + kb + 8 * q) = stage[i];
                }
            }
        }
    }
}

struct SgmArgs {
    const uint16_t* vol;
    uint32_t* sm;
    int H, W, P, p1, p2, dv, du, add;
};

constexpr int kSgmPad = 1 << 24;   // a plane beyond P: above every L + p1 and m + p2, so no minimum picks it
constexpr int kSgmAhead = 4;       // pixels of a line whose loads are in flight ahead of the recurrence

// the minimum over the 64 lanes: two quad permutes and the two row mirrors leave every lane of a row
// of 16 with its row's minimum, four lane reads and scalar minima join the rows
__device__ __forceinline__ int wave_min(int x) {
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false));    // quad_perm:[1,0,3,2]
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xf, 0xf, false));    // quad_perm:[2,3,0,1]
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x141, 0xf, 0xf, false));   // row_half_mirror
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x140, 0xf, 0xf, false));   // row_mirror
    return min(min(__builtin_amdgcn_readlane(x, 0), __builtin_amdgcn_readlane(x, 16)),
               min(__builtin_amdgcn_readlane(x, 32), __builtin_amdgcn_readlane(x, 48)));
}

// One wave per scan line of one direction; lane l holds planes 4l .. 4l + 3 of the line's current
// pixel, so only the two end values of a lane cross lanes.  The first selected direction writes sm,
// the others add to it: a direction's lines touch every pixel exactly once, so there are no atomics.
// VEC: P a multiple of 4 and aligned pointers, one 8-byte load of vol and one 16-byte load / store
// of sm per lane and pixel.
template <bool VEC>
__global__ __launch_bounds__(64) void mvs_sgm_kernel(SgmArgs A) {
    const int lane = threadIdx.x, k0 = lane * 4;
    const int H = A.H, W = A.W, P = A.P, dv = A.dv, du = A.du;
    const int line = blockIdx.x;
    // the line's first pixel (its predecessor lies outside the image) and its length
    int v, u, len;
    if (dv == 0) {
        v = line; u = du > 0 ? 0 : W - 1; len = W;
    } else if (du == 0) {
        u = line; v = dv > 0 ? 0 : H - 1; len = H;
    } else if (line < W) {   // starts on the first row of the direction
        u = line; v = dv > 0 ? 0 : H - 1;
        len = min(H, du > 0 ? W - line : line + 1);
    } else {                 // starts on its first column, below (above) the corner
        const int j = line - W + 1;
        u = du > 0 ? 0 : W - 1; v = dv > 0 ? j : H - 1 - j;
        len = min(W, H - j);
    }
    const size_t first = (size_t)blockIdx.y * H * W + (size_t)v * W + u;
    const ptrdiff_t step = (ptrdiff_t)dv * W + du;
    const uint16_t* __restrict__ vol = A.vol;
    uint32_t* __restrict__ sm = A.sm;
    const bool add = A.add != 0;

    auto load_vol = [&](int t, int (&c)[4]) {
        const size_t at = (first + (ptrdiff_t)t * step) * P + k0;
        if (VEC) {
            uint2 w = make_uint2(0, 0);
            const bool in = k0 < P;
            if (in) w = *reinterpret_cast<const uint2*>(vol + at);
            c[0] = in ? (int)(w.x & 0xffffu) : kSgmPad;
            c[1] = in ? (int)(w.x >> 16) : kSgmPad;
            c[2] = in ? (int)(w.y & 0xffffu) : kSgmPad;
            c[3] = in ? (int)(w.y >> 16) : kSgmPad;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = k0 + i < P ? (int)vol[at + i] : kSgmPad;
        }
    };
    auto load_sm = [&](int t, unsigned (&s)[4]) {
        const size_t at = (first + (ptrdiff_t)t * step) * P + k0;
        if (VEC) {
            uint4 w = make_uint4(0, 0, 0, 0);
            if (k0 < P) w = *reinterpret_cast<const uint4*>(sm + at);
            s[0] = w.x; s[1] = w.y; s[2] = w.z; s[3] = w.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i] = k0 + i < P ? sm[at + i] : 0u;
        }
    };
    auto store_sm = [&](int t, const unsigned (&s)[4]) {
        const size_t at = (first + (ptrdiff_t)t * step) * P + k0;
        if (VEC) {
            if (k0 < P) *reinterpret_cast<uint4*>(sm + at) = make_uint4(s[0], s[1], s[2], s[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k0 + i < P) sm[at + i] = s[i];
        }
    };

    int cv[kSgmAhead][4], nv[kSgmAhead][4];
    unsigned cs[kSgmAhead][4], ns[kSgmAhead][4];
#pragma unroll
    for (int j = 0; j < kSgmAhead; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { cv[j][i] = kSgmPad; cs[j][i] = 0u; nv[j][i] = kSgmPad; ns[j][i] = 0u; }
        if (j < len) {
            load_vol(j, cv[j]);
            if (add) load_sm(j, cs[j]);
        }
    }
    int L[4] = {0, 0, 0, 0};
    for (int t0 = 0; t0 < len; t0 += kSgmAhead) {
#pragma unroll
        for (int j = 0; j < kSgmAhead; ++j) {   // the next pixels' loads, before this group's arithmetic
            const int t = t0 + kSgmAhead + j;
            if (t < len) {
                load_vol(t, nv[j]);
                if (add) load_sm(t, ns[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < kSgmAhead; ++j) {
            const int t = t0 + j;
            if (t >= len) break;
            if (t == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) L[i] = cv[j][i];
            } else {
                const int m = wave_min(min(min(L[0], L[1]), min(L[2], L[3])));
                int lo = __shfl_up(L[3], 1), hi = __shfl_down(L[0], 1);
                lo = lane == 0 ? kSgmPad : lo;
                hi = lane == 63 ? kSgmPad : hi;
                const int cap = m + A.p2, p1 = A.p1;
                const int n0 = min(min(L[0], min(lo, L[1]) + p1), cap) - m;
                const int n1 = min(min(L[1], min(L[0], L[2]) + p1), cap) - m;
                const int n2 = min(min(L[2], min(L[1], L[3]) + p1), cap) - m;
                const int n3 = min(min(L[3], min(L[2], hi) + p1), cap) - m;
                L[0] = cv[j][0] + n0;
                L[1] = cv[j][1] + n1;
                L[2] = cv[j][2] + n2;
                L[3] = cv[j][3] + n3;
            }
            unsigned o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = cs[j][i] + (unsigned)L[i];
            store_sm(t, o);
        }
#pragma unroll
        for (int j = 0; j < kSgmAhead; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) { cv[j][i] = nv[j][i]; cs[j][i] = ns[j][i]; }
    }
}

struct SelectArgs {
    const uint32_t* sm;
    const float* tab;
    const int* meta;
    const float* planes;
    int H, W, S, P, uniq, min_views;
    float* depth;
    int* kstar;    // nullable, like best, second and nv
    int* best;
    int* second;
    uint8_t* nv;
};

// Steps 5 - 7 on the aggregated volume: one lane per pixel walks its run of P values (VEC: four per
// load) with the sweep's state, the four smallest (cost << 8 | plane) keys (sm < 2^24, P <= 256);
// the winner's neighbours are read back and nv is recomputed by projecting at the winner.
template <bool VEC>
__global__ __launch_bounds__(256) void mvs_select_kernel(SelectArgs A) {
    const int H = A.H, W = A.W, S = A.S, P = A.P;
    const size_t HW = (size_t)H * W;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= HW) return;
    const size_t opix = (size_t)blockIdx.y * HW + idx;
    const int* __restrict__ meta = A.meta + (size_t)blockIdx.y * (S + 1);
    const float* __restrict__ tab = A.tab + (size_t)blockIdx.y * (S + 1) * kRec;
    const float* __restrict__ planes = A.planes;
    if (meta[0] < 0) {
        A.depth[opix] = 0.f;
        if (A.kstar) A.kstar[opix] = 0;
        if (A.best) A.best[opix] = 0;
        if (A.second) A.second[opix] = 0;
        if (A.nv) A.nv[opix] = 0;
        return;
    }
    const uint32_t* __restrict__ col = A.sm + opix * P;
    unsigned b0 = 0xffffffffu, b1 = 0xffffffffu, b2 = 0xffffffffu, b3 = 0xffffffffu;
    auto fold = [&](unsigned val, int k) {
        unsigned key = (val << 8) | (unsigned)k, t;
        t = min(b0, key); key = max(b0, key); b0 = t;
        t = min(b1, key); key = max(b1, key); b1 = t;
        t = min(b2, key); key = max(b2, key); b2 = t;
        b3 = min(b3, key);
    };
    if (VEC) {
        for (int k = 0; k < P; k += 4) {
            const uint4 w = *reinterpret_cast<const uint4*>(col + k);
            fold(w.x, k);
            fold(w.y, k + 1);
            fold(w.z, k + 2);
            fold(w.w, k + 3);
        }
    } else {
        for (int k = 0; k < P; ++k) fold(col[k], k);
    }
    const int ks = (int)(b0 & 0xffu), best = (int)(b0 >> 8);
    int second = INT_MAX;
    {
        const unsigned cand[3] = {b3, b2, b1};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int kk = (int)(cand[i] & 0xffu);
            if (cand[i] != 0xffffffffu && abs(kk - ks) >= 2) second = (int)(cand[i] >> 8);
        }
    }
    const int u = (int)(idx % W), v = (int)(idx / W);
    const float z = planes[ks];
    const float X = (((float)u - tab[2]) / tab[0]) * z, Y = (((float)v - tab[3]) / tab[1]) * z;
    int nvbest = 0;
    for (int s = 0; s < S; ++s) {
        if (meta[1 + s] < 0) continue;
        size_t pix;
        float zc;
        nvbest += project(tab + (size_t)(1 + s) * kRec, X, Y, z, H, W, pix, zc) ? 1 : 0;
    }
    float depth = 0.f;
    if (ks > 0 && ks < P - 1 && nvbest >= A.min_views && 256ll * best <= (long long)A.uniq * second) {
        const float i0 = 1.0f / planes[ks], im = 1.0f / planes[ks - 1], ip = 1.0f / planes[ks + 1];
        const float c0 = (float)best, cmf = (float)col[ks - 1], cpf = (float)col[ks + 1];
        const float den = (cmf - c0) + (cpf - c0);
        const float off = den > 0.f ? (cmf - cpf) / (2.0f * den) : 0.f;
        const float step = off >= 0.f ? ip - i0 : i0 - im;
        depth = 1.0f / (i0 + off * step);
    }
    A.depth[opix] = depth;
    if (A.kstar) A.kstar[opix] = ks;
    if (A.best) A.best[opix] = best;
    if (A.second) A.second[opix] = second;
    if (A.nv) A.nv[opix] = (uint8_t)nvbest;
}

constexpr int kSgmMaxP = 256, kSgmMaxPen = 16383;
constexpr int kSgmDir[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};   // (dv, du)

int check_views(const char* fn, int V, int H, int W, int R, int S) {
    SFMHIP_REQUIRE(V >= 0 && H >= 0 && W >= 0 && R >= 0, "%s: bad shape (V %d, H %d, W %d, R %d)", fn, V, H, W, R);
    SFMHIP_REQUIRE(H < (1 << 20) && W < (1 << 20) && (int64_t)H * W < (int64_t)INT_MAX,
                   "%s: an image must hold fewer than 2^31 pixels and 2^20 per side", fn);
    SFMHIP_REQUIRE(R <= 65535, "%s: at most 65535 reference views per call, got %d", fn, R);
    SFMHIP_REQUIRE(S >= 1 && S <= kMaxS, "%s: S must be in [1, %d], got %d", fn, kMaxS, S);
    return SFMHIP_OK;
}

// scratch of a call: the records [R][S + 1][16] f32, then meta [R][S + 1] i32
int prepare(const char* fn, const float* poses, const float* K, int V, const int32_t* refs, const int32_t* srcs, int R,
            int S, hipStream_t st, void** sc, float** tab, int** meta) {
    const size_t n = (size_t)R * (S + 1);
    const hipError_t e = scratch_alloc(sc, n * (kRec * sizeof(float) + sizeof(int)), st);
    if (e != hipSuccess) {
        set_error("%s: scratch: %s", fn, hipGetErrorString(e));
        return SFMHIP_E_HIP;
    }
    *tab = static_cast<float*>(*sc);
    *meta = reinterpret_cast<int*>(*tab + n * kRec);
    hipLaunchKernelGGL(mvs_prepare_kernel, dim3(ceil_div((int64_t)n, 64)), dim3(64), 0, st, poses, K, V, refs, srcs, R,
                       S, *tab, *meta);
    return check_launch("mvs_prepare_kernel");
}

}  // namespace
}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_census(const uint8_t* img, int V, int H, int W, uint64_t* cen, void* stream) {
    const char* fn = "sfmhip_census";
    SFMHIP_REQUIRE(V >= 0 && H >= 0 && W >= 0, "%s: bad shape (V %d, H %d, W %d)", fn, V, H, W);
    SFMHIP_REQUIRE(V <= 65535 && H < (1 << 20) && W < (1 << 20) && (int64_t)H * W < (int64_t)INT_MAX,
                   "%s: at most 65535 views of fewer than 2^31 pixels and 2^20 per side", fn);
    if (V == 0 || H == 0 || W == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(img && cen, "%s: null pointer", fn);
    const int ntx = ceil_div(W, 16);
    hipLaunchKernelGGL(mvs_census_kernel, dim3(ntx * ceil_div(H, 16), V), dim3(256), 0, as_stream(stream), img, H, W,
                       ntx, cen);
    return check_launch("mvs_census_kernel");
}

extern "C" int sfmhip_plane_sweep(const uint64_t* cen, const float* poses, const float* K, int V, int H, int W,
                                  const int32_t* refs, const int32_t* srcs, int R, int S, const float* planes, int P,
                                  int agg_radius, int penalty, int uniq, int min_views, float* depth, int32_t* kstar,
                                  int32_t* best, int32_t* second, uint8_t* nv, void* stream) {
    const char* fn = "sfmhip_plane_sweep";
    int rc = check_views(fn, V, H, W, R, S);
    if (rc != SFMHIP_OK) return rc;
    SFMHIP_REQUIRE(P >= 1 && P <= 65535, "%s: P must be in [1, 65535], got %d", fn, P);
    SFMHIP_REQUIRE(agg_radius >= 0 && agg_radius <= kMaxA, "%s: agg_radius must be in [0, %d], got %d", fn, kMaxA,
                   agg_radius);
    SFMHIP_REQUIRE(penalty >= 0 && penalty <= kMaxPenalty, "%s: penalty must be in [0, %d], got %d", fn, kMaxPenalty,
                   penalty);
    SFMHIP_REQUIRE(uniq >= 0 && uniq <= 256, "%s: uniq must be in [0, 256], got %d", fn, uniq);
    SFMHIP_REQUIRE(min_views >= 0, "%s: min_views must be >= 0, got %d", fn, min_views);
    if (R == 0 || H == 0 || W == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(poses && K && refs && srcs && planes && depth && (cen || V == 0), "%s: null pointer", fn);
    hipStream_t st = as_stream(stream);
    void* sc = nullptr;
    SweepArgs A = {};
    float* tab = nullptr;
    int* meta = nullptr;
    rc = prepare(fn, poses, K, V, refs, srcs, R, S, st, &sc, &tab, &meta);
    if (rc == SFMHIP_OK) {
        A.cen = cen;
        A.tab = tab;
        A.meta = meta;
        A.planes = planes;
        A.H = H;
        A.W = W;
        A.S = S;
        A.P = P;
        A.a = agg_radius;
        A.penalty = penalty;
        A.uniq = uniq;
        A.min_views = min_views;

        A.depth = depth;
        A.kstar = kstar;
        A.best = best;
        A.second = second;
        A.nv = nv;
        A.ntx = ceil_div(W, kTileW);
        hipLaunchKernelGGL((mvs_sweep_kernel<kTileW, kTileH>), dim3(A.ntx * ceil_div(H, kTileH), R),
                           dim3(kTileW * kTileH), 0, st, A);
        rc = check_launch("mvs_sweep_kernel");
    }
    if (sc) scratch_free(sc, st);
    return rc;
}

extern "C" int sfmhip_depth_consistency(const float* depth, const float* poses, const float* K, int V, int H, int W,
                                        const int32_t* refs, const int32_t* srcs, int R, int S, float eps,
                                        int min_consistent, uint8_t* count, float* filtered, void* stream) {
    const char* fn = "sfmhip_depth_consistency";
    int rc = check_views(fn, V, H, W, R, S);
    if (rc != SFMHIP_OK) return rc;
    SFMHIP_REQUIRE(eps >= 0.f && eps < 0x1p60f, "%s: eps must be finite and >= 0", fn);   // a NaN fails
    SFMHIP_REQUIRE(min_consistent >= 0, "%s: min_consistent must be >= 0, got %d", fn, min_consistent);
    if (R == 0 || H == 0 || W == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(poses && K && refs && srcs && count && filtered && (depth || V == 0), "%s: null pointer", fn);
    SFMHIP_REQUIRE((const void*)depth != (const void*)filtered, "%s: the filtered depth must not alias the input", fn);
    hipStream_t st = as_stream(stream);
    void* sc = nullptr;
    float* tab = nullptr;
    int* meta = nullptr;
    rc = prepare(fn, poses, K, V, refs, srcs, R, S, st, &sc, &tab, &meta);
    if (rc == SFMHIP_OK) {
        const int ntx = ceil_div(W, 16);
        hipLaunchKernelGGL(mvs_filter_kernel, dim3(ntx * ceil_div(H, 16), R), dim3(256), 0, st, depth, tab, meta, H, W,
                           S, ntx, eps, min_consistent, count, filtered);
        rc = check_launch("mvs_filter_kernel");
    }
    if (sc) scratch_free(sc, st);
    return rc;
}

extern "C" int sfmhip_cost_volume(const uint64_t* cen, const float* poses, const float* K, int V, int H, int W,
                                  const int32_t* refs, const int32_t* srcs, int R, int S, const float* planes, int P,
                                  int agg_radius, int penalty, uint16_t* vol, void* stream) {
    const char* fn = "sfmhip_cost_volume";
    int rc = check_views(fn, V, H, W, R, S);
    if (rc != SFMHIP_OK) return rc;
    SFMHIP_REQUIRE(P >= 1 && P <= 65535, "%s: P must be in [1, 65535], got %d", fn, P);
    SFMHIP_REQUIRE(agg_radius >= 0 && agg_radius <= kMaxA, "%s: agg_radius must be in [0, %d], got %d", fn, kMaxA,
                   agg_radius);
    SFMHIP_REQUIRE(penalty >= 0 && penalty <= kMaxPenalty, "%s: penalty must be in [0, %d], got %d", fn, kMaxPenalty,
                   penalty);
    if (R == 0 || H == 0 || W == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(poses && K && refs && srcs && planes && vol && (cen || V == 0), "%s: null pointer", fn);
    hipStream_t st = as_stream(stream);
    void* sc = nullptr;
    float* tab = nullptr;
    int* meta = nullptr;
    rc = prepare(fn, poses, K, V, refs, srcs, R, S, st, &sc, &tab, &meta);
    if (rc == SFMHIP_OK) {
        VolumeArgs A = {};
        A.H = H;
        A.W = W;
        A.S = S;
        A.P = P;
        A.a = agg_radius;
        A.penalty = penalty;
        A.ntx = ceil_div(W, kTileW);
        const dim3 grid(A.ntx * ceil_div(H, kTileH), R), block(kTileW * kTileH);
        if (P % 8 == 0 && reinterpret_cast<uintptr_t>(vol) % 16 == 0)
            hipLaunchKernelGGL((mvs_volume_kernel<kTileW, kTileH, true>), grid, block, 0, st, A, cen, (const float*)tab,
                               (const int*)meta, planes, vol);
        else
            hipLaunchKernelGGL((mvs_volume_kernel<kTileW, kTileH, false>), grid, block, 0, st, A, cen,
                               (const float*)tab, (const int*)meta, planes, vol);
        rc = check_launch("mvs_volume_kernel");
    }
    if (sc) scratch_free(sc, st);
    return rc;
}

extern "C" int sfmhip_sgm_aggregate(const uint16_t* vol, int R, int H, int W, int P, int p1, int p2, int path_mask,
                                    uint32_t* sm, void* stream) {
    const char* fn = "sfmhip_sgm_aggregate";
    SFMHIP_REQUIRE(R >= 0 && H >= 0 && W >= 0, "%s: bad shape (R %d, H %d, W %d)", fn, R, H, W);
    SFMHIP_REQUIRE(H < (1 << 20) && W < (1 << 20) && (int64_t)H * W < (int64_t)INT_MAX,
                   "%s: an image must hold fewer than 2^31 pixels and 2^20 per side", fn);
    SFMHIP_REQUIRE(R <= 65535, "%s: at most 65535 reference views per call, got %d", fn, R);
    SFMHIP_REQUIRE(P >= 1 && P <= kSgmMaxP, "%s: P must be in [1, %d], got %d", fn, kSgmMaxP, P);
    SFMHIP_REQUIRE(p1 >= 0 && p1 <= p2 && p2 <= kSgmMaxPen, "%s: need 0 <= p1 <= p2 <= %d, got p1 %d, p2 %d", fn,
                   kSgmMaxPen, p1, p2);
    SFMHIP_REQUIRE(path_mask >= 1 && path_mask <= 0xff, "%s: path_mask must be in [1, 255], got %d", fn, path_mask);
    if (R == 0 || H == 0 || W == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(vol && sm, "%s: null pointer", fn);
    hipStream_t st = as_stream(stream);
    const bool vec = P % 4 == 0 && reinterpret_cast<uintptr_t>(vol) % 8 == 0 && reinterpret_cast<uintptr_t>(sm) % 16 == 0;
    SgmArgs A = {vol, sm, H, W, P, p1, p2, 0, 0, 0};
    for (int d = 0; d < 8; ++d) {
        if (!(path_mask >> d & 1)) continue;
        A.dv = kSgmDir[d][0];
        A.du = kSgmDir[d][1];
        const int lines = A.dv == 0 ? H : A.du == 0 ? W : H + W - 1;
        if (vec)
            hipLaunchKernelGGL(mvs_sgm_kernel<true>, dim3(lines, R), dim3(64), 0, st, A);
        else
            hipLaunchKernelGGL(mvs_sgm_kernel<false>, dim3(lines, R), dim3(64), 0, st, A);
        const int rc = check_launch("mvs_sgm_kernel");
        if (rc != SFMHIP_OK) return rc;
        A.add = 1;   // the first selected direction writes sm, the others add to it
    }
    return SFMHIP_OK;
}

extern "C" int sfmhip_volume_select(const uint32_t* sm, const float* poses, const float* K, int V, int H, int W,
                                    const int32_t* refs, const int32_t* srcs, int R, int S, const float* planes, int P,
                                    int uniq, int min_views, float* depth, int32_t* kstar, int32_t* best,
                                    int32_t* second, uint8_t* nv, void* stream) {
    const char* fn = "sfmhip_volume_select";
    int rc = check_views(fn, V, H, W, R, S);
    if (rc != SFMHIP_OK) return rc;
    SFMHIP_REQUIRE(P >= 1 && P <= kSgmMaxP, "%s: P must be in [1, %d], got %d", fn, kSgmMaxP, P);
    SFMHIP_REQUIRE(uniq >= 0 && uniq <= 256, "%s: uniq must be in [0, 256], got %d", fn, uniq);
    SFMHIP_REQUIRE(min_views >= 0, "%s: min_views must be >= 0, got %d", fn, min_views);
    if (R == 0 || H == 0 || W == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(sm && poses && K && refs && srcs && planes && depth, "%s: null pointer", fn);
    hipStream_t st = as_stream(stream);
    void* sc = nullptr;
    float* tab = nullptr;
    int* meta = nullptr;
    rc = prepare(fn, poses, K, V, refs, srcs, R, S, st, &sc, &tab, &meta);
    if (rc == SFMHIP_OK) {
        SelectArgs A = {};
        A.sm = sm;
        A.tab = tab;
        A.meta = meta;
        A.planes = planes;
        A.H = H;
        A.W = W;
        A.S = S;
        A.P = P;
        A.uniq = uniq;
        A.min_views = min_views;
        A.depth = depth;
        A.kstar = kstar;
        A.best = best;
        A.second = second;
        A.nv = nv;
        const dim3 grid(ceil_div((int64_t)H * W, 256), R);
        if (P % 4 == 0 && reinterpret_cast<uintptr_t>(sm) % 16 == 0)
            hipLaunchKernelGGL(mvs_select_kernel<true>, grid, dim3(256), 0, st, A);
        else
            hipLaunchKernelGGL(mvs_select_kernel<false>, grid, dim3(256), 0, st, A);
        rc = check_launch("mvs_select_kernel");
    }
    if (sc) scratch_free(sc, st);
    return rc;
}
