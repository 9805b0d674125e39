// raycast.hip — V8: depth, normal and colour maps of the fused TSDF grid (T, Wt[, C]) seen
// from V cameras (semantics: include/sfmhip.h V8, restated in numpy by
// tests/tsdf_raycast_ref.py).  Two kernels:
//   prepare  one workgroup per brick of 8^3 voxels: G = T where observed, else NaN (one array
//            for value and validity: a NaN corner makes the trilinear value NaN), and one byte
//            per brick: 1 = no sample whose cell origin lies in the brick can have F < iso
//   march    one lane per pixel, a wave = an 8 x 8 pixel tile, a workgroup = 16 x 16 pixels;
//            a lane stops at its first hit.  With skipping, a lane leaves out runs of samples
//            that lie outside the grid on one side of an axis, or in one ruled-out brick: it
//            proposes the end of a run from a float estimate and keeps it only when the
//            sample at that end is of the same kind (i_a(k) is monotone in k, so everything
//            between is too).  A failed proposal costs one cell computation.
// All f32 with -ffp-contract=off: depth and rgba are bit-identical to the numpy form.
#include "common.h"
#include <climits>
#include <cmath>

namespace sfmhip {
namespace {

constexpr int kBrick = 8, kBrickShift = 3;
constexpr int kMaxSamples = 65536;

struct RcGeo {
    float bmin[3], bmax[3], s[3];   // x, y, z
    int dim[3];                     // W, H, D
    int nbx, nby, nbz;
};

// ---- prepare --------------------------------------------------------------------
// Brick (bx, by, bz) owns voxels [8b, 8b + 8) per axis; a sample whose cell origin is one of
// them reads voxels [8b, 8b + 8] (clipped to the grid).  Over the observed ones of those 9^3:
// L = min T, A = max |T|.  Ruled out: none observed, or A < 2^126 and
// L >= iso + (2^-19 A + 2^-126) (in f64: exact enough, the margin is 1.6x the bound).
__global__ __launch_bounds__(256) void rc_prepare_kernel(const float* __restrict__ T, const float* __restrict__ Wt,
                                                         RcGeo g, float iso, float minw, float* __restrict__ G,
                                                         uint8_t* __restrict__ tab) {
    __shared__ float sL[4], sA[4];
    const int W = g.dim[0], H = g.dim[1], D = g.dim[2];
    const int x0 = blockIdx.x * kBrick, y0 = blockIdx.y * kBrick, z0 = blockIdx.z * kBrick;
    float L = INFINITY, A = 0.f;
    for (int i = threadIdx.x; i < 9 * 9 * 9; i += 256) {
        const int lx = i % 9, ly = (i / 9) % 9, lz = i / 81;
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        if (x >= W || y >= H || z >= D) continue;
        const size_t v = ((size_t)z * H + y) * W + x;
        const float t = T[v], w = Wt[v];
        const bool obs = w >= minw && isfinite(t);
        if (lx < kBrick && ly < kBrick && lz < kBrick) G[v] = obs ? t : __builtin_nanf("");
        if (obs) {
            L = fminf(L, t);
            A = fmaxf(A, fabsf(t));
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        L = fminf(L, __shfl_xor(L, off, 64));
        A = fmaxf(A, __shfl_xor(A, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        sL[threadIdx.x >> 6] = L;
        sA[threadIdx.x >> 6] = A;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        L = fminf(fminf(sL[0], sL[1]), fminf(sL[2], sL[3]));
        A = fmaxf(fmaxf(sA[0], sA[1]), fmaxf(sA[2], sA[3]));
        bool out = L == INFINITY;   // nothing observed
        if (!out && A < 0x1p126f) out = (double)L >= (double)iso + ((double)A * 0x1p-19 + 0x1p-126);
        tab[((size_t)blockIdx.z * g.nby + blockIdx.y) * g.nbx + blockIdx.x] = out ? 1 : 0;
    }
}

// ---- march ------------------------------------------------------------------------
struct Ray {
    float o[3], dw[3];
};

// out-code bits: 2a = below the grid on axis a, 2a + 1 = above, 6 = NaN
struct Cell {
    float f[3];
    int i[3];
    unsigned oc;
};

__device__ __forceinline__ Cell cell_at(const Ray& r, const RcGeo& g, float t) {
    Cell c;
    c.oc = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = r.o[a] + t * r.dw[a];
        const float q = (p - g.bmin[a]) / g.s[a];
        const float fl = floorf(q);
        const float hi = (float)(g.dim[a] - 2);
        unsigned b = 0;
        if (fl < 0.f) b = 1u << (2 * a);
        else if (fl > hi) b = 2u << (2 * a);
        else if (!(fl >= 0.f)) b = 64u;
        c.oc |= b;
        c.f[a] = q - fl;
        c.i[a] = b ? 0 : (int)fl;
    }
    return c;
}

__device__ __forceinline__ float lerp(float a, float b, float w) { return a + w * (b - a); }

// the 8 corners of an in-range cell, index dx + 2 dy + 4 dz
__device__ __forceinline__ void load_corners(const float* __restrict__ G, const RcGeo& g, const Cell& c, float* t) {
    const unsigned W = (unsigned)g.dim[0], HW = W * (unsigned)g.dim[1];
    const unsigned b = (unsigned)c.i[2] * HW + (unsigned)c.i[1] * W + (unsigned)c.i[0];
    t[0] = G[b];
    t[1] = G[b + 1];
    t[2] = G[b + W];
    t[3] = G[b + W + 1];
    t[4] = G[b + HW];
    t[5] = G[b + HW + 1];
    t[6] = G[b + HW + W];
    t[7] = G[b + HW + W + 1];
}

__device__ __forceinline__ float eval_F(const float* __restrict__ G, const RcGeo& g, const Cell& c) {
    if (c.oc) return __builtin_nanf("");
    float t[8];
    load_corners(G, g, c, t);
    const float a00 = lerp(t[0], t[1], c.f[0]), a01 = lerp(t[2], t[3], c.f[0]);
    const float a10 = lerp(t[4], t[5], c.f[0]), a11 = lerp(t[6], t[7], c.f[0]);
    return lerp(lerp(a00, a01, c.f[1]), lerp(a10, a11, c.f[1]), c.f[2]);
}

__device__ __forceinline__ unsigned brick_of(const RcGeo& g, const Cell& c) {
    return ((unsigned)(c.i[2] >> kBrickShift) * (unsigned)g.nby + (unsigned)(c.i[1] >> kBrickShift)) *
               (unsigned)g.nbx + (unsigned)(c.i[0] >> kBrickShift);
}

// float -> sample index in [0, n] (NaN -> 0)
__device__ __forceinline__ int clamp_index(float x, int n) { return (int)fminf(fmaxf(x, 0.f), (float)n); }

struct RcArgs {
    RcGeo g;
    const float* poses;
    const float* Kf;
    int Hd, Wd;
    float iso, t_near, step;
    int n;
};

template <bool SKIP>
__global__ __launch_bounds__(256) void rc_march_kernel(const float* __restrict__ G, const uint8_t* __restrict__ tab,
                                                       const uint4* __restrict__ C, RcArgs A,
                                                       float* __restrict__ depth, float* __restrict__ normals,
                                                       uchar4* __restrict__ rgba, int32_t* __restrict__ steps) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int v = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const int view = blockIdx.z;
    if (u >= A.Wd || v >= A.Hd) return;
    const RcGeo& g = A.g;
    const size_t pix = ((size_t)view * A.Hd + v) * A.Wd + u;

    float P[12], K[4];
    bool good = true;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        P[q] = A.poses[view * 12 + q];
        good = good && fabsf(P[q]) < 0x1p60f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        K[q] = A.Kf[view * 4 + q];
        good = good && fabsf(K[q]) < 0x1p60f;
    }
    good = good && K[0] != 0.f && K[1] != 0.f;

    bool hit = false;
    int evals = 0;
    float d = 0.f;
    Ray r;
    if (good) {
        const float dcx = ((float)u - K[2]) / K[0], dcy = ((float)v - K[3]) / K[1];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            r.o[a] = -((P[a] * P[3] + P[4 + a] * P[7]) + P[8 + a] * P[11]);
            r.dw[a] = (P[a] * dcx + P[4 + a] * dcy) + P[8 + a];
        }
        const float iso = A.iso;
        const int n = A.n;
        auto t_of = [&](int k) { return A.t_near + (float)k * A.step; };
        float Fp = 0.f, Fc = 0.f;
        int k = 1;
        if (!SKIP) {
            Fp = eval_F(G, g, cell_at(r, g, t_of(0)));
            evals = 1;
            for (; k < n; ++k) {
                Fc = eval_F(G, g, cell_at(r, g, t_of(k)));
                ++evals;
                if (Fp >= iso && Fc < iso) {
                    hit = true;
                    break;
                }
                Fp = Fc;
            }
        } else {
            int n_eff = n;
            // a non-finite origin or direction component makes every p_a non-finite: no valid sample
            bool fin = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) fin = fin && isfinite(r.o[a]) && isfinite(r.dw[a]);
            if (!fin) n_eff = 0;
            const float inv_step = 1.0f / A.step;
            float inv_dw[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) inv_dw[a] = 1.0f / r.dw[a];
            if (n_eff > 2) {
                // box clipping: slab estimates of the entry and exit parameters, each kept only
                // when the samples at both ends of the clipped run are outside on the same side
                float tin = -INFINITY, tout = INFINITY;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float t0 = (g.bmin[a] - r.o[a]) * inv_dw[a], t1 = (g.bmax[a] - r.o[a]) * inv_dw[a];
                    tin = fmaxf(tin, fminf(t0, t1));
                    tout = fminf(tout, fmaxf(t0, t1));
                }
                const Cell last = cell_at(r, g, t_of(n - 1));
                const int kx = clamp_index(ceilf((tout - A.t_near) * inv_step) + 2.f, n);
                if (kx < n - 1 && (last.oc & 63u)) {
                    const Cell e = cell_at(r, g, t_of(kx));
                    if (e.oc & last.oc & 63u) n_eff = kx;   // samples kx .. n-1 are outside
                }
                const int ki = min(clamp_index(floorf((tin - A.t_near) * inv_step) - 2.f, n), n_eff - 1);
                if (ki > 1) {
                    const Cell c1 = cell_at(r, g, t_of(1)), e = cell_at(r, g, t_of(ki));
                    if (c1.oc & e.oc & 63u) k = ki + 1;   // samples 1 .. ki are outside
                }
            }
            bool have = false;
            int jump = 1;
            while (k < n_eff) {
                const Cell c = cell_at(r, g, t_of(k));
                bool skip = false;
                int adv = 1;
                if (c.oc) {   // outside the grid: not valid
                    skip = true;
                    const int kk = min(k + jump, n_eff - 1);
                    if (kk > k && (c.oc & 63u)) {
                        const Cell e = cell_at(r, g, t_of(kk));
                        if (c.oc & e.oc & 63u) {
                            adv = kk - k + 1;
                            jump = min(jump * 2, 1 << 14);
                        } else {
                            jump = max(jump >> 1, 1);
                        }
                    }
                } else {
                    const unsigned bi = brick_of(g, c);
                    if (tab[bi]) {   // a brick in which no sample has F < iso
                        skip = true;
                        // where the ray leaves the brick (cell origins [8b, 8b + 8) per axis)
                        float tex = INFINITY;
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            const int b0 = (c.i[a] >> kBrickShift) << kBrickShift;
                            const float edge = g.bmin[a] + (float)(r.dw[a] > 0.f ? b0 + kBrick : b0) * g.s[a];
                            const float ta = (edge - r.o[a]) * inv_dw[a];
                            if (r.dw[a] != 0.f) tex = fminf(tex, ta);
                        }
                        const int kk = min(clamp_index(floorf((tex - A.t_near) * inv_step) - 1.f, n), n_eff - 1);
                        if (kk > k) {
                            const Cell e = cell_at(r, g, t_of(kk));
                            if (!e.oc && brick_of(g, e) == bi) adv = kk - k + 1;
                        }
                    }
                }
                if (skip) {
                    k += adv;
                    have = false;
                    continue;
                }
                if (!have) {
                    Fp = eval_F(G, g, cell_at(r, g, t_of(k - 1)));
                    ++evals;
                }
                Fc = eval_F(G, g, c);
                ++evals;
                if (Fp >= iso && Fc < iso) {
                    hit = true;
                    break;
                }
                Fp = Fc;
                have = true;
                ++k;
            }
        }
        if (hit) d = t_of(k - 1) + A.step * ((Fp - iso) / (Fp - Fc));
    }
    depth[pix] = d;
    if (steps) steps[pix] = evals;
    if (!normals && !rgba) return;

    float nrm[3] = {0.f, 0.f, 0.f};
    uchar4 col = make_uchar4(0, 0, 0, 0);
    if (hit) {
        const Cell c = cell_at(r, g, d);
        float t[8];
        bool valid = c.oc == 0;
        if (valid) {
            load_corners(G, g, c, t);
#pragma unroll
            for (int j = 0; j < 8; ++j) valid = valid && (t[j] == t[j]);
        }
        if (valid && normals) {
            const float fx = c.f[0], fy = c.f[1], fz = c.f[2];
            float gr[3];
            gr[0] = lerp(lerp(t[1] - t[0], t[3] - t[2], fy), lerp(t[5] - t[4], t[7] - t[6], fy), fz) / g.s[0];
            gr[1] = lerp(lerp(t[2] - t[0], t[3] - t[1], fx), lerp(t[6] - t[4], t[7] - t[5], fx), fz) / g.s[1];
            gr[2] = lerp(lerp(t[4] - t[0], t[5] - t[1], fx), lerp(t[6] - t[2], t[7] - t[3], fx), fy) / g.s[2];
            const float len = sqrtf((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2]);
            if (len > 0.f && isfinite(len)) {
#pragma unroll
                for (int a = 0; a < 3; ++a) nrm[a] = gr[a] / len;
            }
        }
        if (valid && rgba) {
            const unsigned W = (unsigned)g.dim[0], HW = W * (unsigned)g.dim[1];
            const unsigned b = (unsigned)c.i[2] * HW + (unsigned)c.i[1] * W + (unsigned)c.i[0];
            float num[3] = {0.f, 0.f, 0.f}, den = 0.f;
            bool any = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint4 q = C[b + (j & 1) + ((j >> 1) & 1) * W + (j >> 2) * HW];
                if (q.w == 0u) continue;
                any = true;
                const float ux = (j & 1) ? c.f[0] : 1.0f - c.f[0];
                const float uy = (j & 2) ? c.f[1] : 1.0f - c.f[1];
                const float uz = (j & 4) ? c.f[2] : 1.0f - c.f[2];
                const float w = (ux * uy) * uz, cn = (float)q.w;
                num[0] = num[0] + w * ((float)q.x / cn);
                num[1] = num[1] + w * ((float)q.y / cn);
                num[2] = num[2] + w * ((float)q.z / cn);
                den = den + w;
            }
            if (any) {
                unsigned char o8[3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    o8[a] = (unsigned char)__builtin_rintf(fminf(255.f, fmaxf(0.f, num[a] / den)));
                col = make_uchar4(o8[0], o8[1], o8[2], 255);
            }
        }
    }
    if (normals) {
        normals[pix * 3] = nrm[0];
        normals[pix * 3 + 1] = nrm[1];
        normals[pix * 3 + 2] = nrm[2];
    }
    if (rgba) rgba[pix] = col;
}

}  // namespace
}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_tsdf_raycast(const float* T, const float* Wt, const uint32_t* C, int D, int H, int W,
                                   const float* poses, const float* Kf, int V, int Hd, int Wd, const float* bmin,
                                   const float* bmax, float iso, float min_weight, float t_near, float step,
                                   int n_samples, float* depth, float* normals, uint8_t* rgba, int32_t* steps,
                                   void* stream) {
    const char* fn = "sfmhip_tsdf_raycast";
    SFMHIP_REQUIRE(D >= 2 && H >= 2 && W >= 2, "%s: bad grid shape (%d,%d,%d)", fn, D, H, W);
    SFMHIP_REQUIRE((int64_t)D * H * W < (int64_t)INT_MAX, "%s: the grid must hold fewer than 2^31 voxels", fn);
    SFMHIP_REQUIRE(V >= 0 && Hd >= 0 && Wd >= 0, "%s: bad image shape (%d,%d,%d)", fn, V, Hd, Wd);
    SFMHIP_REQUIRE(V <= 65535 && Hd < (1 << 20) && Wd < (1 << 20), "%s: too many views or pixels", fn);
    SFMHIP_REQUIRE(min_weight > 0.f, "%s: min_weight must be > 0", fn);
    SFMHIP_REQUIRE(t_near >= 0.f && std::isfinite(t_near), "%s: near must be finite and >= 0", fn);
    SFMHIP_REQUIRE(step > 0.f && std::isfinite(step), "%s: step must be finite and > 0", fn);
    SFMHIP_REQUIRE(n_samples >= 1 && n_samples <= kMaxSamples, "%s: n_samples must be in [1, %d], got %d", fn,
                   kMaxSamples, n_samples);
    SFMHIP_REQUIRE(bmin && bmax, "%s: null pointer (bounds)", fn);
    RcArgs A;
    RcGeo& g = A.g;
    g.dim[0] = W;
    g.dim[1] = H;
    g.dim[2] = D;
    for (int a = 0; a < 3; ++a) {
        SFMHIP_REQUIRE(std::fabs(bmin[a]) < 0x1p60f && std::fabs(bmax[a]) < 0x1p60f,
                       "%s: bounds must be finite and below 2^60 in magnitude", fn);
        g.bmin[a] = bmin[a];
        g.bmax[a] = bmax[a];
        g.s[a] = (bmax[a] - bmin[a]) / (float)(g.dim[a] - 1);
        SFMHIP_REQUIRE(g.s[a] > 0.f, "%s: bmax must be above bmin on every axis", fn);
    }
    if (V == 0 || Hd == 0 || Wd == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(T && Wt && poses && Kf && depth, "%s: null pointer", fn);
    SFMHIP_REQUIRE(!rgba || C, "%s: rgba needs the colour grid C", fn);
    SFMHIP_REQUIRE((reinterpret_cast<uintptr_t>(C) & 15u) == 0 && (reinterpret_cast<uintptr_t>(rgba) & 3u) == 0,
                   "%s: C must be 16-byte and rgba 4-byte aligned", fn);
    g.nbx = ceil_div(W, kBrick);
    g.nby = ceil_div(H, kBrick);
    g.nbz = ceil_div(D, kBrick);
    SFMHIP_REQUIRE(g.nby <= 65535 && g.nbz <= 65535 && ceil_div(Hd, 16) <= 65535, "%s: grid or image too large", fn);
    A.poses = poses;
    A.Kf = Kf;
    A.Hd = Hd;
    A.Wd = Wd;
    A.iso = iso;
    A.t_near = t_near;
    A.step = step;
    A.n = n_samples;
    // the monotonicity argument of the skip needs every t_k finite (no inf * 0)
    const float t_last = t_near + (float)(n_samples - 1) * step;
    const bool skip = knobs().raycast_skip != 0 && std::isfinite(t_last);

    hipStream_t st = as_stream(stream);
    const size_t nvox = (size_t)D * H * W, nbricks = (size_t)g.nbx * g.nby * g.nbz;
    void* sc = nullptr;
    const hipError_t e = scratch_alloc(&sc, nvox * sizeof(float) + nbricks, st);
    if (e != hipSuccess) {
        set_error("%s: scratch: %s", fn, hipGetErrorString(e));
        return SFMHIP_E_HIP;
    }
    float* G = static_cast<float*>(sc);
    uint8_t* tab = reinterpret_cast<uint8_t*>(G + nvox);
    hipLaunchKernelGGL(rc_prepare_kernel, dim3(g.nbx, g.nby, g.nbz), dim3(256), 0, st, T, Wt, g, iso, min_weight, G,
                       tab);
    int rc = check_launch("rc_prepare_kernel");
    if (rc == SFMHIP_OK) {
        const dim3 grid(ceil_div(Wd, 16), ceil_div(Hd, 16), V);
        const uint4* C4 = reinterpret_cast<const uint4*>(C);
        uchar4* out4 = reinterpret_cast<uchar4*>(rgba);
        if (skip)
            hipLaunchKernelGGL(rc_march_kernel<true>, grid, dim3(256), 0, st, G, tab, C4, A, depth, normals, out4,
                               steps);
        else
            hipLaunchKernelGGL(rc_march_kernel<false>, grid, dim3(256), 0, st, G, tab, C4, A, depth, normals, out4,
                               steps);
        rc = check_launch("rc_march_kernel");
    }
    scratch_free(sc, st);
    return rc;
}
