// sift.hip — V11: SIFT keypoints and descriptors (the V11 block of include/sfmhip.h).
// Four entries: the Gaussian pyramid, scale-space extrema with sub-sample refinement, orientation
// assignment and the 128-d descriptor.  Every output is defined to the bit: f32 steps in the
// order of the header (-ffp-contract=off), integer histogram sums, no floating-point atomics and
// no device transcendentals (the tables come from the host, the angle is the polynomial turn()).
#include "common.h"

#include <climits>

using namespace sfmhip;

namespace {

constexpr int kS = 3;            // intervals per octave
constexpr int kL = kS + 3;       // Gaussian levels per octave
constexpr int kMaxO = 16;
constexpr int kTapStride = 27;
constexpr int kMaxR = 13;
constexpr int kTW = 64, kTH = 64;   // output tile of one blur block

struct Pyr {
    int O;
    int h[kMaxO], w[kMaxO];
    int64_t off[kMaxO];   // start of octave o inside one view's pyramid (floats)
    int64_t per;          // floats per view
};

Pyr make_pyr(int H, int W, int O) {
    Pyr P;
    P.O = O;
    int64_t off = 0;
    for (int o = 0; o < kMaxO; ++o) {
        P.h[o] = o < O ? ((H - 1) >> o) + 1 : 0;
        P.w[o] = o < O ? ((W - 1) >> o) + 1 : 0;
        P.off[o] = off;
        off += (int64_t)kL * P.h[o] * P.w[o];
    }
    P.per = off;
    return P;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- 1 pyramid -------------------------------------------------------------------------------
// One block blurs a kTH x kTW tile: the tile plus a halo of R in LDS, the row pass into LDS (all
// kTH + 2R rows), the column pass to global memory.  The radius is a template parameter: the tap
// loops unroll, the taps sit in scalar registers, and a thread makes 4 neighbouring outputs from
// one window of 2R + 4 LDS values (16-byte LDS reads along a row) instead of 4 (2R + 1).  Every
// output still sums its 2R + 1 products in ascending k from 0, whatever the tile or the thread:
// neither enters the arithmetic.
template <int R, typename T>
__global__ __launch_bounds__(256) void sift_blur_kernel(const T* __restrict__ src, int64_t src_stride,
                                                        float* __restrict__ dst, int64_t dst_stride, int H, int W,
                                                        const float* __restrict__ taps) {
    constexpr int NT = 2 * R + 1;
    constexpr int ROWS = kTH + 2 * R, COLS = kTW + 2 * R;
    constexpr int NV = (NT + 3 + 3) / 4 * 4;   // the window of 4 outputs, in whole float4
    constexpr int TS = kTW - 4 + NV;           // row stride of the tile: a multiple of 4, >= COLS
    __shared__ __attribute__((aligned(16))) float tile[ROWS * TS];
    __shared__ float rowp[ROWS * kTW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    src += (int64_t)blockIdx.z * src_stride;
    dst += (int64_t)blockIdx.z * dst_stride;
    float tp[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) tp[k] = taps[k];
    for (int idx = tid; idx < ROWS * COLS; idx += 256) {
        const int ty = idx / COLS, tx = idx - ty * COLS;
        const int gy = clampi(y0 + ty - R, 0, H - 1), gx = clampi(x0 + tx - R, 0, W - 1);
        tile[ty * TS + tx] = (float)src[(int64_t)gy * W + gx];
    }
    __syncthreads();
    for (int item = tid; item < ROWS * (kTW / 4); item += 256) {
        const int ty = item / (kTW / 4), g = item - ty * (kTW / 4);
        const float4* p = reinterpret_cast<const float4*>(tile + ty * TS + 4 * g);
        float v[NV];
#pragma unroll
        for (int c = 0; c < NV / 4; ++c) {
            const float4 q = p[c];
            v[4 * c] = q.x;
            v[4 * c + 1] = q.y;
            v[4 * c + 2] = q.z;
            v[4 * c + 3] = q.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < NT; ++k) acc = acc + tp[k] * v[k + j];
            rowp[ty * kTW + 4 * g + j] = acc;
        }
    }
    __syncthreads();
    for (int item = tid; item < (kTH / 4) * kTW; item += 256) {
        const int yg = item / kTW, tx = item - yg * kTW;
        const int gx = x0 + tx, gy = y0 + 4 * yg;
        if (gx >= W || gy >= H) continue;
        const float* p = rowp + (4 * yg) * kTW + tx;
        float v[NT + 3];
#pragma unroll
        for (int m = 0; m < NT + 3; ++m) v[m] = p[m * kTW];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < NT; ++k) acc = acc + tp[k] * v[k + j];
            if (gy + j < H) dst[(int64_t)(gy + j) * W + gx] = acc;
        }
    }
}

template <typename T>
void launch_blur(int r, dim3 grid, hipStream_t st, const T* src, int64_t src_stride, float* dst, int64_t dst_stride,
                 int H, int W, const float* taps) {
#define SIFT_BLUR_CASE(R)                                                                                             \
    case R:                                                                                                           \
        hipLaunchKernelGGL((sift_blur_kernel<R, T>), grid, dim3(256), 0, st, src, src_stride, dst, dst_stride, H, W, \
                           taps);                                                                                     \
        break;
    switch (r) {
        SIFT_BLUR_CASE(0) SIFT_BLUR_CASE(1) SIFT_BLUR_CASE(2) SIFT_BLUR_CASE(3) SIFT_BLUR_CASE(4) SIFT_BLUR_CASE(5)
        SIFT_BLUR_CASE(6) SIFT_BLUR_CASE(7) SIFT_BLUR_CASE(8) SIFT_BLUR_CASE(9) SIFT_BLUR_CASE(10) SIFT_BLUR_CASE(11)
        SIFT_BLUR_CASE(12) SIFT_BLUR_CASE(13)
    }
#undef SIFT_BLUR_CASE
}

__global__ __launch_bounds__(256) void sift_subsample_kernel(const float* __restrict__ src, int64_t stride, int Hs,
                                                             int Ws, float* __restrict__ dst, int Hd, int Wd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)Hd * Wd) return;
    const int y = (int)(i / Wd), x = (int)(i - (int64_t)y * Wd);
    src += (int64_t)blockIdx.y * stride;
    dst += (int64_t)blockIdx.y * stride;
    dst[i] = src[(int64_t)(2 * y) * Ws + 2 * x];   // 2y <= Hs - 1 and 2x <= Ws - 1 by Hd = (Hs + 1) / 2
    (void)Hs;
}

// ---- 2 detect --------------------------------------------------------------------------------
struct DetectParams {
    int border;
    float prethresh, contrast_thr, edge_r;
};

struct Dog {
    const float* g;   // level 0 of the octave
    int64_t hw;
    int W;
    __device__ __forceinline__ float operator()(int l, int y, int x) const {
        const int64_t i = (int64_t)y * W + x;
        return g[(int64_t)(l + 1) * hw + i] - g[(int64_t)l * hw + i];
    }
};

__device__ __forceinline__ bool sift_is_start(const Dog& D, int H, int W, int l, int y, int x, const DetectParams& p) {
    if (y < p.border || y > H - 1 - p.border || x < p.border || x > W - 1 - p.border) return false;
    const float v = D(l, y, x);
    if (!(fabsf(v) > p.prethresh)) return false;
    bool gt = true, lt = true;
    for (int dl = -1; dl <= 1; ++dl)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dl == 0 && dy == 0 && dx == 0) continue;
                const float n = D(l + dl, y + dy, x + dx);
                gt = gt && (v > n);
                lt = lt && (v < n);
            }
    return gt || lt;
}

// The quadratic fit of the header's step 2 from the start sample (l, y, x); out: the 8-word record.
__device__ bool sift_refine(const Dog& D, int H, int W, int o, int l, int y, int x, const DetectParams& p,
                            const float* __restrict__ sig, int32_t* out) {
    float gx = 0, gy = 0, gl = 0, hxx = 0, hyy = 0, hxy = 0, ox = 0, oy = 0, ol = 0, c = 0;
    bool conv = false;
    for (int it = 0; it < 5; ++it) {
        c = D(l, y, x);
        const float xp = D(l, y, x + 1), xm = D(l, y, x - 1), yp = D(l, y + 1, x), ym = D(l, y - 1, x);
        const float lp = D(l + 1, y, x), lm = D(l - 1, y, x);
        gx = (xp - xm) * 0.5f;
        gy = (yp - ym) * 0.5f;
        gl = (lp - lm) * 0.5f;
        const float c2 = 2.0f * c;
        hxx = (xp + xm) - c2;
        hyy = (yp + ym) - c2;
        const float hll = (lp + lm) - c2;
        hxy = ((D(l, y + 1, x + 1) - D(l, y + 1, x - 1)) - (D(l, y - 1, x + 1) - D(l, y - 1, x - 1))) * 0.25f;
        const float hxl = ((D(l + 1, y, x + 1) - D(l + 1, y, x - 1)) - (D(l - 1, y, x + 1) - D(l - 1, y, x - 1))) * 0.25f;
        const float hyl = ((D(l + 1, y + 1, x) - D(l + 1, y - 1, x)) - (D(l - 1, y + 1, x) - D(l - 1, y - 1, x))) * 0.25f;
        const float A00 = hyy * hll - hyl * hyl, A01 = hxl * hyl - hxy * hll, A02 = hxy * hyl - hxl * hyy;
        const float A11 = hxx * hll - hxl * hxl, A12 = hxy * hxl - hxx * hyl, A22 = hxx * hyy - hxy * hxy;
        const float det = (hxx * A00 + hxy * A01) + hxl * A02;
        if (!(fabsf(det) > 0.0f)) return false;
        ox = -(((A00 * gx + A01 * gy) + A02 * gl) / det);
        oy = -(((A01 * gx + A11 * gy) + A12 * gl) / det);
        ol = -(((A02 * gx + A12 * gy) + A22 * gl) / det);
        if (fabsf(ox) < 0.5f && fabsf(oy) < 0.5f && fabsf(ol) < 0.5f) {
            conv = true;
            break;
        }
        if (!(fabsf(ox) <= 1048576.0f && fabsf(oy) <= 1048576.0f && fabsf(ol) <= 1048576.0f)) return false;
        l += (int)rintf(ol);
        y += (int)rintf(oy);
        x += (int)rintf(ox);
        if (l < 1 || l > kS || y < p.border || y > H - 1 - p.border || x < p.border || x > W - 1 - p.border) return false;
    }
    if (!conv) return false;
    const float resp = c + 0.5f * ((gx * ox + gy * oy) + gl * ol);
    if (!(fabsf(resp) * 3.0f >= p.contrast_thr)) return false;
    const float tr = hxx + hyy, d2 = hxx * hyy - hxy * hxy;
    if (!(d2 > 0.0f)) return false;
    const float e1 = p.edge_r + 1.0f;
    if (!((tr * tr) * p.edge_r < (e1 * e1) * d2)) return false;
    const float s0 = sig[l];
    const float sc = ol >= 0.0f ? s0 + ol * (sig[l + 1] - s0) : s0 + ol * (s0 - sig[l - 1]);
    const float fx = (float)x + ox, fy = (float)y + oy, po = (float)(1 << o);
    out[0] = o;
    out[1] = l;
    out[2] = __float_as_int(fx);
    out[3] = __float_as_int(fy);
    out[4] = __float_as_int(sc);
    out[5] = __float_as_int(fabsf(resp));
    out[6] = __float_as_int(fx * po);
    out[7] = __float_as_int(fy * po);
    return true;
}

// One thread per sample of DoG levels 1..S of one octave; a block covers 256 consecutive samples
// of one level in row-major order, and the blocks of a view are numbered in (octave, level,
// chunk) order, so block sums scanned in that order give the output order of the header.
// WRITE = false: bc[view][block] = survivors of the block.  WRITE = true: bc holds the exclusive
// scan and total[view] its sum, and the survivors are written at bc + their rank in the block; a
// block without survivors, or whose first lies beyond cap, leaves at once (most do).
template <bool WRITE>
__global__ __launch_bounds__(256) void sift_detect_kernel(const float* __restrict__ pyr, int64_t per, int64_t off, int H,
                                                          int W, int o, int nchunk, int boff, int nb,
                                                          DetectParams p, const float* __restrict__ sig, int cap,
                                                          int32_t* __restrict__ bc, const int32_t* __restrict__ total,
                                                          int32_t* __restrict__ rec) {
    __shared__ int wc[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int v = blockIdx.y;
    const int64_t bi = (int64_t)v * nb + boff + blockIdx.x;
    if (WRITE) {
        const int lo = bc[bi], hi = boff + (int)blockIdx.x + 1 < nb ? bc[bi + 1] : total[v];
        if (hi == lo || lo >= cap) return;   // the same for the whole block
    }
    const int l = 1 + blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
    const int64_t hw = (int64_t)H * W, i = (int64_t)chunk * 256 + tid;
    Dog D{pyr + (int64_t)v * per + off, hw, W};
    bool keep = false;
    int32_t r[8];
    if (i < hw) {
        const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        if (sift_is_start(D, H, W, l, y, x, p)) keep = sift_refine(D, H, W, o, l, y, x, p, sig, r);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wc[wv] = __popcll(m);
    __syncthreads();
    if (!WRITE) {
        if (tid == 0) bc[bi] = wc[0] + wc[1] + wc[2] + wc[3];
    } else if (keep) {
        int64_t pos = bc[bi] + __popcll(m & ((1ull << lane) - 1ull));
        for (int j = 0; j < wv; ++j) pos += wc[j];
        if (pos < cap) {
            int32_t* dst = rec + ((int64_t)v * cap + pos) * 8;
            for (int j = 0; j < 8; ++j) dst[j] = r[j];
        }
    }
}

// Exclusive scan of n int32 in place, one block per row of `a` (row stride n); total[row] = the sum.
// A thread sums its own run of ceil(n / 256) entries, the 256 run sums are scanned in LDS, and the
// thread walks its run again: two barriers' worth of steps whatever n is.
__global__ __launch_bounds__(256) void sift_scan_kernel(int32_t* __restrict__ a, int n, int32_t* __restrict__ total) {
    __shared__ int sh[256];
    const int tid = threadIdx.x;
    a += (int64_t)blockIdx.x * n;
    const int per = (n + 255) / 256;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += a[i];
    sh[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int t = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    int run = sh[tid] - sum;
    for (int i = lo; i < hi; ++i) {
        const int val = a[i];
        a[i] = run;
        run += val;
    }
    if (tid == 255) total[blockIdx.x] = sh[255];
}

// ---- turn() and the bilinear sample ------------------------------------------------------------
__device__ __forceinline__ float sift_turn(float y, float x) {
    const float a = fabsf(x), b = fabsf(y);
    const float m = fmaxf(a, b);
    const float t = m == 0.0f ? 0.0f : fminf(a, b) / m;
    const float u = t * t;
    float p = 0x1.b4a748p-9f * u + -0x1.bd6ba4p-7f;
    p = p * u + 0x1.d67172p-6f;
    p = p * u + -0x1.aec82ap-5f;
    p = p * u + 0x1.45e8e8p-3f;
    p = p * t;
    if (b > a) p = 0.25f - p;
    if (__float_as_uint(x) >> 31) p = 0.5f - p;
    if (__float_as_uint(y) >> 31) p = 1.0f - p;
    if (p >= 1.0f) p = 0.0f;
    return p;
}

__device__ __forceinline__ float sift_sample(const float* __restrict__ G, int H, int W, float px, float py) {
    const float x0 = floorf(px), y0 = floorf(py);
    const float fx = px - x0, fy = py - y0;
    const int xi = (int)fminf(fmaxf(x0, -1.0f), (float)W), yi = (int)fminf(fmaxf(y0, -1.0f), (float)H);
    const int i0 = clampi(xi, 0, W - 1), i1 = clampi(xi + 1, 0, W - 1);
    const int j0 = clampi(yi, 0, H - 1), j1 = clampi(yi + 1, 0, H - 1);
    const float* r0 = G + (int64_t)j0 * W;
    const float* r1 = G + (int64_t)j1 * W;
    const float top = r0[i0] * (1.0f - fx) + r0[i1] * fx;
    const float bot = r1[i0] * (1.0f - fx) + r1[i1] * fx;
    return top * (1.0f - fy) + bot * fy;
}

struct RecView {
    int o, l, q;
    float x, y, sc;
    bool ok;
};

__device__ __forceinline__ RecView sift_read_rec(const int32_t* r, int O) {
    RecView k;
    k.o = r[0];
    k.l = r[1] & 0xff;
    k.q = (r[1] >> 8) & 1023;
    k.x = __int_as_float(r[2]);
    k.y = __int_as_float(r[3]);
    k.sc = __int_as_float(r[4]);
    // a record outside the contract reads nothing: octave and level in range, x, y and the scale
    // finite and at most 2^20 in magnitude, the scale positive (a NaN fails every comparison)
    k.ok = k.o >= 0 && k.o < O && k.l >= 1 && k.l <= kS && fabsf(k.x) <= 1048576.0f && fabsf(k.y) <= 1048576.0f &&
           k.sc > 0.0f && k.sc <= 1048576.0f;
    return k;
}

// ---- 3 orient ---------------------------------------------------------------------------------
// One wave (a 64-thread block) per record: the 19 x 19 patch in LDS, an integer histogram by LDS
// atomics (integers: any order gives the same sum), lanes 0..35 smooth and test their bin.
// Writes npk[v][k] (0..4) and pk[v][k][4] (the quantised orientations in ascending bin order).
__global__ __launch_bounds__(64) void sift_orient_kernel(const float* __restrict__ pyr, Pyr P,
                                                         const int32_t* __restrict__ rec,
                                                         const int32_t* __restrict__ count, int cap,
                                                         const float* __restrict__ wo, int32_t* __restrict__ npk,
                                                         int32_t* __restrict__ pk) {
    __shared__ float patch[19 * 19];
    __shared__ int ih[36];
    __shared__ float hf[2][36];
    const int lane = threadIdx.x, v = blockIdx.y, k = blockIdx.x;
    const int n = min(count[v], cap);
    if (k >= n) return;   // the whole block leaves together
    const RecView r = sift_read_rec(rec + ((int64_t)v * cap + k) * 8, P.O);
    const int64_t slot = (int64_t)v * cap + k;
    if (!r.ok) {
        if (lane == 0) npk[slot] = 0;
        return;
    }
    const int H = P.h[r.o], W = P.w[r.o];
    const float* G = pyr + (int64_t)v * P.per + P.off[r.o] + (int64_t)r.l * H * W;
    const float h = (r.sc * 4.5f) * 0.125f;
    for (int idx = lane; idx < 361; idx += 64) {
        const int i = idx / 19, j = idx - i * 19;
        patch[idx] = sift_sample(G, H, W, r.x + (float)(j - 9) * h, r.y + (float)(i - 9) * h);
    }
    if (lane < 36) ih[lane] = 0;
    __syncthreads();
    for (int idx = lane; idx < 289; idx += 64) {
        const int a = idx / 17, b = idx - a * 17;
        const int i = a + 1, j = b + 1;
        const float gx = patch[i * 19 + j + 1] - patch[i * 19 + j - 1];
        const float gy = patch[(i + 1) * 19 + j] - patch[(i - 1) * 19 + j];
        const float w = sqrtf(gx * gx + gy * gy) * wo[idx];
        const int bin = min((int)floorf(sift_turn(gy, gx) * 36.0f), 35);
        atomicAdd(&ih[bin], (int)rintf(fminf(w * 1024.0f, 4194304.0f)));
    }
    __syncthreads();
    if (lane < 36) hf[0][lane] = (float)ih[lane];
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        if (lane < 36) {
            const float* s = hf[pass];
            const float val = (s[(lane + 35) % 36] + s[(lane + 1) % 36]) * 0.25f + s[lane] * 0.5f;
            if (pass == 0) hf[1][lane] = val;
            else ih[lane] = __float_as_int(val);
        }
        __syncthreads();
    }
    // the twice-smoothed histogram now sits in ih as float bits
    bool peak = false;
    int q = 0;
    if (lane < 36) {
        float M = __int_as_float(ih[0]);
        for (int b = 1; b < 36; ++b) M = fmaxf(M, __int_as_float(ih[b]));
        const float c = __int_as_float(ih[lane]);
        const float lf = __int_as_float(ih[(lane + 35) % 36]), rt = __int_as_float(ih[(lane + 1) % 36]);
        peak = c > lf && c > rt && c >= 0.8f * M;
        if (peak) {
            const float bf = ((float)lane + 0.5f) + 0.5f * (lf - rt) / ((lf - 2.0f * c) + rt);
            q = ((int)rintf((bf * 1024.0f) / 36.0f)) & 1023;
        }
    }
    const unsigned long long m = __ballot(peak);
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    if (peak && rank < 4) pk[slot * 4 + rank] = q;
    if (lane == 0) npk[slot] = min(__popcll(m), 4);
}

// One block per view: scans npk over the records in input order and writes the oriented records.
__global__ __launch_bounds__(256) void sift_orient_emit_kernel(const int32_t* __restrict__ rec,
                                                               const int32_t* __restrict__ count, int cap,
                                                               const int32_t* __restrict__ npk,
                                                               const int32_t* __restrict__ pk, int cap_o,
                                                               int32_t* __restrict__ orec, int32_t* __restrict__ ocount) {
    __shared__ int sh[256];
    __shared__ int run;
    const int tid = threadIdx.x, v = blockIdx.x;
    const int n = min(count[v], cap);
    if (tid == 0) run = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int k = c0 + tid;
        const int64_t slot = (int64_t)v * cap + k;
        const int val = k < n ? npk[slot] : 0;
        sh[tid] = val;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int t = tid >= d ? sh[tid - d] : 0;
            __syncthreads();
            sh[tid] += t;
            __syncthreads();
        }
        const int base = run + sh[tid] - val;
        for (int j = 0; j < val; ++j) {
            const int64_t pos = (int64_t)base + j;
            if (pos < cap_o) {
                const int32_t* s = rec + slot * 8;
                int32_t* d = orec + ((int64_t)v * cap_o + pos) * 8;
                d[0] = s[0];
                d[1] = (s[1] & 0xff) | (pk[slot * 4 + j] << 8);
                for (int w = 2; w < 8; ++w) d[w] = s[w];
            }
        }
        __syncthreads();
        if (tid == 255) run += sh[255];
        __syncthreads();
    }
    if (tid == 0) ocount[v] = run;
}

// ---- 4 describe -------------------------------------------------------------------------------
// One wave per oriented record: the 18 x 18 rotated patch in LDS, then per sample its weighted
// magnitude and orientation pair, then a lane per two histogram bins gathering its 8 x 8 support
// in row-major order (the order of the header), then the two normalisations.
__global__ __launch_bounds__(64) void sift_describe_kernel(const float* __restrict__ pyr, Pyr P,
                                                           const int32_t* __restrict__ orec,
                                                           const int32_t* __restrict__ ocount, int cap_o,
                                                           const float* __restrict__ wd, const float* __restrict__ cw,
                                                           const float* __restrict__ cs, uint8_t* __restrict__ desc) {
    __shared__ float patch[18 * 18];
    __shared__ float mw[256], fo[256];
    __shared__ int o0[256];
    __shared__ float cws[64];
    __shared__ float d[128];
    const int lane = threadIdx.x, v = blockIdx.y, k = blockIdx.x;
    const int n = min(ocount[v], cap_o);
    if (k >= n) return;
    const int64_t slot = (int64_t)v * cap_o + k;
    const RecView r = sift_read_rec(orec + slot * 8, P.O);
    uint8_t* out = desc + slot * 128;
    if (!r.ok) {
        out[lane] = 0;
        out[lane + 64] = 0;
        return;
    }
    const int H = P.h[r.o], W = P.w[r.o];
    const float* G = pyr + (int64_t)v * P.per + P.off[r.o] + (int64_t)r.l * H * W;
    const float c = cs[2 * r.q], s = cs[2 * r.q + 1];
    const float h = (r.sc * 12.0f) * 0.0625f;
    cws[lane] = cw[lane];
    for (int idx = lane; idx < 324; idx += 64) {
        const int i = idx / 18, j = idx - i * 18;
        const float u = (float)j - 8.5f, w = (float)i - 8.5f;
        patch[idx] = sift_sample(G, H, W, r.x + ((u * c) - (w * s)) * h, r.y + ((u * s) + (w * c)) * h);
    }
    __syncthreads();
    for (int idx = lane; idx < 256; idx += 64) {
        const int a = idx >> 4, b = idx & 15;
        const int i = a + 1, j = b + 1;
        const float gx = patch[i * 18 + j + 1] - patch[i * 18 + j - 1];
        const float gy = patch[(i + 1) * 18 + j] - patch[(i - 1) * 18 + j];
        mw[idx] = sqrtf(gx * gx + gy * gy) * wd[idx];
        const float ob = sift_turn(gy, gx) * 8.0f;
        const float f0 = floorf(ob);
        fo[idx] = ob - f0;
        o0[idx] = (int)f0 & 7;
    }
    __syncthreads();
    for (int bin = lane; bin < 128; bin += 64) {
        const int ky = bin >> 5, kx = (bin >> 3) & 3, o = bin & 7;
        const int a0 = max(4 * ky - 2, 0), a1 = min(4 * ky + 5, 15);   // the support of cw[ky]
        const int b0 = max(4 * kx - 2, 0), b1 = min(4 * kx + 5, 15);
        float acc = 0.0f;
        for (int a = a0; a <= a1; ++a) {
            const float wa = cws[ky * 16 + a];
            for (int b = b0; b <= b1; ++b) {
                const int idx = a * 16 + b;
                const int oo = o0[idx];
                float wgt;
                if (o == oo) wgt = 1.0f - fo[idx];
                else if (o == ((oo + 1) & 7)) wgt = fo[idx];
                else continue;
                acc = acc + ((mw[idx] * wa) * cws[kx * 16 + b]) * wgt;
            }
        }
        d[bin] = acc;
    }
    __syncthreads();
    float n2 = 0.0f;
    for (int b = 0; b < 128; ++b) n2 = n2 + d[b] * d[b];
    const float nrm = sqrtf(n2);
    if (!(nrm > 0.0f)) {
        out[lane] = 0;
        out[lane + 64] = 0;
        return;   // uniform over the wave: n2 is the same in every lane
    }
    __syncthreads();
    const float e0 = fminf(d[lane] / nrm, 0.2f), e1 = fminf(d[lane + 64] / nrm, 0.2f);
    __syncthreads();
    d[lane] = e0;
    d[lane + 64] = e1;
    __syncthreads();
    float m2 = 0.0f;
    for (int b = 0; b < 128; ++b) m2 = m2 + d[b] * d[b];
    const float nr2 = sqrtf(m2);
    out[lane] = (uint8_t)fminf(rintf(512.0f * (e0 / nr2)), 255.0f);
    out[lane + 64] = (uint8_t)fminf(rintf(512.0f * (e1 / nr2)), 255.0f);
}

int check_shape(const char* fn, int V, int H, int W, int O) {
    SFMHIP_REQUIRE(V >= 0 && H >= 1 && W >= 1, "%s: bad shape (V %d, H %d, W %d)", fn, V, H, W);
    SFMHIP_REQUIRE(V <= 65535 && (int64_t)H * W < (int64_t)INT_MAX, "%s: at most 65535 views of fewer than 2^31 pixels",
                   fn);
    SFMHIP_REQUIRE(O >= 1 && O <= kMaxO && ((H < W ? H : W) >> (O - 1)) >= 1,
                   "%s: octaves %d outside [1, %d] or the last one is empty for %d x %d", fn, O, kMaxO, H, W);
    return SFMHIP_OK;
}

}  // namespace

extern "C" int sfmhip_sift_pyramid(const uint8_t* img, int V, int H, int W, int O, const float* taps,
                                   const int32_t* radii, float* pyr, void* stream) {
    const char* fn = "sfmhip_sift_pyramid";
    const int rc0 = check_shape(fn, V, H, W, O);
    if (rc0 != SFMHIP_OK) return rc0;
    SFMHIP_REQUIRE(radii, "%s: null pointer (radii)", fn);
    for (int s = 0; s < kL; ++s)
        SFMHIP_REQUIRE(radii[s] >= 0 && radii[s] <= kMaxR, "%s: radius %d of blur %d outside [0, %d]", fn, radii[s], s,
                       kMaxR);
    if (V == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(img && taps && pyr, "%s: null pointer", fn);
    const Pyr P = make_pyr(H, W, O);
    hipStream_t st = as_stream(stream);
    for (int o = 0; o < O; ++o) {
        const int h = P.h[o], w = P.w[o];
        const int64_t hw = (int64_t)h * w;
        float* base = pyr + P.off[o];
        const dim3 grid(ceil_div(w, kTW), ceil_div(h, kTH), V);
        if (o == 0) {
            launch_blur<uint8_t>(radii[0], grid, st, img, hw, base, P.per, h, w, taps);
        } else {
            const float* prev = pyr + P.off[o - 1] + (int64_t)kS * P.h[o - 1] * P.w[o - 1];
            hipLaunchKernelGGL(sift_subsample_kernel, dim3(ceil_div(hw, 256), V), dim3(256), 0, st, prev, P.per,
                               P.h[o - 1], P.w[o - 1], base, h, w);
        }
        for (int s = 1; s < kL; ++s)
            launch_blur<float>(radii[s], grid, st, base + (s - 1) * hw, P.per, base + s * hw, P.per, h, w,
                               taps + s * kTapStride);
    }
    return check_launch("sift_blur_kernel");
}

extern "C" int sfmhip_sift_detect(const float* pyr, int V, int H, int W, int O, const float* sig, int border,
                                  float prethresh, float contrast_thr, float edge_r, int cap, int32_t* rec,
                                  int32_t* count, void* stream) {
    const char* fn = "sfmhip_sift_detect";
    const int rc0 = check_shape(fn, V, H, W, O);
    if (rc0 != SFMHIP_OK) return rc0;
    SFMHIP_REQUIRE(border >= 1 && cap >= 0, "%s: border %d must be >= 1 and cap %d >= 0", fn, border, cap);
    if (V == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(pyr && sig && count && (rec || cap == 0), "%s: null pointer", fn);
    const Pyr P = make_pyr(H, W, O);
    int nchunk[kMaxO], boff[kMaxO], nb = 0;
    for (int o = 0; o < O; ++o) {
        nchunk[o] = ceil_div((int64_t)P.h[o] * P.w[o], 256);
        boff[o] = nb;
        nb += kS * nchunk[o];
    }
    hipStream_t st = as_stream(stream);
    void* sc = nullptr;
    hipError_t e = scratch_alloc(&sc, (size_t)V * nb * sizeof(int32_t), st);
    if (e != hipSuccess) {
        set_error("%s: scratch: %s", fn, hipGetErrorString(e));
        return SFMHIP_E_HIP;
    }
    int32_t* bc = static_cast<int32_t*>(sc);
    const DetectParams p{border, prethresh, contrast_thr, edge_r};
    for (int o = 0; o < O; ++o)
        hipLaunchKernelGGL(sift_detect_kernel<false>, dim3(kS * nchunk[o], V), dim3(256), 0, st, pyr, P.per, P.off[o],
                           P.h[o], P.w[o], o, nchunk[o], boff[o], nb, p, sig, cap, bc, count, rec);
    hipLaunchKernelGGL(sift_scan_kernel, dim3(V), dim3(256), 0, st, bc, nb, count);
    if (cap > 0)
        for (int o = 0; o < O; ++o)
            hipLaunchKernelGGL(sift_detect_kernel<true>, dim3(kS * nchunk[o], V), dim3(256), 0, st, pyr, P.per,
                               P.off[o], P.h[o], P.w[o], o, nchunk[o], boff[o], nb, p, sig, cap, bc, count, rec);
    const int rc = check_launch("sift_detect_kernel");
    scratch_free(sc, st);
    return rc;
}

extern "C" int sfmhip_sift_orient(const float* pyr, int V, int H, int W, int O, const int32_t* rec,
                                  const int32_t* count, int cap, const float* wo, int cap_o, int32_t* orec,
                                  int32_t* ocount, void* stream) {
    const char* fn = "sfmhip_sift_orient";
    const int rc0 = check_shape(fn, V, H, W, O);
    if (rc0 != SFMHIP_OK) return rc0;
    SFMHIP_REQUIRE(cap >= 0 && cap_o >= 0, "%s: cap %d and cap_o %d must be >= 0", fn, cap, cap_o);
    SFMHIP_REQUIRE((int64_t)V * cap < (int64_t)INT_MAX / 8 && (int64_t)V * cap_o < (int64_t)INT_MAX / 8,
                   "%s: V cap and V cap_o must stay below 2^28", fn);
    if (V == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(pyr && count && ocount && wo && (rec || cap == 0) && (orec || cap_o == 0), "%s: null pointer", fn);
    const Pyr P = make_pyr(H, W, O);
    hipStream_t st = as_stream(stream);
    void* sc = nullptr;
    hipError_t e = scratch_alloc(&sc, ((size_t)V * cap * 5 + 4) * sizeof(int32_t), st);
    if (e != hipSuccess) {
        set_error("%s: scratch: %s", fn, hipGetErrorString(e));
        return SFMHIP_E_HIP;
    }
    int32_t* npk = static_cast<int32_t*>(sc);
    int32_t* pk = npk + (size_t)V * cap;
    if (cap > 0)
        hipLaunchKernelGGL(sift_orient_kernel, dim3(cap, V), dim3(64), 0, st, pyr, P, rec, count, cap, wo, npk, pk);
    hipLaunchKernelGGL(sift_orient_emit_kernel, dim3(V), dim3(256), 0, st, rec, count, cap, npk, pk, cap_o, orec,
                       ocount);
    const int rc = check_launch("sift_orient_kernel");
    scratch_free(sc, st);
    return rc;
}

extern "C" int sfmhip_sift_describe(const float* pyr, int V, int H, int W, int O, const int32_t* orec,
                                    const int32_t* ocount, int cap_o, const float* wd, const float* cw,
                                    const float* cs, uint8_t* desc, void* stream) {
    const char* fn = "sfmhip_sift_describe";
    const int rc0 = check_shape(fn, V, H, W, O);
    if (rc0 != SFMHIP_OK) return rc0;
    SFMHIP_REQUIRE(cap_o >= 0 && (int64_t)V * cap_o < (int64_t)INT_MAX / 128, "%s: cap_o %d: V cap_o must be in [0, 2^24)",
                   fn, cap_o);
    if (V == 0 || cap_o == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(pyr && orec && ocount && wd && cw && cs && desc, "%s: null pointer", fn);
    const Pyr P = make_pyr(H, W, O);
    hipLaunchKernelGGL(sift_describe_kernel, dim3(cap_o, V), dim3(64), 0, as_stream(stream), pyr, P, orec, ocount,
                       cap_o, wd, cw, cs, desc);
    return check_launch("sift_describe_kernel");
}
