// mfma_mx_peak.hip — diagnostic: the rate this MI355X sustains for the
// matcher's per-pair work (16x16 output tiles, 4 independent chains per wave, d = 256 per
// distance) on block-scaled FP6 (e2m3) / FP4 (e2m1) MFMAs — v_mfma_scale_f32_16x16x128_f8f6f4,
// two k-steps of 128 per distance — against today's int8 form (v_mfma_i32_16x16x64_i8, four
// k-steps of 64), each with and without the top-2 epilogue per output element.  The MX
// epilogue first converts the f32 dot to an integer key (one v_cvt per distance), then runs
// the int8 form's two-candidate top-2 (max3 + med3 + max).  No LDS, no global traffic in the
// loop: the ceiling the match kernel would be bound by.  The operands pass through an empty
// asm each iteration so that the compiler cannot hoist the (pure) scaled MFMAs out of the loop
// (it did: a first build measured 22-105 POPS).
// EPI 2 is the value-only match kernel's loop epilogue (group maxima, DESIGN K1'): every chain
// starts from a per-tile vector (the kernel's h_j), each tile takes the maximum of its 4 values
// per chain (2 max3), and every 4th tile merges that maximum into a running top two with the
// range id where the best rose (cmp + select + med3 + max).  The int8 arm runs it in i32, the
// FP6 arm in f32 with no conversion; with this epilogue the FP6 operands are e2m3 codes under the
// unit block scale 2^3 (scale byte 130 in every byte: the product of two codes g/8 is the
// integer g_a g_b), the form an FP6 certified filter would run.
// Build: hipcc -O3 --offload-arch=gfx950 -o tools/mfma_mx_peak tools/mfma_mx_peak.hip
// Run:   tools/mfma_mx_peak ITERS   (a multiple of 4)
//        tools/mfma_mx_peak ITERS tile8   (a multiple of 8): only the two arms of kern_fp6_tile8
//        tools/mfma_mx_peak ITERS unscaled   the gate of DESIGN K1'' round 12: first the numerics of the FP6
//                                         MFMA with both scales 0 (the compiler then emits the plain 8-byte
//                                         v_mfma_f32_16x16x128_f8f6f4) on codes of known grid values, then
//                                         the scaled and unscaled forms of kern_fp6_tile8 and of the 32x32x64
//                                         shape, interleaved
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../3d_reconstruction_amd/csrc/fp6_sched.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int max3i(int a, int b, int c) {
    int r;
    asm("v_max3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ int med3i(int a, int b, int c) {
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// today's form: 4 chains x 4 k-steps of v_mfma_i32_16x16x64_i8 per distance tile
template <int EPI>   // 0 none, 1 per-distance top two, 2 group maxima
__global__ __launch_bounds__(256, 2) void kern_i8(const int* __restrict__ seed, int iters, int* out) {
    const int lane = threadIdx.x & 63;
    i32x4 a[4], b[4][4];
    for (int k = 0; k < 4; ++k)
        for (int e = 0; e < 4; ++e) {
            a[k][e] = seed[(blockIdx.x * 97 + lane * 13 + k * 7 + e) & 4095];
            for (int t = 0; t < 4; ++t) b[t][k][e] = seed[(blockIdx.x * 31 + lane * 5 + k * 11 + e * 3 + t * 17) & 4095];
        }
    int t1[4] = {INT_MIN, INT_MIN, INT_MIN, INT_MIN}, t2[4] = {INT_MIN, INT_MIN, INT_MIN, INT_MIN};
    int kv = seed[lane];
    i32x4 hv;
    for (int e = 0; e < 4; ++e) hv[e] = EPI == 2 ? seed[(lane * 3 + e) & 4095] >> 9 : 0;
    int rm[4], wr[4] = {0, 0, 0, 0};
    for (int it = 0; it < iters; it += 4) {
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            // opaque to the compiler: the operands "change" every iteration (no hoisted MFMAs)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                asm volatile("" : "+v"(a[k]));
#pragma unroll
                for (int t = 0; t < 4; ++t) asm volatile("" : "+v"(b[t][k]));
            }
            if (EPI == 2) asm volatile("" : "+v"(hv));
            i32x4 acc[4] = {hv, hv, hv, hv};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[k], b[t][k], acc[t], 0, 0, 0);
            if (EPI == 1) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int q = 0; q < 4; q += 2) {
                        const int ka = acc[t][q] * 256 + kv, kb = acc[t][q + 1] * 256 + kv + 1;
                        const int m = med3i(t1[t], ka, kb);
                        t1[t] = max3i(t1[t], ka, kb);
                        t2[t] = max(t2[t], m);
                    }
            } else if (EPI == 2) {
                // the accumulators' first reader is plain C++ (match.hip, match_fp6.hip: stale values through inline asm)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (jt == 0) rm[t] = INT_MIN;
                    rm[t] = max(max(rm[t], acc[t][0]), acc[t][1]);
                    rm[t] = max(max(rm[t], acc[t][2]), acc[t][3]);
                }
                if (jt == 3) {
                    const int rid = it >> 2;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        wr[t] = rm[t] > t1[t] ? rid : wr[t];
                        t2[t] = med3i(t1[t], t2[t], rm[t]);
                        t1[t] = max(t1[t], rm[t]);
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) t1[t] ^= acc[t][lane & 3];
            }
            kv += 1;
        }
    }
    if (EPI == 2) t1[0] += wr[0] + wr[1] + wr[2] + wr[3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = t1[0] + t2[0] + t1[1] + t2[1] + t1[2] + t2[2] + t1[3] + t2[3];
}

// block-scaled MX: FMT 2 = fp6 e2m3, 4 = fp4 e2m1; 4 chains x 2 k-steps of 128 per distance tile
template <int FMT, int EPI>
__global__ __launch_bounds__(256, 2) void kern_mx(const int* __restrict__ seed, int iters, int* out) {
    const int lane = threadIdx.x & 63;
    i32x8 a[2], b[4][2];
    for (int k = 0; k < 2; ++k)
        for (int e = 0; e < 8; ++e) {
            a[k][e] = seed[(blockIdx.x * 97 + lane * 13 + k * 7 + e) & 4095];
            for (int t = 0; t < 4; ++t) b[t][k][e] = seed[(blockIdx.x * 31 + lane * 5 + k * 11 + e * 3 + t * 17) & 4095];
        }
    // E8M0 block scales: 2^-7 .. 2^0, or the unit scale 2^3 of the integer grid (EPI 2)
    const int sa = EPI == 2 ? (int)0x82828282 : 120 + (lane & 7), sb = EPI == 2 ? (int)0x82828282 : 121 + (lane & 3);
    int t1[4] = {INT_MIN, INT_MIN, INT_MIN, INT_MIN}, t2[4] = {INT_MIN, INT_MIN, INT_MIN, INT_MIN};
    int kv = seed[lane];
    f32x4 hv;
    for (int e = 0; e < 4; ++e) hv[e] = EPI == 2 ? (float)(seed[(lane * 3 + e) & 4095] >> 9) : 0.f;
    const float kLow = -16777216.f;   // below every value: |dot| <= 256 * 60^2, h >= -2^23
    float f1[4] = {kLow, kLow, kLow, kLow}, f2[4] = {kLow, kLow, kLow, kLow}, rm[4];
    int wr[4] = {0, 0, 0, 0};
    for (int it = 0; it < iters; it += 4) {
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                asm volatile("" : "+v"(a[k]));
#pragma unroll
                for (int t = 0; t < 4; ++t) asm volatile("" : "+v"(b[t][k]));
            }
            if (EPI == 2) asm volatile("" : "+v"(hv));
            f32x4 acc[4] = {hv, hv, hv, hv};
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[k], b[t][k], acc[t], FMT, FMT, 0, sa, 0,
                                                                              sb);
            if (EPI == 1) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int q = 0; q < 4; q += 2) {
                        const int ka = (int)acc[t][q] * 256 + kv, kb = (int)acc[t][q + 1] * 256 + kv + 1;
                        const int m = med3i(t1[t], ka, kb);
                        t1[t] = max3i(t1[t], ka, kb);
                        t2[t] = max(t2[t], m);
                    }
            } else if (EPI == 2) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (jt == 0) rm[t] = kLow;
                    rm[t] = __builtin_fmaxf(__builtin_fmaxf(rm[t], acc[t][0]), acc[t][1]);
                    rm[t] = __builtin_fmaxf(__builtin_fmaxf(rm[t], acc[t][2]), acc[t][3]);
                }
                if (jt == 3) {
                    const int rid = it >> 2;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const bool up = rm[t] > f1[t];   // one compare serves the range id and the maximum
                        wr[t] = up ? rid : wr[t];
                        f2[t] = __builtin_amdgcn_fmed3f(f1[t], f2[t], rm[t]);
                        f1[t] = up ? rm[t] : f1[t];
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) t1[t] ^= __float_as_int(acc[t][lane & 3]);
            }
            kv += 1;
        }
    }
    if (EPI == 2)
        for (int t = 0; t < 4; ++t) { t1[t] = (int)f1[t] + wr[t]; t2[t] = (int)f2[t]; }
    out[blockIdx.x * blockDim.x + threadIdx.x] = t1[0] + t2[0] + t1[1] + t2[1] + t1[2] + t2[2] + t1[3] + t2[3];
}

// The FP6 match kernel's real shape (match_fp6.hip, match_fp6_kernel<256>): 8 chains per wave, two k-steps per
// tile, 6-register operands, the f32 group-max epilogue with the per-range merge every 4th tile, unit
// scale, 2 waves per SIMD.  PIPE 0: the tile's 16 MFMAs, then its 16 max3, then (every 4th tile) the 32
// merge instructions, in the order the compiler chooses (clustered).  PIPE 1: the same instructions in the
// order of the kernel's own Fp6Sched<2, 8> (csrc/fp6_sched.h): chain s's two max3 in gaps 13 + s and 14 + s
// of its tile (five MFMAs behind the chain's last, the last chains under the next tile's first MFMAs), the
// merge of a finished range in the free slots of the next range's first two tiles, at most two VALU per
// gap; every gap is closed by a scheduling barrier, so the source order is the issue order.
typedef int i32x2 __attribute__((ext_vector_type(2)));
struct Op6 {
    i32x4 lo;
    i32x2 hi;
    __device__ i32x8 tuple() const { return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], 0, 0}; }
    __device__ void set(int e, int x) { if (e < 4) lo[e] = x; else hi[e - 4] = x; }
};
// SCALED 1: unit block scale 2^3 on both sides, integer products.  SCALED 0: both scales 0, which the compiler
// emits as the unscaled instruction; the products are g_a g_b / 64, so the chain starts and kLow are divided by
// 64 and the top two multiplied by 64 at the end (all exact): the checksum is the scaled form's.
template <int PIPE, int SCALED = 1>
__global__ __launch_bounds__(256, 2) void kern_fp6_tile8(const int* __restrict__ seed, int iters, int* out) {
    constexpr int NS = 8, KK = 2, VG = 4;
    using SC = sfmhip::Fp6Sched<KK, NS>;
    constexpr int kScale = SCALED ? (int)0x82828282 : 0;
    constexpr float kUnit = SCALED ? 1.f : 0.015625f, kBack = SCALED ? 1.f : 64.f;
    const float kLow = -16777216.f * kUnit;
    const int lane = threadIdx.x & 63;
    Op6 a[KK], b[NS][KK];   // 32 codes = 24 bytes in 6 registers, as the kernel holds them
#pragma unroll
    for (int k = 0; k < KK; ++k)
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            a[k].set(e, seed[(blockIdx.x * 97 + lane * 13 + k * 7 + e) & 4095]);
#pragma unroll
            for (int t = 0; t < NS; ++t) b[t][k].set(e, seed[(blockIdx.x * 31 + lane * 5 + k * 11 + e * 3 + t * 17) & 4095]);
        }
    f32x4 hv;
    for (int e = 0; e < 4; ++e) hv[e] = (float)(seed[(lane * 3 + e) & 4095] >> 9) * kUnit;
    float f1[NS], f2[NS], rm[2][NS], half[NS];
    int wr[NS];
    bool up[NS];
    f32x4 acc[NS];
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        f1[t] = f2[t] = rm[0][t] = rm[1][t] = half[t] = kLow;
        wr[t] = 0;
        up[t] = false;
        acc[t] = f32x4{kLow, kLow, kLow, kLow};
    }
#define MERGE_STEP(c, step, m, rid) sfmhip::fp6_merge_step(step, m, rid, up[c], f1[c], f2[c], wr[c])
    int rid_owed = 0;
    for (int it = 0; it < iters; it += 2 * VG) {   // one 128-candidate block: 8 tiles, two ranges
#pragma unroll
        for (int jt = 0; jt < 2 * VG; ++jt) {
            const int R = jt / VG, tt = jt % VG;
            asm volatile("" : "+v"(hv));
            if (PIPE == 0) {
#pragma unroll
                for (int k = 0; k < KK; ++k)
                    asm volatile("" : "+v"(a[k].lo), "+v"(a[k].hi));
#pragma unroll
                for (int t = 0; t < NS; ++t) acc[t] = hv;
#pragma unroll
                for (int k = 0; k < KK; ++k)
#pragma unroll
                    for (int t = 0; t < NS; ++t)
                        acc[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[k].tuple(), b[t][k].tuple(), acc[t], 2, 2,
                                                                                  0, kScale, 0, kScale);
#pragma unroll
                for (int t = 0; t < NS; ++t) {
                    if (tt == 0) rm[0][t] = kLow;
                    rm[0][t] = __builtin_fmaxf(__builtin_fmaxf(rm[0][t], acc[t][0]), acc[t][1]);
                    rm[0][t] = __builtin_fmaxf(__builtin_fmaxf(rm[0][t], acc[t][2]), acc[t][3]);
                }
                if (tt == VG - 1) {
                    const int rid = (it >> 2) + R;
#pragma unroll
                    for (int t = 0; t < NS; ++t)
#pragma unroll
                        for (int step = 0; step < 4; ++step) MERGE_STEP(t, step, rm[0][t], rid);
                }
            } else {
#pragma unroll
                for (int k = 0; k < KK; ++k) {
                    asm volatile("" : "+v"(a[k].lo), "+v"(a[k].hi));
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int t = 0; t < NS; ++t) {
                        acc[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[k].tuple(), b[t][k].tuple(),
                                                                                  k == 0 ? hv : acc[t], 2, 2, 0, kScale, 0,
                                                                                  kScale);
                        __builtin_amdgcn_sched_barrier(0);
                        const int g = k * NS + t;
                        if (const int c = SC::chain(g, 0); c < NS) {
                            const int of = tt - SC::back(g, 0);   // the tile these maxima belong to
                            const float from = of < 0 ? rm[R ^ 1][c] : of == 0 ? kLow : rm[R][c];
                            half[c] = __builtin_fmaxf(__builtin_fmaxf(from, acc[c][0]), acc[c][1]);
                        }
                        if (const int c = SC::chain(g, 1); c < NS)
                            rm[tt == 0 && SC::back(g, 1) ? R ^ 1 : R][c] =
                                __builtin_fmaxf(__builtin_fmaxf(half[c], acc[c][2]), acc[c][3]);
#pragma unroll
                        for (int j = 0; j < SC::kBudget; ++j)
                            if (const int m = SC::merge(tt * SC::MPT + g, j); m >= 0) {
                                __builtin_amdgcn_sched_barrier(0);
                                MERGE_STEP(SC::merge_chain(m), SC::merge_step(m), rm[R ^ 1][SC::merge_chain(m)], rid_owed);
                            }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (tt == VG - 1) rid_owed = (it >> 2) + R;
            }
        }
    }
    if (PIPE == 1) {   // drain: the last tile's owed maxima and the last range's merge
#pragma unroll
        for (int t = SC::kOwedFirst; t < NS; ++t) half[t] = __builtin_fmaxf(__builtin_fmaxf(rm[1][t], acc[t][0]), acc[t][1]);
#pragma unroll
        for (int t = SC::kOwedSecond; t < NS; ++t) rm[1][t] = __builtin_fmaxf(__builtin_fmaxf(half[t], acc[t][2]), acc[t][3]);
#pragma unroll
        for (int t = 0; t < NS; ++t)
#pragma unroll
            for (int step = 0; step < 4; ++step) MERGE_STEP(t, step, rm[1][t], rid_owed);
    }
    int r = 0;
#pragma unroll
    for (int t = 0; t < NS; ++t) r += (int)(f1[t] * kBack) + (int)(f2[t] * kBack) + wr[t];
#undef MERGE_STEP
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;   // the same value in every arm
}

// The same output area per wave (2048 distances of d = 256 per tile step) on v_mfma_scale_f32_32x32x64_f8f6f4:
// 2 chains x 4 k-steps, the candidates on the 16 accumulator registers, so a tile's maxima are 8 max3 per
// chain and a range's merge 4 instructions per chain.  Compiler order.  Measured for the record only.
typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int SCALED>
__global__ __launch_bounds__(256, 2) void kern_fp6_32x32(const int* __restrict__ seed, int iters, int* out) {
    constexpr int NS = 2, KK = 4, VG = 4;
    constexpr int kScale = SCALED ? (int)0x82828282 : 0;
    constexpr float kUnit = SCALED ? 1.f : 0.015625f, kBack = SCALED ? 1.f : 64.f;
    const float kLow = -16777216.f * kUnit;
    const int lane = threadIdx.x & 63;
    Op6 a[KK], b[NS][KK];
#pragma unroll
    for (int k = 0; k < KK; ++k)
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            a[k].set(e, seed[(blockIdx.x * 97 + lane * 13 + k * 7 + e) & 4095]);
#pragma unroll
            for (int t = 0; t < NS; ++t) b[t][k].set(e, seed[(blockIdx.x * 31 + lane * 5 + k * 11 + e * 3 + t * 17) & 4095]);
        }
    f32x16 hv;
    for (int e = 0; e < 16; ++e) hv[e] = (float)(seed[(lane * 3 + e) & 4095] >> 9) * kUnit;
    float f1[NS], f2[NS], rm[NS];
    int wr[NS];
    bool up[NS];
#pragma unroll
    for (int t = 0; t < NS; ++t) { f1[t] = f2[t] = rm[t] = kLow; wr[t] = 0; up[t] = false; }
    for (int it = 0; it < iters; it += 2 * VG) {
#pragma unroll
        for (int jt = 0; jt < 2 * VG; ++jt) {
            const int R = jt / VG, tt = jt % VG;
            asm volatile("" : "+v"(hv));
#pragma unroll
            for (int k = 0; k < KK; ++k) asm volatile("" : "+v"(a[k].lo), "+v"(a[k].hi));
            f32x16 acc[NS];
#pragma unroll
            for (int t = 0; t < NS; ++t) acc[t] = hv;
#pragma unroll
            for (int k = 0; k < KK; ++k)
#pragma unroll
                for (int t = 0; t < NS; ++t)
                    acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[k].tuple(), b[t][k].tuple(), acc[t], 2, 2, 0,
                                                                             kScale, 0, kScale);
#pragma unroll
            for (int t = 0; t < NS; ++t) {
                if (tt == 0) rm[t] = kLow;
#pragma unroll
                for (int e = 0; e < 16; e += 2) rm[t] = __builtin_fmaxf(__builtin_fmaxf(rm[t], acc[t][e]), acc[t][e + 1]);
            }
            if (tt == VG - 1) {
                const int rid = (it >> 2) + R;
#pragma unroll
                for (int t = 0; t < NS; ++t)
#pragma unroll
                    for (int step = 0; step < 4; ++step) sfmhip::fp6_merge_step(step, rm[t], rid, up[t], f1[t], f2[t], wr[t]);
            }
        }
    }
    int r = 0;
#pragma unroll
    for (int t = 0; t < NS; ++t) r += (int)(f1[t] * kBack) + (int)(f2[t] * kBack) + wr[t];
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

// Numerics of one 16 x 16 x 256 tile (two chained MFMAs, as the kernel's KK = 2) on codes the host chose:
// lane (grp, lr) gives codes 32 grp .. 32 grp + 31 of k-step k of row lr on both sides; the chains start from
// c0[row]; out[row][col], row = 4 grp + register (the A side), col = lr (the B side).
template <int SCALED>
__global__ void kern_fp6_check(const int* __restrict__ ca, const int* __restrict__ cb, const float* __restrict__ c0,
                               float* __restrict__ out) {
    constexpr int kScale = SCALED ? (int)0x82828282 : 0;
    const int lane = threadIdx.x & 63, grp = lane / 16, lr = lane % 16;
    Op6 a[2], b[2];
    for (int k = 0; k < 2; ++k)
        for (int e = 0; e < 6; ++e) {
            a[k].set(e, ca[((lr * 2 + k) * 4 + grp) * 6 + e]);
            b[k].set(e, cb[((lr * 2 + k) * 4 + grp) * 6 + e]);
        }
    f32x4 acc;
    for (int e = 0; e < 4; ++e) acc[e] = c0[4 * grp + e];
    for (int k = 0; k < 2; ++k)
        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[k].tuple(), b[k].tuple(), acc, 2, 2, 0, kScale, 0, kScale);
    for (int e = 0; e < 4; ++e) out[(4 * grp + e) * 16 + lr] = acc[e];
}

// grid value g (value g / 8) of an e2m3 code
static int fp6_g(int code) {
    const int n = code & 31, ex = n >> 3, m = n & 7;
    const int g = ex == 0 ? m : (8 + m) << (ex - 1);
    return code & 32 ? -g : g;
}

// Every output of the form with the given scale argument must equal (sum g_a g_b) * unit + c0 exactly.
// Rows 0 / 1 hold +60 / -60 throughout (|dot| = 921,600 at both signs), row 2 alternates them, the rest are
// random codes; c0 runs from -2^23 (the padded rows' start) upwards, in the form's unit.
static int check_numerics(int scaled) {
    static int code[2][16][256];
    unsigned x = 2463534242u;
    for (int side = 0; side < 2; ++side)
        for (int r = 0; r < 16; ++r)
            for (int k = 0; k < 256; ++k) {
                x = x * 1664525u + 1013904223u;
                code[side][r][k] = r == 0 ? 31 : r == 1 ? 63 : r == 2 ? (k & 1 ? 63 : 31) : (int)(x >> 26);
            }
    const double unit = scaled ? 1.0 : 1.0 / 64;
    static int packed[2][16 * 2 * 4 * 6];
    memset(packed, 0, sizeof(packed));
    for (int side = 0; side < 2; ++side)
        for (int r = 0; r < 16; ++r)
            for (int k = 0; k < 256; ++k) {   // code e of a 32-chunk at bits 6 e .. 6 e + 5 of its 24 bytes
                const int chunk = k / 32, e = k % 32, bit = 6 * e;
                unsigned char* bytes = reinterpret_cast<unsigned char*>(&packed[side][(r * 8 + chunk) * 6]);
                const unsigned v = (unsigned)code[side][r][k] << (bit & 7);
                bytes[bit >> 3] |= v & 0xff;
                if (v >> 8) bytes[(bit >> 3) + 1] |= v >> 8;
            }
    float c0[16], host[256];
    for (int r = 0; r < 16; ++r) c0[r] = (float)((r == 3 ? -8388608.0 : r == 4 ? 0.0 : -(double)(r * 524287 % 8388608)) * unit);
    int *da, *db;
    float *dc, *dout;
    hipMalloc(&da, sizeof(packed[0]));
    hipMalloc(&db, sizeof(packed[1]));
    hipMalloc(&dc, sizeof(c0));
    hipMalloc(&dout, sizeof(host));
    hipMemcpy(da, packed[0], sizeof(packed[0]), hipMemcpyHostToDevice);
    hipMemcpy(db, packed[1], sizeof(packed[1]), hipMemcpyHostToDevice);
    hipMemcpy(dc, c0, sizeof(c0), hipMemcpyHostToDevice);
    if (scaled) hipLaunchKernelGGL(kern_fp6_check<1>, dim3(1), dim3(64), 0, 0, da, db, dc, dout);
    else hipLaunchKernelGGL(kern_fp6_check<0>, dim3(1), dim3(64), 0, 0, da, db, dc, dout);
    if (hipMemcpy(host, dout, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess) { printf("check launch failed\n"); return 1; }
    int bad = 0;
    double ratio_lo = 1e300, ratio_hi = -1e300;
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
            long long dot = 0;
            for (int k = 0; k < 256; ++k) dot += (long long)fp6_g(code[0][i][k]) * fp6_g(code[1][j][k]);
            const double want = (double)dot * unit + (double)c0[i];   // exact in double
            const double got = (double)host[i * 16 + j];
            if (got != want) {
                if (bad++ < 8) printf("  MISMATCH [%d][%d]: dot %lld start %.6f want %.6f got %.6f\n", i, j, dot, (double)c0[i], want, got);
            }
            if (dot != 0) {   // the factor the hardware put on g_a g_b
                const double ratio = (got - (double)c0[i]) / (double)dot;
                ratio_lo = ratio < ratio_lo ? ratio : ratio_lo;
                ratio_hi = ratio > ratio_hi ? ratio : ratio_hi;
            }
        }
    printf("numerics, %s: out[0][0] %.6f (dot 921600) out[0][1] %.6f (dot -921600); implied factor on g_a g_b in [%.10g, %.10g] "
           "(expected %.10g); %d of 256 outputs differ from (sum g_a g_b) * %g + start\n",
           scaled ? "scales 0x82828282 (scaled form)" : "scales 0 (unscaled form)", (double)host[0] - (double)c0[0],
           (double)host[1] - (double)c0[0], ratio_lo, ratio_hi, unit, bad, unit);
    hipFree(da); hipFree(db); hipFree(dc); hipFree(dout);
    return bad != 0;
}

// arms of the real shape, interleaved, REPS times each: per-arm min / median / max and the checksum
struct Arm {
    const char* name;
    void (*kern)(const int*, int, int*);
    int group;   // arms of one group compute the same checksum
};
static int run_arms(const Arm* arms, int n_arms, const int* seed, int* out, int blocks, int iters, float (*ms)[7]) {
    const int REPS = 7;
    long long sum[8] = {0};
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    int* host = (int*)malloc((size_t)blocks * 256 * 4);
    for (int rep = -1; rep < REPS; ++rep)   // rep -1 warms up
        for (int arm = 0; arm < n_arms; ++arm) {
            hipEventRecord(e0);
            hipLaunchKernelGGL(arms[arm].kern, dim3(blocks), dim3(256), 0, 0, seed, iters, out);
            hipEventRecord(e1);
            if (hipEventSynchronize(e1) != hipSuccess) { printf("launch failed\n"); return 1; }
            if (rep < 0) {
                hipMemcpy(host, out, (size_t)blocks * 256 * 4, hipMemcpyDeviceToHost);
                for (size_t i = 0; i < (size_t)blocks * 256; ++i) sum[arm] += host[i];
            } else {
                hipEventElapsedTime(&ms[arm][rep], e0, e1);
            }
        }
    free(host);
    // per wave: iters tiles x 8 chains x 16 x 16 outputs x d = 256 x 2 ops; 16 MFMAs of 16x16x128 per tile
    const double ops = (double)blocks * 4 * iters * 8.0 * 16 * 16 * 256 * 2;
    const double mfma_per_simd = (double)blocks * 4 * iters * 16 / (256.0 * 4);
    bool equal = true;
    for (int arm = 0; arm < n_arms; ++arm) {
        float* m = ms[arm];
        for (int i = 0; i < REPS; ++i)
            for (int j = i + 1; j < REPS; ++j)
                if (m[j] < m[i]) { float t = m[i]; m[i] = m[j]; m[j] = t; }
        printf("fp6 %-50s: min %.3f  median %.3f  max %.3f ms  %6.0f TOPS at the median, "
               "%.1f ns per 16x16x128 of work per SIMD, checksum %lld\n",
               arms[arm].name, m[0], m[REPS / 2], m[REPS - 1], ops / m[REPS / 2] / 1e9, m[REPS / 2] * 1e6 / mfma_per_simd,
               sum[arm]);
        for (int o = 0; o < arm; ++o)
            if (arms[o].group == arms[arm].group && sum[o] != sum[arm]) equal = false;
    }
    printf("checksums %s\n", equal ? "equal" : "DIFFER");
    return equal ? 0 : 1;
}

static int run_tile8(const int* seed, int* out, int blocks, int iters) {
    const Arm arms[2] = {{"8 chains x 2 k-steps, clustered (compiler order)", kern_fp6_tile8<0>, 0},
                         {"8 chains x 2 k-steps, pipelined (Fp6Sched order)", kern_fp6_tile8<1>, 0}};
    float ms[2][7];
    return run_arms(arms, 2, seed, out, blocks, iters, ms);
}

// The gate: numerics first (a form that does not multiply the codes as they stand closes the lever), then
// the scaled and unscaled forms interleaved.
static int run_unscaled(const int* seed, int* out, int blocks, int iters) {
    if (check_numerics(1)) { printf("the scaled form is not exact: the probe itself is wrong\n"); return 1; }
    if (check_numerics(0)) { printf("GATE: the unscaled form does not give g_a g_b / 64 exactly: lever closed\n"); return 1; }
    const Arm arms[6] = {{"16x16x128 scaled,   clustered (compiler order)", kern_fp6_tile8<0, 1>, 0},
                         {"16x16x128 unscaled, clustered (compiler order)", kern_fp6_tile8<0, 0>, 0},
                         {"16x16x128 scaled,   pipelined (Fp6Sched order)", kern_fp6_tile8<1, 1>, 0},
                         {"16x16x128 unscaled, pipelined (Fp6Sched order)", kern_fp6_tile8<1, 0>, 0},
                         {"32x32x64  scaled,   clustered (compiler order)", kern_fp6_32x32<1>, 1},
                         {"32x32x64  unscaled, clustered (compiler order)", kern_fp6_32x32<0>, 1}};
    float ms[6][7];
    if (run_arms(arms, 6, seed, out, blocks, iters, ms)) return 1;
    for (int p = 0; p < 4; p += 2)   // sorted by run_arms
        printf("GATE %s: unscaled max %.3f ms %s scaled min %.3f ms (medians %.3f vs %.3f: %+.2f %%)\n",
               p ? "pipelined" : "clustered", ms[p + 1][6], ms[p + 1][6] < ms[p][0] ? "<" : ">=", ms[p][0], ms[p + 1][3], ms[p][3],
               100.0 * (ms[p + 1][3] / ms[p][3] - 1.0));
    printf("32x32x64 against 16x16x128, scaled, medians: %.3f vs %.3f ms (%+.2f %%)\n", ms[4][3], ms[0][3],
           100.0 * (ms[4][3] / ms[0][3] - 1.0));
    return 0;
}

int main(int argc, char** argv) {
    const int blocks = 256 * 2 * 8, iters = (argc > 1 ? atoi(argv[1]) : 2000) & ~3;
    int *seed, *out;
    hipMalloc(&seed, 4096 * 4);
    hipMalloc(&out, (size_t)blocks * 256 * 4);
    int h[4096];
    unsigned x = 12345;
    for (int i = 0; i < 4096; ++i) {
        x = x * 1664525u + 1013904223u;
        h[i] = (int)x;   // uniform random bits: random int8 values, random fp6 / fp4 codes (no NaN encodings)
    }
    hipMemcpy(seed, h, sizeof(h), hipMemcpyHostToDevice);
    if (argc > 2 && !strcmp(argv[2], "tile8")) return run_tile8(seed, out, blocks, iters & ~7);
    if (argc > 2 && !strcmp(argv[2], "unscaled")) return run_unscaled(seed, out, blocks, iters & ~7);
    // per wave-iteration: 4 tiles x 16 x 16 outputs x d = 256 x 2 ops
    const double ops_iter = 4.0 * 16 * 16 * 256 * 2;
    const char* names[8] = {"int8 16x16x64 (today)", "int8 16x16x64 (today)", "fp6 e2m3 16x16x128 scaled",
                            "fp6 e2m3 16x16x128 scaled", "fp4 e2m1 16x16x128 scaled", "fp4 e2m1 16x16x128 scaled",
                            "int8 16x16x64 (today)", "fp6 e2m3 grid, scale 2^3"};
    const char* epi[8] = {"no   epilogue", "top-2 epilogue", "no   epilogue", "top-2 epilogue", "no   epilogue",
                          "top-2 epilogue", "group-max epilogue", "group-max epilogue"};
    for (int c = 0; c < 8; ++c) {
        hipEvent_t e0, e1;
        hipEventCreate(&e0);
        hipEventCreate(&e1);
        for (int rep = 0; rep < 3; ++rep) {
            hipEventRecord(e0);
#define L(K) hipLaunchKernelGGL(K, dim3(blocks), dim3(256), 0, 0, seed, iters, out)
            switch (c) {
                case 0: L((kern_i8<0>)); break;
                case 1: L((kern_i8<1>)); break;
                case 2: L((kern_mx<2, 0>)); break;
                case 3: L((kern_mx<2, 1>)); break;
                case 4: L((kern_mx<4, 0>)); break;
                case 5: L((kern_mx<4, 1>)); break;
                case 6: L((kern_i8<2>)); break;
                default: L((kern_mx<2, 2>)); break;
            }
#undef L
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            const double ops = (double)blocks * 4 * iters * ops_iter;
            if (rep == 2)
                printf("%-28s %-18s: %8.2f ms  %6.0f TOPS (%.1f%% of the 5000 int8 spec)\n", names[c], epi[c], ms,
                       ops / ms / 1e9, ops / ms / 1e9 / 50.0);
        }
    }
    return 0;
}
