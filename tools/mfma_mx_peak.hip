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
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdio>
#include <cstdlib>

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
                // the accumulators' first reader is plain C++ (match.hip: stale values through inline asm)
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
