// match_fp6.hip — the FP6 certified filter of the exact float mode (DESIGN.md K1''): the e2m3 integer
// grid (quantize_fp6_kernel), the dense operand rows (pack_fp6_kernel) and match_fp6_kernel, the
// value-only form of the matcher on v_mfma_f32_16x16x128_f8f6f4: 256 threads, 8 tiles of 16 query rows
// per wave (512 rows per workgroup), image b through the LDS ring in 128-row blocks as two dense planes.
// match_exact.hip launches it through launch_match_fp6 (match_dev.h); the block loop's instruction
// order is fp6_sched.h's.
#include "match_dev.h"
#include "fp6_sched.h"

namespace sfmhip {

// ---------------------------------------------------------------------------
// FP6 (e2m3) integer grid (DESIGN.md K1''): f32 -> g, the point of
//   G = {0..15 step 1, 16..30 step 2, 32..60 step 4} (both signs)
// nearest to y = 127 x (one f32 product), |y| clipped at 60, and its 6-bit code
//   code = sign << 5 | n,   n = exponent << 3 | mantissa (bias 1),   value(code) = +-g / 8:
//   n = g (g < 16), 8 + g / 2 (16 <= g < 32), 16 + g / 4 (g >= 32).
// Tie rule: nearest, ties to the even code n (at every midpoint of G the two neighbours' n differ by
// one; within a step rintf's ties-to-even on |y| / step is that rule, and the region ends 16 and 32 have
// even n).  g = 0 has code 0 whatever the sign of y.  Padded rows: g = 0, code 0.
// One thread per 32 elements: g as int8 [..][d], codes as one 32-byte chunk per 32 elements, code e at
// bits 6 e .. 6 e + 5 of the chunk's first 24 bytes (little endian), the last 8 bytes zero — a row of d
// elements is d bytes in both arrays.
__device__ __forceinline__ int fp6_grid_index(float y, int* g) {
    const float t = fminf(fabsf(y), 60.f);
    int n, m;
    if (t < 16.f) { m = (int)__builtin_rintf(t); n = m; }
    else if (t < 32.f) { const int r = (int)__builtin_rintf(0.5f * t); m = 2 * r; n = r + 8; }
    else { const int r = (int)__builtin_rintf(0.25f * t); m = 4 * r; n = r + 16; }
    const bool neg = y < 0.f && m > 0;
    *g = neg ? -m : m;
    return n | (neg ? 32 : 0);
}
__global__ void quantize_fp6_kernel(const float* __restrict__ in, int64_t n_chunks, int d, int m_pad,
                                    const int32_t* __restrict__ nk, int8_t* __restrict__ g,
                                    uint8_t* __restrict__ code) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks;
         c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e0 = c * 32, row = e0 / d;
        const int img = (int)(row / m_pad), r = (int)(row % m_pad);
        const bool valid = r < nk[img];
        unsigned gw[8], cw[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) gw[w] = cw[w] = 0u;
        if (valid) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 x = *reinterpret_cast<const float4*>(in + e0 + 4 * q);
                const float v[4] = {x.x, x.y, x.z, x.w};
                unsigned pk = 0u;   // 4 codes = 24 bits = bytes 3 q .. 3 q + 2 of the chunk
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    int gv;
                    const int cd = fp6_grid_index(127.f * v[t], &gv);
                    gw[q] |= (unsigned)(gv & 0xff) << (8 * t);
                    pk |= (unsigned)cd << (6 * t);
                }
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int byte = 3 * q + t;
                    cw[byte >> 2] |= ((pk >> (8 * t)) & 0xffu) << (8 * (byte & 3));
                }
            }
        }
        uint4* go = reinterpret_cast<uint4*>(g + e0);
        uint4* co = reinterpret_cast<uint4*>(code + e0);
        go[0] = make_uint4(gw[0], gw[1], gw[2], gw[3]);
        go[1] = make_uint4(gw[4], gw[5], gw[6], gw[7]);
        co[0] = make_uint4(cw[0], cw[1], cw[2], cw[3]);
        co[1] = make_uint4(cw[4], cw[5], cw[6], cw[7]);
    }
}

// ---------------------------------------------------------------------------
// match_fp6_kernel (DESIGN.md K1''): the value-only form of match_kernel (16x16 tiles) with the filter's
// dot products on v_mfma_f32_16x16x128_f8f6f4 (twice the int8 rate per clock).  The operands are the e2m3
// codes of the grid values g (quantize_fp6_kernel; value g / 8) as they stand: both block scales are the
// constant 0, for which the compiler emits the unscaled 8-byte instruction (measured 6.6 % faster in
// registers than the scaled one under the unit scale 2^3: profiles/r12/mx_probe_unscaled.txt), and every
// product is g_a g_b / 64.  The loop therefore runs in units of 2^-6: the chains start from h_j / 64
// (key_values_kernel's hf).  |sum g_a g_b| <= D * 3600 <= 921,600 and h_j >= -2^23, so every partial sum
// of  acc = (<b_j, a_i> + h_j) / 64  is an integer multiple of 2^-6 below 2^18 in magnitude: 24 significant
// bits, exact in f32 whatever the order the array sums in, and a positive power-of-two factor changes no
// maximum, median or comparison: the identities of the value-only form (match_kernel's comment) hold
// as they stand, with g in place of q.  The loop's maxima run in f32 (no conversion per distance); the
// row's top two are multiplied by 64 and converted to int once after the loop (both exact) and
// value_only_tail takes over on the integers <b_j, a_i> + h_j: its
// rescan dots the int8 rows g.  Same LDS ring, XCD remap, candidate blocks and ranges as match_kernel.
// The block loop is software-pipelined by one tile (fp6_sched.h): a tile's maxima and a range's merge
// issue in the gaps between the following MFMAs, in an order the source pins.
//
// Operands: the dense rows of pack_fp6_kernel (3 D / 4 bytes, no padding).  Slot s = 4 kk + grp of a row
// (codes 32 s .. 32 s + 31: the 24 bytes a lane gives the MFMA of k-step kk) is a 16-byte low piece at row
// byte 16 s and an 8-byte high piece at row byte D / 2 + 8 s.  A 128-row block sits in LDS as two planes,
// [128][D / 2] low pieces and behind them [128][D / 4] high pieces (DenseStager), so a lane's operand is
// one ds_read_b128 plus one ds_read_b64 that land in adjacent registers: no copies, no padding read.

// One 32-byte code chunk -> the slot's low and high piece of the dense row, one thread per chunk.
__global__ void pack_fp6_kernel(const uint8_t* __restrict__ code, int64_t n_chunks, int d,
                                uint8_t* __restrict__ dense) {
    const int spr = d / 32;   // slots per row
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks;
         c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = c / spr;
        const int s = (int)(c % spr);
        const uint4 lo = *reinterpret_cast<const uint4*>(code + c * 32);
        const uint2 hi = *reinterpret_cast<const uint2*>(code + c * 32 + 16);
        uint8_t* rp = dense + row * (3 * d / 4);
        *reinterpret_cast<uint4*>(rp + 16 * s) = lo;
        *reinterpret_cast<uint2*>(rp + d / 2 + 8 * s) = hi;
    }
}

// Stage candidate block `src` (128 dense rows) into the two LDS planes of `dst` by LDS-DMA, and its 128
// chain starts into `kdst`.  The LDS image of a wave-instruction is lane-linear (1 KiB), so both swizzles
// sit on the per-lane source address, as in Stager.
//   low plane : 16-byte piece of slot s of row r at  r D/2 + ((s ^ lo_sw(r)) << 4).  ds_read_b128 is
//     served in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32): with lane = 16 grp + lr the
//     rows lr = 4..11 of a group read the neighbouring slot s ^ 1, which the term ((lr + 4) >> 3) & 1
//     undoes; the row term then spreads the group's 16 rows over the 16 16-byte bank slots.
//   high plane: 8-byte piece of slot s of row r at  LO + r D/4 + (((s >> 1) ^ hi_sw(r)) << 4) + 8 (s & 1).
//     ds_read_b64 is served in lanes {0-31}, {32-63}: 16 rows x 2 neighbouring slots, which the row term
//     spreads over the 32 8-byte bank slots.  The swizzle moves 16-byte pairs, the DMA's unit.
template <int D, int WAVES>
struct DenseStager {
    static constexpr int ROW = 3 * D / 4, LB = D / 2, HB = D / 4;   // bytes per dense row, per plane row
    static constexpr int LO = kJB * LB, TILE = kJB * ROW;           // low plane, both planes
    static constexpr int CPR = LB / 16, RPB = 256 / LB;             // low: 16-B pieces per row, rows per 256 B
    static constexpr int UPR = HB / 16, RPH = 256 / HB;             // high: 16-B pairs per row, rows per 256 B
    static constexpr int NLO = LO / 1024 / WAVES, NHI = (TILE - LO) / 1024 / WAVES;   // wave-instructions per wave
    static_assert(NLO * WAVES * 1024 == LO && NHI * WAVES * 1024 == TILE - LO && NLO >= 1 && NHI >= 1,
                  "block / workgroup mismatch");
    static_assert(RPB * CPR == 16 && RPH * UPR == 16, "a 16-row tile covers every bank once");

    __device__ static int lo_sw(int r) { return ((((r & 15) + 4) >> 3) & 1) ^ ((r / RPB) % CPR); }
    __device__ static int hi_sw(int r) { return (r / RPH) % UPR; }
    __device__ static int lo_off(int r, int s) { return r * LB + ((s ^ lo_sw(r)) << 4); }
    __device__ static int hi_off(int r, int s) { return LO + r * HB + ((((s >> 1) ^ hi_sw(r)) << 4) | ((s & 1) << 3)); }

    // The lane's source byte offset inside a block for each of its wave's DMA instructions: computed once,
    // so that a block's addresses are a wave-uniform base (scalar unit) plus these.
    struct Lanes {
        unsigned lo[NLO], hi[NHI], key;
    };
    __device__ static Lanes lanes(int wave, int lane) {
        Lanes l;
#pragma unroll
        for (int u = 0; u < NLO; ++u) {
            const int r = (wave * NLO + u) * (1024 / LB) + lane / CPR;
            l.lo[u] = (unsigned)(r * ROW + (((lane % CPR) ^ lo_sw(r)) << 4));
        }
#pragma unroll
        for (int u = 0; u < NHI; ++u) {
            const int r = (wave * NHI + u) * (1024 / HB) + lane / UPR;
            l.hi[u] = (unsigned)(r * ROW + LB + (((lane % UPR) ^ hi_sw(r)) << 4));
        }
        l.key = (unsigned)(lane * 4);
        return l;
    }

    __device__ static void dma(const uint8_t* src, const int32_t* ksrc, int8_t* dst, int32_t* kdst, int wave,
                               const Lanes& l) {
        // the offsets pass through an empty asm so that their widening to 64 bits stays beside the load: the
        // instruction then takes the scalar base and the 32-bit lane offset as they are (no vector address add)
#pragma unroll
        for (int u = 0; u < NLO; ++u) {
            unsigned o = l.lo[u];
            asm volatile("" : "+v"(o));
            __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src + o),
                                             (__attribute__((address_space(3))) void*)(dst + (wave * NLO + u) * 1024),
                                             16, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < NHI; ++u) {
            unsigned o = l.hi[u];
            asm volatile("" : "+v"(o));
            __builtin_amdgcn_global_load_lds(
                (__attribute__((address_space(1))) void*)(src + o),
                (__attribute__((address_space(3))) void*)(dst + LO + (wave * NHI + u) * 1024), 16, 0, 0);
        }
        if (wave == WAVES - 1) {  // 128 chain starts = 2 x (64 lanes x 4 B)
#pragma unroll
            for (int u = 0; u < 2; ++u)
                __builtin_amdgcn_global_load_lds(
                    (__attribute__((address_space(1))) void*)(reinterpret_cast<const uint8_t*>(ksrc + u * 64) + l.key),
                    (__attribute__((address_space(3))) void*)(kdst + u * 64), 4, 0, 0);
        }
    }
};

// The operand's high piece.  A plain 8-byte read is paired with its neighbour (ds_read2st64_b64) and the
// pieces then need copies into the MFMA's register tuple; a volatile LDS read stays a ds_read_b64 that the
// compiler still counts in its s_waitcnt.
__device__ __forceinline__ i32x2 lds_read_b64(const int8_t* p) {
    return *(const volatile __attribute__((address_space(3))) i32x2*)p;
}

struct Fp6Operand {   // 32 codes: 24 bytes in 6 registers
    i32x4 lo;
    i32x2 hi;
    __device__ i32x8 tuple() const { return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], 0, 0}; }
};

// 8 query tiles of 16 rows per wave, 4 waves: 512 query rows per workgroup.  A candidate operand read from
// LDS feeds 8 MFMAs.  Measured on C3 against 4 tiles x 4 waves and 8 tiles x 2 waves (256 rows per
// workgroup): 53.1 / 58.0 / 64.0 ms (profiles/r10/match_fp6_dense_ab.txt)
constexpr int kFp6Tiles = 8;
constexpr int kFp6Waves = 4;

template <int D, typename OutT>
__global__ __launch_bounds__(64 * kFp6Waves, 2) void match_fp6_kernel(
    const uint8_t* __restrict__ dense, const int8_t* __restrict__ g, const int32_t* __restrict__ norms,
    const int32_t* __restrict__ h, const float* __restrict__ hf, const int32_t* __restrict__ nk, int m_pad,
    const int32_t* __restrict__ pairs, int n_iblk, int nwg, long long rn2, long long rd2,
    OutT* __restrict__ m0, CertArgs ca) {
    constexpr int MF = 16, NS = kFp6Tiles, WAVES = kFp6Waves, VG = kValueOnlyTiles;
    static_assert(D % 128 == 0, "one MFMA takes 128 elements of k");
    static_assert(NS % 4 == 0, "value_only_tail takes four query tiles at a time");
    using S = DenseStager<D, WAVES>;
    constexpr int KK = D / 128;                     // MFMAs per output tile
    using SC = Fp6Sched<KK, NS>;
    static_assert(kJB / MF == 2 * VG, "two ranges per block: the range maxima alternate between two sets");
    static_assert(SC::merge(VG * SC::MPT, 0) == -1, "a range's gaps hold the previous range's merge");
    static_assert(SC::merge_ready(), "a chain's merge starts behind its last maximum");
    constexpr int TILE = S::TILE;
    constexpr int NT = 64 * WAVES;
    constexpr int IW = MF * NS, IB = IW * WAVES;
    constexpr int JT = kJB / MF;
    constexpr int kScale = 0;                       // both scales the constant 0: the unscaled instruction
    constexpr float kLow = -262144.f;               // -2^18, below every value in units of 2^-6 (padded rows: -2^17)

    __shared__ __attribute__((aligned(16))) int8_t lds[2 * TILE + 2 * kJB * 4];

    const int wg = xcd_remap(blockIdx.x, nwg);
    const int pair = wg / n_iblk, ib = wg % n_iblk;
    const int a = pairs[2 * pair], b = pairs[2 * pair + 1];
    const int na_rows = nk[a], nb_rows = nk[b];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane / MF, lr = lane % MF;
    const int ibase = ib * IB + wave * IW;
    OutT* out_m = m0 + (size_t)pair * m_pad;

    if (ib * IB >= na_rows || nb_rows < 2) {  // block-uniform: nothing to match
        const int iend = min(ib * IB + IB, m_pad);
        for (int i = ib * IB + tid; i < iend; i += NT) out_m[i] = -1;
        return;
    }

    const uint8_t* bdense = dense + (size_t)b * m_pad * S::ROW;
    const int32_t* bhf = reinterpret_cast<const int32_t*>(hf) + (size_t)b * m_pad;   // h / 64, f32 bits through the key DMA
    const int nblk = (nb_rows + kJB - 1) / kJB;
    int32_t* kbase = reinterpret_cast<int32_t*>(lds + 2 * TILE);

    const typename S::Lanes dl = S::lanes(wave, lane);
    S::dma(bdense, bhf, lds, kbase, wave, dl);  // block 0 in flight

    // Query rows of image a -> B-operand fragments, resident for the run: 32 codes in 6 registers per k-step
    Fp6Operand bq[NS][KK];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int i = min(ibase + s * MF + lr, m_pad - 1);
        const uint8_t* rp = dense + ((size_t)a * m_pad + i) * S::ROW;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            bq[s][kk].lo = *reinterpret_cast<const i32x4*>(rp + 16 * (kk * 4 + grp));
            bq[s][kk].hi = *reinterpret_cast<const i32x2*>(rp + S::LB + 8 * (kk * 4 + grp));
        }
    }
    // the lane's piece offsets inside a 16-row candidate tile (the swizzles depend on the row only mod 16)
    int lo_b[KK], hi_b[KK];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        lo_b[kk] = S::lo_off(lr, kk * 4 + grp);
        hi_b[kk] = S::hi_off(lr, kk * 4 + grp);
    }

    float w1[NS], w2[NS];   // the top two of the group maxima
    int wr[NS];             // the range where the best rose
    // The loop runs one tile behind itself (Fp6Sched): what a block still owes when it ends (its last tile's
    // last maxima, its second range's merge) is paid in the next block's first gaps, or in the drain.  The
    // state starts at kLow, so the first block's payments change nothing: max(kLow, kLow), and a merge of
    // kLow into (kLow, kLow) leaves w1, w2 and wr as they are (the compare is strict).
    f32x4 acc[NS];
    float half[NS], rm[2][NS];   // half: a tile's first maximum, waiting for its second
    bool up[NS];
    int rid_owed = 0;            // the range id of the merge in flight: carried, since the block has moved on
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        w1[s] = kLow; w2[s] = kLow; wr[s] = 0;
        acc[s] = f32x4{kLow, kLow, kLow, kLow};
        half[s] = rm[0][s] = rm[1][s] = kLow;
        up[s] = false;
    }
    auto merge_step = [&](int c, int step, float m, int rid) {
        fp6_merge_step(step, m, rid, up[c], w1[c], w2[c], wr[c]);
    };

    __syncthreads();

    const uint8_t* bsrc = bdense;   // wave-uniform: the block being staged
    const int32_t* ksrc = bhf;
    for (int blk = 0; blk < nblk; ++blk) {
        const int cur = blk & 1;
        bsrc += TILE;
        ksrc += kJB;
        if (blk + 1 < nblk)  // next block in flight under the MFMAs
            S::dma(bsrc, ksrc, lds + (cur ^ 1) * TILE, kbase + (cur ^ 1) * kJB, wave, dl);
        const int8_t* tl = lds + cur * TILE;
        const float* kl = reinterpret_cast<const float*>(kbase + cur * kJB);
        // the first k-step's operand and chain starts: behind the barrier that published the slot
        Fp6Operand av;
        av.lo = *reinterpret_cast<const i32x4*>(tl + lo_b[0]);
        av.hi = lds_read_b64(tl + hi_b[0]);
        // the lane's four candidate rows of a tile: h_j starts every chain
        f32x4 hv = *reinterpret_cast<const f32x4*>(kl + 4 * grp);
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const int R = jt / VG, tt = jt % VG;   // the tile's range in the block, the tile in its range
            f32x4 hv_n = hv;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                Fp6Operand av_n = av;
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    acc[s] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av.tuple(), bq[s][kk].tuple(),
                                                                              kk == 0 ? hv : acc[s], 2, 2, 0, kScale, 0,
                                                                              kScale);
                    __builtin_amdgcn_sched_barrier(0);   // the source order is the issue order
                    if (s == 0) {
                        // Operand reads run one k-step ahead (none across the block's end: the slot is not
                        // published).  They issue behind the k-step's first MFMA, not in front of it: the
                        // compiler waits for this k-step's operand with lgkmcnt(0), which must not catch them.
                        if (kk + 1 < KK) {
                            av_n.lo = *reinterpret_cast<const i32x4*>(tl + lo_b[kk + 1] + jt * MF * S::LB);
                            av_n.hi = lds_read_b64(tl + hi_b[kk + 1] + jt * MF * S::HB);
                        } else if (jt + 1 < JT) {
                            av_n.lo = *reinterpret_cast<const i32x4*>(tl + lo_b[0] + (jt + 1) * MF * S::LB);
                            av_n.hi = lds_read_b64(tl + hi_b[0] + (jt + 1) * MF * S::HB);
                            hv_n = *reinterpret_cast<const f32x4*>(kl + (jt + 1) * MF + 4 * grp);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    const int gp = kk * NS + s;
                    // 2 VALU per 4 distances; the accumulators' first reader is plain C++ (match_kernel's note)
                    if (const int c = SC::chain(gp, 0); c < NS) {
                        // the tile these maxima belong to: this one or the one before.  A range's first tile
                        // starts from kLow (a two-input max would cost a canonicalising v_max_f32 per value)
                        const int of = tt - SC::back(gp, 0);
                        const float from = of < 0 ? rm[R ^ 1][c] : of == 0 ? kLow : rm[R][c];
                        half[c] = __builtin_fmaxf(__builtin_fmaxf(from, acc[c][0]), acc[c][1]);
                    }
                    if (const int c = SC::chain(gp, 1); c < NS)
                        rm[tt == 0 && SC::back(gp, 1) ? R ^ 1 : R][c] =
                            __builtin_fmaxf(__builtin_fmaxf(half[c], acc[c][2]), acc[c][3]);
#pragma unroll
                    for (int j = 0; j < SC::kBudget; ++j)
                        if (const int k = SC::merge(tt * SC::MPT + gp, j); k >= 0) {
                            __builtin_amdgcn_sched_barrier(0);   // every step in its place
                            merge_step(SC::merge_chain(k), SC::merge_step(k), rm[R ^ 1][SC::merge_chain(k)], rid_owed);
                        }
                    __builtin_amdgcn_sched_barrier(0);
                }
                av = av_n;
            }
            hv = hv_n;
            if (tt == VG - 1) rid_owed = blk * (JT / VG) + R;   // this range's merge rides under the next range
        }
        __syncthreads();  // drains this wave's DMA; next block visible to all waves
    }
    // drain: the last tile's owed maxima, then the last range's merge
#pragma unroll
    for (int s = SC::kOwedFirst; s < NS; ++s)
        half[s] = __builtin_fmaxf(__builtin_fmaxf(rm[1][s], acc[s][0]), acc[s][1]);
#pragma unroll
    for (int s = SC::kOwedSecond; s < NS; ++s)
        rm[1][s] = __builtin_fmaxf(__builtin_fmaxf(half[s], acc[s][2]), acc[s][3]);
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int step = 0; step < 4; ++step) merge_step(s, step, rm[1][s], rid_owed);

    // value_only_tail decides 64 query rows (four tiles, one per lane group) per call
#pragma unroll
    for (int q = 0; q < NS / 4; ++q) {
        int v1[4], v2[4], vr[4];   // back to integers below 2^24 in magnitude (kLow: -2^24): product and conversion exact
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            v1[s] = (int)(64.f * w1[4 * q + s]);
            v2[s] = (int)(64.f * w2[4 * q + s]);
            vr[s] = wr[4 * q + s];
        }
        value_only_tail<D, MF, 4, VG, OutT>(v1, v2, vr, g, g + (size_t)b * m_pad * D, h + (size_t)b * m_pad, norms, a, b,
                                            m_pad, na_rows, ibase + q * 4 * MF, grp, lr, lane, rn2, rd2, out_m, ca);
    }
}

template <typename OutT>
int launch_match_fp6(const FilterLaunch& f, OutT* matches0) {
    static_assert(kMatchFp6Rows == 16 * kFp6Tiles * kFp6Waves, "query rows per workgroup");
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(f.nwg), dim3(64 * kFp6Waves), 0, f.stream, f.dense, f.desc, f.norms, f.keys, f.hf,
                           f.n_kpts, f.m_pad, f.pairs, f.n_iblk, f.nwg, f.rn2, f.rd2, matches0, f.ca);
    };
    switch (f.d) {
        case 128: launch(match_fp6_kernel<128, OutT>); break;
        case 256: launch(match_fp6_kernel<256, OutT>); break;
        default: return SFMHIP_E_UNSUPPORTED;
    }
    return check_launch("match_kernel<cert>");
}
template int launch_match_fp6<int32_t>(const FilterLaunch&, int32_t*);
template int launch_match_fp6<int16_t>(const FilterLaunch&, int16_t*);

}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_desc_quantize_fp6(const float* in, int n_img, int m_pad, int d, const int32_t* n_kpts,
                                        int8_t* g, uint8_t* code, void* stream) {
    SFMHIP_REQUIRE(in && g && code && n_kpts, "sfmhip_desc_quantize_fp6: null pointer");
    SFMHIP_REQUIRE(n_img > 0 && m_pad > 0 && d > 0 && d % 32 == 0, "sfmhip_desc_quantize_fp6: bad shape");
    const int64_t n_chunks = (int64_t)n_img * m_pad * d / 32;
    const int grid = (int)std::min<int64_t>((n_chunks + 255) / 256, 4096);
    hipLaunchKernelGGL(quantize_fp6_kernel, dim3(grid), dim3(256), 0, as_stream(stream), in, n_chunks, d, m_pad,
                       n_kpts, g, code);
    return check_launch("quantize_fp6_kernel");
}

extern "C" int sfmhip_desc_pack_fp6(const uint8_t* code, int n_img, int m_pad, int d, uint8_t* dense, void* stream) {
    SFMHIP_REQUIRE(code && dense, "sfmhip_desc_pack_fp6: null pointer");
    SFMHIP_REQUIRE(n_img > 0 && m_pad > 0 && d > 0 && d % 64 == 0, "sfmhip_desc_pack_fp6: bad shape");
    const int64_t n_chunks = (int64_t)n_img * m_pad * d / 32;
    const int grid = (int)std::min<int64_t>((n_chunks + 255) / 256, 4096);
    hipLaunchKernelGGL(pack_fp6_kernel, dim3(grid), dim3(256), 0, as_stream(stream), code, n_chunks, d, dense);
    return check_launch("pack_fp6_kernel");
}
