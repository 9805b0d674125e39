// match_dev.h — the device pieces the matching units share (match.hip: the int8 matcher, match_fp6.hip:
// the FP6 certified filter, match_exact.hip: the exact float mode's resolve): the candidate-block stager,
// the int8 MFMA traits, the certificate with the value-only form's tail and the undecided-row marks, and
// the host launchers through which match_exact.hip reaches the other two units' templated kernels.
#pragma once

#include "common.h"
#include <climits>

namespace sfmhip {

typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kJB = 128;              // candidate rows per staged LDS block (7-bit local index)

// Byte offset of logical 16-byte chunk c of row r inside a [rows][D] int8 LDS
// tile.  XOR swizzle makes the 16 rows a ds_read_b128 lane group touches land
// on 16 distinct 16-byte bank slots (cdna_hip_programming.md §5.5 T2).
template <int D>
__device__ __forceinline__ int swz_off(int r, int c) {
    constexpr int CPR = D / 16;   // chunks per row
    constexpr int RPB = 256 / D;  // rows per 256-byte bank row
    return r * D + ((c ^ ((r / RPB) % CPR)) << 4);
}

__device__ __forceinline__ int max3i(int a, int b, int c) {
    int r;
    asm("v_max3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// (the min/max pattern instead of the asm selects v_med3_i32 too, but the compiler then reorders the
// C3 loop badly: 434 vs 101 ms, C2 1.32 vs 1.27 ms; profiles/r5/ab/match_med3_ab_r5.txt)
__device__ __forceinline__ int med3i(int a, int b, int c) {
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// ---------------------------------------------------------------------------
// Stage candidate block `blk` of image b into LDS buffer `dst` (XOR-swizzled
// rows) and its 128 packed keys into `kdst` by LDS-DMA (global_load_lds_dwordx4):
// the LDS image is lane-linear per wave-instruction, so the swizzle moves to the
// per-lane SOURCE chunk (cdna_hip_programming.md §5.4 rule 21).  No VGPRs.
template <int D, int WAVES>
struct Stager {
    static constexpr int CPR = D / 16;                 // 16-B chunks per row
    static constexpr int RPB = 256 / D;                // rows per 256-B bank row
    static constexpr int TILE = kJB * D;               // bytes per block
    static constexpr int NI = TILE / 1024;             // 1-KiB wave-instructions per block
    static constexpr int PER_WAVE = NI / WAVES;        // per wave
    static constexpr int LDT = TILE / 16 / (64 * WAVES);  // 16-B register loads per thread
    static_assert(NI % WAVES == 0 && LDT >= 1, "block / workgroup mismatch");

    __device__ static void dma(const int8_t* src, const int32_t* ksrc, int8_t* dst, int32_t* kdst, int wave,
                               int lane) {
#pragma unroll
        for (int u = 0; u < PER_WAVE; ++u) {
            const int ins = wave * PER_WAVE + u;
            const int rows_per_ins = 1024 / D;
            const int r0 = ins * rows_per_ins;
            const int r = r0 + lane / CPR;
            const int c = (lane % CPR) ^ ((r / RPB) % CPR);
            __builtin_amdgcn_global_load_lds(
                (__attribute__((address_space(1))) void*)(src + (size_t)r * D + c * 16),
                (__attribute__((address_space(3))) void*)(dst + r0 * D), 16, 0, 0);
        }
        if (wave == WAVES - 1) {  // 128 keys = 2 x (64 lanes x 4 B)
#pragma unroll
            for (int u = 0; u < 2; ++u)
                __builtin_amdgcn_global_load_lds(
                    (__attribute__((address_space(1))) void*)(ksrc + u * 64 + lane),
                    (__attribute__((address_space(3))) void*)(kdst + u * 64), 4, 0, 0);
        }
    }
};

// MFMA shape traits.  MF = output tile edge (16: v_mfma_i32_16x16x64_i8, the only form in use).
// Lane l holds the 16 bytes of tile row (l % MF) for k-chunk group (l / MF), and the D/C layout is
//   16x16: col = l % 16, row = 4 (l / 16) + q                      (q < 4)
// The k order inside an MFMA is irrelevant here: A and B use the same map.
template <int MF> struct Mfma;
template <> struct Mfma<16> {
    using acc_t = i32x4;
    static constexpr int NREG = 4, KB = 64;   // accumulators per lane, k bytes per MFMA
    __device__ static acc_t run(i32x4 a, i32x4 b, acc_t c) {
        return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
    }
    __device__ static int row(int q, int grp) { return 4 * grp + q; }
};

// ---------------------------------------------------------------------------
// Exact float mode (SURVEY.md §7 hard part 1: an int8 candidate pass with an
// exact re-score).  Float descriptors x are matched through their int8
// quantisation q with a rigorous bound on the quantisation residual:
//   x = v(q) + delta,  v(q) = q / 127 (MODE_FLOAT) or q + 128 (MODE_SIFT),
//   | |x_a - x_b| - |v_a - v_b| | <= |delta_a| + |delta_b| =: E    (triangle inequality)
// with |v_a - v_b| = sqrt(D) / s (D the matcher's exact integer distance, s =
// 127 or 1).  The order statistics obey the same bound, so from the matcher's
// (D1, D2) a row is decided without the floats when the bound settles it:
//   reject  if  den^2 * lo(d1) >= num^2 * hi(d2)
//   accept  if  hi(d1) < lo(d2)  (unique winner = the int8 winner)  and  den^2 hi(d1) < num^2 lo(d2)
// where lo/hi bound the reference distance d = sum_k (x_ak - x_bk)^2 as the
// oracle evaluates it in f64 (relative error <= (d + 2) 2^-53 < 1e-13 for
// d <= 256, covered by the 1e-12 widening; the sqrt/scale/sum roundings by the
// 2^-50 operand margins).  Undecided rows are marked -(3 + D2) and settled
// exactly by match_resolve_kernel.
struct CertArgs {
    const double* erow;   // [n_img][m_pad] residual bound per row (desc_residual_kernel)
    const double* eimg;   // [n_img] max over the image's rows
    double inv_s;         // 1/127 (MODE_FLOAT) or 1 (MODE_SIFT)
    int force;            // 1: no row is certified (every row takes the exact path; tests)
};
constexpr int kUndecidedBase = -3;   // matches0 = kUndecidedBase - D2 marks an undecided row
// match_kernel's value-only form: 16-candidate tiles per recorded winner range (a lane sees 4
// distances per tile, so G = 16 per range; 8 tiles = one range per 128-row block).  The loop takes
// one maximum per range and the post-loop rescan covers one range's G candidates per surviving
// row.  Measured on C3, 4 / 8 tiles: 81.7 / 82.7 ms on all pairs, 1.63 / 1.75 ms on the overlapping
// pairs (profiles/r8/match_rangemax_ab.txt)
constexpr int kValueOnlyTiles = 4;
// int16 graphs (m_pad <= 32767: dist.graph_dtype) carry an upper bound of sqrt(D2) instead:
// mark = kUndecidedBase - u, u = ceil(8 sqrt(D2)) <= 32640 for d <= 256 (D2 <= 256 * 255^2),
// so the mark stays above -32768 and the resolve's candidate radius only grows (by < 1/8).
__device__ __forceinline__ int sqrt8_ceil(int d2) {
    const long long t = 64LL * d2;
    int u = (int)ceil(sqrt((double)t));
    while (u > 0 && (long long)(u - 1) * (u - 1) >= t) --u;
    while ((long long)u * u < t) ++u;
    return u;
}
template <typename OutT>
__device__ __forceinline__ int undecided_mark(int d2) {
    if constexpr (sizeof(OutT) == 2) return kUndecidedBase - sqrt8_ceil(d2);
    else return kUndecidedBase - d2;
}
// an upper bound of sqrt(D2) from a mark (the resolve widens it by 1e-12 relative)
template <typename OutT>
__device__ __forceinline__ double mark_sqrt_d2(int mark) {
    if constexpr (sizeof(OutT) == 2) return (double)(kUndecidedBase - mark) * 0.125;
    else return sqrt((double)(kUndecidedBase - mark));
}

// 1 accept, 0 reject, -1 undecided.  Each integer distance is given as an interval
// [lo, hi] (lo == hi in the packed-key form, hi - lo = 1 in the value-only form below): the
// lower bounds come from lo, the upper bounds from hi.
__device__ __forceinline__ int certify(int d1lo, int d1hi, int d2lo, int d2hi, double E, double inv_s, double rn2,
                                       double rd2) {
    const double up = 1.0 + 0x1p-50, dn = 1.0 - 0x1p-50;
    const double s1l = sqrt((double)d1lo) * inv_s, s1h = sqrt((double)d1hi) * inv_s;
    const double s2l = sqrt((double)d2lo) * inv_s, s2h = sqrt((double)d2hi) * inv_s;
    const double a1 = fmax(s1l * dn - E * up, 0.0), b1 = (s1h + E) * up;
    const double a2 = fmax(s2l * dn - E * up, 0.0), b2 = (s2h + E) * up;
    const double wl = 1.0 - 1e-12, wh = 1.0 + 1e-12;
    const double lo1 = a1 * a1 * wl, hi1 = b1 * b1 * wh, lo2 = a2 * a2 * wl, hi2 = b2 * b2 * wh;
    if (rd2 * lo1 >= rn2 * hi2) return 0;
    if (hi1 < lo2 && rd2 * hi1 < rn2 * lo2) return 1;
    return -1;
}

// The value-only form's tail, shared by match_kernel<.., VG> and match_fp6_kernel: from a lane's top two
// group maxima w1 >= w2 and the range wr where w1 rose (per query tile s) to the row's graph entry: the
// lane-group merge, the pre-test, the rescan of the recorded group for surviving rows and the final
// certificate (match_kernel's comment).  `desc` holds the int8 rows the rescan dots (the kernel's own
// operands, or the grid values g of the FP6 form), bkeys the values h_j of image b.
template <int D, int MF, int NS, int VG, typename OutT>
__device__ __forceinline__ void value_only_tail(const int (&w1)[NS], const int (&w2)[NS], const int (&wr)[NS],
                                                const int8_t* __restrict__ desc, const int8_t* __restrict__ bdesc,
                                                const int32_t* __restrict__ bkeys, const int32_t* __restrict__ norms,
                                                int a, int b, int m_pad, int na_rows, int ibase, int grp, int lr,
                                                int lane, long long rn2, long long rd2, OutT* __restrict__ out_m,
                                                const CertArgs& ca) {
    constexpr int NG = 64 / MF;
    // lanes of the NG groups hold the same query row, disjoint candidate rows: a value-only
    // merge that carries the (range, lane group) of the larger best; lane group s keeps tile s
    int v1 = INT_MIN, v2 = INT_MIN, loc = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        int a1 = w1[s], a2 = w2[s], al = wr[s] * NG + grp;
#pragma unroll
        for (int off = MF; off < 64; off <<= 1) {
            const int o1 = __shfl_xor(a1, off), o2 = __shfl_xor(a2, off), ol = __shfl_xor(al, off);
            const bool mine = a1 > o1 || (a1 == o1 && al < ol);
            a2 = max3i(min(a1, o1), a2, o2);
            al = mine ? al : ol;
            a1 = max(a1, o1);
        }
        if (s == grp) { v1 = a1; v2 = a2; loc = al; }
    }
    // v1 is the exact best; v2 (the second of the group maxima) is the largest value outside
    // the group `loc`, a lower bound of the true second
    const int i = ibase + grp * MF + lr;
    int res = -1, na = 0, du1 = 0, hidx = -1;
    double E = 0.0;
    bool survivor = false;
    if (i < na_rows) {   // na_rows <= m_pad
        na = norms[(size_t)a * m_pad + i];
        du1 = na - 2 * v1;                  // D1 in [du1 - 1, du1]
        const int du2ub = na - 2 * v2;      // D2 in [du1 - 1, du2ub]
        E = ca.erow[(size_t)a * m_pad + i] + ca.eimg[b];
        // pre-test: a reject reads lo(D1) and hi(D2) only, and hi() of an upper bound of D2 is
        // valid, so 0 is final; everything else goes on.  A forced row is marked from du2ub, or
        // from the largest int8 distance where v2 is a padded row's value (all valid candidates
        // in one group: the int16 mark holds sqrt(D2) only up to D 255^2)
        if (ca.force)
            res = undecided_mark<OutT>(min(du2ub, D * 255 * 255));
        else
            survivor = certify(max(du1 - 1, 0), du1, max(du1 - 1, 0), du2ub, E, ca.inv_s, (double)rn2,
                               (double)rd2) != 0;
    }
    // the hidden second and the winner's index, surviving rows only, one row at a time by the
    // whole wave: LPC lanes per candidate of the recorded group, each a D / LPC byte slice of
    // <b_j, a_i>
    constexpr int NC = 4 * VG;
    constexpr int LPC = (64 / NC) < (D / 16) ? (64 / NC) : (D / 16);
    constexpr int BPL = D / LPC;
    const int c = min(lane / LPC, NC - 1), part = lane % LPC;
    unsigned long long bal = __ballot(survivor);
    while (bal) {
        const int l = __builtin_ctzll(bal);
        bal &= bal - 1;
        const int ri = __shfl(i, l), rv = __shfl(v1, l), rl = __shfl(loc, l);
        const int j0 = (rl / NG) * VG * MF + 4 * (rl % NG);   // candidate c: tile c / 4 of the range, row c % 4
        const int j = j0 + (c >> 2) * MF + (c & 3);
        const int8_t* pa = desc + ((size_t)a * m_pad + ri) * D + part * BPL;
        const int8_t* pb = bdesc + (size_t)j * D + part * BPL;
        int dot = 0;
#pragma unroll
        for (int w = 0; w < BPL / 16; ++w) {
            const i32x4 x = *reinterpret_cast<const i32x4*>(pa + 16 * w);
            const i32x4 y = *reinterpret_cast<const i32x4*>(pb + 16 * w);
#pragma unroll
            for (int e = 0; e < 4; ++e) dot = __builtin_amdgcn_sdot4(x[e], y[e], dot, false);
        }
#pragma unroll
        for (int off = 1; off < LPC; off <<= 1) dot += __shfl_xor(dot, off);
        const int u = dot + bkeys[j];   // every lane of candidate c holds u_c
        const bool hit = lane < NC * LPC && part == 0 && u == rv;
        const unsigned long long hb = __ballot(hit);   // >= 1 candidate: the group's maximum is v1
        // the largest value of the group's other candidates: v1 again when it occurs twice
        int x = u == rv ? INT_MIN : u;
#pragma unroll
        for (int off = LPC; off < 64; off <<= 1) x = max(x, __shfl_xor(x, off));
        if (lane == l) {
            const bool one = __popcll(hb) == 1;
            v2 = max(v2, one ? x : rv);
            if (one) {
                const int hc = __builtin_ctzll(hb) / LPC;
                hidx = j0 + (hc >> 2) * MF + (hc & 3);
            }
        }
    }
    // the final decision on the exact second, as the per-distance top two gave it
    if (survivor) {
        const int du2 = na - 2 * v2;   // D2 in [du2 - 1, du2]
        const int v = certify(max(du1 - 1, 0), du1, max(du2 - 1, 0), du2, E, ca.inv_s, (double)rn2, (double)rd2);
        // an accepted row has v1 > v2, so exactly one candidate of its group attains v1
        res = v == 0 ? -1 : (v > 0 && hidx >= 0) ? hidx : undecided_mark<OutT>(du2);
    }
    if (i < m_pad) out_m[i] = (OutT)res;
}

// ---------------------------------------------------------------------------
// Host side.  A templated kernel is launched where it is defined, so match_exact_impl (match_exact.hip)
// reaches the certifying filters and the resolve chain through plain functions, each instantiated for an
// int32 and an int16 graph.  They launch on `stream` and return the status of check_launch
// (SFMHIP_E_UNSUPPORTED without a launch or a message for a d the kernels are not built for).
constexpr int kMatchRows = 256;      // query rows per workgroup of match_kernel (16x16 tiles, 4 per wave, 4 waves)
constexpr int kMatchFp6Rows = 512;   // of match_fp6_kernel (8 tiles per wave, 4 waves)

struct FilterLaunch {
    const int8_t* desc;        // the int8 operands [n_img][m_pad][d] (FP6 filter: the grid values g, for the rescan)
    const int32_t* norms;
    const int32_t* keys;       // the packed keys; the value-only forms take h = keys >> 8 here
    const int32_t* n_kpts;
    int m_pad, d;
    const int32_t* pairs;
    int n_iblk, nwg;           // workgroups per pair, in all
    long long rn2, rd2;        // ratio_num^2, ratio_den^2
    CertArgs ca;
    hipStream_t stream;
    int32_t *dist1, *dist2;    // match_kernel's packed-key form only (both null: its value-only form)
    const uint8_t* dense;      // match_fp6_kernel only: the packed e2m3 rows and hf = h / 64
    const float* hf;
};
// match_kernel<.., CERT = true>: the value-only form when there are no distance outputs (match.hip)
template <typename OutT> int launch_match_cert(const FilterLaunch& f, OutT* matches0);
// match_fp6_kernel (match_fp6.hip)
template <typename OutT> int launch_match_fp6(const FilterLaunch& f, OutT* matches0);
// collect, offsets, flatten, batched resolve and the fallback scan (match_exact.hip)
struct ResolveLaunch;
template <typename OutT> int launch_resolve(const ResolveLaunch& r, OutT* matches0);
// key_values_kernel over n keys; hf may be null (match.hip)
void launch_key_values(const int32_t* keys, int64_t n, int32_t* h, float* hf, hipStream_t stream);

// The checks every pair-matching entry makes, in the order include/sfmhip.h promises: the shape, then the
// empty call (returns SFMHIP_OK with *nwg = 0: the caller returns), then the pointers (`pointers`: all of
// the entry's required ones are non-null) and the size of the launch.  `entry` names the int32 entry;
// mode is checked by the exact entries alone (exact = true).
template <typename OutT>
inline int check_match_call(const char* entry, bool exact, int n_img, int P, int m_pad, int mode, int ratio_num,
                            int ratio_den, bool pointers, int rows_per_wg, int* n_iblk, int* nwg) {
    *n_iblk = *nwg = 0;
    SFMHIP_REQUIRE(n_img > 0 && P >= 0, "%s: bad counts", entry);
    SFMHIP_REQUIRE(m_pad > 0 && m_pad % kJB == 0, "%s: m_pad must be a positive multiple of 128", entry);
    if (exact) SFMHIP_REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 or 1", entry);
    SFMHIP_REQUIRE(ratio_num > 0 && ratio_den > 0 && ratio_num <= 65535 && ratio_den <= 65535,
                   "%s: ratio must be a positive fraction", entry);
    if constexpr (sizeof(OutT) == 2)
        SFMHIP_REQUIRE(m_pad <= 32767, "%s_i16: m_pad must be <= 32767 for an int16 graph", entry);
    if (P == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(pointers, "%s: null pointer", entry);
    *n_iblk = ceil_div(m_pad, rows_per_wg);
    const int64_t nwg64 = (int64_t)P * *n_iblk;
    SFMHIP_REQUIRE(nwg64 < INT_MAX, "%s: too many pairs for one launch", entry);
    *nwg = (int)nwg64;
    return SFMHIP_OK;
}

}  // namespace sfmhip
