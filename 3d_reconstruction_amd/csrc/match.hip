// match.hip — M1 brute-force L2 matching + Lowe ratio test on MFMA (int8), the descriptor
// preparation kernels and the mutual filter.
//
// Reference boundary: the matcher call site matching.py:20,122-128 (LightGlue).
// Semantics: SURVEY.md §8a M1, pinned by oracle/match.py.
//
// Design (DESIGN.md "K1"):
//   * descriptors int8 in HBM, [img][m_pad][d]; squared L2 is exact in int32.
//   * one 256-thread workgroup = one pair x 256 rows of image a; each wave keeps
//     its 4 tiles of 16 rows of image a as MFMA B-operands in registers for the whole run.
//   * image b streams through LDS in 128-row blocks (XOR-swizzled, double
//     buffered, filled by LDS-DMA); v_mfma_i32_16x16x64_i8 computes C'[j][i] = <b_j, a_i>,
//     so a lane owns ONE query row i per tile and four candidate rows j.
//   * fused epilogue, <= 2.5 VALU ops per distance: packed key
//        k = (dot << 8) + keys[j],  keys[j] = (-|b_j|^2 << 7) | (127 - j%128)
//     i.e. k = ((2 dot - |b_j|^2) << 7) | (127 - j%128); larger k = smaller
//     distance, lower index on ties.  top-2 per lane via max3 + med3 + max per
//     two candidates; blocks merge into (best key, best index, second key) with
//     explicit index order.
//   * nothing of the M x N distance matrix is ever written.
// The exact float mode's certifying forms of match_kernel are instantiated here too and launched
// for match_exact.hip by launch_match_cert (match_dev.h).
#include "match_dev.h"
#include <cstdlib>

namespace sfmhip {

// ---------------------------------------------------------------------------
// Quantisation f32 -> int8 (padded rows zeroed).  4 elements per thread.
__global__ void quantize_kernel(const float* __restrict__ in, int64_t total, int d, int m_pad,
                                const int32_t* __restrict__ nk, int mode, int8_t* __restrict__ out) {
    const int64_t n4 = total >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4;
         q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = q << 2;
        const int64_t row = e / d;
        const int img = (int)(row / m_pad);
        const int r = (int)(row % m_pad);
        const float4 x = *reinterpret_cast<const float4*>(in + e);
        char4 o = make_char4(0, 0, 0, 0);
        if (r < nk[img]) {
            float v[4] = {x.x, x.y, x.z, x.w};
            int qv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (mode == 0) {
                    float rr = fminf(fmaxf(__builtin_rintf(v[t]), 0.f), 255.f);
                    qv[t] = (int)rr - 128;
                } else {
                    float rr = __builtin_rintf(127.f * v[t]);
                    rr = fminf(fmaxf(rr, -127.f), 127.f);
                    qv[t] = (int)rr;
                }
            }
            o = make_char4((signed char)qv[0], (signed char)qv[1], (signed char)qv[2], (signed char)qv[3]);
        }
        *reinterpret_cast<char4*>(out + e) = o;
    }
}

// Row norms and packed candidate keys, one thread per row.
__global__ void prepare_kernel(const int8_t* __restrict__ desc, int n_rows, int m_pad, int d,
                               const int32_t* __restrict__ nk, int32_t* __restrict__ norms,
                               int32_t* __restrict__ keys) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const int img = row / m_pad, r = row % m_pad;
    const int8_t* p = desc + (size_t)row * d;
    int s = 0;
    for (int k = 0; k < d; k += 16) {
        const i32x4 v = *reinterpret_cast<const i32x4*>(p + k);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int x = v[w];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int q = (int)(signed char)((x >> (8 * t)) & 0xff);
                s += q * q;
            }
        }
    }
    norms[row] = s;
    const int low = 127 - (r & (kJB - 1));
    keys[row] = (r < nk[img]) ? (-s * 128 + low) : (INT_MIN + low);
}

// h = keys >> 8 (match_kernel's value-only form); hf (nullable) = h / 64 in f32, the chain starts of
// match_fp6_kernel in its unit 2^-6 (|h| <= 2^23 and the factor is a power of two: exact).  Both depend on
// the bank alone: sfmhip_match_key_values builds them once, the entries without them once per call.
__global__ void key_values_kernel(const int32_t* __restrict__ keys, int64_t n, int32_t* __restrict__ h,
                                  float* __restrict__ hf) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int v = keys[e] >> 8;
        h[e] = v;
        if (hf) hf[e] = (float)v * 0.015625f;
    }
}

// Shifted copy for the matcher (sfmhip_desc_prepare_shifted): q' = q + c on valid
// rows (zero on padding rows), with norms and keys adjusted so that the matcher,
// unchanged, returns the distances of the UNSHIFTED descriptors, exactly:
//   2 q'_a.q'_b = 2 q_a.q_b + 2c S_a + 2c S_b + 2c^2 d         (S = sum of q)
//   key'_b  = -(|q_b|^2 + 2c S_b)            (packed with the local index as before)
//   norm'_a = |q_a|^2 + 2c S_a + 2c^2 d      so norm'_a - (2 q'_a.q'_b + key'_b) = |q_a - q_b|^2.
// Same argmin, same ties, same ratio test: only the operand bytes change.  With
// c = 64 and |q| <= 64 the operands are non-negative (sign bits constant), which
// lowers the MFMA array's switching power: the clock-limited int8 rate is ~6 %
// higher (tools/mfma_peak: 2,985 -> 3,176 TOPS with the epilogue).
__global__ void prepare_shifted_kernel(const int8_t* __restrict__ desc, int n_rows, int m_pad, int d,
                                       const int32_t* __restrict__ nk, int c, int8_t* __restrict__ out,
                                       int32_t* __restrict__ norms, int32_t* __restrict__ keys) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const int img = row / m_pad, r = row % m_pad;
    const bool valid = r < nk[img];
    const int8_t* p = desc + (size_t)row * d;
    int8_t* o = out + (size_t)row * d;
    int s = 0, sum = 0;
    for (int k = 0; k < d; k += 16) {
        const i32x4 v = *reinterpret_cast<const i32x4*>(p + k);
        i32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int x = v[e];
            unsigned packed = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int q = (int)(signed char)((x >> (8 * t)) & 0xff);
                s += q * q;
                sum += q;
                packed |= (unsigned)((valid ? q + c : 0) & 0xff) << (8 * t);
            }
            w[e] = (int)packed;
        }
        *reinterpret_cast<i32x4*>(o + k) = w;
    }
    norms[row] = s + 2 * c * sum + 2 * c * c * d;
    const int low = 127 - (r & (kJB - 1));
    keys[row] = valid ? (-(s + 2 * c * sum) * 128 + low) : (INT_MIN + low);
}

// One workgroup = one pair x (WAVES * NS * MF) query rows of image a.  Each
// wave owns NS column tiles of MF query rows as resident B-operand fragments
// and streams image b's 128-row blocks from the LDS ring (LDS-DMA filled).
//
// VG > 0 (certifying build without distance outputs, match_exact_impl): the value-only form.
// The int8 pass is only a filter there, so the candidate's index is not carried through the
// top-2.  With keys[j] = (-nb_j << 7) | low, h_j = keys[j] >> 8 and p_j = (keys[j] >> 7) & 1
// give -nb_j = 2 h_j + p_j (match_exact_impl passes the array h, key_values_kernel, as `keys`:
// the form uses the keys in no other way).  Each accumulator chain starts from h_j instead of 0, so
//   acc = <b_j, a_i> + h_j =: v,   D_ij = na_i - 2 v - p_j  in  {Du - 1, Du},  Du = na_i - 2 v
// (padded rows: dot 0, h = -2^23, below every valid v; |v| < 2^24).  The certificate takes D1 in
// [Du1 - 1, Du1] and D2 in [Du2 - 1, Du2], v1 >= v2 the two largest values of the row (as a
// multiset): the best-v candidate w has D_w <= Du1 and every other candidate D_j >= Du2 - 1, so
// an accept (hi(Du1) < lo(Du2 - 1), which needs v1 > v2) proves w the unique winner, and equal
// values are never accepted.  Undecided rows carry Du2 >= D2 in their mark.
//
// The loop keeps no per-distance top two.  A group is a lane's 4 VG values of one range (4 rows
// x VG candidate tiles); the loop takes each group's maximum (0.5 VALU per distance), and per
// range the top two w1 >= w2 of the maxima and the range where w1 rose (strictly: the earliest
// on ties).  After the lane-group merge v1 = the largest group maximum is the row's exact best,
// `loc` one group that attains it, and v2' = the second of the maxima (as a multiset) = the
// largest value outside `loc`.  A value is missing from the maxima only if its group holds a
// larger or equal one, so the row's true second is v2 = max(v2', x), x the second largest value
// of the group `loc` itself (x = v1 when v1 occurs twice there; when v1 is the maximum of two
// groups, v2' = v1 already).  v2' <= v2 gives Du2ub = na - 2 v2' >= Du2: a reject on
// (Du1, Du2ub) is final (the reject test reads lo(D1) and hi(D2) only, and hi() grows with its
// argument, so the exact Du2 rejects too).  For the rows that survive (< 1 % on C3) the wave
// recomputes u_c = <b_j, a_i> + h_j for the 4 VG candidates of `loc`: exactly one u_c == v1
// gives the winner's index and x = the largest other u_c, two or more give x = v1.  The row is
// then certified on the exact (Du1, Du2), the pair a per-distance top two gives, so the graph
// and the marks do not depend on the grouping.
constexpr int kMatchTiles = 4;   // NS: 16-row query tiles per wave
constexpr int kMatchWaves = 4;
template <int D, bool CERT = false, typename OutT = int32_t, int VG = 0>
__global__ __launch_bounds__(64 * kMatchWaves, 2) void match_kernel(
    const int8_t* __restrict__ desc, const int32_t* __restrict__ norms,
    const int32_t* __restrict__ keys, const int32_t* __restrict__ nk, int m_pad,
    const int32_t* __restrict__ pairs, int n_iblk, int nwg, long long rn2, long long rd2,
    OutT* __restrict__ m0, int32_t* __restrict__ dist1, int32_t* __restrict__ dist2, CertArgs ca) {
    constexpr int MF = 16, NS = kMatchTiles, WAVES = kMatchWaves;
    using S = Stager<D, WAVES>;
    using M = Mfma<MF>;
    using acc_t = typename M::acc_t;
    constexpr int KK = D / M::KB;                   // MFMAs per output tile
    constexpr int CPK = M::KB / 16;                 // 16-B chunks per MFMA k-step
    constexpr int NG = 64 / MF;                     // lane groups sharing a query row
    constexpr int TILE = S::TILE;
    constexpr int NT = 64 * WAVES;
    constexpr int IW = MF * NS;                     // query rows per wave
    constexpr int IB = IW * WAVES;                  // query rows per workgroup
    constexpr int JT = kJB / MF;                    // candidate tiles per block
    static_assert(NS % NG == 0 || NG % NS == 0, "output lane mapping");
    constexpr bool VO = VG > 0;
    static_assert(!VO || (CERT && M::NREG == 4 && NS == NG && JT % VG == 0), "value-only form: 16x16 tiles, NS == NG");

    __shared__ __attribute__((aligned(16))) int8_t lds[2 * TILE + 2 * kJB * 4];

    const int wg = xcd_remap(blockIdx.x, nwg);
    const int pair = wg / n_iblk, ib = wg % n_iblk;
    const int a = pairs[2 * pair], b = pairs[2 * pair + 1];
    const int na_rows = nk[a], nb_rows = nk[b];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the LDS-DMA M0 addresses stay scalar
    const int grp = lane / MF, lr = lane % MF;
    const int ibase = ib * IB + wave * IW;
    OutT* out_m = m0 + (size_t)pair * m_pad;

    if (ib * IB >= na_rows || nb_rows < 2) {  // block-uniform: nothing to match
        const int iend = min(ib * IB + IB, m_pad);
        for (int i = ib * IB + tid; i < iend; i += NT) {
            out_m[i] = -1;
            if (dist1) dist1[(size_t)pair * m_pad + i] = -1;
            if (dist2) dist2[(size_t)pair * m_pad + i] = -1;
        }
        return;
    }

    const int8_t* bdesc = desc + (size_t)b * m_pad * D;
    const int32_t* bkeys = keys + (size_t)b * m_pad;
    const int nblk = (nb_rows + kJB - 1) / kJB;
    int32_t* kbase = reinterpret_cast<int32_t*>(lds + 2 * TILE);

    S::dma(bdesc, bkeys, lds, kbase, wave, lane);  // block 0 in flight

    // Query rows of image a -> MFMA B-operand fragments, resident for the run.
    i32x4 bq[NS][KK];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int i = min(ibase + s * MF + lr, m_pad - 1);
        const int8_t* rp = desc + ((size_t)a * m_pad + i) * D + grp * 16;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) bq[s][kk] = *reinterpret_cast<const i32x4*>(rp + kk * M::KB);
    }

    int g1k[NS], g1i[NS], g2k[NS], g1w[NS], g1b[NS];   // best key, its packed word and block; second key
#pragma unroll
    for (int s = 0; s < NS; ++s) { g1k[s] = INT_MIN; g1i[s] = 0; g1w[s] = 127; g1b[s] = 0; g2k[s] = INT_MIN; }
    int w1[NS], w2[NS], wr[NS];   // value-only form: the top two of the group maxima, the range where the best rose
#pragma unroll
    for (int s = 0; s < NS; ++s) { w1[s] = INT_MIN; w2[s] = INT_MIN; wr[s] = 0; }

    __syncthreads();

    for (int blk = 0; blk < nblk; ++blk) {
        const int cur = blk & 1;
        if (blk + 1 < nblk)  // next block in flight under the MFMAs
            S::dma(bdesc + (size_t)(blk + 1) * TILE, bkeys + (blk + 1) * kJB, lds + (cur ^ 1) * TILE,
                   kbase + (cur ^ 1) * kJB, wave, lane);
        const int8_t* tl = lds + cur * TILE;
        const int32_t* kl = kbase + cur * kJB;
        if constexpr (VO) {
            int rm[NS];   // the running maximum of the lane's 4 VG values of this range
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                if (jt % VG == 0) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) rm[s] = INT_MIN;
                }
                // the lane's four candidate rows of this tile: h_j starts every chain
                const i32x4 hv = *reinterpret_cast<const i32x4*>(kl + jt * MF + M::row(0, grp));
                acc_t acc[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) acc[s] = hv;
                const int r = jt * MF + lr;
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const i32x4 av = *reinterpret_cast<const i32x4*>(tl + swz_off<D>(r, kk * CPK + grp));
#pragma unroll
                    for (int s = 0; s < NS; ++s) acc[s] = M::run(av, bq[s][kk], acc[s]);
                }
                // 2 VALU per 4 distances.  The accumulators are read by plain C++ only (the two max,
                // selected as v_max3_i32): the compiler keeps the MFMA -> VALU read distance only for
                // instructions it can see, not for inline asm (reading the accumulators straight into
                // an asm returned stale values on the device).
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    rm[s] = max(max(rm[s], acc[s][0]), acc[s][1]);
                    rm[s] = max(max(rm[s], acc[s][2]), acc[s][3]);
                }
                // per range: with w1 >= w2 the second of {w1, w2, r} is med3(w1, w2, r), equal values
                // included; the best's range moves only on a strict rise (the earliest range on ties)
                if (jt % VG == VG - 1) {
                    const int rid = blk * (JT / VG) + jt / VG;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        wr[s] = rm[s] > w1[s] ? rid : wr[s];
                        w2[s] = med3i(w1[s], w2[s], rm[s]);
                        w1[s] = max(w1[s], rm[s]);
                    }
                }
            }
            __syncthreads();  // drains this wave's DMA; next block visible to all waves
            continue;
        }
        int t1[NS], t2[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) { t1[s] = INT_MIN; t2[s] = INT_MIN; }
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            acc_t acc[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s] = acc_t{0};
            const int r = jt * MF + lr;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const i32x4 av = *reinterpret_cast<const i32x4*>(tl + swz_off<D>(r, kk * CPK + grp));
#pragma unroll
                for (int s = 0; s < NS; ++s) acc[s] = M::run(av, bq[s][kk], acc[s]);
            }
#pragma unroll
            for (int g = 0; g < M::NREG / 4; ++g) {
                const i32x4 kv = *reinterpret_cast<const i32x4*>(kl + jt * MF + M::row(4 * g, grp));
                // two candidates per step: with t1 >= t2 the top two of {t1, t2, ka, kb} (distinct
                // keys) are max3(t1, ka, kb) and max(t2, med3(t1, ka, kb)) — 5 VALU per 2 distances
                // (2 packings + med3 + max3 + max) instead of 6; the same keys, so the same result
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int ka = acc[s][4 * g + e] * 256 + kv[e];
                        const int kb = acc[s][4 * g + e + 1] * 256 + kv[e + 1];
                        const int m = med3i(t1[s], ka, kb);
                        t1[s] = max3i(t1[s], ka, kb);
                        t2[s] = max(t2[s], m);
                    }
                }
            }
        }
        // merge this block's top-2 into the running (key, packed word + block, second key): the
        // second of {g1, g2, k1, k2} is max3(min(g1, k1), g2, k2); an equal key from a later
        // block never replaces the best (lower index on ties); the index is formed once at the end
        // (d <= 128, where a block has half the MFMAs per merge; at d = 256 the branchy form below
        // measured ~1 % faster: profiles/r3/ab/match_merge_ab_r3as.txt)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if constexpr (D <= 128) {
                const int k1 = t1[s] >> 7, k2 = t2[s] >> 7;
                const bool up = k1 > g1k[s];
                g2k[s] = max3i(min(g1k[s], k1), g2k[s], k2);
                g1w[s] = up ? t1[s] : g1w[s];
                g1b[s] = up ? blk : g1b[s];
                g1k[s] = max(g1k[s], k1);
            } else {
                const int k1 = t1[s] >> 7, k2 = t2[s] >> 7, ix = blk * kJB + 127 - (t1[s] & 127);
                if (k1 > g1k[s]) { g2k[s] = max(g1k[s], k2); g1k[s] = k1; g1i[s] = ix; }
                else             { g2k[s] = max(g2k[s], k1); }
            }
        }
        __syncthreads();  // drains this wave's DMA; next block visible to all waves
    }

    if constexpr (VO) {
        value_only_tail<D, MF, NS, VG, OutT>(w1, w2, wr, desc, bdesc, bkeys, norms, a, b, m_pad, na_rows, ibase, grp, lr,
                                             lane, rn2, rd2, out_m, ca);
        return;
    }
    if constexpr (D <= 128) {
#pragma unroll
        for (int s = 0; s < NS; ++s) g1i[s] = g1b[s] * kJB + 127 - (g1w[s] & 127);
    }
    // lanes of the NG groups hold the same query row, disjoint candidate rows.
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int off = MF; off < 64; off <<= 1) {
            const int ok = __shfl_xor(g1k[s], off), oi = __shfl_xor(g1i[s], off), o2 = __shfl_xor(g2k[s], off);
            const bool mine = (g1k[s] > ok) || (g1k[s] == ok && g1i[s] < oi);
            const int n2 = mine ? max(g2k[s], ok) : max(o2, g1k[s]);
            if (!mine) { g1k[s] = ok; g1i[s] = oi; }
            g2k[s] = n2;
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s % NG != grp % NS) continue;   // one lane group writes each tile
        const int i = ibase + s * MF + lr;
        if (i >= m_pad) continue;
        int res = -1, d1 = -1, d2 = -1;
        if (i < na_rows) {
            const int na = norms[(size_t)a * m_pad + i];
            d1 = na - g1k[s];
            d2 = na - g2k[s];
            if (CERT) {
                const int v = ca.force ? -1
                                       : certify(d1, d1, d2, d2, ca.erow[(size_t)a * m_pad + i] + ca.eimg[b], ca.inv_s,
                                                 (double)rn2, (double)rd2);
                res = v > 0 ? g1i[s] : (v == 0 ? -1 : undecided_mark<OutT>(d2));
            } else if (rd2 * (long long)d1 < rn2 * (long long)d2) {
                res = g1i[s];
            }
        }
        out_m[i] = (OutT)res;
        if (dist1) dist1[(size_t)pair * m_pad + i] = d1;
        if (dist2) dist2[(size_t)pair * m_pad + i] = d2;
    }
}

__global__ void mutual_kernel(int32_t* __restrict__ m0, int32_t* __restrict__ m1, int P, int m_pad) {
    // In place is race-free: an entry is cleared only when it is not mutual, and
    // a reader that sees the cleared value (-1) decides the same way.
    const int64_t total = (int64_t)P * m_pad;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = (e / m_pad) * m_pad;
        const int i = (int)(e - base);
        const int j0 = m0[e];
        const int j1 = m1[e];
        const bool keep0 = j0 >= 0 && m1[base + j0] == i;
        const bool keep1 = j1 >= 0 && m0[base + j1] == i;
        if (j0 >= 0 && !keep0) m0[e] = -1;
        if (j1 >= 0 && !keep1) m1[e] = -1;
    }
}

// Every launch of match_kernel: 16x16x64 int8 MFMA tiles, 4 per wave, 4 waves per workgroup
// (32x32 tiles, 8 tiles per wave and 8-wave workgroups measured slower: DESIGN.md K1).
template <int D, bool CERT, int VG, typename OutT>
static void launch_match_d(const FilterLaunch& f, OutT* matches0) {
    static_assert(kMatchRows == 16 * kMatchTiles * kMatchWaves, "query rows per workgroup");
    hipLaunchKernelGGL((match_kernel<D, CERT, OutT, VG>), dim3(f.nwg), dim3(64 * kMatchWaves), 0, f.stream, f.desc,
                       f.norms, f.keys, f.n_kpts, f.m_pad, f.pairs, f.n_iblk, f.nwg, f.rn2, f.rd2, matches0, f.dist1,
                       f.dist2, f.ca);
}

// CERT = false: the plain matcher.  CERT = true: the certifying forms, value-only (VG tiles per range)
// without distance outputs; the packed-key form exists for an int32 graph alone (an int16 graph has no
// distance outputs).
template <int D, bool CERT, typename OutT>
static int launch_match_form(const FilterLaunch& f, OutT* matches0) {
    if constexpr (!CERT) launch_match_d<D, false, 0>(f, matches0);
    else if (!f.dist1 && !f.dist2) launch_match_d<D, true, kValueOnlyTiles>(f, matches0);
    else if constexpr (sizeof(OutT) == 4) launch_match_d<D, true, 0>(f, matches0);
    else return SFMHIP_E_UNSUPPORTED;
    return check_launch(CERT ? "match_kernel<cert>" : "match_kernel");
}
template <bool CERT, typename OutT>
static int launch_match(const FilterLaunch& f, OutT* matches0) {
    switch (f.d) {
        case 64: return launch_match_form<64, CERT>(f, matches0);
        case 128: return launch_match_form<128, CERT>(f, matches0);
        case 256: return launch_match_form<256, CERT>(f, matches0);
        default: return SFMHIP_E_UNSUPPORTED;
    }
}

template <typename OutT>
int launch_match_cert(const FilterLaunch& f, OutT* matches0) {
    return launch_match<true>(f, matches0);
}
template int launch_match_cert<int32_t>(const FilterLaunch&, int32_t*);
template int launch_match_cert<int16_t>(const FilterLaunch&, int16_t*);

void launch_key_values(const int32_t* keys, int64_t n, int32_t* h, float* hf, hipStream_t stream) {
    hipLaunchKernelGGL(key_values_kernel, dim3(std::min(ceil_div(n, 256), 4096)), dim3(256), 0, stream, keys, n, h, hf);
}

}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_desc_quantize(const float* in, int n_img, int m_pad, int d,
                                    const int32_t* n_kpts, int mode, int8_t* out, void* stream) {
    SFMHIP_REQUIRE(in && out && n_kpts, "sfmhip_desc_quantize: null pointer");
    SFMHIP_REQUIRE(n_img > 0 && m_pad > 0 && d > 0 && d % 4 == 0, "sfmhip_desc_quantize: bad shape");
    SFMHIP_REQUIRE(mode == 0 || mode == 1, "sfmhip_desc_quantize: mode must be 0 or 1");
    const int64_t total = (int64_t)n_img * m_pad * d;
    const int64_t n4 = total / 4;
    const int grid = (int)std::min<int64_t>((n4 + 255) / 256, 4096);
    hipLaunchKernelGGL(quantize_kernel, dim3(grid), dim3(256), 0, as_stream(stream), in, total, d,
                       m_pad, n_kpts, mode, out);
    return check_launch("quantize_kernel");
}

extern "C" int sfmhip_desc_prepare(const int8_t* desc, int n_img, int m_pad, int d,
                                   const int32_t* n_kpts, int32_t* norms, int32_t* keys, void* stream) {
    SFMHIP_REQUIRE(desc && n_kpts && norms && keys, "sfmhip_desc_prepare: null pointer");
    SFMHIP_REQUIRE(n_img > 0 && m_pad > 0 && d > 0 && d % 16 == 0, "sfmhip_desc_prepare: bad shape");
    const int rows = n_img * m_pad;
    hipLaunchKernelGGL(prepare_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, as_stream(stream),
                       desc, rows, m_pad, d, n_kpts, norms, keys);
    return check_launch("prepare_kernel");
}

extern "C" int sfmhip_desc_prepare_shifted(const int8_t* desc, int n_img, int m_pad, int d, const int32_t* n_kpts,
                                           int shift, int8_t* desc_shifted, int32_t* norms, int32_t* keys,
                                           void* stream) {
    SFMHIP_REQUIRE(desc && n_kpts && desc_shifted && norms && keys, "sfmhip_desc_prepare_shifted: null pointer");
    SFMHIP_REQUIRE(n_img > 0 && m_pad > 0 && d > 0 && d % 16 == 0 && d <= 256,
                   "sfmhip_desc_prepare_shifted: bad shape");
    SFMHIP_REQUIRE(shift >= 0 && shift <= 127, "sfmhip_desc_prepare_shifted: shift must be in [0, 127]");
    const int rows = n_img * m_pad;
    hipLaunchKernelGGL(prepare_shifted_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, as_stream(stream), desc,
                       rows, m_pad, d, n_kpts, shift, desc_shifted, norms, keys);
    return check_launch("prepare_shifted_kernel");
}

// The key values of a bank, built once (key_values_kernel): h = keys >> 8 and hf = h / 64 in f32, both
// [n_img][m_pad], from the keys of sfmhip_desc_prepare on g.  They depend on the bank alone; the _kv match
// entries take them in place of a rebuild over all n_img m_pad keys on every call.
extern "C" int sfmhip_match_key_values(const int32_t* keys, int n_img, int m_pad, int32_t* h, float* hf, void* stream) {
    SFMHIP_REQUIRE(keys && h && hf, "sfmhip_match_key_values: null pointer");
    SFMHIP_REQUIRE(n_img > 0 && m_pad > 0, "sfmhip_match_key_values: bad shape");
    launch_key_values(keys, (int64_t)n_img * m_pad, h, hf, as_stream(stream));
    return check_launch("key_values_kernel");
}

template <typename OutT>
static int match_pairs_impl(const int8_t* desc, const int32_t* norms, const int32_t* keys,
                            const int32_t* n_kpts, int n_img, int m_pad, int d,
                            const int32_t* pairs, int P, int ratio_num, int ratio_den,
                            OutT* matches0, int32_t* dist1, int32_t* dist2, void* stream) {
    int n_iblk, nwg;
    if (int rc = check_match_call<OutT>("sfmhip_match_pairs", false, n_img, P, m_pad, 0, ratio_num, ratio_den,
                                        desc && norms && keys && n_kpts && pairs && matches0, kMatchRows, &n_iblk, &nwg))
        return rc;
    if (P == 0) return SFMHIP_OK;
    const long long rn2 = (long long)ratio_num * ratio_num, rd2 = (long long)ratio_den * ratio_den;
    const FilterLaunch f{desc, norms, keys, n_kpts, m_pad, d, pairs, n_iblk, nwg, rn2, rd2, CertArgs{},
                         as_stream(stream), dist1, dist2, nullptr, nullptr};
    const int rc = launch_match<false>(f, matches0);
    if (rc == SFMHIP_E_UNSUPPORTED) set_error("sfmhip_match_pairs: descriptor dim %d not in {64,128,256}", d);
    return rc;
}

extern "C" int sfmhip_match_pairs(const int8_t* desc, const int32_t* norms, const int32_t* keys,
                                  const int32_t* n_kpts, int n_img, int m_pad, int d,
                                  const int32_t* pairs, int P, int ratio_num, int ratio_den,
                                  int32_t* matches0, int32_t* dist1, int32_t* dist2, void* stream) {
    return match_pairs_impl(desc, norms, keys, n_kpts, n_img, m_pad, d, pairs, P, ratio_num, ratio_den, matches0,
                            dist1, dist2, stream);
}

extern "C" int sfmhip_match_pairs_i16(const int8_t* desc, const int32_t* norms, const int32_t* keys,
                                      const int32_t* n_kpts, int n_img, int m_pad, int d,
                                      const int32_t* pairs, int P, int ratio_num, int ratio_den,
                                      int16_t* matches0, void* stream) {
    return match_pairs_impl(desc, norms, keys, n_kpts, n_img, m_pad, d, pairs, P, ratio_num, ratio_den, matches0,
                            (int32_t*)nullptr, (int32_t*)nullptr, stream);
}

extern "C" int sfmhip_mutual_filter(int32_t* matches0, int32_t* matches1, int P, int m_pad, void* stream) {
    SFMHIP_REQUIRE(P >= 0 && m_pad > 0, "sfmhip_mutual_filter: bad shape");
    if (P == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(matches0 && matches1, "sfmhip_mutual_filter: null pointer");
    const int64_t total = (int64_t)P * m_pad;
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(mutual_kernel, dim3(grid), dim3(256), 0, as_stream(stream), matches0, matches1, P,
                       m_pad);
    return check_launch("mutual_kernel");
}
