// match_exact.hip — the exact float mode (DESIGN.md K1', K1''; the certificate: match_dev.h): the
// residual bounds of a bank (desc_residual_kernel), the resolve that settles in f64 every row the
// certifying filter left undecided (collect per image, flatten XCD-major, batched MFMA prefilter, with
// a graph scan as the fallback), and the sfmhip_match_pairs_exact* entries.  The filters themselves
// live in match.hip (int8) and match_fp6.hip (FP6) and are reached through match_dev.h's launchers.
#include "match_dev.h"
#include "resolve_scratch.h"

namespace sfmhip {

// ---------------------------------------------------------------------------
// Exact float mode, part 1: per-row residual bounds E_row >= |x - v(q)| (f64,
// outward margins: the sum of squares and sqrt carry <= d 2^-53 relative, the
// computed components <= 2^-52 (|x| + |v|) absolute) and E_img = max per image
// (non-negative doubles order as their bit patterns).  A non-finite row gets
// +inf: every match it takes part in goes to the exact path.  One wave per row.
__global__ __launch_bounds__(256) void desc_residual_kernel(const float* __restrict__ x, const int8_t* __restrict__ q,
                                                            int n_rows, int m_pad, int d, const int32_t* __restrict__ nk,
                                                            int mode, double* __restrict__ erow,
                                                            unsigned long long* __restrict__ eimg) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int img = row / m_pad, r = row % m_pad;
    if (r >= nk[img]) {
        if (lane == 0) erow[row] = 0.0;
        return;
    }
    const float* xr = x + (size_t)row * d;
    const int8_t* qr = q + (size_t)row * d;
    double s2 = 0.0, x2 = 0.0, v2 = 0.0;
    bool finite = true;
    for (int k = lane; k < d; k += 64) {
        const float xf = xr[k];
        const double xv = (double)xf;
        const double v = mode == 0 ? (double)((int)qr[k] + 128) : (double)qr[k] / 127.0;
        const double dl = xv - v;
        s2 = __builtin_fma(dl, dl, s2);
        x2 = __builtin_fma(xv, xv, x2);
        v2 = __builtin_fma(v, v, v2);
        finite = finite && __builtin_isfinite(xf);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s2 += __shfl_xor(s2, off);
        x2 += __shfl_xor(x2, off);
        v2 += __shfl_xor(v2, off);
    }
    const bool all_finite = __all(finite);
    if (lane == 0) {
        const double e = all_finite ? sqrt(s2) * (1.0 + 0x1p-40) + 0x1p-50 * (sqrt(x2) + sqrt(v2)) * (1.0 + 0x1p-40)
                                    : __builtin_inf();
        erow[row] = e;
        atomicMax(eimg + img, (unsigned long long)__double_as_longlong(e));
    }
}

// Exact float mode, part 2: every row the certificate left undecided
// (matches0 <= kUndecidedBase, carrying the int8 second-best D2) is settled
// against the f32 descriptors, one wave per row, with the oracle's arithmetic:
//   d(i,j) = sum_k (f64(x_ak) - f64(x_bj,k))^2, one IEEE op per step in k order
//   j1 = lowest index attaining min d, d2 = min over j != j1,
//   accept iff den^2 d1 < num^2 d2 exactly (two-product comparison).
// Candidates: only j whose int8 distance D_j can still reach the top two,
//   sqrt(D_j) <= s E + (sqrt(D2) + s E) (1 + 1e-12)  (E = E_row[a,i] + E_img[b]),
// found with v_dot4 over the int8 rows; the f64 distances are evaluated for
// those (at most kResolveCap, else for every j).  A persistent scan over the
// match graph finds the marked rows (grid-stride over 64-row chunks).
constexpr int kResolveCap = 512;
#ifdef SFMHIP_RESOLVE_PROF
// tool-only build (tools/prof_resolve.py): rows, candidates, rows over the cap, max candidates,
// a histogram by 64 — of the batched resolve
__device__ unsigned long long g_rprof[16];
#endif
// One undecided row e (its mark = kUndecidedBase - D2) by one wave; sxa / sqa / scand: the wave's
// LDS rows.
template <int D, typename OutT>
__device__ __forceinline__ void resolve_row(int64_t e, int mark, const int8_t* __restrict__ q,
                                            const float* __restrict__ x, const int32_t* __restrict__ nk, int m_pad,
                                            const int32_t* __restrict__ pairs, const double* __restrict__ erow,
                                            const double* __restrict__ eimg, double s, double rn2, double rd2,
                                            OutT* __restrict__ m0, unsigned* __restrict__ n_resolved, float* sxa,
                                            int* sqa, int* scand, int lane) {
    constexpr int W4 = D / 4;
    const int pair = (int)(e / m_pad), i = (int)(e % m_pad);
    const int a = pairs[2 * pair], b = pairs[2 * pair + 1], nb = nk[b];
    const size_t arow = (size_t)a * m_pad + i;
    for (int k = lane; k < D; k += 64) sxa[k] = x[arow * D + k];
    for (int w = lane; w < W4; w += 64) sqa[w] = reinterpret_cast<const int*>(q + arow * D)[w];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // |q_a|^2
    int na = 0;
    for (int w = lane; w < W4; w += 64) na = __builtin_amdgcn_sdot4(sqa[w], sqa[w], na, false);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) na += __shfl_xor(na, off);
    const double se = (erow[arow] + eimg[b]) * s * (1.0 + 1e-12);
    const double bq = (se + (mark_sqrt_d2<OutT>(mark) + se) * (1.0 + 1e-12)) * (1.0 + 1e-12);
    const double tq = floor(bq * bq) + 1.0;   // every j with D_j <= tq may reach the top two
    int ncand = 0;
    for (int j0 = 0; j0 < nb; j0 += 64) {
        const int j = j0 + lane;
        bool in = false;
        if (j < nb) {
            const int4* qb = reinterpret_cast<const int4*>(q + ((size_t)b * m_pad + j) * D);
            int dot = 0, nbn = 0;
#pragma unroll 4
            for (int w4 = 0; w4 < W4 / 4; ++w4) {
                const int4 t = qb[w4];
                const int4 u = reinterpret_cast<const int4*>(sqa)[w4];
                dot = __builtin_amdgcn_sdot4(t.x, u.x, dot, false);
                dot = __builtin_amdgcn_sdot4(t.y, u.y, dot, false);
                dot = __builtin_amdgcn_sdot4(t.z, u.z, dot, false);
                dot = __builtin_amdgcn_sdot4(t.w, u.w, dot, false);
                nbn = __builtin_amdgcn_sdot4(t.x, t.x, nbn, false);
                nbn = __builtin_amdgcn_sdot4(t.y, t.y, nbn, false);
                nbn = __builtin_amdgcn_sdot4(t.z, t.z, nbn, false);
                nbn = __builtin_amdgcn_sdot4(t.w, t.w, nbn, false);
            }
            in = (double)((long long)na + nbn - 2LL * dot) <= tq;
        }
        const unsigned long long cb = __ballot(in);
        const int pos = ncand + __popcll(cb & ((1ull << lane) - 1ull));
        if (in && pos < kResolveCap) scand[pos] = j;
        ncand += __popcll(cb);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const bool every = ncand > kResolveCap;
    const int nc = every ? nb : ncand;
    double v1 = __builtin_inf(), v2 = __builtin_inf();
    int j1 = INT_MAX;
    for (int t = lane; t < nc; t += 64) {   // ascending j per lane
        const int j = every ? t : scand[t];
        const float4* xb = reinterpret_cast<const float4*>(x + ((size_t)b * m_pad + j) * D);
        double acc = 0.0;
        for (int k4 = 0; k4 < D / 4; ++k4) {
            const float4 xv = xb[k4];
            double df;
            df = (double)sxa[4 * k4] - (double)xv.x;
            acc = acc + df * df;
            df = (double)sxa[4 * k4 + 1] - (double)xv.y;
            acc = acc + df * df;
            df = (double)sxa[4 * k4 + 2] - (double)xv.z;
            acc = acc + df * df;
            df = (double)sxa[4 * k4 + 3] - (double)xv.w;
            acc = acc + df * df;
        }
        if (acc < v1) { v2 = v1; v1 = acc; j1 = j; }
        else if (acc < v2) v2 = acc;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o1 = __shfl_xor(v1, off), o2 = __shfl_xor(v2, off);
        const int oj = __shfl_xor(j1, off);
        const bool mine = v1 < o1 || (v1 == o1 && j1 < oj);
        const double n2 = mine ? fmin(v2, o1) : fmin(o2, v1);
        if (!mine) { v1 = o1; j1 = oj; }
        v2 = n2;
    }
    // den^2 d1 < num^2 d2, exactly: (p, e) two-products compare lexicographically (RN is monotone)
    const double p1 = rd2 * v1, e1 = __builtin_fma(rd2, v1, -p1);
    const double p2 = rn2 * v2, e2 = __builtin_fma(rn2, v2, -p2);
    const bool acc_ok = p1 < p2 || (p1 == p2 && e1 < e2);
    if (lane == 0) {
        m0[e] = (OutT)(acc_ok ? j1 : -1);
        if (n_resolved) atomicAdd(n_resolved, 1u);
    }
    __builtin_amdgcn_wave_barrier();   // LDS rows reused by the next marked row
}

template <int D, typename OutT>
__global__ __launch_bounds__(256) void match_resolve_kernel(const int8_t* __restrict__ q, const float* __restrict__ x,
                                                            const int32_t* __restrict__ nk, int m_pad,
                                                            const int32_t* __restrict__ pairs, int P,
                                                            const double* __restrict__ erow,
                                                            const double* __restrict__ eimg, double s, double rn2,
                                                            double rd2, OutT* __restrict__ m0,
                                                            unsigned* __restrict__ n_resolved,
                                                            const unsigned* __restrict__ overflow = nullptr) {
    if (overflow && *overflow == 0u) return;   // the bucketed pass below settled every row
    constexpr int W4 = D / 4;
    __shared__ float sxa[4][D];
    __shared__ __attribute__((aligned(16))) int sqa[4][W4];
    __shared__ int scand[4][kResolveCap];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = (int64_t)P * m_pad;
    const int64_t nchunk = (total + 63) >> 6;
    for (int64_t c = (int64_t)blockIdx.x * 4 + wave; c < nchunk; c += (int64_t)gridDim.x * 4) {
        const int64_t e0 = c << 6;
        const int v = (e0 + lane < total) ? (int)m0[e0 + lane] : -1;
        unsigned long long bal = __ballot(v <= kUndecidedBase);
        while (bal) {
            const int l = __builtin_ctzll(bal);
            bal &= bal - 1;
            resolve_row<D, OutT>(e0 + l, __shfl(v, l), q, x, nk, m_pad, pairs, erow, eimg, s, rn2, rd2, m0, n_resolved,
                           sxa[wave], sqa[wave], scand[wave], lane);
        }
    }
}

// Default (round 5): the undecided rows are collected per image b (one scan of the match graph
// into buckets of up to kResolveBucket rows), laid out XCD-major (images b = x, x + 8, ... on XCD x)
// and settled kResolveRows at a time per workgroup (match_resolve_batched_kernel), so image b's int8
// rows — the candidate prefilter reads all of them, 1 MB per row at C3 — are read once per batch.
// A bucket overflow sets *overflow and match_resolve_kernel's graph scan settles every row instead.
// The kernels' cnt, list, off, okey, oimg, xr, ir, flat and items are the regions of ResolveScratch
// (resolve_scratch.h) of those names, overflow its flag.
template <typename OutT>
__global__ __launch_bounds__(256) void resolve_collect_kernel(const OutT* __restrict__ m0, int64_t total, int m_pad,
                                                              const int32_t* __restrict__ pairs,
                                                              unsigned* __restrict__ cnt, int64_t* __restrict__ list,
                                                              unsigned* __restrict__ overflow) {
    auto take = [&](int64_t e) {
        const int b = pairs[2 * (int)(e / m_pad) + 1];
        const unsigned slot = atomicAdd(cnt + b, 1u);
        if (slot < (unsigned)kResolveBucket) list[(size_t)b * kResolveBucket + slot] = e;
        else atomicOr(overflow, 1u);
    };
    constexpr int PER = 16 / sizeof(OutT);   // entries per 16-B load (m_pad % 128 == 0: whole loads)
    const int64_t n4 = total / PER;
    const int4* m4 = reinterpret_cast<const int4*>(m0);
    for (int64_t e4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e4 < n4; e4 += (int64_t)gridDim.x * blockDim.x) {
        const int4 v = m4[e4];
        if constexpr (sizeof(OutT) == 2) {
            // 8 int16 entries: a mark is <= -3, i.e. in 0x8000..0xFFFD as an unsigned half
            const unsigned w[4] = {(unsigned)v.x, (unsigned)v.y, (unsigned)v.z, (unsigned)v.w};
            bool any = false;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                any |= (short)(w[h] & 0xFFFFu) <= kUndecidedBase;
                any |= (short)(w[h] >> 16) <= kUndecidedBase;
            }
            if (!any) continue;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                if ((short)(w[h] & 0xFFFFu) <= kUndecidedBase) take(PER * e4 + 2 * h);
                if ((short)(w[h] >> 16) <= kUndecidedBase) take(PER * e4 + 2 * h + 1);
            }
        } else {
            if (min(min(v.x, v.y), min(v.z, v.w)) > kUndecidedBase) continue;
            if (v.x <= kUndecidedBase) take(4 * e4);
            if (v.y <= kUndecidedBase) take(4 * e4 + 1);
            if (v.z <= kUndecidedBase) take(4 * e4 + 2);
            if (v.w <= kUndecidedBase) take(4 * e4 + 3);
        }
    }
}

// The buckets flattened XCD-major (images b = x, x + 8, ... for x = 0..7, each image's rows
// together), with each XCD's range [xr[x], xr[x] + xr[8 + x]): resolve_offsets_kernel (one
// workgroup: position p of that order holds image b(p); an LDS scan over the positions, 1024 at a
// time, gives each image's first flat row and first item), then resolve_flatten_kernel (one entry
// per thread, its image found by a binary search over the offsets in that order).
__global__ __launch_bounds__(1024) void resolve_offsets_kernel(
    const unsigned* __restrict__ cnt, int n_img, unsigned* __restrict__ off, unsigned* __restrict__ okey,
    int* __restrict__ oimg, unsigned* __restrict__ xr, int* __restrict__ items, unsigned* __restrict__ ir,
    const unsigned* __restrict__ overflow) {
    __shared__ unsigned sr[1024], sk[1024];
    __shared__ unsigned sxs[9], sks[9];
    if (*overflow != 0u) return;
    const int tid = threadIdx.x;
    const int cap = n_img * (kResolveBucket / kResolveRows + 1);
    int ps[9];   // first position of XCD x (ps[8] = n_img)
    ps[0] = 0;
#pragma unroll
    for (int x = 0; x < 8; ++x) ps[x + 1] = ps[x] + (x < n_img ? (n_img - x + 7) / 8 : 0);
    unsigned carry_r = 0, carry_k = 0;
    for (int base = 0; base < n_img; base += 1024) {
        const int p = base + tid;
        int b = -1;
        unsigned cb = 0, ni = 0;
        if (p < n_img) {
            int x = 0;
#pragma unroll
            for (int y = 1; y < 8; ++y) x += (p >= ps[y]) ? 1 : 0;
            b = x + 8 * (p - ps[x]);
            cb = min(cnt[b], (unsigned)kResolveBucket);
            ni = (cb + kResolveRows - 1) / kResolveRows;
        }
        sr[tid] = cb;
        sk[tid] = ni;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {   // inclusive scan
            const unsigned vr = tid >= d ? sr[tid - d] : 0u, vk = tid >= d ? sk[tid - d] : 0u;
            __syncthreads();
            sr[tid] += vr;
            sk[tid] += vk;
            __syncthreads();
        }
        const unsigned run = carry_r + sr[tid] - cb, k0 = carry_k + sk[tid] - ni;
        if (b >= 0) {
            off[b] = run;
            okey[p] = run;
            oimg[p] = b;
#pragma unroll
            for (int x = 0; x < 8; ++x)
                if (p == ps[x]) {
                    sxs[x] = run;
                    sks[x] = k0;
                }
            for (unsigned i = 0; i < ni; ++i) {
                items[k0 + i] = (int)(run + i * kResolveRows);                          // first flat row
                items[cap + k0 + i] = (int)min((unsigned)kResolveRows, cb - i * kResolveRows);   // rows
                items[2 * cap + k0 + i] = b;
            }
        }
        carry_r += sr[1023];
        carry_k += sk[1023];
        __syncthreads();
    }
    if (tid < 9) {   // XCDs without images (n_img < 8) start at the end
        if (tid == 8 || ps[tid] >= n_img) {
            sxs[tid] = carry_r;
            sks[tid] = carry_k;
        }
    }
    __syncthreads();
    if (tid < 8) {
        xr[tid] = sxs[tid];
        xr[8 + tid] = sxs[tid + 1] - sxs[tid];
        ir[tid] = sks[tid];
        ir[8 + tid] = sks[tid + 1] - sks[tid];
    }
    if (tid == 0) okey[n_img] = carry_r;
}
__global__ __launch_bounds__(256) void resolve_flatten_kernel(const unsigned* __restrict__ okey,
                                                              const int* __restrict__ oimg, int n_img,
                                                              const int64_t* __restrict__ list,
                                                              int64_t* __restrict__ flat,
                                                              const unsigned* __restrict__ overflow) {
    if (*overflow != 0u) return;
    const unsigned total = okey[n_img];
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        int lo = 0, hi = n_img - 1;   // the last position with okey <= t
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (okey[mid] <= t) lo = mid;
            else hi = mid - 1;
        }
        flat[t] = list[(size_t)oimg[lo] * kResolveBucket + (t - okey[lo])];
    }
}

// Up to kResolveRows undecided rows of one image b per workgroup (the items of the XCD-major
// order above, dealt to the XCD's own workgroups): the query rows staged in LDS, image b's int8
// rows read ONCE for the whole batch by the candidate prefilter (16 candidates x the batch's 16
// rows per MFMA chain, four tiles' loads in flight per wave: 0.41 -> 0.30 ms per C3 call against
// v_dot4 over the candidates, profiles/r5/ab/resolve_mfma_prefilter_ab_r5.txt), then the f64
// distances of each row's candidates by one wave per row (any order: a tie-aware top two, lowest
// index on equal distances) — resolve_row's result.  At C3 a row keeps ~2 candidates, so the
// prefilter (4096 int8 rows of image b per row in the per-row form) is most of the work.
template <int D, typename OutT>
__global__ __launch_bounds__(256) void match_resolve_batched_kernel(
    const int8_t* __restrict__ q /* the matcher's (shifted) int8 operands */, const int32_t* __restrict__ norms,
    const float* __restrict__ x, const int32_t* __restrict__ nk, int m_pad,
    const int32_t* __restrict__ pairs, int n_img, const double* __restrict__ erow, const double* __restrict__ eimg,
    double s, double rn2, double rd2, OutT* __restrict__ m0, unsigned* __restrict__ n_resolved,
    const int64_t* __restrict__ flat, const int* __restrict__ items, const unsigned* __restrict__ ir,
    const unsigned* __restrict__ overflow) {
    constexpr int W4 = D / 4, R = kResolveRows;
    __shared__ __attribute__((aligned(16))) int sqa[R][W4];
    __shared__ float sxa[R][D];
    __shared__ int scand[R][kResolveCap];
    __shared__ int sncand[R], sna[R], sccd[R];
    __shared__ double stq[R];
    __shared__ int64_t se_[R];
    if (*overflow != 0u) return;   // match_resolve_kernel takes every row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = n_img * (kResolveBucket / kResolveRows + 1);
    const int xcd = blockIdx.x % 8, nx = (gridDim.x + 7 - xcd) / 8;
    const unsigned ib = ir[xcd], in = ir[8 + xcd];
    for (unsigned k = blockIdx.x / 8; k < in; k += nx) {
        const int f0 = items[ib + k], nr = items[cap + ib + k], b = items[2 * cap + ib + k];
        const int nb = nk[b];
        for (int t = tid; t < nr * W4; t += 256) {
            const int r = t / W4, w = t % W4;
            const int64_t e = flat[f0 + r];
            const size_t arow = (size_t)pairs[2 * (int)(e / m_pad)] * m_pad + (int)(e % m_pad);
            sqa[r][w] = reinterpret_cast<const int*>(q + arow * D)[w];
        }
        for (int t = tid; t < nr * D; t += 256) {
            const int r = t / D, kk = t % D;
            const int64_t e = flat[f0 + r];
            const size_t arow = (size_t)pairs[2 * (int)(e / m_pad)] * m_pad + (int)(e % m_pad);
            sxa[r][kk] = x[arow * D + kk];
        }
        if (tid < R) sncand[tid] = 0;
        __syncthreads();
        for (int r = wave; r < nr; r += 4) {
            int na = 0;
            for (int w = lane; w < W4; w += 64) na = __builtin_amdgcn_sdot4(sqa[r][w], sqa[r][w], na, false);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) na += __shfl_xor(na, off);
            if (lane == 0) {
                const int64_t e = flat[f0 + r];
                const size_t arow = (size_t)pairs[2 * (int)(e / m_pad)] * m_pad + (int)(e % m_pad);
                const double se = (erow[arow] + eimg[b]) * s * (1.0 + 1e-12);
                const double bq = (se + (mark_sqrt_d2<OutT>((int)m0[e]) + se) * (1.0 + 1e-12)) * (1.0 + 1e-12);
                stq[r] = floor(bq * bq) + 1.0;   // every j with D_j <= tq may reach the top two
                sna[r] = na;
                sccd[r] = norms[arow] - na;   // the matcher's norms carry c^2 d of its operand shift c
                se_[r] = e;
            }
        }
        __syncthreads();
        {   // the prefilter on the matrix cores: <q_j, q_r> for 16 candidates j x the batch's 16 rows r
            // per v_mfma_i32_16x16x64_i8 chain (the matcher's operands, shifted by c: D_j is
            // shift-invariant, |q_j|^2 = norms_j - c^2 d, and the int32 dots are exact, so the
            // candidate set is the one the per-row form tests)
            using M16 = Mfma<16>;
            constexpr int KK = D / M16::KB;
            const int lr = lane & 15, grp = lane >> 4;   // lane: row lr of the batch, candidates 4 grp + e
            i32x4 bqv[KK];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) bqv[kk] = *reinterpret_cast<const i32x4*>(&sqa[lr][kk * 16 + grp * 4]);
            const bool live = lr < nr;
            const long long na_r = live ? (long long)sna[lr] - sccd[lr] : 0;   // |q_r|^2 - c^2 d
            const double tq_r = live ? stq[lr] : -1.0;
            const size_t bbase = (size_t)b * m_pad;
            constexpr int TG = 4;   // 16-candidate tiles per wave step, their loads issued together
            for (int jg = wave * 16; jg < nb; jg += 64 * TG) {
                i32x4 av[TG][KK], nv[TG];
#pragma unroll
                for (int t = 0; t < TG; ++t) {
                    const int j0 = min(jg + 64 * t, m_pad - 16);   // whole rows (m_pad % 128 == 0)
                    const int8_t* rp = q + (bbase + j0 + lr) * D + grp * 16;
#pragma unroll
                    for (int kk = 0; kk < KK; ++kk) av[t][kk] = *reinterpret_cast<const i32x4*>(rp + kk * M16::KB);
                    nv[t] = *reinterpret_cast<const i32x4*>(norms + bbase + j0 + 4 * grp);   // norms of the 4 candidates
                }
#pragma unroll
                for (int t = 0; t < TG; ++t) {
                    const int j0 = jg + 64 * t;
                    i32x4 acc = {0, 0, 0, 0};
#pragma unroll
                    for (int kk = 0; kk < KK; ++kk) acc = M16::run(av[t][kk], bqv[kk], acc);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int j = j0 + 4 * grp + e;
                        if (live && j < nb && (double)(na_r + nv[t][e] - 2LL * acc[e]) <= tq_r) {
                            const int pos = atomicAdd(&sncand[lr], 1);
                            if (pos < kResolveCap) scand[lr][pos] = j;
                        }
                    }
                }
            }
        }
        __syncthreads();
        for (int r = wave; r < nr; r += 4) {   // f64 distances of the row's candidates
            const int ncand = sncand[r];
            const bool every = ncand > kResolveCap;
#ifdef SFMHIP_RESOLVE_PROF
            if (lane == 0) {
                atomicAdd(&g_rprof[0], 1ull);
                atomicAdd(&g_rprof[1], (unsigned long long)ncand);
                if (every) atomicAdd(&g_rprof[2], 1ull);
                atomicMax(&g_rprof[3], (unsigned long long)ncand);
                atomicAdd(&g_rprof[4 + min(ncand / 64, 11)], 1ull);
            }
#endif
            const int nc = every ? nb : ncand;
            double v1 = __builtin_inf(), v2 = __builtin_inf();
            int j1 = INT_MAX;
            for (int t = lane; t < nc; t += 64) {
                const int j = every ? t : scand[r][t];
                const float4* xb = reinterpret_cast<const float4*>(x + ((size_t)b * m_pad + j) * D);
                double acc = 0.0;
                for (int k4 = 0; k4 < D / 4; ++k4) {
                    const float4 xv = xb[k4];
                    double df;
                    df = (double)sxa[r][4 * k4] - (double)xv.x;
                    acc = acc + df * df;
                    df = (double)sxa[r][4 * k4 + 1] - (double)xv.y;
                    acc = acc + df * df;
                    df = (double)sxa[r][4 * k4 + 2] - (double)xv.z;
                    acc = acc + df * df;
                    df = (double)sxa[r][4 * k4 + 3] - (double)xv.w;
                    acc = acc + df * df;
                }
                if (acc < v1 || (acc == v1 && j < j1)) { v2 = v1; v1 = acc; j1 = j; }
                else if (acc < v2) v2 = acc;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double o1 = __shfl_xor(v1, off), o2 = __shfl_xor(v2, off);
                const int oj = __shfl_xor(j1, off);
                const bool mine = v1 < o1 || (v1 == o1 && j1 < oj);
                const double n2 = mine ? fmin(v2, o1) : fmin(o2, v1);
                if (!mine) { v1 = o1; j1 = oj; }
                v2 = n2;
            }
            const double p1 = rd2 * v1, e1 = __builtin_fma(rd2, v1, -p1);
            const double p2 = rn2 * v2, e2 = __builtin_fma(rn2, v2, -p2);
            const bool acc_ok = p1 < p2 || (p1 == p2 && e1 < e2);
            if (lane == 0) {
                m0[se_[r]] = (OutT)(acc_ok ? j1 : -1);
                if (n_resolved) atomicAdd(n_resolved, 1u);
            }
        }
        __syncthreads();   // the batch's LDS is reused by the next item
    }
}

struct ResolveLaunch {
    const int8_t* desc;        // the matcher's (shifted) int8 operands, with their norms: the batched prefilter
    const int32_t* norms;
    const int8_t* desc_q;      // the unshifted int8 rows: the fallback scan
    const float* desc_f;
    const double *resid_row, *resid_img;
    const int32_t* n_kpts;
    int n_img, m_pad, d;
    const int32_t* pairs;
    int P;
    double s, rn2, rd2;        // 1 (MODE_SIFT) or 127, ratio_num^2, ratio_den^2
    uint32_t* n_resolved;
    int n_cu;
    char* scratch;             // the call's scratch buffer and its layout
    ResolveScratch lay;
    hipStream_t stream;
    template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(scratch + off); }
};

template <int D, typename OutT>
static void launch_resolve_d(const ResolveLaunch& r, OutT* matches0) {
    int64_t *list = r.at<int64_t>(r.lay.list), *flat = r.at<int64_t>(r.lay.flat);
    unsigned *cnt = r.at<unsigned>(r.lay.cnt), *flag = r.at<unsigned>(r.lay.flag);
    unsigned *okey = r.at<unsigned>(r.lay.okey), *ir = r.at<unsigned>(r.lay.ir);
    int *oimg = r.at<int>(r.lay.oimg), *items = r.at<int>(r.lay.items);
    const int64_t total = (int64_t)r.P * r.m_pad;
    const int64_t nchunk = (total + 63) / 64;
    const int rgrid = (int)std::min<int64_t>((nchunk + 3) / 4, (int64_t)r.n_cu * 8);
    const int rxgrid = r.n_cu * 2;   // a multiple of 8: every XCD gets the same number of blocks
    hipStream_t s = r.stream;
    hipLaunchKernelGGL(resolve_collect_kernel<OutT>, dim3(rgrid), dim3(256), 0, s, matches0, total, r.m_pad, r.pairs, cnt,
                       list, flag);
    hipLaunchKernelGGL(resolve_offsets_kernel, dim3(1), dim3(1024), 0, s, cnt, r.n_img, r.at<unsigned>(r.lay.off), okey,
                       oimg, r.at<unsigned>(r.lay.xr), items, ir, flag);
    hipLaunchKernelGGL(resolve_flatten_kernel, dim3(r.n_cu), dim3(256), 0, s, okey, oimg, r.n_img, list, flat, flag);
    hipLaunchKernelGGL((match_resolve_batched_kernel<D, OutT>), dim3(rxgrid), dim3(256), 0, s, r.desc, r.norms, r.desc_f,
                       r.n_kpts, r.m_pad, r.pairs, r.n_img, r.resid_row, r.resid_img, r.s, r.rn2, r.rd2, matches0,
                       r.n_resolved, flat, items, ir, flag);
    hipLaunchKernelGGL((match_resolve_kernel<D, OutT>), dim3(rgrid), dim3(256), 0, s, r.desc_q, r.desc_f, r.n_kpts,
                       r.m_pad, r.pairs, r.P, r.resid_row, r.resid_img, r.s, r.rn2, r.rd2, matches0, r.n_resolved, flag);
}

template <typename OutT>
int launch_resolve(const ResolveLaunch& r, OutT* matches0) {
    switch (r.d) {
        case 64: launch_resolve_d<64>(r, matches0); break;
        case 128: launch_resolve_d<128>(r, matches0); break;
        case 256: launch_resolve_d<256>(r, matches0); break;
        default: return SFMHIP_E_UNSUPPORTED;
    }
    return check_launch("match_resolve_kernel");
}
template int launch_resolve<int32_t>(const ResolveLaunch&, int32_t*);
template int launch_resolve<int16_t>(const ResolveLaunch&, int16_t*);

}  // namespace sfmhip

using namespace sfmhip;

#ifdef SFMHIP_RESOLVE_PROF
extern "C" int sfmhip_debug_resolve_prof(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(sfmhip::g_rprof), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -2;
}
#endif

extern "C" int sfmhip_desc_residual(const float* desc_f, const int8_t* desc_q, int n_img, int m_pad, int d,
                                    const int32_t* n_kpts, int mode, double* resid_row, double* resid_img,
                                    void* stream) {
    SFMHIP_REQUIRE(desc_f && desc_q && n_kpts && resid_row && resid_img, "sfmhip_desc_residual: null pointer");
    SFMHIP_REQUIRE(n_img > 0 && m_pad > 0 && d > 0, "sfmhip_desc_residual: bad shape");
    SFMHIP_REQUIRE(mode == 0 || mode == 1, "sfmhip_desc_residual: mode must be 0 or 1");
    const int64_t rows = (int64_t)n_img * m_pad;
    SFMHIP_REQUIRE(rows < INT_MAX, "sfmhip_desc_residual: too many rows");
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(resid_img, 0, (size_t)n_img * sizeof(double), s) != hipSuccess) return check_launch("memset");
    hipLaunchKernelGGL(desc_residual_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, s, desc_f, desc_q, (int)rows, m_pad,
                       d, n_kpts, mode, resid_row, reinterpret_cast<unsigned long long*>(resid_img));
    return check_launch("desc_residual_kernel");
}

// What the FP6 entries bring (null for the int8 entries): dense = the packed e2m3 codes of desc
// (sfmhip_desc_pack_fp6; desc = desc_q = the grid values g, mode 1, no distance outputs), and with the _kv
// entries the bank's key values h / hf (sfmhip_match_key_values); without them they are built from keys in
// this call's scratch.  SFMHIP_MATCH_FP6=0 runs the int8 value-only kernel on g instead.
struct Fp6Bank {
    const uint8_t* dense;
    const int32_t* h;
    const float* hf;
};

template <typename OutT>
static int match_exact_impl(const int8_t* desc, const int32_t* norms, const int32_t* keys,
                            const int8_t* desc_q, const float* desc_f, const double* resid_row,
                            const double* resid_img, int mode, const int32_t* n_kpts, int n_img,
                            int m_pad, int d, const int32_t* pairs, int P, int ratio_num, int ratio_den,
                            OutT* matches0, int32_t* dist1, int32_t* dist2, uint32_t* n_resolved,
                            void* stream, const Fp6Bank* bank) {
    // validate
    const uint8_t* dense = bank ? bank->dense : nullptr;
    const bool fp6 = dense && knobs().match_fp6 != 0;
    if (dense) {
        SFMHIP_REQUIRE(mode == 1 && !dist1 && !dist2 && (d == 128 || d == 256),
                       "sfmhip_match_pairs_exact_fp6: float mode, d in {128,256}, no distance outputs");
    }
    int n_iblk, nwg;
    if (int rc = check_match_call<OutT>(
            "sfmhip_match_pairs_exact", true, n_img, P, m_pad, mode, ratio_num, ratio_den,
            desc && norms && keys && desc_q && desc_f && resid_row && resid_img && n_kpts && pairs && matches0,
            fp6 ? kMatchFp6Rows : kMatchRows, &n_iblk, &nwg))
        return rc;
    if (P == 0) return SFMHIP_OK;
    hipStream_t s = as_stream(stream);
    if (n_resolved && hipMemsetAsync(n_resolved, 0, sizeof(uint32_t), s) != hipSuccess) return check_launch("memset");

    // take scratch: the resolve's regions and, for the value-only forms without the bank's, the key values
    // (no distance outputs: the int16 graph; dist.match_all_pairs_sharded)
    const ResolveScratch lay = resolve_scratch_layout(n_img, m_pad, !dist1 && !dist2, fp6, bank && bank->h);
    char* buf = nullptr;
    if (scratch_alloc(reinterpret_cast<void**>(&buf), lay.bytes, s) != hipSuccess) {
        (void)hipGetLastError();
        set_error("sfmhip_match_pairs_exact: scratch allocation failed");
        return SFMHIP_E_HIP;
    }
    if (hipMemsetAsync(buf + lay.cnt, 0, lay.off - lay.cnt, s) != hipSuccess) {   // cnt and flag
        scratch_free(buf, s);
        return check_launch("memset");
    }

    // run the filter.  SFMHIP_MATCH_CERT=0 (tests): every row through the exact pass
    const long long rn2 = (long long)ratio_num * ratio_num, rd2 = (long long)ratio_den * ratio_den;
    const CertArgs ca{resid_row, resid_img, mode == 0 ? 1.0 : 1.0 / 127.0, knobs().match_cert == 0 ? 1 : 0};
    FilterLaunch f{desc, norms, bank && bank->h ? bank->h : keys, n_kpts, m_pad, d, pairs, n_iblk, nwg, rn2, rd2, ca, s,
                   dist1, dist2, dense, bank ? bank->hf : nullptr};
    if (lay.h_count) {
        int32_t* h = reinterpret_cast<int32_t*>(buf + lay.h);
        float* hf = fp6 ? reinterpret_cast<float*>(buf + lay.hf) : nullptr;
        launch_key_values(keys, (int64_t)lay.h_count, h, hf, s);
        f.keys = h;
        f.hf = hf;
    }
    int rc = fp6 ? launch_match_fp6(f, matches0) : launch_match_cert(f, matches0);

    // run the resolve
    if (rc == SFMHIP_OK) {
        const ResolveLaunch r{desc, norms, desc_q, desc_f, resid_row, resid_img, n_kpts, n_img, m_pad, d, pairs, P,
                              mode == 0 ? 1.0 : 127.0, (double)rn2, (double)rd2, n_resolved, cu_count(), buf, lay, s};
        rc = launch_resolve(r, matches0);
    }
    if (rc == SFMHIP_E_UNSUPPORTED) set_error("sfmhip_match_pairs_exact: descriptor dim %d not in {64,128,256}", d);
    scratch_free(buf, s);
    return rc;
}

extern "C" int sfmhip_match_pairs_exact(const int8_t* desc, const int32_t* norms, const int32_t* keys,
                                        const int8_t* desc_q, const float* desc_f, const double* resid_row,
                                        const double* resid_img, int mode, const int32_t* n_kpts, int n_img,
                                        int m_pad, int d, const int32_t* pairs, int P, int ratio_num, int ratio_den,
                                        int32_t* matches0, int32_t* dist1, int32_t* dist2, uint32_t* n_resolved,
                                        void* stream) {
    return match_exact_impl(desc, norms, keys, desc_q, desc_f, resid_row, resid_img, mode, n_kpts, n_img, m_pad, d,
                            pairs, P, ratio_num, ratio_den, matches0, dist1, dist2, n_resolved, stream, nullptr);
}

extern "C" int sfmhip_match_pairs_exact_i16(const int8_t* desc, const int32_t* norms, const int32_t* keys,
                                            const int8_t* desc_q, const float* desc_f, const double* resid_row,
                                            const double* resid_img, int mode, const int32_t* n_kpts, int n_img,
                                            int m_pad, int d, const int32_t* pairs, int P, int ratio_num,
                                            int ratio_den, int16_t* matches0, uint32_t* n_resolved, void* stream) {
    return match_exact_impl(desc, norms, keys, desc_q, desc_f, resid_row, resid_img, mode, n_kpts, n_img, m_pad, d,
                            pairs, P, ratio_num, ratio_den, matches0, (int32_t*)nullptr, (int32_t*)nullptr,
                            n_resolved, stream, nullptr);
}

// The exact float mode with the FP6 certified filter (DESIGN.md K1''): g from sfmhip_desc_quantize_fp6, dense
// from sfmhip_desc_pack_fp6 on its codes, norms / keys from sfmhip_desc_prepare on g, the residual bounds from
// sfmhip_desc_residual on (desc_f, g, mode 1).  The same graph as sfmhip_match_pairs_exact.
extern "C" int sfmhip_match_pairs_exact_fp6(const uint8_t* dense, const int8_t* g, const int32_t* norms,
                                            const int32_t* keys, const float* desc_f, const double* resid_row,
                                            const double* resid_img, const int32_t* n_kpts, int n_img, int m_pad,
                                            int d, const int32_t* pairs, int P, int ratio_num, int ratio_den,
                                            int32_t* matches0, uint32_t* n_resolved, void* stream) {
    SFMHIP_REQUIRE(dense || P == 0, "sfmhip_match_pairs_exact_fp6: null pointer");
    const Fp6Bank bank{dense, nullptr, nullptr};
    return match_exact_impl(g, norms, keys, g, desc_f, resid_row, resid_img, 1, n_kpts, n_img, m_pad, d, pairs, P,
                            ratio_num, ratio_den, matches0, (int32_t*)nullptr, (int32_t*)nullptr, n_resolved, stream,
                            &bank);
}

extern "C" int sfmhip_match_pairs_exact_fp6_i16(const uint8_t* dense, const int8_t* g, const int32_t* norms,
                                                const int32_t* keys, const float* desc_f, const double* resid_row,
                                                const double* resid_img, const int32_t* n_kpts, int n_img, int m_pad,
                                                int d, const int32_t* pairs, int P, int ratio_num, int ratio_den,
                                                int16_t* matches0, uint32_t* n_resolved, void* stream) {
    SFMHIP_REQUIRE(dense || P == 0, "sfmhip_match_pairs_exact_fp6_i16: null pointer");
    const Fp6Bank bank{dense, nullptr, nullptr};
    return match_exact_impl(g, norms, keys, g, desc_f, resid_row, resid_img, 1, n_kpts, n_img, m_pad, d, pairs, P,
                            ratio_num, ratio_den, matches0, (int32_t*)nullptr, (int32_t*)nullptr, n_resolved, stream,
                            &bank);
}

extern "C" int sfmhip_match_pairs_exact_fp6_kv(const uint8_t* dense, const int8_t* g, const int32_t* norms,
                                               const int32_t* h, const float* hf, const float* desc_f,
                                               const double* resid_row, const double* resid_img, const int32_t* n_kpts,
                                               int n_img, int m_pad, int d, const int32_t* pairs, int P, int ratio_num,
                                               int ratio_den, int32_t* matches0, uint32_t* n_resolved, void* stream) {
    SFMHIP_REQUIRE((dense && hf) || P == 0, "sfmhip_match_pairs_exact_fp6_kv: null pointer");
    const Fp6Bank bank{dense, h, hf};
    return match_exact_impl(g, norms, h, g, desc_f, resid_row, resid_img, 1, n_kpts, n_img, m_pad, d, pairs, P,
                            ratio_num, ratio_den, matches0, (int32_t*)nullptr, (int32_t*)nullptr, n_resolved, stream,
                            &bank);
}

extern "C" int sfmhip_match_pairs_exact_fp6_kv_i16(const uint8_t* dense, const int8_t* g, const int32_t* norms,
                                                   const int32_t* h, const float* hf, const float* desc_f,
                                                   const double* resid_row, const double* resid_img,
                                                   const int32_t* n_kpts, int n_img, int m_pad, int d,
                                                   const int32_t* pairs, int P, int ratio_num, int ratio_den,
                                                   int16_t* matches0, uint32_t* n_resolved, void* stream) {
    SFMHIP_REQUIRE((dense && hf) || P == 0, "sfmhip_match_pairs_exact_fp6_kv_i16: null pointer");
    const Fp6Bank bank{dense, h, hf};
    return match_exact_impl(g, norms, h, g, desc_f, resid_row, resid_img, 1, n_kpts, n_img, m_pad, d, pairs, P,
                            ratio_num, ratio_den, matches0, (int32_t*)nullptr, (int32_t*)nullptr, n_resolved, stream,
                            &bank);
}
