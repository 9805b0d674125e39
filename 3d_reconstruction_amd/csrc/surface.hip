// surface.hip — V6: triangle mesh of the fused TSDF grid (T, Wt) by marching
// tetrahedra on the Kuhn 6-tetrahedron split (semantics: include/sfmhip.h V6,
// restated in numpy by tests/surface_ref.py).  Three phases:
//   classify  one LDS tile (with halo) of T/Wt per workgroup -> a 7-bit active-edge
//             mask per voxel and a triangle count per cell
//   scan      exclusive scans of popcount(mask) and of the triangle counts in linear
//             id order: block sums, one workgroup scanning the sums, the add.  No
//             workgroup ever waits for another, and no atomic decides an index.
//   emit      one vertex (+ normal) per active edge, the faces of every crossing cell
// All f32 with -ffp-contract=off: vertices and faces are bit-identical to the numpy form.
#include "common.h"
#include <climits>

namespace sfmhip {
namespace {

// ---- tables, generated at compile time --------------------------------------
// corner / offset code: bit 0 = x, bit 1 = y, bit 2 = z.  Tetrahedron t = lexicographic
// rank of the axis permutation (a, b, c); corners 0, e_a, e_a + e_b, (1,1,1).
constexpr int tet_code(int t, int j) {
    constexpr int perm[6][2] = {{0, 1}, {0, 2}, {1, 0}, {1, 2}, {2, 0}, {2, 1}};   // (a, b)
    return j == 0 ? 0 : j == 1 ? (1 << perm[t][0]) : j == 2 ? ((1 << perm[t][0]) | (1 << perm[t][1])) : 7;
}
constexpr unsigned tet_codes(int t) {   // 3 bits per tet corner
    return (unsigned)(tet_code(t, 0) | tet_code(t, 1) << 3 | tet_code(t, 2) << 6 | tet_code(t, 3) << 9);
}
// edge slot of an offset code: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) -> 0..6
__host__ __device__ constexpr int slot_of(int code) { return (int)((0x65423100u >> (4 * code)) & 7u); }

// Sign of ((v1-v0) x (v2-v0)) . (towards the outside corners) for the first triangle of
// case m of tetrahedron t with every vertex at its edge's midpoint (integers: doubled
// coordinates); < 0 = the last two vertices are swapped.  0 never happens (checked).
constexpr int tri_sign(int t, int m) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int j = 0; j < 4; ++j) {
        if ((m >> j) & 1) in[ni++] = j;
        else out[no++] = j;
    }
    int e[3][2] = {{0, 0}, {0, 0}, {0, 0}};
    if (ni == 1) {
        for (int v = 0; v < 3; ++v) { e[v][0] = in[0]; e[v][1] = out[v]; }
    } else if (ni == 3) {
        for (int v = 0; v < 3; ++v) { e[v][0] = in[v]; e[v][1] = out[0]; }
    } else if (ni == 2) {   // (pr, ps, qs)
        e[0][0] = in[0]; e[0][1] = out[0];
        e[1][0] = in[0]; e[1][1] = out[1];
        e[2][0] = in[1]; e[2][1] = out[1];
    } else {
        return 1;
    }
    int P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int v = 0; v < 3; ++v)
        for (int a = 0; a < 3; ++a) P[v][a] = ((tet_code(t, e[v][0]) >> a) & 1) + ((tet_code(t, e[v][1]) >> a) & 1);
    const int u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
    const int w[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    const int n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    int dot = 0;
    for (int a = 0; a < 3; ++a) {   // ni * no * (mean(out) - mean(in))
        int so = 0, si = 0;
        for (int j = 0; j < no; ++j) so += (tet_code(t, out[j]) >> a) & 1;
        for (int j = 0; j < ni; ++j) si += (tet_code(t, in[j]) >> a) & 1;
        dot += n[a] * (ni * so - no * si);
    }
    return dot;
}
constexpr unsigned swap_bits(int t) {   // bit m: case m of tetrahedron t swaps
    unsigned b = 0;
    for (int m = 1; m < 15; ++m)
        if (tri_sign(t, m) < 0) b |= 1u << m;
    return b;
}
constexpr bool tables_ok() {
    for (int t = 0; t < 6; ++t)
        for (int m = 1; m < 15; ++m)
            if (tri_sign(t, m) == 0) return false;
    return true;
}
static_assert(tables_ok(), "a marching-tetrahedra case has no orientation");

// triangles of a tetrahedron whose 4 corners have inside bits m
__device__ __forceinline__ int tet_tris(unsigned m) {
    const int n = __popc(m);
    return n == 2 ? 2 : (n & 1);   // 0,4 -> 0; 1,3 -> 1
}
// inside bits of tetrahedron T's corners out of the cell's 8 corner bits
template <int TT>
__device__ __forceinline__ unsigned tet_mask(unsigned in8) {
    constexpr unsigned c = tet_codes(TT);
    return ((in8 >> (c & 7)) & 1u) | (((in8 >> ((c >> 3) & 7)) & 1u) << 1) | (((in8 >> ((c >> 6) & 7)) & 1u) << 2) |
           (((in8 >> ((c >> 9) & 7)) & 1u) << 3);
}
__device__ __forceinline__ int cell_tris(unsigned in8) {
    return tet_tris(tet_mask<0>(in8)) + tet_tris(tet_mask<1>(in8)) + tet_tris(tet_mask<2>(in8)) +
           tet_tris(tet_mask<3>(in8)) + tet_tris(tet_mask<4>(in8)) + tet_tris(tet_mask<5>(in8));
}

// ---- classify -----------------------------------------------------------------
// Tile of 64 x 4 x 8 voxels (x fastest: a wave reads one 256-B row), halo of one voxel
// on every side.  LDS holds T, NaN where the voxel is outside the grid or not observed
// (observed: Wt >= min_weight and T finite), then the validity of every cell that
// touches a tile voxel.
constexpr int kTX = 64, kTY = 4, kTZ = 8;
constexpr int kLX = kTX + 2, kLY = kTY + 2, kLZ = kTZ + 2;
constexpr int kCX = kTX + 1, kCY = kTY + 1, kCZ = kTZ + 1;

__global__ __launch_bounds__(256) void surf_classify_kernel(const float* __restrict__ T, const float* __restrict__ Wt,
                                                            int D, int H, int W, int z0, int z1, float iso, float minw,
                                                            uint8_t* __restrict__ mask, int32_t* __restrict__ tri_cnt) {
    __shared__ float sT[kLZ * kLY * kLX];
    __shared__ uint8_t sV[kCZ * kCY * kCX];
    const int tid = threadIdx.x;
    const int bx = blockIdx.x * kTX, by = blockIdx.y * kTY, bz = z0 + blockIdx.z * kTZ;
    for (int i = tid; i < kLZ * kLY * kLX; i += 256) {
        const int lx = i % kLX, ly = (i / kLX) % kLY, lz = i / (kLX * kLY);
        const int x = bx + lx - 1, y = by + ly - 1, z = bz + lz - 1;
        float v = __builtin_nanf("");
        if (x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D) {
            const size_t g = ((size_t)z * H + y) * W + x;
            const float t = T[g], w = Wt[g];
            if (w >= minw && isfinite(t)) v = t;
        }
        sT[i] = v;
    }
    __syncthreads();
    // cell (cx, cy, cz) of the tile has its origin at tile voxel (cx-1, cy-1, cz-1)
    for (int i = tid; i < kCZ * kCY * kCX; i += 256) {
        const int cx = i % kCX, cy = (i / kCX) % kCY, cz = i / (kCX * kCY);
        const int gz = bz + cz - 1;
        bool ok = gz >= z0 && gz < z1;   // out-of-grid corners are NaN already
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float t = sT[((cz + (c >> 2)) * kLY + cy + ((c >> 1) & 1)) * kLX + cx + (c & 1)];
            ok = ok && (t == t);
        }
        sV[i] = ok ? 1 : 0;
    }
    __syncthreads();
    const int tx = tid & 63, ty = tid >> 6;
    const int x = bx + tx, y = by + ty;
    if (x >= W || y >= H) return;
    const int lx = tx + 1, ly = ty + 1;
    for (int tz = 0; tz < kTZ; ++tz) {
        const int z = bz + tz, lz = tz + 1;
        if (z > z1) break;
        auto tv = [&](int c) { return sT[((lz + (c >> 2)) * kLY + ly + ((c >> 1) & 1)) * kLX + lx + (c & 1)]; };
        // validity of the cell whose origin is this voxel + (dx, dy, dz), each in {-1, 0}
        auto cv = [&](int dx, int dy, int dz) { return sV[((lz + dz) * kCY + ly + dy) * kCX + lx + dx] != 0; };
        const float t0 = tv(0);
        unsigned in8 = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) in8 |= (tv(c) < iso ? 1u : 0u) << c;
        unsigned m = 0;
        if (t0 == t0) {
            const bool c000 = cv(0, 0, 0);
            const bool has[7] = {
                c000 || cv(0, -1, 0) || cv(0, 0, -1) || cv(0, -1, -1),   // (1,0,0)
                c000 || cv(-1, 0, 0) || cv(0, 0, -1) || cv(-1, 0, -1),   // (0,1,0)
                c000 || cv(-1, 0, 0) || cv(0, -1, 0) || cv(-1, -1, 0),   // (0,0,1)
                c000 || cv(0, 0, -1),                                    // (1,1,0)
                c000 || cv(0, -1, 0),                                    // (1,0,1)
                c000 || cv(-1, 0, 0),                                    // (0,1,1)
                c000};                                                   // (1,1,1)
            constexpr int code[7] = {1, 2, 4, 3, 5, 6, 7};
            const unsigned i0 = in8 & 1u;
#pragma unroll
            for (int k = 0; k < 7; ++k)
                if (has[k] && ((in8 >> code[k]) & 1u) != i0) m |= 1u << k;
        }
        mask[((size_t)(z - z0) * H + y) * W + x] = (uint8_t)m;
        if (z < z1 && y < H - 1 && x < W - 1)
            tri_cnt[((size_t)(z - z0) * (H - 1) + y) * (W - 1) + x] = cv(0, 0, 0) ? cell_tris(in8) : 0;
    }
}

// ---- scan -----------------------------------------------------------------------
// Two sequences per call: a = popcount(edge mask) of nv voxels, b = the triangle counts
// of nt cells (in tri_off, scanned in place).  Each gets one extra trailing entry, so
// vert_off[nv] / tri_off[nt] hold the totals.  A workgroup owns 4096 consecutive items,
// 16 per thread.  Workgroups [0, nba) serve a, the rest b.
constexpr int kScanPer = 16, kScanChunk = 256 * kScanPer;

struct ScanJob {
    const uint8_t* mask;
    int32_t* voff;
    int64_t nv;
    int32_t* toff;
    int64_t nt;
    int nba;
};

__device__ __forceinline__ int block_excl_scan(int v, int& total) {
    __shared__ int ws[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < w) base += ws[i];
        tot += ws[i];
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

// the 16 items of this thread (0 past the end); the work arrays are 16-byte aligned
__device__ __forceinline__ void scan_load(const ScanJob& J, bool isb, int64_t i, int* v) {
    const int64_t n = isb ? J.nt : J.nv;
    if (i + kScanPer <= n) {
        if (isb) {
            const int4* p = reinterpret_cast<const int4*>(J.toff + i);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int4 r = p[q];
                v[4 * q] = r.x; v[4 * q + 1] = r.y; v[4 * q + 2] = r.z; v[4 * q + 3] = r.w;
            }
        } else {
            const uint4 r = *reinterpret_cast<const uint4*>(J.mask + i);
            const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int j = 0; j < kScanPer; ++j) v[j] = __popc((w[j >> 2] >> (8 * (j & 3))) & 0x7fu);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        v[j] = 0;
        if (i + j < n) v[j] = isb ? J.toff[i + j] : __popc(J.mask[i + j] & 0x7fu);
    }
}

__global__ __launch_bounds__(256) void surf_scan_sums_kernel(ScanJob J, int32_t* __restrict__ sums) {
    const bool isb = (int)blockIdx.x >= J.nba;
    const int64_t i = ((int64_t)(isb ? blockIdx.x - J.nba : blockIdx.x) * 256 + threadIdx.x) * kScanPer;
    int v[kScanPer], s = 0;
    scan_load(J, isb, i, v);
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) s += v[j];
    int tot;
    block_excl_scan(s, tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// workgroup 0: sums[0, nba), workgroup 1: sums[nba, nb) -> exclusive prefixes in place
// (int32: meaningful while the total fits, which the host checks) and the 64-bit totals
__global__ __launch_bounds__(256) void surf_scan_top_kernel(int32_t* __restrict__ sums, int nba, int nb,
                                                            int64_t* __restrict__ totals) {
    const int lo = blockIdx.x == 0 ? 0 : nba, hi = blockIdx.x == 0 ? nba : nb;
    int64_t carry = 0;
    for (int b0 = lo; b0 < hi; b0 += 256) {
        const int b = b0 + (int)threadIdx.x;
        const int v = b < hi ? sums[b] : 0;
        int tot;
        const int ex = block_excl_scan(v, tot);
        if (b < hi) sums[b] = (int32_t)(carry + ex);
        carry += tot;   // a chunk holds at most 256 * 4096 * 12 < 2^31
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void surf_scan_add_kernel(ScanJob J, const int32_t* __restrict__ sums) {
    const bool isb = (int)blockIdx.x >= J.nba;
    const int64_t i = ((int64_t)(isb ? blockIdx.x - J.nba : blockIdx.x) * 256 + threadIdx.x) * kScanPer;
    const int64_t n = isb ? J.nt : J.nv;   // n + 1 outputs
    int v[kScanPer], s = 0;
    scan_load(J, isb, i, v);
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) s += v[j];
    int tot;
    int run = sums[blockIdx.x] + block_excl_scan(s, tot);
    int32_t* out = (isb ? J.toff : J.voff) + i;
    if (i + kScanPer <= n + 1) {
        int4* o4 = reinterpret_cast<int4*>(out);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int4 r;
            r.x = run; run += v[4 * q];
            r.y = run; run += v[4 * q + 1];
            r.z = run; run += v[4 * q + 2];
            r.w = run; run += v[4 * q + 3];
            o4[q] = r;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        if (i + j <= n) out[j] = run;
        run += v[j];
    }
}

// ---- emit -------------------------------------------------------------------------
struct Geo {
    float bmin[3], step[3];   // x, y, z
};

// gradient of T at voxel (x, y, z): central difference where both neighbours along the
// axis are in the grid and observed, one-sided where one is, else 0
__device__ __forceinline__ void tsdf_gradient(const float* __restrict__ T, const float* __restrict__ Wt, int D, int H,
                                              int W, int x, int y, int z, float minw, const Geo& G, float* g) {
    const size_t c = ((size_t)z * H + y) * W + x;
    const float t = T[c];
    const int pos[3] = {x, y, z}, dim[3] = {W, H, D};
    const size_t stride[3] = {1, (size_t)W, (size_t)W * H};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float tp = 0.f, tm = 0.f;
        bool op = false, om = false;
        if (pos[a] + 1 < dim[a]) {
            tp = T[c + stride[a]];
            op = Wt[c + stride[a]] >= minw && isfinite(tp);
        }
        if (pos[a] >= 1) {
            tm = T[c - stride[a]];
            om = Wt[c - stride[a]] >= minw && isfinite(tm);
        }
        float v = 0.f;
        if (op && om) v = (tp - tm) / (2.0f * G.step[a]);
        else if (op) v = (tp - t) / G.step[a];
        else if (om) v = (t - tm) / G.step[a];
        g[a] = v;
    }
}

__global__ __launch_bounds__(256) void surf_vertex_kernel(const float* __restrict__ T, const float* __restrict__ Wt,
                                                          int D, int H, int W, int z0, int64_t nv, float iso,
                                                          float minw, Geo G, const uint8_t* __restrict__ mask,
                                                          const int32_t* __restrict__ voff,
                                                          float* __restrict__ verts, float* __restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    unsigned m = mask[i] & 0x7fu;
    if (!m) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), z = z0 + (int)(i / ((int64_t)W * H));
    const size_t c = ((size_t)z * H + y) * W + x;
    const float t0 = T[c];
    float g0[3] = {0.f, 0.f, 0.f};
    if (normals) tsdf_gradient(T, Wt, D, H, W, x, y, z, minw, G, g0);
    size_t o = (size_t)voff[i] * 3;
    const int pos[3] = {x, y, z};
    constexpr int code[7] = {1, 2, 4, 3, 5, 6, 7};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        if (!((m >> k) & 1u)) continue;
        const int d[3] = {code[k] & 1, (code[k] >> 1) & 1, code[k] >> 2};
        const float t1 = T[((size_t)(z + d[2]) * H + y + d[1]) * W + x + d[0]];
        const float s = (iso - t0) / (t1 - t0);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float g = (float)pos[a] + s * (float)d[a];
            verts[o + a] = G.bmin[a] + g * G.step[a];
        }
        if (normals) {
            float g1[3], n[3];
            tsdf_gradient(T, Wt, D, H, W, x + d[0], y + d[1], z + d[2], minw, G, g1);
#pragma unroll
            for (int a = 0; a < 3; ++a) n[a] = (1.0f - s) * g0[a] + s * g1[a];
            const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            const bool ok = len > 0.f && isfinite(len);
#pragma unroll
            for (int a = 0; a < 3; ++a) normals[o + a] = ok ? n[a] / len : 0.f;
        }
        o += 3;
    }
}

// V7 vertex colours: the fused colour of voxel v, sum / n per channel (u32 -> f32 RN, IEEE
// division); false when the voxel never took a sample
__device__ __forceinline__ bool voxel_colour(const uint4* __restrict__ C, size_t v, float* col) {
    const uint4 r = C[v];
    if (r.w == 0u) return false;
    const float n = (float)r.w;
    col[0] = (float)r.x / n;
    col[1] = (float)r.y / n;
    col[2] = (float)r.z / n;
    return true;
}

// One thread per voxel, like surf_vertex_kernel: for each active edge the same s, the two
// endpoints' colours interpolated (the coloured one where only one is), 4 bytes per vertex.
__global__ __launch_bounds__(256) void surf_colour_kernel(const float* __restrict__ T, const uint4* __restrict__ C,
                                                          int D, int H, int W, int z0, int64_t nv, float iso,
                                                          const uint8_t* __restrict__ mask,
                                                          const int32_t* __restrict__ voff,
                                                          uchar4* __restrict__ rgba) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const unsigned m = mask[i] & 0x7fu;
    if (!m) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), z = z0 + (int)(i / ((int64_t)W * H));
    const size_t c = ((size_t)z * H + y) * W + x;
    const float t0 = T[c];
    float ca[3] = {0.f, 0.f, 0.f};
    const bool ha = voxel_colour(C, c, ca);
    size_t o = (size_t)voff[i];
    constexpr int code[7] = {1, 2, 4, 3, 5, 6, 7};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        if (!((m >> k) & 1u)) continue;
        // an active edge's far endpoint is in the grid (V6); a mask that says otherwise is not followed
        if (x + (code[k] & 1) >= W || y + ((code[k] >> 1) & 1) >= H || z + (code[k] >> 2) >= D) {
            ++o;
            continue;
        }
        const size_t c1 = ((size_t)(z + (code[k] >> 2)) * H + y + ((code[k] >> 1) & 1)) * W + x + (code[k] & 1);
        const float t1 = T[c1];
        const float s = (iso - t0) / (t1 - t0);
        float cb[3] = {0.f, 0.f, 0.f};
        const bool hb = voxel_colour(C, c1, cb);
        unsigned char out[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float mm = ha && hb ? ca[a] + s * (cb[a] - ca[a]) : ha ? ca[a] : hb ? cb[a] : 0.f;
            out[a] = (unsigned char)__builtin_rintf(fminf(255.f, fmaxf(0.f, mm)));
        }
        rgba[o] = make_uchar4(out[0], out[1], out[2], ha || hb ? 255 : 0);
        ++o;
    }
}

struct CellCtx {
    const uint8_t* mask;
    const int32_t* voff;
    int H, W, x, y, zl;   // zl = z - z0 (the work arrays are local to the range)
};

// index of the vertex on the edge between corners with codes ca, cb (one contains the other)
__device__ __forceinline__ int edge_vertex(const CellCtx& C, int ca, int cb) {
    const int lo = min(ca, cb), k = slot_of(ca ^ cb);
    const size_t ow = ((size_t)(C.zl + (lo >> 2)) * C.H + C.y + ((lo >> 1) & 1)) * C.W + C.x + (lo & 1);
    return C.voff[ow] + __popc(C.mask[ow] & ((1u << k) - 1u));
}

template <int TT>
__device__ __forceinline__ int32_t* emit_tet(const CellCtx& C, unsigned in8, int32_t* __restrict__ f) {
    constexpr unsigned codes = tet_codes(TT), swp = swap_bits(TT);
    const unsigned m = tet_mask<TT>(in8);
    const int n = __popc(m);
    if (n == 0 || n == 4) return f;
    auto code = [&](int j) { return (int)((codes >> (3 * j)) & 7u); };
    auto put = [&](int a, int b, int c) {
        const bool sw = (swp >> m) & 1u;
        f[0] = a;
        f[1] = sw ? c : b;
        f[2] = sw ? b : c;
        f += 3;
    };
    if (n == 2) {
        unsigned mi = m, mo = ~m & 15u;
        const int p = code(__ffs(mi) - 1);
        mi &= mi - 1;
        const int q = code(__ffs(mi) - 1);
        const int r = code(__ffs(mo) - 1);
        mo &= mo - 1;
        const int s = code(__ffs(mo) - 1);
        const int pr = edge_vertex(C, p, r), ps = edge_vertex(C, p, s), qs = edge_vertex(C, q, s),
                  qr = edge_vertex(C, q, r);
        put(pr, ps, qs);
        put(pr, qs, qr);
        return f;
    }
    // one corner alone on its side: its three edges, the other corners ascending
    const unsigned one = n == 1 ? m : (~m & 15u);
    unsigned rest = ~one & 15u;
    const int a = code(__ffs(one) - 1);
    const int b0 = code(__ffs(rest) - 1);
    rest &= rest - 1;
    const int b1 = code(__ffs(rest) - 1);
    rest &= rest - 1;
    const int b2 = code(__ffs(rest) - 1);
    put(edge_vertex(C, a, b0), edge_vertex(C, a, b1), edge_vertex(C, a, b2));
    return f;
}

__global__ __launch_bounds__(256) void surf_face_kernel(const float* __restrict__ T, int H, int W, int z0, int64_t nt,
                                                        float iso, const uint8_t* __restrict__ mask,
                                                        const int32_t* __restrict__ voff,
                                                        const int32_t* __restrict__ toff, int32_t* __restrict__ faces) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const int off = toff[i];
    if (toff[i + 1] == off) return;   // a crossing cell is valid: every corner is observed
    CellCtx C;
    C.mask = mask;
    C.voff = voff;
    C.H = H;
    C.W = W;
    C.x = (int)(i % (W - 1));
    C.y = (int)((i / (W - 1)) % (H - 1));
    C.zl = (int)(i / ((int64_t)(W - 1) * (H - 1)));
    unsigned in8 = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float t = T[((size_t)(z0 + C.zl + (c >> 2)) * H + C.y + ((c >> 1) & 1)) * W + C.x + (c & 1)];
        in8 |= (t < iso ? 1u : 0u) << c;
    }
    int32_t* f = faces + (size_t)off * 3;
    f = emit_tet<0>(C, in8, f);
    f = emit_tet<1>(C, in8, f);
    f = emit_tet<2>(C, in8, f);
    f = emit_tet<3>(C, in8, f);
    f = emit_tet<4>(C, in8, f);
    emit_tet<5>(C, in8, f);
}

// ---- host -------------------------------------------------------------------------
struct Range {
    int64_t nv, nt;   // voxels of layers [z0, z1], cells of layers [z0, z1)
    bool empty;
};

int check_args(const char* fn, int D, int H, int W, int z0, int z1, float min_weight, Range& R) {
    SFMHIP_REQUIRE(D >= 1 && H >= 1 && W >= 1, "%s: bad grid shape (%d,%d,%d)", fn, D, H, W);
    SFMHIP_REQUIRE(0 <= z0 && z0 <= z1 && z1 <= D - 1, "%s: bad z range [%d, %d) for %d cell layers", fn, z0, z1,
                   D - 1);
    SFMHIP_REQUIRE(min_weight > 0.f, "%s: min_weight must be > 0", fn);
    R.empty = z0 == z1 || H < 2 || W < 2;
    R.nv = (int64_t)(z1 - z0 + 1) * H * W;
    R.nt = R.empty ? 0 : (int64_t)(z1 - z0) * (H - 1) * (W - 1);
    if (!R.empty && R.nv >= INT32_MAX) {
        set_error("%s: %lld voxels in one range; split it into z-slabs", fn, (long long)R.nv);
        return SFMHIP_E_OVERFLOW;
    }
    return SFMHIP_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_tsdf_surface_count(const float* T, const float* Wt, int D, int H, int W, int z0, int z1,
                                         float iso, float min_weight, uint8_t* edge_mask, int32_t* vert_off,
                                         int32_t* tri_off, int64_t* totals, void* stream) {
    const char* fn = "sfmhip_tsdf_surface_count";
    Range R;
    const int rc0 = check_args(fn, D, H, W, z0, z1, min_weight, R);
    if (rc0 != SFMHIP_OK) return rc0;
    SFMHIP_REQUIRE(totals, "%s: null pointer (totals)", fn);
    totals[0] = totals[1] = 0;
    if (R.empty) return SFMHIP_OK;
    SFMHIP_REQUIRE(T && Wt && edge_mask && vert_off && tri_off, "%s: null pointer", fn);
    SFMHIP_REQUIRE(aligned16(edge_mask) && aligned16(vert_off) && aligned16(tri_off),
                   "%s: the work arrays must be 16-byte aligned", fn);
    hipStream_t st = as_stream(stream);
    ScanJob J;
    J.mask = edge_mask;
    J.voff = vert_off;
    J.nv = R.nv;
    J.toff = tri_off;
    J.nt = R.nt;
    J.nba = ceil_div(R.nv + 1, kScanChunk);
    const int nb = J.nba + ceil_div(R.nt + 1, kScanChunk);
    void* sc = nullptr;
    hipError_t e = scratch_alloc(&sc, 16 + (size_t)nb * sizeof(int32_t), st);
    if (e != hipSuccess) {
        set_error("%s: scratch: %s", fn, hipGetErrorString(e));
        return SFMHIP_E_HIP;
    }
    int64_t* dtot = static_cast<int64_t*>(sc);
    int32_t* sums = reinterpret_cast<int32_t*>(dtot + 2);
    hipLaunchKernelGGL(surf_classify_kernel, dim3(ceil_div(W, kTX), ceil_div(H, kTY), ceil_div(z1 - z0 + 1, kTZ)),
                       dim3(256), 0, st, T, Wt, D, H, W, z0, z1, iso, min_weight, edge_mask, tri_off);
    int rc = check_launch("surf_classify_kernel");
    if (rc == SFMHIP_OK) {
        hipLaunchKernelGGL(surf_scan_sums_kernel, dim3(nb), dim3(256), 0, st, J, sums);
        hipLaunchKernelGGL(surf_scan_top_kernel, dim3(2), dim3(256), 0, st, sums, J.nba, nb, dtot);
        hipLaunchKernelGGL(surf_scan_add_kernel, dim3(nb), dim3(256), 0, st, J, sums);
        rc = check_launch("surf_scan kernels");
    }
    int64_t host[2] = {0, 0};
    if (rc == SFMHIP_OK) {
        e = hipMemcpyAsync(host, dtot, sizeof(host), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            set_error("%s: %s", fn, hipGetErrorString(e));
            rc = SFMHIP_E_HIP;
        }
    }
    scratch_free(sc, st);
    if (rc != SFMHIP_OK) return rc;
    totals[0] = host[0];
    totals[1] = host[1];
    if (host[0] > INT32_MAX || host[1] > INT32_MAX) {
        set_error("%s: %lld vertices / %lld triangles exceed INT32_MAX; split the range into z-slabs", fn,
                  (long long)host[0], (long long)host[1]);
        return SFMHIP_E_OVERFLOW;
    }
    return SFMHIP_OK;
}

extern "C" int sfmhip_tsdf_surface_emit(const float* T, const float* Wt, int D, int H, int W, int z0, int z1,
                                        float iso, float min_weight, const float* bmin, const float* bmax,
                                        const uint8_t* edge_mask, const int32_t* vert_off, const int32_t* tri_off,
                                        float* vertices, float* normals, int32_t* faces, void* stream) {
    const char* fn = "sfmhip_tsdf_surface_emit";
    Range R;
    const int rc0 = check_args(fn, D, H, W, z0, z1, min_weight, R);
    if (rc0 != SFMHIP_OK) return rc0;
    SFMHIP_REQUIRE(bmin && bmax, "%s: null pointer (bounds)", fn);
    if (R.empty) return SFMHIP_OK;
    SFMHIP_REQUIRE(T && Wt && edge_mask && vert_off && tri_off, "%s: null pointer", fn);
    hipStream_t st = as_stream(stream);
    Geo G;
    const int dim[3] = {W, H, D};
    for (int a = 0; a < 3; ++a) {
        G.bmin[a] = bmin[a];
        G.step[a] = (bmax[a] - bmin[a]) / (float)(dim[a] - 1);
    }
    // vertices / faces (caller-sized from the totals) may be null only when that total is 0:
    // the kernels then find no active edge / crossing cell and store nothing
    hipLaunchKernelGGL(surf_vertex_kernel, dim3(ceil_div(R.nv, 256)), dim3(256), 0, st, T, Wt, D, H, W, z0, R.nv, iso,
                       min_weight, G, edge_mask, vert_off, vertices, normals);
    int rc = check_launch("surf_vertex_kernel");
    if (rc != SFMHIP_OK) return rc;
    hipLaunchKernelGGL(surf_face_kernel, dim3(ceil_div(R.nt, 256)), dim3(256), 0, st, T, H, W, z0, R.nt, iso,
                       edge_mask, vert_off, tri_off, faces);
    return check_launch("surf_face_kernel");
}

extern "C" int sfmhip_tsdf_surface_colours(const float* T, const float* Wt, const uint32_t* C, int D, int H, int W,
                                           int z0, int z1, float iso, float min_weight, const uint8_t* edge_mask,
                                           const int32_t* vert_off, uint8_t* rgba, void* stream) {
    const char* fn = "sfmhip_tsdf_surface_colours";
    Range R;
    const int rc0 = check_args(fn, D, H, W, z0, z1, min_weight, R);
    if (rc0 != SFMHIP_OK) return rc0;
    if (R.empty) return SFMHIP_OK;
    SFMHIP_REQUIRE(T && Wt && C && edge_mask && vert_off, "%s: null pointer", fn);
    SFMHIP_REQUIRE(aligned16(C) && (reinterpret_cast<uintptr_t>(rgba) & 3u) == 0,
                   "%s: C must be 16-byte and rgba 4-byte aligned", fn);
    // rgba (caller-sized from the vertex total) may be null only when that total is 0
    hipLaunchKernelGGL(surf_colour_kernel, dim3(ceil_div(R.nv, 256)), dim3(256), 0, as_stream(stream), T,
                       reinterpret_cast<const uint4*>(C), D, H, W, z0, R.nv, iso, edge_mask, vert_off,
                       reinterpret_cast<uchar4*>(rgba));
    return check_launch("surf_colour_kernel");
}
