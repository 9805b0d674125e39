// undistort.hip — V12: images and depth maps seen through the radial model (fx, fy, cx, cy, k1, k2)
// resampled to a pinhole camera (gx, gy, ox, oy), for the dense path (semantics: include/sfmhip.h
// V12, restated in numpy by tests/undistort_ref.py).  Plain launches on the caller's stream, no
// atomics:
//   axes     one lane per output column and per output row of a view: x = (u - ox) / gx and
//            y = (v - oy) / gy, the two f64 divisions of the map, once per column and row
//            instead of once per pixel, and one lane per view for the skip rule (scratch
//            [V][Wo + Ho + 1] f64: x, y, then 1.0 for a view that counts and 0.0 for one that
//            does not).
//   u8       one lane per output pixel, a workgroup = 256 consecutive pixels of one output row
//            (the row, the view and with them y and the cameras are wave-uniform).  The map in
//            f64, a four-tap gather of C bytes each (neighbouring lanes read neighbouring source
//            pixels), the integer blend.  Stores: see undistort_u8_kernel.
//   f32      the same lane split; one 32-bit load and one 32-bit store per lane.
//   map      the same lane split; X, Y as one 8-byte store per lane.
// The map is f64 with -ffp-contract=off, one IEEE step per operation: every output is
// bit-identical to the numpy form.
#include "common.h"

namespace sfmhip {
namespace {

constexpr int kTile = 256;     // output pixels per workgroup, consecutive in one output row
constexpr int kMaxSide = 32768;

__global__ __launch_bounds__(256) void undistort_axes_kernel(const double* __restrict__ cam_src,
                                                             const double* __restrict__ cam_dst, int V, int Ho, int Wo,
                                                             double* __restrict__ axes) {
    const int n = Wo + Ho + 1;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)V * n) return;
    const int view = (int)(idx / n), j = (int)(idx % n);
    const double* s = cam_src + (size_t)view * 6;
    const double* d = cam_dst + (size_t)view * 4;
    if (j < Wo) {
        axes[idx] = ((double)j - d[2]) / d[0];
    } else if (j < Wo + Ho) {
        axes[idx] = ((double)(j - Wo) - d[3]) / d[1];
    } else {   // the skip rule over the 6 + 4 numbers of the view's two cameras
        bool good = true;
        for (int q = 0; q < 6; ++q) good = good && fabs(s[q]) < 0x1p60;
        for (int q = 0; q < 4; ++q) good = good && fabs(d[q]) < 0x1p60;
        good = good && s[0] != 0.0 && s[1] != 0.0 && d[0] != 0.0 && d[1] != 0.0;
        axes[idx] = good ? 1.0 : 0.0;
    }
}

// output pixel (u, v) of the view -> X, Y in 1/256 px of the source; false (and -1, -1) where the
// pixel or the whole view is invalid
__device__ __forceinline__ bool map_pixel(const double* __restrict__ cam_src, const double* __restrict__ axes, int view,
                                          int u, int v, int H, int W, int Ho, int Wo, int& X, int& Y) {
    const double* s = cam_src + (size_t)view * 6;
    const double* ax = axes + (size_t)view * (Wo + Ho + 1);
    const double x = ax[u], y = ax[Wo + v];
    const double r2 = x * x + y * y;
    const double r4 = r2 * r2;
    const double d = (1.0 + s[4] * r2) + s[5] * r4;
    const double mono = (1.0 + (3.0 * s[4]) * r2) + (5.0 * s[5]) * r4;
    const double sx = (d * x) * s[0] + s[2];
    const double sy = (d * y) * s[1] + s[3];
    const bool fin = mono > 0.0 && fabs(sx) < 0x1p30 && fabs(sy) < 0x1p30;   // a NaN fails
    const double Xd = floor(sx * 256.0 + 0.5), Yd = floor(sy * 256.0 + 0.5);
    const bool valid = ax[Wo + Ho] != 0.0 && fin && Xd >= 0.0 && Xd <= (double)((W - 1) * 256) && Yd >= 0.0 &&
                       Yd <= (double)((H - 1) * 256);
    X = valid ? (int)Xd : -1;
    Y = valid ? (int)Yd : -1;
    return valid;
}

// n bytes of LDS (the image of the global bytes from g on, shifted so that LDS dwords are global
// dwords) -> global, whole dwords where the range covers them
__device__ __forceinline__ void store_tile(const uint8_t* lds, uint8_t* g, int n) {
    const int sh = (int)((uintptr_t)g & 3);
    uint8_t* base = g - sh;
    const int nd = (sh + n + 3) >> 2;
    for (int k = threadIdx.x; k < nd; k += kTile) {
        const int b0 = 4 * k;
        if (b0 >= sh && b0 + 4 <= sh + n) {
            *reinterpret_cast<uint32_t*>(base + b0) = *reinterpret_cast<const uint32_t*>(lds + b0);
        } else {
            for (int j = 0; j < 4; ++j)
                if (b0 + j >= sh && b0 + j < sh + n) base[b0 + j] = lds[b0 + j];
        }
    }
}

// Stores, the faster of two measured forms for each C: C = 1 every lane its byte
// (64 contiguous bytes per wave), C = 4 every lane one dword (dst is 4-byte aligned), C = 3 the
// lanes' bytes go to LDS and the workgroup stores its run of the row as whole dwords.  The mask
// byte is stored by its lane.
template <int C>
__global__ __launch_bounds__(kTile) void undistort_u8_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                             const double* __restrict__ cam_src,
                                                             const double* __restrict__ axes, int Ho, int Wo,
                                                             uint8_t* __restrict__ dst, uint8_t* __restrict__ mask) {
    constexpr bool kLds = C == 3;
    __shared__ __attribute__((aligned(16))) uint8_t s_img[kLds ? kTile * C + 4 : 4];
    const int view = blockIdx.z, v = blockIdx.y;
    const int u0 = blockIdx.x * kTile, u = u0 + (int)threadIdx.x;
    const size_t row = ((size_t)view * Ho + v) * Wo;
    uint8_t* gi = dst + (row + u0) * C;
    const int shi = (int)((uintptr_t)gi & 3);
    if (u < Wo) {
        int X, Y;
        const bool valid = map_pixel(cam_src, axes, view, u, v, H, W, Ho, Wo, X, Y);
        uint32_t o[C];
        for (int c = 0; c < C; ++c) o[c] = 0;
        if (valid) {
            const int x0 = X >> 8, y0 = Y >> 8;
            const uint32_t a = X & 255, b = Y & 255;
            const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
            const uint8_t* r0 = src + ((size_t)view * H + y0) * W * C;
            const uint8_t* r1 = src + ((size_t)view * H + y1) * W * C;
            const uint32_t w00 = (256 - a) * (256 - b), w01 = a * (256 - b), w10 = (256 - a) * b, w11 = a * b;
            for (int c = 0; c < C; ++c)
                o[c] = (w00 * r0[x0 * C + c] + w01 * r0[x1 * C + c] + w10 * r1[x0 * C + c] + w11 * r1[x1 * C + c] +
                        32768u) >> 16;
        }
        mask[row + u] = valid ? 1 : 0;
        if (kLds) {
            for (int c = 0; c < C; ++c) s_img[shi + (int)threadIdx.x * C + c] = (uint8_t)o[c];
        } else if (C == 4) {
            reinterpret_cast<uint32_t*>(gi)[threadIdx.x] = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
        } else {
            for (int c = 0; c < C; ++c) gi[(int)threadIdx.x * C + c] = (uint8_t)o[c];
        }
    }
    if (kLds) {
        __syncthreads();
        store_tile(s_img, gi, min(kTile, Wo - u0) * C);
    }
}

__global__ __launch_bounds__(kTile) void undistort_f32_kernel(const uint32_t* __restrict__ src, int H, int W,
                                                              const double* __restrict__ cam_src,
                                                              const double* __restrict__ axes, int Ho, int Wo,
                                                              uint32_t* __restrict__ dst) {
    const int view = blockIdx.z, v = blockIdx.y;
    const int u = blockIdx.x * kTile + (int)threadIdx.x;
    if (u >= Wo) return;
    int X, Y;
    uint32_t bits = 0;
    if (map_pixel(cam_src, axes, view, u, v, H, W, Ho, Wo, X, Y)) {
        const int x = min((X + 128) >> 8, W - 1), y = min((Y + 128) >> 8, H - 1);
        bits = src[((size_t)view * H + y) * W + x];
    }
    dst[((size_t)view * Ho + v) * Wo + u] = bits;
}

__global__ __launch_bounds__(kTile) void undistort_map_kernel(int H, int W, const double* __restrict__ cam_src,
                                                              const double* __restrict__ axes, int Ho, int Wo,
                                                              int2* __restrict__ map) {
    const int view = blockIdx.z, v = blockIdx.y;
    const int u = blockIdx.x * kTile + (int)threadIdx.x;
    if (u >= Wo) return;
    int X, Y;
    map_pixel(cam_src, axes, view, u, v, H, W, Ho, Wo, X, Y);
    map[((size_t)view * Ho + v) * Wo + u] = make_int2(X, Y);
}

int check_shapes(const char* fn, int V, int H, int W, int Ho, int Wo) {
    SFMHIP_REQUIRE(V >= 0 && H >= 0 && W >= 0 && Ho >= 0 && Wo >= 0, "%s: bad shape (V %d, H %d, W %d, Ho %d, Wo %d)", fn,
                   V, H, W, Ho, Wo);
    SFMHIP_REQUIRE(V <= 65535, "%s: at most 65535 views per call, got %d", fn, V);
    SFMHIP_REQUIRE(H <= kMaxSide && W <= kMaxSide && Ho <= kMaxSide && Wo <= kMaxSide,
                   "%s: an image has at most %d pixels per side", fn, kMaxSide);
    return SFMHIP_OK;
}

// scratch of a call, per view: x of every output column, y of every output row, the view's flag
int axes_of(const char* fn, const double* cam_src, const double* cam_dst, int V, int Ho, int Wo, hipStream_t st,
            void** sc) {
    const size_t n = (size_t)V * (Wo + Ho + 1);
    const hipError_t e = scratch_alloc(sc, n * sizeof(double), st);
    if (e != hipSuccess) {
        set_error("%s: scratch: %s", fn, hipGetErrorString(e));
        return SFMHIP_E_HIP;
    }
    hipLaunchKernelGGL(undistort_axes_kernel, dim3(ceil_div((int64_t)n, 256)), dim3(256), 0, st, cam_src, cam_dst, V, Ho,
                       Wo, static_cast<double*>(*sc));
    return check_launch("undistort_axes_kernel");
}

dim3 grid_of(int V, int Ho, int Wo) { return dim3(ceil_div(Wo, kTile), Ho, V); }

}  // namespace
}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_undistort_u8(const uint8_t* src, int V, int H, int W, int C, const double* cam_src,
                                   const double* cam_dst, int Ho, int Wo, uint8_t* dst, uint8_t* mask, void* stream) {
    const char* fn = "sfmhip_undistort_u8";
    int rc = check_shapes(fn, V, H, W, Ho, Wo);
    if (rc != SFMHIP_OK) return rc;
    SFMHIP_REQUIRE(C == 1 || C == 3 || C == 4, "%s: C must be 1, 3 or 4, got %d", fn, C);
    if (V == 0 || H == 0 || W == 0 || Ho == 0 || Wo == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(src && cam_src && cam_dst && dst && mask, "%s: null pointer", fn);
    SFMHIP_REQUIRE(C != 4 || ((uintptr_t)dst & 3) == 0, "%s: dst must be 4-byte aligned when C is 4", fn);
    hipStream_t st = as_stream(stream);
    void* sc = nullptr;
    rc = axes_of(fn, cam_src, cam_dst, V, Ho, Wo, st, &sc);
    if (rc == SFMHIP_OK) {
        const dim3 grid = grid_of(V, Ho, Wo), block(kTile);
        const double* axes = static_cast<const double*>(sc);
        if (C == 1)
            hipLaunchKernelGGL(undistort_u8_kernel<1>, grid, block, 0, st, src, H, W, cam_src, axes, Ho, Wo, dst, mask);
        else if (C == 3)
            hipLaunchKernelGGL(undistort_u8_kernel<3>, grid, block, 0, st, src, H, W, cam_src, axes, Ho, Wo, dst, mask);
        else
            hipLaunchKernelGGL(undistort_u8_kernel<4>, grid, block, 0, st, src, H, W, cam_src, axes, Ho, Wo, dst, mask);
        rc = check_launch("undistort_u8_kernel");
    }
    if (sc) scratch_free(sc, st);
    return rc;
}

extern "C" int sfmhip_undistort_f32(const float* src, int V, int H, int W, const double* cam_src, const double* cam_dst,
                                    int Ho, int Wo, float* dst, void* stream) {
    const char* fn = "sfmhip_undistort_f32";
    int rc = check_shapes(fn, V, H, W, Ho, Wo);
    if (rc != SFMHIP_OK) return rc;
    if (V == 0 || H == 0 || W == 0 || Ho == 0 || Wo == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(src && cam_src && cam_dst && dst, "%s: null pointer", fn);
    hipStream_t st = as_stream(stream);
    void* sc = nullptr;
    rc = axes_of(fn, cam_src, cam_dst, V, Ho, Wo, st, &sc);
    if (rc == SFMHIP_OK) {
        hipLaunchKernelGGL(undistort_f32_kernel, grid_of(V, Ho, Wo), dim3(kTile), 0, st,
                           reinterpret_cast<const uint32_t*>(src), H, W, cam_src, static_cast<const double*>(sc), Ho, Wo,
                           reinterpret_cast<uint32_t*>(dst));
        rc = check_launch("undistort_f32_kernel");
    }
    if (sc) scratch_free(sc, st);
    return rc;
}

extern "C" int sfmhip_undistort_map(const double* cam_src, const double* cam_dst, int V, int H, int W, int Ho, int Wo,
                                    int32_t* map, void* stream) {
    const char* fn = "sfmhip_undistort_map";
    int rc = check_shapes(fn, V, H, W, Ho, Wo);
    if (rc != SFMHIP_OK) return rc;
    if (V == 0 || Ho == 0 || Wo == 0) return SFMHIP_OK;
    SFMHIP_REQUIRE(cam_src && cam_dst && map, "%s: null pointer", fn);
    SFMHIP_REQUIRE(((uintptr_t)map & 7) == 0, "%s: map must be 8-byte aligned", fn);
    hipStream_t st = as_stream(stream);
    void* sc = nullptr;
    rc = axes_of(fn, cam_src, cam_dst, V, Ho, Wo, st, &sc);
    if (rc == SFMHIP_OK) {
        hipLaunchKernelGGL(undistort_map_kernel, grid_of(V, Ho, Wo), dim3(kTile), 0, st, H, W, cam_src,
                           static_cast<const double*>(sc), Ho, Wo, reinterpret_cast<int2*>(map));
        rc = check_launch("undistort_map_kernel");
    }
    if (sc) scratch_free(sc, st);
    return rc;
}
