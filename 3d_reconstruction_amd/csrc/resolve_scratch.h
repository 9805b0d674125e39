// resolve_scratch.h — the layout of the scratch buffer of one exact-mode call (match_exact.hip).
// Plain C++ (no HIP runtime): tools/resolve_scratch_layout.cpp checks it on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>

namespace sfmhip {

constexpr int kResolveBucket = 4096;   // undecided rows collected per image b; more sets the overflow flag
constexpr int kResolveRows = 16;       // rows of one image settled together (match_resolve_batched_kernel)

// Byte offsets of the regions, in buffer order.  This is the only place they are sized.
struct ResolveScratch {
    size_t list;    // int64 [n_img][kResolveBucket]: the buckets, graph entries of the undecided rows per image b
    size_t cnt;     // unsigned [n_img]: rows per bucket (zeroed before every call, with flag)
    size_t flag;    // unsigned: a bucket overflowed, the fallback scan settles every row
    size_t off;     // unsigned [n_img]: first flat row of image b
    size_t okey;    // unsigned [n_img + 1]: the same offsets in XCD-major order, then the total
    size_t oimg;    // int [n_img]: the image at each XCD-major position
    size_t xr;      // unsigned [16]: per XCD first flat row, rows
    size_t ir;      // unsigned [16]: per XCD first item, items
    size_t flat;    // int64 [n_img][kResolveBucket]: the buckets flattened XCD-major
    size_t items;   // int [3][n_img * (kResolveBucket / kResolveRows + 1)]: first flat row, rows, image
    size_t h;       // int32 [n_img][m_pad]: keys >> 8, when the value-only form runs without the bank's
    size_t hf;      // float [n_img][m_pad]: h / 64, behind h, for the FP6 filter
    size_t bytes;   // the whole buffer
    size_t h_count; // elements of h (0: none built in this call)
};

inline ResolveScratch resolve_scratch_layout(int n_img, int m_pad, bool value_only, bool fp6, bool has_bank_h) {
    const size_t n = (size_t)n_img, u = sizeof(unsigned);
    ResolveScratch r;
    r.list = 0;
    r.cnt = r.list + n * kResolveBucket * sizeof(int64_t);
    r.flag = r.cnt + n * u;
    r.off = r.flag + u;
    r.okey = r.off + n * u;
    r.oimg = r.okey + (n + 1) * u;
    r.xr = r.oimg + n * sizeof(int);
    r.ir = r.xr + 16 * u;
    r.flat = r.ir + 16 * u;   // 8-byte aligned: (4 n + 34) words lie between the two int64 lists
    r.items = r.flat + n * kResolveBucket * sizeof(int64_t);
    r.h = r.items + 3 * n * (kResolveBucket / kResolveRows + 1) * sizeof(int);
    r.h_count = value_only && !has_bank_h ? n * (size_t)m_pad : 0;
    r.hf = r.h + r.h_count * sizeof(int32_t);
    r.bytes = r.hf + (fp6 ? r.h_count * sizeof(float) : 0);
    return r;
}

}  // namespace sfmhip
