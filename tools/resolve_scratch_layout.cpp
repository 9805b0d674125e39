// The scratch layout of an exact-mode call (csrc/resolve_scratch.h) against the pointer carving it
// replaced, restated here as it stood in match_exact_impl.  Host only:
//   c++ -std=c++17 -I3d_reconstruction_amd/csrc tools/resolve_scratch_layout.cpp -o build/resolve_scratch_layout
// Prints every region's byte offset, old and new, for a range of bank sizes and both flags; exit 1 on a
// difference.
#include <cstdio>

#include "resolve_scratch.h"

using namespace sfmhip;

int main() {
    const int sizes[] = {1, 2, 7, 8, 9, 257, 1100};
    const int m_pad = 640;
    int bad = 0;
    for (int n_img : sizes)
        for (int flags = 0; flags < 8; ++flags) {
            const bool value_only = flags & 1, fp6 = flags & 2, has_bank_h = flags & 4;
            // the old carving
            const size_t rlist_bytes = (size_t)n_img * 4096 * sizeof(int64_t);
            const size_t rcnt_bytes = ((size_t)n_img + 1) * sizeof(unsigned);
            const size_t roff_bytes = (3 * (size_t)n_img + 33) * sizeof(unsigned);
            const size_t ritem_bytes = 3 * (size_t)n_img * (4096 / 16 + 1) * sizeof(int);
            const size_t rbytes = 2 * rlist_bytes + rcnt_bytes + roff_bytes + ritem_bytes;
            const size_t hn = value_only && !has_bank_h ? (size_t)n_img * m_pad : 0;
            const size_t cnt = rlist_bytes, flag = cnt + 4 * (size_t)n_img, off = rlist_bytes + rcnt_bytes;
            const size_t okey = off + 4 * (size_t)n_img, oimg = okey + 4 * ((size_t)n_img + 1);
            const size_t xr = oimg + 4 * (size_t)n_img, ir = xr + 64;
            const size_t old_[] = {0, cnt, flag, off, okey, oimg, xr, ir, rlist_bytes + rcnt_bytes + roff_bytes,
                                   2 * rlist_bytes + rcnt_bytes + roff_bytes, rbytes, rbytes + hn * sizeof(int32_t),
                                   rbytes + hn * (fp6 ? 2 : 1) * sizeof(int32_t), hn};
            const ResolveScratch r = resolve_scratch_layout(n_img, m_pad, value_only, fp6, has_bank_h);
            const size_t new_[] = {r.list, r.cnt, r.flag, r.off, r.okey, r.oimg, r.xr, r.ir, r.flat, r.items, r.h, r.hf,
                                   r.bytes, r.h_count};
            const char* names[] = {"list", "cnt", "flag", "off", "okey", "oimg", "xr", "ir", "flat", "items", "h", "hf",
                                   "bytes", "h_count"};
            std::printf("n_img %4d value_only %d fp6 %d bank_h %d:", n_img, value_only, fp6, has_bank_h);
            for (int k = 0; k < 14; ++k) {
                const bool same = old_[k] == new_[k];
                std::printf(" %s %zu/%zu%s", names[k], old_[k], new_[k], same ? "" : " DIFFERENT");
                bad += !same;
            }
            std::printf("\n");
        }
    std::printf("%s\n", bad ? "DIFFERENT" : "all offsets equal");
    return bad ? 1 : 0;
}
