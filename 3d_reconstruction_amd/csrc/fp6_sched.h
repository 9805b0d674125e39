// fp6_sched.h — the instruction order of match_fp6_kernel's block loop (match_fp6.hip), shared with the
// registers-only probe tools/mfma_mx_peak.hip so that the probe times the order the kernel runs.
#pragma once

namespace sfmhip {

// Where the block loop's VALU work sits among the MFMAs (DESIGN.md K1'', "Schedule").  A tile is KK k-steps
// of NS MFMAs, chain s at position kk NS + s; the gap behind position g takes:
//   maxima: chain s's first max3 in gap F + s of its tile and its second one gap later, so the accumulator's
//           first reader comes five MFMAs behind the chain's last MFMA (at three the compiler still pads
//           the readers of the sparse gaps with s_nop).  The last chains' maxima fall into
//           the next tile's first gaps, ahead of that tile's MFMA on the same chain (position s > gap).
//   merge : the 4 NS instructions that fold a finished range's maxima into the top two fill the gaps of
//           the NEXT range up to kBudget instructions per gap, in chain order (chain c is finished by then).
template <int KK, int NS>
struct Fp6Sched {
    static constexpr int MPT = KK * NS;          // MFMAs (= gaps) per candidate tile
    static constexpr int F = (KK - 1) * NS + 5;
    static constexpr int kBudget = KK == 1 ? 3 : 2;   // one k-step per tile carries 3 VALU per MFMA: no room for 2
    static_assert(F + 1 < MPT, "a spilled maximum reads its chain before the next tile rewrites it");
    // maximum `which` (0 first, 1 second) of gap g: its chain (>= NS: none) and whether it belongs to the tile before
    static constexpr int chain(int g, int which) { return (g - F - which + MPT) % MPT; }
    static constexpr bool back(int g, int which) { return g - F - which < 0; }
    static constexpr int load(int g) { return (chain(g, 0) < NS) + (chain(g, 1) < NS); }
    // merge instruction (4 c + step of chain c; -1: none) in slot j of gap h, h counted from the range's start
    // (closed form, so that it folds once the loops are unrolled: maxima `which` fill the gaps F + which ..
    // MPT - 1 of their tile and 0 .. F + which + NS - 1 - MPT of the next)
    static constexpr int before(int g, int which) {
        const int f = F + which, wrap = f + NS - MPT;
        return (g < wrap ? g : wrap) + (g > f ? g - f : 0);
    }
    static constexpr int merge(int h, int j) {
        const int g = h % MPT;
        const int k = (h / MPT) * (kBudget * MPT - 2 * NS) + kBudget * g - before(g, 0) - before(g, 1);
        return (j < kBudget - load(g) && k + j < 4 * NS) ? k + j : -1;
    }
    // Merge instruction k belongs to a pair of chains, 8 instructions a pair: compare, compare, median, median,
    // select, select, select, select, so that no select follows its compare within three instructions.
    static constexpr int merge_chain(int k) { return 2 * (k / 8) + ((0xCA >> (k % 8)) & 1); }
    static constexpr int merge_step(int k) { return (0x3232'1100 >> (4 * (k % 8))) & 15; }
    // when the block ends its last tile still owes the first maximum of the chains from kOwedFirst on and the
    // second of those from kOwedSecond on
    static constexpr int kOwedFirst = MPT - F, kOwedSecond = MPT - F - 1;
    // every chain's range maximum is complete before its merge begins: chain c's second maximum of the range's
    // last tile sits in gap F + 1 + c - MPT of the next range, its first compare is merge instruction 8 (c / 2) + c % 2
    static constexpr bool merge_ready() {
        for (int c = 0; c < NS; ++c) {
            int h = 0;
            while (true) {
                bool found = false;
                for (int j = 0; j < kBudget; ++j) found |= merge(h, j) == 8 * (c / 2) + c % 2;
                if (found) break;
                ++h;
            }
            if (h < F + 1 + c - MPT) return false;
        }
        return true;
    }
};

// Step 0..3 of one chain's merge of a range maximum m (range id rid) into the running top two (w1, w2) and the
// range wr where the best rose.  Strict compare: the earliest range on ties; the one compare serves the id
// and the maximum; the median reads w1 before step 3 replaces it.  The selects take values, not array
// elements: a conditional between two lvalues is a select of addresses, which can keep the arrays in memory.
__device__ __forceinline__ void fp6_merge_step(int step, float m, int rid, bool& up, float& w1, float& w2, int& wr) {
    const float a = w1, b = w2;
    const int r = wr;
    const bool u = up;
    if (step == 0) up = m > a;
    else if (step == 1) w2 = __builtin_amdgcn_fmed3f(a, b, m);
    else if (step == 2) wr = u ? rid : r;
    else w1 = u ? m : a;
}

}  // namespace sfmhip
