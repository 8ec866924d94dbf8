// find_kernels.hpp -- approximate pattern search on 2-bit packed words (include/cute_nt.h, "pattern search"): the windows of
// k <= 32 codes whose Hamming distance to a pattern (wildcard positions excepted) is at most max_mismatches, on the forward
// strand or on both.  Not in the reference; the definition is restated per base by tests/test_find_pattern.py.
//
// Traffic: 0.25 B read per window and, in a real search, a handful of hits written -- the work is integer VALU: per window and
// strand an XOR against the pattern, (y | y >> 1) & care (one bit per compared position that differs), a population count and
// a compare.  The reverse strand needs no reverse complement of the text: window x hits the reverse strand iff x is within
// max_mismatches of the pattern's reverse complement, so it is a second XOR against P' with care' on the same window.
//
// The output size depends on the data, so a call is the three passes of counted_output.hpp, which owns the scratch layout, none of
// which allocates:
//   1. find_count_*: one workgroup per tile of kFindTile windows counts the tile's hits into counts[tile];
//   2. counted_scan: offs[group] = the exclusive offset of each group of kCountedGroup tiles, *count SET to the total;
//   3. find_write_*: a tile whose count is 0 returns at once (nearly every tile of a real search); the others are
//      recomputed (0.25 B/nt: cheaper than staging candidates), a workgroup prefix sum over the lanes' hit counts places each
//      lane's run, and the lane stores its hits in window order, forward before reverse, below out_cap only.
// Shape of a tile, as in word_tile.hpp: lane j owns the 32 windows that START in word j of the tile; it reads that word and the
// next (word_tile_pair) and walks the 32 windows with constant funnel shifts into two hit masks (bit r: window r hits), one per
// strand.  Pattern, care masks and the bound are kernel arguments: wave-uniform, in SGPRs.
// WIDE = false (k <= 16): a window and everything compared with it is one dword -- half the VALU work of the 64-bit form.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"
#include "counted_output.hpp"

namespace cnt {

constexpr int kFindBlock = 256;
constexpr int kFindWaves = kFindBlock / 64;
constexpr uint64_t kFindTileWords = kFindBlock, kFindTile = 32 * kFindTileWords;  // windows per tile: 8192
constexpr uint32_t kFindReverse = 0x100u;                                          // CNT_FIND_REVERSE (asserted equal in find_abi.inc)
static_assert(2 * kFindTile < (1ull << 32), "a tile's hit count is a u32");

// what a call compares with: the pattern and its reverse complement P'_j = P_{k-1-j} ^ 2 packed like a k-mer, and for each a
// care mask with bit 2j set where position j is compared (not a wildcard, j < k)
struct FindPattern {
    uint64_t fwd, fwd_care, rev, rev_care;
    uint32_t max_mismatches;
};

// #{ compared positions at which window x differs from p }: a code differs iff either of its two XOR bits is set
template <bool WIDE>
__device__ __forceinline__ uint32_t find_dist(uint64_t x, uint64_t p, uint64_t care) {
    const uint32_t y0 = (uint32_t)x ^ (uint32_t)p;
    uint32_t d = (uint32_t)__popc((y0 | (y0 >> 1)) & (uint32_t)care);
    if constexpr (WIDE) {
        // dword by dword: the bit that a 64-bit shift would bring into bit 31 is an odd one, which no care mask holds
        const uint32_t y1 = (uint32_t)(x >> 32) ^ (uint32_t)(p >> 32);
        d += (uint32_t)__popc((y1 | (y1 >> 1)) & (uint32_t)(care >> 32));
    }
    return d;
}

// window r (0..31) of the 32 that start in word `lo`, `hi` the word behind it; WIDE = false keeps its low 16 codes
template <bool WIDE>
__device__ __forceinline__ uint64_t find_window(uint64_t lo, uint64_t hi, uint32_t r) {
    const uint64_t win = funnel64(lo, hi, 2 * r);
    return WIDE ? win : (uint64_t)(uint32_t)win;
}

// the hit masks of one lane: bit r of fm / rm = window r is within the bound of the pattern / of its reverse complement.
// The lane's two words are the dwords a[0..3]; window r is a funnel of two (WIDE: three) neighbouring dwords at a constant
// shift -- one v_alignbit_b32 per window dword, nothing 64 bits wide.
template <bool WIDE, bool BOTH>
__device__ __forceinline__ void find_lane_masks(uint64_t lo, uint64_t hi, const FindPattern& p, uint32_t& fm, uint32_t& rm) {
    const uint32_t a[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
    fm = 0;
    rm = 0;
#pragma unroll
    for (uint32_t r = 0; r < 32; ++r) {
        const uint64_t win = ((uint64_t)(WIDE ? window_dword(a + 1, r) : 0u) << 32) | window_dword(a, r);
        fm |= (find_dist<WIDE>(win, p.fwd, p.fwd_care) <= p.max_mismatches ? 1u : 0u) << r;
        if constexpr (BOTH) rm |= (find_dist<WIDE>(win, p.rev, p.rev_care) <= p.max_mismatches ? 1u : 0u) << r;
    }
}

// Tile blockIdx.x + first_tile = input words [256 t, 256 t + 256) = windows [8192 t, 8192 t + 8192); m = len-k+1 >= 1 windows,
// `words` = ceil(len / 32).  A tile whose 257 words all exist takes the 16-B loads, the others (the last one or two) read word by
// word, each read guarded.  Bits beyond len are never part of a reported window: window i < m uses codes i .. i+k-1 <= len-1,
// and the windows at or past m are masked out of the lane's hit masks.
// WRITE = false: counts[tile] = the tile's hits.  WRITE = true: the scan's offs[] and the counts place the tile's entries.
template <bool WIDE, bool BOTH, bool WRITE>
__device__ __forceinline__ void find_tile(const uint8_t* __restrict__ in, uint64_t words, uint64_t m, const FindPattern& p, uint64_t first_tile,
                                          uint32_t* __restrict__ counts, const uint64_t* __restrict__ offs, uint64_t* __restrict__ pos,
                                          uint64_t* __restrict__ info, uint64_t out_cap) {
    __shared__ uint32_t s_cnt[kFindWaves];
    __shared__ uint64_t s_base;
    const uint64_t tile = first_tile + blockIdx.x, w0 = tile * kFindTileWords;
    const uint32_t j = threadIdx.x;
    if constexpr (WRITE) {
        if (counts[tile] == 0) return;
    }
    uint64_t lo, hi;
    word_tile_pair<kFindTileWords>(in, words, w0, j, lo, hi);
    const uint64_t i0 = (w0 + j) * 32;
    const uint32_t valid = codes_below(i0, m);
    uint32_t fm, rm;
    find_lane_masks<WIDE, BOTH>(lo, hi, p, fm, rm);
    fm &= valid;
    rm &= valid;
    const uint32_t c = (uint32_t)__popc(fm) + (uint32_t)__popc(rm);
    const uint32_t x = tile_rank_post(c, s_cnt);  // lane order = window order
    if constexpr (WRITE) {
        if (j == 0) s_base = counted_tile_base(offs, counts, tile);
    }
    __syncthreads();
    if constexpr (!WRITE) {
        if (j == 0) counts[tile] = tile_total<kFindWaves>(s_cnt);
    } else {
        uint64_t at = s_base + tile_before<kFindWaves>(s_cnt, x - c);
        // the lane's hits in window order, forward before reverse; the distance is recomputed for the few windows that hit
        for (uint32_t any = fm | rm; any; any &= any - 1) {
            const uint32_t r = (uint32_t)__builtin_ctz(any);
            const uint64_t win = find_window<WIDE>(lo, hi, r);
            if ((fm >> r) & 1u) {
                if (at < out_cap) {
                    __builtin_nontemporal_store(i0 + r, pos + at);
                    if (info) __builtin_nontemporal_store((uint64_t)find_dist<WIDE>(win, p.fwd, p.fwd_care), info + at);
                }
                ++at;
            }
            if (BOTH && ((rm >> r) & 1u)) {
                if (at < out_cap) {
                    __builtin_nontemporal_store(i0 + r, pos + at);
                    if (info) __builtin_nontemporal_store((uint64_t)(find_dist<WIDE>(win, p.rev, p.rev_care) | kFindReverse), info + at);
                }
                ++at;
            }
        }
    }
}

// The eight kernels: {count, write} x {k <= 16, k <= 32} x {forward, both strands}.  Plain functions over the one body, so that
// each is named for what it does in a profile.
#define CNT_FIND_KERNEL(name, WIDE, BOTH, WRITE)                                                                                             \
    __global__ __launch_bounds__(kFindBlock) void name(const uint8_t* __restrict__ in, uint64_t words, uint64_t m, FindPattern p,           \
                                                       uint64_t first_tile, uint32_t* __restrict__ counts, const uint64_t* __restrict__ offs, \
                                                       uint64_t* __restrict__ pos, uint64_t* __restrict__ info, uint64_t out_cap) {         \
        find_tile<WIDE, BOTH, WRITE>(in, words, m, p, first_tile, counts, offs, pos, info, out_cap);                                         \
    }
CNT_FIND_KERNEL(find_count_k16, false, false, false)
CNT_FIND_KERNEL(find_count_k16_both, false, true, false)
CNT_FIND_KERNEL(find_count_k32, true, false, false)
CNT_FIND_KERNEL(find_count_k32_both, true, true, false)
CNT_FIND_KERNEL(find_write_k16, false, false, true)
CNT_FIND_KERNEL(find_write_k16_both, false, true, true)
CNT_FIND_KERNEL(find_write_k32, true, false, true)
CNT_FIND_KERNEL(find_write_k32_both, true, true, true)
#undef CNT_FIND_KERNEL

using FindKernel = void (*)(const uint8_t*, uint64_t, uint64_t, FindPattern, uint64_t, uint32_t*, const uint64_t*, uint64_t*, uint64_t*, uint64_t);

}  // namespace cnt
