// minimizer_kernels.hpp -- (w,k)-minimizer sampling on 2-bit packed words (include/cute_nt.h, "k-mers"): in each window of
// w consecutive k-mers the position with the smallest (fmix64(k-mer), position), output once per distinct position in
// ascending order.  Not in the reference; the definition is restated in Python and numpy by tests/test_minimizers.py.
//
// The output size depends on the data, so a call is the three passes of counted_output.hpp, which owns the scratch layout:
//   1. minimizer_tiles<false>: one workgroup per tile of kMinTile windows counts the tile's new positions into counts[tile];
//   2. counted_scan;
//   3. minimizer_tiles<true>: the same tiles again, recomputed (the input is 0.25 B/nt: cheaper than staging candidates),
//      store their positions (and k-mers) at counted_tile_base() + their rank in the tile, below out_cap only.
// A tile holds the windows t0-1 .. t0+T-1: the one extra window on the left makes "t is new iff p(t) != p(t-1)" local to
// the tile.  It needs the T+w k-mers t0-1 .. t0+T+w-2; their hashes go to LDS, and log2(w) doubling steps turn them into
// the minimum of 2^L consecutive (hash, position) pairs, 2^L the largest power of two <= w.  A window [s, s+w) is then
// the smaller of the pairs at s and s+w-2^L (the two overlap; on equal hashes the left one, whose position is smaller).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "counted_output.hpp"
#include "kmer_kernels.hpp"
#include "util_kernels.hpp"

namespace cnt {

constexpr int kMinBlock = 256;
constexpr uint32_t kMinTile = 2048, kMinMaxW = 256;                  // windows per tile; the largest w
constexpr uint32_t kMinEntries = kMinTile + kMinMaxW;                  // k-mers a tile hashes, at w = 256
constexpr int kMinRounds = (int)(kMinEntries / kMinBlock);             // entries per lane: e = r * BLOCK + lane
constexpr int kMinWinRounds = (int)(kMinTile / kMinBlock);             // windows per lane: t = t0 + r * BLOCK + lane
constexpr int kMinWaves = kMinBlock / 64;
static_assert(kMinEntries % kMinBlock == 0 && kMinTile % kMinBlock == 0 && kMinEntries < 65536, "local indices are u16");

// k-mer i (i + k <= len) as cnt_kmers writes it: funnel64 (word_tile.hpp) over words i>>5 and i>>5 + 1.  The second word is
// clamped to the last one: when it does not exist the k-mer lies inside word i>>5, and the mask drops what the clamp brought.
__device__ __forceinline__ uint64_t minimizer_kmer(const uint64_t* __restrict__ in, uint64_t last_word, uint64_t i, uint32_t k,
                                                   bool canonical) {
    const uint64_t wd = i >> 5;
    const uint32_t sh = 2u * ((uint32_t)i & 31u);
    const uint64_t lo = in[wd], hi = in[wd + 1 <= last_word ? wd + 1 : last_word];
    const uint64_t x = funnel64(lo, hi, sh) & (~0ull >> (64 - 2 * k));
    return canonical ? kmer_finish<true>(x, k) : kmer_finish<false>(x, k);
}

// Tile blockIdx.x + first_tile.  m = len-k+1 k-mers, W = m-w+1 >= 1 windows (the launcher guarantees both).  k-mers outside
// [0, m) -- k-mer t0-1 of tile 0, the ones past the end -- hash to ~0 and are only seen by windows outside [0, W).
// WRITE = false: counts[tile] = the tile's count of new positions.  WRITE = true: the scan's offs[] and the counts place
// the tile's entries.
template <bool WRITE>
__global__ __launch_bounds__(kMinBlock) void minimizer_tiles(const uint64_t* __restrict__ in, uint64_t len, uint32_t k, uint32_t w,
                                                             uint32_t canonical, uint64_t first_tile, uint32_t* __restrict__ counts,
                                                             const uint64_t* __restrict__ offs, uint64_t* __restrict__ pos,
                                                             uint64_t* __restrict__ val, uint64_t out_cap) {
    __shared__ uint64_t s_h[kMinEntries];
    __shared__ uint16_t s_i[kMinEntries];
    __shared__ uint32_t s_cnt[kMinWinRounds * kMinWaves];
    __shared__ uint64_t s_base;
    const uint64_t tile = first_tile + blockIdx.x, t0 = tile * kMinTile;
    const uint64_t m = len - k + 1, n_win = m - w + 1, last_word = (len - 1) >> 5;
    const uint32_t lane = threadIdx.x, wave = lane >> 6, n_ent = kMinTile + w;
    const bool canon = canonical != 0;

    // level 0: the hash of local k-mer e = k-mer t0-1+e (for t0 = 0 and e = 0 that wraps to ~0, which is >= m)
    uint64_t ch[kMinRounds];
    uint16_t ci[kMinRounds];
#pragma unroll
    for (int r = 0; r < kMinRounds; ++r) {
        const uint32_t e = r * kMinBlock + lane;
        const uint64_t i = t0 + e - 1;
        ch[r] = e < n_ent && i < m ? fmix64(minimizer_kmer(in, last_word, i, k, canon)) : ~0ull;
        ci[r] = (uint16_t)e;
        if (e < n_ent) {
            s_h[e] = ch[r];
            s_i[e] = (uint16_t)e;
        }
    }
    __syncthreads();
    // doubling: level j+1 at e = the smaller of level j at e and at e+d (d = 2^j; ties keep e's: its position is smaller)
    uint32_t d = 1;
    for (; 2 * d <= w; d <<= 1) {
        uint32_t changed = 0;
#pragma unroll
        for (int r = 0; r < kMinRounds; ++r) {
            const uint32_t e = r * kMinBlock + lane;
            if (e + d < n_ent) {
                const uint64_t hb = s_h[e + d];
                if (hb < ch[r]) {
                    ch[r] = hb;
                    ci[r] = s_i[e + d];
                    changed |= 1u << r;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kMinRounds; ++r) {
            if (changed & (1u << r)) {
                const uint32_t e = r * kMinBlock + lane;
                s_h[e] = ch[r];
                s_i[e] = ci[r];
            }
        }
        __syncthreads();
    }
    // window s (local; = window t0-1+s) spans entries [s, s+w): level L at s and at s+w-d cover it
    const uint32_t off = w - d;
    auto argmin = [&](uint32_t s) -> uint32_t { return s_h[s + off] < s_h[s] ? s_i[s + off] : s_i[s]; };
    uint64_t ballots[kMinWinRounds];
    uint32_t p[kMinWinRounds];
#pragma unroll
    for (int r = 0; r < kMinWinRounds; ++r) {
        const uint32_t s = r * kMinBlock + lane + 1;
        const uint64_t t = t0 + s - 1;
        p[r] = argmin(s);
        const bool fresh = t < n_win && (t == 0 || p[r] != argmin(s - 1));
        ballots[r] = __ballot(fresh);
        if ((lane & 63) == 0) s_cnt[r * kMinWaves + wave] = (uint32_t)__popcll(ballots[r]);
    }
    __syncthreads();
    if (!WRITE) {
        if (lane == 0) {
            uint64_t c = 0;
            for (int q = 0; q < kMinWinRounds * kMinWaves; ++q) c += s_cnt[q];
            counts[tile] = (uint32_t)c;
        }
        return;
    }
    // output order = window order = (round, wave, lane): exclusive offsets of the (round, wave) groups, then the rank in the wave
    if (lane == 0) {
        uint32_t c = 0;
        for (int q = 0; q < kMinWinRounds * kMinWaves; ++q) {
            const uint32_t x = s_cnt[q];
            s_cnt[q] = c;
            c += x;
        }
        s_base = counted_tile_base(offs, counts, tile);
    }
    __syncthreads();
    const uint64_t base = s_base;
#pragma unroll
    for (int r = 0; r < kMinWinRounds; ++r) {
        const uint64_t b = ballots[r];
        if (!((b >> (lane & 63)) & 1)) continue;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        const uint64_t j = base + s_cnt[r * kMinWaves + wave] + rank;
        if (j >= out_cap) continue;
        const uint64_t i = t0 + p[r] - 1;
        __builtin_nontemporal_store(i, pos + j);
        if (val) __builtin_nontemporal_store(minimizer_kmer(in, last_word, i, k, canon), val + j);
    }
}

}  // namespace cnt
