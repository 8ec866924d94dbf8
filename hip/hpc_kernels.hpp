// hpc_kernels.hpp -- homopolymer compression on 2-bit packed words (include/cute_nt.h, "homopolymer compression"): every run of
// equal bases collapses to one base, and the position each run started at is reported beside it.  Not in the reference; the
// definition is restated per base by tests/test_hpc.py.
//
// For the codes x_0 .. x_{len-1}: position i is KEPT iff i == 0 or x_i != x_{i-1}.  With the kept positions p_0 < .. < p_{n-1}
// the result is the n codes x_{p_0}, x_{p_1}, .. packed as the encoder packs them, and pos[j] = p_j.  Bits beyond len neither
// extend nor start a run: a position at or past len is never kept, and a kept one is compared with positions below len only.
//
// The packed output is a bit stream: a tile's codes begin at any 2-bit phase of an output word, and a tile that lies inside a
// long run contributes nothing, so any number of tiles can meet in one word.  Passes (hpc_abi.inc), none of which allocates;
// counts / offs and the scan are the counted output of counted_output.hpp:
//   1. hpc_count       one workgroup per tile of kHpcTile positions: counts[tile] = the tile's kept positions;
//   2. counted_scan    offs[group], *count SET to n;
//   3. hpc_zero_edges  one LANE per tile: zeroes the tile's first output word when the tile begins inside it and its last one
//                      when the tile ends inside it -- the only words that tiles share;
//   4. hpc_write[_pos] a tile whose count is 0 returns at once; the others repeat pass 1, compress each lane's word to its kept
//                      codes (five log steps on 2-bit lanes), OR the fragments at their bit offsets into the tile's 257 output
//                      words in LDS, and store those in one coalesced pass: the words pass 3 zeroed are merged atomically
//                      (hpc_merge), every other word is stored plainly.  The positions go through LDS as u16 offsets into the
//                      tile, so that a wave's stores are contiguous.
// Codes at or past out_cap are clipped before the LDS stage; no word at or past cnt_words_for(min(n, out_cap)) is touched.
// Shape of a tile, as in word_tile.hpp: lane j owns the 32 positions of word j of the tile; it reads that word and the one in
// FRONT of it (word_tile_pair with BACK = 1), whose top code decides position 0 of the lane.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"
#include "counted_output.hpp"

namespace cnt {

constexpr int kHpcBlock = 256;
constexpr int kHpcWaves = kHpcBlock / 64;
constexpr uint64_t kHpcTileWords = kHpcBlock, kHpcTile = 32 * kHpcTileWords;  // positions per tile: 8192
static_assert(kHpcTile <= (1u << 16), "a position inside a tile is a u16");

struct HpcArgs {
    const uint8_t* in;
    uint64_t words, len;  // ceil(len / 32); len >= 1
    uint64_t n_tiles;     // ceil(len / kHpcTile)
    uint32_t* counts;
    uint64_t* offs;
    uint64_t *out, *pos;  // pos may be NULL
    uint64_t out_cap;     // codes
};

// The lane's word w and its keep mask: bit 2r set iff position 32 * (word index) + r is kept.
__device__ __forceinline__ uint64_t hpc_keep(const HpcArgs& a, uint64_t tile, uint64_t& w) {
    const uint32_t j = threadIdx.x;
    const uint64_t w0 = tile * kHpcTileWords;
    uint64_t prev;
    word_tile_pair<kHpcTileWords, 1>(a.in, a.words, w0, j, prev, w);  // tile 0 reads guarded: word -1 is 0
    const uint64_t i0 = (w0 + j) * 32;
    const uint64_t d = w ^ ((w << 2) | (prev >> 62));  // code r against code r - 1
    uint64_t keep = (d | (d >> 1)) & 0x5555555555555555ull;
    if (i0 == 0) keep |= 1ull;
    const uint64_t valid = i0 >= a.len ? 0ull : (a.len - i0 >= 32 ? ~0ull : (1ull << (2 * (uint32_t)(a.len - i0))) - 1ull);
    return keep & valid;
}

// The codes of the dword x that `keep` marks (bit 2r), in order, in the low bits; zeros above them.  The compress of Hacker's
// Delight 7-4 with a 2-bit unit: a code moves down by twice the number of dropped codes below it, one binary digit of that number
// per step.  Dword by dword: a 64-bit shift is two or three instructions, and the passes are bound by their VALU work.
__device__ __forceinline__ uint32_t hpc_compress16(uint32_t x, uint32_t keep) {
    uint32_t m = keep | (keep << 1);
    x &= m;
    uint32_t mk = ~m << 2;  // the dropped codes, counted from the code above each
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t mp = mk ^ (mk << 2);  // parity of the dropped codes below
        mp ^= mp << 4;
        mp ^= mp << 8;
        mp ^= mp << 16;
        const uint32_t mv = mp & m;  // the codes that move in this step
        m = (m ^ mv) | (mv >> (2 << i));
        const uint32_t t = x & mv;
        x = (x ^ t) | (t >> (2 << i));
        mk &= ~mp;
    }
    return x;
}
// the same of a word: the high half's codes behind the low half's
__device__ __forceinline__ uint64_t hpc_compress(uint64_t x, uint64_t keep) {
    const uint32_t lo = hpc_compress16((uint32_t)x, (uint32_t)keep), hi = hpc_compress16((uint32_t)(x >> 32), (uint32_t)(keep >> 32));
    return lo | ((uint64_t)hi << (2 * __popc((uint32_t)keep)));
}

// what a tile may write: `room` codes from code `base` on, after the clip at out_cap; room = 0: nothing
struct HpcSpan {
    uint64_t base;
    uint32_t room;
};
__device__ __forceinline__ HpcSpan hpc_span(const HpcArgs& a, uint64_t tile, uint32_t total) {
    const uint64_t base = counted_tile_base(a.offs, a.counts, tile);
    return {base, base >= a.out_cap ? 0u : (uint32_t)(a.out_cap - base < total ? a.out_cap - base : total)};
}
// the span's first / last output word is shared with other tiles
__device__ __forceinline__ bool hpc_head_shared(const HpcSpan& s) { return (s.base & 31u) != 0; }
__device__ __forceinline__ bool hpc_tail_shared(const HpcSpan& s) { return ((s.base + s.room) & 31u) != 0; }

// ORs v into a word that pass 3 zeroed and other tiles merge into at the same time.  A compare-and-swap loop and not an atomic OR:
// with a pinned caller buffer the word is host memory, and swap, add and compare-and-swap are the only atomics a PCIe link
// carries.  The first guess is the zero the word started from; at most two words of a tile come here.
__device__ __forceinline__ void hpc_merge(uint64_t* p, unsigned long long v) {
    unsigned long long* q = reinterpret_cast<unsigned long long*>(p);
    unsigned long long seen = 0, old;
    while ((old = atomicCAS_system(q, seen, seen | v)) != seen) seen = old;
}

// pass 1
__global__ __launch_bounds__(kHpcBlock) void hpc_count(HpcArgs a, uint64_t first_tile) {
    __shared__ uint32_t s_cnt[kHpcWaves];
    const uint64_t tile = first_tile + blockIdx.x;
    uint64_t w;
    const uint64_t keep = hpc_keep(a, tile, w);
    tile_rank_post((uint32_t)__popcll(keep), s_cnt);
    __syncthreads();
    if (threadIdx.x == 0) a.counts[tile] = tile_total<kHpcWaves>(s_cnt);
}

// pass 3: lane = tile first_block * kHpcBlock + blockIdx.x * kHpcBlock + threadIdx.x
__global__ __launch_bounds__(kHpcBlock) void hpc_zero_edges(HpcArgs a, uint64_t first_block) {
    const uint64_t tile = (first_block + blockIdx.x) * kHpcBlock + threadIdx.x;
    if (tile >= a.n_tiles) return;
    const uint32_t total = a.counts[tile];
    if (total == 0) return;
    const HpcSpan s = hpc_span(a, tile, total);
    if (s.room == 0) return;
    if (hpc_head_shared(s)) a.out[s.base >> 5] = 0;
    if (hpc_tail_shared(s)) a.out[(s.base + s.room - 1) >> 5] = 0;
}

// pass 4
template <bool POS>
__device__ __forceinline__ void hpc_write_tile(const HpcArgs& a, uint64_t first_tile) {
    __shared__ unsigned long long s_out[kHpcTileWords + 1];
    __shared__ uint32_t s_cnt[kHpcWaves];
    __shared__ HpcSpan s_span;
    const uint64_t tile = first_tile + blockIdx.x;
    const uint32_t j = threadIdx.x;
    uint64_t w;
    const uint64_t keep = hpc_keep(a, tile, w);  // the load is under way before the count is waited for
    const uint32_t total = a.counts[tile];
    if (total == 0) return;
    s_out[j] = 0;
    if (j == 0) {
        s_out[kHpcTileWords] = 0;
        s_span = hpc_span(a, tile, total);
    }
    const uint32_t c = (uint32_t)__popcll(keep);
    const uint32_t x = tile_rank_post(c, s_cnt);  // lane order = position order
    __syncthreads();
    const HpcSpan s = s_span;
    if (s.room == 0) return;  // everything of the tile lies at or past out_cap
    const uint32_t before = tile_before<kHpcWaves>(s_cnt, x - c);  // the tile's kept positions in front of the lane
    const uint32_t phase = (uint32_t)(s.base & 31u);
    const uint32_t cc = before >= s.room ? 0u : (s.room - before < c ? s.room - before : c);  // the lane's codes below out_cap
    uint64_t frag = hpc_compress(w, keep);
    if (cc < 32) frag &= (1ull << (2 * cc)) - 1ull;
    if (cc) {
        const uint32_t at = phase + before, sh = 2 * (at & 31u);
        atomicOr(&s_out[at >> 5], (unsigned long long)(frag << sh));
        if ((at & 31u) + cc > 32) atomicOr(&s_out[(at >> 5) + 1], (unsigned long long)(frag >> (64 - sh)));
    }
    if constexpr (POS) {
        __shared__ uint16_t s_pos[kHpcTile];
        uint32_t e = before;
        for (uint64_t k = keep; k; k &= k - 1) s_pos[e++] = (uint16_t)(j * 32u + ((uint32_t)__builtin_ctzll(k) >> 1));
        __syncthreads();
        const uint64_t tile0 = tile * kHpcTile;
        for (uint32_t i = j; i < s.room; i += kHpcBlock) __builtin_nontemporal_store(tile0 + s_pos[i], a.pos + s.base + i);
    } else {
        __syncthreads();
    }
    const uint32_t n_words = (phase + s.room + 31u) >> 5;  // <= 257
    uint64_t* out = a.out + (s.base >> 5);
    for (uint32_t k = j; k < n_words; k += kHpcBlock) {
        const unsigned long long v = s_out[k];
        if ((k == 0 && hpc_head_shared(s)) || (k == n_words - 1 && hpc_tail_shared(s))) {
            if (v) hpc_merge(out + k, v);
        } else {
            out[k] = v;
        }
    }
}

__global__ __launch_bounds__(kHpcBlock) void hpc_write(HpcArgs a, uint64_t first_tile) { hpc_write_tile<false>(a, first_tile); }
__global__ __launch_bounds__(kHpcBlock) void hpc_write_pos(HpcArgs a, uint64_t first_tile) { hpc_write_tile<true>(a, first_tile); }

}  // namespace cnt
