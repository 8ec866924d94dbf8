// word_tile.hpp -- what the kernels over 2-bit packed words share on the device: a lane's pair of words, the windows that straddle
// them, the mask of the positions below a bound, the rank of a lane's entries in its tile, code reversal and 64-bit wave shuffles.
// Device-only, every function inlined, no kernel.
//
// Shape of a tile (find, ORF scan, homopolymer compression, k-mer counts): a workgroup of TILE_WORDS lanes owns TILE_WORDS
// consecutive input words, lane j the 32 positions that start in word j of the tile; it reads that word and a neighbour, walks
// its 32 windows with constant shifts into bit masks, and the lanes' entry counts are ranked across the tile in lane order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"

namespace cnt {

// the two words of a 16-B vector, and back (as the buffer builtins' type)
__device__ __forceinline__ void u64_pair(vu4 q, uint64_t& lo, uint64_t& hi) {
    lo = ((uint64_t)q[1] << 32) | q[0];
    hi = ((uint64_t)q[3] << 32) | q[2];
}
__device__ __forceinline__ vu4 pack_u64x2(uint64_t o0, uint64_t o1) {
    return vu4{(uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32)};
}

// Lane j of the tile that begins at word w0: lo = word w0 + j - BACK, hi = the word behind it, of the input's `words` words.  A tile
// whose TILE_WORDS + 1 words all exist takes one 16-B raw-buffer load per lane at 8-B grain, `nt`; the others (the last one or two
// and, with BACK = 1, the first, whose descriptor would begin 8 B in front of the input) read word by word, each read guarded: a
// word that does not exist reads as 0.  That includes the word in FRONT of word 0: its index wraps to ~0, which is not below `words`.
template <uint64_t TILE_WORDS, uint64_t BACK = 0>
__device__ __forceinline__ void word_tile_pair(const uint8_t* __restrict__ in, uint64_t words, uint64_t w0, uint32_t j, uint64_t& lo, uint64_t& hi) {
    if (w0 >= BACK && w0 - BACK + TILE_WORDS + 1 <= words) {
        const __amdgpu_buffer_rsrc_t rin = rsrc_of(in + (w0 - BACK) * 8, (uint32_t)(TILE_WORDS + 1) * 8);
        u64_pair(__builtin_amdgcn_raw_buffer_load_b128(rin, j * 8, 0, kNT), lo, hi);
    } else {
        const uint64_t* in64 = reinterpret_cast<const uint64_t*>(in);
        const uint64_t w = w0 + j - BACK;
        lo = w < words ? in64[w] : 0;
        hi = w + 1 < words ? in64[w + 1] : 0;
    }
}

// The 64 bits from bit sh (even, 0..62) of lo on, hi behind lo.  Branch-free: (hi << 1) << (63 - sh) is hi << (64 - sh) for
// sh = 2..62 and 0 for sh = 0.  With `if (sh)` around the OR the compiler sank the load of hi into the branch, BEHIND the first
// load's s_waitcnt: two dependent trips to memory per tile (tests/test_isa_digest.py counts the loads in flight at the first wait).
__device__ __forceinline__ uint64_t funnel64(uint64_t lo, uint64_t hi, uint32_t sh) { return (lo >> sh) | ((hi << 1) << (63 - sh)); }

// the 32 bits from code r (0..31, a constant after unrolling) of the dwords d[] on: one v_alignbit_b32, nothing 64 bits wide
__device__ __forceinline__ uint32_t window_dword(const uint32_t* d, uint32_t r) {
    const uint32_t i = r >> 4, sh = 2 * (r & 15u);
    return sh ? __builtin_amdgcn_alignbit(d[i + 1], d[i], sh) : d[i];
}

// bit r set iff position i0 + r < x
__device__ __forceinline__ uint32_t codes_below(uint64_t i0, uint64_t x) {
    return x <= i0 ? 0u : (x - i0 >= 32 ? ~0u : (1u << (uint32_t)(x - i0)) - 1u);
}

// the inclusive sum of c over the lanes 0 .. lane of a wave (lane order = output order)
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t c, uint32_t lane) {
    uint32_t x = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    return x;
}

// The rank of a lane's c entries among its tile's, in three pieces around the ONE barrier of the kernel, which has its own
// shared-memory writes to put in front of it.  Before the barrier: the lane's inclusive sum over its wave, the wave's posted to
// s_cnt[wave].  Behind it: the tile's total (count passes), or the entries of the tile in front of the lane (write passes) from
// excl = inclusive sum - c.  A tile's total is below 2^32 (each file's static_assert), so the caller adds the u32 to its 64-bit base once.
__device__ __forceinline__ uint32_t tile_rank_post(uint32_t c, uint32_t* s_cnt) {
    const uint32_t x = wave_inclusive_sum(c, threadIdx.x & 63u);
    if ((threadIdx.x & 63u) == 63u) s_cnt[threadIdx.x >> 6] = x;
    return x;
}
template <int WAVES>
__device__ __forceinline__ uint32_t tile_total(const uint32_t* s_cnt) {
    uint32_t total = 0;
#pragma unroll
    for (int q = 0; q < WAVES; ++q) total += s_cnt[q];
    return total;
}
template <int WAVES>
__device__ __forceinline__ uint32_t tile_before(const uint32_t* s_cnt, uint32_t excl) {
#pragma unroll
    for (int q = 0; q < WAVES - 1; ++q) excl += q < (int)(threadIdx.x >> 6) ? s_cnt[q] : 0u;
    return excl;
}

// reverse the order of the 32 (16) two-bit codes of a word (dword): a bit reverse also swaps the two bits inside each code, so
// they are swapped back
__device__ __forceinline__ uint64_t reverse_codes64(uint64_t x) {
    x = __builtin_bitreverse64(x);
    return ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
}
__device__ __forceinline__ uint32_t reverse_codes32(uint32_t x) {
    x = __builtin_bitreverse32(x);
    return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
}

// 64-bit wave shuffles, as two dwords: the value of lane - o (the lanes below o keep what __shfl_up gives them: their own), and the
// sum over the wave, which lane 0 holds
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int o) {
    const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_down((uint32_t)v, off, 64), hi = __shfl_down((uint32_t)(v >> 32), off, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

}  // namespace cnt
