// kmer_kernels.hpp -- k-mer extraction on 2-bit packed words (include/cute_nt.h, "k-mers"): for each position i < m =
// len-k+1 the k codes i..i+k-1 packed like a sequence of length k (forward), or the smaller of that and its reverse
// complement compared as u64 (canonical).  Not in the reference; the definitions are restated in numpy by tests/test_kmers.py.
//
// Traffic per k-mer: 8 B written, ~0.25 B read -- a write stream.  Shape of complement_tiles / reverse_complement_tiles
// (packed_ops_kernels.hpp): one workgroup per output tile, pairs of consecutive k-mers per lane, each pair one 16-B
// raw-buffer store with the codec tiles' write-through policy.  A pair needs input words w, w+1 (w = k-mer >> 5): one 16-B
// load at an 8-B-aligned address, shared through L1/TA by the ~16 lanes that read the same words.  Two pairs per lane (8-KiB
// tiles) instead of one: 1.73 ms instead of 2.06 for 2^30 nt (forward; 4-KiB tiles meant 2M workgroups per call).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"
#include "word_tile.hpp"

namespace cnt {

constexpr int kKmerBlock = 256, kKmerU = 2;  // U: k-mer pairs per lane (profiles/kmers_tile_ab.jsonl)
constexpr uint64_t kKmersPerTile = (uint64_t)kKmerBlock * 2 * kKmerU;

// `fwd` holds k codes in its low 2k bits, zero above.  Complementing sets the unused high codes to 2; reversing moves them
// to the low end, where the shift by 64-2k drops them.
template <bool CANONICAL>
__device__ __forceinline__ uint64_t kmer_finish(uint64_t fwd, uint32_t k) {
    if constexpr (CANONICAL) {
        const uint64_t rc = reverse_codes64(fwd ^ 0xAAAAAAAAAAAAAAAAull) >> (64 - 2 * k);
        return rc < fwd ? rc : fwd;
    } else {
        return fwd;
    }
}

// Tile: k-mers a .. a+2*BLOCK*U-1 with a = first + 2*BLOCK*U*blockIdx.x; out + 8a is 16-B aligned.  Lane j makes the pairs
// i = a + 2(u*BLOCK + j), i+1 (u < U: each store instruction of a wave covers 1 KiB) from input words w = i>>5 and w+1: the
// 64-bit window at i is a funnel shift of the two, the window at i+1 is that shifted by one code with nt i+32 (in word w+1)
// on top.  The launcher gives tiles only while their end <= 32*(words-1), so word w+1 of every lane lies inside the input.
template <int BLOCK, int U, bool CANONICAL>
__global__ __launch_bounds__(BLOCK) void kmer_tiles(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint64_t first, uint32_t k) {
    const uint64_t a = first + (uint64_t)blockIdx.x * (BLOCK * 2 * U);
    const uint64_t wa = a >> 5;
    // lanes reach word wa + ((a & 31) + 2*BLOCK*U - 1) / 32 + 1 at most
    const __amdgpu_buffer_rsrc_t rin = rsrc_of(in + wa * 8, (BLOCK * U / 16 + 2) * 8);
    const __amdgpu_buffer_rsrc_t rout = rsrc_of(out + a * 8, BLOCK * 16 * U);
    const uint32_t j = threadIdx.x, a31 = (uint32_t)a & 31u;
    vu4 q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) q[u] = __builtin_amdgcn_raw_buffer_load_b128(rin, ((a31 + 2 * (u * BLOCK + j)) >> 5) * 8, 0, kNT);
    const uint64_t mask = ~0ull >> (64 - 2 * k);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        uint64_t lo, hi;
        u64_pair(q[u], lo, hi);
        const uint32_t sh = 2u * ((a31 + 2 * (u * BLOCK + j)) & 31u);
        const uint64_t win0 = funnel64(lo, hi, sh);
        const uint64_t win1 = (win0 >> 2) | (((hi >> sh) & 3ull) << 62);
        const uint64_t o0 = kmer_finish<CANONICAL>(win0 & mask, k), o1 = kmer_finish<CANONICAL>(win1 & mask, k);
        __builtin_amdgcn_raw_buffer_store_b128(pack_u64x2(o0, o1), rout, (u * BLOCK + j) * 16, 0, kSC0 | kSC1 | kNT);
    }
}

// generic: one thread per k-mer in [first, end): the head until the output sits on a 128-B line, the tail past the last
// tile, and calls too short for a tile (the tiles read at 8-B grain: any input phase takes them).  Reads word w+1 only
// when the k-mer reaches into it (i+k-1 < len, so that word exists).
template <bool CANONICAL>
__global__ __launch_bounds__(kBlock) void kmer_generic(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint32_t k,
                                                       uint64_t first, uint64_t end) {
    const uint64_t mask = ~0ull >> (64 - 2 * k);
    for (uint64_t i = first + blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < end; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t w = i >> 5;
        const uint32_t sh = 2u * ((uint32_t)i & 31u);
        uint64_t x = in[w] >> sh;
        if (sh + 2 * k > 64) x |= in[w + 1] << (64 - sh);
        out[i] = kmer_finish<CANONICAL>(x & mask, k);
    }
}

}  // namespace cnt
