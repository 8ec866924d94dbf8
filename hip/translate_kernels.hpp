// translate_kernels.hpp -- codon translation on 2-bit packed words (include/cute_nt.h, "translation"): nucleotides
// [start, start + sub_len) read in threes, forward or as the reverse complement of the region, one table byte per codon.  Not in
// the reference; the definition is restated per codon by tests/test_translate.py.
//
// A codon is 6 bits of the packed stream and its own index into the 64-byte table (the value cnt_kmers writes for k = 3).  3 does
// not divide 32: 16 codons are 96 bits = three dwords at a bit phase that is the same for every lane, since 48 nt are three whole
// dwords.  Two shapes:
//   translate_tiles_fwd   one workgroup per 4096 consecutive output bytes (12288 nt) that start on a 16-B boundary of the output,
//   translate_tiles_rev   16 codons and one 16-B store per lane.  The tile's source dword and bit phase are wave-uniform (start is a
//                         kernel argument); each lane issues one 12-B raw-buffer load and one 4-B load for the dword the phase
//                         spills into (phase 0: aimed outside), both in flight before the first wait, policies of extract_tiles_*.
//                         The table travels as kernel arguments and is staged into 64 B of LDS once per workgroup: 16 consecutive
//                         dwords are 16 different banks, so the byte reads at data-dependent indices never conflict (equal
//                         dwords broadcast).
//   translate_edge        one thread per output byte: the bytes in front of the first 16-B boundary, the remainder behind the last
//                         whole tile, and every call below one tile.
// The reverse strand needs no second path through the table: with v the FORWARD codon value at p = start + sub_len - 3 - 3j,
// out[j] = table[rc3(v)], rc3 swapping the outer codes and complementing all three.  The launcher hands the reverse kernels
// table o rc3 (translate_abi.inc), and they walk the region downward: the reverse tile is the forward tile with the lanes, and the
// 16 bytes of a lane, in opposite order.
// Nothing outside the input words is read: every dword of a lane's 12-B load holds a nucleotide of the region, the fourth dword
// is asked for only when it does, and the descriptor is clipped to the input's extent besides.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"

namespace cnt {

constexpr int kTranslateBlock = 256;
constexpr uint32_t kTranslateTileBytes = 16 * kTranslateBlock;  // output bytes per tile: 4096 = 12288 nt
constexpr uint32_t kTranslateTileDwords = 3 * kTranslateBlock;  // packed dwords a tile consumes, plus one for the phase
constexpr uint32_t kTranslateRevcomp = 0x80u;                   // CNT_TRANSLATE_REVCOMP (asserted equal in translate_abi.inc)
constexpr uint32_t kTranslateOutside = 0xFFFFFFF0u;             // a byte offset no descriptor here reaches: the load returns zeros

// what the kernels of one call share.  table: 64 bytes as 16 dwords, for a reversed call already composed with rc3.
struct TranslateArgs {
    const uint8_t* in;
    uint64_t words;  // the input: cnt_words_for(len) words
    uint64_t start, sub_len;
    uint8_t* out;
    uint32_t rev;  // 1: CNT_TRANSLATE_REVCOMP
    uint32_t table[16];
};

// the table from the kernel arguments (scalar registers) into LDS: thread 0, four 16-B writes, one barrier
__device__ __forceinline__ void translate_stage_table(u32x4* lds, const TranslateArgs& a) {
    if (threadIdx.x == 0) {
        lds[0] = u32x4{a.table[0], a.table[1], a.table[2], a.table[3]};
        lds[1] = u32x4{a.table[4], a.table[5], a.table[6], a.table[7]};
        lds[2] = u32x4{a.table[8], a.table[9], a.table[10], a.table[11]};
        lds[3] = u32x4{a.table[12], a.table[13], a.table[14], a.table[15]};
    }
    __syncthreads();
}

// Output bytes [j_base + j, j_base + j + count) of the call, count < 2^32: thread f the byte j_base + f.  Its codon sits at
// nucleotide p (forward start + 3j, reversed start + sub_len - 3 - 3j) and may straddle two words; p + 2 lies inside the region,
// so the word behind a straddling codon's first is an input word and needs no guard.
__global__ __launch_bounds__(kTranslateBlock) void translate_edge(TranslateArgs a, uint64_t j_base, uint32_t count) {
    __shared__ u32x4 tab[4];
    translate_stage_table(tab, a);
    const uint32_t f = blockIdx.x * (uint32_t)kTranslateBlock + threadIdx.x;
    if (f >= count) return;
    const uint64_t j = j_base + f;
    const uint64_t p = a.rev ? a.start + a.sub_len - 3 - 3 * j : a.start + 3 * j;
    const uint64_t* in = reinterpret_cast<const uint64_t*>(a.in);
    const uint64_t iw = p >> 5;
    const uint32_t sh = 2u * ((uint32_t)p & 31u);
    uint64_t v = in[iw] >> sh;
    if (sh > 58) v |= in[iw + 1] << (64 - sh);  // the codon's last one or two codes are in the next word
    a.out[j] = reinterpret_cast<const uint8_t*>(tab)[v & 63];
}

// Tile t_first + blockIdx.x of the call: output bytes j .. j + 4095, j = j_base + 4096 t (j_base: the bytes the edge kernel takes
// in front of the first 16-B boundary of the output).  P = the lowest nucleotide the tile reads: forward start + 3j, reversed
// start + sub_len - 3(j + 4096) >= start.  The tile is whole, so nucleotides P .. P + 12287 all lie inside the region: they fill
// dwords D = P >> 4 .. D + 767 from bit 2(P & 15) on and, at a non-zero phase, the low bits of dword D + 768.  Every one of those
// dwords holds an input nucleotide, so D < 2 * words and avail = 2 * words - D >= 768, + 1 at a non-zero phase.  Lane slot s reads dwords (P >> 4) + 3s .. + 3 at the bit phase 2(P & 15); forward the
// lane is its own slot and codon m of the slot is byte m of its 16, reversed lane l has slot 255 - l and codon m is byte 15 - m.
template <bool REV>
__device__ __forceinline__ void translate_tile(const TranslateArgs& a, uint64_t j_base, uint64_t t_first) {
    typedef unsigned int vu3 __attribute__((__vector_size__(12)));
    __shared__ u32x4 tab[4];
    const uint32_t l = threadIdx.x, s = REV ? (uint32_t)kTranslateBlock - 1 - l : l;
    const uint64_t j = j_base + (t_first + blockIdx.x) * kTranslateTileBytes;
    const uint64_t P = REV ? a.start + a.sub_len - 3 * (j + kTranslateTileBytes) : a.start + 3 * j;
    const uint64_t D = P >> 4, avail = 2 * a.words - D;  // >= 768 (+ 1 when sh != 0), see above
    const uint32_t sh = 2u * ((uint32_t)P & 15u);
    const __amdgpu_buffer_rsrc_t rin = rsrc_of(a.in + D * 4, (uint32_t)(avail < kTranslateTileDwords + 1 ? avail : kTranslateTileDwords + 1) * 4);
    const __amdgpu_buffer_rsrc_t rout = rsrc_of(a.out + j, kTranslateTileBytes);
    const vu3 v = __builtin_amdgcn_raw_buffer_load_b96(rin, s * 12, 0, kNT);
    const uint32_t e = __builtin_amdgcn_raw_buffer_load_b32(rin, sh ? s * 12 + 12 : kTranslateOutside, 0, kNT);
    translate_stage_table(tab, a);
    // the slot's 96 bits; the funnel is the branch-free (x << 1) << (31 - sh) of the extract tiles, on dwords
    const uint32_t x0 = (v[0] >> sh) | ((v[1] << 1) << (31 - sh)), x1 = (v[1] >> sh) | ((v[2] << 1) << (31 - sh)),
                   x2 = (v[2] >> sh) | ((e << 1) << (31 - sh));
    const uint64_t lo = ((uint64_t)x1 << 32) | x0, hi = ((uint64_t)x2 << 32) | x1;  // bits 0..63 and 32..95
    const uint8_t* t8 = reinterpret_cast<const uint8_t*>(tab);
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) {
        const uint32_t bit = 6 * (REV ? 15 - b : b);
        const uint32_t c = (uint32_t)(bit <= 58 ? lo >> bit : hi >> ((bit - 32) & 63)) & 63u;  // codon 10 straddles bit 64
        o[b >> 2] |= (uint32_t)t8[c] << (8 * (b & 3));
    }
    const u32x4 ov = {o[0], o[1], o[2], o[3]};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(vu4, ov), rout, l * 16, 0, kSC0 | kSC1 | kNT);
}

// plain functions over the one body (find_kernels.hpp and extract_kernels.hpp do the same): named for what they do in a profile
__global__ __launch_bounds__(kTranslateBlock) void translate_tiles_fwd(TranslateArgs a, uint64_t j_base, uint64_t t_first) {
    translate_tile<false>(a, j_base, t_first);
}
__global__ __launch_bounds__(kTranslateBlock) void translate_tiles_rev(TranslateArgs a, uint64_t j_base, uint64_t t_first) {
    translate_tile<true>(a, j_base, t_first);
}

}  // namespace cnt
