// extract_kernels.hpp -- region extraction on 2-bit packed words (include/cute_nt.h, "region extraction"): n regions of one
// length, each packed like a sequence of its own, forward or as the reverse complement of the region.  Not in the reference; the
// definition is restated per base by tests/test_extract.py.
//
// Output word j of a record is ONE 64-bit window of the input at an arbitrary bit phase: forward the window at nucleotide
// start + 32j, reversed the window at start + region_len - 32 - 32j with its codes reversed and complemented (reverse_codes64,
// ^ 0xAAAA...).  A window straddles two input words; the funnel is the branch-free funnel64 (both: word_tile.hpp).  Two shapes:
//   extract_words       one thread per output word, words [j0, j0 + w) of every record: short windows (a gather: address
//                       arithmetic and two dependent loads per word), the remainder of long records behind their tiles, and the
//                       words cnt_subseq_dev peels in front of the first 128-B line of its output.
//   extract_tiles_fwd   records of >= 512 words: one workgroup per 512 consecutive output words of ONE record, two words and
//   extract_tiles_rev   one 16-B store per lane.  The tile's source word and bit phase are wave-uniform (start[i] is a scalar
//                       load, or the kernel argument start0 of cnt_subseq), each lane issues one 16-B and one 8-B raw-buffer
//                       load, both in flight before the first wait, policies of complement_tiles.
// A region is REJECTED when it does not lie inside the sequence (start > len or region_len > len - start: no overflow, so a
// start of 2^64-1 is a rejected region and not a wrap-around): its record is zero words and it is counted once, at its word 0.
// Whatever start[] holds, nothing outside the input words is read: the word kernel reads for accepted regions only, and the
// tiles' descriptors are clipped to the input's extent (empty for a rejected region), so a lane that aims outside reads zeros.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"
#include "find_kernels.hpp"
#include "packed_ops_kernels.hpp"

namespace cnt {

constexpr int kExtractBlock = 256;
constexpr uint32_t kExtractTileWords = 2 * kExtractBlock;  // output words per tile: 512 = 16384 nt
constexpr uint32_t kExtractRevcomp = 0x40u;                 // CNT_EXTRACT_REVCOMP (asserted equal in extract_abi.inc)
constexpr uint32_t kExtractOutside = 0xFFFFFFF0u;           // a byte offset no descriptor here reaches: the load returns zeros

// what the kernels of one call share.  start == nullptr: the one region of cnt_subseq, at start0.
struct ExtractArgs {
    const uint8_t* in;
    uint64_t words, len;  // the input: cnt_words_for(len) words
    const uint64_t* start;
    const uint64_t* info;  // may be nullptr
    uint64_t start0, region_len, rec_words;  // rec_words = R = cnt_words_for(region_len)
    uint32_t rev;                            // 1: CNT_EXTRACT_REVCOMP
    uint8_t* out;
    unsigned long long* rejected;  // may be nullptr
};

struct ExtractRegion {
    uint64_t start;
    bool rev, rejected;
};

__device__ __forceinline__ ExtractRegion extract_region(const ExtractArgs& a, uint64_t i) {
    ExtractRegion r;
    r.start = a.start ? a.start[i] : a.start0;
    const uint32_t strand = a.info ? (uint32_t)(a.info[i] & kFindReverse) : 0u;  // every other bit of info[i] is ignored
    r.rev = (a.rev != 0) != (strand != 0);
    r.rejected = r.start > a.len || a.region_len > a.len - r.start;
    return r;
}

// the codes a record keeps of its word j: all 32, or the low region_len % 32 of its last word
__device__ __forceinline__ uint64_t extract_keep(uint64_t region_len, uint64_t j) {
    const uint64_t rem = region_len - (j << 5);
    return rem >= 32 ? ~0ull : (1ull << (2 * (uint32_t)rem)) - 1;
}

// Words [j0, j0 + w) of every record, w < 2^31: workgroup b of a launch takes the 256 flat words behind the launch's first, which
// is word r_first of the w of record i_first (the launcher's division); the lane's split into (record, word) is a 32-bit divide.
// `left` = flat words from the launch's first to the end of the call.
__global__ __launch_bounds__(kExtractBlock) void extract_words(ExtractArgs a, uint64_t j0, uint32_t w, uint64_t i_first, uint32_t r_first,
                                                               uint64_t left) {
    const uint32_t f = blockIdx.x * (uint32_t)kExtractBlock + threadIdx.x, x = r_first + f, q = x / w;
    const uint64_t i = i_first + q, j = j0 + (x - q * w);
    uint32_t bad = 0;
    if (f < left) {
        const ExtractRegion r = extract_region(a, i);
        const uint64_t* in = reinterpret_cast<const uint64_t*>(a.in);
        uint64_t o = 0;
        if (!r.rejected) {
            uint64_t window;
            // input nts p .. p+31; reversed, p may lie below the region and, for the record's last word, below 0
            const int64_t p = r.rev ? (int64_t)(r.start + a.region_len) - 32 - (int64_t)(j << 5) : (int64_t)(r.start + (j << 5));
            if (p >= 0) {
                const uint64_t iw = (uint64_t)p >> 5;
                const uint32_t sh = 2u * ((uint32_t)p & 31u);
                window = in[iw] >> sh;
                if (sh && iw + 1 < a.words) window |= in[iw + 1] << (64 - sh);  // a word behind the input holds no code of the region
            } else {
                window = in[0] << (2u * (uint32_t)(-p));  // the first -p codes of the window do not exist
            }
            o = (r.rev ? reverse_codes64(window) ^ 0xAAAAAAAAAAAAAAAAull : window) & extract_keep(a.region_len, j);
        }
        reinterpret_cast<uint64_t*>(a.out)[i * a.rec_words + j] = o;
        bad = r.rejected && j == 0 ? 1u : 0u;
    }
    if (a.rejected) wave_add_invalid(bad, a.rejected);  // at most one atomic per wave, none without a rejected region
}

// Tile x = t_first + blockIdx.x counted from tile 0 of record i_first, `tiles` tiles per record: output words
// j_base + 512 t .. + 511 of record i (j_base: the words cnt_subseq_dev peeled, else 0), lane l the words jl = j + 2l, jl + 1.
// A kernel takes the records of its own orientation and leaves the others to its twin.
//   forward   source words J + 2l, J + 2l + 1 (16 B) and J + 2l + 2 (8 B; phase 0: aimed outside), J = (start + 32j) >> 5
//   reversed  as reverse_complement_tiles: with P = start + region_len - 32 - 32j (signed) and J = P >> 5, words J-2l-1, J-2l
//             (16 B) and J-2l+1 (8 B; phase 0: aimed outside).  The record's last word, when it is partial and part of a tile, has
//             its window at P - 32*511 >= -31: word J-511-1 may be word -1.  Then (wave-uniform, phase != 0) the wave loads one
//             word higher -- J-2l, J-2l+1 as 16 B, J-2l-1 as 8 B -- and the last lane's 8-B load aims outside: word -1 reads 0.
template <bool REV>
__device__ __forceinline__ void extract_tile(const ExtractArgs& a, uint64_t j_base, uint32_t tiles, uint64_t i_first, uint32_t t_first) {
    typedef unsigned int vu2 __attribute__((__vector_size__(8)));
    const uint32_t x = t_first + blockIdx.x, q = x / tiles, t = x - q * tiles, l = threadIdx.x;
    const uint64_t i = i_first + q;
    const ExtractRegion r = extract_region(a, i);
    if (r.rev != REV) return;
    const uint64_t j = j_base + (uint64_t)t * kExtractTileWords;
    const __amdgpu_buffer_rsrc_t rout = rsrc_of(a.out + (i * a.rec_words + j) * 8, kExtractTileWords * 8);
    uint64_t win0, win1;
    if constexpr (!REV) {
        const uint64_t S = r.start + (j << 5), J = r.rejected ? 0 : S >> 5;
        const uint32_t sh = 2u * ((uint32_t)S & 31u);
        const uint64_t avail = r.rejected ? 0 : a.words - J;  // J < words for an accepted region
        const __amdgpu_buffer_rsrc_t rin = rsrc_of(a.in + J * 8, (uint32_t)(avail < kExtractTileWords + 2 ? avail : kExtractTileWords + 2) * 8);
        const vu4 v = __builtin_amdgcn_raw_buffer_load_b128(rin, l * 16, 0, kNT);
        const vu2 e = __builtin_amdgcn_raw_buffer_load_b64(rin, sh ? l * 16 + 16 : kExtractOutside, 0, kNT);
        uint64_t w0, w1;
        u64_pair(v, w0, w1);
        const uint64_t w2 = ((uint64_t)e[1] << 32) | e[0];
        win0 = funnel64(w0, w1, sh);
        win1 = funnel64(w1, w2, sh);
    } else {
        const int64_t P = (int64_t)(r.start + a.region_len) - 32 - (int64_t)(j << 5);
        const int64_t lo = r.rejected ? 0 : (P >> 5) - (int64_t)(kExtractTileWords - 1);  // the tile's lowest window word: >= -1
        const bool neg = lo < 0;
        const uint32_t sh = 2u * ((uint32_t)P & 31u);
        const uint64_t b = neg ? 0 : (uint64_t)lo;
        const uint64_t avail = r.rejected ? 0 : a.words - b;
        const __amdgpu_buffer_rsrc_t rin = rsrc_of(a.in + b * 8, (uint32_t)(avail < kExtractTileWords + 2 ? avail : kExtractTileWords + 2) * 8);
        const uint32_t off_e = neg ? (l == kExtractBlock - 1 ? kExtractOutside : (kExtractTileWords - 3 - 2 * l) * 8)
                                   : (sh ? (kExtractTileWords - 2 * l) * 8 : kExtractOutside);
        const vu4 v = __builtin_amdgcn_raw_buffer_load_b128(rin, (kExtractTileWords - 2 - 2 * l) * 8, 0, kNT);
        const vu2 e = __builtin_amdgcn_raw_buffer_load_b64(rin, off_e, 0, kNT);
        uint64_t x0, x1;
        u64_pair(v, x0, x1);
        const uint64_t y = ((uint64_t)e[1] << 32) | e[0];
        const uint64_t wm = neg ? y : x0, wj = neg ? x0 : x1, wp = neg ? x1 : y;  // input words J-2l-1, J-2l, J-2l+1
        win0 = reverse_codes64(funnel64(wj, wp, sh)) ^ 0xAAAAAAAAAAAAAAAAull;
        win1 = reverse_codes64(funnel64(wm, wj, sh)) ^ 0xAAAAAAAAAAAAAAAAull;
    }
    const uint64_t live = r.rejected ? 0 : ~0ull;  // a rejected region's tiles store zeros
    const uint64_t o0 = win0 & extract_keep(a.region_len, j + 2 * l) & live, o1 = win1 & extract_keep(a.region_len, j + 2 * l + 1) & live;
    __builtin_amdgcn_raw_buffer_store_b128(pack_u64x2(o0, o1), rout, l * 16, 0, kSC0 | kSC1 | kNT);
    if (r.rejected && j == 0 && l == 0 && a.rejected)  // the region's word 0 is in this tile: counted here, once
        (void)__hip_atomic_fetch_add(a.rejected, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// plain functions over the one body (find_kernels.hpp does the same): named for what they do in a profile
__global__ __launch_bounds__(kExtractBlock) void extract_tiles_fwd(ExtractArgs a, uint64_t j_base, uint32_t tiles, uint64_t i_first, uint32_t t_first) {
    extract_tile<false>(a, j_base, tiles, i_first, t_first);
}
__global__ __launch_bounds__(kExtractBlock) void extract_tiles_rev(ExtractArgs a, uint64_t j_base, uint32_t tiles, uint64_t i_first, uint32_t t_first) {
    extract_tile<true>(a, j_base, tiles, i_first, t_first);
}

}  // namespace cnt
