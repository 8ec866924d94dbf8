// window_count_kernels.hpp -- windowed base and dinucleotide counts on 2-bit packed words (include/cute_nt.h, "windowed
// composition"): for k = 1 or 2, one record of 4^k u32 per window [j*step, j*step + window), entry v the number of k-mers that lie
// WHOLLY inside the window and whose cnt_kmers value is v.  Not in the reference; the definition is restated three ways by
// tests/test_window_counts.py.
//
// The counting core has no table and no atomic: a word is split into its low-bit plane (x & 0x5555...) and its high-bit plane
// ((x >> 1) & 0x5555...), both are ANDed with the mask of the word's positions that the window counts, and a class is a popcount.
//   k = 1  three popcounts and the total: G = |L & H|, C = |L| - G, T = |H| - G, A = total - |L| - |H| + G.
//   k = 2  the second base's planes come from funnel64(x, next, 2), which puts the code of position p + 1 at position p; the
//          sixteen classes are the ANDs of four first-base masks with four second-base masks.  The position mask ends one
//          position earlier (a k-mer that straddles the window's end is not counted), so neither the bits beyond len nor the word
//          behind the window's last one ever reach a count.
//
// Parallelism follows the window LENGTH, the host picks (window_count_abi.inc):
//   window <= kWindowCountPiece   window_count_k1 / _k2: a group of L lanes (a power of two, 1..64: the words a window can span
//                                 over kWindowCountLaneWords, rounded up) owns one window, lane l the words first + l,
//                                 first + l + L, ...; adjacent lanes read adjacent words.  The group's sums come from __shfl_xor
//                                 at the offsets below L, two counts to a dword, and its lane 0 stores the record with 16-B
//                                 stores.  Guarded 8-B loads: the groups of a workgroup start at any word and overlap, which
//                                 is not the shape of a tile.  Eight words a lane and not one: the shuffles and the window's
//                                 fixed cost, not the popcounts, are what a short window pays for (DESIGN.md "windowed counts":
//                                 1, 2, 4 and 8 words a lane measured, 8 the fastest in every row).
//   longer windows                window_count_piece_k1 / _k2: a window is cut into pieces of kWindowCountPiece nucleotides (one
//                                 tile of word_tile.hpp's shape: 256 lanes, a word and its neighbour per lane, word_tile_pair);
//                                 a workgroup counts a run of consecutive pieces of ONE window in registers, sums over its waves
//                                 and adds the 4^k sums to the record with 32-bit atomics.  window_count_zero, enqueued in front
//                                 of it by the same call, zeroes the records, so the call still SETS its output.  The run length
//                                 is the host's: as short as it takes to fill the chip, so that window == len is spread over all
//                                 of it while the adds to one record stay a few thousand.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"
#include "word_tile.hpp"

namespace cnt {

constexpr int kWindowCountMaxK = 2;
constexpr int kWindowCountBlock = 256;
constexpr int kWindowCountWaves = kWindowCountBlock / 64;
constexpr uint64_t kWindowCountTileWords = kWindowCountBlock, kWindowCountPiece = 32 * kWindowCountTileWords;  // 8192 nt
constexpr uint64_t kWindowCountLaneWords = 8;  // the words a lane of a group takes before the group grows (measured, see above)
constexpr uint64_t kPlane = 0x5555555555555555ull;

struct WindowCountArgs {
    const uint8_t* in;
    uint64_t words;                // ceil(len / 32)
    uint64_t window, step, n_win;  // n_win >= 1, (n_win - 1) * step + window <= len
    uint32_t* out;                 // n_win records of 4^k u32
    uint32_t lanes_log2;           // group kernels: log2 of the lanes that own a window
    uint64_t runs, run_words;      // piece kernels: workgroups per window, and the words each of them walks (whole pieces)
};

// codes_below on a plane: bit 2r set iff position i0 + r < x
__device__ __forceinline__ uint64_t plane_below(uint64_t i0, uint64_t x) {
    return x <= i0 ? 0ull : (x - i0 >= 32 ? kPlane : ((1ull << (2 * (uint32_t)(x - i0))) - 1ull) & kPlane);
}
// the positions of the word at i0 that lie in [s, e), on a plane
__device__ __forceinline__ uint64_t plane_between(uint64_t i0, uint64_t s, uint64_t e) { return plane_below(i0, e) & ~plane_below(i0, s); }

// c[v] += the k-mers with value v that start at the positions m (a plane mask) of the word x; `next` is the word behind x
template <int K>
__device__ __forceinline__ void window_count_word(uint64_t x, uint64_t next, uint64_t m, uint32_t* c) {
    const uint64_t l1 = x & m, h1 = (x >> 1) & m;
    if constexpr (K == 1) {
        const uint32_t g = __popcll(l1 & h1), pl = __popcll(l1), ph = __popcll(h1), total = __popcll(m);
        c[0] += total - pl - ph + g;
        c[1] += pl - g;
        c[2] += ph - g;
        c[3] += g;
    } else {
        const uint64_t y = funnel64(x, next, 2), l2 = y, h2 = y >> 1;  // the odd bits of l2, h2 fall to the first base's planes
        const uint64_t first[4] = {m & ~l1 & ~h1, l1 & ~h1, h1 & ~l1, l1 & h1};
        const uint64_t second[4] = {~l2 & ~h2, l2 & ~h2, h2 & ~l2, l2 & h2};
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int a = 0; a < 4; ++a) c[a | (b << 2)] += __popcll(first[a] & second[b]);
    }
}

// 16-B stores at the 8-B alignment a record has
typedef uint32_t window_count_u4 __attribute__((ext_vector_type(4), aligned(8)));

// Tile t = the kWindowCountBlock >> lanes_log2 windows from t * that on.  Every lane walks the shuffles: the lanes of a window at or
// past n_win have an empty word range, load nothing and store nothing.
template <int K>
__device__ __forceinline__ void window_count_group(const WindowCountArgs& a, uint64_t tile) {
    constexpr int B = K == 1 ? 4 : 16;
    const uint32_t lg = a.lanes_log2, L = 1u << lg, l = threadIdx.x & (L - 1u);
    const uint64_t j = tile * (kWindowCountBlock >> lg) + (threadIdx.x >> lg);
    const bool live = j < a.n_win;
    const uint64_t s = live ? j * a.step : 0, e = s + a.window, ek = e - (K - 1);  // k-mers start in [s, ek)
    const uint64_t last = live ? (ek - 1) >> 5 : 0, last_of_window = (e - 1) >> 5;
    const uint64_t* in64 = reinterpret_cast<const uint64_t*>(a.in);
    // a word behind `last` is not fetched and reads as 0; the neighbour is a word of the window too, or not fetched
    auto load = [&](uint64_t w, uint64_t& x, uint64_t& next) {
        x = live && w <= last ? in64[w] : 0;
        next = K == 2 && live && w < last_of_window ? in64[w + 1] : 0;
    };
    uint32_t c[B] = {};
    uint64_t w = (s >> 5) + l, x, next;
    load(w, x, next);
    while (live && w <= last) {
        const uint64_t wn = w + L, cx = x, cnext = next;
        if (wn <= last) load(wn, x, next);  // the next round's words travel while this one is counted
        window_count_word<K>(cx, cnext, plane_between(w * 32, s, ek), c);
        w = wn;
    }
    // a count is at most the window, below 2^16 here: two of them ride in one shuffle
    static_assert(kWindowCountPiece < (1u << 16), "two counts of a window share a dword on their way through the group");
    uint32_t pair[B / 2];
#pragma unroll
    for (int i = 0; i < B / 2; ++i) pair[i] = c[i] | (c[i + B / 2] << 16);
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1)
        if (o < L) {
#pragma unroll
            for (int i = 0; i < B / 2; ++i) pair[i] += __shfl_xor(pair[i], o, 64);
        }
#pragma unroll
    for (int i = 0; i < B / 2; ++i) {
        c[i] = pair[i] & 0xFFFFu;
        c[i + B / 2] = pair[i] >> 16;
    }
    if (live && l == 0) {
        window_count_u4* rec = reinterpret_cast<window_count_u4*>(a.out + j * B);
#pragma unroll
        for (int i = 0; i < B / 4; ++i) rec[i] = window_count_u4{c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]};
    }
}

// Tile t = run t % runs of window t / runs: the words [first + run * run_words, + run_words) of the window, clipped to its last
// word, tile by tile of kWindowCountTileWords.  word_tile_pair may read words of the input outside the window (never outside the
// input); the position mask drops them.  A run behind the window's last word (a window at a low phase spans fewer words than the
// host provided for) adds nothing.
template <int K>
__device__ __forceinline__ void window_count_piece(const WindowCountArgs& a, uint64_t tile, uint32_t (*s_sum)[16]) {
    constexpr int B = K == 1 ? 4 : 16;
    const uint32_t t = threadIdx.x;
    const uint64_t j = tile / a.runs, run = tile - j * a.runs;
    const uint64_t s = j * a.step, ek = s + a.window - (K - 1);
    const uint64_t begin = (s >> 5) + run * a.run_words, after_last = ((ek - 1) >> 5) + 1;
    const uint64_t end = begin + a.run_words < after_last ? begin + a.run_words : after_last;
    uint32_t c[B] = {};
    uint64_t w0 = begin, lo = 0, hi = 0;
    if (w0 < end) word_tile_pair<kWindowCountTileWords>(a.in, a.words, w0, t, lo, hi);
    while (w0 < end) {
        const uint64_t wn = w0 + kWindowCountTileWords, cur_lo = lo, cur_hi = hi;
        if (wn < end) word_tile_pair<kWindowCountTileWords>(a.in, a.words, wn, t, lo, hi);
        window_count_word<K>(cur_lo, cur_hi, plane_between((w0 + t) * 32, s, ek), c);
        w0 = wn;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
#pragma unroll
        for (int i = 0; i < B; ++i) c[i] += __shfl_xor(c[i], o, 64);
    if ((t & 63u) == 0)
#pragma unroll
        for (int i = 0; i < B; ++i) s_sum[t >> 6][i] = c[i];
    __syncthreads();
    if (t < (uint32_t)B) {
        uint32_t sum = 0;
#pragma unroll
        for (int q = 0; q < kWindowCountWaves; ++q) sum += s_sum[q][t];
        // system scope: with a pinned caller buffer the record is host memory, and an add is an atomic a PCIe link carries
        if (sum) atomicAdd_system(a.out + j * B + t, sum);
    }
}

// Plain kernels over the templated bodies: the product code object keeps its count of templated kernels.
__global__ __launch_bounds__(kWindowCountBlock) void window_count_k1(WindowCountArgs a, uint64_t tile0) { window_count_group<1>(a, tile0 + blockIdx.x); }
__global__ __launch_bounds__(kWindowCountBlock) void window_count_k2(WindowCountArgs a, uint64_t tile0) { window_count_group<2>(a, tile0 + blockIdx.x); }
__global__ __launch_bounds__(kWindowCountBlock) void window_count_piece_k1(WindowCountArgs a, uint64_t tile0) {
    __shared__ uint32_t s_sum[kWindowCountWaves][16];
    window_count_piece<1>(a, tile0 + blockIdx.x, s_sum);
}
__global__ __launch_bounds__(kWindowCountBlock) void window_count_piece_k2(WindowCountArgs a, uint64_t tile0) {
    __shared__ uint32_t s_sum[kWindowCountWaves][16];
    window_count_piece<2>(a, tile0 + blockIdx.x, s_sum);
}
// the first n_words 8-B words of the records (a record is 16 or 64 B) = 0; one word per lane
__global__ __launch_bounds__(kWindowCountBlock) void window_count_zero(uint64_t* __restrict__ out, uint64_t n_words, uint64_t tile0) {
    const uint64_t i = (tile0 + blockIdx.x) * kWindowCountBlock + threadIdx.x;
    if (i < n_words) out[i] = 0;
}

}  // namespace cnt
