// kmer_count_kernels.hpp -- k-mer counting on 2-bit packed words (include/cute_nt.h, "k-mer counts"): the histogram over 4^k
// bins of the values cnt_kmers would write, 1 <= k <= 12, forward or canonical.  Not in the reference; the definition is
// restated by tests/test_kmer_counts.py as a bincount of the scalar oracle's k-mers.
//
// Traffic: 0.25 B read per k-mer and nothing streamed out -- the work is on-chip adds, not memory.  One kernel body, two
// regimes (template argument, so that the product object gains two kernels and no more):
//   kmer_count<true>   k <= kKmerCountLdsMaxK: a private table of 32-bit counters in 64 KiB of LDS (two workgroups per CU),
//                      flushed once at the end into the caller's u64 table with 64-bit global atomics;
//   kmer_count<false>  larger k: 64-bit global atomics straight into the caller's table.
// Shape of both: persistent workgroups of 1024 lanes stride over tiles of 1024 input words.  Lane j of a tile owns the 32
// k-mers that START in word j of the tile: it reads that word and the next (word_tile.hpp: word_tile_pair) and walks the 32
// windows with constant funnel shifts.  k <= 12 means 2k <= 24 bits, so a window is the
// low dword of the 64-bit funnel and the canonical form is a 32-bit bit reverse.
//
// The two hazards of a histogram:
//   few bins (k <= 5)   64 lanes over 4 .. 1024 bins would serialise on equal LDS addresses.  The 16384 counters hold
//                       R = min(256, 16384 / 4^k) replicas of the table, counter of bin v in replica r at v*R + r, and a lane
//                       uses replica lane % R: for R >= 32 the 32 lanes of an LDS lane group sit on 32 different banks whatever
//                       their k-mers are.  The flush sums the replicas.
//   skewed data         a lane's 32 k-mers are CONSECUTIVE, so a homopolymer run is a run of equal values inside the lane: the
//                       lane folds equal neighbours and adds a run as one add of its length.  All-A input costs one add per
//                       lane and tile instead of 32.  Short-period repeats (ACACAC...) have no equal neighbours and still send
//                       every lane to the same few bins: correct, but the adds serialise (include/cute_nt.h quotes the cost).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"
#include "word_tile.hpp"

namespace cnt {

constexpr int kKmerCountMaxK = 12;
constexpr int kKmerCountLdsMaxK = 7;  // measured split (DESIGN.md "k-mer counts"): the LDS table still wins at k = 7
constexpr int kKmerCountBlock = 1024;  // 16 waves: two workgroups fill a CU's 8 waves per SIMD
constexpr uint32_t kKmerCountSlots = 16384;  // 32-bit LDS counters per workgroup: 64 KiB
constexpr uint32_t kKmerCountMaxReplicas = 256;
constexpr uint64_t kKmerCountTileWords = kKmerCountBlock, kKmerCountTileKmers = 32 * kKmerCountTileWords;
// A 32-bit LDS counter holds at most the k-mers its workgroup sees before the flush.  The launcher gives a workgroup at most
// this many tiles (it widens the grid beyond the persistent size when len asks for it), so no counter can wrap.
constexpr uint64_t kKmerCountMaxTilesPerGroup = (1ull << 17) - 1;
static_assert(kKmerCountMaxTilesPerGroup * kKmerCountTileKmers < (1ull << 32), "an LDS counter would wrap before its flush");
static_assert((1u << (2 * kKmerCountLdsMaxK)) <= kKmerCountSlots && kKmerCountSlots * 4 <= 65536, "the LDS table is at most 64 KiB");

// log2 of the replica count R of the LDS table for this k
__host__ __device__ constexpr uint32_t kmer_count_replica_log2(uint32_t k) {
    uint32_t r = 0;
    while ((2u << r) <= kKmerCountMaxReplicas && ((uint64_t)(2u << r) << (2 * k)) <= kKmerCountSlots) ++r;
    return r;
}

// kmer_finish for k <= 12 in 32 bits: `fwd` holds k codes in its low 2k bits, zero above
template <bool CANONICAL>
__device__ __forceinline__ uint32_t kmer_count_finish(uint32_t fwd, uint32_t k) {
    if constexpr (CANONICAL) {
        const uint32_t rc = reverse_codes32(fwd ^ 0xAAAAAAAAu) >> (32 - 2 * k);
        return rc < fwd ? rc : fwd;
    } else {
        return fwd;
    }
}

template <bool LDS>
__device__ __forceinline__ void kmer_count_add(uint32_t* table, unsigned long long* counts, uint32_t v, uint32_t run, uint32_t rlog, uint32_t rep) {
    if constexpr (LDS) atomicAdd(&table[(v << rlog) + rep], run);
    else atomicAdd(&counts[v], (unsigned long long)run);
}

// one lane's k-mers: the first nv (FULL: all 32) windows that start in word `lo`, `hi` the word behind it; equal neighbours
// are folded into one add
template <bool LDS, bool CANONICAL, bool FULL>
__device__ __forceinline__ void kmer_count_lane(uint64_t lo, uint64_t hi, uint32_t nv, uint32_t k, uint32_t mask, uint32_t* table,
                                                unsigned long long* counts, uint32_t rlog, uint32_t rep) {
    uint32_t prev = 0, run = 0;
#pragma unroll
    for (uint32_t r = 0; r < 32; ++r) {
        if (FULL || r < nv) {
            const uint32_t win = r == 0 ? (uint32_t)lo : (uint32_t)((lo >> (2 * r)) | (hi << (64 - 2 * r)));
            const uint32_t v = kmer_count_finish<CANONICAL>(win & mask, k);
            if (run != 0 && v != prev) {
                kmer_count_add<LDS>(table, counts, prev, run, rlog, rep);
                run = 0;
            }
            prev = v;
            ++run;
        }
    }
    if (run != 0) kmer_count_add<LDS>(table, counts, prev, run, rlog, rep);
}

// counts[v] += #{ i < m : k-mer i == v }.  Tile t = input words [1024 t, 1024 t + 1024) = k-mers [32768 t, 32768 t + 32768);
// workgroup b takes tiles b, b + gridDim.x, ...  `words` = ceil(len / 32): a tile whose 1025 words all exist takes the 16-B
// loads, the others (the last one or two) read word by word, each read guarded.  Bits beyond len are never part of a counted
// window: k-mer i < m uses codes i .. i+k-1 <= len-1.
template <bool LDS>
__global__ __launch_bounds__(kKmerCountBlock) void kmer_count(const uint8_t* __restrict__ in, uint64_t words, uint64_t m, uint32_t k, uint32_t canonical,
                                                             uint64_t n_tiles, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t table[LDS ? kKmerCountSlots : 1];
    const uint32_t j = threadIdx.x, rlog = kmer_count_replica_log2(k), rep = j & ((1u << rlog) - 1u);
    const uint32_t mask = (1u << (2 * k)) - 1u;
    if constexpr (LDS) {
        for (uint32_t i = j; i < kKmerCountSlots; i += kKmerCountBlock) table[i] = 0;
        __syncthreads();
    }
    auto load = [&](uint64_t t, uint64_t& lo, uint64_t& hi) { word_tile_pair<kKmerCountTileWords>(in, words, t * kKmerCountTileWords, j, lo, hi); };
    uint64_t t = blockIdx.x, lo = 0, hi = 0;
    if (t < n_tiles) load(t, lo, hi);
    while (t < n_tiles) {
        const uint64_t tn = t + gridDim.x, cur_lo = lo, cur_hi = hi;
        if (tn < n_tiles) load(tn, lo, hi);  // the next tile's words travel while this one is counted
        const uint64_t i0 = (t * kKmerCountTileWords + j) * 32;
        if ((t + 1) * kKmerCountTileKmers <= m) {
            if (canonical) kmer_count_lane<LDS, true, true>(cur_lo, cur_hi, 32, k, mask, table, counts, rlog, rep);
            else kmer_count_lane<LDS, false, true>(cur_lo, cur_hi, 32, k, mask, table, counts, rlog, rep);
        } else {
            const uint32_t nv = i0 >= m ? 0u : (uint32_t)(m - i0 < 32 ? m - i0 : 32);
            if (canonical) kmer_count_lane<LDS, true, false>(cur_lo, cur_hi, nv, k, mask, table, counts, rlog, rep);
            else kmer_count_lane<LDS, false, false>(cur_lo, cur_hi, nv, k, mask, table, counts, rlog, rep);
        }
        t = tn;
    }
    if constexpr (LDS) {
        // flush: bin by bin the sum of its replicas, non-zero sums added to the caller's table.  Each workgroup starts at
        // another bin, so the workgroups that finish together do not all add to the same line; a lane starts at another
        // replica, so the lanes of a wave read different banks.
        __syncthreads();
        const uint32_t bins = 1u << (2 * k), reps = 1u << rlog;
        for (uint32_t b0 = j; b0 < bins; b0 += kKmerCountBlock) {
            const uint32_t b = (b0 + blockIdx.x * 64u) & (bins - 1u);
            uint64_t sum = 0;
            for (uint32_t r = 0; r < reps; ++r) sum += table[(b << rlog) + ((r + j) & (reps - 1u))];
            if (sum) atomicAdd(&counts[b], (unsigned long long)sum);
        }
    }
}

}  // namespace cnt
