// orf_kernels.hpp -- open-reading-frame scan on 2-bit packed words (include/cute_nt.h, "ORF scan"): the stop-free runs of the
// three frame lanes of one strand or of both, each trimmed to its start codon when a start set is given.  Not in the reference;
// the definition is restated per position by tests/test_orfs.py.
//
// An entry is emitted by the bound `hi` that closes its run: a stop codon of its lane and strand, or the end of the sequence.
// What the emitter needs -- the previous stop of its lane `lo`, and the start behind it -- can lie any number of tiles back, so
// it is carried by a scan and never walked to.  The carried value of a (strand, lane) pair over a range of positions is
//     stop   the last stop of the pair in the range, or none
//     start  the start that an ORF opening behind `stop` (behind the range's beginning when there is none) would take: on the
//            forward strand the FIRST start of the pair behind `stop`, on the reverse strand the LAST one; or none
// and two neighbouring ranges A, B combine to  B  when B holds a stop, else to  (A.stop, forward: A.start else B.start; reverse:
// B.start else A.start).  The operator is associative with (none, none) as its identity; it is applied inside a lane's word,
// across the 64 lanes of a wave (shuffles), across the four waves of a tile (LDS) and across tiles (orf_carry).  Inside a tile
// a pair's value is one dword, stop + 1 - tile0 in the high half and start + 1 - tile0 in the low one, 0 = none.
//
// Passes (orf_abi.inc), none of which allocates; counts / offs and passes 3 to 5 are the counted output of counted_output.hpp:
//   1. orf_summary   one workgroup per tile of kOrfTile positions: sums[pair][tile] = the tile's value of each pair;
//   2. orf_carry     one workgroup per pair turns the tiles' values into carry[pair][tile], the value of everything in front of
//                    the tile, in sequence coordinates (u64, ~0 = none);
//   3. orf_count     counts[tile] = the entries the tile's bounds emit;
//   4. counted_scan
//   5. orf_write     a tile whose count is 0 returns at once; the others repeat pass 3 and store their entries in order.
// Shape of a tile, as in word_tile.hpp: lane j owns the 32 positions that start in word j of the tile; it reads that word and
// the next (word_tile_pair: two look-ahead nucleotides).  The four sets (stops and starts of either strand, the reverse ones already composed
// with the codon's reverse complement) are staged as a 64-entry table in LDS, one byte lane per set: eight look-ups shifted into
// one accumulator give eight positions of all four masks.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"
#include "counted_output.hpp"
#include "find_kernels.hpp"

namespace cnt {

constexpr int kOrfBlock = 256;
constexpr int kOrfWaves = kOrfBlock / 64;
constexpr uint64_t kOrfTileWords = kOrfBlock, kOrfTile = 32 * kOrfTileWords;  // positions per tile: 8192
constexpr int kOrfCarryBlock = 1024;                                           // orf_carry: one tile per lane and round
constexpr int kOrfPairs = 6;                                                   // pair = 3 * strand + lane
constexpr uint32_t kOrfOpenEnd = 0x400u, kOrfNoStop = 0x800u;                 // CNT_ORF_* (asserted equal in orf_abi.inc)
constexpr uint64_t kOrfNone = ~0ull;
static_assert(kOrfTile + 1 < (1u << 16), "a position of a tile, plus one, is half a dword");

struct OrfArgs {
    const uint8_t* in;
    uint64_t words, len;      // ceil(len / 32); len >= 3
    uint64_t stops[2], starts[2];  // [1]: the reverse strand's, composed with rc3; stops[1] = 0: forward strand only
    uint64_t min_len;         // >= 3
    uint64_t n_tiles;         // len / kOrfTile + 1: the positions 0 .. len
    uint32_t* sums;           // [kOrfPairs][n_tiles]
    uint64_t* carry;          // [kOrfPairs][2][n_tiles]: stop, start
    uint32_t* counts;
    uint64_t* offs;
    uint64_t *pos, *length, *info;
    uint64_t out_cap;
};

// A then B, inside a tile
__device__ __forceinline__ uint32_t orf_combine(uint32_t a, uint32_t b, bool rev) {
    const uint32_t sa = a & 0xFFFFu, sb = b & 0xFFFFu;
    const uint32_t st = rev ? (sb ? sb : sa) : (sa ? sa : sb);
    return (b >> 16) ? b : ((a & 0xFFFF0000u) | st);
}

// What a lane knows of its 32 positions: bit r of stops[s] / starts[s] = position i0 + r is a stop / a start of strand s.  The
// three positions len-2 .. len are stops of every strand scanned: they close the top runs.
struct OrfLane {
    uint64_t i0;
    uint32_t stops[2], starts[2];
    uint32_t m3;  // i0 % 3
};

// stages the table (the caller synchronises) and builds the lane's masks
__device__ __forceinline__ OrfLane orf_lane(const OrfArgs& a, uint64_t tile, uint32_t* s_tab) {
    const uint32_t j = threadIdx.x;
    if (j < 64) {
        s_tab[j] = (uint32_t)((a.stops[0] >> j) & 1u) | ((uint32_t)((a.starts[0] >> j) & 1u) << 8) | ((uint32_t)((a.stops[1] >> j) & 1u) << 16) |
                   ((uint32_t)((a.starts[1] >> j) & 1u) << 24);
    }
    const uint64_t w0 = tile * kOrfTileWords;
    uint64_t lo, hi;
    word_tile_pair<kOrfTileWords>(a.in, a.words, w0, j, lo, hi);
    __syncthreads();
    const uint32_t d[3] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi};
    uint32_t acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        acc[g] = 0;
#pragma unroll
        for (int r = 8 * g + 7; r >= 8 * g; --r)  // downward: position r of the group ends in bit r of each byte
            acc[g] = (acc[g] << 1) | s_tab[window_dword(d, r) & 63u];
    }
    OrfLane L;
    L.i0 = (w0 + j) * 32;
    L.m3 = (2u * (uint32_t)(tile % 3) + 2u * j) % 3u;  // 8192 = 32 = 2 (mod 3)
    const uint32_t valid = codes_below(L.i0, a.len - 2), ends = codes_below(L.i0, a.len + 1) & ~valid;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int b = 16 * s;
        const uint32_t st = ((acc[0] >> b) & 0xFFu) | (((acc[1] >> b) & 0xFFu) << 8) | (((acc[2] >> b) & 0xFFu) << 16) | (((acc[3] >> b) & 0xFFu) << 24);
        const uint32_t sa = ((acc[0] >> (b + 8)) & 0xFFu) | (((acc[1] >> (b + 8)) & 0xFFu) << 8) | (((acc[2] >> (b + 8)) & 0xFFu) << 16) |
                            (((acc[3] >> (b + 8)) & 0xFFu) << 24);
        L.stops[s] = (st & valid) | ((s == 0 || a.stops[1]) ? ends : 0u);
        L.starts[s] = sa & valid;
    }
    return L;
}

// The value of each pair over the lane's 32 positions, then the inclusive scan of it over the wave; x[p] of lane 63 is the wave's.
__device__ __forceinline__ void orf_wave_scan(const OrfLane& L, bool both, uint32_t (&x)[kOrfPairs]) {
    const uint32_t rel = threadIdx.x * 32u + 1u, lane = threadIdx.x & 63u;
#pragma unroll
    for (int p = 0; p < kOrfPairs; ++p) {
        const int s = p / 3;
        const uint32_t mask = 0x49249249u << ((p % 3 + 3u - L.m3) % 3u);  // the positions of lane p % 3
        const uint32_t st = L.stops[s] & mask;
        const uint32_t top = st ? 31u - (uint32_t)__builtin_clz(st) : 0u;
        const uint32_t sa = L.starts[s] & mask & (st ? ~((2u << top) - 1u) : ~0u);
        const uint32_t at = s ? 31u - (uint32_t)__builtin_clz(sa | 1u) : (uint32_t)__builtin_ctz(sa | 0x80000000u);
        x[p] = (st ? (rel + top) << 16 : 0u) | (sa ? rel + at : 0u);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int p = 0; p < kOrfPairs; ++p) {
            if (p >= 3 && !both) continue;
            const uint32_t y = __shfl_up(x[p], o, 64);
            if (lane >= (uint32_t)o) x[p] = orf_combine(y, x[p], p >= 3);
        }
    }
}

// pass 1
__global__ __launch_bounds__(kOrfBlock) void orf_summary(OrfArgs a, uint64_t first_tile) {
    __shared__ uint32_t s_tab[64];
    __shared__ uint32_t s_w[kOrfWaves][kOrfPairs];
    const uint64_t tile = first_tile + blockIdx.x;
    const bool both = a.stops[1] != 0;
    const OrfLane L = orf_lane(a, tile, s_tab);
    uint32_t x[kOrfPairs];
    orf_wave_scan(L, both, x);
    if ((threadIdx.x & 63u) == 63u) {
#pragma unroll
        for (int p = 0; p < kOrfPairs; ++p) s_w[threadIdx.x >> 6][p] = x[p];
    }
    __syncthreads();
    if (threadIdx.x < (both ? kOrfPairs : 3)) {
        const uint32_t p = threadIdx.x;
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < kOrfWaves; ++q) v = orf_combine(v, s_w[q][p], p >= 3);
        a.sums[p * a.n_tiles + tile] = v;
    }
}

// A then B, in sequence coordinates
__device__ __forceinline__ void orf_combine64(uint64_t& stop, uint64_t& start, uint64_t b_stop, uint64_t b_start, bool rev) {
    if (b_stop != kOrfNone) {
        stop = b_stop;
        start = b_start;
    } else if (rev ? b_start != kOrfNone : start == kOrfNone) {
        start = b_start;
    }
}

// pass 2: workgroup p scans pair p, kOrfCarryBlock tiles a round
__global__ __launch_bounds__(kOrfCarryBlock) void orf_carry(const uint32_t* __restrict__ sums, uint64_t* __restrict__ carry, uint64_t n_tiles) {
    __shared__ uint64_t s_w[kOrfCarryBlock / 64][2];
    const uint32_t p = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool rev = p >= 3;
    const uint32_t* in = sums + p * n_tiles;
    uint64_t* out_stop = carry + 2ull * p * n_tiles;
    uint64_t* out_start = out_stop + n_tiles;
    uint64_t c_stop = kOrfNone, c_start = kOrfNone;  // everything in front of the round
    for (uint64_t first = 0; first < n_tiles; first += kOrfCarryBlock) {
        const uint64_t t = first + threadIdx.x;
        const uint32_t v = t < n_tiles ? in[t] : 0u;
        const uint64_t own_stop = (v >> 16) ? t * kOrfTile + (v >> 16) - 1 : kOrfNone, own_start = (v & 0xFFFFu) ? t * kOrfTile + (v & 0xFFFFu) - 1 : kOrfNone;
        uint64_t stop = own_stop, start = own_start;  // inclusive over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            uint64_t y_stop = shfl_up_u64(stop, o), y_start = shfl_up_u64(start, o);
            if (lane >= (uint32_t)o) {
                orf_combine64(y_stop, y_start, stop, start, rev);
                stop = y_stop;
                start = y_start;
            }
        }
        if (lane == 63) {
            s_w[wave][0] = stop;
            s_w[wave][1] = start;
        }
        uint64_t e_stop = shfl_up_u64(stop, 1), e_start = shfl_up_u64(start, 1);  // exclusive
        if (lane == 0) e_stop = e_start = kOrfNone;
        __syncthreads();
        uint64_t b_stop = c_stop, b_start = c_start;  // everything in front of the wave
#pragma unroll
        for (int q = 0; q < kOrfCarryBlock / 64; ++q) {
            if (q == (int)wave) {
                uint64_t f_stop = b_stop, f_start = b_start;
                orf_combine64(f_stop, f_start, e_stop, e_start, rev);
                if (t < n_tiles) {
                    out_stop[t] = f_stop;
                    out_start[t] = f_start;
                }
            }
            orf_combine64(b_stop, b_start, s_w[q][0], s_w[q][1], rev);
        }
        c_stop = b_stop;
        c_start = b_start;
        __syncthreads();  // s_w is rewritten by the next round
    }
}

// passes 3 and 5.  WRITE = false: counts[tile] = the tile's entries.  WRITE = true: the scan's offs[] and the counts place them.
template <bool WRITE>
__device__ __forceinline__ void orf_tile(const OrfArgs& a, uint64_t first_tile) {
    __shared__ uint32_t s_tab[64];
    __shared__ uint32_t s_w[kOrfWaves][kOrfPairs];
    __shared__ uint64_t s_carry[kOrfPairs][2];
    __shared__ uint32_t s_cnt[kOrfWaves];
    __shared__ uint64_t s_base;
    const uint64_t tile = first_tile + blockIdx.x;
    const uint32_t j = threadIdx.x, lane = j & 63u, wave = j >> 6;
    const bool both = a.stops[1] != 0, have_starts = (a.starts[0] | a.starts[1]) != 0;
    if constexpr (WRITE) {
        if (a.counts[tile] == 0) return;
    }
    if (j < 2 * kOrfPairs) s_carry[j >> 1][j & 1] = (both || j < 6) ? a.carry[j * a.n_tiles + tile] : kOrfNone;
    const OrfLane L = orf_lane(a, tile, s_tab);
    uint32_t x[kOrfPairs];
    orf_wave_scan(L, both, x);
    if (lane == 63) {
#pragma unroll
        for (int p = 0; p < kOrfPairs; ++p) s_w[wave][p] = x[p];
    }
    __syncthreads();
    uint32_t before[kOrfPairs];  // the tile's positions in front of the lane
#pragma unroll
    for (int p = 0; p < kOrfPairs; ++p) {
        uint32_t e = __shfl_up(x[p], 1, 64), v = 0;
        if (lane == 0) e = 0;
#pragma unroll
        for (int q = 0; q < kOrfWaves - 1; ++q) v = q < (int)wave ? orf_combine(v, s_w[q][p], p >= 3) : v;
        before[p] = orf_combine(v, e, p >= 3);
    }
    const uint64_t tile0 = tile * kOrfTile, m = a.len - 2;
    const uint32_t len3 = (uint32_t)(a.len % 3);

    // the entry that bound r of strand s emits, if any
    uint64_t e_pos, e_len, e_info;
    auto entry = [&](int s, uint32_t r) -> bool {
        const uint32_t k = r % 3u, q = (L.m3 + k) % 3u;
        const uint32_t mask = (0x49249249u << k) & ((1u << r) - 1u);  // the positions of the bound's lane in front of it
        const uint32_t st = L.stops[s] & mask;
        const uint64_t hi = L.i0 + r;
        uint64_t lo, at;
        bool lo_end = false;
        if (st) {  // the run opens inside the lane's word
            const uint32_t top = 31u - (uint32_t)__builtin_clz(st);
            const uint32_t sa = L.starts[s] & mask & ~((2u << top) - 1u);
            lo = L.i0 + top;
            at = !sa ? kOrfNone : L.i0 + (s ? 31u - (uint32_t)__builtin_clz(sa) : (uint32_t)__builtin_ctz(sa));
        } else {
            const uint32_t sa = L.starts[s] & mask;
            const uint32_t b = q == 0 ? before[3 * s] : q == 1 ? before[3 * s + 1] : before[3 * s + 2];
            uint64_t stop = s_carry[3 * s + q][0], start = s_carry[3 * s + q][1];
            orf_combine64(stop, start, (b >> 16) ? tile0 + (b >> 16) - 1 : kOrfNone, (b & 0xFFFFu) ? tile0 + (b & 0xFFFFu) - 1 : kOrfNone, s != 0);
            orf_combine64(stop, start, kOrfNone, !sa ? kOrfNone : L.i0 + (s ? 31u - (uint32_t)__builtin_clz(sa) : (uint32_t)__builtin_ctz(sa)), s != 0);
            lo_end = stop == kOrfNone;
            lo = lo_end ? (uint64_t)q - 3 : stop;  // lane - 3, mod 2^64: lo + 3 is the lane
            at = start;
        }
        if (have_starts && at == kOrfNone) return false;
        e_pos = have_starts && !s ? at : lo + 3;
        e_len = !have_starts ? hi - lo - 3 : s ? at - lo : hi - at;
        const bool hi_end = hi >= m;
        e_info = s ? ((len3 + 3u - q) % 3u) | kFindReverse | (hi_end ? kOrfOpenEnd : 0u) | (lo_end ? kOrfNoStop : 0u)
                   : q | (lo_end ? kOrfOpenEnd : 0u) | (hi_end ? kOrfNoStop : 0u);
        return e_len >= a.min_len;
    };

    uint32_t fm = 0, rm = 0;  // bit r: bound r emits an entry
    for (uint32_t any = L.stops[0]; any; any &= any - 1) {
        const uint32_t r = (uint32_t)__builtin_ctz(any);
        fm |= entry(0, r) ? 1u << r : 0u;
    }
    if (both) {
        for (uint32_t any = L.stops[1]; any; any &= any - 1) {
            const uint32_t r = (uint32_t)__builtin_ctz(any);
            rm |= entry(1, r) ? 1u << r : 0u;
        }
    }
    const uint32_t c = (uint32_t)__popc(fm) + (uint32_t)__popc(rm);
    const uint32_t n = tile_rank_post(c, s_cnt);  // lane order = position order
    if constexpr (WRITE) {
        if (j == 0) s_base = counted_tile_base(a.offs, a.counts, tile);
    }
    __syncthreads();
    if constexpr (!WRITE) {
        if (j == 0) a.counts[tile] = tile_total<kOrfWaves>(s_cnt);
    } else {
        uint64_t at = s_base + tile_before<kOrfWaves>(s_cnt, n - c);
        // the lane's entries by their bound, forward before reverse; recomputed for the few bounds that emit
        for (uint32_t any = fm | rm; any; any &= any - 1) {
            const uint32_t r = (uint32_t)__builtin_ctz(any);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (!(((s ? rm : fm) >> r) & 1u)) continue;
                if (at < a.out_cap) {
                    entry(s, r);
                    __builtin_nontemporal_store(e_pos, a.pos + at);
                    __builtin_nontemporal_store(e_len, a.length + at);
                    if (a.info) __builtin_nontemporal_store(e_info, a.info + at);
                }
                ++at;
            }
        }
    }
}

__global__ __launch_bounds__(kOrfBlock) void orf_count(OrfArgs a, uint64_t first_tile) { orf_tile<false>(a, first_tile); }
__global__ __launch_bounds__(kOrfBlock) void orf_write(OrfArgs a, uint64_t first_tile) { orf_tile<true>(a, first_tile); }

}  // namespace cnt
