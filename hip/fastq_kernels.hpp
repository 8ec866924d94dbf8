// fastq_kernels.hpp -- FASTQ text straight to 2-bit packed words, with the quality bytes and a record table (include/cute_nt.h,
// "text formats: FASTQ").  Not in the reference; the definition is restated three ways by tests/test_fastq.py.
//
// For the bytes t_0 .. t_{L-1}: the LINE NUMBER of byte p is k(p) = #{ q < p : t_q == 0x0A } (a line feed belongs to the line it
// ends) and its ROLE is k(p) mod 4: 0 name, 1 sequence, 2 separator, 3 quality -- strict four-line FASTQ, nothing is inferred from
// '@' or '+'.  0x0A and 0x0D are dropped in every role; the other role-1 bytes are encoded as cnt_n_to_bits_ex encodes them, the
// other role-3 bytes are copied to `qual` as they are; the line starts of role 0 are the records: their byte offset and the number
// of sequence and of quality bytes in front of them.
//
// Tiles and lanes are fasta_kernels.hpp's: kFastaTile bytes of the 16-B ALIGNED address space the text lies in, lane j owns the 32
// bytes [32 j, 32 j + 32) of its tile; a lane whose 32 bytes do not all lie inside the text reads byte by byte under guards.  What
// a lane needs from the bytes in front of it is its incoming PHASE, the line number mod 4 of its first byte: the tile's carry plus
// the line feeds of the lanes in front of it (word_tile.hpp's tile rank).  From the phase and the lane's line-feed mask the two
// bits of every byte's line number follow by two prefix XORs (fastq_roles).  Passes (fastq_abi.inc), none of which allocates:
//   1. fastq_lines      one workgroup per tile: lines[tile] = the tile's number of line feeds;
//   2. fastq_line_scan  ONE workgroup, a group of kCountedGroup tiles per lane and round: carry[tile] = the line number mod 4 at
//                       the tile's first byte -- through tiles without any line feed, and across its own rounds;
//   3. fastq_count      with the carry, one workgroup per tile: counts[tile] = its sequence bytes, qual_counts[tile] = its quality
//                       bytes, rec_counts[tile] = its records, flaws[tile] = its invalid sequence bytes and malformed line starts;
//   4. fastq_scan       ONE workgroup: offs[group] of the three streams as counted_scan would write them, and the five totals --
//                       no atomic anywhere;
//   5. hpc_zero_edges   (hpc_kernels.hpp, as it stands) zeroes the at most two words of `out` a tile shares with others;
//   6. fastq_write      a tile with nothing to write returns at once; the others repeat pass 3's masks, encode their 32 bytes to
//                       a word, compress it to the sequence codes (hpc_compress), OR the fragments into the tile's 257 output
//                       words in LDS and store those coalesced, the shared ones through hpc_merge; the quality bytes are staged
//                       in LDS as bytes, at the 16-B phase of their place in `qual`, and stored in aligned 16-B pieces with the
//                       ragged ends by bytes -- tiles write disjoint byte ranges, nothing is merged; a lane that holds records
//                       stores their three table entries itself.
// Codes at or past out_cap, quality bytes at or past qual_cap and records at or past rec_cap are clipped; the counts are not.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fasta_kernels.hpp"

namespace cnt {

constexpr int kFastqScanBlock = 1024;  // fastq_line_scan, fastq_scan: one group of tiles per lane and round
constexpr uint32_t kFastqQualLds = (uint32_t)kFastaTile + 32;  // a tile's quality bytes behind a stage of up to 15, in whole 16 B
static_assert(kFastaTile < (1u << 16), "a tile's counts are 16-bit fields");

struct FastqArgs {
    const uint8_t* base;  // text - phase: 16-B aligned
    uint32_t phase;       // 0..15: where the text begins in tile 0
    uint64_t len;         // bytes of text, >= 1
    uint64_t n_tiles;     // ceil((phase + len) / kFastaTile)
    uint32_t* lines;      // [n_tiles] pass 1 -> pass 2
    uint8_t* carry;       // [n_tiles] pass 2 -> passes 3 and 6
    uint32_t* flaws;      // [n_tiles] pass 3 -> pass 4: invalid | malformed << 16
    uint32_t *counts, *qual_counts, *rec_counts;  // counted_output.hpp's two regions, once per stream
    uint64_t *offs, *qual_offs, *rec_offs;
    uint64_t* out;
    uint8_t* qual;                                     // may be NULL
    uint64_t *rec_text, *rec_start, *rec_qual;         // all three or none
    uint64_t out_cap, qual_cap, rec_cap;               // codes, bytes, records
    uint64_t* totals;                                  // the caller's five counts
};

// What a lane knows of its 32 bytes; bit i = byte i.  Bytes outside the text read as 0 and have no bit anywhere.
struct FastqLane {
    u32x4 q[2];      // the bytes
    int64_t s;       // position in the text of byte 0 (negative in front of it)
    uint32_t valid;  // inside the text
    uint32_t nl;     // 0x0A
    uint32_t drop;   // 0x0A or 0x0D
    uint32_t ls;     // line starts
    uint32_t at;     // '@'
    uint32_t plus;   // '+'
    uint32_t bad;    // outside the alphabet of cnt_validate
};

template <bool ALLOW_N>
__device__ __forceinline__ FastqLane fastq_lane(const FastqArgs& a, uint64_t tile) {
    FastqLane l;
    const uint32_t j = threadIdx.x;
    const uint64_t at = tile * kFastaTile + j * kFastaLaneBytes;  // in the aligned space
    l.s = (int64_t)at - (int64_t)a.phase;
    const int64_t len = (int64_t)a.len;
    if (l.s >= 0 && l.s + 32 <= len) {
        const u32x4* p = reinterpret_cast<const u32x4*>(a.base + at);
        l.q[0] = p[0];
        l.q[1] = p[1];
        l.valid = ~0u;
    } else {
        uint32_t d[8] = {};
        l.valid = 0;
        for (int i = 0; i < 32; ++i) {
            const int64_t p = l.s + i;
            if (p >= 0 && p < len) {
                d[i >> 2] |= (uint32_t)a.base[at + i] << (8 * (i & 3));
                l.valid |= 1u << i;
            }
        }
        l.q[0] = u32x4{d[0], d[1], d[2], d[3]};
        l.q[1] = u32x4{d[4], d[5], d[6], d[7]};
    }
    uint32_t cr = 0;
    l.nl = l.at = l.plus = l.bad = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t x = l.q[h][e], sh = 16 * h + 4 * e;
            l.nl |= fasta_gather4(fasta_eq4(x, 0x0A0A0A0Au)) << sh;
            cr |= fasta_gather4(fasta_eq4(x, 0x0D0D0D0Du)) << sh;
            l.at |= fasta_gather4(fasta_eq4(x, 0x40404040u)) << sh;
            l.plus |= fasta_gather4(fasta_eq4(x, 0x2B2B2B2Bu)) << sh;
            l.bad |= fasta_gather4(invalid_mask<ALLOW_N>(x)) << sh;
        }
    // byte 0 is a line start when the byte in front of it is a line feed: the neighbour lane's bit 31, or for the first lane of
    // a wave one guarded byte read; position 0 of the text is one whatever lies in front of it
    uint32_t prev = __shfl_up(l.nl >> 31, 1, 64);
    if ((j & 63u) == 0) prev = (l.s >= 1 && l.s <= len) ? (uint32_t)(a.base[at - 1] == 0x0A) : 0u;
    if (l.s <= 0) prev = 0;
    l.ls = (l.nl << 1) | prev;
    if (l.s <= 0 && l.s > -32) l.ls |= 1u << (uint32_t)(-l.s);
    l.ls &= l.valid;
    l.drop = l.nl | cr;
    l.bad &= l.valid;
    return l;
}

// bit i = the XOR of the bits 0 .. i of m
__device__ __forceinline__ uint32_t fastq_pxor(uint32_t m) {
    m ^= m << 1;
    m ^= m << 2;
    m ^= m << 4;
    m ^= m << 8;
    return m ^ (m << 16);
}

// The two bits of every byte's line number, from the lane's line feeds and the line number `phi` (mod 4) of its byte 0.  The low
// bit flips behind every line feed; the high bit flips behind the line feeds that end an odd line.
struct FastqRoles {
    uint32_t seq, qual;  // role 1, role 3
    uint32_t rec, sep;   // role 0, role 2
};
__device__ __forceinline__ FastqRoles fastq_roles(uint32_t nl, uint32_t phi) {
    const uint32_t b0 = fastq_pxor(nl << 1) ^ (phi & 1u ? ~0u : 0u);
    const uint32_t b1 = fastq_pxor((nl & b0) << 1) ^ (phi & 2u ? ~0u : 0u);
    return {b0 & ~b1, b0 & b1, ~b0 & ~b1, ~b0 & b1};
}

// pass 1
__global__ __launch_bounds__(kFastaBlock) void fastq_lines(FastqArgs a, uint64_t first_tile) {
    __shared__ uint32_t s_nl[kFastaWaves];
    const uint64_t tile = first_tile + blockIdx.x;
    const FastqLane l = fastq_lane<false>(a, tile);
    tile_rank_post((uint32_t)__popc(l.nl), s_nl);
    __syncthreads();
    if (threadIdx.x == 0) a.lines[tile] = tile_total<kFastaWaves>(s_nl);
}

// the kCountedGroup entries of group g of a per-tile u32 array (whole groups exist and are 16-B aligned), those past n_tiles as 0
__device__ __forceinline__ void fastq_group(const uint32_t* p, uint64_t g, uint64_t n_groups, uint64_t n_tiles, uint32_t (&v)[kCountedGroup]) {
#pragma unroll
    for (int e = 0; e < kCountedGroup; ++e) v[e] = 0;
    if (g >= n_groups) return;
    const u32x4* q = reinterpret_cast<const u32x4*>(p + g * kCountedGroup);
#pragma unroll
    for (int u = 0; u < kCountedGroup / 4; ++u) {
        const u32x4 c = q[u];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * u + e] = g * kCountedGroup + 4 * u + e < n_tiles ? c[e] : 0u;
    }
}

// pass 2: one workgroup.  Lane j of a round owns the kCountedGroup tiles of group first + j; only the line feeds mod 4 matter.
__global__ __launch_bounds__(kFastqScanBlock) void fastq_line_scan(FastqArgs a) {
    constexpr int W = kFastqScanBlock / 64;
    __shared__ uint32_t s_w[W];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n_groups = (a.n_tiles + kCountedGroup - 1) / kCountedGroup;
    uint32_t carry = 0;  // the text begins on line 0
    for (uint64_t first = 0; first < n_groups; first += kFastqScanBlock) {
        const uint64_t g = first + threadIdx.x;
        uint32_t n[kCountedGroup];
        fastq_group(a.lines, g, n_groups, a.n_tiles, n);
        uint32_t sum = 0;
#pragma unroll
        for (int e = 0; e < kCountedGroup; ++e) sum += n[e] & 3u;
        const uint32_t x = wave_inclusive_sum(sum, lane);
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        uint32_t before = carry + x - sum, total = 0;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const uint32_t y = s_w[q];
            before += q < (int)wave ? y : 0u;
            total += y;
        }
        if (g < n_groups) {  // the group's carries whole: one 16-B store
            uint32_t c[kCountedGroup / 4] = {};
#pragma unroll
            for (int e = 0; e < kCountedGroup; ++e) {
                c[e >> 2] |= (before & 3u) << (8 * (e & 3));
                before += n[e];
            }
            *reinterpret_cast<u32x4*>(a.carry + g * kCountedGroup) = u32x4{c[0], c[1], c[2], c[3]};
        }
        carry = (carry + total) & 3u;
        __syncthreads();  // s_w is rewritten by the next round
    }
}

// pass 3
template <bool ALLOW_N>
__device__ __forceinline__ void fastq_count_tile(const FastqArgs& a, uint64_t first_tile) {
    __shared__ uint32_t s_nl[kFastaWaves], s_mal[kFastaWaves];
    __shared__ uint64_t s_sum[kFastaWaves];
    const uint64_t tile = first_tile + blockIdx.x;
    const FastqLane l = fastq_lane<ALLOW_N>(a, tile);
    const uint32_t c_nl = (uint32_t)__popc(l.nl);
    const uint32_t x_nl = tile_rank_post(c_nl, s_nl);
    const uint32_t carry = a.carry[tile];
    __syncthreads();
    const FastqRoles r = fastq_roles(l.nl, carry + tile_before<kFastaWaves>(s_nl, x_nl - c_nl));
    const uint32_t seq = l.valid & r.seq & ~l.drop, qual = l.valid & r.qual & ~l.drop;
    uint64_t v = (uint64_t)__popc(seq) | ((uint64_t)__popc(qual) << 16) | ((uint64_t)__popc(l.ls & r.rec) << 32) | ((uint64_t)__popc(seq & l.bad) << 48);
    v = wave_sum_u64(v);  // a wave's fields stay below 2^12
    uint32_t m = (uint32_t)(__popc(l.ls & r.rec & ~l.at) + __popc(l.ls & r.sep & ~l.plus));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m += __shfl_down(m, off, 64);
    if ((threadIdx.x & 63u) == 0) {
        s_sum[threadIdx.x >> 6] = v;
        s_mal[threadIdx.x >> 6] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t sum = 0;
#pragma unroll
        for (int q = 0; q < kFastaWaves; ++q) sum += s_sum[q];
        a.counts[tile] = (uint32_t)sum & 0xFFFFu;
        a.qual_counts[tile] = (uint32_t)(sum >> 16) & 0xFFFFu;
        a.rec_counts[tile] = (uint32_t)(sum >> 32) & 0xFFFFu;
        a.flaws[tile] = (uint32_t)(sum >> 48) | (tile_total<kFastaWaves>(s_mal) << 16);
    }
}
__global__ __launch_bounds__(kFastaBlock) void fastq_count(FastqArgs a, uint64_t first_tile) { fastq_count_tile<false>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fastq_count_n(FastqArgs a, uint64_t first_tile) { fastq_count_tile<true>(a, first_tile); }

// pass 4: one workgroup, the three streams scanned as counted_scan scans one; the flaws are only summed
__global__ __launch_bounds__(kFastqScanBlock) void fastq_scan(FastqArgs a) {
    constexpr int W = kFastqScanBlock / 64;
    __shared__ uint64_t s_seq[W], s_qual[W], s_rec[W], s_bad[W], s_mal[W];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n_groups = (a.n_tiles + kCountedGroup - 1) / kCountedGroup;
    uint64_t seq_carry = 0, qual_carry = 0, rec_carry = 0, bad_total = 0, mal_total = 0;
    for (uint64_t first = 0; first < n_groups; first += kFastqScanBlock) {
        const uint64_t g = first + threadIdx.x;
        uint32_t v[kCountedGroup];
        uint64_t seq_sum = 0, qual_sum = 0, rec_sum = 0, bad_sum = 0, mal_sum = 0;
        fastq_group(a.counts, g, n_groups, a.n_tiles, v);
#pragma unroll
        for (int e = 0; e < kCountedGroup; ++e) seq_sum += v[e];
        fastq_group(a.qual_counts, g, n_groups, a.n_tiles, v);
#pragma unroll
        for (int e = 0; e < kCountedGroup; ++e) qual_sum += v[e];
        fastq_group(a.rec_counts, g, n_groups, a.n_tiles, v);
#pragma unroll
        for (int e = 0; e < kCountedGroup; ++e) rec_sum += v[e];
        fastq_group(a.flaws, g, n_groups, a.n_tiles, v);
#pragma unroll
        for (int e = 0; e < kCountedGroup; ++e) {
            bad_sum += v[e] & 0xFFFFu;
            mal_sum += v[e] >> 16;
        }
        uint64_t x = seq_sum, y = qual_sum, z = rec_sum;  // inclusive scans over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t xu = shfl_up_u64(x, o), yu = shfl_up_u64(y, o), zu = shfl_up_u64(z, o);
            if (lane >= (uint32_t)o) {
                x += xu;
                y += yu;
                z += zu;
            }
        }
        const uint64_t bad_wave = wave_sum_u64(bad_sum), mal_wave = wave_sum_u64(mal_sum);
        if (lane == 63) {
            s_seq[wave] = x;
            s_qual[wave] = y;
            s_rec[wave] = z;
        }
        if (lane == 0) {
            s_bad[wave] = bad_wave;
            s_mal[wave] = mal_wave;
        }
        __syncthreads();
        uint64_t seq_before = seq_carry + x - seq_sum, qual_before = qual_carry + y - qual_sum, rec_before = rec_carry + z - rec_sum;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            seq_before += q < (int)wave ? s_seq[q] : 0;
            qual_before += q < (int)wave ? s_qual[q] : 0;
            rec_before += q < (int)wave ? s_rec[q] : 0;
            seq_carry += s_seq[q];
            qual_carry += s_qual[q];
            rec_carry += s_rec[q];
            bad_total += s_bad[q];
            mal_total += s_mal[q];
        }
        if (g < n_groups) {
            a.offs[g] = seq_before;
            a.qual_offs[g] = qual_before;
            a.rec_offs[g] = rec_before;
        }
        __syncthreads();  // the shared arrays are rewritten by the next round
    }
    if (threadIdx.x == 0) {
        a.totals[0] = seq_carry;
        a.totals[1] = rec_carry;
        a.totals[2] = bad_total;
        a.totals[3] = qual_carry;
        a.totals[4] = mal_total;
    }
}

// A lane's quality bytes (mask qm of its dwords w) to the LDS bytes s_q[at ..], in order.  A lane that holds 32 of them -- most
// lanes hold 32 or none -- writes whole dwords, shifted to the byte phase of `at`, and its ragged first and last dword by bytes:
// the neighbours' bytes lie in the same dwords.
__device__ __forceinline__ void fastq_stage_qual(uint32_t* s_qw, uint32_t at, uint32_t qm, const uint32_t (&w)[8]) {
    uint8_t* s_q = reinterpret_cast<uint8_t*>(s_qw);
    if (qm == ~0u) {
        const uint32_t sh = at & 3u, d = at >> 2;
        if (sh == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) s_qw[d + k] = w[k];
        } else {
            const uint32_t head = 4 - sh;  // bytes of a dword of the lane that end the dword of LDS in front
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if ((uint32_t)i < head) s_q[at + i] = (uint8_t)(w[0] >> (8 * i));
#pragma unroll
            for (int k = 0; k < 7; ++k) s_qw[d + 1 + k] = __builtin_amdgcn_alignbit(w[k + 1], w[k], 8 * head);
#pragma unroll
            for (int i = 1; i < 4; ++i)
                if ((uint32_t)i >= head) s_q[at + 28 + i] = (uint8_t)(w[7] >> (8 * i));
        }
    } else {
        uint32_t p = at;
#pragma unroll
        for (int i = 0; i < 32; ++i)
            if ((qm >> i) & 1u) s_q[p++] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

// pass 6
template <bool STRICT, bool REC, bool QUAL>
__device__ __forceinline__ void fastq_write_tile(const FastqArgs& a, uint64_t first_tile) {
    __shared__ unsigned long long s_out[kHpcTileWords + 1];
    __shared__ __attribute__((aligned(16))) uint32_t s_qw[kFastqQualLds / 4];
    __shared__ uint32_t s_nl[kFastaWaves];
    __shared__ uint64_t s_cnt[kFastaWaves];
    __shared__ HpcSpan s_span;
    __shared__ uint64_t s_qual_base, s_rec_base;
    const uint64_t tile = first_tile + blockIdx.x;
    const uint32_t j = threadIdx.x, lane = j & 63u;
    const uint32_t total = a.counts[tile], qual_total = QUAL ? a.qual_counts[tile] : 0u, rec_total = REC ? a.rec_counts[tile] : 0u;
    if (total == 0 && qual_total == 0 && rec_total == 0) return;
    const FastqLane l = fastq_lane<false>(a, tile);
    const uint32_t c_nl = (uint32_t)__popc(l.nl);
    const uint32_t x_nl = tile_rank_post(c_nl, s_nl);
    s_out[j] = 0;
    if (j == 0) {
        s_out[kHpcTileWords] = 0;
        const uint64_t base = counted_tile_base(a.offs, a.counts, tile);
        s_span = {base, base >= a.out_cap ? 0u : (uint32_t)(a.out_cap - base < total ? a.out_cap - base : total)};
        if (QUAL || REC) s_qual_base = counted_tile_base(a.qual_offs, a.qual_counts, tile);
        if (REC) s_rec_base = counted_tile_base(a.rec_offs, a.rec_counts, tile);
    }
    const uint32_t carry = a.carry[tile];
    __syncthreads();
    const FastqRoles r = fastq_roles(l.nl, carry + tile_before<kFastaWaves>(s_nl, x_nl - c_nl));
    const uint32_t seq = l.valid & r.seq & ~l.drop, qm = l.valid & r.qual & ~l.drop, rs = l.ls & r.rec;
    // the lane's three counts ranked in one scan: 16-bit fields, a tile's totals stay at or below 8192
    const uint64_t mine = (uint64_t)__popc(seq) | ((uint64_t)__popc(qm) << 16) | ((uint64_t)(REC ? __popc(rs) : 0) << 32);
    uint64_t x = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = shfl_up_u64(x, o);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63u) s_cnt[j >> 6] = x;
    __syncthreads();
    uint64_t front = x - mine;  // the tile's entries in front of the lane
#pragma unroll
    for (int q = 0; q < kFastaWaves - 1; ++q) front += q < (int)(j >> 6) ? s_cnt[q] : 0ull;
    const uint32_t before = (uint32_t)front & 0xFFFFu, qual_before = (uint32_t)(front >> 16) & 0xFFFFu, rec_before = (uint32_t)(front >> 32) & 0xFFFFu;
    const uint32_t c = (uint32_t)__popc(seq);
    const HpcSpan s = s_span;
    const uint64_t qual_base = (QUAL || REC) ? s_qual_base : 0;
    if (REC) {
        uint64_t e = s_rec_base + rec_before;
        for (uint32_t m = rs; m && e < a.rec_cap; m &= m - 1, ++e) {
            const uint32_t i = (uint32_t)__builtin_ctz(m), below = (1u << i) - 1u;
            a.rec_text[e] = (uint64_t)(l.s + i);
            a.rec_start[e] = s.base + before + (uint32_t)__popc(seq & below);
            a.rec_qual[e] = qual_base + qual_before + (uint32_t)__popc(qm & below);
        }
    }
    const uint32_t phase = (uint32_t)(s.base & 31u);
    if (s.room) {  // uniform: some sequence byte of the tile lies below out_cap
        const uint32_t cc = before >= s.room ? 0u : (s.room - before < c ? s.room - before : c);  // the lane's codes below out_cap
        if (cc) {
            const uint64_t w = (uint64_t)enc16<STRICT>(l.q[0]) | ((uint64_t)enc16<STRICT>(l.q[1]) << 32);
            uint64_t frag = hpc_compress(w, fasta_spread(seq));
            if (cc < 32) frag &= (1ull << (2 * cc)) - 1ull;
            const uint32_t at = phase + before, sh = 2 * (at & 31u);
            atomicOr(&s_out[at >> 5], (unsigned long long)(frag << sh));
            if ((at & 31u) + cc > 32) atomicOr(&s_out[(at >> 5) + 1], (unsigned long long)(frag >> (64 - sh)));
        }
    }
    // the tile's quality bytes below qual_cap: `qual_room` of them from byte qual_base of qual on, staged at the 16-B phase of
    // their address so that the inner 16-B pieces are aligned in LDS and in memory alike
    uint32_t qual_room = 0, stage = 0;
    if (QUAL) {
        qual_room = qual_base >= a.qual_cap ? 0u : (uint32_t)(a.qual_cap - qual_base < qual_total ? a.qual_cap - qual_base : qual_total);
        stage = (uint32_t)(reinterpret_cast<uintptr_t>(a.qual + qual_base) & 15u);
        if (qual_room && qm) {
            const uint32_t w[8] = {l.q[0][0], l.q[0][1], l.q[0][2], l.q[0][3], l.q[1][0], l.q[1][1], l.q[1][2], l.q[1][3]};
            fastq_stage_qual(s_qw, stage + qual_before, qm, w);
        }
    }
    __syncthreads();
    if (s.room) {
        const uint32_t n_words = (phase + s.room + 31u) >> 5;  // <= 257
        uint64_t* out = a.out + (s.base >> 5);
        for (uint32_t k = j; k < n_words; k += kFastaBlock) {
            const unsigned long long v = s_out[k];
            if ((k == 0 && hpc_head_shared(s)) || (k == n_words - 1 && hpc_tail_shared(s))) {
                if (v) hpc_merge(out + k, v);
            } else {
                out[k] = v;
            }
        }
    }
    if (QUAL && qual_room) {
        const uint8_t* s_q = reinterpret_cast<const uint8_t*>(s_qw);
        const uintptr_t dst = reinterpret_cast<uintptr_t>(a.qual + qual_base) - stage;  // 16-B aligned; only [stage, end) of it is written
        const uint32_t end = stage + qual_room, n_pieces = (end + 15u) >> 4;            // <= 513
        for (uint32_t k = j; k < n_pieces; k += kFastaBlock) {
            const uint32_t lo = 16 * k;
            if (lo >= stage && lo + 16 <= end) {
                *reinterpret_cast<u32x4*>(dst + lo) = *reinterpret_cast<const u32x4*>(s_q + lo);
            } else {
                for (uint32_t b = lo < stage ? stage : lo; b < lo + 16 && b < end; ++b) *reinterpret_cast<uint8_t*>(dst + b) = s_q[b];
            }
        }
    }
}
__global__ __launch_bounds__(kFastaBlock) void fastq_write(FastqArgs a, uint64_t first_tile) { fastq_write_tile<false, false, false>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fastq_write_rec(FastqArgs a, uint64_t first_tile) { fastq_write_tile<false, true, false>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fastq_write_qual(FastqArgs a, uint64_t first_tile) { fastq_write_tile<false, false, true>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fastq_write_qual_rec(FastqArgs a, uint64_t first_tile) { fastq_write_tile<false, true, true>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fastq_write_lut(FastqArgs a, uint64_t first_tile) { fastq_write_tile<true, false, false>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fastq_write_lut_rec(FastqArgs a, uint64_t first_tile) { fastq_write_tile<true, true, false>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fastq_write_lut_qual(FastqArgs a, uint64_t first_tile) { fastq_write_tile<true, false, true>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fastq_write_lut_qual_rec(FastqArgs a, uint64_t first_tile) { fastq_write_tile<true, true, true>(a, first_tile); }

}  // namespace cnt
