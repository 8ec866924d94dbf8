// fasta_kernels.hpp -- FASTA text straight to 2-bit packed words, with a record table (include/cute_nt.h, "text formats: FASTA").
// Not in the reference; the definition is restated three ways by tests/test_fasta.py.
//
// For the bytes t_0 .. t_{L-1}: p is a LINE START iff p == 0 or t_{p-1} == 0x0A; t_p is a HEADER byte iff the last line start <= p
// holds '>'.  Header bytes, 0x0A and 0x0D are dropped, every other byte is KEPT and encoded as cnt_n_to_bits_ex encodes it; the
// line starts that hold '>' are the records: their byte offset, and the number of kept bytes in front of them.
//
// A tile is kFastaTile bytes of the 16-B ALIGNED address space the text lies in (the text itself may begin at any byte): lane j of
// the workgroup owns the 32 bytes [32 j, 32 j + 32) of the tile, two aligned 16-B loads, and everything it knows about them is
// five 32-bit masks (line feed, carriage return, '>', outside the alphabet, inside the text).  A lane whose 32 bytes do not all
// lie inside the text -- the first and the last of a call -- reads byte by byte, each read guarded: no byte outside
// [text, text + len) is read.  Whether a byte is a header byte depends on the last line start in front of it; "the KIND of the
// last line start" (none, sequence, header) is carried lane to lane by ballots, wave to wave through LDS and tile to tile by
// fasta_scan.  Passes (fasta_abi.inc), none of which allocates:
//   1. fasta_summary   one workgroup per tile: the kind of the tile's last line start, its kept and invalid bytes counted as if
//                      the tile began on a sequence line, those of them that lie in front of the tile's first line start (what a
//                      tile that begins inside a header loses), packed into one u64; rec_counts[tile] = its header lines;
//   2. fasta_scan      ONE workgroup, a group of kCountedGroup tiles per lane and round: resolves the kinds into carry[tile]
//                      (1: the tile begins inside a header), settles counts[tile], and writes what counted_scan would: offs[group]
//                      for the kept bytes and for the records, and the three totals -- no atomic anywhere;
//   3. hpc_zero_edges  (hpc_kernels.hpp, as it stands) zeroes the at most two output words a tile shares with others;
//   4. fasta_write     a tile without kept bytes and records returns at once; the others repeat pass 1's masks with the carry,
//                      encode their 32 bytes to a word, compress it to the kept codes (hpc_compress), OR the fragments into the
//                      tile's 257 output words in LDS and store those coalesced, the shared ones through hpc_merge; a lane
//                      that holds header lines stores their two table entries itself.
// Codes at or past out_cap and records at or past rec_cap are clipped; the counts are not.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"
#include "counted_output.hpp"
#include "hpc_kernels.hpp"

namespace cnt {

constexpr int kFastaBlock = 256;
constexpr int kFastaWaves = kFastaBlock / 64;
constexpr uint64_t kFastaLaneBytes = 32, kFastaTile = kFastaLaneBytes * kFastaBlock;  // bytes per tile: 8192
constexpr int kFastaScanBlock = 1024;                                                 // fasta_scan: one group of tiles per lane and round
static_assert(kFastaBlock == kHpcBlock && kFastaTile == kHpcTile, "hpc_zero_edges takes one lane per tile of either call");
static_assert(kFastaTile < (1u << 14), "a tile's counts are 14-bit fields of its summary");

// kind of a line start
constexpr uint32_t kFastaNone = 0, kFastaSeq = 1, kFastaHeader = 2;
// a tile's summary: four 14-bit counts and the kind
constexpr uint32_t kFastaSumKept = 0, kFastaSumKeptHead = 14, kFastaSumBad = 28, kFastaSumBadHead = 42, kFastaSumKind = 56;

struct FastaArgs {
    const uint8_t* base;  // text - phase: 16-B aligned
    uint32_t phase;       // 0..15: where the text begins in tile 0
    uint64_t len;         // bytes of text, >= 1
    uint64_t n_tiles;     // ceil((phase + len) / kFastaTile)
    uint64_t* sums;       // [n_tiles] pass 1 -> pass 2
    uint8_t* carry;       // [n_tiles] pass 2 -> pass 4
    uint32_t *counts, *rec_counts;  // counted_output.hpp's two regions, once for the kept bytes and once for the records
    uint64_t *offs, *rec_offs;
    uint64_t *out, *rec_text, *rec_start;  // the record arrays may both be NULL
    uint64_t out_cap, rec_cap;             // codes, records
    uint64_t* totals;                      // the caller's three counts
};

// 0x80 in every byte of x that equals the byte repeated in c4
__device__ __forceinline__ uint32_t fasta_eq4(uint32_t x, uint32_t c4) {
    const uint32_t z = x ^ c4;
    return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
}
// bits 7, 15, 23, 31 of m as bits 0..3: the four products land on bits 28..31 and no other two on one bit, so nothing carries
__device__ __forceinline__ uint32_t fasta_gather4(uint32_t m) { return ((m >> 7) * 0x10204080u) >> 28; }

// bit i of a mask -> bit 2 i (hpc_compress's keep mask)
__device__ __forceinline__ uint64_t fasta_spread(uint32_t m) {
    uint64_t x = m;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    return (x | (x << 1)) & 0x5555555555555555ull;
}

// What a lane knows of its 32 bytes; bit i = byte i.  Bytes outside the text read as 0 and have no bit anywhere.
struct FastaLane {
    u32x4 q[2];      // the bytes
    int64_t s;       // position in the text of byte 0 (negative in front of it)
    uint32_t valid;  // inside the text
    uint32_t drop;   // 0x0A or 0x0D
    uint32_t ls;     // line starts
    uint32_t hs;     // line starts that hold '>'
    uint32_t bad;    // outside the alphabet of cnt_validate
};

template <bool ALLOW_N>
__device__ __forceinline__ FastaLane fasta_lane(const FastaArgs& a, uint64_t tile) {
    FastaLane l;
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
    uint32_t nl = 0, cr = 0, gt = 0;
    l.bad = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t x = l.q[h][e], sh = 16 * h + 4 * e;
            nl |= fasta_gather4(fasta_eq4(x, 0x0A0A0A0Au)) << sh;
            cr |= fasta_gather4(fasta_eq4(x, 0x0D0D0D0Du)) << sh;
            gt |= fasta_gather4(fasta_eq4(x, 0x3E3E3E3Eu)) << sh;
            l.bad |= fasta_gather4(invalid_mask<ALLOW_N>(x)) << sh;
        }
    // byte 0 is a line start when the byte in front of it is a line feed: the neighbour lane's bit 31, or for the first lane of
    // a wave one guarded byte read; position 0 of the text is one whatever lies in front of it
    uint32_t prev = __shfl_up(nl >> 31, 1, 64);
    if ((j & 63u) == 0) prev = (l.s >= 1 && l.s <= len) ? (uint32_t)(a.base[at - 1] == 0x0A) : 0u;
    if (l.s <= 0) prev = 0;
    l.ls = (nl << 1) | prev;
    if (l.s <= 0 && l.s > -32) l.ls |= 1u << (uint32_t)(-l.s);
    l.ls &= l.valid;
    l.hs = l.ls & gt;
    l.drop = nl | cr;
    l.bad &= l.valid;
    return l;
}

// the kind of the lane's last line start
__device__ __forceinline__ uint32_t fasta_lane_kind(const FastaLane& l) {
    if (!l.ls) return kFastaNone;
    return (l.hs >> (31 - __builtin_clz(l.ls))) & 1u ? kFastaHeader : kFastaSeq;
}

// The kind of the last line start in the lanes in front of this one, inside the tile: kFastaNone when there is none.  Posts
// the wave's own to s_kind[wave]; the caller's barrier comes between the two halves.
struct FastaWaveKind {
    uint32_t in_wave;  // from the lanes of the wave in front of this one
};
__device__ __forceinline__ FastaWaveKind fasta_kind_post(uint32_t kind, uint32_t* s_kind) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t has = __ballot(kind != kFastaNone), hdr = __ballot(kind == kFastaHeader);
    const uint64_t below = has & ((1ull << lane) - 1ull);
    FastaWaveKind k;
    k.in_wave = below ? ((hdr >> (63 - __builtin_clzll(below))) & 1ull ? kFastaHeader : kFastaSeq) : kFastaNone;
    if (lane == 0) s_kind[threadIdx.x >> 6] = has ? ((hdr >> (63 - __builtin_clzll(has))) & 1ull ? kFastaHeader : kFastaSeq) : kFastaNone;
    return k;
}
__device__ __forceinline__ uint32_t fasta_kind_before(const FastaWaveKind& k, const uint32_t* s_kind) {
    uint32_t kind = k.in_wave;
#pragma unroll
    for (int q = kFastaWaves - 2; q >= 0; --q)
        if (kind == kFastaNone && q < (int)(threadIdx.x >> 6)) kind = s_kind[q];
    return kind;
}

// the bytes in front of the lane's first line start
__device__ __forceinline__ uint32_t fasta_head_mask(const FastaLane& l) { return l.ls ? (l.ls & (0u - l.ls)) - 1u : ~0u; }

// The lane's header bytes, `header` saying whether the byte in front of the lane is one.  A header runs from its '>' to the
// byte in front of the next line start: adding hs to (no line start | hs) carries from each '>' through the bytes behind it and
// stops on the next line start, so the bits the sum changed are the header and that line start; a line start that holds '>'
// itself stays set under the carry and is put back.
__device__ __forceinline__ uint32_t fasta_header_mask(const FastaLane& l, bool header) {
    const uint32_t run = ~l.ls | l.hs;
    const uint32_t h = (((run + l.hs) ^ run) & ~(l.ls & ~l.hs)) | l.hs;
    return h | (header ? fasta_head_mask(l) : 0u);
}

// pass 1
template <bool ALLOW_N>
__device__ __forceinline__ void fasta_summary_tile(const FastaArgs& a, uint64_t first_tile) {
    __shared__ uint32_t s_kind[kFastaWaves];
    __shared__ uint64_t s_sum[kFastaWaves];
    __shared__ uint32_t s_rec[kFastaWaves];
    const uint64_t tile = first_tile + blockIdx.x;
    const FastaLane l = fasta_lane<ALLOW_N>(a, tile);
    const FastaWaveKind wk = fasta_kind_post(fasta_lane_kind(l), s_kind);
    __syncthreads();
    const uint32_t before = fasta_kind_before(wk, s_kind);
    // as if the tile began on a sequence line; `head`: what lies in front of the tile's first line start
    const uint32_t kept = l.valid & ~l.drop & ~fasta_header_mask(l, before == kFastaHeader);
    const uint32_t head = before == kFastaNone ? fasta_head_mask(l) : 0u;
    uint64_t v = ((uint64_t)__popc(kept) << kFastaSumKept) | ((uint64_t)__popc(kept & head) << kFastaSumKeptHead) |
                 ((uint64_t)__popc(kept & l.bad) << kFastaSumBad) | ((uint64_t)__popc(kept & head & l.bad) << kFastaSumBadHead);
    v = wave_sum_u64(v);  // a wave's fields stay below 2^12
    uint32_t r = (uint32_t)__popc(l.hs);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
    if ((threadIdx.x & 63u) == 0) {
        s_sum[threadIdx.x >> 6] = v;
        s_rec[threadIdx.x >> 6] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t sum = 0;
        uint32_t kind = kFastaNone;
#pragma unroll
        for (int q = 0; q < kFastaWaves; ++q) {
            sum += s_sum[q];
            if (s_kind[q] != kFastaNone) kind = s_kind[q];
        }
        a.sums[tile] = sum | ((uint64_t)kind << kFastaSumKind);
        a.rec_counts[tile] = tile_total<kFastaWaves>(s_rec);
    }
}
__global__ __launch_bounds__(kFastaBlock) void fasta_summary(FastaArgs a, uint64_t first_tile) { fasta_summary_tile<false>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fasta_summary_n(FastaArgs a, uint64_t first_tile) { fasta_summary_tile<true>(a, first_tile); }

// pass 2: one workgroup.  Lane j of a round owns the kCountedGroup tiles of group first + j: it reads their summaries (eight 16-B
// loads) and record counts (four; the scratch holds whole groups, 16-B aligned), learns from the lanes, waves and rounds in front of it whether its first tile begins inside a
// header, walks its tiles with that, and the sums of the kept bytes and of the records are scanned over the workgroup as
// counted_scan scans them.  The scratch past n_tiles holds anything and is masked.
__global__ __launch_bounds__(kFastaScanBlock) void fasta_scan(FastaArgs a) {
    constexpr int W = kFastaScanBlock / 64;
    __shared__ uint32_t s_kind[W];
    __shared__ uint64_t s_kept[W], s_rec[W], s_bad[W];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n_groups = (a.n_tiles + kCountedGroup - 1) / kCountedGroup;
    uint64_t kept_carry = 0, rec_carry = 0, bad_total = 0;
    bool header_carry = false;  // the text begins on a line start; tile 0 defines its own
    for (uint64_t first = 0; first < n_groups; first += kFastaScanBlock) {
        const uint64_t g = first + threadIdx.x, t0 = g * kCountedGroup;
        uint64_t sum[kCountedGroup] = {};
        uint32_t rec[kCountedGroup] = {};
        if (g < n_groups) {  // whole groups exist and are 16-B aligned: twelve 16-B loads, the entries past n_tiles masked
            const u32x4* ps = reinterpret_cast<const u32x4*>(a.sums + t0);
            const u32x4* pr = reinterpret_cast<const u32x4*>(a.rec_counts + t0);
#pragma unroll
            for (int u = 0; u < kCountedGroup / 2; ++u) {
                const u32x4 v = ps[u];
                sum[2 * u] = ((uint64_t)v.y << 32) | v.x;
                sum[2 * u + 1] = ((uint64_t)v.w << 32) | v.z;
            }
#pragma unroll
            for (int u = 0; u < kCountedGroup / 4; ++u) {
                const u32x4 v = pr[u];
#pragma unroll
                for (int e = 0; e < 4; ++e) rec[4 * u + e] = v[e];
            }
#pragma unroll
            for (int e = 0; e < kCountedGroup; ++e) {
                const bool live = t0 + e < a.n_tiles;
                sum[e] = live ? sum[e] : 0ull;
                rec[e] = live ? rec[e] : 0u;
            }
        }
        uint32_t kind = kFastaNone;
#pragma unroll
        for (int e = 0; e < kCountedGroup; ++e) {
            const uint32_t k = (uint32_t)(sum[e] >> kFastaSumKind) & 3u;
            kind = k != kFastaNone ? k : kind;
        }
        // the kind in front of the group: lanes of the wave, waves of the round, rounds
        const uint64_t has = __ballot(kind != kFastaNone), hdr = __ballot(kind == kFastaHeader);
        const uint64_t below = has & ((1ull << lane) - 1ull);
        uint32_t before = below ? ((hdr >> (63 - __builtin_clzll(below))) & 1ull ? kFastaHeader : kFastaSeq) : kFastaNone;
        if (lane == 0) s_kind[wave] = has ? ((hdr >> (63 - __builtin_clzll(has))) & 1ull ? kFastaHeader : kFastaSeq) : kFastaNone;
        __syncthreads();
        uint32_t round_kind = kFastaNone;  // of the whole round, for the next one
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const uint32_t k = s_kind[q];
            round_kind = k != kFastaNone ? k : round_kind;
        }
#pragma unroll
        for (int q = W - 2; q >= 0; --q)
            if (before == kFastaNone && q < (int)wave) before = s_kind[q];
        bool header = before == kFastaNone ? header_carry : before == kFastaHeader;
        uint64_t kept_sum = 0, rec_sum = 0, bad_sum = 0;
        uint32_t kept_of[kCountedGroup], carry_of[kCountedGroup / 4] = {};
#pragma unroll
        for (int e = 0; e < kCountedGroup; ++e) {
            const uint64_t s = sum[e];
            const uint32_t kept = ((uint32_t)(s >> kFastaSumKept) & 0x3FFFu) - (header ? (uint32_t)(s >> kFastaSumKeptHead) & 0x3FFFu : 0u);
            const uint32_t bad = ((uint32_t)(s >> kFastaSumBad) & 0x3FFFu) - (header ? (uint32_t)(s >> kFastaSumBadHead) & 0x3FFFu : 0u);
            kept_of[e] = kept;
            carry_of[e >> 2] |= (header ? 1u : 0u) << (8 * (e & 3));
            kept_sum += kept;
            bad_sum += bad;
            rec_sum += rec[e];
            const uint32_t k = (uint32_t)(s >> kFastaSumKind) & 3u;
            header = k != kFastaNone ? k == kFastaHeader : header;
        }
        if (g < n_groups) {  // the group's counts and carries whole: four 16-B stores and one (a masked entry is 0)
            u32x4* pc = reinterpret_cast<u32x4*>(a.counts + t0);
#pragma unroll
            for (int u = 0; u < kCountedGroup / 4; ++u) pc[u] = u32x4{kept_of[4 * u], kept_of[4 * u + 1], kept_of[4 * u + 2], kept_of[4 * u + 3]};
            *reinterpret_cast<u32x4*>(a.carry + t0) = u32x4{carry_of[0], carry_of[1], carry_of[2], carry_of[3]};
        }
        uint64_t x = kept_sum, y = rec_sum;  // inclusive scans over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t xu = shfl_up_u64(x, o), yu = shfl_up_u64(y, o);
            if (lane >= (uint32_t)o) {
                x += xu;
                y += yu;
            }
        }
        const uint64_t bad_wave = wave_sum_u64(bad_sum);
        if (lane == 63) {
            s_kept[wave] = x;
            s_rec[wave] = y;
        }
        if (lane == 0) s_bad[wave] = bad_wave;
        __syncthreads();
        uint64_t kept_before = kept_carry + x - kept_sum, rec_before = rec_carry + y - rec_sum;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            kept_before += q < (int)wave ? s_kept[q] : 0;
            rec_before += q < (int)wave ? s_rec[q] : 0;
            kept_carry += s_kept[q];
            rec_carry += s_rec[q];
            bad_total += s_bad[q];
        }
        if (g < n_groups) {
            a.offs[g] = kept_before;
            a.rec_offs[g] = rec_before;
        }
        header_carry = round_kind == kFastaNone ? header_carry : round_kind == kFastaHeader;
        __syncthreads();  // the shared arrays are rewritten by the next round
    }
    if (threadIdx.x == 0) {
        a.totals[0] = kept_carry;
        a.totals[1] = rec_carry;
        a.totals[2] = bad_total;
    }
}

// pass 4
template <bool STRICT, bool REC>
__device__ __forceinline__ void fasta_write_tile(const FastaArgs& a, uint64_t first_tile) {
    __shared__ unsigned long long s_out[kHpcTileWords + 1];
    __shared__ uint32_t s_kind[kFastaWaves], s_cnt[kFastaWaves], s_rcnt[kFastaWaves];
    __shared__ HpcSpan s_span;
    __shared__ uint64_t s_rec_base;
    const uint64_t tile = first_tile + blockIdx.x;
    const uint32_t j = threadIdx.x;
    const uint32_t total = a.counts[tile], rec_total = REC ? a.rec_counts[tile] : 0u;
    if (total == 0 && rec_total == 0) return;
    const FastaLane l = fasta_lane<false>(a, tile);
    const FastaWaveKind wk = fasta_kind_post(fasta_lane_kind(l), s_kind);
    s_out[j] = 0;
    if (j == 0) {
        s_out[kHpcTileWords] = 0;
        const uint64_t base = counted_tile_base(a.offs, a.counts, tile);
        s_span = {base, base >= a.out_cap ? 0u : (uint32_t)(a.out_cap - base < total ? a.out_cap - base : total)};
        if (REC) s_rec_base = counted_tile_base(a.rec_offs, a.rec_counts, tile);
    }
    const bool header_in = a.carry[tile] != 0;
    __syncthreads();
    uint32_t before_kind = fasta_kind_before(wk, s_kind);
    if (before_kind == kFastaNone) before_kind = header_in ? kFastaHeader : kFastaSeq;
    const uint32_t kept = l.valid & ~l.drop & ~fasta_header_mask(l, before_kind == kFastaHeader);
    const uint32_t c = (uint32_t)__popc(kept), rc = REC ? (uint32_t)__popc(l.hs) : 0u;
    const uint32_t x = tile_rank_post(c, s_cnt);
    uint32_t rx = 0;
    if (REC) rx = tile_rank_post(rc, s_rcnt);
    __syncthreads();
    const HpcSpan s = s_span;
    const uint32_t before = tile_before<kFastaWaves>(s_cnt, x - c);  // the tile's kept bytes in front of the lane
    if (REC) {
        uint64_t r = s_rec_base + tile_before<kFastaWaves>(s_rcnt, rx - rc);
        for (uint32_t m = l.hs; m && r < a.rec_cap; m &= m - 1, ++r) {
            const uint32_t i = (uint32_t)__builtin_ctz(m);
            a.rec_text[r] = (uint64_t)(l.s + i);
            a.rec_start[r] = s.base + before + (uint32_t)__popc(kept & ((1u << i) - 1u));
        }
    }
    if (s.room == 0) return;  // uniform: no kept byte of the tile lies below out_cap
    const uint32_t phase = (uint32_t)(s.base & 31u);
    const uint32_t cc = before >= s.room ? 0u : (s.room - before < c ? s.room - before : c);  // the lane's codes below out_cap
    const uint64_t w = (uint64_t)enc16<STRICT>(l.q[0]) | ((uint64_t)enc16<STRICT>(l.q[1]) << 32);
    uint64_t frag = hpc_compress(w, fasta_spread(kept));
    if (cc < 32) frag &= (1ull << (2 * cc)) - 1ull;
    if (cc) {
        const uint32_t at = phase + before, sh = 2 * (at & 31u);
        atomicOr(&s_out[at >> 5], (unsigned long long)(frag << sh));
        if ((at & 31u) + cc > 32) atomicOr(&s_out[(at >> 5) + 1], (unsigned long long)(frag >> (64 - sh)));
    }
    __syncthreads();
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
__global__ __launch_bounds__(kFastaBlock) void fasta_write(FastaArgs a, uint64_t first_tile) { fasta_write_tile<false, false>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fasta_write_rec(FastaArgs a, uint64_t first_tile) { fasta_write_tile<false, true>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fasta_write_lut(FastaArgs a, uint64_t first_tile) { fasta_write_tile<true, false>(a, first_tile); }
__global__ __launch_bounds__(kFastaBlock) void fasta_write_lut_rec(FastaArgs a, uint64_t first_tile) { fasta_write_tile<true, true>(a, first_tile); }

}  // namespace cnt
