// fasta_write_kernels.hpp -- 2-bit packed words to FASTA text: header lines and wrapped lines (include/cute_nt.h, "text formats:
// FASTA write").  Not in the reference, which stops at bits_to_n_*; the definition is restated twice by tests/test_fasta_write.py,
// and cnt_fasta_to_bits reads back what this writes.
//
// The text is a chain of R + 1 PIECES: piece 0 is the lead, the bases in front of the first record as headerless lines; piece
// r + 1 is record r: '>', its name, a line feed, and its bases in lines of W letters.  Only the lead may be empty, a record holds
// at least its '>' and its line feed.  The kernels see the EFFECTIVE width: W == 0 and W > len both mean "one line per body",
// which a width of max(len, 1) gives as well, so 1 <= W <= 2^36 here and byte j of a body has column j % (W + 1).
// Passes (fasta_write_abi.inc), none of which allocates:
//   1. fasta_out_sizes    one lane per piece: its byte size as a u64 (a record may hold 2^36 bases: counted_output.hpp's u32 tile
//                         counts do not fit) and its descents; an exclusive scan inside the workgroup into off[piece], the
//                         workgroup's total and its descents into sums[block] and bad[block];
//   2. fasta_out_scan     ONE workgroup, a block per lane and round, the carry going from round to round as counted_scan's does:
//                         sums[block] becomes the text offset of the block's first piece; sets the two counts, the total forced
//                         to 0 when anything is malformed, and leaves both in the scratch's head -- no atomic anywhere;
//   3. fasta_out_offsets  one lane per piece: off[piece] becomes its offset in the text, off[R + 1] the total, and the lanes that
//                         own records store rec_text.  A malformed table stores nothing;
//   4. fasta_out_write    tiled over OUTPUT bytes on the 16-B grid d_text lies in (the text itself may begin at any byte): a
//                         workgroup owns 16 KiB of it, a wave 4 KiB, a lane four 16-B chunks, so that a wave's searches and its
//                         chain of dependent loads (offsets, tables, packed words) are paid once per 4 KiB.  The grid is sized by
//                         the host-known footprint; a wave whose bytes lie at or past min(total, text_cap) leaves.  A wave finds
//                         the pieces of its first and of its last byte by a 64-way search over off[], every lane a probe.  When
//                         both are one piece and the first byte lies in its body -- a genome -- ONE division by W + 1 gives the
//                         wave's line and column, each chunk gets its own by 32-bit arithmetic, and the lanes take the wave's
//                         chunks in turn: a store instruction writes 1 KiB in a row.  Otherwise -- reads -- a lane owns 64 bytes
//                         in a row, searches the wave's piece range for its first byte, divides itself and carries its state from
//                         chunk to chunk (both divisions in double precision, fasta_out_div).  A chunk that lies in one body, 16
//                         bases or more from its end, at W >= 16 holds at most one line feed: 32 bits of codes from one funnelled
//                         pair of packed words, the decoder's dec4, the line feed spliced in per dword, one store.  Every other
//                         chunk is walked byte by byte through headers, names (copied bytewise), bodies and record ends -- an
//                         empty record with an empty name is 2 bytes, so 16 bytes can span 8 records.  Whole chunks are stored
//                         aligned; bytes are stored one by one, each guarded, only in the chunks that hold one of the text's
//                         two ends.
// A malformed table sets the total to 0, so pass 4 runs on monotone tables or not at all: whatever the tables hold, nothing is
// read outside the cnt_words_for(len) words, the R and R + 1 table entries and the names_len name bytes, and nothing is written
// outside min(total, text_cap) bytes of the text.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_kernels.hpp"
#include "word_tile.hpp"

namespace cnt {

constexpr int kFastaOutBlock = 256;
constexpr int kFastaOutWaves = kFastaOutBlock / 64;
constexpr int kFastaOutChunks = 4;  // 16-B chunks a lane writes
constexpr uint64_t kFastaOutLaneBytes = 16 * kFastaOutChunks, kFastaOutTile = kFastaOutLaneBytes * kFastaOutBlock;  // bytes of text per tile: 16384
constexpr uint64_t kFastaOutWaveBytes = kFastaOutLaneBytes * 64;
constexpr int kFastaOutScanBlock = 1024;  // fasta_out_scan: one block of pieces per lane and round

struct FastaOutArgs {
    const uint64_t* bits;  // cnt_words_for(len) words
    uint64_t len, words;
    const uint64_t* rec_start;  // [n_rec], NULL without a record
    uint64_t n_rec;
    const uint8_t* names;      // names_len bytes, NULL: every name is empty
    const uint64_t* name_off;  // [n_rec + 1], NULL with names
    uint64_t names_len;
    uint64_t width;  // effective: 1 .. max(len, 1)
    uint8_t* base;   // text - phase: 16-B aligned
    uint32_t phase;  // 0..15: where the text begins in tile 0
    uint64_t cap;    // text_cap
    uint64_t* rec_text;  // [n_rec] or NULL
    uint64_t* counts;    // the caller's two counts
    uint64_t* head;      // scratch: the total and the malformed count, for passes 3 and 4
    uint64_t* off;       // scratch [n_rec + 2]
    uint64_t* sums;      // scratch [n_blocks]
    uint64_t* bad;       // scratch [n_blocks]
    uint64_t n_blocks;   // ceil((n_rec + 1) / kFastaOutBlock)
};

// bytes of body(a, a + l): l letters and a line feed behind every line.  Wraps for an l that no well-formed table gives.
__device__ __forceinline__ uint64_t fasta_out_body_bytes(uint64_t l, uint64_t w) { return l + l / w + (l % w != 0); }

// What a lane knows of a piece: where its bases begin and how many there are, where its name begins, and the bytes of its header.
struct FastaOutPiece {
    uint64_t first, bases;  // s_r and s_{r+1} - s_r
    uint64_t name;          // o_r
    uint64_t header;        // 0 for the lead, else name bytes + 2
};
__device__ __forceinline__ FastaOutPiece fasta_out_piece(const FastaOutArgs& a, uint64_t p) {
    FastaOutPiece q;
    if (p == 0) {
        q.first = 0;
        q.bases = a.n_rec ? a.rec_start[0] : a.len;
        q.name = 0;
        q.header = 0;
    } else {
        const uint64_t r = p - 1;
        q.first = a.rec_start[r];
        q.bases = (r + 1 < a.n_rec ? a.rec_start[r + 1] : a.len) - q.first;
        q.name = a.name_off ? a.name_off[r] : 0;
        q.header = 2 + (a.name_off ? a.name_off[r + 1] - q.name : 0);
    }
    return q;
}

// The end of a size pass, shared with the FASTQ writer's (fastq_write_kernels.hpp): piece p of workgroup `block` holds `size`
// bytes and `bad` descents; the exclusive scan inside the workgroup goes to off[p], the workgroup's two totals to sums[block] and
// bad[block].  Every thread of the workgroup calls it.
__device__ __forceinline__ void fasta_out_block_scan(const FastaOutArgs& a, uint64_t block, uint64_t p, uint64_t size, uint64_t bad) {
    __shared__ uint64_t s_sum[kFastaOutWaves], s_bad[kFastaOutWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t x = size;  // the inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t xu = shfl_up_u64(x, o);
        if (lane >= (uint32_t)o) x += xu;
    }
    const uint64_t bad_wave = wave_sum_u64(bad);
    if (lane == 63) s_sum[wave] = x;
    if (lane == 0) s_bad[wave] = bad_wave;
    __syncthreads();
    uint64_t before = x - size;
#pragma unroll
    for (int q = 0; q < kFastaOutWaves - 1; ++q) before += q < (int)wave ? s_sum[q] : 0;
    if (p <= a.n_rec) a.off[p] = before;
    if (threadIdx.x == 0) {
        uint64_t total = 0, bad_total = 0;
#pragma unroll
        for (int q = 0; q < kFastaOutWaves; ++q) {
            total += s_sum[q];
            bad_total += s_bad[q];
        }
        a.sums[block] = total;
        a.bad[block] = bad_total;
    }
}

// pass 1
__global__ __launch_bounds__(kFastaOutBlock) void fasta_out_sizes(FastaOutArgs a, uint64_t first_block) {
    const uint64_t block = first_block + blockIdx.x, p = block * kFastaOutBlock + threadIdx.x;
    uint64_t size = 0, bad = 0;
    if (p == 0) {
        size = fasta_out_body_bytes(a.n_rec ? a.rec_start[0] : a.len, a.width);
    } else if (p <= a.n_rec) {
        const uint64_t r = p - 1;
        const uint64_t s0 = a.rec_start[r], s1 = r + 1 < a.n_rec ? a.rec_start[r + 1] : a.len;
        bad = s0 > s1;
        size = 2 + fasta_out_body_bytes(s0 > s1 ? 0 : s1 - s0, a.width);
        if (a.name_off) {
            const uint64_t o0 = a.name_off[r], o1 = a.name_off[r + 1];
            bad += o0 > o1;
            if (r + 1 == a.n_rec) bad += o1 > a.names_len;
            size += o0 > o1 ? 0 : o1 - o0;
        }
    }
    fasta_out_block_scan(a, block, p, size, bad);
}

// pass 2: one workgroup
__global__ __launch_bounds__(kFastaOutScanBlock) void fasta_out_scan(FastaOutArgs a) {
    constexpr int W = kFastaOutScanBlock / 64;
    __shared__ uint64_t s_sum[W], s_bad[W];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t carry = 0, bad_total = 0;
    for (uint64_t first = 0; first < a.n_blocks; first += kFastaOutScanBlock) {
        const uint64_t b = first + threadIdx.x;
        const uint64_t sum = b < a.n_blocks ? a.sums[b] : 0, bad = b < a.n_blocks ? a.bad[b] : 0;
        uint64_t x = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t xu = shfl_up_u64(x, o);
            if (lane >= (uint32_t)o) x += xu;
        }
        const uint64_t bad_wave = wave_sum_u64(bad);
        if (lane == 63) s_sum[wave] = x;
        if (lane == 0) s_bad[wave] = bad_wave;
        __syncthreads();
        uint64_t before = carry + x - sum;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            before += q < (int)wave ? s_sum[q] : 0;
            carry += s_sum[q];
            bad_total += s_bad[q];
        }
        if (b < a.n_blocks) a.sums[b] = before;
        __syncthreads();  // the shared arrays are rewritten by the next round
    }
    if (threadIdx.x == 0) {
        const uint64_t total = bad_total ? 0 : carry;
        a.counts[0] = total;
        a.counts[1] = bad_total;
        a.head[0] = total;
        a.head[1] = bad_total;
    }
}

// pass 3
__global__ __launch_bounds__(kFastaOutBlock) void fasta_out_offsets(FastaOutArgs a, uint64_t first_block) {
    const uint64_t block = first_block + blockIdx.x, p = block * kFastaOutBlock + threadIdx.x;
    if (p > a.n_rec) return;
    const bool good = a.head[1] == 0;
    const uint64_t at = a.sums[block] + a.off[p];
    a.off[p] = at;
    if (p == 0) a.off[a.n_rec + 1] = a.head[0];
    if (p && a.rec_text && good) a.rec_text[p - 1] = at;
}

// The largest piece p in [lo, hi) with off[p] <= x, given off[lo] <= x < off[hi]: every lane of the wave probes, the range
// shrinks 64-fold a step.  All 64 lanes call it with the same arguments.
__device__ __forceinline__ uint64_t fasta_out_find(const uint64_t* off, uint64_t lo, uint64_t hi, uint64_t x) {
    const uint32_t lane = threadIdx.x & 63u;
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) >> 6;
        const uint64_t q = lo + (lane + 1) * step;
        const bool below = q < hi && off[q] <= x;
        const uint64_t n = (uint64_t)__popcll(__ballot(below));  // off[] does not descend: the lanes that say yes are the first n
        lo += n * step;
        hi = hi < lo + step ? hi : lo + step;
    }
    return lo;
}

// j / d and the remainder for j < 2^53 and 1 <= d < 2^53 (a body's byte and W + 1 stay below 2^38): both are exact as doubles, the
// rounded quotient is the true one or, where it rounded up to an integer, one more, and one multiply-back settles it -- a fifth of
// the instructions of a 64-bit integer division.
__device__ __forceinline__ uint64_t fasta_out_div(uint64_t j, uint64_t d, uint64_t& rem) {
    uint64_t q = (uint64_t)((double)j / (double)d);
    int64_t r = (int64_t)(j - q * d);
    if (r < 0) {
        --q;
        r += (int64_t)d;
    } else if (r >= (int64_t)d) {
        ++q;
        r -= (int64_t)d;
    }
    rem = (uint64_t)r;
    return q;
}

// Sixteen letters with at most one line feed among them: the bytes of l (16 letters, 4 dwords) below m stay, byte m is a line feed,
// the bytes behind it are l's moved up by one; m >= 16: l as it is.  Per dword and without a branch.
__device__ __forceinline__ u32x4 fasta_out_splice(u32x4 l, uint32_t m) {
    u32x4 r;
    uint32_t prev = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int t = (int)m - 4 * d;  // where the line feed lies in this dword, if 0..3
        const uint32_t moved = __builtin_amdgcn_alignbyte(l[d], prev, 3);  // bytes 4 d - 1 .. 4 d + 2 of l
        const uint32_t keep = t <= 0 ? 0u : (t >= 4 ? ~0u : (1u << (8 * t)) - 1u);
        const bool here = t >= 0 && t < 4;
        const uint32_t feed_mask = here ? 0xFFu << (8 * t) : 0u, feed = here ? 0x0Au << (8 * t) : 0u;
        r[d] = (l[d] & keep) | feed | (moved & ~(keep | feed_mask));
        prev = l[d];
    }
    return r;
}

// pass 4
__global__ __launch_bounds__(kFastaOutBlock) void fasta_out_write(FastaOutArgs a, uint64_t first_tile) {
    const uint64_t tile = first_tile + blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t total = a.head[0];
    const int64_t limit = (int64_t)(total < a.cap ? total : a.cap);  // the bytes of text this call writes
    // the wave's bytes [w0, w1) and the lane's [x0, x1), as positions in the text
    const int64_t wx = (int64_t)(tile * kFastaOutTile + wave * kFastaOutWaveBytes) - (int64_t)a.phase;
    const int64_t w0 = wx < 0 ? 0 : wx, w1 = wx + (int64_t)kFastaOutWaveBytes < limit ? wx + (int64_t)kFastaOutWaveBytes : limit;
    if (w0 >= w1) return;  // the whole wave
    const uint64_t pieces = a.n_rec + 1;
    const uint64_t pf = fasta_out_find(a.off, 0, pieces, (uint64_t)w0);
    // a record holds two bytes or more: the last byte's piece is at most kFastaOutWaveBytes / 2 pieces on
    const uint64_t most = pf + kFastaOutWaveBytes / 2 + 1;
    // the piece ends behind the wave's last byte -- a genome: no second search, one load that the wave needs anyway
    const uint64_t pl = a.off[pf + 1] > (uint64_t)(w1 - 1) ? pf : fasta_out_find(a.off, pf, most < pieces ? most : pieces, (uint64_t)(w1 - 1));
    const uint64_t w = a.width, w1c = w + 1;
    uint64_t p = pf, at = 0, end = 0;  // the piece of the lane's byte, where it begins and ends in the text
    FastaOutPiece pc = {};
    uint64_t u = 0;            // the byte's offset in its piece
    uint64_t col = 0, b = 0;  // in a body: the byte's column, and the bases of the body in front of it
    // FAST: the wave's bytes lie in one body.  One division for the wave; its lanes take the 16-B chunks of the wave's 4 KiB in
    // turn, 64 neighbours to a store instruction, each chunk's line and column from the wave's by 32-bit arithmetic.  Otherwise a
    // lane owns 64 bytes in a row and carries its state from chunk to chunk.
    bool fast = false;
    uint64_t line0 = 0, col0 = 0;
    if (pf == pl) {  // wave-uniform
        at = a.off[p];
        end = a.off[p + 1];
        pc = fasta_out_piece(a, p);
        fast = (uint64_t)w0 - at >= pc.header;
        if (fast) line0 = fasta_out_div((uint64_t)w0 - at - pc.header, w1c, col0);
    }
    const int64_t lx = wx + (int64_t)(lane * kFastaOutLaneBytes);
    const int64_t x0 = fast ? w0 : (lx < 0 ? 0 : lx);  // what bounds the lane's chunks
    const int64_t x1 = fast ? w1 : (lx + (int64_t)kFastaOutLaneBytes < limit ? lx + (int64_t)kFastaOutLaneBytes : limit);
    if (!fast) {
        if (x0 >= x1) return;  // no ballot or shuffle from here on
        if (pf != pl) {
            uint64_t lo = pf, hi = pl + 1;  // off[lo] <= x0 < off[hi]
            while (hi - lo > 1) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (a.off[mid] <= (uint64_t)x0)
                    lo = mid;
                else
                    hi = mid;
            }
            p = lo;
            at = a.off[p];
            end = a.off[p + 1];
            pc = fasta_out_piece(a, p);
        }
        u = (uint64_t)x0 - at;
        if (u >= pc.header) {
            const uint64_t line = fasta_out_div(u - pc.header, w1c, col);
            b = line * w + col;
        }
    }

    // from here the lane walks: (p, u, col, b) is the state at its next byte, carried from one 16-B chunk to the next
    uint64_t size = end - at;
    uint64_t win = 0, win_at = 0;  // 32 codes of the body from base win_at on
    bool have_win = false;
    const uint64_t* bits = a.bits;
#pragma unroll 1
    for (int c = 0; c < kFastaOutChunks; ++c) {
        const int64_t cx = fast ? wx + (int64_t)(c * (int)(kFastaOutWaveBytes / kFastaOutChunks) + lane * 16) : lx + 16 * c;
        const int64_t c0 = cx < x0 ? x0 : cx, c1 = cx + 16 < x1 ? cx + 16 : x1;  // the chunk's bytes [c0, c1) of [cx, cx + 16)
        if (c0 >= c1) continue;
        uint8_t* out = a.base + (uint64_t)(cx + (int64_t)a.phase);
        if (fast) {  // the chunk begins less than kFastaOutWaveBytes behind the wave's first byte
            const uint64_t cc = col0 + (uint64_t)(c0 - w0);
            uint64_t lines;
            if (w1c <= 0x40000000u) {
                const uint32_t q = (uint32_t)cc / (uint32_t)w1c;
                lines = q;
                col = (uint32_t)cc - q * (uint32_t)w1c;
            } else {  // a line longer than a wave's bytes: at most one line end in front of the chunk
                lines = cc >= w1c;
                col = cc - (lines ? w1c : 0);
            }
            b = (line0 + lines) * w + col;
            u = (uint64_t)c0 - at;
            have_win = false;
        }
        // Sixteen bytes of one body that hold at most one line feed -- nearly every chunk of a genome: 16 bases are left in the
        // body, so it does not end here, and with W >= 16 the line feed behind this line's is 17 bytes on.  The codes come from
        // one funnelled pair of words, the letters from the decoder's table, the line feed is spliced in.
        if (u >= pc.header && u < size && w >= 16 && pc.bases - b >= 16 && c1 - c0 == 16) {
            const uint64_t g = pc.first + b, wi = g >> 5;  // g + 15 < len: the word exists
            const uint64_t lo = bits[wi], hi = wi + 1 < a.words ? bits[wi + 1] : 0;
            const uint32_t codes = (uint32_t)funnel64(lo, hi, 2 * (uint32_t)(g & 31u));
            const uint64_t left = w - col;  // letters in front of this line's line feed
            *reinterpret_cast<u32x4*>(out) = fasta_out_splice(dec4(codes), left < 16 ? (uint32_t)left : 16u);
            u += 16;
            b += left < 16 ? 15 : 16;
            col = left < 16 ? 15 - left : col + 16;
            continue;
        }
        uint32_t d[4] = {0, 0, 0, 0};
        const int i0 = (int)(c0 - cx), i1 = (int)(c1 - cx);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < i0 || i >= i1) continue;
            if (u == size) {  // the next piece: a record, never empty
                ++p;
                at = end;
                end = a.off[p + 1];
                size = end - at;
                pc = fasta_out_piece(a, p);
                u = 0;
                col = 0;
                b = 0;
                have_win = false;
            }
            uint32_t byte;
            if (u < pc.header) {
                byte = u == 0 ? 0x3Eu : (u + 1 == pc.header ? 0x0Au : (uint32_t)a.names[pc.name + u - 1]);
            } else if (col == w || b == pc.bases) {
                byte = 0x0Au;
                col = 0;
            } else {
                if (!have_win || b - win_at >= 32) {
                    const uint64_t g = pc.first + b, wi = g >> 5;  // g < len: the word exists
                    const uint64_t lo = bits[wi], hi = wi + 1 < a.words ? bits[wi + 1] : 0;
                    win = funnel64(lo, hi, 2 * (uint32_t)(g & 31u));
                    win_at = b;
                    have_win = true;
                }
                const uint32_t code = (uint32_t)(win >> (2 * (uint32_t)(b - win_at))) & 3u;
                byte = (0x47544341u >> (code << 3)) & 0xFFu;  // "ACTG"[code], the decoder's table
                ++b;
                ++col;
            }
            ++u;
            d[i >> 2] |= byte << (8 * (i & 3));
        }
        if (i0 == 0 && i1 == 16) {
            *reinterpret_cast<u32x4*>(out) = u32x4{d[0], d[1], d[2], d[3]};
        } else {  // one of the text's two ends
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i >= i0 && i < i1) out[i] = (uint8_t)(d[i >> 2] >> (8 * (i & 3)));
        }
    }
}

}  // namespace cnt
