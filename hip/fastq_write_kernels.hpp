// fastq_write_kernels.hpp -- 2-bit packed words and quality bytes to four-line FASTQ text (include/cute_nt.h, "text formats: FASTQ
// write").  Not in the reference, which stops at bits_to_n_*; the definition is restated twice by tests/test_fastq_write.py, and
// cnt_fastq_to_bits reads back what this writes.
//
// Record r is '@', its name, a line feed, its letters, "\n+\n", its qualities and a line feed: |name| + 2 l + 6 bytes, six at the
// least.  The text is the FASTA writer's chain of R + 1 pieces (fasta_write_kernels.hpp) with a lead, piece 0, that is ALWAYS
// empty, so three of the four passes are that writer's own kernels on a FastaOutArgs:
//   1. fastq_out_sizes    one lane per piece: its size and its descents, and rec_start[0] != 0 as one more; the scan inside the
//                         workgroup is fasta_out_block_scan;
//   2. fasta_out_scan     as it is: the text offsets of the workgroups, the two counts, the total forced to 0 when anything is
//                         malformed;
//   3. fasta_out_offsets  as it is: off[piece], off[R + 1] = the total, rec_text;
//   4. fastq_out_write    tiled over OUTPUT bytes on the 16-B grid d_text lies in, with the FASTA writer's geometry: a workgroup
//                         owns 16 KiB, a wave 4 KiB, and a wave's lanes take its 16-B chunks in turn, so that one store
//                         instruction writes 1 KiB in a row.  A wave finds the pieces of its first and last byte by the 64-way
//                         search fasta_out_find; a chunk then finds the piece of its own first byte by bisection inside that
//                         range, beginning at the piece of the lane's chunk before.  There is NO walk over bytes: a chunk is
//                         composed by a loop over the records that overlap it -- one for nearly every chunk, two at a record
//                         seam, three at the most, a record holding six bytes or more.  For a record the chunk takes seven
//                         thresholds from the record's offsets (where '@', the name, its line feed, the letters, the three
//                         bytes "\n+\n" and the qualities end, each as a byte of the chunk, 0..16) and lays the segments over a
//                         vector of line feeds from the back, each under the mask "bytes below its end": the qualities, '+',
//                         the letters, the name, '@'.  The letters are one funnelled pair of packed words through the decoder's
//                         dec4; where they begin inside the chunk the CODES are read from that many bases further in front (or
//                         shifted up, in front of base 0) instead of moving 16 letters up by bytes.  Name and quality bytes lie
//                         at any address: five aligned dword loads and v_alignbyte where all five lie inside the buffer,
//                         sixteen guarded byte loads otherwise -- only within 20 bytes of a source buffer's two ends.  A
//                         candidate is fetched only by the lanes whose chunk holds a byte of it.  Whole chunks are stored
//                         aligned; bytes are stored one by one, each guarded, only in the chunks that hold one of the text's
//                         two ends or the text_cap cut.
// The composition runs in registers; no LDS-staged variant was built: with a wave's lanes on consecutive chunks the stores are
// already whole rows, and staging segments into LDS would need byte-granular LDS writes at every seam.
// A malformed table sets the total to 0, so pass 4 runs on monotone tables that begin at base 0 or not at all: whatever the
// tables hold, nothing is read outside the cnt_words_for(len) words, the len quality bytes, the R and R + 1 table entries and the
// names_len name bytes, and nothing is written outside min(total, text_cap) bytes of the text.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fasta_write_kernels.hpp"

namespace cnt {

struct FastqOutArgs {
    FastaOutArgs f;       // what passes 2 and 3 look at, the tables and the words; f.width is not used
    const uint8_t* qual;  // f.len bytes at any address
};

// pass 1
__global__ __launch_bounds__(kFastaOutBlock) void fastq_out_sizes(FastqOutArgs q, uint64_t first_block) {
    const FastaOutArgs& a = q.f;
    const uint64_t block = first_block + blockIdx.x, p = block * kFastaOutBlock + threadIdx.x;
    uint64_t size = 0, bad = 0;
    if (p == 0) {  // the lead is empty: bases in front of the first record would belong to nothing
        bad = a.rec_start[0] != 0;
    } else if (p <= a.n_rec) {
        const uint64_t r = p - 1;
        const uint64_t s0 = a.rec_start[r], s1 = r + 1 < a.n_rec ? a.rec_start[r + 1] : a.len;
        bad = s0 > s1;
        size = 6 + 2 * (s0 > s1 ? 0 : s1 - s0);
        if (a.name_off) {
            const uint64_t o0 = a.name_off[r], o1 = a.name_off[r + 1];
            bad += o0 > o1;
            if (r + 1 == a.n_rec) bad += o1 > a.names_len;
            size += o0 > o1 ? 0 : o1 - o0;
        }
    }
    fasta_out_block_scan(a, block, p, size, bad);
}

// Where text position `at` lies in the chunk that begins at cx: 0 in front of it, 16 behind it.
__device__ __forceinline__ int fastq_out_rel(uint64_t at, int64_t cx) {
    const int64_t v = (int64_t)at - cx;
    return v < 0 ? 0 : (v > 16 ? 16 : (int)v);
}

// The bytes of a chunk below byte k, 0 <= k <= 16, as a mask.
__device__ __forceinline__ u32x4 fastq_out_below(int k) {
    u32x4 m;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int t = k - 4 * d;
        m[d] = (uint32_t)((1ull << (8 * (t < 0 ? 0 : (t > 4 ? 4 : t)))) - 1ull);
    }
    return m;
}

__device__ __forceinline__ u32x4 fastq_out_pick(u32x4 mask, u32x4 yes, u32x4 no) { return (yes & mask) | (no & ~mask); }

__device__ __forceinline__ u32x4 fastq_out_fill(uint32_t byte) {
    const uint32_t x = byte * 0x01010101u;
    return u32x4{x, x, x, x};
}

// src[i .. i + 16) of a buffer of n bytes at any address, zeros for the bytes outside [0, n): i may be negative or past n.  Five
// dwords on the 4-B grid src lies in and v_alignbyte when all five lie inside the buffer -- everywhere but within 20 bytes of its
// two ends, where the sixteen bytes are read one by one, each guarded.
__device__ __forceinline__ u32x4 fastq_out_bytes16(const uint8_t* src, uint64_t n, int64_t i) {
    const int64_t phase = (int64_t)(reinterpret_cast<uintptr_t>(src) & 3u);
    const int64_t j = i + phase, j4 = j & ~(int64_t)3;  // offsets from the 4-B aligned src - phase, where the buffer is [phase, phase + n)
    u32x4 r = {0, 0, 0, 0};
    if (j4 >= phase && j4 + 20 <= phase + (int64_t)n) {
        const uint32_t* grid = reinterpret_cast<const uint32_t*>(src - phase + j4);
        uint32_t d[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) d[k] = grid[k];
        const uint32_t sh = (uint32_t)j & 3u;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
    } else {
#pragma unroll
        for (int b = 0; b < 16; ++b)
            if (i + b >= 0 && i + b < (int64_t)n) r[b >> 2] |= (uint32_t)src[i + b] << (8 * (b & 3));
    }
    return r;
}

// pass 4
__global__ __launch_bounds__(kFastaOutBlock) void fastq_out_write(FastqOutArgs q, uint64_t first_tile) {
    const FastaOutArgs& a = q.f;
    const uint64_t tile = first_tile + blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t total = a.head[0];
    const int64_t limit = (int64_t)(total < a.cap ? total : a.cap);  // the bytes of text this call writes
    // the wave's bytes [w0, w1), as positions in the text
    const int64_t wx = (int64_t)(tile * kFastaOutTile + wave * kFastaOutWaveBytes) - (int64_t)a.phase;
    const int64_t w0 = wx < 0 ? 0 : wx, w1 = wx + (int64_t)kFastaOutWaveBytes < limit ? wx + (int64_t)kFastaOutWaveBytes : limit;
    if (w0 >= w1) return;  // the whole wave
    const uint64_t pieces = a.n_rec + 1;
    const uint64_t pf = fasta_out_find(a.off, 0, pieces, (uint64_t)w0);  // >= 1: the lead is empty
    // a record holds six bytes or more: off[pf + kFastaOutWaveBytes / 6 + 2] lies behind the wave's last byte
    const uint64_t most = pf + kFastaOutWaveBytes / 6 + 2;
    const uint64_t pl = a.off[pf + 1] > (uint64_t)(w1 - 1) ? pf : fasta_out_find(a.off, pf, most < pieces ? most : pieces, (uint64_t)(w1 - 1));
    const u32x4 feeds = fastq_out_fill(0x0Au);
    uint64_t p = pf;  // the piece of the lane's last chunk: its next one lies 1 KiB on
#pragma unroll 1
    for (int c = 0; c < kFastaOutChunks; ++c) {
        const int64_t cx = wx + (int64_t)(c * (int)(kFastaOutWaveBytes / kFastaOutChunks) + lane * 16);
        const int64_t c0 = cx < w0 ? w0 : cx, c1 = cx + 16 < w1 ? cx + 16 : w1;  // the chunk's bytes [c0, c1) of [cx, cx + 16)
        if (c0 >= c1) continue;
        uint64_t hi = pl + 1;  // off[p] <= c0 < off[hi]
        while (hi - p > 1) {
            const uint64_t mid = p + ((hi - p) >> 1);
            if (a.off[mid] <= (uint64_t)c0)
                p = mid;
            else
                hi = mid;
        }
        u32x4 out = {0, 0, 0, 0};
        for (uint64_t pc = p;; ++pc) {  // the records that overlap the chunk
            const uint64_t r = pc - 1;
            const uint64_t at = a.off[pc], end = a.off[pc + 1];
            const uint64_t s0 = a.rec_start[r], s1 = r + 1 < a.n_rec ? a.rec_start[r + 1] : a.len;
            const uint64_t o0 = a.name_off ? a.name_off[r] : 0, name = a.name_off ? a.name_off[r + 1] - o0 : 0;
            // where the segments begin in the text
            const uint64_t name_at = at + 1, letters_at = name_at + name + 1, plus_at = letters_at + (s1 - s0) + 1, qual_at = plus_at + 2;
            const int k_name = fastq_out_rel(name_at, cx), k_name_end = fastq_out_rel(letters_at - 1, cx), k_letters = fastq_out_rel(letters_at, cx);
            const int k_letters_end = fastq_out_rel(plus_at - 1, cx), k_plus = fastq_out_rel(plus_at, cx), k_plus_end = fastq_out_rel(plus_at + 1, cx);
            const int k_qual = fastq_out_rel(qual_at, cx), k_qual_end = fastq_out_rel(end - 1, cx);
            u32x4 v = feeds;  // the last line feed, and under every layer the line feeds in front of it
            if (k_qual < k_qual_end)  // byte i of the chunk is quality s0 + (cx + i - qual_at)
                v = fastq_out_pick(fastq_out_below(k_qual_end), fastq_out_bytes16(q.qual, a.len, (int64_t)s0 + (cx - (int64_t)qual_at)), v);
            v = fastq_out_pick(fastq_out_below(k_qual), feeds, v);
            v = fastq_out_pick(fastq_out_below(k_plus_end), fastq_out_fill(0x2Bu), v);
            v = fastq_out_pick(fastq_out_below(k_plus), feeds, v);
            if (k_letters < k_letters_end) {
                // byte i of the chunk is base g + i.  g < 0 when the letters begin inside the chunk less than that many bases
                // behind base 0: the codes of base 0 on are moved up; otherwise the bases in front of s0 sit under the mask
                const int64_t g = (int64_t)s0 + (cx - (int64_t)letters_at);
                const uint64_t g0 = g < 0 ? 0 : (uint64_t)g, wi = g0 >> 5;
                const uint64_t lo = wi < a.words ? a.bits[wi] : 0, up = wi + 1 < a.words ? a.bits[wi + 1] : 0;
                const uint32_t codes = (uint32_t)funnel64(lo, up, 2 * (uint32_t)(g0 & 31u)) << (g < 0 ? 2 * (uint32_t)(-g) : 0u);
                v = fastq_out_pick(fastq_out_below(k_letters_end), dec4(codes), v);
            }
            v = fastq_out_pick(fastq_out_below(k_letters), feeds, v);
            if (k_name < k_name_end)
                v = fastq_out_pick(fastq_out_below(k_name_end), fastq_out_bytes16(a.names, a.names_len, (int64_t)o0 + (cx - (int64_t)name_at)), v);
            v = fastq_out_pick(fastq_out_below(k_name), fastq_out_fill(0x40u), v);
            out = fastq_out_pick(fastq_out_below(fastq_out_rel(end, cx)) & ~fastq_out_below(fastq_out_rel(at, cx)), v, out);
            if (end >= (uint64_t)c1) break;  // off[R + 1] is the total, and c1 lies at or in front of it
        }
        uint8_t* dst = a.base + (uint64_t)(cx + (int64_t)a.phase);
        if (c1 - c0 == 16) {
            *reinterpret_cast<u32x4*>(dst) = out;
        } else {  // one of the text's two ends, or the text_cap cut
            const int i0 = (int)(c0 - cx), i1 = (int)(c1 - cx);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i >= i0 && i < i1) dst[i] = (uint8_t)(out[i >> 2] >> (8 * (i & 3)));
        }
    }
}

}  // namespace cnt
