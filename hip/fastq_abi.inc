// fastq_abi.inc -- C-ABI entry points of the FASTQ encode (include/cute_nt.h, "text formats: FASTQ"): the scratch query
// cnt_fastq_to_bits_work_bytes, cnt_fastq_to_bits_dev (enqueue-only on a caller stream: six passes, no allocation, no
// synchronisation, capturable in a graph) and cnt_fastq_to_bits (host tier: cute_nt.hip's host_call in its long form, which
// brings the five counts back and sizes the three record arrays by the second).  Included at the end of cute_nt.hip, behind
// fasta_abi.inc.
//
// Pass order of cnt_fastq_to_bits_dev (fastq_kernels.hpp): fastq_lines, fastq_line_scan, fastq_count, fastq_scan, hpc_zero_edges,
// fastq_write.
#include "fastq_kernels.hpp"

namespace {

constexpr unsigned kFastqFlags = CNT_STRICT_LUT | CNT_ALLOW_N;
constexpr size_t kFastqCounts = 5 * 8;  // bytes of the counts
static_assert(CNT_FASTQ_N == 0 && CNT_FASTQ_RECORDS == 1 && CNT_FASTQ_INVALID == 2 && CNT_FASTQ_QUAL == 3 && CNT_FASTQ_MALFORMED == 4,
              "fastq_scan stores the totals in this order");

// The scratch: counted_output.hpp's two regions for the sequence bytes, for the quality bytes and for the records, and per tile
// of whole groups one u32 of line feeds, one u32 of flaws and one byte of carry.  Laid out for fasta_tiles_most(len) tiles, so
// that the query needs no address.
size_t fastq_scratch_bytes(uint64_t tiles) {
    if (!tiles) return 0;
    const uint64_t groups = (tiles + kCountedGroup - 1) / kCountedGroup;
    return 3 * counted_scratch_bytes(tiles) + groups * kCountedGroup * (4 + 4 + 1);
}
struct FastqScratch {
    CountedScratch seq, qual, rec;
    uint32_t *lines, *flaws;
    uint8_t* carry;
};
FastqScratch fastq_carve(void* d_work, uint64_t tiles) {
    const uint64_t groups = (tiles + kCountedGroup - 1) / kCountedGroup;
    FastqScratch w;
    w.seq = counted_carve(d_work, tiles);
    w.qual = counted_carve(w.seq.behind, tiles);
    w.rec = counted_carve(w.qual.behind, tiles);
    w.lines = static_cast<uint32_t*>(w.rec.behind);  // whole groups are 64 B: every region stays 16-B aligned
    w.flaws = w.lines + groups * kCountedGroup;
    w.carry = reinterpret_cast<uint8_t*>(w.flaws + groups * kCountedGroup);
    return w;
}

// the buffers of a call and their extents in bytes, for the overlap rule: the text is the one that is only read
struct FastqBufs {
    const void* p[7];
    size_t bytes[7];
};

// The argument checks both tiers share, before any device work, in the header's order (1 .. 6); *cap, *qcap and *rcap = the most
// codes, quality bytes and records that can be written, which size the footprints.  CNT_OK with len == 0: nothing to compute.
int fastq_args(const void* text, size_t len, unsigned flags, const void* out, size_t out_cap, const void* qual, size_t qual_cap, const void* rec_text,
               const void* rec_start, const void* rec_qual, size_t rec_cap, const void* counts, size_t* cap, size_t* qcap, size_t* rcap, FastqBufs* b) {
    if (flags & ~kFastqFlags) return CNT_EINVAL;
    *cap = std::min(len, out_cap);
    *qcap = std::min(len, qual_cap);
    *rcap = std::min(len, rec_cap);
    if (len == 0) return CNT_OK;
    if (!text || !out || !counts) return CNT_EINVAL;
    if (!aligned(out, 8) || !aligned(counts, 8) || !aligned(rec_text, 8) || !aligned(rec_start, 8) || !aligned(rec_qual, 8)) return CNT_EINVAL;
    if (!rec_text != !rec_start || !rec_text != !rec_qual) return CNT_EINVAL;
    const size_t rec_bytes = rec_text ? *rcap * 8 : 0;
    *b = {{text, out, qual, rec_text, rec_start, rec_qual, counts}, {len, cnt_words_for(*cap) * 8, qual ? *qcap : 0, rec_bytes, rec_bytes, rec_bytes, kFastqCounts}};
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            if (overlaps(b->p[i], b->bytes[i], b->p[j], b->bytes[j])) return CNT_EINVAL;
    return CNT_OK;
}

}  // namespace

extern "C" {

int cnt_fastq_to_bits_work_bytes(size_t text_len, size_t* bytes) {
    if (!bytes) return CNT_EINVAL;
    *bytes = fastq_scratch_bytes(fasta_tiles_most(text_len));
    return CNT_OK;
}

int cnt_fastq_to_bits_dev(const void* d_text, size_t text_len, unsigned flags, void* d_out, size_t out_cap, void* d_qual, size_t qual_cap, void* d_rec_text,
                          void* d_rec_start, void* d_rec_qual, size_t rec_cap, void* d_counts, void* d_work, size_t work_bytes, void* stream) {
    size_t cap = 0, qcap = 0, rcap = 0;
    FastqBufs b = {};
    CNT_TRY(fastq_args(d_text, text_len, flags, d_out, out_cap, d_qual, qual_cap, d_rec_text, d_rec_start, d_rec_qual, rec_cap, d_counts, &cap, &qcap, &rcap, &b));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (text_len == 0) return d_counts ? hip_rc(hipMemsetAsync(d_counts, 0, kFastqCounts, s)) : CNT_OK;
    const uint64_t most = fasta_tiles_most(text_len);
    const size_t need = fastq_scratch_bytes(most);  // the scratch at the query's size, against everything else of the call
    if (work_bytes < need || !d_work) return CNT_EINVAL;
    for (int i = 0; i < 7; ++i)
        if (overlaps(d_work, need, b.p[i], b.bytes[i])) return CNT_EINVAL;
    const FastqScratch work = fastq_carve(d_work, most);
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(d_text) & 15u);
    const uint64_t n_tiles = ((uint64_t)text_len + phase + kFastaTile - 1) / kFastaTile;  // <= most
    const bool rec = d_rec_text && rcap, qual = d_qual && qcap;
    const FastqArgs a = {static_cast<const uint8_t*>(d_text) - phase, phase, text_len, n_tiles, work.lines, work.carry, work.flaws,
                         work.seq.counts, work.qual.counts, work.rec.counts, work.seq.offs, work.qual.offs, work.rec.offs,
                         static_cast<uint64_t*>(d_out), static_cast<uint8_t*>(d_qual), static_cast<uint64_t*>(d_rec_text), static_cast<uint64_t*>(d_rec_start),
                         static_cast<uint64_t*>(d_rec_qual), cap, qual ? qcap : 0, rec ? rcap : 0, static_cast<uint64_t*>(d_counts)};
    split_launches(n_tiles, kFastaBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(fastq_lines, dim3((unsigned)n), dim3(kFastaBlock), 0, s, a, t); });
    hipLaunchKernelGGL(fastq_line_scan, dim3(1), dim3(kFastqScanBlock), 0, s, a);
    void (*const count)(FastqArgs, uint64_t) = flags & CNT_ALLOW_N ? fastq_count_n : fastq_count;
    split_launches(n_tiles, kFastaBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(count, dim3((unsigned)n), dim3(kFastaBlock), 0, s, a, t); });
    hipLaunchKernelGGL(fastq_scan, dim3(1), dim3(kFastqScanBlock), 0, s, a);
    if (cap || qual || rec) {
        if (cap) {
            // hpc_zero_edges reads the tiles, their counts and offsets, out and out_cap, one lane per tile
            const HpcArgs h = {nullptr, 0, 0, n_tiles, work.seq.counts, work.seq.offs, a.out, nullptr, cap};
            split_launches((n_tiles + kHpcBlock - 1) / kHpcBlock, kHpcBlock,
                           [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(hpc_zero_edges, dim3((unsigned)n), dim3(kHpcBlock), 0, s, h, t); });
        }
        static void (*const kWrite[8])(FastqArgs, uint64_t) = {fastq_write,     fastq_write_rec,     fastq_write_qual,     fastq_write_qual_rec,
                                                               fastq_write_lut, fastq_write_lut_rec, fastq_write_lut_qual, fastq_write_lut_qual_rec};
        void (*const write)(FastqArgs, uint64_t) = kWrite[(flags & CNT_STRICT_LUT ? 4 : 0) + (qual ? 2 : 0) + (rec ? 1 : 0)];
        split_launches(n_tiles, kFastaBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(write, dim3((unsigned)n), dim3(kFastaBlock), 0, s, a, t); });
    }
    return hip_rc(hipGetLastError());
}

int cnt_fastq_to_bits(const uint8_t* text, size_t text_len, unsigned flags, uint64_t* out, size_t out_cap, uint8_t* qual, size_t qual_cap, uint64_t* rec_text,
                      uint64_t* rec_start, uint64_t* rec_qual, size_t rec_cap, uint64_t counts[5]) {
    size_t cap = 0, qcap = 0, rcap = 0;
    FastqBufs fb = {};
    CNT_TRY(fastq_args(text, text_len, flags, out, out_cap, qual, qual_cap, rec_text, rec_start, rec_qual, rec_cap, counts, &cap, &qcap, &rcap, &fb));
    if (text_len == 0) {
        if (counts) std::fill(counts, counts + 5, (uint64_t)0);
        return CNT_OK;
    }
    const size_t work_bytes = fastq_scratch_bytes(fasta_tiles_most(text_len));
    // out and qual travel whole; the record arrays in their first R entries
    const HostBuf b[6] = {{text, text_len, Dir::in},           {out, cnt_words_for(cap) * 8, Dir::out}, {qual, qcap, Dir::out},
                          {rec_text, rcap * 8, Dir::counted}, {rec_start, rcap * 8, Dir::counted},     {rec_qual, rcap * 8, Dir::counted}};
    uint64_t got[5] = {};
    // aux: the device counts, then the scratch
    CNT_TRY(host_call(b, kFastqCounts + work_bytes, got, 5, CNT_FASTQ_RECORDS, false, [&](void* const* d, void* aux, hipStream_t s) {
        return cnt_fastq_to_bits_dev(d[0], text_len, flags, d[1], cap, d[2], qcap, d[3], d[4], d[5], rcap, aux, static_cast<uint8_t*>(aux) + kFastqCounts, work_bytes, s);
    }));
    std::copy(got, got + 5, counts);
    return got[CNT_FASTQ_N] > out_cap || (qual && got[CNT_FASTQ_QUAL] > qual_cap) || (rec_text && got[CNT_FASTQ_RECORDS] > rec_cap) ? CNT_ECAP : CNT_OK;
}

}  // extern "C"
