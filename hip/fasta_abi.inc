// fasta_abi.inc -- C-ABI entry points of the FASTA encode (include/cute_nt.h, "text formats: FASTA"): the scratch query
// cnt_fasta_to_bits_work_bytes, cnt_fasta_to_bits_dev (enqueue-only on a caller stream: four passes, no allocation, no
// synchronisation, capturable in a graph) and cnt_fasta_to_bits (host tier: cute_nt.hip's host_call in its long form, which
// brings the three counts back and sizes the record arrays by the second).  Included at the end of cute_nt.hip, behind
// window_count_abi.inc.
//
// Pass order of cnt_fasta_to_bits_dev (fasta_kernels.hpp): fasta_summary, fasta_scan, hpc_zero_edges, fasta_write.
#include "fasta_kernels.hpp"

namespace {

constexpr unsigned kFastaFlags = CNT_STRICT_LUT | CNT_ALLOW_N;
static_assert(CNT_FASTA_N == 0 && CNT_FASTA_RECORDS == 1 && CNT_FASTA_INVALID == 2, "fasta_scan stores the totals in this order");

// the most tiles a text of len bytes takes, at any address: its first tile begins up to 15 bytes in front of it
uint64_t fasta_tiles_most(size_t len) { return len ? ((uint64_t)len + 15 + kFastaTile - 1) / kFastaTile : 0; }

// The scratch: counted_output.hpp's two regions for the kept bytes, the same again for the records, one u64 of summary and one
// byte of carry per tile of whole groups.  Laid out for fasta_tiles_most(len) tiles, so that the query needs no address.
size_t fasta_scratch_bytes(uint64_t tiles) {
    if (!tiles) return 0;
    const uint64_t groups = (tiles + kCountedGroup - 1) / kCountedGroup;
    return 2 * counted_scratch_bytes(tiles) + groups * kCountedGroup * (8 + 1);
}
struct FastaScratch {
    CountedScratch kept, rec;
    uint64_t* sums;
    uint8_t* carry;
};
FastaScratch fasta_carve(void* d_work, uint64_t tiles) {
    const uint64_t groups = (tiles + kCountedGroup - 1) / kCountedGroup;
    FastaScratch w;
    w.kept = counted_carve(d_work, tiles);
    w.rec = counted_carve(w.kept.behind, tiles);
    w.sums = static_cast<uint64_t*>(w.rec.behind);
    w.carry = reinterpret_cast<uint8_t*>(w.sums + groups * kCountedGroup);
    return w;
}

// The argument checks both tiers share, before any device work, in the header's order (1 .. 6); *cap and *rcap = the most codes
// and records that can be written, which size the footprints.  CNT_OK with len == 0: nothing to compute.
int fasta_args(const void* text, size_t len, unsigned flags, const void* out, size_t out_cap, const void* rec_text, const void* rec_start, size_t rec_cap,
               const void* counts, size_t* cap, size_t* rcap) {
    if (flags & ~kFastaFlags) return CNT_EINVAL;
    *cap = std::min(len, out_cap);
    *rcap = std::min(len, rec_cap);
    if (len == 0) return CNT_OK;
    if (!text || !out || !counts) return CNT_EINVAL;
    if (!aligned(out, 8) || !aligned(counts, 8) || !aligned(rec_text, 8) || !aligned(rec_start, 8)) return CNT_EINVAL;
    if (!rec_text != !rec_start) return CNT_EINVAL;
    const void* p[5] = {text, out, rec_text, rec_start, counts};
    const size_t bytes[5] = {len, cnt_words_for(*cap) * 8, rec_text ? *rcap * 8 : 0, rec_start ? *rcap * 8 : 0, 24};
    for (int i = 0; i < 5; ++i)  // the text is the one buffer that is only read
        for (int j = i + 1; j < 5; ++j)
            if (overlaps(p[i], bytes[i], p[j], bytes[j])) return CNT_EINVAL;
    return CNT_OK;
}

}  // namespace

extern "C" {

int cnt_fasta_to_bits_work_bytes(size_t text_len, size_t* bytes) {
    if (!bytes) return CNT_EINVAL;
    *bytes = fasta_scratch_bytes(fasta_tiles_most(text_len));
    return CNT_OK;
}

int cnt_fasta_to_bits_dev(const void* d_text, size_t text_len, unsigned flags, void* d_out, size_t out_cap, void* d_rec_text, void* d_rec_start,
                          size_t rec_cap, void* d_counts, void* d_work, size_t work_bytes, void* stream) {
    size_t cap = 0, rcap = 0;
    CNT_TRY(fasta_args(d_text, text_len, flags, d_out, out_cap, d_rec_text, d_rec_start, rec_cap, d_counts, &cap, &rcap));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (text_len == 0) return d_counts ? hip_rc(hipMemsetAsync(d_counts, 0, 24, s)) : CNT_OK;
    const uint64_t most = fasta_tiles_most(text_len);
    const size_t need = fasta_scratch_bytes(most);  // the scratch at the query's size, against everything else of the call
    if (work_bytes < need || !d_work) return CNT_EINVAL;
    if (overlaps(d_work, need, d_text, text_len) || overlaps(d_work, need, d_out, cnt_words_for(cap) * 8) ||
        overlaps(d_work, need, d_rec_text, d_rec_text ? rcap * 8 : 0) || overlaps(d_work, need, d_rec_start, d_rec_start ? rcap * 8 : 0) ||
        overlaps(d_work, need, d_counts, 24))
        return CNT_EINVAL;
    const FastaScratch work = fasta_carve(d_work, most);
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(d_text) & 15u);
    const uint64_t n_tiles = ((uint64_t)text_len + phase + kFastaTile - 1) / kFastaTile;  // <= most
    const FastaArgs a = {static_cast<const uint8_t*>(d_text) - phase, phase, text_len, n_tiles, work.sums, work.carry, work.kept.counts, work.rec.counts,
                         work.kept.offs, work.rec.offs, static_cast<uint64_t*>(d_out), static_cast<uint64_t*>(d_rec_text), static_cast<uint64_t*>(d_rec_start),
                         cap, d_rec_text ? rcap : 0, static_cast<uint64_t*>(d_counts)};
    void (*const summary)(FastaArgs, uint64_t) = flags & CNT_ALLOW_N ? fasta_summary_n : fasta_summary;
    split_launches(n_tiles, kFastaBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(summary, dim3((unsigned)n), dim3(kFastaBlock), 0, s, a, t); });
    hipLaunchKernelGGL(fasta_scan, dim3(1), dim3(kFastaScanBlock), 0, s, a);
    const bool rec = d_rec_text && rcap;
    if (cap || rec) {
        if (cap) {
            // hpc_zero_edges reads the tiles, their counts and offsets, out and out_cap, one lane per tile
            const HpcArgs h = {nullptr, 0, 0, n_tiles, work.kept.counts, work.kept.offs, a.out, nullptr, cap};
            split_launches((n_tiles + kHpcBlock - 1) / kHpcBlock, kHpcBlock,
                           [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(hpc_zero_edges, dim3((unsigned)n), dim3(kHpcBlock), 0, s, h, t); });
        }
        void (*const write)(FastaArgs, uint64_t) =
            flags & CNT_STRICT_LUT ? (rec ? fasta_write_lut_rec : fasta_write_lut) : (rec ? fasta_write_rec : fasta_write);
        split_launches(n_tiles, kFastaBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(write, dim3((unsigned)n), dim3(kFastaBlock), 0, s, a, t); });
    }
    return hip_rc(hipGetLastError());
}

int cnt_fasta_to_bits(const uint8_t* text, size_t text_len, unsigned flags, uint64_t* out, size_t out_cap, uint64_t* rec_text, uint64_t* rec_start,
                      size_t rec_cap, uint64_t counts[3]) {
    size_t cap = 0, rcap = 0;
    CNT_TRY(fasta_args(text, text_len, flags, out, out_cap, rec_text, rec_start, rec_cap, counts, &cap, &rcap));
    if (text_len == 0) {
        if (counts) counts[0] = counts[1] = counts[2] = 0;
        return CNT_OK;
    }
    const size_t work_bytes = fasta_scratch_bytes(fasta_tiles_most(text_len));
    // out travels whole (a 32nd of a record array per entry); the record arrays in their first R entries
    const HostBuf b[4] = {{text, text_len, Dir::in}, {out, cnt_words_for(cap) * 8, Dir::out}, {rec_text, rcap * 8, Dir::counted}, {rec_start, rcap * 8, Dir::counted}};
    uint64_t got[3] = {};
    CNT_TRY(host_call(b, 24 + work_bytes, got, 3, CNT_FASTA_RECORDS, false, [&](void* const* d, void* aux, hipStream_t s) {  // aux: the device counts, then the scratch
        return cnt_fasta_to_bits_dev(d[0], text_len, flags, d[1], cap, d[2], d[3], rcap, aux, static_cast<uint8_t*>(aux) + 24, work_bytes, s);
    }));
    counts[0] = got[0];
    counts[1] = got[1];
    counts[2] = got[2];
    return got[0] > out_cap || (rec_text && got[1] > rec_cap) ? CNT_ECAP : CNT_OK;
}

}  // extern "C"
