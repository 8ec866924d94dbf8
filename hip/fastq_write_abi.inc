// fastq_write_abi.inc -- C-ABI entry points of the FASTQ write (include/cute_nt.h, "text formats: FASTQ write"): the host-side
// bound cnt_bits_to_fastq_bound, the scratch query cnt_bits_to_fastq_work_bytes, cnt_bits_to_fastq_dev (enqueue-only on a caller
// stream: four passes, no allocation, no synchronisation, capturable in a graph) and cnt_bits_to_fastq (host tier: cute_nt.hip's
// host_call in its long form, which brings the two counts back).  Included at the end of cute_nt.hip, behind fasta_write_abi.inc,
// whose scratch layout, block count and record limit it shares.
//
// Pass order of cnt_bits_to_fastq_dev (fastq_write_kernels.hpp): fastq_out_sizes, then the FASTA writer's fasta_out_scan and
// fasta_out_offsets as they are, then fastq_out_write.
#include "fastq_write_kernels.hpp"

namespace {

static_assert(CNT_FASTQ_OUT_TEXT == CNT_FASTA_OUT_TEXT && CNT_FASTQ_OUT_MALFORMED == CNT_FASTA_OUT_MALFORMED, "fasta_out_scan stores the counts in this order");

bool fastq_out_bound(size_t len, size_t n_rec, size_t names_len, size_t* bytes) {
    if (2 * len / 2 != len || 6 * n_rec / 6 != n_rec) return false;
    size_t b = 2 * len;
    for (size_t part : {names_len, 6 * n_rec}) {
        if (b + part < b) return false;
        b += part;
    }
    *bytes = b;
    return true;
}

// what a call reads and writes, at the header's extents
struct FastqOutBufs {
    const void* p[8];
    size_t bytes[8];
};
constexpr int kFastqOutWritten = 3;  // text, rec_text and counts come first

// The argument checks both tiers share, before any device work, in the header's order (1 .. 7); *foot = the footprint of the
// text.  *empty: nothing to compute.
int fastq_out_args(const void* bits, size_t len, const void* qual, const void* rec_start, size_t n_rec, const void* names, size_t names_len, const void* name_off,
                   unsigned flags, const void* text, size_t text_cap, const void* rec_text, const void* counts, size_t* foot, bool* empty, FastqOutBufs* bufs) {
    if (flags) return CNT_EINVAL;
    *empty = n_rec == 0;
    *foot = 0;
    if (*empty) return CNT_OK;
    if (!text || !counts || !rec_start || ((!bits || !qual) && len)) return CNT_EINVAL;
    if (!aligned(bits, 8) || !aligned(rec_start, 8) || !aligned(name_off, 8) || !aligned(rec_text, 8) || !aligned(counts, 8)) return CNT_EINVAL;
    if (!names != !name_off) return CNT_EINVAL;
    size_t bound = 0;
    if (!fastq_out_bound(len, n_rec, names_len, &bound) || n_rec > kFastaOutMostRecords) return CNT_EINVAL;
    *foot = std::min(bound, text_cap);
    *bufs = {{text, rec_text, counts, bits, qual, rec_start, names, name_off},
             {*foot, rec_text ? n_rec * 8 : 0, 16, cnt_words_for(len) * 8, len, n_rec * 8, names ? names_len : 0, name_off ? (n_rec + 1) * 8 : 0}};
    for (int i = 0; i < kFastqOutWritten; ++i)
        for (int j = i + 1; j < 8; ++j)
            if (overlaps(bufs->p[i], bufs->bytes[i], bufs->p[j], bufs->bytes[j])) return CNT_EINVAL;
    return CNT_OK;
}

}  // namespace

extern "C" {

int cnt_bits_to_fastq_bound(size_t len, size_t n_rec, size_t names_len, size_t* bytes) {
    if (!bytes) return CNT_EINVAL;
    return fastq_out_bound(len, n_rec, names_len, bytes) ? CNT_OK : CNT_EINVAL;
}

int cnt_bits_to_fastq_work_bytes(size_t n_rec, size_t* bytes) {
    if (!bytes || n_rec > kFastaOutMostRecords) return CNT_EINVAL;
    *bytes = fasta_out_scratch_bytes(n_rec);  // the lead, though empty, is a piece
    return CNT_OK;
}

int cnt_bits_to_fastq_dev(const void* d_bits, size_t len, const void* d_qual, const void* d_rec_start, size_t n_rec, const void* d_names, size_t names_len,
                          const void* d_name_off, unsigned flags, void* d_text, size_t text_cap, void* d_rec_text, void* d_counts, void* d_work, size_t work_bytes,
                          void* stream) {
    size_t foot = 0;
    bool empty = false;
    FastqOutBufs bufs;
    CNT_TRY(fastq_out_args(d_bits, len, d_qual, d_rec_start, n_rec, d_names, names_len, d_name_off, flags, d_text, text_cap, d_rec_text, d_counts, &foot, &empty,
                           &bufs));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (empty) return d_counts ? hip_rc(hipMemsetAsync(d_counts, 0, 16, s)) : CNT_OK;
    const size_t need = fasta_out_scratch_bytes(n_rec);  // the scratch at the query's size, against everything else of the call
    if (work_bytes < need || !d_work) return CNT_EINVAL;
    for (int i = 0; i < 8; ++i)
        if (overlaps(d_work, need, bufs.p[i], bufs.bytes[i])) return CNT_EINVAL;
    const uint64_t n_blocks = fasta_out_blocks(n_rec);
    uint64_t* head = reinterpret_cast<uint64_t*>((reinterpret_cast<uintptr_t>(d_work) + 7) & ~(uintptr_t)7);  // the scratch may sit at any byte
    uint64_t* off = head + 2;
    uint64_t* sums = off + n_rec + 2;
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(d_text) & 15u);
    const uint64_t n_tiles = ((uint64_t)foot + phase + kFastaOutTile - 1) / kFastaOutTile;
    const FastaOutArgs a = {static_cast<const uint64_t*>(d_bits), len, cnt_words_for(len), static_cast<const uint64_t*>(d_rec_start), n_rec,
                            static_cast<const uint8_t*>(d_names), static_cast<const uint64_t*>(d_name_off), names_len, 1,
                            static_cast<uint8_t*>(d_text) - phase, phase, text_cap, static_cast<uint64_t*>(d_rec_text), static_cast<uint64_t*>(d_counts),
                            head, off, sums, sums + n_blocks, n_blocks};
    const FastqOutArgs q = {a, static_cast<const uint8_t*>(d_qual)};
    split_launches(n_blocks, kFastaOutBlock,
                   [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(fastq_out_sizes, dim3((unsigned)n), dim3(kFastaOutBlock), 0, s, q, t); });
    hipLaunchKernelGGL(fasta_out_scan, dim3(1), dim3(kFastaOutScanBlock), 0, s, a);
    split_launches(n_blocks, kFastaOutBlock,
                   [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(fasta_out_offsets, dim3((unsigned)n), dim3(kFastaOutBlock), 0, s, a, t); });
    split_launches(n_tiles, kFastaOutBlock,
                   [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(fastq_out_write, dim3((unsigned)n), dim3(kFastaOutBlock), 0, s, q, t); });
    return hip_rc(hipGetLastError());
}

int cnt_bits_to_fastq(const uint64_t* bits, size_t len, const uint8_t* qual, const uint64_t* rec_start, size_t n_rec, const uint8_t* names, size_t names_len,
                      const uint64_t* name_off, unsigned flags, uint8_t* text, size_t text_cap, uint64_t* rec_text, uint64_t counts[2]) {
    size_t foot = 0;
    bool empty = false;
    FastqOutBufs bufs;
    CNT_TRY(fastq_out_args(bits, len, qual, rec_start, n_rec, names, names_len, name_off, flags, text, text_cap, rec_text, counts, &foot, &empty, &bufs));
    if (empty) {
        if (counts) counts[0] = counts[1] = 0;
        return CNT_OK;
    }
    const size_t work_bytes = fasta_out_scratch_bytes(n_rec);
    const HostBuf b[7] = {{bits, cnt_words_for(len) * 8, Dir::in}, {qual, len, Dir::in}, {rec_start, n_rec * 8, Dir::in}, {names, names_len, Dir::in},
                          {name_off, (n_rec + 1) * 8, Dir::in}, {text, foot, Dir::out}, {rec_text, n_rec * 8, Dir::out}};
    uint64_t got[2] = {}, seen[2] = {};
    bool malformed = false;
    // aux: the device counts, then the scratch.  A malformed table writes nothing: the counts are looked at here, behind the work,
    // and a refusal keeps host_call from copying a staged text and rec_text back over the caller's.
    const int rc = host_call(b, 16 + work_bytes, got, 2, 0, false, [&](void* const* d, void* aux, hipStream_t s) {
        CNT_TRY(cnt_bits_to_fastq_dev(d[0], len, d[1], d[2], n_rec, d[3], names_len, d[4], 0, d[5], text_cap, d[6], aux, static_cast<uint8_t*>(aux) + 16,
                                      work_bytes, s));
        CNT_TRY(hip_rc(hipMemcpyAsync(seen, aux, 16, hipMemcpyDeviceToHost, s)));
        CNT_TRY(hip_rc(hipStreamSynchronize(s)));
        malformed = seen[CNT_FASTQ_OUT_MALFORMED] != 0;
        return malformed ? CNT_EINVAL : CNT_OK;
    });
    if (malformed) {
        counts[CNT_FASTQ_OUT_TEXT] = 0;
        counts[CNT_FASTQ_OUT_MALFORMED] = seen[CNT_FASTQ_OUT_MALFORMED];
        return CNT_EINVAL;
    }
    CNT_TRY(rc);
    counts[0] = got[0];
    counts[1] = got[1];
    return got[CNT_FASTQ_OUT_TEXT] > text_cap ? CNT_ECAP : CNT_OK;
}

}  // extern "C"
