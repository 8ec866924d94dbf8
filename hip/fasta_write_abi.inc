// fasta_write_abi.inc -- C-ABI entry points of the FASTA write (include/cute_nt.h, "text formats: FASTA write"): the host-side
// bound cnt_bits_to_fasta_bound, the scratch query cnt_bits_to_fasta_work_bytes, cnt_bits_to_fasta_dev (enqueue-only on a caller
// stream: four passes, no allocation, no synchronisation, capturable in a graph) and cnt_bits_to_fasta (host tier: cute_nt.hip's
// host_call in its long form, which brings the two counts back).  Included at the end of cute_nt.hip, behind fastq_abi.inc.
//
// Pass order of cnt_bits_to_fasta_dev (fasta_write_kernels.hpp): fasta_out_sizes, fasta_out_scan, fasta_out_offsets,
// fasta_out_write.
#include "fasta_write_kernels.hpp"

namespace {

static_assert(CNT_FASTA_OUT_TEXT == 0 && CNT_FASTA_OUT_MALFORMED == 1, "fasta_out_scan stores the counts in this order");

constexpr size_t kFastaOutMostRecords = (size_t)1 << 48;  // keeps the scratch's size inside size_t

uint64_t fasta_out_blocks(size_t n_rec) { return ((uint64_t)n_rec + 1 + kFastaOutBlock - 1) / kFastaOutBlock; }

// The scratch: 8 bytes to bring it to an 8-B address, two words of head, n_rec + 2 offsets, two words per block of pieces.
size_t fasta_out_scratch_bytes(size_t n_rec) { return 8 + 8 * (2 + ((uint64_t)n_rec + 2) + 2 * fasta_out_blocks(n_rec)); }

bool fasta_out_bound(size_t len, size_t n_rec, size_t names_len, size_t width, size_t* bytes) {
    size_t b = len;
    const size_t parts[4] = {width ? len / width : 0, n_rec + 1, names_len, 2 * n_rec};
    if (n_rec + 1 == 0 || 2 * n_rec / 2 != n_rec) return false;
    for (size_t part : parts) {
        if (b + part < b) return false;
        b += part;
    }
    *bytes = b;
    return true;
}

// what a call reads and writes, at the header's extents
struct FastaOutBufs {
    const void* p[7];
    size_t bytes[7];
};
constexpr int kFastaOutWritten = 3;  // text, rec_text and counts come first

// The argument checks both tiers share, before any device work, in the header's order (1 .. 7); *foot = the footprint of the
// text.  *empty: nothing to compute.
int fasta_out_args(const void* bits, size_t len, const void* rec_start, size_t n_rec, const void* names, size_t names_len, const void* name_off, size_t width,
                   unsigned flags, const void* text, size_t text_cap, const void* rec_text, const void* counts, size_t* foot, bool* empty, FastaOutBufs* bufs) {
    if (flags) return CNT_EINVAL;
    *empty = len == 0 && n_rec == 0;
    *foot = 0;
    if (*empty) return CNT_OK;
    if ((!bits && len) || !text || !counts || (!rec_start && n_rec)) return CNT_EINVAL;
    if (!aligned(bits, 8) || !aligned(rec_start, 8) || !aligned(name_off, 8) || !aligned(rec_text, 8) || !aligned(counts, 8)) return CNT_EINVAL;
    if (!names != !name_off) return CNT_EINVAL;
    size_t bound = 0;
    if (!fasta_out_bound(len, n_rec, names_len, width, &bound) || n_rec > kFastaOutMostRecords) return CNT_EINVAL;
    *foot = std::min(bound, text_cap);
    *bufs = {{text, rec_text, counts, bits, rec_start, names, name_off},
             {*foot, rec_text ? n_rec * 8 : 0, 16, cnt_words_for(len) * 8, n_rec * 8, names ? names_len : 0, name_off ? (n_rec + 1) * 8 : 0}};
    for (int i = 0; i < kFastaOutWritten; ++i)
        for (int j = i + 1; j < 7; ++j)
            if (overlaps(bufs->p[i], bufs->bytes[i], bufs->p[j], bufs->bytes[j])) return CNT_EINVAL;
    return CNT_OK;
}

}  // namespace

extern "C" {

int cnt_bits_to_fasta_bound(size_t len, size_t n_rec, size_t names_len, size_t width, size_t* bytes) {
    if (!bytes) return CNT_EINVAL;
    return fasta_out_bound(len, n_rec, names_len, width, bytes) ? CNT_OK : CNT_EINVAL;
}

int cnt_bits_to_fasta_work_bytes(size_t n_rec, size_t* bytes) {
    if (!bytes || n_rec > kFastaOutMostRecords) return CNT_EINVAL;
    *bytes = fasta_out_scratch_bytes(n_rec);
    return CNT_OK;
}

int cnt_bits_to_fasta_dev(const void* d_bits, size_t len, const void* d_rec_start, size_t n_rec, const void* d_names, size_t names_len, const void* d_name_off,
                          size_t width, unsigned flags, void* d_text, size_t text_cap, void* d_rec_text, void* d_counts, void* d_work, size_t work_bytes,
                          void* stream) {
    size_t foot = 0;
    bool empty = false;
    FastaOutBufs bufs;
    CNT_TRY(fasta_out_args(d_bits, len, d_rec_start, n_rec, d_names, names_len, d_name_off, width, flags, d_text, text_cap, d_rec_text, d_counts, &foot, &empty,
                           &bufs));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (empty) return d_counts ? hip_rc(hipMemsetAsync(d_counts, 0, 16, s)) : CNT_OK;
    const size_t need = fasta_out_scratch_bytes(n_rec);  // the scratch at the query's size, against everything else of the call
    if (work_bytes < need || !d_work) return CNT_EINVAL;
    for (int i = 0; i < 7; ++i)
        if (overlaps(d_work, need, bufs.p[i], bufs.bytes[i])) return CNT_EINVAL;
    const uint64_t n_blocks = fasta_out_blocks(n_rec);
    uint64_t* head = reinterpret_cast<uint64_t*>((reinterpret_cast<uintptr_t>(d_work) + 7) & ~(uintptr_t)7);  // the scratch may sit at any byte
    uint64_t* off = head + 2;
    uint64_t* sums = off + n_rec + 2;
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(d_text) & 15u);
    const uint64_t n_tiles = ((uint64_t)foot + phase + kFastaOutTile - 1) / kFastaOutTile;
    // W == 0 and W > len are one line per body; so is max(len, 1), which keeps the kernels' W + 1 inside 2^36 + 1
    const uint64_t w = width == 0 || width > len ? std::max<uint64_t>(len, 1) : width;
    const FastaOutArgs a = {static_cast<const uint64_t*>(d_bits), len, cnt_words_for(len), static_cast<const uint64_t*>(d_rec_start), n_rec,
                            static_cast<const uint8_t*>(d_names), static_cast<const uint64_t*>(d_name_off), names_len, w,
                            static_cast<uint8_t*>(d_text) - phase, phase, text_cap, static_cast<uint64_t*>(d_rec_text), static_cast<uint64_t*>(d_counts),
                            head, off, sums, sums + n_blocks, n_blocks};
    split_launches(n_blocks, kFastaOutBlock,
                   [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(fasta_out_sizes, dim3((unsigned)n), dim3(kFastaOutBlock), 0, s, a, t); });
    hipLaunchKernelGGL(fasta_out_scan, dim3(1), dim3(kFastaOutScanBlock), 0, s, a);
    split_launches(n_blocks, kFastaOutBlock,
                   [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(fasta_out_offsets, dim3((unsigned)n), dim3(kFastaOutBlock), 0, s, a, t); });
    split_launches(n_tiles, kFastaOutBlock,
                   [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(fasta_out_write, dim3((unsigned)n), dim3(kFastaOutBlock), 0, s, a, t); });
    return hip_rc(hipGetLastError());
}

int cnt_bits_to_fasta(const uint64_t* bits, size_t len, const uint64_t* rec_start, size_t n_rec, const uint8_t* names, size_t names_len,
                      const uint64_t* name_off, size_t width, unsigned flags, uint8_t* text, size_t text_cap, uint64_t* rec_text, uint64_t counts[2]) {
    size_t foot = 0;
    bool empty = false;
    FastaOutBufs bufs;
    CNT_TRY(fasta_out_args(bits, len, rec_start, n_rec, names, names_len, name_off, width, flags, text, text_cap, rec_text, counts, &foot, &empty, &bufs));
    if (empty) {
        if (counts) counts[0] = counts[1] = 0;
        return CNT_OK;
    }
    const size_t work_bytes = fasta_out_scratch_bytes(n_rec);
    const HostBuf b[6] = {{bits, cnt_words_for(len) * 8, Dir::in}, {rec_start, n_rec * 8, Dir::in}, {names, names_len, Dir::in},
                          {name_off, (n_rec + 1) * 8, Dir::in}, {text, foot, Dir::out}, {rec_text, n_rec * 8, Dir::out}};
    uint64_t got[2] = {}, seen[2] = {};
    bool malformed = false;
    // aux: the device counts, then the scratch.  A malformed table writes nothing: the counts are looked at here, behind the work,
    // and a refusal keeps host_call from copying a staged text and rec_text back over the caller's.
    const int rc = host_call(b, 16 + work_bytes, got, 2, 0, false, [&](void* const* d, void* aux, hipStream_t s) {
        CNT_TRY(cnt_bits_to_fasta_dev(d[0], len, d[1], n_rec, d[2], names_len, d[3], width, 0, d[4], text_cap, d[5], aux, static_cast<uint8_t*>(aux) + 16,
                                      work_bytes, s));
        CNT_TRY(hip_rc(hipMemcpyAsync(seen, aux, 16, hipMemcpyDeviceToHost, s)));
        CNT_TRY(hip_rc(hipStreamSynchronize(s)));
        malformed = seen[CNT_FASTA_OUT_MALFORMED] != 0;
        return malformed ? CNT_EINVAL : CNT_OK;
    });
    if (malformed) {
        counts[CNT_FASTA_OUT_TEXT] = 0;
        counts[CNT_FASTA_OUT_MALFORMED] = seen[CNT_FASTA_OUT_MALFORMED];
        return CNT_EINVAL;
    }
    CNT_TRY(rc);
    counts[0] = got[0];
    counts[1] = got[1];
    return got[CNT_FASTA_OUT_TEXT] > text_cap ? CNT_ECAP : CNT_OK;
}

}  // extern "C"
