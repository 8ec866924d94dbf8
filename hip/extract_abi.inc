// extract_abi.inc -- C-ABI entry points of region extraction (include/cute_nt.h, "region extraction"): cnt_subseq_dev and
// cnt_extract_dev (enqueue-only on a caller stream: no allocation, no synchronisation, no scratch, capturable in a graph) and
// cnt_subseq / cnt_extract (host tier: cute_nt.hip's host_call, staged through DevCtx::d_aux, or in place when the caller's
// buffers are pinned).  Included at the end of cute_nt.hip, behind find_abi.inc.
#include "extract_kernels.hpp"

namespace {

static_assert(CNT_EXTRACT_REVCOMP == kExtractRevcomp, "the header's constant is the kernels'");

// the argument checks both tiers share, before any device work, for n regions of region_len nucleotides; *rec_words = R.
// The caller has dealt with empty work (n == 0 or region_len == 0) and with an unknown flag.
int extract_args(const void* bits, size_t len, const void* start, bool want_start, const void* info, size_t n, size_t region_len, const void* out,
                 size_t out_words, const void* rejected, size_t* rec_words) {
    if (!bits || !out || !aligned(bits, 8) || !aligned(out, 8) || (want_start && (!start || !aligned(start, 8))) || (info && !aligned(info, 8)) ||
        (rejected && !aligned(rejected, 8)))
        return CNT_EINVAL;
    const size_t R = cnt_words_for(region_len);
    if (n > SIZE_MAX / 8 / R || out_words < n * R) return CNT_ECAP;  // n * R words, and their bytes, fit a size_t
    if (R / kExtractTileWords > 0x7FFFFFFFu) return CNT_EINVAL;      // a record's tile index is 32 bits wide (2^45 nt)
    const size_t out_bytes = n * R * 8;
    if (overlaps(out, out_bytes, bits, cnt_words_for(len) * 8) || (want_start && overlaps(out, out_bytes, start, n * 8)) ||
        (info && overlaps(out, out_bytes, info, n * 8)))
        return CNT_EINVAL;
    // the counter of rejected regions is written too
    if (rejected && (overlaps(rejected, 8, out, out_bytes) || overlaps(rejected, 8, bits, cnt_words_for(len) * 8) ||
                     (want_start && overlaps(rejected, 8, start, n * 8)) || (info && overlaps(rejected, 8, info, n * 8))))
        return CNT_EINVAL;
    *rec_words = R;
    return CNT_OK;
}

// the launches of a call: the tiles of whole runs of 512 words per record (forward and / or reversed: with info[] both kernels
// walk every tile and each takes the records of its own orientation), then the word kernel on what is left of every record;
// `head` = words of the one record of cnt_subseq_dev in front of the first 128-B line of its output
int extract_launch(const ExtractArgs& a, uint64_t n, uint64_t head, hipStream_t s) {
    const uint64_t R = a.rec_words;
    const uint64_t tiles = (R - head) / kExtractTileWords;  // per record
    if (tiles) {
        const bool fwd = a.info || !a.rev, rev = a.info || a.rev;
        split_launches(n * tiles, kExtractBlock, [&](uint64_t first, uint64_t count) {
            const uint64_t i_first = first / tiles;
            const uint32_t t_first = (uint32_t)(first % tiles);
            if (fwd) hipLaunchKernelGGL(extract_tiles_fwd, dim3((unsigned)count), dim3(kExtractBlock), 0, s, a, head, (uint32_t)tiles, i_first, t_first);
            if (rev) hipLaunchKernelGGL(extract_tiles_rev, dim3((unsigned)count), dim3(kExtractBlock), 0, s, a, head, (uint32_t)tiles, i_first, t_first);
        });
    }
    auto word_kernel = [&](uint64_t j0, uint64_t j1) {  // words [j0, j1) of every record: fewer than 512
        const uint64_t w = j1 - j0, total = n * w;
        split_launches((total + kExtractBlock - 1) / kExtractBlock, kExtractBlock, [&](uint64_t first, uint64_t count) {
            const uint64_t f = first * kExtractBlock;
            hipLaunchKernelGGL(extract_words, dim3((unsigned)count), dim3(kExtractBlock), 0, s, a, j0, (uint32_t)w, f / w, (uint32_t)(f % w), total - f);
        });
    };
    if (head) word_kernel(0, head);
    if (head + tiles * kExtractTileWords < R) word_kernel(head + tiles * kExtractTileWords, R);
    return hip_rc(hipGetLastError());
}

}  // namespace

extern "C" {

int cnt_extract_dev(const void* d_bits, size_t len, const void* d_start, const void* d_info, size_t n, size_t region_len, unsigned flags,
                    void* d_out, size_t out_words, void* d_rejected, void* stream) {
    if (flags & ~CNT_EXTRACT_REVCOMP) return CNT_EINVAL;
    if (n == 0 || region_len == 0) return CNT_OK;
    size_t R = 0;
    CNT_TRY(extract_args(d_bits, len, d_start, true, d_info, n, region_len, d_out, out_words, d_rejected, &R));
    const ExtractArgs a = {static_cast<const uint8_t*>(d_bits), cnt_words_for(len), len, static_cast<const uint64_t*>(d_start),
                           static_cast<const uint64_t*>(d_info), 0, region_len, R, (flags & CNT_EXTRACT_REVCOMP) ? 1u : 0u,
                           static_cast<uint8_t*>(d_out), static_cast<unsigned long long*>(d_rejected)};
    return extract_launch(a, n, 0, static_cast<hipStream_t>(stream));  // no head: records start wherever i * R puts them
}

int cnt_subseq_dev(const void* d_bits, size_t len, size_t start, size_t sub_len, unsigned flags, void* d_out, size_t out_words, void* stream) {
    if (flags & ~CNT_EXTRACT_REVCOMP) return CNT_EINVAL;
    if (sub_len == 0) return CNT_OK;
    if (start > len || sub_len > len - start) return CNT_EINVAL;  // host-known bounds: an error, not a rejected region
    size_t R = 0;
    CNT_TRY(extract_args(d_bits, len, nullptr, false, nullptr, 1, sub_len, d_out, out_words, nullptr, &R));
    const ExtractArgs a = {static_cast<const uint8_t*>(d_bits), cnt_words_for(len), len, nullptr, nullptr, start, sub_len, R,
                           (flags & CNT_EXTRACT_REVCOMP) ? 1u : 0u, static_cast<uint8_t*>(d_out), nullptr};
    // head: output words until the stores sit on a 128-B line (word kernel), as cnt_reverse_complement_dev
    uint64_t head = ((128 - (reinterpret_cast<uintptr_t>(d_out) & 127)) & 127) >> 3;
    if (R < head + kExtractTileWords) head = 0;  // no tile behind it
    return extract_launch(a, 1, head, static_cast<hipStream_t>(stream));
}

int cnt_extract(const uint64_t* bits, size_t len, const uint64_t* start, const uint64_t* info, size_t n, size_t region_len, unsigned flags,
                uint64_t* out, size_t out_words, uint64_t* rejected) {
    if (flags & ~CNT_EXTRACT_REVCOMP) return CNT_EINVAL;
    if (n == 0 || region_len == 0) {
        if (rejected) *rejected = 0;
        return CNT_OK;
    }
    size_t R = 0;
    CNT_TRY(extract_args(bits, len, start, true, info, n, region_len, out, out_words, rejected, &R));
    uint64_t count = 0;
    CNT_TRY(host_call({{bits, cnt_words_for(len) * 8, Dir::in}, {start, n * 8, Dir::in}, {info, n * 8, Dir::in}, {out, n * R * 8, Dir::out}}, 16, &count,
                      true, [&](void* const* d, void* aux, hipStream_t s) {  // aux: the device count of rejected regions, zeroed
                          return cnt_extract_dev(d[0], len, d[1], d[2], n, region_len, flags, d[3], n * R, aux, s);
                      }));
    if (rejected) *rejected = count;
    return CNT_OK;
}

int cnt_subseq(const uint64_t* bits, size_t len, size_t start, size_t sub_len, unsigned flags, uint64_t* out, size_t out_words) {
    if (flags & ~CNT_EXTRACT_REVCOMP) return CNT_EINVAL;
    if (sub_len == 0) return CNT_OK;
    if (start > len || sub_len > len - start) return CNT_EINVAL;
    size_t R = 0;
    CNT_TRY(extract_args(bits, len, nullptr, false, nullptr, 1, sub_len, out, out_words, nullptr, &R));
    return host_call({{bits, cnt_words_for(len) * 8, Dir::in}, {out, R * 8, Dir::out}}, 0, nullptr, false,
                     [&](void* const* d, void*, hipStream_t s) { return cnt_subseq_dev(d[0], len, start, sub_len, flags, d[1], R, s); });
}

}  // extern "C"
