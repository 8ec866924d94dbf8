// find_abi.inc -- C-ABI entry points of approximate pattern search (include/cute_nt.h, "pattern search"): the scratch query
// cnt_find_pattern_work_bytes, cnt_find_pattern_dev (enqueue-only on a caller stream: three kernels, no allocation, no
// synchronisation, capturable in a graph) and cnt_find_pattern (host tier: cute_nt.hip's host_call, staged through DevCtx::d_aux,
// or in place when the caller's input and outputs are pinned).  The scratch layout, the scan, the common argument checks and the
// host tier are counted_output.hpp's.  Included at the end of cute_nt.hip, behind minimizer_abi.inc.
#include "find_kernels.hpp"

namespace {

static_assert(CNT_FIND_REVERSE == kFindReverse, "the header's constant is the kernels'");

uint64_t find_windows(size_t len, unsigned k) { return len >= k ? (uint64_t)len - k + 1 : 0; }

// scratch: the counted output's (counted_output.hpp), one tile per kFindTile windows
uint64_t find_work_bytes(uint64_t m) { return counted_scratch_bytes((m + kFindTile - 1) / kFindTile); }

// bit 2j set for every set bit j < 32 of x
uint64_t find_spread(uint32_t x) {
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

// the reverse complement of k codes packed in the low 2k bits (kmer_finish's, on the host)
uint64_t find_revcomp(uint64_t fwd, unsigned k) {
    uint64_t x = fwd ^ 0xAAAAAAAAAAAAAAAAull, r = 0;
    for (unsigned j = 0; j < k; ++j) r |= ((x >> (2 * j)) & 3ull) << (2 * (k - 1 - j));
    return r;
}

// the argument checks both tiers share, before any device work; *m = the windows, *most = the most hits there can be.
// CNT_OK with m = 0: nothing to compute.
int find_args(const void* bits, size_t len, uint64_t pattern, unsigned k, uint32_t wildcards, unsigned max_mismatches, unsigned flags,
              const void* pos, const void* info, size_t out_cap, const void* count, uint64_t* m, uint64_t* most) {
    if (k == 0 || k > 32 || max_mismatches > k || (flags & ~CNT_FIND_BOTH_STRANDS)) return CNT_EINVAL;
    if (k < 32 && ((pattern >> (2 * k)) || (wildcards >> k))) return CNT_EINVAL;
    *m = find_windows(len, k);
    *most = (flags & CNT_FIND_BOTH_STRANDS) ? 2 * *m : *m;
    if (*m == 0) return CNT_OK;
    return counted_args(bits, len, {{pos, true}, {info, false}}, *most, out_cap, count);
}

}  // namespace

extern "C" {

int cnt_find_pattern_work_bytes(size_t len, unsigned k, size_t* bytes) {
    if (!bytes || k == 0 || k > 32) return CNT_EINVAL;
    *bytes = find_work_bytes(find_windows(len, k));
    return CNT_OK;
}

int cnt_find_pattern_dev(const void* d_bits, size_t len, uint64_t pattern, unsigned k, uint32_t wildcards, unsigned max_mismatches, unsigned flags,
                         void* d_pos, void* d_info, size_t out_cap, void* d_count, void* d_work, size_t work_bytes, void* stream) {
    uint64_t m = 0, most = 0;
    CNT_TRY(find_args(d_bits, len, pattern, k, wildcards, max_mismatches, flags, d_pos, d_info, out_cap, d_count, &m, &most));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (m == 0) return counted_empty_dev(d_count, s);
    CNT_TRY(counted_work(d_work, work_bytes, find_work_bytes(m), d_bits, len, {d_pos, d_info}, most, out_cap, d_count));
    const uint64_t n_tiles = (m + kFindTile - 1) / kFindTile;
    const CountedScratch work = counted_carve(d_work, n_tiles);
    const uint8_t* in = static_cast<const uint8_t*>(d_bits);
    uint64_t* pos = static_cast<uint64_t*>(d_pos);
    uint64_t* info = static_cast<uint64_t*>(d_info);
    const uint32_t used = k < 32 ? (1u << k) - 1u : ~0u, care = ~wildcards & used;
    uint32_t rcare = 0;  // wildcards' bit j = wildcards bit k-1-j
    for (unsigned j = 0; j < k; ++j) rcare |= ((care >> (k - 1 - j)) & 1u) << j;
    const FindPattern p = {pattern, find_spread(care), find_revcomp(pattern, k), find_spread(rcare), (uint32_t)max_mismatches};
    const uint64_t words = cnt_words_for(len);
    const bool wide = k > 16, both = (flags & CNT_FIND_BOTH_STRANDS) != 0;
    static const FindKernel kCount[4] = {find_count_k16, find_count_k16_both, find_count_k32, find_count_k32_both};
    static const FindKernel kWrite[4] = {find_write_k16, find_write_k16_both, find_write_k32, find_write_k32_both};
    const int which = (wide ? 2 : 0) + (both ? 1 : 0);
    split_launches(n_tiles, kFindBlock, [&](uint64_t t, uint64_t n) {
        hipLaunchKernelGGL(kCount[which], dim3((unsigned)n), dim3(kFindBlock), 0, s, in, words, m, p, t, work.counts, work.offs, pos, info, (uint64_t)out_cap);
    });
    counted_scan_enqueue(work, n_tiles, d_count, s);
    split_launches(n_tiles, kFindBlock, [&](uint64_t t, uint64_t n) {
        hipLaunchKernelGGL(kWrite[which], dim3((unsigned)n), dim3(kFindBlock), 0, s, in, words, m, p, t, work.counts, work.offs, pos, info, (uint64_t)out_cap);
    });
    return hip_rc(hipGetLastError());
}

int cnt_find_pattern(const uint64_t* bits, size_t len, uint64_t pattern, unsigned k, uint32_t wildcards, unsigned max_mismatches, unsigned flags,
                     uint64_t* pos, uint64_t* info, size_t out_cap, uint64_t* count) {
    uint64_t m = 0, most = 0;
    CNT_TRY(find_args(bits, len, pattern, k, wildcards, max_mismatches, flags, pos, info, out_cap, count, &m, &most));
    if (m == 0) return counted_empty(count);
    const size_t work_bytes = find_work_bytes(m);
    return counted_host_call(bits, len, {pos, info}, most, out_cap, count, work_bytes,
                             [&](void* const* d, size_t cap, void* d_count, void* d_work, hipStream_t s) {
                                 return cnt_find_pattern_dev(d[0], len, pattern, k, wildcards, max_mismatches, flags, d[1], d[2], cap, d_count, d_work,
                                                             work_bytes, s);
                             });
}

}  // extern "C"
