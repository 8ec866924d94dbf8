// orf_abi.inc -- C-ABI entry points of the open-reading-frame scan (include/cute_nt.h, "ORF scan"): the scratch query
// cnt_orfs_work_bytes, cnt_orfs_dev (enqueue-only on a caller stream: five passes, no allocation, no synchronisation, capturable
// in a graph) and cnt_orfs (host tier: cute_nt.hip's host_call, staged through DevCtx::d_aux, or in place when the caller's input
// and outputs are pinned).  The layout of counts and offs, the scan, the common argument checks and the host tier are
// counted_output.hpp's.  Included at the end of cute_nt.hip, behind translate_abi.inc.
#include "orf_kernels.hpp"

namespace {

static_assert(CNT_ORF_OPEN_END == kOrfOpenEnd && CNT_ORF_NO_STOP == kOrfNoStop, "the header's constants are the kernels'");

// the tiles of a call: the positions 0 .. len, the three closing bounds len-2 .. len among them
uint64_t orf_tiles(size_t len) { return len < 3 ? 0 : (uint64_t)len / kOrfTile + 1; }

// scratch: the counted output's (counted_output.hpp), and behind it sums, kOrfPairs u32 per tile, then carry, 2 * kOrfPairs u64
// per tile
uint64_t orf_work_bytes(uint64_t n_tiles) { return counted_scratch_bytes(n_tiles) + n_tiles * kOrfPairs * (4 + 2 * 8); }

// the set whose test on c is the test of `set` on rc3(c): the outer codes swapped, all three complemented
uint64_t orf_rc3(uint64_t set) {
    uint64_t r = 0;
    for (unsigned c = 0; c < 64; ++c) r |= ((set >> (((c >> 4) | (c & 0xCu) | ((c & 3u) << 4)) ^ 0x2Au)) & 1ull) << c;
    return r;
}

// the argument checks both tiers share, before any device work; *most = the most entries there can be.  CNT_OK with len < 3:
// nothing to compute.
int orf_args(const void* bits, size_t len, uint64_t stops, unsigned flags, const void* pos, const void* length, const void* info, size_t out_cap,
             const void* count, uint64_t* most) {
    if (stops == 0 || (flags & ~CNT_ORF_BOTH_STRANDS)) return CNT_EINVAL;
    *most = (flags & CNT_ORF_BOTH_STRANDS) ? 2 * (uint64_t)len : len;
    if (len < 3) return CNT_OK;
    return counted_args(bits, len, {{pos, true}, {length, true}, {info, false}}, *most, out_cap, count);
}

}  // namespace

extern "C" {

int cnt_orfs_work_bytes(size_t len, size_t* bytes) {
    if (!bytes) return CNT_EINVAL;
    *bytes = orf_work_bytes(orf_tiles(len));
    return CNT_OK;
}

int cnt_orfs_dev(const void* d_bits, size_t len, uint64_t stops, uint64_t starts, size_t min_len, unsigned flags, void* d_pos, void* d_length,
                 void* d_info, size_t out_cap, void* d_count, void* d_work, size_t work_bytes, void* stream) {
    uint64_t most = 0;
    CNT_TRY(orf_args(d_bits, len, stops, flags, d_pos, d_length, d_info, out_cap, d_count, &most));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (len < 3) return counted_empty_dev(d_count, s);
    const uint64_t n_tiles = orf_tiles(len);
    CNT_TRY(counted_work(d_work, work_bytes, orf_work_bytes(n_tiles), d_bits, len, {d_pos, d_length, d_info}, most, out_cap, d_count));
    const CountedScratch work = counted_carve(d_work, n_tiles);
    uint32_t* sums = static_cast<uint32_t*>(work.behind);
    uint64_t* carry = reinterpret_cast<uint64_t*>(sums + n_tiles * kOrfPairs);
    const bool both = (flags & CNT_ORF_BOTH_STRANDS) != 0;
    const OrfArgs a = {static_cast<const uint8_t*>(d_bits),
                       cnt_words_for(len),
                       len,
                       {stops, both ? orf_rc3(stops) : 0},
                       {starts, both ? orf_rc3(starts) : 0},
                       std::max<uint64_t>(min_len, 3),
                       n_tiles,
                       sums,
                       carry,
                       work.counts,
                       work.offs,
                       static_cast<uint64_t*>(d_pos),
                       static_cast<uint64_t*>(d_length),
                       static_cast<uint64_t*>(d_info),
                       out_cap};
    split_launches(n_tiles, kOrfBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(orf_summary, dim3((unsigned)n), dim3(kOrfBlock), 0, s, a, t); });
    hipLaunchKernelGGL(orf_carry, dim3(both ? kOrfPairs : 3), dim3(kOrfCarryBlock), 0, s, sums, carry, n_tiles);
    split_launches(n_tiles, kOrfBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(orf_count, dim3((unsigned)n), dim3(kOrfBlock), 0, s, a, t); });
    counted_scan_enqueue(work, n_tiles, d_count, s);
    split_launches(n_tiles, kOrfBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(orf_write, dim3((unsigned)n), dim3(kOrfBlock), 0, s, a, t); });
    return hip_rc(hipGetLastError());
}

int cnt_orfs(const uint64_t* bits, size_t len, uint64_t stops, uint64_t starts, size_t min_len, unsigned flags, uint64_t* pos, uint64_t* length,
             uint64_t* info, size_t out_cap, uint64_t* count) {
    uint64_t most = 0;
    CNT_TRY(orf_args(bits, len, stops, flags, pos, length, info, out_cap, count, &most));
    if (len < 3) return counted_empty(count);
    const size_t work_bytes = orf_work_bytes(orf_tiles(len));
    return counted_host_call(bits, len, {pos, length, info}, most, out_cap, count, work_bytes,
                             [&](void* const* d, size_t cap, void* d_count, void* d_work, hipStream_t s) {
                                 return cnt_orfs_dev(d[0], len, stops, starts, min_len, flags, d[1], d[2], d[3], cap, d_count, d_work, work_bytes, s);
                             });
}

}  // extern "C"
