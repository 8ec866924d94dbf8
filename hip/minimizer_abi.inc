// minimizer_abi.inc -- C-ABI entry points of (w,k)-minimizer sampling (include/cute_nt.h, "k-mers"): the scratch query
// cnt_minimizers_work_bytes, cnt_minimizers_dev (enqueue-only on a caller stream: three kernels, no allocation, no
// synchronisation, capturable in a graph) and cnt_minimizers (host tier: cute_nt.hip's host_call, staged through DevCtx::d_aux,
// or in place when the caller's input and outputs are pinned).  The scratch layout, the scan, the common argument checks and the
// host tier are counted_output.hpp's.  Included at the end of cute_nt.hip.
#include "minimizer_kernels.hpp"

namespace {

// the number of windows W = m - w + 1 (0 when len < k or m < w)
uint64_t minimizer_windows(size_t len, unsigned k, unsigned w) {
    const uint64_t m = len >= k ? (uint64_t)len - k + 1 : 0;
    return m >= w ? m - w + 1 : 0;
}

// scratch: the counted output's (counted_output.hpp), one tile per kMinTile windows
uint64_t minimizer_work_bytes(uint64_t n_win) { return counted_scratch_bytes((n_win + kMinTile - 1) / kMinTile); }

// the argument checks both tiers share, before any device work; *n_win = W.  CNT_OK with W = 0: nothing to compute.
int minimizer_args(const void* bits, size_t len, unsigned k, unsigned w, unsigned flags, const void* pos, const void* val,
                   size_t out_cap, const void* count, uint64_t* n_win) {
    if (k == 0 || k > 32 || w == 0 || w > kMinMaxW || (flags & ~CNT_KMER_CANONICAL)) return CNT_EINVAL;
    *n_win = minimizer_windows(len, k, w);
    if (*n_win == 0) return CNT_OK;
    return counted_args(bits, len, {{pos, true}, {val, false}}, *n_win, out_cap, count);
}

}  // namespace

extern "C" {

int cnt_minimizers_work_bytes(size_t len, unsigned k, unsigned w, size_t* bytes) {
    if (!bytes || k == 0 || k > 32 || w == 0 || w > kMinMaxW) return CNT_EINVAL;
    *bytes = minimizer_work_bytes(minimizer_windows(len, k, w));
    return CNT_OK;
}

int cnt_minimizers_dev(const void* d_bits, size_t len, unsigned k, unsigned w, unsigned flags, void* d_pos, void* d_val,
                       size_t out_cap, void* d_count, void* d_work, size_t work_bytes, void* stream) {
    uint64_t n_win = 0;
    CNT_TRY(minimizer_args(d_bits, len, k, w, flags, d_pos, d_val, out_cap, d_count, &n_win));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_win == 0) return counted_empty_dev(d_count, s);
    CNT_TRY(counted_work(d_work, work_bytes, minimizer_work_bytes(n_win), d_bits, len, {d_pos, d_val}, n_win, out_cap, d_count));
    const uint64_t n_tiles = (n_win + kMinTile - 1) / kMinTile;
    const CountedScratch work = counted_carve(d_work, n_tiles);
    const uint64_t* in = static_cast<const uint64_t*>(d_bits);
    uint64_t* pos = static_cast<uint64_t*>(d_pos);
    uint64_t* val = static_cast<uint64_t*>(d_val);
    const uint32_t canonical = (flags & CNT_KMER_CANONICAL) ? 1u : 0u;
    split_launches(n_tiles, kMinBlock, [&](uint64_t t, uint64_t n) {
        hipLaunchKernelGGL((minimizer_tiles<false>), dim3((unsigned)n), dim3(kMinBlock), 0, s, in, (uint64_t)len, (uint32_t)k, (uint32_t)w,
                           canonical, t, work.counts, work.offs, pos, val, (uint64_t)out_cap);
    });
    counted_scan_enqueue(work, n_tiles, d_count, s);
    split_launches(n_tiles, kMinBlock, [&](uint64_t t, uint64_t n) {
        hipLaunchKernelGGL((minimizer_tiles<true>), dim3((unsigned)n), dim3(kMinBlock), 0, s, in, (uint64_t)len, (uint32_t)k, (uint32_t)w,
                           canonical, t, work.counts, work.offs, pos, val, (uint64_t)out_cap);
    });
    return hip_rc(hipGetLastError());
}

int cnt_minimizers(const uint64_t* bits, size_t len, unsigned k, unsigned w, unsigned flags, uint64_t* pos, uint64_t* val,
                   size_t out_cap, uint64_t* count) {
    uint64_t n_win = 0;
    CNT_TRY(minimizer_args(bits, len, k, w, flags, pos, val, out_cap, count, &n_win));
    if (n_win == 0) return counted_empty(count);
    const size_t work_bytes = minimizer_work_bytes(n_win);
    return counted_host_call(bits, len, {pos, val}, n_win, out_cap, count, work_bytes,
                             [&](void* const* d, size_t cap, void* d_count, void* d_work, hipStream_t s) {
                                 return cnt_minimizers_dev(d[0], len, k, w, flags, d[1], d[2], cap, d_count, d_work, work_bytes, s);
                             });
}

}  // extern "C"
