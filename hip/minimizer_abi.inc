// minimizer_abi.inc -- C-ABI entry points of (w,k)-minimizer sampling (include/cute_nt.h, "k-mers"): the scratch query
// cnt_minimizers_work_bytes, cnt_minimizers_dev (enqueue-only on a caller stream: three kernels, no allocation, no
// synchronisation, capturable in a graph) and cnt_minimizers (host tier: cute_nt.hip's host_call, staged through DevCtx::d_aux,
// or in place when the caller's input and outputs are pinned).  Included at the end of cute_nt.hip.
#include "minimizer_kernels.hpp"

namespace {

// the number of windows W = m - w + 1 (0 when len < k or m < w)
uint64_t minimizer_windows(size_t len, unsigned k, unsigned w) {
    const uint64_t m = len >= k ? (uint64_t)len - k + 1 : 0;
    return m >= w ? m - w + 1 : 0;
}

// scratch, from d_work aligned up to 16 B: offs, one u64 per group of kMinGroup tiles (an even number of them), then counts,
// one u32 per tile of whole groups
uint64_t minimizer_work_bytes(uint64_t n_win) {
    if (!n_win) return 0;
    const uint64_t groups = ((n_win + kMinTile - 1) / kMinTile + kMinGroup - 1) / kMinGroup;
    return 16 + ((groups + 1) & ~1ull) * 8 + groups * kMinGroup * 4;
}

// the argument checks both tiers share, before any device work; *n_win = W.  CNT_OK with W = 0: nothing to compute.
int minimizer_args(const void* bits, size_t len, unsigned k, unsigned w, unsigned flags, const void* pos, const void* val,
                   size_t out_cap, const void* count, uint64_t* n_win) {
    if (k == 0 || k > 32 || w == 0 || w > kMinMaxW || (flags & ~CNT_KMER_CANONICAL)) return CNT_EINVAL;
    *n_win = minimizer_windows(len, k, w);
    if (*n_win == 0) return CNT_OK;
    if (!bits || !pos || !count || !aligned(bits, 8) || !aligned(pos, 8) || !aligned(count, 8) || (val && !aligned(val, 8)))
        return CNT_EINVAL;
    const size_t in_bytes = cnt_words_for(len) * 8, out_bytes = std::min<uint64_t>(*n_win, out_cap) * 8;
    if (overlaps(bits, in_bytes, pos, out_bytes) || (val && (overlaps(bits, in_bytes, val, out_bytes) || overlaps(pos, out_bytes, val, out_bytes))))
        return CNT_EINVAL;
    return CNT_OK;
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
    if (n_win == 0) return d_count ? hip_rc(hipMemsetAsync(d_count, 0, 8, s)) : CNT_OK;
    if (work_bytes < minimizer_work_bytes(n_win) || !d_work) return CNT_EINVAL;
    const uint64_t n_tiles = (n_win + kMinTile - 1) / kMinTile, groups = (n_tiles + kMinGroup - 1) / kMinGroup;
    uint64_t* offs = reinterpret_cast<uint64_t*>((reinterpret_cast<uintptr_t>(d_work) + 15) & ~(uintptr_t)15);
    uint32_t* counts = reinterpret_cast<uint32_t*>(offs + ((groups + 1) & ~1ull));
    const uint64_t* in = static_cast<const uint64_t*>(d_bits);
    uint64_t* pos = static_cast<uint64_t*>(d_pos);
    uint64_t* val = static_cast<uint64_t*>(d_val);
    uint64_t* count = static_cast<uint64_t*>(d_count);
    const uint32_t canonical = (flags & CNT_KMER_CANONICAL) ? 1u : 0u;
    split_launches(n_tiles, kMinBlock, [&](uint64_t t, uint64_t n) {
        hipLaunchKernelGGL((minimizer_tiles<false>), dim3((unsigned)n), dim3(kMinBlock), 0, s, in, (uint64_t)len, (uint32_t)k, (uint32_t)w,
                           canonical, t, counts, offs, pos, val, (uint64_t)out_cap);
    });
    hipLaunchKernelGGL(minimizer_scan, dim3(1), dim3(kMinScanBlock), 0, s, counts, offs, n_tiles, count);
    split_launches(n_tiles, kMinBlock, [&](uint64_t t, uint64_t n) {
        hipLaunchKernelGGL((minimizer_tiles<true>), dim3((unsigned)n), dim3(kMinBlock), 0, s, in, (uint64_t)len, (uint32_t)k, (uint32_t)w,
                           canonical, t, counts, offs, pos, val, (uint64_t)out_cap);
    });
    return hip_rc(hipGetLastError());
}

int cnt_minimizers(const uint64_t* bits, size_t len, unsigned k, unsigned w, unsigned flags, uint64_t* pos, uint64_t* val,
                   size_t out_cap, uint64_t* count) {
    uint64_t n_win = 0;
    CNT_TRY(minimizer_args(bits, len, k, w, flags, pos, val, out_cap, count, &n_win));
    if (n_win == 0) {
        if (count) *count = 0;
        return CNT_OK;
    }
    // the pinned lane needs cap > 0: an empty pos is never pinned
    const size_t cap = std::min<uint64_t>(n_win, out_cap), work_bytes = minimizer_work_bytes(n_win);
    uint64_t n = 0;
    CNT_TRY(host_call({{bits, cnt_words_for(len) * 8, Dir::in}, {pos, cap * 8, Dir::counted}, {val, cap * 8, Dir::counted}}, 8 + work_bytes, &n,
                      false, [&](void* const* d, void* aux, hipStream_t s) {  // aux: the device count, then the scratch
                          return cnt_minimizers_dev(d[0], len, k, w, flags, d[1], d[2], cap, aux, static_cast<uint8_t*>(aux) + 8, work_bytes, s);
                      }));
    *count = n;
    return n > out_cap ? CNT_ECAP : CNT_OK;
}

}  // extern "C"
