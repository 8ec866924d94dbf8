// kmer_abi.inc -- C-ABI entry points of k-mer extraction (include/cute_nt.h, "k-mers"): cnt_kmers_dev (enqueue-only on a
// caller stream: no allocation, no synchronisation, capturable in a graph) and cnt_kmers (host tier: cute_nt.hip's host_call,
// staged through DevCtx::d_aux, or in place when both caller buffers are pinned).  Included at the end of cute_nt.hip.
#include "kmer_kernels.hpp"

namespace {

// the argument checks both tiers share, before any device work; CNT_OK also for len < k (no k-mer, nothing to do)
int kmer_args(const void* bits, size_t len, unsigned k, unsigned flags, const void* out, size_t out_cap) {
    if (k == 0 || k > 32 || (flags & ~CNT_KMER_CANONICAL)) return CNT_EINVAL;
    if (len < k) return CNT_OK;
    const uint64_t m = (uint64_t)len - k + 1;
    if (!bits || !out || !aligned(bits, 8) || !aligned(out, 8)) return CNT_EINVAL;
    if (overlaps(bits, cnt_words_for(len) * 8, out, std::min<uint64_t>(m, out_cap) * 8)) return CNT_EINVAL;
    if (out_cap < m) return CNT_ECAP;
    return CNT_OK;
}

}  // namespace

extern "C" {

int cnt_kmers_dev(const void* d_bits, size_t len, unsigned k, unsigned flags, void* d_out, size_t out_cap, void* stream) {
    CNT_TRY(kmer_args(d_bits, len, k, flags, d_out, out_cap));
    if (len < k) return CNT_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool canonical = (flags & CNT_KMER_CANONICAL) != 0;
    const uint64_t m = (uint64_t)len - k + 1, words = cnt_words_for(len);
    const uint8_t* in8 = static_cast<const uint8_t*>(d_bits);
    uint8_t* out8 = static_cast<uint8_t*>(d_out);
    // head: k-mers until the stores sit on a 128-B line.  The tiles read the input at 8-B grain, so its phase does not matter.
    uint64_t head = ((128 - (reinterpret_cast<uintptr_t>(d_out) & 127)) & 127) >> 3;
    // a tile [a, a+T) reads input words up to (a+T-1)/32 + 1: tiles end at 32*(words-1) k-mers at the latest
    const uint64_t tile_end = std::min<uint64_t>(m, 32 * (words - 1));
    const uint64_t n_tiles = tile_end > head ? (tile_end - head) / kKmersPerTile : 0;
    split_launches(n_tiles, kKmerBlock, [&](uint64_t t, uint64_t n) {
        const uint64_t first = head + t * kKmersPerTile;
        if (canonical) hipLaunchKernelGGL((kmer_tiles<kKmerBlock, kKmerU, true>), dim3((unsigned)n), dim3(kKmerBlock), 0, s, in8, out8, first, (uint32_t)k);
        else hipLaunchKernelGGL((kmer_tiles<kKmerBlock, kKmerU, false>), dim3((unsigned)n), dim3(kKmerBlock), 0, s, in8, out8, first, (uint32_t)k);
    });
    auto generic = [&](uint64_t first, uint64_t end) {
        if (first >= end) return;
        const dim3 g(generic_grid(end - first));
        const uint64_t* in = static_cast<const uint64_t*>(d_bits);
        uint64_t* out = static_cast<uint64_t*>(d_out);
        if (canonical) hipLaunchKernelGGL((kmer_generic<true>), g, dim3(kBlock), 0, s, in, out, (uint32_t)k, first, end);
        else hipLaunchKernelGGL((kmer_generic<false>), g, dim3(kBlock), 0, s, in, out, (uint32_t)k, first, end);
    };
    if (n_tiles) {
        generic(0, head);
        generic(head + n_tiles * kKmersPerTile, m);
    } else {
        generic(0, m);
    }
    return hip_rc(hipGetLastError());
}

int cnt_kmers(const uint64_t* bits, size_t len, unsigned k, unsigned flags, uint64_t* out, size_t out_cap) {
    CNT_TRY(kmer_args(bits, len, k, flags, out, out_cap));
    if (len < k) return CNT_OK;
    const size_t m = (size_t)len - k + 1;
    return host_call({{bits, cnt_words_for(len) * 8, Dir::in}, {out, m * 8, Dir::out}}, 0, nullptr, false,
                     [&](void* const* d, void*, hipStream_t s) { return cnt_kmers_dev(d[0], len, k, flags, d[1], m, s); });
}

}  // extern "C"
