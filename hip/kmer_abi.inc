// kmer_abi.inc -- C-ABI entry points of k-mer extraction (include/cute_nt.h, "k-mers"): cnt_kmers_dev (enqueue-only on a
// caller stream: no allocation, no synchronisation, capturable in a graph) and cnt_kmers (host tier, the shape of
// packed_ops_abi.inc's host_unary: staged through DevCtx::d_aux, or in place when both caller buffers are pinned).
// Included at the end of cute_nt.hip, after packed_ops_abi.inc (capped_grid, finish).
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
    const uint64_t per_launch = max_tiles_per_launch(kKmerBlock);
    for (uint64_t t = 0; t < n_tiles; t += per_launch) {
        const unsigned n = (unsigned)std::min(per_launch, n_tiles - t);
        const uint64_t first = head + t * kKmersPerTile;
        if (canonical) hipLaunchKernelGGL((kmer_tiles<kKmerBlock, kKmerU, true>), dim3(n), dim3(kKmerBlock), 0, s, in8, out8, first, (uint32_t)k);
        else hipLaunchKernelGGL((kmer_tiles<kKmerBlock, kKmerU, false>), dim3(n), dim3(kKmerBlock), 0, s, in8, out8, first, (uint32_t)k);
    }
    auto generic = [&](uint64_t first, uint64_t end) {
        if (first >= end) return;
        const dim3 g(capped_grid(end - first, kBlock));
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
    const size_t in_bytes = cnt_words_for(len) * 8, out_bytes = ((size_t)len - k + 1) * 8;
    DevCtx* c = nullptr;
    CNT_TRY(t_ctx.get(&c));
    void *dbits = nullptr, *dout = nullptr;
    if (host_range_is_pinned(bits, in_bytes, &dbits) && host_range_is_pinned(out, out_bytes, &dout) && dbits && dout) {
        CNT_TRY(c->ensure_streams());
        hipStream_t s = c->stream[0];
        return finish(s, cnt_kmers_dev(dbits, len, k, flags, dout, out_cap, s));  // pinned in, pinned out: one kernel over the link
    }
    CNT_TRY(c->ensure_aux(0, in_bytes));
    CNT_TRY(c->ensure_aux(1, out_bytes));
    hipStream_t s = c->stream[0];
    int rc = hip_rc(hipMemcpyAsync(c->d_aux[0], bits, in_bytes, hipMemcpyHostToDevice, s));
    if (rc == CNT_OK) rc = cnt_kmers_dev(c->d_aux[0], len, k, flags, c->d_aux[1], out_bytes / 8, s);
    if (rc == CNT_OK) rc = hip_rc(hipMemcpyAsync(out, c->d_aux[1], out_bytes, hipMemcpyDeviceToHost, s));
    return finish(s, rc);
}

}  // extern "C"
