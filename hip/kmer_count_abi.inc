// kmer_count_abi.inc -- C-ABI entry points of k-mer counting (include/cute_nt.h, "k-mer counts"): cnt_kmer_counts_dev (enqueue-
// only on a caller stream: ONE launch that ADDS to the caller's table, no allocation, no synchronisation, capturable in a graph)
// and cnt_kmer_counts (host tier: the packed input through cute_nt.hip's host_call, pinned or staged; the table is always
// accumulated in device scratch and copied back -- the kernel's atomics never go over the link).  Included at the end of
// cute_nt.hip.
#include "kmer_count_kernels.hpp"

namespace {

// the argument checks both tiers share, before any device work.  The device tier has nothing to do when len < k (CNT_OK
// whatever the pointers are); the host tier always writes its 4^k entries, so its table is checked at every len.
int kmer_count_args(const void* bits, size_t len, unsigned k, unsigned flags, const void* counts, size_t counts_cap, bool host) {
    if (k == 0 || k > CNT_KMER_COUNTS_MAX_K || (flags & ~CNT_KMER_CANONICAL)) return CNT_EINVAL;
    if (len < k && !host) return CNT_OK;
    const uint64_t bins = (uint64_t)1 << (2 * k);
    if (!counts || !aligned(counts, 8)) return CNT_EINVAL;
    if (len >= k && (!bits || !aligned(bits, 8))) return CNT_EINVAL;
    if (counts_cap < bins) return CNT_ECAP;
    if (len >= k && overlaps(bits, cnt_words_for(len) * 8, counts, bins * 8)) return CNT_EINVAL;
    return CNT_OK;
}

static_assert(CNT_KMER_COUNTS_MAX_K == kKmerCountMaxK, "the header's constant is the kernels'");
#ifndef CNT_LAB_VARIANTS
static_assert(tune_kmer_count_lds_max_k() == kKmerCountLdsMaxK, "the product build counts in LDS up to kKmerCountLdsMaxK");
#endif

}  // namespace

extern "C" {

int cnt_kmer_counts_dev(const void* d_bits, size_t len, unsigned k, unsigned flags, void* d_counts, size_t counts_cap, void* stream) {
    CNT_TRY(kmer_count_args(d_bits, len, k, flags, d_counts, counts_cap, false));
    if (len < k) return CNT_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t canonical = (flags & CNT_KMER_CANONICAL) ? 1u : 0u;
    const uint64_t m = (uint64_t)len - k + 1, words = cnt_words_for(len);
    const uint64_t n_tiles = (m + kKmerCountTileKmers - 1) / kKmerCountTileKmers;
    const uint8_t* in8 = static_cast<const uint8_t*>(d_bits);
    unsigned long long* counts = static_cast<unsigned long long*>(d_counts);
    // persistent: two workgroups per CU (the LDS regime's 64 KiB each; 8 waves per SIMD in both); more only where a workgroup
    // would otherwise see 2^32 k-mers before its flush (kKmerCountMaxTilesPerGroup: never up to 2^36 nt with >= 8 CUs)
    const uint64_t bound = (n_tiles + kKmerCountMaxTilesPerGroup - 1) / kKmerCountMaxTilesPerGroup;
    if ((int)k <= tune_kmer_count_lds_max_k()) {
        const unsigned grid = (unsigned)std::max<uint64_t>(std::min<uint64_t>(n_tiles, (uint64_t)chip_info().cus * 2), bound);
        hipLaunchKernelGGL((kmer_count<true>), dim3(grid), dim3(kKmerCountBlock), 0, s, in8, words, m, (uint32_t)k, canonical, n_tiles, counts);
    } else {
        const unsigned grid = (unsigned)std::min<uint64_t>(n_tiles, (uint64_t)chip_info().cus * 2);
        hipLaunchKernelGGL((kmer_count<false>), dim3(grid), dim3(kKmerCountBlock), 0, s, in8, words, m, (uint32_t)k, canonical, n_tiles, counts);
    }
    return hip_rc(hipGetLastError());
}

int cnt_kmer_counts(const uint64_t* bits, size_t len, unsigned k, unsigned flags, uint64_t* counts, size_t counts_cap) {
    CNT_TRY(kmer_count_args(bits, len, k, flags, counts, counts_cap, true));
    const size_t bytes = (size_t)8 << (2 * k);
    if (len < k) {
        memset(counts, 0, bytes);
        return CNT_OK;
    }
    // a table that starts in pinned memory and leaves it cannot be handed to hipMemcpyAsync (host_range_leaves_pinned)
    std::vector<uint8_t> bounce;
    if (host_range_leaves_pinned(counts, bytes)) bounce.resize(bytes);
    void* dst = bounce.empty() ? static_cast<void*>(counts) : bounce.data();
    const HostBuf in[1] = {{bits, cnt_words_for(len) * 8, Dir::in}};
    CNT_TRY(host_call(in, bytes, nullptr, false, [&](void* const* d, void* aux, hipStream_t s) {
        HIP_TRY(hipMemsetAsync(aux, 0, bytes, s));
        CNT_TRY(cnt_kmer_counts_dev(d[0], len, k, flags, aux, bytes / 8, s));
        return hip_rc(hipMemcpyAsync(dst, aux, bytes, hipMemcpyDeviceToHost, s));
    }));
    if (!bounce.empty()) memcpy(counts, bounce.data(), bytes);
    return CNT_OK;
}

}  // extern "C"
