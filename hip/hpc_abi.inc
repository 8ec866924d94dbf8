// hpc_abi.inc -- C-ABI entry points of homopolymer compression (include/cute_nt.h, "homopolymer compression"): the scratch query
// cnt_hpc_work_bytes, cnt_hpc_dev (enqueue-only on a caller stream: four passes, no allocation, no synchronisation, capturable in
// a graph) and cnt_hpc (host tier: cute_nt.hip's host_call, staged through DevCtx::d_aux, or in place when the caller's input and
// outputs are pinned).  The scratch layout and the scan are counted_output.hpp's; its argument checks and its host tier take one
// u64 per entry for every output, and the packed output here takes a 32nd of that, so this file has its own.  Included at the end
// of cute_nt.hip, behind orf_abi.inc.
#include "hpc_kernels.hpp"

namespace {

uint64_t hpc_tiles(size_t len) { return ((uint64_t)len + kHpcTile - 1) / kHpcTile; }

// The argument checks both tiers share, before any device work; *cap = the most codes that can be written, which sizes the
// footprints: cnt_words_for(*cap) words of out, *cap entries of pos.  CNT_OK with len == 0: nothing to compute.
int hpc_args(const void* bits, size_t len, unsigned flags, const void* out, const void* pos, size_t out_cap, const void* count, size_t* cap) {
    if (flags) return CNT_EINVAL;
    *cap = std::min(len, out_cap);
    if (len == 0) return CNT_OK;
    if (!bits || !out || !count || !aligned(bits, 8) || !aligned(out, 8) || !aligned(count, 8) || !aligned(pos, 8)) return CNT_EINVAL;
    const size_t in_bytes = cnt_words_for(len) * 8, out_bytes = cnt_words_for(*cap) * 8, pos_bytes = pos ? *cap * 8 : 0;
    if (overlaps(bits, in_bytes, out, out_bytes) || overlaps(bits, in_bytes, pos, pos_bytes) || overlaps(out, out_bytes, pos, pos_bytes)) return CNT_EINVAL;
    if (overlaps(count, 8, bits, in_bytes) || overlaps(count, 8, out, out_bytes) || overlaps(count, 8, pos, pos_bytes)) return CNT_EINVAL;
    return CNT_OK;
}

}  // namespace

extern "C" {

int cnt_hpc_work_bytes(size_t len, size_t* bytes) {
    if (!bytes) return CNT_EINVAL;
    *bytes = counted_scratch_bytes(hpc_tiles(len));
    return CNT_OK;
}

int cnt_hpc_dev(const void* d_bits, size_t len, unsigned flags, void* d_out, void* d_pos, size_t out_cap, void* d_count, void* d_work, size_t work_bytes,
                void* stream) {
    size_t cap = 0;
    CNT_TRY(hpc_args(d_bits, len, flags, d_out, d_pos, out_cap, d_count, &cap));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (len == 0) return counted_empty_dev(d_count, s);
    const uint64_t n_tiles = hpc_tiles(len);
    const size_t need = counted_scratch_bytes(n_tiles);  // the scratch at the query's size, against everything else of the call
    if (work_bytes < need || !d_work) return CNT_EINVAL;
    if (overlaps(d_work, need, d_bits, cnt_words_for(len) * 8) || overlaps(d_work, need, d_out, cnt_words_for(cap) * 8) ||
        overlaps(d_work, need, d_pos, d_pos ? cap * 8 : 0) || overlaps(d_work, need, d_count, 8))
        return CNT_EINVAL;
    const CountedScratch work = counted_carve(d_work, n_tiles);
    const HpcArgs a = {static_cast<const uint8_t*>(d_bits), cnt_words_for(len), len, n_tiles, work.counts, work.offs, static_cast<uint64_t*>(d_out),
                       static_cast<uint64_t*>(d_pos), cap};
    split_launches(n_tiles, kHpcBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(hpc_count, dim3((unsigned)n), dim3(kHpcBlock), 0, s, a, t); });
    counted_scan_enqueue(work, n_tiles, d_count, s);
    if (cap) {
        // one lane per tile
        split_launches((n_tiles + kHpcBlock - 1) / kHpcBlock, kHpcBlock,
                       [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(hpc_zero_edges, dim3((unsigned)n), dim3(kHpcBlock), 0, s, a, t); });
        void (*const write)(HpcArgs, uint64_t) = d_pos ? hpc_write_pos : hpc_write;
        split_launches(n_tiles, kHpcBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(write, dim3((unsigned)n), dim3(kHpcBlock), 0, s, a, t); });
    }
    return hip_rc(hipGetLastError());
}

int cnt_hpc(const uint64_t* bits, size_t len, unsigned flags, uint64_t* out, uint64_t* pos, size_t out_cap, uint64_t* count) {
    size_t cap = 0;
    CNT_TRY(hpc_args(bits, len, flags, out, pos, out_cap, count, &cap));
    if (len == 0) return counted_empty(count);
    const size_t work_bytes = counted_scratch_bytes(hpc_tiles(len));
    // out travels whole (its footprint is a 32nd of a pos); pos in its first n entries
    const HostBuf b[3] = {{bits, cnt_words_for(len) * 8, Dir::in}, {out, cnt_words_for(cap) * 8, Dir::out}, {pos, cap * 8, Dir::counted}};
    uint64_t n = 0;
    CNT_TRY(host_call(b, 8 + work_bytes, &n, false, [&](void* const* d, void* aux, hipStream_t s) {  // aux: the device count, then the scratch
        return cnt_hpc_dev(d[0], len, 0, d[1], d[2], cap, aux, static_cast<uint8_t*>(aux) + 8, work_bytes, s);
    }));
    *count = n;
    return n > out_cap ? CNT_ECAP : CNT_OK;
}

}  // extern "C"
