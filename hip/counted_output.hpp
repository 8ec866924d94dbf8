// counted_output.hpp -- the one layer under the calls whose number of results depends on the data: (w,k)-minimizers
// (minimizer_abi.inc), approximate pattern search (find_abi.inc) and the ORF scan (orf_abi.inc).  Such a call is, on one stream
// and without an allocation:
//   1. a count pass of its own: one workgroup per tile writes the tile's number of entries to counts[tile];
//   2. counted_scan: one workgroup sums the counts by groups of kCountedGroup tiles (one 64-B read per lane), writes each
//      group's exclusive offset to offs[group] and SETS *count to the total;
//   3. a write pass of its own: the same tiles again, recomputed, store their entries at counted_tile_base() + their rank in the
//      tile (word_tile.hpp: tile_rank_post, tile_total, tile_before), below out_cap only.
// A first scan of one u64 per tile, read and written by one lane per 16 consecutive tiles, took 0.52 ms of an 8.2-ms minimizer
// call at 2^30 nt: its loads and stores were 64 cache lines per wave instruction.
//
// The scratch of the three passes is the caller's (cnt_*_work_bytes), any contents, any address.  From d_work aligned up to 16 B:
//   offs    one u64 per group of kCountedGroup tiles, an even number of them (counts stays 16-B aligned)
//   counts  one u32 per tile of whole groups
// and behind them whatever else the call keeps there (the ORF scan: sums and carry).  This file is the only place that knows the
// format: counted_scratch_bytes() sizes it, counted_carve() cuts it, counted_scan and counted_tile_base() read and write it.
//
// The host half (behind the kernel) belongs to the shim: it uses cute_nt.hip's hip_rc, aligned, overlaps, HostBuf and host_call, and
// is included behind them, by way of the three *_kernels.hpp at the end of cute_nt.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>

#include "util_kernels.hpp"
#include "word_tile.hpp"

namespace cnt {

constexpr int kCountedScanBlock = 1024, kCountedGroup = 16;  // the offset scan: one workgroup, a group of 16 tiles per lane

// where the entries of a tile begin: its group's offset plus the counts of the group's earlier tiles
__device__ __forceinline__ uint64_t counted_tile_base(const uint64_t* offs, const uint32_t* counts, uint64_t tile) {
    uint64_t b = offs[tile / kCountedGroup];
    const uint32_t* g = counts + (tile - tile % kCountedGroup);
#pragma unroll
    for (int q = 0; q < kCountedGroup - 1; ++q) b += (uint64_t)q < tile % kCountedGroup ? g[q] : 0u;
    return b;
}

// One workgroup; lane j of a pass sums the kCountedGroup counts of group j (four 16-B loads: counts is 16-B aligned and holds
// whole groups, the entries past n_tiles are ignored), offs[group] = the exclusive prefix; *count = the total (set, not added).
__global__ __launch_bounds__(kCountedScanBlock) void counted_scan(const uint32_t* __restrict__ counts, uint64_t* __restrict__ offs,
                                                                  uint64_t n_tiles, uint64_t* __restrict__ count) {
    __shared__ uint64_t s_w[kCountedScanBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n_groups = (n_tiles + kCountedGroup - 1) / kCountedGroup;
    uint64_t carry = 0;
    for (uint64_t first = 0; first < n_groups; first += kCountedScanBlock) {
        const uint64_t g = first + threadIdx.x;
        uint64_t sum = 0;
        if (g < n_groups) {
            const u32x4* q = reinterpret_cast<const u32x4*>(counts + g * kCountedGroup);
#pragma unroll
            for (int u = 0; u < kCountedGroup / 4; ++u) {
                const u32x4 c = q[u];
#pragma unroll
                for (int e = 0; e < 4; ++e) sum += g * kCountedGroup + 4 * u + e < n_tiles ? c[e] : 0u;
            }
        }
        uint64_t x = sum;  // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = shfl_up_u64(x, o);
            if (lane >= (uint32_t)o) x += y;
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        uint64_t before = carry + x - sum, total = 0;
#pragma unroll
        for (int q = 0; q < kCountedScanBlock / 64; ++q) {
            const uint64_t y = s_w[q];
            before += q < (int)wave ? y : 0;
            total += y;
        }
        if (g < n_groups) offs[g] = before;
        carry += total;
        __syncthreads();  // s_w is rewritten by the next pass
    }
    if (threadIdx.x == 0) *count = carry;
}

// ---- the host half -----------------------------------------------------------------------------------------------------------
// bytes of scratch for n_tiles tiles: the two regions and the 16 B that rounding d_work up can cost; nothing without a tile
inline uint64_t counted_scratch_bytes(uint64_t n_tiles) {
    if (!n_tiles) return 0;
    const uint64_t groups = (n_tiles + kCountedGroup - 1) / kCountedGroup;
    return 16 + ((groups + 1) & ~1ull) * 8 + groups * kCountedGroup * 4;
}

// the regions of a scratch of counted_scratch_bytes(n_tiles) bytes at d_work; `behind` is the first byte after counts, 8-B aligned
// (whole groups are 64 B)
struct CountedScratch {
    uint64_t* offs;
    uint32_t* counts;
    void* behind;
};
inline CountedScratch counted_carve(void* d_work, uint64_t n_tiles) {
    const uint64_t groups = (n_tiles + kCountedGroup - 1) / kCountedGroup;
    uint64_t* offs = reinterpret_cast<uint64_t*>((reinterpret_cast<uintptr_t>(d_work) + 15) & ~(uintptr_t)15);
    uint32_t* counts = reinterpret_cast<uint32_t*>(offs + ((groups + 1) & ~1ull));
    return {offs, counts, counts + groups * kCountedGroup};
}

// pass 2, between a call's count and write passes
inline void counted_scan_enqueue(const CountedScratch& w, uint64_t n_tiles, void* d_count, hipStream_t s) {
    hipLaunchKernelGGL(counted_scan, dim3(1), dim3(kCountedScanBlock), 0, s, w.counts, w.offs, n_tiles, static_cast<uint64_t*>(d_count));
}

// The argument checks every tier of the three calls ends with, before any device work (the call's own parameter checks come first
// and "nothing to compute" returns before these): bits, the required outputs and count present and 8-B aligned, an optional output
// aligned when present, and no two of them sharing memory -- the input at its words, the outputs at the min(most, out_cap) entries
// that can be written, the count at its 8 bytes.  counted_work() is the same rule for the device tier's scratch.
struct CountedOut {
    const void* p;
    bool required;
};
inline int counted_args(const void* bits, size_t len, std::initializer_list<CountedOut> outs, uint64_t most, size_t out_cap, const void* count) {
    if (!bits || !count || !aligned(bits, 8) || !aligned(count, 8)) return CNT_EINVAL;
    for (const CountedOut& o : outs)
        if ((o.required && !o.p) || !aligned(o.p, 8)) return CNT_EINVAL;
    const size_t in_bytes = cnt_words_for(len) * 8, out_bytes = std::min<uint64_t>(most, out_cap) * 8;
    if (overlaps(count, 8, bits, in_bytes)) return CNT_EINVAL;
    for (const CountedOut* o = outs.begin(); o != outs.end(); ++o) {
        if (!o->p) continue;
        if (overlaps(bits, in_bytes, o->p, out_bytes) || overlaps(count, 8, o->p, out_bytes)) return CNT_EINVAL;
        for (const CountedOut* e = outs.begin(); e != o; ++e)
            if (e->p && overlaps(e->p, out_bytes, o->p, out_bytes)) return CNT_EINVAL;
    }
    return CNT_OK;
}

// The device tier's scratch, behind counted_args: present, at least the `need` bytes the call's *_work_bytes query answers, and
// those bytes (not what the caller lent beyond them) sharing none with the input words, an output or the count.
inline int counted_work(const void* d_work, size_t work_bytes, size_t need, const void* bits, size_t len, std::initializer_list<const void*> outs,
                        uint64_t most, size_t out_cap, const void* count) {
    if (work_bytes < need || !d_work) return CNT_EINVAL;
    if (overlaps(d_work, need, bits, cnt_words_for(len) * 8) || overlaps(d_work, need, count, 8)) return CNT_EINVAL;
    for (const void* o : outs)
        if (o && overlaps(d_work, need, o, std::min<uint64_t>(most, out_cap) * 8)) return CNT_EINVAL;
    return CNT_OK;
}

// nothing to compute: the count is 0, on the host and on a stream
inline int counted_empty(uint64_t* count) {
    if (count) *count = 0;
    return CNT_OK;
}
inline int counted_empty_dev(void* d_count, hipStream_t s) { return d_count ? hip_rc(hipMemsetAsync(d_count, 0, 8, s)) : CNT_OK; }

// The host tier of a call with N outputs (an absent optional one is NULL): dev(d, cap, d_count, d_work, s) enqueues the call's _dev
// entry point on the views d[0] = bits, d[1 ..] = outs with capacity cap; the scratch d_work holds work_bytes.  *count = n whether
// or not the entries fitted: CNT_ECAP comes after the work.
template <size_t N, typename F>
int counted_host_call(const uint64_t* bits, size_t len, uint64_t* const (&outs)[N], uint64_t most, size_t out_cap, uint64_t* count,
                      size_t work_bytes, F&& dev) {
    // the pinned lane needs cap > 0: an empty pos is never pinned
    const size_t cap = std::min<uint64_t>(most, out_cap);
    HostBuf b[N + 1] = {{bits, cnt_words_for(len) * 8, Dir::in}};
    for (size_t i = 0; i < N; ++i) b[i + 1] = {outs[i], cap * 8, Dir::counted};
    uint64_t n = 0;
    CNT_TRY(host_call(b, 8 + work_bytes, &n, false, [&](void* const* d, void* aux, hipStream_t s) {  // aux: the device count, then the scratch
        return dev(d, cap, aux, static_cast<void*>(static_cast<uint8_t*>(aux) + 8), s);
    }));
    *count = n;
    return n > out_cap ? CNT_ECAP : CNT_OK;
}

}  // namespace cnt
