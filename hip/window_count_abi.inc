// window_count_abi.inc -- C-ABI entry points of the windowed counts (include/cute_nt.h, "windowed composition"): the query
// cnt_window_counts_n, cnt_window_counts_dev (enqueue-only on a caller stream: one kernel for windows up to kWindowCountPiece, a
// zeroing kernel and the piece kernel for longer ones; no allocation, no synchronisation, no scratch, capturable in a graph) and
// cnt_window_counts (host tier: cute_nt.hip's host_call, pinned input and output in place or both staged).  Included at the end of
// cute_nt.hip, behind hpc_abi.inc.
#include "window_count_kernels.hpp"

namespace {

static_assert(CNT_WINDOW_COUNTS_MAX_K == kWindowCountMaxK, "the header's constant is the kernels'");

// rule 1 of the header's order, and the number of windows
int window_count_shape(size_t len, unsigned k, size_t window, size_t step, unsigned flags, size_t* n_win) {
    if (k == 0 || k > CNT_WINDOW_COUNTS_MAX_K || flags || step == 0 || window < k || ((uint64_t)window >> 32)) return CNT_EINVAL;
    *n_win = len >= window ? (len - window) / step + 1 : 0;
    return CNT_OK;
}

// the argument checks both tiers share, before any device work, in the header's order; CNT_OK with *n_win == 0: nothing to do
int window_count_args(const void* bits, size_t len, unsigned k, size_t window, size_t step, unsigned flags, const void* out, size_t out_cap, size_t* n_win) {
    CNT_TRY(window_count_shape(len, k, window, step, flags, n_win));
    if (*n_win == 0) return CNT_OK;
    if (!bits || !out || !aligned(bits, 8) || !aligned(out, 8)) return CNT_EINVAL;
    if (out_cap < *n_win) return CNT_ECAP;
    if (overlaps(bits, cnt_words_for(len) * 8, out, (*n_win * 4) << (2 * k))) return CNT_EINVAL;
    return CNT_OK;
}

}  // namespace

extern "C" {

int cnt_window_counts_n(size_t len, unsigned k, size_t window, size_t step, size_t* n_windows) {
    size_t n = 0;
    CNT_TRY(window_count_shape(len, k, window, step, 0, &n));
    if (!n_windows) return CNT_EINVAL;
    *n_windows = n;
    return CNT_OK;
}

int cnt_window_counts_dev(const void* d_bits, size_t len, unsigned k, size_t window, size_t step, unsigned flags, void* d_out, size_t out_cap, void* stream) {
    size_t n_win = 0;
    CNT_TRY(window_count_args(d_bits, len, k, window, step, flags, d_out, out_cap, &n_win));
    if (n_win == 0) return CNT_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WindowCountArgs a = {static_cast<const uint8_t*>(d_bits), cnt_words_for(len), window, step, n_win, static_cast<uint32_t*>(d_out), 0, 0, 0};
    const uint64_t span = ((uint64_t)window + 30) / 32 + 1;  // the words a window can touch: it may begin at the last code of a word
    if (window <= kWindowCountPiece) {
        while (a.lanes_log2 < 6 && (kWindowCountLaneWords << a.lanes_log2) < span) ++a.lanes_log2;  // kWindowCountLaneWords words a lane
        const uint64_t per_tile = (uint64_t)kWindowCountBlock >> a.lanes_log2;
        void (*const count)(WindowCountArgs, uint64_t) = k == 1 ? window_count_k1 : window_count_k2;
        split_launches((n_win + per_tile - 1) / per_tile, kWindowCountBlock,
                       [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(count, dim3((unsigned)n), dim3(kWindowCountBlock), 0, s, a, t); });
        return hip_rc(hipGetLastError());
    }
    // Long windows: `pieces` tiles of kWindowCountTileWords words cover a window; a workgroup walks a run of them, as short as it
    // takes to put eight workgroups on every CU -- a call with window == len is cut into that many runs, a call with many windows
    // into one piece per workgroup -- and adds its sums to the record the zeroing kernel cleared.
    const uint64_t out_words = ((uint64_t)n_win * 2) << (2 * (k - 1));  // 8-B words of the records: 2 (k = 1) or 8 (k = 2) each
    split_launches((out_words + kWindowCountBlock - 1) / kWindowCountBlock, kWindowCountBlock, [&](uint64_t t, uint64_t n) {
        hipLaunchKernelGGL(window_count_zero, dim3((unsigned)n), dim3(kWindowCountBlock), 0, s, static_cast<uint64_t*>(d_out), out_words, t);
    });
    const uint64_t pieces = (span + kWindowCountTileWords - 1) / kWindowCountTileWords, want = (uint64_t)chip_info().cus * 8;
    const uint64_t per_run = std::min(pieces, std::max<uint64_t>(1, pieces / std::max<uint64_t>(1, want / n_win)));
    a.runs = (pieces + per_run - 1) / per_run;
    a.run_words = per_run * kWindowCountTileWords;
    void (*const count)(WindowCountArgs, uint64_t) = k == 1 ? window_count_piece_k1 : window_count_piece_k2;
    split_launches((uint64_t)n_win * a.runs, kWindowCountBlock,
                   [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(count, dim3((unsigned)n), dim3(kWindowCountBlock), 0, s, a, t); });
    return hip_rc(hipGetLastError());
}

int cnt_window_counts(const uint64_t* bits, size_t len, unsigned k, size_t window, size_t step, unsigned flags, uint32_t* out, size_t out_cap) {
    size_t n_win = 0;
    CNT_TRY(window_count_args(bits, len, k, window, step, flags, out, out_cap, &n_win));
    if (n_win == 0) return CNT_OK;
    // host_call bounces an output that starts in pinned memory and leaves it (host_range_leaves_pinned), as cnt_kmer_counts does
    const HostBuf b[2] = {{bits, cnt_words_for(len) * 8, Dir::in}, {out, (n_win * 4) << (2 * k), Dir::out}};
    return host_call(b, 0, nullptr, false, [&](void* const* d, void*, hipStream_t s) { return cnt_window_counts_dev(d[0], len, k, window, step, 0, d[1], n_win, s); });
}

}  // extern "C"
