// packed_ops_abi.inc -- C-ABI entry points of the packed-domain operations (include/cute_nt.h,
// "packed-domain operations"): Hamming distance, complement, reverse complement on 2-bit packed
// words, and alphabet validation of ASCII buffers.  Included at the end of cute_nt.hip (one
// translation unit: the kernel headers define non-template __global__ functions).  Device tier
// = enqueue-only on a caller stream; host tier = cute_nt.hip's host_call: whole-buffer H2D / kernel / D2H through per-thread
// grow-only device scratch (convenience entry points, not chunked / not tuned for PCIe) -- or, when the caller's slices
// are pinned, the same kernels reading and writing them over the link.
#include "packed_ops_kernels.hpp"

extern "C" {

// ---- device tier -----------------------------------------------------------------------
int cnt_hamming_dev(const void* d_a, const void* d_b, size_t len, void* d_count, void* stream) {
    if (len == 0) return CNT_OK;
    if (!d_a || !d_b || !d_count || !aligned(d_a, 8) || !aligned(d_b, 8) || !aligned(d_count, 8)) return CNT_EINVAL;
    const uint64_t words = cnt_words_for(len);
    // the counter is written: it shares no byte with either stream (a and b are only read and may overlap each other freely)
    if (overlaps(d_count, 8, d_a, words * 8) || overlaps(d_count, 8, d_b, words * 8)) return CNT_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* count = static_cast<unsigned long long*>(d_count);
    uint64_t done_words = 0;
    constexpr int U = 2;
    constexpr uint64_t kTileWords = (uint64_t)kRedBlock * U * 2;  // 16-B vectors = 2 words each
    // head: when both streams share their 16-B phase, peel words until `a` sits on a 128-B line
    const uintptr_t pa = reinterpret_cast<uintptr_t>(d_a), pb = reinterpret_cast<uintptr_t>(d_b);
    const uint64_t hgrain = len >= ((uint64_t)1 << 24) ? 4096 : 128;  // whole pages for the XCD-interleaved tiles
    uint64_t head_words = ((pa ^ pb) & 15) == 0 ? ((hgrain - (pa & (hgrain - 1))) & (hgrain - 1)) >> 3 : 0;
    if (head_words > (len >> 5)) head_words = 0;
    uint64_t tile_words = 0;
#ifdef CNT_LAB_VARIANTS
    const bool persistent = g_reduce_persistent.load(std::memory_order_relaxed) != 0;
#else
    constexpr bool persistent = true;
#endif
    if (((pa + 8 * head_words) & 15) == 0 && ((pb + 8 * head_words) & 15) == 0 && persistent) {
        // one launch, no scratch: persistent waves over whole RUN-KiB pieces, one atomic each (packed_ops_kernels.hpp)
        constexpr uint64_t kRunWords = (uint64_t)kHammingRunKiB * 1024 / 8;
        const uint64_t n_runs = ((len >> 5) - head_words) / kRunWords;
        if (n_runs) {
            const unsigned grid = (unsigned)std::min<uint64_t>(n_runs, (uint64_t)chip_info().cus * kHammingWavesPerCU);
            const uint8_t* pa8 = static_cast<const uint8_t*>(d_a) + head_words * 8;
            const uint8_t* pb8 = static_cast<const uint8_t*>(d_b) + head_words * 8;
#ifdef CNT_LAB_VARIANTS
            const int order = g_hamming_order.load(std::memory_order_relaxed);
            if (order == 1) hipLaunchKernelGGL((hamming_persist_lab<kHammingRunKiB, 1>), dim3(grid), dim3(64), 0, s, pa8, pb8, n_runs, count);
            else if (order == 2) hipLaunchKernelGGL((hamming_persist_lab<kHammingRunKiB, 2>), dim3(grid), dim3(64), 0, s, pa8, pb8, n_runs, count);
            else
#endif
            hipLaunchKernelGGL((hamming_persist<kHammingRunKiB>), dim3(grid), dim3(64), 0, s, pa8, pb8, n_runs, count);
            HIP_TRY(hipGetLastError());
        }
        tile_words = n_runs * kRunWords;
    }
#ifdef CNT_LAB_VARIANTS
    else if (((pa + 8 * head_words) & 15) == 0 && ((pb + 8 * head_words) & 15) == 0) {  // round 1's form, for A/B runs
        const uint64_t full_words = (len >> 5) - head_words;  // words with all 32 codes valid
        uint64_t n_tiles = full_words / kTileWords;
        unsigned long long* partial = nullptr;  // stream-ordered scratch: one partial sum per workgroup
        if (n_tiles && hipMallocAsync(reinterpret_cast<void**>(&partial), n_tiles * 8, s) != hipSuccess) {
            (void)hipGetLastError();  // no stream-ordered allocator: the generic kernel below takes everything --
            g_reduce_fallbacks.fetch_add(1, std::memory_order_relaxed);  // slow but correct, and counted (tuning key "reduce_fallbacks")
            n_tiles = 0;
        }
        if (n_tiles) {
            split_launches(n_tiles, kRedBlock, [&](uint64_t first, uint64_t n) {
                const uint8_t* pa8 = static_cast<const uint8_t*>(d_a) + (head_words + first * kTileWords) * 8;
                const uint8_t* pb8 = static_cast<const uint8_t*>(d_b) + (head_words + first * kTileWords) * 8;
                if (g_reduce_xi.load(std::memory_order_relaxed))
                    hipLaunchKernelGGL((hamming_tiles<U, true>), dim3((unsigned)n), dim3(kRedBlock), 0, s, pa8, pb8, n, partial + first, xcd_shift());
                else
                    hipLaunchKernelGGL((hamming_tiles<U, false>), dim3((unsigned)n), dim3(kRedBlock), 0, s, pa8, pb8, n, partial + first, xcd_shift());
            });
            hipLaunchKernelGGL(sum_partials, dim3(sum_partials_grid(n_tiles)), dim3(kRedBlock), 0, s, partial, n_tiles, count);
            const int rc = hip_rc(hipGetLastError());
            HIP_TRY(hipFreeAsync(partial, s));
            CNT_TRY(rc);
        }
        tile_words = n_tiles * kTileWords;
    }
#endif
    if (tile_words && head_words) {
        hipLaunchKernelGGL(hamming_generic, dim3(1), dim3(kRedBlock), 0, s, static_cast<const uint64_t*>(d_a),
                           static_cast<const uint64_t*>(d_b), (uint64_t)(32 * head_words), (uint64_t)0, head_words, count);
        HIP_TRY(hipGetLastError());
    }
    done_words = tile_words ? head_words + tile_words : 0;
    if (done_words < words) {
        hipLaunchKernelGGL(hamming_generic, dim3(generic_grid(words - done_words, kRedBlock)), dim3(kRedBlock), 0, s,
                           static_cast<const uint64_t*>(d_a), static_cast<const uint64_t*>(d_b), (uint64_t)len, done_words, words, count);
        HIP_TRY(hipGetLastError());
    }
    return CNT_OK;
}

int cnt_complement_dev(const void* d_bits, size_t len, void* d_out, void* stream) {
    if (len == 0) return CNT_OK;
    if (!d_bits || !d_out || !aligned(d_bits, 8) || !aligned(d_out, 8)) return CNT_EINVAL;
    const uint64_t words = cnt_words_for(len);
    // exactly in place is fine: every lane stores only the words it loaded.  Any other overlap races one workgroup's loads
    // against another's stores.
    if (d_bits != d_out && overlaps(d_bits, words * 8, d_out, words * 8)) return CNT_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint64_t done_words = 0;
    constexpr int B = 256, U = 1;
    constexpr uint64_t kTileWords = (uint64_t)B * U * 2;
    // head: when both streams share their 16-B phase, peel words until the OUTPUT sits on a 128-B line
    const uintptr_t pi = reinterpret_cast<uintptr_t>(d_bits), po = reinterpret_cast<uintptr_t>(d_out);
    uint64_t head_words = ((pi ^ po) & 15) == 0 ? ((128 - (po & 127)) & 127) >> 3 : 0;
    if (head_words > (len >> 5)) head_words = 0;
    if (((pi + 8 * head_words) & 15) == 0 && ((po + 8 * head_words) & 15) == 0) {
        const uint64_t n_tiles = ((len >> 5) - head_words) / kTileWords;
        split_launches(n_tiles, B, [&](uint64_t first, uint64_t n) {
            hipLaunchKernelGGL((complement_tiles<B, U>), dim3((unsigned)n), dim3(B), 0, s,
                               static_cast<const uint8_t*>(d_bits) + (head_words + first * kTileWords) * 8,
                               static_cast<uint8_t*>(d_out) + (head_words + first * kTileWords) * 8, n);
        });
        if (n_tiles && head_words)
            hipLaunchKernelGGL(complement_generic, dim3(1), dim3(kBlock), 0, s, static_cast<const uint64_t*>(d_bits),
                               static_cast<uint64_t*>(d_out), (uint64_t)(32 * head_words), (uint64_t)0, head_words);
        HIP_TRY(hipGetLastError());
        done_words = n_tiles ? head_words + n_tiles * kTileWords : 0;
    }
    if (done_words < words) {
        hipLaunchKernelGGL(complement_generic, dim3(generic_grid(words - done_words)), dim3(kBlock), 0, s,
                           static_cast<const uint64_t*>(d_bits), static_cast<uint64_t*>(d_out), (uint64_t)len, done_words, words);
        HIP_TRY(hipGetLastError());
    }
    return CNT_OK;
}

int cnt_reverse_complement_dev(const void* d_bits, size_t len, void* d_out, void* stream) {
    if (len == 0) return CNT_OK;
    if (!d_bits || !d_out || !aligned(d_bits, 8) || !aligned(d_out, 8)) return CNT_EINVAL;
    const uint64_t words = cnt_words_for(len);
    if (overlaps(d_bits, words * 8, d_out, words * 8)) return CNT_EINVAL;  // not in place, and not shifted onto itself either
    hipStream_t s = static_cast<hipStream_t>(stream);
    constexpr int B = 256;
    constexpr uint64_t kTileWords = (uint64_t)B * 2;
    // head: output words until the stores sit on a 128-B line (word kernel); the tiles then solve the
    // same problem for the input shortened by those 32*head nucleotides -- their loads only need the
    // 8-B alignment every word pointer has
    uint64_t head = ((128 - (reinterpret_cast<uintptr_t>(d_out) & 127)) & 127) >> 3;
    if (head > (len >> 5)) head = 0;
    const uint64_t n_tiles = ((len >> 5) - head) / kTileWords;  // every window of these tiles lies inside the input
    split_launches(n_tiles, B, [&](uint64_t first, uint64_t n) {
        const uint64_t skip = head + first * kTileWords;  // output words in front of this launch
        hipLaunchKernelGGL((reverse_complement_tiles<B>), dim3((unsigned)n), dim3(B), 0, s, static_cast<const uint8_t*>(d_bits),
                           static_cast<uint8_t*>(d_out) + skip * 8, (uint64_t)len - 32 * skip, n);
    });
    auto word_kernel = [&](uint64_t first_word, uint64_t end_word) {
        if (first_word < end_word)
            hipLaunchKernelGGL(reverse_complement_words, dim3(generic_grid(end_word - first_word)), dim3(kBlock), 0, s,
                               static_cast<const uint64_t*>(d_bits), static_cast<uint64_t*>(d_out), (uint64_t)len, first_word, end_word);
    };
    if (n_tiles) {
        word_kernel(0, head);
        word_kernel(head + n_tiles * kTileWords, words);
    } else {
        word_kernel(0, words);
    }
    return hip_rc(hipGetLastError());
}

int cnt_validate_dev(const void* d_n, size_t n_len, unsigned flags, void* d_invalid_count, void* stream) {
    if (flags & ~CNT_ALLOW_N) return CNT_EINVAL;
    if (n_len == 0) return CNT_OK;
    if (!d_n || !d_invalid_count || !aligned(d_invalid_count, 8)) return CNT_EINVAL;
    if (overlaps(d_invalid_count, 8, d_n, n_len)) return CNT_EINVAL;  // the counter is written: not inside the bytes it counts
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* count = static_cast<unsigned long long*>(d_invalid_count);
    const bool allow_n = (flags & CNT_ALLOW_N) != 0;
    const uint8_t* n = static_cast<const uint8_t*>(d_n);
    uint64_t done = 0;
    constexpr int U = 4;
    constexpr uint64_t kTile = (uint64_t)kRedBlock * U * 16;
    // head: bytes until the stream sits on a 128-B line (a count does not care where it starts)
    const uint64_t vgrain = n_len >= ((uint64_t)1 << 22) ? 4096 : 128;  // whole pages for the XCD-interleaved tiles
    uint64_t head = (vgrain - (reinterpret_cast<uintptr_t>(d_n) & (vgrain - 1))) & (vgrain - 1);
    if (head > n_len) head = 0;
#ifdef CNT_LAB_VARIANTS
    const bool persistent = g_reduce_persistent.load(std::memory_order_relaxed) != 0;
#else
    constexpr bool persistent = true;
#endif
    if (persistent) {
        constexpr uint64_t kRun = (uint64_t)kValidateRunKiB * 1024;
        const uint64_t n_runs = (n_len - head) / kRun;
        if (n_runs) {
            const unsigned grid = (unsigned)std::min<uint64_t>(n_runs, (uint64_t)chip_info().cus * kValidateWavesPerCU);
            if (allow_n) hipLaunchKernelGGL((validate_persist<kValidateRunKiB, true>), dim3(grid), dim3(64), 0, s, n + head, n_runs, count);
            else hipLaunchKernelGGL((validate_persist<kValidateRunKiB, false>), dim3(grid), dim3(64), 0, s, n + head, n_runs, count);
            if (head) {
                if (allow_n) hipLaunchKernelGGL((validate_generic<true>), dim3(1), dim3(kRedBlock), 0, s, n, (uint64_t)0, head, count);
                else hipLaunchKernelGGL((validate_generic<false>), dim3(1), dim3(kRedBlock), 0, s, n, (uint64_t)0, head, count);
            }
            HIP_TRY(hipGetLastError());
            done = head + n_runs * kRun;
        }
    }
#ifdef CNT_LAB_VARIANTS
    else {  // round 1's form, for A/B runs
        uint64_t n_tiles = (n_len - head) / kTile;
        unsigned long long* partial = nullptr;
        if (n_tiles && hipMallocAsync(reinterpret_cast<void**>(&partial), n_tiles * 8, s) != hipSuccess) {
            (void)hipGetLastError();
            g_reduce_fallbacks.fetch_add(1, std::memory_order_relaxed);
            n_tiles = 0;
        }
        if (n_tiles) {
            const uint8_t* p = n + head;
            split_launches(n_tiles, kRedBlock, [&](uint64_t first, uint64_t m) {
                const bool xi = g_reduce_xi.load(std::memory_order_relaxed) != 0;
                if (allow_n && xi) hipLaunchKernelGGL((validate_tiles<U, true, true>), dim3((unsigned)m), dim3(kRedBlock), 0, s, p + first * kTile, m, partial + first, xcd_shift());
                else if (allow_n) hipLaunchKernelGGL((validate_tiles<U, true, false>), dim3((unsigned)m), dim3(kRedBlock), 0, s, p + first * kTile, m, partial + first, xcd_shift());
                else if (xi) hipLaunchKernelGGL((validate_tiles<U, false, true>), dim3((unsigned)m), dim3(kRedBlock), 0, s, p + first * kTile, m, partial + first, xcd_shift());
                else hipLaunchKernelGGL((validate_tiles<U, false, false>), dim3((unsigned)m), dim3(kRedBlock), 0, s, p + first * kTile, m, partial + first, xcd_shift());
            });
            hipLaunchKernelGGL(sum_partials, dim3(sum_partials_grid(n_tiles)), dim3(kRedBlock), 0, s, partial, n_tiles, count);
            if (head) {
                if (allow_n) hipLaunchKernelGGL((validate_generic<true>), dim3(1), dim3(kRedBlock), 0, s, n, (uint64_t)0, head, count);
                else hipLaunchKernelGGL((validate_generic<false>), dim3(1), dim3(kRedBlock), 0, s, n, (uint64_t)0, head, count);
            }
            const int rc = hip_rc(hipGetLastError());
            HIP_TRY(hipFreeAsync(partial, s));
            CNT_TRY(rc);
            done = head + n_tiles * kTile;
        }
    }
#endif
    if (done < n_len) {
        const unsigned g = generic_grid(n_len - done, kRedBlock);
        if (allow_n) hipLaunchKernelGGL((validate_generic<true>), dim3(g), dim3(kRedBlock), 0, s, n, done, (uint64_t)n_len, count);
        else hipLaunchKernelGGL((validate_generic<false>), dim3(g), dim3(kRedBlock), 0, s, n, done, (uint64_t)n_len, count);
        HIP_TRY(hipGetLastError());
    }
    return CNT_OK;
}

// ---- host tier: host_call (cute_nt.hip) ---------------------------------------------------
int cnt_hamming(const uint64_t* a, const uint64_t* b, size_t len, uint64_t* distance) {
    if (!distance) return CNT_EINVAL;
    const size_t bytes = cnt_words_for(len) * 8;
    // a result inside a stream it is computed from: refused before anything is written, *distance included
    if ((a && overlaps(distance, 8, a, bytes)) || (b && overlaps(distance, 8, b, bytes))) return CNT_EINVAL;
    *distance = 0;
    if (len == 0) return CNT_OK;
    if (!a || !b) return CNT_EINVAL;
    return host_call({{a, bytes, Dir::in}, {b, bytes, Dir::in}}, 16, distance, true,
                     [&](void* const* d, void* count, hipStream_t s) { return cnt_hamming_dev(d[0], d[1], len, count, s); });
}

static int host_unary(const uint64_t* bits, size_t len, uint64_t* out, int (*fn)(const void*, size_t, void*, void*)) {
    if (len == 0) return CNT_OK;
    if (!bits || !out) return CNT_EINVAL;
    const size_t bytes = cnt_words_for(len) * 8;
    return host_call({{bits, bytes, Dir::in}, {out, bytes, Dir::out}}, 0, nullptr, false,
                     [&](void* const* d, void*, hipStream_t s) { return fn(d[0], len, d[1], s); });
}

int cnt_complement(const uint64_t* bits, size_t len, uint64_t* out) { return host_unary(bits, len, out, cnt_complement_dev); }
int cnt_reverse_complement(const uint64_t* bits, size_t len, uint64_t* out) {
    return host_unary(bits, len, out, cnt_reverse_complement_dev);
}

int cnt_validate(const uint8_t* n, size_t n_len, unsigned flags, uint64_t* invalid) {
    if (!invalid) return CNT_EINVAL;
    if (n && overlaps(invalid, 8, n, n_len)) return CNT_EINVAL;  // before anything is written, *invalid included
    *invalid = 0;
    if (flags & ~CNT_ALLOW_N) return CNT_EINVAL;
    if (n_len == 0) return CNT_OK;
    if (!n) return CNT_EINVAL;
    return host_call({{n, n_len, Dir::in}}, 16, invalid, true,
                     [&](void* const* d, void* count, hipStream_t s) { return cnt_validate_dev(d[0], n_len, flags, count, s); });
}

}  // extern "C"
