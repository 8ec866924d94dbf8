// translate_abi.inc -- C-ABI entry points of codon translation (include/cute_nt.h, "translation"): cnt_translate_dev
// (enqueue-only on a caller stream: no allocation, no synchronisation, no scratch, capturable in a graph; the host table is read
// before the call returns and travels as kernel arguments) and cnt_translate (host tier: cute_nt.hip's host_call, staged through
// DevCtx::d_aux, or in place when the caller's buffers are pinned).  Included at the end of cute_nt.hip, behind extract_abi.inc.
#include "translate_kernels.hpp"

namespace {

static_assert(CNT_TRANSLATE_REVCOMP == kTranslateRevcomp, "the header's constant is the kernels'");

// NCBI table 1 in the order of the codon value x0 | x1 << 2 | x2 << 4 with A=0 C=1 T=2 G=3 (include/cute_nt.h "translation")
constexpr char kStandardCode[65] = "KQ*ETPSAILLVRR*GNHYDTPSAILFVSRCGNHYDTPSAILFVSRCGKQ*ETPSAMLLVRRWG";

// the argument checks both tiers share, before any device work; *out_bytes = M.  The caller has dealt with an unknown flag and
// with sub_len < 3.
int translate_args(const void* bits, size_t len, size_t start, size_t sub_len, const void* out, size_t out_cap, size_t* out_bytes) {
    if (start > len || sub_len > len - start) return CNT_EINVAL;
    const size_t M = sub_len / 3;
    if (!bits || !out || !aligned(bits, 8) || overlaps(out, M, bits, cnt_words_for(len) * 8)) return CNT_EINVAL;
    if (out_cap < M) return CNT_ECAP;
    *out_bytes = M;
    return CNT_OK;
}

// the launches of a call: the tiles of whole runs of 4096 output bytes behind the first 16-B boundary of the output, then the edge
// kernel on the `head` bytes in front of that boundary and on what is left behind the last tile.  A call with no whole tile behind
// the boundary (M < head + 4096) launches no tile: the edge kernel takes all of it from byte 0, so no tile ever starts off a 16-B
// boundary.
int translate_launch(const TranslateArgs& a, uint64_t M, hipStream_t s) {
    uint64_t head = (16 - (reinterpret_cast<uintptr_t>(a.out) & 15)) & 15;
    const uint64_t tiles = M < head + kTranslateTileBytes ? 0 : (M - head) / kTranslateTileBytes;
    if (!tiles) head = 0;  // no tile behind the boundary: one edge launch on [0, M)
    split_launches(tiles, kTranslateBlock, [&](uint64_t first, uint64_t count) {
        hipLaunchKernelGGL(a.rev ? translate_tiles_rev : translate_tiles_fwd, dim3((unsigned)count), dim3(kTranslateBlock), 0, s, a, head, first);
    });
    auto edge = [&](uint64_t j0, uint64_t j1) {  // output bytes [j0, j1): fewer than 4096 + 16
        hipLaunchKernelGGL(translate_edge, dim3((unsigned)((j1 - j0 + kTranslateBlock - 1) / kTranslateBlock)), dim3(kTranslateBlock), 0, s, a, j0, (uint32_t)(j1 - j0));
    };
    if (head) edge(0, head);
    if (head + tiles * kTranslateTileBytes < M) edge(head + tiles * kTranslateTileBytes, M);
    return hip_rc(hipGetLastError());
}

}  // namespace

extern "C" {

int cnt_translate_dev(const void* d_bits, size_t len, size_t start, size_t sub_len, unsigned flags, const uint8_t* table, void* d_out, size_t out_cap,
                      void* stream) {
    if (flags & ~CNT_TRANSLATE_REVCOMP) return CNT_EINVAL;
    if (sub_len < 3) return CNT_OK;
    size_t M = 0;
    CNT_TRY(translate_args(d_bits, len, start, sub_len, d_out, out_cap, &M));
    TranslateArgs a = {static_cast<const uint8_t*>(d_bits), cnt_words_for(len), start, sub_len, static_cast<uint8_t*>(d_out),
                       (flags & CNT_TRANSLATE_REVCOMP) ? 1u : 0u, {}};
    const uint8_t* t = table ? table : reinterpret_cast<const uint8_t*>(kStandardCode);
    uint8_t staged[64];
    for (unsigned c = 0; c < 64; ++c)  // reversed: table o rc3 -- the outer codes swapped, all three complemented
        staged[c] = t[a.rev ? (((c >> 4) | (c & 0xCu) | ((c & 3u) << 4)) ^ 0x2Au) : c];
    memcpy(a.table, staged, 64);
    return translate_launch(a, M, static_cast<hipStream_t>(stream));
}

int cnt_translate(const uint64_t* bits, size_t len, size_t start, size_t sub_len, unsigned flags, const uint8_t* table, uint8_t* out, size_t out_cap) {
    if (flags & ~CNT_TRANSLATE_REVCOMP) return CNT_EINVAL;
    if (sub_len < 3) return CNT_OK;
    size_t M = 0;
    CNT_TRY(translate_args(bits, len, start, sub_len, out, out_cap, &M));
    return host_call({{bits, cnt_words_for(len) * 8, Dir::in}, {out, M, Dir::out}}, 0, nullptr, false,
                     [&](void* const* d, void*, hipStream_t s) { return cnt_translate_dev(d[0], len, start, sub_len, flags, table, d[1], M, s); });
}

}  // extern "C"
