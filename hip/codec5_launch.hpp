// codec5_launch.hpp -- kernel-variant tables + launchers of the 5-letter codec (see
// codec2_launch.hpp for the conventions: variant 0 = shipped default, the rest selectable
// through cnt_set_tuning("encode2" / "decode2", i) for A/B runs).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec2_launch.hpp"
#include "codec5_kernels.hpp"

namespace cnt {

// A row holds its kernel's shape as data (codec2_launch.hpp: the row macros below derive it, and the launch function, from the
// kernel's template arguments).  Launches are counted in WAVE tiles of tile_nt nucleotides; a workgroup takes `waves` of them.
struct Encode2Variant {
    const char* name;
    uint32_t tile_nt;  // nucleotides per wave tile: wpl * 1728
    uint32_t block;    // threads per workgroup: waves * 64
    uint32_t wg_cap;   // resident workgroups per CU (0 = no cap): dynamic LDS on top of `slab`
    uint32_t waves;    // wave tiles per workgroup; only one-wave workgroups carry the edge items
    uint32_t wpl;      // words per lane
    uint32_t pipe_k;   // consecutive tiles per wave of the pipelined kernels (whole groups only), 0 = not pipelined
    uint32_t slab;     // the kernel's static LDS, in the 512-B granules it is allocated in
    TileLaunchFn<Encode2Edges> launch[2];  // [STRICT]
};
using Page2LaunchFn = void (*)(const uint64_t* bits, uint64_t words, uint8_t* out, uint64_t nt0, uint64_t n_tiles, uint32_t lds, uint32_t xs, const Decode2PageEdges& e, hipStream_t s);
struct Decode2Variant {
    const char* name;
    uint32_t tile_nt;  // as Encode2Variant's; page-tiled rows: pages * 4096
    uint32_t block, wg_cap, waves, wpl, pipe_k;
    uint32_t pages;    // 4-KiB output pages per wave of the page-tiled kernel, 0 = word-tiled (what decides which launcher takes the row)
    uint32_t slab;
    TileLaunchFn<Decode2Edges> launch;  // word-tiled rows (launch_decode2)
    Page2LaunchFn page_launch;          // page-tiled rows (launch_decode2_page)
};
// the wave kernels' slab is 3488 B per wave at 2 words per lane, 6944 B at 4
constexpr uint32_t wave_slab5(int waves, int wpl) { return waves == 4 ? 14336u : waves == 2 || wpl == 4 ? 7168u : 3584u; }
constexpr uint32_t kPipeSlab5 = 4608u;  // the pipelined slab is a full 4 KiB (+16 B)

template <int W, int P, int L, int S, int C, bool STRICT>
void encode2_wave_launch(const uint8_t* in, uint8_t* out, uint64_t n, uint32_t lds, uint32_t xs, const Encode2Edges& e, hipStream_t s) {
    hipLaunchKernelGGL((n_to_bits2_wave<W, P, L, S, STRICT, C>), dim3(grid_of((n + W - 1) / W)), dim3(W * 64), lds, s, in, out, n, xs, e);
}
template <int K, int L, int S, bool STRICT>
void encode2_pipe_launch(const uint8_t* in, uint8_t* out, uint64_t n, uint32_t lds, uint32_t, const Encode2Edges& e, hipStream_t s) {
    hipLaunchKernelGGL((n_to_bits2_pipe<K, L, S, STRICT>), dim3(grid_of(n / K)), dim3(64), lds, s, in, out, e);
}
// n_to_bits2_wave<W, P, L, S, STRICT, C>: W waves per workgroup, P words per lane, load / store policies L / S, C tiles per XCD turn
#define CNT_ENC2(name, W, P, L, S, C, cap) \
    {name, (P) * kWaveBytes5, (W) * 64, cap, W, P, 0, wave_slab5(W, P), {encode2_wave_launch<W, P, L, S, C, false>, encode2_wave_launch<W, P, L, S, C, true>}}
// n_to_bits2_pipe<K, L, S, STRICT>: one wave, 2 words per lane, K tiles per wave
#define CNT_ENC2P(name, K, L, S, cap) \
    {name, 2 * kWaveBytes5, 64, cap, 1, 2, K, kPipeSlab5, {encode2_pipe_launch<K, L, S, false>, encode2_pipe_launch<K, L, S, true>}}
constexpr Encode2Variant kEncode2Variants[] = {
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc1, 15 wg/CU", 1, 2, kNT, kSC1, 1, 15),  // 0: default
#ifdef CNT_LAB_VARIANTS
    CNT_ENC2("wave-tiled 4 words/lane, 1 wave/wg, ld=nt st=sc1", 1, 4, kNT, kSC1, 1, 0),  // 1
    CNT_ENC2("wave-tiled 2 words/lane, 2 waves/wg, ld=nt st=sc1", 2, 2, kNT, kSC1, 1, 0),  // 2
    CNT_ENC2("wave-tiled 2 words/lane, 4 waves/wg, ld=nt st=sc1", 4, 2, kNT, kSC1, 1, 0),  // 3
    CNT_ENC2("wave-tiled 1 word/lane, 1 wave/wg, ld=nt st=sc1 (tiles split cache lines)", 1, 1, kNT, kSC1, 1, 0),  // 4
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, plain", 1, 2, 0, 0, 1, 0),  // 5
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc1", 1, 2, kNT, kSC1, 1, 0),  // 6: as 0 without the residency cap
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc1, 20 wg/CU", 1, 2, kNT, kSC1, 1, 20),  // 7
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc1, 16 wg/CU", 1, 2, kNT, kSC1, 1, 16),  // 8
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-pairs, ld=nt st=sc1, 24 wg/CU", 1, 2, kNT, kSC1, 2, 24),  // 9
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-pairs, ld=nt st=sc0|sc1|nt, 24 wg/CU", 1, 2, kNT, kAll, 2, 24),  // 10
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc1, 12 wg/CU", 1, 2, kNT, kSC1, 1, 12),  // 11
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc1, 14 wg/CU", 1, 2, kNT, kSC1, 1, 14),  // 12
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc1, 18 wg/CU", 1, 2, kNT, kSC1, 1, 18),  // 13
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc1, 10 wg/CU", 1, 2, kNT, kSC1, 1, 10),  // 14
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc1, 24 wg/CU", 1, 2, kNT, kSC1, 1, 24),  // 15: the default before the caps were re-swept
    // round 2: 4 words per lane (6912 B of ASCII per wave) was only ever measured uncapped (variant 1); the fused 2-bit
    // kernel's sweep says fat one-wave tiles want a LOW residency cap
    CNT_ENC2("wave-tiled 4 words/lane, 1 wave/wg, ld=nt st=sc1, 7 wg/CU", 1, 4, kNT, kSC1, 1, 7),  // 16
    CNT_ENC2("wave-tiled 4 words/lane, 1 wave/wg, ld=nt st=sc1, 8 wg/CU", 1, 4, kNT, kSC1, 1, 8),  // 17
    CNT_ENC2("wave-tiled 4 words/lane, 1 wave/wg, ld=nt st=sc1, 9 wg/CU", 1, 4, kNT, kSC1, 1, 9),  // 18
    CNT_ENC2("wave-tiled 4 words/lane, 1 wave/wg, ld=nt st=sc1, 10 wg/CU", 1, 4, kNT, kSC1, 1, 10),  // 19
    CNT_ENC2("wave-tiled 4 words/lane, 1 wave/wg, ld=nt st=sc1, 12 wg/CU", 1, 4, kNT, kSC1, 1, 12),  // 20
    CNT_ENC2("wave-tiled 4 words/lane, 1 wave/wg, ld=nt st=sc0|sc1|nt, 8 wg/CU", 1, 4, kNT, kAll, 1, 8),  // 21
    // round 3: the default shape with the store / load policies that were only ever measured together with other changes
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc0|sc1|nt, 15 wg/CU", 1, 2, kNT, kAll, 1, 15),  // 22
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc1|nt, 15 wg/CU", 1, 2, kNT, kSC1 | kNT, 1, 15),  // 23
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=nt, 15 wg/CU", 1, 2, kNT, kNT, 1, 15),  // 24
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=sc1|nt st=sc1, 15 wg/CU", 1, 2, kSC1 | kNT, kSC1, 1, 15),  // 25
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=plain st=sc1, 15 wg/CU", 1, 2, 0, kSC1, 1, 15),  // 26
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, ld=nt st=sc0|sc1|nt, 14 wg/CU", 1, 2, kNT, kAll, 1, 14),  // 27
    // round 4: pipelined -- one wave takes K consecutive tiles and loads tile i+1 before it touches tile i (codec5_kernels.hpp)
    CNT_ENC2P("pipelined K=2, ld=nt st=sc1, 15 wg/CU", 2, kNT, kSC1, 15),  // 28
    CNT_ENC2P("pipelined K=2, ld=nt st=sc1, 12 wg/CU", 2, kNT, kSC1, 12),  // 29
    CNT_ENC2P("pipelined K=2, ld=nt st=sc1, 10 wg/CU", 2, kNT, kSC1, 10),  // 30
    CNT_ENC2P("pipelined K=4, ld=nt st=sc1, 15 wg/CU", 4, kNT, kSC1, 15),  // 31
    CNT_ENC2P("pipelined K=4, ld=nt st=sc1, 12 wg/CU", 4, kNT, kSC1, 12),  // 32
    CNT_ENC2P("pipelined K=4, ld=nt st=sc1, 10 wg/CU", 4, kNT, kSC1, 10),  // 33
    CNT_ENC2P("pipelined K=8, ld=nt st=sc1, 12 wg/CU", 8, kNT, kSC1, 12),  // 34
    CNT_ENC2P("pipelined K=8, ld=nt st=sc1, 8 wg/CU", 8, kNT, kSC1, 8),  // 35
    CNT_ENC2P("pipelined K=2, ld=nt st=sc1, 20 wg/CU", 2, kNT, kSC1, 20),  // 36
    CNT_ENC2P("pipelined K=4, ld=nt st=sc0|sc1|nt, 12 wg/CU", 4, kNT, kAll, 12),  // 37
    // multi-wave workgroups were only ever measured uncapped (variants 2, 3): four waves = 4 KiB of packed output per workgroup
    CNT_ENC2("wave-tiled 2 words/lane, 4 waves/wg, ld=nt st=sc1, 3 wg/CU", 4, 2, kNT, kSC1, 1, 3),  // 38
    CNT_ENC2("wave-tiled 2 words/lane, 4 waves/wg, ld=nt st=sc1, 4 wg/CU", 4, 2, kNT, kSC1, 1, 4),  // 39
    CNT_ENC2("wave-tiled 2 words/lane, 4 waves/wg, ld=nt st=sc1, 5 wg/CU", 4, 2, kNT, kSC1, 1, 5),  // 40
    CNT_ENC2("wave-tiled 2 words/lane, 2 waves/wg, ld=nt st=sc1, 7 wg/CU", 2, 2, kNT, kSC1, 1, 7),  // 41
    CNT_ENC2("wave-tiled 2 words/lane, 2 waves/wg, ld=nt st=sc1, 8 wg/CU", 2, 2, kNT, kSC1, 1, 8),  // 42
    // 32 tiles = 27 whole 4-KiB pages of ASCII: the first group size at which every XCD turn reads whole pages
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-32s (27 pages per turn), ld=nt st=sc1, 15 wg/CU", 1, 2, kNT, kSC1, 32, 15),  // 43
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-32s, ld=nt st=sc1, 12 wg/CU", 1, 2, kNT, kSC1, 32, 12),  // 44
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-32s, ld=nt st=sc1, 18 wg/CU", 1, 2, kNT, kSC1, 32, 18),  // 45
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-quads, ld=nt st=sc1, 15 wg/CU", 1, 2, kNT, kSC1, 4, 15),  // 46: 4 KiB of packed OUTPUT per turn
    CNT_ENC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-8s, ld=nt st=sc1, 15 wg/CU", 1, 2, kNT, kSC1, 8, 15),  // 47
    // branch-free twin of variant 0 (the pipelined kernel with K = 1: all four loads and LDS writes without a lane mask)
    CNT_ENC2P("branch-free K=1, ld=nt st=sc1, 15 wg/CU", 1, kNT, kSC1, 15),  // 48
    CNT_ENC2P("branch-free K=1, ld=nt st=sc1, 16 wg/CU", 1, kNT, kSC1, 16),  // 49
    CNT_ENC2P("branch-free K=1, ld=nt st=sc1, 14 wg/CU", 1, kNT, kSC1, 14),  // 50
    CNT_ENC2P("branch-free K=1, ld=nt st=sc1, 18 wg/CU", 1, kNT, kSC1, 18),  // 51
#endif
};
constexpr int kNumEncode2Variants = sizeof(kEncode2Variants) / sizeof(kEncode2Variants[0]);
#undef CNT_ENC2
#undef CNT_ENC2P

template <int W, int P, int L, int S, int C>
void decode2_wave_launch(const uint8_t* in, uint8_t* out, uint64_t n, uint32_t lds, uint32_t xs, const Decode2Edges& e, hipStream_t s) {
    hipLaunchKernelGGL((bits_to_n2_wave<W, P, L, S, C>), dim3(grid_of((n + W - 1) / W)), dim3(W * 64), lds, s, in, out, n, xs, e);
}
template <int K, int L, int S>
void decode2_pipe_launch(const uint8_t* in, uint8_t* out, uint64_t n, uint32_t lds, uint32_t, const Decode2Edges& e, hipStream_t s) {
    hipLaunchKernelGGL((bits_to_n2_pipe<K, L, S>), dim3(grid_of(n / K)), dim3(64), lds, s, in, out, e);
}
template <int C, int L, int S, int PAGES>
void decode2_page_launch(const uint64_t* bits, uint64_t words, uint8_t* out, uint64_t nt0, uint64_t n, uint32_t lds, uint32_t xs, const Decode2PageEdges& e, hipStream_t s) {
    hipLaunchKernelGGL((bits_to_n2_page<C, L, S, PAGES>), dim3(grid_of(n)), dim3(64), lds, s, bits, words, out, nt0, (uint32_t)n, xs, e);
}
// the arguments as encode's; bits_to_n2_page<C, L, kAll, P>: one wave per P 4-KiB pages of the ASCII (write) stream
#define CNT_DEC2(name, W, P, L, S, C, cap) {name, (P) * kWaveBytes5, (W) * 64, cap, W, P, 0, 0, wave_slab5(W, P), decode2_wave_launch<W, P, L, S, C>, nullptr}
#define CNT_DEC2P(name, K, L, S, cap) {name, 2 * kWaveBytes5, 64, cap, 1, 2, K, 0, kPipeSlab5, decode2_pipe_launch<K, L, S>, nullptr}
#define CNT_DEC2PG(name, C, L, P, cap) {name, (P) * kPageNt5, 64, cap, 1, 0, 0, P, PageTile5<P>::kSlabDwords * 4, nullptr, decode2_page_launch<C, L, kAll, P>}
constexpr Decode2Variant kDecode2Variants[] = {
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-quads, ld=plain st=sc0|sc1|nt, 16 wg/CU", 1, 2, 0, kAll, 4, 16),  // 0: default
#ifdef CNT_LAB_VARIANTS
    CNT_DEC2("wave-tiled 4 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt", 1, 4, 0, kAll, 1, 0),  // 1
    CNT_DEC2("wave-tiled 2 words/lane, 2 waves/wg, ld=plain st=sc0|sc1|nt", 2, 2, 0, kAll, 1, 0),  // 2
    CNT_DEC2("wave-tiled 2 words/lane, 4 waves/wg, ld=plain st=sc0|sc1|nt", 4, 2, 0, kAll, 1, 0),  // 3
    CNT_DEC2("wave-tiled 1 word/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt (tiles split cache lines)", 1, 1, 0, kAll, 1, 0),  // 4
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, plain", 1, 2, 0, 0, 1, 0),  // 5
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt", 1, 2, 0, kAll, 1, 0),  // 6: as 0 without the residency cap
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 20 wg/CU", 1, 2, 0, kAll, 1, 20),  // 7
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 16 wg/CU", 1, 2, 0, kAll, 1, 16),  // 8
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 24 wg/CU", 1, 2, 0, kAll, 1, 24),  // 9: as 0 without the XCD pairing
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-pairs, ld=nt st=sc0|sc1|nt, 24 wg/CU", 1, 2, kNT, kAll, 2, 24),  // 10
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-pairs, ld=plain st=sc0|sc1|nt, 15 wg/CU", 1, 2, 0, kAll, 2, 15),  // 11
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-pairs, ld=plain st=sc0|sc1|nt, 12 wg/CU", 1, 2, 0, kAll, 2, 12),  // 12
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 12 wg/CU", 1, 2, 0, kAll, 1, 12),  // 13
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 14 wg/CU", 1, 2, 0, kAll, 1, 14),  // 14
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 10 wg/CU", 1, 2, 0, kAll, 1, 10),  // 15
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-pairs, ld=plain st=sc0|sc1|nt, 18 wg/CU", 1, 2, 0, kAll, 2, 18),  // 16
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-pairs, ld=plain st=sc0|sc1|nt, 20 wg/CU", 1, 2, 0, kAll, 2, 20),  // 17
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-pairs, ld=plain st=sc0|sc1|nt, 24 wg/CU", 1, 2, 0, kAll, 2, 24),  // 18: the default before the caps were re-swept
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-pairs, ld=plain st=sc0|sc1|nt, 16 wg/CU", 1, 2, 0, kAll, 2, 16),  // 19: the default before the XCD group size was re-swept
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-quads, ld=plain st=sc0|sc1|nt, 15 wg/CU", 1, 2, 0, kAll, 4, 15),  // 20
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-quads, ld=plain st=sc0|sc1|nt, 18 wg/CU", 1, 2, 0, kAll, 4, 18),  // 21
    CNT_DEC2("wave-tiled 4 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 7 wg/CU", 1, 4, 0, kAll, 1, 7),  // 22
    CNT_DEC2("wave-tiled 4 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 8 wg/CU", 1, 4, 0, kAll, 1, 8),  // 23
    CNT_DEC2("wave-tiled 4 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 9 wg/CU", 1, 4, 0, kAll, 1, 9),  // 24
    CNT_DEC2("wave-tiled 4 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 10 wg/CU", 1, 4, 0, kAll, 1, 10),  // 25
    CNT_DEC2("wave-tiled 4 words/lane, 1 wave/wg, ld=plain st=sc0|sc1|nt, 12 wg/CU", 1, 4, 0, kAll, 1, 12),  // 26
    CNT_DEC2("wave-tiled 4 words/lane, 1 wave/wg, xcd-pairs, ld=plain st=sc0|sc1|nt, 8 wg/CU", 1, 4, 0, kAll, 2, 8),  // 27
    CNT_DEC2("wave-tiled 4 words/lane, 1 wave/wg, xcd-pairs, ld=plain st=sc0|sc1|nt, 9 wg/CU", 1, 4, 0, kAll, 2, 9),  // 28
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-quads, ld=plain st=sc1|nt, 16 wg/CU", 1, 2, 0, kSC1 | kNT, 4, 16),  // 29
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-quads, ld=nt st=sc0|sc1|nt, 16 wg/CU", 1, 2, kNT, kAll, 4, 16),  // 30
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-quads, ld=sc1 st=sc0|sc1|nt, 16 wg/CU", 1, 2, kSC1, kAll, 4, 16),  // 31
    // round 4: pipelined -- one wave takes K consecutive tiles and loads tile i+1's words before it expands tile i
    CNT_DEC2P("pipelined K=2, ld=plain st=sc0|sc1|nt, 16 wg/CU", 2, 0, kAll, 16),  // 32
    CNT_DEC2P("pipelined K=2, ld=plain st=sc0|sc1|nt, 12 wg/CU", 2, 0, kAll, 12),  // 33
    CNT_DEC2P("pipelined K=4, ld=plain st=sc0|sc1|nt, 16 wg/CU", 4, 0, kAll, 16),  // 34
    CNT_DEC2P("pipelined K=4, ld=plain st=sc0|sc1|nt, 12 wg/CU", 4, 0, kAll, 12),  // 35
    CNT_DEC2P("pipelined K=4, ld=plain st=sc0|sc1|nt, 10 wg/CU", 4, 0, kAll, 10),  // 36
    CNT_DEC2P("pipelined K=8, ld=plain st=sc0|sc1|nt, 12 wg/CU", 8, 0, kAll, 12),  // 37
    CNT_DEC2P("pipelined K=8, ld=plain st=sc0|sc1|nt, 8 wg/CU", 8, 0, kAll, 8),  // 38
    CNT_DEC2P("pipelined K=2, ld=plain st=sc0|sc1|nt, 20 wg/CU", 2, 0, kAll, 20),  // 39
    CNT_DEC2P("pipelined K=4, ld=plain st=sc0|sc1|nt, 20 wg/CU", 4, 0, kAll, 20),  // 40
    // four waves = one 4-KiB page of packed input per workgroup, under a residency cap for the first time
    CNT_DEC2("wave-tiled 2 words/lane, 4 waves/wg, ld=plain st=sc0|sc1|nt, 3 wg/CU", 4, 2, 0, kAll, 1, 3),  // 41
    CNT_DEC2("wave-tiled 2 words/lane, 4 waves/wg, ld=plain st=sc0|sc1|nt, 4 wg/CU", 4, 2, 0, kAll, 1, 4),  // 42
    CNT_DEC2("wave-tiled 2 words/lane, 4 waves/wg, ld=plain st=sc0|sc1|nt, 5 wg/CU", 4, 2, 0, kAll, 1, 5),  // 43
    CNT_DEC2("wave-tiled 2 words/lane, 2 waves/wg, ld=plain st=sc0|sc1|nt, 7 wg/CU", 2, 2, 0, kAll, 1, 7),  // 44
    CNT_DEC2("wave-tiled 2 words/lane, 2 waves/wg, ld=plain st=sc0|sc1|nt, 8 wg/CU", 2, 2, 0, kAll, 1, 8),  // 45
    // 32 tiles per XCD turn: 27 whole pages of the WRITE stream (and 8 of the read stream) per turn
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-32s, ld=plain st=sc0|sc1|nt, 16 wg/CU", 1, 2, 0, kAll, 32, 16),  // 46
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-32s, ld=plain st=sc0|sc1|nt, 14 wg/CU", 1, 2, 0, kAll, 32, 14),  // 47
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-8s, ld=plain st=sc0|sc1|nt, 16 wg/CU", 1, 2, 0, kAll, 8, 16),  // 48
    CNT_DEC2("wave-tiled 2 words/lane, 1 wave/wg, xcd-16s, ld=plain st=sc0|sc1|nt, 16 wg/CU", 1, 2, 0, kAll, 16, 16),  // 49
    // page tiles: one wave per 4-KiB page of the ASCII (write) stream, bits_to_n2_page
    CNT_DEC2PG("page-tiled, plain order, ld=plain st=sc0|sc1|nt, 12 wg/CU", 1, 0, 1, 12),  // 50
    CNT_DEC2PG("page-tiled, plain order, ld=plain st=sc0|sc1|nt, 13 wg/CU", 1, 0, 1, 13),  // 51
    CNT_DEC2PG("page-tiled, plain order, ld=plain st=sc0|sc1|nt, 14 wg/CU", 1, 0, 1, 14),  // 52
    CNT_DEC2PG("page-tiled, plain order, ld=plain st=sc0|sc1|nt, 11 wg/CU", 1, 0, 1, 11),  // 53
    CNT_DEC2PG("page-tiled, plain order, ld=plain st=sc0|sc1|nt, 10 wg/CU", 1, 0, 1, 10),  // 54
    CNT_DEC2PG("page-tiled, plain order, ld=plain st=sc0|sc1|nt, 16 wg/CU", 1, 0, 1, 16),  // 55
    CNT_DEC2PG("page-tiled, xcd-quads, ld=plain st=sc0|sc1|nt, 12 wg/CU", 4, 0, 1, 12),  // 56
    CNT_DEC2PG("page-tiled, xcd-pairs, ld=plain st=sc0|sc1|nt, 12 wg/CU", 2, 0, 1, 12),  // 57
    CNT_DEC2PG("page-tiled, plain order, ld=nt st=sc0|sc1|nt, 12 wg/CU", 1, kNT, 1, 12),  // 58
    CNT_DEC2PG("page-tiled, plain order, ld=plain st=sc0|sc1|nt, 18 wg/CU", 1, 0, 1, 18),  // 59
    CNT_DEC2PG("page-tiled, plain order, ld=plain st=sc0|sc1|nt, 20 wg/CU", 1, 0, 1, 20),  // 60
    CNT_DEC2PG("page-tiled, plain order, ld=plain st=sc0|sc1|nt, 24 wg/CU", 1, 0, 1, 24),  // 61
    CNT_DEC2PG("page-tiled, plain order, ld=plain st=sc0|sc1|nt, 30 wg/CU", 1, 0, 1, 30),  // 62
    CNT_DEC2PG("page-tiled, xcd-quads, ld=plain st=sc0|sc1|nt, 20 wg/CU", 4, 0, 1, 20),  // 63
    // two pages per wave: 305 words in five rounds (95 % of the expansion lanes busy, against 80 % with one page)
    CNT_DEC2PG("2-page-tiled, plain order, ld=plain st=sc0|sc1|nt, 6 wg/CU", 1, 0, 2, 6),  // 64
    CNT_DEC2PG("2-page-tiled, plain order, ld=plain st=sc0|sc1|nt, 7 wg/CU", 1, 0, 2, 7),  // 65
    CNT_DEC2PG("2-page-tiled, plain order, ld=plain st=sc0|sc1|nt, 8 wg/CU", 1, 0, 2, 8),  // 66
    CNT_DEC2PG("2-page-tiled, plain order, ld=plain st=sc0|sc1|nt, 9 wg/CU", 1, 0, 2, 9),  // 67
    CNT_DEC2PG("2-page-tiled, plain order, ld=plain st=sc0|sc1|nt, 10 wg/CU", 1, 0, 2, 10),  // 68
    CNT_DEC2PG("2-page-tiled, plain order, ld=plain st=sc0|sc1|nt, 12 wg/CU", 1, 0, 2, 12),  // 69
    // branch-free twin of the word-tiled kernel (the pipelined kernel with K = 1; plain order)
    CNT_DEC2P("branch-free K=1, ld=plain st=sc0|sc1|nt, 16 wg/CU", 1, 0, kAll, 16),  // 70
    CNT_DEC2P("branch-free K=1, ld=plain st=sc0|sc1|nt, 14 wg/CU", 1, 0, kAll, 14),  // 71
    CNT_DEC2P("branch-free K=1, ld=plain st=sc0|sc1|nt, 18 wg/CU", 1, 0, kAll, 18),  // 72
#endif
};
constexpr int kNumDecode2Variants = sizeof(kDecode2Variants) / sizeof(kDecode2Variants[0]);
#undef CNT_DEC2
#undef CNT_DEC2P
#undef CNT_DEC2PG

// Whole wave tiles of [d_n, d_n + n_len) plus -- for the one-wave variants, in the same (last) launch -- the edge words `e`
// describes; *done_words = words the tiles cover (0: nothing was launched), *edges_done = whether the edges rode along
// (the multi-wave variants leave them to the caller's generic launches).
template <bool STRICT>
int launch_encode2(int variant, const void* d_n, void* d_out, uint64_t n_len, Encode2Edges e, hipStream_t s, uint64_t* done_words, bool* edges_done,
                   BadCounter bad = BadCounter()) {
    if (bad) variant = 0;  // the checked twin exists for the shipped shape only
    if (variant < 0 || variant >= kNumEncode2Variants) return 1;
    const Encode2Variant& v = kEncode2Variants[variant];
    const uint64_t tile_nt = v.tile_nt, tile_words = tile_nt / 27;
    const uint64_t group = v.pipe_k ? v.pipe_k : 1;  // pipelined: whole groups of K tiles (one workgroup each), the rest are edge words
    const uint64_t total = n_len / tile_nt / group * group;
    *done_words = total * tile_words;
    const bool one_wave = v.waves == 1;
    *edges_done = one_wave && total > 0;
    e.tail_first = e.head_words + *done_words;
    const uint64_t per_launch = max_tiles_per_launch(64) / 8 * 8;  // wave tiles per launch (<= 2^31-1 threads; whole pipeline groups; the XCD maps are bijections for any count)
    const uint32_t xs = xcd_shift();
    const uint32_t lds = lds_pad_for_cap(v.wg_cap, v.slab);
    for_each_launch(total, per_launch, [&](uint64_t first, uint64_t n, bool last) {
        const uint8_t* in = static_cast<const uint8_t*>(d_n) + first * tile_nt;
        uint8_t* out = static_cast<uint8_t*>(d_out) + first * tile_words * 8;
        e.groups = last && one_wave ? edge_groups(e.head_words + (e.words - e.tail_first), 64, n / group) : 0u;
        if (bad)
            hipLaunchKernelGGL((n_to_bits2_wave_checked<2, kNT, kSC1, STRICT>), dim3(grid_of(n)), dim3(64), lds, s, in, out, n, xs, e, bad.p, bad.mask);
        else
            v.launch[STRICT](in, out, n, lds, xs, e, s);
    });
    return 0;
}

// The any-alignment companion of encode2 variant 0: `base` = input pointer rounded down to 128 B,
// `phase` = the 1..127 bytes dropped.  Same LDS footprint per workgroup as variant 0 (15 wg/CU).
constexpr uint32_t kWindowEncode2Tile = 2 * kWaveBytes5;  // nt per tile (128 words)
constexpr uint32_t kWindowEncode2Slack = 128;             // bytes a tile may read behind its end
template <bool STRICT>
void launch_encode2_window(const uint8_t* base, uint32_t phase, uint8_t* out, uint64_t total_tiles, Encode2Edges e, hipStream_t s, BadCounter bad = BadCounter()) {
    const uint32_t xs = xcd_shift();
    const uint32_t lds = lds_pad_for_cap(kEncode2Variants[0].wg_cap, kWindowSlabDwords5 * 4u);  // four whole wave rows: 640 B more than variant 0's
    e.tail_first = e.head_words + total_tiles * (kWindowEncode2Tile / 27);
    for_each_launch(total_tiles, max_tiles_per_launch(64) / 4 * 4, [&](uint64_t first, uint64_t n, bool last) {
        e.groups = last ? edge_groups(e.head_words + (e.words - e.tail_first), 64, n) : 0u;
        if (bad)
            hipLaunchKernelGGL((n_to_bits2_window_checked<kNT, kSC1, STRICT, 1>), dim3(grid_of(n)), dim3(64), lds, s,
                               base + first * kWindowEncode2Tile, out + first * 1024, n, phase, xs, e, bad.p, bad.mask);
        else
            hipLaunchKernelGGL((n_to_bits2_window<kNT, kSC1, STRICT, 1>), dim3(grid_of(n)), dim3(64), lds, s,
                               base + first * kWindowEncode2Tile, out + first * 1024, n, phase, xs, e);
    });
}

// As launch_encode2, for the word-tiled rows; a page-tiled row (launch_decode2_page's) is a bad variant here.
inline int launch_decode2(int variant, const void* d_bits, void* d_out, uint64_t len, Decode2Edges e, hipStream_t s, uint64_t* done_words, bool* edges_done) {
    if (variant < 0 || variant >= kNumDecode2Variants || kDecode2Variants[variant].pages) return 1;
    const Decode2Variant& v = kDecode2Variants[variant];
    const uint64_t tile_nt = v.tile_nt, tile_words = tile_nt / 27;
    const uint64_t group = v.pipe_k ? v.pipe_k : 1;
    const uint64_t total = len / tile_nt / group * group;
    *done_words = total * tile_words;
    const bool one_wave = v.waves == 1;
    *edges_done = one_wave && total > 0;
    e.tail_first = e.head_words + *done_words;
    const uint32_t xs = xcd_shift();
    const uint32_t lds = lds_pad_for_cap(v.wg_cap, v.slab);
    for_each_launch(total, max_tiles_per_launch(64) / 8 * 8, [&](uint64_t first, uint64_t n, bool last) {
        const uint8_t* in = static_cast<const uint8_t*>(d_bits) + first * tile_words * 8;
        uint8_t* out = static_cast<uint8_t*>(d_out) + first * tile_nt;
        e.groups = last && one_wave ? edge_groups(e.head_words + (e.words - e.tail_first), 64, n / group) : 0u;
        v.launch(in, out, n, lds, xs, e, s);
    });
    return 0;
}

#ifdef CNT_LAB_VARIANTS
// Page-tiled decode of a whole call: letters [0, head_nt) in front of the first 128-B line of d_out and the letters behind
// the last whole page ride as edge items in the (last) launch.  Returns 1 for a variant that is not page-tiled, -1 when the
// call holds no whole page (the caller's generic kernel takes it), 0 after launching.
inline int launch_decode2_page(int variant, const uint64_t* bits, uint64_t words, uint8_t* out, uint64_t len, hipStream_t s) {
    if (variant < 0 || variant >= kNumDecode2Variants || !kDecode2Variants[variant].pages) return 1;
    const Decode2Variant& v = kDecode2Variants[variant];
    const uint64_t tile_nt = v.tile_nt;
    const uint64_t head_nt = (128 - (reinterpret_cast<uintptr_t>(out) & 127)) & 127;
    if (len < head_nt + tile_nt) return -1;
    const uint64_t total = (len - head_nt) / tile_nt;
    Decode2PageEdges e{bits, out, len, head_nt, head_nt + total * tile_nt, 0};
    const uint64_t edge_items = (head_nt + 26) / 27 + (e.tail_from < len ? (len + 26) / 27 - e.tail_from / 27 : 0);
    const uint32_t xs = xcd_shift();
    const uint32_t lds = lds_pad_for_cap(v.wg_cap, v.slab);
    for_each_launch(total, max_tiles_per_launch(64) / 8 * 8, [&](uint64_t first, uint64_t n, bool last) {
        e.groups = last ? edge_groups(edge_items, 64, n) : 0u;
        v.page_launch(bits, words, out, head_nt + first * tile_nt, n, lds, xs, e, s);
    });
    return 0;
}
#endif

}  // namespace cnt
