// device_tier.inc -- the device-tier bodies every tier ends in (included inside cute_nt.hip's anonymous
// namespace): alignment plan, head / tail peeling and kernel selection for both codecs and the fused round trip.
// Enqueue-only: no synchronisation, no allocation.
// ---- device-tier bodies (shared by every tier) ------------------------------------
// Alignment plan (profiles/HISTORY.md 4.3a, profiles/r01_align_lab_*.json): stores that are not 64-B aligned cost ~30 %, loads
// off the 128-B line grid 6-11 %.  Both directions therefore peel a short head until the tile
// kernels' STORES sit on 128-B lines, and the load side takes whatever phase results: the stream
// kernels when it is zero, otherwise the window kernel (encode: line-aligned loads, phase applied
// to the packed codes) / the funnel-shifting twin (decode).  Any pointer the ABI accepts runs at
// (nearly) full speed.  The peeled head and the ragged end behind the last whole tile are work items
// of the tile kernel's own launch (DESIGN.md 4: the last workgroups take them after their tile), so a
// call is ONE launch; the generic kernels alone serve inputs shorter than a tile.
// CNT_TAIL_LUT as a word index: words >= lut_from take BYTE_LUT semantics.  2-bit codec: the final PARTIAL word
// (n_to_bits.rs:109-111: `if n.len() & 31 > 0 { ... n_to_bits_lut(&n[end_idx << 5..]) }`); 5-letter codec: every
// word from end_idx = (len - 5) / 27 on (n_to_bits2.rs:120,179-185 -- the 32-B loads of n_to_bits2_pext over-read
// 5 bytes, so its loop stops early and up to two trailing words go through n_to_bits2_lut).
inline uint64_t lut_from_of(size_t n_len, unsigned flags, int unit_nt) {
    if (!(flags & CNT_TAIL_LUT)) return kNoLutWord;
    if (unit_nt == 32) return (n_len & 31) ? (uint64_t)(n_len >> 5) : kNoLutWord;
    return n_len < 5 ? 0 : (uint64_t)((n_len - 5) / 27);
}
constexpr unsigned kEncodeFlags = CNT_STRICT_LUT | CNT_TAIL_LUT;
// the counter of a *_checked call: device memory, 8-byte aligned, never NULL (the unchecked entry points are the way to not count);
// CNT_SPREAD_COUNT (stripped from `flags` here): CNT_COUNT_SLOTS of them
inline bool checked_counter(void* p, unsigned* flags, BadCounter* out) {
    if (!p || !aligned(p, 8)) return false;
    *out = BadCounter(static_cast<unsigned long long*>(p), (*flags & CNT_SPREAD_COUNT) ? (uint32_t)CNT_COUNT_SLOTS - 1 : 0u);
    *flags &= ~CNT_SPREAD_COUNT;
    return true;
}

// `bad` (the *_checked entry points; nullptr otherwise): a device u64 the launch ADDS the number of bytes outside ACGTUacgtu to --
// counted by the same kernels in the same pass, every byte of the call by exactly one tile or edge item (codec2_kernels.hpp).
int encode_impl(const void* d_n, size_t n_len, void* d_out, size_t out_words, unsigned flags, uint64_t lut_from, hipStream_t s, BadCounter bad) {
    const size_t words = cnt_words_for(n_len);
    if (out_words < words) return CNT_ECAP;
    if (flags & ~kEncodeFlags) return CNT_EINVAL;
    if (n_len == 0) return CNT_OK;
    if (!d_n || !d_out || !aligned(d_out, 8) || overlaps(d_n, n_len, d_out, words * 8)) return CNT_EINVAL;
    const bool strict = (flags & CNT_STRICT_LUT) != 0;
    const uint8_t* n = static_cast<const uint8_t*>(d_n);
    uint64_t* out = static_cast<uint64_t*>(d_out);
    auto generic_only = [&]() -> int {
        const unsigned g = generic_grid(words);
        if (bad && strict)
            hipLaunchKernelGGL((n_to_bits_generic_checked<true>), dim3(g), dim3(kBlock), 0, s, n, (uint64_t)n_len, out, (uint64_t)0, (uint64_t)words, lut_from, bad.p, bad.mask);
        else if (bad)
            hipLaunchKernelGGL((n_to_bits_generic_checked<false>), dim3(g), dim3(kBlock), 0, s, n, (uint64_t)n_len, out, (uint64_t)0, (uint64_t)words, lut_from, bad.p, bad.mask);
        else if (strict)
            hipLaunchKernelGGL((n_to_bits_generic<true>), dim3(g), dim3(kBlock), 0, s, n, (uint64_t)n_len, out, (uint64_t)0, (uint64_t)words, lut_from);
        else
            hipLaunchKernelGGL((n_to_bits_generic<false>), dim3(g), dim3(kBlock), 0, s, n, (uint64_t)n_len, out, (uint64_t)0, (uint64_t)words, lut_from);
        return hip_rc(hipGetLastError());
    };
    if (n_len <= tune_small_nt() && (n_len % kEncodeStreamTile) != 0) return generic_only();
    // head: words until the output is on a 128-B LINE (512-B tiles that start on a half line cost 2 %,
    // profiles/r04_align_two_pass.jsonl; up to 15 words = 480 nt, and 16 words move the input by 512 B: its
    // phase does not depend on how far we peel); 512 nt more if the input phase is not zero, so that the window
    // kernel's rounded-down loads stay inside the caller's buffer
    uint64_t head_words = ((128 - (reinterpret_cast<uintptr_t>(d_out) & 127)) & 127) >> 3;
    const uint32_t phase = (uint32_t)((reinterpret_cast<uintptr_t>(n) + 32 * head_words) & 127);
    if (phase && head_words < 4) head_words += 16;  // 128 B of output, 512 B of input: both phases kept
    uint64_t main_nt = 0;
    if (n_len > 32 * head_words) {
        const uint64_t rem = n_len - 32 * head_words;
        const uint8_t* p = n + 32 * head_words;
        uint8_t* o = reinterpret_cast<uint8_t*>(out + head_words);
        // ONE launch: the tiles, and -- as extra workgroups of the same grid -- the head words and the ragged end
        const EncodeEdges e{n, out, (uint64_t)n_len, head_words, 0, (uint64_t)words, lut_from, 0};
        const int v = bad ? 0 : tune_encode();  // the checked twins exist for the shipped shapes only
        if (phase == 0 || ((phase & 15) == 0 && v != 0)) {  // a non-default variant is honoured whenever it can run
            if (strict ? launch_encode<true>(v, p, o, rem, e, s, &main_nt, bad) : launch_encode<false>(v, p, o, rem, e, s, &main_nt, bad))
                return CNT_EINVAL;
        } else if (rem >= kWindowEncodeTile + kWindowEncodeSlack) {
            const uint64_t tiles = (rem - kWindowEncodeSlack) / kWindowEncodeTile;
            if (strict) launch_encode_window<true>(p - phase, phase, o, tiles, e, s, bad);
            else launch_encode_window<false>(p - phase, phase, o, tiles, e, s, bad);
            main_nt = tiles * kWindowEncodeTile;
        }
        HIP_TRY(hipGetLastError());
    }
    if (main_nt == 0) return generic_only();  // shorter than a tile: nothing was launched above
    return CNT_OK;
}
int encode_dev(const void* d_n, size_t n_len, void* d_out, size_t out_words, unsigned flags, hipStream_t s) {
    return encode_impl(d_n, n_len, d_out, out_words, flags, lut_from_of(n_len, flags, 32), s, BadCounter());
}
int encode_checked_dev(const void* d_n, size_t n_len, void* d_out, size_t out_words, unsigned flags, void* d_invalid, hipStream_t s) {
    BadCounter bad;
    if (!checked_counter(d_invalid, &flags, &bad)) return CNT_EINVAL;
    return encode_impl(d_n, n_len, d_out, out_words, flags, lut_from_of(n_len, flags, 32), s, bad);
}

// Decode's tile map gives every XCD turn four consecutive 4-KiB output tiles = 4 KiB of the packed stream (codec2_kernels.hpp):
// on the grid that is one PAGE of the read stream per private L2 and turn, the property the map was chosen for.  Off the
// grid the output is peeled to a page and the packed stream starts wherever that leaves it: r = (address of the first tile's
// packed byte) mod 4096.  Peeling k more output pages (they join the head's byte-granular edge items: <= 12 288 letters of a
// call that has >= 2^20) moves every turn's packed piece by k KiB, so the turns can start within one KiB of a page of the
// packed buffer whatever r is.  `mode`: -1 the shipped rule, 0..3 a forced k, 10 / 11 the candidate rules (lab A/B:
// bench/decode_off_grid.py, profiles/r05_decode_off_grid.md).
inline uint32_t decode_turn_pages(uint32_t r, int mode) {
    if (mode >= 0 && mode <= 3) return (uint32_t)mode;
    const uint32_t after = (4u - (r >> 10)) & 3u;             // the turns start in [page, page + 1 KiB)
    const uint32_t nearest = (4u - ((r + 512u) >> 10)) & 3u;  // ... within 512 B of a page boundary, on either side
    // The shipped rule is `nearest` (profiles/r05_decode_off_grid.md, 64 offset pairs, every mode interleaved in one process,
    // four boxes): with round 4's kernels, against the aligned call, mean -3.1...-4.4 % where k = 0 had -5.2...-7.3 %, `after`
    // -4.5...-4.7 %, plain dispatch order -5.3...-7.5 % and the best k per offset (an oracle) -2.8...-3.9 %; with the window
    // kernel for streams off their lines -2.6...-2.9 %.  What no k reaches: the pairing of a tile's output page with its packed
    // piece (k moves both together; three of the 28 packed offsets lose 7-15 % under every map, plain order included) --
    // operand placement, the caller's.
    return mode == 10 ? after : nearest;
}

// Where decode_dev lays its tiles for buffers at these addresses (host arithmetic; also behind cnt_test_decode_plan, which
// tests/test_decode_plan.py walks over every packed offset and output phase on the CPU box):
//   head    nucleotides in front of the first tile: the output to its 128-B line -- for calls of >= 2^20 nt to its 4-KiB page,
//           so that every tile is one aligned page (worth 2-5 %, profiles/HISTORY.md 4.3a) --, then, for calls whose packed
//           stream no longer fits the Infinity Cache (> 2^30 nt: below that no page of the packed buffer is ever seen by HBM
//           twice and the turns' position measures as nothing, profiles/r05_decode_off_grid.md), the 0-3 further pages that
//           place the XCD turns (decode_turn_pages), then -- window kernel only -- the pages that keep the first window
//           inside the caller's buffer.  Everything in the head is spelled by the launch's edge items, 16 letters apiece.
//   window  the packed stream is off its 128-B lines (q != 0) or off its dwords (sh != 0): bits_to_n_window; else the
//           stream kernel.  (Lab build, tuning key "decode_window" = 0: round 4's kernels -- stream at any q, shifted for sh.)
//   tiles   whole 4-KiB output tiles; the window kernel's are also bounded by the end of the packed buffer (its last
//           window reads up to 12 bytes past the last dword it needs).
struct DecodePlan {
    uint64_t head = 0, tiles = 0;
    uint32_t q = 0, sh = 0;
    bool window = false;
};
// cache_nt: chip_info().cache_nt of the device the call runs on (2^30 on an SPX MI355X; a partitioned device answers less and
// takes the past-the-cache plan from a smaller size on) -- round 5 had the literal 2^30 here.
inline DecodePlan decode_plan(uintptr_t a_bits, uintptr_t a_out, uint64_t len, int rot_mode, bool use_window, uint64_t cache_nt) {
    DecodePlan p;
    const uint64_t grain = len >= ((uint64_t)1 << 20) ? 4096 : 128;
    p.head = (grain - (a_out & (grain - 1))) & (grain - 1);
    const bool past_cache = len > cache_nt;  // the packed stream (len / 4 bytes) no longer fits the device's share of the Infinity Cache
    if (grain == 4096 && (rot_mode >= 0 || past_cache))
        p.head += 4096 * (uint64_t)decode_turn_pages((uint32_t)((a_bits + 4 * (p.head >> 4)) & 4095), rot_mode);
    p.sh = 2 * (uint32_t)(p.head & 15);
    p.q = (uint32_t)(((a_bits + 4 * (p.head >> 4)) & 127) >> 2);
    p.window = use_window && past_cache && (p.q != 0 || p.sh != 0);
    if (p.window && (p.head >> 4) < p.q) p.head += grain == 4096 ? 4 * 4096 : 512;  // 128 B of packed words further on: q, sh and the turns keep their places
    if (len <= p.head) return p;
    p.tiles = (len - p.head) / kWindowDecodeTile;
    if (p.window) {
        const uintptr_t window = (a_bits + 4 * (p.head >> 4)) & ~(uintptr_t)127, end = a_bits + 8 * ((len + 31) >> 5);
        const uint64_t need = 16 * (uint64_t)((p.q + (p.sh ? 1u : 0u) + 3u) >> 2);  // bytes the last tile reads behind its 1 KiB
        const uint64_t fit = end > window + need ? (end - window - need) / (kWindowDecodeTile / 4) : 0;
        p.tiles = std::min(p.tiles, fit);
    }
    return p;
}

int decode_dev(const void* d_bits, size_t words, size_t len, void* d_out, unsigned flags, hipStream_t s) {
    if (len > (words << 5) || (words > (SIZE_MAX >> 5))) return CNT_ELEN;
    if (flags) return CNT_EINVAL;
    if (len == 0) return CNT_OK;
    if (!d_bits || !d_out || !aligned(d_bits, 8) || overlaps(d_bits, cnt_words_for(len) * 8, d_out, len)) return CNT_EINVAL;
    const size_t used_words = cnt_words_for(len);
    const uint64_t* bits = static_cast<const uint64_t*>(d_bits);
    uint8_t* out = static_cast<uint8_t*>(d_out);
    auto generic_only = [&]() -> int {
        hipLaunchKernelGGL(bits_to_n_generic, dim3(generic_grid(used_words)), dim3(kBlock), 0, s, bits, (uint64_t)len, out,
                           (uint64_t)0, (uint64_t)used_words);
        return hip_rc(hipGetLastError());
    };
    if (len <= tune_small_nt() && (len % kWindowDecodeTile) != 0) return generic_only();
    const DecodePlan p = decode_plan(reinterpret_cast<uintptr_t>(bits), reinterpret_cast<uintptr_t>(d_out), len, tune_decode_rot(), tune_decode_window(), decode_cache_nt());
    uint64_t main_nt = 0;
    if (len > p.head) {
        const uint64_t rem = len - p.head;
        const uint8_t* in = reinterpret_cast<const uint8_t*>(bits) + 4 * (p.head >> 4);  // dword of nucleotide `head`
        const DecodeEdges e{bits, out, p.head, 0, (uint64_t)len, 0};  // head + ragged end ride in the same launch
        if (p.window) {
            if (p.tiles) launch_decode_window(in - 4 * p.q, p.q, p.sh, out + p.head, p.tiles, e, s);
            main_nt = p.tiles * kWindowDecodeTile;
        } else if (p.sh == 0) {
            int v = tune_decode();
            if (!aligned(in, 16) && v == 4) v = 0;  // the lds variant loads 16-B vectors
            if (launch_decode(v, in, out + p.head, rem, e, s, &main_nt)) return CNT_EINVAL;
        } else {  // a bit phase inside the Infinity Cache: two adjacent dwords per lane through v_alignbit_b32
            const uint64_t tiles = rem / kShiftedDecodeTile;
            launch_decode_shifted(in, p.sh, out + p.head, tiles, e, s);
            main_nt = tiles * kShiftedDecodeTile;
        }
        HIP_TRY(hipGetLastError());
    }
    if (main_nt == 0) return generic_only();
    return CNT_OK;
}

// Where the any-alignment fused kernel's tiles lie, from the three addresses and the length alone (no device work; also
// behind cnt_test_round_trip_plan, which tests/test_round_trip_plan.py walks over every pointer phase on the CPU box).
// t0: the first nucleotide of the tiles -- its decoded letter sits on a 128-B line of d_back.  p0: the tiles' first packed
// dword -- its ADDRESS is on a 64-B segment (stores that split segments between instructions cost 11-18 %), the one in
// front of t0 or the one behind it.  w0: the nucleotide index of the window's first byte -- the line of d_n that holds the
// smaller of the two; phase / phase2 = how far behind it the decoded / the packed stream start.  Every start within two
// pages of d_back's first line x both segment choices is priced and the cheapest taken (same-process A/B over 28 offset
// triples on two boxes, profiles/r04_round_trip_plan_ab.jsonl: +1.8 / +2.0 % on the aligned call against +2.7 / +2.9 % for
// tiles on d_back's pages and the nearest segment, the plan of the first version):
//   * each further 128-B line a tile reads behind its own 4 KiB is read twice -- by it and by the tile that owns it, as a
//     rule on another XCD's L2 (FETCH_SIZE +3.1 % of the ASCII per line, profiles/r04_fused_any_alignment_traffic.json):
//     1.4 % of the call's traffic;
//   * a window that does not start a 4-KiB page of d_n splits every page of the input between two waves: about 1 %.
// Small buffers take the first line (two candidates): pages do not matter below 1 MiB and the head is the edge items'.
// `limit`: the tiles' window ends there -- n_len, or the start of the final partial word when that word takes another table
// (CNT_TAIL_LUT: BYTE_LUT's, n_to_bits.rs:109-111; the tiles know one).  `mode` is kRoundTripDefaultPlan in the product
// library; the lab build prices the first version's plan (0), "windows on pages at any read-ahead" (1) and "shortest
// read-ahead" (2) for the A/B.
struct RoundTripPlan {
    uint64_t t0 = 0, p0 = 0, tiles = 0;
    int64_t w0 = 0;
    uint32_t phase = 0, phase2 = 0;
};
inline RoundTripPlan round_trip_plan(uintptr_t a_n, uintptr_t a_bits, uintptr_t a_back, uint64_t n_len, uint64_t limit, int mode) {
    RoundTripPlan r;
    const bool big = n_len >= ((uint64_t)1 << 20);
    const uint64_t t00 = (128 - (a_back & 127)) & 127;
    uint64_t best = ~0ull;
    for (uint64_t k = 0; k < (big ? 64u : 2u); ++k) {
        const uint64_t t0 = t00 + 128 * k, m0 = (t0 + 15) >> 4;
        const uint64_t up = m0 + (((64 - ((a_bits + 4 * m0) & 63)) & 63) >> 2);  // first segment-aligned dword at or behind m0
        for (int c = 0; c < 2; ++c) {
            if (c == 1 && up < 16) break;
            const uint64_t cand = c == 0 ? up : up - 16;
            const uint64_t first = std::min<uint64_t>(t0, 16 * cand);
            const int64_t w = (int64_t)first - (int64_t)((a_n + first) & 127);  // window start, in nucleotides from d_n
            if (w < 0) continue;
            const uint64_t reach = (uint64_t)std::max<int64_t>((int64_t)t0 - w, (int64_t)(16 * cand) - w);  // the larger funnel phase
            const uint64_t lines = (reach + 127) / 128;  // lines of the window behind a tile's own 32: ceil(reach / 16) vectors
            const bool window_on_page = ((a_n + (uint64_t)w) & 4095) == 0, tiles_on_page = ((a_back + t0) & 4095) == 0;
            uint64_t price = 0;  // in units of 0.5 % of run time
            if (big) {
                price = 3 * lines + (window_on_page ? 0 : 2);
#ifdef CNT_LAB_VARIANTS  // the A/B's other pricings (tuning key "round_trip_plan")
                if (mode == 0) price = tiles_on_page ? 0 : 1000;
                else if (mode == 1) price = window_on_page ? 0 : 1000;
                else if (mode == 2) price = 0;
#else
                (void)mode;
                (void)tiles_on_page;
#endif
            }
            const uint64_t cost = (price << 32) + (reach << 16) + t0;  // then the shorter read-ahead, then the shorter head
            if (cost < best) {
                best = cost;
                r.t0 = t0;
                r.p0 = cand;
                r.w0 = w;
            }
        }
    }
    if (best == ~0ull) return r;  // no window starts inside the buffer: no tiles
    r.phase = (uint32_t)((int64_t)r.t0 - r.w0);
    r.phase2 = (uint32_t)((int64_t)(16 * r.p0) - r.w0);
    const uint64_t read_behind = 16 * (uint64_t)((std::max(r.phase, r.phase2) + 15) >> 4);  // bytes of the window behind a tile's 4 KiB
    const uint64_t avail = (uint64_t)r.w0 < limit ? limit - (uint64_t)r.w0 : 0;  // inputs that end in front of the first window: no tiles
    r.tiles = avail > read_behind ? (avail - read_behind) / kRoundTripAnyTile : 0;
    return r;
}

// Fused encode + decode (BASELINE.json configs[3]): d_bits = n_to_bits(d_n), d_back = bits_to_n(d_bits, n_len), with the
// ASCII read once and the packed words never read back -- ONE launch at any size and any alignment of the three pointers
// (the reference's loads are unaligned loads, n_to_bits.rs:96: nothing about alignment is the caller's business).  All
// three on 128-B lines: round_trip_stream, no LDS.  Anything else: round_trip_window -- tiles laid on the decoded stream's
// lines, the input phase and the packed stream's phase resolved on the packed codes through the wave's LDS slab; the head
// in front of the first tile, the end behind the last and the border dwords ride in the same launch.  Shorter than a tile:
// the edge body alone.
int round_trip_impl(const void* d_n, size_t n_len, void* d_bits, size_t out_words, void* d_back, unsigned flags, hipStream_t s, BadCounter bad) {
    const size_t words = cnt_words_for(n_len);
    if (out_words < words) return CNT_ECAP;
    if (flags & ~kEncodeFlags) return CNT_EINVAL;
    if (n_len == 0) return CNT_OK;
    if (!d_n || !d_bits || !d_back || !aligned(d_bits, 8)) return CNT_EINVAL;
    if (overlaps(d_n, n_len, d_bits, words * 8) || overlaps(d_n, n_len, d_back, n_len) || overlaps(d_bits, words * 8, d_back, n_len)) return CNT_EINVAL;
    const bool strict = (flags & CNT_STRICT_LUT) != 0;
    const uint64_t lut_from = lut_from_of(n_len, flags, 32);
    const uint8_t* n = static_cast<const uint8_t*>(d_n);
    uint8_t* back = static_cast<uint8_t*>(d_back);
    const uint32_t cap = tune_round_trip_cap();
    if (aligned(d_n, 128) && aligned(d_bits, 128) && aligned(d_back, 128) && n_len >= kRoundTripTile) {
        const uint64_t tiles = n_len / kRoundTripTile;  // the ragged end (< one tile) rides in the same launch
        const int shape = tune_round_trip_shape();
        const RoundTripEdges e{n, static_cast<uint64_t*>(d_bits), back, (uint64_t)n_len, 0, (uint64_t)words, lut_from, 0};
        if (strict) launch_round_trip<true>(n, static_cast<uint8_t*>(d_bits), back, tiles, cap, shape, e, s, bad);
        else launch_round_trip<false>(n, static_cast<uint8_t*>(d_bits), back, tiles, cap, shape, e, s, bad);
        return hip_rc(hipGetLastError());
    }
    // under CNT_TAIL_LUT the final partial word is BYTE_LUT's and the tiles know one table: their window stops in front of it
    const uint64_t limit = lut_from != kNoLutWord && !strict ? (uint64_t)n_len & ~(uint64_t)31 : (uint64_t)n_len;
    const RoundTripPlan pl = round_trip_plan(reinterpret_cast<uintptr_t>(n), reinterpret_cast<uintptr_t>(d_bits), reinterpret_cast<uintptr_t>(d_back), n_len, limit, tune_round_trip_plan());
    const uint64_t t0 = pl.t0, p0 = pl.p0, tiles = pl.tiles;
    const int64_t w0 = pl.w0;
    const uint32_t phase = pl.phase, phase2 = pl.phase2;
    RoundTripEdgesAny e{n, static_cast<uint32_t*>(d_bits), back, (uint64_t)n_len, 0, 0, 0, 0, 2 * (uint64_t)words, lut_from, 0};
    if (tiles) {
        e.t0 = t0;
        e.t1 = t0 + tiles * kRoundTripAnyTile;
        e.p0 = p0;
        e.p1 = p0 + tiles * (kRoundTripAnyTile / 16);
        uint8_t* pk = static_cast<uint8_t*>(d_bits) + 4 * p0;
        if (strict) launch_round_trip_any<true>(n + w0, phase, phase2, pk, back + t0, tiles, cap, e, s, tune_round_trip_window_map(), bad);
        else launch_round_trip_any<false>(n + w0, phase, phase2, pk, back + t0, tiles, cap, e, s, tune_round_trip_window_map(), bad);
    } else {
        const unsigned g = generic_grid(e.dwords);
        if (bad && strict) hipLaunchKernelGGL((round_trip_generic_checked<true>), dim3(g), dim3(kBlock), 0, s, e, bad.p, bad.mask);
        else if (bad) hipLaunchKernelGGL((round_trip_generic_checked<false>), dim3(g), dim3(kBlock), 0, s, e, bad.p, bad.mask);
        else if (strict) hipLaunchKernelGGL((round_trip_generic<true>), dim3(g), dim3(kBlock), 0, s, e);
        else hipLaunchKernelGGL((round_trip_generic<false>), dim3(g), dim3(kBlock), 0, s, e);
    }
    return hip_rc(hipGetLastError());
}
int round_trip_dev(const void* d_n, size_t n_len, void* d_bits, size_t out_words, void* d_back, unsigned flags, hipStream_t s) {
    return round_trip_impl(d_n, n_len, d_bits, out_words, d_back, flags, s, BadCounter());
}
int round_trip_checked_dev(const void* d_n, size_t n_len, void* d_bits, size_t out_words, void* d_back, unsigned flags, void* d_invalid, hipStream_t s) {
    BadCounter bad;
    if (!checked_counter(d_invalid, &flags, &bad)) return CNT_EINVAL;
    return round_trip_impl(d_n, n_len, d_bits, out_words, d_back, flags, s, bad);
}

// 5-letter codec, same alignment plan.  Encode: <= 15 head words put the stores on 128-B lines, the
// input phase goes to n_to_bits2_window.  Decode: the stores are the wide side and 27 is a unit
// mod 128, so a head of k = 19 * (-address mod 128) mod 128 words (27 * 19 = 1 mod 128) puts the
// remaining output on a 128-B line for ANY pointer; the packed side just moves by k words.
int encode2_impl(const void* d_n, size_t n_len, void* d_out, size_t out_words, unsigned flags, uint64_t lut_from, hipStream_t s, BadCounter bad) {
    const size_t words = cnt_words2_for(n_len);
    if (out_words < words) return CNT_ECAP;
    if (flags & ~kEncodeFlags) return CNT_EINVAL;
    if (n_len == 0) return CNT_OK;
    if (!d_n || !d_out || !aligned(d_out, 8) || overlaps(d_n, n_len, d_out, words * 8)) return CNT_EINVAL;
    const bool strict = (flags & CNT_STRICT_LUT) != 0;
    const uint8_t* n = static_cast<const uint8_t*>(d_n);
    uint64_t* out = static_cast<uint64_t*>(d_out);
    auto generic = [&](uint64_t nt_end, uint64_t first_word, uint64_t end_word) {
        if (first_word >= end_word) return;
        const unsigned g = generic_grid(end_word - first_word);
        if (bad && strict)
            hipLaunchKernelGGL((n_to_bits2_generic_checked<true>), dim3(g), dim3(kBlock), 0, s, n, nt_end, out, first_word, end_word, lut_from, bad.p, bad.mask);
        else if (bad)
            hipLaunchKernelGGL((n_to_bits2_generic_checked<false>), dim3(g), dim3(kBlock), 0, s, n, nt_end, out, first_word, end_word, lut_from, bad.p, bad.mask);
        else if (strict)
            hipLaunchKernelGGL((n_to_bits2_generic<true>), dim3(g), dim3(kBlock), 0, s, n, nt_end, out, first_word, end_word, lut_from);
        else
            hipLaunchKernelGGL((n_to_bits2_generic<false>), dim3(g), dim3(kBlock), 0, s, n, nt_end, out, first_word, end_word, lut_from);
    };
    if (n_len <= tune_small_nt() && (n_len % kWindowEncode2Tile) != 0) {
        generic(n_len, 0, words);
        HIP_TRY(hipGetLastError());
        return CNT_OK;
    }
    uint64_t head_words = ((128 - (reinterpret_cast<uintptr_t>(d_out) & 127)) & 127) >> 3;  // the 1-KiB tiles' stores on 128-B lines
    const uint32_t phase = (uint32_t)((reinterpret_cast<uintptr_t>(n) + 27 * head_words) & 127);
    if (phase && head_words < 5) head_words += 16;  // 128 B of output; >= 127 B of input in front of the first window
    const uint32_t phase2 = (uint32_t)((reinterpret_cast<uintptr_t>(n) + 27 * head_words) & 127);
    uint64_t main_words = 0;
    bool edges_done = false;
    // the wave tiles know one table per launch: under CNT_TAIL_LUT they stop in front of the first BYTE_LUT word
    const uint64_t tile_end_nt = (!strict && lut_from < words) ? 27 * lut_from : (uint64_t)n_len;
    if (tile_end_nt > 27 * head_words) {
        const uint64_t rem = tile_end_nt - 27 * head_words;
        const uint8_t* p = n + 27 * head_words;
        uint8_t* o = reinterpret_cast<uint8_t*>(out + head_words);
        const Encode2Edges e{n, out, (uint64_t)n_len, head_words, 0, (uint64_t)words, lut_from, 0};  // head + ragged end: same launch
        const int v = bad ? 0 : tune_encode2();
        if (phase2 == 0 || ((phase2 & 15) == 0 && v != 0)) {
            if (strict ? launch_encode2<true>(v, p, o, rem, e, s, &main_words, &edges_done, bad) : launch_encode2<false>(v, p, o, rem, e, s, &main_words, &edges_done, bad))
                return CNT_EINVAL;
        } else if (n_len - 27 * head_words >= kWindowEncode2Tile + kWindowEncode2Slack && rem >= kWindowEncode2Tile) {
            // the slack is about bytes that exist behind a tile, not about words the tiles may cover
            const uint64_t tiles = std::min<uint64_t>((n_len - 27 * head_words - kWindowEncode2Slack) / kWindowEncode2Tile, rem / kWindowEncode2Tile);
            if (tiles) {
                if (strict) launch_encode2_window<true>(p - phase2, phase2, o, tiles, e, s, bad);
                else launch_encode2_window<false>(p - phase2, phase2, o, tiles, e, s, bad);
                edges_done = true;
            }
            main_words = tiles * (kWindowEncode2Tile / 27);
        }
        HIP_TRY(hipGetLastError());
    }
    if (main_words == 0) {
        generic(n_len, 0, words);
    } else if (!edges_done) {  // the multi-wave variants (A/B only)
        generic(27 * head_words, 0, head_words);
        generic(n_len, head_words + main_words, words);
    }
    HIP_TRY(hipGetLastError());
    return CNT_OK;
}
int encode2_dev(const void* d_n, size_t n_len, void* d_out, size_t out_words, unsigned flags, hipStream_t s) {
    return encode2_impl(d_n, n_len, d_out, out_words, flags, lut_from_of(n_len, flags, 27), s, BadCounter());
}
int encode2_checked_dev(const void* d_n, size_t n_len, void* d_out, size_t out_words, unsigned flags, void* d_invalid, hipStream_t s) {
    BadCounter bad;
    if (!checked_counter(d_invalid, &flags, &bad)) return CNT_EINVAL;
    return encode2_impl(d_n, n_len, d_out, out_words, flags, lut_from_of(n_len, flags, 27), s, bad);
}

int decode2_dev(const void* d_bits, size_t words, size_t len, void* d_out, unsigned flags, hipStream_t s) {
    if (words > SIZE_MAX / 27 || len > words * 27) return CNT_ELEN;
    if (flags) return CNT_EINVAL;
    if (len == 0) return CNT_OK;
    if (!d_bits || !d_out || !aligned(d_bits, 8) || overlaps(d_bits, cnt_words2_for(len) * 8, d_out, len)) return CNT_EINVAL;
    const size_t used_words = cnt_words2_for(len);
    const uint64_t* bits = static_cast<const uint64_t*>(d_bits);
    uint8_t* out = static_cast<uint8_t*>(d_out);
    auto generic = [&](uint64_t nt_end, uint64_t first_word, uint64_t end_word) {
        if (first_word >= end_word) return;
        hipLaunchKernelGGL(bits_to_n2_generic, dim3(generic_grid(end_word - first_word)), dim3(kBlock), 0, s, bits, nt_end, out,
                           first_word, end_word);
    };
    if (len <= tune_small_nt() && (len % kWindowEncode2Tile) != 0) {
        generic(len, 0, used_words);
        HIP_TRY(hipGetLastError());
        return CNT_OK;
    }
#ifdef CNT_LAB_VARIANTS
    const int v = tune_decode2();
    if (v >= 0 && v < kNumDecode2Variants && kDecode2Variants[v].pages) {
        const int rc = launch_decode2_page(v, bits, used_words, out, len, s);
        if (rc > 0) return CNT_EINVAL;
        if (rc < 0) generic(len, 0, used_words);
        HIP_TRY(hipGetLastError());
        return CNT_OK;
    }
#endif
    const uint64_t head_words = (19 * ((128 - (reinterpret_cast<uintptr_t>(d_out) & 127)) & 127)) & 127;
    uint64_t main_words = 0;
    bool edges_done = false;
    if (len > 27 * head_words) {
        const Decode2Edges e{bits, out, (uint64_t)len, head_words, 0, (uint64_t)used_words, 0};  // head + ragged end: same launch
        if (launch_decode2(tune_decode2(), bits + head_words, out + 27 * head_words,
                           len - 27 * head_words, e, s, &main_words, &edges_done))
            return CNT_EINVAL;
        HIP_TRY(hipGetLastError());
    }
    if (main_words == 0) {
        generic(len, 0, used_words);
    } else if (!edges_done) {  // the multi-wave variants (A/B only)
        generic(27 * head_words, 0, head_words);
        generic(len, head_words + main_words, used_words);
    }
    HIP_TRY(hipGetLastError());
    return CNT_OK;
}
