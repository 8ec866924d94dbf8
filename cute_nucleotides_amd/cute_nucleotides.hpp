// cute_nucleotides.hpp -- C++ host-side mirror of the reference crate's public API over the
// C ABI (include/cute_nt.h).  Header-only; link with -lcute_nt_hip.
//
// The reference exposes (src/lib.rs:1-2)
//     cute_nucleotides::n_to_bits::{n_to_bits_*, bits_to_n_*}      src/n_to_bits.rs
//     cute_nucleotides::n_to_bits2::{n_to_bits2_*, bits_to_n2_*}   src/n_to_bits2.rs
// as `fn(&[u8]) -> Vec<u64>` / `fn(&[u64], usize) -> Vec<u8>`.  The same names with the
// `_hip` suffix live here in the same module layout, take spans (pointer + length) and return
// owned vectors, exactly like the Rust functions: callee allocates, caller only lends.
//
// Error behaviour: `len` larger than the packed capacity throws std::length_error with the
// reference's panic text (n_to_bits.rs:52-54); any other failure (HIP error, no device)
// throws std::runtime_error carrying cnt_strerror().  Like the reference's functions these
// are re-entrant and callable from any thread.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../include/cute_nt.h"

namespace cute_nucleotides {

namespace detail {
// The reference's functions allocate their result UNINITIALISED and set its length afterwards (Vec::with_capacity /
// alloc + set_len / from_raw_parts, n_to_bits.rs:88-89,113): the output is written exactly once, by the codec.
// std::vector<T>(n) would first zero-fill it -- single-threaded, page by page: a 1-GiB decode through this mirror cost
// 262 ms against 85 ms for the C call into a fresh malloc (profiles/r03_bench_twin.log).  This allocator makes
// `Vec<T>(n)` default-initialise (= leave alone) trivially constructible elements; everything else is std::allocator.
template <class T>
struct uninit_allocator : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = uninit_allocator<U>;
    };
    uninit_allocator() = default;
    template <class U>
    uninit_allocator(const uninit_allocator<U>&) noexcept {}
    template <class U>
    void construct(U* p) noexcept(noexcept(::new (static_cast<void*>(p)) U)) {
        ::new (static_cast<void*>(p)) U;  // default-initialisation: no zero fill for u8 / u64
    }
    template <class U, class... A>
    void construct(U* p, A&&... a) {
        ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
    }
};
// Vec<T> against a plain std::vector<T> (found by ADL through the allocator's namespace)
template <class T, class B, std::enable_if_t<!std::is_same<B, uninit_allocator<T>>::value, int> = 0>
inline bool operator==(const std::vector<T, uninit_allocator<T>>& a, const std::vector<T, B>& b) {
    return a.size() == b.size() && std::equal(a.begin(), a.end(), b.begin());
}
template <class T, class B, std::enable_if_t<!std::is_same<B, uninit_allocator<T>>::value, int> = 0>
inline bool operator!=(const std::vector<T, uninit_allocator<T>>& a, const std::vector<T, B>& b) { return !(a == b); }
template <class T>
inline bool operator==(const std::vector<T>& a, const std::vector<T, uninit_allocator<T>>& b) { return b == a; }
template <class T>
inline bool operator!=(const std::vector<T>& a, const std::vector<T, uninit_allocator<T>>& b) { return !(b == a); }
inline void check(int status) {
    if (status == CNT_OK) return;
    if (status == CNT_ELEN) throw std::length_error(cnt_strerror(status));  // the reference's panic
    throw std::runtime_error(std::string("libcute_nt_hip: ") + cnt_strerror(status));
}
}  // namespace detail

/// What the `*_hip` functions return: a std::vector whose elements are NOT zero-filled on construction (the
/// reference's `Vec` with `set_len`).  Converts to a plain std::vector with `std::vector<T>(v.begin(), v.end())`.
template <class T>
using Vec = std::vector<T, detail::uninit_allocator<T>>;

namespace n_to_bits {

/// Encode {A,T/U,C,G} -> {00,10,01,11}, 32 nt per u64, LSB first (n_to_bits.rs:34-47 and the
/// four SIMD siblings).  `strict_lut` selects n_to_bits_lut's table semantics for bytes outside
/// the alphabet (they encode as 0) instead of the SIMD variants' (byte>>1)&3; `tail_lut` is the SIMD variants to
/// the letter: bit extraction on whole 32-nt blocks, the table on the final partial word (n_to_bits.rs:109-111).
inline Vec<uint64_t> n_to_bits_hip(const uint8_t* n, size_t len, bool strict_lut = false, bool tail_lut = false) {
    Vec<uint64_t> out(cnt_words_for(len));
    detail::check(cnt_n_to_bits_ex(n, len, out.data(), out.size(), (strict_lut ? CNT_STRICT_LUT : 0u) | (tail_lut ? CNT_TAIL_LUT : 0u)));
    return out;
}
template <class A>
inline Vec<uint64_t> n_to_bits_hip(const std::vector<uint8_t, A>& n) { return n_to_bits_hip(n.data(), n.size()); }

/// The same encode VALIDATED in the same pass over the data: `invalid` receives the number of bytes outside ACGTUacgtu -- what
/// the reference's BYTE_LUT turns into code 0 without a word (n_to_bits.rs:8-21,42; README.md:23 points at a separate check).
/// The words are n_to_bits_hip's whatever the count says.
inline Vec<uint64_t> n_to_bits_hip_checked(const uint8_t* n, size_t len, uint64_t& invalid, bool strict_lut = false, bool tail_lut = false) {
    Vec<uint64_t> out(cnt_words_for(len));
    detail::check(cnt_n_to_bits_checked(n, len, out.data(), out.size(), (strict_lut ? CNT_STRICT_LUT : 0u) | (tail_lut ? CNT_TAIL_LUT : 0u), &invalid));
    return out;
}

/// Decode `len` nucleotides (n_to_bits.rs:51-69 and the three SIMD siblings).
inline Vec<uint8_t> bits_to_n_hip(const uint64_t* bits, size_t words, size_t len) {
    if (len > (words << 5)) detail::check(CNT_ELEN);
    Vec<uint8_t> out(len);
    detail::check(cnt_bits_to_n(bits, words, len, out.data()));
    return out;
}
template <class A>
inline Vec<uint8_t> bits_to_n_hip(const std::vector<uint64_t, A>& bits, size_t len) {
    return bits_to_n_hip(bits.data(), bits.size(), len);
}

/// `_into` forms: the same codecs writing into a vector the CALLER owns (resized without zero-fill, capacity reused).  A
/// loop that times like the reference's harness -- result allocated AND dropped inside the timed call,
/// benches/bench_n_to_bits.rs:6-7 -- then pays neither the page faults of a fresh allocation nor the munmap of the
/// dropped one (1-GiB decode: 22 ms instead of 74 ms, BENCH_r03 host_tier).  Same results and exceptions.
inline void n_to_bits_hip_into(const uint8_t* n, size_t len, Vec<uint64_t>& out, bool strict_lut = false, bool tail_lut = false) {
    out.resize(cnt_words_for(len));
    detail::check(cnt_n_to_bits_ex(n, len, out.data(), out.size(), (strict_lut ? CNT_STRICT_LUT : 0u) | (tail_lut ? CNT_TAIL_LUT : 0u)));
}
inline void bits_to_n_hip_into(const uint64_t* bits, size_t words, size_t len, Vec<uint8_t>& out) {
    if (len > (words << 5)) detail::check(CNT_ELEN);
    out.resize(len);
    detail::check(cnt_bits_to_n(bits, words, len, out.data()));
}

/// Span forms: the 2-bit codec between buffers the CALLER owns -- the forms that can use PINNED memory (`PinnedBuffer`,
/// `HostPin`): a side that lies in pinned memory is not staged, the copy engines read / write it in place (include/cute_nt.h
/// "pinned caller memory").  `out` holds at least cnt_words_for(len) words / `len` bytes; returns the count written.
inline size_t n_to_bits_hip_into(const uint8_t* n, size_t len, uint64_t* out, size_t out_words, bool strict_lut = false, bool tail_lut = false) {
    detail::check(cnt_n_to_bits_ex(n, len, out, out_words, (strict_lut ? CNT_STRICT_LUT : 0u) | (tail_lut ? CNT_TAIL_LUT : 0u)));
    return cnt_words_for(len);
}
inline size_t bits_to_n_hip_into(const uint64_t* bits, size_t words, size_t len, uint8_t* out) {
    if (len > (words << 5)) detail::check(CNT_ELEN);
    detail::check(cnt_bits_to_n(bits, words, len, out));
    return len;
}

/// `count` elements of pinned, device-mapped host memory (cnt_host_alloc; NOT zeroed).  For buffers that live as long as the
/// pipeline: pinned memory cannot be swapped.
template <class T>
class PinnedBuffer {
   public:
    explicit PinnedBuffer(size_t count) : count_(count) {
        void* p = nullptr;
        detail::check(cnt_host_alloc(&p, count * sizeof(T)));
        ptr_ = static_cast<T*>(p);
    }
    ~PinnedBuffer() { (void)cnt_host_free(ptr_); }
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    PinnedBuffer(PinnedBuffer&& o) noexcept : ptr_(o.ptr_), count_(o.count_) { o.ptr_ = nullptr, o.count_ = 0; }
    T* data() { return ptr_; }
    const T* data() const { return ptr_; }
    size_t size() const { return count_; }
    T& operator[](size_t i) { return ptr_[i]; }
    const T& operator[](size_t i) const { return ptr_[i]; }
    T* begin() { return ptr_; }
    T* end() { return ptr_ + count_; }

   private:
    T* ptr_ = nullptr;
    size_t count_ = 0;
};

/// Pins an EXISTING range in place for the guard's lifetime (cnt_host_register: tens of milliseconds per GiB, once).
class HostPin {
   public:
    HostPin(void* p, size_t bytes) : p_(p) { detail::check(cnt_host_register(p, bytes)); }
    ~HostPin() { (void)cnt_host_unregister(p_); }
    HostPin(const HostPin&) = delete;
    HostPin& operator=(const HostPin&) = delete;

   private:
    void* p_;
};

/// would the host tier use [p, p + bytes) in place?
inline bool is_pinned(const void* p, size_t bytes) { return cnt_host_is_pinned(p, bytes) == 1; }

/// The same, cut into contiguous chunks over `ndev` GPUs (<= 0: all visible), no collective.
inline Vec<uint64_t> n_to_bits_hip_sharded(const uint8_t* n, size_t len, int ndev = 0) {
    Vec<uint64_t> out(cnt_words_for(len));
    detail::check(cnt_n_to_bits_sharded(n, len, out.data(), out.size(), ndev));
    return out;
}
inline Vec<uint8_t> bits_to_n_hip_sharded(const uint64_t* bits, size_t words, size_t len, int ndev = 0) {
    if (len > (words << 5)) detail::check(CNT_ELEN);
    Vec<uint8_t> out(len);
    detail::check(cnt_bits_to_n_sharded(bits, words, len, out.data(), ndev));
    return out;
}

}  // namespace n_to_bits

namespace n_to_bits2 {

/// 5-letter codec, 3 nt -> 7 bits, 27 nt per u64 (n_to_bits2.rs:37-74, :118-189).
inline Vec<uint64_t> n_to_bits2_hip(const uint8_t* n, size_t len) {
    Vec<uint64_t> out(cnt_words2_for(len));
    detail::check(cnt_n_to_bits2(n, len, out.data(), out.size()));
    return out;
}
template <class A>
inline Vec<uint64_t> n_to_bits2_hip(const std::vector<uint8_t, A>& n) { return n_to_bits2_hip(n.data(), n.size()); }

/// ... validated in the same pass: `invalid` = bytes outside ACGTUNacgtun (n_to_bits2.rs:8-23)
inline Vec<uint64_t> n_to_bits2_hip_checked(const uint8_t* n, size_t len, uint64_t& invalid) {
    Vec<uint64_t> out(cnt_words2_for(len));
    detail::check(cnt_n_to_bits2_checked(n, len, out.data(), out.size(), 0u, &invalid));
    return out;
}

/// n_to_bits2.rs:78-107, :196-268.
inline Vec<uint8_t> bits_to_n2_hip(const uint64_t* bits, size_t words, size_t len) {
    if (words > SIZE_MAX / 27 || len > words * 27) detail::check(CNT_ELEN);
    Vec<uint8_t> out(len);
    detail::check(cnt_bits_to_n2(bits, words, len, out.data()));
    return out;
}
template <class A>
inline Vec<uint8_t> bits_to_n2_hip(const std::vector<uint64_t, A>& bits, size_t len) {
    return bits_to_n2_hip(bits.data(), bits.size(), len);
}

inline void n_to_bits2_hip_into(const uint8_t* n, size_t len, Vec<uint64_t>& out) {
    out.resize(cnt_words2_for(len));
    detail::check(cnt_n_to_bits2(n, len, out.data(), out.size()));
}
inline void bits_to_n2_hip_into(const uint64_t* bits, size_t words, size_t len, Vec<uint8_t>& out) {
    if (words > SIZE_MAX / 27 || len > words * 27) detail::check(CNT_ELEN);
    out.resize(len);
    detail::check(cnt_bits_to_n2(bits, words, len, out.data()));
}

/// The 5-letter codec over `ndev` GPUs (shards are whole 128-word tiles), no collective.
inline Vec<uint64_t> n_to_bits2_hip_sharded(const uint8_t* n, size_t len, int ndev = 0) {
    Vec<uint64_t> out(cnt_words2_for(len));
    detail::check(cnt_n_to_bits2_sharded(n, len, out.data(), out.size(), ndev));
    return out;
}
inline Vec<uint8_t> bits_to_n2_hip_sharded(const uint64_t* bits, size_t words, size_t len, int ndev = 0) {
    if (words > SIZE_MAX / 27 || len > words * 27) detail::check(CNT_ELEN);
    Vec<uint8_t> out(len);
    detail::check(cnt_bits_to_n2_sharded(bits, words, len, out.data(), ndev));
    return out;
}

}  // namespace n_to_bits2

/// Operations on the packed words themselves (include/cute_nt.h): what needs no decode to ASCII.
namespace packed {

/// Nucleotides [start, start + sub_len) of the `len` packed in `bits` translated codon by codon (include/cute_nt.h "translation"):
/// sub_len / 3 bytes, one entry of the 64-byte `table` per codon (nullptr: the standard genetic code, stops as '*'); with `revcomp`
/// the translation of the region's reverse complement.  Forward frame f of a whole sequence is (f, len - f), reverse frame f is
/// (0, len - f, true).
inline Vec<uint8_t> translate_hip(const uint64_t* bits, size_t words, size_t len, size_t start, size_t sub_len, bool revcomp = false,
                                  const uint8_t* table = nullptr) {
    if (len > (words << 5)) detail::check(CNT_ELEN);
    if (start > len || sub_len > len - start) throw std::out_of_range("translate_hip: the region does not lie inside the sequence");
    Vec<uint8_t> out(sub_len / 3);
    detail::check(cnt_translate(bits, len, start, sub_len, revcomp ? CNT_TRANSLATE_REVCOMP : 0u, table, out.data(), out.size()));
    return out;
}

/// What packed::orfs_hip returns: entry j is the ORF [pos[j], pos[j] + length[j]) with info[j] = its frame plus CNT_FIND_REVERSE,
/// CNT_ORF_OPEN_END and CNT_ORF_NO_STOP.
struct Orfs {
    Vec<uint64_t> pos, length, info;
};

/// The open reading frames of the `len` nucleotides packed in `bits` (include/cute_nt.h "ORF scan"): the stop-free runs of each
/// frame lane, on the forward strand or with `both_strands` on both, trimmed to their first start codon (starts == 0: reported
/// whole), at least `min_len` nucleotides long, ordered by the upper end of the run, forward before reverse.  `stops` and `starts`
/// are 64-bit sets of codon values.  translate_hip(bits, words, len, pos[j], length[j], reverse) is the protein of entry j.
inline Orfs orfs_hip(const uint64_t* bits, size_t words, size_t len, uint64_t stops = CNT_ORF_STOPS_STANDARD, uint64_t starts = CNT_ORF_STARTS_ATG,
                     size_t min_len = 0, bool both_strands = false) {
    if (len > (words << 5)) detail::check(CNT_ELEN);
    if (stops == 0) throw std::invalid_argument("orfs_hip: stops must hold at least one codon");
    const size_t most = len < 3 ? 0 : (both_strands ? 2 * len : len);
    // random sequence: a stop every ~21 codons of a lane; a longer result is fetched again at its reported size
    size_t cap = most < most / 16 + 1024 ? most : most / 16 + 1024;
    const unsigned flags = both_strands ? CNT_ORF_BOTH_STRANDS : 0u;
    Orfs r;
    uint64_t n = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        r.pos.resize(cap);
        r.length.resize(cap);
        r.info.resize(cap);
        const int rc = cnt_orfs(bits, len, stops, starts, min_len, flags, r.pos.data(), r.length.data(), r.info.data(), cap, &n);
        if (rc == CNT_ECAP && attempt == 0) {
            cap = n;
            continue;
        }
        detail::check(rc);
        break;
    }
    r.pos.resize(n);
    r.length.resize(n);
    r.info.resize(n);
    return r;
}

/// What packed::hpc_hip returns: the n run bases packed like any sequence in `out` (cnt_words_for(n) words), and pos[j] = where run
/// j starts in the input; its length is pos[j + 1] - pos[j], and len - pos[n - 1] for the last.
struct Hpc {
    Vec<uint64_t> out;
    size_t n = 0;
    Vec<uint64_t> pos;
};

/// Homopolymer compression of the `len` nucleotides packed in `bits` (include/cute_nt.h "homopolymer compression"): every run of
/// equal bases collapses to one base.  Every packed:: call takes (out.data(), out.size(), n); minimizers_hip on them and a look-up
/// of its positions in `pos` are the input's homopolymer-compressed minimizers.  `with_pos` = false leaves `pos` empty.
inline Hpc hpc_hip(const uint64_t* bits, size_t words, size_t len, bool with_pos = true) {
    if (len > (words << 5)) detail::check(CNT_ELEN);
    // random sequence: three runs per four bases; a longer result is fetched again at its reported size
    const size_t guess = len / 4 * 3 + len / 64 + 64;
    size_t cap = len < guess ? len : guess;
    Hpc r;
    uint64_t n = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        r.out.resize(cnt_words_for(cap));
        if (with_pos) r.pos.resize(cap);
        const int rc = cnt_hpc(bits, len, 0u, r.out.data(), with_pos ? r.pos.data() : nullptr, cap, &n);
        if (rc == CNT_ECAP && attempt == 0) {
            cap = n;
            continue;
        }
        detail::check(rc);
        break;
    }
    r.n = n;
    r.out.resize(cnt_words_for(n));
    if (with_pos) r.pos.resize(n);
    return r;
}

/// The number of windows packed::window_counts_hip reports: (len - window) / step + 1, or 0 when len < window.
inline size_t window_counts_n(size_t len, unsigned k, size_t window, size_t step) {
    size_t n = 0;
    detail::check(cnt_window_counts_n(len, k, window, step, &n));
    return n;
}

/// Base (k = 1) or dinucleotide (k = 2) counts per window of the `len` nucleotides packed in `bits` (include/cute_nt.h "windowed
/// composition"): window_counts_n records of 4^k counts, record j for the positions [j * step, j * step + window), entry v the k-mers
/// wholly inside it whose value is v (k = 1: A, C, T, G; k = 2: first base + 4 * second base).  step = 0 means `window`.
/// (C + G) / window of a k = 1 record is the window's GC content.
inline Vec<uint32_t> window_counts_hip(const uint64_t* bits, size_t words, size_t len, unsigned k, size_t window, size_t step = 0) {
    if (len > (words << 5)) detail::check(CNT_ELEN);
    if (step == 0) step = window;
    const size_t n = window_counts_n(len, k, window, step);
    Vec<uint32_t> out(n << (2 * k));
    detail::check(cnt_window_counts(bits, len, k, window, step, 0u, out.data(), n));
    return out;
}

/// What packed::fasta_to_bits_hip returns: the n kept nucleotides packed like any sequence in `out`, one entry per header line
/// in `rec_text` (the byte offset of its '>') and `rec_start` (the position in `out` of the record's first base; record r ends
/// where record r + 1 starts, the last one at n), and the number of kept bytes outside the alphabet.
struct Fasta {
    Vec<uint64_t> out;
    size_t n = 0;
    Vec<uint64_t> rec_text, rec_start;
    uint64_t invalid = 0;
};

/// Encode FASTA text (include/cute_nt.h "text formats: FASTA"): header lines, line feeds and carriage returns are dropped, every
/// other byte is encoded as n_to_bits_hip encodes it (`strict_lut`: BYTE_LUT), `allow_n` takes N / n out of the invalid count.
/// The record arrays start at a guess and are sized to the reported number of header lines once if the guess was short.
inline Fasta fasta_to_bits_hip(const uint8_t* text, size_t text_len, bool strict_lut = false, bool allow_n = false) {
    const unsigned flags = (strict_lut ? CNT_STRICT_LUT : 0u) | (allow_n ? CNT_ALLOW_N : 0u);
    size_t rec_cap = text_len < 1024 ? text_len : text_len / 4096 + 1024;
    Fasta r;
    uint64_t counts[3] = {0, 0, 0};
    r.out.resize(cnt_words_for(text_len));
    for (int attempt = 0; attempt < 2; ++attempt) {
        r.rec_text.resize(rec_cap);
        r.rec_start.resize(rec_cap);
        const int rc = cnt_fasta_to_bits(text, text_len, flags, r.out.data(), text_len, rec_cap ? r.rec_text.data() : nullptr,
                                         rec_cap ? r.rec_start.data() : nullptr, rec_cap, counts);
        if (rc == CNT_ECAP && attempt == 0) {
            rec_cap = counts[CNT_FASTA_RECORDS];
            continue;
        }
        detail::check(rc);
        break;
    }
    r.n = counts[CNT_FASTA_N];
    r.invalid = counts[CNT_FASTA_INVALID];
    r.out.resize(cnt_words_for(r.n));
    r.rec_text.resize(counts[CNT_FASTA_RECORDS]);
    r.rec_start.resize(counts[CNT_FASTA_RECORDS]);
    return r;
}

/// What packed::fastq_to_bits_hip returns: the n nucleotides packed like any sequence in `out`, the quality bytes in `qual` (empty
/// without with_qual), one entry per record in `rec_text` (the byte offset of its name line), `rec_start` (the position in `out`
/// of its first base) and `rec_qual` (the position in `qual` of its first quality; record r ends where record r + 1 starts, the
/// last one at n and at n_qual), the number of sequence bytes outside the alphabet, and the number of name lines without '@' plus
/// separator lines without '+'.  A well-formed file has malformed == 0 and rec_qual == rec_start.
struct Fastq {
    Vec<uint64_t> out;
    size_t n = 0;
    Vec<uint8_t> qual;
    size_t n_qual = 0;
    Vec<uint64_t> rec_text, rec_start, rec_qual;
    uint64_t invalid = 0, malformed = 0;
};

/// Encode strict four-line FASTQ text (include/cute_nt.h "text formats: FASTQ"): a byte's role is its line number mod 4, line feeds
/// and carriage returns are dropped, the sequence bytes are encoded as n_to_bits_hip encodes them (`strict_lut`: BYTE_LUT) and the
/// quality bytes are copied as they are; `allow_n` takes N / n out of the invalid count.  The record arrays start at a guess and
/// are sized to the reported number of records once if the guess was short.
inline Fastq fastq_to_bits_hip(const uint8_t* text, size_t text_len, bool strict_lut = false, bool allow_n = false, bool with_qual = true) {
    const unsigned flags = (strict_lut ? CNT_STRICT_LUT : 0u) | (allow_n ? CNT_ALLOW_N : 0u);
    size_t rec_cap = text_len < 1024 ? text_len : text_len / 256 + 1024;
    Fastq r;
    uint64_t counts[5] = {0, 0, 0, 0, 0};
    r.out.resize(cnt_words_for(text_len));
    if (with_qual) r.qual.resize(text_len);
    for (int attempt = 0; attempt < 2; ++attempt) {
        r.rec_text.resize(rec_cap);
        r.rec_start.resize(rec_cap);
        r.rec_qual.resize(rec_cap);
        const int rc = cnt_fastq_to_bits(text, text_len, flags, r.out.data(), text_len, with_qual && text_len ? r.qual.data() : nullptr, text_len,
                                         rec_cap ? r.rec_text.data() : nullptr, rec_cap ? r.rec_start.data() : nullptr, rec_cap ? r.rec_qual.data() : nullptr,
                                         rec_cap, counts);
        if (rc == CNT_ECAP && attempt == 0) {
            rec_cap = counts[CNT_FASTQ_RECORDS];
            continue;
        }
        detail::check(rc);
        break;
    }
    r.n = counts[CNT_FASTQ_N];
    r.n_qual = with_qual ? counts[CNT_FASTQ_QUAL] : 0;
    r.invalid = counts[CNT_FASTQ_INVALID];
    r.malformed = counts[CNT_FASTQ_MALFORMED];
    r.out.resize(cnt_words_for(r.n));
    r.qual.resize(r.n_qual);
    r.rec_text.resize(counts[CNT_FASTQ_RECORDS]);
    r.rec_start.resize(counts[CNT_FASTQ_RECORDS]);
    r.rec_qual.resize(counts[CNT_FASTQ_RECORDS]);
    return r;
}

/// The most bytes of FASTA text packed::bits_to_fasta_hip writes: a pure host function, the footprint of the device tier's text.
inline size_t bits_to_fasta_bound(size_t len, size_t n_rec, size_t names_len, size_t width) {
    size_t bytes = 0;
    detail::check(cnt_bits_to_fasta_bound(len, n_rec, names_len, width, &bytes));
    return bytes;
}

/// What packed::bits_to_fasta_hip returns: the text, and per record the byte offset of its '>'.
struct FastaText {
    Vec<uint8_t> text;
    Vec<uint64_t> rec_text;
};

/// Write packed nucleotides as FASTA text (include/cute_nt.h "text formats: FASTA write"): the bases in front of rec_start[0] as
/// headerless lines, then per record '>', its name, a line feed and its bases [rec_start[r], rec_start[r + 1]) -- the last record
/// ends at len -- in lines of `width` letters (0: one line per record).  `names` and `name_off` (n_rec + 1 offsets into names) go
/// together or are both null: every name is empty then.  Names are copied as they are.  A rec_start or name_off that descends is
/// an error and writes nothing.  packed::fasta_to_bits_hip reads the text back to bits, len, rec_start and rec_text.
inline FastaText bits_to_fasta_hip(const uint64_t* bits, size_t len, const uint64_t* rec_start, size_t n_rec, const uint8_t* names, size_t names_len,
                                   const uint64_t* name_off, size_t width = 60) {
    const size_t cap = bits_to_fasta_bound(len, n_rec, names_len, width);
    FastaText r;
    r.text.resize(cap ? cap : 1);
    r.rec_text.resize(n_rec);
    uint64_t counts[2] = {0, 0};
    detail::check(cnt_bits_to_fasta(bits, len, rec_start, n_rec, names, names_len, name_off, width, 0u, r.text.data(), cap, n_rec ? r.rec_text.data() : nullptr,
                                    counts));
    r.text.resize(counts[CNT_FASTA_OUT_TEXT]);
    return r;
}

/// The most bytes of FASTQ text packed::bits_to_fastq_hip writes: a pure host function, the footprint of the device tier's text.
inline size_t bits_to_fastq_bound(size_t len, size_t n_rec, size_t names_len) {
    size_t bytes = 0;
    detail::check(cnt_bits_to_fastq_bound(len, n_rec, names_len, &bytes));
    return bytes;
}

/// Write packed nucleotides and their quality bytes as four-line FASTQ text (include/cute_nt.h "text formats: FASTQ write"): per
/// record '@', its name, a line feed, its bases [rec_start[r], rec_start[r + 1]) -- the first record begins at 0, the last one ends
/// at len -- "\n+\n", the quality bytes of the same positions and a line feed.  `qual` holds len bytes; `names` and `name_off`
/// (n_rec + 1 offsets into names) go together or are both null: every name is empty then.  Names and qualities are copied as they
/// are.  A table that descends or does not begin at 0 is an error and writes nothing.  Returns the text and per record the byte
/// offset of its '@'; packed::fastq_to_bits_hip reads the text back.
inline FastaText bits_to_fastq_hip(const uint64_t* bits, size_t len, const uint8_t* qual, const uint64_t* rec_start, size_t n_rec, const uint8_t* names,
                                   size_t names_len, const uint64_t* name_off) {
    const size_t cap = bits_to_fastq_bound(len, n_rec, names_len);
    FastaText r;
    r.text.resize(cap ? cap : 1);
    r.rec_text.resize(n_rec);
    uint64_t counts[2] = {0, 0};
    detail::check(cnt_bits_to_fastq(bits, len, qual, rec_start, n_rec, names, names_len, name_off, 0u, r.text.data(), cap, n_rec ? r.rec_text.data() : nullptr,
                                    counts));
    r.text.resize(counts[CNT_FASTQ_OUT_TEXT]);
    return r;
}

}  // namespace packed

/// Device-resident tier for C++ callers that do not link HIP themselves (the same shape as the Rust binding's
/// `DeviceBuffer` / `n_to_bits_hip_dev`, rust/src/hip.rs): data already in HBM, enqueue on the default stream,
/// `sync()` waits.  This is the tier the roofline numbers measure.
namespace device {

class DeviceBuffer {
   public:
    explicit DeviceBuffer(size_t bytes) : bytes_(bytes) { detail::check(cnt_dev_alloc(&ptr_, bytes)); }
    DeviceBuffer(const void* host, size_t bytes) : DeviceBuffer(bytes) { detail::check(cnt_dev_upload(ptr_, host, bytes)); }
    ~DeviceBuffer() { (void)cnt_dev_free(ptr_); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    void* data() const { return ptr_; }
    size_t size_bytes() const { return bytes_; }
    template <typename T>
    Vec<T> to_vector(size_t count) const {  // synchronous copy back to the host
        if (count * sizeof(T) > bytes_) throw std::out_of_range("DeviceBuffer::to_vector");
        Vec<T> out(count);
        detail::check(cnt_dev_download(out.data(), ptr_, count * sizeof(T)));
        return out;
    }

   private:
    void* ptr_ = nullptr;
    size_t bytes_ = 0;
};

/// Enqueue the encode of `n_len` resident nucleotides into `out` (>= cnt_words_for(n_len) words).
inline void n_to_bits_hip_dev(const DeviceBuffer& n, size_t n_len, DeviceBuffer& out, bool strict_lut = false) {
    if (n_len > n.size_bytes()) throw std::out_of_range("n_to_bits_hip_dev: n_len");
    detail::check(cnt_n_to_bits_dev(n.data(), n_len, out.data(), out.size_bytes() / 8, strict_lut ? CNT_STRICT_LUT : 0u, nullptr));
}
/// Encode + validity count in ONE pass over the resident ASCII (cnt_n_to_bits_checked_dev): the launch ADDS the number of
/// bytes outside ACGTUacgtu to the u64 at `invalid` (device memory the caller zeroed, e.g. an 8-byte DeviceBuffer).
/// `spread` (CNT_SPREAD_COUNT): `invalid` holds CNT_COUNT_SLOTS u64 (16 KiB) and the count is their sum -- for dirty data.
inline void n_to_bits_hip_checked_dev(const DeviceBuffer& n, size_t n_len, DeviceBuffer& out, DeviceBuffer& invalid, bool strict_lut = false, bool spread = false) {
    if (n_len > n.size_bytes() || invalid.size_bytes() < (spread ? 8u * CNT_COUNT_SLOTS : 8u)) throw std::out_of_range("n_to_bits_hip_checked_dev: sizes");
    detail::check(cnt_n_to_bits_checked_dev(n.data(), n_len, out.data(), out.size_bytes() / 8, (strict_lut ? CNT_STRICT_LUT : 0u) | (spread ? CNT_SPREAD_COUNT : 0u),
                                            invalid.data(), nullptr));
}
/// Enqueue the decode of `len` nucleotides from `words` resident words into `out` (>= len bytes).
inline void bits_to_n_hip_dev(const DeviceBuffer& bits, size_t words, size_t len, DeviceBuffer& out) {
    if (len > (words << 5)) detail::check(CNT_ELEN);
    if (words * 8 > bits.size_bytes() || len > out.size_bytes()) throw std::out_of_range("bits_to_n_hip_dev: sizes");
    detail::check(cnt_bits_to_n_dev(bits.data(), words, len, out.data(), 0u, nullptr));
}
/// Enqueue the translation of nucleotides [start, start + sub_len) of `len` resident ones into `out` (>= sub_len / 3 bytes); see
/// packed::translate_hip.  `table` is HOST memory, read before the call returns.
inline void translate_hip_dev(const DeviceBuffer& bits, size_t len, size_t start, size_t sub_len, DeviceBuffer& out, bool revcomp = false,
                              const uint8_t* table = nullptr) {
    if (len > ((bits.size_bytes() / 8) << 5)) detail::check(CNT_ELEN);
    if (start > len || sub_len > len - start) throw std::out_of_range("translate_hip_dev: the region does not lie inside the sequence");
    detail::check(cnt_translate_dev(bits.data(), len, start, sub_len, revcomp ? CNT_TRANSLATE_REVCOMP : 0u, table, out.data(), out.size_bytes(), nullptr));
}
inline size_t orfs_work_bytes(size_t len) {
    size_t bytes = 0;
    detail::check(cnt_orfs_work_bytes(len, &bytes));
    return bytes;
}
/// Enqueue the ORF scan of `len` resident nucleotides (see packed::orfs_hip): `count` (one u64) is SET to the number of entries n,
/// the first min(n, capacity) go to `pos`, `length` and, when given, `info`; `work` holds >= orfs_work_bytes(len) bytes of any
/// contents.
inline void orfs_hip_dev(const DeviceBuffer& bits, size_t len, uint64_t stops, uint64_t starts, size_t min_len, bool both_strands, DeviceBuffer& pos,
                         DeviceBuffer& length, DeviceBuffer* info, DeviceBuffer& count, DeviceBuffer& work) {
    if (len > ((bits.size_bytes() / 8) << 5)) detail::check(CNT_ELEN);
    if (stops == 0) throw std::invalid_argument("orfs_hip_dev: stops must hold at least one codon");
    size_t cap = (pos.size_bytes() < length.size_bytes() ? pos.size_bytes() : length.size_bytes()) / 8;
    if (info && info->size_bytes() / 8 < cap) cap = info->size_bytes() / 8;
    detail::check(cnt_orfs_dev(bits.data(), len, stops, starts, min_len, both_strands ? CNT_ORF_BOTH_STRANDS : 0u, pos.data(), length.data(),
                               info ? info->data() : nullptr, cap, count.data(), work.data(), work.size_bytes(), nullptr));
}
inline size_t hpc_work_bytes(size_t len) {
    size_t bytes = 0;
    detail::check(cnt_hpc_work_bytes(len, &bytes));
    return bytes;
}
/// Enqueue the homopolymer compression of `len` resident nucleotides (see packed::hpc_hip): `count` (one u64) is SET to the number
/// of runs n, the first min(n, out_cap) run bases go to `out` packed and, when given, their positions to `pos`; `out` holds >=
/// cnt_words_for(min(len, out_cap)) words, `pos` that many entries, `work` >= hpc_work_bytes(len) bytes of any contents.
inline void hpc_hip_dev(const DeviceBuffer& bits, size_t len, DeviceBuffer& out, DeviceBuffer* pos, size_t out_cap, DeviceBuffer& count, DeviceBuffer& work) {
    if (len > ((bits.size_bytes() / 8) << 5)) detail::check(CNT_ELEN);
    const size_t most = len < out_cap ? len : out_cap;
    if (out.size_bytes() / 8 < cnt_words_for(most) || (pos && pos->size_bytes() / 8 < most)) throw std::out_of_range("hpc_hip_dev: an output is smaller than its footprint");
    detail::check(cnt_hpc_dev(bits.data(), len, 0u, out.data(), pos ? pos->data() : nullptr, out_cap, count.data(), work.data(), work.size_bytes(), nullptr));
}
inline size_t fasta_to_bits_work_bytes(size_t text_len) {
    size_t bytes = 0;
    detail::check(cnt_fasta_to_bits_work_bytes(text_len, &bytes));
    return bytes;
}
/// Enqueue the FASTA encode of `text_len` resident bytes (see packed::fasta_to_bits_hip): `counts` (three u64) is SET to n, the
/// number of header lines and the invalid count; `out` receives the first min(n, out_cap) nucleotides and holds at least
/// cnt_words_for(min(text_len, out_cap)) words; `rec_text` and `rec_start` (both or neither) hold at least min(text_len, rec_cap)
/// entries; `work` >= fasta_to_bits_work_bytes(text_len) bytes of any contents.
inline void fasta_to_bits_hip_dev(const DeviceBuffer& text, size_t text_len, DeviceBuffer& out, size_t out_cap, DeviceBuffer* rec_text, DeviceBuffer* rec_start,
                                  size_t rec_cap, DeviceBuffer& counts, DeviceBuffer& work, bool strict_lut = false, bool allow_n = false) {
    if (text_len > text.size_bytes() || counts.size_bytes() < 24) throw std::out_of_range("fasta_to_bits_hip_dev: sizes");
    const size_t most = text_len < out_cap ? text_len : out_cap, rmost = text_len < rec_cap ? text_len : rec_cap;
    if (out.size_bytes() / 8 < cnt_words_for(most) || (rec_text && rec_text->size_bytes() / 8 < rmost) || (rec_start && rec_start->size_bytes() / 8 < rmost))
        throw std::out_of_range("fasta_to_bits_hip_dev: an output is smaller than its footprint");
    detail::check(cnt_fasta_to_bits_dev(text.data(), text_len, (strict_lut ? CNT_STRICT_LUT : 0u) | (allow_n ? CNT_ALLOW_N : 0u), out.data(), out_cap,
                                        rec_text ? rec_text->data() : nullptr, rec_start ? rec_start->data() : nullptr, rec_cap, counts.data(), work.data(),
                                        work.size_bytes(), nullptr));
}
inline size_t bits_to_fasta_work_bytes(size_t n_rec) {
    size_t bytes = 0;
    detail::check(cnt_bits_to_fasta_work_bytes(n_rec, &bytes));
    return bytes;
}
/// Enqueue the FASTA write of `len` resident nucleotides (see packed::bits_to_fasta_hip): `counts` (two u64) is SET to the bytes of
/// text and the malformed count; `rec_start` (null without a record) holds n_rec entries, `names` and `name_off` (both or neither)
/// names_len bytes and n_rec + 1 entries, `text` at least min(packed::bits_to_fasta_bound(...), text_cap) bytes, `rec_text`
/// (optional) n_rec entries, `work` >= bits_to_fasta_work_bytes(n_rec) bytes of any contents.
inline void bits_to_fasta_hip_dev(const DeviceBuffer& bits, size_t len, const DeviceBuffer* rec_start, size_t n_rec, const DeviceBuffer* names, size_t names_len,
                                  const DeviceBuffer* name_off, size_t width, DeviceBuffer& text, size_t text_cap, DeviceBuffer* rec_text, DeviceBuffer& counts,
                                  DeviceBuffer& work) {
    if (len > ((bits.size_bytes() / 8) << 5)) detail::check(CNT_ELEN);
    if (counts.size_bytes() < 16 || (rec_start && rec_start->size_bytes() / 8 < n_rec) || (names && names->size_bytes() < names_len) ||
        (name_off && name_off->size_bytes() / 8 < n_rec + 1))
        throw std::out_of_range("bits_to_fasta_hip_dev: sizes");
    const size_t bound = packed::bits_to_fasta_bound(len, n_rec, names_len, width), foot = bound < text_cap ? bound : text_cap;
    if (text.size_bytes() < foot || (rec_text && rec_text->size_bytes() / 8 < n_rec)) throw std::out_of_range("bits_to_fasta_hip_dev: an output is smaller than its footprint");
    detail::check(cnt_bits_to_fasta_dev(bits.data(), len, rec_start ? rec_start->data() : nullptr, n_rec, names ? names->data() : nullptr, names_len,
                                        name_off ? name_off->data() : nullptr, width, 0u, text.data(), text_cap, rec_text ? rec_text->data() : nullptr, counts.data(),
                                        work.data(), work.size_bytes(), nullptr));
}
inline size_t bits_to_fastq_work_bytes(size_t n_rec) {
    size_t bytes = 0;
    detail::check(cnt_bits_to_fastq_work_bytes(n_rec, &bytes));
    return bytes;
}
/// Enqueue the FASTQ write of `len` resident nucleotides (see packed::bits_to_fastq_hip): `counts` (two u64) is SET to the bytes of
/// text and the malformed count; `qual` holds len bytes, `rec_start` n_rec entries, `names` and `name_off` (both or neither)
/// names_len bytes and n_rec + 1 entries, `text` at least min(packed::bits_to_fastq_bound(...), text_cap) bytes, `rec_text`
/// (optional) n_rec entries, `work` >= bits_to_fastq_work_bytes(n_rec) bytes of any contents.
inline void bits_to_fastq_hip_dev(const DeviceBuffer& bits, size_t len, const DeviceBuffer& qual, const DeviceBuffer& rec_start, size_t n_rec,
                                  const DeviceBuffer* names, size_t names_len, const DeviceBuffer* name_off, DeviceBuffer& text, size_t text_cap,
                                  DeviceBuffer* rec_text, DeviceBuffer& counts, DeviceBuffer& work) {
    if (len > ((bits.size_bytes() / 8) << 5)) detail::check(CNT_ELEN);
    if (counts.size_bytes() < 16 || qual.size_bytes() < len || rec_start.size_bytes() / 8 < n_rec || (names && names->size_bytes() < names_len) ||
        (name_off && name_off->size_bytes() / 8 < n_rec + 1))
        throw std::out_of_range("bits_to_fastq_hip_dev: sizes");
    const size_t bound = packed::bits_to_fastq_bound(len, n_rec, names_len), foot = bound < text_cap ? bound : text_cap;
    if (text.size_bytes() < foot || (rec_text && rec_text->size_bytes() / 8 < n_rec)) throw std::out_of_range("bits_to_fastq_hip_dev: an output is smaller than its footprint");
    detail::check(cnt_bits_to_fastq_dev(bits.data(), len, qual.data(), rec_start.data(), n_rec, names ? names->data() : nullptr, names_len,
                                        name_off ? name_off->data() : nullptr, 0u, text.data(), text_cap, rec_text ? rec_text->data() : nullptr, counts.data(),
                                        work.data(), work.size_bytes(), nullptr));
}
inline size_t fastq_to_bits_work_bytes(size_t text_len) {
    size_t bytes = 0;
    detail::check(cnt_fastq_to_bits_work_bytes(text_len, &bytes));
    return bytes;
}
/// Enqueue the FASTQ encode of `text_len` resident bytes (see packed::fastq_to_bits_hip): `counts` (five u64) is SET to n, the
/// number of records, the invalid count, the number of quality bytes and the malformed count; `out` receives the first
/// min(n, out_cap) nucleotides and holds at least cnt_words_for(min(text_len, out_cap)) words; `qual` (optional) holds at least
/// min(text_len, qual_cap) bytes; `rec_text`, `rec_start` and `rec_qual` (all three or none) hold at least min(text_len, rec_cap)
/// entries; `work` >= fastq_to_bits_work_bytes(text_len) bytes of any contents.
inline void fastq_to_bits_hip_dev(const DeviceBuffer& text, size_t text_len, DeviceBuffer& out, size_t out_cap, DeviceBuffer* qual, size_t qual_cap,
                                  DeviceBuffer* rec_text, DeviceBuffer* rec_start, DeviceBuffer* rec_qual, size_t rec_cap, DeviceBuffer& counts, DeviceBuffer& work,
                                  bool strict_lut = false, bool allow_n = false) {
    if (text_len > text.size_bytes() || counts.size_bytes() < 40) throw std::out_of_range("fastq_to_bits_hip_dev: sizes");
    const size_t most = text_len < out_cap ? text_len : out_cap, qmost = text_len < qual_cap ? text_len : qual_cap, rmost = text_len < rec_cap ? text_len : rec_cap;
    if (out.size_bytes() / 8 < cnt_words_for(most) || (qual && qual->size_bytes() < qmost) || (rec_text && rec_text->size_bytes() / 8 < rmost) ||
        (rec_start && rec_start->size_bytes() / 8 < rmost) || (rec_qual && rec_qual->size_bytes() / 8 < rmost))
        throw std::out_of_range("fastq_to_bits_hip_dev: an output is smaller than its footprint");
    detail::check(cnt_fastq_to_bits_dev(text.data(), text_len, (strict_lut ? CNT_STRICT_LUT : 0u) | (allow_n ? CNT_ALLOW_N : 0u), out.data(), out_cap,
                                        qual ? qual->data() : nullptr, qual_cap, rec_text ? rec_text->data() : nullptr, rec_start ? rec_start->data() : nullptr,
                                        rec_qual ? rec_qual->data() : nullptr, rec_cap, counts.data(), work.data(), work.size_bytes(), nullptr));
}
/// Enqueue the windowed counts of `len` resident nucleotides (see packed::window_counts_hip): the packed::window_counts_n records
/// of 4^k u32 in `out` are SET, nothing behind them is written.  No scratch.
inline void window_counts_hip_dev(const DeviceBuffer& bits, size_t len, unsigned k, size_t window, size_t step, DeviceBuffer& out) {
    if (len > ((bits.size_bytes() / 8) << 5)) detail::check(CNT_ELEN);
    const size_t n = packed::window_counts_n(len, k, window, step);
    if (out.size_bytes() / 4 < (n << (2 * k))) throw std::out_of_range("window_counts_hip_dev: the output is smaller than its records");
    detail::check(cnt_window_counts_dev(bits.data(), len, k, window, step, 0u, out.data(), n, nullptr));
}
inline void sync() { detail::check(cnt_dev_sync(nullptr)); }
inline void set_device(int device) { detail::check(cnt_set_device(device)); }  // what DeviceBuffer allocates on

/// Enqueue-only multi-GPU device tier (cnt_sharded_dev_open / *_enqueue / cnt_sharded_dev_wait): shard k resident on
/// device k, one library stream per shard; every enqueue_* call queues that codec call on every shard and returns at
/// once, wait() drains all of them.  Queue the decode of step s behind its encode, step s+1 behind that, wait once: the
/// devices run back to back with the host a whole queue ahead (word w depends on nucleotides [32w, 32w+32) only,
/// n_to_bits.rs:38-43 -- nothing needs a barrier).
class ShardedDevQueue {
   public:
    explicit ShardedDevQueue(int ndev, bool timed = false) {
        detail::check(cnt_sharded_dev_open(ndev, timed ? CNT_QUEUE_TIMED : 0u, &handle_));
        detail::check(cnt_sharded_dev_shards(handle_, &ndev_));
    }
    /// the queue ADOPTS the caller's streams (streams[k]: a non-null hipStream_t of device k): shard k's ops run in order with
    /// whatever else the caller enqueues there; close() leaves them alone
    explicit ShardedDevQueue(const std::vector<void*>& streams, bool timed = false) {
        detail::check(cnt_sharded_dev_open_on_streams((int)streams.size(), streams.data(), timed ? CNT_QUEUE_TIMED : 0u, &handle_));
        detail::check(cnt_sharded_dev_shards(handle_, &ndev_));
    }
    /// library-owned streams on an explicit device list: shard k runs on devices[k] (any subset, order or repetition)
    static ShardedDevQueue on_devices(const std::vector<int>& devices, bool timed = false) {
        void* h = nullptr;
        detail::check(cnt_sharded_dev_open_on_devices((int)devices.size(), devices.data(), timed ? CNT_QUEUE_TIMED : 0u, &h));
        return ShardedDevQueue(h);
    }
    ShardedDevQueue(ShardedDevQueue&& o) noexcept : handle_(o.handle_), ndev_(o.ndev_) { o.handle_ = nullptr; }
    ~ShardedDevQueue() {
        if (handle_) (void)cnt_sharded_dev_close(handle_);
    }
    /// the device the queue runs shard k on -- for adopted streams what the STREAM says (hipStreamGetDevice), not k
    int device(int k) const {
        int d = -1;
        detail::check(cnt_sharded_dev_device(handle_, k, &d));
        return d;
    }
    /// the validated encode on every shard: shard k's op adds its count of bytes outside ACGTUacgtu to the u64 in invalid[k]
    /// (8 bytes on shard k's device, zeroed by the caller)
    void enqueue_n_to_bits_checked(const std::vector<const DeviceBuffer*>& n, const std::vector<size_t>& n_len, const std::vector<DeviceBuffer*>& out,
                                   const std::vector<DeviceBuffer*>& invalid, bool strict_lut = false) {
        if ((int)n.size() != ndev_ || (int)n_len.size() != ndev_ || (int)out.size() != ndev_ || (int)invalid.size() != ndev_) throw std::invalid_argument("one entry per shard");
        std::vector<const void*> in(n.size());
        std::vector<void*> o(n.size()), c(n.size());
        std::vector<size_t> cap(n.size());
        for (size_t k = 0; k < n.size(); ++k) {
            if (n_len[k] > n[k]->size_bytes() || invalid[k]->size_bytes() < 8) throw std::out_of_range("enqueue_n_to_bits_checked: sizes");
            in[k] = n[k]->data();
            o[k] = out[k]->data();
            c[k] = invalid[k]->data();
            cap[k] = out[k]->size_bytes() / 8;
        }
        detail::check(cnt_n_to_bits_checked_sharded_dev_enqueue(handle_, in.data(), n_len.data(), o.data(), cap.data(), strict_lut ? CNT_STRICT_LUT : 0u, c.data()));
    }
    /// shard k's stream waits ON THE DEVICE for `event` (a hipEvent_t recorded behind the producer of shard k's buffer)
    void wait_event(int k, void* event) { detail::check(cnt_sharded_dev_wait_event(handle_, k, event)); }
    /// records the caller's hipEvent_t (of shard k's device) behind everything queued for shard k so far
    void record_event(int k, void* event) { detail::check(cnt_sharded_dev_record_event(handle_, k, event)); }
    /// the fused encode + decode of cnt_round_trip_dev on every shard
    void enqueue_round_trip(const std::vector<const DeviceBuffer*>& n, const std::vector<size_t>& n_len, const std::vector<DeviceBuffer*>& bits,
                            const std::vector<DeviceBuffer*>& back, bool strict_lut = false) {
        if ((int)n.size() != ndev_ || (int)n_len.size() != ndev_ || (int)bits.size() != ndev_ || (int)back.size() != ndev_) throw std::invalid_argument("one entry per shard");
        std::vector<const void*> in(n.size());
        std::vector<void*> o(n.size()), b(n.size());
        std::vector<size_t> cap(n.size());
        for (size_t k = 0; k < n.size(); ++k) {
            if (n_len[k] > n[k]->size_bytes() || n_len[k] > back[k]->size_bytes()) throw std::out_of_range("enqueue_round_trip: n_len");
            in[k] = n[k]->data();
            o[k] = bits[k]->data();
            b[k] = back[k]->data();
            cap[k] = bits[k]->size_bytes() / 8;
        }
        detail::check(cnt_round_trip_sharded_dev_enqueue(handle_, in.data(), n_len.data(), o.data(), cap.data(), b.data(), strict_lut ? CNT_STRICT_LUT : 0u));
    }
    ShardedDevQueue(const ShardedDevQueue&) = delete;
    ShardedDevQueue& operator=(const ShardedDevQueue&) = delete;
    int shards() const { return ndev_; }
    void enqueue_n_to_bits(const std::vector<const DeviceBuffer*>& n, const std::vector<size_t>& n_len, const std::vector<DeviceBuffer*>& out, bool strict_lut = false) {
        if ((int)n.size() != ndev_ || (int)n_len.size() != ndev_ || (int)out.size() != ndev_) throw std::invalid_argument("one entry per shard");
        std::vector<const void*> in(n.size());
        std::vector<void*> o(n.size());
        std::vector<size_t> cap(n.size());
        for (size_t k = 0; k < n.size(); ++k) {
            if (n_len[k] > n[k]->size_bytes()) throw std::out_of_range("enqueue_n_to_bits: n_len");
            in[k] = n[k]->data();
            o[k] = out[k]->data();
            cap[k] = out[k]->size_bytes() / 8;
        }
        detail::check(cnt_n_to_bits_sharded_dev_enqueue(handle_, in.data(), n_len.data(), o.data(), cap.data(), strict_lut ? CNT_STRICT_LUT : 0u));
    }
    void enqueue_bits_to_n(const std::vector<const DeviceBuffer*>& bits, const std::vector<size_t>& words, const std::vector<size_t>& len, const std::vector<DeviceBuffer*>& out) {
        if ((int)bits.size() != ndev_ || (int)words.size() != ndev_ || (int)len.size() != ndev_ || (int)out.size() != ndev_) throw std::invalid_argument("one entry per shard");
        std::vector<const void*> in(bits.size());
        std::vector<void*> o(bits.size());
        for (size_t k = 0; k < bits.size(); ++k) {
            if (len[k] > (words[k] << 5)) detail::check(CNT_ELEN);
            if (words[k] * 8 > bits[k]->size_bytes() || len[k] > out[k]->size_bytes()) throw std::out_of_range("enqueue_bits_to_n: sizes");
            in[k] = bits[k]->data();
            o[k] = out[k]->data();
        }
        detail::check(cnt_bits_to_n_sharded_dev_enqueue(handle_, in.data(), words.data(), len.data(), o.data(), 0u));
    }
    /// waits for everything queued; per-shard device milliseconds of the batch (zeros unless timed)
    std::vector<float> wait() {
        std::vector<float> ms((size_t)ndev_, 0.f);
        detail::check(cnt_sharded_dev_wait(handle_, ms.data()));
        return ms;
    }
    std::vector<float> op_ms(size_t op) const {
        std::vector<float> ms((size_t)ndev_, 0.f);
        detail::check(cnt_sharded_dev_op_ms(handle_, op, ms.data()));
        return ms;
    }

   private:
    explicit ShardedDevQueue(void* adopted_handle) : handle_(adopted_handle) { detail::check(cnt_sharded_dev_shards(handle_, &ndev_)); }
    void* handle_ = nullptr;
    int ndev_ = 0;
};

}  // namespace device

}  // namespace cute_nucleotides
