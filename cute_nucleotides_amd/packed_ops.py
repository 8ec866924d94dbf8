"""Operations on 2-bit packed nucleotides without decoding: Hamming distance,
complement, reverse complement, k-mer extraction (forward and canonical), k-mer counting (the 4^k spectrum, k <= 12),
(w,k)-minimizers, approximate pattern search on one or both strands, region extraction (a subsequence at any start, or many
windows of one length at the positions a search reported, forward or reverse-complemented), codon translation in any of the six
frames, the open-reading-frame scan on one or both strands, homopolymer compression with run positions, base and dinucleotide
counts per window (GC content on top of them), alphabet validation of ASCII buffers, and the encode of FASTA text with its
record table and of FASTQ text with its qualities and record table, and the way back: packed words to FASTA text with
header lines and wrapped lines.  The reference does
not implement these (its README.md:20-25,45 only points at them); semantics are defined in
include/cute_nt.h and restated by the oracle.  Host tier: numpy; device tier: torch tensors on
torch's current stream."""
import collections
import ctypes

import numpy as np

from . import _lib
from ._lib import (CNT_EXTRACT_REVCOMP, CNT_FIND_BOTH_STRANDS, CNT_FIND_REVERSE, CNT_KMER_CANONICAL, CNT_ORF_BOTH_STRANDS, CNT_ORF_NO_STOP,
                   CNT_ORF_OPEN_END, CNT_ORF_STARTS_ATG, CNT_ORF_STOPS_STANDARD, CNT_TRANSLATE_REVCOMP, check, lib)
from .n_to_bits import _counter, _dev_guard, _enqueue, _out_bytes, _out_words, _p, _u8, _u64

CNT_ALLOW_N = 0x2


def _packed(bits, length):
    """the host tier's packed input: a contiguous uint64 array holding `length` nucleotides"""
    bits = _u64(bits)
    if length > bits.size * 32:
        raise ValueError("The length is greater than the number of nucleotides!")
    return bits


def _packed_dev(bits, length):
    """the device tier's packed input: a contiguous int64 CUDA tensor holding `length` nucleotides; returns torch"""
    torch = _dev_guard(bits)
    if bits.dtype != torch.int64:
        raise TypeError("packed words must be an int64 tensor")
    if length > bits.numel() * 32:
        raise ValueError("The length is greater than the number of nucleotides!")
    return torch


# ---- host tier --------------------------------------------------------------------------
def hamming_hip(a, b, length):
    a, b = _u64(a), _u64(b)  # both types are checked before either length
    a, b = _packed(a, length), _packed(b, length)
    out = ctypes.c_uint64(0)
    check(lib().cnt_hamming(_p(a), _p(b), length, ctypes.byref(out)))
    return out.value


def complement_hip(bits, length):
    bits = _packed(bits, length)
    out = np.empty(lib().cnt_words_for(length), dtype=np.uint64)
    check(lib().cnt_complement(_p(bits), length, _p(out)))
    return out


def reverse_complement_hip(bits, length):
    bits = _packed(bits, length)
    out = np.empty(lib().cnt_words_for(length), dtype=np.uint64)
    check(lib().cnt_reverse_complement(_p(bits), length, _p(out)))
    return out


def _n_kmers(length, k):
    if not 1 <= k <= 32:
        raise ValueError("k must be in 1..32")
    return length - k + 1 if length >= k else 0


def kmers_hip(bits, length, k, canonical=False, out=None):
    """The length-k+1 k-mers of the sequence as np.uint64 (include/cute_nt.h "k-mers"): k-mer i packed like a sequence of
    length k, or with canonical=True the smaller of it and its reverse complement as u64.  `out` (optional, >= m uint64, e.g.
    from pinned_empty) receives them; the [:m] view is returned."""
    bits = _packed(bits, length)
    m = _n_kmers(length, k)
    if out is None:
        out = np.empty(m, dtype=np.uint64)
    elif out.dtype != np.uint64 or not out.flags.c_contiguous or out.size < m:
        raise ValueError("out must be a contiguous uint64 array with >= %d elements" % m)
    check(lib().cnt_kmers(_p(bits), length, k, CNT_KMER_CANONICAL if canonical else 0, _p(out), out.size))
    return out[:m]


KMER_COUNTS_MAX_K = 12


def _n_bins(k):
    if not 1 <= k <= KMER_COUNTS_MAX_K:
        raise ValueError("k must be in 1..%d" % KMER_COUNTS_MAX_K)
    return 4 ** k


def kmer_counts_hip(bits, length, k, canonical=False):
    """The k-mer spectrum of the sequence as np.uint64[4**k] (include/cute_nt.h "k-mer counts"): entry v is the number of
    k-mers whose kmers_hip value (same `canonical`) is v; 1 <= k <= 12.  k = 1 is base composition in code order A, C, T, G."""
    bins = _n_bins(k)
    bits = _packed(bits, length)
    out = np.empty(bins, dtype=np.uint64)
    check(lib().cnt_kmer_counts(_p(bits), length, k, CNT_KMER_CANONICAL if canonical else 0, _p(out), out.size))
    return out


WINDOW_COUNTS_MAX_K = 2


def _window_shape(length, k, window, step):
    """(n_win, step) of the windowed counts after the C rules (include/cute_nt.h "windowed composition", rule 1); step=None
    means window"""
    if not 1 <= k <= WINDOW_COUNTS_MAX_K:
        raise ValueError("k must be in 1..%d" % WINDOW_COUNTS_MAX_K)
    if step is None:
        step = window
    if step < 1:
        raise ValueError("step must be at least 1")
    if not k <= window < 2 ** 32:
        raise ValueError("window must be in k..2^32-1")
    if length < 0:
        raise ValueError("length must not be negative")
    return ((length - window) // step + 1 if length >= window else 0), step


def window_counts_n(length, k, window, step=None):
    """the number of windows window_counts_hip reports: (length - window) // step + 1, or 0 when length < window; there is no
    partial window at the end"""
    n_win, step = _window_shape(length, k, window, step)
    out = ctypes.c_size_t(0)
    check(lib().cnt_window_counts_n(length, k, window, step, ctypes.byref(out)))
    assert out.value == n_win
    return n_win


def window_counts_hip(bits, length, k, window, step=None):
    """Base (k = 1) or dinucleotide (k = 2) counts per window as np.uint32[n_win, 4**k] (include/cute_nt.h "windowed
    composition"): row j counts the k-mers that lie wholly inside [j*step, j*step + window), entry v those whose kmers_hip value
    is v (k = 1: A, C, T, G; k = 2: first base + 4 * second base).  step=None means window: adjacent windows."""
    n_win, step = _window_shape(length, k, window, step)
    bits = _packed(bits, length)
    out = np.empty((n_win, 4 ** k), dtype=np.uint32)
    check(lib().cnt_window_counts(_p(bits), length, k, window, step, 0, _p(out), n_win))
    return out


def gc_content_hip(bits, length, window, step=None):
    """GC content per window as np.float64[n_win]: (C + G) / window, from window_counts_hip with k = 1"""
    c = window_counts_hip(bits, length, 1, window, step)
    return (c[:, 1].astype(np.float64) + c[:, 3]) / window


def _n_windows(length, k, w):
    if not 1 <= w <= 256:
        raise ValueError("w must be in 1..256")
    m = _n_kmers(length, k)
    return m - w + 1 if m >= w else 0


def _counted_hip(fn, cap, n_out, last, *args):
    """The host tier of a call whose output size depends on the data: fn(*args, outputs..., cap, &n) with n_out uint64 outputs of
    `cap` entries, the last one absent (NULL, returned as None) unless `last`.  A guess of cap that was short (CNT_ECAP) is
    replaced once by the n the call reported.  Returns the [:n] views."""
    for attempt in range(2):
        outs = [np.empty(cap, dtype=np.uint64) if last or j < n_out - 1 else None for j in range(n_out)]
        n = ctypes.c_uint64(0)
        rc = fn(*args, *(_p(o) if o is not None else None for o in outs), cap, ctypes.byref(n))
        if rc == _lib.CNT_ECAP and attempt == 0:
            cap = n.value
            continue
        check(rc)
        return tuple(o[: n.value] if o is not None else None for o in outs)


def minimizers_hip(bits, length, k, w, canonical=False, values=True):
    """The (w,k)-minimizers of the sequence (include/cute_nt.h "k-mers"): in each window of w consecutive k-mers the
    position with the smallest (fmix64(k-mer), position), each distinct position once, ascending.  Returns numpy uint64
    (pos, val) of length n, val the k-mers at pos (forward, or canonical with canonical=True), or None with values=False.
    The output buffers start at a guess of n and are sized to the reported n once if the guess was short."""
    bits = _packed(bits, length)
    n_win = _n_windows(length, k, w)
    cap = min(n_win, 2 * n_win // (w + 1) + n_win // 16 + 64)  # a random sequence selects ~2/(w+1) of its windows
    return _counted_hip(lib().cnt_minimizers, cap, 2, values, _p(bits), length, k, w, CNT_KMER_CANONICAL if canonical else 0)


_PATTERN_CODES = {"A": 0, "C": 1, "T": 2, "U": 2, "G": 3}


def pattern_from_ascii(s):
    """(pattern, wildcards, k) of a search pattern spelled in ACGTU (either case) and N: position j's code (A0 C1 T2 G3) at
    bits 2j of `pattern`, N / n a wildcard (bit j of `wildcards`, code 0 in `pattern`).  1..32 letters; anything else raises
    ValueError."""
    if isinstance(s, (bytes, bytearray)):
        s = bytes(s).decode("latin-1")
    if not isinstance(s, str) or not 1 <= len(s) <= 32:
        raise ValueError("a pattern is 1..32 letters of ACGTUN")
    pattern = wildcards = 0
    for j, ch in enumerate(s.upper()):
        if ch == "N":
            wildcards |= 1 << j
        elif ch in _PATTERN_CODES:
            pattern |= _PATTERN_CODES[ch] << (2 * j)
        else:
            raise ValueError("pattern letter %r at %d is not one of ACGTUN" % (s[j], j))
    return pattern, wildcards, len(s)


def _pattern(pattern, max_mismatches):
    """a pattern argument -- the ASCII spelling or the (pattern, wildcards, k) triple -- checked as the library would"""
    if isinstance(pattern, (str, bytes, bytearray)):
        pattern = pattern_from_ascii(pattern)
    p, wild, k = (int(v) for v in pattern)
    if not 1 <= k <= 32:
        raise ValueError("k must be in 1..32")
    if p < 0 or p >> (2 * k) or wild < 0 or wild >> k:
        raise ValueError("pattern bits at or above 2k, or wildcard bits at or above k")
    if not 0 <= max_mismatches <= k:
        raise ValueError("max_mismatches must be in 0..k")
    return p, wild, k


def find_pattern_hip(bits, length, pattern, max_mismatches=0, both_strands=False, info=True):
    """Where `pattern` (an ASCII string for pattern_from_ascii, or its (pattern, wildcards, k) triple) occurs in the sequence
    with at most max_mismatches substitutions (include/cute_nt.h "pattern search"), on the forward strand or with
    both_strands=True also where the reverse strand reads it.  Returns numpy uint64 (pos, info) of length n, ordered by
    position, forward before reverse: info = the hit's mismatch count, plus CNT_FIND_REVERSE on the reverse strand (None with
    info=False).  The output buffers start at a guess of n and are sized to the reported n once if the guess was short."""
    p, wild, k = _pattern(pattern, max_mismatches)
    bits = _packed(bits, length)
    m = _n_kmers(length, k)
    most = 2 * m if both_strands else m
    cap = min(most, most // 1024 + 1024)  # a real search reports a handful of sites
    return _counted_hip(lib().cnt_find_pattern, cap, 2, info, _p(bits), length, p, k, wild, max_mismatches, CNT_FIND_BOTH_STRANDS if both_strands else 0)


def _subseq_bounds(length, start, sub_len):
    start, sub_len = int(start), int(sub_len)
    if start < 0 or sub_len < 0 or start > length or sub_len > length - start:
        raise ValueError("the subsequence [%d, %d + %d) does not lie inside the %d nucleotides" % (start, start, sub_len, length))
    return start, sub_len


def _region_len(region_len):
    region_len = int(region_len)
    if region_len < 0:
        raise ValueError("region_len must not be negative")
    return region_len


def subseq_hip(bits, length, start, sub_len, revcomp=False):
    """Nucleotides [start, start + sub_len) of the sequence as a packed sequence of their own (include/cute_nt.h "region
    extraction"), np.uint64[words_for(sub_len)]; with revcomp=True their reverse complement.  `start` may be any nucleotide,
    not only a multiple of 32.  Bounds outside the sequence raise ValueError."""
    bits = _packed(bits, length)
    start, sub_len = _subseq_bounds(length, start, sub_len)
    out = np.empty(lib().cnt_words_for(sub_len), dtype=np.uint64)
    check(lib().cnt_subseq(_p(bits), length, start, sub_len, CNT_EXTRACT_REVCOMP if revcomp else 0, _p(out), out.size))
    return out


def _regions(starts, info):
    """the host tier's starts / info: contiguous uint64 arrays of one length"""
    starts = np.asarray(starts)
    if starts.dtype != np.uint64:
        raise TypeError("starts must be a uint64 array")
    starts = np.ascontiguousarray(starts).reshape(-1)
    if info is not None:
        info = np.asarray(info)
        if info.dtype != np.uint64:
            raise TypeError("info must be a uint64 array")
        info = np.ascontiguousarray(info).reshape(-1)
        if info.size != starts.size:
            raise ValueError("info must have one entry per start")
    return starts, info


def extract_hip(bits, length, starts, region_len, info=None, revcomp=False):
    """The n regions [starts[i], starts[i] + region_len) of the sequence (include/cute_nt.h "region extraction"): returns
    (records, rejected), records np.uint64[n, R] with R = words_for(region_len), row i packed like a sequence of length
    region_len.  Region i comes out reverse-complemented iff exactly one of `revcomp` and info[i] & CNT_FIND_REVERSE holds --
    `info` may be the array find_pattern_hip returned, so that every hit reads as the pattern does.  A region that does not lie
    inside the sequence is a row of zeros and is counted in `rejected`."""
    bits = _packed(bits, length)
    region_len = _region_len(region_len)
    starts, info = _regions(starts, info)
    n, R = starts.size, lib().cnt_words_for(region_len)
    out = np.empty(n * R, dtype=np.uint64)
    rejected = ctypes.c_uint64(0)
    if bits.size == 0:
        bits = np.zeros(1, dtype=np.uint64)  # no nucleotide: every region is rejected, but the library wants an address
    check(lib().cnt_extract(_p(bits), length, _p(starts), _p(info) if info is not None else None, n, region_len,
                            CNT_EXTRACT_REVCOMP if revcomp else 0, _p(out), out.size, ctypes.byref(rejected)))
    return out.reshape(n, R), rejected.value


# NCBI genetic codes as the NCBI prints them: one amino acid per codon in TCAG order, base 1 slowest
_NCBI_CODES = {
    1: "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    2: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG",
    4: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    11: "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
}
_TCAG_CODES = (2, 1, 0, 3)  # the codes (A0 C1 T2 G3) of T, C, A, G


def codon_table(ncbi_id=1):
    """The 64-byte translation table of an NCBI genetic code (1 standard, 2 vertebrate mitochondrial, 4 mold / protozoan
    mitochondrial and mycoplasma, 11 bacterial; stops as `*`) in the library's index order: entry c = x0 | x1 << 2 | x2 << 4 is
    the amino acid of the codon whose bases have the codes x0, x1, x2 (include/cute_nt.h "translation")."""
    if ncbi_id not in _NCBI_CODES:
        raise ValueError("genetic code %r is not one of %s" % (ncbi_id, sorted(_NCBI_CODES)))
    aas = _NCBI_CODES[ncbi_id]
    table = bytearray(64)
    for i, x0 in enumerate(_TCAG_CODES):
        for j, x1 in enumerate(_TCAG_CODES):
            for k, x2 in enumerate(_TCAG_CODES):
                table[x0 | x1 << 2 | x2 << 4] = ord(aas[16 * i + 4 * j + k])
    return bytes(table)


def _codon_table(table):
    """a table argument as the 64 bytes the library reads (None: its built-in standard code)"""
    if table is None:
        return None
    if isinstance(table, (bytes, bytearray)):
        table = bytes(table)
    elif isinstance(table, np.ndarray):
        if table.dtype != np.uint8:
            raise TypeError("a translation table is 64 bytes: bytes or a uint8 array")
        table = np.ascontiguousarray(table).tobytes()
    else:
        raise TypeError("a translation table is 64 bytes: bytes or a uint8 array")
    if len(table) != 64:
        raise ValueError("a translation table has 64 entries, not %d" % len(table))
    return table


def _translate_region(length, start, sub_len):
    return _subseq_bounds(length, start, length - int(start) if sub_len is None else sub_len)


def _six_frames(length):
    """(start, sub_len, revcomp) of the frames +0, +1, +2, -0, -1, -2 of a whole sequence (a frame past its end is empty)"""
    skip = [min(f, length) for f in range(3)]
    return [(f, length - f, False) for f in skip] + [(0, length - f, True) for f in skip]


def translate_hip(bits, length, start=0, sub_len=None, revcomp=False, table=None):
    """Nucleotides [start, start + sub_len) of the sequence (sub_len=None: to its end) translated codon by codon (include/cute_nt.h
    "translation"): np.uint8[sub_len // 3], one byte of `table` per codon; with revcomp=True the region is read as its reverse
    complement.  `table` is 64 bytes (bytes or a uint8 array, e.g. codon_table(11)); None is the standard genetic code with stops
    as `*`.  Forward frame f of a whole sequence is start=f; reverse frame f is sub_len=length - f with revcomp=True."""
    bits = _packed(bits, length)
    start, sub_len = _translate_region(length, start, sub_len)
    table = _codon_table(table)
    out = np.empty(sub_len // 3, dtype=np.uint8)
    if sub_len >= 3:
        check(lib().cnt_translate(_p(bits), length, start, sub_len, CNT_TRANSLATE_REVCOMP if revcomp else 0, table, _p(out), out.size))
    return out


def six_frames_hip(bits, length, table=None):
    """The six translations of the whole sequence, in the order +0, +1, +2, -0, -1, -2 (see translate_hip)."""
    return [translate_hip(bits, length, start, sub_len, rev, table) for start, sub_len, rev in _six_frames(length)]


def codon_set(codons):
    """The 64-bit set of codon values (include/cute_nt.h "ORF scan") of an iterable of three-letter codons spelled in ACGTU
    (either case): bit x0 | x1 << 2 | x2 << 4 for the codes (A0 C1 T2 G3) of each.  Anything else raises ValueError."""
    if isinstance(codons, (str, bytes, bytearray)):
        raise ValueError("a codon set is a list of three-letter codons, not one string")
    mask = 0
    for codon in codons:
        if isinstance(codon, (bytes, bytearray)):
            codon = bytes(codon).decode("latin-1")
        if not isinstance(codon, str) or len(codon) != 3 or any(ch not in _PATTERN_CODES for ch in codon.upper()):
            raise ValueError("codon %r is not three letters of ACGTU" % (codon,))
        x = [_PATTERN_CODES[ch] for ch in codon.upper()]
        mask |= 1 << (x[0] | x[1] << 2 | x[2] << 4)
    return mask


def _orf_args(stops, starts, min_len):
    """the stops / starts arguments -- masks or lists of codons -- and min_len, checked as the library would"""
    masks = []
    for name, v in (("stops", stops), ("starts", starts)):
        if v is None:
            v = 0
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            v = codon_set(v)
        v = int(v)
        if v < 0 or v >> 64:
            raise ValueError("%s must be a 64-bit set of codon values" % name)
        masks.append(v)
    if masks[0] == 0:
        raise ValueError("stops must hold at least one codon")
    min_len = int(min_len)
    if min_len < 0:
        raise ValueError("min_len must not be negative")
    return masks[0], masks[1], min_len


def orfs_hip(bits, length, stops=CNT_ORF_STOPS_STANDARD, starts=CNT_ORF_STARTS_ATG, min_len=0, both_strands=False, info=True):
    """The open reading frames of the sequence (include/cute_nt.h "ORF scan"): the stop-free runs of each frame lane, on the
    forward strand or with both_strands=True on both, trimmed to their first start codon (starts=0 or None: reported whole), at
    least min_len nucleotides long.  `stops` / `starts` are 64-bit sets of codon values or lists of codons for codon_set.
    Returns numpy uint64 (pos, length, info) of n entries ordered by the upper end of the run, forward before reverse: info =
    the frame, plus CNT_FIND_REVERSE, CNT_ORF_OPEN_END, CNT_ORF_NO_STOP (None with info=False) -- translate_hip(bits, length,
    pos[j], length[j], revcomp=reverse) is the protein, and extract_hip takes pos and info as they are.  The output buffers
    start at a guess of n and are sized to the reported n once if the guess was short."""
    stops, starts, min_len = _orf_args(stops, starts, min_len)
    bits = _packed(bits, length)
    most = (2 * length if both_strands else length) if length >= 3 else 0
    cap = min(most, most // 16 + 1024)  # random sequence: a stop every ~21 codons of a lane
    return _counted_hip(lib().cnt_orfs, cap, 3, info, _p(bits), length, stops, starts, min_len, CNT_ORF_BOTH_STRANDS if both_strands else 0)


def hpc_hip(bits, length, with_pos=False):
    """Homopolymer compression of the sequence (include/cute_nt.h "homopolymer compression"): every run of equal bases collapses
    to one base.  Returns (out, n) -- np.uint64[words_for(n)] holding the n run bases packed like any sequence, so that every
    call here takes (out, n) -- and with with_pos=True (out, n, pos): pos[j] is where run j starts in the input, its length
    pos[j + 1] - pos[j] (length - pos[n - 1] for the last).  The output buffers start at a guess of n and are sized to the
    reported n once if the guess was short."""
    bits = _packed(bits, length)
    cap = min(length, length // 4 * 3 + length // 64 + 64)  # a random sequence keeps three bases of four
    for attempt in range(2):
        out = np.empty(lib().cnt_words_for(cap), dtype=np.uint64)
        pos = np.empty(cap, dtype=np.uint64) if with_pos else None
        n = ctypes.c_uint64(0)
        rc = lib().cnt_hpc(_p(bits), length, 0, _p(out), _p(pos) if with_pos else None, cap, ctypes.byref(n))
        if rc == _lib.CNT_ECAP and attempt == 0:
            cap = n.value
            continue
        check(rc)
        out = out[: lib().cnt_words_for(n.value)]
        return (out, n.value, pos[: n.value]) if with_pos else (out, n.value)


def hpc_minimizers_hip(bits, length, k, w, flags=0):
    """The (w,k)-minimizers of the homopolymer-compressed sequence, in the coordinates of the sequence itself (minimap2 -H): hpc_hip
    with positions, minimizers_hip on its (out, n), and each minimizer's position looked up in the run starts.  `flags` is 0 or
    CNT_KMER_CANONICAL.  Returns numpy uint64 (pos, val): pos[j] is where the first run of minimizer j begins in `bits`, val[j] its
    k-mer of run bases."""
    if flags & ~CNT_KMER_CANONICAL:
        raise ValueError("flags must be 0 or CNT_KMER_CANONICAL")
    out, n, run_pos = hpc_hip(bits, length, with_pos=True)
    pos, val = minimizers_hip(out, n, k, w, canonical=bool(flags & CNT_KMER_CANONICAL))
    return run_pos[pos.astype(np.int64)], val


def _fasta_text(text):
    """the host tier's text: bytes, bytearray, mmap, memoryview or a uint8 array, as a contiguous uint8 array without a copy"""
    if isinstance(text, np.ndarray):
        return _u8(text)
    try:
        return np.frombuffer(text, dtype=np.uint8)
    except (TypeError, ValueError, BufferError):
        raise TypeError("text must be bytes, a bytearray, an mmap or a uint8 array")


def fasta_to_bits_hip(text, strict_lut=False, allow_n=False):
    """Encode FASTA text (include/cute_nt.h "text formats: FASTA"): header lines, line feeds and carriage returns are dropped, every
    other byte is encoded as n_to_bits_hip encodes it (strict_lut: BYTE_LUT).  `text` is bytes, a bytearray, an mmap or a uint8
    array.  Returns (words, n, rec_text, rec_start, invalid): np.uint64[words_for(n)] holding the n kept nucleotides, so that every
    call here takes (words, n); per header line the byte offset of its '>' and the position in `words` of the record's first base
    (record r ends at rec_start[r + 1], the last one at n; fasta_names gives the names); and the number of kept bytes outside
    ACGTUacgtu (allow_n: and Nn).  The record arrays start at a guess of the number of header lines and are sized to the reported
    number once if the guess was short."""
    text = _fasta_text(text)
    length = text.size
    flags = (_lib.CNT_STRICT_LUT if strict_lut else 0) | (CNT_ALLOW_N if allow_n else 0)
    out = np.empty(lib().cnt_words_for(length), dtype=np.uint64)
    rec_cap = min(length, length // 4096 + 1024)  # a header every 4096 bytes or so
    counts = (ctypes.c_uint64 * 3)()
    for attempt in range(2):
        rec_text = np.empty(rec_cap, dtype=np.uint64)
        rec_start = np.empty(rec_cap, dtype=np.uint64)
        rc = lib().cnt_fasta_to_bits(_p(text), length, flags, _p(out) if length else None, length, _p(rec_text), _p(rec_start), rec_cap, counts)
        if rc == _lib.CNT_ECAP and attempt == 0:
            rec_cap = counts[1]
            continue
        check(rc)
        n, records = counts[0], counts[1]
        return out[: lib().cnt_words_for(n)], n, rec_text[:records], rec_start[:records], counts[2]


def fasta_names(text, rec_text):
    """the header lines of a FASTA text at the byte offsets fasta_to_bits_hip reported, as a list of bytes: each without its '>'
    and without its line end (a line feed, or a carriage return and a line feed; the last line may have neither)"""
    buf = _fasta_text(text)
    names = []
    for at in np.asarray(rec_text, dtype=np.uint64).tolist():
        if at >= buf.size or buf[at] != 0x3E:
            raise ValueError("no header line starts at byte %d" % at)
        line, look = b"", 256
        while True:  # a look at a time, so that a short name in a long text costs its own length
            piece = buf[at + 1 + len(line) : at + 1 + len(line) + look].tobytes()
            end = piece.find(b"\n")
            line += piece if end < 0 else piece[:end]
            if end >= 0 or len(piece) < look:
                break
            look *= 4
        names.append(line[:-1] if line.endswith(b"\r") else line)
    return names


Fastq = collections.namedtuple("Fastq", "words n qual rec_text rec_start rec_qual invalid malformed")


def fastq_to_bits_hip(text, strict_lut=False, allow_n=False, with_qual=True):
    """Encode strict four-line FASTQ text (include/cute_nt.h "text formats: FASTQ"): the role of a byte is its line number mod 4
    (name, sequence, separator, quality), line feeds and carriage returns are dropped, the sequence bytes are encoded as
    n_to_bits_hip encodes them (strict_lut: BYTE_LUT) and the quality bytes are copied as they are.  `text` is bytes, a bytearray,
    an mmap or a uint8 array.  Returns the named tuple (words, n, qual, rec_text, rec_start, rec_qual, invalid, malformed):
    np.uint64[words_for(n)] holding the n nucleotides; the quality bytes as np.uint8 (None without with_qual); per record the byte
    offset of its name line and the positions of its first base in `words` and of its first quality in `qual` (record r ends at
    entry r + 1, the last one at n and at qual.size; fastq_names gives the names); the number of sequence bytes outside ACGTUacgtu
    (allow_n: and Nn); and the number of name lines that do not begin with '@' plus separator lines that do not begin with '+'.
    A well-formed file has malformed == 0 and rec_qual equal to rec_start.  The record arrays start at a guess of the number of
    records and are sized to the reported number once if the guess was short."""
    text = _fasta_text(text)
    length = text.size
    flags = (_lib.CNT_STRICT_LUT if strict_lut else 0) | (CNT_ALLOW_N if allow_n else 0)
    out = np.empty(lib().cnt_words_for(length), dtype=np.uint64)
    qual = np.empty(length, dtype=np.uint8) if with_qual else None
    rec_cap = min(length, length // 256 + 1024)  # a record every 256 bytes or so
    counts = (ctypes.c_uint64 * 5)()
    for attempt in range(2):
        rec = [np.empty(rec_cap, dtype=np.uint64) for _ in range(3)]
        rc = lib().cnt_fastq_to_bits(_p(text), length, flags, _p(out) if length else None, length, _p(qual) if with_qual and length else None, length,
                                     _p(rec[0]), _p(rec[1]), _p(rec[2]), rec_cap, counts)
        if rc == _lib.CNT_ECAP and attempt == 0:
            rec_cap = counts[1]
            continue
        check(rc)
        n, records = counts[0], counts[1]
        return Fastq(out[: lib().cnt_words_for(n)], n, qual[: counts[3]] if with_qual else None, rec[0][:records], rec[1][:records], rec[2][:records],
                     counts[2], counts[4])


def fastq_names(text, rec_text):
    """the name lines of a FASTQ text at the byte offsets fastq_to_bits_hip reported, as a list of bytes: each without its '@' and
    without its line end (a line feed, or a carriage return and a line feed; the last line may have neither)"""
    buf = _fasta_text(text)
    names = []
    for at in np.asarray(rec_text, dtype=np.uint64).tolist():
        if at >= buf.size or buf[at] != 0x40 or (at and buf[at - 1] != 0x0A):
            raise ValueError("no name line starts at byte %d" % at)
        line, look = b"", 256
        while True:  # a look at a time, so that a short name in a long text costs its own length
            piece = buf[at + 1 + len(line) : at + 1 + len(line) + look].tobytes()
            end = piece.find(b"\n")
            line += piece if end < 0 else piece[:end]
            if end >= 0 or len(piece) < look:
                break
            look *= 4
        names.append(line[:-1] if line.endswith(b"\r") else line)
    return names


def bits_to_fasta_bound(length, n_rec=0, names_len=0, width=60):
    """the most bytes of FASTA text bits_to_fasta_hip writes for `length` nucleotides in n_rec records whose names hold names_len
    bytes, at `width` letters a line: a pure host function, the footprint of the device tier's `text`"""
    return _work_bytes(lib().cnt_bits_to_fasta_bound, length, n_rec, names_len, width)


def _fasta_name_table(names, n_rec):
    """a list of bytes as fasta_names returns it -> (the names back to back as uint8, never empty; n_rec + 1 uint64 offsets)"""
    names = [bytes(name) for name in names]
    if len(names) != n_rec:
        raise ValueError("one name per record")
    name_off = np.zeros(n_rec + 1, dtype=np.uint64)
    name_off[1:] = np.cumsum([len(name) for name in names], dtype=np.uint64)
    joined = np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8)  # an address even when every name is empty
    return joined, name_off


def bits_to_fasta_hip(bits, length, rec_start=None, names=None, width=60):
    """Write packed nucleotides as FASTA text (include/cute_nt.h "text formats: FASTA write"): the bases in front of
    rec_start[0] as headerless lines, then per record '>', its name, a line feed and its bases [rec_start[r], rec_start[r + 1])
    -- the last record ends at `length` -- in lines of `width` letters (0: one line per record).  `names` is a list of bytes, one
    per record, as fasta_names returns it; None: every name is empty.  Names are copied as they are.  Returns (text, rec_text):
    the text as np.uint8 and the byte offset of every record's '>' as np.uint64.  fasta_to_bits_hip(text) gives `bits`, `length`,
    `rec_start` and `rec_text` back.  A rec_start that descends or passes `length` is an error and writes nothing."""
    bits = _packed(bits, length)
    rec_start = np.zeros(0, dtype=np.uint64) if rec_start is None else _u64(rec_start)
    n_rec = rec_start.size
    width = int(width)
    if width < 0:
        raise ValueError("width must not be negative")
    joined, name_off = _fasta_name_table(names, n_rec) if names is not None else (None, None)
    names_len = int(name_off[-1]) if names is not None else 0
    cap = bits_to_fasta_bound(length, n_rec, names_len, width)
    text = np.empty(max(cap, 1), dtype=np.uint8)
    rec_text = np.empty(n_rec, dtype=np.uint64)
    counts = (ctypes.c_uint64 * 2)()
    check(lib().cnt_bits_to_fasta(_p(bits) if length else None, length, _p(rec_start), n_rec, _p(joined) if names is not None else None, names_len,
                                  _p(name_off) if names is not None else None, width, 0, _p(text), cap, _p(rec_text), counts))
    return text[: counts[0]], rec_text


def bits_to_fastq_bound(length, n_rec=0, names_len=0):
    """the most bytes of FASTQ text bits_to_fastq_hip writes for `length` nucleotides in n_rec records whose names hold names_len
    bytes: a pure host function, the footprint of the device tier's `text`"""
    return _work_bytes(lib().cnt_bits_to_fastq_bound, length, n_rec, names_len)


def bits_to_fastq_hip(bits, length, qual, rec_start, names=None):
    """Write packed nucleotides and their quality bytes as four-line FASTQ text (include/cute_nt.h "text formats: FASTQ write"):
    per record '@', its name, a line feed, its bases [rec_start[r], rec_start[r + 1]) -- the first record begins at 0, the last
    one ends at `length` -- a line feed, '+', a line feed, the quality bytes of the same positions and a line feed.  `qual` is
    bytes or a uint8 array of `length` bytes, copied as they are; `names` is a list of bytes, one per record, as fastq_names
    returns it; None: every name is empty.  Returns the text as bytes; fastq_to_bits_hip(text) gives `bits`, `length`, `qual` and
    `rec_start` (as rec_start and as rec_qual) back.  A rec_start that descends, passes `length` or does not begin at 0 is an
    error and writes nothing."""
    bits = _packed(bits, length)
    qual = _fasta_text(qual)
    if qual.size != length:
        raise ValueError("one quality byte per nucleotide")
    rec_start = _u64(rec_start)
    n_rec = rec_start.size
    joined, name_off = _fasta_name_table(names, n_rec) if names is not None else (None, None)
    names_len = int(name_off[-1]) if names is not None else 0
    cap = bits_to_fastq_bound(length, n_rec, names_len)
    text = np.empty(max(cap, 1), dtype=np.uint8)
    counts = (ctypes.c_uint64 * 2)()
    check(lib().cnt_bits_to_fastq(_p(bits) if length else None, length, _p(qual) if length else None, _p(rec_start), n_rec,
                                  _p(joined) if names is not None else None, names_len, _p(name_off) if names is not None else None, 0, _p(text), cap, None, counts))
    return text[: counts[0]].tobytes()


def validate_hip(n, allow_n=False):
    """Number of bytes that are not nucleotides (0 = the buffer is a valid sequence)."""
    n = _u8(n)
    out = ctypes.c_uint64(0)
    check(lib().cnt_validate(_p(n), n.size, CNT_ALLOW_N if allow_n else 0, ctypes.byref(out)))
    return out.value


# ---- device tier --------------------------------------------------------------------------
def hamming_dev(a, b, length, acc=None):
    torch = _dev_guard(a)
    _dev_guard(b)
    if a.dtype != torch.int64 or b.dtype != torch.int64:
        raise TypeError("packed words must be int64 tensors")
    if a.device != b.device:
        raise ValueError("both sequences must live on the same device")
    if length > min(a.numel(), b.numel()) * 32:
        raise ValueError("The length is greater than the number of nucleotides!")
    acc = _counter(torch, acc, a)
    _enqueue(a, lib().cnt_hamming_dev, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), length, ctypes.c_void_p(acc.data_ptr()))
    return acc  # device scalar: .item() syncs


def _unary_dev(fn, bits, length, out):
    torch = _packed_dev(bits, length)
    words = lib().cnt_words_for(length)
    out = _out_words(torch, out, words, bits)
    _enqueue(bits, fn, ctypes.c_void_p(bits.data_ptr()), length, ctypes.c_void_p(out.data_ptr()))
    return out[:words]


def complement_dev(bits, length, out=None):
    """Device tier of complement_hip, enqueued on torch's current stream: the [:words_for(length)] view of an int64 tensor (`out`
    if given).  In place works: complement_dev(x, n, out=x) overwrites x with its complement (out and bits at the SAME address);
    an `out` that overlaps `bits` in any other way is refused with CNT_EINVAL."""
    return _unary_dev(lib().cnt_complement_dev, bits, length, out)


def reverse_complement_dev(bits, length, out=None):
    """Device tier of reverse_complement_hip, enqueued on torch's current stream.  Not in place: an `out` that shares any word
    with `bits` (out=bits included) is refused with CNT_EINVAL."""
    return _unary_dev(lib().cnt_reverse_complement_dev, bits, length, out)


def kmers_dev(bits, length, k, canonical=False, out=None):
    """Device tier of kmers_hip: `bits` an int64 CUDA tensor, the result the [:m] view of an int64 tensor (`out` if given)
    enqueued on torch's current stream."""
    torch = _packed_dev(bits, length)
    m = _n_kmers(length, k)
    out = _out_words(torch, out, m, bits)
    _enqueue(bits, lib().cnt_kmers_dev, ctypes.c_void_p(bits.data_ptr()), length, k, CNT_KMER_CANONICAL if canonical else 0,
             ctypes.c_void_p(out.data_ptr()), out.numel())
    return out[:m]


def kmer_counts_dev(bits, length, k, canonical=False, out=None):
    """Device tier of kmer_counts_hip, enqueued on torch's current stream: returns the [:4**k] view of an int64 CUDA tensor.
    A given `out` (contiguous int64, on the input's device, >= 4**k entries) is ADDED TO -- count several sequences or chunks
    into one spectrum -- and its entries past 4**k are left alone; without one a zeroed table is allocated."""
    bins = _n_bins(k)
    torch = _packed_dev(bits, length)
    out = torch.zeros(bins, dtype=torch.int64, device=bits.device) if out is None else _out_words(torch, out, bins, bits)
    _enqueue(bits, lib().cnt_kmer_counts_dev, ctypes.c_void_p(bits.data_ptr()), length, k, CNT_KMER_CANONICAL if canonical else 0,
             ctypes.c_void_p(out.data_ptr()), out.numel())
    return out[:bins]


def window_counts_dev(bits, length, k, window, step=None, out=None):
    """Device tier of window_counts_hip, enqueued on torch's current stream: returns the (n_win, 4**k) view of an int32 CUDA
    tensor (the bit pattern of the u32 counts).  A given `out` (contiguous int32, on the input's device, >= n_win * 4**k
    entries, at an 8-byte aligned address) is SET in those entries and left alone behind them."""
    n_win, step = _window_shape(length, k, window, step)
    torch = _packed_dev(bits, length)
    bins = 4 ** k
    if out is None:
        out = torch.empty(n_win * bins, dtype=torch.int32, device=bits.device)
    elif out.dtype != torch.int32 or not out.is_cuda or not out.is_contiguous() or out.device != bits.device or out.numel() < n_win * bins:
        raise ValueError("out must be a contiguous int32 CUDA tensor on the input's device with >= %d elements" % (n_win * bins))
    _enqueue(bits, lib().cnt_window_counts_dev, ctypes.c_void_p(bits.data_ptr()), length, k, window, step, 0, ctypes.c_void_p(out.data_ptr()),
             out.numel() // bins)
    return out.reshape(-1)[: n_win * bins].view(n_win, bins)


def _work_bytes(fn, *args):
    out = ctypes.c_size_t(0)
    check(fn(*args, ctypes.byref(out)))
    return out.value


def _counted_dev(torch, bits, most, pos, others, count, work, need):
    """The device tier's common part of a call whose output size depends on the data.  `pos` is the caller's (any capacity: the
    first min(n, capacity) entries are written) or None for `most` entries; each of `others` is None for a fresh tensor, False
    for an output that is not written, the caller's tensor (at least as long as pos), or an exception to raise in its turn.
    `count` and `work` (>= need bytes) are the caller's or None.  Returns (pos, others, count, ptrs): the tensors (None where
    not written) and the trailing arguments of the _dev entry point from pos to work_bytes."""
    pos = _out_words(torch, pos, 0, bits) if pos is not None else torch.empty(max(most, 1), dtype=torch.int64, device=bits.device)
    outs = []
    for t in others:
        if isinstance(t, Exception):
            raise t
        if t is False:
            outs.append(None)
        else:
            outs.append(_out_words(torch, t, pos.numel(), bits) if t is not None else torch.empty(max(pos.numel(), 1), dtype=torch.int64, device=bits.device))
    count = _out_words(torch, count, 1, bits)
    if work is None:
        work = torch.empty(max(need, 1), dtype=torch.uint8, device=bits.device)
    elif not work.is_cuda or not work.is_contiguous() or work.device != bits.device or work.numel() * work.element_size() < need:
        raise ValueError("work must be a contiguous CUDA tensor on the input's device with >= %d bytes" % need)
    # an empty view has no address (data_ptr() 0); at capacity 0 nothing is written, any aligned address will do
    ptrs = [ctypes.c_void_p(t.data_ptr() or count.data_ptr()) if t is not None else None for t in [pos] + outs]
    ptrs += [pos.numel(), ctypes.c_void_p(count.data_ptr()), ctypes.c_void_p(work.data_ptr()), work.numel() * work.element_size()]
    return pos, outs, count, ptrs


def minimizers_work_bytes(length, k, w):
    """bytes of device scratch cnt_minimizers_dev needs for this call (0 when there is no window)"""
    return _work_bytes(lib().cnt_minimizers_work_bytes, length, k, w)


def minimizers_dev(bits, length, k, w, canonical=False, values=True, pos=None, val=None, work=None, count=None):
    """Device tier of minimizers_hip, enqueued on torch's current stream without a synchronisation: returns (pos, val,
    count), int64 CUDA tensors, count a 1-element tensor that the call SETS to n; pos[:n] / val[:n] are the result once the
    stream has run (val is None with values=False).  Without `pos` / `val` they hold W = m-w+1 entries, the most n can be;
    given ones of any capacity receive the first min(n, capacity) entries.  `work` (>= minimizers_work_bytes bytes, any
    contents) and `count` may be reused across calls, e.g. in a captured graph."""
    torch = _packed_dev(bits, length)
    n_win = _n_windows(length, k, w)
    # a given pos / val may hold fewer than W entries (the first min(n, capacity) are written); val at least as many as pos
    if not values:
        val = ValueError("val given with values=False") if val is not None else False
    pos, (val,), count, ptrs = _counted_dev(torch, bits, n_win, pos, [val], count, work, minimizers_work_bytes(length, k, w))
    _enqueue(bits, lib().cnt_minimizers_dev, ctypes.c_void_p(bits.data_ptr()), length, k, w, CNT_KMER_CANONICAL if canonical else 0, *ptrs)
    return pos, val, count


def _info_arg(info):
    """info=True|False|tensor of find_pattern_dev and orfs_dev as _counted_dev takes it"""
    return None if info is True else False if info is False or info is None else info


def find_pattern_work_bytes(length, k):
    """bytes of device scratch cnt_find_pattern_dev needs for this call (0 when there is no window)"""
    return _work_bytes(lib().cnt_find_pattern_work_bytes, length, k)


def find_pattern_dev(bits, length, pattern, max_mismatches=0, both_strands=False, info=True, pos=None, work=None, count=None):
    """Device tier of find_pattern_hip, enqueued on torch's current stream without a synchronisation: returns (pos, info,
    count), int64 CUDA tensors, count a 1-element tensor that the call SETS to n; pos[:n] / info[:n] are the result once the
    stream has run.  `info` is True (a fresh tensor), False (none is written, None is returned) or the int64 tensor to write,
    at least as long as `pos`.  Without `pos` the outputs hold the most n can be (m windows, 2m with both_strands); a given
    one of any capacity receives the first min(n, capacity) entries.  `work` (>= find_pattern_work_bytes bytes, any contents)
    and `count` may be reused across calls, e.g. in a captured graph."""
    p, wild, k = _pattern(pattern, max_mismatches)
    torch = _packed_dev(bits, length)
    m = _n_kmers(length, k)
    most = 2 * m if both_strands else m
    pos, (inf,), count, ptrs = _counted_dev(torch, bits, most, pos, [_info_arg(info)], count, work, find_pattern_work_bytes(length, k))
    _enqueue(bits, lib().cnt_find_pattern_dev, ctypes.c_void_p(bits.data_ptr()), length, p, k, wild, max_mismatches,
             CNT_FIND_BOTH_STRANDS if both_strands else 0, *ptrs)
    return pos, inf, count


def subseq_dev(bits, length, start, sub_len, revcomp=False, out=None):
    """Device tier of subseq_hip, enqueued on torch's current stream: `bits` an int64 CUDA tensor, the result the
    [:words_for(sub_len)] view of an int64 tensor (`out` if given)."""
    torch = _packed_dev(bits, length)
    start, sub_len = _subseq_bounds(length, start, sub_len)
    words = lib().cnt_words_for(sub_len)
    out = _out_words(torch, out, words, bits)
    if sub_len:
        _enqueue(bits, lib().cnt_subseq_dev, ctypes.c_void_p(bits.data_ptr()), length, start, sub_len, CNT_EXTRACT_REVCOMP if revcomp else 0,
                 ctypes.c_void_p(out.data_ptr()), out.numel())
    return out[:words]


def _regions_dev(torch, starts, info, like):
    """the device tier's starts / info: contiguous int64 CUDA tensors of one length on the input's device"""
    for name, t in (("starts", starts), ("info", info)):
        if t is None:
            continue
        if not hasattr(t, "is_cuda") or t.dtype != torch.int64:
            raise TypeError("%s must be an int64 tensor" % name)
        if not t.is_cuda or not t.is_contiguous() or t.device != like.device or t.dim() != 1:
            raise ValueError("%s must be a contiguous 1-d CUDA tensor on the input's device" % name)
    if info is not None and info.numel() != starts.numel():
        raise ValueError("info must have one entry per start")


def extract_dev(bits, length, starts, region_len, info=None, revcomp=False, out=None, rejected=None):
    """Device tier of extract_hip, enqueued on torch's current stream without a synchronisation: `starts` (and `info`, e.g. the
    pos and info find_pattern_dev wrote) are int64 CUDA tensors holding the u64 values.  Returns (records, rejected): the
    [n, R] view of an int64 tensor (`out` if given, >= n*R elements) and a 1-element int64 tensor the call ADDS the number of
    rejected regions to (a fresh zeroed one unless the caller passes its own, which the caller zeroes)."""
    torch = _packed_dev(bits, length)
    region_len = _region_len(region_len)
    _regions_dev(torch, starts, info, bits)
    n, R = starts.numel(), lib().cnt_words_for(region_len)
    out = _out_words(torch, out, n * R, bits)
    rejected = _counter(torch, rejected, bits)
    if n and region_len:
        src = bits if bits.numel() else torch.zeros(1, dtype=torch.int64, device=bits.device)  # no nucleotide: every region is rejected
        _enqueue(bits, lib().cnt_extract_dev, ctypes.c_void_p(src.data_ptr()), length, ctypes.c_void_p(starts.data_ptr()),
                 ctypes.c_void_p(info.data_ptr()) if info is not None else None, n, region_len, CNT_EXTRACT_REVCOMP if revcomp else 0,
                 ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(rejected.data_ptr()))
    return out[: n * R].view(n, R), rejected


def translate_dev(bits, length, start=0, sub_len=None, revcomp=False, table=None, out=None):
    """Device tier of translate_hip, enqueued on torch's current stream: `bits` an int64 CUDA tensor, the result the
    [:sub_len // 3] view of a uint8 tensor (`out` if given, at any byte address).  `table` is HOST memory (bytes or a uint8 numpy
    array): the library reads it before this call returns."""
    torch = _packed_dev(bits, length)
    start, sub_len = _translate_region(length, start, sub_len)
    table = _codon_table(table)
    m = sub_len // 3
    out = _out_bytes(torch, out, m, bits)
    if sub_len >= 3:
        _enqueue(bits, lib().cnt_translate_dev, ctypes.c_void_p(bits.data_ptr()), length, start, sub_len, CNT_TRANSLATE_REVCOMP if revcomp else 0,
                 table, ctypes.c_void_p(out.data_ptr()), out.numel())
    return out[:m]


def six_frames_dev(bits, length, table=None):
    """Device tier of six_frames_hip: six uint8 CUDA tensors in the order +0, +1, +2, -0, -1, -2."""
    return [translate_dev(bits, length, start, sub_len, rev, table) for start, sub_len, rev in _six_frames(length)]


def orfs_work_bytes(length):
    """bytes of device scratch cnt_orfs_dev needs for a sequence of this length (0 below 3 nucleotides)"""
    return _work_bytes(lib().cnt_orfs_work_bytes, length)


def orfs_dev(bits, length, stops=CNT_ORF_STOPS_STANDARD, starts=CNT_ORF_STARTS_ATG, min_len=0, both_strands=False, info=True, pos=None, lens=None,
             work=None, count=None):
    """Device tier of orfs_hip, enqueued on torch's current stream without a synchronisation: returns (pos, length, info,
    count), int64 CUDA tensors, count a 1-element tensor that the call SETS to n; the [:n] views are the result once the stream
    has run.  `info` is True (a fresh tensor), False (none is written, None is returned) or the int64 tensor to write, at least
    as long as `pos`; a given `lens` is at least as long as `pos` too.  Without `pos` the outputs hold the most n can be (one
    entry per nucleotide and strand); a given one of any capacity receives the first min(n, capacity) entries.  `work` (>=
    orfs_work_bytes bytes, any contents) and `count` may be reused across calls, e.g. in a captured graph."""
    stops, starts, min_len = _orf_args(stops, starts, min_len)
    torch = _packed_dev(bits, length)
    most = (2 * length if both_strands else length) if length >= 3 else 0
    pos, (lens, inf), count, ptrs = _counted_dev(torch, bits, most, pos, [lens, _info_arg(info)], count, work, orfs_work_bytes(length))
    _enqueue(bits, lib().cnt_orfs_dev, ctypes.c_void_p(bits.data_ptr()), length, stops, starts, min_len, CNT_ORF_BOTH_STRANDS if both_strands else 0, *ptrs)
    return pos, lens, inf, count


def hpc_work_bytes(length):
    """bytes of device scratch cnt_hpc_dev needs for a sequence of this length (0 without a nucleotide)"""
    return _work_bytes(lib().cnt_hpc_work_bytes, length)


def hpc_dev(bits, length, out, count, work, pos=None, out_cap=None):
    """Device tier of hpc_hip, enqueued on torch's current stream without a synchronisation; returns nothing.  All tensors are
    the caller's, contiguous and on the input's device: `out` (int64) receives the run bases packed, `pos` (int64, optional) the
    run starts, `count` (int64, one element) is SET to the number of runs n, `work` holds >= hpc_work_bytes(length) bytes of any
    contents.  `out_cap` (runs; default: what `out`, and `pos` when given, can hold, at most length) bounds what is written: the
    first min(n, out_cap) runs, inside words_for(min(length, out_cap)) words of `out`.  Every tensor may be reused across calls,
    e.g. in a captured graph."""
    torch = _packed_dev(bits, length)
    for name, t, dtype in (("out", out, torch.int64), ("pos", pos, torch.int64), ("count", count, torch.int64), ("work", work, None)):
        if t is None and name == "pos":
            continue
        if not hasattr(t, "is_cuda") or (dtype is not None and t.dtype != dtype):
            raise TypeError("%s must be a%s tensor" % (name, "n int64" if dtype is not None else ""))
        if not t.is_cuda or not t.is_contiguous() or t.device != bits.device:
            raise ValueError("%s must be a contiguous CUDA tensor on the input's device" % name)
    if count.numel() < 1:
        raise ValueError("count must hold one element")
    need = hpc_work_bytes(length)
    if work.numel() * work.element_size() < need:
        raise ValueError("work must hold >= %d bytes" % need)
    fits = min(length, out.numel() * 32, pos.numel() if pos is not None else length)
    if out_cap is None:
        out_cap = fits
    out_cap = int(out_cap)
    if out_cap < 0 or min(length, out_cap) > fits:
        raise ValueError("out_cap runs do not fit the outputs")
    # an empty tensor has no address (data_ptr() 0); at capacity 0 nothing is written, any aligned address will do
    _enqueue(bits, lib().cnt_hpc_dev, ctypes.c_void_p(bits.data_ptr()), length, 0, ctypes.c_void_p(out.data_ptr() or count.data_ptr()),
             ctypes.c_void_p(pos.data_ptr() or count.data_ptr()) if pos is not None else None, out_cap, ctypes.c_void_p(count.data_ptr()),
             ctypes.c_void_p(work.data_ptr() or count.data_ptr()), work.numel() * work.element_size())


def fasta_to_bits_work_bytes(text_len):
    """bytes of device scratch cnt_fasta_to_bits_dev needs for a text of this many bytes (0 without a byte)"""
    return _work_bytes(lib().cnt_fasta_to_bits_work_bytes, text_len)


def fasta_to_bits_dev(text, out, counts, work, rec_text=None, rec_start=None, out_cap=None, rec_cap=None, strict_lut=False, allow_n=False):
    """Device tier of fasta_to_bits_hip, enqueued on torch's current stream without a synchronisation; returns nothing.  All
    tensors are the caller's, contiguous and on the text's device: `text` (uint8, at any byte address) the FASTA bytes, `out`
    (int64) receives the kept nucleotides packed, `rec_text` and `rec_start` (int64, both or neither) the record table, `counts`
    (int64, three elements) is SET to n, the number of header lines and the invalid count, `work` holds >=
    fasta_to_bits_work_bytes(text.numel()) bytes of any contents.  `out_cap` (nucleotides) and `rec_cap` (records) default to what
    the outputs can hold and bound what is written.  Every tensor may be reused across calls, e.g. in a captured graph."""
    torch = _dev_guard(text)
    if text.dtype != torch.uint8:
        raise TypeError("text must be a uint8 tensor")
    if (rec_text is None) != (rec_start is None):
        raise ValueError("rec_text and rec_start go together")
    for name, t, dtype in (("out", out, torch.int64), ("rec_text", rec_text, torch.int64), ("rec_start", rec_start, torch.int64),
                           ("counts", counts, torch.int64), ("work", work, None)):
        if t is None and name.startswith("rec_"):
            continue
        if not hasattr(t, "is_cuda") or (dtype is not None and t.dtype != dtype):
            raise TypeError("%s must be a%s tensor" % (name, "n int64" if dtype is not None else ""))
        if not t.is_cuda or not t.is_contiguous() or t.device != text.device:
            raise ValueError("%s must be a contiguous CUDA tensor on the text's device" % name)
    if counts.numel() < 3:
        raise ValueError("counts must hold three elements")
    length = text.numel()
    need = fasta_to_bits_work_bytes(length)
    if work.numel() * work.element_size() < need:
        raise ValueError("work must hold >= %d bytes" % need)
    fits = min(length, out.numel() * 32)
    out_cap = fits if out_cap is None else int(out_cap)
    if out_cap < 0 or min(length, out_cap) > fits:
        raise ValueError("out_cap nucleotides do not fit out")
    rec_fits = min(length, rec_text.numel(), rec_start.numel()) if rec_text is not None else 0
    rec_cap = rec_fits if rec_cap is None else int(rec_cap)
    if rec_cap < 0 or (rec_text is not None and min(length, rec_cap) > rec_fits):
        raise ValueError("rec_cap records do not fit the record arrays")
    spare = counts.data_ptr()  # an empty tensor has no address (data_ptr() 0); at capacity 0 nothing is written, any aligned address will do
    flags = (_lib.CNT_STRICT_LUT if strict_lut else 0) | (CNT_ALLOW_N if allow_n else 0)
    _enqueue(text, lib().cnt_fasta_to_bits_dev, ctypes.c_void_p(text.data_ptr()), length, flags, ctypes.c_void_p(out.data_ptr() or spare), out_cap,
             ctypes.c_void_p(rec_text.data_ptr() or spare) if rec_text is not None else None,
             ctypes.c_void_p(rec_start.data_ptr() or spare) if rec_text is not None else None, rec_cap, ctypes.c_void_p(counts.data_ptr()),
             ctypes.c_void_p(work.data_ptr() or spare), work.numel() * work.element_size())


def fastq_to_bits_work_bytes(text_len):
    """bytes of device scratch cnt_fastq_to_bits_dev needs for a text of this many bytes (0 without a byte)"""
    return _work_bytes(lib().cnt_fastq_to_bits_work_bytes, text_len)


def fastq_to_bits_dev(text, out, counts, work, qual=None, rec_text=None, rec_start=None, rec_qual=None, out_cap=None, qual_cap=None, rec_cap=None,
                      strict_lut=False, allow_n=False):
    """Device tier of fastq_to_bits_hip, enqueued on torch's current stream without a synchronisation; returns nothing.  All
    tensors are the caller's, contiguous and on the text's device: `text` (uint8, at any byte address) the FASTQ bytes, `out`
    (int64) receives the nucleotides packed, `qual` (uint8, at any byte address, optional) the quality bytes, `rec_text`,
    `rec_start` and `rec_qual` (int64, all three or none) the record table, `counts` (int64, five elements) is SET to n, the number
    of records, the invalid count, the number of quality bytes and the malformed count, `work` holds >=
    fastq_to_bits_work_bytes(text.numel()) bytes of any contents.  `out_cap` (nucleotides), `qual_cap` (bytes) and `rec_cap`
    (records) default to what the outputs can hold and bound what is written.  Every tensor may be reused across calls, e.g. in a
    captured graph."""
    torch = _dev_guard(text)
    if text.dtype != torch.uint8:
        raise TypeError("text must be a uint8 tensor")
    recs = (rec_text, rec_start, rec_qual)
    if any(r is None for r in recs) != all(r is None for r in recs):
        raise ValueError("rec_text, rec_start and rec_qual go together")
    for name, t, dtype in (("out", out, torch.int64), ("qual", qual, torch.uint8), ("rec_text", rec_text, torch.int64), ("rec_start", rec_start, torch.int64),
                           ("rec_qual", rec_qual, torch.int64), ("counts", counts, torch.int64), ("work", work, None)):
        if t is None and (name.startswith("rec_") or name == "qual"):
            continue
        if not hasattr(t, "is_cuda") or (dtype is not None and t.dtype != dtype):
            raise TypeError("%s must be a%s tensor" % (name, (" uint8" if dtype == torch.uint8 else "n int64") if dtype is not None else ""))
        if not t.is_cuda or not t.is_contiguous() or t.device != text.device:
            raise ValueError("%s must be a contiguous CUDA tensor on the text's device" % name)
    if counts.numel() < 5:
        raise ValueError("counts must hold five elements")
    length = text.numel()
    need = fastq_to_bits_work_bytes(length)
    if work.numel() * work.element_size() < need:
        raise ValueError("work must hold >= %d bytes" % need)
    fits = min(length, out.numel() * 32)
    out_cap = fits if out_cap is None else int(out_cap)
    if out_cap < 0 or min(length, out_cap) > fits:
        raise ValueError("out_cap nucleotides do not fit out")
    qual_fits = min(length, qual.numel()) if qual is not None else 0
    qual_cap = qual_fits if qual_cap is None else int(qual_cap)
    if qual_cap < 0 or (qual is not None and min(length, qual_cap) > qual_fits):
        raise ValueError("qual_cap bytes do not fit qual")
    rec_fits = min(length, *(r.numel() for r in recs)) if rec_text is not None else 0
    rec_cap = rec_fits if rec_cap is None else int(rec_cap)
    if rec_cap < 0 or (rec_text is not None and min(length, rec_cap) > rec_fits):
        raise ValueError("rec_cap records do not fit the record arrays")
    spare = counts.data_ptr()  # an empty tensor has no address (data_ptr() 0); at capacity 0 nothing is written, any aligned address will do
    flags = (_lib.CNT_STRICT_LUT if strict_lut else 0) | (CNT_ALLOW_N if allow_n else 0)
    at = lambda t: ctypes.c_void_p(t.data_ptr() or spare) if t is not None else None  # noqa: E731
    _enqueue(text, lib().cnt_fastq_to_bits_dev, ctypes.c_void_p(text.data_ptr()), length, flags, at(out), out_cap, at(qual), qual_cap, at(rec_text), at(rec_start),
             at(rec_qual), rec_cap, ctypes.c_void_p(counts.data_ptr()), at(work), work.numel() * work.element_size())


def bits_to_fasta_work_bytes(n_rec):
    """bytes of device scratch cnt_bits_to_fasta_dev needs for this many records: it depends on nothing else"""
    return _work_bytes(lib().cnt_bits_to_fasta_work_bytes, n_rec)


def bits_to_fasta_dev(bits, length, text, counts, work, rec_start=None, names=None, name_off=None, width=60, rec_text=None, text_cap=None):
    """Device tier of bits_to_fasta_hip, enqueued on torch's current stream without a synchronisation; returns nothing.  All
    tensors are the caller's, contiguous and on the input's device: `bits` (int64) the packed words, `rec_start` (int64, optional)
    the first base of every record, `names` (uint8, at any byte address) and `name_off` (int64, one entry more than rec_start; both
    or neither) the names back to back and where each begins, `text` (uint8, at any byte address) receives the text, `rec_text`
    (int64, optional, as long as rec_start) the byte offset of every '>', `counts` (int64, two elements) is SET to the bytes of
    text and the malformed count, `work` holds >= bits_to_fasta_work_bytes(records) bytes of any contents.  `text_cap` (bytes)
    defaults to what `text` holds and bounds what is written: min(bits_to_fasta_bound(...), text_cap) bytes at the most.  Every
    tensor may be reused across calls, e.g. in a captured graph."""
    torch = _packed_dev(bits, length)
    if (names is None) != (name_off is None):
        raise ValueError("names and name_off go together")
    for name, t, dtype in (("rec_start", rec_start, torch.int64), ("names", names, torch.uint8), ("name_off", name_off, torch.int64), ("text", text, torch.uint8),
                           ("rec_text", rec_text, torch.int64), ("counts", counts, torch.int64), ("work", work, None)):
        if t is None and name in ("rec_start", "names", "name_off", "rec_text"):
            continue
        if not hasattr(t, "is_cuda") or (dtype is not None and t.dtype != dtype):
            raise TypeError("%s must be a%s tensor" % (name, (" uint8" if dtype == torch.uint8 else "n int64") if dtype is not None else ""))
        if not t.is_cuda or not t.is_contiguous() or t.device != bits.device:
            raise ValueError("%s must be a contiguous CUDA tensor on the input's device" % name)
    if counts.numel() < 2:
        raise ValueError("counts must hold two elements")
    n_rec = rec_start.numel() if rec_start is not None else 0
    if name_off is not None and name_off.numel() != n_rec + 1:
        raise ValueError("name_off must hold one entry more than rec_start")
    if rec_text is not None and rec_text.numel() < n_rec:
        raise ValueError("rec_text must hold one entry per record")
    need = bits_to_fasta_work_bytes(n_rec)
    if work.numel() * work.element_size() < need:
        raise ValueError("work must hold >= %d bytes" % need)
    names_len = names.numel() if names is not None else 0
    width = int(width)
    if width < 0:
        raise ValueError("width must not be negative")
    bound = bits_to_fasta_bound(length, n_rec, names_len, width)
    text_cap = text.numel() if text_cap is None else int(text_cap)
    if text_cap < 0 or min(bound, text_cap) > text.numel():
        raise ValueError("text_cap bytes do not fit text")
    spare = counts.data_ptr()  # an empty tensor has no address (data_ptr() 0); nothing of it is read or written, any aligned address will do
    at = lambda t: ctypes.c_void_p(t.data_ptr() or spare) if t is not None else None  # noqa: E731
    _enqueue(bits, lib().cnt_bits_to_fasta_dev, at(bits) if length else None, length, at(rec_start) if n_rec else None, n_rec, at(names), names_len, at(name_off),
             width, 0, at(text), text_cap, at(rec_text), ctypes.c_void_p(counts.data_ptr()), at(work), work.numel() * work.element_size())


def bits_to_fastq_work_bytes(n_rec):
    """bytes of device scratch cnt_bits_to_fastq_dev needs for this many records: it depends on nothing else"""
    return _work_bytes(lib().cnt_bits_to_fastq_work_bytes, n_rec)


def bits_to_fastq_dev(bits, length, qual, rec_start, text, counts, work, names=None, name_off=None, rec_text=None, text_cap=None):
    """Device tier of bits_to_fastq_hip, enqueued on torch's current stream without a synchronisation; returns nothing.  All
    tensors are the caller's, contiguous and on the input's device: `bits` (int64) the packed words, `qual` (uint8, at any byte
    address, at least `length` bytes) the quality bytes, `rec_start` (int64) the first base of every record, `names` (uint8, at any
    byte address) and `name_off` (int64, one entry more than rec_start; both or neither) the names back to back and where each
    begins, `text` (uint8, at any byte address) receives the text, `rec_text` (int64, optional, as long as rec_start) the byte
    offset of every '@', `counts` (int64, two elements) is SET to the bytes of text and the malformed count, `work` holds >=
    bits_to_fastq_work_bytes(records) bytes of any contents.  `text_cap` (bytes) defaults to what `text` holds and bounds what is
    written: min(bits_to_fastq_bound(...), text_cap) bytes at the most.  Every tensor may be reused across calls, e.g. in a
    captured graph."""
    torch = _packed_dev(bits, length)
    if (names is None) != (name_off is None):
        raise ValueError("names and name_off go together")
    for name, t, dtype in (("qual", qual, torch.uint8), ("rec_start", rec_start, torch.int64), ("names", names, torch.uint8), ("name_off", name_off, torch.int64),
                           ("text", text, torch.uint8), ("rec_text", rec_text, torch.int64), ("counts", counts, torch.int64), ("work", work, None)):
        if t is None and name in ("names", "name_off", "rec_text"):
            continue
        if not hasattr(t, "is_cuda") or (dtype is not None and t.dtype != dtype):
            raise TypeError("%s must be a%s tensor" % (name, (" uint8" if dtype == torch.uint8 else "n int64") if dtype is not None else ""))
        if not t.is_cuda or not t.is_contiguous() or t.device != bits.device:
            raise ValueError("%s must be a contiguous CUDA tensor on the input's device" % name)
    if counts.numel() < 2:
        raise ValueError("counts must hold two elements")
    if qual.numel() < length:
        raise ValueError("qual must hold one byte per nucleotide")
    n_rec = rec_start.numel()
    if name_off is not None and name_off.numel() != n_rec + 1:
        raise ValueError("name_off must hold one entry more than rec_start")
    if rec_text is not None and rec_text.numel() < n_rec:
        raise ValueError("rec_text must hold one entry per record")
    need = bits_to_fastq_work_bytes(n_rec)
    if work.numel() * work.element_size() < need:
        raise ValueError("work must hold >= %d bytes" % need)
    names_len = names.numel() if names is not None else 0
    bound = bits_to_fastq_bound(length, n_rec, names_len)
    text_cap = text.numel() if text_cap is None else int(text_cap)
    if text_cap < 0 or min(bound, text_cap) > text.numel():
        raise ValueError("text_cap bytes do not fit text")
    spare = counts.data_ptr()  # an empty tensor has no address (data_ptr() 0); nothing of it is read or written, any aligned address will do
    at = lambda t: ctypes.c_void_p(t.data_ptr() or spare) if t is not None else None  # noqa: E731
    _enqueue(bits, lib().cnt_bits_to_fastq_dev, at(bits) if length else None, length, at(qual) if length else None, at(rec_start) if n_rec else None, n_rec,
             at(names), names_len, at(name_off), 0, at(text), text_cap, at(rec_text), ctypes.c_void_p(counts.data_ptr()), at(work), work.numel() * work.element_size())


def validate_dev(n, allow_n=False, acc=None):
    torch = _dev_guard(n)
    if n.dtype != torch.uint8:
        raise TypeError("nucleotides must be a uint8 tensor")
    acc = _counter(torch, acc, n)
    _enqueue(n, lib().cnt_validate_dev, ctypes.c_void_p(n.data_ptr()), n.numel(), CNT_ALLOW_N if allow_n else 0, ctypes.c_void_p(acc.data_ptr()))
    return acc
