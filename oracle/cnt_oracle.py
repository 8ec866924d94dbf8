"""ctypes loader for oracle/libcnt_oracle.so -- TEST INFRASTRUCTURE ONLY.

Importable only from tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg (see oracle/cnt_oracle.h).  The product package
(cute_nucleotides_amd) never imports this module.

Also holds `np_*` numpy restatements of the two scalar 2-bit functions (same
reference lines) used as a third, independent opinion in tests/test_oracle.py.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libcnt_oracle.so")

ELEN_MESSAGE = "The length is greater than the number of nucleotides!"  # n_to_bits.rs:53


def build(force=False):
    """Compile oracle/libcnt_oracle.so with gcc (seconds)."""
    srcs = [os.path.join(_HERE, f) for f in ("cnt_oracle.c", "cnt_simd_port.c", "cnt_oracle.h")]
    if (not force) and os.path.exists(_LIB_PATH) and all(
        os.path.getmtime(_LIB_PATH) >= os.path.getmtime(s) for s in srcs
    ):
        return _LIB_PATH
    subprocess.check_call(["make", "-C", _HERE, "-B", "libcnt_oracle.so"], stdout=subprocess.DEVNULL)
    return _LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            build()
        L = ctypes.CDLL(_LIB_PATH)
        u8p, u64p, sz = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t
        for name in (
            "cnt_oracle_n_to_bits_lut",
            "cnt_oracle_n_to_bits_bitextract",
            "cnt_oracle_n_to_bits2_lut",
            "cnt_port_n_to_bits_pext",
            "cnt_port_n_to_bits_shift",
            "cnt_port_n_to_bits_movemask",
            "cnt_port_n_to_bits_mul",
            "cnt_port_n_to_bits2_pext",
        ):
            f = getattr(L, name)
            f.argtypes = [u8p, sz, u64p, sz]
            f.restype = ctypes.c_int
        for name in (
            "cnt_oracle_bits_to_n_lut",
            "cnt_oracle_bits_to_n2_lut",
            "cnt_port_bits_to_n_shuffle",
            "cnt_port_bits_to_n_pdep",
            "cnt_port_bits_to_n_clmul",
            "cnt_port_bits_to_n2_pdep",
        ):
            f = getattr(L, name)
            f.argtypes = [u64p, sz, sz, u8p]
            f.restype = ctypes.c_int
        L.cnt_oracle_words_for.argtypes = [sz]
        L.cnt_oracle_words_for.restype = sz
        L.cnt_oracle_words2_for.argtypes = [sz]
        L.cnt_oracle_words2_for.restype = sz
        L.cnt_port_cpu_ok.restype = ctypes.c_int
        L.cnt_oracle_hamming.argtypes = [u64p, u64p, sz]
        L.cnt_oracle_hamming.restype = ctypes.c_uint64
        L.cnt_oracle_complement.argtypes = [u64p, sz, u64p]
        L.cnt_oracle_complement.restype = None
        L.cnt_oracle_reverse_complement.argtypes = [u64p, sz, u64p]
        L.cnt_oracle_reverse_complement.restype = None
        L.cnt_oracle_validate.argtypes = [u8p, sz, ctypes.c_int]
        L.cnt_oracle_validate.restype = ctypes.c_uint64
        L.cnt_oracle_kmers.argtypes = [u64p, sz, ctypes.c_uint, ctypes.c_uint, u64p]
        L.cnt_oracle_kmers.restype = ctypes.c_int
        L.cnt_port_time_alloc_inclusive.argtypes = [ctypes.c_int, ctypes.c_void_p, sz, ctypes.c_int]
        L.cnt_port_time_alloc_inclusive.restype = ctypes.c_double
        L.cnt_oracle_fill_random_acgt.argtypes = [u8p, sz, sz, ctypes.c_uint64]
        L.cnt_oracle_fill_random_acgt.restype = None
        L.cnt_oracle_fill_random_acgtn.argtypes = [u8p, sz, sz, ctypes.c_uint64]
        L.cnt_oracle_fill_random_acgtn.restype = None
        L.cnt_oracle_checksum_words.argtypes = [u64p, sz, sz]
        L.cnt_oracle_checksum_words.restype = ctypes.c_uint64
        _lib = L
    return _lib


def _as_u8(n):
    if isinstance(n, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(n), dtype=np.uint8)
    a = np.ascontiguousarray(n, dtype=np.uint8)
    return a


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a.size else ctypes.c_void_p(0)


def _check(rc):
    if rc == 1:
        raise ValueError(ELEN_MESSAGE)
    if rc != 0:
        raise RuntimeError("oracle error %d" % rc)


def _encode(fname, n, five=False):
    n = _as_u8(n)
    L = lib()
    words = (L.cnt_oracle_words2_for if five else L.cnt_oracle_words_for)(n.size)
    out = np.empty(words, dtype=np.uint64)
    _check(getattr(L, fname)(_ptr(n), n.size, _ptr(out), words))
    return out


def _aligned_u8(nbytes, align=32):
    raw = np.empty(nbytes + align, dtype=np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off : off + nbytes]


def _decode(fname, bits, length, cap_bytes):
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    out = _aligned_u8(max(cap_bytes, 1))
    _check(getattr(lib(), fname)(_ptr(bits), bits.size, length, _ptr(out)))
    return out[:length].copy()


# ---- the parity oracle (scalar) -------------------------------------------------
def n_to_bits_lut(n):
    return _encode("cnt_oracle_n_to_bits_lut", n)


def bits_to_n_lut(bits, length):
    return _decode("cnt_oracle_bits_to_n_lut", bits, length, length)


def n_to_bits_bitextract(n):
    return _encode("cnt_oracle_n_to_bits_bitextract", n)


def n_to_bits2_lut(n):
    return _encode("cnt_oracle_n_to_bits2_lut", n, five=True)


def bits_to_n2_lut(bits, length):
    return _decode("cnt_oracle_bits_to_n2_lut", bits, length, length)


# ---- SIMD ports -------------------------------------------------------------------
def port_cpu_ok():
    return bool(lib().cnt_port_cpu_ok())


def n_to_bits_pext(n):
    return _encode("cnt_port_n_to_bits_pext", n)


def n_to_bits_shift(n):
    return _encode("cnt_port_n_to_bits_shift", n)


def n_to_bits_movemask(n):
    return _encode("cnt_port_n_to_bits_movemask", n)


def n_to_bits_mul(n):
    return _encode("cnt_port_n_to_bits_mul", n)


def n_to_bits2_pext(n):
    return _encode("cnt_port_n_to_bits2_pext", n, five=True)


def bits_to_n_shuffle(bits, length):
    return _decode("cnt_port_bits_to_n_shuffle", bits, length, len(bits) * 32)


def bits_to_n_pdep(bits, length):
    return _decode("cnt_port_bits_to_n_pdep", bits, length, len(bits) * 32)


def bits_to_n_clmul(bits, length):
    return _decode("cnt_port_bits_to_n_clmul", bits, length, len(bits) * 32)


def bits_to_n2_pdep(bits, length):
    return _decode("cnt_port_bits_to_n2_pdep", bits, length, len(bits) * 27 + 5)


# ---- packed-domain operations (not in the reference; parity unpinned) --------------------
def hamming(a, b, length):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    return int(lib().cnt_oracle_hamming(_ptr(a), _ptr(b), length))


def complement(bits, length):
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    out = np.empty((length + 31) // 32, dtype=np.uint64)
    lib().cnt_oracle_complement(_ptr(bits), length, _ptr(out))
    return out


def reverse_complement(bits, length):
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    out = np.empty((length + 31) // 32, dtype=np.uint64)
    lib().cnt_oracle_reverse_complement(_ptr(bits), length, _ptr(out))
    return out


def validate(n, allow_n=False):
    n = _as_u8(n)
    return int(lib().cnt_oracle_validate(_ptr(n), n.size, 1 if allow_n else 0))


KMER_CANONICAL = 0x10  # == CNT_KMER_CANONICAL


def kmers(bits, length, k, canonical=False):
    """the length-k+1 k-mers of the first `length` codes of `bits` (np.uint64; none when length < k), forward or canonical:
    the scalar definition, rolled one code at a time (cnt_oracle_kmers)"""
    if not 1 <= k <= 32:
        raise ValueError("k must be in 1..32")
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    if length > bits.size * 32:
        raise ValueError(ELEN_MESSAGE)
    out = np.empty(max(length - k + 1, 0), dtype=np.uint64)
    if out.size:
        _check(lib().cnt_oracle_kmers(_ptr(bits), length, k, KMER_CANONICAL if canonical else 0, _ptr(out)))
    return out


# ---- generator + checksum ---------------------------------------------------------
def fill_random_acgt(n_len, seed, first_nt=0):
    out = np.empty(n_len, dtype=np.uint8)
    lib().cnt_oracle_fill_random_acgt(_ptr(out), first_nt, n_len, seed & 0xFFFFFFFFFFFFFFFF)
    return out


def fill_random_acgtn(n_len, seed, first_nt=0):
    out = np.empty(n_len, dtype=np.uint8)
    lib().cnt_oracle_fill_random_acgtn(_ptr(out), first_nt, n_len, seed & 0xFFFFFFFFFFFFFFFF)
    return out


def checksum_words(words, first_word=0):
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return int(lib().cnt_oracle_checksum_words(_ptr(w), first_word, w.size))


# ---- numpy restatement (independent third opinion; small inputs) ------------------
_NP_BYTE_LUT = np.zeros(256, dtype=np.uint64)
for _c, _v in ((b"aA", 0), (b"cC", 1), (b"tTuU", 2), (b"gG", 3)):  # n_to_bits.rs:8-21
    for _b in _c:
        _NP_BYTE_LUT[_b] = _v
_NP_BITS_LUT = np.frombuffer(b"ACTG", dtype=np.uint8)  # n_to_bits.rs:23-30


def np_n_to_bits_lut(n):
    """n_to_bits.rs:34-47 in numpy: OR of code << 2*(i&31) into word i>>5."""
    n = _as_u8(n)
    words = (n.size + 31) // 32
    codes = np.zeros(words * 32, dtype=np.uint64)
    codes[: n.size] = _NP_BYTE_LUT[n]
    shifts = (np.arange(32, dtype=np.uint64) * np.uint64(2))[None, :]
    return np.bitwise_or.reduce(codes.reshape(words, 32) << shifts, axis=1) if words else np.empty(0, np.uint64)


def np_bits_to_n_lut(bits, length):
    """n_to_bits.rs:51-69 in numpy."""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    if length > bits.size * 32:
        raise ValueError(ELEN_MESSAGE)
    i = np.arange(length, dtype=np.uint64)
    codes = (bits[(i >> np.uint64(5)).astype(np.int64)] >> ((i & np.uint64(31)) << np.uint64(1))) & np.uint64(3)
    return _NP_BITS_LUT[codes.astype(np.int64)]


# ---- whole-stream expected values (large-size checks) ------------------------------
# The oracle's answer for a whole seeded stream of any length, computed chunk by chunk on a thread pool (the ctypes calls
# release the GIL), so that a device output of 2^36 nt can be compared in full through one position-salted checksum.
# Every function regenerates the stream the device generator writes into a buffer filled with `first_nt`:
# fill_random_acgt for "encode" / "complement" / "reverse_complement" / hamming / validate, fill_random_acgtn for
# "encode5".  `plants` are (index into that buffer, byte) pairs written into the regenerated ASCII before it is
# encoded or validated, as a test writes them on the device (an array of shape (k, 2) is accepted too).
STREAM_KINDS = ("encode", "encode5", "complement", "reverse_complement")
STREAM_CHUNK_NT = 16 << 20  # 16 Mi nt: a few GiB of host memory at 64 workers


def _workers(workers):
    return workers or min(os.cpu_count() or 1, 64)


def _plants(plants):
    p = np.asarray(plants, dtype=np.int64).reshape(-1, 2)
    order = np.argsort(p[:, 0], kind="stable")  # a later plant at the same position wins, as a later device write would
    return p[order, 0].copy(), p[order, 1].astype(np.uint8)


def _stream_ascii(five, seed, first_nt, lo, m, plants):
    """bytes [lo, lo + m) of the buffer filled with (seed, first_nt), plants applied; any lo, generated from the word
    boundary at or below first_nt + lo (the generators are only regenerable there) and sliced"""
    g = first_nt + lo
    g0 = g - g % 27 if five else g & ~31
    n = (fill_random_acgtn if five else fill_random_acgt)(m + g - g0, seed, first_nt=g0)[g - g0 :]
    pos, byt = plants
    i, j = np.searchsorted(pos, lo), np.searchsorted(pos, lo + m)
    if j > i:
        n[pos[i:j] - lo] = byt[i:j]
    return n


def _chunks(n_len, chunk_nt, grain):
    k = chunk_nt or STREAM_CHUNK_NT
    k -= k % grain
    if k <= 0:
        raise ValueError("chunk_nt must hold at least one output word (%d nt)" % grain)
    return [(lo, min(k, n_len - lo)) for lo in range(0, n_len, k)]


def _run(fn, chunks, workers):
    from concurrent.futures import ThreadPoolExecutor

    lib()  # load once, before the workers
    with ThreadPoolExecutor(max_workers=_workers(workers)) as ex:
        return list(ex.map(lambda c: fn(*c), chunks))


def stream_checksum(kind, seed, n_len, first_nt=0, plants=(), per_chunk=False, chunk_nt=None, workers=None):
    """checksum_words of the oracle's output words for the stream of n_len nt at `first_nt`, salted with the GLOBAL word
    index (first word = first_nt / 32, or / 27 for "encode5"): the value devutil.checksum_words(out, first_word=...) has
    to give.  "complement" / "reverse_complement" are of n_to_bits_lut of the stream, length n_len.  per_chunk=True
    returns the list of per-chunk checksums instead (chunks of `chunk_nt`, rounded down to whole output words)."""
    if kind not in STREAM_KINDS:
        raise ValueError("kind must be one of %s" % (STREAM_KINDS,))
    five = kind == "encode5"
    grain = 27 if five else 32
    if first_nt % grain:
        raise ValueError("first_nt must start an output word (a multiple of %d)" % grain)
    w0 = first_nt // grain
    pl = _plants(plants)

    def chunk(lo, m):
        if kind == "reverse_complement":
            # output nt [lo, lo + m) are the complements of input nt [n_len - lo - m, n_len - lo), reversed: the prefix of
            # the reverse complement of the input from the word boundary at or below n_len - lo - m up to n_len - lo
            a = n_len - lo - m
            a0 = a & ~31
            x = n_to_bits_lut(_stream_ascii(False, seed, first_nt, a0, n_len - lo - a0, pl))
            out = reverse_complement(x, n_len - lo - a0)[: (m + 31) // 32]
        else:
            x = (n_to_bits2_lut if five else n_to_bits_lut)(_stream_ascii(five, seed, first_nt, lo, m, pl))
            out = complement(x, m) if kind == "complement" else x
        return checksum_words(out, first_word=w0 + lo // grain)

    sums = _run(chunk, _chunks(n_len, chunk_nt, grain), workers)
    return sums if per_chunk else sum(sums) % (1 << 64)


def stream_hamming(seed_a, seed_b, n_len, first_nt_a=0, first_nt_b=0, per_chunk=False, chunk_nt=None, workers=None):
    """hamming of n_to_bits_lut of two streams of n_len nt (fill_random_acgt at seed_a / first_nt_a and seed_b /
    first_nt_b, both multiples of 32)"""
    if first_nt_a % 32 or first_nt_b % 32:
        raise ValueError("first_nt_a / first_nt_b must be multiples of 32")
    none = _plants(())

    def chunk(lo, m):
        a = n_to_bits_lut(_stream_ascii(False, seed_a, first_nt_a, lo, m, none))
        b = n_to_bits_lut(_stream_ascii(False, seed_b, first_nt_b, lo, m, none))
        return hamming(a, b, m)

    counts = _run(chunk, _chunks(n_len, chunk_nt, 32), workers)
    return counts if per_chunk else sum(counts)


def stream_validate(seed, n_len, first_nt=0, plants=(), allow_n=False, per_chunk=False, chunk_nt=None, workers=None):
    """validate of the fill_random_acgt stream of n_len nt at first_nt (any nt: the buffer may start inside a word),
    plants applied"""
    pl = _plants(plants)
    counts = _run(lambda lo, m: validate(_stream_ascii(False, seed, first_nt, lo, m, pl), allow_n=allow_n),
                  _chunks(n_len, chunk_nt, 1), workers)
    return counts if per_chunk else sum(counts)


def stream_kmers_checksum(seed, n_len, k, canonical, first_nt=0, per_chunk=False, chunk_nt=None, workers=None):
    """checksum_words of the k-mers (kmers()) of the fill_random_acgt stream of n_len nt at `first_nt` (any nt), salted
    with the k-mer index: the value devutil.checksum_words(out) of the whole k-mer output has to give.  Chunk [lo, lo + m)
    of the k-mers is made from nt [lo, lo + m + k - 1) of the stream.  per_chunk=True returns the list of per-chunk
    checksums instead (chunks of `chunk_nt` k-mers; any chunk size: a k-mer is one output word)."""
    if not 1 <= k <= 32:
        raise ValueError("k must be in 1..32")
    none = _plants(())

    def chunk(lo, m):
        x = n_to_bits_lut(_stream_ascii(False, seed, first_nt, lo, m + k - 1, none))
        return checksum_words(kmers(x, m + k - 1, k, canonical), first_word=lo)

    sums = _run(chunk, _chunks(max(n_len - k + 1, 0), chunk_nt, 1), workers)
    return sums if per_chunk else sum(sums) % (1 << 64)
