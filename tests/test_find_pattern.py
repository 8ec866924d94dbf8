"""Approximate pattern search on packed words (include/cute_nt.h "pattern search"): the windows of k codes within
max_mismatches substitutions of a pattern with wildcard positions, on the forward strand or on both, ordered by position,
forward before reverse.  Not in the reference, so the CPU part pins two references against each other -- the definition as a
literal per-position, per-base loop over the codes read straight from the words, and a vectorised numpy form on
oracle.kmers -- checks the properties the definition implies, pattern_from_ascii, every argument error, the scratch query
and the ISA of the eight kernels.  The GPU part compares both tiers with the numpy reference bit for bit: planted
occurrences and near-misses around every length edge and input phase, capacities and sentinels, the dense extreme, hits
across tile and launch edges on the lab build, a captured graph and a side stream, pinned against staged host buffers, a
fuzz loop, and once past 2^32 positions against a chunked host reference."""
import ctypes
import os
import re
import sys
import time

import numpy as np
import pytest

from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch
from test_kmers import assert_split_launches_by_max_tiles_per_launch
from test_minimizers import assert_counted_output_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNT_FIND_BOTH_STRANDS = 0x20
CNT_FIND_REVERSE = 0x100
TILE = 8192  # windows per workgroup tile (hip/find_kernels.hpp kFindTile)
LETTERS = np.frombuffer(b"ACTG", dtype=np.uint8)  # code order A0 C1 T2 G3
GUIDE = "GATTACAGATTACAGATTACNGG"  # a 20-nt guide + the NGG PAM


# ---- patterns ---------------------------------------------------------------------------------------------------------
def pack_pattern(codes, wild):
    """(pattern, wildcards, k) of a list of codes and a list of wildcard flags; wildcard positions carry code 0"""
    p = sum((0 if w else int(c)) << (2 * j) for j, (c, w) in enumerate(zip(codes, wild)))
    return p, sum(1 << j for j, w in enumerate(wild) if w), len(codes)


def unpack_pattern(pat):
    p, wild, k = pat
    return [(p >> (2 * j)) & 3 for j in range(k)], [bool((wild >> j) & 1) for j in range(k)]


def revcomp_pattern(codes, wild):
    """P'_j = P_{k-1-j} ^ 2, wildcards' bit j = wildcards bit k-1-j"""
    return [c ^ 2 for c in reversed(codes)], list(reversed(wild))


def random_pattern(rng, k, n_wild):
    codes = [int(c) for c in rng.integers(0, 4, k)]
    wild = [False] * k
    for j in rng.choice(k, n_wild, replace=False):
        wild[int(j)] = True
    return codes, wild


# ---- references -------------------------------------------------------------------------------------------------------
def codes_of(words, length):
    """the codes of a packed sequence as a uint8 array, straight from the layout: code i at bits 2 (i & 31) of word i >> 5"""
    w = np.asarray(words, dtype=np.uint64)
    i = np.arange(length, dtype=np.uint64)
    return ((w[(i >> np.uint64(5)).astype(np.int64)] >> (np.uint64(2) * (i & np.uint64(31)))) & np.uint64(3)).astype(np.uint8)


def def_find(words, length, pat, d, both):
    """the definition, literally: for every window and strand, count base by base the compared positions that differ"""
    P, W = unpack_pattern(pat)
    k = len(P)
    s = [int(c) for c in codes_of(words, length)]
    strands = [(0, P, W)] + ([(1,) + tuple(revcomp_pattern(P, W))] if both else [])
    pos, info = [], []
    for i in range(length - k + 1 if length >= k else 0):
        for strand, Q, V in strands:
            dist = 0
            for j in range(k):
                if not V[j] and s[i + j] != Q[j]:
                    dist += 1
            if dist <= d:
                pos.append(i)
                info.append(dist + (CNT_FIND_REVERSE if strand else 0))
    return np.array(pos, dtype=np.uint64), np.array(info, dtype=np.uint64)


def np_dist(x, codes, wild):
    """mismatch counts of the forward k-mers x against (codes, wild): popcount((y | y >> 1) & care) of the XOR"""
    p, w, k = pack_pattern(codes, wild)
    care = sum(1 << (2 * j) for j in range(k) if not (w >> j) & 1)
    y = x ^ np.uint64(p)
    return np.bitwise_count((y | (y >> np.uint64(1))) & np.uint64(care)).astype(np.int64)


def np_find(x, pat, d, both, first=0):
    """the vectorised reference on the forward k-mers x = oracle.kmers(words, length, k) (window `first` + index): (pos, info)"""
    P, W = unpack_pattern(pat)
    x = np.asarray(x, dtype=np.uint64)
    df = np_dist(x, P, W)
    keys, dist = [np.flatnonzero(df <= d) * 2], [df[df <= d]]
    if both:
        dr = np_dist(x, *revcomp_pattern(P, W))
        keys.append(np.flatnonzero(dr <= d) * 2 + 1)
        dist.append(dr[dr <= d] + CNT_FIND_REVERSE)
    keys, dist = np.concatenate(keys), np.concatenate(dist)
    order = np.argsort(keys, kind="stable")
    return (keys[order] // 2 + first).astype(np.uint64), dist[order].astype(np.uint64)


def ref_find(oracle, words, length, pat, d, both):
    k = pat[2]
    if length < k:
        return np.empty(0, dtype=np.uint64), np.empty(0, dtype=np.uint64)
    return np_find(oracle.kmers(np.ascontiguousarray(words), length, k, False), pat, d, both)


def words_of_codes(oracle, codes, extra=0, rng=None):
    """packed words of a code array; with `rng`, garbage above len in the last word and `extra` garbage words behind it"""
    n = len(codes)
    w = oracle.n_to_bits_lut(LETTERS[np.asarray(codes, dtype=np.int64)]) if n else np.zeros(0, dtype=np.uint64)
    w = np.concatenate([w, np.zeros(extra + (1 if n == 0 else 0), dtype=np.uint64)])
    if rng is not None:
        if n & 31:
            w[(n - 1) >> 5] |= np.uint64(int(rng.integers(0, 2**62)) >> (2 * (n & 31)) << (2 * (n & 31)))
        w[(n + 31) >> 5 :] = rng.integers(0, 2**64, w.size - ((n + 31) >> 5), dtype=np.uint64)
    return w


def mutated(rng, codes, wild, e):
    """a copy of the pattern (wildcards filled at random) with exactly e substitutions at compared positions"""
    out = [int(rng.integers(0, 4)) if w else c for c, w in zip(codes, wild)]
    compared = [j for j, w in enumerate(wild) if not w]
    for j in rng.choice(compared, e, replace=False):
        out[int(j)] = (out[int(j)] + int(rng.integers(1, 4))) & 3
    return out


def planted_sequence(rng, n_len, pat, d, both, at=None):
    """random codes with copies of the pattern (and, with `both`, of its reverse complement) planted with 0 .. d+1
    substitutions at compared positions, at disjoint random sites (or at the sites `at`, while they last).  Returns the codes
    and the plants [(site, strand, substitutions)]; a plant with e <= d must be reported, one with e = d+1 is a near-miss."""
    P, W = unpack_pattern(pat)
    k = len(P)
    s = rng.integers(0, 4, n_len).astype(np.uint8)
    compared = k - sum(W)
    wanted = [(strand, e) for e in (0, d + 1, d, 1) for strand in ((0, 1) if both else (0,)) if e <= min(d + 1, compared)]
    slots = n_len // (k + 1)
    sites = list(at) if at is not None else [int(j) * (k + 1) + int(rng.integers(0, 2)) for j in rng.permutation(slots)[: len(wanted)]]
    plants = []
    for site, (strand, e) in zip(sites, wanted):
        Q, V = revcomp_pattern(P, W) if strand else (P, W)
        s[site : site + k] = mutated(rng, Q, V, e)
        plants.append((site, strand, e))
    return s, plants


def assert_plants(want, plants, d, both, need_all):
    """the condition on the REFERENCE, before the library is called: every plant within the bound is an expected hit at its
    distance, every near-miss at d+1 is not an expected hit; with need_all, at least one of each exists per searched strand"""
    got = {(int(p), int(i) >> 8): int(i) & 0xFF for p, i in zip(*want)}
    hits = {0: 0, 1: 0}
    misses = 0
    for site, strand, e in plants:
        if e <= d:
            assert got.get((site, strand), -1) <= e and (site, strand) in got, (site, strand, e)
            hits[strand] += 1
        else:
            # a plant was made with exactly d+1 substitutions at compared positions: its distance IS d+1
            assert (site, strand) not in got, (site, strand, e)
            misses += 1
    if need_all:
        assert hits[0] >= 1 and (not both or hits[1] >= 1) and misses >= 1, (hits, misses)
    return hits, misses


# ---- CPU: the references --------------------------------------------------------------------------------------------------
KS = [1, 2, 7, 15, 16, 17, 23, 31, 32]


@pytest.mark.parametrize("k", KS)
def test_numpy_reference_against_the_definition(oracle, k):
    rng = np.random.default_rng(4200 + k)
    for n_wild in sorted({0, k // 3, k - 1}):
        codes, wild = random_pattern(rng, k, n_wild)
        pat = pack_pattern(codes, wild)
        compared = k - n_wild
        for d in sorted({0, min(1, compared), min(3, compared), k}):
            for n_len in (k - 1, k, k + 1, 3 * k + 40, 700):
                if n_len < 0:
                    continue
                s, plants = planted_sequence(rng, n_len, pat, d, True)
                words = words_of_codes(oracle, s, extra=1, rng=rng)
                for both in (False, True):
                    want = def_find(words, n_len, pat, d, both)
                    got = ref_find(oracle, words, n_len, pat, d, both)
                    tag = (k, n_wild, d, n_len, both)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), tag
                    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64
                    if d < compared:
                        assert_plants(got, [p for p in plants if both or p[1] == 0], d, both, n_len >= 700 and (k > 2 or n_wild == 0))


def test_properties(oracle):
    rng = np.random.default_rng(11)
    comp = np.array([2, 3, 0, 1], dtype=np.uint8)  # code ^ 2
    for k, n_wild, d in ((7, 0, 1), (12, 2, 2), (23, 3, 3), (32, 0, 5), (16, 5, 0)):
        codes, wild = random_pattern(rng, k, n_wild)
        pat = pack_pattern(codes, wild)
        n_len = 3000
        s, _ = planted_sequence(rng, n_len, pat, d, True)
        m = n_len - k + 1
        w, rw = words_of_codes(oracle, s), words_of_codes(oracle, comp[s[::-1]])
        # hit (i, strand, dist) of s <-> hit (m-1-i, other strand, dist) of revcomp(s)
        a, b = ref_find(oracle, w, n_len, pat, d, True), ref_find(oracle, rw, n_len, pat, d, True)
        assert a[0].size >= 4
        sa = sorted((int(p), int(i) >> 8, int(i) & 0xFF) for p, i in zip(*a))
        sb = sorted((m - 1 - int(p), 1 - (int(i) >> 8), int(i) & 0xFF) for p, i in zip(*b))
        assert sa == sb, (k, n_wild, d)
        # the forward-only result is the forward entries of the both-strand result
        f = ref_find(oracle, w, n_len, pat, d, False)
        keep = a[1] < CNT_FIND_REVERSE
        assert np.array_equal(f[0], a[0][keep]) and np.array_equal(f[1], a[1][keep])
        # max_mismatches = k hits every window, on both strands: n = 2m, forward first
        pos, info = ref_find(oracle, w, n_len, pat, k, True)
        assert np.array_equal(pos, np.repeat(np.arange(m, dtype=np.uint64), 2))
        assert ((info[0::2] & CNT_FIND_REVERSE) == 0).all() and ((info[1::2] & CNT_FIND_REVERSE) != 0).all()
        # all positions wildcard: every window at distance 0
        allw = pack_pattern([0] * k, [True] * k)
        pos, info = ref_find(oracle, w, n_len, allw, 0, False)
        assert np.array_equal(pos, np.arange(m, dtype=np.uint64)) and not info.any()
    # a palindromic pattern (its own reverse complement) gives paired entries, forward first, equal distances
    pal = pack_pattern([0, 0, 1, 3, 2, 2], [False] * 6)  # AACGTT
    assert revcomp_pattern(*unpack_pattern(pal)) == unpack_pattern(pal)
    s, _ = planted_sequence(rng, 2000, pal, 1, False)
    pos, info = ref_find(oracle, words_of_codes(oracle, s), 2000, pal, 1, True)
    assert pos.size >= 2 and pos.size % 2 == 0 and np.array_equal(pos[0::2], pos[1::2])
    assert np.array_equal(info[0::2] + CNT_FIND_REVERSE, info[1::2])


# ---- CPU: the Python layer and the ABI ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


def test_pattern_from_ascii(oracle):
    from cute_nucleotides_amd import packed_ops as po

    p, w, k = po.pattern_from_ascii(GUIDE)
    assert k == 23 and w == 1 << 20
    codes, wild = unpack_pattern((p, w, k))
    assert wild == [j == 20 for j in range(23)] and codes[20] == 0
    spelled = "".join("N" if wl else "ACTG"[c] for c, wl in zip(codes, wild))
    assert spelled == GUIDE  # round trip
    # the packing is the codec's: the pattern without wildcards is the first word of its encoding = its own k-mer 0
    s = "ACGTTGCAACGT"
    assert po.pattern_from_ascii(s)[0] == int(oracle.n_to_bits_lut(np.frombuffer(s.encode(), dtype=np.uint8))[0])
    assert po.pattern_from_ascii("acgun") == po.pattern_from_ascii("ACGTN") == po.pattern_from_ascii(b"ACGUN") == (0b0010_1101_00, 1 << 4, 5)
    assert po.pattern_from_ascii("G" * 32) == ((1 << 64) - 1, 0, 32) and po.pattern_from_ascii("N") == (0, 1, 1)
    for bad in ("", "A" * 33, "ACGR", "AC-T", "AC T", "ACGT\n", 5, None):
        with pytest.raises(ValueError):
            po.pattern_from_ascii(bad)


def test_python_wrappers_raise_value_error(L):
    from cute_nucleotides_amd import packed_ops as po

    w = np.zeros(2, dtype=np.uint64)
    for pat, d in (((0, 0, 0), 0), ((0, 0, 33), 0), ((1 << 10, 0, 5), 0), ((0, 1 << 5, 5), 0), (("ACGT"), 5), ("ACGT", -1), ("ACGX", 0)):
        with pytest.raises(ValueError):
            po.find_pattern_hip(w, 64, pat, d)
    with pytest.raises(ValueError):
        po.find_pattern_hip(w, 65, "ACGT")  # longer than the words hold
    pos, info = po.find_pattern_hip(w, 3, "ACGT", 1, both_strands=True)  # m == 0: answered without a device
    assert pos.size == 0 and info.size == 0
    pos, info = po.find_pattern_hip(w, 0, "A", info=False)
    assert pos.size == 0 and info is None
    assert po.find_pattern_work_bytes(3, 4) == 0


def _work_bytes(L, n_len, k):
    out = ctypes.c_size_t(12345)
    assert L.cnt_find_pattern_work_bytes(n_len, k, ctypes.byref(out)) == 0
    return out.value


def test_work_bytes_query(L):
    from cute_nucleotides_amd import _lib
    from cute_nucleotides_amd import packed_ops as po

    assert _work_bytes(L, 0, 1) == 0 and _work_bytes(L, 22, 23) == 0  # m == 0
    assert _work_bytes(L, 23, 23) == 16 + 2 * 8 + 16 * 4  # one window: one group of 16 tiles
    for m in (1, TILE - 1, TILE, TILE + 1, 5 * TILE, 16 * TILE, 16 * TILE + 1, 33 * 16 * TILE, (1 << 32) + 1):
        n_len = m + 23 - 1
        groups = -(-(-(-m // TILE)) // 16)
        want = 16 + (groups + groups % 2) * 8 + groups * 16 * 4  # alignment slack, one u64 offset per group, one u32 count per tile
        assert _work_bytes(L, n_len, 23) == want == po.find_pattern_work_bytes(n_len, 23), m
    for k in (0, 33, 64):
        assert L.cnt_find_pattern_work_bytes(100, k, ctypes.byref(ctypes.c_size_t())) == _lib.CNT_EINVAL
    assert L.cnt_find_pattern_work_bytes(100, 5, None) == _lib.CNT_EINVAL


def test_abi_errors_come_before_any_device_work(L):
    from cute_nucleotides_amd import _lib

    buf = np.zeros(4096, dtype=np.uint64)
    q = lambda word, byte=0: ctypes.c_void_p(buf.ctypes.data + 8 * word + byte)  # noqa: E731
    out = np.full(512, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    o = lambda word, byte=0: ctypes.c_void_p(out.ctypes.data + 8 * word + byte)  # noqa: E731
    cnt = np.full(2, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    c = lambda byte=0: ctypes.c_void_p(cnt.ctypes.data + byte)  # noqa: E731
    work = q(3000)  # 100 nt, k = 23: m = 78, one tile, 96 B of scratch
    P, WILD = 0x155555555555 & ((1 << 46) - 1), 1 << 20
    for dev in (False, True):
        def call(bits, n_len, pattern, k, wild, d, flags, pos, info, cap, count, work_bytes=96):
            if dev:
                return L.cnt_find_pattern_dev(bits, n_len, pattern, k, wild, d, flags, pos, info, cap, count, work, work_bytes, None)
            return L.cnt_find_pattern(bits, n_len, pattern, k, wild, d, flags, pos, info, cap, count)

        tag = "dev" if dev else "host"
        ok = (q(0), 100, P, 23, WILD, 3, 0, o(0), o(200), 64, c())
        # k out of range, pattern bits at or above 2k, wildcard bits at or above k, max_mismatches > k -- even without a window
        for k, pattern, wild, d in ((0, 0, 0, 0), (33, 0, 0, 0), (64, 0, 0, 0), (23, 1 << 46, 0, 0), (23, 1 << 63, 0, 0), (5, 1 << 10, 0, 0),
                                    (23, P, 1 << 23, 0), (23, P, 1 << 31, 0), (1, 0, 2, 0), (23, P, WILD, 24), (1, 0, 0, 2), (32, 0, 0, 33)):
            assert call(q(0), 100, pattern, k, wild, d, 0, o(0), o(200), 64, c()) == _lib.CNT_EINVAL, (tag, k, pattern, wild, d)
            assert call(None, 0, pattern, k, wild, d, 0, None, None, 0, None) == _lib.CNT_EINVAL, (tag, k, pattern, wild, d)
        for flags in (0x1, 0x2, 0x4, 0x8, 0x10, 0x40, 0x100, 0x80000000, CNT_FIND_BOTH_STRANDS | 0x1):
            assert call(q(0), 100, P, 23, WILD, 3, flags, o(0), o(200), 64, c()) == _lib.CNT_EINVAL, (tag, flags)
        # NULL bits, pos or count when m > 0 (info may be NULL)
        assert call(None, *ok[1:]) == _lib.CNT_EINVAL
        assert call(*ok[:7], None, o(200), 64, c()) == _lib.CNT_EINVAL
        assert call(*ok[:10], None) == _lib.CNT_EINVAL
        # not 8-B aligned
        for byte in (1, 4, 7):
            assert call(q(0, byte), *ok[1:]) == _lib.CNT_EINVAL
            assert call(*ok[:7], o(0, byte), o(200), 64, c()) == _lib.CNT_EINVAL
            assert call(*ok[:7], o(0), o(200, byte), 64, c()) == _lib.CNT_EINVAL
            assert call(*ok[:10], c(byte)) == _lib.CNT_EINVAL
        # pos or info overlapping the input words (100 nt = 4 words at q(10)) or each other (64 entries each)
        for ow in (10, 12, 13, 8, 0):
            assert call(q(10), *ok[1:7], q(ow), o(200), 64, c()) == _lib.CNT_EINVAL, (tag, ow)
            assert call(q(10), *ok[1:7], o(200), q(ow), 64, c()) == _lib.CNT_EINVAL, (tag, ow)
        for iw in (0, 63, 30):
            assert call(q(10), *ok[1:7], o(0), o(iw), 64, c()) == _lib.CNT_EINVAL, (tag, iw)
        if dev:
            assert call(q(10), *ok[1:], work_bytes=95) == _lib.CNT_EINVAL  # scratch below the query
            assert call(q(10), *ok[1:], work_bytes=0) == _lib.CNT_EINVAL
        # m == 0: CNT_OK without a device, count set to 0 on the host tier (NULL pointers allowed)
        for n_len, k in ((0, 1), (22, 23), (31, 32)):
            assert call(None, n_len, 0, k, 0, k, CNT_FIND_BOTH_STRANDS, None, None, 0, None) == _lib.CNT_OK
            if not dev:
                cnt[0] = 99
                assert call(q(0), n_len, 0, k, 0, 0, 0, o(0), None, 64, c()) == _lib.CNT_OK and cnt[0] == 0
                cnt[0] = 0x5A5A5A5A5A5A5A5A
    assert (out == 0x5A5A5A5A5A5A5A5A).all()  # nothing was written
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        assert L.cnt_find_pattern(q(0), 100, P, 23, WILD, 3, 0, o(0), o(200), 64, c()) == _lib.CNT_ENODEV
        assert L.cnt_find_pattern_dev(q(0), 100, P, 23, WILD, 3, 0, o(0), None, 64, c(), work, 96, None) < 0
        assert (out == 0x5A5A5A5A5A5A5A5A).all()


def test_abi_wiring(L):
    import subprocess

    from cute_nucleotides_amd import _lib

    names = ("cnt_find_pattern", "cnt_find_pattern_dev", "cnt_find_pattern_work_bytes")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(L, name) and name in exported and name + "(" in header
    assert "#define CNT_FIND_BOTH_STRANDS 0x20u" in header and "#define CNT_FIND_REVERSE 0x100u" in header
    assert (_lib.CNT_FIND_BOTH_STRANDS, _lib.CNT_FIND_REVERSE) == (CNT_FIND_BOTH_STRANDS, CNT_FIND_REVERSE)
    for words in ("SET to n", "forward before reverse", "Cost depends on the data", "CNT_ECAP comes after the work"):
        assert words.lower() in header.split("pattern search, 1 <= k <= 32")[1].split("cnt_find_pattern_work_bytes(size_t")[0].lower(), words
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    for sig in (r"pub fn find_pattern_hip\(bits: &\[u64\], len: usize, p: &Pattern, max_mismatches: u32, both_strands: bool\) -> \(Vec<u64>, Vec<u64>\) \{",
                r"pub fn find_pattern_hip_dev\(", r"pub fn find_pattern_work_bytes\(len: usize, k: u32\) -> usize \{", r"pub fn pattern_from_ascii\("):
        assert re.search(sig, rust), sig


# ---- CPU: the ISA and the launch plan ---------------------------------------------------------------------------------------
FIND_KERNELS = ["find_%s_k%d%s" % (p, w, b) for p in ("count", "write") for w in (16, 32) for b in ("", "_both")]


def test_find_kernels_isa():
    """the eight kernels from the product's gfx950 assembly: no scratch, no spills, no waterfall loop, v_bcnt_u32_b32 does the
    counting (one per compared dword and strand and window), the window funnels are 32-bit v_alignbit_b32, static LDS is the
    few words of the prefix sum (the launcher passes no dynamic LDS), the count pass stores one dword per tile and the
    write pass stores positions with `nt`"""
    sys.path.insert(0, os.path.join(ROOT, "bench"))
    import isa_digest

    asm = isa_digest.assembly()
    for name in FIND_KERNELS:
        m = re.search(r"^cnt::%s\(.*?\): +; @(.*?)\.end_amdhsa_kernel" % name, asm, re.S | re.M)
        assert m, name + " not in the product's assembly"
        text = m.group(1)
        body = [l.strip() for l in text.splitlines() if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        assert "scratch_" not in text and "s_xor_b64 exec, exec" not in text, name
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", text), name
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", text).group(1))
        assert lds <= 64, (name, lds)
        assert int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", text).group(1)) <= 96, name
        meta = re.search(r"\.name:\s+cnt::%s\(.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)" % name, asm, re.S)
        assert meta and meta.group(1) == "0" and meta.group(2) == "0", (name, meta and meta.groups())
        bcnt = sum(1 for i in body if i.startswith("v_bcnt_u32_b32"))
        per_window = (2 if "k32" in name else 1) * (2 if "both" in name else 1)
        assert bcnt >= 32 * per_window, (name, bcnt)
        assert sum(1 for i in body if i.startswith("v_alignbit_b32")) >= 24, name
        stores = [i for i in body if "_store" in i and not i.startswith("ds_")]
        if "count" in name:
            assert len(stores) == 1 and stores[0].startswith("global_store_dword "), (name, stores)
        else:
            assert stores and all(i.startswith("global_store_dwordx2") and " nt" in i for i in stores), (name, stores)
    assert len(isa_digest.kernels(asm)) < 60  # the product's templated kernels: none added


FIND_HW_LAUNCH_TILES = ((0x7FFFFFFF // 256) // 64) * 64  # max_tiles_per_launch(256) of the product build


def find_plan(n_len, k, launch_tiles=FIND_HW_LAUNCH_TILES):
    """(tiles, kernel launches) of a device call: ceil(m / 8192) tiles, counted and written in ceil(tiles / launch_tiles)
    launches each, one scan launch between them; m = 0: no kernel (a memset of the count)"""
    m = n_len - k + 1 if n_len >= k else 0
    tiles = -(-m // TILE)
    return tiles, (2 * -(-tiles // launch_tiles) + 1) if tiles else 0


def test_find_plan_matches_the_launcher_and_splitter_source():
    src = open(os.path.join(ROOT, "hip", "find_kernels.hpp")).read()
    assert "constexpr int kFindBlock = 256;" in src and "kFindTileWords = kFindBlock, kFindTile = 32 * kFindTileWords;" in src
    abi = open(os.path.join(ROOT, "hip", "find_abi.inc")).read()
    scan = "counted_scan_enqueue(work, n_tiles, d_count, s);"
    for line in ("const uint64_t n_tiles = (m + kFindTile - 1) / kFindTile;", "const CountedScratch work = counted_carve(d_work, n_tiles);", scan,
                 "if (m == 0) return counted_empty_dev(d_count, s);"):
        assert line in abi, line
    assert_counted_output_source()
    tiles = "split_launches(n_tiles, kFindBlock, [&](uint64_t t, uint64_t n) {"
    assert abi.count(tiles) == 2 and abi.count("counted_scan") == 1
    assert abi.index(tiles) < abi.index(scan) < abi.rindex(tiles)
    assert_split_launches_by_max_tiles_per_launch()
    assert FIND_HW_LAUNCH_TILES == 8388544
    assert find_plan((1 << 32) + 33, 23) == (524289, 3)
    assert find_plan(64 * TILE * 3 + 22, 23, 64) == (192, 7) and find_plan(64 * TILE * 3 + 23, 23, 64) == (193, 9)


# ---------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
SENTINEL = -0x3C3C3C3C3C3C3C3D
HOST_SENTINEL = 0xDEADBEEFDEADBEEF


def _host_call(L, bits, n_len, pat, d, both, pos, info, cap):
    n = ctypes.c_uint64(0xDEAD)
    rc = L.cnt_find_pattern(bits.ctypes.data, n_len, pat[0], pat[2], pat[1], d, CNT_FIND_BOTH_STRANDS if both else 0, pos.ctypes.data,
                            info.ctypes.data if info is not None else None, cap, ctypes.byref(n))
    return rc, n.value


def _dev_result(pos, info, count):
    n = int(count.item())
    return n, pos[:n].cpu().numpy().view(np.uint64), (info[:n].cpu().numpy().view(np.uint64) if info is not None else None)


def _edge_lengths(k):
    """m = 0, 1, 2; one word; one tile - 1, exactly, + 1; several tiles and a ragged end"""
    return [k - 1, k, k + 1, 32, 33, 64 + k] + [m + k - 1 for m in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 3 * TILE + 77)]


CASES = [  # (k, wildcards, d): narrow and wide kernels, no / some / all-but-three wildcards, bounds 0 .. 5
    (1, 0, 0), (2, 0, 1), (7, 1, 1), (12, 0, 3), (15, 4, 2), (16, 0, 0), (16, 13, 1), (17, 0, 3), (23, 1, 3), (23, 1, 5), (31, 9, 0), (32, 0, 5), (32, 29, 2),
]


@gpu
@pytest.mark.parametrize("k,n_wild,d", CASES)
def test_gpu_planted_occurrences_both_tiers(oracle, k, n_wild, d):
    """random sequences with planted copies of the pattern and of its reverse complement at 0 .. d+1 substitutions, at every
    length edge and every 8-B phase of d_bits, both tiers, one strand and both, exact against the numpy reference.  The
    condition, asserted on the reference before the library is called: every length with room for the plants (>= 16 (k+1)
    nt) holds at least one expected hit per searched strand and one near-miss at d+1 that is not an expected hit, so no
    length of a case passes by finding nothing; the shorter lengths (no window, one, two, one word) are there for the edges."""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(1000 * k + 10 * n_wild + d)
    codes, wild = random_pattern(rng, k, n_wild)
    pat = pack_pattern(codes, wild)
    assert d + 1 <= k - n_wild  # a near-miss at d+1 exists
    roomy = 0
    for li, n_len in enumerate(_edge_lengths(k)):
        s, plants = planted_sequence(rng, n_len, pat, d, True)
        for phase in range(4) if li % 3 == 0 else (li % 4,):
            allw = np.concatenate([rng.integers(0, 2**64, phase, dtype=np.uint64), words_of_codes(oracle, s, extra=2, rng=rng)])
            nw = max((n_len + 31) // 32, 1)
            src = allw[phase : phase + nw]
            dall = torch.from_numpy(allw.view(np.int64)).cuda()
            for both in (False, True):
                want = ref_find(oracle, src, n_len, pat, d, both)
                room = n_len >= 16 * (k + 1)
                hits, misses = assert_plants(want, [p for p in plants if both or p[1] == 0], d, both, room)
                roomy += room
                tag = (k, n_wild, d, n_len, phase, both)
                pos, info = po.find_pattern_hip(src, n_len, pat, d, both_strands=both)
                assert np.array_equal(pos, want[0]) and np.array_equal(info, want[1]), tag + ("host",)
                n, gp, gi = _dev_result(*po.find_pattern_dev(dall[phase : phase + nw], n_len, pat, d, both_strands=both))
                assert n == want[0].size and np.array_equal(gp, want[0]) and np.array_equal(gi, want[1]), tag + ("device",)
    assert roomy >= 12


@gpu
def test_gpu_ascii_pattern_and_strands(oracle):
    """the guide + NGG spelling through both wrappers: a site on each strand, the N free, the GG not"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(5)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    s = bytearray(LETTERS[rng.integers(0, 4, 5000)].tobytes())
    site = GUIDE.replace("N", "T").encode()
    s[100:123] = site
    s[TILE // 2 : TILE // 2 + 23] = GUIDE.replace("N", "C").encode().translate(comp)[::-1]
    s[3000:3023] = site[:21] + b"AG"  # a broken PAM: one mismatch
    words = oracle.n_to_bits_lut(np.frombuffer(bytes(s), dtype=np.uint8))
    pos, info = po.find_pattern_hip(words, 5000, GUIDE, 0, both_strands=True)
    assert pos.tolist() == [100, TILE // 2] and info.tolist() == [0, CNT_FIND_REVERSE]
    pos, info, count = po.find_pattern_dev(torch.from_numpy(words.view(np.int64)).cuda(), 5000, GUIDE, 1, both_strands=True)
    n, gp, gi = _dev_result(pos, info, count)
    want = ref_find(oracle, words, 5000, po.pattern_from_ascii(GUIDE), 1, True)
    assert np.array_equal(gp, want[0]) and np.array_equal(gi, want[1]) and {100, TILE // 2, 3000} <= set(gp.tolist())
    assert gi[gp.tolist().index(3000)] == 1


@gpu
def test_gpu_capacity_sentinels_no_info_and_dense(oracle, L):
    """out_cap of 0, 1, n-1, n, n+1 at 8-B phases of pos / info with sentinels on both sides that survive; info = NULL; the
    count SET over a poisoned value with its neighbours untouched; the host tier's CNT_ECAP with *count = n after writing
    the prefix, staged and pinned; the dense extreme (max_mismatches = k, both strands: n = 2m) on a few tiles"""
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(3)
    pbuf = torch.empty(8 * TILE + 64, dtype=torch.int64, device="cuda")
    ibuf = torch.empty(8 * TILE + 64, dtype=torch.int64, device="cuda")
    cbuf = torch.empty(4, dtype=torch.int64, device="cuda")
    for k, n_wild, d, both, n_len in ((23, 1, 3, True, 3 * TILE + 5), (12, 0, 2, False, TILE + 100), (5, 1, 1, True, 2 * TILE + 300), (32, 0, 32, True, 3 * TILE + 40),
                                      (9, 9, 0, False, 2 * TILE + 1)):
        codes, wild = random_pattern(rng, k, n_wild)
        pat = pack_pattern(codes, wild)
        s, _ = planted_sequence(rng, n_len, pat, min(d, k - n_wild - 1) if n_wild < k else 0, both)
        src = words_of_codes(oracle, s, rng=rng)
        d_src = torch.from_numpy(src.view(np.int64)).cuda()
        want_p, want_i = ref_find(oracle, src, n_len, pat, d, both)
        n = want_p.size
        m = n_len - k + 1
        assert n >= 3 and (d < k and n_wild < k or n == (2 * m if both else m))  # the dense cases hit every window
        for ph, cap in ((0, n), (3, n + 1), (5, n - 1), (2, 1), (7, 0)):
            for with_info in (True, False):
                tag = (k, d, both, n_len, ph, cap, with_info)
                pbuf.fill_(SENTINEL)
                ibuf.fill_(SENTINEL)
                cbuf.fill_(SENTINEL)
                po.find_pattern_dev(d_src, n_len, pat, d, both_strands=both, info=ibuf[8 + ph : 8 + ph + cap] if with_info else False,
                                    pos=pbuf[8 + ph : 8 + ph + cap], count=cbuf[1:2])
                torch.cuda.synchronize()
                c = cbuf.cpu().numpy()
                assert c[1] == n and c[0] == SENTINEL and (c[2:] == SENTINEL).all(), tag
                got = min(n, cap)
                p = pbuf.cpu().numpy()
                assert (p[: 8 + ph] == SENTINEL).all() and (p[8 + ph + got :] == SENTINEL).all(), tag
                assert np.array_equal(p[8 + ph : 8 + ph + got].view(np.uint64), want_p[:got]), tag
                i = ibuf.cpu().numpy()
                if with_info:
                    assert (i[: 8 + ph] == SENTINEL).all() and (i[8 + ph + got :] == SENTINEL).all(), tag
                    assert np.array_equal(i[8 + ph : 8 + ph + got].view(np.uint64), want_i[:got]), tag
                else:
                    assert (i == SENTINEL).all(), tag
        for pinned in (False, True):
            bits = cn.pinned_empty(src.size, np.uint64) if pinned else src.copy()
            bits[:] = src
            hp = cn.pinned_empty(n + 16, np.uint64) if pinned else np.empty(n + 16, dtype=np.uint64)
            hi = cn.pinned_empty(n + 16, np.uint64) if pinned else np.empty(n + 16, dtype=np.uint64)
            for cap in (n, n + 1, n - 1, 1, 0):
                for with_info in (True, False):
                    hp[:] = HOST_SENTINEL
                    hi[:] = HOST_SENTINEL
                    rc, got_n = _host_call(L, bits, n_len, pat, d, both, hp, hi if with_info else None, cap)
                    tag = (k, d, both, n_len, cap, with_info, pinned)
                    assert rc == (_lib.CNT_ECAP if n > cap else _lib.CNT_OK) and got_n == n, (tag, rc, got_n)
                    got = min(n, cap)
                    assert np.array_equal(hp[:got], want_p[:got]) and (hp[got:] == HOST_SENTINEL).all(), tag
                    if with_info:
                        assert np.array_equal(hi[:got], want_i[:got]) and (hi[got:] == HOST_SENTINEL).all(), tag
                    else:
                        assert (hi == HOST_SENTINEL).all(), tag
        # the guess-and-retry wrapper: the dense results are far beyond its first guess
        hp2, hi2 = po.find_pattern_hip(src, n_len, pat, d, both_strands=both)
        assert np.array_equal(hp2, want_p) and np.array_equal(hi2, want_i)
    # m == 0 sets the device count to 0
    cbuf.fill_(SENTINEL)
    _, _, count = po.find_pattern_dev(d_src, 22, GUIDE, 3, count=cbuf[1:2])
    assert int(count.item()) == 0 and cbuf.cpu().numpy()[0] == SENTINEL


def _edge_sites(n_len, k, step=TILE):
    """a site across every tile edge: the window starts k/2 codes (at least one) before the edge and ends behind it"""
    return [b - max(k // 2, 1) for b in range(step, n_len - k, step)]


@gpu
@pytest.mark.parametrize("both", [False, True])
def test_gpu_hits_straddling_tile_and_launch_edges(oracle, launch_tiles, both):
    """the lab build cut into launches of 64 / 128 tiles: the pattern planted across EVERY tile edge (so across every launch
    edge too), alternating strands and substitution counts; both passes in several launches, counted in a captured graph"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(launch_tiles)
    for k, n_wild, d, n_len in ((23, 1, 3, launch_tiles * TILE * 3 + 22), (9, 0, 1, launch_tiles * TILE * 2 + 5000), (32, 2, 2, launch_tiles * TILE + 40)):
        codes, wild = random_pattern(rng, k, n_wild)
        pat = pack_pattern(codes, wild)
        s = rng.integers(0, 4, n_len).astype(np.uint8)
        sites = _edge_sites(n_len, k)
        plants = []
        for j, site in enumerate(sites):
            strand, e = (j & 1) if both else 0, (j >> 1) % (d + 2)
            Q, V = revcomp_pattern(codes, wild) if strand else (codes, wild)
            s[site : site + k] = mutated(rng, Q, V, e)
            plants.append((site, strand, e))
        src = words_of_codes(oracle, s, rng=rng)
        want = ref_find(oracle, src, n_len, pat, d, both)
        hits, misses = assert_plants(want, plants, d, both, True)
        assert hits[0] + hits[1] + misses == len(sites) >= launch_tiles - 1
        dsrc = torch.from_numpy(src.view(np.int64)).cuda()
        res = po.find_pattern_dev(dsrc, n_len, pat, d, both_strands=both)
        n, gp, gi = _dev_result(*res)
        assert n == want[0].size and np.array_equal(gp, want[0]) and np.array_equal(gi, want[1]), (k, n_len)
        tiles, launches = find_plan(n_len, k, launch_tiles)
        assert launches >= 5 or n_len < 2 * launch_tiles * TILE
        assert _kernel_nodes_of(torch, lambda: po.find_pattern_dev(dsrc, n_len, pat, d, both_strands=both, pos=res[0], info=res[1], count=res[2])) == launches
        hp, hi = po.find_pattern_hip(src, n_len, pat, d, both_strands=both)
        assert np.array_equal(hp, want[0]) and np.array_equal(hi, want[1])


@gpu
def test_gpu_find_in_a_captured_graph_and_behind_a_side_stream(oracle):
    """encode -> search on both strands -> search of the reverse complement, captured with torch.cuda.graph with the same
    buffers and the same scratch (never zeroed) and replayed on 2 different inputs; then fill -> encode -> search enqueued on
    a side stream with no host sync in between"""
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import devutil, packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    n_len, k, d = (1 << 20) + 4133, 23, 3
    pat = po.pattern_from_ascii(GUIDE)
    words = (n_len + 31) // 32
    d_n = torch.zeros(n_len, dtype=torch.uint8, device="cuda")
    bits = torch.empty(words, dtype=torch.int64, device="cuda")
    rc = torch.empty(words, dtype=torch.int64, device="cuda")
    need = po.find_pattern_work_bytes(n_len, k)
    work = torch.empty(need + 8, dtype=torch.uint8, device="cuda")
    cap = 4096
    outs = [(torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda"),
             torch.empty(1, dtype=torch.int64, device="cuda")) for _ in range(2)]

    def chain():
        cn.n_to_bits_dev(d_n, out=bits)
        po.find_pattern_dev(bits, n_len, pat, d, both_strands=True, pos=outs[0][0], info=outs[0][1], count=outs[0][2], work=work[3:])  # scratch at an odd byte
        po.reverse_complement_dev(bits, n_len, out=rc)
        po.find_pattern_dev(rc, n_len, pat, d, pos=outs[1][0], info=outs[1][1], count=outs[1][2], work=work[3:])  # the same scratch, in stream order

    tiles, launches = find_plan(n_len, k)
    assert _kernel_nodes_of(torch, lambda: po.find_pattern_dev(bits, n_len, pat, d, pos=outs[0][0], info=outs[0][1], count=outs[0][2], work=work)) == launches == 3
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    rng = np.random.default_rng(31)
    for rep in range(2):
        s, plants = planted_sequence(rng, n_len, pat, d, True)
        host = LETTERS[s]
        d_n.copy_(torch.from_numpy(host))
        for o in outs:
            for t in o:
                t.fill_(SENTINEL)
        work.fill_(0x77 + rep)  # the scratch needs no zeroing
        g.replay()
        torch.cuda.synchronize()
        hb = oracle.n_to_bits_lut(host)
        for j, (b, both) in enumerate(((hb, True), (oracle.reverse_complement(hb, n_len), False))):
            want = ref_find(oracle, b, n_len, pat, d, both)
            if j == 0:
                assert_plants(want, plants, d, True, True)
            n, gp, gi = _dev_result(*outs[j])
            assert n == want[0].size >= 2 and np.array_equal(gp, want[0]) and np.array_equal(gi, want[1]), (rep, j)
            assert (outs[j][0][n:].cpu().numpy() == SENTINEL).all(), (rep, j)
    # a producer and its consumer on a side stream, enqueued back to back; 12-nt pattern, two mismatches: thousands of hits
    seed, n2, pat12 = 77, (1 << 22) + 19, po.pattern_from_ascii("ACGTTGCAAGCT")
    want = ref_find(oracle, oracle.n_to_bits_lut(oracle.fill_random_acgt(n2, seed)), n2, pat12, 2, True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        n = torch.zeros(n2, dtype=torch.uint8, device="cuda")
        devutil.fill_random_acgt(n, seed)
        pos, info, count = po.find_pattern_dev(cn.n_to_bits_dev(n), n2, pat12, 2, both_strands=True)
    torch.cuda.current_stream().wait_stream(side)
    got = _dev_result(pos, info, count)
    assert got[0] == want[0].size > 100 and np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1])


@gpu
def test_gpu_pinned_in_place_equals_staged(oracle, L):
    """pinned bits / pos / info (used in place, the kernels reading and writing host memory over the link) against ordinary
    ones (staged): identical results, at a phase inside the pinned allocations, and with only some buffers pinned (staged)"""
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    rng = np.random.default_rng(9)
    for k, n_wild, d, both, n_len in ((23, 1, 3, True, 5 * TILE + 77), (11, 0, 1, False, 2 * TILE + 5), (32, 4, 4, True, TILE - 3)):
        codes, wild = random_pattern(rng, k, n_wild)
        pat = pack_pattern(codes, wild)
        s, plants = planted_sequence(rng, n_len, pat, d, both)
        src = words_of_codes(oracle, s, rng=rng)
        want = ref_find(oracle, src, n_len, pat, d, both)
        assert_plants(want, plants, d, both, True)
        n = want[0].size
        results = []
        for pin_in, pin_out in ((False, False), (True, True), (True, False), (False, True)):
            bits = cn.pinned_empty(src.size + 3, np.uint64)[3:] if pin_in else src.copy()
            bits[:] = src
            hp = cn.pinned_empty(n + 9, np.uint64)[1:] if pin_out else np.empty(n + 8, dtype=np.uint64)
            hi = cn.pinned_empty(n + 9, np.uint64)[1:] if pin_out else np.empty(n + 8, dtype=np.uint64)
            hp[:] = HOST_SENTINEL
            hi[:] = HOST_SENTINEL
            if pin_in and pin_out:
                assert L.cnt_host_is_pinned(bits.ctypes.data, bits.nbytes) == 1 and L.cnt_host_is_pinned(hp.ctypes.data, hp.nbytes) == 1
            rc, got_n = _host_call(L, bits, n_len, pat, d, both, hp, hi, n + 8)
            assert rc == _lib.CNT_OK and got_n == n, (k, pin_in, pin_out, rc, got_n)
            assert (hp[n:] == HOST_SENTINEL).all() and (hi[n:] == HOST_SENTINEL).all()
            results.append((hp[:n].copy(), hi[:n].copy()))
        for p, i in results:
            assert np.array_equal(p, want[0]) and np.array_equal(i, want[1])


@gpu
@pytest.mark.parametrize("seed", range(4))
def test_gpu_find_fuzz(oracle, L, seed):
    """random lengths, k, wildcards, bounds, strands, input phases, capacities and info on / off; both tiers"""
    import torch

    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(7300 + seed)
    for it in range(40):
        k = int(rng.integers(1, 33))
        n_wild = int(rng.choice([0, 0, rng.integers(0, k + 1)]))
        d = int(rng.choice([0, 1, 2, 3, 5, rng.integers(0, k + 1)]))
        d = min(d, k)
        n_len = int(rng.choice([rng.integers(0, 300), rng.integers(0, 3 * TILE), rng.integers(0, 12 * TILE)]))
        both, with_info, pi = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), int(rng.integers(0, 4))
        codes, wild = random_pattern(rng, k, n_wild)
        pat = pack_pattern(codes, wild)
        dp = min(d, max(k - n_wild - 1, 0))
        s, _ = planted_sequence(rng, n_len, pat, dp, both) if n_len >= 8 * (k + 1) and n_wild < k else (rng.integers(0, 4, n_len).astype(np.uint8), [])
        allw = np.concatenate([rng.integers(0, 2**64, pi, dtype=np.uint64), words_of_codes(oracle, s, extra=2, rng=rng)])
        nw = max((n_len + 31) // 32, 1)
        src = allw[pi : pi + nw]
        want = ref_find(oracle, src, n_len, pat, d, both)
        n = want[0].size
        cap = int(rng.choice([n, n + 3, max(n - 1, 0), int(rng.integers(0, n + 1))]))
        tag = (seed, it, n_len, k, n_wild, d, both, with_info, pi, cap, n)
        dall = torch.from_numpy(allw.view(np.int64)).cuda()
        pbuf = torch.full((cap + 8,), SENTINEL, dtype=torch.int64, device="cuda")
        ibuf = torch.full((cap + 8,), SENTINEL, dtype=torch.int64, device="cuda")
        _, _, count = po.find_pattern_dev(dall[pi : pi + nw], n_len, pat, d, both_strands=both, pos=pbuf[3 : 3 + cap], info=ibuf[3 : 3 + cap] if with_info else False)
        got = min(n, cap)
        assert int(count.item()) == n, tag
        p, i = pbuf.cpu().numpy(), ibuf.cpu().numpy()
        assert np.array_equal(p[3 : 3 + got].view(np.uint64), want[0][:got]) and (p[:3] == SENTINEL).all() and (p[3 + got :] == SENTINEL).all(), tag
        if with_info:
            assert np.array_equal(i[3 : 3 + got].view(np.uint64), want[1][:got]) and (i[:3] == SENTINEL).all() and (i[3 + got :] == SENTINEL).all(), tag
        else:
            assert (i == SENTINEL).all(), tag
        hp = np.full(cap + 2, HOST_SENTINEL, dtype=np.uint64)
        hi = np.full(cap + 2, HOST_SENTINEL, dtype=np.uint64)
        rc, hn = _host_call(L, np.ascontiguousarray(src), n_len, pat, d, both, hp, hi if with_info else None, cap)
        assert rc == (_lib.CNT_ECAP if n > cap else _lib.CNT_OK) and hn == n, tag
        assert np.array_equal(hp[:got], want[0][:got]) and (hp[got:] == HOST_SENTINEL).all(), tag
        if with_info:
            assert np.array_equal(hi[:got], want[1][:got]) and (hi[got:] == HOST_SENTINEL).all(), tag


def _set_codes(words, first_nt, at, codes):
    """write `codes` at nucleotide `at` into `words`, which hold the nucleotides from first_nt on; codes outside are dropped"""
    for j, c in enumerate(codes):
        i = at + j - first_nt
        if 0 <= i < words.size * 32:
            sh = np.uint64(2 * (i & 31))
            words[i >> 5] = (words[i >> 5] & ~(np.uint64(3) << sh)) | (np.uint64(c) << sh)


def _host_stream_reference(oracle, seed, n_len, pat, d, both, plants, chunk=1 << 24, workers=12):
    """chunked host reference over oracle.fill_random_acgt with the plants [(site, codes)] written in: chunk c holds windows
    [c*chunk, (c+1)*chunk) and the k-1 codes behind them.  Returns (pos, info) of the whole sequence."""
    from concurrent.futures import ThreadPoolExecutor

    k = pat[2]
    m = n_len - k + 1

    def one(t0):
        c = min(chunk, m - t0)
        nt = c + k - 1
        words = oracle.n_to_bits_lut(oracle.fill_random_acgt(nt, seed, first_nt=t0))
        for site, codes in plants:
            if site + k > t0 and site < t0 + nt:
                _set_codes(words, t0, site, codes)
        return np_find(oracle.kmers(words, nt, k, False), pat, d, both, first=t0)

    parts = []
    starts = list(range(0, m, chunk))
    with ThreadPoolExecutor(workers) as pool:
        for b in range(0, len(starts), workers):
            parts += list(pool.map(one, starts[b : b + workers]))
    return np.concatenate([p for p, _ in parts]), np.concatenate([i for _, i in parts])


@gpu
def test_gpu_find_full_size_past_2p32(oracle, fullsize):
    """2^32 + 2^21 + 33 nt of cnt_fill_random_acgt_dev data, the guide + NGG pattern, three mismatches, both strands: sparse
    hits (about 250 by chance) and sites planted beyond position 2^32 -- across a tile edge, in the last window, on both
    strands, at 0 .. 4 substitutions -- exact against the chunked host reference computed from the same counter-based
    generator with the same plants"""
    import torch

    from conftest import need_free_hbm
    from cute_nucleotides_amd import packed_ops as po
    from test_kmers import _device_sequence

    n_len, d, seed = (1 << 32) + (1 << 21) + 33, 3, 0x66696E64
    pat = po.pattern_from_ascii(GUIDE)
    k = pat[2]
    m = n_len - k + 1
    codes, wild = unpack_pattern(pat)
    rng = np.random.default_rng(8)
    sites = [12345, (1 << 31) + 7, (1 << 32) - 11, (1 << 32) + 37, (1 << 32) + 3 * TILE - 10, (1 << 32) + (1 << 20) + 31, (1 << 32) + (1 << 21) - 64, m - 1]
    assert all(b - a >= k for a, b in zip(sites, sites[1:]))  # disjoint plants
    plants, meta = [], []
    for j, site in enumerate(sites):
        strand, e = j & 1, (0, 0, 3, 1, 2, 4, 3, 0)[j]
        Q, V = revcomp_pattern(codes, wild) if strand else (codes, wild)
        plants.append((site, mutated(rng, Q, V, e)))
        meta.append((site, strand, e))
    need_free_hbm((n_len + (n_len >> 2)) // (1 << 30) + 2)
    bits = _device_sequence(n_len, seed)
    for site, pc in plants:  # the same plants on the device: the few words around each site through the host
        w0 = site >> 5
        piece = bits[w0 : w0 + 3].cpu().numpy().view(np.uint64).copy()
        _set_codes(piece, w0 * 32, site, pc)
        bits[w0 : w0 + 3] = torch.from_numpy(piece.view(np.int64)).cuda()
    cap = 1 << 16
    pos = torch.empty(cap, dtype=torch.int64, device="cuda")
    info = torch.empty(cap, dtype=torch.int64, device="cuda")
    work = torch.empty(po.find_pattern_work_bytes(n_len, k), dtype=torch.uint8, device="cuda")
    po.find_pattern_dev(bits, n_len, pat, d, both_strands=True, pos=pos, info=info, work=work)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, count = po.find_pattern_dev(bits, n_len, pat, d, both_strands=True, pos=pos, info=info, work=work)
    torch.cuda.synchronize()
    fullsize(32, (time.perf_counter() - t0) * 1e3, check="find_pattern k=23 d=3 both strands: kernels")
    n, gp, gi = _dev_result(pos, info, count)
    t1 = time.perf_counter()
    want = _host_stream_reference(oracle, seed, n_len, pat, d, True, plants)
    fullsize(32, (time.perf_counter() - t1) * 1e3, check="find_pattern: chunked host reference")
    hits, misses = assert_plants(want, meta, d, True, True)
    assert hits[0] + hits[1] == 7 and misses == 1
    assert n == want[0].size <= cap, (n, want[0].size)
    assert np.array_equal(gp, want[0]) and np.array_equal(gi, want[1])
    beyond = sum(1 for site, _, e in meta if site >= 1 << 32 and e <= d)  # the planted hits past 2^32 (chance hits come on top)
    assert int(gp[-1]) == m - 1 and beyond == 4 and (gp >= 1 << 32).sum() >= beyond
