"""k-mer extraction on packed words (include/cute_nt.h "k-mers"): forward and canonical k-mers, k = 1..32.  Not in the
reference, so the CPU part pins the scalar oracle (oracle.kmers: rolling values, one code per step) and a numpy window
reference against a definition in letters for every k, and the two whole-stream references against each other; it checks
the ABI's argument errors and wiring, and the ISA of the new kernels.  The GPU part compares both tiers with the
references bit for bit: at every output phase of the 128-B head peel against every input word phase, inside a captured
graph and behind a producer on a side stream, with the host tier's staging shared with the packed-ops host calls, and
whole outputs past 2^31, 2^32 and 2^33 k-mers (the last one in two launches) against the oracle stream checksum."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = bytes.maketrans(b"ACGT", b"TGCA")
KS = [1, 2, 15, 16, 17, 31, 32]
CPU_SIZES = [0, 1, "k-1", "k", 31, 32, 33, 63, 64, 65, 1000, 4099]
CNT_KMER_CANONICAL = 0x10


def _sizes(k, extra=()):
    return sorted({(k - 1 if s == "k-1" else k if s == "k" else s) for s in list(CPU_SIZES) + list(extra)})


# ---- numpy reference ------------------------------------------------------------------------------------------------
_SH = np.arange(32, dtype=np.uint64) * np.uint64(2)


def _reverse_codes(x):
    """the 32 two-bit codes of each u64 in reverse order: swap codes inside bytes, then the bytes"""
    x = ((x >> np.uint64(2)) & np.uint64(0x3333333333333333)) | ((x & np.uint64(0x3333333333333333)) << np.uint64(2))
    x = ((x >> np.uint64(4)) & np.uint64(0x0F0F0F0F0F0F0F0F)) | ((x & np.uint64(0x0F0F0F0F0F0F0F0F)) << np.uint64(4))
    return x.byteswap()


def np_kmers(words, length, k, canonical=False):
    """k-mer 32w+r = the 64-bit window of the packed words at nucleotide 32w+r (words w and w+1 shifted right by 2r codes'
    worth of bits), masked to 2k bits; canonical: min with the reverse complement (complement, reverse the 32 codes, shift
    the k codes down)."""
    m = length - k + 1 if length >= k else 0
    if m == 0:
        return np.empty(0, dtype=np.uint64)
    nw = (m + 31) // 32
    w = np.zeros(nw + 1, dtype=np.uint64)
    have = min((length + 31) // 32, nw + 1)
    w[:have] = np.asarray(words, dtype=np.uint64)[:have]
    lo, hi = w[:-1, None], w[1:, None]
    x = (lo >> _SH) | np.where(_SH == 0, np.uint64(0), (hi << np.uint64(1)) << (np.uint64(63) - _SH))
    x = x.reshape(-1)[:m]
    x &= np.uint64((1 << (2 * k)) - 1)
    if not canonical:
        return x
    rc = _reverse_codes(x ^ np.uint64(0xAAAAAAAAAAAAAAAA)) >> np.uint64(64 - 2 * k)
    return np.minimum(x, rc)


def ascii_kmers(oracle, s, k, canonical=False):
    """the definition in letters: k-mer i = s[i:i+k] packed like a sequence of length k (oracle.n_to_bits_lut of the
    letters, padded with 'A' = code 0 to one word); rc = the reverse complement of those letters, packed the same way"""
    m = len(s) - k + 1 if len(s) >= k else 0
    if m == 0:
        return np.empty(0, dtype=np.uint64)

    def pack(kmers):
        return oracle.n_to_bits_lut(np.frombuffer(b"".join(x + b"A" * (32 - k) for x in kmers), dtype=np.uint8))

    fwd = [s[i : i + k] for i in range(m)]
    f = pack(fwd)
    if not canonical:
        return f
    return np.minimum(f, pack([x.translate(COMP)[::-1] for x in fwd]))


@pytest.mark.parametrize("k", KS)
def test_numpy_reference_against_letters(oracle, k):
    for n_len in _sizes(k):
        s = oracle.fill_random_acgt(n_len, seed=1000 + n_len + k).tobytes()
        words = oracle.np_n_to_bits_lut(np.frombuffer(s, dtype=np.uint8))
        for canonical in (False, True):
            want = ascii_kmers(oracle, s, k, canonical)
            got = np_kmers(words, n_len, k, canonical)
            assert got.dtype == np.uint64 and got.size == max(n_len - k + 1, 0)
            assert np.array_equal(got, want), (n_len, k, canonical)
        if n_len >= k:
            # forward k-mer i decodes to the letters i..i+k-1; bits 2k..63 are zero
            f = np_kmers(words, n_len, k)
            for i in (0, n_len - k, (n_len - k) // 2):
                assert bytes(oracle.bits_to_n_lut(f[i : i + 1], k)) == s[i : i + k]
            assert k == 32 or not (f >> np.uint64(2 * k)).any()
            # strand symmetry: canonical k-mer i of s == canonical k-mer m-1-i of revcomp(s)
            rs = s.translate(COMP)[::-1]
            rw = oracle.np_n_to_bits_lut(np.frombuffer(rs, dtype=np.uint8))
            assert np.array_equal(np_kmers(words, n_len, k, True), np_kmers(rw, n_len, k, True)[::-1])
            # bits beyond len in the last word are ignored
            if n_len & 31:
                g = words.copy()
                g[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(2 * (n_len & 31))
                for canonical in (False, True):
                    assert np.array_equal(np_kmers(g, n_len, k, canonical), np_kmers(words, n_len, k, canonical))


ORACLE_SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 32 * 7 - 1, 32 * 7, 32 * 7 + 1, 32 * 9 + 17]


@pytest.mark.parametrize("k", range(1, 33))
def test_scalar_oracle_against_letters_and_numpy(oracle, k):
    """oracle.kmers (cnt_oracle_kmers: rolling values, one code per step) == the definition in letters == the numpy window
    reference, for every k, at lengths around multiples of 32, with random garbage above len in the last word and in a
    word past it"""
    rng = np.random.default_rng(4000 + k)
    for n_len in sorted(set(ORACLE_SIZES + [k - 1, k, k + 1])):
        words = _random_words(rng, n_len, extra=1)
        s = bytes(oracle.bits_to_n_lut(words, n_len))
        for canonical in (False, True):
            got = oracle.kmers(words, n_len, k, canonical)
            assert got.dtype == np.uint64 and got.size == max(n_len - k + 1, 0)
            assert np.array_equal(got, ascii_kmers(oracle, s, k, canonical)), (n_len, k, canonical)
            assert np.array_equal(got, np_kmers(words, n_len, k, canonical)), (n_len, k, canonical)
            # only the first n_len codes count
            clean = oracle.n_to_bits_lut(np.frombuffer(s, dtype=np.uint8))
            assert np.array_equal(oracle.kmers(clean, n_len, k, canonical), got)
    # canonical differs from forward somewhere (k-mers that are not their own reverse complement's minimum exist)
    w = _random_words(rng, 500)
    assert not np.array_equal(oracle.kmers(w, 500, k, True), oracle.kmers(w, 500, k, False))


def test_scalar_oracle_refuses_bad_arguments(oracle):
    w = np.zeros(2, dtype=np.uint64)
    for k in (0, 33):
        with pytest.raises(ValueError):
            oracle.kmers(w, 64, k)
    with pytest.raises(ValueError):
        oracle.kmers(w, 65, 3)
    assert oracle.kmers(w, 20, 21).size == 0 and oracle.kmers(w, 0, 1, canonical=True).size == 0
    # the C entry point checks k and the flags itself
    out = np.zeros(4, dtype=np.uint64)
    for k, flags in ((0, 0), (33, 0), (5, 0x1), (5, 0x20)):
        assert oracle.lib().cnt_oracle_kmers(w.ctypes.data, 40, k, flags, out.ctypes.data) == 4
    assert not out.any()


def test_numpy_host_checksum_equals_the_oracle_stream(oracle):
    """the two references agree on whole streams: the numpy window reference chunked by _host_checksum, and the scalar
    oracle's stream_kmers_checksum (chunks of different sizes, so their boundaries fall at different k-mers)"""
    for n_len, k, canonical in (((1 << 26) + 17, 31, True), ((1 << 25) + 33, 17, False)):
        seed = 0x6B6D6572 + k
        want = oracle.stream_kmers_checksum(seed, n_len, k, canonical, chunk_nt=(1 << 22) + 5)
        assert _host_checksum(oracle, n_len, k, canonical, seed) == want, (n_len, k, canonical)


def test_canonical_order_is_numeric_not_lexicographic(oracle):
    """the header's one sentence: min() compares the LSB-first packed u64, not the letters"""
    def canon(letters):
        return np_kmers(oracle.n_to_bits_lut(np.frombuffer(letters, dtype=np.uint8)), len(letters), len(letters), True).tolist()

    assert canon(b"CA") == [1]  # "CA" = 1 | 0 << 2, its reverse complement "TG" = 2 | 3 << 2 = 14
    assert canon(b"AG") == canon(b"CT") == [9]  # "CT" = 1 | 2 << 2 = 9 < "AG" = 0 | 3 << 2 = 12, though "AG" < "CT" in letters


# ---- ABI, no device needed ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


def test_abi_errors_come_before_any_device_work(L):
    from cute_nucleotides_amd import _lib

    buf = np.zeros(4096, dtype=np.uint64)
    base = buf.ctypes.data
    q = lambda word, byte=0: ctypes.c_void_p(base + 8 * word + byte)  # noqa: E731
    out = np.full(64, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    o = lambda byte=0: ctypes.c_void_p(out.ctypes.data + byte)  # noqa: E731
    for fn, tail in ((L.cnt_kmers, ()), (L.cnt_kmers_dev, (None,))):
        call = lambda *a: fn(*(a + tail))  # noqa: E731
        # k out of range, unknown flags -- even when there would be no k-mer
        for k in (0, 33, 64):
            assert call(q(0), 100, k, 0, o(), 64) == _lib.CNT_EINVAL, (fn, k)
            assert call(None, 0, k, 0, None, 0) == _lib.CNT_EINVAL
        for flags in (0x1, 0x2, 0x4, 0x8, 0x20, 0x80000000, CNT_KMER_CANONICAL | 0x1):
            assert call(q(0), 100, 21, flags, o(), 64) == _lib.CNT_EINVAL, (fn, flags)
        # NULL pointers when m > 0
        assert call(None, 100, 21, 0, o(), 64) == _lib.CNT_EINVAL
        assert call(q(0), 100, 21, 0, None, 64) == _lib.CNT_EINVAL
        # pointers not 8-B aligned
        for byte in (1, 4, 7):
            assert call(q(0, byte), 100, 21, 0, o(), 64) == _lib.CNT_EINVAL
            assert call(q(0), 100, 21, CNT_KMER_CANONICAL, o(byte), 64) == _lib.CNT_EINVAL
        # output overlapping the input words (100 nt = 4 words at q(10)): inside, straddling either end, identical
        for ow in (10, 12, 13, 8, 0):
            assert call(q(10), 100, 21, 0, q(ow), 80) == _lib.CNT_EINVAL, (fn, ow)
        # capacity: m = 80
        assert call(q(10), 100, 21, 0, q(100), 79) == _lib.CNT_ECAP
        assert call(q(0), 100, 1, 0, o(), 64) == _lib.CNT_ECAP  # m = 100 > 64
        # len < k: zero k-mers, CNT_OK without a device, also with NULL pointers
        assert call(None, 0, 1, 0, None, 0) == _lib.CNT_OK
        assert call(None, 20, 21, CNT_KMER_CANONICAL, None, 0) == _lib.CNT_OK
        assert call(q(0), 31, 32, 0, o(), 0) == _lib.CNT_OK
    assert (out == 0x5A5A5A5A5A5A5A5A).all()  # nothing was written
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        for flags in (0, CNT_KMER_CANONICAL):  # m = 84 - 21 + 1 = 64
            assert L.cnt_kmers(q(0), 84, 21, flags, o(), 64) == _lib.CNT_ENODEV
            assert L.cnt_kmers_dev(q(0), 84, 21, flags, o(), 64, None) < 0
        assert (out == 0x5A5A5A5A5A5A5A5A).all()


def test_python_wrappers_raise_value_error(L):
    from cute_nucleotides_amd import packed_ops as po

    w = np.zeros(2, dtype=np.uint64)
    for k in (0, 33):
        with pytest.raises(ValueError):
            po.kmers_hip(w, 64, k)
    with pytest.raises(ValueError):
        po.kmers_hip(w, 65, 21)  # longer than the words hold
    with pytest.raises(ValueError):
        po.kmers_hip(w, 64, 21, out=np.empty(43, dtype=np.uint64))  # m = 44
    assert po.kmers_hip(w, 20, 21).size == 0 and po.kmers_hip(w, 0, 1, canonical=True).size == 0


def test_abi_wiring(L):
    import subprocess

    from cute_nucleotides_amd import _lib

    for name in ("cnt_kmers", "cnt_kmers_dev"):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
    assert _lib.CNT_KMER_CANONICAL == CNT_KMER_CANONICAL
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert {"cnt_kmers", "cnt_kmers_dev"} <= exported
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    assert "#define CNT_KMER_CANONICAL 0x10u" in header
    for flag in ("CNT_STRICT_LUT 0x1u", "CNT_ALLOW_N 0x2u", "CNT_TAIL_LUT 0x4u", "CNT_SPREAD_COUNT 0x8u"):
        assert flag in header  # the new bit is distinct from every existing flag


KMER_KERNELS = ["void cnt::kmer_tiles<256, 2, false>", "void cnt::kmer_tiles<256, 2, true>", "void cnt::kmer_generic<false>", "void cnt::kmer_generic<true>"]


def test_kmer_kernels_isa():
    sys.path.insert(0, os.path.join(ROOT, "bench"))
    import isa_digest

    found = isa_digest.kernels(isa_digest.assembly())
    for name in KMER_KERNELS:
        assert name in found, name
        e = found[name]
        body = e["body"]
        assert not [i for i in body if "scratch_" in i], name
        assert not [i for i in body if "s_xor_b64 exec, exec" in i], name
        assert e["meta"]["private_segment_fixed_size"] == 0 and e["meta"]["next_free_vgpr"] <= 84, (name, e["meta"])
    for name in KMER_KERNELS[:2]:
        stores = [i for i in found[name]["body"] if "_store" in i]
        assert stores and all(i.startswith("buffer_store_dwordx4") for i in stores), stores
        assert all("sc0" in i and "sc1" in i and " nt" in i for i in stores), stores  # the codec tiles' write-through policy
    assert len(found) < 60, len(found)


# ---- the launcher's plan (hip/kmer_abi.inc), restated for the tests that count launches ---------------------------------
KMERS_PER_TILE = 1024  # kmer_kernels.hpp: 256 lanes x 2 pairs x 2 k-mers
KMER_HW_LAUNCH_TILES = ((0x7FFFFFFF // 256) // 64) * 64  # max_tiles_per_launch(256) of the product build: 8,388,544


def kmer_plan(out_ptr, n_len, k, launch_tiles=KMER_HW_LAUNCH_TILES):
    """(head, tiles, tail, kernel launches) of a call: `head` k-mers until the output sits on a 128-B line, tiles of 1024
    k-mers while they end at or below 32*(words-1), the tail up to m; ceil(tiles / launch_tiles) tile launches plus one
    generic launch for a non-empty head and one for a non-empty tail.  No tile: one generic launch over all m (tail = m)."""
    m = n_len - k + 1
    words = (n_len + 31) // 32
    head = ((128 - (out_ptr & 127)) & 127) >> 3
    tile_end = min(m, 32 * (words - 1))
    tiles = (tile_end - head) // KMERS_PER_TILE if tile_end > head else 0
    if not tiles:
        return 0, 0, m, 1
    tail = m - head - tiles * KMERS_PER_TILE
    return head, tiles, tail, -(-tiles // launch_tiles) + (head > 0) + (tail > 0)


def assert_split_launches_by_max_tiles_per_launch():
    """cute_nt.hip's split_launches, which the launchers call with their block: launches of max_tiles_per_launch(block) tiles,
    taken in order by codec2_launch.hpp's for_each_launch (the one loop over launches), the last one the remainder"""
    shim = open(os.path.join(ROOT, "hip", "cute_nt.hip")).read()
    for line in ("void split_launches(uint64_t n_tiles, int block, F&& launch) {",
                 "for_each_launch(n_tiles, max_tiles_per_launch(block), [&](uint64_t first, uint64_t n, bool) { launch(first, n); });"):
        assert line in shim, line
    loop = open(os.path.join(ROOT, "hip", "codec2_launch.hpp")).read()
    for line in ("void for_each_launch(uint64_t total, uint64_t per_launch, F&& f) {",
                 "for (uint64_t first = 0; first < total; first += per_launch) {",
                 "const uint64_t n = std::min(per_launch, total - first);",
                 "f(first, n, first + n == total);"):
        assert line in loop, line
    # the only loop over launches in hip/
    sources = [f for f in os.listdir(os.path.join(ROOT, "hip")) if f.endswith((".hip", ".hpp", ".inc"))]
    assert sum(open(os.path.join(ROOT, "hip", f)).read().count("first += per_launch") for f in sources) == 1


def test_kmer_plan_matches_the_launcher_and_splitter_source():
    """the constants kmer_plan restates are the ones in the sources"""
    src = open(os.path.join(ROOT, "hip", "kmer_kernels.hpp")).read()
    assert "constexpr int kKmerBlock = 256, kKmerU = 2;" in src and "(uint64_t)kKmerBlock * 2 * kKmerU" in src
    abi = open(os.path.join(ROOT, "hip", "kmer_abi.inc")).read()
    for line in ("uint64_t head = ((128 - (reinterpret_cast<uintptr_t>(d_out) & 127)) & 127) >> 3;",
                 "const uint64_t tile_end = std::min<uint64_t>(m, 32 * (words - 1));",
                 "split_launches(n_tiles, kKmerBlock, [&](uint64_t t, uint64_t n) {"):
        assert line in abi, line
    assert_split_launches_by_max_tiles_per_launch()
    assert KMER_HW_LAUNCH_TILES == 8388544
    # the 2^33 case of test_gpu_kmers_full_size_in_two_launches: heads 0 and 13, two tile launches each
    n_len = (1 << 33) + 4133
    assert kmer_plan(0, n_len, 32) == (0, KMER_HW_LAUNCH_TILES + 68, 6, 3)
    assert kmer_plan(24, n_len, 32) == (13, KMER_HW_LAUNCH_TILES + 67, 1017, 4)


# ---------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
GPU_EXTRA = [32 * 8192 + 7, (1 << 22) + 13, 3 * (1 << 21) + 64]


def _random_words(rng, n_len, extra=0):
    return rng.integers(0, 2**64, (n_len + 31) // 32 + extra, dtype=np.uint64)  # garbage above len in the last word included


@gpu
@pytest.mark.parametrize("k", KS)
def test_gpu_kmers_match_reference(k):
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(k)
    for n_len in _sizes(k, GPU_EXTRA):
        w = _random_words(rng, n_len)
        d = torch.from_numpy(w.view(np.int64)).cuda()
        for canonical in (False, True):
            want = np_kmers(w, n_len, k, canonical)
            assert np.array_equal(po.kmers_hip(w, n_len, k, canonical=canonical), want), (n_len, k, canonical, "host")
            got = po.kmers_dev(d, n_len, k, canonical=canonical)
            assert got.numel() == want.size
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want), (n_len, k, canonical, "device")


@gpu
def test_gpu_kmers_pointer_phases_and_edges():
    """input and output views at word offsets 0..3 (every 16-B phase pairing), garbage above len, a sentinel around and
    behind the m k-mers that must survive"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(77)
    sentinel = -0x3C3C3C3C3C3C3C3D
    lens = [32 * 40 + 17, 32 * 100, 32 * 100 + 1, 512 * 3 + 31, 512 * 5 + 32 * 3 + 5, 32 * 2048 + 19]
    top = max(lens) // 32 + 8
    w = rng.integers(0, 2**64, top, dtype=np.uint64)
    obuf = torch.empty(max(lens) + 64, dtype=torch.int64, device="cuda")
    for k in (1, 17, 31, 32):
        for canonical in (False, True):
            for n_len in lens:
                m = n_len - k + 1
                nw = (n_len + 31) // 32
                for pi in range(4):
                    src = w[pi : pi + nw].copy()
                    src[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(2 * (n_len & 31)) if n_len & 31 else np.uint64(0)
                    dsrc = torch.from_numpy(src.view(np.int64)).cuda()
                    big = torch.empty(nw + 4, dtype=torch.int64, device="cuda")
                    big[pi : pi + nw] = dsrc  # the input as a view at word offset pi
                    want = np_kmers(src, n_len, k, canonical)
                    for po_ in range(4):
                        obuf.fill_(sentinel)
                        view = obuf[8 + po_ : 8 + po_ + m + 5]
                        got = po.kmers_dev(big[pi : pi + nw], n_len, k, canonical=canonical, out=view)
                        assert got.data_ptr() == view.data_ptr()
                        o = obuf.cpu().numpy()
                        assert (o[: 8 + po_] == sentinel).all() and (o[8 + po_ + m :] == sentinel).all(), (k, n_len, pi, po_)
                        assert np.array_equal(o[8 + po_ : 8 + po_ + m].view(np.uint64), want), (k, canonical, n_len, pi, po_)


PHASE_KS = [1, 2, 16, 17, 31, 32]
SENTINEL = -0x3C3C3C3C3C3C3C3D


def _phase_lengths(head, k):
    """n_len for: no tile at all (m = head + 1023), exactly one tile after the head (and a tail), len % 32 == 0 (tile_end
    capped by 32*(words-1) below m), a tail of 0 k-mers after two tiles (m = head + 2048; the cap forbids it for some
    (head, k): then a 1-k-mer tail)"""
    T = KMERS_PER_TILE
    return [head + T - 1 + k - 1, head + T + 40 + k - 1, 32 * ((head + 2 * T + k + 31) // 32 + 1), head + 2 * T + k - 1]


@gpu
def test_gpu_kmers_every_output_phase(oracle):
    """the output at all 16 8-B phases of a 128-B line -- heads 15..0 before the tiles, and every value of a & 31 the tile
    funnel and the input resource's word reach see -- against input views at word phases 0..3, garbage above len; k in
    {1, 2, 16, 17, 31, 32}, both modes; sentinels on both sides survive; compared with the scalar oracle.  Every k-mer
    output plan occurs: no tile, one tile, the 32*(words-1) cap, a tail of 0 k-mers (k > 1: with k = 1 the cap leaves a
    tail always)."""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(1616)
    top = (3 * KMERS_PER_TILE) // 32 + 16
    w = rng.integers(0, 2**64, top, dtype=np.uint64)
    dw = torch.from_numpy(w.view(np.int64)).cuda()
    obuf = torch.empty(3 * KMERS_PER_TILE, dtype=torch.int64, device="cuda")
    assert obuf.data_ptr() % 128 == 0
    base = 16  # words: the output views start at base + phase, base on a 128-B line
    for k in PHASE_KS:
        seen = set()
        for head in range(16):
            phase = (16 - head) % 16
            for j, n_len in enumerate(_phase_lengths(head, k)):
                m = n_len - k + 1
                nw = (n_len + 31) // 32
                h, tiles, tail, _ = kmer_plan(obuf.data_ptr() + 8 * (base + phase), n_len, k)
                assert h == (head if tiles else 0)
                seen.add("none" if not tiles else "one" if tiles == 1 else "tail0" if tail == 0 else "more")
                if j == 2:  # the tiles end at the cap, below m
                    assert n_len % 32 == 0 and tiles and head + tiles * KMERS_PER_TILE <= n_len - 32 < m
                    seen.add("capped")
                for pi in range(4):
                    src = dw[pi : pi + nw]
                    for canonical in (False, True):
                        want = oracle.kmers(w[pi : pi + nw], n_len, k, canonical)
                        obuf.fill_(SENTINEL)
                        view = obuf[base + phase : base + phase + m]
                        got = po.kmers_dev(src, n_len, k, canonical=canonical, out=view)
                        assert got.data_ptr() == view.data_ptr()
                        o = obuf.cpu().numpy()
                        tag = (k, canonical, n_len, head, pi)
                        assert (o[: base + phase] == SENTINEL).all() and (o[base + phase + m :] == SENTINEL).all(), tag
                        assert np.array_equal(o[base + phase : base + phase + m].view(np.uint64), want), tag
        assert {"none", "one", "capped"} <= seen and (k == 1 or "tail0" in seen), (k, seen)


@gpu
def test_gpu_kmers_in_a_captured_graph_and_behind_a_side_stream(oracle):
    """one linear chain captured with torch.cuda.graph -- encode, forward k-mers, canonical k-mers, reverse complement,
    canonical k-mers of that -- with its kernel nodes counted (the k-mer calls' from their plans) and replayed on 3 new
    inputs against the oracle and strand symmetry; then fill -> encode -> k-mers enqueued on a side stream with no host
    sync in between"""
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import devutil, packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    n_len, k = (1 << 20) + 4133, 31
    m, words = n_len - k + 1, (n_len + 31) // 32
    d_n = torch.zeros(n_len, dtype=torch.uint8, device="cuda")
    bits = torch.empty(words, dtype=torch.int64, device="cuda")
    rc = torch.empty(words, dtype=torch.int64, device="cuda")
    obuf = torch.full((3 * m + 64,), SENTINEL, dtype=torch.int64, device="cuda")
    assert obuf.data_ptr() % 128 == 0
    s1 = -(-(m + 8) // 16) * 16 + 3  # word offsets 16a, 16b + 3, 16c + 9: heads 0, 13, 7
    s2 = -(-(s1 + m + 8) // 16) * 16 + 9
    fwd, can, can_rc = obuf[:m], obuf[s1 : s1 + m], obuf[s2 : s2 + m]
    guard = np.ones(obuf.numel(), dtype=bool)
    for s0 in (0, s1, s2):
        guard[s0 : s0 + m] = False

    def chain():
        cn.n_to_bits_dev(d_n, out=bits)
        po.kmers_dev(bits, n_len, k, out=fwd)
        po.kmers_dev(bits, n_len, k, canonical=True, out=can)
        po.reverse_complement_dev(bits, n_len, out=rc)
        po.kmers_dev(rc, n_len, k, canonical=True, out=can_rc)

    plans = [kmer_plan(v.data_ptr(), n_len, k) for v in (fwd, can, can_rc)]
    assert [p[0] for p in plans] == [0, 13, 7]
    nodes = [_kernel_nodes_of(torch, f) for f in (lambda: cn.n_to_bits_dev(d_n, out=bits),
                                                   lambda: po.kmers_dev(bits, n_len, k, out=fwd),
                                                   lambda: po.kmers_dev(bits, n_len, k, canonical=True, out=can),
                                                   lambda: po.reverse_complement_dev(bits, n_len, out=rc),
                                                   lambda: po.kmers_dev(rc, n_len, k, canonical=True, out=can_rc))]
    assert [nodes[1], nodes[2], nodes[4]] == [p[3] for p in plans]
    assert _kernel_nodes_of(torch, chain) == sum(nodes)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain()  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rng = np.random.default_rng(31)
    for rep in range(3):
        host = acgt[rng.integers(0, 4, n_len)]
        d_n.copy_(torch.from_numpy(host))
        obuf.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        hb = oracle.n_to_bits_lut(host)
        a, b = can.cpu().numpy().view(np.uint64), can_rc.cpu().numpy().view(np.uint64)
        assert np.array_equal(fwd.cpu().numpy().view(np.uint64), oracle.kmers(hb, n_len, k)), rep
        assert np.array_equal(a, oracle.kmers(hb, n_len, k, True)), rep
        assert np.array_equal(b, oracle.kmers(oracle.reverse_complement(hb, n_len), n_len, k, True)), rep
        assert np.array_equal(a, b[::-1]), rep
        o = obuf.cpu().numpy()
        assert (o[guard] == SENTINEL).all(), rep
    # a producer and its consumers on a side stream, enqueued back to back
    seed, n2 = 77, (1 << 22) + 19
    want = oracle.stream_kmers_checksum(seed, n2, 21, True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        n = torch.zeros(n2, dtype=torch.uint8, device="cuda")
        devutil.fill_random_acgt(n, seed)
        out = po.kmers_dev(cn.n_to_bits_dev(n), n2, 21, canonical=True)
    torch.cuda.current_stream().wait_stream(side)
    assert devutil.checksum_words(out) == want


@gpu
def test_gpu_kmers_host_tier_shares_staging_with_packed_ops(oracle):
    """staged cnt_kmers calls interleaved in one thread with larger and smaller cnt_complement / cnt_hamming host calls
    (all staged through DevCtx::d_aux); pageable input with a pinned output; two threads calling kmers_hip at once"""
    import threading

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(8)
    for i, (n_len, k) in enumerate((((1 << 20) + 3, 31), (1000, 5), ((1 << 22) + 77, 32), (5000, 1), ((1 << 21) + 9, 17))):
        canonical = bool(i % 2)
        w = _random_words(rng, n_len)
        want = oracle.kmers(w, n_len, k, canonical)
        got = po.kmers_hip(w, n_len, k, canonical=canonical)
        for n2 in (3 * n_len + 5, max(n_len // 7, 1)):
            a, b = _random_words(rng, n2), _random_words(rng, n2)
            assert np.array_equal(po.complement_hip(a, n2), oracle.complement(a, n2)), (i, n2)
            assert po.hamming_hip(a, b, n2) == oracle.hamming(a, b, n2), (i, n2)
            assert np.array_equal(po.kmers_hip(w, n_len, k, canonical=canonical), want), (i, n2)
        assert np.array_equal(got, want), (n_len, k, canonical)
    # pageable in, pinned out
    for n_len, k in ((32 * 4096 + 9, 31), ((1 << 20) + 3, 12)):
        m = n_len - k + 1
        w = _random_words(rng, n_len)
        out = cn.pinned_empty(m + 7, np.uint64)
        assert cn.is_pinned(out) and not cn.is_pinned(w)
        for canonical in (False, True):
            out[:] = 0xDEADBEEFDEADBEEF
            got = po.kmers_hip(w, n_len, k, canonical=canonical, out=out)
            assert np.array_equal(got, oracle.kmers(w, n_len, k, canonical)), (n_len, k, canonical)
            assert (out[m:] == 0xDEADBEEFDEADBEEF).all()
    # two threads at once, each with its own inputs and sizes
    jobs = [(_random_words(rng, n), n, k, c) for n, k, c in (((1 << 21) + 5, 27, True), ((1 << 20) + 77, 9, False))]
    wants = [oracle.kmers(*j) for j in jobs]
    errors = []

    def run(j, want):
        try:
            for _ in range(6):
                if not np.array_equal(po.kmers_hip(j[0], j[1], j[2], canonical=j[3]), want):
                    errors.append(j[1:])
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))

    threads = [threading.Thread(target=run, args=(j, want)) for j, want in zip(jobs, wants)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@gpu
def test_gpu_kmers_pinned_host_buffers():
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(5)
    for n_len, k in ((32 * 4096 + 9, 31), (1000, 17), ((1 << 20) + 3, 21)):
        m = n_len - k + 1
        bits = cn.pinned_empty((n_len + 31) // 32, np.uint64)
        bits[:] = _random_words(rng, n_len)
        out = cn.pinned_empty(m + 7, np.uint64)
        assert cn.is_pinned(bits) and cn.is_pinned(out)
        for canonical in (False, True):
            out[:] = 0xDEADBEEFDEADBEEF
            got = po.kmers_hip(bits, n_len, k, canonical=canonical, out=out)
            assert np.array_equal(got, np_kmers(bits, n_len, k, canonical)), (n_len, k, canonical)
            assert (out[m:] == 0xDEADBEEFDEADBEEF).all()
            # pinned input, pageable output (staged) agrees
            assert np.array_equal(po.kmers_hip(bits, n_len, k, canonical=canonical), got)


def _device_sequence(n_len, seed):
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import devutil

    n = torch.empty(n_len, dtype=torch.uint8, device="cuda")
    devutil.fill_random_acgt(n, seed)
    bits = cn.n_to_bits_dev(n)
    del n
    return bits


@gpu
def test_gpu_kmers_strand_symmetry():
    """canonical k-mer i of s == canonical k-mer m-1-i of revcomp(s), on the device at 2^30+5 nt"""
    import torch

    from conftest import need_free_hbm
    from cute_nucleotides_amd import packed_ops as po

    n_len, k = (1 << 30) + 5, 31
    need_free_hbm(28)
    bits = _device_sequence(n_len, 11)
    rc = po.reverse_complement_dev(bits, n_len)
    a = po.kmers_dev(bits, n_len, k, canonical=True)
    b = po.kmers_dev(rc, n_len, k, canonical=True)
    assert a.numel() == n_len - k + 1
    assert torch.equal(a, torch.flip(b, (0,)))
    # not vacuous: the canonical k-mers are not the forward ones
    assert not torch.equal(a[:2018], po.kmers_dev(bits[:64], 2048, k))


def _host_checksum(oracle, n_len, k, canonical, seed, chunk=1 << 24):
    """oracle.checksum_words of the whole expected output, chunk by chunk: chunk c holds k-mers [c*chunk, (c+1)*chunk) and
    needs nucleotides [c*chunk, (c+1)*chunk + k - 1) -- regenerated by the oracle's counter-based generator.  The checksum
    is a sum over words, so the chunks add up in any order (a few threads: numpy and the oracle release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor

    m = n_len - k + 1

    def one(first):
        mc = min(chunk, m - first)
        s = oracle.fill_random_acgt(mc + k - 1, seed, first_nt=first)
        return oracle.checksum_words(np_kmers(oracle.n_to_bits_lut(s), mc + k - 1, k, canonical), first_word=first)

    with ThreadPoolExecutor(6) as pool:
        return sum(pool.map(one, range(0, m, chunk))) & 0xFFFFFFFFFFFFFFFF


@gpu
@pytest.mark.parametrize("n_len,k,canonical", [((1 << 31) + 17, 31, True), ((1 << 32) + 33, 17, False)], ids=["2^31+17-k31-canonical", "2^32+33-k17-forward"])
def test_gpu_kmers_full_size(oracle, fullsize, n_len, k, canonical):
    """the whole output against the oracle stream checksum (the first differing chunk named on a mismatch); m > 2^32 in
    the second case (64-bit indexing); one changed word is seen"""
    import torch

    import stream_checks
    from conftest import need_free_hbm
    from cute_nucleotides_amd import packed_ops as po

    m = n_len - k + 1
    need_free_hbm((m * 8 + n_len + (n_len >> 2)) // (1 << 30) + 2)
    seed = 0x6B6D6572 + k
    bits = _device_sequence(n_len, seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = po.kmers_dev(bits, n_len, k, canonical=canonical)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    assert out.numel() == m
    fullsize(n_len.bit_length() - 1, ms, check="kmers k=%d %s: kernel" % (k, "canonical" if canonical else "forward"))
    want = stream_checks.check_kmers(out, seed, n_len, k, canonical, record=fullsize)
    stream_checks.assert_mutation_seen(out, m - 3, want)
    stream_checks.assert_mutation_seen(out, (m * 5) // 7, want)


@gpu
def test_gpu_kmers_full_size_in_two_launches(oracle, fullsize):
    """2^33 + 4133 nt, k = 32, canonical: m = 2^33 + 4102 k-mers = 8,388,612 tiles, more than one launch takes
    (8,388,544 tiles of 256 threads), so the product build's several-launch loop runs -- into one buffer at word offsets 0
    and 3 (heads 0 and 13).  Each whole output against the oracle stream checksum; one changed word in each launch's range
    (and in the head and the tail) is seen; the offset-0 call is 3 kernel nodes in a captured graph."""
    import torch

    import stream_checks
    from conftest import need_free_hbm
    from cute_nucleotides_amd import devutil, packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    n_len, k = (1 << 33) + 4133, 32
    m = n_len - k + 1
    need_free_hbm((n_len + (n_len >> 2)) // (1 << 30) + 2)  # the ASCII input and its words; freed before the output
    seed = 0x6B6D3333
    bits = _device_sequence(n_len, seed)
    need_free_hbm(((m + 3) * 8) // (1 << 30) + 2)
    obuf = torch.empty(m + 3, dtype=torch.int64, device="cuda")
    assert obuf.data_ptr() % 128 == 0
    want = None
    for off, plan in ((0, (0, KMER_HW_LAUNCH_TILES + 68, 6, 3)), (3, (13, KMER_HW_LAUNCH_TILES + 67, 1017, 4))):
        view = obuf[off : off + m]
        assert kmer_plan(view.data_ptr(), n_len, k) == plan
        head, tiles = plan[0], plan[1]
        obuf.fill_(-1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        po.kmers_dev(bits, n_len, k, canonical=True, out=view)
        torch.cuda.synchronize()
        fullsize(33, (time.perf_counter() - t0) * 1e3, check="kmers k=32 canonical, out at word %d: kernel" % off)
        want = stream_checks.check_kmers(view, seed, n_len, k, True, label="kmers k=32 canonical, out at word %d" % off,
                                         record=fullsize, want=want)
        second = head + KMER_HW_LAUNCH_TILES * KMERS_PER_TILE  # the first k-mer of the second launch
        for i in (head + 12345 * KMERS_PER_TILE + 7, second - 1, second, second + 33 * KMERS_PER_TILE + 5,
                  head + tiles * KMERS_PER_TILE - 1, m - 2) + ((head - 1,) if head else ()):
            stream_checks.assert_mutation_seen(view, i, want)
        if off == 0:
            assert _kernel_nodes_of(torch, lambda: po.kmers_dev(bits, n_len, k, canonical=True, out=view)) == plan[3]
            assert devutil.checksum_words(view) == want  # the warm-up call of the capture wrote the same values
