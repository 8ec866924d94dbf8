"""Windowed base and dinucleotide counts on packed sequences (include/cute_nt.h "windowed composition": cnt_window_counts_n,
cnt_window_counts_dev, cnt_window_counts; hip/window_count_kernels.hpp, hip/window_count_abi.inc).

CPU part: three independent references -- the definition position by position, explicit slicing of the decoded text, and a
cumulative sum of one-hot k-mer indicators -- are pinned against each other before anything is compared with the last one;
properties of the definition; every argument rule of both tiers and the query in the header's order, with canaries; aliasing of
out against bits; the Python layer; the launch plan in the sources.  GPU part: both tiers word for word against the numpy
reference at every window phase, lane-group size, the piece bound, tails, planted inputs, launch splits, pinned layouts and a
graph capture of the long-window regime."""
import collections
import ctypes
import mmap
import os

import numpy as np
import pytest

from test_aliasing import OVERLAPS, TOUCHES, Arena, homes, place
from test_find_pattern import codes_of, words_of_codes
from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch
from test_kmer_counts import reference as kmer_counts_reference
from test_kmers import assert_split_launches_by_max_tiles_per_launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = "ACTG"  # code order A0 C1 T2 G3
A, C, T, G = 0, 1, 2, 3
PIECE = 8192  # hip/window_count_kernels.hpp kWindowCountPiece: longer windows are cut into pieces that add into the record
BLOCK = 256  # kWindowCountBlock
LANE_WORDS = 8  # kWindowCountLaneWords: the words a lane of a group takes before the group grows


def n_windows(n_len, window, step):
    return (n_len - window) // step + 1 if n_len >= window else 0


# ---- the three references -----------------------------------------------------------------------------------------------------
def def_counts(codes, k, window, step):
    """the definition, per position: out[j][v] = #{ p : j*step <= p and p + k <= j*step + window and x_p == v }"""
    n = len(codes)
    out = [[0] * 4 ** k for _ in range(n_windows(n, window, step))]
    for j, rec in enumerate(out):
        for p in range(n):
            if j * step <= p and p + k <= j * step + window:
                x = int(codes[p]) if k == 1 else int(codes[p]) | (int(codes[p + 1]) << 2)
                rec[x] += 1
    return out


def text_counts(codes, k, window, step):
    """on the decoded text: each window sliced out, each of its k-letter substrings looked up among the 4^k words"""
    s = "".join(NT[c] for c in codes)
    words = [a for a in NT] if k == 1 else [a + b for b in NT for a in NT]  # value = first + 4 * second
    out = []
    for j in range(n_windows(len(s), window, step)):
        w = s[j * step : j * step + window]
        subs = [w[i : i + k] for i in range(len(w) - k + 1)]
        out.append([sum(1 for x in subs if x == word) for word in words])
    return out


def np_counts(codes, k, window, step):
    """vectorised: the cumulative sum of the one-hot indicator of each k-mer value, differenced at the window ends"""
    c = np.asarray(codes, dtype=np.int64)
    n_win = n_windows(c.size, window, step)
    out = np.zeros((n_win, 4 ** k), dtype=np.uint32)
    if n_win == 0:
        return out
    x = c if k == 1 else c[:-1] | (c[1:] << 2)
    lo = np.arange(n_win, dtype=np.int64) * step
    hi = lo + window - k + 1
    for v in range(4 ** k):
        cs = np.concatenate([[0], np.cumsum(x == v)])
        out[:, v] = cs[hi] - cs[lo]
    return out


def sample_cases():
    """a few hundred (codes, k, window, step): every short length, windows around the word size, steps below, at and above window"""
    rng = np.random.default_rng(41)
    cases = []
    for n in range(0, 40):
        for k in (1, 2):
            window = int(rng.integers(k, max(k + 1, n + 3)))
            cases.append((rng.integers(0, 4, n).astype(np.uint8), k, window, int(rng.integers(1, window + 3))))
    for _ in range(160):
        n = int(rng.integers(1, 300))
        k = int(rng.integers(1, 3))
        window = int(rng.choice([k, k + 1, 31, 32, 33, 45, 64, 65, int(rng.integers(k, n + 2))]))
        step = int(rng.choice([1, 7, 33, window, window + 5, int(rng.integers(1, 80))]))
        kind = int(rng.integers(0, 4))
        s = (rng.integers(0, 4, n), np.full(n, rng.integers(0, 4)), np.arange(n) % 2, np.where(rng.random(n) < 0.5, C, G))[kind]
        cases.append((np.asarray(s, dtype=np.uint8), k, window, step))
    return cases


def test_three_references_agree():
    cases = sample_cases()
    assert len(cases) >= 200
    some = 0
    for s, k, window, step in cases:
        d, t, v = def_counts(s, k, window, step), text_counts(s, k, window, step), np_counts(s, k, window, step)
        assert d == t and v.shape == (len(d), 4 ** k) and d == v.tolist(), (s.tolist(), k, window, step)
        some += len(d) > 1
    assert some >= 100


def test_properties(oracle):
    rng = np.random.default_rng(42)
    for s, k, window, step in sample_cases():
        got = np_counts(s, k, window, step)
        n_win = n_windows(len(s), window, step)
        assert got.shape[0] == n_win
        assert (got.sum(axis=1) == window - k + 1).all()  # a k-mer that straddles the end is not counted
        for j in range(n_win):  # the record of window j = the whole-sequence counts of its codes
            sub = s[j * step : j * step + window]
            assert np.array_equal(got[j], np_counts(sub, k, window, window)[0])
        if k == 2 and n_win:  # the table folds to the k = 1 record: over the second base, the first-base counts minus the last base
            one = np_counts(s, 1, window, step).astype(np.int64)
            last = s[np.arange(n_win) * step + window - 1]
            one[np.arange(n_win), last] -= 1
            assert np.array_equal(got.reshape(n_win, 4, 4).sum(axis=1), one)
    # window == len is the whole-sequence table of cnt_kmer_counts, from the scalar oracle's k-mers
    for n in (1, 2, 31, 32, 33, 100, 1000):
        s = rng.integers(0, 4, n).astype(np.uint8)
        for k in (1, 2):
            if n >= k:
                whole = np_counts(s, k, n, 1)
                assert whole.shape == (1, 4 ** k)
                assert np.array_equal(whole[0].astype(np.uint64), kmer_counts_reference(oracle, words_of_codes(oracle, s), n, k))
    assert np.array_equal(codes_of(pack(np.arange(70) % 4), 70), np.arange(70) % 4)


def words_for(n):
    return (n + 31) // 32


def pack(codes):
    """the encoder's layout in numpy: code i at bits 2 (i & 31) of word i >> 5, zeros behind the last code"""
    c = np.asarray(codes, dtype=np.uint64)
    padded = np.zeros(words_for(c.size) * 32, dtype=np.uint64)
    padded[: c.size] = c
    return (padded.reshape(-1, 32) << (np.uint64(2) * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


# ---- CPU: the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


def _no_device(L):
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == 0
    return count.value == 0


def test_window_count_query(L):
    from cute_nucleotides_amd import _lib

    out = ctypes.c_size_t(777)
    for n_len, k, window, step in ((0, 1, 1, 1), (9, 1, 10, 1), (10, 1, 10, 1), (10, 2, 10, 3), (11, 1, 10, 1), (100, 2, 2, 1), (100, 1, 7, 33),
                                   (1 << 36, 1, 64, 64), (1 << 36, 2, (1 << 32) - 1, 1), ((1 << 32) - 2, 2, (1 << 32) - 1, 5)):
        assert L.cnt_window_counts_n(n_len, k, window, step, ctypes.byref(out)) == _lib.CNT_OK
        assert out.value == n_windows(n_len, window, step), (n_len, k, window, step)
    # rule 1 in front of the NULL result; a refused query leaves its result alone
    out.value = 777
    for k, window, step in ((0, 10, 1), (3, 10, 1), (1, 10, 0), (1, 0, 1), (2, 1, 1), (1, 1 << 32, 1), (1, 1 << 40, 1)):
        assert L.cnt_window_counts_n(100, k, window, step, ctypes.byref(out)) == _lib.CNT_EINVAL and out.value == 777, (k, window, step)
        assert L.cnt_window_counts_n(100, k, window, step, None) == _lib.CNT_EINVAL
    assert L.cnt_window_counts_n(100, 1, 10, 1, None) == _lib.CNT_EINVAL and L.cnt_window_counts_n(5, 1, 10, 1, None) == _lib.CNT_EINVAL


def test_abi_errors_come_before_any_device_work(L):
    """the header's order: 1. shape, 2. no window, 3. pointers, 4. capacity, 5. overlap -- each rule tried with every later rule
    broken as well, both tiers, and nothing written anywhere"""
    from cute_nucleotides_amd import _lib

    FILL = 0x5A5A5A5A5A5A5A5A
    buf = np.full(4096, FILL, dtype=np.uint64)
    q = lambda word, byte=0: ctypes.c_void_p(buf.ctypes.data + 8 * word + byte)  # noqa: E731
    n_len, k, window, step = 1000, 2, 100, 50  # 32 words of input at word 100; 19 windows: 19 * 64 B = 152 words of out
    n_win = n_windows(n_len, window, step)
    assert n_win == 19
    for dev in (False, True):
        def call(bits, length, kk, w, st, flags, out, cap):
            if dev:
                return L.cnt_window_counts_dev(bits, length, kk, w, st, flags, out, cap, None)
            return L.cnt_window_counts(bits, length, kk, w, st, flags, out, cap)

        ok = (q(100), n_len, k, window, step, 0, q(1000), n_win)
        bad_later = (q(100, 3), n_len, k, window, step, 0, q(101, 1), 0)  # rules 3, 4 and 5 broken at once
        # 1. the shape
        for kk, w, st, flags in ((0, window, step, 0), (3, window, step, 0), (k, window, step, 1), (k, window, step, 0x10), (k, window, 0, 0),
                                 (2, 1, step, 0), (1, 0, step, 0), (k, 1 << 32, step, 0), (k, (1 << 32) + 5, step, 0)):
            for base in (ok, bad_later, (None, 0, k, window, step, 0, None, 0)):
                assert call(base[0], base[1], kk, w, st, flags, base[6], base[7]) == _lib.CNT_EINVAL, (dev, kk, w, st, flags)
        # 2. no window: CNT_OK whatever the pointers are
        for length in (0, 1, window - 1):
            assert call(None, length, k, window, step, 0, None, 0) == _lib.CNT_OK
            assert call(q(100, 3), length, k, window, step, 0, q(101, 1), 0) == _lib.CNT_OK
            assert call(q(100), length, k, window, step, 0, q(100), 5) == _lib.CNT_OK
        # 3. NULL or not 8-B aligned pointers, in front of the capacity
        for cap in (n_win, 0):
            assert call(None, *ok[1:7], cap) == _lib.CNT_EINVAL and call(*ok[:6], None, cap) == _lib.CNT_EINVAL
            for byte in (1, 4, 7):
                assert call(q(100, byte), *ok[1:7], cap) == _lib.CNT_EINVAL and call(*ok[:6], q(1000, byte), cap) == _lib.CNT_EINVAL
        # 4. the capacity counts records, in front of the overlap
        for cap in (0, 1, n_win - 1):
            assert call(*ok[:7], cap) == _lib.CNT_ECAP and call(*ok[:6], q(101), cap) == _lib.CNT_ECAP, (dev, cap)
        # 5. the n_win records against the 32 input words [100, 132): 152 words of out from ow; a capacity beyond n_win adds nothing
        for ow in (100, 131, 0, 90, 101):
            for cap in (n_win, n_win + 100, 1 << 40):
                assert call(*ok[:6], q(ow), cap) == _lib.CNT_EINVAL, (dev, ow, cap)
        # k = 1 records are a quarter: 38 words from ow
        for ow, rc in ((100, _lib.CNT_EINVAL), (63, _lib.CNT_EINVAL), (131, _lib.CNT_EINVAL)):
            assert call(q(100), n_len, 1, window, step, 0, q(ow), n_win) == rc
        if _no_device(L):
            # past the checks a call needs a device (with one it would run on these host pointers: only tried without)
            for ow in (132, 62, 1000):  # touching behind, touching in front (k = 1: 38 words), far
                assert call(q(100), n_len, 1, window, step, 0, q(ow), n_win) not in (_lib.CNT_OK, _lib.CNT_EINVAL, _lib.CNT_ECAP), (dev, ow)
            assert L.cnt_window_counts(*ok) == _lib.CNT_ENODEV
    assert (buf == FILL).all()  # nothing was written


def test_abi_wiring(L):
    import subprocess

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib, packed_ops as po

    names = ("cnt_window_counts_n", "cnt_window_counts_dev", "cnt_window_counts")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    hpp = open(os.path.join(ROOT, "cute_nucleotides_amd", "cute_nucleotides.hpp")).read()
    for name in names:
        assert name in exported and ("int %s(" % name) in header and ("fn %s(" % name) in rust and (name + "(") in hpp and name in _lib.SIGNATURES, name
    assert "pub fn window_counts_hip(" in rust and "pub fn window_counts_hip_dev(" in rust and "inline Vec<uint32_t> window_counts_hip(" in hpp
    assert "#define CNT_WINDOW_COUNTS_MAX_K 2" in header and "#define CNT_ABI_VERSION" in header
    # the block has a title of its own behind the device utilities, in front of the tuning comment, and names the shared-memory rules
    title = header.index("---- windowed composition on packed sequences ----")
    assert header.index("int cnt_count_mismatch_dev(") < title < header.index("int cnt_window_counts_n(") < header.index("Kernel selection for A/B runs")
    block = header[title : header.index("int cnt_window_counts_n(")]
    assert "SHARED MEMORY rules of that section apply" in block and "in this order" in block
    assert cn.window_counts_hip is po.window_counts_hip and cn.window_counts_dev is po.window_counts_dev
    assert cn.window_counts_n is po.window_counts_n and cn.gc_content_hip is po.gc_content_hip


def test_python_layer_without_a_device(L):
    """shapes, step=None and the error cases, all answered before the library needs a device"""
    from cute_nucleotides_amd import packed_ops as po

    assert po.window_counts_n(100, 1, 10) == 10 == po.window_counts_n(100, 1, 10, 10) and po.window_counts_n(100, 2, 10, 3) == 31
    assert po.window_counts_n(9, 1, 10) == 0 and po.window_counts_n(1 << 36, 2, 1000, 100) == ((1 << 36) - 1000) // 100 + 1
    w = np.zeros(2, dtype=np.uint64)
    for k in (1, 2):
        out = po.window_counts_hip(w, 5, k, 10)  # no window: answered without a device
        assert out.shape == (0, 4 ** k) and out.dtype == np.uint32
    gc = po.gc_content_hip(w, 5, 10)
    assert gc.shape == (0,) and gc.dtype == np.float64
    for fn in (lambda *a: po.window_counts_n(64, *a), lambda *a: po.window_counts_hip(w, 64, *a)):
        for bad in ((0, 10), (3, 10), (1, 0), (2, 1), (1, 1 << 32), (1, 10, 0), (1, 10, -1)):
            with pytest.raises(ValueError):
                fn(*bad)
    with pytest.raises(ValueError):
        po.gc_content_hip(w, 64, 0)
    with pytest.raises(ValueError):
        po.window_counts_hip(w, 65, 1, 10)  # longer than the words hold
    with pytest.raises(TypeError):
        po.window_counts_hip(w.astype(np.int64), 64, 1, 10)


def test_source_plan():
    src = open(os.path.join(ROOT, "hip", "window_count_kernels.hpp")).read()
    assert "constexpr int kWindowCountBlock = 256;" in src and "kWindowCountPiece = 32 * kWindowCountTileWords;  // 8192 nt" in src
    # every kernel is a plain function over a templated device body (the product's count of template kernels does not move)
    kernels = [line for line in src.splitlines() if "__global__" in line]
    assert len(kernels) == 5 and all(line.startswith("__global__ __launch_bounds__(kWindowCountBlock) void window_count_") for line in kernels)
    assert "template" not in "".join(kernels)
    for idiom in ("word_tile_pair<kWindowCountTileWords>", "funnel64(x, next, 2)", "__shfl_xor(", "__popcll(", "atomicAdd_system("):
        assert idiom in src, idiom
    assert "atomicAdd(" not in src and "__shared__ uint32_t s_sum[kWindowCountWaves][16];" in src  # no table: LDS only sums the waves
    abi = open(os.path.join(ROOT, "hip", "window_count_abi.inc")).read()
    assert abi.count("split_launches(") == 3 and abi.count("hipLaunchKernelGGL(") == 3
    assert abi.count("hipMalloc") == 0 and abi.count("Synchronize") == 0 and abi.count("hipMemset") == 0
    assert abi.index("window_count_zero") < abi.index("window_count_piece_k1")
    assert "if (window <= kWindowCountPiece) {" in abi
    assert "{bits, cnt_words_for(len) * 8, Dir::in}, {out, (n_win * 4) << (2 * k), Dir::out}" in abi and "host_call(b, 0, nullptr, false," in abi
    assert_split_launches_by_max_tiles_per_launch()
    shim = open(os.path.join(ROOT, "hip", "cute_nt.hip")).read()
    assert shim.index('#include "hpc_abi.inc"') < shim.index('#include "window_count_abi.inc"')


def plan(k, window, n_win, launch_tiles=((0x7FFFFFFF // BLOCK) // 64) * 64, cus=256):
    """(lane-group size or None, tiles of the counting kernel, kernel launches) as window_count_abi.inc plans them"""
    span = (window + 30) // 32 + 1
    if window <= PIECE:
        lanes = 1
        while lanes < 64 and LANE_WORDS * lanes < span:
            lanes *= 2
        tiles = -(-n_win // (BLOCK // lanes))
        return lanes, tiles, -(-tiles // launch_tiles)
    pieces = -(-span // BLOCK)
    per_run = min(pieces, max(1, pieces // max(1, cus * 8 // n_win)))
    tiles = n_win * -(-pieces // per_run)
    zero_tiles = -(-(n_win * 2 * 4 ** (k - 1)) // BLOCK)
    return None, tiles, -(-tiles // launch_tiles) + -(-zero_tiles // launch_tiles)


def test_plan_covers_every_lane_group():
    assert [plan(1, w, 1)[0] for w in (1, 225, 226, 481, 482, 993, 994, 2017, 2018, 4065, 4066, 8161, 8162, PIECE)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert plan(1, PIECE, 1)[0] == 64 and plan(1, PIECE + 1, 1)[0] is None
    assert plan(1, 1 << 30, 1)[1] >= 2048  # window == len is spread over the chip


# ---- CPU: aliasing ----------------------------------------------------------------------------------------------------------------
Buf = collections.namedtuple("Buf", "name bytes align written")
AliasCall = collections.namedtuple("AliasCall", "name bufs args")
ALIAS_CASES = (  # (len, k, window, step): records larger than the input, and smaller
    (100, 1, 10, 10), (100, 2, 10, 10), (1000, 1, 500, 500), (1000, 2, 999, 1))


def _alias_call(case):
    n_len, k, window, step = case
    n_win = n_windows(n_len, window, step)
    return AliasCall("window_counts", (Buf("bits", words_for(n_len) * 8, 8, False), Buf("out", n_win * 4 ** k * 4, 8, True)), case)


def _alias_run(L, dev, case, p):
    n_len, k, window, step = case
    n_win = n_windows(n_len, window, step)
    if dev:
        return L.cnt_window_counts_dev(ctypes.c_void_p(p["bits"]), n_len, k, window, step, 0, ctypes.c_void_p(p["out"]), n_win, None)
    return L.cnt_window_counts(ctypes.c_void_p(p["bits"]), n_len, k, window, step, 0, ctypes.c_void_p(p["out"]), n_win)


@pytest.mark.parametrize("case", ALIAS_CASES)
def test_out_overlapping_bits_is_refused(L, case):
    from cute_nucleotides_amd import _lib

    call = _alias_call(case)
    bits, out = call.bufs
    arena = Arena()
    home = arena.homes(call)
    assert home == homes(call, arena.base) and abs(home["out"] - home["bits"]) >= 4096  # far apart, each in the middle of its slot
    tried = collections.Counter()
    for dev in (False, True):
        for topology in OVERLAPS:
            at = place(topology, out, bits, home["bits"])
            if at is None:
                continue
            p = dict(home, out=at)
            assert at % 8 == 0 and min(at + out.bytes, home["bits"] + bits.bytes) - max(at, home["bits"]) >= 1
            assert _alias_run(L, dev, case, p) == _lib.CNT_EINVAL and arena.unchanged(), (dev, topology)
            tried[topology] += 1
    assert all(tried[t] == 2 for t in OVERLAPS[:3]) and tried[OVERLAPS[3]] + tried[OVERLAPS[4]] == 2


@pytest.mark.parametrize("case", ALIAS_CASES)
def test_out_touching_bits_is_accepted(L, case):
    """touching placements share no byte: the call gets as far as the same call with its buffers far apart.  Without a device that
    is the runtime's refusal in both tiers and nothing moves; with one, the host tier runs on these host buffers and its result
    is checked (the device tier with touching device buffers: test_gpu_touching_device_buffers)"""
    from cute_nucleotides_amd import _lib

    call = _alias_call(case)
    bits, out = call.bufs
    n_len, k, window, step = case
    no_device = _no_device(L)
    for dev in ((False, True) if no_device else (False,)):
        arena = Arena()
        home = arena.homes(call)
        far = _alias_run(L, dev, case, home)
        assert (far not in (_lib.CNT_OK, _lib.CNT_EINVAL, _lib.CNT_ECAP)) if no_device else far == _lib.CNT_OK
        for topology in TOUCHES:
            arena.view[:] = arena.fill
            p = dict(home, out=place(topology, out, bits, home["bits"]))
            assert p["out"] + out.bytes == p["bits"] or p["bits"] + bits.bytes == p["out"]
            assert _alias_run(L, dev, case, p) == far, (dev, topology)
            if no_device:
                assert arena.unchanged()
            else:
                o = p["out"] - arena.base
                words = arena.fill[home["bits"] - arena.base :][: bits.bytes].view(np.uint64)
                want = np_counts(codes_of(words, n_len), k, window, step)
                assert np.array_equal(arena.view[o : o + out.bytes].view(np.uint32).reshape(want.shape), want), topology
                changed = np.flatnonzero(arena.view != arena.fill)
                assert changed.size == 0 or (o <= changed.min() and changed.max() < o + out.bytes)


# ---------------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
CANARY = 0x3C5A3C5A  # as int32, distinguishable from zeros and from counts below 2^30
PAD = 6  # canary u32 in front of and behind the records: 24 B, so the records sit on an 8-B and not on a 16-B boundary


def input_words(s, ones=True):
    """the packed input with every bit beyond len set (the last word's tail and two more words): none of them may reach a count"""
    n = len(s)
    w = np.concatenate([pack(s), np.zeros(2, dtype=np.uint64)])
    if ones:
        if n & 31:
            w[(n - 1) >> 5] |= np.uint64((2**64 - 1) >> (2 * (n & 31)) << (2 * (n & 31)))
        w[words_for(n) :] = np.uint64(2**64 - 1)
    return w


class Ref:
    """np_counts of one sequence, computed once per (k, window, step) and shared"""

    def __init__(self, s):
        self.s, self.memo = np.asarray(s, dtype=np.uint8), {}

    def __call__(self, k, window, step):
        key = (k, window, step)
        if key not in self.memo:
            self.memo[key] = np_counts(self.s, k, window, step)
            self.memo[key].setflags(write=False)
        return self.memo[key]


def check_dev(ref, k, window, step=None, in_phase=1, tag=()):
    """the device tier through the Python wrapper: the records word for word, canaries in front of and behind them"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    s = ref.s
    n_len = len(s)
    want = ref(k, window, window if step is None else step)
    n_win, bins = want.shape
    d_in = torch.from_numpy(np.concatenate([np.full(in_phase, 0x1234567890ABCDEF, dtype=np.uint64), input_words(s)]).view(np.int64)).cuda()
    d_out = torch.full((PAD + n_win * bins + PAD,), CANARY, dtype=torch.int32, device="cuda")
    got = po.window_counts_dev(d_in[in_phase : in_phase + max(words_for(n_len), 1)], n_len, k, window, step, out=d_out[PAD : PAD + n_win * bins])
    torch.cuda.synchronize()
    tag = tag + (n_len, k, window, step, in_phase)
    assert got.shape == (n_win, bins) and got.dtype == torch.int32
    h = d_out.cpu().numpy()
    assert (h[:PAD] == CANARY).all() and (h[PAD + n_win * bins :] == CANARY).all(), tag + ("canary",)
    rec = h[PAD : PAD + n_win * bins].view(np.uint32).reshape(n_win, bins)
    assert np.array_equal(rec, want), tag + (np.argwhere(rec != want)[:4].tolist(),)
    return n_win


def check_host(L, ref, k, window, step=None, pinned=False, tag=()):
    """the host tier through the C ABI, pageable or pinned buffers at a phase inside their allocations"""
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    s = ref.s
    n_len = len(s)
    step = window if step is None else step
    want = ref(k, window, step)
    n_win, bins = want.shape
    words = input_words(s)
    alloc = (lambda n, dt: cn.pinned_empty(n, dt)) if pinned else (lambda n, dt: np.empty(n, dtype=dt))
    bits = alloc(words.size + 3, np.uint64)[3:]
    bits[:] = words
    out = alloc(PAD + n_win * bins + PAD, np.uint32)
    out[:] = CANARY
    rc = L.cnt_window_counts(bits.ctypes.data, n_len, k, window, step, 0, out[PAD:].ctypes.data, n_win)
    tag = tag + (n_len, k, window, step, pinned)
    assert rc == _lib.CNT_OK, tag + (rc,)
    assert (out[:PAD] == CANARY).all() and (out[PAD + n_win * bins :] == CANARY).all(), tag + ("canary",)
    assert np.array_equal(out[PAD : PAD + n_win * bins].reshape(n_win, bins), want), tag
    return n_win


def check_both(L, ref, k, window, step=None, **kw):
    check_dev(ref, k, window, step, **kw)
    return check_host(L, ref, k, window, step, tag=kw.get("tag", ()))


@pytest.fixture(scope="module")
def seqs():
    """the sequences the GPU tests share, each with its memo of references"""
    rng = np.random.default_rng(43)
    out = {"r%d" % n: Ref(rng.integers(0, 4, n)) for n in (32, 33, 63, 1000, 4096 + 31, 40000, 70001)}
    out["big"] = Ref(rng.integers(0, 4, (1 << 20) + 17))
    return out


@gpu
def test_gpu_every_window_phase_both_tiers(L, seqs):
    """steps coprime with 32 walk the window start through all 2-bit phases of a word; windows of k, k + 1 and around one and two
    words; every bit beyond len set; a first window in word 0 and a last one that ends in the last word"""
    for name in ("r1000", "r4127"):
        ref = seqs[name]
        for k in (1, 2):
            for step in (7, 33):
                for window in (k, k + 1, 31, 32, 33, 45, 64, 65):
                    n_win = check_both(L, ref, k, window, step, tag=(name,))
                    assert n_win >= 29 and ((n_win - 1) * step + window - 1) // 32 >= words_for(len(ref.s)) - 2


@gpu
def test_gpu_gaps_overlap_and_adjacent_windows(L, seqs):
    ref = seqs["r40000"]
    for k in (1, 2):
        for window, step in ((50, 1), (1000, 100), (64, 64), (1000, 1000), (40, 97), (3000, 4001), (5000, 1)):
            check_dev(ref, k, window, step)
        check_host(L, ref, k, 1000, 100)
        check_host(L, ref, k, 40, 97)
    assert check_dev(seqs["big"], 1, 64, 64) == ((1 << 20) + 17) // 64
    check_dev(seqs["big"], 2, 1000, 100)
    check_host(L, seqs["big"], 2, 1024)


@gpu
def test_gpu_every_lane_group_size(L, seqs):
    """a window can span (window + 30) // 32 + 1 words; at each power of two of that from 1 to 256, one word below and one above:
    every lane-group size L (a lane takes 8 words before the group grows: L changes behind 8, 16, ... 256 words), its last window
    length and the first of the next; steps that move the phase"""
    ref = seqs["r70001"]
    seen = set()
    for span in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        for window in {max(1, 32 * (span - 1) - 30), 32 * (span - 1) + 1}:  # the shortest and the longest window of this span
            if window > PIECE:
                continue
            seen.add(plan(1, window, 1)[0])
            for k in (1, 2):
                if window >= k:  # one lane per window is k = 1 with window = 1 alone
                    check_dev(ref, k, window, 37 if window < 2000 else 1237, in_phase=k - 1, tag=(span,))
        check_host(L, ref, min(span, 2), min(32 * (span - 1) + 1, PIECE), 997, tag=(span,))
    assert seen == {1, 2, 4, 8, 16, 32, 64}


@gpu
def test_gpu_the_piece_bound_and_long_windows(L, seqs):
    """window at the bound - 1, at it and one above (the last window of the lane groups, the first of the pieces); windows of
    several pieces at every phase; window == len for a len of several pieces that is no multiple of 32"""
    ref = seqs["r70001"]
    for k in (1, 2):
        for window in (PIECE - 1, PIECE, PIECE + 1):
            check_both(L, ref, k, window, 1013)
            check_dev(ref, k, window, window)
        for window, step in ((PIECE + 31, 1), (2 * PIECE, 33), (2 * PIECE + 1, 4099), (3 * PIECE + 77, 7777), (60000, 5000)):
            check_dev(ref, k, window, step)
        assert check_both(L, ref, k, 70001) == 1  # window == len: 8.5 pieces, len % 32 == 17
        assert check_dev(seqs["big"], k, (1 << 20) + 17) == 1
        check_dev(seqs["big"], k, 300000, 100001)
    assert plan(1, (1 << 20) + 17, 1)[1] > 64  # more than one workgroup, let alone one wave


@gpu
def test_gpu_tails_beyond_len(L):
    """len % 32 in {0, 1, 31} with the last window ending exactly at len and every bit beyond len set: the k = 2 counts must not
    see the position behind the last base; a sequence of one word; short and long windows"""
    rng = np.random.default_rng(44)
    for n_len in (32, 33, 63, 64, 65, 95, 3 * PIECE, 3 * PIECE + 1, 3 * PIECE + 31):
        ref = Ref(rng.integers(0, 4, n_len))
        for k in (1, 2):
            for window, step in ((n_len, 1), (k, 1), (31, 1), (n_len - 1, 1), (min(n_len, 20), n_len - min(n_len, 20) or 1)):
                n_win = check_both(L, ref, k, window, step, in_phase=n_len & 1)
                assert (n_win - 1) * step + window == n_len  # the last window ends at len
            if n_len > 2 * PIECE:
                assert check_both(L, ref, k, PIECE + 5, n_len - PIECE - 5) == 2
    for n_len in (1, 2, 5, 31, 32):  # one word
        ref = Ref(rng.integers(0, 4, n_len))
        for k in (1, 2):
            for window in range(k, n_len + 1, 3):
                check_both(L, ref, k, window, 1)


@gpu
def test_gpu_planted_extremes(L):
    """all-A (every count in one class), ACAC... (two classes, two dinucleotides), and a CG-only block that ends exactly at a
    window edge, begins one base in front of another and straddles a third"""
    n_len = 5 * PIECE + 77
    rng = np.random.default_rng(45)
    block = rng.integers(0, 2, n_len).astype(np.uint8) * 2  # {A, T} background
    block[1000:2000] = np.where(rng.random(1000) < 0.5, C, G)
    block[3 * PIECE - 1 : 3 * PIECE + 500] = np.where(rng.random(501) < 0.5, C, G)
    for name, s in (("all A", np.full(n_len, A)), ("all G", np.full(n_len, G)), ("ACAC", np.arange(n_len) % 2), ("CG block", block)):
        ref = Ref(s)
        for k in (1, 2):
            for window, step in ((1000, 1000), (500, 250), (64, 64), (PIECE, PIECE), (3 * PIECE, PIECE), (n_len, 1)):
                check_dev(ref, k, window, step, tag=(name,))
            check_host(L, ref, k, 1000, 1000, tag=(name,))
        one = ref(1, 1000, 1000)
        if name == "all A":
            assert (one[:, A] == 1000).all() and (ref(2, 1000, 1000)[:, 0] == 999).all()
        if name == "ACAC":
            assert (one[:, A] == 500).all() and (one[:, C] == 500).all() and set(np.flatnonzero(ref(2, 64, 64).sum(axis=0))) == {A | C << 2, C | A << 2}
        if name == "CG block":
            assert one[1, C] + one[1, G] == 1000 and one[0, C] + one[0, G] == 0 and one[2, C] + one[2, G] == 0


@gpu
def test_gpu_python_layer(seqs):
    """the host wrappers on the real library: shapes, step=None, gc_content_hip against the reference"""
    from cute_nucleotides_amd import packed_ops as po

    ref = seqs["r40000"]
    bits, n_len = pack(ref.s), len(ref.s)
    for k in (1, 2):
        got = po.window_counts_hip(bits, n_len, k, 1000)
        assert got.shape == (40, 4 ** k) and got.dtype == np.uint32 and np.array_equal(got, ref(k, 1000, 1000))
        assert np.array_equal(po.window_counts_hip(bits, n_len, k, 1000, 100), ref(k, 1000, 100))
        assert po.window_counts_n(n_len, k, 1000, 100) == ref(k, 1000, 100).shape[0]
    one = ref(1, 1000, 100).astype(np.float64)
    gc = po.gc_content_hip(bits, n_len, 1000, 100)
    assert gc.dtype == np.float64 and np.array_equal(gc, (one[:, C] + one[:, G]) / 1000) and 0.4 < gc.mean() < 0.6
    import torch

    d = torch.from_numpy(bits.view(np.int64)).cuda()
    fresh = po.window_counts_dev(d, n_len, 2, 1000)  # step=None, no out
    assert fresh.shape == (40, 16) and np.array_equal(fresh.cpu().numpy().view(np.uint32), ref(2, 1000, 1000))
    with pytest.raises(ValueError):
        po.window_counts_dev(d, n_len, 1, 1000, out=torch.empty(159, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        po.window_counts_dev(d, n_len, 1, 1000, out=torch.empty(160, dtype=torch.int64, device="cuda"))


@gpu
def test_gpu_several_launches(launch_tiles, seqs):
    """the lab build cut into launches of 64 / 128 tiles: the lane-group kernel and the zeroing + piece kernels each in more than
    two launches, counted in a captured graph"""
    import torch

    from cute_nucleotides_amd import _lib, packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    cus = ctypes.c_int(0)
    assert _lib.lib().cnt_chip_info(0, ctypes.byref(cus), None, None) == 0
    ref = seqs["r70001"]
    n_len = len(ref.s)
    d = torch.from_numpy(pack(ref.s).view(np.int64)).cuda()
    for k, window, step in ((1, 45, 1), (2, 64, 1), (1, 4096, 16), (2, 3000, 10), (1, PIECE, 16), (1, PIECE + 1, 61), (2, 3 * PIECE, 97)):
        n_win = check_dev(ref, k, window, step, tag=(launch_tiles,))
        _, tiles, launches = plan(k, window, n_win, launch_tiles, cus.value)
        assert tiles > 2 * launch_tiles and launches >= 3, (k, window, step, tiles)
        out = torch.empty(n_win * 4 ** k, dtype=torch.int32, device="cuda")
        assert _kernel_nodes_of(torch, lambda: po.window_counts_dev(d, n_len, k, window, step, out=out)) == launches, (k, window, step)


@gpu
def test_gpu_host_tier_pinned_layouts(L, seqs):
    """pinned input and output in place (plain stores and, for long windows, the adds go over the link), pageable ones staged, and an
    output that starts in a registered range and leaves it"""
    ref = seqs["r40000"]
    for k in (1, 2):
        for window, step in ((1000, 100), (64, 64), (PIECE + 100, 3000), (40000, 1)):
            for pinned in (False, True):
                check_host(L, ref, k, window, step, pinned=pinned)
    page = mmap.PAGESIZE
    arena = mmap.mmap(-1, 2 * page + (1 << 16))
    raw = np.frombuffer(arena, dtype=np.uint8)
    base = raw.ctypes.data
    assert base % page == 0 and L.cnt_host_register(ctypes.c_void_p(base), 2 * page) == 0
    try:
        for k, window, step in ((2, 64, 64), (1, PIECE + 100, 10)):
            want = ref(k, window, step)
            nbytes = want.size * 4
            assert 1024 < nbytes < (1 << 16) - 1024
            raw[:] = 0xC3
            start = 2 * page - 1024  # the records begin 1 KiB in front of the registration's end
            assert L.cnt_host_is_pinned(ctypes.c_void_p(base + start), 1024) == 1 and L.cnt_host_is_pinned(ctypes.c_void_p(base + start), nbytes) == 0
            bits = pack(ref.s)
            assert L.cnt_window_counts(bits.ctypes.data, len(ref.s), k, window, step, 0, ctypes.c_void_p(base + start), want.shape[0]) == 0
            assert np.array_equal(raw[start : start + nbytes].view(np.uint32).reshape(want.shape), want)
            assert (raw[:start] == 0xC3).all() and (raw[start + nbytes :] == 0xC3).all()
    finally:
        assert L.cnt_host_unregister(ctypes.c_void_p(base)) == 0
        del raw


@gpu
def test_gpu_no_window_touches_nothing(L):
    """n_win == 0 with garbage pointers, device tier: CNT_OK, and a stream that is still healthy afterwards"""
    import torch

    from cute_nucleotides_amd import _lib

    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n_len, k, window in ((0, 1, 1), (9, 2, 10), (1 << 20, 1, (1 << 20) + 1)):
        assert L.cnt_window_counts_dev(ctypes.c_void_p(0xDEAD0001), n_len, k, window, 1, 0, ctypes.c_void_p(0xBEEF0003), 0, s) == _lib.CNT_OK
        assert L.cnt_window_counts(ctypes.c_void_p(0xDEAD0001), n_len, k, window, 1, 0, ctypes.c_void_p(0xBEEF0003), 0) == _lib.CNT_OK
    torch.cuda.synchronize()
    assert int(torch.ones(4, device="cuda").sum().item()) == 4


@gpu
@pytest.mark.parametrize("order", ["in|out", "out|in"])
def test_gpu_touching_device_buffers(order, seqs):
    """out right behind bits and right in front of it in one allocation: accepted, right, and the input words as they were"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    ref = seqs["r1000"]
    n_len, nw = 1000, words_for(1000)
    for k, window, step in ((1, 100, 50), (2, 64, 7)):
        want = ref(k, window, step)
        ow = want.size // 2  # 8-B words of the records
        whole = torch.full((nw + ow + 2,), -1, dtype=torch.int64, device="cuda")
        lo_in = 1 if order == "in|out" else 1 + ow
        lo_out = 1 + nw if order == "in|out" else 1
        words = torch.from_numpy(pack(ref.s).view(np.int64)).cuda()
        whole[lo_in : lo_in + nw] = words
        got = po.window_counts_dev(whole[lo_in : lo_in + nw], n_len, k, window, step, out=whole[lo_out : lo_out + ow].view(torch.int32))
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want), (order, k)
        assert torch.equal(whole[lo_in : lo_in + nw], words) and int(whole[0]) == -1 and int(whole[-1]) == -1


@gpu
def test_gpu_long_windows_in_a_captured_graph(seqs):
    """one capture of a long-window call (zeroing kernel + pieces), replayed once onto a poisoned output and changed input"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(46)
    n_len, k, window, step = 70001, 2, 2 * PIECE + 5, 3001
    n_win = n_windows(n_len, window, step)
    bits = torch.zeros(words_for(n_len), dtype=torch.int64, device="cuda")
    out = torch.zeros(PAD + n_win * 16 + PAD, dtype=torch.int32, device="cuda")
    call = lambda: po.window_counts_dev(bits, n_len, k, window, step, out=out[PAD : PAD + n_win * 16])  # noqa: E731
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()  # module load outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    s = rng.integers(0, 4, n_len).astype(np.uint8)
    bits.copy_(torch.from_numpy(pack(s).view(np.int64)))
    out.fill_(CANARY)
    g.replay()
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:PAD] == CANARY).all() and (h[PAD + n_win * 16 :] == CANARY).all()
    assert np.array_equal(h[PAD : PAD + n_win * 16].view(np.uint32).reshape(n_win, 16), np_counts(s, k, window, step))
