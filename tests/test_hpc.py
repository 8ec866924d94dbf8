"""Homopolymer compression on packed sequences (include/cute_nt.h "homopolymer compression", hip/hpc_kernels.hpp, hip/hpc_abi.inc):
every run of equal bases collapses to one base, the result is a packed sequence again, and the position each run started at is
reported beside it.  Not in the reference: the definition is restated here three ways -- per base as a scalar loop, on the text
with itertools.groupby, and vectorised in numpy -- and the three are pinned against each other before the library is compared
with the last one.

CPU part: the references, the properties of the definition, every argument rule of both tiers in the order the header states
them (all of them precede device work), the scratch query, the launch plan in the source, and the Python layer.  GPU part: both
tiers word for word and entry for entry against the numpy reference, with canaries around every footprint."""
import ctypes
import itertools
import math
import os
import types

import numpy as np
import pytest

from test_find_pattern import codes_of, words_of_codes
from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch
from test_kmers import assert_split_launches_by_max_tiles_per_launch
from test_minimizers import assert_counted_output_source, np_minimizers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 8192  # positions per workgroup tile (hip/hpc_kernels.hpp kHpcTile)
NT = "ACTG"  # code order A0 C1 T2 G3
CNT_KMER_CANONICAL = 0x10
A, C, T, G = 0, 1, 2, 3


# ---- the three references -----------------------------------------------------------------------------------------------------
def def_hpc(codes):
    """the definition, per base: position i is kept iff i == 0 or x_i != x_{i-1}"""
    out, pos = [], []
    for i in range(len(codes)):
        if i == 0 or codes[i] != codes[i - 1]:
            out.append(int(codes[i]))
            pos.append(i)
    return out, pos


def text_hpc(codes):
    """on the text: decode, group equal letters, encode; the positions from the group lengths"""
    s = "".join(NT[c] for c in codes)
    out, pos, at = [], [], 0
    for ch, grp in itertools.groupby(s):
        out.append(NT.index(ch))
        pos.append(at)
        at += len(list(grp))
    return out, pos


def np_hpc(codes):
    """vectorised: (run bases as uint8, run starts as uint64)"""
    c = np.asarray(codes, dtype=np.uint8)
    if c.size == 0:
        return c, np.zeros(0, dtype=np.uint64)
    keep = np.r_[True, c[1:] != c[:-1]]
    return c[keep], np.flatnonzero(keep).astype(np.uint64)


def words_for(n):
    return (n + 31) // 32


def pack(codes):
    """the encoder's layout in numpy: code i at bits 2 (i & 31) of word i >> 5, zeros behind the last code"""
    c = np.asarray(codes, dtype=np.uint64)
    padded = np.zeros(words_for(c.size) * 32, dtype=np.uint64)
    padded[: c.size] = c
    return (padded.reshape(-1, 32) << (np.uint64(2) * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


def run_lengths_seq(rng, n_len, mean_run, alphabet=4):
    """codes of n_len positions whose runs have geometric lengths of the given mean"""
    n_runs = max(int(2 * n_len / mean_run) + 8, 8)
    lens = rng.geometric(1.0 / mean_run, n_runs) if mean_run > 1 else np.ones(n_runs, dtype=np.int64)
    base = np.cumsum(rng.integers(1, alphabet, n_runs)) % alphabet  # a neighbour never repeats
    s = np.repeat(base, lens)[:n_len].astype(np.uint8)
    assert s.size == n_len
    return s


def sample_sequences():
    """a few hundred random and planted sequences: short ones of every length, runs of every length scale, two-letter ones"""
    rng = np.random.default_rng(11)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in range(0, 70)]
    seqs += [run_lengths_seq(rng, int(rng.integers(1, 400)), float(rng.choice([1, 1.3, 2, 5, 40, 300]))) for _ in range(180)]
    seqs += [(rng.random(int(rng.integers(1, 300))) < 0.1).astype(np.uint8) for _ in range(40)]  # {A, C} at P(A) = 0.9
    seqs += [np.full(n, c, dtype=np.uint8) for n in (1, 2, 33, 100) for c in range(4)]
    seqs += [np.arange(n, dtype=np.uint8) % 2 for n in (1, 2, 31, 32, 33, 65)] + [np.arange(n, dtype=np.uint8) % 3 for n in (3, 64, 97)]
    return seqs


def test_three_references_agree(oracle):
    seqs = sample_sequences()
    assert len(seqs) >= 300
    for s in seqs:
        d, t, v = def_hpc(s), text_hpc(s), np_hpc(s)
        assert d == t and d[0] == v[0].tolist() and d[1] == v[1].tolist(), s.tolist()
    # and the test's own packing is the encoder's
    rng = np.random.default_rng(12)
    for n in (0, 1, 31, 32, 33, 64, 1000):
        s = rng.integers(0, 4, n).astype(np.uint8)
        assert np.array_equal(pack(s), words_of_codes(oracle, s)[: words_for(n)]) and np.array_equal(codes_of(pack(s), n), s), n


def test_properties():
    for s in sample_sequences():
        out, pos = np_hpc(s)
        n = out.size
        assert n <= s.size and (n >= 1) == (s.size >= 1)
        assert (out[1:] != out[:-1]).all()  # no two adjacent codes of the output are equal
        again, pos2 = np_hpc(out)  # idempotent
        assert np.array_equal(again, out) and np.array_equal(pos2, np.arange(n, dtype=np.uint64))
        lens = np.diff(np.r_[pos, np.uint64(s.size)].astype(np.int64))
        assert (lens >= 1).all() and np.array_equal(np.repeat(out, lens), s)  # the run lengths from pos give the input back
        assert (n == s.size) == bool((s[1:] != s[:-1]).all())
        if s.size and (s == s[0]).all():
            assert n == 1 and pos.tolist() == [0]


# ---- CPU: the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


def _work_bytes(L, n_len):
    out = ctypes.c_size_t(12345)
    assert L.cnt_hpc_work_bytes(n_len, ctypes.byref(out)) == 0
    return out.value


def test_work_bytes_query(L):
    from cute_nucleotides_amd import _lib
    from cute_nucleotides_amd import packed_ops as po

    assert _work_bytes(L, 0) == 0 == po.hpc_work_bytes(0)
    assert _work_bytes(L, 1) == 16 + 2 * 8 + 16 * 4  # one tile: one group of 16 tiles
    last = 0
    for n_len in (1, TILE - 1, TILE, TILE + 1, 5 * TILE, 16 * TILE - 1, 16 * TILE, 16 * TILE + 1, 33 * 16 * TILE, (1 << 32) + 1, 1 << 36):
        tiles = -(-n_len // TILE)
        groups = -(-tiles // 16)
        want = 16 + (groups + groups % 2) * 8 + groups * 16 * 4  # hip/counted_output.hpp counted_scratch_bytes
        assert _work_bytes(L, n_len) == want == po.hpc_work_bytes(n_len), n_len
        assert want >= last  # monotone
        last = want
    assert _work_bytes(L, 16 * TILE) < _work_bytes(L, 16 * TILE + 1)  # it changes at a tile edge: tile 17 opens a group
    assert (1 << 36) // 4096 < last < (1 << 36) // 1024  # 2^36 nt: tens of MiB, no overflow
    assert L.cnt_hpc_work_bytes(100, None) == _lib.CNT_EINVAL and L.cnt_hpc_work_bytes(0, None) == _lib.CNT_EINVAL


def test_abi_errors_come_before_any_device_work(L):
    from cute_nucleotides_amd import _lib

    FILL = 0x5A5A5A5A5A5A5A5A
    buf = np.zeros(4096, dtype=np.uint64)
    q = lambda word, byte=0: ctypes.c_void_p(buf.ctypes.data + 8 * word + byte)  # noqa: E731
    out = np.full(4096, FILL, dtype=np.uint64)
    o = lambda word, byte=0: ctypes.c_void_p(out.ctypes.data + 8 * word + byte)  # noqa: E731
    cnt = np.full(2, FILL, dtype=np.uint64)
    c = lambda byte=0: ctypes.c_void_p(cnt.ctypes.data + byte)  # noqa: E731
    work = q(3000)
    n_len = 1000  # 32 words of input; at out_cap 640: a footprint of 20 words of out, 640 entries of pos
    need = _work_bytes(L, n_len)
    assert need == 96
    for dev in (False, True):
        def call(bits, length, flags, po_out, pos, cap, count, work_bytes=need, wk=work):
            if dev:
                return L.cnt_hpc_dev(bits, length, flags, po_out, pos, cap, count, wk, work_bytes, None)
            return L.cnt_hpc(bits, length, flags, po_out, pos, cap, count)

        tag = "dev" if dev else "host"
        ok = (q(100), n_len, 0, o(0), o(100), 640, c())
        # 1. a non-zero flag, even without work
        for flags in (0x1, 0x2, 0x100, 0x200, 0x80000000):
            assert call(*ok[:2], flags, *ok[3:]) == _lib.CNT_EINVAL, (tag, flags)
            assert call(None, 0, flags, None, None, 0, None) == _lib.CNT_EINVAL, (tag, flags)
            assert call(q(100), 0, flags, o(0), o(100), 640, c()) == _lib.CNT_EINVAL, (tag, flags)
        # 2. len == 0: CNT_OK whatever else is passed; the host count is set to 0 and nothing else is touched
        assert call(None, 0, 0, None, None, 0, None, 0, None) == _lib.CNT_OK
        assert call(q(100, 3), 0, 0, q(100, 1), q(100, 5), 640, None, 0, None) == _lib.CNT_OK  # rule 3 is not reached
        if not dev:
            cnt[0] = 99
            assert call(q(100), 0, 0, o(0), o(100), 640, c()) == _lib.CNT_OK and cnt[0] == 0 and cnt[1] == FILL
            cnt[0] = FILL
        # 3. NULL bits, out or count (pos may be NULL: that is past the checks, and needs a device)
        assert call(None, *ok[1:]) == _lib.CNT_EINVAL
        assert call(*ok[:3], None, *ok[4:]) == _lib.CNT_EINVAL
        assert call(*ok[:6], None) == _lib.CNT_EINVAL
        for byte in (1, 4, 7):  # not 8-B aligned
            assert call(q(100, byte), *ok[1:]) == _lib.CNT_EINVAL
            assert call(*ok[:3], o(0, byte), *ok[4:]) == _lib.CNT_EINVAL
            assert call(*ok[:4], o(100, byte), *ok[5:]) == _lib.CNT_EINVAL
            assert call(*ok[:6], c(byte)) == _lib.CNT_EINVAL
        # overlaps, on the FOOTPRINT: the input is words [100, 132) of buf; at out_cap 640 out takes 20 words and pos 640
        for ow in (100, 131, 81, 90, 120):  # out: 20 words from ow
            assert call(q(100), n_len, 0, q(ow), o(100), 640, c()) == _lib.CNT_EINVAL, (tag, "out", ow)
        for pw in (100, 131, 0, 50):  # pos: 640 entries from pw
            assert call(q(100), n_len, 0, o(0), q(pw), 640, c()) == _lib.CNT_EINVAL, (tag, "pos", pw)
        for pw in (0, 19):  # pos against out's 20 words at o(0), and out inside pos
            assert call(q(100), n_len, 0, o(0), o(pw), 640, c()) == _lib.CNT_EINVAL, (tag, "pos/out", pw)
        assert call(q(100), n_len, 0, o(639), o(0), 640, c()) == _lib.CNT_EINVAL
        # the footprint follows min(len, out_cap), not the result and not the raw capacity: at out_cap 33 out is two words, and
        # from word 99 on they reach the input; 33 entries of pos from word 68 on do too
        assert call(q(100), n_len, 0, q(99), o(100), 33, c()) == _lib.CNT_EINVAL
        assert call(q(100), n_len, 0, o(0), q(68), 33, c()) == _lib.CNT_EINVAL
        if not dev:
            # ... while neighbours that touch nothing pass the checks (the host tier then runs, or finds no device): 20 words of out
            # right in front of the input and right behind it, at out_cap 32 one word of out and 32 entries of pos beside it, and
            # at capacity 0 no footprint at all
            c2 = ctypes.c_uint64(0)
            for args in ((q(80), None, 640), (q(132), None, 640), (q(99), q(132), 32), (q(132), q(68), 32), (q(131), q(100), 0)):
                assert call(q(100), n_len, 0, *args, ctypes.byref(c2)) != _lib.CNT_EINVAL, args[2]
        assert call(q(100), n_len, 0, o(0), o(1), 1 << 40, c()) == _lib.CNT_EINVAL  # a huge capacity is clipped to len: 32 words of out over pos
        if dev:
            assert call(*ok, work_bytes=need - 1) == _lib.CNT_EINVAL  # scratch below the query
            assert call(*ok, work_bytes=0) == _lib.CNT_EINVAL
            assert call(*ok, wk=None) == _lib.CNT_EINVAL
    assert (out == FILL).all() and (cnt == FILL).all()  # nothing was written
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        assert L.cnt_hpc(q(100), n_len, 0, o(0), o(100), 640, c()) == _lib.CNT_ENODEV
        assert L.cnt_hpc(q(100), n_len, 0, q(131), None, 0, c()) == _lib.CNT_ENODEV  # capacity 0: out may sit anywhere
        assert L.cnt_hpc_dev(q(100), n_len, 0, o(0), None, 640, c(), work, need, None) < 0
        assert (out == FILL).all()


def test_abi_wiring(L):
    import subprocess

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib, packed_ops as po

    names = ("cnt_hpc", "cnt_hpc_dev", "cnt_hpc_work_bytes")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    hpp = open(os.path.join(ROOT, "cute_nucleotides_amd", "cute_nucleotides.hpp")).read()
    for name in names:
        assert name in exported and ("int %s(" % name) in header and ("fn %s(" % name) in rust and (name + "(") in hpp, name
    assert "pub fn hpc_hip(" in rust and "inline Hpc hpc_hip(" in hpp
    assert cn.hpc_hip is po.hpc_hip and cn.hpc_dev is po.hpc_dev and cn.hpc_work_bytes is po.hpc_work_bytes and cn.hpc_minimizers_hip is po.hpc_minimizers_hip
    assert "#define CNT_ABI_VERSION" in header  # symbols were only added: the version did not move
    w = np.zeros(2, dtype=np.uint64)
    with pytest.raises(ValueError):
        po.hpc_hip(w, 65)  # longer than the words hold
    with pytest.raises(TypeError):
        po.hpc_hip(w.astype(np.int64), 64)
    out, n = po.hpc_hip(w, 0)  # nothing to compress: answered without a device
    assert out.size == 0 and n == 0
    out, n, pos = po.hpc_hip(w, 0, with_pos=True)
    assert out.size == 0 and n == 0 and pos.size == 0 and pos.dtype == np.uint64
    with pytest.raises(ValueError):
        po.hpc_minimizers_hip(w, 64, 15, 10, flags=2)


def test_hpc_plan_matches_the_launcher_and_splitter_source():
    src = open(os.path.join(ROOT, "hip", "hpc_kernels.hpp")).read()
    assert "constexpr int kHpcBlock = 256;" in src and "kHpcTileWords = kHpcBlock, kHpcTile = 32 * kHpcTileWords;" in src
    # every kernel is a plain function (the product's count of template kernels does not move)
    kernels = [line for line in src.splitlines() if "__global__" in line]
    assert len(kernels) == 4 and all(line.startswith("__global__ __launch_bounds__(kHpcBlock) void hpc_") for line in kernels)
    assert "template" not in "".join(kernels)
    abi = open(os.path.join(ROOT, "hip", "hpc_abi.inc")).read()
    scan = "counted_scan_enqueue(work, n_tiles, d_count, s);"
    empty = "if (len == 0) return counted_empty_dev(d_count, s);"
    for line in (scan, empty, "const CountedScratch work = counted_carve(d_work, n_tiles);",
                 "uint64_t hpc_tiles(size_t len) { return ((uint64_t)len + kHpcTile - 1) / kHpcTile; }"):
        assert line in abi, line
    tiles = "split_launches(n_tiles, kHpcBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(%s, dim3((unsigned)n), dim3(kHpcBlock), 0, s, a, t); });"
    zero = "split_launches((n_tiles + kHpcBlock - 1) / kHpcBlock, kHpcBlock,"
    assert abi.count("split_launches(n_tiles, kHpcBlock") == 2 and abi.count("split_launches(") == 3 and abi.count("counted_scan_enqueue(") == 1
    assert abi.count("hipLaunchKernelGGL(") == 3 and abi.count("hipMalloc") == 0 and abi.count("Synchronize") == 0
    assert abi.index(empty) < abi.index(tiles % "hpc_count") < abi.index(scan) < abi.index(zero) < abi.index(tiles % "write")
    assert_counted_output_source()
    assert_split_launches_by_max_tiles_per_launch()
    shim = open(os.path.join(ROOT, "hip", "cute_nt.hip")).read()
    assert shim.index('#include "orf_abi.inc"') < shim.index('#include "hpc_abi.inc"') and shim.count("hpc_abi.inc") == 3


def hpc_plan(n_len, launch_tiles=((0x7FFFFFFF // 256) // 64) * 64):
    """(tiles, kernel launches) of a device call with a capacity: two tile passes in ceil(tiles / launch_tiles) launches each,
    the offset scan, and the edge-zeroing pass with one lane per tile"""
    tiles = -(-n_len // TILE)
    return tiles, (2 * -(-tiles // launch_tiles) + 1 + -(-(-(-tiles // 256)) // launch_tiles)) if tiles else 0


# ---- CPU: the Python layer ------------------------------------------------------------------------------------------------------
def _fake_lib(calls):
    """a stand-in for the library whose cnt_hpc is the numpy reference behind the C calling convention"""
    from cute_nucleotides_amd import _lib

    def u64_at(p, n):
        return np.frombuffer((ctypes.c_uint64 * n).from_address(p.value), dtype=np.uint64) if n else np.zeros(0, dtype=np.uint64)

    def cnt_hpc(bits, length, flags, out, pos, cap, count):
        calls.append(cap)
        assert flags == 0
        ref, rpos = np_hpc(codes_of(u64_at(bits, words_for(length)), length))
        m = min(ref.size, cap)
        u64_at(out, words_for(m))[:] = pack(ref[:m])
        if pos is not None and pos.value:
            u64_at(pos, m)[:] = rpos[:m]
        count._obj.value = ref.size
        return _lib.CNT_ECAP if ref.size > cap else _lib.CNT_OK

    return types.SimpleNamespace(cnt_hpc=cnt_hpc, cnt_words_for=words_for)


def test_hpc_hip_retries_once_with_the_reported_count(monkeypatch):
    from cute_nucleotides_amd import packed_ops as po

    calls = []
    fake = _fake_lib(calls)
    monkeypatch.setattr(po, "lib", lambda: fake)
    rng = np.random.default_rng(13)
    # random ACGT fits the first guess; strictly alternating codes keep everything and do not
    s = rng.integers(0, 4, 5000).astype(np.uint8)
    ref, rpos = np_hpc(s)
    out, n, pos = po.hpc_hip(pack(s), s.size, with_pos=True)
    assert len(calls) == 1 and n == ref.size and np.array_equal(out, pack(ref)) and np.array_equal(pos, rpos)
    del calls[:]
    s = (np.arange(5000) % 2).astype(np.uint8)
    out, n, pos = po.hpc_hip(pack(s), s.size, with_pos=True)
    assert len(calls) == 2 and calls[0] < 5000 and calls[1] == 5000 and n == 5000
    assert np.array_equal(out, pack(s)) and np.array_equal(pos, np.arange(5000, dtype=np.uint64))
    del calls[:]
    out, n = po.hpc_hip(pack(s), s.size)
    assert len(calls) == 2 and n == 5000 and np.array_equal(out, pack(s))
    # a third CNT_ECAP is an error, not a loop
    fake.cnt_hpc = lambda *a: 2
    with pytest.raises(Exception):
        po.hpc_hip(pack(s), s.size)


def np_hpc_minimizers(s, k, w, canonical):
    """the composition on the references: minimizers of the compressed sequence, positions mapped back through the run starts"""
    ref, rpos = np_hpc(s)
    mpos, mval = np_minimizers(pack(ref) if ref.size else np.zeros(1, dtype=np.uint64), ref.size, k, w, canonical)
    return rpos[mpos.astype(np.int64)], mval


def test_hpc_minimizers_maps_positions_back(oracle, monkeypatch):
    from cute_nucleotides_amd import packed_ops as po

    seen = []

    def fake_hpc(bits, length, with_pos=False):
        assert with_pos
        ref, rpos = np_hpc(codes_of(bits, length))
        return pack(ref), ref.size, rpos

    def fake_minimizers(bits, length, k, w, canonical=False, values=True):
        seen.append((length, k, w, canonical))
        return np_minimizers(bits, length, k, w, canonical)

    monkeypatch.setattr(po, "hpc_hip", fake_hpc)
    monkeypatch.setattr(po, "minimizers_hip", fake_minimizers)
    rng = np.random.default_rng(14)
    s = run_lengths_seq(rng, 3000, 2.5)
    ref, rpos = np_hpc(s)
    for flags in (0, CNT_KMER_CANONICAL):
        pos, val = po.hpc_minimizers_hip(pack(s), s.size, 15, 10, flags)
        assert seen[-1] == (ref.size, 15, 10, bool(flags))
        want = np_hpc_minimizers(s, 15, 10, bool(flags))
        assert pos.dtype == np.uint64 and np.array_equal(pos, want[0]) and np.array_equal(val, want[1]) and pos.size > 50
        # a mapped position is a run start, and the k run bases from it on spell the minimizer's forward k-mer
        assert np.isin(pos, rpos).all() and (np.diff(pos.astype(np.int64)) > 0).all()
        assert int(pos[-1]) > ref.size  # really mapped: beyond any coordinate of the compressed sequence


# ---------------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
CANARY = -0x3C3C3C3C3C3C3C3D
HOST_CANARY = 0xDEADBEEFDEADBEEF
PAD = 5  # canary words in front of and behind every footprint


def input_words(s, rng=None, ones=False):
    """the packed input: zero padding, or with `ones` every bit beyond len set, or with `rng` garbage there; two more words behind"""
    n = len(s)
    w = np.concatenate([pack(s), np.zeros(2 + (1 if n == 0 else 0), dtype=np.uint64)])
    if ones or rng is not None:
        fill = (lambda k: np.full(k, 2**64 - 1, dtype=np.uint64)) if ones else (lambda k: rng.integers(0, 2**64, k, dtype=np.uint64))
        if n & 31:
            w[(n - 1) >> 5] |= fill(1)[0] >> np.uint64(2 * (n & 31)) << np.uint64(2 * (n & 31))
        w[words_for(n) :] = fill(w.size - words_for(n))
    return w


def expect(s, cap):
    """(n, the words that must be written, the positions that must be written) at capacity cap"""
    ref, rpos = np_hpc(s)
    m = min(ref.size, cap)
    return ref.size, pack(ref[:m]), rpos[:m]


def check_dev(s, cap=None, with_pos=True, in_phase=0, out_phase=0, words=None, tag=()):
    """the device tier on the codes s: result words, zero slots behind m, pos, count, and canaries around every footprint"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    n_len = len(s)
    cap = n_len if cap is None else cap
    words = input_words(s) if words is None else words
    foot = min(n_len, cap)
    n, want_out, want_pos = expect(s, cap)
    d_in = torch.from_numpy(np.concatenate([np.full(in_phase, 0x1234567890ABCDEF, dtype=np.uint64), words]).view(np.int64)).cuda()
    d_out = torch.full((PAD + out_phase + words_for(foot) + PAD,), CANARY, dtype=torch.int64, device="cuda")
    d_pos = torch.full((PAD + foot + PAD,), CANARY, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((3,), CANARY, dtype=torch.int64, device="cuda")
    d_work = torch.full((po.hpc_work_bytes(n_len) + 8,), 0x77, dtype=torch.uint8, device="cuda")
    o0 = PAD + out_phase
    po.hpc_dev(d_in[in_phase : in_phase + max(words_for(n_len), 1)], n_len, out=d_out[o0 : o0 + words_for(foot)], count=d_cnt[1:2],
               work=d_work[4:], pos=d_pos[PAD : PAD + foot] if with_pos else None, out_cap=cap)  # the scratch at a 4-B-misaligned address
    torch.cuda.synchronize()
    tag = tag + (n_len, cap, with_pos, in_phase, out_phase)
    assert d_cnt.cpu().numpy().tolist() == [CANARY, n, CANARY], tag + (n,)
    h = d_out.cpu().numpy()
    assert (h[:o0] == CANARY).all() and (h[o0 + words_for(foot) :] == CANARY).all(), tag + ("out canary",)
    got = h[o0 : o0 + want_out.size].view(np.uint64)
    assert np.array_equal(got, want_out), tag + ("out", np.flatnonzero(got != want_out)[:4].tolist())
    h = d_pos.cpu().numpy()
    if with_pos:
        assert (h[:PAD] == CANARY).all() and (h[PAD + foot :] == CANARY).all(), tag + ("pos canary",)
        got = h[PAD : PAD + want_pos.size].view(np.uint64)
        assert np.array_equal(got, want_pos), tag + ("pos", np.flatnonzero(got != want_pos)[:4].tolist())
    else:
        assert (h == CANARY).all(), tag
    return n


def check_host(L, s, cap=None, with_pos=True, pinned=False, words=None, tag=()):
    """the host tier on the codes s, pageable or pinned buffers, at a phase inside their allocations"""
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    n_len = len(s)
    cap = n_len if cap is None else cap
    words = input_words(s) if words is None else words
    foot = min(n_len, cap)
    n, want_out, want_pos = expect(s, cap)
    alloc = (lambda k: cn.pinned_empty(k, np.uint64)) if pinned else (lambda k: np.empty(k, dtype=np.uint64))
    bits = alloc(words.size + 3)[3:]
    bits[:] = words
    out, pos = alloc(PAD + words_for(foot) + PAD), alloc(PAD + foot + PAD)
    out[:] = HOST_CANARY
    pos[:] = HOST_CANARY
    cnt = ctypes.c_uint64(0xDEAD)
    rc = L.cnt_hpc(bits.ctypes.data, n_len, 0, out[PAD:].ctypes.data, pos[PAD:].ctypes.data if with_pos else None, cap, ctypes.byref(cnt))
    tag = tag + (n_len, cap, with_pos, pinned)
    assert rc == (_lib.CNT_ECAP if n > cap else _lib.CNT_OK) and cnt.value == n, tag + (rc, cnt.value, n)
    assert (out[:PAD] == HOST_CANARY).all() and (out[PAD + words_for(foot) :] == HOST_CANARY).all(), tag + ("out canary",)
    assert np.array_equal(out[PAD : PAD + want_out.size], want_out), tag + ("out",)
    if with_pos:
        assert (pos[:PAD] == HOST_CANARY).all() and (pos[PAD + foot :] == HOST_CANARY).all(), tag + ("pos canary",)
        assert np.array_equal(pos[PAD : PAD + want_pos.size], want_pos), tag + ("pos",)
    else:
        assert (pos == HOST_CANARY).all(), tag
    return n


LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193, 5 * 8192 + 1)


@gpu
def test_gpu_lengths_and_padding_both_tiers(L):
    """each length with the last base A (the padding's code) and not A; zero padding, ones and garbage beyond len; random ACGT
    and runs of mean length 6"""
    rng = np.random.default_rng(21)
    for n_len in LENGTHS:
        for last in (A, G):
            for mean in (1.33, 6):
                s = run_lengths_seq(rng, n_len, mean) if mean > 2 else rng.integers(0, 4, n_len).astype(np.uint8)
                s[-1] = last
                if n_len > 1 and mean > 2:
                    s[-2] = last  # the last run has two bases: padding of the same code must not make it three, or a new one
                for pad in ("zeros", "ones", "garbage"):
                    w = input_words(s, rng if pad == "garbage" else None, ones=pad == "ones")
                    check_dev(s, words=w, in_phase=1, out_phase=1, tag=(last, mean, pad))
                    if pad != "garbage" and (mean > 2 or n_len in (1, 33, 8193)):
                        check_host(L, s, words=w, tag=(last, mean, pad))


@gpu
@pytest.mark.parametrize("n_len", [TILE, 2 * TILE - 32, 2 * TILE, 2 * TILE + 1, 3 * TILE + 1])
def test_gpu_word_in_front_at_the_fast_path_boundary(n_len):
    """A tile takes the 16-B loads iff it is not tile 0 and the 257 words from the one in FRONT of it on all exist (hip/word_tile.hpp,
    word_tile_pair with BACK = 1).  T: tile 0 alone, guarded.  2T - 32, 2T, 2T + 1: tile 1's last word is one past, at and inside
    the input.  3T + 1: fast tiles between a guarded first and a guarded last.  Inputs in which the word in front decides a kept
    position: one base throughout (only position 0 is kept, in every tile), and runs that end exactly at the last code of word 255
    and of word 256 (and of the same words of every later tile), so that word 256 / 257 begins a run."""
    rng = np.random.default_rng(30)
    runs = run_lengths_seq(rng, n_len, 3)
    for t in range(TILE, n_len, TILE):
        for lo, hi, code in ((t - 7, t, C), (t, t + 32, G), (t + 32, t + 37, T)):
            runs[lo:min(hi, n_len)] = code
    for name, s in (("one base", np.full(n_len, T, dtype=np.uint8)), ("runs to the word edges", runs)):
        for with_pos in (True, False):
            n = check_dev(s, with_pos=with_pos, in_phase=int(with_pos), tag=(name,))
            assert name != "one base" or n == 1
    kept = np_hpc(runs)[1].astype(np.int64)
    for t in range(TILE, n_len, TILE):
        assert t in kept and (t + 32 in kept or t + 32 >= n_len) and not ((kept > t) & (kept < min(t + 32, n_len))).any()


def _seam_cases(rng):
    """(name, codes): runs at every seam of the tile shape"""
    n_len = 5 * TILE + 1
    cases = []
    for name, lo, hi in (("across a word boundary", 32 * 7 - 3, 32 * 7 + 5), ("across two word boundaries", 32 * 9 - 1, 32 * 11 + 1),
                         ("across a wave boundary", 64 * 32 - 10, 64 * 32 + 40), ("across a tile boundary", TILE - 17, TILE + 9),
                         ("from a word start", 32 * 40, 32 * 40 + 7), ("from a tile start", 2 * TILE, 2 * TILE + 100),
                         ("up to a tile end", 3 * TILE - 50, 3 * TILE), ("a whole word", 32 * 50, 32 * 51), ("a whole tile", TILE, 2 * TILE),
                         ("three whole tiles", TILE, 4 * TILE), ("three tiles and both flanks", TILE - 5, 4 * TILE + 3),
                         ("from position 0", 0, 70), ("to the end", n_len - 100, n_len)):
        for code in (A, T):
            s = rng.integers(0, 4, n_len).astype(np.uint8)
            s[lo:hi] = code
            if lo > 0:
                s[lo - 1] = (code + 1) & 3
            if hi < n_len:
                s[hi] = (code + 2) & 3
            cases.append(("%s of %s" % (name, NT[code]), s))
    for n in (1, 33, TILE, 3 * TILE + 5):
        cases += [("constant %s x %d" % (NT[c], n), np.full(n, c, dtype=np.uint8)) for c in (A, G)]
    for n in (64, TILE, 2 * TILE + 77):
        cases.append(("ACAC x %d" % n, (np.arange(n) % 2).astype(np.uint8)))
        cases.append(("ACG x %d" % n, np.array([A, C, G], dtype=np.uint8)[np.arange(n) % 3]))
    for n in (TILE + 3, 6 * TILE + 1):
        cases.append(("{A,C} at P(A) = 0.9 x %d" % n, (rng.random(n) < 0.1).astype(np.uint8)))
    return cases


@gpu
def test_gpu_runs_at_every_seam(L):
    rng = np.random.default_rng(22)
    phases = set()
    for j, (name, s) in enumerate(_seam_cases(rng)):
        n = check_dev(s, in_phase=j % 2, out_phase=(j // 2) % 2, tag=(name,))
        check_dev(s, with_pos=False, tag=(name,))
        if j % 4 == 0:
            check_host(L, s, tag=(name,))
        if name.startswith("constant"):
            assert n == 1
        if name.startswith("AC"):
            assert n == s.size
        if name.startswith("three"):
            ref_pos = np_hpc(s)[1].astype(np.int64)
            assert not ((ref_pos > TILE) & (ref_pos < 4 * TILE)).any()  # tiles 1 to 3 contribute nothing
        if name.startswith("{A,C}"):
            ref_pos = np_hpc(s)[1].astype(np.int64)
            per_tile = np.bincount(ref_pos // TILE)
            phases |= set((np.cumsum(per_tile)[:-1] % 32).tolist())
            assert np.diff(ref_pos).max() > 40
    assert len(phases) >= 4  # tile bases at several 2-bit phases of a word


@gpu
def test_gpu_capacities(L):
    """out_cap in {0, 1, 31, 32, 33, n-1, n, n+1, len} with pos present and NULL: the count is always n, the clipped last word is
    masked, nothing outside the footprint is written; the host tier answers CNT_ECAP exactly when n > out_cap"""
    rng = np.random.default_rng(23)
    for s in (run_lengths_seq(rng, 2 * TILE + 77, 3), rng.integers(0, 4, TILE + 1).astype(np.uint8), (rng.random(3 * TILE) < 0.1).astype(np.uint8),
              run_lengths_seq(rng, 100, 2)):
        n = np_hpc(s)[0].size
        assert n > 34
        for cap in (0, 1, 31, 32, 33, n - 1, n, n + 1, len(s)):
            for with_pos in (True, False):
                check_dev(s, cap=cap, with_pos=with_pos, out_phase=cap & 1)
                if len(s) < 2 * TILE or cap in (0, n - 1, n):
                    check_host(L, s, cap=cap, with_pos=with_pos)


@gpu
def test_gpu_runs_across_launch_seams(launch_tiles):
    """the lab build cut into launches of 64 / 128 tiles, 129 and 257 tiles: a run across every launch seam, another that covers
    the tiles on both sides of one; the passes in several launches, counted in a captured graph"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(launch_tiles)
    for tiles in (129, 257):
        n_len = (tiles - 1) * TILE + 4001
        s = rng.integers(0, 4, n_len).astype(np.uint8)
        seams = list(range(launch_tiles * TILE, n_len, launch_tiles * TILE))
        for j, e in enumerate(seams):
            lo, hi = (e - 13, e + 21) if j % 2 == 0 else (e - TILE - 9, min(e + TILE + 5, n_len - 2))
            s[lo:hi] = j & 3
            s[lo - 1], s[hi] = (j + 1) & 3, (j + 2) & 3
        ref_pos = np_hpc(s)[1].astype(np.int64)
        assert all(not ((ref_pos > e - 13) & (ref_pos < e + 21)).any() for e in seams)
        check_dev(s, tag=(launch_tiles, tiles))
        check_dev(s, with_pos=False, cap=len(s) // 2, tag=(launch_tiles, tiles))
        got_tiles, launches = hpc_plan(n_len, launch_tiles)
        assert got_tiles == tiles and launches == 2 * -(-tiles // launch_tiles) + 2
        d = torch.from_numpy(pack(s).view(np.int64)).cuda()
        out, pos = torch.empty(words_for(n_len), dtype=torch.int64, device="cuda"), torch.empty(n_len, dtype=torch.int64, device="cuda")
        cnt, work = torch.empty(1, dtype=torch.int64, device="cuda"), torch.empty(po.hpc_work_bytes(n_len), dtype=torch.uint8, device="cuda")
        assert _kernel_nodes_of(torch, lambda: po.hpc_dev(d, n_len, out, cnt, work, pos=pos)) == launches


@gpu
def test_gpu_hpc_in_a_captured_graph_and_behind_a_side_stream():
    """one torch.cuda.graph capture of the call (with and without pos, on the same scratch in turn) replayed twice on changed
    input; then the call enqueued on a side stream behind the copy that makes its input, no host sync in between"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(24)
    n_len = 9 * TILE + 1234
    nw = words_for(n_len)
    bits = torch.zeros(nw, dtype=torch.int64, device="cuda")
    outs = [torch.empty(nw, dtype=torch.int64, device="cuda") for _ in range(2)]
    pos = torch.empty(n_len, dtype=torch.int64, device="cuda")
    cnts = torch.empty(2, dtype=torch.int64, device="cuda")
    work = torch.empty(po.hpc_work_bytes(n_len), dtype=torch.uint8, device="cuda")

    def chain():
        po.hpc_dev(bits, n_len, outs[0], cnts[0:1], work, pos=pos)
        po.hpc_dev(bits, n_len, outs[1], cnts[1:2], work)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain()  # module load outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for rep, mean in enumerate((1.33, 20)):
        s = run_lengths_seq(rng, n_len, mean) if mean > 2 else rng.integers(0, 4, n_len).astype(np.uint8)
        bits.copy_(torch.from_numpy(pack(s).view(np.int64)))
        for t in outs + [pos, cnts]:
            t.fill_(CANARY)
        work.fill_(0x77 + rep)  # the scratch needs no zeroing
        g.replay()
        torch.cuda.synchronize()
        n, want_out, want_pos = expect(s, n_len)
        assert cnts.cpu().numpy().tolist() == [n, n], rep
        for o in outs:
            assert np.array_equal(o[: want_out.size].cpu().numpy().view(np.uint64), want_out), rep
        assert np.array_equal(pos[:n].cpu().numpy().view(np.uint64), want_pos) and (pos[n:].cpu().numpy() == CANARY).all(), rep
    s = run_lengths_seq(rng, n_len, 4)
    host = torch.from_numpy(pack(s).view(np.int64)).pin_memory()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        bits.copy_(host, non_blocking=True)
        po.hpc_dev(bits, n_len, outs[0], cnts[0:1], work, pos=pos)
    torch.cuda.current_stream().wait_stream(side)
    n, want_out, want_pos = expect(s, n_len)
    assert int(cnts[0].item()) == n and np.array_equal(outs[0][: want_out.size].cpu().numpy().view(np.uint64), want_out)
    assert np.array_equal(pos[:n].cpu().numpy().view(np.uint64), want_pos)


@gpu
def test_gpu_host_tier_pinned_and_pageable(L):
    """pinned host buffers (used in place: the kernels' plain stores and atomic ORs go over the link) and pageable ones (staged)"""
    rng = np.random.default_rng(25)
    for s in (run_lengths_seq(rng, 3 * TILE + 77, 2), (rng.random(2 * TILE + 5) < 0.1).astype(np.uint8), rng.integers(0, 4, 45).astype(np.uint8)):
        n = np_hpc(s)[0].size
        for pinned in (False, True):
            for cap in (len(s), n, n - 1):
                for with_pos in (True, False):
                    check_host(L, s, cap=cap, with_pos=with_pos, pinned=pinned)
    # the guess-and-retry wrapper on the real library, short of its first guess and not
    from cute_nucleotides_amd import packed_ops as po

    for s in ((np.arange(3 * TILE + 5) % 2).astype(np.uint8), run_lengths_seq(rng, 2 * TILE, 3)):
        out, n, pos = po.hpc_hip(pack(s), len(s), with_pos=True)
        ref, rpos = np_hpc(s)
        assert n == ref.size and np.array_equal(out, pack(ref)) and np.array_equal(pos, rpos)
        out, n = po.hpc_hip(pack(s), len(s))
        assert n == ref.size and np.array_equal(out, pack(ref))


@gpu
def test_gpu_hpc_minimizers_composition(oracle):
    """hpc_minimizers_hip against the numpy minimizer reference run on the numpy-compressed sequence, mapped back"""
    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(26)
    for s in (run_lengths_seq(rng, 4 * TILE + 99, 2.2), rng.integers(0, 4, 20000).astype(np.uint8)):
        for flags in (0, CNT_KMER_CANONICAL):
            pos, val = po.hpc_minimizers_hip(pack(s), len(s), 15, 10, flags)
            want = np_hpc_minimizers(s, 15, 10, bool(flags))
            assert pos.size > 500 and np.array_equal(pos, want[0]) and np.array_equal(val, want[1]), flags


@gpu
def test_gpu_hpc_fuzz(L):
    """200 cases: random len in [1, 40000], random run-length distribution, random capacity, random phases"""
    rng = np.random.default_rng(27)
    for case in range(200):
        n_len = int(rng.integers(1, 40001))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            s = rng.integers(0, 4, n_len).astype(np.uint8)
        elif kind == 1:
            s = (rng.random(n_len) < rng.choice([0.5, 0.1, 0.01, 0.0005])).astype(np.uint8) * np.uint8(rng.integers(1, 4))
        else:
            s = run_lengths_seq(rng, n_len, float(rng.choice([1, 1.5, 3, 20, 500, 9000])), alphabet=int(rng.integers(2, 5)))
        n = np_hpc(s)[0].size
        cap = [n_len, n, max(n - 1, 0), int(rng.integers(0, n_len + 1)), n + 1, int(rng.integers(0, n + 1))][int(rng.integers(0, 6))]
        w = input_words(s, rng)
        check_dev(s, cap=cap, with_pos=bool(rng.integers(0, 4)), in_phase=int(rng.integers(0, 3)), out_phase=int(rng.integers(0, 3)), words=w, tag=(case, kind))
        if case % 10 == 0:
            check_host(L, s, cap=cap, with_pos=bool(rng.integers(0, 2)), pinned=case % 20 == 0, words=w, tag=(case, kind))


@gpu
def test_gpu_hpc_positions_past_2p32(fullsize):
    """2^32 + 3 * 8192 + 17 nt whose first 2^32 are A (a memset) in front of a random tail that does not start with A: more than
    half a million tiles that contribute nothing in front of the first output word, and positions above 2^32"""
    import time

    import torch

    from conftest import need_free_hbm
    from cute_nucleotides_amd import packed_ops as po

    P32 = 1 << 32
    n_len = P32 + 3 * TILE + 17
    need_free_hbm(3)
    rng = np.random.default_rng(28)
    tail = run_lengths_seq(rng, n_len - P32, 2)
    tail[0] = G
    ref, rpos = np_hpc(tail)
    n = 1 + ref.size
    bits = torch.zeros(words_for(n_len) + 1, dtype=torch.int64, device="cuda")
    bits[P32 // 32 : P32 // 32 + words_for(tail.size)] = torch.from_numpy(pack(tail).view(np.int64)).cuda()
    cap = n + 40
    out = torch.full((words_for(cap) + PAD,), CANARY, dtype=torch.int64, device="cuda")
    pos = torch.full((cap + PAD,), CANARY, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), CANARY, dtype=torch.int64, device="cuda")
    work = torch.empty(po.hpc_work_bytes(n_len), dtype=torch.uint8, device="cuda")
    po.hpc_dev(bits[:-1], n_len, out[: words_for(cap)], cnt, work, pos=pos[:cap], out_cap=cap)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    po.hpc_dev(bits[:-1], n_len, out[: words_for(cap)], cnt, work, pos=pos[:cap], out_cap=cap)
    torch.cuda.synchronize()
    fullsize(32, (time.perf_counter() - t0) * 1e3, check="hpc of 2^32 A and a random tail: kernels")
    assert int(cnt.item()) == n
    want_out = pack(np.r_[np.uint8(A), ref])
    h = out.cpu().numpy()
    assert np.array_equal(h[: want_out.size].view(np.uint64), want_out) and (h[words_for(cap) :] == CANARY).all()
    h = pos.cpu().numpy()
    assert h[0] == 0 and np.array_equal(h[1:n].view(np.uint64), rpos + np.uint64(P32)) and (h[n:] == CANARY).all()
    assert int(h[1]) == P32 and int(h[n - 1]) > P32 + 3 * TILE


@gpu
def test_gpu_hpc_output_offsets_past_2p32(fullsize):
    """a 96-nt pattern (three words, first base != last base, Q of its positions kept) repeated to just over 2^32 * 96 / Q nt, so
    that n > 2^32: the output is the Q-code pattern repeated, compared on the device in periods of Q words (lcm(Q, 32) codes
    divide them); pos is NULL"""
    import time

    import torch

    from conftest import need_free_hbm
    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(29)
    pat = rng.integers(0, 4, 96).astype(np.uint8)
    pat[95] = (pat[0] + 1) & 3
    pat[94] = (pat[95] + 1) & 3
    ref = np_hpc(pat)[0]
    Q = ref.size
    assert 60 <= Q < 96 and pat[0] != pat[95]
    repeats = (1 << 32) // Q + 2
    n_len, n = 96 * repeats, Q * repeats
    assert n > (1 << 32) and np_hpc(np.tile(pat, 3))[0].size == 3 * Q and (32 * Q) % math.lcm(Q, 32) == 0
    need_free_hbm(4)
    bits = torch.from_numpy(pack(pat).view(np.int64)).cuda().repeat(repeats)
    out = torch.full((words_for(n) + PAD,), CANARY, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), CANARY, dtype=torch.int64, device="cuda")
    work = torch.empty(po.hpc_work_bytes(n_len), dtype=torch.uint8, device="cuda")
    po.hpc_dev(bits, n_len, out[: words_for(n)], cnt, work, out_cap=n)  # warm-up
    out.fill_(CANARY)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    po.hpc_dev(bits, n_len, out[: words_for(n)], cnt, work, out_cap=n)
    torch.cuda.synchronize()
    fullsize(32, (time.perf_counter() - t0) * 1e3, check="hpc with n > 2^32, no pos: kernels", log2_out=32)
    assert int(cnt.item()) == n == Q * repeats
    period = pack(np.tile(ref, 32))  # Q words
    assert period.size == Q
    whole = words_for(n) // Q
    d_period = torch.from_numpy(period.view(np.int64)).cuda()
    assert bool((out[: whole * Q].view(whole, Q) == d_period).all())
    rest = n - whole * Q * 32  # the codes behind the last whole period, zeros behind them
    assert 0 <= rest < 32 * Q
    want = pack(np.tile(ref, 32)[:rest])
    h = out[whole * Q :].cpu().numpy()
    assert np.array_equal(h[: want.size].view(np.uint64), want) and (h[want.size :] == CANARY).all() and h.size == want.size + PAD
