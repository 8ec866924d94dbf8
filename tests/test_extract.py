"""Region extraction on packed words (include/cute_nt.h "region extraction"): n regions of one length, each written as a packed
sequence of its own, forward or as the reverse complement of the region; cnt_subseq is the one region with host-known bounds.
Not in the reference, so the CPU part pins two references against each other -- the definition as a literal per-base loop over
the codes read straight from the words, and a vectorised numpy form on the words -- checks the properties the definition
implies, the Python layer's errors, every argument error of the ABI, the empty calls and the ISA of the three kernels.  The GPU
part compares both tiers with the numpy reference bit for bit: every start phase and the tile edges of a subsequence, every
8-B phase of its output, windows with every combination of flag and info, rejected regions among valid ones with sentinels
around the output, search -> extract end to end, tiles across launch edges on the lab build, a captured graph on a side
stream, pinned against staged host buffers, a fuzz loop, and once with starts past 2^32."""
import ctypes
import os
import re
import sys
import time

import numpy as np
import pytest

from test_find_pattern import LETTERS, codes_of, words_of_codes
from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch
from test_kmers import assert_split_launches_by_max_tiles_per_launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNT_EXTRACT_REVCOMP = 0x40
CNT_FIND_REVERSE = 0x100
TILE_WORDS = 512  # output words per workgroup tile (hip/extract_kernels.hpp kExtractTileWords)
TILE = 32 * TILE_WORDS  # 16384 nt
U64 = np.uint64
MAX64 = (1 << 64) - 1


def words_for(n):
    return (n + 31) // 32


# ---- references -------------------------------------------------------------------------------------------------------
def reversed_flags(n, info, flag):
    """region i is reversed iff exactly one of: the flag; info[i] & CNT_FIND_REVERSE"""
    r = np.full(n, bool(flag))
    if info is not None:
        r ^= (np.asarray(info, dtype=U64) & U64(CNT_FIND_REVERSE)) != 0
    return r


def def_extract(oracle, words, length, starts, region_len, info=None, flag=False):
    """the definition, literally, base by base on the codes of the sequence; records packed by the oracle's encoder"""
    s = codes_of(words, length)
    R = words_for(region_len)
    out = np.zeros((len(starts), R), dtype=U64)
    rejected = 0
    for i, (st, rev) in enumerate(zip(starts, reversed_flags(len(starts), info, flag))):
        st = int(st)
        if st > length or region_len > length - st:
            rejected += 1
            continue
        rec = [0] * region_len
        for j in range(region_len):
            rec[j] = (int(s[st + region_len - 1 - j]) ^ 2) if rev else int(s[st + j])
        if region_len:
            out[i] = oracle.n_to_bits_lut(LETTERS[np.asarray(rec, dtype=np.int64)])
    return out, rejected


def np_reverse_codes(x):
    x = ((x >> U64(2)) & U64(0x3333333333333333)) | ((x & U64(0x3333333333333333)) << U64(2))
    x = ((x >> U64(4)) & U64(0x0F0F0F0F0F0F0F0F)) | ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4))
    return x.byteswap()


def np_extract(words, length, starts, region_len, info=None, flag=False, first_word=0):
    """the vectorised reference on the words: every output word is one 64-bit window of the input.  `words` holds the input from
    word `first_word` on (only the words the accepted regions touch need to be there); returns (records[n, R], rejected)"""
    w = np.concatenate([np.asarray(words, dtype=U64), np.zeros(2, dtype=U64)])
    starts = [int(v) for v in starts]
    n, R = len(starts), words_for(region_len)
    rev = reversed_flags(n, info, flag)
    ok = np.array([st <= length and region_len <= length - st for st in starts], dtype=bool).reshape(n)
    out = np.zeros((n, R), dtype=U64)
    if R == 0 or n == 0:
        return out, int(n - ok.sum())
    st = np.array([v - 32 * first_word if good else 0 for v, good in zip(starts, ok)], dtype=np.int64)[:, None]
    j = np.arange(R, dtype=np.int64)[None, :]
    p = np.where(rev[:, None], st + region_len - 32 - 32 * j, st + 32 * j)
    pp = np.maximum(p, 0)
    iw, sh = pp >> 5, (2 * (pp & 31)).astype(U64)
    iw = np.minimum(iw, w.size - 2)
    win = (w[iw] >> sh) | np.where(sh > 0, (w[iw + 1] << U64(1)) << (U64(63) - sh), U64(0))
    neg = p < 0  # reversed, the record's last word: the first -p codes of the window do not exist
    win = np.where(neg, w[0] << (2 * np.where(neg, -p, 0)).astype(U64), win)
    win = np.where(rev[:, None], np_reverse_codes(win) ^ U64(0xAAAAAAAAAAAAAAAA), win)
    rem = region_len - 32 * j
    keep = np.where(rem >= 32, U64(MAX64), (U64(1) << (2 * np.clip(rem, 0, 31)).astype(U64)) - U64(1))
    out = np.where(ok[:, None], win & keep, U64(0))
    return out, int(n - ok.sum())


def np_subseq(words, length, start, sub_len, rev=False, first_word=0):
    return np_extract(words, length, [start], sub_len, None, rev, first_word)[0].reshape(-1)


def random_words(oracle, rng, n_len, extra=2):
    """a random sequence as words: garbage above len in the last word and `extra` garbage words behind it"""
    return words_of_codes(oracle, rng.integers(0, 4, n_len).astype(np.uint8), extra=extra, rng=rng)


def clean(words, n_len):
    """the words of the sequence alone, unused high bits zero"""
    w = np.array(words[: max(words_for(n_len), 0)], dtype=U64)
    if n_len & 31:
        w[-1] &= U64((1 << (2 * (n_len & 31))) - 1)
    return w


# ---- CPU: the references ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev", [False, True])
def test_numpy_reference_against_the_definition(oracle, rev):
    rng = np.random.default_rng(17 + rev)
    n_len = 32 * 9 + 13
    words = random_words(oracle, rng, n_len)
    for region_len in (0, 1, 5, 31, 32, 33, 64, 65, 100, 129):
        starts = [ph for ph in range(32) if ph + region_len <= n_len] + [32, 64 + 7, n_len - region_len, n_len - region_len + 1, n_len + 1, MAX64]
        info = rng.integers(0, 2, len(starts)).astype(U64) * U64(CNT_FIND_REVERSE) + rng.integers(0, 256, len(starts)).astype(U64)
        for inf in (None, info):
            want, wr = def_extract(oracle, words, n_len, starts, region_len, inf, rev)
            got, gr = np_extract(words, n_len, starts, region_len, inf, rev)
            assert np.array_equal(got, want) and gr == wr == 3, (region_len, rev, inf is None)
            assert got.dtype == U64 and got.shape == (len(starts), words_for(region_len))
    # the same from a slice of the words: only the words a region touches
    got = np_subseq(words[3:], n_len, 32 * 3 + 17, 150, rev, first_word=3)
    assert np.array_equal(got, def_extract(oracle, words, n_len, [32 * 3 + 17], 150, None, rev)[0][0])


def test_properties(oracle):
    rng = np.random.default_rng(5)
    for n_len in (1, 31, 32, 33, 700, 2 * TILE + 77):
        words = random_words(oracle, rng, n_len)
        s = clean(words, n_len)
        assert np.array_equal(np_subseq(words, n_len, 0, n_len), s)
        assert np.array_equal(np_subseq(words, n_len, 0, n_len, True), oracle.reverse_complement(s, n_len))
        for _ in range(8):
            a = int(rng.integers(0, n_len + 1))
            l = int(rng.integers(0, n_len - a + 1))
            b = int(rng.integers(0, l + 1))
            m = int(rng.integers(0, l - b + 1))
            sub = np_subseq(words, n_len, a, l)
            assert np.array_equal(np_subseq(np.concatenate([sub, np.zeros(1, dtype=U64)]), l, b, m), np_subseq(words, n_len, a + b, m)), (n_len, a, l, b, m)
            if l:
                assert np.array_equal(np_subseq(words, n_len, a, l, True), oracle.reverse_complement(sub, l)), (n_len, a, l)
                # the decoded record is the slice of the decoded sequence
                assert bytes(oracle.bits_to_n_lut(sub, l)) == bytes(oracle.bits_to_n_lut(s, n_len))[a : a + l]


# ---- CPU: the Python layer and the ABI --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


def test_python_wrappers_raise(L):
    import torch

    from cute_nucleotides_amd import packed_ops as po

    w = np.zeros(2, dtype=U64)
    st = np.zeros(3, dtype=U64)
    for start, sub_len in ((65, 0), (0, 65), (60, 5), (-1, 3), (3, -1), (1 << 64, 1)):
        with pytest.raises(ValueError):
            po.subseq_hip(w, 64, start, sub_len)
    with pytest.raises(ValueError):
        po.subseq_hip(w, 65, 0, 1)  # longer than the words hold
    with pytest.raises(TypeError):
        po.subseq_hip(w.astype(np.int64), 64, 0, 1)
    with pytest.raises(TypeError):
        po.extract_hip(w, 64, st.astype(np.int64), 5)
    with pytest.raises(TypeError):
        po.extract_hip(w, 64, [0, 1], 5)  # a list is an int64 array
    with pytest.raises(TypeError):
        po.extract_hip(w, 64, st, 5, info=np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError):
        po.extract_hip(w, 64, st, 5, info=np.zeros(2, dtype=U64))
    with pytest.raises(ValueError):
        po.extract_hip(w, 64, st, -1)
    with pytest.raises(ValueError):
        po.extract_hip(w, 65, st, 5)
    # the device wrappers check before the library is called: CPU tensors are refused
    tw, ts = torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError):
        po.subseq_dev(tw, 64, 0, 5)
    with pytest.raises(ValueError):
        po.extract_dev(tw, 64, ts, 5)
    # empty work is answered without a device
    assert po.subseq_hip(w, 64, 64, 0).size == 0 and po.subseq_hip(w, 64, 7, 0, revcomp=True).size == 0
    rec, rej = po.extract_hip(w, 64, st[:0], 5)
    assert rec.shape == (0, 1) and rej == 0
    rec, rej = po.extract_hip(w, 64, st, 0, info=st)
    assert rec.shape == (3, 0) and rej == 0


def test_abi_errors_come_before_any_device_work(L):
    from cute_nucleotides_amd import _lib

    buf = np.zeros(4096, dtype=U64)
    q = lambda word, byte=0: ctypes.c_void_p(buf.ctypes.data + 8 * word + byte)  # noqa: E731
    out = np.full(512, 0x5A5A5A5A5A5A5A5A, dtype=U64)
    o = lambda word, byte=0: ctypes.c_void_p(out.ctypes.data + 8 * word + byte)  # noqa: E731
    rej = np.full(2, 0x5A5A5A5A5A5A5A5A, dtype=U64)
    c = lambda byte=0: ctypes.c_void_p(rej.ctypes.data + byte)  # noqa: E731
    EINVAL, ECAP, OK = _lib.CNT_EINVAL, _lib.CNT_ECAP, _lib.CNT_OK
    for dev in (False, True):
        def extract(bits, n_len, start, info, n, region_len, flags, dst, out_words, rejected):
            if dev:
                return L.cnt_extract_dev(bits, n_len, start, info, n, region_len, flags, dst, out_words, rejected, None)
            return L.cnt_extract(bits, n_len, start, info, n, region_len, flags, dst, out_words, ctypes.cast(rejected, ctypes.POINTER(ctypes.c_uint64)))

        def subseq(bits, n_len, start, sub_len, flags, dst, out_words):
            if dev:
                return L.cnt_subseq_dev(bits, n_len, start, sub_len, flags, dst, out_words, None)
            return L.cnt_subseq(bits, n_len, start, sub_len, flags, dst, out_words)

        tag = "dev" if dev else "host"
        # 100 nt = 4 words at q(10), 8 starts at q(100), info at q(200), 8 records of 40 nt = 2 words each
        ok = (q(10), 100, q(100), q(200), 8, 40, 0, o(0), 16, c())
        sok = (q(10), 100, 7, 40, 0, o(0), 2)
        for flags in (0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x80, 0x100, 0x80000000, CNT_EXTRACT_REVCOMP | 0x1):
            assert extract(*ok[:6], flags, *ok[7:]) == EINVAL, (tag, flags)
            assert extract(None, 0, None, None, 0, 0, flags, None, 0, None) == EINVAL, (tag, flags)  # even without work
            assert subseq(*sok[:4], flags, *sok[5:]) == EINVAL, (tag, flags)
            assert subseq(None, 0, 0, 0, flags, None, 0) == EINVAL, (tag, flags)
        # NULL bits, start or out (info and rejected may be NULL)
        assert extract(None, *ok[1:]) == EINVAL and extract(*ok[:2], None, *ok[3:]) == EINVAL and extract(*ok[:7], None, 16, c()) == EINVAL
        assert subseq(None, *sok[1:]) == EINVAL and subseq(*sok[:5], None, 2) == EINVAL
        # not 8-B aligned
        for byte in (1, 4, 7):
            assert extract(q(10, byte), *ok[1:]) == EINVAL
            assert extract(*ok[:2], q(100, byte), *ok[3:]) == EINVAL
            assert extract(*ok[:3], q(200, byte), *ok[4:]) == EINVAL
            assert extract(*ok[:7], o(0, byte), 16, c()) == EINVAL
            assert extract(*ok[:9], c(byte)) == EINVAL
            assert subseq(q(10, byte), *sok[1:]) == EINVAL and subseq(*sok[:5], o(0, byte), 2) == EINVAL
        # out (16 words) overlapping the input words, the starts or info
        for ow in (10, 13, 0, 9):
            assert extract(*ok[:7], q(ow), 16, c()) == EINVAL, (tag, ow)
        for ow in (100, 107, 85, 92):
            assert extract(*ok[:7], q(ow), 16, c()) == EINVAL, (tag, ow)
        for ow in (200, 207, 185):
            assert extract(*ok[:7], q(ow), 16, c()) == EINVAL, (tag, ow)
        for ow in (10, 13, 9):
            assert subseq(*sok[:5], q(ow), 2) == EINVAL, (tag, ow)
        # capacity: out_words < n*R, and n * R overflowing size_t
        assert extract(*ok[:8], 15, c()) == ECAP and subseq(*sok[:6], 1) == ECAP
        assert extract(*ok[:4], 1 << 63, 40, 0, o(0), MAX64, c()) == ECAP
        assert extract(*ok[:4], 1 << 61, 32, 0, o(0), MAX64, c()) == ECAP  # the bytes of n * R words
        # cnt_subseq: host-known bounds
        for start, sub_len in ((101, 1), (100, 1), (61, 40), (0, 101), (MAX64, 2), (2, MAX64)):
            assert subseq(q(10), 100, start, sub_len, 0, o(0), 512) == EINVAL, (tag, start, sub_len)
        # empty work: CNT_OK without a device, whatever the pointers; the host tier sets *rejected = 0
        for n, region_len in ((0, 40), (8, 0), (0, 0)):
            assert extract(None, 100, None, None, n, region_len, CNT_EXTRACT_REVCOMP, None, 0, None) == OK
            if not dev:
                rej[0] = 99
                assert extract(*ok[:4], n, region_len, 0, o(0), 16, c()) == OK and rej[0] == 0
                rej[0] = 0x5A5A5A5A5A5A5A5A
        assert subseq(None, 100, 100, 0, 0, None, 0) == OK and subseq(None, 100, 500, 0, CNT_EXTRACT_REVCOMP, None, 0) == OK
    assert (out == 0x5A5A5A5A5A5A5A5A).all() and (rej == 0x5A5A5A5A5A5A5A5A).all()  # nothing was written
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        assert L.cnt_extract(q(10), 100, q(100), q(200), 8, 40, 0, o(0), 16, None) == _lib.CNT_ENODEV
        assert L.cnt_subseq(q(10), 100, 7, 40, 0, o(0), 2) == _lib.CNT_ENODEV
        assert L.cnt_extract_dev(q(10), 100, q(100), None, 8, 40, 0, o(0), 16, None, None) < 0
        assert L.cnt_subseq_dev(q(10), 100, 7, 40, 0, o(0), 2, None) < 0
        assert (out == 0x5A5A5A5A5A5A5A5A).all()


def test_abi_wiring(L):
    import subprocess

    from cute_nucleotides_amd import _lib

    names = ("cnt_subseq", "cnt_subseq_dev", "cnt_extract", "cnt_extract_dev")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(L, name) and name in exported and name + "(" in header
    assert "#define CNT_EXTRACT_REVCOMP 0x40u" in header and _lib.CNT_EXTRACT_REVCOMP == CNT_EXTRACT_REVCOMP
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    for sig in (r"pub fn subseq_hip\(", r"pub fn subseq_hip_dev\(", r"pub fn extract_hip\(", r"pub fn extract_hip_dev\("):
        assert re.search(sig, rust), sig


# ---- CPU: the ISA and the launch plan ---------------------------------------------------------------------------------
EXTRACT_KERNELS = ["extract_words", "extract_tiles_fwd", "extract_tiles_rev"]


def test_extract_kernels_isa():
    """the three kernels from the product's gfx950 assembly: no scratch, no spills, <= 84 VGPRs, no LDS; the tile kernels reach
    memory through raw-buffer instructions only (their start / info reads are scalar loads), with both loads in flight before
    the first wait for memory, `nt` loads, `sc0 sc1 nt` stores and no waterfall loop"""
    sys.path.insert(0, os.path.join(ROOT, "bench"))
    import isa_digest

    asm = isa_digest.assembly()
    for name in EXTRACT_KERNELS:
        m = re.search(r"^cnt::%s\(.*?\): +; @(.*?)\.end_amdhsa_kernel" % name, asm, re.S | re.M)
        assert m, name + " not in the product's assembly"
        text = m.group(1)
        body = [l.strip().split(";")[0].strip() for l in text.splitlines() if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        assert "scratch_" not in text, name
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", text), name
        assert re.search(r"\.amdhsa_group_segment_fixed_size\s+0\b", text), name
        assert int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", text).group(1)) <= 84, name
        meta = re.search(r"\.name:\s+cnt::%s\(.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)" % name, asm, re.S)
        assert meta and meta.group(1) == "0" and meta.group(2) == "0", (name, meta and meta.groups())
        if "tiles" not in name:
            continue
        t = isa_digest.summarise({"body": body}, False)
        assert "s_xor_b64 exec, exec" not in text, name
        assert "global_load" not in t["counts"] and "global_store" not in t["counts"] and "flat_" not in text, (name, t["counts"])
        assert t["counts"]["buffer_load_dwordx4"] == 1 and t["counts"]["buffer_load_dwordx2"] == 1 and t["counts"]["buffer_store_dwordx4"] == 1, (name, t["counts"])
        assert t["loads"] == 2 and t["loads_before_first_wait"] == 2, (name, t["loads_before_first_wait"], t["loads"])
        assert t["load_policies"] == ["nt"] and t["store_policies"] == ["sc0 nt sc1"], name
    assert len(isa_digest.kernels(asm)) < 60  # the product's templated kernels: none added


HW_LAUNCH_TILES = ((0x7FFFFFFF // 256) // 64) * 64  # max_tiles_per_launch(256) of the product build


def extract_plan(n, region_len, head=0, both=False, launch_tiles=HW_LAUNCH_TILES):
    """kernel launches of a device call: per record (R - head) // 512 tiles, all records' tiles in launches of launch_tiles
    (twice with info: one kernel per orientation), then the word kernel (256 words per workgroup) on [0, head) and on the
    words behind the tiles of every record"""
    R = words_for(region_len)
    if R < head + TILE_WORDS:
        head = 0
    tiles = (R - head) // TILE_WORDS
    launches = -(-(n * tiles) // launch_tiles) * (2 if both else 1)
    for w in (head, R - head - tiles * TILE_WORDS):
        launches += -(-(-(-(n * w) // 256)) // launch_tiles)
    return launches


def test_extract_plan_matches_the_launcher_and_splitter_source():
    src = open(os.path.join(ROOT, "hip", "extract_kernels.hpp")).read()
    assert "constexpr int kExtractBlock = 256;" in src and "constexpr uint32_t kExtractTileWords = 2 * kExtractBlock;" in src
    abi = open(os.path.join(ROOT, "hip", "extract_abi.inc")).read()
    for line in ("const uint64_t tiles = (R - head) / kExtractTileWords;  // per record",
                 "split_launches(n * tiles, kExtractBlock, [&](uint64_t first, uint64_t count) {",
                 "split_launches((total + kExtractBlock - 1) / kExtractBlock, kExtractBlock, [&](uint64_t first, uint64_t count) {",
                 "uint64_t head = ((128 - (reinterpret_cast<uintptr_t>(d_out) & 127)) & 127) >> 3;",
                 "if (R < head + kExtractTileWords) head = 0;  // no tile behind it"):
        assert line in abi, line
    assert abi.count("hipLaunchKernelGGL(") == 3
    assert_split_launches_by_max_tiles_per_launch()
    assert HW_LAUNCH_TILES == 8388544
    assert extract_plan(1, 2 * TILE + 5) == 2 and extract_plan(1, 2 * TILE + 5, head=3) == 3 and extract_plan(1, 2 * TILE) == 1
    assert extract_plan(5000, 23) == 1 and extract_plan(3, TILE + 7, both=True) == 3 and extract_plan(1, TILE + 32, head=3) == 2
    assert extract_plan(70000, 33, launch_tiles=64) == 9 and extract_plan(1, 64 * TILE * 2 + 40, launch_tiles=64) == 3


# ---------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
SENTINEL = -0x3C3C3C3C3C3C3C3D
HOST_SENTINEL = 0xDEADBEEFDEADBEEF
SUB_LENS = [1, 31, 32, 33, 63, 64, 65, TILE - 1, TILE, TILE + 1, TILE + 33, 2 * TILE + 5, 3 * TILE]


def _dev_words(t):
    return t.cpu().numpy().view(U64)


@gpu
@pytest.mark.parametrize("rev", [False, True])
def test_gpu_subseq_every_phase_and_tile_edge_both_tiers(oracle, rev):
    """start at every phase 0..31, at a multiple of 32 and at len - sub_len (len % 32 != 0), sub_len around every word and tile
    edge, both tiers, against the numpy reference.  The unused high bits of the last input word and the two words behind the
    input are random: the result must not depend on them."""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(100 + rev)
    n_len = 3 * TILE + 32 * 40 + 13
    words = random_words(oracle, rng, n_len)
    assert np.array_equal(clean(words, n_len)[:-1], words[: words_for(n_len) - 1]) and not np.array_equal(clean(words, n_len), words[: words_for(n_len)])
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    for sub_len in SUB_LENS:
        starts = sorted({ph for ph in range(32)} | {32 * 37, n_len - sub_len})
        want, _ = np_extract(words, n_len, starts, sub_len, None, rev)
        for row, start in enumerate(starts):
            assert start + sub_len <= n_len
            got = po.subseq_dev(dwords, n_len, start, sub_len, revcomp=rev)
            assert np.array_equal(_dev_words(got), want[row]), (sub_len, start, rev, "device")
            if start % 5 == 0 or start >= 32:  # the host tier stages the same kernels: a third of the phases
                assert np.array_equal(po.subseq_hip(words[: words_for(n_len)], n_len, start, sub_len, revcomp=rev), want[row]), (sub_len, start, rev, "host")
    # the whole sequence: forward it is the cleaned input, reversed the oracle's reverse complement
    whole = _dev_words(po.subseq_dev(dwords, n_len, 0, n_len, revcomp=rev))
    assert np.array_equal(whole, oracle.reverse_complement(clean(words, n_len), n_len) if rev else clean(words, n_len))


@gpu
def test_gpu_subseq_output_at_every_phase_of_a_line(oracle):
    """d_out at each 8-B phase of a 128-B line for a tiled length: the head peel in front of the tiles, sentinels around"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(7)
    n_len, sub_len = 3 * TILE + 999, 2 * TILE + 5
    R = words_for(sub_len)
    words = random_words(oracle, rng, n_len)
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    buf = torch.empty(R + 64, dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 128 == 0
    for rev in (False, True):
        for start in (0, 17, 32 * 5, n_len - sub_len):
            want = np_subseq(words, n_len, start, sub_len, rev)
            for ph in range(16):
                buf.fill_(SENTINEL)
                got = po.subseq_dev(dwords, n_len, start, sub_len, revcomp=rev, out=buf[8 + ph : 8 + ph + R])
                assert got.data_ptr() == buf.data_ptr() + 8 * (8 + ph)
                b = buf.cpu().numpy()
                assert np.array_equal(b[8 + ph : 8 + ph + R].view(U64), want), (rev, start, ph)
                assert (b[: 8 + ph] == SENTINEL).all() and (b[8 + ph + R :] == SENTINEL).all(), (rev, start, ph)


def _info_modes(rng, n):
    low = rng.integers(0, 256, n).astype(U64) | (rng.integers(0, 2, n).astype(U64) << U64(9)) | (rng.integers(0, 2, n).astype(U64) << U64(63))
    return {"absent": None, "forward": np.zeros(n, dtype=U64), "reversed": np.full(n, CNT_FIND_REVERSE, dtype=U64),
            "mixed": low | (rng.integers(0, 2, n).astype(U64) * U64(CNT_FIND_REVERSE))}


def _host_extract(L, bits, n_len, starts, info, region_len, flags, out, out_words, rejected=True):
    r = ctypes.c_uint64(0xDEAD)
    rc = L.cnt_extract(bits.ctypes.data, n_len, starts.ctypes.data, info.ctypes.data if info is not None else None, starts.size, region_len, flags,
                       out.ctypes.data, out_words, ctypes.byref(r) if rejected else None)
    return rc, r.value


@gpu
@pytest.mark.parametrize("region_len", [1, 23, 32, 33, 100, TILE + 7, 2 * TILE])
def test_gpu_extract_both_tiers(oracle, region_len):
    """n windows at random starts plus start = 0 and start = len - region_len, info absent / all forward / all reversed / mixed
    with other bits set, the flag on and off: every XOR combination, both tiers, against the numpy reference"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(region_len)
    n_len = 100000 + 13
    words = random_words(oracle, rng, n_len)
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    R = words_for(region_len)
    for n in ((1, 2, 3) if region_len > TILE else (1, 2, 257, 5000)):
        starts = rng.integers(0, n_len - region_len + 1, n).astype(U64)
        starts[0] = n_len - region_len
        if n > 1:
            starts[1] = 0
        dstarts = torch.from_numpy(starts.view(np.int64)).cuda()
        for mode, info in _info_modes(rng, n).items():
            dinfo = torch.from_numpy(info.view(np.int64)).cuda() if info is not None else None
            for flag in (False, True):
                want, _ = np_extract(words, n_len, starts, region_len, info, flag)
                tag = (region_len, n, mode, flag)
                if n <= 2 and region_len <= 100:
                    assert np.array_equal(want, def_extract(oracle, words, n_len, starts, region_len, info, flag)[0]), tag
                rec, rej = po.extract_dev(dwords, n_len, dstarts, region_len, info=dinfo, revcomp=flag)
                assert rec.shape == (n, R) and int(rej.item()) == 0 and np.array_equal(_dev_words(rec), want), tag + ("device",)
                rec, rej = po.extract_hip(words[: words_for(n_len)], n_len, starts, region_len, info=info, revcomp=flag)
                assert rec.shape == (n, R) and rej == 0 and np.array_equal(rec, want), tag + ("host",)


@gpu
def test_gpu_rejected_regions_counter_and_sentinels(oracle, L):
    """regions that do not lie inside the sequence, among valid ones: start = len - region_len + 1, len + 1, 2^64 - 1, and
    region_len > len; zero records, the device counter grown by their number over a non-zero value, the host counter SET,
    NULL counters, and sentinels in front of out and behind out[n*R) untouched"""
    import torch

    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(21)
    n_len = 4 * TILE + 21
    words = random_words(oracle, rng, n_len)
    src = np.ascontiguousarray(words[: words_for(n_len)])
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    for region_len in (23, 100, TILE + 7, 2 * TILE, n_len + 1):
        R = words_for(region_len)
        bad = [n_len - region_len + 1, n_len + 1, MAX64, MAX64 - 31, n_len + (1 << 40)] if region_len <= n_len else []
        good = [0, 5, n_len - region_len] if region_len <= n_len else [0, 1, n_len]
        starts = np.array([good[0], *bad[:2], good[1], *bad[2:], good[2]], dtype=U64)
        n = starts.size
        n_bad = len(bad) if region_len <= n_len else n
        info = _info_modes(rng, n)["mixed"]
        for inf in (None, info):
            for flag in (False, True):
                want, wr = np_extract(words, n_len, starts, region_len, inf, flag)
                assert wr == n_bad and (want[[1, 2]] == 0).all() and (region_len > n_len or want[[0, 3]].any())
                tag = (region_len, inf is None, flag)
                buf = torch.full((n * R + 16,), SENTINEL, dtype=torch.int64, device="cuda")
                cnt = torch.full((3,), SENTINEL, dtype=torch.int64, device="cuda")
                cnt[1] = 1000
                dinfo = torch.from_numpy(inf.view(np.int64)).cuda() if inf is not None else None
                rec, rej = po.extract_dev(dwords, n_len, torch.from_numpy(starts.view(np.int64)).cuda(), region_len, info=dinfo, revcomp=flag,
                                          out=buf[8 : 8 + n * R], rejected=cnt[1:2])
                b, c = buf.cpu().numpy(), cnt.cpu().numpy()
                assert np.array_equal(b[8 : 8 + n * R].view(U64).reshape(n, R), want), tag
                assert (b[:8] == SENTINEL).all() and (b[8 + n * R :] == SENTINEL).all(), tag
                assert c[1] == 1000 + n_bad and c[0] == SENTINEL and c[2] == SENTINEL, (tag, c)
                # d_rejected = NULL
                buf.fill_(SENTINEL)
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                dst = torch.from_numpy(starts.view(np.int64)).cuda()
                assert L.cnt_extract_dev(dwords.data_ptr(), n_len, dst.data_ptr(), dinfo.data_ptr() if inf is not None else None, n, region_len,
                                         CNT_EXTRACT_REVCOMP if flag else 0, buf.data_ptr() + 64, n * R + 3, None, stream) == _lib.CNT_OK
                assert np.array_equal(buf.cpu().numpy()[8 : 8 + n * R].view(U64).reshape(n, R), want), tag
                # host tier: *rejected is SET (over a poisoned value); NULL works
                hout = np.full(n * R + 8, HOST_SENTINEL, dtype=U64)
                rc, hr = _host_extract(L, src, n_len, starts, inf, region_len, CNT_EXTRACT_REVCOMP if flag else 0, hout[4:], n * R + 2)
                assert rc == _lib.CNT_OK and hr == n_bad, (tag, rc, hr)
                assert np.array_equal(hout[4 : 4 + n * R].reshape(n, R), want) and (hout[:4] == HOST_SENTINEL).all() and (hout[4 + n * R :] == HOST_SENTINEL).all(), tag
                hout[:] = HOST_SENTINEL
                rc, _ = _host_extract(L, src, n_len, starts, inf, region_len, CNT_EXTRACT_REVCOMP if flag else 0, hout[4:], n * R, rejected=False)
                assert rc == _lib.CNT_OK and np.array_equal(hout[4 : 4 + n * R].reshape(n, R), want), tag


@gpu
def test_gpu_search_then_extract_end_to_end(oracle):
    """find_pattern_dev on both strands over planted, mutated occurrences, then extract_dev with its pos and info as they are:
    every record, read forward, is within the hit's reported mismatch count of the pattern"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_find_pattern import mutated, pack_pattern, random_pattern, revcomp_pattern

    rng = np.random.default_rng(77)
    k, d, n_len = 23, 3, 200000 + 9
    codes, wild = random_pattern(rng, k, 0)
    pat = pack_pattern(codes, wild)
    s = rng.integers(0, 4, n_len).astype(np.uint8)
    sites = [int(v) * 50 + 3 for v in rng.permutation(n_len // 50 - 1)[:40]] + [0, n_len - k]
    for j, site in enumerate(sites):
        Q, V = revcomp_pattern(codes, wild) if j & 1 else (codes, wild)
        s[site : site + k] = mutated(rng, Q, V, j % (d + 1))
    words = words_of_codes(oracle, s, extra=1, rng=rng)
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    pos, info, count = po.find_pattern_dev(dwords, n_len, pat, d, both_strands=True)
    n = int(count.item())
    assert n >= len(sites)
    rec, rej = po.extract_dev(dwords, n_len, pos[:n].contiguous(), k, info=info[:n].contiguous())
    got, inf, p = _dev_words(rec).reshape(-1), _dev_words(info[:n]), _dev_words(pos[:n])
    assert int(rej.item()) == 0 and got.shape == (n,)
    y = got ^ U64(pat[0])
    dist = np.bitwise_count((y | (y >> U64(1))) & U64(0x5555555555555555))
    assert (got >> U64(2 * k) == 0).all() and np.array_equal(dist, inf & U64(0xFF)), (dist, inf)
    assert (dist <= d).all() and ((inf & U64(CNT_FIND_REVERSE)) != 0).sum() >= len(sites) // 2 and set(sites) <= set(int(v) for v in p)


@gpu
def test_gpu_tiles_across_launch_edges(oracle, launch_tiles):
    """the lab build cut into launches of 64 / 128 tiles: a tiled subsequence (forward and reversed) and a many-window extract
    whose word-kernel workgroups span several launches, with the launches counted in a captured graph"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(launch_tiles)
    sub_len = launch_tiles * TILE * 2 + TILE + 16 * 32 + 40  # 18 words behind the tiles: a head peel of up to 15 leaves their number as it is
    n_len = sub_len + 77
    words = random_words(oracle, rng, n_len)
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    out = torch.empty(words_for(sub_len) + 16, dtype=torch.int64, device="cuda")
    for rev in (False, True):
        for start, ph in ((0, 0), (45, 0), (77, 5)):
            got = po.subseq_dev(dwords, n_len, start, sub_len, revcomp=rev, out=out[ph : ph + words_for(sub_len)])
            assert np.array_equal(_dev_words(got), np_subseq(words, n_len, start, sub_len, rev)), (rev, start, ph)
            head = (16 - ph) % 16
            want = extract_plan(1, sub_len, head=head, launch_tiles=launch_tiles)
            assert want == 3 + 1 + (1 if head else 0)
            assert _kernel_nodes_of(torch, lambda: po.subseq_dev(dwords, n_len, start, sub_len, revcomp=rev, out=out[ph : ph + words_for(sub_len)])) == want
    for n, region_len in ((70000, 33), (3 * launch_tiles + 5, TILE + 7)):
        starts = rng.integers(0, n_len - region_len + 1, n).astype(U64)
        info = _info_modes(rng, n)["mixed"]
        dstarts, dinfo = torch.from_numpy(starts.view(np.int64)).cuda(), torch.from_numpy(info.view(np.int64)).cuda()
        rec, rej = po.extract_dev(dwords, n_len, dstarts, region_len, info=dinfo)
        assert np.array_equal(_dev_words(rec), np_extract(words, n_len, starts, region_len, info)[0]) and int(rej.item()) == 0
        want = extract_plan(n, region_len, both=True, launch_tiles=launch_tiles)
        assert want >= 5
        assert _kernel_nodes_of(torch, lambda: po.extract_dev(dwords, n_len, dstarts, region_len, info=dinfo, out=rec.view(-1), rejected=rej)) == want
        hrec, hrej = po.extract_hip(words[: words_for(n_len)], n_len, starts, region_len, info=info)
        assert np.array_equal(hrec, _dev_words(rec)) and hrej == 0


@gpu
def test_gpu_extract_in_a_captured_graph_on_a_side_stream(oracle):
    """extract_dev captured with torch.cuda.graph on a side stream and replayed twice on changed starts and strands"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(3)
    n_len, n = (1 << 18) + 11, 3000
    words = random_words(oracle, rng, n_len)
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    outs = []
    for region_len in (101, TILE + 33):
        m = n if region_len < TILE else 3
        dstarts = torch.zeros(m, dtype=torch.int64, device="cuda")
        dinfo = torch.zeros(m, dtype=torch.int64, device="cuda")
        rec = torch.empty(m * words_for(region_len), dtype=torch.int64, device="cuda")
        rej = torch.zeros(1, dtype=torch.int64, device="cuda")
        outs.append((region_len, m, dstarts, dinfo, rec, rej))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for region_len, m, dstarts, dinfo, rec, rej in outs:  # module load outside the capture
            po.extract_dev(dwords, n_len, dstarts, region_len, info=dinfo, out=rec, rejected=rej)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for region_len, m, dstarts, dinfo, rec, rej in outs:
            po.extract_dev(dwords, n_len, dstarts, region_len, info=dinfo, revcomp=True, out=rec, rejected=rej)
    for rep in range(2):
        want = []
        for region_len, m, dstarts, dinfo, rec, rej in outs:
            starts = rng.integers(0, n_len - region_len + 1, m).astype(U64)
            starts[rep] = n_len  # one rejected region per replay
            info = _info_modes(rng, m)["mixed"]
            dstarts.copy_(torch.from_numpy(starts.view(np.int64)))
            dinfo.copy_(torch.from_numpy(info.view(np.int64)))
            rec.fill_(SENTINEL)
            rej.fill_(10 * rep)
            want.append(np_extract(words, n_len, starts, region_len, info, True))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for (region_len, m, dstarts, dinfo, rec, rej), (w, wr) in zip(outs, want):
            assert wr == 1 and int(rej.item()) == 10 * rep + 1, (rep, region_len)
            assert np.array_equal(_dev_words(rec).reshape(w.shape), w), (rep, region_len)


@gpu
def test_gpu_pinned_in_place_equals_staged(oracle, L):
    """cnt_extract with every buffer pinned (used in place, the kernels reading and writing host memory over the link) against
    ordinary ones (staged) and against only some pinned (staged): identical results, at a phase inside the pinned allocations"""
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    rng = np.random.default_rng(9)
    n_len = 3 * TILE + 77
    words = random_words(oracle, rng, n_len)
    src = words[: words_for(n_len)]
    for n, region_len in ((300, 100), (3, TILE + 7)):
        R = words_for(region_len)
        starts = rng.integers(0, n_len - region_len + 1, n).astype(U64)
        starts[1] = n_len - region_len + 1  # rejected
        info = _info_modes(rng, n)["mixed"]
        want, wr = np_extract(words, n_len, starts, region_len, info, True)
        for pin_in, pin_out in ((False, False), (True, True), (True, False), (False, True)):
            bits = cn.pinned_empty(src.size + 3, U64)[3:] if pin_in else src.copy()
            hs = cn.pinned_empty(n + 1, U64)[1:] if pin_in else starts.copy()
            hi = cn.pinned_empty(n + 1, U64)[1:] if pin_in else info.copy()
            bits[:], hs[:], hi[:] = src, starts, info
            out = cn.pinned_empty(n * R + 9, U64)[1:] if pin_out else np.empty(n * R + 8, dtype=U64)
            out[:] = HOST_SENTINEL
            if pin_in and pin_out:
                assert all(L.cnt_host_is_pinned(a.ctypes.data, a.nbytes) == 1 for a in (bits, hs, hi, out))
            rc, hr = _host_extract(L, bits, n_len, hs, hi, region_len, CNT_EXTRACT_REVCOMP, out, n * R + 8)
            assert rc == _lib.CNT_OK and hr == wr == 1, (region_len, pin_in, pin_out, rc, hr)
            assert np.array_equal(out[: n * R].reshape(n, R), want) and (out[n * R :] == HOST_SENTINEL).all(), (region_len, pin_in, pin_out)


@gpu
@pytest.mark.parametrize("seed", range(4))
def test_gpu_extract_fuzz(oracle, L, seed):
    """random lengths, counts, region lengths, starts (some outside), info, flags and input phases; both tiers"""
    import torch

    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(9100 + seed)
    for it in range(30):
        n_len = int(rng.choice([rng.integers(0, 300), rng.integers(0, 3 * TILE), rng.integers(0, 1 << 20)]))
        region_len = int(rng.choice([rng.integers(0, 70), rng.integers(0, 2000), rng.integers(0, 4 * TILE)]))
        R = words_for(region_len)
        n = int(rng.integers(0, max(2, min(3000, (1 << 17) // max(R, 1)))))
        hi = max(n_len - region_len, 0) + (2 if it % 3 == 0 else 1)  # a third of the iterations draw starts one past the last valid one
        starts = rng.integers(0, hi, n).astype(U64)
        if n and it % 5 == 0:
            starts[int(rng.integers(0, n))] = U64(MAX64 - int(rng.integers(0, 64)))
        info = _info_modes(rng, n)[str(rng.choice(["absent", "forward", "reversed", "mixed"]))]
        flag, pi = bool(rng.integers(0, 2)), int(rng.integers(0, 4))
        allw = np.concatenate([rng.integers(0, 2**64, pi, dtype=U64), random_words(oracle, rng, n_len)])
        nw = max(words_for(n_len), 1)
        src = np.ascontiguousarray(allw[pi : pi + nw])
        want, wr = np_extract(allw[pi:], n_len, starts, region_len, info, flag)
        tag = (seed, it, n_len, n, region_len, flag, pi)
        dall = torch.from_numpy(allw.view(np.int64)).cuda()
        buf = torch.full((n * R + 8,), SENTINEL, dtype=torch.int64, device="cuda")
        dinfo = torch.from_numpy(info.view(np.int64)).cuda() if info is not None else None
        rec, rej = po.extract_dev(dall[pi : pi + nw], n_len, torch.from_numpy(starts.view(np.int64)).cuda(), region_len, info=dinfo, revcomp=flag, out=buf[3 : 3 + n * R])
        b = buf.cpu().numpy()
        assert int(rej.item()) == (wr if region_len else 0), tag
        assert np.array_equal(b[3 : 3 + n * R].view(U64).reshape(n, R), want) and (b[:3] == SENTINEL).all() and (b[3 + n * R :] == SENTINEL).all(), tag
        hrec, hrej = po.extract_hip(src, n_len, starts, region_len, info=info, revcomp=flag)
        assert np.array_equal(hrec, want) and hrej == (wr if region_len else 0), tag
        if region_len <= n_len:
            start = int(rng.integers(0, n_len - region_len + 1))
            ws = np_subseq(allw[pi:], n_len, start, region_len, flag)
            assert np.array_equal(_dev_words(po.subseq_dev(dall[pi : pi + nw], n_len, start, region_len, revcomp=flag)), ws), tag
            assert np.array_equal(po.subseq_hip(src, n_len, start, region_len, revcomp=flag), ws), tag


@gpu
def test_gpu_extract_full_size_past_2p32(oracle, fullsize):
    """random packed words for 2^32 + 2^16 nt (1 GiB): a tiled subsequence and a few windows with start > 2^32, forward and
    reversed, against the reference computed from only the input words they touch"""
    import torch

    from conftest import need_free_hbm
    from cute_nucleotides_amd import packed_ops as po

    n_len = (1 << 32) + (1 << 16)
    need_free_hbm(3)
    torch.manual_seed(32)
    bits = torch.randint(-(1 << 63), (1 << 63) - 1, (words_for(n_len),), dtype=torch.int64, device="cuda")
    sub_len = 2 * TILE + 1000 + 7
    starts = [(1 << 32) + 12345, (1 << 32) + (1 << 16) - sub_len, (1 << 32) - 5]
    t0 = time.perf_counter()
    for start in starts:
        w0 = start >> 5
        piece = _dev_words(bits[w0 : w0 + words_for(sub_len) + 2])
        for rev in (False, True):
            got = _dev_words(po.subseq_dev(bits, n_len, start, sub_len, revcomp=rev))
            assert np.array_equal(got, np_subseq(piece, n_len, start, sub_len, rev, first_word=w0)), (start, rev)
    for region_len in (101, 1000):
        # windows in one neighbourhood past 2^32, so that the reference needs one slice of the input
        base = (1 << 32) + 4096 + 3
        win = np.array([base, base + 1, base + 31, base + 777, base + 20000, n_len - region_len], dtype=U64)
        w0 = base >> 5
        piece = _dev_words(bits[w0:])
        info = np.array([0, CNT_FIND_REVERSE, 3, CNT_FIND_REVERSE | 2, 0, CNT_FIND_REVERSE], dtype=U64)
        rec, rej = po.extract_dev(bits, n_len, torch.from_numpy(win.view(np.int64)).cuda(), region_len, info=torch.from_numpy(info.view(np.int64)).cuda())
        want, _ = np_extract(piece, n_len, win, region_len, info, False, first_word=w0)
        assert int(rej.item()) == 0 and np.array_equal(_dev_words(rec), want), region_len
    fullsize(32, (time.perf_counter() - t0) * 1e3, check="subseq + extract with start > 2^32: kernels and sliced references")
