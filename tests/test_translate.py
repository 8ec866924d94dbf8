"""Codon translation on packed words (include/cute_nt.h "translation"): nucleotides [start, start + sub_len) read in threes,
forward or as the reverse complement of the region, one table byte per codon.  Not in the reference, so the CPU part pins two
references against each other -- the definition as a literal per-codon loop over the codes read straight from the words, with
the standard code looked up in a dictionary of letters written out here, and a vectorised numpy form on the words -- checks the
tables of packed_ops.codon_table, the properties the definition implies, the Python layer's errors, every argument error of the
ABI in the order the header gives, the wiring, the ISA of the three kernels and the launch plan.  The GPU part compares both
tiers with the numpy reference byte for byte: every start phase mod 32 and mod 3 with the tile edges, every byte phase of the
output, custom tables and a table freed right after the call, tiles across launch edges on the lab build, a captured graph on
a side stream, pinned against staged host buffers, search -> translate end to end, a fuzz loop, and once past 2^32."""
import ctypes
import os
import re
import sys
import time

import numpy as np
import pytest

from test_extract import clean, np_subseq, random_words, words_for
from test_find_pattern import codes_of, words_of_codes
from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch
from test_kmers import assert_split_launches_by_max_tiles_per_launch, np_kmers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNT_TRANSLATE_REVCOMP = 0x80
T = 4096  # output bytes per workgroup tile (hip/translate_kernels.hpp kTranslateTileBytes): 12288 nt
U64 = np.uint64
MAX64 = (1 << 64) - 1
STANDARD = b"KQ*ETPSAILLVRR*GNHYDTPSAILFVSRCGNHYDTPSAILFVSRCGKQ*ETPSAMLLVRRWG"  # the header's string, index x0 | x1<<2 | x2<<4

# the standard genetic code, codon by codon in letters (NCBI table 1)
CODON_AA = {
    "TTT": "F", "TTC": "F", "TTA": "L", "TTG": "L", "TCT": "S", "TCC": "S", "TCA": "S", "TCG": "S",
    "TAT": "Y", "TAC": "Y", "TAA": "*", "TAG": "*", "TGT": "C", "TGC": "C", "TGA": "*", "TGG": "W",
    "CTT": "L", "CTC": "L", "CTA": "L", "CTG": "L", "CCT": "P", "CCC": "P", "CCA": "P", "CCG": "P",
    "CAT": "H", "CAC": "H", "CAA": "Q", "CAG": "Q", "CGT": "R", "CGC": "R", "CGA": "R", "CGG": "R",
    "ATT": "I", "ATC": "I", "ATA": "I", "ATG": "M", "ACT": "T", "ACC": "T", "ACA": "T", "ACG": "T",
    "AAT": "N", "AAC": "N", "AAA": "K", "AAG": "K", "AGT": "S", "AGC": "S", "AGA": "R", "AGG": "R",
    "GTT": "V", "GTC": "V", "GTA": "V", "GTG": "V", "GCT": "A", "GCC": "A", "GCA": "A", "GCG": "A",
    "GAT": "D", "GAC": "D", "GAA": "E", "GAG": "E", "GGT": "G", "GGC": "G", "GGA": "G", "GGG": "G",
}
NT = "ACTG"  # code order A0 C1 T2 G3
DICT_TABLE = np.array([ord(CODON_AA[NT[c & 3] + NT[(c >> 2) & 3] + NT[c >> 4]]) for c in range(64)], dtype=np.uint8)
IDENTITY = np.arange(64, dtype=np.uint8)


# ---- references -------------------------------------------------------------------------------------------------------
def def_translate(words, length, start, sub_len, rev=False, table=None):
    """the definition, literally, codon by codon on the codes of the sequence; the standard code through the dictionary"""
    s = codes_of(words, length)
    out = bytearray()
    for j in range(sub_len // 3):
        if rev:
            r = [int(s[start + sub_len - 1 - (3 * j + i)]) ^ 2 for i in range(3)]
        else:
            r = [int(s[start + 3 * j + i]) for i in range(3)]
        if table is None:
            out.append(ord(CODON_AA[NT[r[0]] + NT[r[1]] + NT[r[2]]]))
        else:
            out.append(int(table[r[0] | r[1] << 2 | r[2] << 4]))
    return np.frombuffer(bytes(out), dtype=np.uint8)


def np_translate(words, length, start, sub_len, rev=False, table=None, first_word=0):
    """the vectorised reference on the words: every codon is the low 6 bits of one 64-bit window of the input; reversed, the
    forward codon at start + sub_len - 3 - 3j with its outer codes swapped and all three complemented.  `words` holds the input
    from word `first_word` on (only the words the region touches need to be there)"""
    w = np.concatenate([np.asarray(words, dtype=U64), np.zeros(2, dtype=U64)])
    M = sub_len // 3
    j = np.arange(M, dtype=np.int64)
    p = (start - 32 * first_word) + (sub_len - 3 - 3 * j if rev else 3 * j)
    iw, sh = p >> 5, (2 * (p & 31)).astype(U64)
    v = (w[iw] >> sh) | np.where(sh > 0, (w[iw + 1] << U64(1)) << (U64(63) - sh), U64(0))
    c = (v & U64(63)).astype(np.int64)
    if rev:
        c = ((c >> 4) | (c & 12) | ((c & 3) << 4)) ^ 0x2A
    tab = DICT_TABLE if table is None else np.frombuffer(bytes(table), dtype=np.uint8)
    return tab[c]


def ascii_translate(s):
    return np.frombuffer("".join(CODON_AA[s[i : i + 3]] for i in range(0, len(s) - len(s) % 3, 3)).encode(), dtype=np.uint8)


def random_table(rng):
    t = rng.integers(0, 256, 64).astype(np.uint8)
    t[int(rng.integers(0, 32))] = 0x00
    t[32 + int(rng.integers(0, 32))] = 0xFF
    return t


# ---- CPU: the references ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev", [False, True])
def test_numpy_reference_against_the_definition(oracle, rev):
    rng = np.random.default_rng(31 + rev)
    n_len = 32 * 5 + 13  # 173 >= 95 + 70, len % 32 != 0
    words = random_words(oracle, rng, n_len)
    table = random_table(rng)
    for start in range(96):
        for sub_len in range(71):
            for tab in (None, table):
                want = def_translate(words, n_len, start, sub_len, rev, tab)
                got = np_translate(words, n_len, start, sub_len, rev, tab)
                assert got.dtype == np.uint8 and got.shape == (sub_len // 3,) and np.array_equal(got, want), (start, sub_len, rev, tab is None)
    # the same from a slice of the words: only the words a region touches
    assert np.array_equal(np_translate(words[2:], n_len, 32 * 2 + 5, 100, rev, first_word=2), def_translate(words, n_len, 32 * 2 + 5, 100, rev))


def test_codon_tables():
    from cute_nucleotides_amd import packed_ops as po

    assert po.codon_table(1) == STANDARD == bytes(DICT_TABLE) == po.codon_table() and len(STANDARD) == 64
    assert po.codon_table(11) == po.codon_table(1)
    index = lambda codon: NT.index(codon[0]) | NT.index(codon[1]) << 2 | NT.index(codon[2]) << 4  # noqa: E731
    for ncbi_id, changed in ((2, {"TGA": "W", "ATA": "M", "AGA": "*", "AGG": "*"}), (4, {"TGA": "W"})):
        t = po.codon_table(ncbi_id)
        differ = {c for c in range(64) if t[c] != STANDARD[c]}
        assert differ == {index(codon) for codon in changed}, (ncbi_id, differ)
        for codon, aa in changed.items():
            assert chr(t[index(codon)]) == aa, (ncbi_id, codon)
    for bad in (0, 3, 12, "1", None):
        with pytest.raises(ValueError):
            po.codon_table(bad)


def test_properties(oracle):
    rng = np.random.default_rng(6)
    table = random_table(rng)
    for n_len in (3, 31, 32, 33, 700, 3 * T + 77):
        words = random_words(oracle, rng, n_len)
        kmers = np_kmers(words, n_len, 3)
        for _ in range(8):
            a = int(rng.integers(0, n_len + 1))
            l = int(rng.integers(0, n_len - a + 1))
            for tab in (None, table):
                fwd = np_translate(words, n_len, a, l, False, tab)
                sub = np.concatenate([np_subseq(words, n_len, a, l), np.zeros(1, dtype=U64)])
                # the region's own record, translated from its start 0
                assert np.array_equal(np_translate(sub, l, 0, l, False, tab), fwd), (n_len, a, l)
                assert np.array_equal(np_translate(sub, l, 0, l, True, tab), np_translate(words, n_len, a, l, True, tab)), (n_len, a, l)
                if l:
                    # reversed = forward on the oracle's reverse complement of the region
                    rc = np.concatenate([oracle.reverse_complement(sub[:-1], l), np.zeros(1, dtype=U64)])
                    assert np.array_equal(np_translate(words, n_len, a, l, True, tab), np_translate(rc, l, 0, l, False, tab)), (n_len, a, l)
            # the identity table returns the codon values: every third 3-mer
            assert np.array_equal(np_translate(words, n_len, a, l, False, IDENTITY), kmers[a : a + l - 2 : 3].astype(np.uint8)[: l // 3]), (n_len, a, l)
    # the six frames of a decoded sequence
    n_len = 1000 + 7
    words = random_words(oracle, rng, n_len)
    s = bytes(oracle.bits_to_n_lut(clean(words, n_len), n_len)).decode()
    rc = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    for f in range(3):
        assert np.array_equal(np_translate(words, n_len, f, n_len - f), ascii_translate(s[f:]))
        assert np.array_equal(np_translate(words, n_len, 0, n_len - f, True), ascii_translate(rc[f:]))


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
    for start, sub_len in ((65, 0), (0, 65), (60, 5), (-1, 3), (3, -1), (1 << 64, 1), (65, None)):
        with pytest.raises(ValueError):
            po.translate_hip(w, 64, start, sub_len)
    with pytest.raises(ValueError):
        po.translate_hip(w, 65, 0, 3)  # longer than the words hold
    with pytest.raises(TypeError):
        po.translate_hip(w.astype(np.int64), 64, 0, 3)
    for table in (b"", b"A" * 63, b"A" * 65, bytearray(10), np.zeros(63, dtype=np.uint8), np.zeros((8, 9), dtype=np.uint8)):
        with pytest.raises(ValueError):
            po.translate_hip(w, 64, 0, 30, table=table)
    for table in ("A" * 64, list(range(64)), np.zeros(64, dtype=np.int8), np.zeros(64, dtype=np.uint64), 5):
        with pytest.raises(TypeError):
            po.translate_hip(w, 64, 0, 30, table=table)
    # the device wrappers check before the library is called: CPU tensors are refused
    tw = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError):
        po.translate_dev(tw, 64, 0, 30)
    with pytest.raises(ValueError):
        po.six_frames_dev(tw, 64)
    # sub_len < 3 is answered without a device
    for start, sub_len, rev in ((0, 0, False), (64, 0, True), (7, 2, False), (62, None, True), (63, 1, False)):
        got = po.translate_hip(w, 64, start, sub_len, revcomp=rev, table=bytes(IDENTITY))
        assert got.dtype == np.uint8 and got.size == 0
    assert [f.size for f in po.six_frames_hip(w, 2)] == [0] * 6 and [f.size for f in po.six_frames_hip(w, 0)] == [0] * 6


def test_abi_errors_come_before_any_device_work(L):
    from cute_nucleotides_amd import _lib

    buf = np.zeros(4096, dtype=U64)
    q = lambda word, byte=0: ctypes.c_void_p(buf.ctypes.data + 8 * word + byte)  # noqa: E731
    out = np.full(4096, 0x5A, dtype=np.uint8)
    o = lambda byte=0: ctypes.c_void_p(out.ctypes.data + byte)  # noqa: E731
    table = (ctypes.c_uint8 * 64)(*range(64))
    EINVAL, ECAP, OK = _lib.CNT_EINVAL, _lib.CNT_ECAP, _lib.CNT_OK
    for dev in (False, True):
        def translate(bits, n_len, start, sub_len, flags, tab, dst, out_cap):
            if dev:
                return L.cnt_translate_dev(bits, n_len, start, sub_len, flags, tab, dst, out_cap, None)
            return L.cnt_translate(bits, n_len, start, sub_len, flags, tab, dst, out_cap)

        tag = "dev" if dev else "host"
        # 100 nt = 4 words at q(10), nucleotides [7, 47): M = 13 bytes at o(100), an odd address
        ok = (q(10), 100, 7, 40, 0, table, o(101), 13)
        # 1. every unknown flag bit, alone and beside the known one, even without work and with bad everything else
        unknown = [1 << b for b in range(32) if (1 << b) != CNT_TRANSLATE_REVCOMP] + [CNT_TRANSLATE_REVCOMP | 0x1, CNT_TRANSLATE_REVCOMP | 0x40, 0xFFFFFFFF]
        assert 0x40 in unknown and 0x100 in unknown
        for flags in unknown:
            assert translate(*ok[:4], flags, *ok[5:]) == EINVAL, (tag, flags)
            assert translate(None, 0, 0, 0, flags, None, None, 0) == EINVAL, (tag, flags)
            assert translate(None, 100, 500, 2, flags, None, None, 0) == EINVAL, (tag, flags)
        # 2. sub_len < 3: CNT_OK, whatever the pointers and start are
        for sub_len in (0, 1, 2):
            for flags in (0, CNT_TRANSLATE_REVCOMP):
                assert translate(None, 100, 0, sub_len, flags, None, None, 0) == OK
                assert translate(None, 100, 500, sub_len, flags, None, None, 0) == OK
                assert translate(q(10, 3), 100, MAX64, sub_len, flags, table, q(10), 0) == OK
        # 3. bounds, before the pointers are looked at
        for start, sub_len in ((101, 3), (100, 3), (98, 3), (61, 40), (0, 101), (MAX64, 3), (2, MAX64)):
            assert translate(q(10), 100, start, sub_len, 0, table, o(0), 4096) == EINVAL, (tag, start, sub_len)
            assert translate(None, 100, start, sub_len, 0, None, None, 0) == EINVAL, (tag, start, sub_len)
        # 4. NULL bits or out (the table may be NULL), bits not 8-B aligned, out overlapping the input words
        assert translate(None, *ok[1:]) == EINVAL and translate(*ok[:6], None, 13) == EINVAL
        for byte in (1, 2, 4, 7):
            assert translate(q(10, byte), *ok[1:]) == EINVAL, (tag, byte)
        for word, byte in ((10, 0), (13, 7), (9, 0), (8, 4), (11, 3)):  # 13 bytes against words 10..13
            assert translate(*ok[:6], q(word, byte), 13) == EINVAL, (tag, word, byte)
        # ... before the capacity is
        assert translate(*ok[:6], q(10), 0) == EINVAL and translate(None, *ok[1:7], 0) == EINVAL
        # 5. capacity, in bytes
        assert translate(*ok[:7], 12) == ECAP and translate(*ok[:7], 0) == ECAP
        assert translate(q(10), 100, 0, 100, CNT_TRANSLATE_REVCOMP, None, o(0), 32) == ECAP
    assert (out == 0x5A).all() and not buf.any()  # nothing was written
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        assert L.cnt_translate(q(10), 100, 7, 40, 0, table, o(101), 13) == _lib.CNT_ENODEV
        assert L.cnt_translate(q(10), 100, 0, 100, CNT_TRANSLATE_REVCOMP, None, o(0), 33) == _lib.CNT_ENODEV
        assert L.cnt_translate(q(14), 100, 7, 40, 0, None, q(14, -13), 13) == _lib.CNT_ENODEV  # out ends where the words begin
        assert L.cnt_translate_dev(q(10), 100, 7, 40, 0, table, o(101), 13, None) < 0
        assert (out == 0x5A).all()


def test_abi_wiring(L):
    import subprocess

    from cute_nucleotides_amd import _lib, packed_ops as po

    names = ("cnt_translate", "cnt_translate_dev")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    mirror = open(os.path.join(ROOT, "cute_nucleotides_amd", "cute_nucleotides.hpp")).read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(L, name) and name in exported and name + "(" in header
        assert "fn %s(" % name in rust and "check(%s(" % name in rust and "detail::check(%s(" % name in mirror
    assert "#define CNT_TRANSLATE_REVCOMP 0x80u" in header and _lib.CNT_TRANSLATE_REVCOMP == CNT_TRANSLATE_REVCOMP
    assert STANDARD.decode() in header and STANDARD.decode() in open(os.path.join(ROOT, "hip", "translate_abi.inc")).read()
    for sig in (r"pub fn translate_hip\(", r"pub fn translate_hip_dev\(", r"const CNT_TRANSLATE_REVCOMP: c_uint = 0x80;"):
        assert re.search(sig, rust), sig
    for sig in ("inline Vec<uint8_t> translate_hip(", "inline void translate_hip_dev("):
        assert sig in mirror, sig
    for name in ("translate_hip", "translate_dev", "six_frames_hip", "six_frames_dev", "codon_table"):
        assert callable(getattr(po, name)), name


# ---- CPU: the ISA and the launch plan ---------------------------------------------------------------------------------
TRANSLATE_KERNELS = ["translate_edge", "translate_tiles_fwd", "translate_tiles_rev"]


def test_translate_kernels_isa():
    """the three kernels from the product's gfx950 assembly: no scratch, no spills, <= 84 VGPRs, an LDS segment of the 64 table
    bytes; the tile kernels reach global memory through raw-buffer instructions only, every load in flight before the first
    wait for memory, `nt` loads and `sc0 sc1 nt` stores, with no waterfall loop, and look the codons up in LDS.  Properties
    only: how many instructions the compiler makes of them is not pinned"""
    sys.path.insert(0, os.path.join(ROOT, "bench"))
    import isa_digest

    asm = isa_digest.assembly()
    for name in TRANSLATE_KERNELS:
        m = re.search(r"^cnt::%s\(.*?\): +; @(.*?)\.end_amdhsa_kernel" % name, asm, re.S | re.M)
        assert m, name + " not in the product's assembly"
        text = m.group(1)
        body = [l.strip().split(";")[0].strip() for l in text.splitlines() if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        assert "scratch_" not in text, name
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", text), name
        assert re.search(r"\.amdhsa_group_segment_fixed_size\s+64\b", text), name
        assert int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", text).group(1)) <= 84, name
        meta = re.search(r"\.name:\s+cnt::%s\(.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)" % name, asm, re.S)
        assert meta and meta.group(1) == "0" and meta.group(2) == "0", (name, meta and meta.groups())
        if "tiles" not in name:
            continue
        t = isa_digest.summarise({"body": body}, False)
        assert "s_xor_b64 exec, exec" not in text, name
        assert "global_load" not in t["counts"] and "global_store" not in t["counts"] and "flat_" not in text, (name, t["counts"])
        ops = [ins.split()[0] for ins in body if ins]
        assert any(op.startswith("buffer_load") for op in ops) and any(op.startswith("buffer_store") for op in ops), name
        assert t["loads"] >= 1 and t["loads_before_first_wait"] == t["loads"], (name, t["loads_before_first_wait"], t["loads"])
        assert t["load_policies"] == ["nt"] and t["store_policies"] == ["sc0 nt sc1"], name
        assert any(op.startswith("ds_read") for op in ops), name
    assert len(isa_digest.kernels(asm)) < 60  # the product's templated kernels: none added


HW_LAUNCH_TILES = ((0x7FFFFFFF // 256) // 64) * 64  # max_tiles_per_launch(256) of the product build


def translate_split(sub_len, out_phase=0):
    """(head, tiles) of a device call: the bytes the edge kernel takes in front of the first 16-B boundary of the output and the
    whole tiles behind it.  Without a whole tile behind the boundary there is no tile and no head: the edge kernel takes it all,
    so no tile ever starts off a 16-B boundary"""
    M = sub_len // 3
    head = (16 - out_phase % 16) % 16
    tiles = 0 if M < head + T else (M - head) // T
    if not tiles:
        head = 0
    assert (out_phase + head) % 16 == 0 or not tiles
    return head, tiles


def translate_plan(sub_len, out_phase=0, launch_tiles=HW_LAUNCH_TILES):
    """kernel launches of a device call: the tiles behind the first 16-B boundary of the output in launches of launch_tiles, then
    the edge kernel once on the bytes in front of the boundary and once on those behind the last tile"""
    M = sub_len // 3
    if sub_len < 3:
        return 0
    head, tiles = translate_split(sub_len, out_phase)
    return -(-tiles // launch_tiles) + (1 if head else 0) + (1 if head + tiles * T < M else 0)


def test_translate_plan_matches_the_launcher_and_splitter_source():
    src = open(os.path.join(ROOT, "hip", "translate_kernels.hpp")).read()
    assert "constexpr int kTranslateBlock = 256;" in src and "constexpr uint32_t kTranslateTileBytes = 16 * kTranslateBlock;" in src
    assert T == 16 * 256
    abi = open(os.path.join(ROOT, "hip", "translate_abi.inc")).read()
    for line in ("if (sub_len < 3) return CNT_OK;",
                 "const size_t M = sub_len / 3;",
                 "uint64_t head = (16 - (reinterpret_cast<uintptr_t>(a.out) & 15)) & 15;",
                 "const uint64_t tiles = M < head + kTranslateTileBytes ? 0 : (M - head) / kTranslateTileBytes;",
                 "if (!tiles) head = 0;  // no tile behind the boundary: one edge launch on [0, M)",
                 "split_launches(tiles, kTranslateBlock, [&](uint64_t first, uint64_t count) {",
                 "if (head) edge(0, head);",
                 "if (head + tiles * kTranslateTileBytes < M) edge(head + tiles * kTranslateTileBytes, M);"):
        assert line in abi, line
    assert abi.count("hipLaunchKernelGGL(") == 2  # the tiles of the call's strand, the edge
    assert_split_launches_by_max_tiles_per_launch()
    assert HW_LAUNCH_TILES == 8388544
    assert translate_plan(2) == 0 and translate_plan(3) == 1 and translate_plan(3 * T - 1) == 1 and translate_plan(3 * T) == 1
    assert translate_plan(3 * T + 2) == 1 and translate_plan(3 * T + 3) == 2 and translate_plan(3 * T, 5) == 1
    # one tile's worth of bytes at an output that is off the boundary: no tile, one edge launch on all of it
    for ph in range(1, 16):
        head = 16 - ph
        for M in (T, T + 1, T + head - 1):
            if M < T + head:  # at phase 15 the head is one byte and T + 1 has its tile
                assert translate_split(3 * M, ph) == (0, 0) and translate_plan(3 * M, ph) == 1, (ph, M)
        assert translate_split(3 * (T + head), ph) == (head, 1) and translate_plan(3 * (T + head), ph) == 2
        assert translate_split(3 * (T + head + 1), ph) == (head, 1) and translate_plan(3 * (T + head + 1), ph) == 3
    assert translate_split(3 * T, 0) == (0, 1) and translate_split(3 * T, 16) == (0, 1) and translate_split(3 * T - 1, 0) == (0, 0)
    assert translate_plan(3 * (T + 10), 5) == 1 and translate_plan(3 * (T + 11), 5) == 2 and translate_plan(3 * (T + 12), 5) == 3 and translate_plan(3 * (2 * T + 5) + 1, 127) == 3
    assert translate_plan(3 * (129 * T + 7), 0, 64) == 4 and translate_plan(3 * 128 * T, 16, 64) == 2


# ---------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
SENTINEL = 0xA5
SUB_LENS = [3 * m + r for m in (1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 5) for r in (0, 1, 2)]


def _bytes(t):
    return t.cpu().numpy()


@gpu
@pytest.mark.parametrize("rev", [False, True])
def test_gpu_translate_every_phase_and_tile_edge_both_tiers(oracle, rev):
    """start at every phase 0..95 (all of mod 32 x mod 3) and at len - sub_len (len % 32 != 0), sub_len around every lane and
    tile edge with every remainder mod 3, both tiers, against the numpy reference.  The unused high bits of the last input
    word and the two words behind the input are random: the result must not depend on them."""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(200 + rev)
    n_len = 95 + max(SUB_LENS) + 32 * 3 + 13
    assert n_len % 32 and n_len % 3
    words = random_words(oracle, rng, n_len)
    words[words_for(n_len) - 1] |= U64(1) << U64(63)  # whatever the draw was, a bit above len is set
    assert not np.array_equal(clean(words, n_len), words[: words_for(n_len)])
    src = np.ascontiguousarray(words[: words_for(n_len)])
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    table = random_table(rng)
    for sub_len in SUB_LENS:
        for start in list(range(96)) + [n_len - sub_len]:
            assert start + sub_len <= n_len
            tab = None if start % 2 else table
            want = np_translate(words, n_len, start, sub_len, rev, tab)
            got = po.translate_dev(dwords, n_len, start, sub_len, revcomp=rev, table=tab)
            assert got.dtype == torch.uint8 and np.array_equal(_bytes(got), want), (sub_len, start, rev, "device")
            if start % 3 == 0 or start >= 96:  # the host tier stages the same kernels: a third of the phases
                assert np.array_equal(po.translate_hip(src, n_len, start, sub_len, revcomp=rev, table=tab), want), (sub_len, start, rev, "host")


@gpu
def test_gpu_six_frames_of_a_whole_sequence(oracle):
    """the six frames of a whole sequence of several tiles equal decoding it with the oracle and translating the letters with
    the dictionary, both tiers; sub_len=None reads to the end"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(12)
    for n_len in (3 * 3 * T + 3 * 77 + 2, 100, 5):
        words = random_words(oracle, rng, n_len)
        s = bytes(oracle.bits_to_n_lut(clean(words, n_len), n_len)).decode()
        rc = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
        want = [ascii_translate(s[f:]) for f in range(3)] + [ascii_translate(rc[f:]) for f in range(3)]
        dwords = torch.from_numpy(words.view(np.int64)).cuda()
        got = po.six_frames_dev(dwords, n_len)
        hgot = po.six_frames_hip(words[: words_for(n_len)], n_len, table=po.codon_table(11))
        assert len(got) == len(hgot) == 6
        for f in range(6):
            assert np.array_equal(_bytes(got[f]), want[f]), (n_len, f, "device")
            assert np.array_equal(hgot[f], want[f]), (n_len, f, "host")
        assert np.array_equal(_bytes(po.translate_dev(dwords, n_len, 1)), want[1])


@gpu
def test_gpu_translate_output_at_every_byte_phase(oracle):
    """d_out at each byte phase 0..15 of a 16-B unit and at byte 127 of a 128-B line for a tiled length: the edge bytes in front
    of the tiles, sentinels in front and behind"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(8)
    sub_len = 3 * (2 * T + 5) + 1
    M = sub_len // 3
    n_len = sub_len + 999
    words = random_words(oracle, rng, n_len)
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    buf = torch.empty(M + 512, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 128 == 0
    for rev in (False, True):
        for start in (0, 17, n_len - sub_len):
            want = np_translate(words, n_len, start, sub_len, rev)
            for ph in list(range(16)) + [127]:
                buf.fill_(SENTINEL)
                got = po.translate_dev(dwords, n_len, start, sub_len, revcomp=rev, out=buf[128 + ph : 128 + ph + M + 3])
                assert got.data_ptr() == buf.data_ptr() + 128 + ph and got.numel() == M
                b = _bytes(buf)
                assert np.array_equal(b[128 + ph : 128 + ph + M], want), (rev, start, ph)
                assert (b[: 128 + ph] == SENTINEL).all() and (b[128 + ph + M :] == SENTINEL).all(), (rev, start, ph)


@gpu
def test_gpu_one_tile_of_bytes_off_the_output_boundary(oracle):
    """M in {T, T + 1, T + head - 1} at every output byte phase 1..15, head = 16 - phase: a tile's worth of bytes with no whole tile
    behind the first 16-B boundary.  The plan gives the whole call to the edge kernel (one launch, counted in a captured graph at
    three phases); M = T + head and T + head + 1 are the first lengths with a tile.  Both strands, sentinels in front and behind"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(17)
    n_len = 3 * (T + 17) + 2 + 45
    words = random_words(oracle, rng, n_len)
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    table = random_table(rng)
    buf = torch.empty(T + 17 + 256, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 128 == 0
    for rev in (False, True):
        for ph in range(1, 16):
            head = 16 - ph
            for M in (T, T + 1, T + head - 1, T + head, T + head + 1):
                sub_len, start = 3 * M + (ph + M) % 3, 1 + 2 * ph
                tab = None if ph % 2 else table
                want = np_translate(words, n_len, start, sub_len, rev, tab)
                buf.fill_(SENTINEL)
                dst = buf[128 + ph : 128 + ph + M]
                got = po.translate_dev(dwords, n_len, start, sub_len, revcomp=rev, table=tab, out=dst)
                assert got.data_ptr() == buf.data_ptr() + 128 + ph and got.numel() == M
                b = _bytes(buf)
                assert np.array_equal(b[128 + ph : 128 + ph + M], want), (rev, ph, M)
                assert (b[: 128 + ph] == SENTINEL).all() and (b[128 + ph + M :] == SENTINEL).all(), (rev, ph, M)
                assert translate_split(sub_len, ph) == ((0, 0) if M < T + head else (head, 1))
                if ph in (1, 5, 15):
                    nodes = _kernel_nodes_of(torch, lambda: po.translate_dev(dwords, n_len, start, sub_len, revcomp=rev, table=tab, out=dst))
                    assert nodes == translate_plan(sub_len, ph) == (1 if M < T + head else 2 if M == T + head else 3), (rev, ph, M)


@gpu
def test_gpu_custom_tables_and_a_table_freed_after_the_call(oracle, L):
    """the identity table returns the codon values, a random table with 0x00 and 0xFF among its bytes is looked up as it is,
    and the host table may be overwritten and freed as soon as cnt_translate_dev has returned, before the stream has run"""
    import torch

    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(44)
    n_len = 3 * (3 * T + 100) + 2
    words = random_words(oracle, rng, n_len)
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    table = random_table(rng)
    assert 0x00 in table and 0xFF in table
    kmers = np_kmers(words, n_len, 3)
    for rev in (False, True):
        for start, sub_len in ((0, n_len), (5, n_len - 5), (32, 3 * T), (7, 50)):
            for tab in (IDENTITY, table, bytes(table), bytearray(table)):
                want = np_translate(words, n_len, start, sub_len, rev, tab)
                assert np.array_equal(_bytes(po.translate_dev(dwords, n_len, start, sub_len, revcomp=rev, table=tab)), want), (rev, start, sub_len)
                assert np.array_equal(po.translate_hip(words[: words_for(n_len)], n_len, start, sub_len, revcomp=rev, table=tab), want), (rev, start, sub_len)
            if not rev:
                got = _bytes(po.translate_dev(dwords, n_len, start, sub_len, table=IDENTITY))
                assert np.array_equal(got, kmers[start : start + sub_len - 2 : 3].astype(np.uint8)[: sub_len // 3])
    # the ABI itself: a table in memory of its own, overwritten and released right after the enqueue
    M = n_len // 3
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rev in (False, True):
        want = np_translate(words, n_len, 0, n_len, rev, table)
        out = torch.full((M,), SENTINEL, dtype=torch.uint8, device="cuda")
        held = (ctypes.c_uint8 * 64)(*table.tolist())
        rc = L.cnt_translate_dev(dwords.data_ptr(), n_len, 0, n_len, CNT_TRANSLATE_REVCOMP if rev else 0, held, out.data_ptr(), M, stream)
        ctypes.memset(held, 0x11, 64)
        del held
        assert rc == _lib.CNT_OK
        torch.cuda.synchronize()
        assert np.array_equal(_bytes(out), want), rev


@gpu
def test_gpu_tiles_across_launch_edges(oracle, launch_tiles):
    """the lab build cut into launches of 64 / 128 tiles: a region of 2 launches + 1 tile plus a remainder, both strands, at an
    aligned and at an odd output address, with the launches counted in a captured graph and held to the plan"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(launch_tiles)
    M = (2 * launch_tiles + 1) * T + 1000
    sub_len = 3 * M + 1
    n_len = sub_len + 77
    words = random_words(oracle, rng, n_len)
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    out = torch.empty(M + 64, dtype=torch.uint8, device="cuda")
    for rev in (False, True):
        for start, ph in ((0, 0), (46, 0), (77, 5)):
            dst = out[ph : ph + M]
            got = po.translate_dev(dwords, n_len, start, sub_len, revcomp=rev, out=dst)
            assert np.array_equal(_bytes(got), np_translate(words, n_len, start, sub_len, rev)), (rev, start, ph)
            want = translate_plan(sub_len, ph, launch_tiles)
            assert want == 3 + 1 + (1 if ph else 0)
            assert _kernel_nodes_of(torch, lambda: po.translate_dev(dwords, n_len, start, sub_len, revcomp=rev, out=dst)) == want
    hgot = po.translate_hip(words[: words_for(n_len)], n_len, 46, sub_len, revcomp=True)
    assert np.array_equal(hgot, np_translate(words, n_len, 46, sub_len, True))


@gpu
def test_gpu_translate_in_a_captured_graph_on_a_side_stream(oracle):
    """translate_dev, forward and reversed, captured with torch.cuda.graph on a side stream and replayed twice on changed
    input words"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(4)
    n_len = 3 * (3 * T + 50) + 40
    table = random_table(rng)
    calls = [(5, n_len - 5, False, None), (0, n_len - 1, True, table), (33, 100, True, None)]
    dwords = torch.zeros(words_for(n_len) + 2, dtype=torch.int64, device="cuda")
    outs = [torch.empty(sub_len // 3 + 1, dtype=torch.uint8, device="cuda")[1:] for _, sub_len, _, _ in calls]  # odd addresses
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for (start, sub_len, rev, tab), dst in zip(calls, outs):  # module load outside the capture
            po.translate_dev(dwords, n_len, start, sub_len, revcomp=rev, table=tab, out=dst)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for (start, sub_len, rev, tab), dst in zip(calls, outs):
            po.translate_dev(dwords, n_len, start, sub_len, revcomp=rev, table=tab, out=dst)
    kept = table.copy()
    table[:] = 0  # the captured launches hold their own copy
    for rep in range(2):
        words = random_words(oracle, rng, n_len)
        dwords.copy_(torch.from_numpy(words.view(np.int64)))
        for dst in outs:
            dst.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for (start, sub_len, rev, tab), dst in zip(calls, outs):
            want = np_translate(words, n_len, start, sub_len, rev, None if tab is None else kept)
            assert np.array_equal(_bytes(dst), want), (rep, start, sub_len, rev)


@gpu
def test_gpu_pinned_in_place_equals_staged(oracle, L):
    """cnt_translate with both buffers pinned (used in place, the kernels reading and writing host memory over the link) against
    ordinary ones (staged) and against only one pinned (staged): identical results, at a phase inside the pinned allocations"""
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    rng = np.random.default_rng(10)
    n_len = 3 * (2 * T + 300) + 77
    words = random_words(oracle, rng, n_len)
    src = words[: words_for(n_len)]
    table = random_table(rng)
    held = (ctypes.c_uint8 * 64)(*table.tolist())
    for start, sub_len in ((17, n_len - 17), (40, 200)):
        M = sub_len // 3
        for rev in (False, True):
            want = np_translate(words, n_len, start, sub_len, rev, table)
            for pin_in, pin_out in ((False, False), (True, True), (True, False), (False, True)):
                bits = cn.pinned_empty(src.size + 3, U64)[3:] if pin_in else src.copy()
                bits[:] = src
                out = cn.pinned_empty(M + 16, np.uint8)[5:] if pin_out else np.empty(M + 11, dtype=np.uint8)
                out[:] = SENTINEL
                if pin_in and pin_out:
                    assert all(L.cnt_host_is_pinned(a.ctypes.data, a.nbytes) == 1 for a in (bits, out))
                rc = L.cnt_translate(bits.ctypes.data, n_len, start, sub_len, CNT_TRANSLATE_REVCOMP if rev else 0, held, out.ctypes.data, M + 11)
                assert rc == _lib.CNT_OK, (start, sub_len, rev, pin_in, pin_out, rc)
                assert np.array_equal(out[:M], want) and (out[M:] == SENTINEL).all(), (start, sub_len, rev, pin_in, pin_out)


@gpu
def test_gpu_search_then_translate_end_to_end(oracle):
    """find_pattern_dev on both strands over planted copies of an ATG... motif and of its reverse complement, then every hit
    translated from its position: the first amino acid is M on forward hits read forward and on reverse hits read with
    revcomp=True, and the whole motif translates to the same peptide"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(78)
    motif = "ATGGCCATTGTAATGGGCCGCTGA"  # M A I V M G R *
    k, n_len = len(motif), 150000 + 11
    codes = [NT.index(ch) for ch in motif]
    rc_codes = [c ^ 2 for c in reversed(codes)]
    s = rng.integers(0, 4, n_len).astype(np.uint8)
    sites = [int(v) * 60 + 30 for v in rng.permutation(n_len // 60 - 1)[:30]] + [0, n_len - k]
    for j, site in enumerate(sites):
        s[site : site + k] = rc_codes if j & 1 else codes
    words = words_of_codes(oracle, s, extra=1, rng=rng)
    dwords = torch.from_numpy(words.view(np.int64)).cuda()
    pos, info, count = po.find_pattern_dev(dwords, n_len, motif, 0, both_strands=True)
    n = int(count.item())
    p, inf = pos[:n].cpu().numpy().view(U64), info[:n].cpu().numpy().view(U64)
    assert n >= len(sites) and set(sites) <= {int(v) for v in p}
    reverse = (inf & U64(0x100)) != 0
    assert reverse.sum() >= len(sites) // 2 and (~reverse).sum() >= len(sites) // 2
    for at, rev in zip(p, reverse):
        got = bytes(_bytes(po.translate_dev(dwords, n_len, int(at), k, revcomp=bool(rev))))
        assert got[:1] == b"M" and got == b"MAIVMGR*", (int(at), bool(rev), got)
        assert bytes(po.translate_hip(words[: words_for(n_len)], n_len, int(at), k, revcomp=bool(rev))) == b"MAIVMGR*"


@gpu
@pytest.mark.parametrize("seed", range(4))
def test_gpu_translate_fuzz(oracle, seed):
    """random lengths, starts, region lengths, strands, tables, input word phases and output byte phases; both tiers"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(9200 + seed)
    for it in range(30):
        n_len = int(rng.choice([rng.integers(0, 300), rng.integers(0, 9 * T), rng.integers(0, 1 << 20)]))
        start = int(rng.integers(0, n_len + 1))
        sub_len = int(rng.choice([rng.integers(0, min(n_len - start, 70) + 1), rng.integers(0, n_len - start + 1), n_len - start]))
        rev, pi, po_ = bool(rng.integers(0, 2)), int(rng.integers(0, 4)), int(rng.integers(0, 130))
        tab = [None, IDENTITY, random_table(rng)][int(rng.integers(0, 3))]
        allw = np.concatenate([rng.integers(0, 2**64, pi, dtype=U64), random_words(oracle, rng, n_len)])
        nw = max(words_for(n_len), 1)
        M = sub_len // 3
        want = np_translate(allw[pi:], n_len, start, sub_len, rev, tab)
        tag = (seed, it, n_len, start, sub_len, rev, pi, po_)
        dall = torch.from_numpy(allw.view(np.int64)).cuda()
        buf = torch.full((M + po_ + 40,), SENTINEL, dtype=torch.uint8, device="cuda")
        got = po.translate_dev(dall[pi : pi + nw], n_len, start, sub_len, revcomp=rev, table=tab, out=buf[po_ : po_ + M + 7])
        b = _bytes(buf)
        assert got.numel() == M and np.array_equal(b[po_ : po_ + M], want), tag
        assert (b[:po_] == SENTINEL).all() and (b[po_ + M :] == SENTINEL).all(), tag
        assert np.array_equal(po.translate_hip(np.ascontiguousarray(allw[pi : pi + nw]), n_len, start, sub_len, revcomp=rev, table=tab), want), tag


@gpu
def test_gpu_translate_full_size_past_2p32(oracle, fullsize):
    """random packed words for 2^32 + 2^16 nt (1 GiB): regions of two tiles and a remainder that start past 2^32, straddle it and
    end at len, forward and reversed, against the reference computed from only the input words they touch"""
    import torch

    from conftest import need_free_hbm
    from cute_nucleotides_amd import packed_ops as po

    n_len = (1 << 32) + (1 << 16)
    need_free_hbm(3)
    torch.manual_seed(33)
    bits = torch.randint(-(1 << 63), (1 << 63) - 1, (words_for(n_len),), dtype=torch.int64, device="cuda")
    sub_len = 2 * T * 3 + 1000
    table = random_table(np.random.default_rng(2))
    t0 = time.perf_counter()
    for start in ((1 << 32) + 12345, (1 << 32) - 5, n_len - sub_len):
        w0 = start >> 5
        piece = bits[w0 : w0 + words_for(sub_len) + 2].cpu().numpy().view(U64)
        for rev in (False, True):
            for tab in (None, table):
                got = _bytes(po.translate_dev(bits, n_len, start, sub_len, revcomp=rev, table=tab))
                assert np.array_equal(got, np_translate(piece, n_len, start, sub_len, rev, tab, first_word=w0)), (start, rev)
    fullsize(32, (time.perf_counter() - t0) * 1e3, check="translate with start > 2^32: kernels and sliced references")
