"""Packed words and quality bytes to four-line FASTQ text (include/cute_nt.h "text formats: FASTQ write",
hip/fastq_write_kernels.hpp, hip/fastq_write_abi.inc).  Not in the reference, which stops at bits_to_n_*: the definition is
restated here twice -- a byte-by-byte writer and a numpy closed form -- the two are pinned against each other, and the text is
read back through tests/test_fastq.py's def_fastq: cnt_fastq_to_bits(cnt_bits_to_fastq(x)) == x on well-formed input.

CPU part: the references, the round trip and the bound, malformed tables, every argument rule of both tiers and both queries in
the order the header states them (all of them precede device work), an aliasing sweep of every (written, other) pair, the Python
layer without a device, the header's comment.  GPU part: both tiers byte for byte against the numpy reference, with canaries
around the text's footprint, rec_text and counts, and every source buffer at the end of its allocation."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from test_aliasing import OVERLAPS, TOUCHES, Arena, Buf, Call, pairs, place, shared_bytes
from test_fasta import np_words, words_for
from test_fastq import def_fastq
from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16384  # bytes of text per workgroup tile of the write pass (hip/fasta_write_kernels.hpp kFastaOutTile)
ROW, WAVE = 1024, 4096  # bytes one store instruction of a wave writes, and bytes per wave of a tile
BLOCK = 256  # pieces per workgroup of the size pass
ROUND = 1024 * BLOCK  # pieces one round of fasta_out_scan takes
NL, AT, PLUS = 0x0A, 0x40, 0x2B
ACTG = np.frombuffer(b"ACTG", dtype=np.uint8)  # the decoder's table
QUALS = np.arange(33, 127, dtype=np.uint8)  # '!' .. '~': neither a line feed nor a carriage return
KINDS = ("@", "name", "name line feed", "letters", "\\n+\\n", "qualities", "last line feed")


# ---- the two references ---------------------------------------------------------------------------------------------------------
def malformed_count(length, rec_start, name_off, names_len):
    if not len(rec_start):
        return 0
    s = [int(x) for x in rec_start] + [length]
    bad = sum(1 for r in range(len(rec_start)) if s[r] > s[r + 1]) + (1 if s[0] != 0 else 0)
    if name_off is not None:
        o = [int(x) for x in name_off]
        bad += sum(1 for r in range(len(rec_start)) if o[r] > o[r + 1]) + (1 if o[-1] > names_len else 0)
    return bad


def def_write(letters, qual, rec_start, names, name_off):
    """the definition, byte by byte: (text, rec_text, malformed).  letters: the decoded sequence as bytes; qual: as many bytes;
    names: the name bytes or None; name_off: R + 1 offsets or None"""
    bad = malformed_count(len(letters), rec_start, name_off, len(names) if names is not None else 0)
    if bad:
        return b"", [], bad
    s = [int(x) for x in rec_start] + [len(letters)]
    text, rec_text = bytearray(), []
    for r in range(len(rec_start)):
        rec_text.append(len(text))
        text.append(AT)
        if name_off is not None:
            for k in range(int(name_off[r]), int(name_off[r + 1])):
                text.append(names[k])
        text.append(NL)
        for i in range(s[r], s[r + 1]):
            text.append(letters[i])
        text += b"\n+\n"
        for i in range(s[r], s[r + 1]):
            text.append(qual[i])
        text.append(NL)
    return bytes(text), rec_text, 0


def _spans(starts, lens):
    """the indices starts[r] .. starts[r] + lens[r] of every r, back to back"""
    ends = np.cumsum(lens)
    return np.repeat(starts - (ends - lens), lens) + np.arange(int(ends[-1]) if lens.size else 0, dtype=np.int64)


def np_write(letters, qual, rec_start, names, name_off):
    """the closed form: record r begins at the sum of the sizes in front of it, and every segment of it lies at a fixed offset from
    there.  (text as uint8, rec_text as uint64, malformed)"""
    letters = np.frombuffer(bytes(letters), dtype=np.uint8) if not isinstance(letters, np.ndarray) else letters
    qual = np.frombuffer(bytes(qual), dtype=np.uint8) if not isinstance(qual, np.ndarray) else qual
    bad = malformed_count(letters.size, rec_start, name_off, len(names) if names is not None else 0)
    if bad or not len(rec_start):
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint64), bad
    s = np.r_[np.asarray(rec_start, dtype=np.int64), letters.size]
    l = np.diff(s)
    o = np.asarray(name_off, dtype=np.int64) if name_off is not None else np.zeros(s.size, dtype=np.int64)
    nl = np.diff(o)
    size = nl + 2 * l + 6
    at = np.cumsum(size) - size
    text = np.full(int(size.sum()), NL, dtype=np.uint8)
    text[at] = AT
    if name_off is not None and nl.sum():
        text[_spans(at + 1, nl)] = np.frombuffer(bytes(names), dtype=np.uint8)[_spans(o[:-1], nl)]
    if letters.size:
        text[_spans(at + 2 + nl, l)] = letters[_spans(s[:-1], l)]
        text[_spans(at + 5 + nl + l, l)] = qual[_spans(s[:-1], l)]
    text[at + 3 + nl + l] = PLUS
    return text, at.astype(np.uint64), 0


def bound(length, n_rec, names_len):
    return 2 * length + names_len + 6 * n_rec


def random_letters(rng, n):
    return ACTG[rng.integers(0, 4, n)].tobytes()


def make_case(rng, lens, name_lens=None, name_alphabet=b"abc 1@+|", slack=(0, 0)):
    """(letters, qual, rec_start, names, name_off) of records with these base counts; slack: unused name bytes in front of the
    first name and behind the last"""
    lens = [int(x) for x in lens]
    starts = (np.cumsum([0] + lens[:-1])).tolist() if len(lens) else []
    n = sum(lens)
    letters, qual = random_letters(rng, n), QUALS[rng.integers(0, QUALS.size, n)].tobytes()
    if name_lens is None:
        return letters, qual, starts, None, None
    alphabet = np.frombuffer(name_alphabet, dtype=np.uint8)
    names = alphabet[rng.integers(0, alphabet.size, slack[0] + sum(name_lens) + slack[1])].tobytes()
    return letters, qual, starts, names, (slack[0] + np.cumsum([0] + [int(x) for x in name_lens])).tolist()


def random_case(rng, most=120, name_alphabet=b"abc 1@+|"):
    n_rec = int(rng.choice([1, 1, 2, 3, 9]))
    lens = [int(rng.choice([0, 1, 15, 16, 17, int(rng.integers(0, most))])) for _ in range(n_rec)]
    name_lens = [int(rng.choice([0, 1, int(rng.integers(0, 45))])) for _ in range(n_rec)] if rng.random() < 0.7 else None
    slack = (int(rng.integers(0, 4)), int(rng.integers(0, 4))) if rng.random() < 0.3 else (0, 0)
    return make_case(rng, lens, name_lens, name_alphabet, slack)


def test_two_references_agree():
    rng = np.random.default_rng(171)
    cases = [random_case(rng) for _ in range(1200)]
    cases += [make_case(rng, [0], [0]), make_case(rng, [0, 0, 0], None), make_case(rng, [0, 5, 0], [3, 0, 2]), make_case(rng, [], None)]
    seen = set()
    for case in cases:
        d, v = def_write(*case), np_write(*case)
        assert d[0] == v[0].tobytes() and d[1] == v[1].tolist() and d[2] == v[2] == 0, case
        seen.add((case[3] is None, len(case[0]) == 0))
    assert seen >= {(True, False), (False, False), (False, True)}
    assert def_write(b"ACGT", b"IIII", [0, 4], None, None) == (b"@\nACGT\n+\nIIII\n@\n\n+\n\n", [0, 14], 0)  # 0 + 2 * 4 + 6
    assert def_write(b"", b"", [0], b"", [0, 0]) == (b"@\n\n+\n\n", [0], 0)
    assert def_write(b"ACGTA", b"#5F!~", [0, 2], b"xr1 ab", [1, 3, 6]) == (b"@r1\nAC\n+\n#5\n@ ab\nGTA\n+\nF!~\n", [0, 12], 0)
    assert def_write(b"ACGT", b"IIII", [], None, None) == (b"", [], 0)  # no record, no text, whatever len is


def test_round_trip_through_the_fastq_definition_and_the_bound():
    """cnt_fastq_to_bits's definition reads the text back: the sequence bytes are the letters, the quality bytes the qualities,
    rec_text is the writer's, rec_start and rec_qual the input -- when no name and no quality holds a line feed or a carriage
    return (names may hold '\\r' in front of their end, '@' and '+': a role is a line number, not a first byte)"""
    rng = np.random.default_rng(172)
    exact = slack = 0
    for _ in range(3000):
        case = random_case(rng, most=200, name_alphabet=b"ab 1@+\r|")
        letters, qual, rec_start, names, name_off = case
        text, rec_text, bad = def_write(*case)
        back = def_fastq(text)
        assert bad == 0 and back.seq == letters and back.qual == qual and back.rec_text == rec_text, case
        assert back.rec_start == back.rec_qual == list(rec_start) and back.malformed == 0, case
        names_len = len(names) if names is not None else 0
        used = name_off[-1] - name_off[0] if name_off is not None else 0
        b = bound(len(letters), len(rec_start), names_len)
        assert len(text) == 2 * len(letters) + 6 * len(rec_start) + used <= b and (len(text) == b) == (used == names_len)
        exact += used == names_len
        slack += used < names_len
    assert exact > 1000 and slack > 100


MALFORMED = (  # (length, rec_start, names_len, name_off, the count)
    (10, [0, 5, 3], 0, None, 1),  # a descent
    (10, [0, 5, 4, 9, 8], 0, None, 2),
    (10, [0, 11], 0, None, 1),  # rec_start[r] > len: s_r > s_R
    (10, [0, 11, 12], 0, None, 1),
    (10, [0, 5], 8, [0, 5, 4], 1),  # a descent of the names
    (10, [0, 5], 8, [0, 5, 9], 1),  # o_R > names_len
    (10, [0, 5], 8, [9, 9, 9], 1),
    (10, [0, 5], 8, [10, 9, 12], 2),
    (10, [3], 0, None, 1),  # s_0 != 0: bases that belong to no record
    (10, [1, 5], 8, [0, 2, 4], 1),
    (10, [5, 3], 8, [3, 2, 9], 4),  # everything at once: s_0 != 0, a descent of each table, o_R > names_len
    (0, [1], 0, [0, 0], 2),  # s_0 != 0 and s_0 > len
)


def test_malformed_tables_in_the_references():
    for length, rec_start, names_len, name_off, count in MALFORMED:
        letters, names = (b"ACGT" * 3)[:length], (b"n" * names_len if name_off is not None else None)
        d = def_write(letters, b"I" * length, rec_start, names, name_off)
        v = np_write(letters, b"I" * length, rec_start, names, name_off)
        assert d == (b"", [], count) and v[0].size == 0 and v[1].size == 0 and v[2] == count, (length, rec_start, name_off)


# ---- CPU: the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


FILL = 0x5A
U64P = ctypes.POINTER(ctypes.c_uint64)


def test_argument_checks_in_the_stated_order(L):
    """every check of the header's list, each with all EARLIER checks passing and, where it can, a LATER one failing too -- the
    later one must not be reached; the fill around every buffer: a refused call writes nothing"""
    from cute_nucleotides_amd import _lib

    OK, EINVAL = _lib.CNT_OK, _lib.CNT_EINVAL
    vp = ctypes.c_void_p
    arena = np.full(1 << 16, FILL, dtype=np.uint8)
    base = arena.ctypes.data + (-arena.ctypes.data % 128)
    at = lambda k: vp(base + 4096 * k)  # noqa: E731 -- buffer k of a call, each in a 4-KiB slot of its own
    n_len, R, NAMES = 1000, 10, 40
    need, got = ctypes.c_size_t(0), ctypes.c_size_t(0)
    # 1. the queries: a NULL bytes
    assert L.cnt_bits_to_fastq_work_bytes(R, None) == EINVAL and L.cnt_bits_to_fastq_bound(n_len, R, NAMES, None) == EINVAL
    sizes = []
    for r in (0, 1, BLOCK - 2, BLOCK - 1, BLOCK, ROUND, 1 << 30):
        assert L.cnt_bits_to_fastq_work_bytes(r, ctypes.byref(need)) == OK
        sizes.append(need.value)
    assert sizes == sorted(sizes) and 0 < sizes[0] <= 64 and sizes[-1] < 9 * (1 << 30)  # it depends on n_rec only: 8 bytes and a little a record
    assert L.cnt_bits_to_fastq_work_bytes(1 << 62, ctypes.byref(need)) == EINVAL and L.cnt_bits_to_fastq_work_bytes((1 << 48) + 1, ctypes.byref(need)) == EINVAL
    for length, r, names_len in ((0, 0, 0), (1000, 10, 40), (1, 0, 0), (0, 1, 0), (1 << 36, 1 << 20, 1 << 25)):
        assert L.cnt_bits_to_fastq_bound(length, r, names_len, ctypes.byref(got)) == OK and got.value == bound(length, r, names_len)
    big = (1 << 64) - 1
    for args in ((big, 0, 0), (1 << 63, 0, 0), (0, big, 0), (0, 1 << 62, 0), (1, 0, big), ((1 << 63) - 1, 0, 2), (1 << 62, 1 << 61, 0), (0, (1 << 61) + (1 << 60), 1 << 63)):
        got.value = 77
        assert L.cnt_bits_to_fastq_bound(*args, ctypes.byref(got)) == EINVAL and got.value == 77, args
    assert L.cnt_bits_to_fastq_work_bytes(R, ctypes.byref(need)) == OK
    need = need.value

    # slots: 0 bits, 1 rec_start, 2 names, 3 name_off, 4 text, 5 qual, 6 rec_text, 7 counts, 8 work
    def dev(bits=at(0), n=n_len, qual=at(5), rs=at(1), r=R, names=at(2), names_len=NAMES, no=at(3), flags=0, text=at(4), cap=3000, rt=at(6), counts=at(7), work=at(8),
            work_bytes=need):
        return L.cnt_bits_to_fastq_dev(bits, n, qual, rs, r, names, names_len, no, flags, text, cap, rt, counts, work, work_bytes, None)

    def host(bits=at(0), n=n_len, qual=at(5), rs=at(1), r=R, names=at(2), names_len=NAMES, no=at(3), flags=0, text=at(4), cap=3000, rt=at(6), counts=at(7)):
        return L.cnt_bits_to_fastq(bits, n, qual, rs, r, names, names_len, no, flags, text, cap, rt, ctypes.cast(counts, U64P))

    def untouched():
        return bool((arena == FILL).all())

    off = lambda k, d: vp(at(k).value + d)  # noqa: E731
    for call in (dev, host):
        # 1. an unknown flag, before everything: on empty work, with NULL pointers
        for flags in (1, 2, 4, 0x80000000):
            assert call(flags=flags) == EINVAL and call(flags=flags, r=0) == EINVAL and call(flags=flags, bits=None, text=None, counts=None) == EINVAL
        # 2. no record, whatever len is: CNT_OK whatever the pointers are (a host count is zeroed, a device one needs a device)
        assert call(r=0, bits=None, qual=None, rs=None, text=None, rt=off(6, 4), counts=None, names=None) == OK and untouched()
        assert call(n=0, r=0, counts=None, no=None, names_len=big) == OK and untouched()
        # 3. the NULLs -- in front of 4 (a misaligned rec_text), 5 and 7
        for null in ({"bits": None}, {"qual": None}, {"text": None}, {"counts": None}, {"rs": None}):
            assert call(**null) == EINVAL and call(**null, rt=off(6, 4)) == EINVAL and call(**null, names=None) == EINVAL and call(**null, names_len=big) == EINVAL
        # 4. alignment of bits, rec_start, name_off, rec_text and counts; text, qual and names may sit anywhere -- in front of 5, 6 and 7
        for name, slot in (("bits", 0), ("rs", 1), ("no", 3), ("rt", 6), ("counts", 7)):
            for d in (1, 4, 7):
                assert call(**{name: off(slot, d)}) == EINVAL
        assert call(rt=off(6, 4), names=None) == EINVAL and call(bits=off(0, 4), text=at(0)) == EINVAL and call(rs=off(1, 4), n=1 << 63) == EINVAL
        # 5. names without name_off, and the reverse -- in front of 6 and 7
        assert call(names=None) == EINVAL and call(no=None) == EINVAL and call(names=None, text=at(0)) == EINVAL and call(no=None, names_len=big) == EINVAL
        # 6. the bound overflowing size_t, n_rec above 2^48 -- in front of 7
        assert call(names_len=big) == EINVAL and call(names_len=big, text=at(0)) == EINVAL and call(r=1 << 62, text=at(0)) == EINVAL
        assert call(r=(1 << 48) + 1, text=at(0)) == EINVAL
        # 7. overlaps, at the stated extents: the footprint of text (here the bound, 2100 bytes), R entries, 16 bytes of counts, len quality bytes
        assert bound(n_len, R, NAMES) == 2100
        assert call(text=at(0)) == EINVAL and call(text=off(1, 8 * R - 1)) == EINVAL and call(text=off(2, NAMES - 1)) == EINVAL and call(text=off(3, 8 * R + 7)) == EINVAL
        assert call(text=off(5, n_len - 1)) == EINVAL and call(text=off(5, -2099)) == EINVAL and call(rt=off(5, 992)) == EINVAL and call(counts=off(5, -8)) == EINVAL
        assert call(rt=off(4, 2096)) == EINVAL and call(text=off(6, -2099)) == EINVAL and call(counts=off(4, 2096)) == EINVAL
        assert call(rt=at(1)) == EINVAL and call(rt=off(3, 8 * R)) == EINVAL and call(counts=off(6, 8 * R - 8)) == EINVAL and call(counts=off(0, 256 - 8)) == EINVAL
        assert call(counts=off(1, -8)) == EINVAL  # the second count lies in rec_start
        assert call(text=off(4, 0), cap=100, counts=off(4, 96)) == EINVAL  # the footprint is min(bound, text_cap)
        assert untouched()
    # 8. the device tier's scratch, after everything else
    assert dev(work=None) == EINVAL and dev(work_bytes=need - 1) == EINVAL and dev(work_bytes=0) == EINVAL
    for other in (0, 1, 2, 3, 4, 5, 6, 7):
        assert dev(work=vp(at(other).value - need + 8)) == EINVAL  # the last 8 bytes of the query's answer reach into the buffer
    assert dev(work=None, text=at(0)) == EINVAL and untouched()
    # the host tier sets its counts on empty work, and only them
    c = np.full(4, 7, dtype=np.uint64)
    assert L.cnt_bits_to_fastq(None, 5, None, None, 0, None, 0, None, 0, None, 0, None, ctypes.cast(vp(c.ctypes.data + 8), U64P)) == OK
    assert c.tolist() == [7, 0, 0, 7]
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        ENODEV = _lib.CNT_ENODEV
        assert host() == ENODEV and host(names=None, no=None) == ENODEV and host(rt=None) == ENODEV
        assert host(text=at(0), cap=0) == ENODEV  # capacity 0: text may sit anywhere, but not at NULL
        assert host(text=off(4, 3), names=off(2, 5), qual=off(5, 3), counts=off(4, 3 + 2100 + 1)) == ENODEV  # text, names and qual at any byte; buffers that touch
        assert host(bits=None, qual=None, n=0, text=at(0)) == ENODEV
        assert dev(work=off(8, 4), work_bytes=need) < 0  # a scratch at any address
        assert untouched()


def fastq_write_calls(L):
    """the two tiers as test_aliasing's table rows: every buffer with its extent, its alignment and whether it is written"""
    vp = ctypes.c_void_p
    up = lambda a: ctypes.cast(vp(a), U64P)  # noqa: E731
    n_len, R, names_len, cap = 800, 24, 96, 1832  # every extent a multiple of 8, so that an 8-B aligned buffer can touch its end
    assert bound(n_len, R, names_len) == 1840
    need = ctypes.c_size_t(0)
    assert L.cnt_bits_to_fastq_work_bytes(R, ctypes.byref(need)) == 0 and need.value % 8 == 0
    need = need.value
    bufs = [Buf("bits", words_for(n_len) * 8, 8, False), Buf("qual", n_len, 1, False), Buf("rec_start", R * 8, 8, False), Buf("names", names_len, 1, False),
            Buf("name_off", (R + 1) * 8, 8, False), Buf("text", cap, 1, True), Buf("rec_text", R * 8, 8, True), Buf("counts", 16, 8, True)]
    dev = Call("cnt_bits_to_fastq_dev", bufs + [Buf("work", need, 8, True)],
               lambda p: L.cnt_bits_to_fastq_dev(vp(p["bits"]), n_len, vp(p["qual"]), vp(p["rec_start"]), R, vp(p["names"]), names_len, vp(p["name_off"]), 0, vp(p["text"]),
                                                 cap, vp(p["rec_text"]), vp(p["counts"]), vp(p["work"]), need + 64, None), frozenset())
    host = Call("cnt_bits_to_fastq", bufs,
                lambda p: L.cnt_bits_to_fastq(vp(p["bits"]), n_len, vp(p["qual"]), vp(p["rec_start"]), R, vp(p["names"]), names_len, vp(p["name_off"]), 0, vp(p["text"]), cap,
                                              vp(p["rec_text"]), up(p["counts"])), frozenset())
    return [dev, host]


def test_aliasing_sweep_of_every_written_buffer(L):
    """every (written, other) pair of both tiers: the five overlapping placements are CNT_EINVAL and write nothing, the two
    touching ones pass the argument checks"""
    from cute_nucleotides_amd import _lib

    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    arena = Arena(slots=9)
    tried = 0
    for call in fastq_write_calls(L):
        assert len(pairs(call)) == (4 * 8 if call.name.endswith("_dev") else 3 * 7)
        for w, o in pairs(call):
            for topology in OVERLAPS + TOUCHES:
                p = arena.homes(call)
                p[w.name] = place(topology, w, o, p[o.name])
                if p[w.name] is None:
                    continue
                shared = shared_bytes(p, w, o)
                if topology in OVERLAPS:
                    assert shared > 0 and call.fn(p) == _lib.CNT_EINVAL, (call.name, w.name, o.name, topology)
                    tried += 1
                elif count.value == 0:  # with a device the call would run on host memory
                    rc = call.fn(p)
                    assert shared == 0 and (rc == _lib.CNT_ENODEV or rc < 0), (call.name, w.name, o.name, topology, rc)
                assert arena.unchanged(), (call.name, w.name, o.name, topology)
    assert tried >= (4 * 8 + 3 * 7) * 3  # the first three placements exist for every pair


def test_abi_wiring(L):
    import subprocess

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib, packed_ops as po

    names = ("cnt_bits_to_fastq", "cnt_bits_to_fastq_dev", "cnt_bits_to_fastq_work_bytes", "cnt_bits_to_fastq_bound")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    hpp = open(os.path.join(ROOT, "cute_nucleotides_amd", "cute_nucleotides.hpp")).read()
    for name in names:
        assert name in exported and ("int %s(" % name) in header and ("fn %s(" % name) in rust and (name + "(") in hpp and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["cnt_bits_to_fastq_dev"][1]) == 16 and len(_lib.SIGNATURES["cnt_bits_to_fastq"][1]) == 13
    assert "pub fn bits_to_fastq_hip(" in rust and "inline FastaText bits_to_fastq_hip(" in hpp and "pub fn bits_to_fastq_hip_dev(" in rust
    assert "pub fn bits_to_fastq_bound(" in rust and "pub fn bits_to_fastq_work_bytes(" in rust and "inline void bits_to_fastq_hip_dev(" in hpp
    for name in ("bits_to_fastq_hip", "bits_to_fastq_dev", "bits_to_fastq_work_bytes", "bits_to_fastq_bound"):
        assert getattr(cn, name) is getattr(po, name) and name in cn.__all__
    assert "#define CNT_ABI_VERSION 1" in header  # symbols were only added: the version did not move
    shim = open(os.path.join(ROOT, "hip", "cute_nt.hip")).read()
    assert shim.index('#include "fasta_write_abi.inc"') < shim.index('#include "fastq_write_abi.inc"')


def test_header_comment_and_section_place():
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    title = "/* ---- text formats: FASTQ write ----"
    assert header.count(title) == 1
    at = header.index(title)
    assert header.index("/* ---- text formats: FASTA write ----") < header.index("int cnt_bits_to_fasta(") < at < header.index("Kernel selection for A/B runs")
    section = header[at : header.index("Kernel selection for A/B runs")]
    for k, name in enumerate(("CNT_FASTQ_OUT_TEXT", "CNT_FASTQ_OUT_MALFORMED")):
        assert re.search(r"#define %s +%d\b" % (name, k), section) and "counts[%s]" % name in section, name
    checks = ["1. an unknown flag", "2. n_rec == 0, whatever len is", "3. a NULL text, a NULL counts, a NULL rec_start, a NULL bits or a NULL qual with len > 0",
              "4. a bits, rec_start, name_off, rec_text or counts that is not 8-B aligned", "5. names without name_off", "6. the bound overflowing size_t",
              "7. a written buffer sharing a byte", "8. device tier: a NULL d_work"]
    places = [section.index(c) for c in checks]
    assert places == sorted(places)
    for word in ("A MALFORMED TABLE WRITES NO TEXT", "CNT_EINVAL after the work", "CNT_ECAP after the work", "enqueue-only", "capturable in a graph", "2^36",
                 "NOT validated", "(s_0 != 0)", "2 len + names_len + 6 n_rec", "depends on n_rec only", "ONE table serves bases and qualities", "n_rec above 2^48",
                 "wrapped FASTQ lines", "CRLF", "a name behind the '+'", "constant-quality fill", "separate rec_qual tables", "paired", "5-letter", "gzip",
                 "no LDS-staged variant was built", "profiles/fastq_write_bench.jsonl"):
        assert word in section, word
    fasta_write = header[header.index("/* ---- text formats: FASTA write ----") : at]
    assert "Out of scope: FASTQ writing" in fasta_write  # that section's text stays as it was


def test_write_plan_matches_the_launcher_source():
    src = open(os.path.join(ROOT, "hip", "fastq_write_kernels.hpp")).read()
    kernels = [line for line in src.splitlines() if line.startswith("__global__")]
    assert len(kernels) == 2 and all("template" not in k for k in kernels) and not re.search(r"atomic\w*\(|\basm\b", src)
    assert "fasta_out_find(a.off, 0, pieces," in src and "fasta_out_block_scan(a, block, p, size, bad);" in src and '#include "fasta_write_kernels.hpp"' in src
    abi = open(os.path.join(ROOT, "hip", "fastq_write_abi.inc")).read()
    order = ["hipMemsetAsync(d_counts, 0, 16, s)", "hipLaunchKernelGGL(fastq_out_sizes,", "hipLaunchKernelGGL(fasta_out_scan, dim3(1), dim3(kFastaOutScanBlock), 0, s, a);",
             "hipLaunchKernelGGL(fasta_out_offsets,", "hipLaunchKernelGGL(fastq_out_write,"]
    places = [abi.index(o) for o in order]
    assert places == sorted(places)
    assert abi.count("hipLaunchKernelGGL(") == 4 and abi.count("split_launches(") == 3 and abi.count("hipMalloc") == 0
    assert "host_call(b, 16 + work_bytes, got, 2, 0, false," in abi


def write_plan(foot, n_rec, phase=0, launch_tiles=((0x7FFFFFFF // 256) // 64) * 64):
    """(tiles, kernel launches) of a device call: the size pass and the offset pass over blocks of pieces, the scan, the write pass"""
    tiles, blocks = -(-(foot + phase) // T), -(-(n_rec + 1) // BLOCK)
    return tiles, 2 * -(-blocks // launch_tiles) + 1 + -(-tiles // launch_tiles)


# ---- CPU: the Python layer ------------------------------------------------------------------------------------------------------
def letters_of(words, n):
    """the decoder in numpy: the letters of n codes"""
    w = np.asarray(words, dtype=np.uint64)
    codes = (w[:, None] >> (np.uint64(2) * np.arange(32, dtype=np.uint64))) & np.uint64(3)
    return ACTG[codes.reshape(-1)[:n].astype(np.int64)]


def _fake_lib(calls):
    """a stand-in for the library whose cnt_bits_to_fastq is the numpy reference behind the C calling convention"""
    from cute_nucleotides_amd import _lib

    def arr(p, n, ct=ctypes.c_uint64, dt=np.uint64):
        return np.frombuffer((ct * n).from_address(p.value), dtype=dt) if n and p is not None else np.zeros(0, dtype=dt)

    def cnt_bits_to_fastq_bound(length, n_rec, names_len, out):
        out._obj.value = bound(length, n_rec, names_len)
        return 0

    def cnt_bits_to_fastq(bits, length, qual, rec_start, n_rec, names, names_len, name_off, flags, text, text_cap, rec_text, counts):
        calls.append((length, n_rec, names_len, flags, text_cap, names is None, name_off is None, rec_text is None))
        letters = letters_of(arr(bits, words_for(length)), length) if length else np.zeros(0, dtype=np.uint8)
        nm = arr(names, names_len, ctypes.c_uint8, np.uint8).tobytes() if names is not None else None
        got, rt, bad = np_write(letters, arr(qual, length, ctypes.c_uint8, np.uint8), arr(rec_start, n_rec).tolist(), nm,
                                arr(name_off, n_rec + 1).tolist() if name_off is not None else None)
        counts[0], counts[1] = got.size, bad
        if bad:
            return _lib.CNT_EINVAL
        m = min(got.size, text_cap)
        arr(text, m, ctypes.c_uint8, np.uint8)[:] = got[:m]
        if rec_text is not None:
            arr(rec_text, n_rec)[:] = rt
        return _lib.CNT_ECAP if got.size > text_cap else _lib.CNT_OK

    return types.SimpleNamespace(cnt_bits_to_fastq=cnt_bits_to_fastq, cnt_bits_to_fastq_bound=cnt_bits_to_fastq_bound, cnt_words_for=words_for)


def test_bits_to_fastq_hip_builds_the_name_table(monkeypatch):
    from cute_nucleotides_amd import packed_ops as po

    calls = []
    monkeypatch.setattr(po, "lib", lambda: _fake_lib(calls))
    rng = np.random.default_rng(173)
    for k in range(40):
        letters, qual, rec_start, names, name_off = random_case(rng)
        words = np_words(np.frombuffer(letters, dtype=np.uint8), False)
        name_list = [names[name_off[r] : name_off[r + 1]] for r in range(len(rec_start))] if names is not None else None
        del calls[:]
        text = po.bits_to_fastq_hip(words, len(letters), qual if k % 2 else np.frombuffer(qual, dtype=np.uint8), np.asarray(rec_start, dtype=np.uint64), name_list)
        assert isinstance(text, bytes) and text == def_write(letters, qual, rec_start, names, name_off)[0]
        names_len = name_off[-1] - name_off[0] if names is not None else 0  # the table is rebuilt without the slack
        assert calls == [(len(letters), len(rec_start), names_len, 0, bound(len(letters), len(rec_start), names_len), names is None, names is None, True)]
    # the names are what fastq_names returns
    text = po.bits_to_fastq_hip(np_words(np.frombuffer(b"ACGTAC", dtype=np.uint8), False), 6, b"II#5F!", np.array([0, 4], dtype=np.uint64), [b"a b", bytearray(b"")])
    assert text == b"@a b\nACGT\n+\nII#5\n@\nAC\n+\nF!\n" and po.fastq_names(text, [0, 17]) == [b"a b", b""]
    assert po.bits_to_fastq_hip(np.zeros(0, dtype=np.uint64), 0, b"", np.zeros(0, dtype=np.uint64)) == b""
    # a malformed table is an error; so are a name list of another length, qualities of another length and words of another type
    with pytest.raises(Exception):
        po.bits_to_fastq_hip(np.zeros(1, dtype=np.uint64), 10, b"I" * 10, np.array([0, 5, 3], dtype=np.uint64))
    with pytest.raises(Exception):
        po.bits_to_fastq_hip(np.zeros(1, dtype=np.uint64), 10, b"I" * 10, np.array([2], dtype=np.uint64))  # s_0 != 0
    with pytest.raises(ValueError):
        po.bits_to_fastq_hip(np.zeros(1, dtype=np.uint64), 10, b"I" * 10, np.array([0], dtype=np.uint64), [b"a", b"b"])
    with pytest.raises(ValueError):
        po.bits_to_fastq_hip(np.zeros(1, dtype=np.uint64), 10, b"I" * 9, np.array([0], dtype=np.uint64))
    with pytest.raises(ValueError):
        po.bits_to_fastq_hip(np.zeros(1, dtype=np.uint64), 33, b"I" * 33, np.array([0], dtype=np.uint64))
    with pytest.raises(TypeError):
        po.bits_to_fastq_hip(np.zeros(1, dtype=np.int32), 10, b"I" * 10, np.array([0], dtype=np.uint64))
    with pytest.raises(TypeError):
        po.bits_to_fastq_hip(np.zeros(1, dtype=np.uint64), 10, "I" * 10, np.array([0], dtype=np.uint64))


def test_device_wrapper_argument_errors():
    torch = pytest.importorskip("torch")
    from cute_nucleotides_amd import packed_ops as po

    t, q = torch.zeros(10, dtype=torch.int64), torch.zeros(10, dtype=torch.uint8)
    with pytest.raises(ValueError):
        po.bits_to_fastq_dev(t, 10, q, t, q, t, q)  # not on a device


# ---------------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
CANARY = -0x3C3C3C3C3C3C3C3D
BYTE = 0xC3  # the canary's bytes
HOST_CANARY = 0xDEADBEEFDEADBEEF
PAD = 5  # canary words in front of and behind rec_text and counts
GUARD = 64  # canary bytes in front of and behind the text's footprint


def case_words(letters):
    return np_words(np.frombuffer(bytes(letters), dtype=np.uint8), False)


def at_the_end(torch, data, phase, poison=b"\n@+"):
    """a device tensor that ends where `data` ends: the bytes at byte phase `phase` (mod 16) of an allocation with nothing behind
    them and poison in front -- a byte read outside would be a line feed, an '@' or a '+', or lie outside the allocation"""
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    lead = 16 + (phase - data.size) % 16  # the parent is 256-B aligned: the data ends 16-B aligned plus phase
    parent = torch.from_numpy(np.r_[np.resize(np.frombuffer(poison, dtype=np.uint8), lead), data].copy()).cuda()
    view = parent[lead:]
    assert view.numel() == data.size and (data.size == 0 or (view.data_ptr() + data.size) % 16 == phase % 16)
    return view


def check_dev(case, text_cap=None, text_phase=0, qual_phase=0, names_phase=0, with_rec_text=True, dirty_bits=True, tag=()):
    """the device tier on the case: text, rec_text, counts, canaries around every footprint.  Returns (|text|, malformed)"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    letters, qual, rec_start, names, name_off = case
    n, R = len(letters), len(rec_start)
    names_len = len(names) if names is not None else 0
    want, want_rt, bad = np_write(*case)
    b = bound(n, R, names_len)
    cap = b if text_cap is None else text_cap
    foot = min(b, cap)
    words = case_words(letters)
    if dirty_bits and n % 32:  # bits beyond len are ignored
        words[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(2 * (n % 32))
    d_bits = torch.from_numpy(words.view(np.int64)).cuda()  # no word behind the last
    d_qual = at_the_end(torch, qual, qual_phase)
    d_rs = torch.from_numpy(np.asarray(rec_start, dtype=np.uint64).view(np.int64)).cuda()
    d_names = d_no = None
    if names is not None:
        d_names = at_the_end(torch, names, names_phase)
        d_no = torch.from_numpy(np.asarray(name_off, dtype=np.uint64).view(np.int64)).cuda()
    d_parent = torch.full((GUARD + text_phase + foot + GUARD,), BYTE, dtype=torch.uint8, device="cuda")
    d_text = d_parent[GUARD + text_phase : GUARD + text_phase + foot]
    assert foot == 0 or d_text.data_ptr() % 16 == text_phase % 16
    d_rt = torch.full((PAD + R + PAD,), CANARY, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((4,), CANARY, dtype=torch.int64, device="cuda")
    d_work = torch.full((po.bits_to_fastq_work_bytes(R) + 8,), 0x77, dtype=torch.uint8, device="cuda")
    po.bits_to_fastq_dev(d_bits, n, d_qual, d_rs, d_text, d_cnt[1:3], d_work[4:], names=d_names, name_off=d_no,  # the scratch 4 bytes off
                         rec_text=d_rt[PAD : PAD + R] if with_rec_text else None, text_cap=cap)
    torch.cuda.synchronize()
    tag = tag + (n, R, names_len, cap, text_phase, qual_phase, names_phase)
    assert d_cnt.cpu().numpy().tolist() == [CANARY, want.size, bad, CANARY], tag
    h = d_parent.cpu().numpy()
    lo = GUARD + text_phase
    m = min(want.size, cap)
    assert (h[:lo] == BYTE).all() and (h[lo + foot :] == BYTE).all(), tag + ("text canary",)
    got = h[lo : lo + m]
    if not np.array_equal(got, want[:m]):
        k = int(np.flatnonzero(got != want[:m])[0])
        raise AssertionError(tag + ("text", k, got[max(k - 20, 0) : k + 20].tobytes(), want[max(k - 20, 0) : k + 20].tobytes()))
    rt = d_rt.cpu().numpy()
    if bad:
        assert (h == BYTE).all() and (rt == CANARY).all(), tag + ("malformed",)
    elif with_rec_text:
        assert (rt[:PAD] == CANARY).all() and (rt[PAD + R :] == CANARY).all() and np.array_equal(rt[PAD : PAD + R].view(np.uint64), want_rt), tag + ("rec_text",)
    else:
        assert (rt == CANARY).all(), tag + ("rec_text",)
    return want.size, bad


PINNED_SLOTS = {}  # the eight pinned buffers of a host call, kept and grown across calls: hundreds of calls, a handful of allocations


def pinned_slot(cn, slot, k, dtype):
    """k elements at the start of pinned block `slot`, which grows by doubling; the call's extent ends inside the allocation"""
    nbytes = max(k, 1) * np.dtype(dtype).itemsize
    if slot not in PINNED_SLOTS or PINNED_SLOTS[slot].nbytes < nbytes:
        PINNED_SLOTS[slot] = cn.pinned_empty(1 << max(nbytes - 1, 4095).bit_length(), np.uint8)
    return PINNED_SLOTS[slot][:nbytes].view(dtype)[:k]


def check_host(L, case, text_cap=None, with_rec_text=True, pinned=False, tag=()):
    """the host tier on the case, pageable or pinned buffers, text, qual and names at odd bytes inside their allocations"""
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    letters, qual, rec_start, names, name_off = case
    n, R = len(letters), len(rec_start)
    names_len = len(names) if names is not None else 0
    want, want_rt, bad = np_write(*case)
    b = bound(n, R, names_len)
    cap = b if text_cap is None else text_cap
    foot = min(b, cap)
    slot = iter(range(8))
    alloc = (lambda k, dt=np.uint64: pinned_slot(cn, next(slot), k, dt)) if pinned else (lambda k, dt=np.uint64: np.empty(k, dtype=dt))
    bits, rs, no = alloc(words_for(n) + 1), alloc(R + 1), alloc(R + 2)
    bits[: words_for(n)] = case_words(letters)
    rs[:R] = np.asarray(rec_start, dtype=np.uint64)
    nm, ql = alloc(names_len + 8, np.uint8), alloc(n + 8, np.uint8)
    ql[5 : 5 + n] = np.frombuffer(bytes(qual), dtype=np.uint8)
    if names is not None:
        no[: R + 1] = np.asarray(name_off, dtype=np.uint64)
        nm[3 : 3 + names_len] = np.frombuffer(bytes(names), dtype=np.uint8)
    text, rt, cnt = alloc(GUARD + 3 + foot + GUARD, np.uint8), alloc(PAD + R + PAD), alloc(4)
    text[:] = BYTE
    rt[:] = HOST_CANARY
    cnt[:] = HOST_CANARY
    rc = L.cnt_bits_to_fastq(bits.ctypes.data if n else None, n, ql[5:].ctypes.data if n else None, rs.ctypes.data, R, nm[3:].ctypes.data if names is not None else None,
                             names_len, no.ctypes.data if names is not None else None, 0, text[GUARD + 3 :].ctypes.data, cap,
                             rt[PAD:].ctypes.data if with_rec_text else None, cnt[1:].ctypes.data)
    tag = tag + (n, R, names_len, cap, pinned)
    assert rc == (_lib.CNT_EINVAL if bad else _lib.CNT_ECAP if want.size > cap else _lib.CNT_OK), tag + (rc,)
    assert cnt.tolist() == [HOST_CANARY, want.size, bad, HOST_CANARY], tag + (cnt.tolist(),)
    lo, m = GUARD + 3, min(want.size, cap)
    assert (text[:lo] == BYTE).all() and (text[lo + foot :] == BYTE).all() and np.array_equal(text[lo : lo + m], want[:m]), tag + ("text",)
    if bad:
        assert (text == BYTE).all() and (rt == HOST_CANARY).all(), tag + ("malformed",)
    elif with_rec_text:
        assert (rt[:PAD] == HOST_CANARY).all() and (rt[PAD + R :] == HOST_CANARY).all() and np.array_equal(rt[PAD : PAD + R], want_rt), tag + ("rec_text",)
    else:
        assert (rt == HOST_CANARY).all(), tag + ("rec_text",)
    return want.size, bad


SMALL_LENS = (0, 1, 5, 9, 10, 15, 16, 17, 31, 32, 33, 150)
SMALL_NAMES = (0, 1, 13, 40)


@gpu
@pytest.mark.parametrize("n_rec", [1, 2, 3, 9])
def test_gpu_small_shapes(L, n_rec):
    """the smallest shapes at which a chunk holds one, two or three records and a seam falls on every byte of a chunk: record
    lengths and name lengths drawn from the short lists, every record length in the first record once, both tiers"""
    rng = np.random.default_rng(180 + n_rec)
    ran = 0
    for first in SMALL_LENS:
        for first_name in SMALL_NAMES + (None,):
            lens = [first] + [int(x) for x in rng.choice(SMALL_LENS, n_rec - 1)]
            name_lens = None if first_name is None else [first_name] + [int(x) for x in rng.choice(SMALL_NAMES, n_rec - 1)]
            case = make_case(rng, lens, name_lens)
            total = bound(sum(lens), n_rec, sum(name_lens or [0]))
            assert check_dev(case, text_phase=ran % 16, qual_phase=ran % 5, names_phase=ran % 7, with_rec_text=ran % 5 != 0) == (total, 0)
            if ran % 6 == 0:
                check_host(L, case, with_rec_text=ran % 12 != 0)
            ran += 1
    assert ran == 60


@gpu
def test_gpu_pointer_phases():
    """text at every phase 0..15, qual and names at phases {0, 1, 3, 8, 15} of the 16-B grid (so every phase of the 4-B grid their
    loads lie on); a table of about 20 KiB of text.  Then packed words whose first record begins at a base that is no multiple of
    32: the table of a caller that hands in a suffix of its words cannot, so the records in front are what moves the phase"""
    rng = np.random.default_rng(183)
    case = make_case(rng, [70, 0, 4000, 1, 333, 150, 5000], [5, 0, 40, 1, 300, 13, 2], slack=(3, 2))
    total = bound(9554, 7, 361)  # the five bytes of slack in `names` are not text
    assert 19000 < total < 21000
    for tp in range(16):
        assert check_dev(case, text_phase=tp, qual_phase=tp % 5, names_phase=tp % 3) == (total, 0)
    for qp in (0, 1, 3, 8, 15):
        for npz in (0, 1, 3, 8, 15):
            assert check_dev(case, text_phase=(qp + npz) % 16, qual_phase=qp, names_phase=npz) == (total, 0)
    for first in range(1, 33):  # record 1 begins at base `first`, every residue of a word
        check_dev(make_case(rng, [first, 2 * T + 5, 40], [3, 0, 7]), text_phase=first % 16)
        check_dev(make_case(rng, [first, 45, 1, 33], None), text_phase=first % 16, qual_phase=first % 4)


def seam_case(rng, kind, at):
    """two records, the second one's segment `kind` beginning at text byte `at`"""
    name, bases = 40, 150
    inside = (0, 1, 1 + name, 2 + name, 2 + name + bases, 5 + name + bases, 5 + name + 2 * bases)[kind]
    first = at - inside - 6  # record 0: 6 + its name + twice its bases
    assert first >= 40
    name0 = 20 + first % 2
    case = make_case(rng, [(first - name0) // 2, bases], [name0, name])
    assert int(np_write(*case)[1][1]) + inside == at
    return case


@gpu
@pytest.mark.parametrize("edge", [T + WAVE + 2 * ROW + 16 * 7, T + WAVE + 2 * ROW, T + 2 * WAVE, 2 * T], ids=["chunk", "row", "wave", "tile"])
def test_gpu_seams(L, edge):
    """each of the seven segment kinds beginning at bytes E - 2 .. E + 1 of the 16-B grid, E the edge of a 16-B chunk, of the 1 KiB
    one store instruction writes, of a wave's 4 KiB and of a tile -- so that every kind straddles E, and the one-byte kinds lie on
    either side of it; then one record of 2^16 bases across several tiles"""
    rng = np.random.default_rng(184)
    ran = 0
    for kind in range(len(KINDS)):
        for d in (-2, -1, 0, 1):
            phase = (5 * ran) % 16
            check_dev(seam_case(rng, kind, edge + d - phase), text_phase=phase, qual_phase=ran % 4, names_phase=ran % 3, tag=(KINDS[kind], d))
            ran += 1
    check_host(L, seam_case(rng, 3, edge))
    for phase in (0, 11):
        check_dev(make_case(rng, [7, 1 << 16, 9], [13, 40, 0]), text_phase=phase, tag=("long",))


@gpu
def test_gpu_empty_records():
    """5000 records of 6 bytes, three to a chunk: the longest piece range a wave can meet; then with a 1-base record here and there"""
    rng = np.random.default_rng(185)
    assert check_dev(make_case(rng, [0] * 5000, None), text_phase=3) == (30000, 0)
    assert check_dev(make_case(rng, [0] * 5000, [0] * 5000), text_phase=14) == (30000, 0)
    lens = (rng.random(5000) < 0.02).astype(np.int64)
    assert check_dev(make_case(rng, lens, [0] * 5000), text_phase=9) == (30000 + 2 * int(lens.sum()), 0)


@gpu
def test_gpu_capacities(L):
    """a text of about 40 KiB cut at 0, 1, 15, 16, 17, every seam of every record +- 1, |text| - 1, |text| and the bound: the
    prefix is written, the canaries behind the footprint stay, the counts stay full, and the host tier answers CNT_ECAP exactly
    when |text| > text_cap"""
    rng = np.random.default_rng(186)
    lens, name_lens = [150, 0, 9000, 33, 10300], [40, 0, 13, 1, 2]
    case = make_case(rng, lens, name_lens, slack=(0, 4))
    total = bound(sum(lens), 5, sum(name_lens))
    assert 39000 < total < 41000 and bound(sum(lens), 5, len(case[3])) == total + 4
    caps, at = {0, 1, 15, 16, 17, total - 1, total, total + 4}, 0
    for l, nl in zip(lens, name_lens):
        for seam in (0, 1, 1 + nl, 2 + nl, 2 + nl + l, 5 + nl + l, 5 + nl + 2 * l):
            caps |= {at + seam + d for d in (-1, 0, 1) if at + seam + d >= 0}
        at += 6 + nl + 2 * l
    assert at == total and len(caps) > 60
    for k, cap in enumerate(sorted(caps)):
        assert check_dev(case, text_cap=cap, text_phase=k % 16, tag=(cap,)) == (total, 0)
        check_host(L, case, text_cap=cap, pinned=k % 2 == 0, with_rec_text=k % 3 != 0, tag=(cap,))


@gpu
def test_gpu_malformed_tables(L):
    """the counts are set, the canaries and every byte of text and rec_text are untouched, the host tier returns CNT_EINVAL"""
    rng = np.random.default_rng(188)
    for length, rec_start, names_len, name_off, count in MALFORMED:
        case = (random_letters(rng, length), b"I" * length, rec_start, (b"n" * names_len if name_off is not None else None), name_off)
        assert check_dev(case) == (0, count)
        assert check_host(L, case) == (0, count) and check_host(L, case, pinned=True) == (0, count)
    # tables that would send a kernel far outside: huge starts, huge name offsets, a descent late in a long table
    huge = (1 << 64) - 1
    for rec_start, name_off in (([0, huge], None), ([huge, huge], None), ([huge, 0], None), ([0, 10], [0, huge, 5]), ([0, 10], [huge, huge, huge]),
                                ([0, 10], [0, 1 << 40, 1 << 41]), ([1 << 63, 1 << 63], [0, 0, 0])):
        case = (random_letters(rng, 100), b"I" * 100, rec_start, b"n" * 20 if name_off is not None else None, name_off)
        assert check_dev(case)[1] > 0 and check_host(L, case)[1] > 0
    starts = np.sort(rng.integers(0, 5000, 3 * BLOCK)).tolist()
    starts[0] = 0
    starts[2 * BLOCK + 5] = starts[2 * BLOCK + 6] + 1
    assert check_dev((random_letters(rng, 5000), b"#" * 5000, starts, None, None), text_phase=5) == (0, 1)


@gpu
def test_gpu_scan_round_edge():
    """R + 1 pieces one more than a round of the one-workgroup scan and 300: records of 0 to 3 bases, about 3 MB of text"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(189)
    n_rec = ROUND + 300
    lens = rng.integers(0, 4, n_rec)
    case = make_case(rng, lens, None)
    want, want_rt, _ = np_write(*case)
    n = len(case[0])
    assert 2 * (1 << 20) < want.size < 4 * (1 << 20)
    d_bits = torch.from_numpy(case_words(case[0]).view(np.int64)).cuda()
    d_qual = torch.from_numpy(np.frombuffer(case[1], dtype=np.uint8).copy()).cuda()
    d_rs = torch.from_numpy(np.asarray(case[2], dtype=np.int64)).cuda()
    foot = bound(n, n_rec, 0)
    d_text = torch.full((foot + GUARD,), BYTE, dtype=torch.uint8, device="cuda")
    d_rt = torch.full((n_rec + PAD,), CANARY, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((2,), CANARY, dtype=torch.int64, device="cuda")
    d_work = torch.full((po.bits_to_fastq_work_bytes(n_rec),), 0x77, dtype=torch.uint8, device="cuda")
    po.bits_to_fastq_dev(d_bits, n, d_qual, d_rs, d_text[:foot], d_cnt, d_work, rec_text=d_rt[:n_rec])
    torch.cuda.synchronize()
    assert d_cnt.cpu().numpy().tolist() == [want.size, 0] and foot == want.size
    h = d_text.cpu().numpy()
    assert np.array_equal(h[:foot], want) and (h[foot:] == BYTE).all()
    rt = d_rt.cpu().numpy()
    assert np.array_equal(rt[:n_rec].view(np.uint64), want_rt) and (rt[n_rec:] == CANARY).all()


@gpu
def test_gpu_records_across_launch_seams(launch_tiles):
    """the lab build cut into launches of 64 / 128 tiles: a text of three launches and a bit, a record across every launch seam of
    the write pass, the size pass in several launches too; the launches counted in a captured graph"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(launch_tiles)
    per_launch = launch_tiles * T
    n_small = launch_tiles * BLOCK + 10  # enough empty records for several launches of the size pass
    lens, name_lens, at = [0] * n_small, [0] * n_small, 6 * n_small
    assert at < per_launch
    while at < 3 * per_launch + 5000:  # reads whose sizes share no factor with the seams
        lens.append(int(rng.integers(1000, 3000)))
        name_lens.append(int(rng.integers(0, 60)))
        at += 6 + name_lens[-1] + 2 * lens[-1]
    case = make_case(rng, lens, name_lens)
    total, _ = check_dev(case, tag=(launch_tiles,))
    rt = np_write(*case)[1].astype(np.int64)
    ends = np.r_[rt[1:], total]
    for seam in (per_launch, 2 * per_launch, 3 * per_launch):  # a record begins in front of each seam and ends behind it
        r = int(np.searchsorted(rt, seam, side="right")) - 1
        assert rt[r] < seam - 16 and ends[r] > seam + 16, (seam, rt[r], ends[r])
    n, R = len(case[0]), len(lens)
    foot = bound(n, R, len(case[3]))
    tiles, launches = write_plan(foot, R, 0, launch_tiles)
    assert tiles > 3 * launch_tiles and launches >= 2 * 2 + 1 + 4
    d_bits = torch.from_numpy(case_words(case[0]).view(np.int64)).cuda()
    d_qual = torch.from_numpy(np.frombuffer(case[1], dtype=np.uint8).copy()).cuda()
    d_rs, d_no = (torch.from_numpy(np.asarray(x, dtype=np.int64)).cuda() for x in (case[2], case[4]))
    d_names = torch.from_numpy(np.frombuffer(case[3], dtype=np.uint8).copy()).cuda()
    text, cnt = torch.empty(foot, dtype=torch.uint8, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
    work = torch.empty(po.bits_to_fastq_work_bytes(R), dtype=torch.uint8, device="cuda")
    assert _kernel_nodes_of(torch, lambda: po.bits_to_fastq_dev(d_bits, n, d_qual, d_rs, text, cnt, work, names=d_names, name_off=d_no)) == launches


@gpu
def test_gpu_write_in_a_captured_graph_and_behind_a_side_stream():
    """one torch.cuda.graph capture of the call replayed twice on changed words, qualities and tables; then the call enqueued on a
    side stream behind the copies that make its input, no host sync in between"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(191)
    R, n = 50, 5 * T
    bits, qual = torch.zeros(words_for(n), dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    rs, no = torch.zeros(R, dtype=torch.int64, device="cuda"), torch.zeros(R + 1, dtype=torch.int64, device="cuda")
    names = torch.zeros(R * 10, dtype=torch.uint8, device="cuda")
    foot = bound(n, R, R * 10)
    text, rt, cnt = torch.empty(foot, dtype=torch.uint8, device="cuda"), torch.empty(R, dtype=torch.int64, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
    work = torch.empty(po.bits_to_fastq_work_bytes(R), dtype=torch.uint8, device="cuda")

    def call():
        po.bits_to_fastq_dev(bits, n, qual, rs, text, cnt, work, names=names, name_off=no, rec_text=rt)

    def make():
        cuts = np.sort(rng.integers(0, n, R))
        cuts[0] = 0
        return random_letters(rng, n), QUALS[rng.integers(0, QUALS.size, n)].tobytes(), cuts.tolist(), random_letters(rng, R * 10), (np.arange(R + 1) * 10).tolist()

    def load(case, non_blocking=False):
        for dst, src in ((bits, case_words(case[0]).view(np.int64)), (qual, np.frombuffer(case[1], dtype=np.uint8).copy()), (rs, np.asarray(case[2], dtype=np.int64)),
                         (no, np.asarray(case[4], dtype=np.int64)), (names, np.frombuffer(case[3], dtype=np.uint8).copy())):
            dst.copy_(torch.from_numpy(src).pin_memory() if non_blocking else torch.from_numpy(src), non_blocking=non_blocking)

    def verify(case, rep):
        want, want_rt, _ = np_write(*case)
        assert cnt.cpu().numpy().tolist() == [want.size, 0], rep
        assert np.array_equal(text[: want.size].cpu().numpy(), want) and np.array_equal(rt.cpu().numpy().view(np.uint64), want_rt), rep

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()  # module load outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for rep in range(2):
        case = make()
        load(case)
        for x in (text, rt, cnt):
            x.fill_(0x5A)
        work.fill_(0x77 + rep)  # the scratch needs no zeroing
        g.replay()
        torch.cuda.synchronize()
        verify(case, rep)
    case = make()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        load(case, non_blocking=True)
        call()
    torch.cuda.current_stream().wait_stream(side)
    verify(case, 2)


@gpu
def test_gpu_round_trip_on_the_device():
    """bits_to_fastq_dev then fastq_to_bits_dev gives back the words, the qualities, rec_start == rec_qual == the input and a
    rec_text equal to the writer's; then the other way through the host tier: text, fastq_to_bits_hip, bits_to_fastq_hip with
    the names fastq_names cuts out, and the same text"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(192)
    R = 300
    case = make_case(rng, [int(x) for x in rng.choice([0, 1, 59, 60, 61, 150, 2000, T], R)], [int(x) for x in rng.integers(0, 50, R)])
    letters, qual, rec_start, names, name_off = case
    n = len(letters)
    words = case_words(letters)
    d_bits = torch.from_numpy(words.view(np.int64)).cuda()
    d_qual = torch.from_numpy(np.frombuffer(qual, dtype=np.uint8).copy()).cuda()
    d_rs, d_no = (torch.from_numpy(np.asarray(x, dtype=np.int64)).cuda() for x in (rec_start, name_off))
    d_names = torch.from_numpy(np.frombuffer(names, dtype=np.uint8).copy()).cuda()
    foot = bound(n, R, len(names))
    text, rt, cnt = torch.empty(foot, dtype=torch.uint8, device="cuda"), torch.empty(R, dtype=torch.int64, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
    work = torch.empty(po.bits_to_fastq_work_bytes(R), dtype=torch.uint8, device="cuda")
    po.bits_to_fastq_dev(d_bits, n, d_qual, d_rs, text, cnt, work, names=d_names, name_off=d_no, rec_text=rt)
    total, bad = cnt.cpu().numpy().tolist()
    want = np_write(*case)[0]
    assert bad == 0 and total == want.size == foot
    back = torch.full((words_for(total),), CANARY, dtype=torch.int64, device="cuda")
    qual2 = torch.full((total,), BYTE, dtype=torch.uint8, device="cuda")
    rt2, rs2, rq2 = (torch.empty(R + 5, dtype=torch.int64, device="cuda") for _ in range(3))
    cnt2 = torch.empty(5, dtype=torch.int64, device="cuda")
    work2 = torch.empty(po.fastq_to_bits_work_bytes(total), dtype=torch.uint8, device="cuda")
    po.fastq_to_bits_dev(text[:total], back, cnt2, work2, qual=qual2, rec_text=rt2, rec_start=rs2, rec_qual=rq2)
    assert cnt2.cpu().numpy().tolist() == [n, R, 0, n, 0]
    assert torch.equal(back[: words_for(n)], d_bits) and torch.equal(qual2[:n], d_qual)
    assert torch.equal(rs2[:R], d_rs) and torch.equal(rq2[:R], d_rs) and torch.equal(rt2[:R], rt)
    # the other way, through the host tier and the Python layer
    source = want.tobytes()
    f = po.fastq_to_bits_hip(source)
    assert f.malformed == 0 and f.invalid == 0 and np.array_equal(f.rec_start, f.rec_qual)
    assert po.bits_to_fastq_hip(f.words, f.n, f.qual, f.rec_start, po.fastq_names(source, f.rec_text)) == source


@gpu
def test_gpu_host_tier_pinned_and_pageable(L):
    """pinned host buffers (used in place) and pageable ones (staged); then the Python wrapper on the real library"""
    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(193)
    cases = (make_case(rng, [2 * T + 77, 0, 1000], [2, 0, 41]), make_case(rng, [T + 5], None), make_case(rng, [0, 0], None), make_case(rng, [150] * 100, [40] * 100))
    for case in cases:
        total = len(def_write(*case)[0])
        for pinned in (False, True):
            for cap in (None, total, total - 1):
                for with_rec_text in (True, False):
                    check_host(L, case, text_cap=cap, with_rec_text=with_rec_text, pinned=pinned)
    letters, qual, rec_start, names, name_off = cases[0]
    name_list = [names[name_off[r] : name_off[r + 1]] for r in range(3)]
    text = po.bits_to_fastq_hip(case_words(letters), len(letters), qual, np.asarray(rec_start, dtype=np.uint64), name_list)
    assert text == def_write(*cases[0])[0]
    with pytest.raises(Exception):
        po.bits_to_fastq_hip(case_words(letters), len(letters), qual, np.array([0, 5, 3], dtype=np.uint64))


@gpu
def test_gpu_fuzz(L):
    """300 random tables under 64 KiB of text against the numpy reference: record and name lengths from a byte to several tiles,
    capacities, phases of every pointer.  No case is skipped"""
    rng = np.random.default_rng(194)
    for k in range(300):
        n_rec = int(rng.choice([1, 2, 5, 40, 300]))
        most = int(rng.choice([3, 70, 500 if n_rec <= 40 else 70, T // n_rec if n_rec <= 5 else 70]))
        lens = [int(x) for x in rng.integers(0, most + 1, n_rec)]
        name_most = int(rng.choice([1, 30, T // 2 if n_rec <= 2 else 30]))
        name_lens = [int(x) for x in rng.integers(0, name_most + 1, n_rec)] if rng.random() < 0.7 else ([0] * n_rec if rng.random() < 0.5 else None)
        case = make_case(rng, lens, name_lens, slack=(int(rng.integers(0, 3)), int(rng.integers(0, 3))))
        total = bound(sum(lens), n_rec, sum(name_lens or [0]))
        assert total < 64 * 1024
        cap = [None, None, total, max(total - 1, 0), int(rng.integers(0, total + 1))][int(rng.integers(0, 5))]
        got = check_dev(case, text_cap=cap, text_phase=int(rng.integers(0, 16)), qual_phase=int(rng.integers(0, 16)), names_phase=int(rng.integers(0, 16)),
                        with_rec_text=bool(rng.integers(0, 4)), tag=(k,))
        assert got == (total, 0)
        if k % 10 == 0:
            check_host(L, case, text_cap=cap, pinned=k % 20 == 0, tag=(k,))
