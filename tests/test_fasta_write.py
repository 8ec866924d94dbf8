"""Packed words to FASTA text: header lines and wrapped lines (include/cute_nt.h "text formats: FASTA write",
hip/fasta_write_kernels.hpp, hip/fasta_write_abi.inc).  Not in the reference, which stops at bits_to_n_*: the definition is
restated here twice -- a byte-by-byte writer and a numpy closed form -- the two are pinned against each other, and the text is
read back through tests/test_fasta.py's def_fasta: cnt_fasta_to_bits(cnt_bits_to_fasta(x)) == x on well-formed input.

CPU part: the references, the round trip and the bound, malformed tables, every argument rule of both tiers and both queries in
the order the header states them (all of them precede device work), an aliasing sweep of every (written, other) pair, the Python
layer without a device, the header's comment.  GPU part: both tiers byte for byte against the numpy reference, with canaries
around the text's footprint, rec_text and counts."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from test_aliasing import OVERLAPS, TOUCHES, Arena, Buf, Call, pairs, place, shared_bytes
from test_fasta import def_fasta, np_fasta, np_words, words_for
from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16384  # bytes of text per workgroup tile of the write pass (hip/fasta_write_kernels.hpp kFastaOutTile)
LANE, WAVE = 64, 64 * 64  # bytes per lane and per wave of a tile; a lane writes four 16-B chunks
BLOCK = 256  # pieces per workgroup of the size pass
ROUND = 1024 * BLOCK  # pieces one round of fasta_out_scan takes: kFastaOutScanBlock lanes, a block each
NL, GT = 0x0A, 0x3E
ACTG = np.frombuffer(b"ACTG", dtype=np.uint8)  # the decoder's table
WIDTHS = (0, 1, 2, 3, 7, 15, 16, 17, 60, 61, 80)


# ---- the two references ---------------------------------------------------------------------------------------------------------
def malformed_count(length, rec_start, name_off, names_len):
    s = [int(x) for x in rec_start] + [length]
    bad = sum(1 for r in range(len(rec_start)) if s[r] > s[r + 1])
    if name_off is not None:
        o = [int(x) for x in name_off]
        bad += sum(1 for r in range(len(rec_start)) if o[r] > o[r + 1]) + (1 if o[-1] > names_len else 0)
    return bad


def def_body(letters, width):
    """body(a, b) of the definition on the letters [a, b), byte by byte"""
    out = bytearray()
    for i, c in enumerate(letters):
        out.append(c)
        if width and (i + 1) % width == 0:
            out.append(NL)
    if len(letters) and (width == 0 or len(letters) % width):
        out.append(NL)
    return bytes(out)


def def_write(letters, rec_start, names, name_off, width):
    """the definition, byte by byte: (text, rec_text, malformed).  letters: the decoded sequence as bytes; names: the name bytes or
    None; name_off: R + 1 offsets or None"""
    bad = malformed_count(len(letters), rec_start, name_off, len(names) if names is not None else 0)
    if bad:
        return b"", [], bad
    s = [int(x) for x in rec_start] + [len(letters)]
    text, rec_text = bytearray(def_body(letters[: s[0]], width)), []
    for r in range(len(rec_start)):
        rec_text.append(len(text))
        text.append(GT)
        if name_off is not None:
            text += names[int(name_off[r]) : int(name_off[r + 1])]
        text.append(NL)
        text += def_body(letters[s[r] : s[r + 1]], width)
    return bytes(text), rec_text, 0


def np_body(letters, a, b, width):
    """the closed form: output byte j of a body has column j % (W + 1), line j / (W + 1) and base line * W + col"""
    l = b - a
    w = width if width else max(l, 1)
    j = np.arange(l + -(-l // w), dtype=np.int64)
    col, line = j % (w + 1), j // (w + 1)
    base = line * w + col
    feed = (col == w) | (base >= l)
    return np.where(feed, np.uint8(NL), letters[a + np.minimum(base, max(l - 1, 0))] if l else np.uint8(NL)).astype(np.uint8)


def np_write(letters, rec_start, names, name_off, width):
    """vectorised per piece: (text as uint8, rec_text as uint64, malformed)"""
    letters = np.frombuffer(bytes(letters), dtype=np.uint8) if not isinstance(letters, np.ndarray) else letters
    bad = malformed_count(letters.size, rec_start, name_off, len(names) if names is not None else 0)
    if bad:
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint64), bad
    s = [int(x) for x in rec_start] + [letters.size]
    nm = np.frombuffer(bytes(names), dtype=np.uint8) if names is not None else None
    parts, sizes = [np_body(letters, 0, s[0], width)], []
    for r in range(len(rec_start)):
        name = nm[int(name_off[r]) : int(name_off[r + 1])] if name_off is not None else np.zeros(0, dtype=np.uint8)
        body = np_body(letters, s[r], s[r + 1], width)
        parts += [np.array([GT], dtype=np.uint8), name, np.array([NL], dtype=np.uint8), body]
        sizes.append(2 + name.size + body.size)
    rec_text = parts[0].size + np.cumsum([0] + sizes[:-1]) if sizes else np.zeros(0)
    return np.concatenate(parts), np.asarray(rec_text, dtype=np.uint64), 0


def bound(length, n_rec, names_len, width):
    return length + (length // width if width else 0) + (n_rec + 1) + names_len + 2 * n_rec


def random_letters(rng, n):
    return ACTG[rng.integers(0, 4, n)].tobytes()


def make_case(rng, lens, name_lens=None, lead=0, width=60, name_alphabet=b"abc 1>|"):
    """(letters, rec_start, names, name_off, width) of records with these base counts behind `lead` headerless bases"""
    starts = (lead + np.cumsum([0] + list(lens[:-1]))).tolist() if len(lens) else []
    letters = random_letters(rng, lead + sum(lens))
    if name_lens is None:
        return letters, starts, None, None, width
    alphabet = np.frombuffer(name_alphabet, dtype=np.uint8)
    names = alphabet[rng.integers(0, alphabet.size, sum(name_lens))].tobytes()
    return letters, starts, names, np.cumsum([0] + list(name_lens)).tolist(), width


def random_case(rng, most=120):
    width = int(rng.choice(WIDTHS + (most + 5, 1 << 40)))
    n_rec = int(rng.choice([0, 0, 1, 2, 3, 9]))
    lens = [int(rng.choice([0, 0, 1, width or 1, (width or 1) + 1, max((width or 1) - 1, 0), int(rng.integers(0, most))])) % (most + 1) for _ in range(n_rec)]
    lead = int(rng.choice([0, 0, 1, int(rng.integers(0, most))]))
    name_lens = [int(rng.choice([0, 0, 1, int(rng.integers(0, 12))])) for _ in range(n_rec)] if rng.random() < 0.7 else None
    return make_case(rng, lens, name_lens, lead, width)


def sample_cases():
    rng = np.random.default_rng(71)
    cases = [random_case(rng) for _ in range(1000)]
    for width in WIDTHS + (500,):
        cases.append(make_case(rng, [], None, 77, width))  # R == 0: a plain line-wrapped decode
        cases.append(make_case(rng, [0, 0, 0], [0, 0, 0], 0, width))  # len == 0 with R > 0
        cases.append(make_case(rng, [0, 5, 0], [3, 0, 2], 9, width))
    cases.append(make_case(rng, [], None, 0, 60))
    return cases


def test_two_references_agree():
    cases = sample_cases()
    assert len(cases) >= 1000
    seen = set()
    for letters, rec_start, names, name_off, width in cases:
        d, v = def_write(letters, rec_start, names, name_off, width), np_write(letters, rec_start, names, name_off, width)
        assert d[0] == v[0].tobytes() and d[1] == v[1].tolist() and d[2] == v[2] == 0, (letters, rec_start, names, name_off, width)
        seen.add((width, len(rec_start) == 0, bool(rec_start) and rec_start[0] > 0, len(letters) == 0))
    assert {w for w, *_ in seen} >= set(WIDTHS) and any(r0 for _, r0, _, _ in seen) and any(lead for _, _, lead, _ in seen) and any(e for *_, e in seen)
    assert def_write(b"", [], None, None, 60) == (b"", [], 0)
    assert def_write(b"ACGTA", [2], b"xy", [0, 2], 2) == (b"AC\n>xy\nGT\nA\n", [3], 0)
    assert def_write(b"ACGT", [0, 4], None, None, 0) == (b">\nACGT\n>\n", [0, 7], 0)


def test_round_trip_through_the_fasta_definition_and_the_bound():
    """cnt_fasta_to_bits's definition reads the text back: the kept bytes are the letters, rec_text is the writer's, rec_start the
    input -- when no name holds a line feed and no line of the lead begins with '>' (letters never do)"""
    rng = np.random.default_rng(72)
    exact = 0
    for k in range(3000):
        letters, rec_start, names, name_off, width = make_case(rng, *_shape(rng), name_alphabet=b"abc 1>|\r") if k % 2 else random_case(rng)
        if names is not None and NL in names:
            continue
        text, rec_text, bad = def_write(letters, rec_start, names, name_off, width)
        kept, rt, rs = def_fasta(text)
        assert bad == 0 and kept == letters and rt == rec_text and rs == list(rec_start), (letters, rec_start, names, name_off, width)
        names_len = len(names) if names is not None else 0
        b = bound(len(letters), len(rec_start), names_len, width)
        assert len(text) <= b
        pieces = [rec_start[0] if rec_start else len(letters)] + np.diff(list(rec_start) + [len(letters)]).tolist()
        lines = sum(-(-p // width) if width else int(p > 0) for p in pieces)
        assert len(text) == len(letters) + lines + 2 * len(rec_start) + names_len
        # the slack: the bound gives every piece a ragged last line and counts the whole lines of the sequence, not of the pieces
        if width:
            slack = len(letters) // width - sum(p // width for p in pieces) + sum(1 for p in pieces if p % width == 0)
        else:
            slack = sum(1 for p in pieces if p == 0)
        assert slack >= 0 and len(text) == b - slack
        exact += slack == 0
    assert exact > 100


def _shape(rng):
    n_rec = int(rng.integers(0, 6))
    return ([int(rng.integers(0, 200)) for _ in range(n_rec)], [int(rng.integers(0, 30)) for _ in range(n_rec)], int(rng.integers(0, 100)),
            int(rng.choice(WIDTHS)))


MALFORMED = (  # (length, rec_start, names_len, name_off, the count)
    (10, [5, 3], 0, None, 1),  # a descent
    (10, [3, 5, 4, 9, 8], 0, None, 2),
    (10, [11], 0, None, 1),  # rec_start[r] > len: s_r > s_R
    (10, [11, 12], 0, None, 1),
    (10, [0, 5], 8, [0, 5, 4], 1),  # a descent of the names
    (10, [0, 5], 8, [0, 5, 9], 1),  # o_R > names_len
    (10, [0, 5], 8, [9, 9, 9], 1),
    (10, [0, 5], 8, [10, 9, 12], 2),
    (10, [5, 3], 8, [3, 2, 9], 3),  # everything at once
    (0, [1], 0, [0, 0], 1),
)


def test_malformed_tables_in_the_references():
    for length, rec_start, names_len, name_off, count in MALFORMED:
        letters, names = b"ACGT" * 3, (b"n" * names_len if name_off is not None else None)
        d = def_write(letters[:length], rec_start, names, name_off, 4)
        v = np_write(letters[:length], rec_start, names, name_off, 4)
        assert d == (b"", [], count) and v[0].size == 0 and v[1].size == 0 and v[2] == count


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
    assert L.cnt_bits_to_fasta_work_bytes(R, None) == EINVAL and L.cnt_bits_to_fasta_bound(n_len, R, NAMES, 60, None) == EINVAL
    sizes = []
    for r in (0, 1, BLOCK - 2, BLOCK - 1, BLOCK, ROUND, 1 << 30):
        assert L.cnt_bits_to_fasta_work_bytes(r, ctypes.byref(need)) == OK
        sizes.append(need.value)
    assert sizes == sorted(sizes) and 0 < sizes[0] <= 64 and sizes[-1] < 9 * (1 << 30)  # it depends on n_rec only: 8 bytes and a little a record
    assert L.cnt_bits_to_fasta_work_bytes(1 << 62, ctypes.byref(need)) == EINVAL
    for length, r, names_len, width in ((0, 0, 0, 0), (1000, 10, 40, 60), (1000, 10, 40, 0), (59, 0, 0, 60), (60, 0, 0, 60), (1 << 36, 1 << 20, 1 << 25, 1)):
        assert L.cnt_bits_to_fasta_bound(length, r, names_len, width, ctypes.byref(got)) == OK and got.value == bound(length, r, names_len, width)
    big = (1 << 64) - 1
    for args in ((big, 0, 0, 1), (big, 0, 0, 0), (0, big, 0, 0), (0, 1 << 63, 0, 0), (0, (1 << 63) - 1, 0, 60), (1, 0, big, 60), (1 << 63, 0, 1 << 63, 0)):
        got.value = 77
        assert L.cnt_bits_to_fasta_bound(*args, ctypes.byref(got)) == EINVAL and got.value == 77, args
    assert L.cnt_bits_to_fasta_work_bytes(R, ctypes.byref(need)) == OK
    need = need.value

    # slots: 0 bits, 1 rec_start, 2 names, 3 name_off, 4 text, 6 rec_text, 7 counts, 8 work
    def dev(bits=at(0), n=n_len, rs=at(1), r=R, names=at(2), names_len=NAMES, no=at(3), width=60, flags=0, text=at(4), cap=2000, rt=at(6), counts=at(7),
            work=at(8), work_bytes=need):
        return L.cnt_bits_to_fasta_dev(bits, n, rs, r, names, names_len, no, width, flags, text, cap, rt, counts, work, work_bytes, None)

    def host(bits=at(0), n=n_len, rs=at(1), r=R, names=at(2), names_len=NAMES, no=at(3), width=60, flags=0, text=at(4), cap=2000, rt=at(6), counts=at(7)):
        return L.cnt_bits_to_fasta(bits, n, rs, r, names, names_len, no, width, flags, text, cap, rt, ctypes.cast(counts, U64P))

    def untouched():
        return bool((arena == FILL).all())

    off = lambda k, d: vp(at(k).value + d)  # noqa: E731
    for call in (dev, host):
        # 1. an unknown flag, before everything: on empty work, with NULL pointers
        for flags in (1, 2, 4, 0x80000000):
            assert call(flags=flags) == EINVAL and call(flags=flags, n=0, r=0) == EINVAL and call(flags=flags, bits=None, text=None, counts=None) == EINVAL
        # 2. nothing to compute: CNT_OK whatever the pointers are (a host count is zeroed, a device one needs a device)
        assert call(n=0, r=0, bits=None, rs=None, text=None, rt=off(6, 4), counts=None, names=None) == OK and untouched()
        # 3. the NULLs -- in front of 4 (a misaligned rec_text), 5 and 7
        for null in ({"bits": None}, {"text": None}, {"counts": None}, {"rs": None}):
            assert call(**null) == EINVAL and call(**null, rt=off(6, 4)) == EINVAL and call(**null, names=None) == EINVAL
        # 4. alignment of bits, rec_start, name_off, rec_text and counts; text and names may sit anywhere -- in front of 5, 6 and 7
        for name, slot in (("bits", 0), ("rs", 1), ("no", 3), ("rt", 6), ("counts", 7)):
            for d in (1, 4, 7):
                assert call(**{name: off(slot, d)}) == EINVAL
        assert call(rt=off(6, 4), names=None) == EINVAL and call(bits=off(0, 4), text=at(0)) == EINVAL and call(rs=off(1, 4), n=1 << 63, names_len=1 << 63) == EINVAL
        # 5. names without name_off, and the reverse -- in front of 6 and 7
        assert call(names=None) == EINVAL and call(no=None) == EINVAL and call(names=None, text=at(0)) == EINVAL and call(no=None, names_len=big) == EINVAL
        # 6. the bound overflowing size_t -- in front of 7
        assert call(names_len=big) == EINVAL and call(names_len=big, text=at(0)) == EINVAL and call(r=1 << 63, text=at(0)) == EINVAL
        # 7. overlaps, at the stated extents: the footprint of text (here the bound, 1087 bytes), R entries, 16 bytes of counts
        assert bound(n_len, R, NAMES, 60) == 1087
        assert call(text=at(0)) == EINVAL and call(text=off(1, 8 * R - 1)) == EINVAL and call(text=off(2, NAMES - 1)) == EINVAL and call(text=off(3, 8 * R + 7)) == EINVAL
        assert call(rt=off(4, 1080)) == EINVAL and call(text=off(6, -1086)) == EINVAL and call(counts=off(4, 1080)) == EINVAL
        assert call(rt=at(1)) == EINVAL and call(rt=off(3, 8 * R)) == EINVAL and call(counts=off(6, 8 * R - 8)) == EINVAL and call(counts=off(0, 256 - 8)) == EINVAL
        assert call(counts=off(1, -8)) == EINVAL  # the second count lies in rec_start
        assert call(text=off(4, 0), cap=100, counts=off(4, 96)) == EINVAL  # the footprint is min(bound, text_cap)
        assert untouched()
    # 8. the device tier's scratch, after everything else
    assert dev(work=None) == EINVAL and dev(work_bytes=need - 1) == EINVAL and dev(work_bytes=0) == EINVAL
    for other in (0, 1, 2, 3, 4, 6, 7):
        assert dev(work=vp(at(other).value - need + 8)) == EINVAL  # the last 8 bytes of the query's answer reach into the buffer
    assert dev(work=None, text=at(0)) == EINVAL and untouched()
    # the host tier sets its counts on empty work, and only them
    c = np.full(4, 7, dtype=np.uint64)
    assert L.cnt_bits_to_fasta(None, 0, None, 0, None, 0, None, 60, 0, None, 0, None, ctypes.cast(vp(c.ctypes.data + 8), U64P)) == OK
    assert c.tolist() == [7, 0, 0, 7]
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        ENODEV = _lib.CNT_ENODEV
        assert host() == ENODEV and host(names=None, no=None) == ENODEV and host(rt=None) == ENODEV and host(rs=None, r=0, names=None, no=None) == ENODEV
        assert host(text=at(0), cap=0) == ENODEV  # capacity 0: text may sit anywhere, but not at NULL
        assert host(text=off(4, 3), names=off(2, 5), counts=off(4, 3 + 1087 + 6)) == ENODEV  # text and names at any byte; buffers that touch
        assert host(bits=None, n=0, text=at(0)) == ENODEV and host(width=0) == ENODEV and host(width=big) == ENODEV
        assert dev(work=off(8, 4), work_bytes=need) < 0  # a scratch at any address
        assert untouched()


def fasta_write_calls(L):
    """the two tiers as test_aliasing's table rows: every buffer with its extent, its alignment and whether it is written"""
    vp = ctypes.c_void_p
    up = lambda a: ctypes.cast(vp(a), U64P)  # noqa: E731
    n_len, R, names_len, cap = 1000, 24, 96, 1184  # every extent a multiple of 8, so that an 8-B aligned buffer can touch its end
    assert bound(n_len, R, names_len, 60) == 1185
    need = ctypes.c_size_t(0)
    assert L.cnt_bits_to_fasta_work_bytes(R, ctypes.byref(need)) == 0 and need.value % 8 == 0
    need = need.value
    bufs = [Buf("bits", words_for(n_len) * 8, 8, False), Buf("rec_start", R * 8, 8, False), Buf("names", names_len, 1, False), Buf("name_off", (R + 1) * 8, 8, False),
            Buf("text", cap, 1, True), Buf("rec_text", R * 8, 8, True), Buf("counts", 16, 8, True)]
    dev = Call("cnt_bits_to_fasta_dev", bufs + [Buf("work", need, 8, True)],
               lambda p: L.cnt_bits_to_fasta_dev(vp(p["bits"]), n_len, vp(p["rec_start"]), R, vp(p["names"]), names_len, vp(p["name_off"]), 60, 0, vp(p["text"]), cap,
                                                 vp(p["rec_text"]), vp(p["counts"]), vp(p["work"]), need + 64, None), frozenset())
    host = Call("cnt_bits_to_fasta", bufs,
                lambda p: L.cnt_bits_to_fasta(vp(p["bits"]), n_len, vp(p["rec_start"]), R, vp(p["names"]), names_len, vp(p["name_off"]), 60, 0, vp(p["text"]), cap,
                                              vp(p["rec_text"]), up(p["counts"])), frozenset())
    return [dev, host]


def test_aliasing_sweep_of_every_written_buffer(L):
    """every (written, other) pair of both tiers: the five overlapping placements are CNT_EINVAL and write nothing, the two
    touching ones pass the argument checks"""
    from cute_nucleotides_amd import _lib

    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    arena = Arena()
    tried = 0
    for call in fasta_write_calls(L):
        assert len(pairs(call)) == (4 * 7 if call.name.endswith("_dev") else 3 * 6)
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
    assert tried >= (4 * 7 + 3 * 6) * 3  # the first three placements exist for every pair


def test_abi_wiring(L):
    import subprocess

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib, packed_ops as po

    names = ("cnt_bits_to_fasta", "cnt_bits_to_fasta_dev", "cnt_bits_to_fasta_work_bytes", "cnt_bits_to_fasta_bound")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    hpp = open(os.path.join(ROOT, "cute_nucleotides_amd", "cute_nucleotides.hpp")).read()
    for name in names:
        assert name in exported and ("int %s(" % name) in header and ("fn %s(" % name) in rust and (name + "(") in hpp and name in _lib.SIGNATURES, name
    assert "pub fn bits_to_fasta_hip(" in rust and "inline FastaText bits_to_fasta_hip(" in hpp and "pub fn bits_to_fasta_hip_dev(" in rust
    assert "pub fn bits_to_fasta_bound(" in rust and "pub fn bits_to_fasta_work_bytes(" in rust
    for name in ("bits_to_fasta_hip", "bits_to_fasta_dev", "bits_to_fasta_work_bytes", "bits_to_fasta_bound"):
        assert getattr(cn, name) is getattr(po, name) and name in cn.__all__
    assert "#define CNT_ABI_VERSION 1" in header  # symbols were only added: the version did not move
    shim = open(os.path.join(ROOT, "hip", "cute_nt.hip")).read()
    assert shim.index('#include "fastq_abi.inc"') < shim.index('#include "fasta_write_abi.inc"')


def test_header_comment_and_section_place():
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    title = "/* ---- text formats: FASTA write ----"
    assert header.count(title) == 1
    at = header.index(title)
    assert header.index("/* ---- text formats: FASTQ ----") < header.index("int cnt_fastq_to_bits(") < at < header.index("Kernel selection for A/B runs")
    section = header[at : header.index("Kernel selection for A/B runs")]
    for k, name in enumerate(("CNT_FASTA_OUT_TEXT", "CNT_FASTA_OUT_MALFORMED")):
        assert re.search(r"#define %s +%d\b" % (name, k), section) and "counts[%s]" % name in section, name
    checks = ["1. an unknown flag", "2. len == 0 and n_rec == 0", "3. a NULL bits with len > 0, a NULL text, a NULL counts, a NULL rec_start with n_rec > 0",
              "4. a bits, rec_start, name_off, rec_text or counts that is not 8-B aligned", "5. names without name_off", "6. the bound overflowing size_t",
              "7. a written buffer sharing a byte", "8. device tier: a NULL d_work"]
    places = [section.index(c) for c in checks]
    assert places == sorted(places)
    for word in ("A MALFORMED TABLE WRITES NO TEXT", "CNT_EINVAL after the work", "CNT_ECAP after the work", "enqueue-only", "capturable in a graph", "2^36",
                 "NOT validated", "FASTQ writing", "CRLF", "gzip", "per-record widths", "depends on n_rec only", "len + (W ? len / W : 0) + (R + 1) + names_len"):
        assert word in section, word
    fasta = header[header.index("/* ---- text formats: FASTA ----") : header.index("/* ---- text formats: FASTQ ----")]
    assert "line-wrapped decode" not in fasta  # no longer out of scope there


def test_write_plan_matches_the_launcher_source():
    src = open(os.path.join(ROOT, "hip", "fasta_write_kernels.hpp")).read()
    assert "constexpr int kFastaOutBlock = 256;" in src and "kFastaOutLaneBytes = 16 * kFastaOutChunks, kFastaOutTile = kFastaOutLaneBytes * kFastaOutBlock;" in src and "kFastaOutChunks = 4;" in src
    assert "constexpr int kFastaOutScanBlock = 1024;" in src and T == 64 * 256 and ROUND == 1024 * BLOCK
    kernels = [line for line in src.splitlines() if line.startswith("__global__")]
    assert len(kernels) == 4 and not re.search(r"atomic\w*\(|\basm\b", src)
    abi = open(os.path.join(ROOT, "hip", "fasta_write_abi.inc")).read()
    order = ["hipMemsetAsync(d_counts, 0, 16, s)", "hipLaunchKernelGGL(fasta_out_sizes,", "hipLaunchKernelGGL(fasta_out_scan, dim3(1), dim3(kFastaOutScanBlock), 0, s, a);",
             "hipLaunchKernelGGL(fasta_out_offsets,", "hipLaunchKernelGGL(fasta_out_write,"]
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
    """a stand-in for the library whose cnt_bits_to_fasta is the numpy reference behind the C calling convention"""
    from cute_nucleotides_amd import _lib

    def u64_at(p, n):
        return np.frombuffer((ctypes.c_uint64 * n).from_address(p.value), dtype=np.uint64) if n else np.zeros(0, dtype=np.uint64)

    def cnt_bits_to_fasta_bound(length, n_rec, names_len, width, out):
        out._obj.value = bound(length, n_rec, names_len, width)
        return 0

    def cnt_bits_to_fasta(bits, length, rec_start, n_rec, names, names_len, name_off, width, flags, text, text_cap, rec_text, counts):
        calls.append((length, n_rec, names_len, width, flags, text_cap, names is None, name_off is None))
        letters = letters_of(u64_at(bits, words_for(length)), length) if length else np.zeros(0, dtype=np.uint8)
        nm = bytes((ctypes.c_uint8 * names_len).from_address(names.value)) if names is not None and names_len else (b"" if names is not None else None)
        got, rt, bad = np_write(letters, u64_at(rec_start, n_rec).tolist(), nm, u64_at(name_off, n_rec + 1).tolist() if name_off is not None else None, width)
        counts[0], counts[1] = got.size, bad
        if bad:
            return _lib.CNT_EINVAL
        m = min(got.size, text_cap)
        if m:
            np.frombuffer((ctypes.c_uint8 * m).from_address(text.value), dtype=np.uint8)[:] = got[:m]
        u64_at(rec_text, n_rec)[:] = rt
        return _lib.CNT_ECAP if got.size > text_cap else _lib.CNT_OK

    return types.SimpleNamespace(cnt_bits_to_fasta=cnt_bits_to_fasta, cnt_bits_to_fasta_bound=cnt_bits_to_fasta_bound, cnt_words_for=words_for)


def test_bits_to_fasta_hip_builds_the_name_table(monkeypatch):
    from cute_nucleotides_amd import packed_ops as po

    calls = []
    monkeypatch.setattr(po, "lib", lambda: _fake_lib(calls))
    rng = np.random.default_rng(73)
    for _ in range(40):
        letters, rec_start, names, name_off, width = random_case(rng)
        width = min(width, 1 << 30)
        words = np_words(np.frombuffer(letters, dtype=np.uint8), False)
        name_list = [names[name_off[r] : name_off[r + 1]] for r in range(len(rec_start))] if names is not None else None
        del calls[:]
        text, rec_text = po.bits_to_fasta_hip(words, len(letters), np.asarray(rec_start, dtype=np.uint64) if rec_start else None, name_list, width)
        want = def_write(letters, rec_start, names, name_off, width)
        assert text.dtype == np.uint8 and rec_text.dtype == np.uint64 and text.tobytes() == want[0] and rec_text.tolist() == want[1]
        names_len = len(names) if names is not None else 0
        assert calls == [(len(letters), len(rec_start), names_len, width, 0, bound(len(letters), len(rec_start), names_len, width), names is None, names is None)]
    # the default width is 60, the names are what fasta_names returns
    text, rec_text = po.bits_to_fasta_hip(np_words(np.frombuffer(b"ACGT" * 20, dtype=np.uint8), False), 80, np.array([0, 70], dtype=np.uint64), [b"a b", bytearray(b"")])
    assert text.tobytes() == b">a b\n" + b"ACGT" * 15 + b"\n" + b"ACGTACGTAC\n>\nGTACGTACGT\n" and rec_text.tolist() == [0, 77]
    assert po.fasta_names(text, rec_text) == [b"a b", b""]
    assert po.bits_to_fasta_hip(np.zeros(0, dtype=np.uint64), 0)[0].size == 0
    # a malformed table is an error; so are a name list of another length, a negative width and words of another type
    with pytest.raises(Exception):
        po.bits_to_fasta_hip(np.zeros(1, dtype=np.uint64), 10, np.array([5, 3], dtype=np.uint64))
    with pytest.raises(ValueError):
        po.bits_to_fasta_hip(np.zeros(1, dtype=np.uint64), 10, np.array([5], dtype=np.uint64), [b"a", b"b"])
    with pytest.raises(ValueError):
        po.bits_to_fasta_hip(np.zeros(1, dtype=np.uint64), 10, width=-1)
    with pytest.raises(ValueError):
        po.bits_to_fasta_hip(np.zeros(1, dtype=np.uint64), 33)
    with pytest.raises(TypeError):
        po.bits_to_fasta_hip(np.zeros(1, dtype=np.int32), 10)


def test_device_wrapper_argument_errors():
    torch = pytest.importorskip("torch")
    from cute_nucleotides_amd import packed_ops as po

    t = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(ValueError):
        po.bits_to_fasta_dev(t, 10, t, t, t)  # not on a device


# ---------------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
CANARY = -0x3C3C3C3C3C3C3C3D
BYTE = 0xC3  # the canary's bytes
HOST_CANARY = 0xDEADBEEFDEADBEEF
PAD = 5  # canary words in front of and behind rec_text and counts
GUARD = 64  # canary bytes in front of and behind the text's footprint


def case_words(letters):
    return np_words(np.frombuffer(bytes(letters), dtype=np.uint8), False)


def check_dev(case, text_cap=None, text_phase=0, names_phase=0, with_rec_text=True, dirty_bits=True, tag=()):
    """the device tier on the case: text, rec_text, counts, canaries around every footprint.  Returns (|text|, malformed)"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    letters, rec_start, names, name_off, width = case
    n, R = len(letters), len(rec_start)
    names_len = len(names) if names is not None else 0
    want, want_rt, bad = np_write(letters, rec_start, names, name_off, width)
    b = bound(n, R, names_len, width)
    cap = b if text_cap is None else text_cap
    foot = min(b, cap)
    words = case_words(letters)
    if dirty_bits and n % 32:  # bits beyond len are ignored
        words[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(2 * (n % 32))
    d_bits = torch.from_numpy(np.r_[words, np.zeros(1, dtype=np.uint64)].view(np.int64)).cuda()[: words.size]
    d_rs = torch.from_numpy(np.asarray(rec_start, dtype=np.uint64).view(np.int64)).cuda() if R else None
    d_names = d_no = None
    if names is not None:
        parent = torch.from_numpy(np.frombuffer(b"\n" * (16 + names_phase) + bytes(names) + b"\n>" * 8, dtype=np.uint8).copy()).cuda()
        d_names = parent[16 + names_phase : 16 + names_phase + names_len]
        d_no = torch.from_numpy(np.asarray(name_off, dtype=np.uint64).view(np.int64)).cuda()
    d_parent = torch.full((GUARD + text_phase + foot + GUARD,), BYTE, dtype=torch.uint8, device="cuda")
    d_text = d_parent[GUARD + text_phase : GUARD + text_phase + foot]
    assert foot == 0 or d_text.data_ptr() % 16 == text_phase % 16
    d_rt = torch.full((PAD + R + PAD,), CANARY, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((4,), CANARY, dtype=torch.int64, device="cuda")
    d_work = torch.full((po.bits_to_fasta_work_bytes(R) + 8,), 0x77, dtype=torch.uint8, device="cuda")
    po.bits_to_fasta_dev(d_bits, n, d_text, d_cnt[1:3], d_work[4:], rec_start=d_rs, names=d_names, name_off=d_no, width=width,  # the scratch 4 bytes off
                         rec_text=d_rt[PAD : PAD + R] if with_rec_text else None, text_cap=cap)
    torch.cuda.synchronize()
    tag = tag + (n, R, names_len, width, cap, text_phase, names_phase)
    assert d_cnt.cpu().numpy().tolist() == [CANARY, want.size, bad, CANARY], tag
    h = d_parent.cpu().numpy()
    lo = GUARD + text_phase
    m = min(want.size, cap)
    assert (h[:lo] == BYTE).all() and (h[lo + foot :] == BYTE).all(), tag + ("text canary",)
    got = h[lo : lo + m]
    assert np.array_equal(got, want[:m]), tag + ("text", np.flatnonzero(got != want[:m])[:4].tolist(), got[:80].tobytes(), want[:80].tobytes())
    rt = d_rt.cpu().numpy()
    if bad:
        assert (h == BYTE).all() and (rt == CANARY).all(), tag + ("malformed",)
    elif with_rec_text:
        assert (rt[:PAD] == CANARY).all() and (rt[PAD + R :] == CANARY).all() and np.array_equal(rt[PAD : PAD + R].view(np.uint64), want_rt), tag + ("rec_text",)
    else:
        assert (rt == CANARY).all(), tag + ("rec_text",)
    return want.size, bad


def check_host(L, case, text_cap=None, with_rec_text=True, pinned=False, tag=()):
    """the host tier on the case, pageable or pinned buffers, text and names at odd bytes inside their allocations"""
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    letters, rec_start, names, name_off, width = case
    n, R = len(letters), len(rec_start)
    names_len = len(names) if names is not None else 0
    want, want_rt, bad = np_write(letters, rec_start, names, name_off, width)
    b = bound(n, R, names_len, width)
    cap = b if text_cap is None else text_cap
    foot = min(b, cap)
    alloc = (lambda k, dt=np.uint64: cn.pinned_empty(k, dt)) if pinned else (lambda k, dt=np.uint64: np.empty(k, dtype=dt))
    bits, rs, no = alloc(words_for(n) + 1), alloc(R + 1), alloc(R + 2)
    bits[: words_for(n)] = case_words(letters)
    rs[:R] = np.asarray(rec_start, dtype=np.uint64)
    nm = alloc(names_len + 8, np.uint8)
    if names is not None:
        no[: R + 1] = np.asarray(name_off, dtype=np.uint64)
        nm[3 : 3 + names_len] = np.frombuffer(bytes(names), dtype=np.uint8)
    text, rt, cnt = alloc(GUARD + 3 + foot + GUARD, np.uint8), alloc(PAD + R + PAD), alloc(4)
    text[:] = BYTE
    rt[:] = HOST_CANARY
    cnt[:] = HOST_CANARY
    rc = L.cnt_bits_to_fasta(bits.ctypes.data if n else None, n, rs.ctypes.data if R else None, R, nm[3:].ctypes.data if names is not None else None, names_len,
                             no.ctypes.data if names is not None else None, width, 0, text[GUARD + 3 :].ctypes.data, cap,
                             rt[PAD:].ctypes.data if with_rec_text else None, cnt[1:].ctypes.data)
    tag = tag + (n, R, names_len, width, cap, pinned)
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


def case_of_total(rng, total):
    """a case whose text holds exactly `total` bytes: records in front, and a last record at width 0 that fills up"""
    if total < 4:
        return make_case(rng, [], None, max(total - 1, 0), 0) if total != 1 else None
    width = int(rng.choice((0, 1, 7, 60)))
    for _ in range(200):
        n_rec = int(rng.integers(0, min(3, total // 8) + 1))
        lens, name_lens = [int(rng.integers(0, total // 4 + 1)) for _ in range(n_rec)], [int(rng.integers(0, 6)) for _ in range(n_rec)]
        case = make_case(rng, lens, name_lens, int(rng.integers(0, total // 4 + 1)), width)
        size = def_write(*case)[0]
        rest = total - len(size) - 2
        if rest >= 0 and (width == 0 and rest != 1 or width == 1 and rest % 2 == 0 or width > 1 and rest % (width + 1) != 1):
            bases = rest - (rest > 0) if width == 0 else rest // 2 if width == 1 else rest - -(-rest // (width + 1))
            case = make_case(rng, lens + [bases], name_lens + [0], len(case[0]) - sum(lens), width)
            if len(def_write(*case)[0]) == total:
                return case
    return None


@gpu
def test_gpu_every_total_length_and_random_small_cases(L):
    """texts of every length 0..200 (1 is no text: a body holds two bytes or none), then 300 random small cases, both tiers"""
    rng = np.random.default_rng(81)
    for total in range(201):
        case = case_of_total(rng, total)
        assert (case is None) == (total == 1), total
        if case is not None:
            assert check_dev(case, text_phase=total % 16, names_phase=total % 7) == (total, 0)
            check_host(L, case)
    for k in range(300):
        case = random_case(rng, most=400)
        check_dev(case, text_phase=k % 16, names_phase=k % 8, with_rec_text=k % 5 != 0, tag=(k,))
        if k % 4 == 0:
            check_host(L, case, with_rec_text=k % 8 != 0, tag=(k,))


SEAM_WIDTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 60, 61, 63, 64, 80, T - 1, T, T + 1)
EDGES = (("tile", T), ("second tile", 2 * T), ("wave", T + WAVE), ("lane", T + 37 * LANE), ("16 bytes", T + WAVE + LANE + 16), ("third chunk", 5 * LANE + 32))


def seam_case(rng, width, at, variant):
    """records placed so that record 1's '>' is text byte `at`: the line feed that ends record 0 lies at at - 1, record 1's one-byte
    name at at + 1 and its line feed at at + 2; behind it records of 0, 1, W-1, W and W+1 bases"""
    w = width or 40
    sizes = [0, 1, w - 1, w, w + 1]
    l0 = min(2 * w + 3, max(at - 8, 0) // 2)
    head = 2 + len(def_body(b"A" * l0, width))
    if at - head < 0:
        return None
    lens = [l0, sizes[variant % 5]] + sizes + [5]
    name_lens = [at - head, 1] + [0, 2, 0, 17, 1] + [3]
    case = make_case(rng, lens, name_lens, 0, width)
    assert int(np_write(*case)[1][1]) == at
    return case


@gpu
@pytest.mark.parametrize("phase", [0, 5, 15])
def test_gpu_seams(L, phase):
    """a record end, a '>', the last byte of a name and a header's line feed at output bytes E - 1, E and E + 1 of the 16-B grid for
    E a tile, wave and lane edge; the line feeds of wrapped lines wander over the edges with the widths"""
    rng = np.random.default_rng(82 + phase)
    ran = 0
    for width in SEAM_WIDTHS:
        for where, edge in EDGES:
            for d in range(-3, 3):
                case = seam_case(rng, width, edge + d - phase, ran)
                assert case is not None
                check_dev(case, text_phase=phase, names_phase=ran % 8, tag=(where, d))
                ran += 1
                if ran % 40 == 0:
                    check_host(L, case, tag=(where, d))
        # one long body whose line feeds fall on every residue of the lane grid, behind a header of 2 + k bytes
        for k in (0, 1, 2):
            check_dev(make_case(rng, [3 * T + 7], [k], 0, width), text_phase=phase, tag=("long", k))
    assert ran == len(SEAM_WIDTHS) * len(EDGES) * 6


@gpu
def test_gpu_pointer_phases():
    """all 16 phases of d_text crossed with 8 phases of d_names"""
    rng = np.random.default_rng(83)
    case = make_case(rng, [70, 0, 2 * T + 100, 1, 333], [5, 0, 40, 1, 2 * T + 3], 50, 60)
    sizes = {check_dev(case, text_phase=tp, names_phase=npz) for tp in range(16) for npz in range(8)}
    assert len(sizes) == 1


@gpu
def test_gpu_bit_phases():
    """a body starting at every bit phase: rec_start % 32 in 0..31, at the fast path's size and at a small one"""
    rng = np.random.default_rng(84)
    for lead in range(32):
        check_dev(make_case(rng, [3 * T + 5, 40], [3, 0], lead, 60), text_phase=lead % 16)
        check_dev(make_case(rng, [45, 1, 33], None, lead, 7), text_phase=lead % 16)
        check_dev(make_case(rng, [], None, 2 * T + lead, 61))


@gpu
def test_gpu_capacities(L):
    """text_cap in {0, 1, |text| - 1, |text|, |text| + 1}: the prefix is written, the canaries behind the footprint stay, the counts
    stay full and the host tier answers CNT_ECAP after the work"""
    rng = np.random.default_rng(85)
    for case in (make_case(rng, [100, 0, 2 * T + 77, 61], [4, 0, 30, 1], 33, 60), make_case(rng, [], None, T + 99, 80), make_case(rng, [5, 3], [1, 1], 0, 0)):
        total = len(def_write(*case)[0])
        for cap in (0, 1, total - 1, total, total + 1):
            for phase in (0, 9):
                assert check_dev(case, text_cap=cap, text_phase=phase) == (total, 0)
            check_host(L, case, text_cap=cap)
            check_host(L, case, text_cap=cap, pinned=True, with_rec_text=False)


@gpu
def test_gpu_fast_path():
    """one record of 3 T + 7 letters at widths 60 and T + 1 (and, around them, the widths at which a lane's division changes)"""
    rng = np.random.default_rng(86)
    for width in (60, T + 1, 0, 1, 15, T - 1, T, 1 << 31, (1 << 36) + 1):
        for named in (None, [0], [40]):
            check_dev(make_case(rng, [3 * T + 7], named, 0, width), text_phase=width % 16)
    check_dev(make_case(rng, [], None, 40 * T + 1, 60))


@gpu
def test_gpu_general_path():
    """thousands of 2-byte records ('>' and a line feed), and reads of 150 with 40-byte names"""
    rng = np.random.default_rng(87)
    assert check_dev(make_case(rng, [0] * 5000, None, 0, 60), text_phase=3) == (10000, 0)
    assert check_dev(make_case(rng, [0] * 5000, [0] * 5000, 0, 0)) == (10000, 0)
    total, _ = check_dev(make_case(rng, [150] * 700, [40] * 700, 0, 0), text_phase=7, names_phase=3)
    assert total == 700 * (42 + 151)
    check_dev(make_case(rng, [150] * 700, [40] * 700, 11, 60), text_phase=12)
    check_dev(make_case(rng, [int(x) for x in rng.integers(0, 400, 600)], [int(x) for x in rng.integers(0, 60, 600)], 0, 80))


@gpu
@pytest.mark.parametrize("n_rec", [BLOCK - 2, BLOCK - 1, BLOCK, 2 * BLOCK - 1, ROUND - 2, ROUND - 1, ROUND, ROUND + 1])
def test_gpu_size_scan_edges(n_rec):
    """R + 1 pieces at the edge of a workgroup of the size pass and of a round of the one-workgroup scan, +-1: empty records and
    empty names but for a few planted ones, the expected text written down in closed form"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(n_rec)
    planted = sorted({0, 1, BLOCK - 2, BLOCK - 1, BLOCK, n_rec // 2, n_rec - 2, n_rec - 1} & set(range(n_rec)))
    lens = np.zeros(n_rec, dtype=np.int64)
    lens[planted] = rng.integers(1, 100, len(planted))
    lead = 3
    letters = random_letters(rng, lead + int(lens.sum()))
    starts = lead + np.cumsum(lens) - lens
    sizes = 2 + lens + -(-lens // 60)
    rec_text = 4 + np.cumsum(sizes) - sizes
    want = np.tile(np.array([GT, NL], dtype=np.uint8), n_rec)  # the empty records; the planted ones spliced in from the back
    for r in reversed(planted):
        body = np_body(np.frombuffer(letters, dtype=np.uint8), int(starts[r]), int(starts[r] + lens[r]), 60)
        want = np.r_[want[: 2 * r + 2], body, want[2 * r + 2 :]]
    want = np.r_[np_body(np.frombuffer(letters, dtype=np.uint8), 0, lead, 60), want]
    d_bits = torch.from_numpy(case_words(letters).view(np.int64)).cuda()
    d_rs = torch.from_numpy(starts.astype(np.int64)).cuda()
    foot = bound(len(letters), n_rec, 0, 60)
    d_text = torch.full((foot + GUARD,), BYTE, dtype=torch.uint8, device="cuda")
    d_rt = torch.full((n_rec + PAD,), CANARY, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((2,), CANARY, dtype=torch.int64, device="cuda")
    d_work = torch.full((po.bits_to_fasta_work_bytes(n_rec),), 0x77, dtype=torch.uint8, device="cuda")
    po.bits_to_fasta_dev(d_bits, len(letters), d_text[:foot], d_cnt, d_work, rec_start=d_rs, width=60, rec_text=d_rt[:n_rec])
    torch.cuda.synchronize()
    assert d_cnt.cpu().numpy().tolist() == [want.size, 0] and want.size < (1 << 20)
    h = d_text.cpu().numpy()
    assert np.array_equal(h[: want.size], want) and (h[foot:] == BYTE).all()
    rt = d_rt.cpu().numpy()
    assert np.array_equal(rt[:n_rec], rec_text) and (rt[n_rec:] == CANARY).all()


@gpu
def test_gpu_records_across_launch_seams(launch_tiles):
    """the lab build cut into launches of 64 / 128 tiles: a header, a name and a record end across every launch seam of the write
    pass, the size pass in several launches too; the launches counted in a captured graph"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(launch_tiles)
    per_launch = launch_tiles * T
    lens, name_lens, at = [], [], 0
    for seam in range(1, 4):  # a record whose header begins 20 bytes in front of each seam
        fill = seam * per_launch - 20 - at
        body = fill - 2 - 7  # a 7-byte name
        bases = body - -(-body // 61)
        lens.append(bases)
        name_lens.append(7)
        at += 2 + 7 + bases + -(-bases // 60)
        lens.append(30)
        name_lens.append(45)  # the name lies across the seam
        at += 2 + 45 + 31
    n_small = launch_tiles * BLOCK + 10  # and enough empty records for several launches of the size pass
    case = make_case(rng, lens + [0] * n_small, name_lens + [0] * n_small, 0, 60)
    total, _ = check_dev(case, tag=(launch_tiles,))
    rt = np_write(*case)[1].tolist()
    assert [rt[2 * k + 1] // per_launch != (rt[2 * k + 1] + 47) // per_launch for k in range(3)] == [True] * 3
    n, R = len(case[0]), len(case[1])
    foot = bound(n, R, len(case[2]), 60)
    tiles, launches = write_plan(foot, R, 0, launch_tiles)
    assert tiles > 3 * launch_tiles and launches >= 2 * 2 + 1 + 4
    d_bits = torch.from_numpy(case_words(case[0]).view(np.int64)).cuda()
    d_rs, d_no = (torch.from_numpy(np.asarray(x, dtype=np.int64)).cuda() for x in (case[1], case[3]))
    d_names = torch.from_numpy(np.frombuffer(case[2], dtype=np.uint8).copy()).cuda()
    text, cnt = torch.empty(foot, dtype=torch.uint8, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
    work = torch.empty(po.bits_to_fasta_work_bytes(R), dtype=torch.uint8, device="cuda")
    assert _kernel_nodes_of(torch, lambda: po.bits_to_fasta_dev(d_bits, n, text, cnt, work, rec_start=d_rs, names=d_names, name_off=d_no, width=60)) == launches


@gpu
def test_gpu_malformed_tables(L):
    """the counts are set, the canaries and every byte of text and rec_text are untouched, the host tier returns CNT_EINVAL"""
    rng = np.random.default_rng(88)
    for length, rec_start, names_len, name_off, count in MALFORMED:
        case = (random_letters(rng, length), rec_start, (b"n" * names_len if name_off is not None else None), name_off, 4)
        assert check_dev(case) == (0, count)
        assert check_host(L, case) == (0, count) and check_host(L, case, pinned=True) == (0, count)
    # tables that would send a kernel far outside: huge starts, huge name offsets, a descent late in a long table
    huge = (1 << 64) - 1
    for rec_start, name_off in (([0, huge], None), ([huge, huge], None), ([huge, 0], None), ([0, 10], [0, huge, 5]), ([0, 10], [huge, huge, huge]),
                                ([0, 10], [0, 1 << 40, 1 << 41])):
        case = (random_letters(rng, 100), rec_start, b"n" * 20 if name_off is not None else None, name_off, 60)
        assert check_dev(case)[1] > 0 and check_host(L, case)[1] > 0
    starts = np.sort(rng.integers(0, 5000, 3 * BLOCK)).tolist()
    starts[2 * BLOCK + 5] = starts[2 * BLOCK + 6] + 1
    assert check_dev((random_letters(rng, 5000), starts, None, None, 60), text_phase=5) == (0, 1)


@gpu
def test_gpu_64_bit_offsets():
    """len = 2^32 + 4096 in a lead of 2^32 - 7 bases and one record, width 60, a text of about 4.07 GiB: windows at the start,
    around the header and at the end against the closed form, counts and rec_text exactly"""
    import torch

    from conftest import need_free_hbm
    from cute_nucleotides_amd import packed_ops as po

    need_free_hbm(8)
    n, start, width, name = (1 << 32) + 4096, (1 << 32) - 7, 60, b"chr2 a second record"
    d_bits = torch.randint(-(1 << 62), 1 << 62, (n // 32,), dtype=torch.int64, device="cuda")
    d_bits *= 3  # the top codes too
    lead_bytes = start + -(-start // width)
    rest = n - start
    total = lead_bytes + 2 + len(name) + rest + -(-rest // width)
    foot = bound(n, 1, len(name), width)
    assert total > 4 * (1 << 30) and foot >= total
    d_text = torch.full((foot + GUARD,), BYTE, dtype=torch.uint8, device="cuda")
    d_rs = torch.tensor([start], dtype=torch.int64, device="cuda")
    d_no = torch.tensor([0, len(name)], dtype=torch.int64, device="cuda")
    d_names = torch.from_numpy(np.frombuffer(name, dtype=np.uint8).copy()).cuda()
    d_rt = torch.full((2,), CANARY, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((2,), CANARY, dtype=torch.int64, device="cuda")
    d_work = torch.empty(po.bits_to_fasta_work_bytes(1), dtype=torch.uint8, device="cuda")
    po.bits_to_fasta_dev(d_bits, n, d_text[:foot], d_cnt, d_work, rec_start=d_rs, names=d_names, name_off=d_no, width=width, rec_text=d_rt[:1])
    torch.cuda.synchronize()
    assert d_cnt.cpu().numpy().tolist() == [total, 0] and d_rt.cpu().numpy().tolist() == [lead_bytes, CANARY]
    assert bool((d_text[total:] == BYTE).all())

    def body_window(a, l, j0, j1):
        """bytes [j0, j1) of body(a, a + l) in closed form, the codes fetched from the device"""
        j = np.arange(j0, j1, dtype=np.int64)
        col, line = j % (width + 1), j // (width + 1)
        base = line * width + col
        feed = (col == width) | (base >= l)
        g = a + np.minimum(base, l - 1)
        w0 = int(g.min()) // 32
        words = d_bits[w0 : int(g.max()) // 32 + 1].cpu().numpy().view(np.uint64)
        codes = (words[g // 32 - w0] >> (np.uint64(2) * (g % 32).astype(np.uint64))) & np.uint64(3)
        return np.where(feed, np.uint8(NL), ACTG[codes.astype(np.int64)]).astype(np.uint8)

    span = 3 * T + 11
    assert np.array_equal(d_text[:span].cpu().numpy(), body_window(0, start, 0, span))
    head = lead_bytes + 2 + len(name)
    body_bytes = rest + -(-rest // width)  # the record is the text's end: 4103 bases behind the header
    assert head + body_bytes == total
    around = np.r_[body_window(0, start, lead_bytes - span, lead_bytes), np.frombuffer(b">" + name + b"\n", dtype=np.uint8),
                   body_window(start, rest, 0, body_bytes)]
    assert np.array_equal(d_text[lead_bytes - span : total].cpu().numpy(), around)
    # a window in the lead past byte 2^32 of the text
    j0 = (1 << 32) + 12345
    assert np.array_equal(d_text[j0 : j0 + span].cpu().numpy(), body_window(0, start, j0, j0 + span))


@gpu
@pytest.mark.parametrize("width", [0, 60])
def test_gpu_round_trip_on_the_device(width):
    """bits_to_fasta_dev then fasta_to_bits_dev gives back the words, n, rec_start, and a rec_text equal to the writer's"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(89 + width)
    R = 300
    case = make_case(rng, [int(x) for x in rng.choice([0, 1, 59, 60, 61, 150, 2000, 3 * T], R)], [int(x) for x in rng.integers(0, 50, R)], 123, width)
    letters, rec_start, names, name_off, _ = case
    n = len(letters)
    words = case_words(letters)
    d_bits = torch.from_numpy(words.view(np.int64)).cuda()
    d_rs, d_no = (torch.from_numpy(np.asarray(x, dtype=np.int64)).cuda() for x in (rec_start, name_off))
    d_names = torch.from_numpy(np.frombuffer(names, dtype=np.uint8).copy()).cuda()
    foot = bound(n, R, len(names), width)
    text, rt, cnt = torch.empty(foot, dtype=torch.uint8, device="cuda"), torch.empty(R, dtype=torch.int64, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
    work = torch.empty(po.bits_to_fasta_work_bytes(R), dtype=torch.uint8, device="cuda")
    po.bits_to_fasta_dev(d_bits, n, text, cnt, work, rec_start=d_rs, names=d_names, name_off=d_no, width=width, rec_text=rt)
    total, bad = cnt.cpu().numpy().tolist()
    assert bad == 0 and total == np_write(*case)[0].size
    back = torch.full((words_for(total),), CANARY, dtype=torch.int64, device="cuda")
    rt2, rs2 = torch.empty(R + 5, dtype=torch.int64, device="cuda"), torch.empty(R + 5, dtype=torch.int64, device="cuda")
    cnt2 = torch.empty(3, dtype=torch.int64, device="cuda")
    work2 = torch.empty(po.fasta_to_bits_work_bytes(total), dtype=torch.uint8, device="cuda")
    po.fasta_to_bits_dev(text[:total], back, cnt2, work2, rec_text=rt2, rec_start=rs2)
    assert cnt2.cpu().numpy().tolist() == [n, R, 0]
    assert torch.equal(back[: words_for(n)], d_bits) and torch.equal(rs2[:R], d_rs) and torch.equal(rt2[:R], rt)
    assert po.fasta_names(text[:total].cpu().numpy(), rt.cpu().numpy().view(np.uint64)) == [names[name_off[r] : name_off[r + 1]] for r in range(R)]


@gpu
def test_gpu_composition_with_extract():
    """cnt_extract windows written as records: the rows of 96 bases it leaves back to back are a packed sequence whose record r
    begins at 96 r"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(90)
    n, k, R = 20000, 96, 40
    letters = random_letters(rng, n)
    d_bits = torch.from_numpy(case_words(letters).view(np.int64)).cuda()
    pos = np.sort(rng.integers(0, n - k, R))
    rows, rejected = po.extract_dev(d_bits, n, torch.from_numpy(pos.astype(np.int64)).cuda(), k)
    assert int(rejected.item()) == 0
    names = [b"win@%d" % p for p in pos]
    d_rs = torch.arange(R, dtype=torch.int64, device="cuda") * k
    d_no = torch.from_numpy(np.cumsum([0] + [len(x) for x in names]).astype(np.int64)).cuda()
    d_names = torch.from_numpy(np.frombuffer(b"".join(names), dtype=np.uint8).copy()).cuda()
    foot = bound(R * k, R, d_names.numel(), 60)
    text, cnt = torch.empty(foot, dtype=torch.uint8, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
    work = torch.empty(po.bits_to_fasta_work_bytes(R), dtype=torch.uint8, device="cuda")
    po.bits_to_fasta_dev(rows.reshape(-1), R * k, text, cnt, work, rec_start=d_rs, names=d_names, name_off=d_no, width=60)
    total = int(cnt[0].item())
    want = b"".join(b">" + nm + b"\n" + letters[int(p) : int(p) + 60] + b"\n" + letters[int(p) + 60 : int(p) + k] + b"\n" for nm, p in zip(names, pos))
    assert text[:total].cpu().numpy().tobytes() == want and cnt[1].item() == 0


@gpu
def test_gpu_write_in_a_captured_graph_and_behind_a_side_stream():
    """one torch.cuda.graph capture of the call replayed twice on changed words and tables; then the call enqueued on a side stream
    behind the copy that makes its input, no host sync in between"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(91)
    R, n = 50, 9 * T
    bits = torch.zeros(words_for(n), dtype=torch.int64, device="cuda")
    rs, no = torch.zeros(R, dtype=torch.int64, device="cuda"), torch.zeros(R + 1, dtype=torch.int64, device="cuda")
    names = torch.zeros(R * 10, dtype=torch.uint8, device="cuda")
    foot = bound(n, R, R * 10, 60)
    text, rt, cnt = torch.empty(foot, dtype=torch.uint8, device="cuda"), torch.empty(R, dtype=torch.int64, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
    work = torch.empty(po.bits_to_fasta_work_bytes(R), dtype=torch.uint8, device="cuda")

    def call():
        po.bits_to_fasta_dev(bits, n, text, cnt, work, rec_start=rs, names=names, name_off=no, width=60, rec_text=rt)

    def make():
        cuts = np.sort(rng.integers(0, n, R))
        return random_letters(rng, n), cuts.tolist(), random_letters(rng, R * 10), (np.arange(R + 1) * 10).tolist(), 60

    def load(case, non_blocking=False):
        for dst, src in ((bits, case_words(case[0]).view(np.int64)), (rs, np.asarray(case[1], dtype=np.int64)), (no, np.asarray(case[3], dtype=np.int64)),
                         (names, np.frombuffer(case[2], dtype=np.uint8).copy())):
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
def test_gpu_host_tier_pinned_and_pageable(L):
    """pinned host buffers (used in place) and pageable ones (staged); then the Python wrapper on the real library, and its text
    read back by fasta_to_bits_hip"""
    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(92)
    cases = (make_case(rng, [3 * T + 77, 0, 1000], [2, 0, 41], 61, 60), make_case(rng, [], None, 2 * T + 5, 0), make_case(rng, [0, 0], None, 0, 60),
             make_case(rng, [150] * 100, [40] * 100, 0, 0))
    for case in cases:
        total = len(def_write(*case)[0])
        for pinned in (False, True):
            for cap in (None, total, total - 1):
                for with_rec_text in (True, False):
                    check_host(L, case, text_cap=cap, with_rec_text=with_rec_text, pinned=pinned)
    letters, rec_start, names, name_off, width = cases[0]
    name_list = [names[name_off[r] : name_off[r + 1]] for r in range(3)]
    text, rec_text = po.bits_to_fasta_hip(case_words(letters), len(letters), np.asarray(rec_start, dtype=np.uint64), name_list, width)
    want = def_write(*cases[0])
    assert text.tobytes() == want[0] and rec_text.tolist() == want[1]
    words, n, rt, rs, invalid = po.fasta_to_bits_hip(text)
    assert n == len(letters) and invalid == 0 and np.array_equal(words, case_words(letters)) and rs.tolist() == rec_start and np.array_equal(rt, rec_text)
    assert po.fasta_names(text, rt) == name_list
    assert po.bits_to_fasta_hip(case_words(letters), len(letters), width=0)[0].tobytes() == letters + b"\n"
    with pytest.raises(Exception):
        po.bits_to_fasta_hip(case_words(letters), len(letters), np.array([5, 3], dtype=np.uint64))


@gpu
def test_gpu_fuzz(L):
    """300 random shapes against the numpy reference: random widths, record and name lengths up to several tiles, capacities, phases"""
    rng = np.random.default_rng(93)
    for k in range(300):
        width = int(rng.choice(SEAM_WIDTHS + (3, 7, 1000, 1 << 33)))
        n_rec = int(rng.choice([0, 1, 2, 5, 40, 300]))
        most = int(rng.choice([3, 70, 500, 3 * T])) if n_rec <= 40 else int(rng.choice([3, 70, 200]))
        lens = [int(x) for x in rng.integers(0, most + 1, n_rec)]
        name_lens = [int(x) for x in rng.integers(0, int(rng.choice([1, 30, T + 50])) + 1, n_rec)] if rng.random() < 0.7 and n_rec <= 40 else ([0] * n_rec if rng.random() < 0.5 else None)
        case = make_case(rng, lens, name_lens, int(rng.choice([0, 1, 31, 32, int(rng.integers(0, 2 * T))])), width)
        total = len(def_write(*case)[0])
        cap = [None, None, total, max(total - 1, 0), int(rng.integers(0, total + 1))][int(rng.integers(0, 5))]
        check_dev(case, text_cap=cap, text_phase=int(rng.integers(0, 16)), names_phase=int(rng.integers(0, 8)), with_rec_text=bool(rng.integers(0, 4)), tag=(k,))
        if k % 10 == 0:
            check_host(L, case, text_cap=cap, pinned=k % 20 == 0, tag=(k,))
