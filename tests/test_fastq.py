"""FASTQ text straight to packed words, with the quality bytes and a record table (include/cute_nt.h "text formats: FASTQ",
hip/fastq_kernels.hpp, hip/fastq_abi.inc): a byte's role is its line number mod 4 (name, sequence, separator, quality), line feeds
and carriage returns are dropped, the sequence bytes are encoded as the encoder encodes them, the quality bytes are copied, and
each name line is reported with its byte offset and the positions of its first base and first quality.  Not in the reference: the
definition is restated here three ways -- byte by byte, bytes.split(b"\\n") line by line, and vectorised in numpy -- and the three
are pinned against each other before the library is compared with the last one.

CPU part: the references, the properties of the definition, every argument rule of both tiers and the query in the order the
header states them, an aliasing sweep of every (written, other) pair, the wiring, the launch plan in the sources, the header's
comment and the Python layer without a device.  GPU part: both tiers word for word, byte for byte and entry for entry against the
numpy reference, with canaries around every footprint."""
import collections
import ctypes
import os
import re
import types

import numpy as np
import pytest

from cute_nucleotides_amd.packed_ops import Fastq  # the Python layer's result: its fields are what the references below restate

from test_aliasing import OVERLAPS, TOUCHES, Arena, Buf, Call, pairs, place, shared_bytes
from test_fasta import LUT, columns, np_fasta, np_invalid, np_words, random_text, words_for  # noqa: F401
from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 8192  # bytes per workgroup tile (hip/fasta_kernels.hpp kFastaTile)
LANE, WAVE = 32, 64 * 32  # bytes per lane and per wave of a tile
ROUND = 1024 * 16  # tiles one round of each one-workgroup scan takes: kFastqScanBlock lanes, kCountedGroup tiles each
CNT_STRICT_LUT, CNT_ALLOW_N, CNT_TAIL_LUT = 1, 2, 4
NL, CR, AT, PLUS = 0x0A, 0x0D, 0x40, 0x2B
ALPHABET = b"ACGTN@+I#\n\n\n\r "  # a triple weight on the line feed

Ref = collections.namedtuple("Ref", "seq qual rec_text rec_start rec_qual malformed")


# ---- the three references -----------------------------------------------------------------------------------------------------
def def_fastq(text):
    """the definition, byte by byte"""
    seq, qual, rt, rs, rq, malformed, line = bytearray(), bytearray(), [], [], [], 0, 0
    for p, b in enumerate(text):
        role = line % 4
        if p == 0 or text[p - 1] == NL:
            if role == 0:
                rt.append(p)
                rs.append(len(seq))
                rq.append(len(qual))
                malformed += b != AT
            if role == 2:
                malformed += b != PLUS
        if b != NL and b != CR:
            if role == 1:
                seq.append(b)
            if role == 3:
                qual.append(b)
        line += b == NL
    return Ref(bytes(seq), bytes(qual), rt, rs, rq, malformed)


def lines_fastq(text):
    """line by line: the pieces between line feeds, a trailing empty piece dropped (a final line feed opens no line)"""
    seq, qual, rt, rs, rq, malformed, at = bytearray(), bytearray(), [], [], [], 0, 0
    pieces = bytes(text).split(b"\n")
    if pieces[-1] == b"":
        pieces.pop()
    for k, line in enumerate(pieces):
        if k % 4 == 0:
            rt.append(at)
            rs.append(len(seq))
            rq.append(len(qual))
            malformed += not line.startswith(b"@")
        elif k % 4 == 1:
            seq += line.replace(b"\r", b"")
        elif k % 4 == 2:
            malformed += not line.startswith(b"+")
        else:
            qual += line.replace(b"\r", b"")
        at += len(line) + 1
    return Ref(bytes(seq), bytes(qual), rt, rs, rq, malformed)


def np_masks(text):
    """(t, role, line_start, sequence mask, quality mask) of a non-empty text"""
    t = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    nl = t == NL
    role = (np.cumsum(nl) - nl) & 3
    line_start = np.r_[True, nl[:-1]]
    drop = nl | (t == CR)
    return t, role, line_start, (role == 1) & ~drop, (role == 3) & ~drop


def np_fastq(text):
    """vectorised: sequence and quality bytes as uint8, the record arrays as uint64"""
    if len(text) == 0:
        z = np.zeros(0, dtype=np.uint64)
        return Ref(np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), z, z, z, 0)
    t, role, line_start, sm, qm = np_masks(text)
    h = np.flatnonzero(line_start & (role == 0))
    malformed = int((line_start & (role == 0) & (t != AT)).sum() + (line_start & (role == 2) & (t != PLUS)).sum())
    return Ref(t[sm], t[qm], h.astype(np.uint64), (np.cumsum(sm) - sm)[h].astype(np.uint64), (np.cumsum(qm) - qm)[h].astype(np.uint64), malformed)


def fq_record(rng, read_len, eol=b"\n", name_len=None, letters=b"ACGT"):
    name = b"@" + random_text(rng, int(rng.integers(0, 9)) if name_len is None else name_len - 1, b"abc @+1")
    return name + eol + random_text(rng, read_len, letters) + eol + b"+" + eol + random_text(rng, read_len, b"I#@+5F") + eol


def well_formed(rng, n_records, lo=1, hi=26, eol=b"\n", letters=b"ACGT"):
    return b"".join(fq_record(rng, int(rng.integers(lo, hi)), eol, letters=letters) for _ in range(n_records))


def small_fastq(rng, n):
    """n bytes of FASTQ-like text: mostly whole records of short lines, now and then a carriage return, a blank line, a missing
    line or an N"""
    parts, size = [], 0
    while size < n:
        r = rng.random()
        if r < 0.8:
            p = fq_record(rng, int(rng.integers(1, 26)), b"\r\n" if rng.random() < 0.3 else b"\n", letters=b"ACGTACGTacgtN")
        elif r < 0.9:
            p = b"\n"
        else:
            p = random_text(rng, int(rng.integers(1, 20)), b"ACGT@+I") + b"\n"
        parts.append(p)
        size += len(p)
    return b"".join(parts)[:n]


HAND = [b"@", b"\n", b"@\n", b"\n@", b"@r\nA\n+\nI", b"@r\nA\n+\nI\n", b"\r\n", b"A\r\r\nC", b"@r\nA\n+\n@\n@s\nC\n+\n+\n", b"\n\n\n\n\n", b"@a\nAC\n\nII\n"]


def sample_texts():
    rng = np.random.default_rng(141)
    texts = [random_text(rng, n, ALPHABET) for n in range(60)] + [small_fastq(rng, n) for n in range(60)]
    texts += [random_text(rng, int(rng.integers(1, 400)), ALPHABET) for _ in range(720)]
    texts += [small_fastq(rng, int(rng.integers(1, 600))) for _ in range(400)]
    return texts + HAND


def same(d, v):
    return (d.seq == v.seq.tobytes() and d.qual == v.qual.tobytes() and d.rec_text == v.rec_text.tolist() and d.rec_start == v.rec_start.tolist()
            and d.rec_qual == v.rec_qual.tolist() and d.malformed == v.malformed)


def test_three_references_agree():
    texts = sample_texts()
    assert len(texts) >= 1250 and {len(t) for t in texts} >= set(range(60))
    for t in texts:
        d, l, v = def_fastq(t), lines_fastq(t), np_fastq(t)
        assert d == l and same(d, v), t
    assert sum(len(def_fastq(t).rec_text) for t in texts) > 2000
    assert def_fastq(b"@r\nA\n+\nI") == def_fastq(b"@r\nA\n+\nI\n") == Ref(b"A", b"I", [0], [0], [0], 0)
    assert def_fastq(b"\n") == Ref(b"", b"", [0], [0], [0], 1) and def_fastq(b"\n@") == Ref(b"@", b"", [0], [0], [0], 1)
    assert def_fastq(b"A\r\r\nC") == Ref(b"C", b"", [0], [0], [0], 1) and def_fastq(b"@r\nA\n+\n@\n@s\nC\n+\n+\n").malformed == 0


def test_properties():
    rng = np.random.default_rng(143)
    for t in sample_texts():
        r = np_fastq(t)
        n, Q = r.seq.size, r.qual.size
        for a in (r.rec_text, r.rec_start, r.rec_qual):
            assert (np.diff(a.astype(np.int64)) >= 0).all()
        assert (np.diff(r.rec_text.astype(np.int64)) > 0).all() and (r.rec_start <= n).all() and (r.rec_qual <= Q).all() and n + Q <= len(t)
        for h in r.rec_text.tolist():  # a line start whose line number is 0 mod 4
            assert (h == 0 or t[h - 1] == NL) and t[:h].count(b"\n") % 4 == 0
        assert r.rec_text.size == -(-len(bytes(t).split(b"\n")[: -1 if bytes(t).endswith(b"\n") or not t else None]) // 4)
        unix = t.replace(b"\r", b"")
        a, b = np_fastq(unix), np_fastq(unix.replace(b"\n", b"\r\n"))
        assert a.seq.tobytes() == b.seq.tobytes() and a.qual.tobytes() == b.qual.tobytes() and a.malformed == b.malformed
        assert np.array_equal(a.rec_start, b.rec_start) and np.array_equal(a.rec_qual, b.rec_qual) and a.rec_text.size == b.rec_text.size
    for eol in (b"\n", b"\r\n"):
        for _ in range(40):
            t = well_formed(rng, int(rng.integers(1, 30)), eol=eol)
            r = np_fastq(t)
            assert r.malformed == 0 and np.array_equal(r.rec_qual, r.rec_start) and r.qual.size == r.seq.size > 0
            # one line feed less: the roles behind it shift, and the file no longer looks like FASTQ
            feeds = [p for p in range(len(t) - 1) if t[p] == NL]
            p = feeds[int(rng.integers(0, len(feeds)))]
            cut = np_fastq(t[:p] + t[p + 1 :])
            assert cut.malformed > 0 or cut.qual.size != cut.seq.size or not np.array_equal(cut.rec_qual, cut.rec_start)
            assert cut.rec_text.size <= r.rec_text.size
            if len(feeds) - feeds.index(p) > 8:
                assert cut.malformed > 0


def test_fasta_cross_check():
    """a well-formed FASTQ rewritten as FASTA text gives the same kept bytes and rec_start through test_fasta's np_fasta"""
    rng = np.random.default_rng(144)
    for _ in range(60):
        t = well_formed(rng, int(rng.integers(1, 40)), eol=b"\r\n" if rng.random() < 0.3 else b"\n")
        lines = t.split(b"\n")[:-1]
        fasta = b"".join(b">" + lines[k][1:] + b"\n" + lines[k + 1] + b"\n" for k in range(0, len(lines), 4))
        r, (kept, _, rec_start) = np_fastq(t), np_fasta(fasta)
        assert kept.tobytes() == r.seq.tobytes() and np.array_equal(rec_start, r.rec_start)


# ---- CPU: the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


FILL = 0x5A
U64P = ctypes.POINTER(ctypes.c_uint64)


def test_argument_checks_in_the_stated_order(L):
    """every check of the header's list, each with all EARLIER checks passing and, where it can, a LATER one failing too; canaries
    (the fill) around every buffer: a refused call writes nothing"""
    from cute_nucleotides_amd import _lib

    OK, EINVAL = _lib.CNT_OK, _lib.CNT_EINVAL
    vp = ctypes.c_void_p
    arena = np.full(1 << 16, FILL, dtype=np.uint8)
    base = arena.ctypes.data + (-arena.ctypes.data % 128)
    at = lambda k: vp(base + 4096 * k)  # noqa: E731 -- buffer k of a call, each in a 4-KiB slot of its own
    n_len = 1000
    need = ctypes.c_size_t(0)
    # 1. the query: a NULL bytes; the answer is 0 without a byte, grows with the text, and does not depend on any address
    assert L.cnt_fastq_to_bits_work_bytes(n_len, None) == EINVAL and L.cnt_fastq_to_bits_work_bytes(0, None) == EINVAL
    assert L.cnt_fastq_to_bits_work_bytes(0, ctypes.byref(need)) == OK and need.value == 0
    sizes = []
    for n in (1, TILE - 15, TILE - 14, TILE, 16 * TILE, 16 * TILE + 1, 1 << 30, 1 << 36):
        assert L.cnt_fastq_to_bits_work_bytes(n, ctypes.byref(need)) == OK
        sizes.append(need.value)
    assert sizes == sorted(sizes) and sizes[0] >= 16 * (4 * 3 + 9) and sizes[1] == sizes[0] and sizes[4] > sizes[3] and sizes[-1] < (1 << 36) // 256
    assert L.cnt_fastq_to_bits_work_bytes(n_len, ctypes.byref(need)) == OK
    need = need.value

    def dev(text=at(0), n=n_len, flags=0, out=at(1), out_cap=n_len, qual=at(2), qual_cap=n_len, rt=at(3), rs=at(4), rq=at(5), rec_cap=50, counts=at(6), work=at(7),
            work_bytes=need):
        return L.cnt_fastq_to_bits_dev(text, n, flags, out, out_cap, qual, qual_cap, rt, rs, rq, rec_cap, counts, work, work_bytes, None)

    def host(text=at(0), n=n_len, flags=0, out=at(1), out_cap=n_len, qual=at(2), qual_cap=n_len, rt=at(3), rs=at(4), rq=at(5), rec_cap=50, counts=at(6)):
        c = lambda p: ctypes.cast(p, U64P)  # noqa: E731
        return L.cnt_fastq_to_bits(text, n, flags, c(out), out_cap, qual, qual_cap, c(rt), c(rs), c(rq), rec_cap, c(counts))

    def untouched():
        return bool((arena == FILL).all())

    for call in (dev, host):
        # 1. an unknown flag, before everything: at length 0, with NULL pointers
        for flags in (CNT_TAIL_LUT, 8, 0x10, 0x80000000, CNT_STRICT_LUT | CNT_TAIL_LUT):
            assert call(flags=flags) == EINVAL and call(flags=flags, n=0) == EINVAL and call(flags=flags, text=None, out=None, counts=None) == EINVAL
        # 2. nothing to compute: CNT_OK whatever the pointers are (a host count is zeroed, a device one needs a device)
        assert call(n=0, text=None, out=None, rt=None, rs=at(4), counts=None) == OK and untouched()
        # 3. a NULL text, out or counts -- in front of 4 (a misaligned record array), 5 and 6
        for null in ("text", "out", "counts"):
            assert call(**{null: None}) == EINVAL and call(**{null: None}, rt=vp(at(3).value + 4)) == EINVAL and call(**{null: None}, rs=None) == EINVAL
        # 4. alignment of out, counts and the record arrays; the text and qual may sit anywhere -- in front of 5 and 6
        for name, slot in (("out", 1), ("counts", 6), ("rt", 3), ("rs", 4), ("rq", 5)):
            for off in (1, 4, 7):
                assert call(**{name: vp(at(slot).value + off)}) == EINVAL
        assert call(out=vp(at(1).value + 4), rs=None) == EINVAL and call(rq=vp(at(5).value + 4), out=at(0)) == EINVAL
        # 5. some but not all of the record arrays -- in front of 6
        for gone in (("rt",), ("rs",), ("rq",), ("rt", "rs"), ("rs", "rq"), ("rt", "rq")):
            assert call(**{g: None for g in gone}) == EINVAL and call(**{g: None for g in gone}, out=at(0)) == EINVAL
        # 6. overlaps, at the stated extents: the footprint of out, min(text_len, qual_cap) bytes, min(text_len, rec_cap) entries,
        #    40 bytes of counts
        assert call(out=at(0)) == EINVAL and call(rt=at(4)) == EINVAL and call(rq=at(3)) == EINVAL and call(counts=vp(at(1).value + 8)) == EINVAL
        assert call(counts=vp(at(0).value + n_len - 8)) == EINVAL and call(rs=vp(at(3).value + 8 * 49)) == EINVAL
        assert call(counts=vp(at(4).value - 32)) == EINVAL  # the fifth count lies in rec_start
        assert call(qual=vp(at(0).value + n_len - 1)) == EINVAL and call(qual=vp(at(1).value - n_len + 1)) == EINVAL
        assert call(qual=vp(at(3).value - 50), qual_cap=51) == EINVAL and call(qual=vp(at(6).value + 39)) == EINVAL
        assert untouched()
    # 7. the device tier's scratch, after everything else
    assert dev(work=None) == EINVAL and dev(work_bytes=need - 1) == EINVAL and dev(work_bytes=0) == EINVAL
    for other in (0, 1, 2, 3, 4, 5, 6):
        assert dev(work=vp(at(other).value - need + 8)) == EINVAL  # the last 8 bytes of the query's answer reach into the buffer
    assert dev(work=None, out=at(0)) == EINVAL and untouched()
    # the host tier sets its counts at length 0, and only them
    c = np.full(7, 7, dtype=np.uint64)
    assert L.cnt_fastq_to_bits(None, 0, CNT_ALLOW_N, None, 5, None, 5, None, None, None, 5, ctypes.cast(vp(c.ctypes.data + 8), U64P)) == OK
    assert c.tolist() == [7, 0, 0, 0, 0, 0, 7]
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        assert host() == _lib.CNT_ENODEV and host(rt=None, rs=None, rq=None, rec_cap=1 << 40) == _lib.CNT_ENODEV and host(qual=None) == _lib.CNT_ENODEV
        assert host(out=at(0), out_cap=0) == _lib.CNT_ENODEV and host(qual=at(0), qual_cap=0) == _lib.CNT_ENODEV  # capacity 0: anywhere
        assert host(text=vp(at(0).value + 3), qual=vp(at(2).value + 5), rs=vp(at(3).value + 8 * 50)) == _lib.CNT_ENODEV  # touching arrays; any byte
        assert host(qual=vp(at(3).value - 50), qual_cap=50) == _lib.CNT_ENODEV  # qual ends where rec_text begins
        assert dev(work=vp(at(7).value + 4)) < 0  # a scratch at any address
        assert untouched()


def fastq_calls(L):
    """the two tiers as test_aliasing's table rows: every buffer with its extent, its alignment and whether it is written"""
    vp = ctypes.c_void_p
    up = lambda a: ctypes.cast(vp(a), U64P)  # noqa: E731
    n_len, out_cap, qual_cap, rec_cap = 1000, 200, 96, 24  # byte extents: multiples of 8, so that an 8-B aligned buffer can touch their end
    need = ctypes.c_size_t(0)
    assert L.cnt_fastq_to_bits_work_bytes(n_len, ctypes.byref(need)) == 0
    need = need.value
    bufs = [Buf("text", n_len, 1, False), Buf("out", words_for(out_cap) * 8, 8, True), Buf("qual", qual_cap, 1, True), Buf("rec_text", rec_cap * 8, 8, True),
            Buf("rec_start", rec_cap * 8, 8, True), Buf("rec_qual", rec_cap * 8, 8, True), Buf("counts", 40, 8, True)]
    dev = Call("cnt_fastq_to_bits_dev", bufs + [Buf("work", need, 8, True)],
               lambda p: L.cnt_fastq_to_bits_dev(vp(p["text"]), n_len, 0, vp(p["out"]), out_cap, vp(p["qual"]), qual_cap, vp(p["rec_text"]), vp(p["rec_start"]),
                                                 vp(p["rec_qual"]), rec_cap, vp(p["counts"]), vp(p["work"]), need + 64, None), frozenset())
    host = Call("cnt_fastq_to_bits", bufs,
                lambda p: L.cnt_fastq_to_bits(vp(p["text"]), n_len, 3, up(p["out"]), out_cap, vp(p["qual"]), qual_cap, up(p["rec_text"]), up(p["rec_start"]),
                                              up(p["rec_qual"]), rec_cap, up(p["counts"])), frozenset())
    return [dev, host]


def test_aliasing_sweep_of_every_written_buffer(L):
    """every (written, other) pair of both tiers: the five overlapping placements are CNT_EINVAL and write nothing, the two
    touching ones pass the argument checks"""
    from cute_nucleotides_amd import _lib

    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    arena = Arena()
    tried = 0
    for call in fastq_calls(L):
        assert len(pairs(call)) == (7 * 7 if call.name.endswith("_dev") else 6 * 6)
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
    assert tried >= 300


def test_abi_wiring(L):
    import subprocess

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib, packed_ops as po

    names = ("cnt_fastq_to_bits", "cnt_fastq_to_bits_dev", "cnt_fastq_to_bits_work_bytes")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    hpp = open(os.path.join(ROOT, "cute_nucleotides_amd", "cute_nucleotides.hpp")).read()
    for name in names:
        assert name in exported and ("int %s(" % name) in header and ("fn %s(" % name) in rust and (name + "(") in hpp and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["cnt_fastq_to_bits_dev"][1]) == 15 and len(_lib.SIGNATURES["cnt_fastq_to_bits"][1]) == 12
    assert "pub fn fastq_to_bits_hip(" in rust and "inline Fastq fastq_to_bits_hip(" in hpp and "pub fn fastq_to_bits_hip_dev(" in rust
    for name in ("fastq_to_bits_hip", "fastq_to_bits_dev", "fastq_to_bits_work_bytes", "fastq_names"):
        assert getattr(cn, name) is getattr(po, name) and name in cn.__all__
    assert "#define CNT_ABI_VERSION 1" in header  # symbols were only added: the version did not move


def test_header_comment_and_section_place():
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    title = "/* ---- text formats: FASTQ ----"
    assert header.count(title) == 1
    at = header.index(title)
    # behind the FASTA section, in front of the tuning knobs, outside the span tests/test_aliasing.py holds to its table
    assert header.index("/* ---- text formats: FASTA ----") < header.index("int cnt_fasta_to_bits(") < at < header.index("Kernel selection for A/B runs")
    assert not (header.index("---- packed-domain operations") < at < header.index("---- device utilities"))
    section = header[at : header.index("Kernel selection for A/B runs")]
    for k, name in enumerate(("CNT_FASTQ_N", "CNT_FASTQ_RECORDS", "CNT_FASTQ_INVALID", "CNT_FASTQ_QUAL", "CNT_FASTQ_MALFORMED")):
        assert re.search(r"#define %s +%d\b" % (name, k), section) and "counts[%s]" % name in section, name
    checks = ["1. an unknown flag", "2. text_len == 0", "3. a NULL text, out or counts", "4. an out, counts, rec_text, rec_start or rec_qual that is not 8-B aligned",
              "5. some but not all of the three record arrays", "6. a written buffer sharing a byte", "7. device tier: a NULL d_work"]
    places = [section.index(c) for c in checks]
    assert places == sorted(places)
    for word in ("wrapped over several lines", "5-letter variant", "quality binning or Phred decoding", "paired", "interleaved files", "gzip", "2^36", "40 bytes",
                 "enqueue-only", "capturable in a graph", "CNT_ECAP after the work", "strict", "k(p) mod 4", "any byte address"):
        assert word in section, word


TILES = "split_launches(n_tiles, kFastaBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(%s, dim3((unsigned)n), dim3(kFastaBlock), 0, s, a, t); });"


def test_fastq_plan_matches_the_launcher_source():
    src = open(os.path.join(ROOT, "hip", "fastq_kernels.hpp")).read()
    assert '#include "fasta_kernels.hpp"' in src and "constexpr int kFastqScanBlock = 1024;" in src and ROUND == 1024 * 16 and TILE == 32 * 256
    kernels = [line for line in src.splitlines() if line.startswith("__global__")]
    assert len(kernels) == 13 and sum("(kFastaBlock) void fastq_" in k for k in kernels) == 11 and sum("(kFastqScanBlock) void fastq_" in k for k in kernels) == 2
    assert not any(line.startswith("template") and "__global__" in line for line in src.splitlines())
    assert not re.search(r"template <[^>]*>\s*\n?__global__", src)  # plain kernels around templated bodies
    # no atomic to global memory but the merge of the shared words
    assert src.count("atomicOr(&s_out[") == 2 and src.count("atomicOr(") == 2 and src.count("hpc_merge(out + k, v)") == 1
    assert not re.search(r"atomic(Add|CAS|Max|Min|Exch|And|Xor|Inc)", src)
    assert "hpc_compress(w, fasta_spread(seq))" in src
    abi = open(os.path.join(ROOT, "hip", "fastq_abi.inc")).read()
    line_scan = "hipLaunchKernelGGL(fastq_line_scan, dim3(1), dim3(kFastqScanBlock), 0, s, a);"
    scan = "hipLaunchKernelGGL(fastq_scan, dim3(1), dim3(kFastqScanBlock), 0, s, a);"
    zero = "hipLaunchKernelGGL(hpc_zero_edges, dim3((unsigned)n), dim3(kHpcBlock), 0, s, h, t);"
    empty = "if (text_len == 0) return d_counts ? hip_rc(hipMemsetAsync(d_counts, 0, kFastqCounts, s)) : CNT_OK;"
    order = [abi.index(x) for x in (empty, TILES % "fastq_lines", line_scan, TILES % "count", scan, zero, TILES % "write")]
    assert order == sorted(order) and "constexpr size_t kFastqCounts = 5 * 8;" in abi
    assert abi.count("hipLaunchKernelGGL(") == 6 and abi.count("split_launches(") == 4 and abi.count("hipMalloc") == 0 and abi.count("Synchronize") == 0
    assert "host_call(b, kFastqCounts + work_bytes, got, 5, CNT_FASTQ_RECORDS, false," in abi
    assert "{qual, qcap, Dir::out}" in abi and abi.count("Dir::counted") == 3
    shim = open(os.path.join(ROOT, "hip", "cute_nt.hip")).read()
    assert shim.index('#include "fasta_abi.inc"') < shim.index('#include "fastq_abi.inc"')


def fastq_plan(text_len, phase=0, launch_tiles=((0x7FFFFFFF // 256) // 64) * 64):
    """(tiles, kernel launches) of a device call with capacities: three tile passes, two scans, the edge zeroing with a lane per tile"""
    tiles = -(-(text_len + phase) // TILE)
    return tiles, 3 * -(-tiles // launch_tiles) + 2 + -(-(-(-tiles // 256)) // launch_tiles)


# ---- CPU: the Python layer ------------------------------------------------------------------------------------------------------
def _fake_lib(calls):
    """a stand-in for the library whose cnt_fastq_to_bits is the numpy reference behind the C calling convention"""
    from cute_nucleotides_amd import _lib

    def arr(p, n, ct=ctypes.c_uint64, dt=np.uint64):
        return np.frombuffer((ct * n).from_address(p.value), dtype=dt) if n else np.zeros(0, dtype=dt)

    def cnt_fastq_to_bits(text, length, flags, out, out_cap, qual, qual_cap, rec_text, rec_start, rec_qual, rec_cap, counts):
        calls.append((out_cap, qual_cap if qual is not None else None, rec_cap, flags))
        t = arr(text, length, ctypes.c_uint8, np.uint8)
        r = np_fastq(t)
        m, q, k = min(r.seq.size, out_cap), min(r.qual.size, qual_cap), min(r.rec_text.size, rec_cap)
        if length:
            arr(out, words_for(m))[:] = np_words(r.seq[:m], flags & CNT_STRICT_LUT)
            if qual is not None:
                arr(qual, q, ctypes.c_uint8, np.uint8)[:] = r.qual[:q]
            for p, a in ((rec_text, r.rec_text), (rec_start, r.rec_start), (rec_qual, r.rec_qual)):
                arr(p, k)[:] = a[:k]
        for i, v in enumerate((r.seq.size, r.rec_text.size, np_invalid(r.seq, flags & CNT_ALLOW_N), r.qual.size, r.malformed)):
            counts[i] = v
        short = r.seq.size > out_cap or (qual is not None and r.qual.size > qual_cap) or r.rec_text.size > rec_cap
        return _lib.CNT_ECAP if short else _lib.CNT_OK

    return types.SimpleNamespace(cnt_fastq_to_bits=cnt_fastq_to_bits, cnt_words_for=words_for)


def test_fastq_to_bits_hip_retries_once_with_the_reported_count(monkeypatch):
    from cute_nucleotides_amd import packed_ops as po

    calls = []
    fake = _fake_lib(calls)
    monkeypatch.setattr(po, "lib", lambda: fake)
    rng = np.random.default_rng(145)
    few = small_fastq(rng, 30000)  # inside the first guess
    r = np_fastq(few)
    guess = len(few) // 256 + 1024
    assert 100 < r.rec_text.size < guess
    for text in (few, bytearray(few), np.frombuffer(few, dtype=np.uint8), memoryview(few)):
        del calls[:]
        got = po.fastq_to_bits_hip(text, allow_n=True)
        assert len(calls) == 1 and calls[0] == (len(few), len(few), guess, CNT_ALLOW_N)
        assert got.n == r.seq.size and np.array_equal(got.words, np_words(r.seq, False)) and np.array_equal(got.qual, r.qual) and got.qual.dtype == np.uint8
        assert np.array_equal(got.rec_text, r.rec_text) and np.array_equal(got.rec_start, r.rec_start) and np.array_equal(got.rec_qual, r.rec_qual)
        assert got.invalid == np_invalid(r.seq, True) and got.malformed == r.malformed and got.words.dtype == got.rec_text.dtype == got.rec_qual.dtype == np.uint64
        assert isinstance(got, Fastq) and Fastq._fields == ("words", "n", "qual", "rec_text", "rec_start", "rec_qual", "invalid", "malformed")
    many = b"@r\nA\n+\nI\n" * 3000  # more records than the guess: one retry at the reported number
    del calls[:]
    got = po.fastq_to_bits_hip(many, strict_lut=True, with_qual=False)
    assert [c[2] for c in calls] == [len(many) // 256 + 1024, 3000] and calls[1][3] == CNT_STRICT_LUT and calls[0][1] is None and got.qual is None
    assert got.n == 3000 and got.rec_text.tolist() == list(range(0, 27000, 9)) and got.rec_start.tolist() == got.rec_qual.tolist() == list(range(3000))
    assert got.invalid == 0 and got.malformed == 0 and np.array_equal(got.words, np_words(np.full(3000, 65, dtype=np.uint8), True))
    del calls[:]
    got = po.fastq_to_bits_hip(b"")
    assert (got.words.size, got.n, got.qual.size, got.rec_text.size, got.rec_start.size, got.rec_qual.size, got.invalid, got.malformed) == (0,) * 8
    # a second CNT_ECAP is an error, not a loop; so is any other status
    fake.cnt_fastq_to_bits = lambda *a: 2
    with pytest.raises(Exception):
        po.fastq_to_bits_hip(many)
    for bad in ("ACGT", 5, np.zeros(4, dtype=np.int32), [65, 67]):
        with pytest.raises(TypeError):
            po.fastq_to_bits_hip(bad)


def test_fastq_names():
    from cute_nucleotides_amd import packed_ops as po

    long_name = b"x" * 70000
    text = b"@one two\nAC\n+\nII\n@\r\n\r\n+\r\n\r\n@three@3\r\nGG\n+three\n@+\n@" + long_name + b"\nA\n+\nI\n@last"
    rt = np_fastq(text).rec_text
    want = [b"one two", b"", b"three@3", long_name, b"last"]
    assert np_fastq(text).malformed == 0 and po.fastq_names(text, rt) == want and po.fastq_names(bytearray(text), rt.tolist()) == want
    assert po.fastq_names(np.frombuffer(text, dtype=np.uint8), rt[1:3]) == want[1:3] and po.fastq_names(text, []) == []
    assert po.fastq_names(b"@only\r", [0]) == [b"only"] and po.fastq_names(b"@", [0]) == [b""]
    for bad in ([1], [len(text)], [9], [text.index(b"@3")]):
        with pytest.raises(ValueError):
            po.fastq_names(text, bad)
    rng = np.random.default_rng(146)
    for _ in range(50):
        t = well_formed(rng, 20, eol=b"\r\n" if rng.random() < 0.5 else b"\n")
        heads = [line[1:].rstrip(b"\r") for line in t.split(b"\n")[:-1][::4]]
        assert po.fastq_names(t, np_fastq(t).rec_text) == heads


def test_device_wrapper_argument_errors():
    torch = pytest.importorskip("torch")
    from cute_nucleotides_amd import packed_ops as po

    t = torch.zeros(10, dtype=torch.uint8)
    with pytest.raises(ValueError):
        po.fastq_to_bits_dev(t, t, t, t)  # not on a device


# ---------------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
CANARY = -0x3C3C3C3C3C3C3C3D
QCANARY = 0xC3
HOST_CANARY = 0xDEADBEEFDEADBEEF
PAD = 5  # canary words in front of and behind every footprint
QPAD = 40  # canary bytes around qual
POISON = (b"\n@", b"@@", b"@\n", b"\n\n")  # in front of and behind the text: a byte looked at there changes the result


def expect(text, flags, out_cap, qual_cap, rec_cap):
    """(the five counts, the words, quality bytes and record entries that must be written) at these capacities"""
    r = np_fastq(text)
    m, q, k = min(r.seq.size, out_cap), min(r.qual.size, qual_cap), min(r.rec_text.size, rec_cap)
    counts = [r.seq.size, r.rec_text.size, np_invalid(r.seq, flags & CNT_ALLOW_N), r.qual.size, r.malformed]
    return counts, np_words(r.seq[:m], flags & CNT_STRICT_LUT), r.qual[:q], (r.rec_text[:k], r.rec_start[:k], r.rec_qual[:k])


def check_dev(text, flags=0, out_cap=None, qual_cap=None, rec_cap=None, with_qual=True, with_rec=True, text_phase=0, qual_phase=0, out_phase=0, tag=()):
    """the device tier on the text: words, quality bytes, record table, counts, canaries around every footprint, the text unchanged"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    n_len = len(text)
    out_cap = n_len if out_cap is None else out_cap
    qual_cap = n_len if qual_cap is None else qual_cap
    rec_cap = n_len if rec_cap is None else rec_cap
    foot, qfoot, rfoot = min(n_len, out_cap), min(n_len, qual_cap), min(n_len, rec_cap)
    counts, want_out, want_qual, want_rec = expect(text, flags, out_cap, qual_cap, rec_cap)
    poison = POISON[(text_phase + n_len) % 4]
    front = (poison * 40)[-(64 + text_phase) :]  # the allocation is 256-B aligned: the text begins at byte phase text_phase of 16
    parent = np.frombuffer(front + bytes(text) + poison * 8, dtype=np.uint8)
    d_parent = torch.from_numpy(parent.copy()).cuda()
    d_text = d_parent[len(front) : len(front) + n_len]
    assert n_len == 0 or d_text.data_ptr() % 16 == text_phase % 16
    d_out = torch.full((PAD + out_phase + words_for(foot) + PAD,), CANARY, dtype=torch.int64, device="cuda")
    q0 = QPAD + qual_phase
    d_qual = torch.full((q0 + qfoot + QPAD,), QCANARY, dtype=torch.uint8, device="cuda")
    o0 = PAD + out_phase
    d_recs = [torch.full((o0 + rfoot + PAD,), CANARY, dtype=torch.int64, device="cuda") for _ in range(3)]
    d_cnt = torch.full((7,), CANARY, dtype=torch.int64, device="cuda")
    d_work = torch.full((po.fastq_to_bits_work_bytes(n_len) + 8,), 0x77, dtype=torch.uint8, device="cuda")
    rec = [d[o0 : o0 + rfoot] if with_rec else None for d in d_recs]
    po.fastq_to_bits_dev(d_text, d_out[o0 : o0 + words_for(foot)], d_cnt[1:6], d_work[4:],  # the scratch at a 4-B-misaligned address
                         qual=d_qual[q0 : q0 + qfoot] if with_qual else None, rec_text=rec[0], rec_start=rec[1], rec_qual=rec[2], out_cap=out_cap,
                         qual_cap=qual_cap if with_qual else None, rec_cap=rec_cap if with_rec else None, strict_lut=bool(flags & CNT_STRICT_LUT),
                         allow_n=bool(flags & CNT_ALLOW_N))
    torch.cuda.synchronize()
    tag = tag + (n_len, flags, out_cap, qual_cap, rec_cap, with_qual, with_rec, text_phase, qual_phase, out_phase)
    assert d_cnt.cpu().numpy().tolist() == [CANARY] + counts + [CANARY], tag + (counts,)
    assert np.array_equal(d_parent.cpu().numpy(), parent), tag + ("text",)
    h = d_out.cpu().numpy()
    assert (h[:o0] == CANARY).all() and (h[o0 + words_for(foot) :] == CANARY).all(), tag + ("out canary",)
    got = h[o0 : o0 + want_out.size].view(np.uint64)
    assert np.array_equal(got, want_out), tag + ("out", np.flatnonzero(got != want_out)[:4].tolist())
    h = d_qual.cpu().numpy()
    if with_qual:
        assert (h[:q0] == QCANARY).all() and (h[q0 + qfoot :] == QCANARY).all(), tag + ("qual canary",)
        got = h[q0 : q0 + want_qual.size]
        assert np.array_equal(got, want_qual), tag + ("qual", np.flatnonzero(got != want_qual)[:4].tolist())
    else:
        assert (h == QCANARY).all(), tag + ("qual",)
    for name, d, want in zip(("rec_text", "rec_start", "rec_qual"), d_recs, want_rec):
        h = d.cpu().numpy()
        if with_rec:
            assert (h[:o0] == CANARY).all() and (h[o0 + want.size :] == CANARY).all(), tag + (name, "canary")  # nothing past min(R, rec_cap)
            got = h[o0 : o0 + want.size].view(np.uint64)
            assert np.array_equal(got, want), tag + (name, np.flatnonzero(got != want)[:4].tolist())
        else:
            assert (h == CANARY).all(), tag + (name,)
    return tuple(counts)


def check_host(L, text, flags=0, out_cap=None, qual_cap=None, rec_cap=None, with_qual=True, with_rec=True, pinned=False, tag=()):
    """the host tier on the text, pageable or pinned buffers, the text and qual at odd bytes inside their allocations"""
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    n_len = len(text)
    out_cap = n_len if out_cap is None else out_cap
    qual_cap = n_len if qual_cap is None else qual_cap
    rec_cap = n_len if rec_cap is None else rec_cap
    foot, qfoot, rfoot = min(n_len, out_cap), min(n_len, qual_cap), min(n_len, rec_cap)
    counts, want_out, want_qual, want_rec = expect(text, flags, out_cap, qual_cap, rec_cap)
    alloc = (lambda k, dt=np.uint64: cn.pinned_empty(k, dt)) if pinned else (lambda k, dt=np.uint64: np.empty(k, dtype=dt))
    buf = alloc(n_len + 8, np.uint8)
    buf[:] = AT
    buf[3 : 3 + n_len] = np.frombuffer(bytes(text), dtype=np.uint8)
    out, cnt, qual = alloc(PAD + words_for(foot) + PAD), alloc(7), alloc(QPAD + 3 + qfoot + QPAD, np.uint8)
    recs = [alloc(PAD + rfoot + PAD) for _ in range(3)]
    for a in [out, cnt] + recs:
        a[:] = HOST_CANARY
    qual[:] = QCANARY
    q0 = QPAD + 3
    rc = L.cnt_fastq_to_bits(buf[3:].ctypes.data, n_len, flags, out[PAD:].ctypes.data, out_cap, qual[q0:].ctypes.data if with_qual else None, qual_cap,
                             *(r[PAD:].ctypes.data if with_rec else None for r in recs), rec_cap, cnt[1:].ctypes.data)
    tag = tag + (n_len, flags, out_cap, qual_cap, rec_cap, with_qual, with_rec, pinned)
    short = counts[0] > out_cap or (with_qual and counts[3] > qual_cap) or (with_rec and counts[1] > rec_cap)
    assert rc == (_lib.CNT_ECAP if short else _lib.CNT_OK), tag + (rc, counts)
    assert cnt.tolist() == [HOST_CANARY] + counts + [HOST_CANARY], tag + (cnt.tolist(), counts)
    assert (out[:PAD] == HOST_CANARY).all() and (out[PAD + words_for(foot) :] == HOST_CANARY).all(), tag + ("out canary",)
    assert np.array_equal(out[PAD : PAD + want_out.size], want_out), tag + ("out",)
    if with_qual:
        assert (qual[:q0] == QCANARY).all() and (qual[q0 + qfoot :] == QCANARY).all(), tag + ("qual canary",)
        assert np.array_equal(qual[q0 : q0 + want_qual.size], want_qual), tag + ("qual",)
    else:
        assert (qual == QCANARY).all(), tag + ("qual",)
    for name, a, want in zip(("rec_text", "rec_start", "rec_qual"), recs, want_rec):
        if with_rec:
            assert (a[:PAD] == HOST_CANARY).all() and (a[PAD + want.size :] == HOST_CANARY).all(), tag + (name, "canary")
            assert np.array_equal(a[PAD : PAD + want.size], want), tag + (name,)
        else:
            assert (a == HOST_CANARY).all(), tag + (name,)
    return tuple(counts)


@gpu
def test_gpu_small_lengths_both_tiers(L):
    """every text_len 0..300, alternating FASTQ-like and random texts, and a file of three records of 150 bases"""
    rng = np.random.default_rng(151)
    for n_len in range(301):
        text = small_fastq(rng, n_len) if n_len % 2 else random_text(rng, n_len, ALPHABET)
        check_dev(text, flags=n_len & 3, text_phase=n_len % 17, qual_phase=n_len % 5, out_phase=n_len & 1)
        check_host(L, text, flags=(n_len >> 1) & 3)
    for eol in (b"\n", b"\r\n"):
        text = b"".join(fq_record(rng, 150, eol, name_len=40) for _ in range(3))
        for phase in (0, 9):
            assert check_dev(text, text_phase=phase) == (450, 3, 0, 450, 0)
        assert check_host(L, text) == (450, 3, 0, 450, 0)


FILLS = (b"abc 12@+", b"ACGT", b"+xyz", b"I#5F@+")  # what a stretched or long line of each role is made of


def planted(rng, p, role, n_len, eol=b"\n", long_len=None):
    """a text of about n_len bytes of short well-formed records in which a line of `role` begins exactly at byte p: the line in
    front of it is stretched; with long_len that line itself holds long_len bytes without a line feed"""
    parts, pos = [], 0
    while pos < p - 600:
        parts.append(fq_record(rng, int(rng.integers(20, 80)), eol))
        pos += len(parts[-1])
    lines = [b"@n1", random_text(rng, 30, b"ACGT"), b"+", random_text(rng, 30, b"I#5F"), b"@n2", random_text(rng, 25, b"ACGT"), b"+", random_text(rng, 25, b"I#5F")]
    if p - pos < 200:  # next to the beginning of the text: the shortest lines
        lines[:4] = [b"@n", b"AC", b"+", b"II"]
    t = role if role else 4
    if long_len is not None:
        lines[t] = (b"@" if role == 0 else b"+" if role == 2 else b"") + random_text(rng, long_len, FILLS[role])
    lines = [x + eol for x in lines]
    grow = p - pos - sum(len(x) for x in lines[:t])
    assert grow >= 0
    lines[t - 1] = lines[t - 1][: -len(eol)] + random_text(rng, grow, FILLS[(t - 1) % 4]) + eol
    parts += lines
    pos += sum(len(x) for x in lines)
    while pos < n_len:
        parts.append(fq_record(rng, int(rng.integers(20, 80)), eol))
        pos += len(parts[-1])
    text = b"".join(parts)
    assert text[p - 1] == NL and text[:p].count(b"\n") % 4 == role
    return text


def _seam_cases(rng, phase):
    """(name, text): every seam of the definition at the tile, wave and lane edges, for a text that begins at byte `phase` of 16"""
    cases = []
    n_len = 3 * TILE + 501
    edges = (("tile", TILE), ("second tile", 2 * TILE), ("wave", TILE + WAVE), ("lane", TILE + 7 * LANE), ("first lane", LANE))
    for where, e in edges:
        for role in range(4):
            for delta in (-1, 0, 1):
                cases.append(("role %d begins %+d of a %s edge" % (role, delta, where), planted(rng, e - phase + delta, role, n_len)))
            cases.append(("carriage return | line feed in front of role %d at a %s edge" % (role, where), planted(rng, e - phase + 1, role, n_len, eol=b"\r\n")))
    for role in range(4):
        for k in (1, 2, 5):
            cases.append(("a role-%d line over %d whole tiles" % (role, k), planted(rng, TILE - 100 - phase, role, (k + 2) * TILE, long_len=k * TILE + 300)))
        cut = planted(rng, TILE + 40 - phase, role, TILE + 40)[: TILE + 40 - phase + 9]
        assert not cut.endswith(b"\n")
        cases.append(("a text that ends inside role %d" % role, cut))
    cases.append(("line feeds only", b"\n" * (TILE + 70)))
    cases.append(("no line feed at all", random_text(rng, 2 * TILE + 5, b"ACGT@+")))
    # a tile without a base between two tiles that share an output word, and the same for the quality stream
    first = b"@a\n" + random_text(rng, TILE - phase - 4, b"ACGT") + b"\n"  # tile 0 ends on the line feed
    cases.append(("a tile without a base", first + b"+\n" + random_text(rng, TILE - 3, b"I#") + b"\n" + well_formed(rng, 20, 20, 60)))
    first = b"@a\nAC\n+\n" + random_text(rng, TILE - phase - 9, b"I#5") + b"\n"
    cases.append(("a tile without a quality", first + b"@" + b"n" * (TILE - 2) + b"\n" + b"ACGT\n+\nIIII\n" + well_formed(rng, 20, 20, 60)))
    # 45 tiles that each hold 1..3 bases and as many qualities: a long name, then three short lines
    parts = [b"@a\n" + random_text(rng, TILE - phase - 4, b"ACGT") + b"\n+\n" + random_text(rng, TILE - 3, b"I#") + b"\n"]
    for tile in range(45):
        k = 1 + tile % 3
        parts.append(b"@" + b"h" * (TILE - 6 - 2 * k) + b"\n" + random_text(rng, k, b"ACGT") + b"\n+\n" + random_text(rng, k, b"I#5") + b"\n")
    cases.append(("45 tiles of 1..3 bases and qualities", b"".join(parts) + b"@e\nACGTAC\n+\nIIIIII"))
    return cases


def per_tile(mask, phase, tiles):
    return np.bincount((np.flatnonzero(mask) + phase) // TILE, minlength=tiles)[:tiles]


@gpu
@pytest.mark.parametrize("phase", [0, 5])
def test_gpu_seams(L, phase):
    rng = np.random.default_rng(152 + phase)
    for j, (name, text) in enumerate(_seam_cases(rng, phase)):
        counts = check_dev(text, text_phase=phase, qual_phase=j % 16, out_phase=j & 1, flags=j & 3, tag=(name,))
        if j % 4 == 0:
            check_dev(text, text_phase=phase, with_rec=False, with_qual=bool(j & 4), tag=(name,))
            check_host(L, text, tag=(name,))
        if name.startswith("a role") or name.startswith("role") or name.startswith("carriage"):
            assert counts[4] == 0 and counts[1] > 10, name
        if name.startswith("45 tiles"):
            _, _, _, sm, qm = np_masks(text)
            for m in (sm, qm):
                c = per_tile(m, phase, 47)
                assert ((c[2:47] >= 1) & (c[2:47] <= 3)).all() and counts[1] == 47 and counts[4] == 0
        if name.startswith("a tile without a base"):
            c = per_tile(np_masks(text)[3], phase, 3)
            assert c[0] % 32 != 0 and c[1] == 0 and c[2] > 0
        if name.startswith("a tile without a quality"):
            c = per_tile(np_masks(text)[4], phase, 3)
            assert c[0] > 0 and c[1] == 0 and c[2] > 0


@gpu
def test_gpu_pointer_phases():
    """d_text and d_qual at every byte phase 0..16, poison '@' and line feeds just in front of and behind the text (check_dev
    plants them at every call); d_out and the record arrays at 8-B phases"""
    rng = np.random.default_rng(153)
    texts = [well_formed(rng, 40, 100, 400) + fq_record(rng, 2 * TILE + 77) + well_formed(rng, 5, 100, 200, eol=b"\r\n"), well_formed(rng, 3, 10, 20),
             random_text(rng, TILE + 40, ALPHABET)]
    for text in texts:
        results = {check_dev(text, text_phase=phase, qual_phase=(phase * 7) % 17, out_phase=phase % 3, flags=phase & 1) for phase in range(17)}
        results |= {check_dev(text, text_phase=3, qual_phase=phase, flags=phase & 1) for phase in range(17)}
        assert len(results) == 1
    # the last line feed of the text opens no line: the poison '@' behind it is no record
    assert POISON[(12 + 10) % 4][:1] == b"@" and check_dev(b"@r\nAC\n+\nII\n", text_phase=12) == (2, 1, 0, 2, 0)


@gpu
def test_gpu_capacities(L):
    """out_cap, qual_cap and rec_cap at their edges: the counts stay full, the clipped last word is masked, nothing past the
    clipped extents is written; the host tier answers CNT_ECAP after the work"""
    rng = np.random.default_rng(154)
    big = well_formed(rng, 12, 1, 3000)
    for text in (big, small_fastq(rng, 900)):
        r = np_fastq(text)
        n, Q, R = r.seq.size, r.qual.size, r.rec_text.size
        assert n > 34 and Q > 18 and R > 2
        for j, out_cap in enumerate((0, 1, 31, 32, 33, n - 1, n)):
            for rec_cap in (0, 1, R - 1, R):
                check_dev(text, out_cap=out_cap, rec_cap=rec_cap, out_phase=out_cap & 1, qual_cap=(Q, Q - 1)[j & 1])
                check_host(L, text, out_cap=out_cap, rec_cap=rec_cap)
            check_dev(text, out_cap=out_cap, with_rec=False, with_qual=False)
            check_host(L, text, out_cap=out_cap, with_rec=False, rec_cap=0, with_qual=False, qual_cap=0)  # absent arrays run out of nothing
        for j, qual_cap in enumerate((0, 1, 3, 4, 5, 15, 16, 17, Q - 1, Q)):
            check_dev(text, qual_cap=qual_cap, qual_phase=j % 16, text_phase=j)
            check_dev(text, qual_cap=qual_cap, qual_phase=(j + 9) % 16, out_cap=33, rec_cap=1, with_rec=bool(j & 1))
            check_host(L, text, qual_cap=qual_cap)
            check_host(L, text, qual_cap=qual_cap, with_rec=False, pinned=True)


@gpu
def test_gpu_flags(L):
    rng = np.random.default_rng(155)
    text = b"@r\nACGTNnacgtu7\x80\xff U@\r\n+\n" + random_text(rng, TILE + 300, bytes(range(256)).replace(b"\n", b"")) + b"\n@s\nNNNN\n+\n" + bytes(range(11, 256))
    invalid = set()
    for flags in (0, CNT_STRICT_LUT, CNT_ALLOW_N, CNT_STRICT_LUT | CNT_ALLOW_N):
        check_dev(text, flags=flags)
        check_host(L, text, flags=flags)
        invalid.add(expect(text, flags, 0, 0, 0)[0][2])
    assert len(invalid) == 2
    r = np_fastq(text)
    assert not np.array_equal(np_words(r.seq, True), np_words(r.seq, False)) and len(set(r.qual.tolist())) > 250


@gpu
def test_gpu_roles_across_launch_seams(launch_tiles):
    """the lab build cut into launches of 64 / 128 tiles, 257 tiles: a role change on every launch seam and a long line across it;
    the passes in several launches, counted in a captured graph"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(launch_tiles)
    tiles = 257
    parts, pos = [], 0
    for j, e in enumerate(range(launch_tiles * TILE, tiles * TILE, launch_tiles * TILE)):
        # a line of role j % 4 ends exactly on the seam, the next role begins on it with a line that runs 3000 bytes past it
        piece = planted(rng, e - pos, (j + 1) % 4, e - pos, long_len=3000)
        cut = piece[: e - pos + 3001 + (1 if (j + 1) % 2 == 0 else 0)]  # up to and with the long line's line feed
        cut = cut[: cut.rindex(b"\n") + 1]
        while cut.count(b"\n") % 4:
            cut += FILLS[cut.count(b"\n") % 4][:1] + b"\n"  # finish the record
        parts.append(cut)
        pos += len(cut)
    parts.append(well_formed(rng, 1, 10, 20))
    text = b"".join(parts)
    text += fq_record(rng, ((tiles - 1) * TILE + 4001 - len(text) - 6) // 2, name_len=2)
    n_len = len(text)
    assert fastq_plan(n_len, 0, launch_tiles)[0] == tiles
    for e in range(launch_tiles * TILE, n_len, launch_tiles * TILE):
        assert text[e - 1] == NL or b"\n" not in text[e - 2000 : e + 2000]
    counts = check_dev(text, tag=(launch_tiles,))
    assert counts[4] == 0 and counts[1] > 50
    check_dev(text, out_cap=counts[0] // 2, qual_cap=counts[3] // 3, with_rec=False, tag=(launch_tiles,))
    got_tiles, launches = fastq_plan(n_len, 0, launch_tiles)
    assert launches == 3 * -(-tiles // launch_tiles) + 3
    d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    out, rt, rs, rq = (torch.empty(k, dtype=torch.int64, device="cuda") for k in (words_for(n_len), 100, 100, 100))
    qual = torch.empty(n_len, dtype=torch.uint8, device="cuda")
    cnt, work = torch.empty(5, dtype=torch.int64, device="cuda"), torch.empty(po.fastq_to_bits_work_bytes(n_len), dtype=torch.uint8, device="cuda")
    assert _kernel_nodes_of(torch, lambda: po.fastq_to_bits_dev(d, out, cnt, work, qual=qual, rec_text=rt, rec_start=rs, rec_qual=rq)) == launches


@gpu
def test_gpu_scan_round_edge():
    """just past the tiles one round of each one-workgroup scan takes (1024 lanes of 16 tiles), with a sequence line several tiles
    long lying across that edge, so that the second round begins with a carry of 1; a short record in front keeps the pattern off
    the tile grid.  A pattern of 16 whole records is tiled on the device in front of and behind the long record, the expected
    result is tiled from the numpy reference of the pattern, and the same construction is checked whole at a small size."""
    import torch

    from cute_nucleotides_amd import n_to_bits as nb, packed_ops as po

    rng = np.random.default_rng(156)
    pattern = b"".join(fq_record(rng, 150, name_len=40) for _ in range(16))
    P = np_fastq(pattern)
    per = P.seq.size
    assert len(pattern) == 16 * 345 and per == P.qual.size == 2400 and P.malformed == 0 and P.rec_text.size == 16
    prefix = b"@p\nACG\n+\nIII\n"
    r1, r2 = (ROUND * TILE - TILE - 100) // len(pattern), 40
    long_len = ROUND * TILE + 2 * TILE + 50 - r1 * len(pattern)
    long_rec = lambda k: b"@long\n" + b"G" * k + b"\n+\nIIIII\n"  # noqa: E731
    assert len(prefix) + r1 * len(pattern) + 6 < (ROUND - 1) * TILE and r1 * len(pattern) + long_len > (ROUND + 2) * TILE
    # the same construction at a size the numpy reference takes whole
    small = prefix + pattern * 3 + long_rec(3 * TILE) + pattern * 2
    s = np_fastq(small)
    assert s.seq.tobytes() == b"ACG" + P.seq.tobytes() * 3 + b"G" * (3 * TILE) + P.seq.tobytes() * 2 and s.malformed == 0
    assert s.qual.tobytes() == b"III" + P.qual.tobytes() * 3 + b"IIIII" + P.qual.tobytes() * 2 and s.rec_text.size == 2 + 5 * 16
    assert s.rec_text[1 + 16 : 1 + 32].tolist() == (P.rec_text + np.uint64(len(prefix) + len(pattern))).tolist()
    assert s.rec_start[1 + 16 : 1 + 32].tolist() == (P.rec_start + np.uint64(3 + per)).tolist()
    check_dev(small, text_phase=7)
    as_dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()  # noqa: E731
    d_pat = as_dev(pattern)
    d_text = torch.cat([as_dev(prefix), d_pat.repeat(r1), as_dev(long_rec(long_len)), d_pat.repeat(r2)])
    n_len = d_text.numel()
    assert fastq_plan(n_len)[0] > ROUND + 2
    n, Q, R = 3 + (r1 + r2) * per + long_len, 3 + (r1 + r2) * per + 5, 2 + (r1 + r2) * 16
    out = torch.full((words_for(n) + PAD,), CANARY, dtype=torch.int64, device="cuda")
    qual = torch.full((Q + QPAD,), QCANARY, dtype=torch.uint8, device="cuda")
    rt, rs, rq = (torch.full((R + 4,), CANARY, dtype=torch.int64, device="cuda") for _ in range(3))
    cnt = torch.full((5,), CANARY, dtype=torch.int64, device="cuda")
    work = torch.empty(po.fastq_to_bits_work_bytes(n_len), dtype=torch.uint8, device="cuda")
    po.fastq_to_bits_dev(d_text, out[: words_for(n)], cnt, work, qual=qual[:Q], rec_text=rt[:R], rec_start=rs[:R], rec_qual=rq[:R], out_cap=n)
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tolist() == [n, R, 0, Q, 0]
    d_seq, d_q = as_dev(P.seq.tobytes()), as_dev(P.qual.tobytes())
    want = nb.n_to_bits_dev(torch.cat([as_dev(b"ACG"), d_seq.repeat(r1), as_dev(b"G" * long_len), d_seq.repeat(r2)]))
    assert torch.equal(out[: words_for(n)], want[: words_for(n)]) and bool((out[words_for(n) :] == CANARY).all())
    assert torch.equal(qual[:Q], torch.cat([as_dev(b"III"), d_q.repeat(r1), as_dev(b"IIIII"), d_q.repeat(r2)])) and bool((qual[Q:] == QCANARY).all())
    # records: the prefix's, r1 patterns, the long one, r2 patterns; entry = the pattern's own + what lies in front of the copy
    mid = 1 + 16 * r1
    fronts = {"rt": (len(prefix), len(pattern), len(long_rec(long_len))), "rs": (3, per, long_len), "rq": (3, per, 5)}
    for key, arr, ref in (("rt", rt, P.rec_text), ("rs", rs, P.rec_start), ("rq", rq, P.rec_qual)):
        lead, step, gap = fronts[key]
        d_ref = torch.from_numpy(ref.astype(np.int64)).cuda()
        steps = lambda k: torch.arange(k, device="cuda", dtype=torch.int64)[:, None] * step  # noqa: E731
        assert int(arr[0]) == 0 and int(arr[mid]) == lead + r1 * step and bool((arr[R:] == CANARY).all()), key
        assert bool((arr[1:mid].view(r1, 16) == d_ref + lead + steps(r1)).all()), key
        assert bool((arr[mid + 1 : R].view(r2, 16) == d_ref + lead + r1 * step + gap + steps(r2)).all()), key


@gpu
def test_gpu_fastq_in_a_captured_graph_and_behind_a_side_stream():
    """one torch.cuda.graph capture of the call (with and without qual and the record table, on the same scratch in turn) replayed
    twice on changed text; then the call enqueued on a side stream behind the copy that makes its input, no host sync in between"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(157)
    n_len = 9 * TILE + 1234
    text = torch.zeros(n_len, dtype=torch.uint8, device="cuda")
    outs = [torch.empty(words_for(n_len), dtype=torch.int64, device="cuda") for _ in range(2)]
    qual = torch.empty(n_len, dtype=torch.uint8, device="cuda")
    rt, rs, rq = (torch.empty(n_len, dtype=torch.int64, device="cuda") for _ in range(3))
    cnts = torch.empty(10, dtype=torch.int64, device="cuda")
    work = torch.empty(po.fastq_to_bits_work_bytes(n_len), dtype=torch.uint8, device="cuda")

    def chain():
        po.fastq_to_bits_dev(text, outs[0], cnts[0:5], work, qual=qual, rec_text=rt, rec_start=rs, rec_qual=rq)
        po.fastq_to_bits_dev(text, outs[1], cnts[5:10], work, strict_lut=True)

    def make(rep):
        body = well_formed(rng, 60, 1, 3000, letters=b"ACGTN") + b"@g%d\n" % rep
        return (body + b"A" * n_len)[:n_len]

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain()  # module load outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()

    def verify(t, strict_second, rep):
        counts, want, want_q, want_rec = expect(t, 0, n_len, n_len, n_len)
        assert cnts[0:5].cpu().numpy().tolist() == counts, rep
        assert np.array_equal(outs[0][: want.size].cpu().numpy().view(np.uint64), want), rep
        assert np.array_equal(qual[: want_q.size].cpu().numpy(), want_q), rep
        for a, w in zip((rt, rs, rq), want_rec):
            assert np.array_equal(a[: w.size].cpu().numpy().view(np.uint64), w), rep
        if strict_second:
            assert cnts[5:10].cpu().numpy().tolist() == counts, rep
            assert np.array_equal(outs[1][: want.size].cpu().numpy().view(np.uint64), expect(t, CNT_STRICT_LUT, n_len, 0, 0)[1]), rep

    for rep in range(2):
        t = make(rep)
        text.copy_(torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()))
        for x in outs + [rt, rs, rq, cnts]:
            x.fill_(CANARY)
        qual.fill_(QCANARY)
        work.fill_(0x77 + rep)  # the scratch needs no zeroing
        g.replay()
        torch.cuda.synchronize()
        verify(t, True, rep)
        assert (rt[int(cnts[1].item()) :].cpu().numpy() == CANARY).all() and (qual[int(cnts[3].item()) :].cpu().numpy() == QCANARY).all()
    t = make(2)
    host = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).pin_memory()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        text.copy_(host, non_blocking=True)
        po.fastq_to_bits_dev(text, outs[0], cnts[0:5], work, qual=qual, rec_text=rt, rec_start=rs, rec_qual=rq)
    torch.cuda.current_stream().wait_stream(side)
    verify(t, False, 2)


@gpu
def test_gpu_host_tier_pinned_and_pageable(L):
    """pinned host buffers (used in place: the plain stores and the merges of shared words go over the link) and pageable ones
    (staged); then the guess-and-retry wrapper on the real library"""
    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(158)
    sparse = b"".join(b"@" + b"h" * (TILE - 10) + b"\nA\n+\nI\n" + b"@" + b"h" * (TILE - 10) + b"\nC\n+\n#\n" for _ in range(3))  # tiles that merge into one word
    for text in (well_formed(rng, 30, 100, 1000) + well_formed(rng, 5, 100, 300, eol=b"\r\n"), sparse, small_fastq(rng, 45)):
        r = np_fastq(text)
        n, Q, R = r.seq.size, r.qual.size, r.rec_text.size
        for pinned in (False, True):
            for out_cap, qual_cap, rec_cap in ((len(text),) * 3, (n, Q, R), (max(n - 1, 0), Q, R), (n, max(Q - 1, 0), R), (n, Q, max(R - 1, 0))):
                for with_rec, with_qual in ((True, True), (False, True), (True, False)):
                    check_host(L, text, out_cap=out_cap, qual_cap=qual_cap, rec_cap=rec_cap, with_rec=with_rec, with_qual=with_qual, pinned=pinned, flags=CNT_ALLOW_N)
    for text in (b"@r\nA\n+\nI\n" * 3000, fq_record(rng, 2 * TILE)):
        got = po.fastq_to_bits_hip(text)
        r = np_fastq(text)
        assert got.n == r.seq.size and got.invalid == 0 and got.malformed == 0 and np.array_equal(got.words, np_words(r.seq, False)) and np.array_equal(got.qual, r.qual)
        assert np.array_equal(got.rec_text, r.rec_text) and np.array_equal(got.rec_start, r.rec_start) and np.array_equal(got.rec_qual, r.rec_qual)
    assert po.fastq_names(b"@r\nA\n+\nI\n" * 3, po.fastq_to_bits_hip(b"@r\nA\n+\nI\n" * 3, with_qual=False).rec_text) == [b"r"] * 3


@gpu
def test_gpu_composition_with_subseq_and_fasta():
    """for each record, cnt_subseq_dev of the call's words at rec_start equals the plain encode of the record's own bases; the FASTA
    rewriting of the same file through fasta_to_bits_dev gives the same words and rec_start"""
    import torch

    from cute_nucleotides_amd import n_to_bits as nb, packed_ops as po

    rng = np.random.default_rng(159)
    reads = [random_text(rng, int(k), b"ACGT") for k in (1, 61, 5000, 33, 2 * TILE + 1, 32, 150)]
    eols = [b"\n", b"\r\n", b"\n", b"\n", b"\r\n", b"\n", b"\n"]
    text = b"".join(b"@rec %d" % r + e + s + e + b"+" + e + b"I" * len(s) + e for r, (s, e) in enumerate(zip(reads, eols)))
    fasta = b"".join(b">rec %d\n" % r + s + b"\n" for r, s in enumerate(reads))
    as_dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()  # noqa: E731
    d_text = as_dev(text)
    out, out_fa = (torch.zeros(words_for(len(text)), dtype=torch.int64, device="cuda") for _ in range(2))
    rt, rs, rq, fa_rt, fa_rs = (torch.empty(16, dtype=torch.int64, device="cuda") for _ in range(5))
    cnt, fa_cnt = torch.empty(5, dtype=torch.int64, device="cuda"), torch.empty(3, dtype=torch.int64, device="cuda")
    work = torch.empty(po.fastq_to_bits_work_bytes(len(text)), dtype=torch.uint8, device="cuda")
    po.fastq_to_bits_dev(d_text, out, cnt, work, rec_text=rt, rec_start=rs, rec_qual=rq)
    n, R, invalid, Q, malformed = cnt.cpu().numpy().tolist()
    assert R == len(reads) and Q == n and invalid == 0 and malformed == 0 and torch.equal(rs[:R], rq[:R])
    starts = rs[:R].cpu().numpy().tolist() + [n]
    for r, own in enumerate(reads):
        assert starts[r + 1] - starts[r] == len(own), r
        assert torch.equal(po.subseq_dev(out[: words_for(n)], n, starts[r], len(own)), nb.n_to_bits_dev(as_dev(own))), r
    fa_work = torch.empty(po.fasta_to_bits_work_bytes(len(fasta)), dtype=torch.uint8, device="cuda")
    po.fasta_to_bits_dev(as_dev(fasta), out_fa, fa_cnt, fa_work, rec_text=fa_rt, rec_start=fa_rs)
    assert fa_cnt.cpu().numpy().tolist() == [n, R, 0] and torch.equal(out_fa[: words_for(n)], out[: words_for(n)]) and torch.equal(fa_rs[:R], rs[:R])


@gpu
def test_gpu_fastq_fuzz(L):
    """200 random texts: random alphabet weights, line lengths up to several tiles, random capacities, flags and phases"""
    rng = np.random.default_rng(160)
    for case in range(200):
        kind = int(rng.integers(0, 4))
        n_len = int(rng.integers(1, 40001))
        if kind == 0:
            text = random_text(rng, n_len, ALPHABET)
        elif kind == 1:
            text = small_fastq(rng, n_len)
        elif kind == 2:
            text = random_text(rng, n_len, b"ACGT" * int(rng.choice([1, 30, 2000])) + b"@+\n\r")
        else:
            parts, size = [], 0
            while size < n_len:
                p = fq_record(rng, int(rng.choice([1, 30, 150, 4000, TILE, 3 * TILE])), b"\r\n" if rng.random() < 0.2 else b"\n", name_len=int(rng.choice([1, 40, TILE + 3])))
                parts.append(p)
                size += len(p)
            text = b"".join(parts)[:n_len]
        r = np_fastq(text)
        n, Q, R = r.seq.size, r.qual.size, r.rec_text.size
        out_cap = [n_len, n, max(n - 1, 0), int(rng.integers(0, n_len + 1)), int(rng.integers(0, n + 1))][int(rng.integers(0, 5))]
        qual_cap = [n_len, Q, max(Q - 1, 0), int(rng.integers(0, n_len + 1)), int(rng.integers(0, Q + 1))][int(rng.integers(0, 5))]
        rec_cap = [n_len, R, max(R - 1, 0), int(rng.integers(0, R + 1)), 0][int(rng.integers(0, 5))]
        flags = int(rng.integers(0, 4))
        check_dev(text, flags=flags, out_cap=out_cap, qual_cap=qual_cap, rec_cap=rec_cap, with_qual=bool(rng.integers(0, 4)), with_rec=bool(rng.integers(0, 4)),
                  text_phase=int(rng.integers(0, 16)), qual_phase=int(rng.integers(0, 16)), out_phase=int(rng.integers(0, 3)), tag=(case, kind))
        if case % 10 == 0:
            check_host(L, text, flags=flags, out_cap=out_cap, qual_cap=qual_cap, rec_cap=rec_cap, with_qual=bool(rng.integers(0, 2)), with_rec=bool(rng.integers(0, 2)),
                       pinned=case % 20 == 0, tag=(case, kind))
