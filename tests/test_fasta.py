"""FASTA text straight to packed words, with a record table (include/cute_nt.h "text formats: FASTA", hip/fasta_kernels.hpp,
hip/fasta_abi.inc): header lines, line feeds and carriage returns are dropped, every other byte is encoded as the encoder encodes
it, and each header line is reported with its byte offset and the position of its first base.  Not in the reference: the
definition is restated here three ways -- a byte-by-byte state machine, bytes.split(b"\\n") line by line, and vectorised in numpy
-- and the three are pinned against each other before the library is compared with the last one.

CPU part: the references, the properties of the definition, every argument rule of both tiers and the query in the order the
header states them (all of them precede device work), an aliasing sweep of every (written, other) pair, the Python layer without
a device, the launch plan in the sources and the header's comment.  GPU part: both tiers word for word and entry for entry
against the numpy reference, with canaries around every footprint."""
import ctypes
import mmap
import os
import re
import types

import numpy as np
import pytest

from test_aliasing import OVERLAPS, TOUCHES, Arena, Buf, Call, pairs, place, shared_bytes
from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 8192  # bytes per workgroup tile (hip/fasta_kernels.hpp kFastaTile)
LANE, WAVE = 32, 64 * 32  # bytes per lane and per wave of a tile
ROUND = 1024 * 16  # tiles one round of fasta_scan takes: kFastaScanBlock lanes, kCountedGroup tiles each
CNT_STRICT_LUT, CNT_ALLOW_N, CNT_TAIL_LUT = 1, 2, 4
NL, CR, GT = 0x0A, 0x0D, 0x3E
ALPHABET = b"ACGTacgtN>\n\n\n\r\x80 "  # a triple weight on the line feed


# ---- the three references -----------------------------------------------------------------------------------------------------
def def_fasta(text):
    """the definition, byte by byte: (kept bytes, rec_text, rec_start)"""
    kept, rec_text, rec_start = bytearray(), [], []
    header = False
    for p, b in enumerate(text):
        if p == 0 or text[p - 1] == NL:
            header = b == GT
            if header:
                rec_text.append(p)
                rec_start.append(len(kept))
        if not header and b != NL and b != CR:
            kept.append(b)
    return bytes(kept), rec_text, rec_start


def lines_fasta(text):
    """line by line: a line that starts with '>' is a record, every other line is kept without its carriage returns"""
    kept, rec_text, rec_start, at = bytearray(), [], [], 0
    for line in bytes(text).split(b"\n"):
        if line.startswith(b">"):
            rec_text.append(at)
            rec_start.append(len(kept))
        else:
            kept += line.replace(b"\r", b"")
        at += len(line) + 1
    return bytes(kept), rec_text, rec_start


def np_fasta(text):
    """vectorised: (kept bytes as uint8, rec_text, rec_start as uint64)"""
    t = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    if t.size == 0:
        return t, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    line_start = np.r_[True, t[:-1] == NL]
    last = np.maximum.accumulate(np.where(line_start, np.arange(t.size), 0))  # the last line start at or in front of each byte
    keep = (t[last] != GT) & (t != NL) & (t != CR)
    before = np.cumsum(keep) - keep  # kept bytes in front of each byte
    h = np.flatnonzero(line_start & (t == GT))
    return t[keep], h.astype(np.uint64), before[h].astype(np.uint64)


def words_for(n):
    return (n + 31) // 32


LUT = np.zeros(256, dtype=np.uint64)  # CNT_STRICT_LUT: the byte table, 0 for every byte outside the alphabet
for _letter, _code in zip(b"ACTUGactug", (0, 1, 2, 2, 3) * 2):
    LUT[_letter] = _code


def np_words(kept, strict):
    """the encoder's words of the kept bytes in numpy: (byte >> 1) & 3, or the byte table; zeros behind the last code"""
    k = np.asarray(kept, dtype=np.uint8)
    codes = LUT[k] if strict else ((k >> 1) & 3).astype(np.uint64)
    padded = np.zeros(words_for(k.size) * 32, dtype=np.uint64)
    padded[: k.size] = codes
    return np.bitwise_or.reduce(padded.reshape(-1, 32) << (np.uint64(2) * np.arange(32, dtype=np.uint64)), axis=1) if k.size else np.zeros(0, dtype=np.uint64)


VALID = np.zeros((2, 256), dtype=bool)
VALID[:, list(b"ACGTUacgtu")] = True
VALID[1, list(b"Nn")] = True


def np_invalid(kept, allow_n):
    return int((~VALID[int(bool(allow_n))][np.asarray(kept, dtype=np.uint8)]).sum())


def random_text(rng, n, alphabet=ALPHABET):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)])


def small_fasta(rng, n):
    """n bytes of FASTA-like text: short names, lines of 1..25 letters, now and then a carriage return, a blank line, an N"""
    parts, size = [], 0
    while size < n:
        r = rng.random()
        if r < 0.25:
            p = b">" + random_text(rng, int(rng.integers(0, 9)), b"abc >1") + (b"\r\n" if rng.random() < 0.3 else b"\n")
        elif r < 0.3:
            p = b"\n"
        else:
            p = random_text(rng, int(rng.integers(1, 26)), b"ACGTACGTacgtN") + (b"\r\n" if rng.random() < 0.3 else b"\n")
        parts.append(p)
        size += len(p)
    return b"".join(parts)[:n]


def sample_texts():
    rng = np.random.default_rng(41)
    texts = [random_text(rng, n) for n in range(60)] + [small_fasta(rng, n) for n in range(60)]
    texts += [random_text(rng, int(rng.integers(1, 400))) for _ in range(720)]
    texts += [small_fasta(rng, int(rng.integers(1, 600))) for _ in range(400)]
    texts += [b">", b"\n", b">\n", b"\n>", b">>", b"A>", b"\r", b"\r\n>x", b">x\r", b"A\n>", b"A\n>\nC", b"\n\n>\n\n", b">a\n>b\n>c", b"A\r\r\nC"]
    return texts


def test_three_references_agree():
    texts = sample_texts()
    assert len(texts) >= 1250 and {len(t) for t in texts} >= set(range(60))
    for t in texts:
        d, l, v = def_fasta(t), lines_fasta(t), np_fasta(t)
        assert d == l and d[0] == v[0].tobytes() and d[1] == v[1].tolist() and d[2] == v[2].tolist(), t
    recs = sum(len(def_fasta(t)[1]) for t in texts)
    assert recs > 2000 and sum(1 for t in texts if def_fasta(t)[1] and def_fasta(t)[2][0] > 0) > 100  # bases in front of the first header


def test_expected_words_and_invalid_count_are_the_oracles(oracle):
    """np_words against the oracle's encoders on all 256 byte values (bit extraction on whole words: its ragged end goes through
    the table), np_invalid against oracle.validate"""
    rng = np.random.default_rng(42)
    for n in (0, 1, 31, 32, 33, 64, 256, 1000, 4096):
        k = rng.integers(0, 256, n, dtype=np.uint8)
        k[: min(n, 256)] = np.arange(min(n, 256), dtype=np.uint8)
        assert np.array_equal(np_words(k, True), oracle.n_to_bits_lut(k)[: words_for(n)]), n
        whole = n // 32 * 32
        assert np.array_equal(np_words(k[:whole], False), oracle.n_to_bits_bitextract(k[:whole])[: whole // 32]), n
        for allow_n in (False, True):
            assert np_invalid(k, allow_n) == oracle.validate(k, allow_n), n
    for t in sample_texts()[::25]:
        kept = np_fasta(t)[0]
        assert np.array_equal(np_words(kept, True), oracle.n_to_bits_lut(kept)[: words_for(kept.size)]) and np_invalid(kept, True) == oracle.validate(kept, True)


def test_properties():
    rng = np.random.default_rng(43)
    for t in sample_texts():
        kept, rec_text, rec_start = np_fasta(t)
        n = kept.size
        assert n <= len(t) and (np.diff(rec_text.astype(np.int64)) > 0).all() and (np.diff(rec_start.astype(np.int64)) >= 0).all()
        assert all(t[int(h)] == GT and (h == 0 or t[int(h) - 1] == NL) for h in rec_text) and (rec_start <= n).all()
        # stripping is idempotent on header-free text
        again = np_fasta(kept.tobytes())
        if GT not in kept.tobytes()[:1]:
            assert again[0].tobytes() == kept.tobytes() and again[1].size == 0
        # the records' own text, stripped, is the kept bytes behind rec_start[0]
        ends = np.r_[rec_text[1:], np.uint64(len(t))].astype(np.int64)
        own = b"".join(np_fasta(t[int(a) : int(b)])[0].tobytes() for a, b in zip(rec_text.astype(np.int64), ends))
        assert own == (kept[int(rec_start[0]) :].tobytes() if rec_text.size else b"")
        for r in range(rec_text.size):
            piece = np_fasta(t[int(rec_text[r]) : int(ends[r])])[0]
            assert piece.size == int(np.r_[rec_start, np.uint64(n)][r + 1] - rec_start[r])
        # \r\n and \n texts give equal results, up to the byte offsets
        unix = t.replace(b"\r", b"")
        dos = unix.replace(b"\n", b"\r\n")
        a, b = np_fasta(unix), np_fasta(dos)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2]) and a[1].size == b[1].size
        # '>' inside a line changes nothing but the invalid count
        if len(t) > 2:
            p = int(rng.integers(1, len(t)))
            if t[p - 1] != NL and t[p] in b"ACGTacgt":
                u = t[:p] + b">" + t[p + 1 :]
                ku, rt, rs = np_fasta(u)
                assert ku.size == n and np.array_equal(rt, rec_text) and np.array_equal(rs, rec_start)
                assert np_invalid(ku, False) == np_invalid(kept, False) + (1 if np_fasta(t[: p + 1])[0].size > np_fasta(t[:p])[0].size else 0)


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
    later one must not be reached; canaries (the fill) around every buffer: a refused call writes nothing"""
    from cute_nucleotides_amd import _lib

    OK, EINVAL = _lib.CNT_OK, _lib.CNT_EINVAL
    vp = ctypes.c_void_p
    arena = np.full(1 << 16, FILL, dtype=np.uint8)
    base = arena.ctypes.data + (-arena.ctypes.data % 128)
    at = lambda k: vp(base + 4096 * k)  # noqa: E731 -- buffer k of a call, each in a 4-KiB slot of its own
    n_len = 1000
    need = ctypes.c_size_t(0)
    # 1. the query: a NULL bytes; the answer is 0 without a byte, grows with the text, and does not depend on any address
    assert L.cnt_fasta_to_bits_work_bytes(n_len, None) == EINVAL and L.cnt_fasta_to_bits_work_bytes(0, None) == EINVAL
    assert L.cnt_fasta_to_bits_work_bytes(0, ctypes.byref(need)) == OK and need.value == 0
    sizes = []
    for n in (1, TILE - 15, TILE - 14, TILE, 16 * TILE, 16 * TILE + 1, 1 << 30, 1 << 36):
        assert L.cnt_fasta_to_bits_work_bytes(n, ctypes.byref(need)) == OK
        sizes.append(need.value)
    assert sizes == sorted(sizes) and sizes[0] >= 96 and sizes[1] == sizes[0] and sizes[-1] < (1 << 36) // 256  # bytes per text byte
    assert L.cnt_fasta_to_bits_work_bytes(n_len, ctypes.byref(need)) == OK
    need = need.value

    def dev(text=at(0), n=n_len, flags=0, out=at(1), out_cap=n_len, rt=at(2), rs=at(4), rec_cap=50, counts=at(6), work=at(7), work_bytes=need):
        return L.cnt_fasta_to_bits_dev(text, n, flags, out, out_cap, rt, rs, rec_cap, counts, work, work_bytes, None)

    def host(text=at(0), n=n_len, flags=0, out=at(1), out_cap=n_len, rt=at(2), rs=at(4), rec_cap=50, counts=at(6)):
        return L.cnt_fasta_to_bits(text, n, flags, ctypes.cast(out, U64P), out_cap, ctypes.cast(rt, U64P), ctypes.cast(rs, U64P), rec_cap, ctypes.cast(counts, U64P))

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
            assert call(**{null: None}) == EINVAL and call(**{null: None}, rt=vp(at(2).value + 4)) == EINVAL and call(**{null: None}, rs=None) == EINVAL
        # 4. alignment of out, counts and the record arrays; the text may sit anywhere -- in front of 5 and 6
        for name, slot in (("out", 1), ("counts", 6), ("rt", 2), ("rs", 4)):
            for off in (1, 4, 7):
                assert call(**{name: vp(at(slot).value + off)}) == EINVAL
        assert call(out=vp(at(1).value + 4), rs=None) == EINVAL and call(rt=vp(at(2).value + 4), out=at(0)) == EINVAL
        # 5. one record array without the other -- in front of 6
        assert call(rt=None) == EINVAL and call(rs=None) == EINVAL and call(rt=None, out=at(0)) == EINVAL
        # 6. overlaps, at the stated extents: the footprint of out, min(text_len, rec_cap) entries, 24 bytes of counts
        assert call(out=at(0)) == EINVAL and call(rt=at(4)) == EINVAL and call(counts=vp(at(1).value + 8)) == EINVAL
        assert call(counts=vp(at(0).value + n_len - 8)) == EINVAL and call(rs=vp(at(2).value + 8 * 49)) == EINVAL
        assert call(counts=vp(at(4).value - 16)) == EINVAL  # the third count lies in rec_start
        assert untouched()
    # 7. the device tier's scratch, after everything else
    assert dev(work=None) == EINVAL and dev(work_bytes=need - 1) == EINVAL and dev(work_bytes=0) == EINVAL
    for other in (0, 1, 2, 4, 6):
        assert dev(work=vp(at(other).value - need + 8)) == EINVAL  # the last 8 bytes of the query's answer reach into the buffer
    assert dev(work=None, out=at(0)) == EINVAL and untouched()
    # the host tier sets its counts at length 0, and only them
    c = np.full(5, 7, dtype=np.uint64)
    assert L.cnt_fasta_to_bits(None, 0, CNT_ALLOW_N, None, 5, None, None, 5, ctypes.cast(vp(c.ctypes.data + 8), U64P)) == OK
    assert c.tolist() == [7, 0, 0, 0, 7]
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        assert host() == _lib.CNT_ENODEV and host(rt=None, rs=None, rec_cap=1 << 40) == _lib.CNT_ENODEV
        assert host(out=at(0), out_cap=0) == _lib.CNT_ENODEV  # capacity 0: out may sit anywhere
        assert host(text=vp(at(0).value + 3), rs=vp(at(2).value + 8 * 50)) == _lib.CNT_ENODEV  # the arrays touch; the text at any byte
        assert dev(work=vp(at(7).value + 4)) < 0  # a scratch at any address
        assert untouched()


def fasta_calls(L):
    """the two tiers as test_aliasing's table rows: every buffer with its extent, its alignment and whether it is written"""
    vp = ctypes.c_void_p
    up = lambda a: ctypes.cast(vp(a), U64P)  # noqa: E731
    n_len, out_cap, rec_cap = 1000, 200, 24  # ASCII bytes: a multiple of 8, so that an 8-B aligned buffer can touch their end
    need = ctypes.c_size_t(0)
    assert L.cnt_fasta_to_bits_work_bytes(n_len, ctypes.byref(need)) == 0
    need = need.value
    bufs = [Buf("text", n_len, 1, False), Buf("out", words_for(out_cap) * 8, 8, True), Buf("rec_text", rec_cap * 8, 8, True),
            Buf("rec_start", rec_cap * 8, 8, True), Buf("counts", 24, 8, True)]
    dev = Call("cnt_fasta_to_bits_dev", bufs + [Buf("work", need, 8, True)],
               lambda p: L.cnt_fasta_to_bits_dev(vp(p["text"]), n_len, 0, vp(p["out"]), out_cap, vp(p["rec_text"]), vp(p["rec_start"]), rec_cap, vp(p["counts"]),
                                                 vp(p["work"]), need + 64, None), frozenset())
    host = Call("cnt_fasta_to_bits", bufs,
                lambda p: L.cnt_fasta_to_bits(vp(p["text"]), n_len, 3, up(p["out"]), out_cap, up(p["rec_text"]), up(p["rec_start"]), rec_cap, up(p["counts"])),
                frozenset())
    return [dev, host]


def test_aliasing_sweep_of_every_written_buffer(L):
    """every (written, other) pair of both tiers: the five overlapping placements are CNT_EINVAL and write nothing, the two
    touching ones pass the argument checks"""
    from cute_nucleotides_amd import _lib

    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    arena = Arena()
    tried = 0
    for call in fasta_calls(L):
        assert len(pairs(call)) == (5 * 5 if call.name.endswith("_dev") else 4 * 4)
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
    assert tried >= 150


def test_abi_wiring(L):
    import subprocess

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib, packed_ops as po

    names = ("cnt_fasta_to_bits", "cnt_fasta_to_bits_dev", "cnt_fasta_to_bits_work_bytes")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    hpp = open(os.path.join(ROOT, "cute_nucleotides_amd", "cute_nucleotides.hpp")).read()
    for name in names:
        assert name in exported and ("int %s(" % name) in header and ("fn %s(" % name) in rust and (name + "(") in hpp and name in _lib.SIGNATURES, name
    assert "pub fn fasta_to_bits_hip(" in rust and "inline Fasta fasta_to_bits_hip(" in hpp and "pub fn fasta_to_bits_hip_dev(" in rust
    for name in ("fasta_to_bits_hip", "fasta_to_bits_dev", "fasta_to_bits_work_bytes", "fasta_names"):
        assert getattr(cn, name) is getattr(po, name) and name in cn.__all__
    assert "#define CNT_ABI_VERSION 1" in header  # symbols were only added: the version did not move


def test_header_comment_and_section_place():
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    title = "/* ---- text formats: FASTA ----"
    assert header.count(title) == 1
    at = header.index(title)
    # behind the windowed composition, not inside the span tests/test_aliasing.py holds to its table
    assert header.index("---- windowed composition") < header.index("int cnt_window_counts(") < at < header.index("Kernel selection for A/B runs")
    assert not (header.index("---- packed-domain operations") < at < header.index("---- device utilities"))
    section = header[at : header.index("Kernel selection for A/B runs")]
    for k, name in enumerate(("CNT_FASTA_N", "CNT_FASTA_RECORDS", "CNT_FASTA_INVALID")):
        assert re.search(r"#define %s %d\b" % (name, k), section) and "counts[%s]" % name in section, name
    checks = ["1. an unknown flag", "2. text_len == 0", "3. a NULL text, out or counts", "4. an out, counts, rec_text or rec_start that is not 8-B aligned",
              "5. one record array without the other", "6. a written buffer sharing a byte", "7. device tier: a NULL d_work"]
    places = [section.index(c) for c in checks]
    assert places == sorted(places)
    for word in ("FASTQ", "';' comments", "5-letter variant", "nucleotide-to-byte-offset map", "line-wrapped decode", "gzip", "2^36", "CNT_TAIL_LUT included",
                 "enqueue-only", "capturable in a graph", "CNT_ECAP after the work"):
        assert word in section, word


def test_fasta_plan_matches_the_launcher_source():
    src = open(os.path.join(ROOT, "hip", "fasta_kernels.hpp")).read()
    assert "constexpr int kFastaBlock = 256;" in src and "kFastaLaneBytes = 32, kFastaTile = kFastaLaneBytes * kFastaBlock;" in src
    assert "constexpr int kFastaScanBlock = 1024;" in src and ROUND == 1024 * 16 and TILE == 32 * 256
    counted = open(os.path.join(ROOT, "hip", "counted_output.hpp")).read()
    assert "kCountedGroup = 16;" in counted
    kernels = [line for line in src.splitlines() if line.startswith("__global__")]
    assert len(kernels) == 7 and sum("(kFastaBlock) void fasta_" in k for k in kernels) == 6 and sum("(kFastaScanBlock) void fasta_scan(" in k for k in kernels) == 1
    # no atomic to global memory but the merge of the shared words; nothing scattered per dropped or invalid byte
    assert src.count("atomicOr(&s_out[") == 2 and src.count("atomicOr(") == 2 and src.count("hpc_merge(out + k, v)") == 1
    assert not re.search(r"atomic(Add|CAS|Max|Min|Exch|And|Xor|Inc)", src)
    assert "hpc_compress(w, fasta_spread(kept))" in src and '#include "hpc_kernels.hpp"' in src
    abi = open(os.path.join(ROOT, "hip", "fasta_abi.inc")).read()
    tiles = "split_launches(n_tiles, kFastaBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(%s, dim3((unsigned)n), dim3(kFastaBlock), 0, s, a, t); });"
    scan = "hipLaunchKernelGGL(fasta_scan, dim3(1), dim3(kFastaScanBlock), 0, s, a);"
    zero = "hipLaunchKernelGGL(hpc_zero_edges, dim3((unsigned)n), dim3(kHpcBlock), 0, s, h, t);"
    empty = "if (text_len == 0) return d_counts ? hip_rc(hipMemsetAsync(d_counts, 0, 24, s)) : CNT_OK;"
    assert abi.index(empty) < abi.index(tiles % "summary") < abi.index(scan) < abi.index(zero) < abi.index(tiles % "write")
    assert abi.count("hipLaunchKernelGGL(") == 4 and abi.count("split_launches(") == 3 and abi.count("hipMalloc") == 0 and abi.count("Synchronize") == 0
    assert "host_call(b, 24 + work_bytes, got, 3, CNT_FASTA_RECORDS, false," in abi
    shim = open(os.path.join(ROOT, "hip", "cute_nt.hip")).read()
    assert shim.index('#include "window_count_abi.inc"') < shim.index('#include "fasta_abi.inc"')
    # the short form of host_call, which every earlier caller uses, is the long one with one word that sizes the counted buffers
    assert "return host_call(b, aux_bytes, result, 1, 0, zero, static_cast<F&&>(dev));" in shim


def fasta_plan(text_len, phase=0, launch_tiles=((0x7FFFFFFF // 256) // 64) * 64):
    """(tiles, kernel launches) of a device call with capacities: two tile passes, the scan, the edge zeroing with a lane per tile"""
    tiles = -(-(text_len + phase) // TILE)
    return tiles, 2 * -(-tiles // launch_tiles) + 1 + -(-(-(-tiles // 256)) // launch_tiles)


# ---- CPU: the Python layer ------------------------------------------------------------------------------------------------------
def _fake_lib(calls):
    """a stand-in for the library whose cnt_fasta_to_bits is the numpy reference behind the C calling convention"""
    from cute_nucleotides_amd import _lib

    def u64_at(p, n):
        return np.frombuffer((ctypes.c_uint64 * n).from_address(p.value), dtype=np.uint64) if n else np.zeros(0, dtype=np.uint64)

    def cnt_fasta_to_bits(text, length, flags, out, out_cap, rec_text, rec_start, rec_cap, counts):
        calls.append((out_cap, rec_cap, flags))
        t = np.frombuffer((ctypes.c_uint8 * length).from_address(text.value), dtype=np.uint8) if length else np.zeros(0, dtype=np.uint8)
        kept, rt, rs = np_fasta(t)
        m, r = min(kept.size, out_cap), min(rt.size, rec_cap)
        if length:
            u64_at(out, words_for(m))[:] = np_words(kept[:m], flags & CNT_STRICT_LUT)
            u64_at(rec_text, r)[:] = rt[:r]
            u64_at(rec_start, r)[:] = rs[:r]
        counts[0], counts[1], counts[2] = kept.size, rt.size, np_invalid(kept, flags & CNT_ALLOW_N)
        return _lib.CNT_ECAP if kept.size > out_cap or rt.size > rec_cap else _lib.CNT_OK

    return types.SimpleNamespace(cnt_fasta_to_bits=cnt_fasta_to_bits, cnt_words_for=words_for)


def test_fasta_to_bits_hip_retries_once_with_the_reported_count(monkeypatch, tmp_path):
    from cute_nucleotides_amd import packed_ops as po

    calls = []
    fake = _fake_lib(calls)
    monkeypatch.setattr(po, "lib", lambda: fake)
    rng = np.random.default_rng(44)
    few = small_fasta(rng, 30000)  # about 700 records: inside the first guess
    kept, rt, rs = np_fasta(few)
    assert 100 < rt.size < 1024
    path = tmp_path / "few.fa"
    path.write_bytes(few)
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mapped:
        for text in (few, bytearray(few), np.frombuffer(few, dtype=np.uint8), mapped, memoryview(few)):
            del calls[:]
            words, n, rec_text, rec_start, invalid = po.fasta_to_bits_hip(text, allow_n=True)
            assert len(calls) == 1 and calls[0] == (len(few), len(few) // 4096 + 1024, CNT_ALLOW_N)
            assert n == kept.size and np.array_equal(words, np_words(kept, False)) and np.array_equal(rec_text, rt) and np.array_equal(rec_start, rs)
            assert invalid == np_invalid(kept, True) and words.dtype == rec_text.dtype == rec_start.dtype == np.uint64
    many = b">r\nA\n" * 3000  # more records than the guess: one retry at the reported number
    del calls[:]
    words, n, rec_text, rec_start, invalid = po.fasta_to_bits_hip(many, strict_lut=True)
    assert [c[1] for c in calls] == [len(many) // 4096 + 1024, 3000] and calls[1][2] == CNT_STRICT_LUT
    assert n == 3000 and rec_text.tolist() == list(range(0, 15000, 5)) and rec_start.tolist() == list(range(3000)) and invalid == 0
    assert np.array_equal(words, np_words(np.full(3000, 65, dtype=np.uint8), True))
    # nothing to encode
    del calls[:]
    words, n, rec_text, rec_start, invalid = po.fasta_to_bits_hip(b"")
    assert (words.size, n, rec_text.size, rec_start.size, invalid) == (0, 0, 0, 0, 0)
    # a second CNT_ECAP is an error, not a loop; so is any other status
    fake.cnt_fasta_to_bits = lambda *a: 2
    with pytest.raises(Exception):
        po.fasta_to_bits_hip(many)
    for bad in ("ACGT", 5, np.zeros(4, dtype=np.int32), [65, 67]):
        with pytest.raises(TypeError):
            po.fasta_to_bits_hip(bad)


def test_fasta_names():
    from cute_nucleotides_amd import packed_ops as po

    long_name = b"x" * 70000
    text = b"ACGT\n>one two\nAC\n>\r\n>three>3\r\nGG\n>" + long_name + b"\nA\n>last"
    rt = np_fasta(text)[1]
    want = [b"one two", b"", b"three>3", long_name, b"last"]
    assert po.fasta_names(text, rt) == want and po.fasta_names(bytearray(text), rt.tolist()) == want
    assert po.fasta_names(np.frombuffer(text, dtype=np.uint8), rt[1:3]) == want[1:3] and po.fasta_names(text, []) == []
    assert po.fasta_names(b">only\r", [0]) == [b"only"] and po.fasta_names(b">", [0]) == [b""]
    for bad in ([1], [len(text)], [4]):
        with pytest.raises(ValueError):
            po.fasta_names(text, bad)
    rng = np.random.default_rng(45)
    for _ in range(50):
        t = small_fasta(rng, 500)
        heads = [line[1:].rstrip(b"\r") for line in t.split(b"\n") if line.startswith(b">")]
        assert po.fasta_names(t, np_fasta(t)[1]) == heads


def test_device_wrapper_argument_errors():
    torch = pytest.importorskip("torch")
    from cute_nucleotides_amd import packed_ops as po

    t = torch.zeros(10, dtype=torch.uint8)
    with pytest.raises(ValueError):
        po.fasta_to_bits_dev(t, t, t, t)  # not on a device


# ---------------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
CANARY = -0x3C3C3C3C3C3C3C3D
HOST_CANARY = 0xDEADBEEFDEADBEEF
PAD = 5  # canary words in front of and behind every footprint
POISON = (b"\n>", b">>", b">\n", b"\n\n")  # in front of and behind the text: a byte looked at there changes the result


def expect(text, flags, out_cap, rec_cap):
    """(n, R, invalid, the words, rec_text and rec_start that must be written) at these capacities"""
    kept, rt, rs = np_fasta(text)
    m, r = min(kept.size, out_cap), min(rt.size, rec_cap)
    return kept.size, rt.size, np_invalid(kept, flags & CNT_ALLOW_N), np_words(kept[:m], flags & CNT_STRICT_LUT), rt[:r], rs[:r]


def check_dev(text, flags=0, out_cap=None, rec_cap=None, with_rec=True, text_phase=0, out_phase=0, tag=()):
    """the device tier on the text: words, record table, counts, canaries around every footprint, the text itself unchanged"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    n_len = len(text)
    out_cap = n_len if out_cap is None else out_cap
    rec_cap = n_len if rec_cap is None else rec_cap
    foot, rfoot = min(n_len, out_cap), min(n_len, rec_cap)
    n, R, invalid, want_out, want_rt, want_rs = expect(text, flags, out_cap, rec_cap)
    poison = POISON[(text_phase + n_len) % 4]
    front = (poison * 40)[-(64 + text_phase) :]  # the allocation is 256-B aligned: the text begins at byte phase text_phase of 16
    parent = np.frombuffer(front + bytes(text) + poison * 8, dtype=np.uint8)
    d_parent = torch.from_numpy(parent.copy()).cuda()
    d_text = d_parent[len(front) : len(front) + n_len]
    assert n_len == 0 or d_text.data_ptr() % 16 == text_phase % 16
    d_out = torch.full((PAD + out_phase + words_for(foot) + PAD,), CANARY, dtype=torch.int64, device="cuda")
    d_rt = torch.full((PAD + out_phase + rfoot + PAD,), CANARY, dtype=torch.int64, device="cuda")
    d_rs = torch.full((PAD + rfoot + PAD + 1,), CANARY, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((5,), CANARY, dtype=torch.int64, device="cuda")
    d_work = torch.full((po.fasta_to_bits_work_bytes(n_len) + 8,), 0x77, dtype=torch.uint8, device="cuda")
    o0 = PAD + out_phase
    po.fasta_to_bits_dev(d_text, d_out[o0 : o0 + words_for(foot)], d_cnt[1:4], d_work[4:],  # the scratch at a 4-B-misaligned address
                         rec_text=d_rt[o0 : o0 + rfoot] if with_rec else None, rec_start=d_rs[PAD + 1 : PAD + 1 + rfoot] if with_rec else None,
                         out_cap=out_cap, rec_cap=rec_cap if with_rec else None, strict_lut=bool(flags & CNT_STRICT_LUT), allow_n=bool(flags & CNT_ALLOW_N))
    torch.cuda.synchronize()
    tag = tag + (n_len, flags, out_cap, rec_cap, with_rec, text_phase, out_phase)
    assert d_cnt.cpu().numpy().tolist() == [CANARY, n, R, invalid, CANARY], tag + (n, R, invalid)
    assert np.array_equal(d_parent.cpu().numpy(), parent), tag + ("text",)
    h = d_out.cpu().numpy()
    assert (h[:o0] == CANARY).all() and (h[o0 + words_for(foot) :] == CANARY).all(), tag + ("out canary",)
    got = h[o0 : o0 + want_out.size].view(np.uint64)
    assert np.array_equal(got, want_out), tag + ("out", np.flatnonzero(got != want_out)[:4].tolist())
    for name, h, lo, want in (("rec_text", d_rt.cpu().numpy(), o0, want_rt), ("rec_start", d_rs.cpu().numpy(), PAD + 1, want_rs)):
        if with_rec:
            assert (h[:lo] == CANARY).all() and (h[lo + want.size :] == CANARY).all(), tag + (name, "canary")  # nothing past min(R, rec_cap)
            got = h[lo : lo + want.size].view(np.uint64)
            assert np.array_equal(got, want), tag + (name, np.flatnonzero(got != want)[:4].tolist())
        else:
            assert (h == CANARY).all(), tag + (name,)
    return n, R


def check_host(L, text, flags=0, out_cap=None, rec_cap=None, with_rec=True, pinned=False, tag=()):
    """the host tier on the text, pageable or pinned buffers, the text at an odd byte inside its allocation"""
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    n_len = len(text)
    out_cap = n_len if out_cap is None else out_cap
    rec_cap = n_len if rec_cap is None else rec_cap
    foot, rfoot = min(n_len, out_cap), min(n_len, rec_cap)
    n, R, invalid, want_out, want_rt, want_rs = expect(text, flags, out_cap, rec_cap)
    alloc = (lambda k, dt=np.uint64: cn.pinned_empty(k, dt)) if pinned else (lambda k, dt=np.uint64: np.empty(k, dtype=dt))
    buf = alloc(n_len + 8, np.uint8)
    buf[:] = GT
    buf[3 : 3 + n_len] = np.frombuffer(bytes(text), dtype=np.uint8)
    out, rt, rs, cnt = alloc(PAD + words_for(foot) + PAD), alloc(PAD + rfoot + PAD), alloc(PAD + rfoot + PAD), alloc(5)
    for a in (out, rt, rs, cnt):
        a[:] = HOST_CANARY
    rc = L.cnt_fasta_to_bits(buf[3:].ctypes.data, n_len, flags, out[PAD:].ctypes.data, out_cap, rt[PAD:].ctypes.data if with_rec else None,
                             rs[PAD:].ctypes.data if with_rec else None, rec_cap, cnt[1:].ctypes.data)
    tag = tag + (n_len, flags, out_cap, rec_cap, with_rec, pinned)
    assert rc == (_lib.CNT_ECAP if n > out_cap or (with_rec and R > rec_cap) else _lib.CNT_OK), tag + (rc, n, R)
    assert cnt.tolist() == [HOST_CANARY, n, R, invalid, HOST_CANARY], tag + (cnt.tolist(), n, R, invalid)
    assert (out[:PAD] == HOST_CANARY).all() and (out[PAD + words_for(foot) :] == HOST_CANARY).all(), tag + ("out canary",)
    assert np.array_equal(out[PAD : PAD + want_out.size], want_out), tag + ("out",)
    for name, a, want in (("rec_text", rt, want_rt), ("rec_start", rs, want_rs)):
        if with_rec:
            assert (a[:PAD] == HOST_CANARY).all() and (a[PAD + want.size :] == HOST_CANARY).all(), tag + (name, "canary")
            assert np.array_equal(a[PAD : PAD + want.size], want), tag + (name,)
        else:
            assert (a == HOST_CANARY).all(), tag + (name,)
    return n, R


def columns(rng, n_bases, width=60, eol=b"\n", letters=b"ACGT"):
    """n_bases random letters in lines of `width`"""
    s = random_text(rng, n_bases, letters)
    return b"".join(s[i : i + width] + eol for i in range(0, n_bases, width))


@gpu
def test_gpu_small_lengths_both_tiers(L):
    """every text_len 0..300 of random small FASTA, and a 60-column file of three records"""
    rng = np.random.default_rng(51)
    for n_len in range(301):
        text = small_fasta(rng, n_len) if n_len % 3 else random_text(rng, n_len)
        check_dev(text, flags=n_len & 3, text_phase=n_len % 17, out_phase=n_len & 1)
        check_host(L, text, flags=(n_len >> 1) & 3)
    for eol in (b"\n", b"\r\n"):
        text = b"".join(b">rec%d description" % r + eol + columns(rng, bases, eol=eol) for r, bases in enumerate((250, 60, 1234)))
        for phase in (0, 9):
            assert check_dev(text, text_phase=phase) == (250 + 60 + 1234, 3)
        assert check_host(L, text) == (1544, 3)


def _planted(rng, n_len, phase):
    """a 61-column text whose every line is plain sequence, as a bytearray, and where aligned byte e lies in it: e - phase"""
    t = bytearray(columns(rng, n_len)[:n_len])
    return t, (lambda e: e - phase)


def _seam_cases(rng, phase):
    """(name, text): every seam of the definition at the tile, wave and lane edges, for a text that begins at byte `phase` of 16"""
    cases = []
    n_len = 3 * TILE + 501
    edges = (("tile", TILE), ("second tile", 2 * TILE), ("wave", TILE + WAVE), ("lane", TILE + 7 * LANE), ("first lane", LANE))
    for where, e in edges:
        t, at = _planted(rng, n_len, phase)
        p = at(e)
        t[p - 1 : p + 12] = b"\n>name here\nA"  # the line feed ends one unit, the '>' begins the next
        cases.append(("line feed | '>' at a %s edge" % where, t))
        t, at = _planted(rng, n_len, phase)
        p = at(e)
        t[p - 3 : p + 3] = b"AC\r\nGT"  # \r | \n
        cases.append(("carriage return | line feed at a %s edge" % where, t))
        t, at = _planted(rng, n_len, phase)
        p = at(e)
        t[p - 20 : p + 1] = b"\n>" + b"h" * 17 + b"\r\n"  # the header's line feed is the first byte of the next unit
        cases.append(("a header's line feed behind a %s edge" % where, t))
        t, at = _planted(rng, n_len, phase)
        p = at(e)
        t[p - 2 : p + 2] = b"\n>\nC"  # an empty name whose line feed is the first byte behind the edge
        cases.append(("'>' | line feed at a %s edge" % where, t))
    for h in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE):
        for start in (0, 100, TILE - 3):
            name = b">" + random_text(rng, h - 2, b"ACGT >\r") + b"\n"  # h bytes with the line feed; '>' and \r inside are header bytes
            text = (columns(rng, start)[: start - 1] + b"\n" if start else b"") + name + columns(rng, 300)
            cases.append(("a header of %d bytes at %d" % (h, start), bytearray(text)))
    cases.append(("a header at byte 0", bytearray(b">x\n" + columns(rng, 500))))
    cases.append(("a header without a line feed at the end", bytearray(columns(rng, TILE + 50) + b">the end")))
    cases.append(("a long header without a line feed at the end", bytearray(columns(rng, 50) + b">" + b"e" * (2 * TILE + 9))))
    for k in (0, 1, 30, TILE - 1 - phase, TILE - phase, 2 * TILE + 3):
        cases.append(("one header only, %d bytes" % (k + 1), bytearray(b">" + b"x" * k)))
    cases.append(("line feeds only", bytearray(b"\n" * (TILE + 70))))
    cases.append(("no line feed at all", bytearray(random_text(rng, 2 * TILE + 5, b"ACGT"))))
    # a tile of dropped bytes only between two tiles that share an output word
    for filler in (b">" + b"h" * (TILE - 2) + b"\n", b"\r\n" * (TILE // 2)):
        first = random_text(rng, TILE - phase - 1, b"ACGT") + b"\n"  # tile 0 ends on the line feed and keeps 8191 - phase codes
        cases.append(("a tile of dropped bytes only (%r...)" % filler[:2], bytearray(first + filler + random_text(rng, 700, b"ACGT"))))
    # 45 tiles that each keep 1..3 bases: a long header and one-base lines, many tiles merged into one word
    parts = [random_text(rng, TILE - phase - 1, b"ACGT") + b"\n"]
    for tile in range(45):
        k = 1 + tile % 3
        parts.append(b">" + b"h" * (TILE - 2 - 2 * k) + b"\n" + b"".join(random_text(rng, 1, b"ACGT") + b"\n" for _ in range(k)))
    cases.append(("45 tiles of 1..3 bases", bytearray(b"".join(parts) + b"ACGTAC")))
    return cases


@gpu
@pytest.mark.parametrize("phase", [0, 5])
def test_gpu_seams(L, phase):
    rng = np.random.default_rng(52 + phase)
    for j, (name, text) in enumerate(_seam_cases(rng, phase)):
        text = bytes(text)
        n, R = check_dev(text, text_phase=phase, out_phase=j & 1, flags=j & 3, tag=(name,))
        check_dev(text, text_phase=phase, with_rec=False, tag=(name,))
        if j % 3 == 0:
            check_host(L, text, tag=(name,))
        if name.startswith("one header only"):
            assert (n, R) == (0, 1)
        if name.startswith("45 tiles"):
            kept, rt, rs = np_fasta(text)
            per_tile = np.bincount((np.flatnonzero(np_keep_mask(text)) + phase) // TILE, minlength=46)
            assert ((per_tile[1:46] >= 1) & (per_tile[1:46] <= 3)).all() and R == 45 and n == (TILE - phase - 1) + 90 + 6
        if name.startswith("a tile of dropped bytes only"):
            per_tile = np.bincount((np.flatnonzero(np_keep_mask(text)) + phase) // TILE, minlength=3)
            assert per_tile[0] % 32 != 0 and per_tile[1] == 0 and per_tile[2] > 0


def np_keep_mask(text):
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    line_start = np.r_[True, t[:-1] == NL]
    last = np.maximum.accumulate(np.where(line_start, np.arange(t.size), 0))
    return (t[last] != GT) & (t != NL) & (t != CR)


@gpu
def test_gpu_pointer_phases():
    """d_text at every byte phase 0..16 of its parent, poison '>' and line feeds just in front of and behind the view (check_dev
    plants them at every call); d_out and the record arrays at 8-B phases"""
    rng = np.random.default_rng(53)
    texts = [b">r1\n" + columns(rng, 3 * TILE + 77) + b">r2 x\r\n" + columns(rng, 500, eol=b"\r\n"), columns(rng, 100), random_text(rng, TILE + 40)]
    for text in texts:
        results = {check_dev(text, text_phase=phase, out_phase=phase % 3, flags=phase & 1) for phase in range(17)}
        assert len(results) == 1
    # the last line feed of the text makes no line start: the poison '>' behind it is no record
    assert POISON[(12 + 5) % 4][:1] == b">" and check_dev(b"ACGT\n", text_phase=12) == (4, 0)


@gpu
def test_gpu_capacities(L):
    """out_cap in {0, 1, 31, 32, 33, n-1, n} and rec_cap in {0, 1, R-1, R}: the counts stay full, the clipped last word is masked,
    nothing past the clipped extents is written; the host tier answers CNT_ECAP after the work"""
    rng = np.random.default_rng(54)
    big = b"".join(b">r%d\n" % r + columns(rng, int(rng.integers(1, 3000))) for r in range(12))
    for text in (big, small_fasta(rng, 900)):
        n, R = np_fasta(text)[0].size, np_fasta(text)[1].size
        assert n > 34 and R > 2
        for out_cap in (0, 1, 31, 32, 33, n - 1, n):
            for rec_cap in (0, 1, R - 1, R):
                check_dev(text, out_cap=out_cap, rec_cap=rec_cap, out_phase=out_cap & 1)
                check_host(L, text, out_cap=out_cap, rec_cap=rec_cap)
            check_dev(text, out_cap=out_cap, with_rec=False)
            check_host(L, text, out_cap=out_cap, with_rec=False, rec_cap=0)  # no record array: rec_cap is nothing to run out of


@gpu
def test_gpu_flags(L):
    rng = np.random.default_rng(55)
    text = b">r\nACGTNnacgtu7\x80\xff U>\r\n" + random_text(rng, TILE + 300, bytes(range(256)).replace(b"\n", b"")) + b"\n>s\nNNNN"
    invalid = set()
    for flags in (0, CNT_STRICT_LUT, CNT_ALLOW_N, CNT_STRICT_LUT | CNT_ALLOW_N):
        check_dev(text, flags=flags)
        check_host(L, text, flags=flags)
        invalid.add(expect(text, flags, 0, 0)[2])
    assert len(invalid) == 2
    kept = np_fasta(text)[0]
    assert not np.array_equal(np_words(kept, True), np_words(kept, False))


@gpu
def test_gpu_records_across_launch_seams(launch_tiles):
    """the lab build cut into launches of 64 / 128 tiles, 257 tiles: a header across every launch seam, a line feed | '>' on the
    next; the passes in several launches, counted in a captured graph"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(launch_tiles)
    tiles = 257
    n_len = (tiles - 1) * TILE + 4001
    t = bytearray(columns(rng, n_len)[:n_len])
    for j, e in enumerate(range(launch_tiles * TILE, n_len, launch_tiles * TILE)):
        if j % 2 == 0:
            t[e - 40 : e + 30] = b"\n>" + b"s" * 67 + b"\n"
        else:
            t[e - 1 : e + 5] = b"\n>ab\nA"
    text = bytes(t)
    n, R = check_dev(text, tag=(launch_tiles,))
    assert R == len(range(launch_tiles * TILE, n_len, launch_tiles * TILE))
    check_dev(text, out_cap=n // 2, with_rec=False, tag=(launch_tiles,))
    got_tiles, launches = fasta_plan(n_len, 0, launch_tiles)
    assert got_tiles == tiles and launches == 2 * -(-tiles // launch_tiles) + 2
    d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    out, rt, rs = (torch.empty(k, dtype=torch.int64, device="cuda") for k in (words_for(n_len), 100, 100))
    cnt, work = torch.empty(3, dtype=torch.int64, device="cuda"), torch.empty(po.fasta_to_bits_work_bytes(n_len), dtype=torch.uint8, device="cuda")
    assert _kernel_nodes_of(torch, lambda: po.fasta_to_bits_dev(d, out, cnt, work, rec_text=rt, rec_start=rs)) == launches


@gpu
def test_gpu_scan_round_edge():
    """just past the tiles one round of fasta_scan takes (1024 lanes of 16 tiles), with a header lying across that edge: a pattern
    of 64 lines tiled in front of and behind it, the expected result tiled from the numpy reference of the pattern"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(56)
    pattern = columns(rng, 64 * 60)
    kept = np_fasta(pattern)[0]
    assert len(pattern) == 3904 and kept.size == 3840
    r1 = (ROUND * TILE - TILE - 100) // len(pattern)
    header = b">" + b"h" * (ROUND * TILE + 2 * TILE + 50 - r1 * len(pattern) - 2) + b"\n"
    r2 = 40
    assert r1 * len(pattern) < (ROUND - 1) * TILE and r1 * len(pattern) + len(header) > (ROUND + 2) * TILE
    # the same construction at a size the numpy reference takes whole
    small = pattern * 3 + header[: 3 * TILE] + b"\n" + pattern * 2
    s_kept, s_rt, s_rs = np_fasta(small)
    assert s_kept.tobytes() == kept.tobytes() * 5 and s_rt.tolist() == [3 * len(pattern)] and s_rs.tolist() == [3 * kept.size]
    d_pat = torch.from_numpy(np.frombuffer(pattern, dtype=np.uint8).copy()).cuda()
    d_text = torch.cat([d_pat.repeat(r1), torch.from_numpy(np.frombuffer(header, dtype=np.uint8).copy()).cuda(), d_pat.repeat(r2)])
    n_len = d_text.numel()
    assert fasta_plan(n_len)[0] > ROUND + 2
    n = (r1 + r2) * kept.size
    out = torch.full((words_for(n) + PAD,), CANARY, dtype=torch.int64, device="cuda")
    rt, rs = (torch.full((4,), CANARY, dtype=torch.int64, device="cuda") for _ in range(2))
    cnt = torch.full((3,), CANARY, dtype=torch.int64, device="cuda")
    work = torch.empty(po.fasta_to_bits_work_bytes(n_len), dtype=torch.uint8, device="cuda")
    po.fasta_to_bits_dev(d_text, out[: words_for(n)], cnt, work, rec_text=rt, rec_start=rs, out_cap=n)
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tolist() == [n, 1, 0]
    assert rt.cpu().numpy().tolist() == [r1 * len(pattern)] + [CANARY] * 3 and rs.cpu().numpy().tolist() == [r1 * kept.size] + [CANARY] * 3
    d_want = torch.from_numpy(np_words(kept, False).view(np.int64)).cuda()
    assert bool((out[: words_for(n)].view(r1 + r2, d_want.numel()) == d_want).all()) and bool((out[words_for(n) :] == CANARY).all())


@gpu
def test_gpu_fasta_in_a_captured_graph_and_behind_a_side_stream():
    """one torch.cuda.graph capture of the call (with and without the record table, on the same scratch in turn) replayed twice on
    changed text; then the call enqueued on a side stream behind the copy that makes its input, no host sync in between"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(57)
    n_len = 9 * TILE + 1234
    text = torch.zeros(n_len, dtype=torch.uint8, device="cuda")
    outs = [torch.empty(words_for(n_len), dtype=torch.int64, device="cuda") for _ in range(2)]
    rt, rs = torch.empty(n_len, dtype=torch.int64, device="cuda"), torch.empty(n_len, dtype=torch.int64, device="cuda")
    cnts = torch.empty(6, dtype=torch.int64, device="cuda")
    work = torch.empty(po.fasta_to_bits_work_bytes(n_len), dtype=torch.uint8, device="cuda")

    def chain():
        po.fasta_to_bits_dev(text, outs[0], cnts[0:3], work, rec_text=rt, rec_start=rs)
        po.fasta_to_bits_dev(text, outs[1], cnts[3:6], work, strict_lut=True)

    def make(rep):
        body = b"".join(b">g%d %d\n" % (rep, r) + columns(rng, int(rng.integers(1, 9000)), letters=b"ACGTN") for r in range(40))
        return (body + b"A" * n_len)[:n_len]

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain()  # module load outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()

    def verify(t, strict_second, rep):
        n, R, invalid, want, want_rt, want_rs = expect(t, 0, n_len, n_len)
        assert cnts[0:3].cpu().numpy().tolist() == [n, R, invalid], rep
        assert np.array_equal(outs[0][: want.size].cpu().numpy().view(np.uint64), want), rep
        assert np.array_equal(rt[:R].cpu().numpy().view(np.uint64), want_rt) and np.array_equal(rs[:R].cpu().numpy().view(np.uint64), want_rs), rep
        if strict_second:
            assert cnts[3:6].cpu().numpy().tolist() == [n, R, invalid], rep
            assert np.array_equal(outs[1][: want.size].cpu().numpy().view(np.uint64), expect(t, CNT_STRICT_LUT, n_len, 0)[3]), rep

    for rep in range(2):
        t = make(rep)
        text.copy_(torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()))
        for x in outs + [rt, rs, cnts]:
            x.fill_(CANARY)
        work.fill_(0x77 + rep)  # the scratch needs no zeroing
        g.replay()
        torch.cuda.synchronize()
        verify(t, True, rep)
        assert (rt[int(cnts[1].item()) :].cpu().numpy() == CANARY).all()
    t = make(2)
    host = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).pin_memory()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        text.copy_(host, non_blocking=True)
        po.fasta_to_bits_dev(text, outs[0], cnts[0:3], work, rec_text=rt, rec_start=rs)
    torch.cuda.current_stream().wait_stream(side)
    verify(t, False, 2)


@gpu
def test_gpu_host_tier_pinned_and_pageable(L):
    """pinned host buffers (used in place: the plain stores and the merges of shared words go over the link) and pageable ones
    (staged); then the guess-and-retry wrapper on the real library"""
    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(58)
    sparse = b"".join(b">" + b"h" * (TILE - 6) + b"\nA\nC\n" for _ in range(6))  # tiles that share one output word, merged over the link
    for text in (b">a\n" + columns(rng, 3 * TILE + 77) + b">b\r\n" + columns(rng, 1000, eol=b"\r\n"), sparse, small_fasta(rng, 45)):
        n, R = np_fasta(text)[0].size, np_fasta(text)[1].size
        for pinned in (False, True):
            for out_cap, rec_cap in ((len(text), len(text)), (n, R), (max(n - 1, 0), R), (n, max(R - 1, 0))):
                for with_rec in (True, False):
                    check_host(L, text, out_cap=out_cap, rec_cap=rec_cap, with_rec=with_rec, pinned=pinned, flags=CNT_ALLOW_N)
    for text in (b">r\nA\n" * 3000, b">x\n" + columns(rng, 2 * TILE)):
        words, n, rec_text, rec_start, invalid = po.fasta_to_bits_hip(text)
        kept, rt, rs = np_fasta(text)
        assert n == kept.size and invalid == 0 and np.array_equal(words, np_words(kept, False)) and np.array_equal(rec_text, rt) and np.array_equal(rec_start, rs)
    assert po.fasta_names(b">r\nA\n" * 3, po.fasta_to_bits_hip(b">r\nA\n" * 3)[2]) == [b"r"] * 3


@gpu
def test_gpu_composition_with_subseq():
    """for each record, cnt_subseq_dev of the call's words at rec_start equals the plain encode of the record's own stripped lines"""
    import torch

    from cute_nucleotides_amd import n_to_bits as nb, packed_ops as po

    rng = np.random.default_rng(59)
    bodies = [columns(rng, int(k), eol=rng.choice([b"\n", b"\r\n"])) for k in (1, 61, 0, 5000, 33, 2 * TILE + 1, 32)]
    text = b"".join(b">rec %d\n" % r + body for r, body in enumerate(bodies))
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    out = torch.empty(words_for(len(text)), dtype=torch.int64, device="cuda")
    rt, rs = torch.empty(16, dtype=torch.int64, device="cuda"), torch.empty(16, dtype=torch.int64, device="cuda")
    cnt = torch.empty(3, dtype=torch.int64, device="cuda")
    work = torch.empty(po.fasta_to_bits_work_bytes(len(text)), dtype=torch.uint8, device="cuda")
    po.fasta_to_bits_dev(d_text, out, cnt, work, rec_text=rt, rec_start=rs)
    n, R, _ = cnt.cpu().numpy().tolist()
    assert R == len(bodies)
    starts = rs[:R].cpu().numpy().tolist() + [n]
    for r, body in enumerate(bodies):
        own = body.replace(b"\r", b"").replace(b"\n", b"")
        assert starts[r + 1] - starts[r] == len(own), r
        if not own:
            continue
        want = nb.n_to_bits_dev(torch.from_numpy(np.frombuffer(own, dtype=np.uint8).copy()).cuda())
        got = po.subseq_dev(out[: max(words_for(n), 1)], n, starts[r], len(own))
        assert torch.equal(got, want), r


@gpu
def test_gpu_fasta_fuzz(L):
    """200 random texts: random alphabet weights, header lengths up to several tiles, random capacities, flags and phases"""
    rng = np.random.default_rng(60)
    for case in range(200):
        kind = int(rng.integers(0, 4))
        n_len = int(rng.integers(1, 40001))
        if kind == 0:
            text = random_text(rng, n_len)
        elif kind == 1:
            text = small_fasta(rng, n_len)
        elif kind == 2:
            text = random_text(rng, n_len, b"ACGT" * int(rng.choice([1, 30, 2000])) + b">\n\r")
        else:
            parts, size = [], 0
            while size < n_len:
                p = (b">" + b"h" * int(rng.choice([0, 3, 100, TILE, 3 * TILE])) + b"\n") if rng.random() < 0.3 else columns(rng, int(rng.integers(1, 4000)), int(rng.choice([1, 60, 80])))
                parts.append(p)
                size += len(p)
            text = b"".join(parts)[:n_len]
        n, R = np_fasta(text)[0].size, np_fasta(text)[1].size
        out_cap = [n_len, n, max(n - 1, 0), int(rng.integers(0, n_len + 1)), int(rng.integers(0, n + 1))][int(rng.integers(0, 5))]
        rec_cap = [n_len, R, max(R - 1, 0), int(rng.integers(0, R + 1)), 0][int(rng.integers(0, 5))]
        flags = int(rng.integers(0, 4))
        check_dev(text, flags=flags, out_cap=out_cap, rec_cap=rec_cap, with_rec=bool(rng.integers(0, 4)), text_phase=int(rng.integers(0, 16)),
                  out_phase=int(rng.integers(0, 3)), tag=(case, kind))
        if case % 10 == 0:
            check_host(L, text, flags=flags, out_cap=out_cap, rec_cap=rec_cap, with_rec=bool(rng.integers(0, 2)), pinned=case % 20 == 0, tag=(case, kind))
