"""Open-reading-frame scan on packed words (include/cute_nt.h "ORF scan"): the stop-free runs of the three frame lanes of one
strand or of both, each trimmed to its start codon, ordered by the bound that closes the run.  Not in the reference, so the CPU
part pins three references against each other -- the definition as a literal scalar loop over the bounds of each lane, an
independent text-based six-frame scan (decode, reverse-complement the string, split each frame at the stop codons, find the
first ATG), and a vectorised numpy form -- checks the properties the definition implies, every argument error, the scratch
query, the Python layer, and the ISA and launch plan of the four kernels.  The GPU part compares both tiers entry by entry with
the numpy reference.  Random ACGT has a stop every ~21 codons and never exercises a carry, so the carry cases are random {A,C,G}
(no stop and no ATG on either strand: every such codon holds a T) with stops and starts planted at chosen positions."""
import ctypes
import os
import re
import sys
import time

import numpy as np
import pytest

from test_find_pattern import _set_codes, codes_of, words_of_codes
from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch
from test_kmers import assert_split_launches_by_max_tiles_per_launch
from test_minimizers import assert_counted_output_source
from test_translate import np_translate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNT_FIND_REVERSE = 0x100
CNT_ORF_BOTH_STRANDS = 0x200
CNT_ORF_OPEN_END = 0x400
CNT_ORF_NO_STOP = 0x800
TILE = 8192  # positions per workgroup tile (hip/orf_kernels.hpp kOrfTile)
NT = "ACTG"  # code order A0 C1 T2 G3
CODE = {ch: c for c, ch in enumerate(NT)}


def codon(s):
    return CODE[s[0]] | CODE[s[1]] << 2 | CODE[s[2]] << 4


STOPS = (1 << codon("TAA")) | (1 << codon("TGA")) | (1 << codon("TAG"))
ATG = 1 << codon("ATG")
assert STOPS == (1 << 2) | (1 << 14) | (1 << 50) and ATG == 1 << 56  # the header's constants
TAA, TAG, TGA, CAT, TTA = ([CODE[ch] for ch in s] for s in ("TAA", "TAG", "TGA", "CAT", "TTA"))
ATG_CODES = [CODE[ch] for ch in "ATG"]


def rc3(c):
    return ((c >> 4) | (c & 0xC) | ((c & 3) << 4)) ^ 0x2A


def rc3_set(mask):
    """the set whose test on c is the test of `mask` on rc3(c)"""
    return sum(1 << c for c in range(64) if (mask >> rc3(c)) & 1)


# ---- references -------------------------------------------------------------------------------------------------------
def def_orfs(s, stops, starts, min_len, both):
    """the definition, literally, on the codes s: per strand and lane the bounds, the runs between them, the ORF of each run;
    then the order.  Returns a list of (pos, length, info)."""
    n = len(s)
    if n < 3:
        return []
    c = [int(s[p]) | int(s[p + 1]) << 2 | int(s[p + 2]) << 4 for p in range(n - 2)]
    out = []
    for strand in (0, 1) if both else (0,):
        test = (lambda p: c[p]) if strand == 0 else (lambda p: rc3(c[p]))
        for lane in range(3):
            t = next(v for v in (n - 2, n - 1, n) if v % 3 == lane)
            bounds = [lane - 3] + [p for p in range(lane, n - 2, 3) if (stops >> test(p)) & 1] + [t]
            for lo, hi in zip(bounds, bounds[1:]):
                if starts == 0:
                    pos, length = lo + 3, hi - lo - 3
                else:
                    a = [p for p in range(lo + 3, hi, 3) if (starts >> test(p)) & 1]
                    if not a:
                        continue
                    pos, length = (a[0], hi - a[0]) if strand == 0 else (lo + 3, a[-1] + 3 - (lo + 3))
                if length < 3 or length < min_len:
                    continue
                opening, closing = (lo, hi) if strand == 0 else (hi, lo)
                info = (pos % 3 if strand == 0 else (n - pos - length) % 3) | (CNT_FIND_REVERSE if strand else 0)
                info |= (CNT_ORF_OPEN_END if opening in (lane - 3, t) else 0) | (CNT_ORF_NO_STOP if closing in (lane - 3, t) else 0)
                out.append((hi, strand, pos, length, info))
    out.sort(key=lambda e: (e[0], e[1]))
    return [e[2:] for e in out]


def text_orfs(s, with_atg, min_len, both):
    """an independent scan on text, standard stops: every frame of the string (and of its reverse complement) split at the stop
    codons, each piece trimmed to its first ATG; coordinates mapped back to the forward strand.  Returns a SET of (pos, length,
    strand, frame, open_end, no_stop)."""
    text = "".join(NT[int(x)] for x in s)
    n = len(text)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    found = set()
    for strand in (0, 1) if both else (0,):
        t = text if strand == 0 else "".join(comp[ch] for ch in reversed(text))
        for frame in range(3):
            codons = [t[i : i + 3] for i in range(frame, n - 2, 3)]
            piece_start, first = 0, True  # a piece is codons [piece_start, j)
            for j in range(len(codons) + 1):
                at_end = j == len(codons)
                if not at_end and codons[j] not in ("TAA", "TAG", "TGA"):
                    continue
                piece = codons[piece_start:j]
                k = piece.index("ATG") if with_atg and "ATG" in piece else (None if with_atg else 0)
                if k is not None and len(piece) - k >= 1:
                    b, e = frame + 3 * (piece_start + k), frame + 3 * j  # [b, e) on the strand as read
                    length = e - b
                    if length >= 3 and length >= min_len:
                        pos = b if strand == 0 else n - e
                        found.add((pos, length, strand, frame, first, at_end))
                piece_start, first = j + 1, False
    return found


def as_set(entries, n):
    """(pos, length, info) entries in text_orfs's form"""
    return {(p, l, (i >> 8) & 1, i & 3, bool(i & CNT_ORF_OPEN_END), bool(i & CNT_ORF_NO_STOP)) for p, l, i in entries}


def sites_of(c, stops, starts, both, first=0):
    """the stop and start positions of each strand scanned, ascending int64, from the codon values c of positions first + j"""
    c = np.asarray(c).astype(np.uint64)
    out = []
    for strand in (0, 1) if both else (0,):
        sm, am = (stops, starts) if strand == 0 else (rc3_set(stops), rc3_set(starts))
        out.append((np.flatnonzero((np.uint64(sm) >> c) & np.uint64(1)).astype(np.int64) + first,
                    np.flatnonzero((np.uint64(am) >> c) & np.uint64(1)).astype(np.int64) + first))
    return out


def orfs_from_sites(n, sites, have_starts, min_len):
    """the entries of a sequence of n nucleotides whose stops and starts are the positions sites[strand] = (stops, starts): the
    definition on sorted position arrays.  Returns uint64 (pos, length, info)."""
    if n < 3:
        return tuple(np.empty(0, dtype=np.uint64) for _ in range(3))
    parts = []
    for strand, (sp, ap) in enumerate(sites):
        for lane in range(3):
            t = next(v for v in (n - 2, n - 1, n) if v % 3 == lane)
            bounds = np.concatenate([[lane - 3], sp[sp % 3 == lane], [t]]).astype(np.int64)
            lo, hi = bounds[:-1], bounds[1:]
            if have_starts:
                a = ap[ap % 3 == lane]
                if strand == 0:
                    j = np.searchsorted(a, lo, side="right")  # the first start behind lo
                    ok = j < a.size
                    at = a[np.minimum(j, max(a.size - 1, 0))] if a.size else np.zeros_like(lo)
                    ok &= at < hi
                    pos, length = at, hi - at
                else:
                    j = np.searchsorted(a, hi, side="left") - 1  # the last start in front of hi
                    ok = j >= 0
                    at = a[np.maximum(j, 0)] if a.size else np.zeros_like(lo)
                    ok &= at > lo
                    pos, length = lo + 3, at - lo
            else:
                ok, pos, length = np.ones(lo.size, dtype=bool), lo + 3, hi - lo - 3
            ok &= (length >= 3) & (length >= min_len)
            lo_end, hi_end = lo < 0, hi >= n - 2
            frame = np.full(lo.size, lane if strand == 0 else (n - lane) % 3, dtype=np.int64)  # reverse: pos + length = lane (mod 3)
            opening, closing = (lo_end, hi_end) if strand == 0 else (hi_end, lo_end)
            info = frame | (CNT_FIND_REVERSE if strand else 0) | np.where(opening, CNT_ORF_OPEN_END, 0) | np.where(closing, CNT_ORF_NO_STOP, 0)
            parts.append((2 * hi[ok] + strand, pos[ok], length[ok], info[ok]))
    key = np.concatenate([p[0] for p in parts])
    order = np.argsort(key, kind="stable")
    return tuple(np.concatenate([p[j] for p in parts])[order].astype(np.uint64) for j in (1, 2, 3))


def codons_of(s):
    s = np.asarray(s).astype(np.int64)
    return s[:-2] | s[1:-1] << 2 | s[2:] << 4 if s.size >= 3 else np.empty(0, dtype=np.int64)


def np_orfs(s, stops, starts, min_len, both):
    """the vectorised reference on the codes s"""
    return orfs_from_sites(len(s), sites_of(codons_of(s), stops, starts, both), starts != 0, min_len)


def ref_orfs(words, n, stops, starts, min_len, both):
    return np_orfs(codes_of(words, n), stops, starts, min_len, both)


def acg(rng, n):
    """random {A, C, G}: no stop codon and no ATG on either strand"""
    return np.array([0, 1, 3], dtype=np.uint8)[rng.integers(0, 3, n)]


def plant(s, at, codes):
    """the codon `codes` at position `at`, with a G in front and CC behind: none of the codons that overlap the plant is a stop or
    a start of either strand but the planted one (clipped to the sequence; the references take whatever comes of that)"""
    for j, c in enumerate([3] + list(codes) + [1, 1]):
        if 0 <= at - 1 + j < len(s):
            s[at - 1 + j] = c


# ---- CPU: the references ----------------------------------------------------------------------------------------------
def test_references_against_an_independent_text_scan():
    rng = np.random.default_rng(77)
    seen = 0
    for it in range(1200):
        n = int(rng.integers(0, 81))
        s = rng.integers(0, 4, n).astype(np.uint8)
        if it % 3 == 0:  # a stop-poor sequence: long runs, open ends
            s = acg(rng, n)
            for _ in range(int(rng.integers(0, 4))):
                at = int(rng.integers(0, max(n - 2, 1)))
                s[at : at + 3] = [TAA, TAG, TGA, ATG_CODES, CAT, TTA][int(rng.integers(0, 6))][: n - at]
        for with_atg in (False, True):
            for both in (False, True):
                min_len = int(rng.choice([0, 0, 3, 6, rng.integers(0, 40)]))
                got = def_orfs(s, STOPS, ATG if with_atg else 0, min_len, both)
                assert as_set(got, n) == text_orfs(s, with_atg, min_len, both), (it, n, with_atg, both, min_len)
                assert len(set(got)) == len(got)
                vec = np_orfs(s, STOPS, ATG if with_atg else 0, min_len, both)
                assert [tuple(int(v) for v in e) for e in zip(*vec)] == got, (it, n, with_atg, both, min_len)
                seen += len(got)
    assert seen > 5000


def test_numpy_reference_against_the_definition_with_custom_sets():
    """sets that overlap their own rc3 image, starts that are stops, one-codon sets"""
    rng = np.random.default_rng(78)
    for it in range(300):
        n = int(rng.integers(0, 120))
        s = rng.integers(0, 4, n).astype(np.uint8)
        stops = int(rng.integers(1, 2**63)) & int(rng.integers(1, 2**63)) & int(rng.integers(1, 2**63)) or 1
        starts = int(rng.choice([0, int(rng.integers(1, 2**63)) & int(rng.integers(1, 2**63)), stops]))
        for both in (False, True):
            min_len = int(rng.choice([0, 3, 9]))
            want = def_orfs(s, stops, starts, min_len, both)
            vec = np_orfs(s, stops, starts, min_len, both)
            assert [tuple(int(v) for v in e) for e in zip(*vec)] == want, (it, n, hex(stops), hex(starts), both)


def test_properties(oracle):
    rng = np.random.default_rng(12)
    comp = np.array([2, 3, 0, 1], dtype=np.uint8)  # code ^ 2
    for it in range(30):
        n = int(rng.integers(300, 900))
        s = rng.integers(0, 4, n).astype(np.uint8)
        for starts in (0, ATG):
            # strand symmetry: the ORFs of revcomp(s) are those of s under pos -> n - pos - length and the other strand
            a = np_orfs(s, STOPS, starts, 0, True)
            b = np_orfs(comp[s[::-1]], STOPS, starts, 0, True)
            sa = sorted((int(p), int(l), int(i)) for p, l, i in zip(*a))
            sb = sorted((n - int(p) - int(l), int(l), int(i) ^ CNT_FIND_REVERSE) for p, l, i in zip(*b))
            assert sa == sb and len(sa) >= 1, (it, starts)
            # one strand is the forward entries of both
            f = np_orfs(s, STOPS, starts, 0, False)
            keep = (a[2] & np.uint64(CNT_FIND_REVERSE)) == 0
            assert all(np.array_equal(x, y[keep]) for x, y in zip(f, a))
            # every ORF translates to a protein with no stop inside, beginning with M when trimmed, followed by a stop unless
            # CNT_ORF_NO_STOP is set; the frame is the one of cnt_translate's six frames
            words = words_of_codes(oracle, s)
            for p, l, i in zip(*(x.astype(np.int64) for x in a)):
                rev = bool(i & CNT_FIND_REVERSE)
                prot = bytes(np_translate(words, n, int(p), int(l), rev))
                assert b"*" not in prot and len(prot) == l // 3 and l % 3 == 0
                assert not starts or prot[:1] == b"M"
                frame = int(i) & 3
                assert frame == (p % 3 if not rev else (n - p - l) % 3)
                if i & CNT_ORF_NO_STOP:
                    assert (p < 3) if rev else (p + l > n - 3)
                else:
                    after = np_translate(words, n, int(p) - 3, 3, True) if rev else np_translate(words, n, int(p + l), 3, False)
                    assert bytes(after) == b"*"
            # min_len filters and nothing else
            for min_len in (4, 30, 90):
                g = np_orfs(s, STOPS, starts, min_len, True)
                k2 = a[1] >= min_len
                assert all(np.array_equal(x, y[k2]) for x, y in zip(g, a))
            # with starts == 0 the order is pos + length ascending
            if not starts:
                assert (np.diff((a[0] + a[1]).astype(np.int64)) >= 0).all()


# ---- CPU: the Python layer and the ABI ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


def test_python_wrappers_raise_value_error(L):
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import packed_ops as po

    assert cn.orfs_hip is po.orfs_hip and cn.orfs_dev is po.orfs_dev and cn.orfs_work_bytes is po.orfs_work_bytes and cn.codon_set is po.codon_set
    assert po.codon_set(["TAA", "tga", b"UAG"]) == STOPS and po.codon_set(["ATG"]) == ATG and po.codon_set([]) == 0
    w = np.zeros(2, dtype=np.uint64)
    for bad in (["TA"], ["TAAA"], ["TAN"], [5], "TAA", b"TAA"):
        with pytest.raises(ValueError):
            po.codon_set(bad)
    for kw in (dict(stops=0), dict(stops=[]), dict(stops=-1), dict(stops=1 << 64), dict(starts=-1), dict(starts=1 << 64), dict(starts=["AT"]), dict(min_len=-1)):
        with pytest.raises(ValueError):
            po.orfs_hip(w, 64, **kw)
    with pytest.raises(ValueError):
        po.orfs_hip(w, 65)  # longer than the words hold
    pos, length, info = po.orfs_hip(w, 2, both_strands=True)  # no codon: answered without a device
    assert pos.size == 0 and length.size == 0 and info.size == 0
    pos, length, info = po.orfs_hip(w, 0, stops=["TAA"], starts=None, info=False)
    assert pos.size == 0 and info is None
    assert po.orfs_work_bytes(2) == 0


def _work_bytes(L, n_len):
    out = ctypes.c_size_t(12345)
    assert L.cnt_orfs_work_bytes(n_len, ctypes.byref(out)) == 0
    return out.value


def orf_tiles(n_len):
    return n_len // TILE + 1 if n_len >= 3 else 0


def test_work_bytes_query(L):
    from cute_nucleotides_amd import _lib
    from cute_nucleotides_amd import packed_ops as po

    assert [_work_bytes(L, n) for n in (0, 1, 2)] == [0, 0, 0]
    assert _work_bytes(L, 3) == 16 + 2 * 8 + 16 * 4 + 6 * (4 + 16)  # one tile: one group of 16 tiles, six pairs of (value, carry)
    last = 0
    for n_len in (3, TILE - 1, TILE, TILE + 1, 5 * TILE, 16 * TILE - 1, 16 * TILE, 33 * 16 * TILE, (1 << 32) + 1, 1 << 36):
        tiles = orf_tiles(n_len)
        groups = -(-tiles // 16)
        want = 16 + (groups + groups % 2) * 8 + groups * 16 * 4 + tiles * 6 * 20
        assert _work_bytes(L, n_len) == want == po.orfs_work_bytes(n_len), n_len
        assert want >= last  # monotone
        last = want
    assert (1 << 36) // 128 < last < (1 << 36) // 32  # 2^36 nt: about 1 GiB, no overflow
    assert L.cnt_orfs_work_bytes(100, None) == _lib.CNT_EINVAL


def test_abi_errors_come_before_any_device_work(L):
    from cute_nucleotides_amd import _lib

    buf = np.zeros(4096, dtype=np.uint64)
    q = lambda word, byte=0: ctypes.c_void_p(buf.ctypes.data + 8 * word + byte)  # noqa: E731
    out = np.full(768, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    o = lambda word, byte=0: ctypes.c_void_p(out.ctypes.data + 8 * word + byte)  # noqa: E731
    cnt = np.full(2, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    c = lambda byte=0: ctypes.c_void_p(cnt.ctypes.data + byte)  # noqa: E731
    work = q(3000)
    need = _work_bytes(L, 100)
    assert need == 216
    for dev in (False, True):
        def call(bits, n_len, stops, starts, min_len, flags, pos, length, info, cap, count, work_bytes=need, wk=work):
            if dev:
                return L.cnt_orfs_dev(bits, n_len, stops, starts, min_len, flags, pos, length, info, cap, count, wk, work_bytes, None)
            return L.cnt_orfs(bits, n_len, stops, starts, min_len, flags, pos, length, info, cap, count)

        tag = "dev" if dev else "host"
        ok = (q(0), 100, STOPS, ATG, 0, 0, o(0), o(200), o(400), 64, c())
        # stops == 0 or an unknown flag -- even without work
        assert call(q(0), 100, 0, ATG, 0, 0, *ok[6:]) == _lib.CNT_EINVAL
        assert call(None, 0, 0, 0, 0, 0, None, None, None, 0, None) == _lib.CNT_EINVAL
        for flags in (0x1, 0x2, 0x20, 0x40, 0x80, 0x100, 0x400, 0x800, 0x80000000, CNT_ORF_BOTH_STRANDS | 0x1):
            assert call(*ok[:5], flags, *ok[6:]) == _lib.CNT_EINVAL, (tag, flags)
            assert call(None, 0, STOPS, 0, 0, flags, None, None, None, 0, None) == _lib.CNT_EINVAL, (tag, flags)
        # NULL bits, pos, length or count when len >= 3 (info may be NULL)
        assert call(None, *ok[1:]) == _lib.CNT_EINVAL
        assert call(*ok[:6], None, *ok[7:]) == _lib.CNT_EINVAL
        assert call(*ok[:7], None, *ok[8:]) == _lib.CNT_EINVAL
        assert call(*ok[:10], None) == _lib.CNT_EINVAL
        # not 8-B aligned
        for byte in (1, 4, 7):
            assert call(q(0, byte), *ok[1:]) == _lib.CNT_EINVAL
            assert call(*ok[:6], o(0, byte), *ok[7:]) == _lib.CNT_EINVAL
            assert call(*ok[:7], o(200, byte), *ok[8:]) == _lib.CNT_EINVAL
            assert call(*ok[:8], o(400, byte), *ok[9:]) == _lib.CNT_EINVAL
            assert call(*ok[:10], c(byte)) == _lib.CNT_EINVAL
        # an output overlapping the input words (100 nt = 4 words at q(10)) or another output (64 entries each)
        for ow in (10, 12, 13, 8, 0):
            assert call(q(10), *ok[1:6], q(ow), o(200), o(400), 64, c()) == _lib.CNT_EINVAL, (tag, ow)
            assert call(q(10), *ok[1:6], o(0), q(ow), o(400), 64, c()) == _lib.CNT_EINVAL, (tag, ow)
            assert call(q(10), *ok[1:6], o(0), o(200), q(ow), 64, c()) == _lib.CNT_EINVAL, (tag, ow)
        for w2 in (0, 63, 30):
            assert call(q(10), *ok[1:6], o(0), o(w2), o(400), 64, c()) == _lib.CNT_EINVAL, (tag, w2)
            assert call(q(10), *ok[1:6], o(0), o(200), o(w2), 64, c()) == _lib.CNT_EINVAL, (tag, w2)
            assert call(q(10), *ok[1:6], o(0), o(200), o(200 + w2), 64, c()) == _lib.CNT_EINVAL, (tag, w2)
        if dev:
            assert call(q(10), *ok[1:], work_bytes=need - 1) == _lib.CNT_EINVAL  # scratch below the query
            assert call(q(10), *ok[1:], work_bytes=0) == _lib.CNT_EINVAL
            assert call(q(10), *ok[1:], wk=None) == _lib.CNT_EINVAL
        # len < 3: CNT_OK without a device, count set to 0 on the host tier (NULL pointers allowed)
        for n_len in (0, 1, 2):
            assert call(None, n_len, STOPS, ATG, 0, CNT_ORF_BOTH_STRANDS, None, None, None, 0, None, 0, None) == _lib.CNT_OK
            if not dev:
                cnt[0] = 99
                assert call(q(0), n_len, STOPS, 0, 0, 0, o(0), o(200), None, 64, c()) == _lib.CNT_OK and cnt[0] == 0
                cnt[0] = 0x5A5A5A5A5A5A5A5A
    assert (out == 0x5A5A5A5A5A5A5A5A).all()  # nothing was written
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        assert L.cnt_orfs(q(0), 100, STOPS, ATG, 0, 0, o(0), o(200), o(400), 64, c()) == _lib.CNT_ENODEV
        assert L.cnt_orfs_dev(q(0), 100, STOPS, ATG, 0, 0, o(0), o(200), None, 64, c(), work, need, None) < 0
        assert (out == 0x5A5A5A5A5A5A5A5A).all()


def test_abi_wiring(L):
    import subprocess

    from cute_nucleotides_amd import _lib

    names = ("cnt_orfs", "cnt_orfs_dev", "cnt_orfs_work_bytes")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(L, name) and name in exported and name + "(" in header
    for line in ("#define CNT_ORF_BOTH_STRANDS 0x200u", "#define CNT_ORF_OPEN_END 0x400u", "#define CNT_ORF_NO_STOP 0x800u",
                 "#define CNT_ORF_STOPS_STANDARD ((1ull << 2) | (1ull << 14) | (1ull << 50))", "#define CNT_ORF_STARTS_ATG (1ull << 56)"):
        assert line in header, line
    assert (_lib.CNT_ORF_BOTH_STRANDS, _lib.CNT_ORF_OPEN_END, _lib.CNT_ORF_NO_STOP) == (CNT_ORF_BOTH_STRANDS, CNT_ORF_OPEN_END, CNT_ORF_NO_STOP)
    assert (_lib.CNT_ORF_STOPS_STANDARD, _lib.CNT_ORF_STARTS_ATG) == (STOPS, ATG)
    section = header.split("/* ORF scan:")[1].split("cnt_orfs_work_bytes(size_t")[0].lower()
    for words in ("SET to n", "forward before reverse at equal hi", "never walked to", "CNT_ECAP"):
        assert words.lower() in section, words
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    for sig in (r"pub fn orfs_hip\(bits: &\[u64\], len: usize, stops: u64, starts: u64, min_len: usize, both_strands: bool\) -> \(Vec<u64>, Vec<u64>, Vec<u64>\) \{",
                r"pub fn orfs_hip_dev\(", r"pub fn orfs_work_bytes\(len: usize\) -> usize \{"):
        assert re.search(sig, rust), sig
    cpp = open(os.path.join(ROOT, "cute_nucleotides_amd", "cute_nucleotides.hpp")).read()
    assert "inline Orfs orfs_hip(" in cpp and "inline void orfs_hip_dev(" in cpp


# ---- CPU: the ISA and the launch plan ---------------------------------------------------------------------------------------
ORF_KERNELS = ["orf_summary", "orf_carry", "orf_count", "orf_write"]


def test_orf_kernels_isa():
    """the four kernels from the product's gfx950 assembly: no scratch, no spills, registers and static LDS within the bounds
    read off the build (38 / 33 / 40 / 52 VGPRs; 352 / 256 / 464 / 472 B of LDS: the table, the waves' values, the carry-in),
    no dynamic LDS (the launcher passes none), and no templated kernel added to the product"""
    sys.path.insert(0, os.path.join(ROOT, "bench"))
    import isa_digest

    asm = isa_digest.assembly()
    for name in ORF_KERNELS:
        m = re.search(r"^cnt::%s\(.*?\): +; @(.*?)\.end_amdhsa_kernel" % name, asm, re.S | re.M)
        assert m, name + " not in the product's assembly"
        text = m.group(1)
        assert "scratch_" not in text, name
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", text), name
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", text).group(1))
        assert lds <= 512, (name, lds)
        assert int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", text).group(1)) <= 64, name
        meta = re.search(r"\.name:\s+cnt::%s\(.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)" % name, asm, re.S)
        assert meta and meta.group(1) == "0" and meta.group(2) == "0", (name, meta and meta.groups())
        block = re.search(r"\.name:\s+cnt::%s\(.*?\.wavefront_size" % name, asm, re.S).group(0)
        assert re.search(r"\.uses_dynamic_stack:\s+false", block) and "dynamic_lds" not in block, name
    abi = open(os.path.join(ROOT, "hip", "orf_abi.inc")).read()
    assert abi.count("counted_scan_enqueue(") == 1  # the scan's launch is the one in counted_output.hpp
    abi += open(os.path.join(ROOT, "hip", "counted_output.hpp")).read()
    launches = re.findall(r"hipLaunchKernelGGL\((\w+), dim3\([^;]*?\), dim3\(\w+\), (\w+), s,", abi)
    assert sorted(k for k, _ in launches) == sorted(ORF_KERNELS + ["counted_scan"]) and all(lds == "0" for _, lds in launches)
    assert len(isa_digest.kernels(asm)) < 60  # the product's templated kernels: none added


ORF_HW_LAUNCH_TILES = ((0x7FFFFFFF // 256) // 64) * 64  # max_tiles_per_launch(256) of the product build


def orf_plan(n_len, launch_tiles=ORF_HW_LAUNCH_TILES):
    """(tiles, kernel launches) of a device call: len / 8192 + 1 tiles (the positions 0 .. len), three tile passes in
    ceil(tiles / launch_tiles) launches each, the carry pass and the offset scan; len < 3: no kernel (a memset of the count)"""
    tiles = orf_tiles(n_len)
    return tiles, (3 * -(-tiles // launch_tiles) + 2) if tiles else 0


def test_orf_plan_matches_the_launcher_and_splitter_source():
    src = open(os.path.join(ROOT, "hip", "orf_kernels.hpp")).read()
    assert "constexpr int kOrfBlock = 256;" in src and "kOrfTileWords = kOrfBlock, kOrfTile = 32 * kOrfTileWords;" in src
    assert "constexpr int kOrfPairs = 6;" in src
    abi = open(os.path.join(ROOT, "hip", "orf_abi.inc")).read()
    scan = "counted_scan_enqueue(work, n_tiles, d_count, s);"
    carry = "hipLaunchKernelGGL(orf_carry, dim3(both ? kOrfPairs : 3), dim3(kOrfCarryBlock), 0, s, sums, carry, n_tiles);"
    for line in ("uint64_t orf_tiles(size_t len) { return len < 3 ? 0 : (uint64_t)len / kOrfTile + 1; }", scan, carry,
                 "if (len < 3) return counted_empty_dev(d_count, s);", "const uint64_t n_tiles = orf_tiles(len);",
                 "const CountedScratch work = counted_carve(d_work, n_tiles);",
                 "uint64_t orf_work_bytes(uint64_t n_tiles) { return counted_scratch_bytes(n_tiles) + n_tiles * kOrfPairs * (4 + 2 * 8); }"):
        assert line in abi, line
    assert_counted_output_source()
    shared = open(os.path.join(ROOT, "hip", "counted_output.hpp")).read()
    assert "return 16 + ((groups + 1) & ~1ull) * 8 + groups * kCountedGroup * 4;" in shared
    tiles = "split_launches(n_tiles, kOrfBlock, [&](uint64_t t, uint64_t n) { hipLaunchKernelGGL(orf_%s, dim3((unsigned)n), dim3(kOrfBlock), 0, s, a, t); });"
    at = [abi.index(tiles % k) for k in ("summary", "count", "write")]
    assert abi.count("split_launches(") == 3 and at[0] < abi.index(carry) < at[1] < abi.index(scan) < at[2]
    assert_split_launches_by_max_tiles_per_launch()
    assert ORF_HW_LAUNCH_TILES == 8388544
    assert orf_plan(2) == (0, 0) and orf_plan(3) == (1, 5) and orf_plan(TILE - 1) == (1, 5) and orf_plan(TILE) == (2, 5)
    assert orf_plan((1 << 32) + 33) == (524289, 5) and orf_plan(1 << 36) == ((1 << 23) + 1, 8)
    assert orf_plan(64 * TILE * 3 + 22, 64) == (193, 14) and orf_plan(64 * TILE * 3 - 1, 64) == (192, 11)


# ---------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
SENTINEL = -0x3C3C3C3C3C3C3C3D
HOST_SENTINEL = 0xDEADBEEFDEADBEEF


def _host_call(L, bits, n_len, stops, starts, min_len, both, pos, length, info, cap):
    n = ctypes.c_uint64(0xDEAD)
    rc = L.cnt_orfs(bits.ctypes.data, n_len, stops, starts, min_len, CNT_ORF_BOTH_STRANDS if both else 0, pos.ctypes.data, length.ctypes.data,
                    info.ctypes.data if info is not None else None, cap, ctypes.byref(n))
    return rc, n.value


def _dev_result(pos, length, info, count):
    n = int(count.item())
    return (n,) + tuple(t[:n].cpu().numpy().view(np.uint64) if t is not None else None for t in (pos, length, info))


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def check_both_tiers(oracle, s, stops, starts, min_len, both, tag, rng=None, phase=0, host=True):
    """both tiers on the codes s against the numpy reference; returns the reference"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    n_len = len(s)
    pre = rng.integers(0, 2**64, phase, dtype=np.uint64) if phase else np.zeros(0, dtype=np.uint64)
    allw = np.concatenate([pre, words_of_codes(oracle, s, extra=2, rng=rng)])
    nw = max((n_len + 31) // 32, 1)
    src = allw[phase : phase + nw]
    want = np_orfs(s, stops, starts, min_len, both)
    dall = torch.from_numpy(allw.view(np.int64)).cuda()
    got = _dev_result(*po.orfs_dev(dall[phase : phase + nw], n_len, stops, starts, min_len, both_strands=both))
    assert got[0] == want[0].size and _same(got[1:], want), tag + ("device", got[0], want[0].size)
    if host:
        assert _same(po.orfs_hip(np.ascontiguousarray(src), n_len, stops, starts, min_len, both_strands=both), want), tag + ("host",)
    return want


@gpu
def test_gpu_short_lengths_both_tiers(oracle):
    """every length 0 .. 70 of random ACGT, whole runs and ATG-trimmed, one strand and both"""
    rng = np.random.default_rng(1)
    total = 0
    for n_len in range(71):
        s = rng.integers(0, 4, n_len).astype(np.uint8)
        for starts in (0, ATG):
            for both in (False, True):
                total += check_both_tiers(oracle, s, STOPS, starts, 0, both, (n_len, starts, both), rng=rng, phase=n_len % 3, host=n_len % 4 == 0)[0].size
    assert total > 500


@gpu
def test_gpu_stops_straddling_tile_edges(oracle):
    """lengths T-3 .. T+3, 2T +- 2 and 3T + 1: a stop codon of either strand planted at offsets -2, -1 and 0 of each tile
    boundary (its three nucleotides straddle the boundary; the three offsets are the three lanes), starts of both strands in
    front of it in the same lane"""
    rng = np.random.default_rng(2)
    lengths = [TILE + d for d in range(-3, 4)] + [2 * TILE - 2, 2 * TILE + 2, 3 * TILE + 1]
    emitted = 0
    for n_len in lengths:
        for off in (-2, -1, 0):
            for stop in (TAA, TTA):  # a forward stop, a reverse stop (TAA read on the reverse strand)
                s = acg(rng, n_len)
                for b in range(TILE, n_len + 3, TILE):
                    plant(s, b + off, stop)
                    plant(s, b + off - 60, ATG_CODES)
                    plant(s, b + off - 90, CAT)
                    plant(s, b + off - 3000, stop)  # and a stop deep inside the tile, same lane
                for starts in (0, ATG):
                    for both in (False, True):
                        want = check_both_tiers(oracle, s, STOPS, starts, 0, both, (n_len, off, stop, starts, both), rng=rng, host=False)
                        emitted += want[0].size
                        if n_len >= TILE + 3 and (both or stop is TAA):  # the bound at the boundary emitted an entry
                            his = (want[0] + want[1]).astype(np.int64) if not starts else None
                            assert his is None or (TILE + off) in his.tolist(), (n_len, off, stop, both)
    assert emitted > 400


def _carry_case(rng, n_len, plants):
    s = acg(rng, n_len)
    for at, codes in plants:
        plant(s, at, codes)
    return s


@gpu
def test_gpu_runs_carried_across_tiles(oracle):
    """5 tiles whose tiles 1-3 hold no stop on either strand: a start in tile 0 and a stop in tile 4; the only start in tile 2;
    and one lane stop-free over the whole sequence -- one entry with both CNT_ORF_OPEN_END and CNT_ORF_NO_STOP"""
    rng = np.random.default_rng(3)
    n_len = 5 * TILE - 7
    for lane in range(3):
        a0, z4 = 3 * 700 + lane, 4 * TILE + 3 * 500 + (lane - 4 * TILE) % 3
        a2 = 2 * TILE + 3 * 1000 + (lane - 2 * TILE) % 3
        assert a0 % 3 == a2 % 3 == z4 % 3 == lane
        cases = {
            "start in tile 0": [(3 * 100 + lane, TAA), (a0, ATG_CODES), (z4, TAA)],
            "start in tile 2": [(3 * 100 + lane, TAA), (a2, ATG_CODES), (z4, TAA)],
            "reverse, start in tile 4": [(3 * 100 + lane, TTA), (z4 - 300, CAT), (z4, TTA)],
            "reverse, start in tile 2": [(3 * 100 + lane, TTA), (a2, CAT), (z4, TTA)],
            "two starts: the first forward, the last reverse": [(3 * 100 + lane, TAA), (3 * 101 + lane, TTA), (a0, ATG_CODES), (a0 + 3, CAT), (a2, ATG_CODES), (a2 + 3, CAT),
                                                               (z4, TAA), (z4 + 3, TTA)],
            "no stop at all": [(a2, ATG_CODES), (a2 + 300, CAT)],
        }
        for name, plants in cases.items():
            s = _carry_case(rng, n_len, plants)
            for starts in (0, ATG):
                for both in (False, True):
                    want = check_both_tiers(oracle, s, STOPS, starts, 300, both, (lane, name, starts, both), rng=rng, host=starts == ATG and both)
                    long = want[1].astype(np.int64) > TILE  # across at least one whole tile
                    if name == "no stop at all":
                        if not starts:  # every lane runs from end to end
                            both_ends = (want[2] & np.uint64(CNT_ORF_OPEN_END | CNT_ORF_NO_STOP)) == CNT_ORF_OPEN_END | CNT_ORF_NO_STOP
                            assert both_ends.all() and want[0].size == (6 if both else 3) and long.all()
                    elif name.startswith("reverse"):
                        assert long.sum() >= (1 if both else 0) + (0 if starts else 1), (lane, name, starts, both)
                    else:
                        assert long.sum() >= 1, (lane, name, starts, both)
                    if name == "start in tile 2" and starts:
                        assert a2 in want[0].tolist()
                    if name == "reverse, start in tile 2" and starts and both:
                        k = want[0].tolist().index(3 * 100 + lane + 3)
                        assert int(want[1][k]) == a2 + 3 - (3 * 100 + lane + 3) and int(want[2][k]) & CNT_FIND_REVERSE


@gpu
@pytest.mark.parametrize("both", [False, True])
def test_gpu_runs_across_launch_edges(oracle, launch_tiles, both):
    """the lab build cut into launches of 64 / 128 tiles, 3 launches of tiles + 22 nt: sparse stops so that a run crosses every
    launch boundary, in every lane; the passes in several launches, counted in a captured graph"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(launch_tiles)
    n_len = launch_tiles * TILE * 3 + 22
    s = acg(rng, n_len)
    edges = [launch_tiles * TILE * j for j in (1, 2, 3)]
    for j, e in enumerate(edges):
        for lane in range(3):
            lo, hi = e - 3 * (5000 + 11 * lane) - (e - lane) % 3, e + 3 * (7000 + 13 * lane) + (lane - e) % 3
            assert lo % 3 == hi % 3 == lane and lo < e < hi
            if hi + 3 > n_len:
                hi = lo + 3 * ((n_len - 3 - lo) // 3)
            plant(s, lo, TAA if (j + lane) % 2 == 0 else TTA)
            plant(s, hi, TAA if (j + lane) % 2 == 0 else TTA)
            plant(s, lo + 3 * 40, ATG_CODES)
            plant(s, hi - 3 * 40, CAT)
    src = words_of_codes(oracle, s, rng=rng)
    dsrc = torch.from_numpy(src.view(np.int64)).cuda()
    tiles, launches = orf_plan(n_len, launch_tiles)
    assert tiles == 3 * launch_tiles + 1 and launches == 14
    for starts in (0, ATG):
        want = np_orfs(s, STOPS, starts, 600, both)
        crossing = sum(1 for p, l in zip(want[0].astype(np.int64), want[1].astype(np.int64)) for e in edges if p < e < p + l)
        assert crossing >= (3 if both or not starts else 1), (starts, both, crossing)
        res = po.orfs_dev(dsrc, n_len, STOPS, starts, 600, both_strands=both)
        got = _dev_result(*res)
        assert got[0] == want[0].size and _same(got[1:], want), (starts, both, got[0], want[0].size)
        assert _kernel_nodes_of(torch, lambda: po.orfs_dev(dsrc, n_len, STOPS, starts, 600, both_strands=both, pos=res[0], lens=res[1], info=res[2], count=res[3])) == launches
    assert _same(po.orfs_hip(src, n_len, STOPS, ATG, 600, both_strands=both), np_orfs(s, STOPS, ATG, 600, both))


@gpu
def test_gpu_capacity_sentinels_no_info_dense_and_ties(oracle, L):
    """out_cap of 0, n-1, n, n+1 at 8-B phases of the outputs with sentinels on both sides that survive; info = NULL; the count
    SET over a poisoned value; the host tier's CNT_ECAP with *count = n after writing the prefix, staged and pinned; the dense
    extreme (min_len 0 on random ACGT); and a stop set that overlaps its own rc3 image, so that one position bounds a run on both
    strands: forward before reverse"""
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(4)
    tie = STOPS | rc3_set(STOPS) | (1 << codon("ACG")) | (1 << codon("CGT"))  # ACG and CGT are each other's reverse complement
    assert rc3_set(tie) == tie
    bufs = [torch.empty(4 * TILE + 64, dtype=torch.int64, device="cuda") for _ in range(3)]
    cbuf = torch.empty(4, dtype=torch.int64, device="cuda")
    for stops, starts, min_len, both, n_len in ((STOPS, 0, 0, True, 2 * TILE + 77), (STOPS, ATG, 0, True, 3 * TILE + 5), (tie, 0, 0, True, TILE + 300),
                                                (tie, ATG | 1, 6, True, TILE + 31), (STOPS, ATG, 30, False, 2 * TILE + 1)):
        s = rng.integers(0, 4, n_len).astype(np.uint8)
        src = words_of_codes(oracle, s, rng=rng)
        d_src = torch.from_numpy(src.view(np.int64)).cuda()
        want = np_orfs(s, stops, starts, min_len, both)
        n = want[0].size
        assert n >= 50 and n <= bufs[0].numel() - 64
        if stops == tie and not starts:
            his = (want[0] + want[1]).astype(np.int64)
            same = np.flatnonzero(his[1:] == his[:-1])
            assert same.size > 20 and not (want[2][same] & np.uint64(CNT_FIND_REVERSE)).any() and (want[2][same + 1] & np.uint64(CNT_FIND_REVERSE)).all()
        for ph, cap in ((0, n), (3, n + 1), (5, n - 1), (7, 0)):
            for with_info in (True, False):
                tag = (hex(stops), starts, both, n_len, ph, cap, with_info)
                for b in bufs:
                    b.fill_(SENTINEL)
                cbuf.fill_(SENTINEL)
                po.orfs_dev(d_src, n_len, stops, starts, min_len, both_strands=both, pos=bufs[0][8 + ph : 8 + ph + cap], lens=bufs[1][8 + ph : 8 + ph + cap],
                            info=bufs[2][8 + ph : 8 + ph + cap] if with_info else False, count=cbuf[1:2])
                torch.cuda.synchronize()
                c = cbuf.cpu().numpy()
                assert c[1] == n and c[0] == SENTINEL and (c[2:] == SENTINEL).all(), tag
                got = min(n, cap)
                for j, b in enumerate(bufs):
                    h = b.cpu().numpy()
                    if j == 2 and not with_info:
                        assert (h == SENTINEL).all(), tag
                        continue
                    assert (h[: 8 + ph] == SENTINEL).all() and (h[8 + ph + got :] == SENTINEL).all(), tag + (j,)
                    assert np.array_equal(h[8 + ph : 8 + ph + got].view(np.uint64), want[j][:got]), tag + (j,)
        for pinned in (False, True):
            bits = cn.pinned_empty(src.size, np.uint64) if pinned else src.copy()
            bits[:] = src
            hb = [cn.pinned_empty(n + 16, np.uint64) if pinned else np.empty(n + 16, dtype=np.uint64) for _ in range(3)]
            for cap in (n, n + 1, n - 1, 0):
                for with_info in (True, False):
                    for h in hb:
                        h[:] = HOST_SENTINEL
                    rc, got_n = _host_call(L, bits, n_len, stops, starts, min_len, both, hb[0], hb[1], hb[2] if with_info else None, cap)
                    tag = (hex(stops), starts, both, n_len, cap, with_info, pinned)
                    assert rc == (_lib.CNT_ECAP if n > cap else _lib.CNT_OK) and got_n == n, (tag, rc, got_n)
                    got = min(n, cap)
                    for j, h in enumerate(hb):
                        if j == 2 and not with_info:
                            assert (h == HOST_SENTINEL).all(), tag
                        else:
                            assert np.array_equal(h[:got], want[j][:got]) and (h[got:] == HOST_SENTINEL).all(), tag + (j,)
        # the guess-and-retry wrapper
        assert _same(po.orfs_hip(src, n_len, stops, starts, min_len, both_strands=both), want)
    # len < 3 sets the device count to 0
    cbuf.fill_(SENTINEL)
    count = po.orfs_dev(d_src, 2, count=cbuf[1:2])[3]
    assert int(count.item()) == 0 and cbuf.cpu().numpy()[0] == SENTINEL


def _planted(rng, n_len, density):
    """random {A,C,G} with stops and starts of both strands planted at `density` per nucleotide"""
    s = acg(rng, n_len)
    kinds = [TAA, TAG, TGA, TTA, ATG_CODES, ATG_CODES, CAT, CAT]
    for at in rng.integers(0, max(n_len - 2, 1), int(n_len * density)):
        plant(s, int(at), kinds[int(rng.integers(0, len(kinds)))])
    return s


@gpu
def test_gpu_orfs_in_a_captured_graph_and_behind_a_side_stream(oracle):
    """encode -> scan of both strands -> reverse complement -> scan of the forward strand, captured with torch.cuda.graph with the
    same buffers and the same scratch (never zeroed) and replayed on 2 different inputs; then encode -> scan enqueued on a side
    stream with no host sync in between"""
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    n_len = (1 << 19) + 4133
    words = (n_len + 31) // 32
    d_n = torch.zeros(n_len, dtype=torch.uint8, device="cuda")
    bits = torch.empty(words, dtype=torch.int64, device="cuda")
    rc = torch.empty(words, dtype=torch.int64, device="cuda")
    work = torch.empty(po.orfs_work_bytes(n_len) + 8, dtype=torch.uint8, device="cuda")
    cap = 1 << 15
    outs = [tuple(torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)) + (torch.empty(1, dtype=torch.int64, device="cuda"),) for _ in range(2)]

    def scan(src, o, both):
        return po.orfs_dev(src, n_len, STOPS, ATG, 150, both_strands=both, pos=o[0], lens=o[1], info=o[2], count=o[3], work=work[3:])  # scratch at an odd byte

    def chain():
        cn.n_to_bits_dev(d_n, out=bits)
        scan(bits, outs[0], True)
        po.reverse_complement_dev(bits, n_len, out=rc)
        scan(rc, outs[1], False)  # the same scratch, in stream order

    assert _kernel_nodes_of(torch, lambda: scan(bits, outs[0], True)) == orf_plan(n_len)[1] == 5
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    rng = np.random.default_rng(31)
    comp = np.array([2, 3, 0, 1], dtype=np.uint8)
    letters = np.frombuffer(b"ACTG", dtype=np.uint8)
    for rep in range(2):
        s = _planted(rng, n_len, 0.002) if rep else rng.integers(0, 4, n_len).astype(np.uint8)
        d_n.copy_(torch.from_numpy(letters[s]))
        for o in outs:
            for t in o:
                t.fill_(SENTINEL)
        work.fill_(0x77 + rep)  # the scratch needs no zeroing
        g.replay()
        torch.cuda.synchronize()
        for j, (codes, both) in enumerate(((s, True), (comp[s[::-1]], False))):
            want = np_orfs(codes, STOPS, ATG, 150, both)
            got = _dev_result(*outs[j])
            assert got[0] == want[0].size >= 20 and _same(got[1:], want), (rep, j, got[0], want[0].size)
            assert (outs[j][0][got[0] :].cpu().numpy() == SENTINEL).all(), (rep, j)
    s = _planted(rng, n_len, 0.001)
    want = np_orfs(s, STOPS, 0, 900, True)
    host_n = torch.from_numpy(letters[s])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        n = host_n.cuda()
        res = po.orfs_dev(cn.n_to_bits_dev(n), n_len, STOPS, 0, 900, both_strands=True)
    torch.cuda.current_stream().wait_stream(side)
    got = _dev_result(*res)
    assert got[0] == want[0].size > 50 and _same(got[1:], want)


@gpu
def test_gpu_pinned_in_place_equals_staged(oracle, L):
    """pinned bits / pos / length / info (used in place, the kernels reading and writing host memory over the link) against
    ordinary ones (staged): identical results, at a phase inside the pinned allocations, and with only some buffers pinned"""
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    rng = np.random.default_rng(9)
    for starts, min_len, both, n_len in ((ATG, 0, True, 3 * TILE + 77), (0, 60, False, 2 * TILE + 5), (ATG, 90, True, TILE - 3)):
        s = rng.integers(0, 4, n_len).astype(np.uint8)
        src = words_of_codes(oracle, s, rng=rng)
        want = np_orfs(s, STOPS, starts, min_len, both)
        n = want[0].size
        assert n >= 10
        for pin_in, pin_out in ((False, False), (True, True), (True, False), (False, True)):
            bits = cn.pinned_empty(src.size + 3, np.uint64)[3:] if pin_in else src.copy()
            bits[:] = src
            hb = [cn.pinned_empty(n + 9, np.uint64)[1:] if pin_out else np.empty(n + 8, dtype=np.uint64) for _ in range(3)]
            for h in hb:
                h[:] = HOST_SENTINEL
            if pin_in and pin_out:
                assert L.cnt_host_is_pinned(bits.ctypes.data, bits.nbytes) == 1 and L.cnt_host_is_pinned(hb[0].ctypes.data, hb[0].nbytes) == 1
            rc, got_n = _host_call(L, bits, n_len, STOPS, starts, min_len, both, hb[0], hb[1], hb[2], n + 8)
            assert rc == _lib.CNT_OK and got_n == n, (starts, pin_in, pin_out, rc, got_n)
            for h, w in zip(hb, want):
                assert np.array_equal(h[:n], w) and (h[n:] == HOST_SENTINEL).all(), (starts, pin_in, pin_out)


@gpu
@pytest.mark.parametrize("seed", range(4))
def test_gpu_orfs_fuzz(oracle, L, seed):
    """random lengths up to 2^18, random {A,C,G} with a random density of planted stops and starts (or plain random ACGT), custom
    sets now and then, random min_len, strands, input phases (whole words into a larger buffer), capacities and info on / off;
    both tiers"""
    import torch

    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(7400 + seed)
    for it in range(24):
        n_len = int(rng.choice([rng.integers(0, 300), rng.integers(0, 3 * TILE), rng.integers(0, 1 << 18)]))
        density = float(rng.choice([0.0, 1e-4, 1e-3, 1e-2, 0.1]))
        s = rng.integers(0, 4, n_len).astype(np.uint8) if it % 4 == 3 else _planted(rng, n_len, density)
        stops = STOPS if it % 5 else (int(rng.integers(1, 2**63)) & int(rng.integers(1, 2**63)) & int(rng.integers(1, 2**63)) or 4)
        starts = int(rng.choice([0, ATG, ATG | (1 << codon("GTG"))]))
        min_len = int(rng.choice([0, 3, 30, 300, rng.integers(0, 20000)]))
        both, with_info, pi = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), int(rng.integers(0, 4))
        allw = np.concatenate([rng.integers(0, 2**64, pi, dtype=np.uint64), words_of_codes(oracle, s, extra=2, rng=rng)])
        nw = max((n_len + 31) // 32, 1)
        src = allw[pi : pi + nw]
        want = np_orfs(s, stops, starts, min_len, both)
        n = want[0].size
        cap = int(rng.choice([n, n + 3, max(n - 1, 0), int(rng.integers(0, n + 1))]))
        tag = (seed, it, n_len, density, hex(stops), hex(starts), min_len, both, with_info, pi, cap, n)
        dall = torch.from_numpy(allw.view(np.int64)).cuda()
        bufs = [torch.full((cap + 8,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(3)]
        count = po.orfs_dev(dall[pi : pi + nw], n_len, stops, starts, min_len, both_strands=both, pos=bufs[0][3 : 3 + cap], lens=bufs[1][3 : 3 + cap],
                            info=bufs[2][3 : 3 + cap] if with_info else False)[3]
        got = min(n, cap)
        assert int(count.item()) == n, tag
        for j, b in enumerate(bufs):
            h = b.cpu().numpy()
            if j == 2 and not with_info:
                assert (h == SENTINEL).all(), tag
            else:
                assert np.array_equal(h[3 : 3 + got].view(np.uint64), want[j][:got]) and (h[:3] == SENTINEL).all() and (h[3 + got :] == SENTINEL).all(), tag + (j,)
        hb = [np.full(cap + 2, HOST_SENTINEL, dtype=np.uint64) for _ in range(3)]
        rc, hn = _host_call(L, np.ascontiguousarray(src), n_len, stops, starts, min_len, both, hb[0], hb[1], hb[2] if with_info else None, cap)
        assert rc == (_lib.CNT_ECAP if n > cap else _lib.CNT_OK) and hn == n, tag
        for j, h in enumerate(hb):
            if j < 2 or with_info:
                assert np.array_equal(h[:got], want[j][:got]) and (h[got:] == HOST_SENTINEL).all(), tag + (j,)


@gpu
def test_gpu_scan_then_translate_and_extract_end_to_end(oracle):
    """the pipeline the entries are made for: every ORF's protein through translate_dev from pos / length / strand as reported,
    and the ORFs of one length through extract_dev with pos and info as they are"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(21)
    n_len = 3 * TILE + 50
    s = rng.integers(0, 4, n_len).astype(np.uint8)
    src = words_of_codes(oracle, s)
    bits = torch.from_numpy(src.view(np.int64)).cuda()
    n, pos, length, info = _dev_result(*po.orfs_dev(bits, n_len, min_len=90, both_strands=True))
    assert n >= 10
    for p, l, i in list(zip(pos.astype(np.int64), length.astype(np.int64), info.astype(np.int64)))[:40]:
        prot = bytes(po.translate_dev(bits, n_len, int(p), int(l), revcomp=bool(i & CNT_FIND_REVERSE)).cpu().numpy())
        assert prot[:1] == b"M" and b"*" not in prot and len(prot) == l // 3
    L0 = int(np.bincount(length.astype(np.int64)).argmax())
    sel = np.flatnonzero(length.astype(np.int64) == L0)
    recs, rejected = po.extract_dev(bits, n_len, torch.from_numpy(pos[sel].view(np.int64)).cuda(), L0, info=torch.from_numpy(info[sel].view(np.int64)).cuda())
    assert int(rejected.item()) == 0
    recs = recs.cpu().numpy().view(np.uint64)
    for r in recs:
        assert codes_of(r, 3).tolist() == ATG_CODES  # each reads as its strand does: it begins with ATG


@gpu
def test_gpu_orfs_full_size_past_2p32(oracle, fullsize):
    """2^32 + 2^21 + 35 nt of random {A,C,G} made on the device (random words with every T turned into G), stops and starts
    of both strands planted before and beyond position 2^32 -- runs of millions of nucleotides, one across 2^32, one lane open
    from end to end -- exact against the reference run on the sites found in the few words around each plant"""
    import torch

    from conftest import need_free_hbm
    from cute_nucleotides_amd import packed_ops as po

    n_len = (1 << 32) + (1 << 21) + 35
    words = (n_len + 31) // 32
    need_free_hbm(6)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x6F7266)
    bits = torch.randint(-(1 << 63), (1 << 63) - 1, (words,), dtype=torch.int64, device="cuda", generator=gen)
    bits |= (bits >> 1) & 0x5555555555555555  # code 2 (T) becomes 3 (G): A 1/4, C 1/4, G 1/2
    assert int(po.kmer_counts_dev(bits, n_len, 1)[2].item()) == 0  # no T: no stop and no ATG on either strand
    rng = np.random.default_rng(8)
    P32 = 1 << 32
    plants = [(3 * 1000 + 1, TAA), (3 * 5000 + 1, ATG_CODES), (P32 - 3 * 70000 + 2, ATG_CODES), (P32 + 3 * 333 + (1 - P32) % 3, TAA),  # lane 1: a run across 2^32
              (3 * 2000 + 2, TTA), ((1 << 31) + 1 + (2 - ((1 << 31) + 1)) % 3, CAT), (P32 + TILE * 9 - 1 + (2 - (P32 + TILE * 9 - 1)) % 3, TTA),  # lane 2, reverse
              (P32 + (1 << 20) + 4 + (1 - (P32 + (1 << 20) + 4)) % 3, ATG_CODES), (n_len - 3 - (n_len - 3 - 1) % 3, TAG)]  # lane 1 again, to the last codons
    plants.sort()
    assert all(b[0] - a[0] >= 8 for a, b in zip(plants, plants[1:]))
    for at, codes in plants:
        w0 = (at - 1) >> 5
        piece = bits[w0 : w0 + 2].cpu().numpy().view(np.uint64).copy()
        _set_codes(piece, w0 * 32, at - 1, [3] + codes + [1, 1])  # plant()'s padding
        bits[w0 : w0 + piece.size] = torch.from_numpy(piece.view(np.int64)).cuda()
    cap = 1 << 10
    outs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)]
    work = torch.empty(po.orfs_work_bytes(n_len), dtype=torch.uint8, device="cuda")
    po.orfs_dev(bits, n_len, STOPS, ATG, 3000, both_strands=True, pos=outs[0], lens=outs[1], info=outs[2], work=work)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    count = po.orfs_dev(bits, n_len, STOPS, ATG, 3000, both_strands=True, pos=outs[0], lens=outs[1], info=outs[2], work=work)[3]
    torch.cuda.synchronize()
    fullsize(32, (time.perf_counter() - t0) * 1e3, check="orfs ATG min_len=3000 both strands: kernels")
    # the sites: the codons that touch a plant, read back from the device words
    sites = [[[], []], [[], []]]
    for at, _ in plants:
        first = max(at - 4, 0)
        w0 = first >> 5
        piece = bits[w0 : w0 + 3].cpu().numpy().view(np.uint64)
        last = min(at + 7, n_len, (w0 + piece.size) * 32)
        c = codons_of(codes_of(piece, last - w0 * 32)[first - w0 * 32 :])
        for strand, (sp, ap) in enumerate(sites_of(c, STOPS, ATG, True, first=first)):
            sites[strand][0] += sp.tolist()
            sites[strand][1] += ap.tolist()
    sites = [(np.unique(np.array(sp, dtype=np.int64)), np.unique(np.array(ap, dtype=np.int64))) for sp, ap in sites]
    for starts, min_len in ((ATG, 3000), (0, 0)):
        want = orfs_from_sites(n_len, sites, starts != 0, min_len)
        count = po.orfs_dev(bits, n_len, STOPS, starts, min_len, both_strands=True, pos=outs[0], lens=outs[1], info=outs[2], work=work)[3]
        got = _dev_result(outs[0], outs[1], outs[2], count)
        assert got[0] == want[0].size <= cap and _same(got[1:], want), (starts, got[0], want[0].size)
        ends = (want[0] + want[1]).astype(np.int64)
        assert ((want[0].astype(np.int64) < P32) & (ends > P32)).sum() >= 1 and (want[0].astype(np.int64) > P32).sum() >= 1
        if not starts:  # lane 0 holds no plant: open from end to end on both strands
            whole = (want[2] & np.uint64(CNT_ORF_OPEN_END | CNT_ORF_NO_STOP)) == CNT_ORF_OPEN_END | CNT_ORF_NO_STOP
            assert whole.sum() >= 2 and (want[1][whole].astype(np.int64) >= n_len - 5).all()
