"""Pinned caller memory in every layout a caller can build (include/cute_nt.h "pinned caller memory"): each side of a host call
ordinary, hipHostMalloc'ed (cnt_host_alloc at element offsets 0 / 1 / 5, torch pin_memory) or registered in place
(cnt_host_register) as a whole registration, an interior slice off its pages, its exact extent and one element more, a slice
that runs out of a registration or into one, across two adjacent registrations, across an unregistered hole between two, and
after cnt_host_unregister.  Every host entry point -- both codecs with their flag modes and validated forms, the sharded encode,
and the six packed-domain calls of host_call -- at sizes on both sides of each lane boundary.

Per case, in this order: cnt_host_is_pinned on every side against what the layout is (before anything runs on it: a wrong
answer fails the test here, it never hands a hole to a kernel); the results bit for bit against the CPU oracle, return codes
exact; canaries intact around every output, inside the pinned or registered block too; and on the hooks build at pipeline
sizes the trace's in-place flags (tags 5 / 6) against the predicate.  A range that starts in pinned memory and leaves it is
staged like ordinary memory, through the codecs' pinned ring or host_call's ordinary bounce copy: the runtime refuses a
hipMemcpy of such a range."""
import ctypes
import mmap

import numpy as np
import pytest

from test_minimizers import np_minimizers

pytestmark = pytest.mark.gpu

PAGE = mmap.PAGESIZE
CANARY = 0xA5
ALPHA = np.frombuffer(b"ACGTUacgtu", dtype=np.uint8)
ALPHA5 = np.frombuffer(b"ACGTNacgtnUu", dtype=np.uint8)

# layout -> what cnt_host_is_pinned must answer for the side's whole range
EXPECT = {"plain": 0, "alloc0": 1, "alloc1": 1, "alloc5": 1, "torch": 1, "reg_whole": 1, "reg_interior": 1, "reg_exact": 1,
          "reg_exact_plus": 0, "reg_then_plain": 0, "plain_then_reg": 0, "adjacent": 0, "hole": 0, "unregistered": 0}
LAYOUTS = list(EXPECT)


def _pages(nbytes):
    return -(-nbytes // PAGE) * PAGE


def _lib():
    from cute_nucleotides_amd import _lib

    return _lib.lib()


class Side:
    """`nbytes` of one side of a call, placed as `kind` says inside a backing buffer that is all canary bytes elsewhere.
    Registered layouts are cut from one page-aligned anonymous mapping; close() unregisters what is still registered."""

    def __init__(self, kind, nbytes, elem):
        import cute_nucleotides_amd as cn

        assert Side.fits(kind, nbytes, elem), (kind, nbytes, elem)
        self.kind, self.nbytes, self.regs, self.keep = kind, nbytes, [], None
        if kind == "plain":
            self.back, self.start = np.empty(nbytes + 256, np.uint8), 64
        elif kind.startswith("alloc"):
            off = int(kind[5:]) * elem
            self.back, self.start = cn.pinned_empty(nbytes + off + 128, np.uint8), off
        elif kind == "torch":
            import torch

            self.keep = torch.empty(nbytes + 128, dtype=torch.uint8, pin_memory=True)
            self.back, self.start = self.keep.numpy(), 0
        else:
            self._arena(kind, nbytes, elem)
        assert self.start + nbytes <= self.back.size, (kind, nbytes)
        self.back[:] = CANARY
        self.p = self.back.ctypes.data + self.start

    def _arena(self, kind, nbytes, elem):
        regs = []
        if kind in ("reg_whole", "reg_exact", "reg_exact_plus", "unregistered"):
            start, total = 0, _pages(nbytes) + PAGE
            size = {"reg_whole": _pages(nbytes), "reg_exact": nbytes, "reg_exact_plus": nbytes - elem, "unregistered": _pages(nbytes)}[kind]
            regs = [(0, size)]
        elif kind == "reg_interior":  # off its page and on an odd word (letters: off the word as well)
            start = PAGE + 3 * 8 + (5 if elem == 1 else 0)
            total = _pages(start + nbytes) + 2 * PAGE
            regs = [(0, total - PAGE)]
        else:  # the range crosses the page boundary b: from [.., b) into [b, ..), or for the hole into [b + PAGE, ..)
            gap = PAGE if kind == "hole" else 0
            head = max(elem, (nbytes - gap) // 2 // elem * elem)
            b = _pages(head) + PAGE
            start, end = b - head, b - head + nbytes
            total = _pages(end) + 2 * PAGE
            regs = {"reg_then_plain": [(0, b)], "plain_then_reg": [(b, total - PAGE - b)],
                    "adjacent": [(0, b), (b, total - PAGE - b)], "hole": [(0, b), (b + PAGE, total - 2 * PAGE - b)]}[kind]
        self.keep = mmap.mmap(-1, total)
        self.back, self.start = np.frombuffer(self.keep, np.uint8), start
        L, base = _lib(), self.back.ctypes.data
        for off, size in regs:
            assert L.cnt_host_register(ctypes.c_void_p(base + off), size) == 0, (kind, off, size)
            self.regs.append(base + off)
        if kind == "unregistered":
            self.close()

    @staticmethod
    def fits(kind, nbytes, elem):
        """can this layout be built around a range of nbytes?"""
        if kind in ("reg_then_plain", "plain_then_reg", "adjacent"):
            return nbytes >= 2 * elem
        if kind == "hole":
            return nbytes >= PAGE + 2 * elem
        return kind != "reg_exact_plus" or nbytes > elem

    def arr(self, dtype):
        return self.back[self.start : self.start + self.nbytes].view(dtype)

    def vp(self):
        return ctypes.c_void_p(self.p)

    def assert_pinned(self, tag):
        got = _lib().cnt_host_is_pinned(self.vp(), self.nbytes)
        assert got == EXPECT[self.kind], ("cnt_host_is_pinned", self.kind, self.nbytes, got) + tuple(tag)

    def assert_canaries(self, used, tag):
        """every byte of the backing buffer outside [start, start + used) still holds its canary"""
        b = self.back
        assert (b[: self.start] == CANARY).all() and (b[self.start + used :] == CANARY).all(), ("canary", self.kind, used) + tuple(tag)

    def close(self):
        L = _lib()
        while self.regs:
            assert L.cnt_host_unregister(ctypes.c_void_p(self.regs.pop())) == 0


def _sides(specs, tag):
    """build every side, then check the predicate on every one of them before the caller runs anything"""
    sides = []
    try:
        for kind, nbytes, elem in specs:
            sides.append(Side(kind, nbytes, elem))
        for s in sides:
            s.assert_pinned(tag)
    except BaseException:
        _close(sides)  # nothing stays registered behind a failed check
        raise
    return sides


def _close(sides):
    for s in sides:
        s.close()


def _pairs(full):
    """(input layout, output layout): each layout on both sides; with `full` also against cnt_host_alloc'ed and ordinary memory
    on the other side"""
    out = [(k, k) for k in LAYOUTS]
    if full:
        out += [(k, "alloc0") for k in LAYOUTS if k != "alloc0"] + [("alloc0", k) for k in LAYOUTS if k != "alloc0"]
        out += [("plain", k) for k in ("reg_interior", "torch")] + [(k, "plain") for k in ("reg_interior", "torch")]
    return out


def _trace(L):
    tags = (ctypes.c_int * 4096)()
    us = (ctypes.c_double * 4096)()
    k = L.cnt_test_host_trace(tags, us, 4096)
    return {tags[i]: us[i] for i in range(k) if tags[i] in (5, 6)}


# ---- the codecs ------------------------------------------------------------------------------------------------------
class CodecData:
    def __init__(self, oracle, n_len):
        rng = np.random.default_rng(n_len)
        self.n_len = n_len
        self.letters = ALPHA[rng.integers(0, 10, n_len)]
        self.words = oracle.n_to_bits_lut(self.letters)
        self.back = oracle.bits_to_n_lut(self.words, n_len)
        self.dirty = self.letters.copy()
        self.dirty[rng.integers(0, n_len, 7)] = 0x21
        self.dirty_words, self.dirty_bad = oracle.n_to_bits_lut(self.dirty), oracle.validate(self.dirty)
        self.clean5 = ALPHA5[rng.integers(0, 12, n_len)]
        self.clean_words5 = oracle.n_to_bits2_lut(self.clean5)
        self.letters5 = self.clean5.copy()
        self.letters5[rng.integers(0, n_len, 5)] = 0x2E
        self.words5, self.bad5 = oracle.n_to_bits2_lut(self.letters5), oracle.validate(self.letters5, allow_n=True)
        self.back5 = oracle.bits_to_n2_lut(self.words5, n_len)


def _codec_case(L, d, kind_in, kind_out, trace=False):
    from cute_nucleotides_amd import _lib

    n_len, words, words5 = d.n_len, d.words.size, d.words5.size
    tag = (n_len, kind_in, kind_out)
    sides = _sides([(kind_in, n_len, 1), (kind_out, words * 8, 8), (kind_in, n_len, 1), (kind_out, words5 * 8, 8)], tag)
    n, w, back, w5 = sides
    want_in, want_out = EXPECT[kind_in], EXPECT[kind_out]
    try:
        bad = ctypes.c_uint64(1 << 60)
        n.arr(np.uint8)[:] = d.letters
        for flags in (None, 0, _lib.CNT_STRICT_LUT, _lib.CNT_TAIL_LUT):
            w.back[:] = CANARY
            rc = L.cnt_n_to_bits(n.vp(), n_len, w.vp(), words) if flags is None else L.cnt_n_to_bits_ex(n.vp(), n_len, w.vp(), words, flags)
            assert rc == 0 and np.array_equal(w.arr(np.uint64), d.words), tag + ("encode", flags, rc)
            w.assert_canaries(words * 8, tag)
            if trace:
                assert _trace(L) == {5: float(want_in), 6: float(want_out)}, tag + ("encode trace",)
        back.back[:] = CANARY
        assert L.cnt_bits_to_n(w.vp(), words, n_len, back.vp()) == 0
        assert np.array_equal(back.arr(np.uint8), d.back), tag + ("decode",)
        back.assert_canaries(n_len, tag)
        if trace:
            assert _trace(L) == {5: float(want_out), 6: float(want_in)}, tag + ("decode trace",)
        n.arr(np.uint8)[:] = d.dirty
        w.back[:] = CANARY
        assert L.cnt_n_to_bits_checked(n.vp(), n_len, w.vp(), words, _lib.CNT_STRICT_LUT, ctypes.byref(bad)) == 0
        assert bad.value == d.dirty_bad and np.array_equal(w.arr(np.uint64), d.dirty_words), tag + ("checked", bad.value)
        w.assert_canaries(words * 8, tag)
        # the 5-letter codec: its default table agrees with BYTE_LUT on the alphabet; the checked form counts the strays
        n.arr(np.uint8)[:] = d.clean5
        assert L.cnt_n_to_bits2(n.vp(), n_len, w5.vp(), words5) == 0
        assert np.array_equal(w5.arr(np.uint64), d.clean_words5), tag + ("encode2",)
        w5.assert_canaries(words5 * 8, tag)
        n.arr(np.uint8)[:] = d.letters5
        w5.back[:] = CANARY
        assert L.cnt_n_to_bits2_checked(n.vp(), n_len, w5.vp(), words5, _lib.CNT_STRICT_LUT, ctypes.byref(bad)) == 0
        assert bad.value == d.bad5 and np.array_equal(w5.arr(np.uint64), d.words5), tag + ("checked2", bad.value)
        w5.assert_canaries(words5 * 8, tag)
        back.back[:] = CANARY
        assert L.cnt_bits_to_n2(w5.vp(), words5, n_len, back.vp()) == 0
        assert np.array_equal(back.arr(np.uint8), d.back5), tag + ("decode2",)
        back.assert_canaries(n_len, tag)
    finally:
        _close(sides)


# below the single-kernel lane (2^16), just above it, past the zero-copy path of the encode (2^21) and of the decode (2^22)
@pytest.mark.parametrize("n_len", [(1 << 16) - 5, (1 << 16) + 3, (1 << 21) + 5, (1 << 22) + 5])
def test_codecs_on_every_layout(oracle, n_len):
    d = CodecData(oracle, n_len)
    L = _lib()
    for kind_in, kind_out in _pairs(full=n_len < (1 << 21)):
        if Side.fits(kind_in, n_len, 1) and Side.fits(kind_out, d.words.size * 8, 8):
            _codec_case(L, d, kind_in, kind_out)


def test_codecs_on_every_layout_past_the_single_kernel_lane(oracle, hooks_build):
    """2^25 + 31 nt: the pipeline, whose trace says which sides it used in place -- the predicate's answer on every layout"""
    d = CodecData(oracle, (1 << 25) + 31)
    for kind_in, kind_out in _pairs(full=False) + [("reg_interior", "plain"), ("plain", "reg_interior"), ("hole", "reg_whole")]:
        _codec_case(hooks_build, d, kind_in, kind_out, trace=True)


def test_sharded_encode_on_registered_layouts(oracle, hooks_build):
    """every shard's worker asks about its own part of the caller's slices: parts inside one registration go in place, the
    others are staged, and the words are the oracle's"""
    from cute_nucleotides_amd import sharding

    n_len = (1 << 23) + 999
    rng = np.random.default_rng(5)
    letters = ALPHA[rng.integers(0, 10, n_len)]
    want = oracle.n_to_bits_lut(letters)
    L = hooks_build
    sharding.alias_devices(True)
    try:
        for kind in ("reg_interior", "reg_exact", "adjacent", "hole", "reg_then_plain", "plain_then_reg"):
            sides = _sides([(kind, n_len, 1), (kind, want.size * 8, 8)], (n_len, kind))
            try:
                n, w = sides
                n.arr(np.uint8)[:] = letters
                for ndev in (1, 3):
                    w.back[:] = CANARY
                    assert L.cnt_n_to_bits_sharded(n.vp(), n_len, w.vp(), want.size, ndev) == 0
                    assert np.array_equal(w.arr(np.uint64), want), (kind, ndev)
                    w.assert_canaries(want.size * 8, (kind, ndev))
            finally:
                _close(sides)
    finally:
        sharding.alias_devices(False)


# ---- the packed-domain calls (host_call: one lane at every size) ---------------------------------------------------------
K, KW, WW = 21, 15, 10  # k of the k-mers; k and w of the minimizers


class PackedData:
    def __init__(self, oracle, n_len):
        rng = np.random.default_rng(100 + n_len)
        self.n_len = n_len
        self.letters = ALPHA[rng.integers(0, 10, n_len)]
        self.letters[rng.integers(0, n_len, 3)] = 0x2D
        self.invalid = oracle.validate(self.letters)
        self.a = rng.integers(0, 2**64, (n_len + 31) // 32, dtype=np.uint64)  # garbage above len in the last word included
        self.b = rng.integers(0, 2**64, self.a.size, dtype=np.uint64)
        self.dist = oracle.hamming(self.a, self.b, n_len)
        self.comp, self.rc = oracle.complement(self.a, n_len), oracle.reverse_complement(self.a, n_len)
        self.kmers = {c: oracle.kmers(self.a, n_len, K, c) for c in (False, True)}
        self.mini = {c: np_minimizers(self.a, n_len, KW, WW, c) for c in (False, True)}
        m = n_len - KW + 1
        self.windows = max(m - WW + 1, 0)


def _packed_case(L, d, kind_in, kind_out):
    from cute_nucleotides_amd import _lib

    n_len, words = d.n_len, d.a.size
    tag = (n_len, kind_in, kind_out)
    m = max(n_len - K + 1, 0)
    specs = [(kind_in, words * 8, 8), (kind_out, words * 8, 8), (kind_out, words * 8, 8), (kind_in, n_len, 1)]
    specs += [(kind_out, m * 8, 8)] if m else []
    sides = _sides(specs, tag)
    a, b, out, letters = sides[:4]
    try:
        a.arr(np.uint64)[:], b.arr(np.uint64)[:], letters.arr(np.uint8)[:] = d.a, d.b, d.letters
        dist, bad = ctypes.c_uint64(1 << 60), ctypes.c_uint64(1 << 60)
        assert L.cnt_hamming(a.vp(), b.vp(), n_len, ctypes.byref(dist)) == 0 and dist.value == d.dist, tag + ("hamming", dist.value)
        for fn, want in ((L.cnt_complement, d.comp), (L.cnt_reverse_complement, d.rc)):
            out.back[:] = CANARY
            assert fn(a.vp(), n_len, out.vp()) == 0 and np.array_equal(out.arr(np.uint64), want), tag + (fn.__name__,)
            out.assert_canaries(words * 8, tag + (fn.__name__,))
        assert L.cnt_validate(letters.vp(), n_len, 0, ctypes.byref(bad)) == 0 and bad.value == d.invalid, tag + ("validate", bad.value)
        if m:
            kout = sides[4]
            for canonical in (False, True):
                kout.back[:] = CANARY
                rc = L.cnt_kmers(a.vp(), n_len, K, _lib.CNT_KMER_CANONICAL if canonical else 0, kout.vp(), m)
                assert rc == 0 and np.array_equal(kout.arr(np.uint64), d.kmers[canonical]), tag + ("kmers", canonical, rc)
                kout.assert_canaries(m * 8, tag + ("kmers",))
    finally:
        _close(sides)
    if d.windows:
        _minimizer_case(L, d, kind_in, kind_out, kind_out)


def _minimizer_case(L, d, kind_in, kind_pos, kind_val):
    """cnt_minimizers with room for every window, for exactly the count, and for half of it (CNT_ECAP: that prefix, no more);
    with and without values"""
    from cute_nucleotides_amd import _lib

    n_len, words = d.n_len, d.a.size
    for canonical in (False, True):
        want_p, want_v = d.mini[canonical]
        cnt = want_p.size
        for cap in (d.windows, cnt, max(cnt // 2, 1)):
            for values in (True, False):
                tag = (n_len, kind_in, kind_pos, kind_val, canonical, cap, values)
                specs = [(kind_in, words * 8, 8), (kind_pos, min(cap, d.windows) * 8, 8)]
                specs += [(kind_val, min(cap, d.windows) * 8, 8)] if values else []
                if not all(Side.fits(*s) for s in specs):
                    continue
                sides = _sides(specs, tag)
                try:
                    sides[0].arr(np.uint64)[:] = d.a
                    pos, val = sides[1], sides[2] if values else None
                    got = ctypes.c_uint64(1 << 60)
                    rc = L.cnt_minimizers(sides[0].vp(), n_len, KW, WW, _lib.CNT_KMER_CANONICAL if canonical else 0, pos.vp(),
                                          val.vp() if values else None, cap, ctypes.byref(got))
                    assert rc == (_lib.CNT_ECAP if cnt > cap else 0) and got.value == cnt, tag + (rc, got.value)
                    k = min(cap, cnt)
                    assert np.array_equal(pos.arr(np.uint64)[:k], want_p[:k]), tag + ("pos",)
                    pos.assert_canaries(k * 8, tag + ("pos",))
                    if values:
                        assert np.array_equal(val.arr(np.uint64)[:k], want_v[:k]), tag + ("val",)
                        val.assert_canaries(k * 8, tag + ("val",))
                finally:
                    _close(sides)


@pytest.mark.parametrize("n_len", [1, 31, 4097, (1 << 20) + 3])
def test_packed_ops_on_every_layout(oracle, n_len):
    d = PackedData(oracle, n_len)
    L = _lib()
    for kind_in, kind_out in _pairs(full=True):
        fits = all(Side.fits(kind_in, nb, e) for nb, e in ((d.a.size * 8, 8), (n_len, 1)))
        if fits and Side.fits(kind_out, d.a.size * 8, 8):
            _packed_case(L, d, kind_in, kind_out)


# ---- the lane rules of host_call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_len", [4097, (1 << 20) + 3])
def test_host_call_lane_rules(oracle, n_len):
    """two reading sides that overlap stay in place; an output that overlaps its input is staged and equals the oracle of
    the ORIGINAL input; minimizers with one output pinned and the other ordinary are staged and copy back exactly
    min(count, out_cap) entries"""
    d = PackedData(oracle, n_len)
    L = _lib()
    words = d.a.size
    for kind in ("alloc1", "reg_interior", "reg_exact", "plain"):  # three pinned layouts and ordinary, pageable memory
        # hamming(a, a): the same buffer twice, both Dir::in
        sides = _sides([(kind, (words + 1) * 8, 8)], (n_len, kind))
        (s,) = sides
        try:
            s.arr(np.uint64)[:words] = d.a
            dist = ctypes.c_uint64(1 << 60)
            assert L.cnt_hamming(s.vp(), s.vp(), n_len, ctypes.byref(dist)) == 0 and dist.value == 0, (n_len, kind)
            # an output one word past its input, inside the same allocation / registration: staged, from the original words
            for fn, want in ((L.cnt_complement, d.comp), (L.cnt_reverse_complement, d.rc)):
                s.back[:] = CANARY
                s.arr(np.uint64)[:words] = d.a
                assert fn(s.vp(), n_len, ctypes.c_void_p(s.p + 8)) == 0, (n_len, kind, fn.__name__)
                assert np.array_equal(s.arr(np.uint64)[1:], want), (n_len, kind, fn.__name__)
                s.assert_canaries((words + 1) * 8, (n_len, kind, fn.__name__))
        finally:
            _close(sides)
    # one side pinned, the other ordinary: all staged
    for kind_in, kind_pos, kind_val in (("alloc0", "alloc0", "plain"), ("reg_interior", "plain", "reg_interior"),
                                        ("plain", "reg_interior", "alloc0")):
        _minimizer_case(L, d, kind_in, kind_pos, kind_val)


def test_predicate_on_every_layout():
    """cnt_host_is_pinned alone, every layout at a few sizes and both element widths; every wrong answer is listed"""
    wrong = []
    for nbytes, elem in ((8, 8), (1032, 8), (PAGE + 16, 8), (65539, 1), ((1 << 20) + 8, 8), (3 << 20, 1)):
        for kind in LAYOUTS:
            if Side.fits(kind, nbytes, elem):
                s = Side(kind, nbytes, elem)
                try:
                    got = _lib().cnt_host_is_pinned(s.vp(), nbytes)
                finally:
                    s.close()
                if got != EXPECT[kind]:
                    wrong.append((kind, nbytes, got))
    assert not wrong, wrong


def test_predicate_at_the_edges_of_a_registration():
    """the exact extent of a registration is pinned, one byte more is not, nor one byte in front; a page-aligned piece
    anywhere inside is; the same ranges are ordinary after cnt_host_unregister; hipHostMalloc'ed memory keeps its answers"""
    import cute_nucleotides_amd as cn

    L = _lib()
    arena = mmap.mmap(-1, 8 * PAGE)
    buf = np.frombuffer(arena, np.uint8)
    base = buf.ctypes.data
    p = lambda off: ctypes.c_void_p(base + off)
    size = 5 * PAGE + 123
    assert L.cnt_host_is_pinned(p(PAGE), size) == 0
    assert L.cnt_host_register(p(PAGE), size) == 0
    try:
        assert L.cnt_host_is_pinned(p(PAGE), size) == 1
        assert L.cnt_host_is_pinned(p(PAGE), size + 1) == 0
        assert L.cnt_host_is_pinned(p(PAGE - 1), 2) == 0 and L.cnt_host_is_pinned(p(PAGE - 1), size + 1) == 0
        assert L.cnt_host_is_pinned(p(PAGE + size - 1), 1) == 1 and L.cnt_host_is_pinned(p(PAGE + size - 1), 2) == 0
        for off in (0, 1, 24, PAGE + 24, 3 * PAGE - 7):
            assert L.cnt_host_is_pinned(p(PAGE + off), size - off) == 1, off
            assert L.cnt_host_is_pinned(p(PAGE + off), size - off + 1) == 0, off
            assert L.cnt_host_is_pinned(p(PAGE + off), 1) == 1, off
    finally:
        assert L.cnt_host_unregister(p(PAGE)) == 0
    assert L.cnt_host_is_pinned(p(PAGE), size) == 0 and L.cnt_host_is_pinned(p(PAGE + 24), 8) == 0
    a = cn.pinned_empty(3 * PAGE, np.uint8)
    q = a.ctypes.data
    assert L.cnt_host_is_pinned(ctypes.c_void_p(q + PAGE + 24), 2 * PAGE - 24) == 1
    assert L.cnt_host_is_pinned(ctypes.c_void_p(q + PAGE + 24), 2 * PAGE - 23 + (1 << 22)) == 0
