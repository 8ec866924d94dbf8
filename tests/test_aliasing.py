"""Argument aliasing of every packed-domain call (include/cute_nt.h, "SHARED MEMORY"): a buffer a call writes shares no byte
with any other buffer of that call, buffers it only reads may overlap freely, and two exceptions stay -- cnt_complement_dev
exactly in place, and the host tiers of complement and reverse complement, which stage an overlapping call.

CPU part: one table of every entry point of both tiers with its buffers, their extents and which of them it writes; from it every
(written buffer, other buffer) pair is tried at five overlapping placements (all CNT_EINVAL, nothing written) and at the two
touching ones (accepted).  Every check precedes device work, so no device is needed.  Then the argument contract of the four
oldest calls, and the header's error lists against the table.  GPU part: what the rule ALLOWS really works on the device --
in-place complement at every path of its launcher, touching buffers of seven calls, overlapping read-only streams -- and the
Python layer hands the refusals on."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest

from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64P = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


def words_for(n):
    return (n + 31) // 32


# ---- the table ------------------------------------------------------------------------------------------------------------------
# a buffer of a call: its extent in bytes as rule 1 of the header states it, the alignment the call asks of its pointer (also the
# step of the placements below: the "element"), and whether the call writes it
Buf = collections.namedtuple("Buf", "name bytes align written")
# a call: fn(addresses by buffer name) -> status.  in_place: the (written, other) pairs that may start at the same address.
Call = collections.namedtuple("Call", "name bufs fn in_place")

N_LEN = 100  # nucleotides of every packed input: 4 words, the last one ragged
IN = words_for(N_LEN) * 8
CAP = 24  # capacity of the counted outputs: below what each call could report, so the extent is min(most, out_cap)
LENT = 64  # bytes of d_work lent beyond the query's answer: not part of its extent


def _query(L, fn, *args):
    out = ctypes.c_size_t(1 << 40)
    assert fn(*args, ctypes.byref(out)) == 0
    return out.value


def table(L):
    """every packed-domain entry point of both tiers, except the host tiers of complement and reverse complement (rule 3)"""
    vp = ctypes.c_void_p
    up = lambda a: ctypes.cast(vp(a), U64P)  # noqa: E731 -- the host tiers' typed result pointers
    rd = lambda name, nbytes=IN, align=8: Buf(name, nbytes, align, False)  # noqa: E731
    wr = lambda name, nbytes, align=8: Buf(name, nbytes, align, True)  # noqa: E731
    calls = []

    def add(name, bufs, fn, in_place=()):
        calls.append(Call(name, bufs, fn, frozenset(in_place)))

    add("cnt_hamming_dev", [rd("a"), rd("b"), wr("count", 8)], lambda p: L.cnt_hamming_dev(vp(p["a"]), vp(p["b"]), N_LEN, vp(p["count"]), None))
    add("cnt_hamming", [rd("a"), rd("b"), wr("count", 8)], lambda p: L.cnt_hamming(vp(p["a"]), vp(p["b"]), N_LEN, up(p["count"])))
    add("cnt_complement_dev", [rd("bits"), wr("out", IN)], lambda p: L.cnt_complement_dev(vp(p["bits"]), N_LEN, vp(p["out"]), None),
        in_place=[("out", "bits")])
    add("cnt_reverse_complement_dev", [rd("bits"), wr("out", IN)], lambda p: L.cnt_reverse_complement_dev(vp(p["bits"]), N_LEN, vp(p["out"]), None))
    n_len = 104  # ASCII bytes: a multiple of 8, so that an 8-B aligned counter can touch their end
    add("cnt_validate_dev", [rd("n", n_len, 1), wr("count", 8)], lambda p: L.cnt_validate_dev(vp(p["n"]), n_len, 0, vp(p["count"]), None))
    add("cnt_validate", [rd("n", n_len, 1), wr("count", 8)], lambda p: L.cnt_validate(vp(p["n"]), n_len, 2, up(p["count"])))

    k = 17
    m = N_LEN - k + 1
    add("cnt_kmers_dev", [rd("bits"), wr("out", m * 8)], lambda p: L.cnt_kmers_dev(vp(p["bits"]), N_LEN, k, 0x10, vp(p["out"]), m, None))
    add("cnt_kmers", [rd("bits"), wr("out", m * 8)], lambda p: L.cnt_kmers(vp(p["bits"]), N_LEN, k, 0, vp(p["out"]), m))
    bins = 4 ** 3
    add("cnt_kmer_counts_dev", [rd("bits"), wr("counts", bins * 8)], lambda p: L.cnt_kmer_counts_dev(vp(p["bits"]), N_LEN, 3, 0, vp(p["counts"]), bins + 5, None))
    add("cnt_kmer_counts", [rd("bits"), wr("counts", bins * 8)], lambda p: L.cnt_kmer_counts(vp(p["bits"]), N_LEN, 3, 0x10, vp(p["counts"]), bins))

    # the counted family: most > CAP for each, so CAP entries of every output can be written
    mk, mw = 5, 4
    assert N_LEN - mk + 1 - mw + 1 > CAP
    need = _query(L, L.cnt_minimizers_work_bytes, N_LEN, mk, mw)
    outs = [wr("pos", CAP * 8), wr("val", CAP * 8), wr("count", 8)]
    add("cnt_minimizers_dev", [rd("bits")] + outs + [wr("work", need)],
        lambda p: L.cnt_minimizers_dev(vp(p["bits"]), N_LEN, mk, mw, 0, vp(p["pos"]), vp(p["val"]), CAP, vp(p["count"]), vp(p["work"]), need + LENT, None))
    add("cnt_minimizers", [rd("bits")] + outs, lambda p: L.cnt_minimizers(vp(p["bits"]), N_LEN, mk, mw, 0x10, vp(p["pos"]), vp(p["val"]), CAP, vp(p["count"])))
    fk = 8
    need_f = _query(L, L.cnt_find_pattern_work_bytes, N_LEN, fk)
    outs = [wr("pos", CAP * 8), wr("info", CAP * 8), wr("count", 8)]
    add("cnt_find_pattern_dev", [rd("bits")] + outs + [wr("work", need_f)],
        lambda p: L.cnt_find_pattern_dev(vp(p["bits"]), N_LEN, 0x1B1B, fk, 0, 2, 0x20, vp(p["pos"]), vp(p["info"]), CAP, vp(p["count"]), vp(p["work"]),
                                         need_f + LENT, None))
    add("cnt_find_pattern", [rd("bits")] + outs,
        lambda p: L.cnt_find_pattern(vp(p["bits"]), N_LEN, 0x1B1B, fk, 0, 2, 0, vp(p["pos"]), vp(p["info"]), CAP, vp(p["count"])))
    need_o = _query(L, L.cnt_orfs_work_bytes, N_LEN)
    stops, starts = (1 << 2) | (1 << 14) | (1 << 50), 1 << 56
    outs = [wr("pos", CAP * 8), wr("length", CAP * 8), wr("info", CAP * 8), wr("count", 8)]
    add("cnt_orfs_dev", [rd("bits")] + outs + [wr("work", need_o)],
        lambda p: L.cnt_orfs_dev(vp(p["bits"]), N_LEN, stops, starts, 0, 0x200, vp(p["pos"]), vp(p["length"]), vp(p["info"]), CAP, vp(p["count"]),
                                 vp(p["work"]), need_o + LENT, None))
    add("cnt_orfs", [rd("bits")] + outs,
        lambda p: L.cnt_orfs(vp(p["bits"]), N_LEN, stops, 0, 0, 0, vp(p["pos"]), vp(p["length"]), vp(p["info"]), CAP, vp(p["count"])))
    # hpc: the footprint of out is cnt_words_for(min(len, out_cap)) words, pos holds min(len, out_cap) entries
    hcap = 70
    need_h = _query(L, L.cnt_hpc_work_bytes, N_LEN)
    outs = [wr("out", words_for(hcap) * 8), wr("pos", hcap * 8), wr("count", 8)]
    add("cnt_hpc_dev", [rd("bits")] + outs + [wr("work", need_h)],
        lambda p: L.cnt_hpc_dev(vp(p["bits"]), N_LEN, 0, vp(p["out"]), vp(p["pos"]), hcap, vp(p["count"]), vp(p["work"]), need_h + LENT, None))
    add("cnt_hpc", [rd("bits")] + outs, lambda p: L.cnt_hpc(vp(p["bits"]), N_LEN, 0, vp(p["out"]), vp(p["pos"]), hcap, vp(p["count"])))

    sub = 70
    R = words_for(sub)
    add("cnt_subseq_dev", [rd("bits"), wr("out", R * 8)], lambda p: L.cnt_subseq_dev(vp(p["bits"]), N_LEN, 5, sub, 0x40, vp(p["out"]), R + 3, None))
    add("cnt_subseq", [rd("bits"), wr("out", R * 8)], lambda p: L.cnt_subseq(vp(p["bits"]), N_LEN, 5, sub, 0, vp(p["out"]), R))
    n_reg, reg = 5, 40
    RR = words_for(reg)
    bufs = [rd("bits"), rd("start", n_reg * 8), rd("info", n_reg * 8), wr("out", n_reg * RR * 8), wr("rejected", 8)]
    add("cnt_extract_dev", bufs,
        lambda p: L.cnt_extract_dev(vp(p["bits"]), N_LEN, vp(p["start"]), vp(p["info"]), n_reg, reg, 0, vp(p["out"]), n_reg * RR, vp(p["rejected"]), None))
    add("cnt_extract", bufs,
        lambda p: L.cnt_extract(vp(p["bits"]), N_LEN, vp(p["start"]), vp(p["info"]), n_reg, reg, 0x40, vp(p["out"]), n_reg * RR + 2, up(p["rejected"])))
    tsub = 92
    M = tsub // 3  # 30 bytes at any byte address
    add("cnt_translate_dev", [rd("bits"), wr("out", M, 1)], lambda p: L.cnt_translate_dev(vp(p["bits"]), N_LEN, 1, tsub, 0x80, None, vp(p["out"]), M, None))
    add("cnt_translate", [rd("bits"), wr("out", M, 1)], lambda p: L.cnt_translate(vp(p["bits"]), N_LEN, 1, tsub, 0, None, vp(p["out"]), M + 9))
    return calls


EXPECTED_CALLS = {"cnt_" + n + t for n in ("hamming", "validate", "kmers", "kmer_counts", "minimizers", "find_pattern", "subseq", "extract", "translate",
                                           "orfs", "hpc") for t in ("", "_dev")} | {"cnt_complement_dev", "cnt_reverse_complement_dev"}


# ---- placements -----------------------------------------------------------------------------------------------------------------
SLOT = 8192  # every buffer of a call rests in the middle of a slot of its own: whatever moves stays 2 KiB and more from the others
OVERLAPS = ("identical start", "starts one element inside", "ends one element inside", "strictly inside", "strictly around")
TOUCHES = ("touching behind", "touching in front")


def down(x, a):
    return x - x % a


def place(topology, w, o, at):
    """the address of buffer w for this topology against buffer o resting at `at`, or None where the extents do not allow it.
    w is always on its own alignment; o's home is 128-B aligned."""
    a = w.align
    if topology == "identical start":
        return at
    if topology == "starts one element inside":  # the last place on w's alignment that still holds a byte of o
        return down(at + o.bytes - 1, a)
    if topology == "ends one element inside":  # w's last element holds o's first byte (a == 1: w's last byte IS o's first)
        assert w.bytes % a == 0
        return at + a - w.bytes
    if topology == "strictly inside":
        return at + a if w.bytes + 2 * a <= o.bytes else None
    if topology == "strictly around":
        return at - a if at - a + w.bytes >= at + o.bytes + 1 else None
    if topology == "touching behind":  # o's end is w's start (next place on w's alignment: every extent here ends on one)
        assert (at + o.bytes) % a == 0
        return at + o.bytes
    if topology == "touching in front":  # w's end is o's start
        assert (at - w.bytes) % a == 0
        return at - w.bytes
    raise AssertionError(topology)


def shared_bytes(p, w, o):
    return max(0, min(p[w.name] + w.bytes, p[o.name] + o.bytes) - max(p[w.name], p[o.name]))


class Arena:
    """one 128-B aligned host array of known contents in which all buffers of a call lie"""

    def __init__(self, slots=8):
        self.size = SLOT * slots
        self.raw = np.empty(self.size + 128, dtype=np.uint8)
        off = -self.raw.ctypes.data % 128
        self.view = self.raw[off : off + self.size]
        self.base = self.view.ctypes.data
        assert self.base % 128 == 0
        self.fill = np.random.default_rng(5).integers(0, 256, self.size, dtype=np.uint8)
        self.view[:] = self.fill

    def homes(self, call):
        assert len(call.bufs) <= self.size // SLOT, call.name
        return homes(call, self.base)

    def unchanged(self):
        return np.array_equal(self.view, self.fill)


def homes(call, base=0):
    """where the buffers of a call rest: far apart, each in the middle of its slot"""
    assert all(b.bytes + 16 <= SLOT // 4 for b in call.bufs), call.name
    return {b.name: base + SLOT * i + SLOT // 2 for i, b in enumerate(call.bufs)}


def pairs(call):
    return [(w, o) for w in call.bufs if w.written for o in call.bufs if o is not w]


def test_table_lists_every_packed_domain_entry_point(L):
    """the table against the header: every int cnt_*() declared between the packed-domain section's title and the device utilities
    is in it, except the scratch queries and the two host tiers whose overlaps are legal; extents come from the queries"""
    calls = table(L)
    names = [c.name for c in calls]
    assert len(set(names)) == len(names) and set(names) == EXPECTED_CALLS
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    section = header[header.index("---- packed-domain operations") : header.index("---- device utilities")]
    declared = set(re.findall(r"^int (cnt_\w+)\(", section, flags=re.M))
    assert declared - set(names) == {"cnt_complement", "cnt_reverse_complement", "cnt_minimizers_work_bytes", "cnt_find_pattern_work_bytes",
                                     "cnt_orfs_work_bytes", "cnt_hpc_work_bytes"}
    assert set(names) <= declared
    for c in calls:
        assert any(b.written for b in c.bufs) and not all(b.written for b in c.bufs), c.name
        if c.name.endswith("_dev") and c.name[4:-4] in ("minimizers", "find_pattern", "orfs", "hpc"):
            (work,) = [b for b in c.bufs if b.name == "work"]
            assert work.written and work.bytes >= 96  # one tile's scratch (hip/counted_output.hpp), from the query
        else:
            assert not [b for b in c.bufs if b.name == "work"]


def _call_ids():
    return sorted(EXPECTED_CALLS)


@pytest.mark.parametrize("name", _call_ids())
def test_written_buffer_overlapping_another_is_refused(L, name):
    """every (written, other) pair of the call at every overlapping placement the extents allow: CNT_EINVAL and nothing in the
    array moved -- a host count or distance lies in the array too, and a refused call leaves it alone.  The one exception:
    cnt_complement_dev exactly in place is NOT refused (it needs a device from there on: tried only where there is none)."""
    from cute_nucleotides_amd import _lib

    (call,) = [c for c in table(L) if c.name == name]
    arena = Arena()
    home = arena.homes(call)
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    wrong, tried = [], collections.Counter()
    for w, o in pairs(call):
        for topology in OVERLAPS:
            at = place(topology, w, o, home[o.name])
            if at is None:
                continue
            p = dict(home, **{w.name: at})
            assert at % w.align == 0 and shared_bytes(p, w, o) >= 1, (name, w.name, o.name, topology)
            if topology == "starts one element inside":
                assert shared_bytes(p, w, o) <= w.align
            if topology == "ends one element inside":
                assert shared_bytes(p, w, o) <= max(w.align, o.align)
            if topology == "identical start" and (w.name, o.name) in call.in_place:
                if count.value == 0:  # legal: past the checks it asks for a device
                    far = call.fn(home)
                    assert far != _lib.CNT_EINVAL and call.fn(p) == far, (name, "in place")
                    assert arena.unchanged()
                continue
            rc = call.fn(p)
            tried[topology] += 1
            if rc != _lib.CNT_EINVAL or not arena.unchanged():
                wrong.append((w.name, o.name, topology, rc, "array changed" if not arena.unchanged() else ""))
                arena.view[:] = arena.fill
    assert not wrong, (name, wrong)
    # the first three placements exist for every pair, and between them the last two for every pair of unequal extents
    n_pairs = len(pairs(call))
    for topology in OVERLAPS[1:3]:
        assert tried[topology] == n_pairs, (name, topology)
    assert tried[OVERLAPS[0]] == n_pairs - len(call.in_place)
    uneven = sum(1 for w, o in pairs(call) if abs(w.bytes - o.bytes) >= 2 * w.align + 1)
    assert tried[OVERLAPS[3]] + tried[OVERLAPS[4]] >= uneven, (name, tried)


def test_both_containments_are_exercised(L):
    """strictly inside and strictly around each happen for a written buffer of every kind: a count or counter inside an input and
    inside an output, an output around an input and inside one, scratch around a count and inside an output"""
    seen = collections.defaultdict(set)
    for call in table(L):
        home = homes(call)
        for w, o in pairs(call):
            for topology in OVERLAPS[3:]:
                if place(topology, w, o, home[o.name]) is not None:
                    seen[topology].add((call.name, w.name, o.name))
    inside, around = seen["strictly inside"], seen["strictly around"]
    for want in (("cnt_hamming_dev", "count", "a"), ("cnt_validate", "count", "n"), ("cnt_find_pattern_dev", "count", "pos"),
                 ("cnt_translate_dev", "out", "bits"), ("cnt_extract_dev", "rejected", "info"), ("cnt_hpc", "out", "pos"),
                 ("cnt_orfs_dev", "pos", "work")):
        assert want in inside, want
    for want in (("cnt_kmers_dev", "out", "bits"), ("cnt_kmer_counts", "counts", "bits"), ("cnt_minimizers_dev", "work", "count"),
                 ("cnt_find_pattern_dev", "work", "bits"), ("cnt_extract", "out", "start"), ("cnt_hpc_dev", "pos", "out"),
                 ("cnt_orfs", "pos", "count")):
        assert want in around, want


def _no_device(L):
    from cute_nucleotides_amd import _lib

    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    return count.value == 0


@pytest.mark.parametrize("name", _call_ids())
def test_touching_buffers_are_accepted(L, name):
    """every pair again with the two buffers touching, in both orders: no shared byte, so the call gets as far as the same call
    with its buffers far apart -- today the runtime's "no device" for the device tiers and CNT_ENODEV for the host tiers, which
    is not asserted.  Past the checks a call runs, and on a box with a device it would run on host pointers: only tried without
    one.  d_work is lent LENT bytes more than the query answers: a buffer that touches the query's extent lies inside what was
    lent, and is fine."""
    from cute_nucleotides_amd import _lib

    if not _no_device(L):
        pytest.skip("a HIP device is visible: an accepted call would run on these host pointers")
    (call,) = [c for c in table(L) if c.name == name]
    arena = Arena()
    home = arena.homes(call)
    far = call.fn(home)
    assert far not in (_lib.CNT_OK, _lib.CNT_EINVAL, _lib.CNT_ECAP), (name, far)
    wrong, zeroed = [], set(range(home["count"] - arena.base, home["count"] - arena.base + 8)) if name in ("cnt_hamming", "cnt_validate") else set()
    for w, o in pairs(call):
        for topology in TOUCHES:
            p = dict(home, **{w.name: place(topology, w, o, home[o.name])})
            assert shared_bytes(p, w, o) == 0 and (p[w.name] + w.bytes == p[o.name] or p[o.name] + o.bytes == p[w.name])
            rc = call.fn(p)
            if rc != far:
                wrong.append((w.name, o.name, topology, rc))
            if zeroed:
                zeroed |= set(range(p["count"] - arena.base, p["count"] - arena.base + 8))
    assert not wrong, (name, far, wrong)
    # cnt_hamming and cnt_validate zero their host result before they ask for a device; nothing else moved
    changed = set(np.flatnonzero(arena.view != arena.fill).tolist())
    assert changed <= zeroed, (name, sorted(changed - zeroed)[:8])


def test_read_only_buffers_may_overlap(L):
    """hamming's a and b at every placement, both tiers: the same status as far apart (no device here), and CNT_EINVAL never"""
    from cute_nucleotides_amd import _lib

    if not _no_device(L):
        pytest.skip("a HIP device is visible: an accepted call would run on these host pointers (the GPU part covers it)")
    for call in table(L):
        if call.name not in ("cnt_hamming", "cnt_hamming_dev"):
            continue
        arena = Arena()
        home = arena.homes(call)
        far = call.fn(home)
        assert far not in (_lib.CNT_OK, _lib.CNT_EINVAL)
        a, b = call.bufs[0], call.bufs[1]
        n = 0
        for w, o in ((a, b), (b, a)):
            for topology in OVERLAPS + TOUCHES:
                at = place(topology, w, o, home[o.name])
                if at is not None:
                    assert call.fn(dict(home, **{w.name: at})) == far, (call.name, w.name, topology)
                    n += 1
        assert n == 2 * 5  # equal extents: neither contains the other


def test_header_error_lists_mention_overlap_for_every_call(L):
    """the comment in front of each call's declaration states its overlap errors, so the header and the table stay in step; the
    four oldest calls share one comment, in which each has a paragraph of its own"""
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    for call in table(L):
        at = header.index("int %s(" % call.name)
        comment = header[header.rindex("\n/*", 0, at) : at]  # the comment that begins a line, not the ones behind a #define
        assert comment.index("*/") < len(comment) and "overlapping" in comment and "CNT_EINVAL" in comment, call.name
        for b in call.bufs:  # every written buffer but the plain outputs is named where overlap is spoken of
            if b.written and b.name in ("count", "work", "rejected"):
                word = {"count": "count", "work": "d_work", "rejected": "rejected"}[b.name]
                assert re.search(r"%s\w*[^.;:]*overlapping|overlapping[^.;:]*%s" % (word, word), comment, flags=re.S), (call.name, b.name)
    old = header[header.index(" * SHARED MEMORY, every call of this section") : header.index("#define CNT_ALLOW_N")]
    for rule in ("WRITES shares no byte", "only READS may overlap", "d_out == d_bits EXACTLY", "*_work_bytes", "before any device work", "merely touch"):
        assert rule in old, rule
    ops = ["hamming", "complement", "reverse_complement", "validate"]
    starts = [old.index("\n *   %s " % op) for op in ops] + [len(old)]
    assert starts == sorted(starts)
    for op, lo, hi in zip(ops, starts, starts[1:]):
        assert "overlap" in old[lo:hi] and "CNT_EINVAL" in old[lo:hi], op
    assert "in place" in old[starts[1] : starts[2]] and "Host tier: any overlap is legal" in old[starts[2] : starts[3]]
    assert "codec call" not in header[: header.index("#ifndef CUTE_NT_H")]  # the rule is no longer the codec's alone
    (einval,) = re.findall(r"#define CNT_EINVAL 1 /\*(.*?)\*/", header, flags=re.S)
    assert "overlapping" in einval and "codec" not in einval


def test_argument_contract_of_the_four_oldest_calls(L):
    """cnt_hamming*, cnt_complement*, cnt_reverse_complement*, cnt_validate*: NULL and misaligned pointers, the unknown flag, empty
    work, the host tiers' result pointers -- all answered before any device work"""
    from cute_nucleotides_amd import _lib

    EINVAL, OK = _lib.CNT_EINVAL, _lib.CNT_OK
    arena = Arena(2)
    q = lambda off: ctypes.c_void_p(arena.base + off)  # noqa: E731
    a, b, out, cnt = 0, 1024, 2048, 4096
    # device tier: NULL for each pointer with len > 0, each word pointer at +4 bytes
    dev = [(L.cnt_hamming_dev, lambda x, y, z: (x, y, N_LEN, z, None), (a, b, cnt), 3),
           (L.cnt_complement_dev, lambda x, y: (x, N_LEN, y, None), (a, out), 2),
           (L.cnt_reverse_complement_dev, lambda x, y: (x, N_LEN, y, None), (a, out), 2),
           (L.cnt_validate_dev, lambda x, y: (x, N_LEN, 0, y, None), (a, cnt), 2)]
    for fn, args, offs, n in dev:
        for i in range(n):
            ptrs = [q(o) for o in offs]
            ptrs[i] = None
            assert fn(*args(*ptrs)) == EINVAL, (fn.__name__, "NULL", i)
            if fn is L.cnt_validate_dev and i == 0:
                continue  # ASCII: any alignment
            for byte in (4, 1, 7):
                ptrs = [q(o) for o in offs]
                ptrs[i] = q(offs[i] + byte)
                assert fn(*args(*ptrs)) == EINVAL, (fn.__name__, "misaligned", i, byte)
    # len == 0: CNT_OK whatever the pointers are
    assert L.cnt_hamming_dev(None, None, 0, None, None) == OK and L.cnt_hamming_dev(q(4), q(4), 0, q(4), None) == OK
    assert L.cnt_complement_dev(None, 0, None, None) == OK and L.cnt_reverse_complement_dev(None, 0, None, None) == OK
    assert L.cnt_reverse_complement_dev(q(a), 0, q(a), None) == OK  # nothing to do: not an overlap either
    assert L.cnt_validate_dev(None, 0, 0, None, None) == OK and L.cnt_validate_dev(None, 0, 2, None, None) == OK
    # validate's unknown flag is CNT_EINVAL even without work; CNT_ALLOW_N = 2 is the one flag
    for flags in (1, 4, 0x10, 0x80000000, 3):
        assert L.cnt_validate_dev(q(a), N_LEN, flags, q(cnt), None) == EINVAL, flags
        assert L.cnt_validate_dev(None, 0, flags, None, None) == EINVAL, flags
        inv = ctypes.c_uint64(99)
        assert L.cnt_validate(q(a), N_LEN, flags, ctypes.byref(inv)) == EINVAL and inv.value == 0, flags
        inv = ctypes.c_uint64(99)
        assert L.cnt_validate(None, 0, flags, ctypes.byref(inv)) == EINVAL and inv.value == 0, flags
    # host tier: the result pointer is never optional, and is zeroed before the checks behind it fail
    assert L.cnt_hamming(q(a), q(b), N_LEN, None) == EINVAL and L.cnt_hamming(None, None, 0, None) == EINVAL
    assert L.cnt_validate(q(a), N_LEN, 0, None) == EINVAL and L.cnt_validate(None, 0, 0, None) == EINVAL
    for x, y in ((None, q(b)), (q(a), None), (None, None)):
        d = ctypes.c_uint64(99)
        assert L.cnt_hamming(x, y, N_LEN, ctypes.byref(d)) == EINVAL and d.value == 0
    d = ctypes.c_uint64(99)
    assert L.cnt_hamming(None, None, 0, ctypes.byref(d)) == OK and d.value == 0
    inv = ctypes.c_uint64(99)
    assert L.cnt_validate(None, N_LEN, 0, ctypes.byref(inv)) == EINVAL and inv.value == 0
    inv = ctypes.c_uint64(99)
    assert L.cnt_validate(None, 0, 2, ctypes.byref(inv)) == OK and inv.value == 0
    for fn in (L.cnt_complement, L.cnt_reverse_complement):
        assert fn(None, N_LEN, q(out)) == EINVAL and fn(q(a), N_LEN, None) == EINVAL and fn(None, 0, None) == OK
    assert arena.unchanged()


# ---------------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
SENTINEL = 0x3C5A3C5A3C5A3C5A  # as int64 and in every byte lane distinguishable from zeros and from small counts
TILE_WORDS = 512  # complement and reverse-complement tiles (16384 nt); a head is at most 15 words
BIG = 3 * TILE_WORDS * 32 + 15 * 32 + 7  # tiles, a head at every phase but 0, and a ragged tail


def random_words(rng, n_len, garbage=True):
    """the packed words of a random sequence, with garbage above len in the last word"""
    w = rng.integers(0, 2**64, max(words_for(n_len), 1), dtype=np.uint64)
    if n_len & 31 and not garbage:
        w[-1] &= np.uint64((1 << (2 * (n_len & 31))) - 1)
    return w


def _i64(words):
    import torch

    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64))


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def in_place_complement(oracle, rng, n_len, phase):
    """complement_dev(x, n, out=x) with x `phase` words off a 128-B line, sentinels on both sides"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    words = words_for(n_len)
    orig = random_words(rng, n_len)
    front = 16 + phase
    buf = torch.full((front + words + 16,), SENTINEL, dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 128 == 0
    x = buf[front : front + words]
    x.copy_(_i64(orig))
    got = po.complement_dev(x, n_len, out=x)
    torch.cuda.synchronize()
    assert got.data_ptr() == x.data_ptr()
    h = buf.cpu().numpy()
    want = oracle.complement(orig, n_len)
    bad = np.flatnonzero(h[front : front + words].view(np.uint64) != want)
    assert bad.size == 0, (n_len, phase, bad[:4].tolist())
    assert (h[:front] == SENTINEL).all() and (h[front + words :] == SENTINEL).all(), (n_len, phase, "sentinel")


@gpu
@pytest.mark.parametrize("n_len", [1, 31, 32, 33, 511 * 32, 512 * 32, BIG])
def test_gpu_complement_in_place(oracle, n_len):
    """exactly in place is race-free by construction (each lane stores the words it loaded) and documented: every path of the
    launcher -- words only, one tile short, exactly one tile, tiles with head and tail -- at four phases of the buffer"""
    rng = np.random.default_rng(n_len)
    for phase in (0, 1, 2, 15):
        in_place_complement(oracle, rng, n_len, phase)


@gpu
def test_gpu_complement_in_place_across_a_launch_split(oracle, launch_tiles):
    words = launch_tiles * TILE_WORDS * 2 + TILE_WORDS * 5 + 77
    in_place_complement(oracle, np.random.default_rng(launch_tiles), 32 * words - 9, 3)


class Touching:
    """one device allocation [sentinel | parts, back to back | sentinel]; a part is (name, bytes); word parts start 8-B aligned"""

    def __init__(self, parts):
        import torch

        self.torch = torch
        self.front = 128
        self.at, off = {}, self.front
        for name, nbytes in parts:
            self.at[name] = (off, nbytes)
            off += nbytes
        self.end = off
        self.raw = torch.full((off + 128,), 0x5A, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 128 == 0

    def words(self, name):
        off, nbytes = self.at[name]
        assert off % 8 == 0 and nbytes % 8 == 0, (name, off, nbytes)
        return self.raw[off : off + nbytes].view(self.torch.int64)

    def bytes(self, name):
        off, nbytes = self.at[name]
        return self.raw[off : off + nbytes]

    def assert_sentinels(self, tag):
        h = self.raw.cpu().numpy()
        assert (h[: self.front] == 0x5A).all() and (h[self.end :] == 0x5A).all(), tag


def _touching_cases(oracle):
    """(name, input nt, parts of the output side as (name, bytes), run(bits, outs) -> None, check(orig, outs) -> None)"""
    from cute_nucleotides_amd import packed_ops as po
    from test_extract import np_subseq
    from test_hpc import np_hpc, pack
    from test_find_pattern import codes_of
    from test_kmer_counts import reference as counts_reference
    from test_translate import np_translate

    cases = []

    def unary(fn, ref):
        def run(bits, n, o):
            fn(bits, n, out=o["out"])

        def check(orig, n, o):
            assert np.array_equal(_u64(o["out"]), ref(orig, n))

        return run, check

    for name, fn, ref in (("complement", po.complement_dev, oracle.complement), ("reverse_complement", po.reverse_complement_dev, oracle.reverse_complement)):
        cases.append((name, BIG, [("out", words_for(BIG) * 8)], *unary(fn, ref)))

    n, k = 3000, 17
    cases.append(("kmers", n, [("out", (n - k + 1) * 8)], lambda bits, n, o: po.kmers_dev(bits, n, 17, out=o["out"]),
                  lambda orig, n, o: np.testing.assert_array_equal(_u64(o["out"]), oracle.kmers(orig, n, 17))))
    n, sub = 20000, 20000 - 5 - 3
    cases.append(("subseq", n, [("out", words_for(sub) * 8)], lambda bits, n, o: po.subseq_dev(bits, n, 5, n - 8, out=o["out"]),
                  lambda orig, n, o: np.testing.assert_array_equal(_u64(o["out"]), np_subseq(orig, n, 5, n - 8))))
    # translate at start 1: M bytes directly behind the words; in front of them M is a multiple of 8, so that the words stay aligned
    for n, sub in ((40000, 39999), (40000, 3 * 13328)):
        M = sub // 3
        cases.append(("translate %d" % M, n, [("out8", M)], lambda bits, n, o, sub=sub: po.translate_dev(bits, n, 1, sub, out=o["out8"]),
                      lambda orig, n, o, sub=sub: np.testing.assert_array_equal(o["out8"].cpu().numpy(), np_translate(orig, n, 1, sub))))
    n = 3 * 8192 + 77

    def run_hpc(bits, n, o):
        import torch

        o["count"] = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
        work = torch.empty(po.hpc_work_bytes(n), dtype=torch.uint8, device="cuda")
        po.hpc_dev(bits, n, o["out"], o["count"], work, pos=o["pos"])

    def check_hpc(orig, n, o):
        ref, rpos = np_hpc(codes_of(orig, n))
        assert int(o["count"].item()) == ref.size
        want = pack(ref)
        assert np.array_equal(_u64(o["out"])[: want.size], want) and np.array_equal(_u64(o["pos"])[: ref.size], rpos)

    cases.append(("hpc", n, [("out", words_for(n) * 8), ("pos", n * 8)], run_hpc, check_hpc))

    def run_counts(bits, n, o):
        o["counts"].zero_()  # the device tier ADDS to a table the caller zeroed
        po.kmer_counts_dev(bits, n, 3, out=o["counts"])

    cases.append(("kmer_counts", 5000, [("counts", 64 * 8)], run_counts,
                  lambda orig, n, o: np.testing.assert_array_equal(_u64(o["counts"]), counts_reference(oracle, orig, n, 3))))
    return cases


@gpu
@pytest.mark.parametrize("order", ["in|out", "out|in"])
def test_gpu_touching_device_buffers(oracle, order):
    """the end of one buffer is the start of the other, no shared byte, in both orders: the call is accepted, computes the
    reference, leaves its input words as they were and the sentinels on the far sides intact"""
    import torch

    rng = np.random.default_rng(41)
    ran = []
    for name, n_len, out_parts, run, check in _touching_cases(oracle):
        in_part = [("in", words_for(n_len) * 8)]
        if order == "out|in" and sum(b for _, b in out_parts) % 8:
            continue  # the odd M of translate: the words behind it would be misaligned
        parts = in_part + out_parts if order == "in|out" else out_parts[::-1] + in_part
        t = Touching(parts)
        orig = random_words(rng, n_len)
        bits = t.words("in")
        bits.copy_(_i64(orig))
        outs = {nm: (t.bytes(nm) if nm == "out8" else t.words(nm)) for nm, _ in out_parts}
        first, last = parts[0][0], parts[-1][0]
        assert t.at[first][0] == t.front and sum(t.at[last]) == t.end
        for (n0, _), (n1, _) in zip(parts, parts[1:]):
            assert sum(t.at[n0]) == t.at[n1][0]  # back to back
        run(bits, n_len, outs)
        torch.cuda.synchronize()
        check(orig, n_len, outs)
        assert np.array_equal(_u64(bits), orig), (name, order, "input changed")
        t.assert_sentinels((name, order))
        ran.append(name)
    assert len(ran) == (8 if order == "in|out" else 7) and {"complement", "reverse_complement", "kmers", "subseq", "hpc", "kmer_counts"} <= set(ran)
    assert any(r.startswith("translate") for r in ran)


@gpu
def test_gpu_hamming_of_overlapping_streams(oracle):
    """buffers a call only reads may overlap in any way: a sequence against itself shifted by 1, 2, 16 and 1024 words (one
    persistent piece is 1024 words), whole words and a ragged end; against itself unshifted the distance is 0"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(42)
    w = 2 * 1024 + 40
    host = rng.integers(0, 2**64, w + 1024, dtype=np.uint64)
    x = _i64(host).cuda()
    for k in (1, 2, 16, 1024):
        for n_len in (32 * w, 32 * w - 45):
            got = int(po.hamming_dev(x[0:w], x[k : k + w], n_len).item())
            want = oracle.hamming(host[0:w], host[k : k + w], n_len)
            assert got == want and want > n_len // 2, (k, n_len, got, want)
    for n_len in (32 * w, 32 * w - 45):
        assert int(po.hamming_dev(x[:w], x[:w], n_len).item()) == 0
    assert int(po.hamming_dev(x, x, 32 * x.numel()).item()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_u64(x), host)


@gpu
def test_gpu_python_layer_hands_the_refusals_on(oracle):
    import torch

    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(43)
    w = 700
    n_len = 32 * w - 3
    host = rng.integers(0, 2**64, w + 4, dtype=np.uint64)
    x = _i64(host).cuda()
    for call in (lambda: po.reverse_complement_dev(x[:w], n_len, out=x[:w]), lambda: po.reverse_complement_dev(x[:w], n_len, out=x[1 : 1 + w]),
                 lambda: po.complement_dev(x[:w], n_len, out=x[2 : 2 + w])):
        with pytest.raises(_lib.CuteNtError) as e:
            call()
        assert e.value.status == _lib.CNT_EINVAL
        torch.cuda.synchronize()
        assert np.array_equal(_u64(x), host)
    # ... and what is legal beside them still runs: in place, and behind the input
    assert np.array_equal(_u64(po.complement_dev(x[:w], n_len, out=x[:w])), oracle.complement(host[:w], n_len))
