"""k-mer counting on packed words (include/cute_nt.h "k-mer counts"): counts[v] = the number of k-mers whose cnt_kmers value
is v, over 4^k bins, k = 1..12, forward and canonical.  Every comparison is exact.  The reference is a bincount of the scalar
oracle's k-mers (oracle.kmers, which tests/test_kmers.py holds to the definition in letters); the CPU part pins that
reference against letters for k = 1..3 and checks the ABI's argument errors, the wrappers and the ISA of the two kernels.
The GPU part compares both tiers with the reference at every k: lengths around the word and tile edges, random / all-A /
period-2 / period-3 / poly-T-run inputs, garbage above len, every 8-B phase of the input, the device tier's ADD and the
host tier's SET semantics, pinned and registered host buffers, a captured graph, 2^33 nt through one 32-bit LDS counter
path, and 2^32 nt against torch.bincount over kmers_dev."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = bytes.maketrans(b"ACGT", b"TGCA")
CNT_KMER_CANONICAL = 0x10
MAX_K = 12
LDS_MAX_K = 7  # kKmerCountLdsMaxK
TILE = 32 * 1024  # k-mers per tile of kmer_count: kKmerCountBlock lanes x 32
KS = list(range(1, MAX_K + 1))
CODE = {"A": 0, "C": 1, "T": 2, "G": 3}


def reference(oracle, words, n_len, k, canonical=False):
    return np.bincount(oracle.kmers(words, n_len, k, canonical).astype(np.int64), minlength=4 ** k).astype(np.uint64)


def _value(kmer):
    """a k-mer in letters -> its packed value (first letter in the low bits)"""
    return sum(CODE[c] << (2 * j) for j, c in enumerate(kmer))


def _canonical_value(kmer):
    return min(_value(kmer), _value(kmer.translate({65: 84, 84: 65, 67: 71, 71: 67})[::-1]))


def _pack(oracle, s):
    return oracle.n_to_bits_lut(np.frombuffer(s, dtype=np.uint8))


# ---- the reference against letters ------------------------------------------------------------------------------------
def test_reference_is_base_composition_for_k1(oracle):
    for n_len in (0, 1, 31, 32, 33, 1000, 4099):
        s = oracle.fill_random_acgt(n_len, seed=50 + n_len).tobytes()
        got = reference(oracle, _pack(oracle, s), n_len, 1)
        assert got.tolist() == [s.count(b"A"), s.count(b"C"), s.count(b"T"), s.count(b"G")], n_len
        assert int(got.sum()) == n_len


@pytest.mark.parametrize("k", [2, 3])
def test_reference_counts_substrings(oracle, k):
    import itertools

    for n_len in (0, k - 1, k, 33, 64, 1000, 4099):
        s = oracle.fill_random_acgt(n_len, seed=70 + n_len + k).tobytes()
        text = s.decode()
        m = max(n_len - k + 1, 0)
        words = _pack(oracle, s)
        fwd, can = reference(oracle, words, n_len, k), reference(oracle, words, n_len, k, True)
        want_f, want_c = np.zeros(4 ** k, dtype=np.uint64), np.zeros(4 ** k, dtype=np.uint64)
        for letters in itertools.product("ACGT", repeat=k):
            kmer = "".join(letters)
            n = sum(1 for i in range(m) if text[i : i + k] == kmer)  # overlapping occurrences
            want_f[_value(kmer)] += np.uint64(n)
            want_c[_canonical_value(kmer)] += np.uint64(n)
        assert np.array_equal(fwd, want_f) and np.array_equal(can, want_c), (n_len, k)
        assert int(fwd.sum()) == m and int(can.sum()) == m
        # bins of non-canonical values are zero
        non_canonical = [_value("".join(x)) for x in itertools.product("ACGT", repeat=k) if _canonical_value("".join(x)) != _value("".join(x))]
        assert non_canonical and not can[non_canonical].any()


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 12])
def test_reference_of_the_reverse_complement_is_a_permutation_of_bins(oracle, k):
    """the forward spectrum of revcomp(s) is the forward spectrum of s with bin v moved to bin rc(v)"""
    n_len = 4099
    s = oracle.fill_random_acgt(n_len, seed=90 + k).tobytes()
    fwd = reference(oracle, _pack(oracle, s), n_len, k)
    rev = reference(oracle, _pack(oracle, s.translate(COMP)[::-1]), n_len, k)
    v = np.arange(4 ** k, dtype=np.uint64)
    rc = np.zeros_like(v)
    for j in range(k):  # code j of v, complemented (^2), lands at position k-1-j
        rc |= (((v >> np.uint64(2 * j)) & np.uint64(3)) ^ np.uint64(2)) << np.uint64(2 * (k - 1 - j))
    assert np.array_equal(rev[rc.astype(np.int64)], fwd)
    assert np.array_equal(reference(oracle, _pack(oracle, s), n_len, k, True), reference(oracle, _pack(oracle, s.translate(COMP)[::-1]), n_len, k, True))


# ---- ABI, no device needed ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


def test_abi_errors_come_before_any_device_work(L):
    from cute_nucleotides_amd import _lib

    buf = np.zeros(4096, dtype=np.uint64)
    base = buf.ctypes.data
    q = lambda word, byte=0: ctypes.c_void_p(base + 8 * word + byte)  # noqa: E731
    out = np.full(256, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    o = lambda byte=0: ctypes.c_void_p(out.ctypes.data + byte)  # noqa: E731
    for fn, tail, host in ((L.cnt_kmer_counts, (), True), (L.cnt_kmer_counts_dev, (None,), False)):
        call = lambda *a: fn(*(a + tail))  # noqa: E731
        for k in (0, 13, 32, 64):  # k out of range -- even when there would be no k-mer
            assert call(q(0), 100, k, 0, o(), 256) == _lib.CNT_EINVAL, (fn, k)
            assert call(None, 0, k, 0, None, 0) == _lib.CNT_EINVAL
        for flags in (0x1, 0x2, 0x4, 0x8, 0x20, 0x80000000, CNT_KMER_CANONICAL | 0x1):
            assert call(q(0), 100, 4, flags, o(), 256) == _lib.CNT_EINVAL, (fn, flags)
        assert call(None, 100, 4, 0, o(), 256) == _lib.CNT_EINVAL  # NULL pointers when there is work
        assert call(q(0), 100, 4, 0, None, 256) == _lib.CNT_EINVAL
        for byte in (1, 4, 7):  # pointers not 8-B aligned
            assert call(q(0, byte), 100, 4, 0, o(), 256) == _lib.CNT_EINVAL
            assert call(q(0), 100, 4, CNT_KMER_CANONICAL, o(byte), 256) == _lib.CNT_EINVAL
        # the table overlapping the input words (100 nt = 4 words at q(300)): inside, straddling either end, identical
        for tw in (300, 302, 303, 100, 48):
            assert call(q(300), 100, 4, 0, q(tw), 256) == _lib.CNT_EINVAL, (fn, tw)
        # capacity: 4^k - 1 entries
        for k in (1, 4, 7, 8, 12):
            assert call(q(0), 100, k, 0, o(), 4 ** k - 1) == _lib.CNT_ECAP, (fn, k)
        # len < k: the device tier has nothing to do, whatever the pointers are
        if not host:
            assert call(None, 0, 1, 0, None, 0) == _lib.CNT_OK
            assert call(None, 11, 12, CNT_KMER_CANONICAL, None, 0) == _lib.CNT_OK
            assert call(q(0), 3, 4, 0, o(), 0) == _lib.CNT_OK
    assert (out == 0x5A5A5A5A5A5A5A5A).all()  # nothing was written
    # len < k on the host tier: its table is still checked, and SET to zero -- without a device
    assert L.cnt_kmer_counts(None, 0, 1, 0, None, 4) == _lib.CNT_EINVAL
    assert L.cnt_kmer_counts(None, 3, 4, 0, o(), 255) == _lib.CNT_ECAP
    assert (out == 0x5A5A5A5A5A5A5A5A).all()
    assert L.cnt_kmer_counts(None, 3, 4, CNT_KMER_CANONICAL, o(), 256) == _lib.CNT_OK and not out.any()
    out[:] = 0x5A5A5A5A5A5A5A5A
    assert L.cnt_kmer_counts(q(0), 1, 2, 0, o(), 200) == _lib.CNT_OK
    assert not out[:16].any() and (out[16:] == 0x5A5A5A5A5A5A5A5A).all()  # entries past 4^k are never written
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    if count.value == 0:
        out[:] = 0x5A5A5A5A5A5A5A5A
        for flags in (0, CNT_KMER_CANONICAL):  # past the argument checks a call needs a device
            assert L.cnt_kmer_counts(q(0), 100, 4, flags, o(), 256) == _lib.CNT_ENODEV
            assert L.cnt_kmer_counts_dev(q(0), 100, 4, flags, o(), 256, None) < 0
        assert (out == 0x5A5A5A5A5A5A5A5A).all()


def test_python_wrappers_raise_value_error(L):
    from cute_nucleotides_amd import packed_ops as po

    w = np.zeros(2, dtype=np.uint64)
    for k in (0, 13, 32):
        with pytest.raises(ValueError):
            po.kmer_counts_hip(w, 64, k)
        with pytest.raises(ValueError):
            po.kmer_counts_dev(None, 64, k)  # before the tensor is looked at, before any library call
    with pytest.raises(ValueError):
        po.kmer_counts_hip(w, 65, 4)  # longer than the words hold
    got = po.kmer_counts_hip(w, 3, 4, canonical=True)  # no k-mer: 4^k zeros, no device needed
    assert got.dtype == np.uint64 and got.shape == (256,) and not got.any()


def test_abi_wiring(L):
    import subprocess

    from cute_nucleotides_amd import _lib, packed_ops as po

    for name in ("cnt_kmer_counts", "cnt_kmer_counts_dev"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert {"cnt_kmer_counts", "cnt_kmer_counts_dev"} <= exported
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    assert "#define CNT_KMER_COUNTS_MAX_K 12" in header and po.KMER_COUNTS_MAX_K == MAX_K
    src = open(os.path.join(ROOT, "hip", "kmer_count_kernels.hpp")).read()
    assert "constexpr int kKmerCountLdsMaxK = %d;" % LDS_MAX_K in src and "constexpr int kKmerCountBlock = %d;" % (TILE // 32) in src
    assert "static_assert(kKmerCountMaxTilesPerGroup * kKmerCountTileKmers < (1ull << 32)" in src  # the flush bound


KERNELS = {"lds": "void cnt::kmer_count<true>", "global": "void cnt::kmer_count<false>"}


def test_kmer_count_kernels_isa():
    sys.path.insert(0, os.path.join(ROOT, "bench"))
    import isa_digest

    found = isa_digest.kernels(isa_digest.assembly())
    for name in KERNELS.values():
        assert name in found, name
        e = found[name]
        assert not [i for i in e["body"] if "scratch_" in i], name
        assert e["meta"]["private_segment_fixed_size"] == 0 and e["meta"]["next_free_vgpr"] <= 84, (name, e["meta"])
    lds, glob = found[KERNELS["lds"]], found[KERNELS["global"]]
    assert 0 < lds["meta"]["group_segment_fixed_size"] <= 65536 and glob["meta"]["group_segment_fixed_size"] == 0
    assert [i for i in lds["body"] if i.startswith("ds_add_u32")]
    assert not [i for i in lds["body"] if i.startswith("ds_add_rtn")]  # no-return adds
    for e in (lds, glob):  # the flush of the one, every add of the other: one 64-bit atomic add, no compare-and-swap loop
        assert [i for i in e["body"] if i.startswith(("global_atomic_add_x2", "buffer_atomic_add_x2"))]
        assert not [i for i in e["body"] if "cmpswap" in i]
        assert not [i for i in e["body"] if "atomic_add" in i and ("sc0" in i.split() or "glc" in i.split())]  # no-return
    assert len(found) < 60, len(found)


# ---------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
SIZES = [0, "k-1", "k", 31, 32, 33, 63, 64, 65, 1000, 4099, TILE - 1, TILE, TILE + 1, 32 * TILE + 31, (1 << 22) + 5]


def _sizes(k):
    return sorted({(k - 1 if s == "k-1" else k if s == "k" else s) for s in SIZES} | {TILE + k - 2, TILE + k - 1, TILE + k})  # m just below / at / above one tile


def _patterns(oracle, n_len, seed):
    """(name, ASCII) of the five inputs of a length"""
    rnd = oracle.fill_random_acgt(n_len, seed=seed)
    run = rnd.copy()
    if n_len > 100000:
        lo = (n_len - 100000) // 2
        run[lo : lo + 100000] = ord("T")
    else:
        run[n_len // 4 : n_len - n_len // 4] = ord("T")
    rep = lambda unit: np.frombuffer((unit * (n_len // len(unit) + 1))[:n_len], dtype=np.uint8)  # noqa: E731
    return [("random", rnd), ("all-A", rep(b"A")), ("AC", rep(b"AC")), ("ACG", rep(b"ACG")), ("poly-T run", run)]


def _host(bits, n_len, k, canonical):
    from cute_nucleotides_amd import packed_ops as po

    return po.kmer_counts_hip(bits, n_len, k, canonical=canonical)


def _dev(d_bits, n_len, k, canonical, out=None):
    from cute_nucleotides_amd import packed_ops as po

    return po.kmer_counts_dev(d_bits, n_len, k, canonical=canonical, out=out).cpu().numpy().view(np.uint64)


@gpu
@pytest.mark.parametrize("k", KS)
def test_gpu_counts_match_reference(oracle, k):
    import torch

    for n_len in _sizes(k):
        for name, s in _patterns(oracle, n_len, seed=300 + k):
            w = oracle.n_to_bits_lut(s)
            d = torch.from_numpy(w.view(np.int64)).cuda() if n_len else torch.zeros(1, dtype=torch.int64, device="cuda")
            for canonical in (False, True):
                want = reference(oracle, w, n_len, k, canonical)
                assert int(want.sum()) == max(n_len - k + 1, 0)
                assert np.array_equal(_dev(d, n_len, k, canonical), want), (n_len, k, name, canonical, "device")
                assert np.array_equal(_host(w, n_len, k, canonical), want), (n_len, k, name, canonical, "host")


@gpu
def test_gpu_counts_ignore_garbage_and_take_every_input_phase(oracle):
    """garbage above len in the last word and in a word past it; the input as a view at word offsets 0..3 of an allocation"""
    import torch

    rng = np.random.default_rng(12)
    for k in (1, 3, 5, 7, 8, 12):
        for n_len in (1000, 32 * 100, TILE + 77, 3 * TILE + 32 * 5 + 9):
            nw = (n_len + 31) // 32
            clean = oracle.n_to_bits_lut(oracle.fill_random_acgt(n_len, seed=n_len + k))
            dirty = np.concatenate([clean, rng.integers(0, 2**64, 1, dtype=np.uint64)])
            if n_len & 31:
                dirty[nw - 1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(2 * (n_len & 31))
            for canonical in (False, True):
                want = reference(oracle, clean, n_len, k, canonical)
                assert np.array_equal(_host(dirty, n_len, k, canonical), want), (k, n_len, canonical, "host")
                for phase in range(4):
                    big = torch.from_numpy(rng.integers(-2**63, 2**63, nw + 8, dtype=np.int64)).cuda()
                    big[phase : phase + nw + 1] = torch.from_numpy(dirty.view(np.int64)).cuda()
                    view = big[phase : phase + nw + 1]
                    assert view.data_ptr() % 32 == (big.data_ptr() + 8 * phase) % 32
                    assert np.array_equal(_dev(view, n_len, k, canonical), want), (k, n_len, canonical, phase)


@gpu
def test_gpu_device_tier_adds_and_host_tier_sets(oracle):
    import torch

    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(3)
    for k in (1, 4, 7, 8, 10):
        bins = 4 ** k
        a_len, b_len = 3 * TILE + 17, 50001
        a = oracle.n_to_bits_lut(oracle.fill_random_acgt(a_len, seed=k))
        b = oracle.n_to_bits_lut(oracle.fill_random_acgt(b_len, seed=100 + k))
        da, db = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(b.view(np.int64)).cuda()
        for canonical in (False, True):
            ra, rb = reference(oracle, a, a_len, k, canonical), reference(oracle, b, b_len, k, canonical)
            # a pre-filled table comes back as pattern + reference; entries past 4^k are untouched
            pattern = rng.integers(0, 2**62, bins + 5, dtype=np.int64)
            table = torch.from_numpy(pattern.copy()).cuda()
            got = po.kmer_counts_dev(da, a_len, k, canonical=canonical, out=table)
            assert got.data_ptr() == table.data_ptr() and got.numel() == bins
            t = table.cpu().numpy()
            assert np.array_equal(t[:bins].view(np.uint64), pattern[:bins].view(np.uint64) + ra), (k, canonical)
            assert np.array_equal(t[bins:], pattern[bins:])
            # two sequences into one table
            table = torch.zeros(bins, dtype=torch.int64, device="cuda")
            po.kmer_counts_dev(da, a_len, k, canonical=canonical, out=table)
            po.kmer_counts_dev(db, b_len, k, canonical=canonical, out=table)
            assert np.array_equal(table.cpu().numpy().view(np.uint64), ra + rb), (k, canonical)
            # a sequence with no k-mer adds nothing
            po.kmer_counts_dev(db, k - 1, k, canonical=canonical, out=table)
            assert np.array_equal(table.cpu().numpy().view(np.uint64), ra + rb)
            # the host tier overwrites garbage with exactly the reference, and nothing past 4^k
            out = rng.integers(0, 2**64, bins + 3, dtype=np.uint64)
            keep = out[bins:].copy()
            _lib.check(_lib.lib().cnt_kmer_counts(a.ctypes.data, a_len, k, CNT_KMER_CANONICAL if canonical else 0, out.ctypes.data, out.size))
            assert np.array_equal(out[:bins], ra) and np.array_equal(out[bins:], keep), (k, canonical)


@gpu
def test_gpu_host_tier_with_pageable_pinned_and_registered_buffers(oracle):
    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib

    for k, n_len in ((3, 100003), (7, (1 << 20) + 3), (9, 3 * TILE + 1)):
        bins, nw = 4 ** k, (n_len + 31) // 32
        w = oracle.n_to_bits_lut(oracle.fill_random_acgt(n_len, seed=7 + k))
        want = reference(oracle, w, n_len, k, True)

        def call(bits, out):
            out[:] = 0xDEADBEEFDEADBEEF
            _lib.check(_lib.lib().cnt_kmer_counts(bits.ctypes.data, n_len, k, CNT_KMER_CANONICAL, out.ctypes.data, out.size))
            assert np.array_equal(out[:bins], want) and (out[bins:] == 0xDEADBEEFDEADBEEF).all(), (k, n_len)

        pin_in, pin_out = cn.pinned_empty(nw, np.uint64), cn.pinned_empty(bins + 2, np.uint64)
        pin_in[:] = w
        reg_in, reg_out = w.copy(), np.empty(bins + 2, dtype=np.uint64)
        assert cn.is_pinned(pin_in) and cn.is_pinned(pin_out) and not cn.is_pinned(w)
        with cn.host_registered(reg_in), cn.host_registered(reg_out):
            assert cn.is_pinned(reg_in) and cn.is_pinned(reg_out)
            for bits in (w, pin_in, reg_in):
                for out in (np.empty(bins + 2, dtype=np.uint64), pin_out, reg_out):
                    call(bits, out)


@gpu
def test_gpu_counts_in_a_captured_graph(oracle):
    """one launch per call; the graph's table after three replays is 3 x the reference (plus the warm-up's, zeroed before)"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    n_len = 5 * TILE + 4133
    w = oracle.n_to_bits_lut(oracle.fill_random_acgt(n_len, seed=21))
    d = torch.from_numpy(w.view(np.int64)).cuda()
    for k in (2, 7, 8, 12):
        for canonical in (False, True):
            table = torch.zeros(4 ** k, dtype=torch.int64, device="cuda")
            fn = lambda: po.kmer_counts_dev(d, n_len, k, canonical=canonical, out=table)  # noqa: E731
            assert _kernel_nodes_of(torch, fn) == 1
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                fn()  # warm-up outside capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            table.zero_()
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            want = reference(oracle, w, n_len, k, canonical)
            assert np.array_equal(table.cpu().numpy().view(np.uint64), want * np.uint64(3)), (k, canonical)


@gpu
@pytest.mark.parametrize("k", [1, LDS_MAX_K])
def test_gpu_all_a_at_2_to_33_carries_past_32_bits(fullsize, k):
    """2^33 nt of A (2 GiB of zero words) in the LDS regime: counts[0] = 2^33-k+1 is past any 32-bit counter, so the run
    folding, the launcher's bound on what a workgroup sees before its flush and the 64-bit flush all hold"""
    import torch

    from conftest import need_free_hbm
    from cute_nucleotides_amd import packed_ops as po

    n_len = 1 << 33
    need_free_hbm(4)
    bits = torch.zeros(n_len // 32, dtype=torch.int64, device="cuda")
    for canonical in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = po.kmer_counts_dev(bits, n_len, k, canonical=canonical)
        torch.cuda.synchronize()
        fullsize(33, (time.perf_counter() - t0) * 1e3, check="kmer counts k=%d %s, all-A" % (k, "canonical" if canonical else "forward"))
        got = got.cpu().numpy().view(np.uint64)
        assert int(got[0]) == n_len - k + 1 and not got[1:].any(), (k, canonical, int(got[0]))


@gpu
@pytest.mark.parametrize("k", [8, 12])
def test_gpu_all_a_in_the_global_regime(k):
    """every add of the global regime on one word: 2^26 nt (its adds are 64-bit from the start, nothing to carry)"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    n_len = 1 << 26
    bits = torch.zeros(n_len // 32, dtype=torch.int64, device="cuda")
    for canonical in (False, True):
        got = po.kmer_counts_dev(bits, n_len, k, canonical=canonical).cpu().numpy().view(np.uint64)
        assert int(got[0]) == n_len - k + 1 and not got[1:].any(), (k, canonical)


@gpu
@pytest.mark.parametrize("k", [4, LDS_MAX_K, LDS_MAX_K + 1, 12])
def test_gpu_counts_full_size(fullsize, k):
    """2^32 nt of device-generated random sequence against torch.bincount over kmers_dev's output (which the k-mer tests
    hold to the oracle), taken in chunks of 2^28 k-mers; forward and canonical"""
    import torch

    import cute_nucleotides_amd as cn
    from conftest import need_free_hbm
    from cute_nucleotides_amd import devutil, packed_ops as po

    n_len, chunk = 1 << 32, 1 << 28
    m, bins = n_len - k + 1, 4 ** k
    need_free_hbm(10)
    n = torch.empty(n_len, dtype=torch.uint8, device="cuda")
    devutil.fill_random_acgt(n, 0x636F756E74 + k)
    bits = cn.n_to_bits_dev(n)
    del n
    buf = torch.empty(chunk, dtype=torch.int64, device="cuda")
    for canonical in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = po.kmer_counts_dev(bits, n_len, k, canonical=canonical)
        torch.cuda.synchronize()
        fullsize(32, (time.perf_counter() - t0) * 1e3, check="kmer counts k=%d %s: kernel" % (k, "canonical" if canonical else "forward"))
        want = torch.zeros(bins, dtype=torch.int64, device="cuda")
        for first in range(0, m, chunk):  # k-mers [first, first + mc) start at word first/32 and need mc + k - 1 nucleotides
            mc = min(chunk, m - first)
            part = po.kmers_dev(bits[first // 32 :], mc + k - 1, k, canonical=canonical, out=buf)
            want += torch.bincount(part, minlength=bins)
        assert int(want.sum()) == m and int(got.sum()) == m
        assert torch.equal(got, want), (k, canonical, int((got != want).sum()))
