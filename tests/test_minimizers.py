"""(w,k)-minimizers on packed words (include/cute_nt.h "k-mers"): in each window of w consecutive k-mers the position with the
smallest (fmix64(k-mer), position), each distinct position once, ascending.  Not in the reference, so the CPU part pins
two references against each other -- the definition as a literal window loop over oracle.kmers, and a vectorised numpy
form (fmix64 on uint64 arrays, sparse-table doubling over (hash, position) pairs, chunks with halos) -- for every k,
window widths from 1 to 256, sizes around m = w and tie-heavy sequences; it pins fmix64 to the project's C definition,
checks the properties the definition implies, every argument error, the ISA of the new kernels and the launch plan.  The
GPU part compares both tiers with the references bit for bit: around tile edges, at input word phases 0..3 with
sentinels around both outputs, without values, with too small a capacity, on equal minimal k-mers across tile edges,
inside a captured graph and behind a side stream, in several launches on the lab build, in a fuzz loop, and once past 2^32
positions against a chunked host checksum."""
import ctypes
import os
import re
import sys
import time

import numpy as np
import pytest

from test_gpu_multi_launch import launch_tiles  # noqa: F401 -- the fixture: the lab build at 64 / 128 tiles per launch
from test_kmers import assert_split_launches_by_max_tiles_per_launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = bytes.maketrans(b"ACGT", b"TGCA")
CNT_KMER_CANONICAL = 0x10
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
WS = [1, 2, 3, 5, 8, 16, 17, 64, 255, 256]
TILE = 2048  # windows per workgroup tile (hip/minimizer_kernels.hpp kMinTile)


# ---- references -----------------------------------------------------------------------------------------------------
def fmix64(x):
    """the splitmix64 finaliser of include/cute_nt.h, on a Python int"""
    z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def np_fmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def n_windows(length, k, w):
    m = length - k + 1 if length >= k else 0
    return m - w + 1 if m >= w else 0


def def_minimizers(oracle, words, length, k, w, canonical=False):
    """the definition, literally: x = oracle.kmers, h = fmix64(x), p(t) = the i in [t, t+w) with the smallest (h_i, i),
    the distinct p(t) in ascending order"""
    x = [int(v) for v in oracle.kmers(words, length, k, canonical)]
    h = [fmix64(v) for v in x]
    out = []
    for t in range(n_windows(length, k, w)):
        p = min(range(t, t + w), key=lambda i: (h[i], i))
        if not out or out[-1] != p:
            out.append(p)
    return np.array(out, dtype=np.uint64), np.array([x[p] for p in out], dtype=np.uint64)


def window_argmin(h, w, ties_right=False):
    """p(t) for every window [t, t+w) of the hash array h: sparse-table doubling over (h, i) pairs up to 2^L <= w, then
    the smaller of the pairs at t and t+w-2^L.  Ties go to the left pair (its position is smaller), or with ties_right to
    the right (the largest position: a window whose two answers differ has a tie at its minimum)."""
    H, I = h, np.arange(h.size, dtype=np.int64)
    better = np.less_equal if ties_right else np.less
    d = 1
    while 2 * d <= w:
        take = better(H[d:], H[:-d])
        H, I = np.where(take, H[d:], H[:-d]), np.where(take, I[d:], I[:-d])
        d *= 2
    nw = h.size - w + 1
    take = better(H[w - d : w - d + nw], H[:nw])
    return np.where(take, I[w - d : w - d + nw], I[:nw])


def np_minimizers(words, length, k, w, canonical=False, x=None, chunk=None):
    """the vectorised reference: (pos, val) as uint64 arrays.  `x` the k-mers when the caller has them; `chunk` windows at a
    time with a halo of w-1 k-mers, the previous chunk's last p(t) deciding whether the next chunk's first is new."""
    from oracle import cnt_oracle as orc

    nw = n_windows(length, k, w)
    if nw == 0:
        return np.empty(0, dtype=np.uint64), np.empty(0, dtype=np.uint64)
    if x is None:
        x = orc.kmers(words, length, k, canonical)
    h = np_fmix64(x)
    chunk = chunk or nw
    parts, last = [], -1
    for t0 in range(0, nw, chunk):
        c = min(chunk, nw - t0)
        p = window_argmin(h[t0 : t0 + c + w - 1], w) + t0
        keep = np.empty(c, dtype=bool)
        keep[0] = p[0] != last
        keep[1:] = p[1:] != p[:-1]
        parts.append(p[keep])
        last = p[-1]
    pos = np.concatenate(parts).astype(np.uint64)
    return pos, x[pos.astype(np.int64)]


def _words(oracle, s):
    return oracle.n_to_bits_lut(np.frombuffer(s, dtype=np.uint8)) if s else np.zeros(1, dtype=np.uint64)


def _tie_heavy(rng, n):
    """poly-A, (AC)*, (ACG)*, and a random sequence with planted repeats of one 40-mer"""
    out = [b"A" * n, (b"AC" * n)[:n], (b"ACG" * n)[:n]]
    s = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes())
    rep = bytes(s[:40])
    for at in rng.integers(0, max(n - 40, 1), max(n // 60, 1)):
        s[at : at + 40] = rep[: n - at]
    out.append(bytes(s[:n]))
    return out


# ---- CPU: the references ----------------------------------------------------------------------------------------------
def test_fmix64_is_the_projects_c_definition(oracle):
    """checksum_words([x - GOLDEN], 0) = fmix64(x - GOLDEN + 1 * GOLDEN): the C fmix64 behind cnt_checksum_words_dev"""
    rng = np.random.default_rng(64)
    xs = [0, 1, 2, M64, GOLDEN, 0x8000000000000000] + [int(v) for v in rng.integers(0, 2**64, 200, dtype=np.uint64)]
    got = np_fmix64(np.array(xs, dtype=np.uint64))
    for x, g in zip(xs, got):
        want = oracle.checksum_words(np.array([(x - GOLDEN) & M64], dtype=np.uint64), 0)
        assert fmix64(x) == want == int(g), hex(x)
    assert fmix64(0) == 0 and len({fmix64(x) for x in range(5000)}) == 5000


@pytest.mark.parametrize("k", [1, 2, 3, 7, 12, 15, 16, 17, 21, 31, 32])
def test_numpy_reference_against_the_definition(oracle, k):
    rng = np.random.default_rng(900 + k)
    for w in WS:
        lens = {k - 1, k, k + w - 3, k + w - 2, k + w - 1, k + w, k + w + 1, k + w + 40, k + 3 * w + 17}
        for n_len in sorted(x for x in lens if x >= 0):
            seqs = [oracle.fill_random_acgt(n_len, seed=n_len * 131 + w).tobytes()]
            if w in (1, 3, 17, 256) and n_len:
                seqs += _tie_heavy(rng, n_len)
            for s in seqs:
                words = _words(oracle, s)
                for canonical in (False, True):
                    want = def_minimizers(oracle, words, n_len, k, w, canonical)
                    got = np_minimizers(words, n_len, k, w, canonical)
                    tag = (k, w, n_len, canonical, s[:8])
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), tag
                    assert got[0].dtype == np.uint64 and got[0].size <= n_windows(n_len, k, w)


@pytest.mark.parametrize("w", WS)
def test_chunked_reference_equals_the_whole(oracle, w):
    """the chunk / halo / carried p(t-1) logic the full-size check uses, at chunk sizes around w, and on poly-A (every
    window's minimum tied) where the chunk boundaries fall inside runs of equal k-mers"""
    for n_len, k, seed in ((20000, 21, 1), (5000, 3, 2)):
        words = oracle.n_to_bits_lut(oracle.fill_random_acgt(n_len, seed))
        for canonical in (False, True):
            whole = np_minimizers(words, n_len, k, w, canonical)
            for chunk in (1, 7, max(w - 1, 1), w, w + 1, 1000):
                got = np_minimizers(words, n_len, k, w, canonical, chunk=chunk)
                assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1]), (w, n_len, k, canonical, chunk)
    a = _words(oracle, b"A" * 3000)
    assert np.array_equal(np_minimizers(a, 3000, 5, w, chunk=77)[0], np.arange(3000 - 5 - w + 2, dtype=np.uint64))


def test_properties(oracle):
    rng = np.random.default_rng(7)
    for n_len, k in ((5000, 1), (5000, 9), (20000, 21), (3000, 32)):
        words = oracle.n_to_bits_lut(oracle.fill_random_acgt(n_len, seed=n_len + k))
        m = n_len - k + 1
        for canonical in (False, True):
            x = oracle.kmers(words, n_len, k, canonical)
            pos, val = np_minimizers(words, n_len, k, 1, canonical)  # w = 1: every k-mer
            assert np.array_equal(pos, np.arange(m, dtype=np.uint64)) and np.array_equal(val, x)
            for w in WS[1:]:
                pos, val = np_minimizers(words, n_len, k, w, canonical)
                d = np.diff(pos.astype(np.int64))
                assert (d > 0).all() and (d <= w).all(), (n_len, k, w)  # strictly increasing, at most w apart
                assert pos[0] < w and pos[-1] >= m - w, (n_len, k, w)  # the first and the last window are covered
                assert np.array_equal(val, x[pos.astype(np.int64)])
    # canonical strand symmetry on inputs with no tie in any window: positions of revcomp(s) are m-1-p
    for n_len, k, w in ((30000, 21, 11), (30000, 31, 19), (10000, 15, 64)):
        s = oracle.fill_random_acgt(n_len, seed=w).tobytes()
        words, rwords = _words(oracle, s), _words(oracle, s.translate(COMP)[::-1])
        m = n_len - k + 1
        h = np_fmix64(oracle.kmers(words, n_len, k, True))
        assert np.array_equal(window_argmin(h, w), window_argmin(h, w, ties_right=True))  # no tie at any window minimum
        a = np_minimizers(words, n_len, k, w, True)[0].astype(np.int64)
        b = np_minimizers(rwords, n_len, k, w, True)[0].astype(np.int64)
        assert np.array_equal(b, (m - 1 - a)[::-1]), (k, w)
    # ties: the leftmost equal k-mer wins -- in (AC)* the two forward 2-mers alternate, so every other position is picked
    s = b"AC" * 500
    pos, val = np_minimizers(_words(oracle, s), 1000, 2, 5)
    assert len(set(val.tolist())) == 1 and (np.diff(pos.astype(np.int64)) == 2).all()


@pytest.mark.parametrize("w", [1, 5, 10, 11, 19, 64, 256])
def test_density_of_random_sequences(oracle, w):
    """about 2/(w+1) of the windows of a random sequence select a new position (k >= 12: ties are rare)"""
    n_len = 1 << 22
    words = oracle.n_to_bits_lut(oracle.fill_random_acgt(n_len, seed=0x44 + w))
    for k, canonical in ((12, False), (21, True), (31, False)):
        pos, _ = np_minimizers(words, n_len, k, w, canonical)
        density = pos.size / n_windows(n_len, k, w)
        assert abs(density / (2 / (w + 1)) - 1) < 0.05, (w, k, canonical, density)


# ---- CPU: the ABI ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


def _work_bytes(L, n_len, k, w):
    out = ctypes.c_size_t(12345)
    assert L.cnt_minimizers_work_bytes(n_len, k, w, ctypes.byref(out)) == 0
    return out.value


def test_work_bytes_query(L):
    from cute_nucleotides_amd import _lib
    from cute_nucleotides_amd import packed_ops as po

    assert _work_bytes(L, 0, 1, 1) == 0 and _work_bytes(L, 30, 21, 11) == 0  # m = 10 < w
    assert _work_bytes(L, 31, 21, 11) == 16 + 2 * 8 + 16 * 4  # one window: one group of 16 tiles
    for W in (1, TILE - 1, TILE, TILE + 1, 5 * TILE, 16 * TILE, 16 * TILE + 1, 33 * 16 * TILE, (1 << 32) + 1):
        n_len = W + 11 - 1 + 21 - 1
        groups = -(-(-(-W // TILE)) // 16)
        want = 16 + (groups + groups % 2) * 8 + groups * 16 * 4  # alignment slack, one u64 offset per group, one u32 count per tile
        assert _work_bytes(L, n_len, 21, 11) == want == po.minimizers_work_bytes(n_len, 21, 11), W
    for k, w in ((0, 5), (33, 5), (5, 0), (5, 257)):
        assert L.cnt_minimizers_work_bytes(100, k, w, ctypes.byref(ctypes.c_size_t())) == _lib.CNT_EINVAL
    assert L.cnt_minimizers_work_bytes(100, 5, 5, None) == _lib.CNT_EINVAL


def test_abi_errors_come_before_any_device_work(L):
    from cute_nucleotides_amd import _lib

    buf = np.zeros(4096, dtype=np.uint64)
    base = buf.ctypes.data
    q = lambda word, byte=0: ctypes.c_void_p(base + 8 * word + byte)  # noqa: E731
    out = np.full(256, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    o = lambda word, byte=0: ctypes.c_void_p(out.ctypes.data + 8 * word + byte)  # noqa: E731
    cnt = np.full(2, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    c = lambda byte=0: ctypes.c_void_p(cnt.ctypes.data + byte)  # noqa: E731
    work = q(3000)  # 100 nt, k = 21, w = 11: m = 80, W = 70, 96 B of scratch
    for dev in (False, True):
        def call(bits, n_len, k, w, flags, pos, val, cap, count, work_bytes=96):
            if dev:
                return L.cnt_minimizers_dev(bits, n_len, k, w, flags, pos, val, cap, count, work, work_bytes, None)
            return L.cnt_minimizers(bits, n_len, k, w, flags, pos, val, cap, count)

        tag = "dev" if dev else "host"
        # k, w, flags out of range -- even when there would be no window
        for k, w in ((0, 5), (33, 5), (64, 5), (21, 0), (21, 257), (21, 1 << 20)):
            assert call(q(0), 100, k, w, 0, o(0), o(100), 64, c()) == _lib.CNT_EINVAL, (tag, k, w)
            assert call(None, 0, k, w, 0, None, None, 0, None) == _lib.CNT_EINVAL, (tag, k, w)
        for flags in (0x1, 0x2, 0x4, 0x8, 0x20, 0x80000000, CNT_KMER_CANONICAL | 0x1):
            assert call(q(0), 100, 21, 11, flags, o(0), o(100), 64, c()) == _lib.CNT_EINVAL, (tag, flags)
        # NULL bits, pos or count when W > 0 (val may be NULL)
        assert call(None, 100, 21, 11, 0, o(0), o(100), 64, c()) == _lib.CNT_EINVAL
        assert call(q(0), 100, 21, 11, 0, None, o(100), 64, c()) == _lib.CNT_EINVAL
        assert call(q(0), 100, 21, 11, 0, o(0), o(100), 64, None) == _lib.CNT_EINVAL
        # not 8-B aligned
        for byte in (1, 4, 7):
            assert call(q(0, byte), 100, 21, 11, 0, o(0), o(100), 64, c()) == _lib.CNT_EINVAL
            assert call(q(0), 100, 21, 11, 0, o(0, byte), o(100), 64, c()) == _lib.CNT_EINVAL
            assert call(q(0), 100, 21, 11, 0, o(0), o(100, byte), 64, c()) == _lib.CNT_EINVAL
            assert call(q(0), 100, 21, 11, 0, o(0), o(100), 64, c(byte)) == _lib.CNT_EINVAL
        # pos or val overlapping the input words (100 nt = 4 words at q(10)) or each other (64 entries each)
        for ow in (10, 12, 13, 8, 0):
            assert call(q(10), 100, 21, 11, 0, q(ow), o(100), 64, c()) == _lib.CNT_EINVAL, (tag, ow)
            assert call(q(10), 100, 21, 11, 0, o(100), q(ow), 64, c()) == _lib.CNT_EINVAL, (tag, ow)
        for vw in (0, 63, 30):
            assert call(q(10), 100, 21, 11, 0, o(0), o(vw), 64, c()) == _lib.CNT_EINVAL, (tag, vw)
        # ... only the min(W, out_cap) entries that can be written count: adjacent ranges are fine
        if dev:
            assert call(q(10), 100, 21, 11, 0, o(0), o(100), 64, c(), work_bytes=95) == _lib.CNT_EINVAL  # scratch below the query
            assert call(q(10), 100, 21, 11, 0, o(0), o(100), 64, c(), work_bytes=0) == _lib.CNT_EINVAL
        # W == 0: CNT_OK without a device, count set to 0 on the host tier (NULL pointers allowed)
        for n_len, k, w in ((0, 1, 1), (20, 21, 1), (30, 21, 11), (31, 32, 1)):
            assert call(None, n_len, k, w, CNT_KMER_CANONICAL, None, None, 0, None) == _lib.CNT_OK
            if not dev:
                cnt[0] = 99
                assert call(q(0), n_len, k, w, 0, o(0), None, 64, c()) == _lib.CNT_OK and cnt[0] == 0
                cnt[0] = 0x5A5A5A5A5A5A5A5A
    assert (out == 0x5A5A5A5A5A5A5A5A).all()  # nothing was written
    count = ctypes.c_int(-1)
    assert L.cnt_device_count(ctypes.byref(count)) == _lib.CNT_OK
    if count.value == 0:
        # past the argument checks a call needs a device (on a GPU box these would run on host pointers: only tried without one)
        assert L.cnt_minimizers(q(0), 100, 21, 11, 0, o(0), o(100), 64, c()) == _lib.CNT_ENODEV
        assert L.cnt_minimizers_dev(q(0), 100, 21, 11, 0, o(0), None, 64, c(), work, 96, None) < 0
        assert (out == 0x5A5A5A5A5A5A5A5A).all()


def test_python_wrappers_raise_value_error(L):
    from cute_nucleotides_amd import packed_ops as po

    w = np.zeros(2, dtype=np.uint64)
    for k, win in ((0, 5), (33, 5), (5, 0), (5, 257)):
        with pytest.raises(ValueError):
            po.minimizers_hip(w, 64, k, win)
    with pytest.raises(ValueError):
        po.minimizers_hip(w, 65, 21, 3)  # longer than the words hold
    pos, val = po.minimizers_hip(w, 30, 21, 11)
    assert pos.size == 0 and val.size == 0
    pos, val = po.minimizers_hip(w, 0, 1, 1, canonical=True, values=False)
    assert pos.size == 0 and val is None


def test_abi_wiring(L):
    import subprocess

    from cute_nucleotides_amd import _lib

    names = ("cnt_minimizers", "cnt_minimizers_dev", "cnt_minimizers_work_bytes")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "cute_nt.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(L, name) and name in exported and name + "(" in header
    for words in ("SET to n", "add to a caller-zeroed counter", "CNT_ECAP comes after the work", "not minimap2"):
        assert words.lower() in header.lower(), words
    rust = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    for sig in (r"pub fn minimizers_hip\(bits: &\[u64\], len: usize, k: u32, w: u32, canonical: bool\) -> \(Vec<u64>, Vec<u64>\) \{",
                r"pub fn minimizers_hip_dev\(", r"pub fn minimizers_work_bytes\(len: usize, k: u32, w: u32\) -> usize \{"):
        assert re.search(sig, rust), sig


# ---- CPU: the ISA and the launch plan ------------------------------------------------------------------------------------
MIN_KERNELS = ["void cnt::minimizer_tiles<false>", "void cnt::minimizer_tiles<true>"]


@pytest.fixture(scope="module")
def product_asm():
    sys.path.insert(0, os.path.join(ROOT, "bench"))
    import isa_digest

    return isa_digest, isa_digest.assembly()


def test_minimizer_kernels_isa(product_asm):
    """no scratch, no waterfall loop, LDS within one tile's (hash, index) arrays, VGPRs bounded; the scan (not a template,
    so outside isa_digest's list) read from the same assembly; the product stays below 60 templated kernels"""
    isa_digest, asm = product_asm
    found = isa_digest.kernels(asm)
    for name in MIN_KERNELS:
        assert name in found, name
        e = found[name]
        assert not [i for i in e["body"] if "scratch_" in i], name
        assert not [i for i in e["body"] if "s_xor_b64 exec, exec" in i], name
        meta = e["meta"]
        assert meta["private_segment_fixed_size"] == 0 and meta["next_free_vgpr"] <= 96, (name, meta)
        assert meta["group_segment_fixed_size"] <= 24 * 1024, (name, meta)  # (2048 + 256) x 10 B + the group counts
    stores = [i for i in found["void cnt::minimizer_tiles<true>"]["body"] if "_store" in i and not i.startswith("ds_")]
    assert stores and all(i.startswith("global_store_dwordx2") and " nt" in i for i in stores), stores
    assert not [i for i in found["void cnt::minimizer_tiles<false>"]["body"] if i.startswith(("global_store_dwordx2", "buffer_store")) and " nt" in i]
    m = re.search(r"^cnt::counted_scan\(.*?\): +; @(.*?)\.end_amdhsa_kernel", asm, re.S | re.M)
    assert m, "counted_scan not in the product's assembly"
    scan = m.group(1)
    assert "scratch_" not in scan and "s_xor_b64 exec, exec" not in scan
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", scan)
    assert len(found) < 60, len(found)


MIN_HW_LAUNCH_TILES = ((0x7FFFFFFF // 256) // 64) * 64  # max_tiles_per_launch(256) of the product build


def minimizer_plan(n_len, k, w, launch_tiles=MIN_HW_LAUNCH_TILES):
    """(tiles, kernel launches) of a device call: ceil(W / 2048) tiles, counted and written in ceil(tiles / launch_tiles)
    launches each, one scan launch between them; W = 0: no kernel (a memset of the count)"""
    nw = n_windows(n_len, k, w)
    tiles = -(-nw // TILE)
    return tiles, (2 * -(-tiles // launch_tiles) + 1) if tiles else 0


def assert_counted_output_source():
    """what the three launchers reach through hip/counted_output.hpp: the one scan launch and the early exit for an empty input"""
    src = open(os.path.join(ROOT, "hip", "counted_output.hpp")).read()
    for line in ("hipLaunchKernelGGL(counted_scan, dim3(1), dim3(kCountedScanBlock), 0, s, w.counts, w.offs, n_tiles, static_cast<uint64_t*>(d_count));",
                 "inline int counted_empty_dev(void* d_count, hipStream_t s) { return d_count ? hip_rc(hipMemsetAsync(d_count, 0, 8, s)) : CNT_OK; }"):
        assert line in src, line
    assert src.count("hipLaunchKernelGGL(") == 1


def test_minimizer_plan_matches_the_launcher_and_splitter_source():
    src = open(os.path.join(ROOT, "hip", "minimizer_kernels.hpp")).read()
    assert "constexpr int kMinBlock = 256;" in src and "constexpr uint32_t kMinTile = 2048, kMinMaxW = 256;" in src
    abi = open(os.path.join(ROOT, "hip", "minimizer_abi.inc")).read()
    scan = "counted_scan_enqueue(work, n_tiles, d_count, s);"
    for line in ("const uint64_t n_tiles = (n_win + kMinTile - 1) / kMinTile;", "const CountedScratch work = counted_carve(d_work, n_tiles);", scan,
                 "if (n_win == 0) return counted_empty_dev(d_count, s);"):
        assert line in abi, line
    assert_counted_output_source()
    # the two tile passes, each in launches of max_tiles_per_launch(kMinBlock) tiles, with the one scan launch between them
    tiles = "split_launches(n_tiles, kMinBlock, [&](uint64_t t, uint64_t n) {"
    assert abi.count(tiles) == 2 and abi.count("counted_scan") == 1
    assert abi.index(tiles) < abi.index(scan) < abi.rindex(tiles)
    assert_split_launches_by_max_tiles_per_launch()
    assert MIN_HW_LAUNCH_TILES == 8388544
    assert minimizer_plan((1 << 32) + 33, 21, 11) == (2097153, 3)
    assert minimizer_plan(64 * TILE * 3 + 30, 21, 11, 64) == (192, 7) and minimizer_plan(64 * TILE * 3 + 31, 21, 11, 64) == (193, 9)


# ---------------------------------------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu
SENTINEL = -0x3C3C3C3C3C3C3C3D


def _random_words(rng, n_len, extra=0):
    return rng.integers(0, 2**64, (n_len + 31) // 32 + extra, dtype=np.uint64)  # garbage above len in the last word included


def _host_call(L, bits, n_len, k, w, canonical, pos, val, cap):
    n = ctypes.c_uint64(0xDEAD)
    rc = L.cnt_minimizers(bits.ctypes.data, n_len, k, w, CNT_KMER_CANONICAL if canonical else 0, pos.ctypes.data,
                          val.ctypes.data if val is not None else None, cap, ctypes.byref(n))
    return rc, n.value


def _dev_result(pos, val, count):
    n = int(count.item())
    return n, pos[:n].cpu().numpy().view(np.uint64), (val[:n].cpu().numpy().view(np.uint64) if val is not None else None)


def _edge_lengths(k, w):
    """W = 0 (m < w), 1 (m == w), less than a tile, T-1, T, T+1, 2T+-1, 3T + 77"""
    T = TILE
    return [k + w - 3, k + w - 2, k + w + 400] + [W + w + k - 2 for W in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 3 * T + 77)]


@gpu
@pytest.mark.parametrize("k", [1, 15, 21, 32])
def test_gpu_minimizers_match_reference(oracle, k):
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(k)
    for w in WS:
        for n_len in _edge_lengths(k, w):
            if n_len < 0:
                continue
            words = _random_words(rng, n_len)
            d = torch.from_numpy(words.view(np.int64)).cuda()
            for canonical in (False, True):
                want = np_minimizers(words, n_len, k, w, canonical)
                tag = (k, w, n_len, canonical)
                pos, val = po.minimizers_hip(words, n_len, k, w, canonical=canonical)
                assert np.array_equal(pos, want[0]) and np.array_equal(val, want[1]), tag + ("host",)
                n, gp, gv = _dev_result(*po.minimizers_dev(d, n_len, k, w, canonical=canonical))
                assert n == want[0].size and np.array_equal(gp, want[0]) and np.array_equal(gv, want[1]), tag + ("device",)


@gpu
def test_gpu_minimizers_phases_sentinels_no_values_and_capacity(oracle, L):
    """input views at word phases 0..3 with garbage above len; pos / val views at 8-B phases with sentinels on both sides
    that survive past n and past out_cap; val = NULL; out_cap < n writes the prefix, sets the count to n, writes nothing
    past the cap, and the host tier answers CNT_ECAP after writing the prefix"""
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(3)
    top = 3 * TILE // 32 * 4 + 64
    words_all = rng.integers(0, 2**64, top, dtype=np.uint64)
    d_all = torch.from_numpy(words_all.view(np.int64)).cuda()
    pbuf = torch.empty(5 * TILE, dtype=torch.int64, device="cuda")
    vbuf = torch.empty(5 * TILE, dtype=torch.int64, device="cuda")
    cbuf = torch.empty(4, dtype=torch.int64, device="cuda")
    for k, w, n_len in ((21, 11, 3 * TILE + 5), (5, 3, TILE + 100), (32, 256, 2 * TILE + 300), (1, 1, TILE + 7), (16, 17, 5000)):
        nw = (n_len + 31) // 32
        for pi in range(4):
            src = words_all[pi : pi + nw]
            for canonical in (False, True):
                want_p, want_v = np_minimizers(src, n_len, k, w, canonical)
                n = want_p.size
                for ph, cap in ((0, n), (3, n + 9), (5, n - 1), (1, n // 3), (2, 1), (7, 0)):
                    for values in (True, False):
                        tag = (k, w, n_len, pi, canonical, ph, cap, values)
                        pbuf.fill_(SENTINEL)
                        vbuf.fill_(SENTINEL)
                        cbuf.fill_(SENTINEL)
                        pos, val, count = po.minimizers_dev(d_all[pi : pi + nw], n_len, k, w, canonical=canonical, values=values,
                                                            pos=pbuf[8 + ph : 8 + ph + cap], val=vbuf[8 + ph : 8 + ph + cap] if values else None,
                                                            count=cbuf[1:2])
                        torch.cuda.synchronize()
                        c = cbuf.cpu().numpy()
                        assert c[1] == n and c[0] == SENTINEL and (c[2:] == SENTINEL).all(), tag
                        got = min(n, cap)
                        p = pbuf.cpu().numpy()
                        assert (p[: 8 + ph] == SENTINEL).all() and (p[8 + ph + got :] == SENTINEL).all(), tag
                        assert np.array_equal(p[8 + ph : 8 + ph + got].view(np.uint64), want_p[:got]), tag
                        v = vbuf.cpu().numpy()
                        if values:
                            assert (v[: 8 + ph] == SENTINEL).all() and (v[8 + ph + got :] == SENTINEL).all(), tag
                            assert np.array_equal(v[8 + ph : 8 + ph + got].view(np.uint64), want_v[:got]), tag
                        else:
                            assert (v == SENTINEL).all(), tag
                # host tier: staged, then pinned in and out (in place), the same capacities
                for pinned in (False, True):
                    bits = cn.pinned_empty(nw, np.uint64) if pinned else src.copy()
                    bits[:] = src
                    hp = cn.pinned_empty(n + 16, np.uint64) if pinned else np.empty(n + 16, dtype=np.uint64)
                    hv = cn.pinned_empty(n + 16, np.uint64) if pinned else np.empty(n + 16, dtype=np.uint64)
                    for cap in (n, n + 9, n - 1, n // 3, 0):
                        for values in (True, False):
                            hp[:] = 0xDEADBEEFDEADBEEF
                            hv[:] = 0xDEADBEEFDEADBEEF
                            rc, got_n = _host_call(L, bits, n_len, k, w, canonical, hp, hv if values else None, cap)
                            tag = (k, w, n_len, pi, canonical, cap, values, pinned)
                            assert rc == (_lib.CNT_ECAP if n > cap else _lib.CNT_OK) and got_n == n, (tag, rc, got_n)
                            got = min(n, cap)
                            assert np.array_equal(hp[:got], want_p[:got]) and (hp[got:] == 0xDEADBEEFDEADBEEF).all(), tag
                            if values:
                                assert np.array_equal(hv[:got], want_v[:got]) and (hv[got:] == 0xDEADBEEFDEADBEEF).all(), tag
                            else:
                                assert (hv == 0xDEADBEEFDEADBEEF).all(), tag
    # W == 0 sets the device count to 0
    cbuf.fill_(SENTINEL)
    _, _, count = po.minimizers_dev(d_all, 30, 21, 11, count=cbuf[1:2])
    assert int(count.item()) == 0 and cbuf.cpu().numpy()[0] == SENTINEL


@gpu
@pytest.mark.parametrize("canonical", [False, True])
def test_gpu_equal_minimal_kmers_across_tile_edges(oracle, canonical):
    """poly-A across tile edges at every w of the list: every window's minimum is tied, the leftmost wins, so every position
    0..W-1 is selected (one per window, the tile's first window new against its left neighbour); then a run of equal
    minimal k-mers planted across one tile edge inside a random sequence"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    k = 11
    for w in WS:
        for n_len in (2 * TILE + w + k - 2, TILE + w + k - 1, 3 * TILE + w + 40):
            s = b"A" * n_len
            words = _words(oracle, s)
            d = torch.from_numpy(words.view(np.int64)).cuda()
            W = n_windows(n_len, k, w)
            n, gp, gv = _dev_result(*po.minimizers_dev(d, n_len, k, w, canonical=canonical))
            assert n == W and np.array_equal(gp, np.arange(W, dtype=np.uint64)) and not gv.any(), (w, n_len)
            hp, hv = po.minimizers_hip(words, n_len, k, w, canonical=canonical)
            assert np.array_equal(hp, gp) and np.array_equal(hv, gv), (w, n_len)
    rng = np.random.default_rng(12)
    for w in (5, 17, 64, 256):
        n_len = 3 * TILE + 2 * w + k
        s = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n_len)].tobytes())
        lo = TILE - w // 2
        s[lo : lo + w + k] = b"A" * (w + k)  # w+1 equal k-mers from TILE - w/2 on: whenever one is minimal, the leftmost in the window wins
        words = _words(oracle, bytes(s))
        d = torch.from_numpy(words.view(np.int64)).cuda()
        want = np_minimizers(words, n_len, k, w, canonical)
        n, gp, gv = _dev_result(*po.minimizers_dev(d, n_len, k, w, canonical=canonical))
        assert n == want[0].size and np.array_equal(gp, want[0]) and np.array_equal(gv, want[1]), w


@gpu
def test_gpu_minimizers_in_a_captured_graph_and_behind_a_side_stream(oracle):
    """encode -> forward minimizers -> canonical minimizers of the reverse complement, captured with torch.cuda.graph with
    the same work buffers and replayed on 3 new inputs (kernel nodes counted from the plan); then fill -> encode ->
    minimizers enqueued on a side stream with no host sync in between"""
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import devutil, packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    n_len, k, w = (1 << 20) + 4133, 21, 11
    words = (n_len + 31) // 32
    W = n_windows(n_len, k, w)
    d_n = torch.zeros(n_len, dtype=torch.uint8, device="cuda")
    bits = torch.empty(words, dtype=torch.int64, device="cuda")
    rc = torch.empty(words, dtype=torch.int64, device="cuda")
    need = po.minimizers_work_bytes(n_len, k, w)
    work = [torch.empty(need + 8, dtype=torch.uint8, device="cuda") for _ in range(2)]
    outs = [(torch.empty(W, dtype=torch.int64, device="cuda"), torch.empty(W, dtype=torch.int64, device="cuda"),
             torch.empty(1, dtype=torch.int64, device="cuda")) for _ in range(2)]

    def chain():
        cn.n_to_bits_dev(d_n, out=bits)
        po.minimizers_dev(bits, n_len, k, w, pos=outs[0][0], val=outs[0][1], count=outs[0][2], work=work[0][3:])  # scratch at an odd byte
        po.reverse_complement_dev(bits, n_len, out=rc)
        po.minimizers_dev(rc, n_len, k, w, canonical=True, pos=outs[1][0], val=outs[1][1], count=outs[1][2], work=work[1])

    tiles, launches = minimizer_plan(n_len, k, w)
    assert _kernel_nodes_of(torch, lambda: po.minimizers_dev(bits, n_len, k, w, pos=outs[0][0], val=outs[0][1], count=outs[0][2], work=work[0])) == launches == 3
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rng = np.random.default_rng(31)
    for rep in range(3):
        host = acgt[rng.integers(0, 4, n_len)]
        d_n.copy_(torch.from_numpy(host))
        for o in outs:
            for t in o:
                t.fill_(SENTINEL)
        for t in work:
            t.fill_(0x77)  # the scratch needs no zeroing
        g.replay()
        torch.cuda.synchronize()
        hb = oracle.n_to_bits_lut(host)
        for j, (b, canonical) in enumerate(((hb, False), (oracle.reverse_complement(hb, n_len), True))):
            want = np_minimizers(b, n_len, k, w, canonical)
            n, gp, gv = _dev_result(*outs[j])
            assert n == want[0].size and np.array_equal(gp, want[0]) and np.array_equal(gv, want[1]), (rep, j)
            assert (outs[j][0][n:].cpu().numpy() == SENTINEL).all(), (rep, j)
    # a producer and its consumer on a side stream, enqueued back to back
    seed, n2 = 77, (1 << 22) + 19
    want = np_minimizers(oracle.n_to_bits_lut(oracle.fill_random_acgt(n2, seed)), n2, 21, 11, True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        n = torch.zeros(n2, dtype=torch.uint8, device="cuda")
        devutil.fill_random_acgt(n, seed)
        pos, val, count = po.minimizers_dev(cn.n_to_bits_dev(n), n2, 21, 11, canonical=True)
    torch.cuda.current_stream().wait_stream(side)
    got = _dev_result(pos, val, count)
    assert got[0] == want[0].size and np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1])


@gpu
def test_gpu_minimizers_in_several_launches(oracle, launch_tiles):
    """the lab build cut into launches of 64 / 128 tiles: both passes of a call in several launches, counted in a captured
    graph, against the reference, with the host tier on the same input"""
    import torch

    from cute_nucleotides_amd import packed_ops as po
    from test_gpu_codec2 import _kernel_nodes_of

    rng = np.random.default_rng(launch_tiles)
    for n_len, k, w, canonical in ((launch_tiles * TILE * 3 + 30, 21, 11, False), (launch_tiles * TILE + 5000, 31, 19, True),
                                   (launch_tiles * TILE * 2 + 255 + 14, 15, 256, True)):
        words = _random_words(rng, n_len)
        d = torch.from_numpy(words.view(np.int64)).cuda()
        want = np_minimizers(words, n_len, k, w, canonical)
        res = po.minimizers_dev(d, n_len, k, w, canonical=canonical)
        n, gp, gv = _dev_result(*res)
        assert n == want[0].size and np.array_equal(gp, want[0]) and np.array_equal(gv, want[1]), (n_len, k, w)
        tiles, launches = minimizer_plan(n_len, k, w, launch_tiles)
        assert launches >= 5
        assert _kernel_nodes_of(torch, lambda: po.minimizers_dev(d, n_len, k, w, canonical=canonical, pos=res[0], val=res[1], count=res[2])) == launches
        hp, hv = po.minimizers_hip(words, n_len, k, w, canonical=canonical)
        assert np.array_equal(hp, want[0]) and np.array_equal(hv, want[1])


@gpu
@pytest.mark.parametrize("seed", range(4))
def test_gpu_minimizers_fuzz(oracle, L, seed):
    """random lengths, k, w, modes, input phases, capacities and values on / off, tie-heavy inputs among them; both tiers"""
    import torch

    from cute_nucleotides_amd import _lib, packed_ops as po

    rng = np.random.default_rng(2100 + seed)
    for it in range(40):
        k, w = int(rng.integers(1, 33)), int(rng.choice([1, 2, 3, 4, 7, 10, 11, 19, 32, 100, 255, 256, int(rng.integers(1, 257))]))
        n_len = int(rng.choice([rng.integers(0, 300), rng.integers(0, 5 * TILE), rng.integers(0, 40 * TILE)]))
        canonical, values, pi = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), int(rng.integers(0, 4))
        nw = max((n_len + 31) // 32, 1)
        if it % 5 == 4 and n_len:
            src = _words(oracle, _tie_heavy(rng, n_len)[int(rng.integers(0, 4))])
            allw = np.concatenate([rng.integers(0, 2**64, pi, dtype=np.uint64), src, rng.integers(0, 2**64, 4, dtype=np.uint64)])
        else:
            allw = rng.integers(0, 2**64, nw + 4 + pi, dtype=np.uint64)
        src = allw[pi : pi + nw]
        want = np_minimizers(src, n_len, k, w, canonical)
        n = want[0].size
        cap = int(rng.choice([n, n + 3, max(n - 1, 0), int(rng.integers(0, n + 1))]))
        tag = (seed, it, n_len, k, w, canonical, values, pi, cap)
        d = torch.from_numpy(allw.view(np.int64)).cuda()
        pbuf = torch.full((cap + 8,), SENTINEL, dtype=torch.int64, device="cuda")
        vbuf = torch.full((cap + 8,), SENTINEL, dtype=torch.int64, device="cuda")
        pos, val, count = po.minimizers_dev(d[pi : pi + nw], n_len, k, w, canonical=canonical, values=values, pos=pbuf[3 : 3 + cap],
                                            val=vbuf[3 : 3 + cap] if values else None)
        got = min(n, cap)
        assert int(count.item()) == n, tag
        p, v = pbuf.cpu().numpy(), vbuf.cpu().numpy()
        assert np.array_equal(p[3 : 3 + got].view(np.uint64), want[0][:got]) and (p[:3] == SENTINEL).all() and (p[3 + got :] == SENTINEL).all(), tag
        if values:
            assert np.array_equal(v[3 : 3 + got].view(np.uint64), want[1][:got]) and (v[3 + got :] == SENTINEL).all(), tag
        else:
            assert (v == SENTINEL).all(), tag
        hp = np.full(cap + 2, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        hv = np.full(cap + 2, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        rc, hn = _host_call(L, np.ascontiguousarray(src), n_len, k, w, canonical, hp, hv if values else None, cap)
        W = n_windows(n_len, k, w)
        assert rc == (_lib.CNT_ECAP if n > cap else _lib.CNT_OK) and hn == n, tag
        assert np.array_equal(hp[:got], want[0][:got]) and (hp[got:] == 0xDEADBEEFDEADBEEF).all(), tag
        if values:
            assert np.array_equal(hv[:got], want[1][:got]), tag
        if values and W:
            hp2, hv2 = po.minimizers_hip(src, n_len, k, w, canonical=canonical)  # the guess-and-retry wrapper
            assert np.array_equal(hp2, want[0]) and np.array_equal(hv2, want[1]), tag


def _host_stream_reference(oracle, seed, n_len, k, w, canonical, chunk=1 << 22, workers=12):
    """chunked host reference over oracle.fill_random_acgt: chunk c holds windows [c*chunk, (c+1)*chunk) and needs the
    k-mers up to (c+1)*chunk + w - 1; a chunk's first window is new unless its p equals the previous chunk's last.  The
    output's checksums (oracle.checksum_words at the global output index) are summed in order; per chunk it keeps
    (first output index, entries, pos checksum, val checksum) to name a bad chunk.  Returns (n, pos sum, val sum, chunks)."""
    from concurrent.futures import ThreadPoolExecutor

    nw = n_windows(n_len, k, w)

    def one(t0):
        c = min(chunk, nw - t0)
        nt = c + w - 1 + k - 1
        s = oracle.fill_random_acgt(nt, seed, first_nt=t0)
        x = oracle.kmers(oracle.n_to_bits_lut(s), nt, k, canonical)
        p = window_argmin(np_fmix64(x), w)
        keep = np.empty(c, dtype=bool)
        keep[0] = True
        keep[1:] = p[1:] != p[:-1]
        sel = p[keep]
        return int(p[0]) + t0, int(p[-1]) + t0, (sel + t0).astype(np.uint64), x[sel]

    n, ps, vs, chunks, last = 0, 0, 0, [], -1
    starts = list(range(0, nw, chunk))
    with ThreadPoolExecutor(workers) as pool:
        for b in range(0, len(starts), workers):
            for first_p, last_p, pos, val in pool.map(one, starts[b : b + workers]):
                if first_p == last:
                    pos, val = pos[1:], val[1:]
                cp, cv = oracle.checksum_words(pos, first_word=n), oracle.checksum_words(val, first_word=n)
                chunks.append((n, pos.size, cp, cv))
                ps, vs, n, last = ps + cp, vs + cv, n + pos.size, last_p
    return n, ps & M64, vs & M64, chunks, chunk


@gpu
def test_gpu_minimizers_full_size_past_2p32(oracle, fullsize):
    """2^32 + 33 nt, k = 21, w = 11, canonical, device tier on cnt_fill_random_acgt_dev input: n and the checksums of pos
    and val against the chunked host reference (the first bad chunk named on a mismatch); positions pass 2^32; one
    changed entry is seen"""
    import torch

    import stream_checks
    from conftest import need_free_hbm
    from cute_nucleotides_amd import devutil, packed_ops as po
    from test_kmers import _device_sequence

    n_len, k, w, seed = (1 << 32) + 33, 21, 11, 0x6D696E69
    W = n_windows(n_len, k, w)
    cap = 2 * W // (w + 1) + W // 50
    need_free_hbm((n_len + (n_len >> 2)) // (1 << 30) + 2)
    bits = _device_sequence(n_len, seed)
    need_free_hbm((2 * cap * 8) // (1 << 30) + 2)
    pos = torch.empty(cap, dtype=torch.int64, device="cuda")
    val = torch.empty(cap, dtype=torch.int64, device="cuda")
    work = torch.empty(po.minimizers_work_bytes(n_len, k, w), dtype=torch.uint8, device="cuda")
    po.minimizers_dev(bits, n_len, k, w, canonical=True, pos=pos, val=val, work=work)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, count = po.minimizers_dev(bits, n_len, k, w, canonical=True, pos=pos, val=val, work=work)
    torch.cuda.synchronize()
    fullsize(32, (time.perf_counter() - t0) * 1e3, check="minimizers k=21 w=11 canonical: kernels")
    n = int(count.item())
    t1 = time.perf_counter()
    want_n, want_p, want_v, chunks, chunk = _host_stream_reference(oracle, seed, n_len, k, w, True)
    fullsize(32, (time.perf_counter() - t1) * 1e3, check="minimizers: chunked host reference")
    assert n == want_n, (n, want_n)
    assert n <= cap and int(pos[n - 1].item()) >= 1 << 32
    gp, gv = devutil.checksum_words(pos[:n]), devutil.checksum_words(val[:n])
    if (gp, gv) != (want_p, want_v):
        bad = "no chunk differs on its own"
        for c, (j0, cnt, cp, cv) in enumerate(chunks):
            if devutil.checksum_words(pos[j0 : j0 + cnt], first_word=j0) != cp or devutil.checksum_words(val[j0 : j0 + cnt], first_word=j0) != cv:
                bad = "first differing chunk %d of %d: output entries [%d, %d), windows [%d, %d)" % (c, len(chunks), j0, j0 + cnt, c * chunk, (c + 1) * chunk)
                break
        pytest.fail("minimizers past 2^32: checksums pos %#x val %#x != reference %#x %#x; %s" % (gp, gv, want_p, want_v, bad))
    for i in (n - 3, (n * 5) // 7):
        stream_checks.assert_mutation_seen(pos[:n], i, want_p)
    stream_checks.assert_mutation_seen(val[:n], n // 3, want_v)
