"""The caller's scratch of the three scan-based device calls (cnt_minimizers_dev, cnt_find_pattern_dev, cnt_orfs_dev), and the
edges of the two scans behind them.

The queries cnt_*_work_bytes promise that a call touches nothing outside the bytes it is handed, whatever they hold and wherever
they start.  The CPU part restates the launchers' carving of those bytes as a model (scratch_layout, written_extent), holds it to
the three queries, and tests the guard checker on synthetic buffers.  The GPU part hands every call EXACTLY the queried bytes, at
byte phases 0, 1, 7, 8 and 15 of a 16-B-aligned buffer, between two 256-B guards of 0xA5, once zeroed and once filled with 0xFF:
the results equal the references both times, no byte outside the model's body changes, and the bytes that do change begin at the
aligned base and end at the model's written extent -- the guards sit on the edges.  The last part puts stops, starts and hits at
the edges of orf_carry (64 tiles to a wave, 1024 to a round) and of counted_scan (64 groups of 16 tiles to a wave) in one
sequence of 1027 tiles.  Every comparison is exact; every reference is one of the suite's own."""
import ctypes
import os

import numpy as np
import pytest

from test_find_pattern import CNT_FIND_BOTH_STRANDS, pack_pattern, planted_sequence, assert_plants, random_pattern, ref_find, words_of_codes
from test_minimizers import CNT_KMER_CANONICAL, _random_words, np_minimizers
from test_orfs import (ATG, ATG_CODES, CAT, CNT_FIND_REVERSE, CNT_ORF_BOTH_STRANDS, CNT_ORF_NO_STOP, CNT_ORF_OPEN_END, CODE, STOPS, TAA, TAG, TGA, TTA,
                       _planted, acg, np_orfs, orf_tiles, plant)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("minimizers", "find", "orfs")
TILE = {"minimizers": 2048, "find": 8192, "orfs": 8192}  # kMinTile windows, kFindTile windows, kOrfTile positions
GROUP = 16      # kCountedGroup: tiles per offset of the shared scan
ORF_PAIRS = 6   # kOrfPairs: (strand, lane)
MIN_K, MIN_W = 15, 10
FIND_K, FIND_D = 12, 4


# ---- the model ------------------------------------------------------------------------------------------------------------
# The carving, stated once, in hip/counted_output.hpp (counted_carve; `behind` is its third member):
#     const uint64_t groups = (n_tiles + kCountedGroup - 1) / kCountedGroup;
#     uint64_t* offs = reinterpret_cast<uint64_t*>((reinterpret_cast<uintptr_t>(d_work) + 15) & ~(uintptr_t)15);
#     uint32_t* counts = reinterpret_cast<uint32_t*>(offs + ((groups + 1) & ~1ull));
#     return {offs, counts, counts + groups * kCountedGroup};
# which hip/minimizer_abi.inc, hip/find_abi.inc and hip/orf_abi.inc each call on their own number of tiles, and in hip/orf_abi.inc
# behind it
#     uint32_t* sums = static_cast<uint32_t*>(work.behind);
#     uint64_t* carry = reinterpret_cast<uint64_t*>(sums + n_tiles * kOrfPairs);
# with carry holding 2 * kOrfPairs u64 per tile (hip/orf_kernels.hpp: "uint64_t* carry;  // [kOrfPairs][2][n_tiles]: stop, start").
# The byte formula of the queries is there too (counted_scratch_bytes), and orf_abi.inc adds its own regions to it.
CARVE_CALL = "const CountedScratch work = counted_carve(d_work, n_tiles);"
CARVING = {
    "counted_output.hpp": ["constexpr int kCountedScanBlock = 1024, kCountedGroup = 16;",
                           "const uint64_t groups = (n_tiles + kCountedGroup - 1) / kCountedGroup;",
                           "uint64_t* offs = reinterpret_cast<uint64_t*>((reinterpret_cast<uintptr_t>(d_work) + 15) & ~(uintptr_t)15);",
                           "uint32_t* counts = reinterpret_cast<uint32_t*>(offs + ((groups + 1) & ~1ull));",
                           "return {offs, counts, counts + groups * kCountedGroup};",
                           "if (!n_tiles) return 0;",
                           "return 16 + ((groups + 1) & ~1ull) * 8 + groups * kCountedGroup * 4;"],
    "minimizer_abi.inc": ["const uint64_t n_tiles = (n_win + kMinTile - 1) / kMinTile;", CARVE_CALL,
                          "uint64_t minimizer_work_bytes(uint64_t n_win) { return counted_scratch_bytes((n_win + kMinTile - 1) / kMinTile); }"],
    "find_abi.inc": ["const uint64_t n_tiles = (m + kFindTile - 1) / kFindTile;", CARVE_CALL,
                     "uint64_t find_work_bytes(uint64_t m) { return counted_scratch_bytes((m + kFindTile - 1) / kFindTile); }"],
    "orf_abi.inc": ["const uint64_t n_tiles = orf_tiles(len);", CARVE_CALL,
                    "uint32_t* sums = static_cast<uint32_t*>(work.behind);",
                    "uint64_t* carry = reinterpret_cast<uint64_t*>(sums + n_tiles * kOrfPairs);",
                    "uint64_t orf_work_bytes(uint64_t n_tiles) { return counted_scratch_bytes(n_tiles) + n_tiles * kOrfPairs * (4 + 2 * 8); }"],
}
# The stores into the scratch, all there are:
#   offs[0 .. groups)        hip/counted_output.hpp counted_scan        "if (g < n_groups) offs[g] = before;"
#   counts[0 .. n_tiles)     hip/minimizer_kernels.hpp minimizer_tiles  "counts[tile] = (uint32_t)c;"
#                            hip/find_kernels.hpp find_tile             "if (j == 0) counts[tile] = tile_total<kFindWaves>(s_cnt);"
#                            hip/orf_kernels.hpp orf_tile               "if (j == 0) a.counts[tile] = tile_total<kOrfWaves>(s_cnt);"
#   sums[p][0 .. n_tiles)    hip/orf_kernels.hpp orf_summary            "if (threadIdx.x < (both ? kOrfPairs : 3)) {" ... "a.sums[p * a.n_tiles + tile] = v;"
#   carry[p][0 .. 2)[0 .. n_tiles)  hip/orf_kernels.hpp orf_carry       "uint64_t* out_stop = carry + 2ull * p * n_tiles;" "uint64_t* out_start = out_stop + n_tiles;"
#                            "if (t < n_tiles) {" "out_stop[t] = f_stop;" "out_start[t] = f_start;", p = blockIdx.x of the launch
#                            hip/orf_abi.inc "hipLaunchKernelGGL(orf_carry, dim3(both ? kOrfPairs : 3), dim3(kOrfCarryBlock), 0, s, sums, carry, n_tiles);"
# every tile of a call runs its count pass and every group its scan lane, so a call that has finished HAS written all of these;
# the odd offs slot, the counts of the tiles a last group lacks and, on one strand, pairs 3 .. 5 of sums and carry are never stored.
STORES = {
    "counted_output.hpp": ["if (g < n_groups) offs[g] = before;"],
    "minimizer_kernels.hpp": ["counts[tile] = (uint32_t)c;"],
    "find_kernels.hpp": ["if (j == 0) counts[tile] = tile_total<kFindWaves>(s_cnt);"],
    "orf_kernels.hpp": ["if (j == 0) a.counts[tile] = tile_total<kOrfWaves>(s_cnt);", "if (threadIdx.x < (both ? kOrfPairs : 3)) {", "a.sums[p * a.n_tiles + tile] = v;",
                        "uint64_t* out_stop = carry + 2ull * p * n_tiles;", "uint64_t* out_start = out_stop + n_tiles;", "out_stop[t] = f_stop;",
                        "out_start[t] = f_start;", "uint64_t* carry;           // [kOrfPairs][2][n_tiles]: stop, start"],
    "orf_abi.inc": ["hipLaunchKernelGGL(orf_carry, dim3(both ? kOrfPairs : 3), dim3(kOrfCarryBlock), 0, s, sums, carry, n_tiles);"],
}


def scratch_layout(op, n_tiles, both=False):
    """byte extents [lo, hi) of the regions of a call's scratch, relative to its base (d_work rounded up to 16 B), and `body`,
    the end of the last one.  The layout does not depend on `both`: one strand leaves the tail of sums and carry unused."""
    assert op in OPS
    groups = -(-n_tiles // GROUP)
    offs = (0, (groups + groups % 2) * 8)
    counts = (offs[1], offs[1] + groups * GROUP * 4)
    lay = {"offs": offs, "counts": counts, "body": counts[1]}
    if op == "orfs":
        sums = (counts[1], counts[1] + n_tiles * ORF_PAIRS * 4)
        carry = (sums[1], sums[1] + n_tiles * ORF_PAIRS * 2 * 8)
        lay.update(sums=sums, carry=carry, body=carry[1])
    return lay


def model_work_bytes(op, n_tiles):
    """what the query answers: the body and the 16 B that rounding d_work up can cost; nothing without a tile"""
    return 16 + scratch_layout(op, n_tiles)["body"] if n_tiles else 0


def written_extent(op, n_tiles, both=False):
    """the [lo, hi) byte ranges, relative to the base and ascending, that a finished call has written (STORES above)"""
    lay = scratch_layout(op, n_tiles, both)
    groups = -(-n_tiles // GROUP)
    ext = [(0, groups * 8), (lay["counts"][0], lay["counts"][0] + n_tiles * 4)]
    if op == "orfs":
        pairs = ORF_PAIRS if both else 3
        ext += [(lay["sums"][0], lay["sums"][0] + pairs * n_tiles * 4), (lay["carry"][0], lay["carry"][0] + pairs * 2 * n_tiles * 8)]
    return ext


def assert_contained(prefill, after, lo, hi):
    """raises, naming the first offending offset, if a byte outside [lo, hi) differs from its prefill"""
    prefill, after = np.asarray(prefill, dtype=np.uint8), np.asarray(after, dtype=np.uint8)
    assert prefill.shape == after.shape and prefill.ndim == 1 and 0 <= lo <= hi <= prefill.size
    changed = np.flatnonzero(prefill != after)
    outside = changed[(changed < lo) | (changed >= hi)]
    if outside.size:
        at = int(outside[0])
        raise AssertionError("byte %d outside the scratch body [%d, %d) changed from 0x%02X to 0x%02X (%d such bytes)"
                             % (at, lo, hi, int(prefill[at]), int(after[at]), outside.size))


def length_for(op, tiles):
    """the smallest length whose call has `tiles` tiles (for ORFs: 100 nt into the last tile)"""
    if op == "orfs":
        return (tiles - 1) * TILE[op] + 100
    if op == "find":
        return (tiles - 1) * TILE[op] + 1 + FIND_K - 1          # m = len - k + 1 windows
    return (tiles - 1) * TILE[op] + 1 + MIN_K - 1 + MIN_W - 1   # W = len - k + 1 - w + 1 windows


def tiles_of(op, n_len):
    if op == "orfs":
        return orf_tiles(n_len)
    n = n_len - FIND_K + 1 if op == "find" else n_len - MIN_K + 1 - MIN_W + 1
    return -(-max(n, 0) // TILE[op])


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from cute_nucleotides_amd import _lib, build

    build.build()
    return _lib.lib()


def _query(op, n_len):
    from cute_nucleotides_amd import packed_ops as po

    if op == "minimizers":
        return po.minimizers_work_bytes(n_len, MIN_K, MIN_W)
    return po.find_pattern_work_bytes(n_len, FIND_K) if op == "find" else po.orfs_work_bytes(n_len)


@pytest.mark.parametrize("op", OPS)
def test_layout_model_equals_the_queries(L, op):
    for tiles in (1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 16385):
        n_len = length_for(op, tiles)
        assert tiles_of(op, n_len) == tiles and tiles_of(op, n_len - (101 if op == "orfs" else 1)) == tiles - 1
        lay = scratch_layout(op, tiles)
        assert _query(op, n_len) == 16 + lay["body"] == model_work_bytes(op, tiles), (op, tiles)
        # the regions follow each other without a gap, each aligned for its element, and the written extent lies inside them
        names = ("offs", "counts") + (("sums", "carry") if op == "orfs" else ())
        assert lay["offs"][0] == 0 and all(lay[a][1] == lay[b][0] for a, b in zip(names, names[1:])) and lay[names[-1]][1] == lay["body"]
        assert lay["counts"][0] % 16 == 0 and all(lay[n][0] % 8 == 0 for n in names)
        for both in (False, True):
            ext = written_extent(op, tiles, both)
            assert len(ext) == len(names) and all(lay[n][0] == lo < hi <= lay[n][1] for n, (lo, hi) in zip(names, ext))
            assert ext[-1][1] == lay["body"] or (op != "orfs" and tiles % GROUP) or (op == "orfs" and not both)
    # no tile: no scratch
    assert model_work_bytes(op, 0) == 0 and scratch_layout(op, 0)["body"] == 0
    for n_len in (0, 1, 2) + ((FIND_K - 1,) if op == "find" else (MIN_K + MIN_W - 3,) if op == "minimizers" else ()):
        assert tiles_of(op, n_len) == 0 and _query(op, n_len) == 0, (op, n_len)


def test_layout_model_quotes_the_sources():
    """the lines the model is read off are the launchers' and the kernels': a change of the carving or of a store shows up here"""
    for quotes in (CARVING, STORES):
        for name, lines in quotes.items():
            text = " ".join(open(os.path.join(ROOT, "hip", name)).read().split())
            for line in lines:
                assert " ".join(line.split()) in text, (name, line)
    # the carving lines and the byte formula are stated in counted_output.hpp alone
    for name in ("minimizer_abi.inc", "find_abi.inc", "orf_abi.inc", "minimizer_kernels.hpp", "find_kernels.hpp", "orf_kernels.hpp"):
        text = open(os.path.join(ROOT, "hip", name)).read()
        assert "& ~(uintptr_t)15" not in text and "& ~1ull" not in text and "return 16 +" not in text, name


def test_guard_checker_on_synthetic_buffers():
    rng = np.random.default_rng(5)
    size, lo, hi = 256 + 16 + 200 + 256, 272, 272 + 184
    pre = np.full(size, 0xA5, dtype=np.uint8)
    pre[257 : 257 + 200] = 0xFF
    inside = pre.copy()
    inside[lo:hi] = rng.integers(0, 256, hi - lo, dtype=np.uint8)
    inside[lo], inside[hi - 1] = 0, 0
    assert_contained(pre, pre.copy(), lo, hi)  # nothing written at all
    assert_contained(pre, inside, lo, hi)      # written inside only, both edge bytes included
    for at in (lo - 1, hi, size - 1, 0, 255, 256, hi + 15):
        bad = inside.copy()
        bad[at] ^= 0x01
        with pytest.raises(AssertionError, match=r"byte %d outside" % at):
            assert_contained(pre, bad, lo, hi)
    two = inside.copy()
    two[hi + 3] ^= 0x80
    two[lo - 2] ^= 0x80
    with pytest.raises(AssertionError, match=r"byte %d outside .*\(2 such bytes\)" % (lo - 2)):  # the FIRST offender is named
        assert_contained(pre, two, lo, hi)
    assert_contained(pre, two, lo - 2, hi + 4)
    with pytest.raises(AssertionError):
        assert_contained(pre, inside[:-1], lo, hi)  # not the same buffer


# ---- GPU: containment, any contents, any alignment --------------------------------------------------------------------------
gpu = pytest.mark.gpu
GUARD = 256
PHASES = (0, 1, 7, 8, 15)
SENTINEL = -0x3C3C3C3C3C3C3C3D
CONTAINED_TILES = (1, 15, 16, 17, 32, 33)


def _input_and_reference(oracle, op, tiles, option, seed):
    """(words, length, pattern, reference) of the containment runs: inputs on which most tiles emit, so that the write pass runs
    everywhere"""
    rng = np.random.default_rng(seed)
    n_len, pat = length_for(op, tiles), None
    if op == "minimizers":  # random ACGT: one new position per (w + 1) / 2 windows
        words = _random_words(rng, n_len)
        want = np_minimizers(words, n_len, MIN_K, MIN_W, option)
        dense = want[0].size >= max(1, (tiles - 1) * (TILE[op] // MIN_W))
    elif op == "find":  # random ACGT has 8192 * 46666 / 4^12 = 23 windows per tile and strand within 4 substitutions; plants on top
        pat = pack_pattern(*random_pattern(rng, FIND_K, 0))
        m = n_len - FIND_K + 1
        free = max((m - 1 - FIND_K - 1) // (FIND_K + 1), 0)
        sites = [m - 1] + [int(j) * (FIND_K + 1) for j in rng.permutation(free)[:8]]  # the last window (the last tile's only one) is a hit
        s, plants = planted_sequence(rng, n_len, pat, FIND_D, option, at=sites)
        words = words_of_codes(oracle, s, rng=rng)
        want = ref_find(oracle, words, n_len, pat, FIND_D, option)
        assert_plants(want, plants, FIND_D, option, need_all=n_len >= 200)
        dense = np.unique(want[0] // np.uint64(TILE[op])).size == tiles  # every tile emits
    else:  # 82 planted stops and starts per tile
        s = _planted(rng, n_len, 0.01)
        words = words_of_codes(oracle, s, rng=rng)
        want = np_orfs(s, STOPS, ATG, 0, option)
        fwd = (want[2] & np.uint64(CNT_FIND_REVERSE)) == 0  # a forward entry is closed by the bound at pos + length
        dense = np.unique((want[0] + want[1])[fwd] // np.uint64(TILE[op])).size >= tiles - 1 and want[0].size >= 10 * (tiles - 1)
    assert dense, (op, tiles, option, want[0].size)
    return words, n_len, pat, want


class _Call:
    """one device call on an input made for (op, tiles, option) with outputs of its own (capacity >= the reference's count, so the
    write pass leaves no entry out) and its reference: enqueue(work) through the Python wrapper, enqueue_raw(work) through the C
    ABI with work_bytes = the view's size, check(tag) after a synchronisation"""

    def __init__(self, oracle, op, tiles, option, seed):
        import torch

        from cute_nucleotides_amd import packed_ops as po

        self.op, self.tiles, self.option = op, tiles, option
        words, self.n_len, self.pat, self.want = _input_and_reference(oracle, op, tiles, option, seed)
        self.n = self.want[0].size
        self.need = _query(op, self.n_len)
        assert tiles_of(op, self.n_len) == tiles and self.need == model_work_bytes(op, tiles)
        self.bits = torch.from_numpy(words.view(np.int64)).cuda()
        cap = self.n + 8
        assert cap >= self.n  # nothing is left out by the capacity
        self.outs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in self.want]
        self.count = torch.empty(1, dtype=torch.int64, device="cuda")
        self.torch, self.po = torch, po

    def clear(self):
        for t in self.outs + [self.count]:
            t.fill_(SENTINEL)

    def enqueue(self, work):
        po, o = self.po, self.outs
        if self.op == "minimizers":
            po.minimizers_dev(self.bits, self.n_len, MIN_K, MIN_W, canonical=self.option, pos=o[0], val=o[1], work=work, count=self.count)
        elif self.op == "find":
            po.find_pattern_dev(self.bits, self.n_len, self.pat, FIND_D, both_strands=self.option, pos=o[0], info=o[1], work=work, count=self.count)
        else:
            po.orfs_dev(self.bits, self.n_len, STOPS, ATG, 0, both_strands=self.option, pos=o[0], lens=o[1], info=o[2], work=work, count=self.count)

    def enqueue_raw(self, work):
        from cute_nucleotides_amd import _lib

        lib = _lib.lib()
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        o, cap, nbytes = self.outs, self.outs[0].numel(), work.numel()
        stream = ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        if self.op == "minimizers":
            return lib.cnt_minimizers_dev(p(self.bits), self.n_len, MIN_K, MIN_W, CNT_KMER_CANONICAL if self.option else 0, p(o[0]), p(o[1]), cap,
                                          p(self.count), p(work), nbytes, stream)
        if self.op == "find":
            return lib.cnt_find_pattern_dev(p(self.bits), self.n_len, self.pat[0], FIND_K, self.pat[1], FIND_D, CNT_FIND_BOTH_STRANDS if self.option else 0,
                                            p(o[0]), p(o[1]), cap, p(self.count), p(work), nbytes, stream)
        return lib.cnt_orfs_dev(p(self.bits), self.n_len, STOPS, ATG, 0, CNT_ORF_BOTH_STRANDS if self.option else 0, p(o[0]), p(o[1]), p(o[2]), cap,
                                p(self.count), p(work), nbytes, stream)

    def check(self, tag):
        n = int(self.count.item())
        assert n == self.n, tag + (n, self.n)
        for j, (o, w) in enumerate(zip(self.outs, self.want)):
            h = o.cpu().numpy()
            assert np.array_equal(h[:n].view(np.uint64), w) and (h[n:] == SENTINEL).all(), tag + (j,)


def _check_contained(call, raw=False):
    """the call on exactly its queried bytes at every phase, zeroed and filled with 0xFF, between the guards.  Returns the
    high-water mark of the written bytes, relative to the aligned base."""
    import torch

    from cute_nucleotides_amd import _lib

    op, tiles, both = call.op, call.tiles, call.option and call.op == "orfs"
    need, lay, ext = call.need, scratch_layout(op, tiles, both), written_extent(op, tiles, both)
    assert need == 16 + lay["body"]
    buf = torch.empty(GUARD + 16 + need + GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    high = None
    for ph in PHASES:
        v0 = GUARD + ph
        lo = (v0 + 15) & ~15  # the buffer's base is 16-B aligned: offsets round as addresses do
        hi = lo + lay["body"]
        assert v0 <= lo and hi <= v0 + need
        written = np.zeros(buf.numel(), dtype=bool)
        for fill in (0x00, 0xFF):
            tag = (op, tiles, call.option, ph, fill, raw)
            pre = np.full(buf.numel(), 0xA5, dtype=np.uint8)
            pre[v0 : v0 + need] = fill
            buf.fill_(0xA5)
            view = buf[v0 : v0 + need]
            view.fill_(fill)
            call.clear()
            if raw:
                assert view.numel() == need and call.enqueue_raw(view) == _lib.CNT_OK, tag
            else:
                call.enqueue(view)
            torch.cuda.synchronize()
            after = buf.cpu().numpy()
            call.check(tag)  # the same result from either prefill: the scratch needs no initialisation
            assert_contained(pre, after, lo, hi)  # neither guard, nor the view outside [base, base + body)
            written |= after != pre
        at = np.flatnonzero(written)  # every byte stored differs from 0x00 or from 0xFF
        assert at.size and int(at[0]) == lo and int(at[-1]) + 1 == lo + ext[-1][1], (op, tiles, call.option, ph, int(at[0]) - lo, int(at[-1]) + 1 - lo, ext)
        for a, b in ext:
            assert written[lo + a : lo + b].all(), (op, tiles, call.option, ph, a, b)
        high = int(at[-1]) + 1 - lo
    print("scratch high-water %-10s tiles %2d option %d%s: observed %d, model %d, body %d, queried %d"
          % (op, tiles, call.option, " raw" if raw else "", high, ext[-1][1], lay["body"], need))
    return high


@gpu
@pytest.mark.parametrize("option", [False, True])  # minimizers: canonical; find, ORFs: both strands
@pytest.mark.parametrize("op", OPS)
def test_gpu_scratch_is_contained_at_any_contents_and_alignment(oracle, op, option):
    for tiles in CONTAINED_TILES:
        call = _Call(oracle, op, tiles, option, seed=1000 * OPS.index(op) + 2 * tiles + option)
        assert _check_contained(call) == written_extent(op, tiles, option and op == "orfs")[-1][1]


@gpu
@pytest.mark.parametrize("op", OPS)
def test_gpu_scratch_is_contained_through_the_c_abi(oracle, op):
    """work_bytes == the query exactly, at every phase: CNT_OK and the same containment"""
    call = _Call(oracle, op, 17, True, seed=77 + OPS.index(op))
    assert _check_contained(call, raw=True) == written_extent(op, 17, op == "orfs")[-1][1]


@gpu
def test_gpu_one_scratch_shared_by_all_three_ops_in_stream_order(oracle):
    """ORFs, find, minimizers and ORFs again enqueued back to back on one stream, all on one scratch view sized for the largest
    of them and left as the previous call left it, no host synchronisation in between"""
    import torch

    calls = [_Call(oracle, "orfs", 17, True, 1), _Call(oracle, "find", 33, True, 2), _Call(oracle, "minimizers", 32, True, 3), _Call(oracle, "orfs", 16, False, 4)]
    need = max(c.need for c in calls)
    body = max(scratch_layout(c.op, c.tiles)["body"] for c in calls)
    assert need == 16 + body and len({c.need for c in calls}) == 4
    buf = torch.empty(GUARD + 16 + need + GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    side = torch.cuda.Stream()
    for ph in (7, 0):
        v0 = GUARD + ph
        lo = (v0 + 15) & ~15
        pre = np.full(buf.numel(), 0xA5, dtype=np.uint8)
        pre[v0 : v0 + need] = 0xFF
        buf.fill_(0xA5)
        buf[v0 : v0 + need].fill_(0xFF)
        for c in calls:
            c.clear()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for c in calls:
                c.enqueue(buf[v0 : v0 + need])
        side.synchronize()
        for j, c in enumerate(calls):
            c.check((j, c.op, ph))
        assert_contained(pre, buf.cpu().numpy(), lo, lo + body)


# ---- GPU: orf_carry and the offset scan at their own edges -------------------------------------------------------------------
T = 8192
WAVE, ROUND = 64, 1024              # orf_carry: tiles per wave and per round (kOrfCarryBlock)
N_EDGE = 1026 * T + 11              # 1027 tiles; the last holds 11 nucleotides and the three closing bounds
EDGE = ROUND * T
# The last tile's 11 nucleotides for rotation r (lanes: X = r, Y = r + 1, Z = r + 2; tile 1026 begins in lane 0): forward stops in
# the lanes of Y and Z, a reverse stop (CTA) in the lane of Z, no ATG and no CAT; "GG" goes in front (what plant() puts there).
TAILS = ("ATAAACTATAA", "CTATAAAATAA", "TAAACTATAAA")


def _at(tile, off, lane):
    """the first position at or behind tile * T + off in the lane"""
    p = tile * T + off
    return p + (lane - p) % 3


def _edge_sequence(rng, r):
    """random {A,C,G} with the scenarios of the edges planted, rotation r of the lanes.  Forward lane X: the wave edge (stop in
    tile 63, ATG in tile 64, stop in tile 65), fillers that close an entry in tiles 1022 and 1023, then the round edge (stop in the
    last word of tile 1023, ATG in the first word of tile 1024, stops in tiles 1024 and 1025 with an ATG between them: the three
    lanes are all taken across tile 1024, so the entry that tile 1024 must close is the round edge's own).  Forward lane Y: the
    first-start rule (stop in tile 5, ATG in tiles 1023 and 1024, stop in tile 1026).  Forward lane Z: a run carried through a whole
    round (stop and ATG in tile 0, stop in tile 1026).  Reverse, lane Z: the last-start rule (TTA in tiles 2 and 1026 -- CTA there --
    CAT in tiles 1023 and 1024).  Reverse, lane X: a stop straddling the round edge at offset r - 2.  Returns the codes and the
    named positions."""
    lx, ly, lz = r, (r + 1) % 3, (r + 2) % 3
    s = acg(rng, N_EDGE)
    P = dict(
        stop63=_at(63, 4000, lx), atg64=_at(64, 4000, lx), stop65=_at(65, 4000, lx),
        atg1022=_at(1022, 300, lx), stop1022=_at(1022, 3000, lx), atg1023=_at(1023, 600, lx),
        stop1023=EDGE - 8 - (EDGE - 8 - lx) % 3, atg1024=EDGE + 8 + (lx - EDGE - 8) % 3,
        stop1024=_at(1024, 4000, lx), atg1024b=_at(1024, 5000, lx), stop1025=_at(1025, 2000, lx),
        y_stop5=_at(5, 1000, ly), y_atg1023=_at(1023, 2000, ly), y_atg1024=_at(1024, 2500, ly),
        z_stop0=_at(0, 300, lz), z_atg0=_at(0, 900, lz),
        r_tta2=_at(2, 1500, lz), r_cat1023=_at(1023, 5000, lz), r_cat1024=_at(1024, 6500, lz),
        e_tta=EDGE + r - 2)
    assert EDGE - 32 <= P["stop1023"] and P["stop1023"] + 4 < EDGE - 3 and EDGE + 4 < P["atg1024"] - 1 and P["atg1024"] + 2 < EDGE + 32  # the edge's two words
    assert P["e_tta"] % 3 == lx and all(P[k] % 3 == lx for k in P if k[:2] not in ("y_", "z_", "r_", "e_"))
    assert all(P[k] % 3 == ly for k in P if k[:2] == "y_") and all(P[k] % 3 == lz for k in P if k[:2] in ("z_", "r_"))
    kinds = dict(stop63=TAA, stop65=TGA, stop1022=TAG, stop1023=TAA, stop1024=TGA, stop1025=TAG, y_stop5=TGA, z_stop0=TAA, r_tta2=TTA, e_tta=TTA)
    for name, at in P.items():
        plant(s, at, kinds.get(name, CAT if "cat" in name else ATG_CODES))
    s[1026 * T - 2 :] = [CODE[ch] for ch in "GG" + TAILS[r]]
    return s, P


def _entries(want):
    """{pos: length} of the forward entries and of the reverse ones, and {pos: info} of all"""
    rev = (want[2] & np.uint64(CNT_FIND_REVERSE)) != 0
    return tuple({int(p): int(l) for p, l in zip(want[0][k], want[1][k])} for k in (~rev, rev)) + ({int(p): int(i) for p, i in zip(want[0], want[2])},)


def _assert_edge_reference(want, P, starts, both):
    """what the reference must show before the library is asked"""
    fwd, rev, info = _entries(want)
    if starts:
        assert fwd[P["atg64"]] == P["stop65"] - P["atg64"]                      # the wave edge: begins at the ATG of tile 64
        assert fwd[P["atg1024"]] == P["stop1024"] - P["atg1024"]                # the round edge: begins at the ATG of tile 1024
        for a in (P["y_atg1023"], P["z_atg0"]):  # closed by a stop of tile 1026, not by the end of the sequence
            assert 1026 * T <= a + fwd[a] <= N_EDGE - 3 and not info[a] & CNT_ORF_NO_STOP
        assert P["y_atg1024"] not in fwd    # the first start
        assert fwd[P["z_atg0"]] > ROUND * T  # carried through a whole round
        if both:  # the last start: the reverse entry opened by the TTA of tile 2 ends at the CAT of tile 1024
            assert rev[P["r_tta2"] + 3] == P["r_cat1024"] + 3 - (P["r_tta2"] + 3) and not info[P["r_tta2"] + 3] & (CNT_ORF_OPEN_END | CNT_ORF_NO_STOP)
    else:
        assert fwd[P["stop63"] + 3] == P["stop65"] - P["stop63"] - 3
        assert fwd[P["stop1023"] + 3] == P["stop1024"] - P["stop1023"] - 3
        assert fwd[P["y_stop5"] + 3] > (1026 - 6) * T and fwd[P["z_stop0"] + 3] > ROUND * T
        if both:  # the runs on either side of the stop that straddles the round edge
            assert rev[P["e_tta"] + 3] >= 300 and any(p + l == P["e_tta"] for p, l in rev.items())
    assert int(want[1].max()) > ROUND * T  # an entry longer than a round of tiles
    closed = {(p + l) // T for p, l in fwd.items()}  # a forward entry is closed by the bound at pos + length
    assert {1022, 1023, 1024, 1025} <= closed, sorted(closed)  # counts on both sides of the scan's group 63 | 64


def _run_edge_sequence(oracle, s, check, host):
    import torch

    from cute_nucleotides_amd import packed_ops as po

    src = words_of_codes(oracle, s)
    bits = torch.from_numpy(src.view(np.int64)).cuda()
    for starts in (0, ATG):
        for both in (False, True):
            want = np_orfs(s, STOPS, starts, 300, both)
            check(want, starts, both)
            n = want[0].size
            outs = [torch.full((n + 8,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(3)]
            count = po.orfs_dev(bits, len(s), STOPS, starts, 300, both_strands=both, pos=outs[0], lens=outs[1], info=outs[2])[3]
            assert int(count.item()) == n, (starts, both, int(count.item()), n)
            for j, o in enumerate(outs):
                h = o.cpu().numpy()
                assert np.array_equal(h[:n].view(np.uint64), want[j]) and (h[n:] == SENTINEL).all(), (starts, both, j)
            if host and starts and both:
                got = po.orfs_hip(src, len(s), STOPS, starts, 300, both_strands=True)
                assert all(np.array_equal(g, w) for g, w in zip(got, want))


@gpu
@pytest.mark.parametrize("r", range(3))
def test_gpu_orf_carry_at_wave_and_round_edges(oracle, r):
    """1027 tiles: _edge_sequence's scenarios with the lanes rotated by r, whole runs and ATG-trimmed, one strand and both, entry
    by entry against np_orfs; the host tier once"""
    assert orf_tiles(N_EDGE) == ROUND + 3 and N_EDGE % T == 11
    s, P = _edge_sequence(np.random.default_rng(60 + r), r)
    _run_edge_sequence(oracle, s, lambda want, starts, both: _assert_edge_reference(want, P, starts, both), host=r == 0)


@gpu
@pytest.mark.parametrize("off", (-2, -1, 0))
def test_gpu_orf_forward_stop_straddling_the_round_edge(oracle, off):
    """a forward stop whose three nucleotides straddle position 1024 * 8192 (offsets -2 and -1: the bound belongs to tile 1023, the
    last lane of orf_carry's first round; offset 0: to tile 1024, the first lane of the second), starts on either side in its lane"""
    lane = (EDGE + off) % 3
    s = acg(np.random.default_rng(70 + off), N_EDGE)
    a0, a1, z = _at(1022, 5000, lane), _at(1024, 3000, lane), _at(1025, 100, lane)
    for at, codes in ((a0, ATG_CODES), (EDGE + off, TAA), (a1, ATG_CODES), (z, TAG), (_at(1023, 7000, (lane + 1) % 3), CAT), (_at(1025, 900, (lane + 1) % 3), TTA)):
        plant(s, at, codes)

    def check(want, starts, both):
        fwd, rev, _ = _entries(want)
        if starts:
            assert fwd[a0] == EDGE + off - a0 and fwd[a1] == z - a1
        else:
            assert fwd[EDGE + off + 3] == z - (EDGE + off) - 3 and any(p + l == EDGE + off for p, l in fwd.items())
        assert not both or len(rev) >= 1

    _run_edge_sequence(oracle, s, check, host=False)


@gpu
@pytest.mark.parametrize("both", [False, True])
def test_gpu_find_offsets_across_the_scan_wave_edge(oracle, both):
    """1026 tiles of windows, k = 12, the all-T pattern exactly (absent from random {A,C,G}): hits planted on both sides of the
    scan's group edges 0 | 1 (tiles 15, 16, 17), 62 | 63 (1007, 1008) and 63 | 64 -- the edge between its waves -- (1023, 1024,
    1025), in the last window, and across the tile edges there; with both strands all-A runs as well"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    k = FIND_K
    pat = pack_pattern([CODE["T"]] * k, [False] * k)
    rng = np.random.default_rng(90 + both)
    s = acg(rng, N_EDGE)
    m = N_EDGE - k + 1
    assert m == 1026 * T and tiles_of("find", N_EDGE) == 1026
    t_sites = [t * T + 1234 + 17 * j for j, t in enumerate((15, 16, 17, 1007, 1008, 1023, 1024, 1025))]
    t_sites += [16 * T - 1, 16 * T + 40, 1008 * T - 1, 1008 * T + 40, EDGE - 6, EDGE + 40, EDGE - 60, m - 1]  # last and first windows of tiles, one across the edge
    a_sites = [15 * T + 5000, 1008 * T + 5000, EDGE - 200, EDGE + 5000, 1025 * T + 7000]
    for p in t_sites:
        s[p : p + k] = CODE["T"]
    for p in a_sites:
        s[p : p + k] = CODE["A"]
    src = words_of_codes(oracle, s)
    want = ref_find(oracle, src, N_EDGE, pat, 0, both)
    hits = {(int(p), int(i) >> 8) for p, i in zip(*want)}
    assert all((p, 0) in hits for p in t_sites) and (not both or all((p, 1) in hits for p in a_sites))
    assert (want[1] & np.uint64(0xFF)).max() == 0 and want[0].size >= len(t_sites) + (len(a_sites) if both else 0)
    per_tile = np.bincount((want[0] // np.uint64(T)).astype(np.int64), minlength=1026)
    assert all(per_tile[t] >= 1 for t in (15, 16, 17, 1007, 1008, 1023, 1024, 1025)) and per_tile[:15].sum() <= 8 * both
    n = want[0].size
    outs = [torch.full((n + 8,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(2)]
    count = po.find_pattern_dev(torch.from_numpy(src.view(np.int64)).cuda(), N_EDGE, pat, 0, both_strands=both, pos=outs[0], info=outs[1])[2]
    assert int(count.item()) == n, (int(count.item()), n)
    for j, o in enumerate(outs):
        h = o.cpu().numpy()
        assert np.array_equal(h[:n].view(np.uint64), want[j]) and (h[n:] == SENTINEL).all(), j
