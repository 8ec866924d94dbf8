"""The three persistent kernels where their grid wraps: hamming_persist<8>, validate_persist<16, ALLOW_N> and
kmer_count<true/false> walk pieces g, g+G, g+2G, ... with the next piece's loads in flight, G sized from the device's CU
count.  Every other small-shape test has fewer pieces than G, so each wave takes one piece, the loop body runs once and the
prefetch is always the re-read; only the 2^32 / 2^33-nt cases go round the loop, each at one length.

The CPU part quotes the constants and the loop lines the model restates, runs the model of the walk (and of the lab build's
hamming_order 1 / 2 arithmetic) over every (G, n) around the wrap, and holds the inputs of the GPU part to the condition that
makes a total worth comparing: on the run grid the launcher really uses (behind the head it peels) every piece holds another,
non-zero count, so "piece i dropped, piece j counted twice" moves the total.  That is a condition on the inputs, not a
tolerance: every comparison in this file is exact.

The GPU part reads the CU count through cnt_chip_info (a partitioned device has a smaller G and gets smaller inputs) and
calls both tiers at n = G-1, G, G+1, 2G-1, 2G, 2G+1 (3G+1) pieces, against the scalar oracle and against the closed-form sum
of the planted weights."""
import ctypes
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

# hip/packed_ops_kernels.hpp, hip/kmer_count_kernels.hpp, hip/kmer_count_abi.inc (test_constants_and_loops_quote_the_sources)
HAMMING_RUN_KIB, HAMMING_WAVES_PER_CU = 8, 2
VALIDATE_RUN_KIB, VALIDATE_WAVES_PER_CU = 16, 4
KMER_GROUPS_PER_CU = 2
KMER_BLOCK = 1024

H_RUN_WORDS = HAMMING_RUN_KIB * 1024 // 8  # packed words per piece and stream
H_RUN_NT = 32 * H_RUN_WORDS
V_RUN = VALIDATE_RUN_KIB * 1024  # bytes per piece
TILE_WORDS = KMER_BLOCK
TILE = 32 * TILE_WORDS  # k-mers per tile
H_PAGE_GRAIN_NT, V_PAGE_GRAIN_BYTES = 1 << 24, 1 << 22  # from these sizes on the launchers peel to a 4-KiB page, not a 128-B line

# piece counts on either side of G and 2G, as functions of the G the device has
RUN_COUNTS = {"G-1": lambda G: G - 1, "G": lambda G: G, "G+1": lambda G: G + 1, "2G-1": lambda G: 2 * G - 1, "2G": lambda G: 2 * G,
              "2G+1": lambda G: 2 * G + 1, "3G+1": lambda G: 3 * G + 1}
TILE_COUNTS = [c for c in RUN_COUNTS if c != "3G+1"]
# CU counts the CPU part rehearses the inputs at (the GPU part takes the device's): the smallest device there can be, an odd
# one, one XCD of a partitioned MI355X, the whole of it
MODEL_CUS = (1, 3, 32, 256)


def grids(cus):
    """the persistent grid sizes of a device with `cus` compute units"""
    return {"hamming": cus * HAMMING_WAVES_PER_CU, "validate": cus * VALIDATE_WAVES_PER_CU, "kmer": cus * KMER_GROUPS_PER_CU}


def _device_cus():
    import torch

    from cute_nucleotides_amd import _lib

    cus = ctypes.c_int(0)
    _lib.check(_lib.lib().cnt_chip_info(torch.cuda.current_device(), ctypes.byref(cus), None, None))
    assert cus.value >= 1
    return cus.value


def _src(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_constants_and_loops_quote_the_sources():
    kernels, abi = _src("hip", "packed_ops_kernels.hpp"), _src("hip", "packed_ops_abi.inc")
    assert "constexpr int kHammingRunKiB = %d, kHammingWavesPerCU = %d;" % (HAMMING_RUN_KIB, HAMMING_WAVES_PER_CU) in kernels
    assert "constexpr int kValidateRunKiB = %d, kValidateWavesPerCU = %d;" % (VALIDATE_RUN_KIB, VALIDATE_WAVES_PER_CU) in kernels
    assert "std::min<uint64_t>(n_runs, (uint64_t)chip_info().cus * kHammingWavesPerCU)" in abi
    assert "std::min<uint64_t>(n_runs, (uint64_t)chip_info().cus * kValidateWavesPerCU)" in abi
    assert "(hamming_persist<kHammingRunKiB>), dim3(grid), dim3(64)" in abi
    assert abi.count("(validate_persist<kValidateRunKiB, ") == 2
    # the walk of both reductions (walk(reread=True)) and of the lab orders (walk_lab)
    assert kernels.count("for (uint64_t t = g; t < n_runs; t += G) {") == 4
    assert kernels.count("const uint64_t nx = t + G < n_runs ? t + G : t;") == 2
    assert "const uint64_t last = g + (n_runs - 1 - g) / G * G;" in kernels
    assert "load(a, g + G <= last ? g + G : last, va2);" in kernels
    assert "load(a, t + 2 * G <= last ? t + 2 * G : last, va2);" in kernels
    assert kernels.count("load(b, t + G <= last ? t + G : last, vb);") == 2
    # the head rules (hamming_run_grid, validate_run_grid)
    assert "const uint64_t hgrain = len >= ((uint64_t)1 << 24) ? 4096 : 128;" in abi
    assert "uint64_t head_words = ((pa ^ pb) & 15) == 0 ? ((hgrain - (pa & (hgrain - 1))) & (hgrain - 1)) >> 3 : 0;" in abi
    assert "if (head_words > (len >> 5)) head_words = 0;" in abi
    assert "const uint64_t n_runs = ((len >> 5) - head_words) / kRunWords;" in abi
    assert "const uint64_t vgrain = n_len >= ((uint64_t)1 << 22) ? 4096 : 128;" in abi
    assert "uint64_t head = (vgrain - (reinterpret_cast<uintptr_t>(d_n) & (vgrain - 1))) & (vgrain - 1);" in abi
    assert "if (head > n_len) head = 0;" in abi and "const uint64_t n_runs = (n_len - head) / kRun;" in abi
    kk, ka = _src("hip", "kmer_count_kernels.hpp"), _src("hip", "kmer_count_abi.inc")
    assert "constexpr int kKmerCountBlock = %d;" % KMER_BLOCK in kk
    assert "kKmerCountTileWords = kKmerCountBlock, kKmerCountTileKmers = 32 * kKmerCountTileWords;" in kk
    assert ka.count("std::min<uint64_t>(n_tiles, (uint64_t)chip_info().cus * %d)" % KMER_GROUPS_PER_CU) == 2  # both launches
    assert "const uint64_t tn = t + gridDim.x, cur_lo = lo, cur_hi = hi;" in kk
    assert "if (tn < n_tiles) load(tn, lo, hi);" in kk  # walk(reread=False)
    # kmer_tile_is_fast: the shared loader's condition, which kmer_count instantiates at its tile size with BACK = 0 (the default)
    wt = _src("hip", "word_tile.hpp")
    assert "template <uint64_t TILE_WORDS, uint64_t BACK = 0>" in wt and wt.count("if (w0 >= BACK && w0 - BACK + TILE_WORDS + 1 <= words) {") == 1
    assert "word_tile_pair<kKmerCountTileWords>(in, words, t * kKmerCountTileWords, j, lo, hi);" in kk


# ---- the model of the walk ------------------------------------------------------------------------------------------------
def walk(G, n, reread=True, mutant=None):
    """The loop of hamming_persist / validate_persist (reread=True: the last iteration re-reads its own piece) and of
    kmer_count (reread=False: no load past the last tile), for n pieces on a persistent grid of G: the launcher starts
    min(G, n) waves, a wave counts what its registers hold and then loads the next piece into them.  Returns per wave
    (pieces counted, pieces loaded).  mutant: "twice" counts the re-read piece again, "early" stops one round early,
    "unclamped" prefetches t + G whatever n is."""
    grid, out = min(G, n), []
    for g in range(grid):
        held, counted, loaded, t = g, [], [g], g
        while (t + grid < n) if mutant == "early" else (t < n):
            nx = t + grid if t + grid < n or mutant == "unclamped" else t if reread else None
            counted.append(held)
            if nx is not None:
                loaded.append(nx)
                held = nx
            t += grid
        if mutant == "twice":
            counted.append(held)
        out.append((counted, loaded))
    return out


def walk_lab(G, n, order):
    """hamming_persist_lab<RUN, ORDER>: both orders clamp to `last`, the wave's last piece; order 2 keeps stream a one piece
    ahead of stream b (a[t + 2G] in flight with b[t + G]).  Returns per wave (pairs (a piece, b piece) counted, pieces loaded)."""
    grid, out = min(G, n), []
    for g in range(grid):
        last = g + (n - 1 - g) // grid * grid
        clamp = lambda p: p if p <= last else last  # noqa: E731
        counted, t = [], g
        if order == 2:
            va, va2, vb = g, clamp(g + grid), g
            loaded = [va, va2, vb]
            while t < n:
                counted.append((va, vb))
                va, va2, vb = va2, clamp(t + 2 * grid), clamp(t + grid)
                loaded += [va2, vb]
                t += grid
        else:
            va = vb = g
            loaded = [va, vb]
            while t < n:
                counted.append((va, vb))
                va = vb = clamp(t + grid)
                loaded += [va, vb]
                t += grid
        out.append((counted, loaded))
    return out


def _flat(waves, j):
    return np.fromiter(itertools.chain.from_iterable(w[j] for w in waves), dtype=np.int64)


def total(weights, waves):
    """what a reduction that walks like `waves` makes of per-piece counts `weights`"""
    return int(np.asarray(weights, dtype=np.int64)[_flat(waves, 0)].sum())


@pytest.mark.parametrize("G", [1, 2, 3, 64, 512, 1024])
def test_walk_counts_every_piece_once_and_loads_inside_the_buffer(G):
    for n in range(max(G - 1, 1), 3 * G + 3):
        # wave by wave the pieces g, g + grid, ...: every piece exactly once, and in the order of the loop's own index t (which
        # kmer_count uses to place a tile's k-mers)
        in_turn = np.argsort(np.arange(n) % min(G, n), kind="stable")
        for reread in (True, False):
            waves = walk(G, n, reread)
            assert len(waves) == min(G, n)
            assert np.array_equal(_flat(waves, 0), in_turn), (G, n, reread)
            loaded = _flat(waves, 1)
            assert loaded.min() >= 0 and loaded.max() < n, (G, n, reread)  # the prefetch reads real memory
        for order in (1, 2):
            waves = walk_lab(G, n, order)
            pairs = np.fromiter(itertools.chain.from_iterable(p for w in waves for p in w[0]), dtype=np.int64).reshape(-1, 2)
            assert np.array_equal(pairs[:, 0], in_turn) and np.array_equal(pairs[:, 1], in_turn), (G, n, order)  # a's piece t with b's piece t
            loaded = _flat(waves, 1)
            assert loaded.min() >= 0 and loaded.max() < n, (G, n, order)


def _assert_mutants_are_seen(weights, G):
    """With these per-piece counts the total tells the kernels' walk from its two wrong neighbours that stay inside the
    buffer.  The third, the unclamped prefetch, cannot move a total -- what the last iteration loads is never counted --
    which is why the bound on the loaded pieces is a check of its own: here the mutant must break it."""
    n = len(weights)
    truth = total(weights, walk(G, n))
    assert truth == int(np.sum(weights))
    assert total(weights, walk(G, n, mutant="twice")) != truth, (G, n)
    assert total(weights, walk(G, n, mutant="early")) != truth, (G, n)
    unclamped = walk(G, n, mutant="unclamped")
    assert _flat(unclamped, 1).max() >= n and total(weights, unclamped) == truth, (G, n)


# ---- inputs that tell pieces apart ----------------------------------------------------------------------------------------
def _spread(rng, counts, span):
    """counts[r] distinct offsets in [0, span) for every piece r, flat in piece order: an arithmetic progression mod span
    with an odd step (span is a power of two), started on the piece's first offset for r % 3 == 0 and on its last for
    r % 3 == 1.  Returns (piece of each offset, rank of each offset within its piece, offsets)."""
    n = counts.size
    assert span & (span - 1) == 0 and (n == 0 or counts.max() <= span)
    r = np.arange(n, dtype=np.int64)
    step = rng.integers(0, span // 2, n, dtype=np.int64) * 2 + 1
    first = np.where(r % 3 == 0, 0, np.where(r % 3 == 1, span - 1, rng.integers(0, span, n, dtype=np.int64)))
    piece = np.repeat(r, counts)
    rank = np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)
    return piece, rank, (first[piece] + rank * step[piece]) % span


def hamming_run_grid(pa, pb, n_len):
    """(head_words, n_runs) of cnt_hamming_dev for streams at addresses pa, pb: when both share their 16-B phase it peels
    words until `a` sits on a line (a 4-KiB page from 2^24 nt on), whole 8-KiB pieces follow; streams at different phases
    get no piece at all (hamming_generic takes everything)."""
    grain = 4096 if n_len >= H_PAGE_GRAIN_NT else 128
    head = ((-pa) % grain) // 8 if (pa ^ pb) & 15 == 0 else 0
    if head > n_len // 32:
        head = 0
    if (pa + 8 * head) & 15 or (pb + 8 * head) & 15:
        return 0, 0
    return head, (n_len // 32 - head) // H_RUN_WORDS


def hamming_len_for(pa, n_runs, tail_nt=0):
    """the length at which streams at address pa (both at that 16-B phase) get exactly n_runs pieces and tail_nt (< one piece)
    nucleotides behind them"""
    for grain in (128, 4096):
        n_len = 32 * (((-pa) % grain) // 8 + n_runs * H_RUN_WORDS) + tail_nt
        if (n_len >= H_PAGE_GRAIN_NT) == (grain == 4096):
            break
    assert hamming_run_grid(pa, pa, n_len)[1] == n_runs, (pa, n_runs, tail_nt)
    return n_len


def hamming_plan(pa, pb, n_len, seed):
    """The nucleotides in which b will differ from a: r + 1 of them in piece r of the run grid of (pa, pb, n_len), some on the
    first and last code of pieces, two in the head the launcher peels and two in the tail behind the last piece where those
    exist.  Returns (sorted positions, first nucleotide of the run grid, n_runs)."""
    rng = np.random.default_rng(seed)
    head, n_runs = hamming_run_grid(pa, pb, n_len)
    origin, end = 32 * head, 32 * (head + n_runs * H_RUN_WORDS)
    piece, _, off = _spread(rng, np.arange(n_runs, dtype=np.int64) + 1, H_RUN_NT)
    extra = [p for lo, hi in ((0, origin), (end, n_len)) if hi > lo for p in {lo, hi - 1}]
    pos = np.concatenate([origin + piece * H_RUN_NT + off, np.array(extra, dtype=np.int64)])
    return np.sort(pos), origin, n_runs


def hamming_weights(pos, origin, n_runs):
    """per-piece number of differing codes on the grid that starts at nucleotide `origin`, and the number outside it"""
    r = (pos - origin) // H_RUN_NT
    inside = (pos >= origin) & (r < n_runs)
    return np.bincount(r[inside], minlength=n_runs), int((~inside).sum())


def hamming_data(pos, n_len, seed):
    """(a, b): a random, b = a with the code at every position of pos changed; different garbage above n_len in both"""
    rng = np.random.default_rng(seed + 1)
    words = (n_len + 31) // 32
    a = rng.integers(0, 2**64, words, dtype=np.uint64)
    b = a.copy()
    flip = rng.integers(1, 4, pos.size, dtype=np.uint64) << (2 * (pos & 31)).astype(np.uint64)  # pos is sorted: so are the words
    uniq, starts = np.unique(pos >> 5, return_index=True)
    b[uniq] ^= np.bitwise_xor.reduceat(flip, starts)
    if n_len & 31:
        b[-1] ^= np.uint64(int(rng.integers(0, 2**62)) << 2 * (n_len & 31) & 0xFFFFFFFFFFFFFFFF | 1 << 2 * (n_len & 31))
    return a, b


def _assert_tells_pieces_apart(weights, n_runs):
    assert weights.size == n_runs and weights.min(initial=1) >= 1
    assert np.unique(weights).size == n_runs  # pairwise distinct


def _hamming_checked_plan(pa, pb, n_len, seed):
    """hamming_plan, held to the condition: positions distinct, piece r holds r + 1 of them.  Returns (pos, n_runs, expected)."""
    pos, origin, n_runs = hamming_plan(pa, pb, n_len, seed)
    assert np.unique(pos).size == pos.size and pos[0] >= 0 and pos[-1] < n_len
    weights, outside = hamming_weights(pos, origin, n_runs)
    _assert_tells_pieces_apart(weights, n_runs)
    assert np.array_equal(weights, np.arange(n_runs) + 1)
    return pos, n_runs, n_runs * (n_runs + 1) // 2 + outside


# the views of the page-offset test: `a` this many words past a 4-KiB boundary; b at the same 16-B phase, on the same page
# offset or another one; one b at another 16-B phase as the control that goes to hamming_generic whole
PAGE_LENS = [(1 << 24) - 32, 1 << 24, (1 << 24) + 32 * 8192 + 7]
PAGE_OFFSETS_WORDS = [1, 2, 17, 256, 511]
B_SHIFTS_WORDS = [0, 2, 256]
B_CONTROL_SHIFT_WORDS = 1
RAGGED_NT = 45


def _hamming_inputs(G):
    """(pa, pb, n_len) modulo the page of every product-build Hamming call of the GPU part on a grid of G"""
    for f in RUN_COUNTS.values():
        for tail in (0, RAGGED_NT):
            yield 0, 0, hamming_len_for(0, f(G), tail)
    for n_len in PAGE_LENS:
        for off in PAGE_OFFSETS_WORDS:
            for shift in B_SHIFTS_WORDS + [B_CONTROL_SHIFT_WORDS]:
                yield 8 * off, 8 * (off + shift), n_len
    yield 8, 8, 32 * (G + 1) * H_RUN_WORDS  # the head peel takes the (G+1)-th piece


@pytest.mark.parametrize("cus", MODEL_CUS)
def test_hamming_inputs_tell_pieces_apart(cus):
    G = grids(cus)["hamming"]
    seen = set()
    for pa, pb, n_len in _hamming_inputs(G):
        pos, n_runs, expected = _hamming_checked_plan(pa, pb, n_len, seed=n_len)
        assert expected == pos.size
        seen.add(n_runs)
        if n_runs:
            _assert_mutants_are_seen(np.arange(n_runs) + 1, G)
    assert {f(G) for f in RUN_COUNTS.values()} <= seen and 0 in seen  # 0: the control at unequal phases
    assert hamming_run_grid(8, 8, 32 * (G + 1) * H_RUN_WORDS)[1] == G
    # the lab orders' extra piece counts
    for n_runs in (1, 2):
        _hamming_checked_plan(0, 0, hamming_len_for(0, n_runs), seed=n_runs)


def test_hamming_head_rule_at_the_page_offsets():
    """what the page-offset views exercise: below 2^24 nt the head is the distance to a 128-B line, from 2^24 nt on to a 4-KiB
    page (up to 511 words through hamming_generic), whatever page offset b has as long as it shares a's 16-B phase"""
    for off in PAGE_OFFSETS_WORDS:
        for shift in B_SHIFTS_WORDS:
            assert hamming_run_grid(8 * off, 8 * (off + shift), PAGE_LENS[0]) == ((-off) % 16, ((PAGE_LENS[0] >> 5) - (-off) % 16) // H_RUN_WORDS)
            for n_len in PAGE_LENS[1:]:
                assert hamming_run_grid(8 * off, 8 * (off + shift), n_len) == (512 - off, ((n_len >> 5) - (512 - off)) // H_RUN_WORDS)
        for n_len in PAGE_LENS:
            assert hamming_run_grid(8 * off, 8 * (off + B_CONTROL_SHIFT_WORDS), n_len) == (0, 0)


def test_hamming_data_carries_the_plan(oracle):
    """the arrays really differ in the planned codes and nowhere else: piece by piece through the oracle, on a small grid"""
    for pa, tail in ((0, 0), (8, RAGGED_NT), (8 * 15, 7)):
        n_len = hamming_len_for(pa, 7, tail)
        pos, n_runs, expected = _hamming_checked_plan(pa, pa, n_len, seed=3)
        a, b = hamming_data(pos, n_len, seed=3)
        head = hamming_run_grid(pa, pa, n_len)[0]
        for r in range(n_runs):
            w = slice(head + r * H_RUN_WORDS, head + (r + 1) * H_RUN_WORDS)
            assert oracle.hamming(a[w], b[w], H_RUN_NT) == r + 1
        assert oracle.hamming(a, b, n_len) == expected
        if n_len & 31:
            assert (int(a[-1]) ^ int(b[-1])) >> (2 * (n_len & 31)) != 0  # garbage above len differs, and is not counted


def validate_run_grid(ptr, n_len):
    """(head bytes, n_runs) of cnt_validate_dev for a buffer at address ptr: bytes until the stream sits on a 128-B line (a
    4-KiB page from 4 MiB on) go to validate_generic, whole 16-KiB pieces follow"""
    grain = 4096 if n_len >= V_PAGE_GRAIN_BYTES else 128
    head = (-ptr) % grain
    if head > n_len:
        head = 0
    return head, (n_len - head) // V_RUN


def validate_len_for(ptr, n_runs, tail=0):
    for grain in (128, 4096):
        n_len = (-ptr) % grain + n_runs * V_RUN + tail
        if (n_len >= V_PAGE_GRAIN_BYTES) == (grain == 4096):
            break
    assert validate_run_grid(ptr, n_len)[1] == n_runs, (ptr, n_runs, tail)
    return n_len


OUTSIDE = np.frombuffer(b"X-.*" + bytes([0, 0x1F, 0x80, 0xFF]), dtype=np.uint8)  # outside every alphabet
N_OR_n = np.frombuffer(b"Nn", dtype=np.uint8)  # invalid unless allow_n
VALIDATE_PAGE_OFFSETS = [0, 1, 4095]
VALIDATE_TAIL = 300


def validate_plan(ptr, n_len, seed):
    """The bytes planted into valid ASCII: piece r of the run grid of (ptr, n_len) gets r + 1 bytes outside every alphabet and
    (r % 5) + 1 of N / n, so the strict count and the allow_n count both differ from piece to piece; some on the first and last
    byte of pieces; the head (first and last byte) and the tail (last byte, outside every alphabet) get theirs where they
    exist.  Returns (positions, bytes, head, n_runs)."""
    rng = np.random.default_rng(seed)
    head, n_runs = validate_run_grid(ptr, n_len)
    r = np.arange(n_runs, dtype=np.int64)
    outside = r + 1
    piece, rank, off = _spread(rng, outside + r % 5 + 1, V_RUN)
    byte = np.where(rank < outside[piece], OUTSIDE[rng.integers(0, OUTSIDE.size, piece.size)], N_OR_n[rng.integers(0, 2, piece.size)])
    end = head + n_runs * V_RUN
    extra = ([(0, OUTSIDE[0])] if head else []) + ([(head - 1, N_OR_n[0])] if head > 1 else []) + ([(n_len - 1, OUTSIDE[1])] if n_len > end else [])
    pos = np.concatenate([head + piece * V_RUN + off, np.array([p for p, _ in extra], dtype=np.int64)])
    byte = np.concatenate([byte, np.array([v for _, v in extra], dtype=np.uint8)]).astype(np.uint8)
    return pos, byte, head, n_runs


def _validate_checked_plan(ptr, n_len, seed):
    """validate_plan, held to the condition in both modes.  Returns (pos, byte, {allow_n: expected}, per-piece (strict, allow_n) counts)."""
    pos, byte, head, n_runs = validate_plan(ptr, n_len, seed)
    assert np.unique(pos).size == pos.size and pos.min() >= 0 and pos.max() < n_len
    is_n = np.isin(byte, N_OR_n)
    assert not np.isin(byte, np.frombuffer(b"ACGTUacgtu", dtype=np.uint8)).any()
    r = (pos - head) // V_RUN
    inside = (pos >= head) & (r < n_runs)
    strict = np.bincount(r[inside], minlength=n_runs)
    allow = np.bincount(r[inside & ~is_n], minlength=n_runs)
    _assert_tells_pieces_apart(strict, n_runs)
    _assert_tells_pieces_apart(allow, n_runs)
    i = np.arange(n_runs)
    assert np.array_equal(allow, i + 1) and np.array_equal(strict, i + 1 + i % 5 + 1)
    return pos, byte, {False: pos.size, True: int((~is_n).sum())}, (strict, allow)


def validate_data(pos, byte, n_len, seed):
    rng = np.random.default_rng(seed + 1)
    n = np.frombuffer(b"ACGTUacgtu", dtype=np.uint8)[rng.integers(0, 10, n_len, dtype=np.uint8)]
    n[pos] = byte
    return n


def _validate_inputs(G):
    """(page offset, n_len) of every validate call of the GPU part on a grid of G; the host tier stages into the library's own
    page-aligned scratch, which is offset 0"""
    for f in RUN_COUNTS.values():
        for off in VALIDATE_PAGE_OFFSETS:
            for tail in (0, VALIDATE_TAIL):
                yield off, validate_len_for(off, f(G), tail)


@pytest.mark.parametrize("cus", MODEL_CUS)
def test_validate_inputs_tell_pieces_apart(cus):
    G = grids(cus)["validate"]
    for off, n_len in _validate_inputs(G):
        _, _, expected, (strict, allow) = _validate_checked_plan(off, n_len, seed=n_len)
        assert expected[False] > expected[True] > 0
        if off == 1:  # the weights depend on n_runs alone
            _assert_mutants_are_seen(strict, G)
            _assert_mutants_are_seen(allow, G)


def test_validate_data_carries_the_plan(oracle):
    for off, tail in ((0, 0), (1, VALIDATE_TAIL), (4095, 0), (127, 5)):
        n_len = validate_len_for(off, 7, tail)
        pos, byte, expected, _ = _validate_checked_plan(off, n_len, seed=5)
        n = validate_data(pos, byte, n_len, seed=5)
        head = validate_run_grid(off, n_len)[0]
        for r in range(7):
            run = n[head + r * V_RUN : head + (r + 1) * V_RUN]
            assert (oracle.validate(run), oracle.validate(run, allow_n=True)) == (r + 1 + r % 5 + 1, r + 1)
        for allow in (False, True):
            assert oracle.validate(n, allow_n=allow) == expected[allow]


def kmer_tiles(n_len, k):
    """(m, words, n_tiles) of cnt_kmer_counts_dev"""
    m = n_len - k + 1
    return m, (n_len + 31) // 32, (m + TILE - 1) // TILE


def kmer_tile_is_fast(t, words):
    """kmer_count's load of tile t takes the 16-B loads iff the tile's 1025 words all exist"""
    return t * TILE_WORDS + TILE_WORDS + 1 <= words


# Case (c), the ragged last tile in round two.  One call cannot have both m = G * 32768 + 1 (then words = 1024 G + 1) and words
# = 1024 (G + 1), so these are three lengths, all with n_tiles = G + 1: the last tile with a single k-mer; words exactly
# (G + 1) * 1024, the last tile one word short of the 16-B path; and words one more, the last tile on the 16-B path (k >= 2).
RAGGED_TILE_LENS = {"one-kmer": lambda G, k: G * TILE + k, "words=1024(G+1)": lambda G, k: (G + 1) * TILE - 3,
                    "words=1024(G+1)+1": lambda G, k: (G + 1) * TILE + 1}
RAGGED_TILE_KS = [(7, False), (12, True)]  # the LDS limit forward, the last global k canonical
BOUNDARY_KS = [(3, False), (7, True), (8, True), (12, False)]  # the 256-replica table, the LDS limit, the first and last global k


@pytest.mark.parametrize("cus", MODEL_CUS)
def test_kmer_ragged_tile_lengths_sit_where_they_should(cus):
    G = grids(cus)["kmer"]
    for k, _ in RAGGED_TILE_KS:
        m, words, n_tiles = kmer_tiles(RAGGED_TILE_LENS["one-kmer"](G, k), k)
        assert (m, n_tiles) == (G * TILE + 1, G + 1) and kmer_tile_is_fast(G - 1, words) and not kmer_tile_is_fast(G, words)
        m, words, n_tiles = kmer_tiles(RAGGED_TILE_LENS["words=1024(G+1)"](G, k), k)
        assert (words, n_tiles) == ((G + 1) * TILE_WORDS, G + 1) and not kmer_tile_is_fast(G, words)
        m, words, n_tiles = kmer_tiles(RAGGED_TILE_LENS["words=1024(G+1)+1"](G, k), k)
        assert (words, n_tiles) == ((G + 1) * TILE_WORDS + 1, G + 1) and kmer_tile_is_fast(G, words) and m < (G + 1) * TILE
    for f in (RUN_COUNTS[c] for c in TILE_COUNTS):
        for k in range(1, 13):
            assert kmer_tiles(f(G) * TILE, k)[2] == f(G)  # the all-A lengths
        for k, _ in BOUNDARY_KS:
            assert kmer_tiles(f(G) * TILE - 77, k)[2] == f(G)  # the boundary-run lengths


# ---------------------------------------------------------------------------------------------------------------- GPU part
def _at_page_offset(torch, host, off_bytes):
    """a device copy of the numpy array `host` whose first byte lies off_bytes past a 4-KiB boundary, as a uint8 view"""
    raw = torch.empty(host.nbytes + 4096 + off_bytes, dtype=torch.uint8, device="cuda")
    lo = (-raw.data_ptr()) % 4096 + off_bytes
    view = raw[lo : lo + host.nbytes]
    view.copy_(torch.from_numpy(host.view(np.uint8)))
    assert (view.data_ptr() - off_bytes) % 4096 == 0  # from the address, not from the index
    return view


def _words_at(torch, host, off_words):
    return _at_page_offset(torch, host, 8 * off_words).view(torch.int64)


@gpu
def test_gpu_grids_of_this_device(capsys):
    """the G the other tests run at (shown with -s / in the captured output): every list of piece counts lies on both sides of it"""
    g = grids(_device_cus())
    with capsys.disabled():
        print("\npersistent grids on this device: %d CUs -> hamming G = %d, validate G = %d, kmer_count G = %d"
              % (_device_cus(), g["hamming"], g["validate"], g["kmer"]))
    assert g["hamming"] >= 2 and g["validate"] >= 4 and g["kmer"] >= 2


def _hamming_case(torch, oracle, n_runs, tail):
    """inputs with n_runs weighted pieces (+ tail nt) on pages; returns (da, db, a, b, n_len, expected)"""
    n_len = hamming_len_for(0, n_runs, tail)
    pos, got_runs, expected = _hamming_checked_plan(0, 0, n_len, seed=n_len)
    assert got_runs == n_runs
    a, b = hamming_data(pos, n_len, seed=n_len)
    assert oracle.hamming(a, b, n_len) == expected  # the closed-form sum of the weights is the oracle's value
    da, db = _words_at(torch, a, 0), _words_at(torch, b, 0)
    assert hamming_run_grid(da.data_ptr(), db.data_ptr(), n_len) == (0, n_runs)
    return da, db, a, b, n_len, expected


@gpu
@pytest.mark.parametrize("count", list(RUN_COUNTS))
def test_gpu_hamming_where_the_grid_wraps(oracle, count):
    import torch

    from cute_nucleotides_amd import packed_ops as po

    G = grids(_device_cus())["hamming"]
    n_runs = RUN_COUNTS[count](G)
    for tail in (0, RAGGED_NT):
        da, db, a, b, n_len, expected = _hamming_case(torch, oracle, n_runs, tail)
        got = int(po.hamming_dev(da, db, n_len).item())
        assert got == expected, (G, n_runs, tail, got - expected)
        got = po.hamming_hip(a, b, n_len)  # staged through the library's page-aligned scratch: the same grid
        assert got == expected, (G, n_runs, tail, got - expected)
        if count in ("G+1", "2G") and tail == 0:  # the calls ADD to the caller's counter
            acc = torch.zeros(1, dtype=torch.int64, device="cuda")
            po.hamming_dev(da, db, n_len, acc=acc)
            po.hamming_dev(da, db, n_len, acc=acc)
            assert int(acc.item()) == 2 * expected


@gpu
@pytest.mark.parametrize("n_len", PAGE_LENS)
def test_gpu_hamming_page_offsets_around_the_page_grain(oracle, n_len):
    """len on both sides of 2^24 nt, where the head grain goes from 128 B to 4096 B: `a` 1 .. 511 words past a page, so up to 511
    words go through hamming_generic and the pieces lie on the grid behind them; b at a's 16-B phase on the same page offset
    and on two others; and b at another phase, which sends the whole call to hamming_generic"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    for off in PAGE_OFFSETS_WORDS:
        pos, n_runs, expected = _hamming_checked_plan(8 * off, 8 * off, n_len, seed=n_len + off)
        a, b = hamming_data(pos, n_len, seed=n_len + off)
        assert oracle.hamming(a, b, n_len) == expected
        da = _words_at(torch, a, off)
        assert da.data_ptr() % 4096 == 8 * off
        for shift in B_SHIFTS_WORDS + [B_CONTROL_SHIFT_WORDS]:
            db = _words_at(torch, b, off + shift)
            grid = hamming_run_grid(da.data_ptr(), db.data_ptr(), n_len)
            if shift == B_CONTROL_SHIFT_WORDS:
                assert grid == (0, 0)
            else:
                assert grid == (((-off) % 16 if n_len < H_PAGE_GRAIN_NT else 512 - off), n_runs) and n_runs > 0
            got = int(po.hamming_dev(da, db, n_len).item())
            assert got == expected, (n_len, off, shift, got - expected)


@gpu
def test_gpu_hamming_head_peel_takes_a_piece(oracle):
    """(G + 1) pieces' worth of words one word past a page: the head peel leaves G whole pieces, one round exactly full, and the
    rest of the last piece goes to the tail kernel"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    G = grids(_device_cus())["hamming"]
    n_len = 32 * (G + 1) * H_RUN_WORDS
    pos, n_runs, expected = _hamming_checked_plan(8, 8, n_len, seed=11)
    assert (n_len // 32 // H_RUN_WORDS, n_runs) == (G + 1, G)
    a, b = hamming_data(pos, n_len, seed=11)
    assert oracle.hamming(a, b, n_len) == expected
    da, db = _words_at(torch, a, 1), _words_at(torch, b, 1)
    assert hamming_run_grid(da.data_ptr(), db.data_ptr(), n_len)[1] == G
    assert int(po.hamming_dev(da, db, n_len).item()) == expected


@gpu
@pytest.mark.parametrize("order", [1, 2])
def test_gpu_hamming_lab_orders_match_the_shipped_kernel(oracle, lab_build, order):
    """hamming_persist_lab<8, 1> (blocks) and <8, 2> (stream a one piece ahead, clamped to the wave's last piece), which
    bench/bench_packed_ops.py times against the shipped kernel: the same value as hamming_persist and the oracle at every piece
    count around the wrap, and at 1 and 2 pieces, where order 2's prologue already clamps"""
    import torch

    from cute_nucleotides_amd import devutil, packed_ops as po

    G = grids(_device_cus())["hamming"]
    counts = sorted({f(G) for f in RUN_COUNTS.values()} | {1, 2})
    try:
        for n_runs in counts:
            for tail in (0, RAGGED_NT):
                da, db, a, b, n_len, expected = _hamming_case(torch, oracle, n_runs, tail)
                devutil.set_tuning("hamming_order", 0)
                shipped = int(po.hamming_dev(da, db, n_len).item())
                devutil.set_tuning("hamming_order", order)
                assert devutil.get_tuning("hamming_order") == order
                got = int(po.hamming_dev(da, db, n_len).item())
                assert got == shipped == expected, (order, G, n_runs, tail, got - expected, shipped - expected)
    finally:
        devutil.set_tuning("hamming_order", 0)


@gpu
@pytest.mark.parametrize("where", ["dev+0", "dev+1", "dev+4095", "host"])
@pytest.mark.parametrize("count", list(RUN_COUNTS))
def test_gpu_validate_where_the_grid_wraps(oracle, count, where):
    """the buffer 0, 1 and 4095 bytes past a page (heads of 0, 4095 and 1 bytes through validate_generic), the plants on the
    grid each offset produces; with and without a ragged tail of 300 bytes that holds one plant; both modes"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    G = grids(_device_cus())["validate"]
    n_runs = RUN_COUNTS[count](G)
    off = 0 if where == "host" else int(where[4:])
    n_len = validate_len_for(off, n_runs, VALIDATE_TAIL)
    body = validate_len_for(off, n_runs)
    assert body == n_len - VALIDATE_TAIL
    pos, byte, expected, _ = _validate_checked_plan(off, n_len, seed=n_len)
    in_tail = int((pos >= body).sum())
    assert in_tail == 1 and validate_run_grid(off, body) == validate_run_grid(off, n_len)  # one plant in the tail, one grid for both lengths
    n = validate_data(pos, byte, n_len, seed=n_len)
    d = None if where == "host" else _at_page_offset(torch, n, off)
    for allow in (False, True):
        want = oracle.validate(n, allow_n=allow)
        assert want == expected[allow]
        for m, want_m in ((n_len, want), (body, want - in_tail)):  # a count: the oracle's value of the body is the whole's minus the tail's
            if d is None:
                got = po.validate_hip(n[:m], allow_n=allow)
            else:
                assert validate_run_grid(d.data_ptr(), m) == ((-off) % 4096 if m >= V_PAGE_GRAIN_BYTES else (-off) % 128, n_runs)
                got = int(po.validate_dev(d[:m], allow_n=allow).item())
            assert got == want_m, (G, n_runs, where, allow, m - body, got - want_m)
    assert oracle.validate(n[body:]) == oracle.validate(n[body:], allow_n=True) == in_tail


def _counts_dev(po, d_bits, n_len, k, canonical):
    return po.kmer_counts_dev(d_bits, n_len, k, canonical=canonical).cpu().numpy().view(np.uint64)


@gpu
@pytest.mark.parametrize("count", TILE_COUNTS)
def test_gpu_kmer_counts_all_a_where_the_grid_wraps(count):
    """all-A, every k, both modes, both tiers: counts[0] = len - k + 1 and every other bin zero, whichever tile a workgroup
    takes in its second and third round (a dropped or doubled tile moves counts[0] by up to 32768)"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    G = grids(_device_cus())["kmer"]
    n_tiles = RUN_COUNTS[count](G)
    n_len = n_tiles * TILE
    host = np.zeros(n_len // 32, dtype=np.uint64)
    bits = torch.zeros(n_len // 32, dtype=torch.int64, device="cuda")
    for k in range(1, 13):
        assert kmer_tiles(n_len, k)[2] == n_tiles
        for canonical in (False, True):
            got_dev, got_host = _counts_dev(po, bits, n_len, k, canonical), po.kmer_counts_hip(host, n_len, k, canonical=canonical)
            for tier, got in (("device", got_dev), ("host", got_host)):
                assert int(got[0]) == n_len - k + 1 and not got[1:].any(), (G, n_tiles, k, canonical, tier, int(got[0]) - (n_len - k + 1))


def _reference(oracle, words, n_len, k, canonical):
    return np.bincount(oracle.kmers(words, n_len, k, canonical).astype(np.int64), minlength=4**k).astype(np.uint64)


@gpu
@pytest.mark.parametrize("count", ["G+1", "2G+1"])
def test_gpu_kmer_counts_with_a_run_across_the_round_boundary(oracle, count):
    """random sequence (no two tiles hold the same spectrum, so a tile counted for another shows) with a poly-T run laid across
    the start of tile G, the first tile any workgroup takes in its second round (and of tile 2G); one reference per k, shared by
    both tiers"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    G = grids(_device_cus())["kmer"]
    n_tiles = RUN_COUNTS[count](G)
    n_len = n_tiles * TILE - 77
    s = oracle.fill_random_acgt(n_len, seed=900 + n_tiles)
    for edge in (G * TILE, 2 * G * TILE):
        if edge < n_len:
            s[edge - 1500 : edge + 700] = ord("T")
    w = oracle.n_to_bits_lut(s)
    d = torch.from_numpy(w.view(np.int64)).cuda()
    for k, canonical in BOUNDARY_KS:
        assert kmer_tiles(n_len, k)[2] == n_tiles
        want = _reference(oracle, w, n_len, k, canonical)
        assert int(want.sum()) == n_len - k + 1
        assert np.array_equal(_counts_dev(po, d, n_len, k, canonical), want), (G, n_tiles, k, canonical, "device")
        assert np.array_equal(po.kmer_counts_hip(w, n_len, k, canonical=canonical), want), (G, n_tiles, k, canonical, "host")


@gpu
@pytest.mark.parametrize("shape", list(RAGGED_TILE_LENS))
def test_gpu_kmer_counts_ragged_last_tile_in_round_two(oracle, shape):
    """n_tiles = G + 1: workgroup 0's second tile is the guarded ragged one -- holding one k-mer, or one word short of the 16-B
    path, or just on it; random garbage above len and in a word past it; the input at both 8-B phases of a 16-B line"""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    G = grids(_device_cus())["kmer"]
    rng = np.random.default_rng(31)
    for k, canonical in RAGGED_TILE_KS:
        n_len = RAGGED_TILE_LENS[shape](G, k)
        m, nw, n_tiles = kmer_tiles(n_len, k)
        assert n_tiles == G + 1
        clean = oracle.n_to_bits_lut(oracle.fill_random_acgt(n_len, seed=n_len + k))
        dirty = np.concatenate([clean, rng.integers(0, 2**64, 1, dtype=np.uint64)])
        if n_len & 31:
            dirty[nw - 1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(2 * (n_len & 31))
        want = _reference(oracle, clean, n_len, k, canonical)
        assert int(want.sum()) == m
        assert np.array_equal(po.kmer_counts_hip(dirty, n_len, k, canonical=canonical), want), (G, shape, k, "host")
        for phase in (0, 1):
            view = _words_at(torch, dirty, phase)
            assert view.data_ptr() % 16 == 8 * phase
            assert np.array_equal(_counts_dev(po, view, n_len, k, canonical), want), (G, shape, k, phase)
