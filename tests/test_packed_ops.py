"""Packed-domain operations: Hamming distance, complement, reverse complement,
validation.  These are NOT in the reference (parity unpinned): the CPU part pins the oracle's
scalar definitions against plain-Python/ASCII-level definitions, the GPU part compares the
HIP kernels with the oracle bit for bit and checks algebraic properties at large sizes."""
import time

import numpy as np
import pytest

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _ascii(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]


@pytest.mark.parametrize("n_len", [0, 1, 5, 31, 32, 33, 64, 100, 1000, 4099])
def test_oracle_definitions_against_ascii_level_semantics(oracle, n_len):
    rng = np.random.default_rng(n_len)
    a, b = _ascii(rng, n_len), _ascii(rng, n_len)
    pa, pb = oracle.n_to_bits_lut(a), oracle.n_to_bits_lut(b)
    assert oracle.hamming(pa, pb, n_len) == int((a != b).sum())
    comp = oracle.complement(pa, n_len)
    assert bytes(oracle.bits_to_n_lut(comp, n_len)) == bytes(a).translate(COMP)
    rc = oracle.reverse_complement(pa, n_len)
    assert bytes(oracle.bits_to_n_lut(rc, n_len)) == bytes(a).translate(COMP)[::-1]
    # unused high bits stay zero, like every encoder's output
    if n_len & 31:
        assert int(comp[-1]) >> (2 * (n_len & 31)) == 0 and int(rc[-1]) >> (2 * (n_len & 31)) == 0
    # garbage beyond len in the inputs is ignored
    if n_len & 31:
        pa2 = pa.copy()
        pa2[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(2 * (n_len & 31))
        assert oracle.hamming(pa2, pb, n_len) == oracle.hamming(pa, pb, n_len)
        assert np.array_equal(oracle.complement(pa2, n_len), comp)
        assert np.array_equal(oracle.reverse_complement(pa2, n_len), rc)


def test_oracle_validate():
    from oracle import cnt_oracle as orc

    allb = np.arange(256, dtype=np.uint8)
    assert orc.validate(allb) == 256 - 10
    assert orc.validate(allb, allow_n=True) == 256 - 12
    assert orc.validate(b"ACGTUacgtu" * 100) == 0
    assert orc.validate(b"ACGTN") == 1 and orc.validate(b"ACGTN", allow_n=True) == 0
    assert orc.validate(b"") == 0


# ---------------------------------------------------------------------------- GPU part
gpu = pytest.mark.gpu

SIZES = [0, 1, 5, 31, 32, 33, 63, 64, 65, 1000, 4099, 32 * 8192, 32 * 8192 + 7, (1 << 22) + 13, 3 * (1 << 21) + 64]


@pytest.fixture(params=[1, 0], ids=["persistent", "tiles+second-pass"])
def reduce_form(request):
    """both forms of the reductions: one launch of persistent waves (shipped: the product build, no knob) and round 1's
    tiles + stream-ordered scratch + second pass (lab build only, tuning key reduce_persistent)"""
    if request.param == 1:
        yield 1
        return
    request.getfixturevalue("lab_build")
    from cute_nucleotides_amd import devutil

    devutil.set_tuning("reduce_persistent", 0)
    yield 0
    devutil.set_tuning("reduce_persistent", 1)


@gpu
@pytest.mark.parametrize("n_len", SIZES)
def test_gpu_ops_match_oracle(oracle, n_len, reduce_form):
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(n_len + 3)
    words = (n_len + 31) // 32
    a = rng.integers(0, 2**64, words, dtype=np.uint64)  # includes garbage beyond len in the last word
    b = a.copy()
    flip = rng.integers(0, 2**64, words, dtype=np.uint64) & rng.integers(0, 2**64, words, dtype=np.uint64)
    b ^= flip
    assert po.hamming_hip(a, b, n_len) == oracle.hamming(a, b, n_len)
    assert np.array_equal(po.complement_hip(a, n_len), oracle.complement(a, n_len))
    assert np.array_equal(po.reverse_complement_hip(a, n_len), oracle.reverse_complement(a, n_len))
    if words:
        da, db = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(b.view(np.int64)).cuda()
        assert int(po.hamming_dev(da, db, n_len).item()) == oracle.hamming(a, b, n_len)
        assert np.array_equal(po.complement_dev(da, n_len).cpu().numpy().view(np.uint64), oracle.complement(a, n_len))
        assert np.array_equal(po.reverse_complement_dev(da, n_len).cpu().numpy().view(np.uint64), oracle.reverse_complement(a, n_len))
        # unaligned (8-B but not 16-B aligned) device pointers take the generic path
        if words > 3:
            m = (words - 1) * 32 if n_len == words * 32 else n_len - 32
            assert int(po.hamming_dev(da[1:], db[1:], m).item()) == oracle.hamming(a[1:], b[1:], m)
            assert np.array_equal(po.complement_dev(da[1:], m).cpu().numpy().view(np.uint64), oracle.complement(a[1:], m))


@gpu
def test_gpu_validate(oracle, reduce_form):
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(1)
    for n_len in (0, 1, 15, 16, 17, 65536, 65536 * 3 + 5, (1 << 22) + 3):
        n = rng.integers(0, 256, n_len, dtype=np.uint8)
        for allow in (False, True):
            assert po.validate_hip(n, allow_n=allow) == oracle.validate(n, allow_n=allow)
            if n_len:
                d = torch.from_numpy(n).cuda()
                assert int(po.validate_dev(d, allow_n=allow).item()) == oracle.validate(n, allow_n=allow)
                if n_len > 1:
                    assert int(po.validate_dev(d[1:], allow_n=allow).item()) == oracle.validate(n[1:], allow_n=allow)
        good = np.frombuffer(b"ACGTUacgtu", dtype=np.uint8)[rng.integers(0, 10, n_len)]
        assert po.validate_hip(good) == 0


@gpu
def test_gpu_ops_pointer_phases(oracle, reduce_form):
    """Word pointers at every 8-B phase of a 128-B line (equal and unequal phases of the two
    streams), ASCII pointers at odd bytes: heads are peeled, results and guard words unchanged."""
    import torch

    from cute_nucleotides_amd import packed_ops as po

    rng = np.random.default_rng(9)
    words = 3 * 8192 + 40
    a = rng.integers(0, 2**64, words + 40, dtype=np.uint64)
    b = a ^ (rng.integers(0, 2**64, words + 40, dtype=np.uint64) & rng.integers(0, 2**64, words + 40, dtype=np.uint64))
    da, db = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(b.view(np.int64)).cuda()
    obuf = torch.empty(words + 64, dtype=torch.int64, device="cuda")
    for pa in (0, 1, 2, 3, 7, 8, 15, 16, 17):
        for pb in (pa, pa + 1, pa + 2, 0):
            for n_len in (words * 32, words * 32 - 45, 64 * 32 + 3):
                w = (n_len + 31) // 32
                got = int(po.hamming_dev(da[pa : pa + w], db[pb : pb + w], n_len).item())
                assert got == oracle.hamming(a[pa : pa + w], b[pb : pb + w], n_len), (pa, pb, n_len)
                obuf.fill_(-1)
                po.complement_dev(da[pa : pa + w], n_len, out=obuf[8 + pb : 8 + pb + w])
                o = obuf.cpu().numpy()
                assert (o[: 8 + pb] == -1).all() and (o[8 + pb + w :] == -1).all()
                assert np.array_equal(o[8 + pb : 8 + pb + w].view(np.uint64), oracle.complement(a[pa : pa + w], n_len)), (pa, pb, n_len)
    # reverse complement: output phase x every window phase (len % 32) x tile-count boundaries
    for po_ in (0, 1, 2, 5, 15, 16):
        for pi_ in (0, 1):
            for n_len in [512 * 32 * 2 + k for k in (0, 1, 5, 31, 32, 33)] + [512 * 32 + 16 * 32 - 1, 512 * 32 + 15 * 32 + 1, words * 32 - 7, 40 * 32]:
                w = (n_len + 31) // 32
                obuf.fill_(-1)
                po.reverse_complement_dev(da[pi_ : pi_ + w], n_len, out=obuf[8 + po_ : 8 + po_ + w])
                o = obuf.cpu().numpy()
                assert (o[: 8 + po_] == -1).all() and (o[8 + po_ + w :] == -1).all()
                assert np.array_equal(o[8 + po_ : 8 + po_ + w].view(np.uint64), oracle.reverse_complement(a[pi_ : pi_ + w], n_len)), (po_, pi_, n_len)
    n = rng.integers(0, 256, 5 * 65536 + 300, dtype=np.uint8)
    d = torch.from_numpy(n).cuda()
    for off in (0, 1, 7, 16, 100, 127, 128, 129):
        for n_len in (n.size - off, 65536 + 127, 65536 + 128, 200):
            for allow in (False, True):
                assert int(po.validate_dev(d[off : off + n_len], allow_n=allow).item()) == oracle.validate(n[off : off + n_len], allow_n=allow)


@gpu
def test_gpu_large_properties(oracle):
    """2^32 nt: rc(rc(x)) == x, complement is an involution, hamming(x, complement(x)) == len,
    hamming(x, x) == 0, and encode(valid ASCII) validates clean."""
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import devutil, packed_ops as po

    n_len = (1 << 32) + 77
    d = torch.empty(n_len, dtype=torch.uint8, device="cuda")
    devutil.fill_random_acgt(d, 5)
    assert int(po.validate_dev(d).item()) == 0
    d[12345] = ord("N")
    d[n_len - 1] = 0
    assert int(po.validate_dev(d).item()) == 2 and int(po.validate_dev(d, allow_n=True).item()) == 1
    devutil.fill_random_acgt(d, 5)
    x = cn.n_to_bits_dev(d)
    c = po.complement_dev(x, n_len)
    assert int(po.hamming_dev(x, x, n_len).item()) == 0
    assert int(po.hamming_dev(x, c, n_len).item()) == n_len
    assert devutil.count_mismatch(po.complement_dev(c, n_len), x) == 0
    rc = po.reverse_complement_dev(x, n_len)
    assert devutil.count_mismatch(po.reverse_complement_dev(rc, n_len), x) == 0
    # the head of rc is the complement of the reversed tail of the ASCII
    tail = d[n_len - 1000 :].cpu().numpy()
    head = cn.bits_to_n_dev(rc, 1000).cpu().numpy()
    assert bytes(head) == bytes(tail).translate(COMP)[::-1]
    # the reductions above took their scratch from the stream-ordered allocator; none fell back to the slow path
    assert devutil.get_tuning("reduce_fallbacks") == 0


VALIDATE_RUN = 16 << 10  # bytes per run of validate's persistent waves (hip/packed_ops_kernels.hpp kValidateRunKiB)


def _large_validate_plants(n_len, seed=4242):
    """(positions, bytes) planted for validate into a page-aligned buffer of n_len bytes.  The runs of the buffer are
    [16 Ki r, 16 Ki (r+1)); those of the buffer from its byte 1 on start at byte 4096.  Region r gets 1..64 plants in
    [16 Ki r, 16 Ki r + 4096) and, drawn independently, 1..64 in [16 Ki r + 4096, 16 Ki (r+1)): every run of both grids
    holds plants, and their number varies from run to run (a dropped run and one counted twice change the total unless
    the two hold the same count).  A few more sit on run boundaries +-1, at the edges of the shifted head and on the last
    byte.  The bytes mix N / n with bytes outside every alphabet."""
    rng = np.random.default_rng(seed)
    R = n_len // VALIDATE_RUN
    base = np.arange(R, dtype=np.int64) * VALIDATE_RUN
    k_lo, k_hi = rng.integers(1, 65, R), rng.integers(1, 65, R)
    lo = np.repeat(base, k_lo) + rng.integers(0, 4096, int(k_lo.sum()))
    hi = np.repeat(base, k_hi) + rng.integers(4096, VALIDATE_RUN, int(k_hi.sum()))
    edges = np.concatenate([(b[:, None] + np.array([-1, 0, 1])).ravel() for b in (base[1::997], base[1::991] + 4096)] + [np.array([1, 4095, 4096, n_len - 1])])
    pos = np.unique(np.concatenate([lo, hi, edges]))
    pos = pos[(pos >= 0) & (pos < n_len)]
    alphabet = np.frombuffer(b"NnX-" + bytes([0, 0x80, 0xFF]), dtype=np.uint8)
    return pos, alphabet[rng.integers(0, alphabet.size, pos.size)]


def test_large_validate_plant_layout_tells_runs_apart():
    """the plants of test_gpu_large_ops_match_the_oracle_in_full, on the CPU: every run of both grids (the page-aligned
    buffer and the same buffer from byte 1 on) holds plants in both modes' strict count, and two runs almost never hold
    the same (strict, allow_n) pair of counts -- so dropping one run while counting another twice moves a total"""
    n_len = (1 << 32) + 77
    pos, bad = _large_validate_plants(n_len)
    is_n = (bad == ord("N")) | (bad == ord("n"))
    for origin in (0, 4096):
        n_runs = (n_len - origin) // VALIDATE_RUN

        def per_run(p):
            r = (p[p >= origin] - origin) // VALIDATE_RUN
            return np.bincount(r[r < n_runs], minlength=n_runs)

        strict, allow = per_run(pos), per_run(pos[~is_n])
        assert strict.min() >= 2, origin
        _, same_strict = np.unique(strict, return_counts=True)
        _, same_pair = np.unique(strict * 4096 + allow, return_counts=True)
        p_strict = float(((same_strict / n_runs) ** 2).sum())  # chance that two random runs share the strict count
        p_pair = float(((same_pair / n_runs) ** 2).sum())
        assert p_strict < 0.02 and p_pair < 0.002, (origin, p_strict, p_pair)


@gpu
def test_gpu_large_ops_match_the_oracle_in_full(oracle, fullsize):
    """2^32 + 77 nt, every output compared with the oracle's whole-stream value (the properties above cannot see a
    mistake that is consistent with itself: a mirrored index that is its own inverse, a dropped reduction run counted
    twice by another): complement and reverse complement by full-length checksum, hamming against a second stream,
    validate with plants in every 16-KiB run of both run grids (input on the page, and one byte off it) whose number
    differs from run to run, so that a dropped run and a run counted twice do not cancel, N and bytes outside every
    alphabet mixed so the two modes differ.  Then the same off the 16-B grid: streams at different
    phases (hamming_generic over everything), complement from word phase 1 (complement_generic), reverse complement
    into word phase 1, validate of d[1:] (head peel, runs at a shifted base).  Each check is shown to see one changed
    word or byte that nothing sampled covers."""
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import devutil, packed_ops as po
    from stream_checks import assert_mutation_seen, check_hamming, check_validate, check_words

    n_len = (1 << 32) + 77
    W = (n_len + 31) // 32
    buf = torch.empty(n_len + 4096, dtype=torch.uint8, device="cuda")
    d = buf[(-buf.data_ptr()) % 4096 :][:n_len]  # on a page: validate's runs of d and of d[1:] then lie on different grids
    devutil.fill_random_acgt(d, 6)
    y = cn.n_to_bits_dev(d)
    devutil.fill_random_acgt(d, 5)
    x = cn.n_to_bits_dev(d)
    c = po.complement_dev(x, n_len)
    want_c = check_words(c, "complement", 5, n_len, label="complement", record=fullsize)
    assert_mutation_seen(c, W // 2 + 12345, want_c)
    del c
    rc = po.reverse_complement_dev(x, n_len)
    want_rc = check_words(rc, "reverse_complement", 5, n_len, label="reverse complement", record=fullsize)
    assert_mutation_seen(rc, W // 3 + 54321, want_rc)
    del rc
    want_h = check_hamming(x, y, n_len, 5, 6)
    i_m = W // 5 + 777  # one word of y made equal to x's: distance of that word drops to 0
    saved = y[i_m : i_m + 1].clone()
    y[i_m : i_m + 1].copy_(x[i_m : i_m + 1])
    assert int(po.hamming_dev(x, y, n_len).item()) != want_h
    y[i_m : i_m + 1].copy_(saved)
    assert int(po.hamming_dev(x, y, n_len).item()) == want_h

    # off the 16-B grid: w whole words from word 1 of x (nt 32 on), against words 0.. of y
    w = n_len // 32 - 1
    check_hamming(x[1 : 1 + w], y[0:w], 32 * w, 5, 6, first_nt_a=32, first_nt_b=0, label="hamming at different phases")
    del y
    cg = po.complement_dev(x[1 : 1 + w], 32 * w, out=torch.empty(w, dtype=torch.int64, device="cuda"))
    check_words(cg, "complement", 5, 32 * w, first_nt=32, label="complement from word phase 1", record=fullsize)
    del cg
    obuf = torch.full((W + 2,), -1, dtype=torch.int64, device="cuda")
    po.reverse_complement_dev(x, n_len, out=obuf[1 : 1 + W])
    assert int(obuf[0].item()) == -1 and int(obuf[W + 1].item()) == -1
    check_words(obuf[1 : 1 + W], "reverse_complement", 5, n_len, label="reverse complement into word phase 1", want=want_rc)
    del obuf, x

    # validate: d is on a page, so its runs are [16 Ki r, 16 Ki (r+1)); d[1:] peels 4095 head bytes and runs from d's
    # byte 4096 on.  Every run of both grids holds plants, and their counts differ from run to run (the layout is pinned on
    # the CPU by test_large_validate_plant_layout_tells_runs_apart).
    pos, bad = _large_validate_plants(n_len)
    n_bad_n = int(((bad == ord("N")) | (bad == ord("n"))).sum())
    assert 0 < n_bad_n < pos.size
    d[torch.from_numpy(pos).cuda()] = torch.from_numpy(bad).cuda()
    plants = np.stack([pos, bad.astype(np.int64)], axis=1)
    t0 = time.perf_counter()
    for allow in (False, True):
        want_v = check_validate(d, 5, n_len, plants=plants, allow_n=allow)
        assert want_v == pos.size - (n_bad_n if allow else 0)
        # d[1:]: the buffer filled at nt 0, seen from nt 1; plants shift by one, the one at byte 0 (if any) drops out
        sh = plants[plants[:, 0] >= 1] - np.array([1, 0])
        check_validate(d[1:], 5, n_len - 1, first_nt=1, plants=sh, allow_n=allow, label="validate of d[1:]")
    fullsize(32, (time.perf_counter() - t0) * 1e3, check="full-length oracle: validate, %d plants" % pos.size)
    p_m = int((n_len // VALIDATE_RUN) // 3 * VALIDATE_RUN + 4000)
    while pos[np.searchsorted(pos, p_m)] == p_m:  # a byte no plant took
        p_m += 1
    orig = int(d[p_m].item())
    d[p_m] = ord("X")
    assert int(po.validate_dev(d).item()) == pos.size + 1
    d[p_m] = orig
    assert int(po.validate_dev(d).item()) == pos.size


@gpu
def test_reductions_are_graph_capturable_and_accumulate(oracle):
    """Since round 2 hamming / validate neither synchronise nor allocate (one launch of persistent waves): a whole
    encode -> hamming -> validate chain records into a HIP graph and replays on new buffer contents; the counters are
    the caller's and the calls ADD to them (two calls into one counter = the sum)."""
    import torch

    import cute_nucleotides_amd as cn
    from cute_nucleotides_amd import packed_ops as po

    n_len = (1 << 21) + 4099  # tiles' worth of persistent pieces plus a ragged tail and a word tail
    rng = np.random.default_rng(9)
    d_a = torch.zeros(n_len, dtype=torch.uint8, device="cuda")
    d_b = torch.zeros(n_len, dtype=torch.uint8, device="cuda")
    p_a = torch.zeros((n_len + 31) // 32, dtype=torch.int64, device="cuda")
    p_b = torch.zeros_like(p_a)
    ham = torch.zeros(1, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")

    def chain():
        ham.zero_()
        bad.zero_()
        cn.n_to_bits_dev(d_a, out=p_a)
        cn.n_to_bits_dev(d_b, out=p_b)
        po.hamming_dev(p_a, p_b, n_len, acc=ham)
        po.validate_dev(d_a, acc=bad)
        po.validate_dev(d_b, acc=bad)  # accumulates into the same counter

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain()  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for seed in (1, 2, 3):
        a = _ascii(rng, n_len)
        b = _ascii(rng, n_len)
        b[rng.integers(0, n_len, 50)] = ord("N")
        a[7] = 0
        d_a.copy_(torch.from_numpy(a))
        d_b.copy_(torch.from_numpy(b))
        g.replay()
        torch.cuda.synchronize()
        # expected values from the oracle's definitions on what the encoder makes of the bytes
        pa, pb = p_a.cpu().numpy().view(np.uint64), p_b.cpu().numpy().view(np.uint64)
        assert int(ham.item()) == oracle.hamming(pa, pb, n_len), seed
        assert int(bad.item()) == oracle.validate(a) + oracle.validate(b), seed
        assert oracle.validate(a) >= 1 and oracle.validate(b) >= 1
    with pytest.raises(ValueError):
        po.hamming_dev(p_a, p_b, n_len, acc=torch.zeros(1, dtype=torch.int32, device="cuda"))
