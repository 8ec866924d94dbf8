"""The oracle's whole-stream expected values (oracle/cnt_oracle.py stream_*), which the full-size GPU tests compare whole
outputs against: each equals the direct oracle call on the concatenated input, at ragged lengths, at a non-zero start,
with dozens of forced tiny chunks, with plants on chunk boundaries and on the last nt, and for any worker count; and the
checksum they add up sees a swapped pair of words or one flipped bit."""
import numpy as np
import pytest

ACGT_KINDS = ("encode", "complement", "reverse_complement")


def _direct(oracle, kind, seed, n_len, first_nt=0, plants=()):
    """the oracle's output words for the whole stream, in one call on the concatenated input"""
    five = kind == "encode5"
    n = (oracle.fill_random_acgtn if five else oracle.fill_random_acgt)(n_len, seed, first_nt=first_nt)
    for pos, byte in plants:
        n[pos] = byte
    if five:
        return oracle.n_to_bits2_lut(n)
    x = oracle.n_to_bits_lut(n)
    if kind == "complement":
        return oracle.complement(x, n_len)
    if kind == "reverse_complement":
        return oracle.reverse_complement(x, n_len)
    return x


def _check_kind(oracle, kind, seed, n_len, first_nt=0, plants=(), chunk_nt=None, workers=None):
    grain = 27 if kind == "encode5" else 32
    want = _direct(oracle, kind, seed, n_len, first_nt, plants)
    fw = first_nt // grain
    got = oracle.stream_checksum(kind, seed, n_len, first_nt=first_nt, plants=plants, chunk_nt=chunk_nt, workers=workers)
    assert got == oracle.checksum_words(want, first_word=fw), (kind, n_len, first_nt, chunk_nt)
    # per chunk: the checksums of the direct words' slices at the same word boundaries
    k = (chunk_nt or oracle.STREAM_CHUNK_NT) // grain
    per = oracle.stream_checksum(kind, seed, n_len, first_nt=first_nt, plants=plants, per_chunk=True, chunk_nt=chunk_nt, workers=workers)
    assert per == [oracle.checksum_words(want[c * k : (c + 1) * k], first_word=fw + c * k) for c in range(len(per))]
    assert len(per) == max(1, -(-want.size // k)) or n_len == 0
    assert sum(per) % (1 << 64) == got


@pytest.mark.parametrize("kind", ACGT_KINDS)
@pytest.mark.parametrize("n_len", [0, 1, 31, 32, 33, 32 * 40, 32 * 40 + 1, 32 * 40 + 17, 32 * 40 + 31, 100003, (1 << 20) + 5])
def test_stream_checksum_equals_the_direct_oracle_call(oracle, kind, n_len):
    _check_kind(oracle, kind, 0x5EED, n_len)
    _check_kind(oracle, kind, 0x5EED, n_len, chunk_nt=32 * 7)  # dozens of chunks (and more) at every length above
    _check_kind(oracle, kind, 17, n_len, first_nt=32 * 12345, chunk_nt=32 * 100)


@pytest.mark.parametrize("n_len", [0, 1, 26, 27, 28, 27 * 50, 27 * 50 + 1, 27 * 50 + 26, 100003, 27 * 40000 + 13])
def test_stream_checksum_encode5_equals_the_direct_oracle_call(oracle, n_len):
    _check_kind(oracle, "encode5", 31, n_len)
    _check_kind(oracle, "encode5", 31, n_len, chunk_nt=27 * 5)
    _check_kind(oracle, "encode5", 31, n_len, first_nt=27 * 999, chunk_nt=1000)  # rounded down to 999 = 37 words


@pytest.mark.parametrize("l_mod", [0, 1, 31, 17])
def test_stream_reverse_complement_at_every_kind_of_ragged_end(oracle, l_mod):
    """output chunk c needs input nt [L - s - K, L - s), off the generator's word grid when L % 32 != 0"""
    for n_len in (32 * 64 + l_mod, 32 * 1000 + l_mod):
        for chunk_nt in (32, 32 * 3, 32 * 64, None):
            _check_kind(oracle, "reverse_complement", 9, n_len, first_nt=32 * 7, chunk_nt=chunk_nt)


def test_plants_on_chunk_boundaries_and_on_the_last_nt(oracle):
    n_len = 32 * 50 * 10 + 13
    k = 32 * 50
    plants = [(0, ord("N")), (k - 1, 0), (k, ord("x")), (k + 1, 0xFF), (3 * k - 1, ord("n")), (3 * k, ord("-")),
              (7 * k + 5, ord("U")), (n_len - 1, 0)]
    for kind in ACGT_KINDS:
        _check_kind(oracle, kind, 3, n_len, plants=plants, chunk_nt=k)
        _check_kind(oracle, kind, 3, n_len, first_nt=32 * 5, plants=plants, chunk_nt=k)
    n5 = 27 * 300 + 8
    k5 = 27 * 30
    plants5 = [(0, 0), (k5 - 1, ord("X")), (k5, ord("z")), (4 * k5 + 1, 0x80), (n5 - 1, ord("?"))]
    _check_kind(oracle, "encode5", 4, n5, plants=plants5, chunk_nt=k5)
    # plants given as an array, and unsorted, give the same value
    arr = np.array(plants[::-1], dtype=np.int64)
    assert oracle.stream_checksum("encode", 3, n_len, plants=arr, chunk_nt=k) == oracle.stream_checksum("encode", 3, n_len, plants=plants)
    # and they do change the value
    assert oracle.stream_checksum("encode", 3, n_len, plants=plants) != oracle.stream_checksum("encode", 3, n_len)


def test_stream_hamming_equals_the_direct_oracle_call(oracle):
    for n_len in (0, 1, 31, 32, 33, 32 * 40 + 17, 100003):
        for fa, fb in ((0, 0), (32, 0), (0, 32 * 9), (32 * 1000, 32 * 3)):
            a = oracle.n_to_bits_lut(oracle.fill_random_acgt(n_len, 1, first_nt=fa))
            b = oracle.n_to_bits_lut(oracle.fill_random_acgt(n_len, 2, first_nt=fb))
            want = oracle.hamming(a, b, n_len)
            assert oracle.stream_hamming(1, 2, n_len, first_nt_a=fa, first_nt_b=fb) == want, (n_len, fa, fb)
            per = oracle.stream_hamming(1, 2, n_len, first_nt_a=fa, first_nt_b=fb, per_chunk=True, chunk_nt=32 * 5)
            assert sum(per) == want and (n_len == 0 or len(per) == -(-n_len // 160))
    # the same seed at the same offset is distance 0; at a shifted offset it is not
    assert oracle.stream_hamming(4, 4, 100003, chunk_nt=32 * 7) == 0
    assert oracle.stream_hamming(4, 4, 100003, first_nt_a=32, chunk_nt=32 * 7) > 0
    with pytest.raises(ValueError):
        oracle.stream_hamming(1, 2, 100, first_nt_a=1)


def test_stream_validate_equals_the_direct_oracle_call(oracle):
    for n_len, first_nt in ((0, 0), (1, 0), (100003, 0), (100003, 1), (32 * 50 + 7, 32 * 3 + 5), (4099, 31)):
        n = oracle.fill_random_acgt(n_len + (first_nt & 31), 6, first_nt=first_nt & ~31)[first_nt & 31 :]
        plants = [(p, b) for p, b in ((0, ord("N")), (n_len // 2, 0), (n_len // 2 + 1, ord("n")), (n_len - 1, ord("*"))) if 0 <= p < n_len]
        for p, b in plants:
            n[p] = b
        for allow in (False, True):
            want = oracle.validate(n, allow_n=allow)
            for chunk_nt in (None, 7, 1000):
                assert oracle.stream_validate(6, n_len, first_nt=first_nt, plants=plants, allow_n=allow, chunk_nt=chunk_nt) == want
            per = oracle.stream_validate(6, n_len, first_nt=first_nt, plants=plants, allow_n=allow, per_chunk=True, chunk_nt=1000)
            assert sum(per) == want
    # a clean stream validates clean; with N allowed an N plant is not counted, a byte outside every alphabet is
    plants = [(10, ord("N")), (20, ord("n")), (30, 0), (40, ord("X"))]
    assert oracle.stream_validate(6, 1 << 16) == 0
    assert oracle.stream_validate(6, 1 << 16, plants=plants) == 4
    assert oracle.stream_validate(6, 1 << 16, plants=plants, allow_n=True) == 2


def test_stream_functions_refuse_unaligned_word_starts_and_unknown_kinds(oracle):
    with pytest.raises(ValueError):
        oracle.stream_checksum("encode", 1, 100, first_nt=5)
    with pytest.raises(ValueError):
        oracle.stream_checksum("encode5", 1, 100, first_nt=32)
    with pytest.raises(ValueError):
        oracle.stream_checksum("decode", 1, 100)
    with pytest.raises(ValueError):
        oracle.stream_checksum("encode5", 1, 100, chunk_nt=20)  # no whole 27-nt word in a chunk


def test_worker_count_does_not_change_the_result(oracle):
    n_len = 32 * 3000 + 19
    plants = [(32 * 100, 0), (n_len - 1, ord("N"))]
    for kind in ACGT_KINDS + ("encode5",):
        first_nt = 27 * 32 * 4
        vals = {w: oracle.stream_checksum(kind, 8, n_len, first_nt=first_nt, plants=plants, per_chunk=True, chunk_nt=32 * 27 * 2, workers=w)
                for w in (1, 3, 16)}
        assert vals[1] == vals[3] == vals[16], kind
    assert len({oracle.stream_hamming(1, 2, n_len, chunk_nt=320, workers=w) for w in (1, 5, 16)}) == 1
    assert len({oracle.stream_validate(1, n_len, plants=plants, chunk_nt=333, workers=w) for w in (1, 5, 16)}) == 1


def test_per_chunk_checksum_sees_a_swap_and_a_bit_flip(oracle):
    """extends test_oracle.py::test_checksum_position_sensitive to the per-chunk sum the full-size tests compare: the
    sum of the chunk checksums at their global salts equals the whole checksum, and swapping two words -- inside one chunk
    or across a chunk boundary -- or flipping one bit of one word changes the total and exactly the chunks touched"""
    n_len, k = 32 * 4000, 32 * 250
    fw = 77
    want = _direct(oracle, "encode", 12, n_len, first_nt=32 * fw)
    per = oracle.stream_checksum("encode", 12, n_len, first_nt=32 * fw, per_chunk=True, chunk_nt=k)
    kw = k // 32
    total = sum(per) % (1 << 64)
    assert total == oracle.checksum_words(want, first_word=fw)

    def chunk_sums(words):
        return [oracle.checksum_words(words[c * kw : (c + 1) * kw], first_word=fw + c * kw) for c in range(len(per))]

    assert chunk_sums(want) == per
    for i, j in ((10, 11), (kw - 1, kw), (5, 3 * kw + 5)):
        assert want[i] != want[j]
        w2 = want.copy()
        w2[[i, j]] = w2[[j, i]]
        s2 = chunk_sums(w2)
        assert sum(s2) % (1 << 64) != total
        assert {c for c in range(len(per)) if s2[c] != per[c]} == {i // kw, j // kw}
    for bit in (0, 1, 37, 63):
        w3 = want.copy()
        w3[2 * kw + 3] ^= np.uint64(1 << bit)
        s3 = chunk_sums(w3)
        assert sum(s3) % (1 << 64) != total
        assert [c for c in range(len(per)) if s3[c] != per[c]] == [2]


# ---- k-mers: stream_kmers_checksum, the whole-output value of the full-size k-mer tests ----------------------------------
def _direct_kmers(oracle, seed, n_len, k, canonical, first_nt=0):
    """the k-mers of the whole stream in one oracle call; any first_nt (generated from the word boundary below, sliced)"""
    g0 = first_nt & ~31
    n = oracle.fill_random_acgt(n_len + first_nt - g0, seed, first_nt=g0)[first_nt - g0 :]
    return oracle.kmers(oracle.n_to_bits_lut(n), n_len, k, canonical)


@pytest.mark.parametrize("k", [1, 2, 17, 31, 32])
@pytest.mark.parametrize("canonical", [False, True])
def test_stream_kmers_checksum_equals_the_direct_oracle_call(oracle, k, canonical):
    """chunk c of the k-mers is made from nt [lo, lo + m + k - 1): forced tiny chunks put the chunk boundaries inside
    k-mers (and, for k > chunk, several boundaries inside one k-mer), at word starts 0, 32*w and off the word grid"""
    for n_len in (0, k - 1, k, k + 1, 31, 32, 33, 32 * 40 + 17, 100003):
        for first_nt in (0, 32 * 12345, 45):
            want = _direct_kmers(oracle, 0x5EED + k, n_len, k, canonical, first_nt)
            total = oracle.checksum_words(want)
            for chunk_nt in (None, 1, 7, 33, 1000):
                if chunk_nt is not None and chunk_nt * 200 < n_len:
                    continue  # a few hundred chunks at most
                got = oracle.stream_kmers_checksum(0x5EED + k, n_len, k, canonical, first_nt=first_nt, chunk_nt=chunk_nt)
                assert got == total, (k, canonical, n_len, first_nt, chunk_nt)
            per = oracle.stream_kmers_checksum(0x5EED + k, n_len, k, canonical, first_nt=first_nt, per_chunk=True, chunk_nt=33)
            assert per == [oracle.checksum_words(want[c * 33 : (c + 1) * 33], first_word=c * 33) for c in range(len(per))]
            assert len(per) == -(-want.size // 33) and sum(per) % (1 << 64) == total


def test_stream_kmers_worker_count_does_not_change_the_result(oracle):
    n_len = 32 * 3000 + 19
    for k, canonical in ((1, False), (32, True), (21, True)):
        vals = {w: oracle.stream_kmers_checksum(3, n_len, k, canonical, first_nt=32 * 5, per_chunk=True, chunk_nt=999, workers=w)
                for w in (1, 3, 16)}
        assert vals[1] == vals[3] == vals[16] and len(vals[1]) == -(-(n_len - k + 1) // 999), (k, canonical)


def test_stream_kmers_per_chunk_sums_see_a_swap(oracle):
    """the per-chunk checksums add up to the total, and two swapped k-mers -- inside one chunk or across chunks -- change
    the total and exactly the chunks touched; forward and canonical streams differ"""
    n_len, k, kc = 32 * 2000 + 7, 31, 32 * 250 + 3
    want = _direct_kmers(oracle, 12, n_len, k, True)
    per = oracle.stream_kmers_checksum(12, n_len, k, True, per_chunk=True, chunk_nt=kc)
    total = oracle.stream_kmers_checksum(12, n_len, k, True)
    assert sum(per) % (1 << 64) == total == oracle.checksum_words(want)

    def chunk_sums(x):
        return [oracle.checksum_words(x[c * kc : (c + 1) * kc], first_word=c * kc) for c in range(len(per))]

    assert chunk_sums(want) == per
    for i, j in ((10, 11), (kc - 1, kc), (5, 3 * kc + 5)):
        assert want[i] != want[j]
        w2 = want.copy()
        w2[[i, j]] = w2[[j, i]]
        s2 = chunk_sums(w2)
        assert sum(s2) % (1 << 64) != total
        assert {c for c in range(len(per)) if s2[c] != per[c]} == {i // kc, j // kc}
    assert oracle.stream_kmers_checksum(12, n_len, k, False) != total
    with pytest.raises(ValueError):
        oracle.stream_kmers_checksum(12, n_len, 33, False)
