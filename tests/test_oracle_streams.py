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
