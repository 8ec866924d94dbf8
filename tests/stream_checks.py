"""Full-length checks of large device outputs against the oracle's whole-stream expected values (oracle/cnt_oracle.py
stream_*), shared by the full-size GPU tests.  One device checksum of the whole output is compared with the oracle's; on
a mismatch the per-chunk checksums name the first chunk that differs.  The mutation check shows that the comparison sees
one changed word where no sampled chunk looks."""
import time

import pytest


def _grain(kind):
    return 27 if kind == "encode5" else 32


def check_words(words, kind, seed, n_len, first_nt=0, plants=(), label="", record=None, want=None):
    """devutil.checksum_words(words) at the global word index == oracle.stream_checksum(kind, ...): `words` is the whole
    output for the n_len-nt stream at `first_nt` (an int64 CUDA tensor, any 8-B phase).  Returns the expected checksum.
    `record` (the `fullsize` fixture) logs the check's wall time; `want` is the oracle's value when a check of the same
    stream already computed it."""
    from cute_nucleotides_amd import devutil
    from oracle import cnt_oracle as orc

    fw = first_nt // _grain(kind)
    t0 = time.perf_counter()
    if want is None:
        want = orc.stream_checksum(kind, seed, n_len, first_nt=first_nt, plants=plants)
    got = devutil.checksum_words(words, first_word=fw)
    if record is not None:
        record(n_len.bit_length() - 1, (time.perf_counter() - t0) * 1e3, check="full-length oracle: " + (label or kind))
    if got != want:
        pytest.fail("%s: full-length checksum %#x != oracle %#x; %s" % (label or kind, got, want,
                                                                        first_bad_chunk(words, kind, seed, n_len, first_nt, plants)))
    return want


def first_bad_chunk(words, kind, seed, n_len, first_nt=0, plants=()):
    """names the first chunk of the output whose device checksum differs from the oracle's (chunks of STREAM_CHUNK_NT)"""
    from cute_nucleotides_amd import devutil
    from oracle import cnt_oracle as orc

    g = _grain(kind)
    fw, kw = first_nt // g, orc.STREAM_CHUNK_NT // g
    per = orc.stream_checksum(kind, seed, n_len, first_nt=first_nt, plants=plants, per_chunk=True)
    for c, want in enumerate(per):
        got = devutil.checksum_words(words[c * kw : (c + 1) * kw], first_word=fw + c * kw)
        if got != want:
            return "first differing chunk %d of %d: words [%d, %d), nt [%d, %d) of the output" % (
                c, len(per), c * kw, min((c + 1) * kw, words.numel()), c * kw * g, min((c + 1) * kw * g, n_len))
    return "no chunk differs on its own (words beyond the output?)"


def check_hamming(a, b, n_len, seed_a, seed_b, first_nt_a=0, first_nt_b=0, label="hamming"):
    """packed_ops.hamming_dev(a, b, n_len) == oracle.stream_hamming(...): `a` / `b` hold the encoded streams from their
    first words on.  On a mismatch the per-chunk distances (device over word slices) name the first chunk that differs.
    Returns the expected distance."""
    from cute_nucleotides_amd import packed_ops as po
    from oracle import cnt_oracle as orc

    want = orc.stream_hamming(seed_a, seed_b, n_len, first_nt_a=first_nt_a, first_nt_b=first_nt_b)
    got = int(po.hamming_dev(a, b, n_len).item())
    if got != want:
        per = orc.stream_hamming(seed_a, seed_b, n_len, first_nt_a=first_nt_a, first_nt_b=first_nt_b, per_chunk=True)
        kw = orc.STREAM_CHUNK_NT // 32
        where = "no chunk differs on its own"
        for c, w in enumerate(per):
            m = min(kw * 32, n_len - c * kw * 32)
            g = int(po.hamming_dev(a[c * kw : (c + 1) * kw], b[c * kw : (c + 1) * kw], m).item())
            if g != w:
                where = "first differing chunk %d of %d: nt [%d, %d), device %d, oracle %d" % (c, len(per), c * kw * 32, c * kw * 32 + m, g, w)
                break
        pytest.fail("%s: %d != oracle %d; %s" % (label, got, want, where))
    return want


def check_validate(n, seed, n_len, first_nt=0, plants=(), allow_n=False, label="validate"):
    """packed_ops.validate_dev(n) == oracle.stream_validate(...): `n` holds the n_len bytes of the stream from `first_nt`
    on (any byte).  On a mismatch the per-chunk counts (device over byte slices) name the first chunk that differs.
    Returns the expected count."""
    from cute_nucleotides_amd import packed_ops as po
    from oracle import cnt_oracle as orc

    want = orc.stream_validate(seed, n_len, first_nt=first_nt, plants=plants, allow_n=allow_n)
    got = int(po.validate_dev(n, allow_n=allow_n).item())
    if got != want:
        per = orc.stream_validate(seed, n_len, first_nt=first_nt, plants=plants, allow_n=allow_n, per_chunk=True)
        k = orc.STREAM_CHUNK_NT
        where = "no chunk differs on its own"
        for c, w in enumerate(per):
            g = int(po.validate_dev(n[c * k : (c + 1) * k], allow_n=allow_n).item())
            if g != w:
                where = "first differing chunk %d of %d: bytes [%d, %d), device %d, oracle %d" % (c, len(per), c * k, min((c + 1) * k, n_len), g, w)
                break
        pytest.fail("%s (allow_n=%s): %d != oracle %d; %s" % (label, allow_n, got, want, where))
    return want


def assert_mutation_seen(words, index, want, first_word=0):
    """XOR one word of `words` (an index no sampled chunk covers): the full-length checksum must no longer match `want`;
    the word is restored and the checksum matches again"""
    from cute_nucleotides_amd import devutil

    w = words[index : index + 1]
    w.bitwise_xor_(1 << 41)
    try:
        assert devutil.checksum_words(words, first_word=first_word) != want, index
    finally:
        w.bitwise_xor_(1 << 41)
    assert devutil.checksum_words(words, first_word=first_word) == want


def check_kmers(out, seed, n_len, k, canonical, label="", record=None, want=None, workers=16):
    """devutil.checksum_words(out) == oracle.stream_kmers_checksum(...): `out` is the whole k-mer output (an int64 CUDA
    tensor, any 8-B phase) of the fill_random_acgt stream of n_len nt.  On a mismatch the per-chunk checksums name the
    first chunk of k-mers that differs.  Returns the expected checksum; `record` and `want` as in check_words."""
    from cute_nucleotides_amd import devutil
    from oracle import cnt_oracle as orc

    label = label or "kmers k=%d %s" % (k, "canonical" if canonical else "forward")
    t0 = time.perf_counter()
    if want is None:
        want = orc.stream_kmers_checksum(seed, n_len, k, canonical, workers=workers)
    got = devutil.checksum_words(out)
    if record is not None:
        record(n_len.bit_length() - 1, (time.perf_counter() - t0) * 1e3, check="full-length oracle: " + label)
    if got != want:
        pytest.fail("%s: full-length checksum %#x != oracle %#x; %s" % (label, got, want, first_bad_kmer_chunk(out, seed, n_len, k, canonical, workers)))
    return want


def first_bad_kmer_chunk(out, seed, n_len, k, canonical, workers=16):
    """names the first chunk of STREAM_CHUNK_NT k-mers whose device checksum differs from the oracle's"""
    from cute_nucleotides_amd import devutil
    from oracle import cnt_oracle as orc

    kc = orc.STREAM_CHUNK_NT
    per = orc.stream_kmers_checksum(seed, n_len, k, canonical, per_chunk=True, workers=workers)
    for c, want in enumerate(per):
        if devutil.checksum_words(out[c * kc : (c + 1) * kc], first_word=c * kc) != want:
            return "first differing chunk %d of %d: k-mers [%d, %d)" % (c, len(per), c * kc, min((c + 1) * kc, out.numel()))
    return "no chunk differs on its own (k-mers beyond the output?)"
