#!/usr/bin/env python3
"""Device-tier throughput of k-mer counting (packed_ops.kmer_counts_dev) on one MI355X, product build, 2^30 nt by default,
k in {1, 2, 3, 4, 6, 7, 8, 10, 12}, forward and canonical, on random and on all-A input.  One JSON row per case, every
figure of a row taken in the same run:
  ms                 median of event-timed back-to-back calls (the table is not zeroed in between: the call adds)
  Gnt_s              nt / ms
  kmers_ms           cnt_kmers_dev at the same len, k and flags: a lower bound on any route through materialised k-mers
  baseline_ms        kmers_dev + torch.bincount(minlength=4**k) on its output (in chunks of 2^28 k-mers, summed): the route
                     there was before this call
  regime             "lds" (k <= kKmerCountLdsMaxK) or "global"
  all_a_over_random  on the all-A rows: ms over the random row's ms of the same k, flags and size
The all-A rows of the global regime put every add on one word: they are taken at 2^26 nt with one timed call per
measurement, next to a random row of that size.
--split-ab: on the LAB build, k = 6 and 7 in both regimes (cnt_set_tuning "kmer_count_lds_max_k"), random input: the
measurement kKmerCountLdsMaxK is picked from."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import cute_nucleotides_amd as cn  # noqa: E402
from cute_nucleotides_amd import _lib, devutil, packed_ops as po  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-nt", type=int, default=30)
ap.add_argument("--log2-nt-one-word", type=int, default=26, help="size of the global regime's all-A rows")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--ks", default="1,2,3,4,6,7,8,10,12")
ap.add_argument("--split-ab", action="store_true")
a = ap.parse_args()
LDS_MAX_K = 7  # kKmerCountLdsMaxK (hip/kmer_count_kernels.hpp)


def timed(fn, iters=None, inner=None):
    """median over `iters` measurements of `inner` back-to-back calls between two events (per call); `inner` defaults to
    what keeps one measurement near 50 ms, from a first timed call after the warm-up"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    if inner is None:
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        inner = max(1, min(5, int(50 / max(e0.elapsed_time(e1), 1e-3))))
    ts = []
    for _ in range(iters or a.iters):
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    ts.sort()
    return ts[len(ts) // 2]


def random_bits(n_len):
    d = torch.empty(n_len, dtype=torch.uint8, device="cuda")
    devutil.fill_random_acgt(d, 1)
    bits = cn.n_to_bits_dev(d)
    del d
    return bits


def baseline(bits, n_len, k, canonical, out, chunk=1 << 28):
    """kmers_dev, then torch.bincount over its output in chunks of 2^28 k-mers, summed (one torch.bincount call over 2^30
    k-mers ends the process with an arithmetic exception inside torch, before any of this library's code runs)"""
    kmers = po.kmers_dev(bits, n_len, k, canonical=canonical, out=out)
    total = torch.zeros(4 ** k, dtype=torch.int64, device="cuda")
    for first in range(0, kmers.numel(), chunk):
        total += torch.bincount(kmers[first : first + chunk], minlength=4 ** k)
    return total


def row(bits, n_len, k, canonical, kind, out, one_call=False):
    table = torch.zeros(4 ** k, dtype=torch.int64, device="cuda")
    few = dict(iters=3, inner=1)
    ms = timed(lambda: po.kmer_counts_dev(bits, n_len, k, canonical=canonical, out=table), **(few if one_call else {}))
    kmers_ms = timed(lambda: po.kmers_dev(bits, n_len, k, canonical=canonical, out=out))
    baseline_ms = timed(lambda: baseline(bits, n_len, k, canonical, out), **few)
    return {"op": "kmer_counts", "k": k, "canonical": canonical, "input": kind, "nt": n_len, "regime": "lds" if k <= LDS_MAX_K else "global",
            "ms": round(ms, 4), "Gnt_s": round(n_len / ms / 1e6, 1), "kmers_ms": round(kmers_ms, 4), "baseline_ms": round(baseline_ms, 4)}


RANDOM_MS = {}  # (k, canonical, nt) -> ms of the random row


def emit(r):
    key = (r["k"], r["canonical"], r["nt"])
    if r.get("input") == "random":
        RANDOM_MS[key] = r["ms"]
    elif key in RANDOM_MS:
        r["all_a_over_random"] = round(r["ms"] / RANDOM_MS[key], 3)
    print(json.dumps(r), flush=True)


ks = [int(x) for x in a.ks.split(",")]
n_len = 1 << a.log2_nt
if a.split_ab:
    _lib.use_lab_build(True)
    bits = random_bits(n_len)
    for k in (6, 7):
        for canonical in (False, True):
            r = {"op": "kmer_counts_split_ab", "k": k, "canonical": canonical, "input": "random", "nt": n_len}
            for regime, max_k in (("lds", 7), ("global", k - 1)):
                _lib.check(_lib.lib().cnt_set_tuning(b"kmer_count_lds_max_k", max_k))
                table = torch.zeros(4 ** k, dtype=torch.int64, device="cuda")
                r[regime + "_ms"] = round(timed(lambda: po.kmer_counts_dev(bits, n_len, k, canonical=canonical, out=table)), 4)
            _lib.check(_lib.lib().cnt_set_tuning(b"kmer_count_lds_max_k", 7))
            print(json.dumps(r), flush=True)
    sys.exit(0)

out = torch.empty(n_len, dtype=torch.int64, device="cuda")  # >= m for every k
small = 1 << a.log2_nt_one_word
for kind in ("random", "all-A"):
    bits = random_bits(n_len) if kind == "random" else torch.zeros(n_len // 32, dtype=torch.int64, device="cuda")
    for k in ks:
        for canonical in (False, True):
            if k <= LDS_MAX_K:
                emit(row(bits, n_len, k, canonical, kind, out))
            elif kind == "random":
                emit(row(bits, n_len, k, canonical, kind, out))
                emit(row(bits, small, k, canonical, kind, out))  # the partner of the all-A row
            else:
                emit(row(bits, small, k, canonical, kind, out, one_call=True))
