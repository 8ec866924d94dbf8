#!/usr/bin/env python3
"""Device-tier throughput of k-mer extraction (packed_ops.kmers_dev) on one MI355X, product build, 2^30 nt by default,
k = 21 and 31, forward and canonical.  One JSON row per case:
  ms            median of event-timed back-to-back calls (bench_packed_ops.py's `timed`)
  bytes         algorithmic bytes: 8*m written + 8*ceil(len/32) read, m = len-k+1
  frac_of_8TBs  bytes / ms against the 8 TB/s HBM peak
  vs_fill       the same-run write ceiling -- a torch fill of the same m*8 output bytes, timed the same way -- over ms
  launches      kernel launches of one call (counted by torch.profiler)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import cute_nucleotides_amd as cn  # noqa: E402
from cute_nucleotides_amd import devutil, packed_ops as po  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-nt", type=int, default=30)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--ks", default="21,31")
a = ap.parse_args()


def timed(fn, inner=5):
    """median over a.iters measurements of `inner` back-to-back calls between two events (per call)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    ts = []
    for _ in range(a.iters):
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    ts.sort()
    return ts[len(ts) // 2]


def launches(fn):
    """kernel launches of one call, from torch.profiler's device activity (None if the profiler records none)"""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "kmer" in e.name)
    return n or None


n_len = 1 << a.log2_nt
d = torch.empty(n_len, dtype=torch.uint8, device="cuda")
devutil.fill_random_acgt(d, 1)
bits = cn.n_to_bits_dev(d)
del d
words = bits.numel()
out = torch.empty(n_len, dtype=torch.int64, device="cuda")  # >= m for every k
for k in (int(x) for x in a.ks.split(",")):
    m = n_len - k + 1
    fill_ms = timed(lambda: out[:m].fill_(0))
    for canonical in (False, True):
        fn = lambda: po.kmers_dev(bits, n_len, k, canonical=canonical, out=out)  # noqa: E731
        ms = timed(fn)
        nbytes = 8 * m + 8 * words
        print(json.dumps({"op": "kmers", "k": k, "canonical": canonical, "nt": n_len, "kmers": m, "ms": round(ms, 4), "bytes": nbytes,
                          "GBs": round(nbytes / ms / 1e6, 1), "frac_of_8TBs": round(nbytes / ms / 1e6 / 8000, 4),
                          "fill_ms": round(fill_ms, 4), "vs_fill": round(fill_ms / ms, 4), "launches": launches(fn)}), flush=True)
