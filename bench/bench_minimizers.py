#!/usr/bin/env python3
"""Device-tier throughput of (w,k)-minimizer sampling (packed_ops.minimizers_dev) on one MI355X, product build, 2^30 nt by
default, (k, w) = (15, 10), (21, 11), (31, 19), forward and canonical, positions and values.  One JSON row per case:
  ms            median of event-timed back-to-back calls (bench_kmers.py's `timed`), the same buffers every call
  Gnts          nucleotides per ns
  n, density    minimizers of the call, and n / W against 2 / (w+1)
  bytes         algorithmic bytes: two reads of the 8*ceil(len/32) input bytes (count and write pass) + 16*n written
  GBs           bytes / ms
  kmers_ms      the same-run cnt_kmers_dev (8 B per k-mer written) at the same len and k, timed the same way
  vs_kmers      kmers_ms / ms
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
ap.add_argument("--cases", default="15:10,21:11,31:19", help="k:w pairs")
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
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and ("minimizer" in e.name or "counted_scan" in e.name))
    return n or None


n_len = 1 << a.log2_nt
d = torch.empty(n_len, dtype=torch.uint8, device="cuda")
devutil.fill_random_acgt(d, 1)
bits = cn.n_to_bits_dev(d)
del d
words = bits.numel()
kout = torch.empty(n_len, dtype=torch.int64, device="cuda")  # >= m for every k
cap = n_len // 4  # >= 2/(w+1) of the windows for every w >= 8
pos = torch.empty(cap, dtype=torch.int64, device="cuda")
val = torch.empty(cap, dtype=torch.int64, device="cuda")
count = torch.empty(1, dtype=torch.int64, device="cuda")
for k, w in (tuple(int(y) for y in x.split(":")) for x in a.cases.split(",")):
    m = n_len - k + 1
    nw = m - w + 1
    work = torch.empty(po.minimizers_work_bytes(n_len, k, w), dtype=torch.uint8, device="cuda")
    kmers_ms = timed(lambda: po.kmers_dev(bits, n_len, k, out=kout))
    for canonical in (False, True):
        fn = lambda: po.minimizers_dev(bits, n_len, k, w, canonical=canonical, pos=pos, val=val, count=count, work=work)  # noqa: E731
        ms = timed(fn)
        n = int(count.item())
        assert n <= cap
        nbytes = 2 * 8 * words + 16 * n
        print(json.dumps({"op": "minimizers", "k": k, "w": w, "canonical": canonical, "nt": n_len, "windows": nw, "n": n,
                          "density": round(n / nw, 5), "expected_density": round(2 / (w + 1), 5), "ms": round(ms, 4),
                          "Gnts": round(n_len / ms / 1e6, 2), "bytes": nbytes, "GBs": round(nbytes / ms / 1e6, 1),
                          "kmers_ms": round(kmers_ms, 4), "vs_kmers": round(kmers_ms / ms, 4), "launches": launches(fn)}), flush=True)
