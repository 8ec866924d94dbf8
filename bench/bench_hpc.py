#!/usr/bin/env python3
"""Device-tier throughput of homopolymer compression (packed_ops.hpc_dev) on one MI355X, product build, 2^30 nt by default.
Inputs: cnt_fill_random_acgt_dev data (n ~ 0.75 len: runs of 1.33 nt) and a long-run input -- random {A,C} words thinned twice, so
that a C falls on one position in 64: runs of ~32 nt, tiles whose bases sit at every 2-bit phase of a word, n ~ len / 32.  Every
case is first checked at 2^22 nt against a numpy restatement of the definition.  One JSON row per case, printed and appended to
--out, every figure of a row taken in the same run:
  ms, min_ms, max_ms   median / extremes of --iters (>= 20) event-timed calls after a warm-up, the same buffers every call
  Gnts                 nucleotides per ns
  n                    runs of the input
  GBs                  the algorithm's traffic over ms: 0.25 B/nt read twice, n / 4 B of packed output and, with pos, 8 n B
  complement_ms        cnt_complement_dev on the same words (0.25 B read + 0.25 B written per nt), timed the same way: the yardstick
  vs_complement        ms / complement_ms
With --trace-only the script runs three calls with pos and three without on each input and nothing else: the workload of a
rocprofv3 --kernel-trace --stats run for the per-pass split (profiles/hpc_kernel_trace.md).

Measured 2026-10-19, one MI355X, product build (profiles/hpc_bench.jsonl, profiles/hpc_kernel_trace.md), 2^30 nt:
  random ACGT   n = 805312467: 0.427 ms without pos (4.72x the complement call's 0.0906 ms), 1.922 ms with pos (21.2x)
  long runs     n = 33031223:  0.373 ms without pos (4.13x of 0.0904 ms),                   0.432 ms with pos (4.78x)
  passes        hpc_count 92 us, counted_scan 20 us, hpc_zero_edges 6 us, hpc_write 321 / 273 us, hpc_write_pos 1760 / 343 us
The write pass is the longest.  With pos on random ACGT it stores 6.4 GB of positions at 3.7 TB/s; without pos it takes 3.5x the
time hpc_count takes for the same read although it writes only 0.2 GB: what bounds it was not isolated (no counters collected)."""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import cute_nucleotides_amd as cn  # noqa: E402
from cute_nucleotides_amd import _lib, devutil, packed_ops as po  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-nt", type=int, default=30)
ap.add_argument("--log2-nt-check", type=int, default=22)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--trace-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpc_bench.jsonl"))
a = ap.parse_args()
assert a.iters >= 20 and not _lib.is_lab_build()
STAMP = {"date": datetime.date.today().isoformat(), "build": "product"}


def timed(fn, iters):
    """(median, min, max) over `iters` calls, each between two events of its own"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def emit(row):
    row.update(STAMP)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


def sequence(kind, n_len):
    """the packed words of an input"""
    if kind == "acgt":
        d = torch.empty(n_len, dtype=torch.uint8, device="cuda")
        devutil.fill_random_acgt(d, 1)
        return cn.n_to_bits_dev(d)
    words = (n_len + 31) // 32
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    w = torch.randint(-(1 << 63), (1 << 63) - 1, (words,), dtype=torch.int64, device="cuda", generator=gen)
    for _ in range(2):  # the even bits of six random words ANDed: a C at one position in 64, an A elsewhere
        w &= torch.randint(-(1 << 63), (1 << 63) - 1, (words,), dtype=torch.int64, device="cuda", generator=gen)
        w &= torch.randint(-(1 << 63), (1 << 63) - 1, (words,), dtype=torch.int64, device="cuda", generator=gen)
    w &= torch.randint(-(1 << 63), (1 << 63) - 1, (words,), dtype=torch.int64, device="cuda", generator=gen)
    w &= 0x5555555555555555
    return w


def np_reference(words, n):
    """the definition (include/cute_nt.h "homopolymer compression"): (packed run bases, run starts)"""
    i = np.arange(n, dtype=np.uint64)
    s = ((words[(i >> np.uint64(5)).astype(np.int64)] >> (np.uint64(2) * (i & np.uint64(31)))) & np.uint64(3))
    keep = np.r_[True, s[1:] != s[:-1]]
    kept = s[keep]
    padded = np.zeros((kept.size + 31) // 32 * 32, dtype=np.uint64)
    padded[: kept.size] = kept
    return (padded.reshape(-1, 32) << (np.uint64(2) * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64), np.flatnonzero(keep).astype(np.uint64)


n_len, n_check = 1 << a.log2_nt, 1 << a.log2_nt_check
words = n_len // 32
out = torch.empty(words, dtype=torch.int64, device="cuda")
pos = torch.empty(n_len, dtype=torch.int64, device="cuda")
count = torch.empty(1, dtype=torch.int64, device="cuda")
work = torch.empty(po.hpc_work_bytes(n_len), dtype=torch.uint8, device="cuda")
comp = torch.empty(words, dtype=torch.int64, device="cuda")

for kind in ("acgt", "ac_long_runs"):
    bits = sequence(kind, n_len)
    if a.trace_only:
        for with_pos in (True, False):
            for _ in range(3):
                po.hpc_dev(bits, n_len, out, count, work, pos=pos if with_pos else None)
        torch.cuda.synchronize()
        continue
    host = bits[: n_check // 32].cpu().numpy().view(np.uint64)
    want_out, want_pos = np_reference(host, n_check)
    for with_pos in (True, False):
        po.hpc_dev(bits, n_check, out, count, work, pos=pos if with_pos else None)
        n = int(count.item())
        assert n == want_pos.size and np.array_equal(out[: want_out.size].cpu().numpy().view(np.uint64), want_out), (kind, with_pos, n)
        assert not with_pos or np.array_equal(pos[:n].cpu().numpy().view(np.uint64), want_pos), kind
    yard = timed(lambda: po.complement_dev(bits, n_len, out=comp), a.iters)
    for with_pos in (False, True):
        ms = timed(lambda: po.hpc_dev(bits, n_len, out, count, work, pos=pos if with_pos else None), a.iters)
        n = int(count.item())
        traffic = 2 * n_len / 4 + n / 4 + (8 * n if with_pos else 0)
        emit({"op": "hpc", "input": kind, "pos": with_pos, "nt": n_len, "n": n, "ms": round(ms[0], 4), "min_ms": round(ms[1], 4), "max_ms": round(ms[2], 4),
              "Gnts": round(n_len / ms[0] / 1e6, 2), "GBs": round(traffic / ms[0] / 1e6, 1), "complement_ms": round(yard[0], 4),
              "complement_min_ms": round(yard[1], 4), "complement_max_ms": round(yard[2], 4), "vs_complement": round(ms[0] / yard[0], 3),
              "work_bytes": work.numel(), "iters": a.iters})
    del bits
    torch.cuda.empty_cache()
