#!/usr/bin/env python3
"""Device-tier throughput of the windowed counts (packed_ops.window_counts_dev) on one MI355X, product build, 2^30 nt of
cnt_fill_random_acgt_dev data by default, k = 1 and k = 2:
  window = step in {64, 1024, 65536}   adjacent windows: lane groups of 1 and 8 lanes, and the piece kernels
  window = 1000, step = 100            overlapping windows: every input word is counted window / step = 10 times
  window = len                         one record: the check that a long window is spread over the chip
Every case is first checked at 2^22 nt against a numpy restatement of the definition.  One JSON row per case, printed and
appended to --out, every figure of a row taken in the same run:
  ms, min_ms, max_ms   median / extremes of --iters (>= 20) event-timed calls after a warm-up, the same buffers every call
  Gnts                 nucleotides of the sequence per ns
  n_win, overlap       records written, and window / step when the windows overlap (else 1)
  read_B, write_B      the algorithm's bytes: the input words once (step >= window) or `overlap` times, and the records
  GBs                  (read_B + write_B) / ms
  kmer_counts_ms       cnt_kmer_counts_dev at the same k on the same words (the whole-sequence table), timed the same way
  hamming_ms           cnt_hamming_dev(a, a): two read streams of the same words, the read-stream yardstick
  vs_kmer_counts       ms / kmer_counts_ms
With --trace-only the script runs three calls of each case and nothing else: the workload of a rocprofv3 --kernel-trace --stats
run.

Measured 2026-10-20, one MI355X, product build (profiles/window_counts_bench.jsonl), 2^30 nt, k = 1 / k = 2:
  window = step = 64 / 1024 / 65536   0.102 / 0.340 ms, 0.072 / 0.151 ms, 0.068 / 0.143 ms
  window = 1000, step = 100           0.646 / 1.689 ms: 9.0 x / 11.2 x the 1024-nt row at equal input, for an overlap of 10
  window = len                        0.076 / 0.142 ms = 0.34 x / 0.66 x cnt_kmer_counts_dev (0.226 / 0.216 ms) in the same run
  cnt_hamming_dev(a, a)               0.077 ms"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_counts_bench.jsonl"))
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


def np_reference(words, n, k, window, step):
    """the definition (include/cute_nt.h "windowed composition"): cumulative sums of the k-mer indicators, differenced"""
    i = np.arange(n, dtype=np.uint64)
    c = ((words[(i >> np.uint64(5)).astype(np.int64)] >> (np.uint64(2) * (i & np.uint64(31)))) & np.uint64(3)).astype(np.int64)
    x = c if k == 1 else c[:-1] | (c[1:] << 2)
    n_win = (n - window) // step + 1
    lo = np.arange(n_win, dtype=np.int64) * step
    out = np.empty((n_win, 4 ** k), dtype=np.uint32)
    for v in range(4 ** k):
        cs = np.concatenate([[0], np.cumsum(x == v)])
        out[:, v] = cs[lo + window - k + 1] - cs[lo]
    return out


def cases(n):
    return [(64, 64), (1024, 1024), (65536, 65536), (1000, 100), (n, n)]


n_len, n_check = 1 << a.log2_nt, 1 << a.log2_nt_check
d = torch.empty(n_len, dtype=torch.uint8, device="cuda")
devutil.fill_random_acgt(d, 1)
bits = cn.n_to_bits_dev(d)
del d
torch.cuda.empty_cache()
most = max(po.window_counts_n(n_len, 1, w, s) for w, s in cases(n_len))
out = torch.empty(most * 16, dtype=torch.int32, device="cuda")

if a.trace_only:
    for k in (1, 2):
        for window, step in cases(n_len):
            for _ in range(3):
                po.window_counts_dev(bits, n_len, k, window, step, out=out)
    torch.cuda.synchronize()
    sys.exit(0)

host = bits[: n_check // 32].cpu().numpy().view(np.uint64)
for k in (1, 2):
    for window, step in cases(n_check):
        got = po.window_counts_dev(bits, n_check, k, window, step, out=out).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, np_reference(host, n_check, k, window, step)), (k, window, step)

acc = torch.zeros(1, dtype=torch.int64, device="cuda")
hamming = timed(lambda: po.hamming_dev(bits, bits, n_len, acc=acc), a.iters)
for k in (1, 2):
    table = torch.zeros(4 ** k, dtype=torch.int64, device="cuda")
    yard = timed(lambda: po.kmer_counts_dev(bits, n_len, k, out=table), a.iters)
    for window, step in cases(n_len):
        ms = timed(lambda: po.window_counts_dev(bits, n_len, k, window, step, out=out), a.iters)
        n_win = po.window_counts_n(n_len, k, window, step)
        overlap = window / step if step < window else 1
        read_b, write_b = n_len / 4 * overlap, n_win * 4 ** k * 4
        emit({"op": "window_counts", "k": k, "window": window, "step": step, "nt": n_len, "n_win": n_win, "overlap": overlap,
              "ms": round(ms[0], 4), "min_ms": round(ms[1], 4), "max_ms": round(ms[2], 4), "Gnts": round(n_len / ms[0] / 1e6, 2),
              "read_B": int(read_b), "write_B": write_b, "GBs": round((read_b + write_b) / ms[0] / 1e6, 1),
              "kmer_counts_ms": round(yard[0], 4), "kmer_counts_min_ms": round(yard[1], 4), "kmer_counts_max_ms": round(yard[2], 4),
              "hamming_ms": round(hamming[0], 4), "hamming_min_ms": round(hamming[1], 4), "hamming_max_ms": round(hamming[2], 4),
              "vs_kmer_counts": round(ms[0] / yard[0], 3), "iters": a.iters})
