#!/usr/bin/env python3
"""Device-tier throughput of the FASTA encode (packed_ops.fasta_to_bits_dev) on one MI355X, product build, 2^30 bytes by default.
Inputs: 60-column FASTA of random ACGT with a 40-byte header line every 2^20 bases, once with line feeds and once with carriage
return + line feed.  Every input is first checked at 2^22 bytes against a numpy restatement of the definition.  One JSON row per
input, printed and appended to --out, every figure of a row taken in the same run:
  ms, min_ms, max_ms     median / extremes of --iters (>= 20) event-timed calls after a warm-up, the same buffers every call
  GBs                    text bytes per ns
  n, records, invalid    what the call reported
  floor_ms               cnt_n_to_bits_checked_dev on the already-stripped bytes, timed the same way: what the encode alone costs
  vs_floor               ms / floor_ms (reported, not gated)
  torch_strip_ms         what a user has on the device today, the keep mask GIVEN: text[mask] and cnt_n_to_bits_dev on the result
  torch_mask_strip_ms    the same with the mask built in torch first (line starts, cummax, header test), median of 3 calls
  host_strip_encode_s    the host alternative, once: bytes.translate and a header filter on the CPU, then n_to_bits_hip
The one condition: ms < torch_strip_ms in the same run (asserted).
With --trace-only the script runs three calls on each input and nothing else: the workload of a rocprofv3 --kernel-trace --stats
run for the per-pass split (profiles/fasta_kernel_trace.md).

Measured 2026-10-20, one MI355X, product build (profiles/fasta_bench.jsonl, profiles/fasta_kernel_trace.md), 2^30 bytes, lf / crlf:
  the call               1.040 / 1.040 ms (1032 GB/s of text), n = 1056099114 / 1039065226, 1008 / 991 records
  floor                  0.199 / 0.198 ms: the call costs 5.2 x the checked encode of the stripped bytes
  torch strip + encode   9.568 / 9.387 ms with the mask given (9.2 x / 9.0 x the call), 3478 / 3432 ms with the mask built in torch
  CPU strip + host tier  3.1 / 2.9 s
  passes                 fasta_summary 342 us, fasta_scan 131 us, hpc_zero_edges 7 us, fasta_write_rec 572 us
The tile passes are not bound by memory (the floor reads and encodes the same bytes in 0.2 ms): the byte masks cost a lane about 50
VALU operations per dword.  No counters were collected."""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import cute_nucleotides_amd as cn  # noqa: E402
from cute_nucleotides_amd import _lib, devutil, packed_ops as po  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-bytes", type=int, default=30)
ap.add_argument("--log2-bytes-check", type=int, default=22)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--trace-only", action="store_true")
ap.add_argument("--no-host", action="store_true", help="skip the host alternative (seconds of CPU time at 2^30)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_bench.jsonl"))
a = ap.parse_args()
assert a.iters >= 20 and not _lib.is_lab_build()
STAMP = {"date": datetime.date.today().isoformat(), "build": "product"}
BASES, COLUMNS, HEADER = 1 << 20, 60, 40


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


def fasta(n_bytes, eol):
    """n_bytes of FASTA on the device: records of a 40-byte header line and 2^20 random bases in lines of 60"""
    lines = -(-BASES // COLUMNS)
    body = BASES + lines * len(eol)
    rec = np.full(HEADER + body, 0x0A, dtype=np.uint8)
    name = (b">record " + b"x" * HEADER)[: HEADER - len(eol)] + eol
    rec[:HEADER] = np.frombuffer(name, dtype=np.uint8)
    line, col = np.divmod(np.arange(BASES), COLUMNS)
    slots = HEADER + line * (COLUMNS + len(eol)) + col  # where the bases of a record lie in its text
    ends = np.setdiff1d(np.arange(HEADER, HEADER + body), slots)
    rec[ends] = np.frombuffer(eol * lines, dtype=np.uint8)
    records = -(-n_bytes // rec.size)
    text = torch.from_numpy(rec).cuda().repeat(records).view(records, rec.size)
    letters = torch.empty(records * BASES, dtype=torch.uint8, device="cuda")
    devutil.fill_random_acgt(letters, 1)
    text[:, torch.from_numpy(slots).cuda()] = letters.view(records, BASES)
    return text.view(-1)[:n_bytes].clone()


def np_reference(t):
    """the definition (include/cute_nt.h "text formats: FASTA"): (kept bytes, rec_text, rec_start)"""
    line_start = np.r_[True, t[:-1] == 0x0A]
    last = np.maximum.accumulate(np.where(line_start, np.arange(t.size), 0))
    keep = (t[last] != 0x3E) & (t != 0x0A) & (t != 0x0D)
    h = np.flatnonzero(line_start & (t == 0x3E))
    return t[keep], h.astype(np.uint64), (np.cumsum(keep) - keep)[h].astype(np.uint64)


def torch_mask(t):
    """the keep mask in torch, as np_reference builds it"""
    line_start = torch.ones_like(t, dtype=torch.bool)
    line_start[1:] = t[:-1] == 0x0A
    at = torch.arange(t.numel(), device=t.device)
    last = torch.cummax(torch.where(line_start, at, torch.zeros_like(at)), 0).values
    return (t[last] != 0x3E) & (t != 0x0A) & (t != 0x0D)


n_bytes, n_check = 1 << a.log2_bytes, 1 << a.log2_bytes_check
out = torch.empty(n_bytes // 32 + 1, dtype=torch.int64, device="cuda")
rec_cap = n_bytes // BASES + 1024
rec_text, rec_start = (torch.empty(rec_cap, dtype=torch.int64, device="cuda") for _ in range(2))
counts = torch.empty(3, dtype=torch.int64, device="cuda")
work = torch.empty(po.fasta_to_bits_work_bytes(n_bytes), dtype=torch.uint8, device="cuda")

for name, eol in (("lf", b"\n"), ("crlf", b"\r\n")):
    text = fasta(n_bytes, eol)

    def call(t=text):
        po.fasta_to_bits_dev(t, out, counts, work, rec_text=rec_text, rec_start=rec_start)

    if a.trace_only:
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        continue
    kept, want_rt, want_rs = np_reference(text[:n_check].cpu().numpy())
    call(text[:n_check])
    n, records, invalid = counts.cpu().numpy().tolist()
    assert (n, records, invalid) == (kept.size, want_rt.size, 0), (name, n, records, invalid)
    assert torch.equal(out[: (n + 31) // 32], cn.n_to_bits_dev(torch.from_numpy(kept).cuda())), name
    assert np.array_equal(rec_text[:records].cpu().numpy().view(np.uint64), want_rt) and np.array_equal(rec_start[:records].cpu().numpy().view(np.uint64), want_rs)
    ms = timed(call, a.iters)
    n, records, invalid = counts.cpu().numpy().tolist()
    mask = torch_mask(text)
    stripped = text[mask]
    assert stripped.numel() == n and torch.equal(out[: (n + 31) // 32], cn.n_to_bits_dev(stripped)), name  # the whole result, against the alternative
    floor_out, acc = torch.empty((n + 31) // 32, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    floor = timed(lambda: cn.n_to_bits_checked_dev(stripped, out=floor_out, acc=acc), a.iters)
    strip = timed(lambda: cn.n_to_bits_dev(text[mask], out=floor_out), a.iters)
    del mask, stripped
    torch.cuda.empty_cache()
    mask_strip = timed(lambda: cn.n_to_bits_dev(text[torch_mask(text)], out=floor_out), 3)
    torch.cuda.empty_cache()
    host_s = None
    if not a.no_host:
        raw = text.cpu().numpy().tobytes()
        t0 = time.perf_counter()
        bases = b"".join(line for line in raw.translate(None, b"\r").split(b"\n") if not line.startswith(b">"))
        words = cn.n_to_bits_hip(bases)
        host_s = time.perf_counter() - t0
        assert len(bases) == n and words.size == (n + 31) // 32
        del raw, bases, words
    emit({"op": "fasta_to_bits", "input": name, "bytes": n_bytes, "n": n, "records": records, "invalid": invalid, "ms": round(ms[0], 4), "min_ms": round(ms[1], 4),
          "max_ms": round(ms[2], 4), "GBs": round(n_bytes / ms[0] / 1e6, 1), "floor_ms": round(floor[0], 4), "floor_min_ms": round(floor[1], 4),
          "floor_max_ms": round(floor[2], 4), "vs_floor": round(ms[0] / floor[0], 3), "torch_strip_ms": round(strip[0], 4), "torch_strip_min_ms": round(strip[1], 4),
          "torch_mask_strip_ms": round(mask_strip[0], 4), "host_strip_encode_s": None if host_s is None else round(host_s, 3), "work_bytes": work.numel(),
          "iters": a.iters})
    assert ms[0] < strip[0], "the call is not faster than a torch mask strip and an encode: %r" % ((ms, strip),)
    del text
    torch.cuda.empty_cache()
