#!/usr/bin/env python3
"""Device-tier throughput of the FASTQ encode (packed_ops.fastq_to_bits_dev) on one MI355X, product build, 2^30 bytes by default.
Inputs: four-line records with 40-byte name lines, random ACGT and random qualities: reads of 150 bases once with line feeds and
once with carriage return + line feed, and reads of 20,000 bases with line feeds.  Every input is first checked at 2^22 bytes
against a numpy restatement of the definition.  One JSON row per input, printed and appended to --out, every figure of a row taken
in the same run:
  ms, min_ms, max_ms     median / extremes of --iters (>= 20) event-timed calls after a warm-up, the same buffers every call
  GBs                    text bytes per ns (FASTA's call: 1032 GB/s)
  counts                 what the call reported: n, records, invalid, quality bytes, malformed
  no_qual_ms             the call without qual and without the record table
  floor_ms               cnt_n_to_bits_checked_dev on the already-stripped bases plus a device copy of the Q quality bytes
  vs_floor               ms / floor_ms (reported, not gated)
  torch_strip_ms         what a user has on the device today, both keep masks GIVEN: text[seq_mask] through cnt_n_to_bits_dev, and
                         text[qual_mask]
The one condition: ms < torch_strip_ms in the same run (asserted).
With --trace-only the script runs three calls on each input and nothing else: the workload of a rocprofv3 --kernel-trace --stats
run for the per-pass split (profiles/fastq_kernel_trace.md).

Measured 2026-10-20, one MI355X, product build (profiles/fastq_bench.jsonl, profiles/fastq_kernel_trace.md), 2^30 bytes, reads of
150 lf / reads of 150 crlf / reads of 20,000 lf:
  the call               1.555 / 1.567 / 1.440 ms (691 / 685 / 746 GB/s of text), n = 468201436 / 464153550 / 536281968
  without qual, table    1.174 / 1.174 / 1.051 ms
  floor                  0.271 / 0.271 / 0.312 ms: the call costs 5.7 x / 5.8 x / 4.6 x the checked encode plus the copy
  torch strips + encode  13.61 / 13.53 / 14.13 ms with both masks given (8.8 x / 8.6 x / 9.8 x the call)
  passes (150 lf)        fastq_lines 185 us, fastq_line_scan 22 us, fastq_count 418 us, fastq_scan 184 us, hpc_zero_edges 7 us,
                         fastq_write_qual_rec 802 us
The tile passes are not bound by memory (the floor reads and encodes the same bases and copies the same qualities in 0.3 ms): VALU
work on the byte masks and the byte-wise LDS staging of lanes that hold a line end are the supposed bound.  No counters were
collected."""
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
ap.add_argument("--log2-bytes", type=int, default=30)
ap.add_argument("--log2-bytes-check", type=int, default=22)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--trace-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_bench.jsonl"))
a = ap.parse_args()
assert a.iters >= 20 and not _lib.is_lab_build()
STAMP = {"date": datetime.date.today().isoformat(), "build": "product"}
NAME = 40


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


def fastq(n_bytes, read, eol):
    """n_bytes of FASTQ on the device: records of a 40-byte name line, `read` random bases, '+' and `read` random qualities"""
    name = (b"@read " + b"x" * NAME)[: NAME - len(eol)] + eol
    rec = np.frombuffer(name + b"A" * read + eol + b"+" + eol + b"I" * read + eol, dtype=np.uint8)
    seq_at = NAME + np.arange(read)
    qual_at = seq_at + read + 2 * len(eol) + 1
    records = -(-n_bytes // rec.size)
    text = torch.from_numpy(rec.copy()).cuda().repeat(records).view(records, rec.size)
    letters = torch.empty(records * read, dtype=torch.uint8, device="cuda")
    devutil.fill_random_acgt(letters, 1)
    text[:, torch.from_numpy(seq_at).cuda()] = letters.view(records, read)
    del letters
    text[:, torch.from_numpy(qual_at).cuda()] = torch.randint(33, 74, (records, read), dtype=torch.uint8, device="cuda")
    return text.view(-1)[:n_bytes].clone()


def np_reference(t):
    """the definition (include/cute_nt.h "text formats: FASTQ"): (bases, qualities, rec_text, rec_start, rec_qual, malformed)"""
    nl = t == 0x0A
    role = (np.cumsum(nl) - nl) & 3
    line_start = np.r_[True, nl[:-1]]
    drop = nl | (t == 0x0D)
    sm, qm = (role == 1) & ~drop, (role == 3) & ~drop
    h = np.flatnonzero(line_start & (role == 0))
    malformed = int((line_start & (role == 0) & (t != 0x40)).sum() + (line_start & (role == 2) & (t != 0x2B)).sum())
    return t[sm], t[qm], h.astype(np.uint64), (np.cumsum(sm) - sm)[h].astype(np.uint64), (np.cumsum(qm) - qm)[h].astype(np.uint64), malformed


def torch_masks(t):
    """the two keep masks in torch, as np_reference builds them"""
    nl = t == 0x0A
    role = (torch.cumsum(nl, 0, dtype=torch.int32) - nl.to(torch.int32)) & 3
    keep = ~nl & (t != 0x0D)
    return (role == 1) & keep, (role == 3) & keep


n_bytes, n_check = 1 << a.log2_bytes, 1 << a.log2_bytes_check
out = torch.empty(n_bytes // 32 + 1, dtype=torch.int64, device="cuda")
qual = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
rec_cap = n_bytes // (2 * 150 + NAME) + 1024
rec_text, rec_start, rec_qual = (torch.empty(rec_cap, dtype=torch.int64, device="cuda") for _ in range(3))
counts = torch.empty(5, dtype=torch.int64, device="cuda")
work = torch.empty(po.fastq_to_bits_work_bytes(n_bytes), dtype=torch.uint8, device="cuda")

for name, read, eol in (("150_lf", 150, b"\n"), ("150_crlf", 150, b"\r\n"), ("20000_lf", 20000, b"\n")):
    text = fastq(n_bytes, read, eol)

    def call(t=text):
        po.fastq_to_bits_dev(t, out, counts, work, qual=qual, rec_text=rec_text, rec_start=rec_start, rec_qual=rec_qual)

    if a.trace_only:
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        continue
    bases, quals, want_rt, want_rs, want_rq, malformed = np_reference(text[:n_check].cpu().numpy())
    call(text[:n_check])
    got = counts.cpu().numpy().tolist()
    assert got == [bases.size, want_rt.size, 0, quals.size, malformed], (name, got)
    assert torch.equal(out[: (got[0] + 31) // 32], cn.n_to_bits_dev(torch.from_numpy(bases).cuda())), name
    assert np.array_equal(qual[: got[3]].cpu().numpy(), quals), name
    for arr, want in ((rec_text, want_rt), (rec_start, want_rs), (rec_qual, want_rq)):
        assert np.array_equal(arr[: got[1]].cpu().numpy().view(np.uint64), want), name
    ms = timed(call, a.iters)
    n, records, invalid, Q, malformed = counts.cpu().numpy().tolist()
    seq_mask, qual_mask = torch_masks(text)
    torch.cuda.empty_cache()
    stripped, q_stripped = text[seq_mask], text[qual_mask]
    # the whole result, against the alternative
    assert stripped.numel() == n and q_stripped.numel() == Q and invalid == 0 and malformed <= 1, (name, n, Q, invalid, malformed)
    assert torch.equal(out[: (n + 31) // 32], cn.n_to_bits_dev(stripped)) and torch.equal(qual[:Q], q_stripped), name
    assert records == -(-n_bytes // (NAME + 2 * read + 1 + 3 * len(eol))) and int(rec_text[records - 1]) == (records - 1) * (NAME + 2 * read + 1 + 3 * len(eol))
    no_qual = timed(lambda: po.fastq_to_bits_dev(text, out, counts, work), a.iters)
    floor_out, acc = torch.empty((n + 31) // 32, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    floor_qual = torch.empty(Q, dtype=torch.uint8, device="cuda")

    def floor_call():
        cn.n_to_bits_checked_dev(stripped, out=floor_out, acc=acc)
        floor_qual.copy_(q_stripped)

    def strip_call():
        cn.n_to_bits_dev(text[seq_mask], out=floor_out)
        return text[qual_mask]

    floor = timed(floor_call, a.iters)
    strip = timed(strip_call, a.iters)
    emit({"op": "fastq_to_bits", "input": name, "bytes": n_bytes, "n": n, "records": records, "invalid": invalid, "qual": Q, "malformed": malformed,
          "ms": round(ms[0], 4), "min_ms": round(ms[1], 4), "max_ms": round(ms[2], 4), "GBs": round(n_bytes / ms[0] / 1e6, 1), "no_qual_ms": round(no_qual[0], 4),
          "floor_ms": round(floor[0], 4), "floor_min_ms": round(floor[1], 4), "floor_max_ms": round(floor[2], 4), "vs_floor": round(ms[0] / floor[0], 3),
          "torch_strip_ms": round(strip[0], 4), "torch_strip_min_ms": round(strip[1], 4), "fasta_GBs": 1032, "work_bytes": work.numel(), "iters": a.iters})
    assert ms[0] < strip[0], "the call is not faster than two torch mask strips and an encode: %r" % ((ms, strip),)
    del text, seq_mask, qual_mask, stripped, q_stripped, floor_out, floor_qual
    torch.cuda.empty_cache()
