#!/usr/bin/env python3
"""Device-tier throughput of the FASTA write (packed_ops.bits_to_fasta_dev) on one MI355X, product build, 2^30 bases by default,
width 60.  Three shapes: the bases as ONE record, as records of 2^20 bases, and as reads of 150, every record with a 40-byte
name.  Every shape is first checked at 2^22 bases against a numpy restatement of the definition, and at full size against the
torch alternative below.  One JSON row per shape, printed and appended to --out, every figure of a row taken in the same run:
  ms, min_ms, max_ms     median / extremes of --iters (>= 20) event-timed calls after a warm-up, the same buffers every call
  GBs                    text bytes per ns
  text_bytes, records    what the call reported, and the records given
  floor_ms               cnt_bits_to_n_dev at the same len, timed the same way: the same loads, the same stores less the line feeds
                         and names
  vs_floor               ms / floor_ms (reported, not gated)
  torch_scatter_ms       what a user has on the device today, the indices GIVEN: decode, fill the text with line feeds, scatter the
                         letters and the header bytes by index
  vs_torch               torch_scatter_ms / ms
With --trace-only the script runs three calls on each shape and nothing else: the workload of a rocprofv3 --kernel-trace --stats
run for the per-pass split (profiles/fasta_write_kernel_trace.md).

Measured 2026-10-20, one MI355X, product build (profiles/fasta_write_bench.jsonl, profiles/fasta_write_kernel_trace.md), 2^30 bases,
one record / 1024 records of 2^20 / 7,158,278 reads of 150:
  the call               0.472 / 0.525 / 3.947 ms (2314 / 2081 / 354 GB/s of text)
  floor                  0.190 / 0.191 / 0.191 ms: the call costs 2.5 x / 2.7 x / 20.7 x the plain decode
  torch decode + scatter 3.40 / 3.49 / 4.59 ms with the indices given (7.2 x / 6.6 x / 1.2 x the call)
  passes                 fasta_out_sizes 5 / 5 / 48 us, fasta_out_scan 5 / 5 / 67 us, fasta_out_offsets 4 / 5 / 29 us,
                         fasta_out_write 452 / 494 / 3762 us
The write pass is not bound by memory (the floor moves the same bytes in 0.19 ms): a wave's chain of dependent loads in front of its
first store and, for reads, the diverging byte-by-byte walk are the supposed bounds.  No counters were collected."""
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
ap.add_argument("--log2-bases", type=int, default=30)
ap.add_argument("--log2-bases-check", type=int, default=22)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--trace-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_write_bench.jsonl"))
a = ap.parse_args()
assert a.iters >= 20 and not _lib.is_lab_build()
STAMP = {"date": datetime.date.today().isoformat(), "build": "product"}
WIDTH, NAME = 60, 40


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


def np_reference(letters, rec_len, names):
    """the definition (include/cute_nt.h "text formats: FASTA write") for records of one length, in numpy: the text"""
    parts = []
    for r in range(letters.size // rec_len):
        body = letters[r * rec_len : (r + 1) * rec_len]
        lines = -(-rec_len // WIDTH)
        padded = np.full(lines * WIDTH, 0, dtype=np.uint8)
        padded[:rec_len] = body
        rows = np.c_[padded.reshape(lines, WIDTH), np.full(lines, 0x0A, dtype=np.uint8)].reshape(-1)
        parts += [np.frombuffer(b">", dtype=np.uint8), names[r * NAME : (r + 1) * NAME], np.frombuffer(b"\n", dtype=np.uint8), rows[rows != 0]]
    return np.concatenate(parts)


def indices(n, rec_len, device):
    """where every letter and every header byte lies in the text, for records of one length: (letter_idx, header_idx, total)"""
    body = rec_len + -(-rec_len // WIDTH)
    piece = 2 + NAME + body
    g = torch.arange(n, dtype=torch.int64, device=device)
    r = g // rec_len
    g -= r * rec_len
    letter_idx = r * piece + (1 + NAME + 1) + g + g // WIDTH
    del g, r
    records = n // rec_len
    header_idx = (torch.arange(records, dtype=torch.int64, device=device) * piece)[:, None] + torch.arange(1 + NAME + 1, dtype=torch.int64, device=device)[None, :]
    return letter_idx, header_idx.reshape(-1), records * piece


n_most, n_check = 1 << a.log2_bases, 1 << a.log2_bases_check
for shape, rec_len_of in (("one_record", lambda n: n), ("records_2^20", lambda n: min(n, 1 << 20)), ("reads_150", lambda n: 150)):
    for n_want in (n_check, n_most):
        rec_len = rec_len_of(n_want)
        records = n_want // rec_len
        n = records * rec_len
        letters = torch.empty(n, dtype=torch.uint8, device="cuda")
        devutil.fill_random_acgt(letters, 7)
        bits = cn.n_to_bits_dev(letters)
        rec_start = torch.arange(records, dtype=torch.int64, device="cuda") * rec_len
        name_off = torch.arange(records + 1, dtype=torch.int64, device="cuda") * NAME
        names = (torch.arange(records * NAME, dtype=torch.int64, device="cuda") % 26 + 0x61).to(torch.uint8)
        bound = po.bits_to_fasta_bound(n, records, records * NAME, WIDTH)
        text = torch.empty(bound, dtype=torch.uint8, device="cuda")
        rec_text = torch.empty(records, dtype=torch.int64, device="cuda")
        counts = torch.empty(2, dtype=torch.int64, device="cuda")
        work = torch.empty(po.bits_to_fasta_work_bytes(records), dtype=torch.uint8, device="cuda")

        def call():
            po.bits_to_fasta_dev(bits, n, text, counts, work, rec_start=rec_start, names=names, name_off=name_off, width=WIDTH, rec_text=rec_text)

        if a.trace_only:
            if n_want == n_most:
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
            continue
        call()
        total, malformed = counts.cpu().numpy().tolist()
        assert malformed == 0 and total <= bound, (shape, total, malformed)
        if n_want == n_check:
            want = np_reference(letters.cpu().numpy(), rec_len, names.cpu().numpy())
            assert total == want.size and np.array_equal(text[:total].cpu().numpy(), want), shape
            continue
        ms = timed(call, a.iters)
        back = torch.empty(n, dtype=torch.uint8, device="cuda")
        floor = timed(lambda: cn.bits_to_n_dev(bits, n, out=back), a.iters)
        assert torch.equal(back, letters)
        letter_idx, header_idx, want_total = indices(n, rec_len, "cuda")
        header = torch.cat([torch.full((records, 1), 0x3E, dtype=torch.uint8, device="cuda"), names.view(records, NAME),
                            torch.full((records, 1), 0x0A, dtype=torch.uint8, device="cuda")], 1).reshape(-1)
        alt = torch.empty(want_total, dtype=torch.uint8, device="cuda")

        def scatter():
            cn.bits_to_n_dev(bits, n, out=back)
            alt.fill_(0x0A)
            alt[letter_idx] = back
            alt[header_idx] = header

        torch_ms = timed(scatter, a.iters)
        assert want_total == total and torch.equal(alt, text[:total]), shape  # the whole result, against the alternative
        assert torch.equal(rec_text, torch.arange(records, dtype=torch.int64, device="cuda") * (total // records)), shape
        emit({"op": "bits_to_fasta", "shape": shape, "bases": n, "records": records, "width": WIDTH, "name_bytes": NAME, "text_bytes": total, "ms": round(ms[0], 4),
              "min_ms": round(ms[1], 4), "max_ms": round(ms[2], 4), "GBs": round(total / ms[0] / 1e6, 1), "floor_ms": round(floor[0], 4), "floor_min_ms": round(floor[1], 4),
              "floor_max_ms": round(floor[2], 4), "vs_floor": round(ms[0] / floor[0], 3), "torch_scatter_ms": round(torch_ms[0], 4),
              "torch_scatter_min_ms": round(torch_ms[1], 4), "vs_torch": round(torch_ms[0] / ms[0], 2), "work_bytes": work.numel(), "iters": a.iters})
        del letter_idx, header_idx, alt, header, back
    del letters, bits, text, rec_start, name_off, names, rec_text
    torch.cuda.empty_cache()
