#!/usr/bin/env python3
"""Device-tier throughput of the FASTQ write (packed_ops.bits_to_fastq_dev) on one MI355X, product build, 2^30 bases by default,
the shapes of bench_fasta_write.py that are reads: reads of 150 and reads of 20,000, every record with a 40-byte name.  Every
shape is first checked at 2^22 bases against a numpy restatement of the definition, and at full size against the torch
alternative below.  One JSON row per shape, printed and appended to --out, every figure of a row taken in the same run, the four
timed things taking turns call by call:
  ms, min_ms, max_ms     (a) median / extremes of --iters (>= 20) event-timed calls after a warm-up, the same buffers every call
  GBs                    text bytes per ns
  floor_ms               (b) cnt_bits_to_n_dev at the same len plus device copies of the len quality bytes and of the name bytes:
                         the loads and stores of the call less the tables and the seven constant bytes a record
  vs_floor               ms / floor_ms (reported, not gated)
  fasta_ms, fasta_GBs    (c) cnt_bits_to_fasta_dev at width 0 on the same table: the byte walk at every seam
  GBs_vs_fasta           GBs / fasta_GBs.  THE ACCEPTANCE CONDITION: at least 1 on reads of 150, no margin; the script ends with
                         status 1 behind its rows when it does not hold
  torch_scatter_ms       (d) what a user has on the device today, the indices GIVEN: decode, fill the text with line feeds, scatter
                         the letters, the qualities and the constant and name bytes by index
  vs_torch               torch_scatter_ms / ms
With --trace-only the script runs three calls on each shape and nothing else: the workload of a rocprofv3 --kernel-trace --stats
run for the per-pass split (profiles/fastq_write_kernel_trace.md)."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_write_bench.jsonl"))
a = ap.parse_args()
assert a.iters >= 20 and not _lib.is_lab_build()
STAMP = {"date": datetime.date.today().isoformat(), "build": "product"}
NAME = 40


def timed(fns, iters):
    """[(median, min, max)] of each of `fns` over `iters` rounds in which they take turns, each call between two events of its own"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def emit(row):
    row.update(STAMP)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


def np_reference(letters, qual, rec_len, names):
    """the definition (include/cute_nt.h "text formats: FASTQ write") for records of one length, in numpy: the text"""
    records = letters.size // rec_len
    col = lambda byte: np.full((records, 1), byte, dtype=np.uint8)  # noqa: E731
    return np.concatenate([col(0x40), names.reshape(records, NAME), col(0x0A), letters.reshape(records, rec_len), col(0x0A), col(0x2B), col(0x0A),
                           qual.reshape(records, rec_len), col(0x0A)], axis=1).reshape(-1)


failed = False
n_most, n_check = 1 << a.log2_bases, 1 << a.log2_bases_check
for shape, rec_len in (("reads_150", 150), ("reads_20000", 20000)):
    for n_want in (n_check, n_most):
        records = n_want // rec_len
        n = records * rec_len
        piece = NAME + 2 * rec_len + 6
        letters = torch.empty(n, dtype=torch.uint8, device="cuda")
        devutil.fill_random_acgt(letters, 7)
        bits = cn.n_to_bits_dev(letters)
        qual = torch.randint(33, 127, (n,), dtype=torch.uint8, device="cuda")
        rec_start = torch.arange(records, dtype=torch.int64, device="cuda") * rec_len
        name_off = torch.arange(records + 1, dtype=torch.int64, device="cuda") * NAME
        names = (torch.arange(records * NAME, dtype=torch.int64, device="cuda") % 26 + 0x61).to(torch.uint8)
        bound = po.bits_to_fastq_bound(n, records, records * NAME)
        assert bound == records * piece
        text = torch.empty(bound, dtype=torch.uint8, device="cuda")
        rec_text = torch.empty(records, dtype=torch.int64, device="cuda")
        counts = torch.empty(2, dtype=torch.int64, device="cuda")
        work = torch.empty(po.bits_to_fastq_work_bytes(records), dtype=torch.uint8, device="cuda")

        def call():
            po.bits_to_fastq_dev(bits, n, qual, rec_start, text, counts, work, names=names, name_off=name_off, rec_text=rec_text)

        if a.trace_only:
            if n_want == n_most:
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
            continue
        call()
        total, malformed = counts.cpu().numpy().tolist()
        assert malformed == 0 and total == bound, (shape, total, malformed)
        if n_want == n_check:
            want = np_reference(letters.cpu().numpy(), qual.cpu().numpy(), rec_len, names.cpu().numpy())
            assert np.array_equal(text.cpu().numpy(), want), shape
            continue
        # (b) the floor
        back, qual_copy, names_copy = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty_like(qual), torch.empty_like(names)

        def floor():
            cn.bits_to_n_dev(bits, n, out=back)
            qual_copy.copy_(qual)
            names_copy.copy_(names)

        # (c) the FASTA writer at width 0 on the same table
        fasta_text = torch.empty(po.bits_to_fasta_bound(n, records, records * NAME, 0), dtype=torch.uint8, device="cuda")
        fasta_counts = torch.empty(2, dtype=torch.int64, device="cuda")
        fasta_work = torch.empty(po.bits_to_fasta_work_bytes(records), dtype=torch.uint8, device="cuda")

        def fasta():
            po.bits_to_fasta_dev(bits, n, fasta_text, fasta_counts, fasta_work, rec_start=rec_start, names=names, name_off=name_off, width=0)

        # (d) torch: where every letter, every quality and every other byte of a record lies in the text, GIVEN
        g = torch.arange(n, dtype=torch.int64, device="cuda")
        r = g // rec_len
        letter_idx = r * (piece - rec_len) + g + (NAME + 2)  # r * piece + NAME + 2 + (g - r * rec_len)
        del g, r
        qual_idx = letter_idx + (rec_len + 3)
        inside = torch.cat([torch.arange(NAME + 1, dtype=torch.int64, device="cuda"), torch.tensor([NAME + 3 + rec_len], dtype=torch.int64, device="cuda")])
        rest_idx = ((torch.arange(records, dtype=torch.int64, device="cuda") * piece)[:, None] + inside[None, :]).reshape(-1)
        rest = torch.cat([torch.full((records, 1), 0x40, dtype=torch.uint8, device="cuda"), names.view(records, NAME),
                          torch.full((records, 1), 0x2B, dtype=torch.uint8, device="cuda")], 1).reshape(-1)
        alt = torch.empty(total, dtype=torch.uint8, device="cuda")

        def scatter():
            cn.bits_to_n_dev(bits, n, out=back)
            alt.fill_(0x0A)
            alt[letter_idx] = back
            alt[qual_idx] = qual
            alt[rest_idx] = rest

        ms, floor_ms, fasta_ms, torch_ms = timed([call, floor, fasta, scatter], a.iters)
        fasta_total, fasta_bad = fasta_counts.cpu().numpy().tolist()
        assert fasta_bad == 0 and fasta_total == records * (NAME + 2 + rec_len + 1) and torch.equal(back, letters)
        assert torch.equal(alt, text), shape  # the whole result, against the alternative
        assert torch.equal(rec_text, torch.arange(records, dtype=torch.int64, device="cuda") * piece), shape
        gbs, fasta_gbs = total / ms[0] / 1e6, fasta_total / fasta_ms[0] / 1e6
        emit({"op": "bits_to_fastq", "shape": shape, "bases": n, "records": records, "name_bytes": NAME, "text_bytes": total, "ms": round(ms[0], 4),
              "min_ms": round(ms[1], 4), "max_ms": round(ms[2], 4), "GBs": round(gbs, 1), "floor_ms": round(floor_ms[0], 4), "floor_min_ms": round(floor_ms[1], 4),
              "floor_max_ms": round(floor_ms[2], 4), "vs_floor": round(ms[0] / floor_ms[0], 3), "fasta_text_bytes": fasta_total, "fasta_ms": round(fasta_ms[0], 4),
              "fasta_min_ms": round(fasta_ms[1], 4), "fasta_max_ms": round(fasta_ms[2], 4), "fasta_GBs": round(fasta_gbs, 1), "GBs_vs_fasta": round(gbs / fasta_gbs, 3),
              "ms_vs_fasta": round(ms[0] / fasta_ms[0], 3), "torch_scatter_ms": round(torch_ms[0], 4), "torch_scatter_min_ms": round(torch_ms[1], 4),
              "vs_torch": round(torch_ms[0] / ms[0], 2), "work_bytes": work.numel(), "iters": a.iters})
        failed = failed or (shape == "reads_150" and gbs < fasta_gbs)
        del letter_idx, qual_idx, rest_idx, rest, alt, back, qual_copy, names_copy, fasta_text
    del letters, bits, qual, text, rec_start, name_off, names, rec_text
    torch.cuda.empty_cache()
if failed:
    sys.exit("the acceptance condition does not hold: on reads of 150 the FASTQ write moves fewer GB/s of text than the FASTA write")
